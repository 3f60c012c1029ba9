"""A numpy model of the grammar-aware draft pick ("The draft under the grammar"), for the CPU and
the GPU tests.  Conventions of grammar_ref: bf16 values travel as uint16 bit patterns, the pool is int16 [P, V], a slot
has a base (< 0: no grammar) and a state relative to it (-1: violated).

    s = state                          (base < 0 or no pool: no grammar, every column grammar-legal, s unused)
    for m = 1 .. n-1:
        legal(v) = (no grammar or pool[base + s, v] >= 0) and (no bias row or bias[v] != -inf)
        if grammar and s < 0: stop
        c = the lowest legal column among those whose logit is maximal over the legal, non-NaN columns
        if there is no such column: stop
        block[m] = c
        if grammar: s = grammar_ref.step(pool, base, s, c)
"stop" leaves block[m .. n-1] as they were; a slot with neither a grammar nor a bias row is left untouched."""
import numpy as np

import grammar_ref as G


def legal_cols(V: int, pool, base: int, s: int, bias=None) -> np.ndarray:
    """bool [V]: the columns a pick may take in state s (base < 0 or pool None: no grammar)."""
    ok = np.ones(V, dtype=bool)
    if pool is not None and base >= 0:
        ok &= pool[base + s] >= 0
    if bias is not None:
        ok &= ~np.isneginf(np.asarray(bias, dtype=np.float32))
    return ok


def pick_row(xbits, ok) -> int:
    """The lowest column of ok among those whose value is maximal over ok's non-NaN columns (-0 == +0); -1: none."""
    z = G.bits_to_f32(xbits)
    cand = ok & ~np.isnan(z)
    if not cand.any():
        return -1
    m = z[cand].max()
    return int(np.nonzero(cand & (z == m))[0][0])


def pick(xbits, n: int, block, pool=None, base: int = -1, state: int = -1, bias=None):
    """dfl_grammar_draft_rows for one slot: xbits uint16 [>= n, V] (row m predicts block slot m), block the ids on entry
    (int64 [>= n]).  Returns (the block after the pick — a copy —, the states the rows were picked in, one per written
    row m = 1 .. and, under a grammar, the state after the last written id behind them)."""
    xbits = np.asarray(xbits, dtype=np.uint16)
    out = np.array(block, dtype=np.int64, copy=True)
    V = xbits.shape[1]
    gram = pool is not None and base >= 0
    states = []
    if not gram and bias is None:
        return out, states
    s = int(state)
    if gram and (s < 0 or base + s >= pool.shape[0]):
        s = -1
    for m in range(1, min(int(n), 16)):
        if gram and s < 0:
            break
        c = pick_row(xbits[m], legal_cols(V, pool, base, s, bias))
        if c < 0:
            break
        states.append(s if gram else -1)
        out[m] = c
        if gram:
            s = G.step(pool, base, s, c)
    if gram:
        states.append(s)
    return out, states
