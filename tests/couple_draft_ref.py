"""A numpy model of the coupled draft draw, on top of sampling_ref (the noise) and
grammar_draft_ref (the walk under the automaton), for the CPU and the GPU tests.

The draft's slot j of the block that starts at `start` is

    d_j = argmax_v fmaf(bf16(draft_logit_j[v]), invT, g(seed, TARGET, p = start + j, v, extra = 0)),    j = 1 .. bs - 1

(lowest v on ties): the noise the target's verify row j - 1 draws position start + (j - 1) + 1 with.  Under a grammar the
maximum runs over the legal columns of the state reached over the picks before it (`pick`).

The keys are formed in float64 and rounded once to float32, as fmaf rounds: two keys that meet in float32 tie, and the
lowest column wins, as on the device.  What is left between the mirror and the device are the two logf roundings of
sampling_ref; `gap` (top-1 minus the best key below it) is what a test screens its own inputs with."""
import numpy as np

import grammar_draft_ref as GD
import grammar_ref as G
import sampling_ref as S


def keys(x, inv_t, seed: int, p: int, stream: int = S.TARGET, extra: int = 0) -> np.ndarray:
    """float32 [V]: fmaf(x[v], invT, g(seed, stream, p, v, extra)) for one row of bf16-valued fp32 logits."""
    x = np.asarray(x, dtype=np.float32)
    g = S.gumbel(seed, stream, np.int64(p), np.arange(x.shape[0]), extra).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x.astype(np.float64) * np.float64(np.float32(inv_t)) + g).astype(np.float32)


def argmax_lowest(k: np.ndarray, ok=None):
    """(the lowest column of `ok` among those whose key is maximal over ok's non-NaN columns, or -1; top-1 minus the best
    key below it — inf where there is none or the maximum is infinite)."""
    cand = ~np.isnan(k) if ok is None else (ok & ~np.isnan(k))
    if not cand.any():
        return -1, np.inf
    m = k[cand].max()
    below = cand & (k < m)
    gap = float(np.float64(m) - np.float64(k[below].max())) if (below.any() and np.isfinite(m)) else np.inf
    return int(np.nonzero(cand & (k == m))[0][0]), gap


def draw(logits, temperature: float, seed: int, start: int, bs: int, stream: int = S.TARGET):
    """The coupled draft draw of one block: logits fp32 [>= bs, V] (bf16-valued; row j predicts block slot j).  Returns
    (ids int64 [bs] with ids[0] = -1, gaps [bs]).  stream = S.DRAFT: the policy loop's own draw (extra = start)."""
    ids, gaps = np.full(bs, -1, np.int64), np.full(bs, np.inf)
    for j in range(1, bs):
        k = keys(logits[j], S.inv_t(temperature), seed, start + j, stream, start if stream == S.DRAFT else 0)
        ids[j], gaps[j] = argmax_lowest(k)
    return ids, gaps


def target_draw(logits, temperature: float, seed: int, start: int, rows: int):
    """What the verify draws: row r of the target's logits predicts position start + r + 1."""
    out = [argmax_lowest(keys(logits[r], S.inv_t(temperature), seed, start + r + 1)) for r in range(rows)]
    return np.array([o[0] for o in out], np.int64), np.array([o[1] for o in out])


def pick(xbits, n: int, block, *, seed: int, inv_t, pos0: int, pool=None, base: int = -1, state: int = -1, bias=None):
    """dfl_grammar_draft_sample_rows for one slot, the noise form of grammar_draft_ref.pick: the same walk and stops, the
    compared quantity the key of position pos0 + m.  inv_t not > 0: grammar_draft_ref.pick itself.  Returns (the block
    after the pick — a copy —, the states as grammar_draft_ref.pick lists them, the gap of every written row)."""
    if not float(inv_t) > 0:
        out, states = GD.pick(xbits, n, block, pool, base, state, bias)
        return out, states, []
    xbits = np.asarray(xbits, dtype=np.uint16)
    out = np.array(block, dtype=np.int64, copy=True)
    V = xbits.shape[1]
    gram = pool is not None and base >= 0
    states, gaps = [], []
    if not gram and bias is None:
        return out, states, gaps
    s = int(state)
    if gram and (s < 0 or base + s >= pool.shape[0]):
        s = -1
    for m in range(1, min(int(n), 16)):
        if gram and s < 0:
            break
        k = keys(G.bits_to_f32(xbits[m]), inv_t, seed, pos0 + m)
        c, gap = argmax_lowest(k, GD.legal_cols(V, pool, base, s, bias))
        if c < 0:
            break
        states.append(s if gram else -1)
        gaps.append(gap)
        out[m] = c
        if gram:
            s = G.step(pool, base, s, c)
    if gram:
        states.append(s)
    return out, states, gaps


def softmax(x, temperature: float) -> np.ndarray:
    z = np.asarray(x, dtype=np.float64) * float(S.inv_t(temperature))
    e = np.exp(z - z.max())
    return e / e.sum()


def match_probability(p, q) -> float:
    """P(argmax_i log p_i + g_i == argmax_i log q_i + g_i) under shared Gumbel noise:
    sum_i 1 / sum_j max(p_j / p_i, q_j / q_i) over the i with p_i, q_i > 0."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    tot = 0.0
    for i in np.nonzero((p > 0) & (q > 0))[0]:
        tot += 1.0 / np.maximum(p / p[i], q / q[i]).sum()
    return float(tot)
