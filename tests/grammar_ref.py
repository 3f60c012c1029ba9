"""A numpy model of the grammar contract, for the CPU and the GPU tests.

bf16 values travel as uint16 bit patterns.  The pool is int16 [pool_states, V]; a slot has a base (< 0: no grammar) and
a state relative to it (-1: violated, sticky).  One step from state s over id v:
    v outside [0, V)                  -> -1
    n = pool[base + s, v];  n < 0     -> -1       (also where base + n would leave the pool)
Row m of a slot walks its state through block[1 .. m]; a live row is  z = pool[base + s] < 0 ? -inf : x,  a dead row
(no grammar, a violated slot, a step that fails) is x itself."""
import numpy as np

NEG_INF = np.uint16(0xFF80)


def bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(y: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def step(pool, base: int, s: int, v: int) -> int:
    P, V = pool.shape
    if base < 0 or s < 0 or base + s >= P or not 0 <= int(v) < V:
        return -1
    n = int(pool[base + s, int(v)])
    return -1 if (n < 0 or base + n >= P) else n


def walk(pool, base: int, s: int, ids) -> int:
    """The state after ids, -1 from the first failing step on."""
    if base < 0 or s < 0 or base + s >= pool.shape[0]:
        return -1
    for v in ids:
        s = step(pool, base, s, v)
        if s < 0:
            return -1
    return s


def advance(pool, base: int, s: int, ids) -> int:
    """dfl_grammar_advance for one slot: a slot without grammar or already violated is left alone."""
    if base < 0 or s < 0 or len(ids) == 0:
        return s
    return walk(pool, base, s, ids)


def mask_row(xbits, pool, base: int, s: int) -> np.ndarray:
    """One row by the state s it is in (s < 0 or base < 0: dead, copied)."""
    xbits = np.asarray(xbits, dtype=np.uint16)
    if base < 0 or s < 0:
        return xbits.copy()
    return np.where(pool[base + s] < 0, NEG_INF, xbits).astype(np.uint16)


def rows(xbits, pool, base: int, s: int, block=None, row0: int = 0):
    """dfl_grammar_rows for one slot's tile: xbits [n, V] are rows row0 .. row0 + n - 1; block: the slot's block ids (row m
    walks block[1 .. m]; None: no walk).  Returns (z bits [n, V], argmax [n], the states the rows arrived in [n])."""
    xbits = np.asarray(xbits, dtype=np.uint16)
    z, am, st = np.empty_like(xbits), np.zeros(len(xbits), np.int64), np.zeros(len(xbits), np.int64)
    for i in range(len(xbits)):
        m = row0 + i
        st[i] = walk(pool, base, s, [] if block is None else list(block[1:1 + m]))
        z[i] = mask_row(xbits[i], pool, base, int(st[i]))
        am[i] = argmax_lowest(z[i])
    return z, am, st


def argmax_lowest(zbits) -> int:
    """Lowest column among those equal to the maximum over the values that are not NaN (-0 == +0); 0 for a row of NaNs."""
    z = bits_to_f32(zbits)
    ok = ~np.isnan(z)
    if not ok.any():
        return 0
    m = z[ok].max()
    return int(np.nonzero(ok & (z == m))[0][0])


def bf16_ulp_gap(zbits) -> float:
    """Top-1 minus top-2 of a processed row in bf16 ulps of the top-1 value."""
    z = bits_to_f32(zbits).astype(np.float64)
    z = z[~np.isnan(z)]
    top = np.partition(z, -2)[-2:]
    if not np.isfinite(top[0]):
        return float("inf")
    ulp = 2.0 ** (np.floor(np.log2(max(abs(top[1]), 2.0 ** -126))) - 7)
    return float((top[1] - top[0]) / ulp)


def decode_alone(logits_fn, pool, base: int, start: int, prompt, n_new: int, pick=None):
    """The target alone under the grammar, one token at a time: logits_fn(ids) -> bf16 bits [V] of the row that predicts
    the next token; pick(zbits, position) -> token (default: argmax_lowest).  Returns (ids, final state)."""
    ids, s = list(prompt), start
    for _ in range(n_new):
        z = mask_row(logits_fn(ids), pool, base, s)
        v = argmax_lowest(z) if pick is None else int(pick(z, len(ids)))
        ids.append(v)
        s = step(pool, base, s, v)
    return ids, s


# ---- the inputs the kernel tests share ----
def case_rows(rng, n: int, V: int) -> np.ndarray:
    """bf16 bits [n, V]: N(0, 4^2) with a few NaN, +-inf and +-0 entries."""
    x = f32_to_bf16_bits((rng.standard_normal((n, V)) * 4).astype(np.float32)).reshape(n, V)
    for b in (0x7FC0, 0xFF80, 0x7F80, 0x8000, 0x0000):
        if V >= 64:
            x[rng.integers(0, n, 3), rng.integers(0, V, 3)] = b
    return x


def case_dfa(rng, S: int, V: int, p_legal: float = 0.3) -> np.ndarray:
    """int16 [S, V]: each column legal with probability p_legal, successors uniform; every state keeps one legal token."""
    nxt = np.where(rng.random((S, V)) < p_legal, rng.integers(0, S, (S, V)), -1).astype(np.int16)
    for s in range(S):
        if (nxt[s] < 0).all():
            nxt[s, rng.integers(0, V)] = rng.integers(0, S)
    return nxt
