"""A numpy model of the penalty contract, for the CPU and the GPU tests.

bf16 values travel as uint16 bit patterns.  Predicting the token at index p of a request's ids with n_in prompt tokens:
seen(v) = v occurs in ids[0 .. p-1]; c(v) = occurrences of v in ids[n_in .. p-1].  With x the bf16 logit widened to fp32:
    y1 = seen ? (x > 0 ? x / r : x * r) : x         (fp32)
    y2 = y1 - (c > 0 ? a : 0)                       (fp32)
    y3 = fmaf(-f, float(c), y2)                     (one rounding: through float64 here)
    z  = bf16_rne(y3)
A NaN keeps its bits.  Ids outside [0, V) are not counted."""
import numpy as np

PROMPT_BIT = np.uint32(0x80000000)


def bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(y: np.ndarray) -> np.ndarray:
    """Round to nearest even; NaNs are the caller's business."""
    u = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def table_of(ids, n_in: int, end: int, V: int) -> np.ndarray:
    """The table row after ids[0:n_in] were counted as prompt and ids[n_in:end] as output: bit 31 = seen in the prompt,
    bits 0..30 = occurrences in the output."""
    ids = np.asarray(ids, dtype=np.int64)
    t = np.zeros(V, dtype=np.uint32)
    p = ids[:n_in]
    p = p[(p >= 0) & (p < V)]
    t[p] |= PROMPT_BIT
    o = ids[n_in:end]
    o = o[(o >= 0) & (o < V)]
    np.add.at(t, o, np.uint32(1))
    return t.view(np.int32)


def seen_counts(table: np.ndarray, block_tokens=()) -> tuple:
    """(seen bool [V], c int64 [V]) of a table row plus in-block (output) tokens."""
    t = np.asarray(table).view(np.uint32)
    V = t.shape[0]
    c = (t & np.uint32(0x7FFFFFFF)).astype(np.int64)
    seen = t != 0
    b = np.asarray(list(block_tokens), dtype=np.int64)
    b = b[(b >= 0) & (b < V)]
    np.add.at(c, b, 1)
    seen = seen.copy()
    seen[b] = True
    return seen, c


def step3_f64(xbits, seen, c, r: float, a: float, f: float) -> np.ndarray:
    """y3 before its rounding to fp32, as float64 (steps 1 and 2 in fp32)."""
    x = bits_to_f32(xbits)
    r32, a32, f32 = np.float32(r), np.float32(a), np.float32(f)
    with np.errstate(all="ignore"):
        y1 = np.where(seen, np.where(x > 0, x / r32, x * r32), x).astype(np.float32)
        y2 = np.where(c > 0, y1 - a32, y1).astype(np.float32)
        return (-np.float64(f32)) * np.float32(c).astype(np.float64) + y2.astype(np.float64)


def penalise(xbits, seen, c, r: float, a: float, f: float) -> np.ndarray:
    """The contract: bf16 bits in, penalised bf16 bits out."""
    xbits = np.asarray(xbits, dtype=np.uint16)
    with np.errstate(all="ignore"):
        y3 = step3_f64(xbits, seen, c, r, a, f).astype(np.float32)
    z = f32_to_bf16_bits(y3)
    return np.where(np.isnan(bits_to_f32(xbits)), xbits, z).astype(np.uint16)


def near_midpoint(xbits, seen, c, r: float, a: float, f: float, rel: float = 1e-6) -> np.ndarray:
    """True where the float64 value of step 3 lies within `rel` (relative) of the midpoint between two neighbouring
    bf16 values: there the one rounding of the fused step and this model's two may pick different neighbours."""
    y = step3_f64(xbits, seen, c, r, a, f)
    with np.errstate(all="ignore"):
        lo = (np.abs(y).astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000))   # truncation (may sit one fp32 ulp off)
        out = np.zeros(y.shape, dtype=bool)
        for d in (-1, 0, 1):   # the bf16 value below |y| and its neighbours: the rounding to fp32 can cross one
            b0 = (lo.astype(np.int64) + d * 0x10000).clip(0, 0x7F7F0000).astype(np.uint32)
            v0 = b0.view(np.float32).astype(np.float64)
            v1 = (b0 + np.uint32(0x10000)).view(np.float32).astype(np.float64)
            mid = 0.5 * (v0 + v1)
            out |= np.isfinite(y) & np.isfinite(mid) & (np.abs(np.abs(y) - mid) <= rel * np.abs(mid))
    return out


def neighbours_ok(got, want, near) -> np.ndarray:
    """Elementwise: equal bits, or — where `near` — one bf16 step apart."""
    got, want = np.asarray(got, dtype=np.uint16), np.asarray(want, dtype=np.uint16)
    step = np.abs(got.astype(np.int32) - want.astype(np.int32)) <= 1
    return (got == want) | (near & step)


def argmax_lowest(zbits) -> int:
    """Lowest column among those equal to the maximum over the values that are not NaN (-0 == +0); 0 for a row of NaNs."""
    z = bits_to_f32(zbits)
    ok = ~np.isnan(z)
    if not ok.any():
        return 0
    m = z[ok].max()
    return int(np.nonzero(ok & (z == m))[0][0])


def history(ids, n_in: int, p: int, V: int) -> tuple:
    """(seen, c) for predicting index p straight from the definition."""
    return seen_counts(table_of(ids, n_in, p, V))


def bf16_ulp_gap(zbits) -> float:
    """Top-1 minus top-2 of a penalised row in bf16 ulps of the top-1 value."""
    z = bits_to_f32(zbits).astype(np.float64)
    z = z[~np.isnan(z)]
    top = np.partition(z, -2)[-2:]
    ulp = 2.0 ** (np.floor(np.log2(max(abs(top[1]), 2.0 ** -126))) - 7)
    return float((top[1] - top[0]) / ulp)


# ---- the inputs the kernel tests share (and the CPU tests check against the midpoint cap) ----
# Penalty values without short binary or decimal expansions: with r = 1.3 one bf16 logit in a hundred lands x * r on an
# exact bf16 midpoint (1.2890625 * 1.3 = 1.67578125), which the cap below is not meant for.
KERNEL_PARAMS = ((1.2873, 0.2173, 0.2519), (0.7811, -0.1391, 0.0713))
SPECIALS = (0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7FFF, 0x0000, 0x8000, 0x0001, 0x8001, 0x7F7F, 0xFF7F)   # +-inf, NaNs, +-0, ...


def case_rows(rng, rows: int, V: int, specials: bool = True) -> np.ndarray:
    """bf16 bits [rows, V]: N(0, 4^2) with every pattern of SPECIALS planted twice per row."""
    x = f32_to_bf16_bits((rng.standard_normal((rows, V)) * 4).astype(np.float32)).reshape(rows, V)
    if specials:
        for r in range(rows):
            cols = rng.choice(V, 2 * len(SPECIALS), replace=False)
            x[r, cols] = np.tile(np.array(SPECIALS, dtype=np.uint16), 2)
    return x


def case_table(rng, V: int) -> np.ndarray:
    """int32 [V]: a tenth prompt-only entries, a tenth output-only (counts 1..5), a tenth both, the rest untouched."""
    u = rng.random(V)
    t = np.zeros(V, dtype=np.uint32)
    t[u < 0.2] |= PROMPT_BIT
    out = (u >= 0.1) & (u < 0.3)
    t[out] += rng.integers(1, 6, int(out.sum())).astype(np.uint32)
    return t.view(np.int32)
