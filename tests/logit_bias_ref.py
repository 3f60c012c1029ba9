"""A numpy model of the logit-bias contract, for the CPU and the GPU tests.

bf16 values travel as uint16 bit patterns.  With x the bf16 logit widened to fp32 and b the slot's fp32 table value:
    z = (b == 0)    ? x            the bits of x copied
      : (b == -inf) ? -inf
      :               bf16_rne(x + b)       (one fp32 add; a NaN x keeps its bits)
    if p < min_pos:  z[s] = -inf for every stop id s in [0, V)
A table value that is NaN or +inf reads as 0.  Row m of tile t = tiles_per_req q + j predicts position
    p = (pos_word >= 0 ? dyn[t][pos_word] : pos_base) + pos_add + 16 j + m."""
import numpy as np

NEG_INF = np.uint16(0xFF80)


def bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_bits(y: np.ndarray) -> np.ndarray:
    """Round to nearest even; NaNs are the caller's business."""
    u = np.ascontiguousarray(y, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return ((u >> 16) & 0xFFFF).astype(np.uint16)


def table_value(b) -> np.ndarray:
    """The table as the kernel reads it: NaN and +inf read as 0."""
    b = np.asarray(b, dtype=np.float32)
    return np.where(np.isnan(b) | (b == np.inf), np.float32(0), b).astype(np.float32)


def sum_f32(xbits, b) -> np.ndarray:
    """The value before its rounding to bf16: x where b == 0, -inf where b == -inf, the fp32 sum elsewhere."""
    x = bits_to_f32(xbits)
    b = table_value(b)
    with np.errstate(all="ignore"):
        s = (x + b).astype(np.float32)
    return np.where(b == 0, x, np.where(b == -np.inf, np.float32(-np.inf), s)).astype(np.float32)


def position(t: int, m: int, tiles_per_req: int = 1, dyn=None, pos_word: int = -1, pos_base: int = 0,
             pos_add: int = 0) -> int:
    j = t % tiles_per_req
    base = int(dyn[t][pos_word]) if (dyn is not None and pos_word >= 0) else pos_base
    return base + pos_add + 16 * j + m


def process(xbits, b, p: int = 0, min_pos: int = 0, stop_ids=()) -> np.ndarray:
    """The contract for one row: bf16 bits in, processed bf16 bits out."""
    xbits = np.asarray(xbits, dtype=np.uint16)
    bv = table_value(b)
    x = bits_to_f32(xbits)
    z = f32_to_bf16_bits(sum_f32(xbits, bv))
    z = np.where((bv == 0) | (np.isnan(x) & (bv != -np.inf)), xbits, z)
    z = np.where(bv == -np.inf, NEG_INF, z).astype(np.uint16)
    if p < min_pos:
        V = xbits.shape[-1]
        for s in stop_ids:
            if 0 <= int(s) < V:
                z[..., int(s)] = NEG_INF
    return z


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


# ---- the inputs the kernel tests share ----
SPECIALS = (0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7FFF, 0x0000, 0x8000, 0x0001, 0x8001, 0x7F7F, 0xFF7F)   # +-inf, NaNs, +-0, ...


def case_rows(rng, rows: int, V: int) -> np.ndarray:
    """bf16 bits [rows, V]: N(0, 4^2)."""
    return f32_to_bf16_bits((rng.standard_normal((rows, V)) * 4).astype(np.float32)).reshape(rows, V)


def case_table(rng, V: int) -> np.ndarray:
    """fp32 [V]: half zeros (a tenth of them -0.0), a quarter finite biases N(0, 3^2), an eighth bans, and — as device
    values only — NaN and +inf entries that read as 0."""
    u = rng.random(V)
    b = np.zeros(V, dtype=np.float32)
    b[u < 0.05] = np.float32(-0.0)
    fin = (u >= 0.5) & (u < 0.75)
    b[fin] = (rng.standard_normal(int(fin.sum())) * 3).astype(np.float32)
    b[(u >= 0.75) & (u < 0.875)] = -np.inf
    b[(u >= 0.875) & (u < 0.9)] = np.nan
    b[(u >= 0.9) & (u < 0.925)] = np.inf
    return b
