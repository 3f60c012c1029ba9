"""The numpy mirror of dfl_min_p_rows: bf16 bits in and out, every operation in float32 and rounded
once.  x: the row's logits widened to fp32; invT = float32(1 / T); L = float32(ln(min_p)), -inf for min_p = 0:

    m   = max over the entries of x that are not NaN          (-0 == +0)
    d_v = fl32(fl32(x_v - m) * invT)
    z_v = x_v if x_v == m or d_v >= L else -inf                (bits copied; a NaN x_v keeps its bits too)

A row is copied whole when the slot is off (L is -inf, > 0 or NaN), when it is greedy (invT not > 0) or when m is not
finite.  kept: the number of columns with x_v == m or d_v >= L (a NaN is not counted); a copied row reports V."""
import math

import numpy as np

NEG_INF = 0xFF80
# bit patterns every case set should carry: -inf, +inf, NaNs of both signs with payloads, +-0, the largest finite values
SPECIALS = (0xFF80, 0x7F80, 0x7FC1, 0xFFFF, 0x7F81, 0x0000, 0x8000, 0x7F7F, 0xFF7F)


def widen(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bits, round to nearest even (only used to build inputs)."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = u + 0x7FFF + ((u >> 16) & 1)
    return (u >> 16).astype(np.uint16)


def log_min_p(min_p) -> np.float32:
    """float32(ln(min_p)) as the host computes it; -inf for None / 0."""
    if min_p is None or min_p == 0:
        return np.float32(-np.inf)
    return np.float32(math.log(float(min_p)))


def inv_t(temperature: float) -> np.float32:
    return np.float32(1.0 / float(temperature))


def row_max(x: np.ndarray) -> np.float32:
    """The maximum over the entries that are not NaN; -inf when there is none."""
    ok = ~np.isnan(x)
    return np.float32(x[ok].max()) if ok.any() else np.float32(-np.inf)


def process(bits: np.ndarray, L, invT):
    """(masked bits, kept) of one row [V] of bf16 bits under device values L and invT (any bit pattern)."""
    bits = np.asarray(bits, dtype=np.uint16)
    L, invT = np.float32(L), np.float32(invT)
    V = bits.shape[0]
    on = bool(L <= 0) and bool(L > -np.inf) and bool(invT > 0)
    x = widen(bits)
    m = row_max(x)
    if not on or not np.isfinite(m):
        return bits.copy(), V
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((x - m).astype(np.float32) * invT).astype(np.float32)
        keep = (x == m) | (d >= L)
    out = np.where(keep | np.isnan(x), bits, np.uint16(NEG_INF)).astype(np.uint16)
    return out, int(keep.sum())


def argmax_lowest(bits: np.ndarray) -> int:
    """The lowest column among those equal to the maximum over the values that are not NaN; 0 for a row of NaNs."""
    x = widen(bits)
    ok = ~np.isnan(x)
    if not ok.any():
        return 0
    return int(np.nonzero(ok & (x == x[ok].max()))[0][0])


def case_rows(rng, rows: int, V: int, scale: float = 3.0) -> np.ndarray:
    """Random bf16 logits [rows, V]: a normal bulk, so that thresholds of every size cut through it."""
    return to_bits(rng.standard_normal((rows, V)).astype(np.float32) * np.float32(scale))
