"""numpy mirror of the seeded sampler's noise (dflash_amd/csrc/dfl_rng.h), bit for bit up to the two logf roundings.

    key     = (seed & 0xffffffff, seed >> 32)
    counter = (v >> 2, p, extra, stream)
    w       = Philox4x32-10(counter, key)[v & 3]
    u       = ((w >> 9) + 0.5) * 2^-23          strictly inside (0, 1)
    g       = -log(-log(u))
    draw    = argmax_v fmaf(bf16(logit_v), invT, g_v)      (lowest v on ties)
"""
from __future__ import annotations

import numpy as np

TARGET, DRAFT = 0, 1
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, seed: int):
    """Random123's Philox4x32 with 10 rounds over broadcastable uint32 counter words; returns the four output words."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for r in range(10):
        if r > 0:
            k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
    return [x.astype(np.uint32) for x in c]


def words(seed: int, stream: int, p, v, extra=0) -> np.ndarray:
    """uint32 word of column v at position p (broadcast over p and v)."""
    p, v, extra = np.broadcast_arrays(np.asarray(p, dtype=np.int64), np.asarray(v, dtype=np.int64),
                                      np.asarray(extra, dtype=np.int64))
    w = philox4x32_10(v >> 2, p & 0xFFFFFFFF, extra & 0xFFFFFFFF, np.full(v.shape, stream), seed)
    sel = (v & 3).astype(np.int64)
    return np.choose(sel, w).astype(np.uint32)


def uniform(seed: int, stream: int, p, v, extra=0) -> np.ndarray:
    """float32 u strictly inside (0, 1) (exact: (2k + 1) * 2^-24)."""
    w = words(seed, stream, p, v, extra)
    return ((w >> np.uint32(9)).astype(np.float32) * np.float32(2.0 ** -23) + np.float32(2.0 ** -24)).astype(np.float32)


def gumbel(seed: int, stream: int, p, v, extra=0) -> np.ndarray:
    u = uniform(seed, stream, p, v, extra)
    return (-np.log(-np.log(u))).astype(np.float32)


def inv_t(temperature: float) -> np.float32:
    return np.float32(1.0 / float(temperature))


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 (round to nearest even) -> fp32."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = (b + np.uint64(0x7FFF) + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16) << np.uint64(16)
    return b.astype(np.uint32).view(np.float32)


def perturbed(logits_bf16: np.ndarray, temperature: float, seed: int, stream: int, positions, extra=0) -> np.ndarray:
    """[rows, V] fp32 values (already bf16-valued) -> the values the draw compares, in float64 (fmaf = one rounding of
    the exact product-sum; float64 holds that exactly enough for the screens the tests apply)."""
    x = np.asarray(logits_bf16, dtype=np.float32)
    rows, V = x.shape
    pos = np.asarray(positions, dtype=np.int64).reshape(rows, 1)
    ext = np.asarray(extra, dtype=np.int64).reshape(-1, 1) if np.ndim(extra) else extra
    g = gumbel(seed, stream, pos, np.arange(V)[None, :], ext).astype(np.float64)
    return x.astype(np.float64) * float(inv_t(temperature)) + g


def draw(logits_bf16, temperature, seed, stream, positions, extra=0):
    """ids [rows] and the perturbed top-2 gap [rows]."""
    z = perturbed(logits_bf16, temperature, seed, stream, positions, extra)
    ids = z.argmax(axis=1)
    top2 = np.sort(z, axis=1)[:, -2:]
    return ids, top2[:, 1] - top2[:, 0]
