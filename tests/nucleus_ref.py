"""numpy fp64 model of the filtered draw's contract ("Filtered draw"), on top of sampling_ref.

One row of bf16-valued logits x, invT = float32(1 / T), an integer K >= 0 (0 = off), 0 < P <= 1 (>= 1 = off):
    t_k   = the K-th largest value counted with multiplicity (the row minimum if K == 0 or K >= V)
    w_v   = exp(invT (x_v - max x)),  Z_k = sum of w over {x >= t_k}
    t_p   = the largest t with  sum_{x_v >= t_k, x_v >= t} w_v >= P Z_k          (t_k with P off)
    kept  = {v : x_v >= max(t_k, t_p)}            ties at a threshold are kept whole
    draw  = argmax over kept of fmaf(x_v, invT, g_v), the noise of sampling_ref, lowest v on ties
"""
from __future__ import annotations

import numpy as np

import sampling_ref as SR


def top_k_threshold(x: np.ndarray, top_k: int) -> float:
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[0]
    if top_k <= 0 or top_k >= V:
        return float(x.min())
    return float(np.partition(x, V - top_k)[V - top_k])


def top_p_thresholds(x: np.ndarray, temperature: float, top_ps, t_k: float) -> list:
    """t_p for each top_p of `top_ps` (Python floats, taken as given: the tests pass P (1 +- eps) here)."""
    x = np.asarray(x, dtype=np.float32)
    vals, counts = np.unique(x[x >= np.float32(t_k)], return_counts=True)       # ascending distinct values
    vals, counts = vals[::-1].astype(np.float64), counts[::-1].astype(np.float64)
    with np.errstate(invalid="ignore"):
        w = counts * np.exp(float(SR.inv_t(temperature)) * (vals - vals[0]))
    cum = np.cumsum(w)
    out = []
    for top_p in top_ps:
        hit = np.nonzero(cum >= top_p * cum[-1])[0]
        out.append(float(t_k) if top_p >= 1.0 else float(vals[hit[0]] if hit.size else vals[-1]))
    return out


def top_p_threshold(x: np.ndarray, temperature: float, top_p: float, t_k: float) -> float:
    return top_p_thresholds(x, temperature, [top_p], t_k)[0]


def thresholds(x: np.ndarray, temperature: float, top_k: int, top_p: float):
    """(t_k, t_p, t): the top-k threshold, the top-p threshold over what top-k left, and their maximum."""
    t_k = top_k_threshold(x, top_k)
    t_p = top_p_threshold(x, temperature, float(np.float32(top_p)), t_k)
    return t_k, t_p, max(t_k, t_p)


def threshold_brute(x: np.ndarray, temperature: float, top_k: int, top_p: float) -> float:
    """The same threshold by a plain sort and an element-by-element scan (for small rows)."""
    x = np.asarray(x, dtype=np.float32)
    V = x.shape[0]
    order = sorted((float(v) for v in x), reverse=True)
    t_k = order[top_k - 1] if 0 < top_k < V else order[-1]
    kept = [v for v in order if v >= t_k]
    if float(np.float32(top_p)) >= 1.0:
        return t_k
    it = float(SR.inv_t(temperature))
    w = [float(np.exp(it * (v - kept[0]))) for v in kept]
    Z = sum(w)
    best = kept[-1]
    for t in sorted(set(kept)):                       # ascending: the last t that still holds the mass is the largest
        if sum(wi for v, wi in zip(kept, w) if v >= t) >= float(np.float32(top_p)) * Z:
            best = t
    return max(t_k, best)


def draw_over(logits_bf16: np.ndarray, thr, temperature: float, seed: int, stream: int, positions, extra=0):
    """ids [rows] of the draw over {x >= thr[row]} and the perturbed top-2 gap inside that set (inf for a set of one)."""
    x = np.asarray(logits_bf16, dtype=np.float32)
    z = SR.perturbed(x, temperature, seed, stream, positions, extra)
    z = np.where(x >= np.asarray(thr, dtype=np.float32).reshape(-1, 1), z, -np.inf)
    ids = z.argmax(axis=1)
    top2 = np.sort(z, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):
        gaps = top2[:, 1] - top2[:, 0]
    return ids, np.where(np.isnan(gaps), np.inf, gaps)
