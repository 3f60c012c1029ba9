"""NumPy fp64 reference of dfl_logprob_rows (include/dflash_hip.h), written from the definition:
log-sum-exp over the finite entries, the chosen id's log-probability, the top N by (value descending, column ascending),
and the rule that scatters a row's numbers to the position its token commits at."""
import numpy as np


def bf16_round(x):
    """float32 values after one round-to-nearest-even to bf16 (kept as float32)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32)


def lse(row):
    """max + log(sum exp(x - max)) in fp64: the maximum over the finite values, non-finite entries contribute 0; a row
    without a finite value gives -inf."""
    with np.errstate(invalid="ignore"):      # (a signalling NaN among the inputs: the cast may say so)
        x = np.asarray(row, dtype=np.float64)
    fin = np.isfinite(x)
    if not fin.any():
        return -np.inf
    m = x[fin].max()
    return m + np.log(np.exp(x[fin] - m).sum())


def logprob(row, idx):
    """x[idx] - lse; NaN for an id outside [0, V)."""
    x = np.asarray(row, dtype=np.float64)
    if not 0 <= idx < x.shape[0]:
        return np.nan
    with np.errstate(invalid="ignore"):      # (-inf) - (-inf) = NaN is the definition, not an accident
        return x[idx] - lse(x)


def top(row, n):
    """(ids [n], log-probabilities [n]) of the n columns first by (value descending, column ascending); -0 == +0.  Rows
    hold no NaN here.  Entries past the row's width are id -1 and NaN."""
    x = np.asarray(row, dtype=np.float64) + 0.0            # (-0 + 0 = +0)
    order = np.lexsort((np.arange(x.shape[0]), -x))[:n]   # stable: value descending, then column ascending
    ids = np.full(n, -1, dtype=np.int64)
    lps = np.full(n, np.nan)
    ids[:order.size] = order
    with np.errstate(invalid="ignore"):
        lps[:order.size] = x[order] - lse(x)
    return ids, lps


def position(pos0, pos_add, j, m):
    """Where row m of tile j (of its request) writes: the position rule of the filtered draw."""
    return pos0 + pos_add + 16 * j + m


def scatter(lp_buf, start, row_values):
    """One verify cycle starting at `start`: row j's value lands at position start + j + 1 (dropped past the buffer)."""
    for j, v in enumerate(row_values):
        p = position(start, 1, 0, j)
        if 0 <= p < lp_buf.shape[0]:
            lp_buf[p] = v


def tolerance(lse_ref):
    """|kernel - reference| allowed on a log-probability.  The kernel sums per thread sequentially (at most 152 positive
    fp32 terms: <= 152 * 2^-24 ~ 9e-6 relative on the sum, hence absolute on its log), then 6 butterfly and 15 wave adds
    (21 * 2^-24), a few ulp for expf / logf on values <= 1 and log(sum) <= 12, and half an ulp of the larger operand in
    max + log(sum) and in x - lse: 2^-16 absolute plus 2^-22 relative to |lse|."""
    return 2.0 ** -16 + 2.0 ** -22 * abs(lse_ref)
