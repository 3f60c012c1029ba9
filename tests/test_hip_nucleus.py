"""Top-k / top-p on the seeded draw ("Filtered draw"): dfl_sample_rows_nucleus against the numpy
fp64 model of the contract (nucleus_ref.py) through its two diagnostic outputs, the final threshold and the kept count,
and its ids against the model's draw over the reported kept set."""
import numpy as np
import pytest
import torch

import nucleus_ref as NR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
EPS = 1e-4   # relative slack on P: ten times the worst-case error of ~150 sequential fp32 adds, a 10-level tree and a 2-ulp exp
VS = [1000, 4208, 151936]
_ROWS = {}


def dev():
    return torch.device("cuda", 0)


def _rows(V, scale, tiles=1):
    """bf16 logits [tiles, 16, V] on the GPU and their fp32 copy on the host, made once per shape."""
    key = (V, scale, tiles)
    if key not in _ROWS:
        g = torch.Generator(device=dev()).manual_seed(V + int(10 * scale) + tiles)
        x = (torch.randn(tiles, 16, V, generator=g, device=dev()) * scale).to(BF16)
        _ROWS[key] = (x, x.float().cpu().numpy())
    return _ROWS[key]


def _launch(logits, n_rows=None, **kw):
    """ids, thresholds, kept of one launch; outputs pre-filled so that unwritten rows show."""
    from dflash_amd import ops
    shape = (logits.shape[0], 16) if logits.dim() == 3 else (logits.shape[0] if n_rows is None else n_rows,)
    ids = torch.full(shape, -1, dtype=torch.int64, device=dev())
    thr = torch.full(shape, -7.0, dtype=torch.float32, device=dev())
    kept = torch.full(shape, -1, dtype=torch.int32, device=dev())
    ops.sample_rows_nucleus(logits, temperature=T, out=ids, thresholds=thr, kept=kept, **kw)
    return ids, thr, kept


def _check_thresholds(x, thr, kept, K, P):
    """Each row's reported threshold against the model: the top-k part exact, the top-p part inside
    [t_model(P (1 + eps)), t_model(P (1 - eps))]; the kept count exactly count(x >= reported threshold)."""
    P32 = float(np.float32(P))
    for r in range(x.shape[0]):
        t_k = NR.top_k_threshold(x[r], K)
        if P32 >= 1.0:
            assert thr[r] == np.float32(t_k), (r, thr[r], t_k)
        else:
            lo, hi = NR.top_p_thresholds(x[r], T, [P32 * (1 + EPS), P32 * (1 - EPS)], t_k)
            assert max(t_k, lo) <= thr[r] <= max(t_k, hi), (r, thr[r], t_k, lo, hi)
        assert kept[r] == int((x[r] >= thr[r]).sum()), (r, kept[r])


def _check_ids(ids, x, thr, positions, seed, gap=1e-3, keep=0.95, stream=SR.TARGET, extra=0):
    exp, gaps = NR.draw_over(x, thr, T, seed, stream, positions, extra)
    safe = gaps > gap
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(np.asarray(ids)[safe], exp[safe]), (np.asarray(ids)[safe] != exp[safe]).sum()


# ---------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("V", VS)
def test_filters_off_is_the_plain_draw(V):
    """K = 0 / P = 1 (and K >= V): ids bit-equal to dfl_sample_rows on the same logits, seeds and positions, in the
    tile / record form and in the host-position form; the threshold is the row minimum and everything is kept."""
    from dflash_amd import ops
    lg, x = _rows(V, 2.0, tiles=2)
    rec = torch.zeros(2, 8, dtype=torch.int32)
    rec[0, ops.DYN_BS], rec[0, ops.DYN_POS0], rec[1, ops.DYN_BS], rec[1, ops.DYN_POS0] = 16, 700, 9, 4000
    rec = rec.to(dev())
    sd = [5, 2 ** 63 + 11]
    seeds = torch.tensor([ops.seed_i64(s) for s in sd], dtype=torch.int64, device=dev())
    ids, thr, kept = _launch(lg, seed=seeds, dyn=rec, nrows_dyn_word=ops.DYN_BS, pos_word=ops.DYN_POS0, pos_add=1)
    for t, n in ((0, 16), (1, 9)):
        pos0 = int(rec[t, ops.DYN_POS0]) + 1
        assert torch.equal(ids[t, :n], ops.sample_rows(lg[t, :n], seed=sd[t], temperature=T, pos0=pos0)), t
        assert int((ids[t, n:] != -1).sum()) == 0 and int((kept[t, n:] != -1).sum()) == 0
        assert np.array_equal(thr[t, :n].cpu().numpy(), x[t, :n].min(axis=1)) and bool((kept[t, :n] == V).all())
    g = torch.Generator().manual_seed(2)
    pos = torch.randint(0, 1 << 30, (16,), generator=g).to(torch.int32).to(dev())
    for kw in ({}, {"top_k": V + 7}, {"top_k": V}):
        ids2, _, kept2 = _launch(lg[1], seed=77, positions=pos, stream=ops.RNG_DRAFT, extra=9, **kw)
        assert torch.equal(ids2, ops.sample_rows(lg[1], seed=77, temperature=T, positions=pos, stream=ops.RNG_DRAFT,
                                                 extra=9))
        assert bool((kept2 == V).all())


@pytest.mark.parametrize("V", VS)
def test_top_k_1_is_the_argmax(V):
    lg, x = _rows(V, 2.0)
    ids, thr, kept = _launch(lg[0], seed=3, top_k=1, pos_base=10)
    top2 = np.sort(x[0], axis=1)[:, -2:]
    free = top2[:, 1] > top2[:, 0]                       # tie-free rows
    assert free.sum() >= 8
    assert np.array_equal(ids.cpu().numpy()[free], x[0].argmax(axis=1)[free])
    assert np.array_equal(thr.cpu().numpy(), top2[:, 1]) and bool((kept.cpu().numpy()[free] == 1).all())


@pytest.mark.parametrize("scale", [2.0, 0.3])
@pytest.mark.parametrize("V", VS)
def test_thresholds_counts_and_ids_against_the_model(V, scale):
    lg, x = _rows(V, scale)
    pos0, seed = 123456, 2 ** 41 + 3
    for K, P in ((50, 1.0), (0, 0.9), (50, 0.9), (0, 0.5), (V + 7, 1.0)):
        ids, thr, kept = _launch(lg[0], seed=seed, top_k=K, top_p=P, pos_base=pos0)
        thr, kept = thr.cpu().numpy(), kept.cpu().numpy()
        _check_thresholds(x[0], thr, kept, K, P)
        _check_ids(ids.cpu().numpy(), x[0], thr, pos0 + np.arange(16), seed)


def test_engineered_rows():
    V = 4208
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(16, V, generator=g) * 2).clamp(max=4.0)
    # row 0: 10 values above 5.0, then 30 equal to 5.0 straddling the 25th place
    x[0, 100:110] = torch.linspace(6, 9, 10)
    x[0, 200:260:2] = 5.0
    # row 1: constant
    x[1] = 1.5
    # row 2: the first token alone holds more than P
    x[2] = torch.randn(V, generator=g) * 0.3
    x[2, 0] = 20.0
    # row 3: -inf entries and a spread wide enough that exp underflows
    x[3, ::3] = float("-inf")
    x[3, 5], x[3, 11], x[3, 17] = 300.0, 299.5, 299.0
    lg = x.to(BF16).to(dev())
    xr = lg.float().cpu().numpy()

    ids, thr, kept = _launch(lg, seed=4, top_k=25, pos_base=0)
    assert float(thr[0]) == 5.0 and int(kept[0]) == 40 and 100 <= int(ids[0]) < 260
    assert float(thr[1]) == 1.5 and int(kept[1]) == V
    _check_thresholds(xr, thr.cpu().numpy(), kept.cpu().numpy(), 25, 1.0)

    for K, P in ((0, 0.3), (5, 0.9), (0, 0.9)):
        ids, thr, kept = _launch(lg, seed=4, top_k=K, top_p=P, pos_base=0)
        thr_h, kept_h = thr.cpu().numpy(), kept.cpu().numpy()
        _check_thresholds(xr, thr_h, kept_h, K, P)
        assert thr_h[1] == 1.5 and kept_h[1] == V                      # a constant row is kept whole for any P < 1
        assert (thr_h[2], kept_h[2], int(ids[2])) == (20.0, 1, 0)
        assert np.isfinite(xr[3, int(ids[3])]) and int(ids[3]) in (5, 11, 17)
        _check_ids(ids.cpu().numpy(), xr, thr_h, np.arange(16), 4, keep=0.8)
    # without a filter too, a -inf column is never drawn
    ids, _, _ = _launch(lg, seed=4, pos_base=0)
    assert np.isfinite(xr[np.arange(16), ids.cpu().numpy()]).all()


@pytest.mark.parametrize("tpr", [1, 2])
def test_ragged_tiles_with_per_request_parameters(tpr):
    """3 requests x tiles_per_req tiles, row counts from the records, seeds / top_k / top_p from device arrays indexed by
    request: every tile equals the single-tile call with that request's scalars; rows past the count stay untouched."""
    from dflash_amd import ops
    V, R = 4208, 3
    lg, x = _rows(V, 2.0, tiles=R * tpr)
    bs = [16, 11, 5] if tpr == 1 else [32, 27, 21]
    rec = torch.zeros(R * tpr, 8, dtype=torch.int32)
    for t in range(R * tpr):
        q, j = divmod(t, tpr)
        rec[t, ops.DYN_BS], rec[t, ops.DYN_POS0] = min(16, bs[q] - 16 * j), 500 + 97 * q
    rec = rec.to(dev())
    sd, Ks, Ps = [3, 2 ** 63 + 5, 77], [50, 0, 1], [0.9, 0.5, 1.0]
    seeds = torch.tensor([ops.seed_i64(s) for s in sd], dtype=torch.int64, device=dev())
    ids, thr, kept = _launch(lg, seed=seeds, top_k=torch.tensor(Ks, dtype=torch.int32, device=dev()),
                             top_p=torch.tensor(Ps, dtype=torch.float32, device=dev()), dyn=rec,
                             nrows_dyn_word=ops.DYN_BS, pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=tpr)
    for t in range(R * tpr):
        q, j = divmod(t, tpr)
        n, pos0 = int(rec[t, ops.DYN_BS]), 500 + 97 * q + 1 + 16 * j
        one = _launch(lg[t, :n], seed=sd[q], top_k=Ks[q], top_p=Ps[q], pos_base=pos0)
        for got, exp in zip((ids, thr, kept), one):
            assert torch.equal(got[t, :n], exp), (t, got[t, :n], exp)
        assert int((ids[t, n:] != -1).sum()) == 0 and int((kept[t, n:] != -1).sum()) == 0
        _check_thresholds(x[t, :n], thr[t, :n].cpu().numpy(), kept[t, :n].cpu().numpy(), Ks[q], Ps[q])


def _chi2(counts, p, top=8):
    idx = np.argsort(-p)[:top]
    n = counts.sum()
    obs = np.concatenate([counts[idx], [n - counts[idx].sum()]]).astype(np.float64)
    exp = np.concatenate([p[idx], [max(1e-12, 1 - p[idx].sum())]]) * n
    keep = exp > 5
    return float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum()), int(keep.sum()) - 1


@pytest.mark.parametrize("K,P", [(0, 0.8), (12, 1.0)])
def test_draws_follow_the_renormalised_softmax_of_the_kept_set(K, P):
    """20480 draws from one fixed row with the positions varied: none outside the model's kept set, and inside it the
    counts follow softmax(x / T) renormalised over the set."""
    V, n = 256, 20480
    g = torch.Generator().manual_seed(4)
    row = (torch.randn(V, generator=g) * 2).to(BF16)
    lg = row.to(dev()).expand(n // 16, 16, V).contiguous()
    pos = torch.arange(n, dtype=torch.int32, device=dev())
    ids, _, _ = _launch(lg, seed=21, top_k=K, top_p=P, positions=pos)
    x = row.float().numpy()
    t = NR.thresholds(x, T, K, P)[2]
    inside = x >= np.float32(t)
    counts = np.bincount(ids.cpu().numpy().ravel(), minlength=V)
    assert counts[~inside].sum() == 0
    p = np.where(inside, np.exp((x.astype(np.float64) - x.max()) * float(SR.inv_t(T))), 0.0)
    chi2, dof = _chi2(counts, p / p.sum())
    assert dof >= 4 and chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)


def test_two_runs_are_identical():
    lg, _ = _rows(151936, 2.0)
    a = _launch(lg[0], seed=9, top_k=50, top_p=0.9, pos_base=5)
    b = _launch(lg[0], seed=9, top_k=50, top_p=0.9, pos_base=5)
    c = _launch(lg[0], seed=9, top_k=0, top_p=0.9, pos_base=5)
    d = _launch(lg[0], seed=9, top_k=0, top_p=0.9, pos_base=5)
    for u, v in zip(a + c, b + d):
        assert torch.equal(u, v)
