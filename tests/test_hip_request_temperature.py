"""Per-request temperature at the kernel level ("Per-request temperature"): the ring-form lm_head
with invT read per request slot (dfl_gemm_sample_batch with inv_ts) and the filtered draw with the same (dfl_sample_rows_nucleus with inv_t_dev).
A sampled slot draws what dfl_gemm_sample_batch / dfl_sample_rows draw at that slot's own T; a greedy slot (invT not > 0)
emits the ids of dfl_gemm_argmax_batch, respectively writes nothing."""
import numpy as np
import pytest
import torch

import helpers as H
import nucleus_ref as NR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V, K = 4208, 4096
TS = [0.7, 0.0, 1.3, 0.4]                        # the requests' temperatures, truncated to the request count
SEEDS = [3, 2 ** 63 + 5, 77, 1 << 40]
CASES = [(1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (4, 2)]
EPS = 1e-4   # relative slack on P, as in test_hip_nucleus.py
_CASE = {}


def dev():
    return torch.device("cuda", 0)


def _case():
    """One weight, one set of four activation tiles and their bf16 logits on the host, shared by every test here."""
    if not _CASE:
        from dflash_amd import ops
        g = torch.Generator(device=dev()).manual_seed(41)
        W = (torch.randn(V, K, generator=g, device=dev()) * 0.02).to(BF16)
        x = torch.randn(4, 16, K, generator=g, device=dev()).to(BF16)
        _CASE.update(W=W, wp=ops.pack_weight(W), x=x, ref=SR.bf16_round((x.float() @ W.float().T).cpu().numpy()),
                     gws=torch.zeros(ops.lib().dfl_gemm_batch_ws_bytes(V, K), dtype=torch.uint8, device=dev()))
    return _CASE


def _records(R, tpr):
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    bs = [16, 11, 16, 5][:R] if tpr == 1 else [16, 9, 16, 14][:R]
    rec = torch.zeros(MT, 8, dtype=torch.int32)
    for t in range(R):
        rec[t, ops.DYN_BS], rec[t, ops.DYN_POS0] = bs[t], 500 + 97 * (t // tpr)
    return MT, bs, rec.to(dev())


def _slot_values(R, tpr, MT, temps):
    """seeds and inv_ts of the MT / tpr request slots: the live requests' values, zeros behind them."""
    from dflash_amd import ops
    n = MT // tpr
    ts = (list(temps)[:R // tpr] + [0.0] * n)[:n]
    seeds = torch.tensor([ops.seed_i64(s) for s in SEEDS[:n]], dtype=torch.int64, device=dev())
    inv = torch.tensor([ops.inv_temperature(t) if t > 0 else 0.0 for t in ts], dtype=torch.float32, device=dev())
    return ts, seeds, inv


def _launch_t(wp, x, R, tpr, rec, seeds, inv_ts, gws):
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    logits = torch.zeros(MT, 16, V, dtype=BF16, device=dev())
    ops.gemm_sample_batch(wp, ops.brows_frag(H.frag_of(x[:MT])), R, V, K, 0, 16, gws, ids, 0, rec, seeds=seeds, inv_ts=inv_ts,
                          pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=tpr, nrows_dyn_word=ops.DYN_BS, logits=logits)
    return ids, logits


def _argmax_ids(wp, x, R, rec, gws):
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    ops.gemm_argmax_batch(wp, ops.brows_frag(H.frag_of(x[:MT])), R, V, K, 0, 16, gws, ids, 0, rec, nrows_dyn_word=ops.DYN_BS)
    return ids


def _check_vs_mirror(ids, ref_bf16, rows, positions, seed, T, gap=1e-3, keep=0.95):
    """test_hip_sampling.py's screen with the temperature a parameter."""
    exp, gaps = SR.draw(ref_bf16[rows], T, seed, SR.TARGET, positions, 0)
    safe = gaps > gap
    assert safe.mean() >= keep, safe.mean()
    got = np.asarray(ids)
    assert np.array_equal(got[safe], exp[safe]), (got[safe] != exp[safe]).sum()


def _check_launch(ids, logits, greedy, R, tpr, bs, ts, seeds, ref=None):
    """(a) sampled tiles == dfl_sample_rows over the launch's own logits at the request's T and position, (b) greedy
    tiles == dfl_gemm_argmax_batch, (c) rows past a tile's count untouched, (d) sampled tiles against the numpy mirror."""
    from dflash_amd import ops
    for t in range(R):
        q, j, n = t // tpr, t % tpr, bs[t]
        pos0 = 500 + 97 * q + 1 + 16 * j
        sd = int(seeds[q]) & 0xFFFFFFFFFFFFFFFF
        if ts[q] > 0:
            two = ops.sample_rows(logits[t, :n], seed=sd, temperature=ts[q], pos0=pos0)
            assert torch.equal(ids[t, :n], two), (t, ts[q])
            if ref is not None:
                _check_vs_mirror(ids[t, :n].cpu().numpy(), ref[t], np.arange(n), pos0 + np.arange(n), sd, ts[q])
        else:
            assert torch.equal(ids[t, :n], greedy[t, :n]), t
        assert int((ids[t, n:] != -1).sum()) == 0, t
    assert int((ids[R:] != -1).sum()) == 0


# ---------------------------------------------------------------------------------------------------------- lm_head
@pytest.mark.parametrize("R,tpr", CASES)
def test_gemm_sample_batch_t_draws_each_request_at_its_own_temperature(R, tpr):
    c = _case()
    MT, bs, rec = _records(R, tpr)
    ts, seeds, inv = _slot_values(R, tpr, MT, TS)
    ids, logits = _launch_t(c["wp"], c["x"], R, tpr, rec, seeds, inv, c["gws"])
    greedy = _argmax_ids(c["wp"], c["x"], R, rec, c["gws"])
    _check_launch(ids, logits, greedy, R, tpr, bs, ts, seeds, ref=c["ref"])


@pytest.mark.parametrize("R", [4, 2])
def test_uniform_temperatures_equal_the_single_temperature_entry(R):
    from dflash_amd import ops
    c = _case()
    MT, bs, rec = _records(R, 1)
    ts, seeds, inv = _slot_values(R, 1, MT, [0.7] * 4)
    ids, _ = _launch_t(c["wp"], c["x"], R, 1, rec, seeds, inv, c["gws"])
    old = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    ops.gemm_sample_batch(c["wp"], ops.brows_frag(H.frag_of(c["x"][:MT])), R, V, K, 0, 16, c["gws"], old, 0, rec, seeds=seeds,
                          temperature=0.7, pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=1, nrows_dyn_word=ops.DYN_BS)
    assert torch.equal(ids, old)


def test_exact_tie_in_a_greedy_tile_takes_the_lower_index():
    """Weight rows 5 and 4100 identical and the maximum of every row: the two columns' sums are the same bits (same
    weights, same walk over K) and meet only in the cross-workgroup finish.  The greedy tile emits 5, as
    dfl_gemm_argmax_batch does; the sampled tile beside it still equals its own two-step draw."""
    from dflash_amd import ops
    c = _case()
    g = torch.Generator(device=dev()).manual_seed(7)
    u = torch.randint(0, 2, (K,), generator=g, device=dev()).float() * 2 - 1
    W = c["W"].clone()
    W[5] = W[4100] = (0.06 * u).to(BF16)
    x = (c["x"].float() + u).to(BF16)          # every row: logit ~ 0.06 K against ~ +-2 elsewhere
    wp = ops.pack_weight(W)
    R, tpr = 2, 1
    MT, bs, rec = _records(R, tpr)
    ts, seeds, inv = _slot_values(R, tpr, MT, [0.0, 0.7])
    ids, logits = _launch_t(wp, x, R, tpr, rec, seeds, inv, c["gws"])
    lg = logits[0, :bs[0]].float()
    assert bool((lg[:, 5] == lg[:, 4100]).all()) and bool((lg.max(dim=1).values == lg[:, 5]).all())
    assert bool((ids[0, :bs[0]] == 5).all())
    _check_launch(ids, logits, _argmax_ids(wp, x, R, rec, c["gws"]), R, tpr, bs, ts, seeds)


def test_device_values_are_read_on_every_launch():
    """What a replayed graph relies on: the same launch arguments, inv_ts overwritten in place between two launches."""
    c = _case()
    R, tpr = 4, 1
    MT, bs, rec = _records(R, tpr)
    ts, seeds, inv = _slot_values(R, tpr, MT, TS)
    greedy = _argmax_ids(c["wp"], c["x"], R, rec, c["gws"])
    ids, logits = _launch_t(c["wp"], c["x"], R, tpr, rec, seeds, inv, c["gws"])
    _check_launch(ids, logits, greedy, R, tpr, bs, ts, seeds)
    ts2, _, inv2 = _slot_values(R, tpr, MT, [0.0, 0.7, 0.0, 1.3])   # greedy and sampled swapped
    inv.copy_(inv2)
    ids2, logits2 = _launch_t(c["wp"], c["x"], R, tpr, rec, seeds, inv, c["gws"])
    _check_launch(ids2, logits2, greedy, R, tpr, bs, ts2, seeds)
    assert torch.equal(logits, logits2) and not torch.equal(ids, ids2)


# ---------------------------------------------------------------------------------------------------------- nucleus
def _check_thresholds(x, thr, kept, K_, P, T):
    """test_hip_nucleus.py's check with the temperature a parameter: every row, no screen."""
    P32 = float(np.float32(P))
    for r in range(x.shape[0]):
        t_k = NR.top_k_threshold(x[r], K_)
        if P32 >= 1.0:
            assert thr[r] == np.float32(t_k), (r, thr[r], t_k)
        else:
            lo, hi = NR.top_p_thresholds(x[r], T, [P32 * (1 + EPS), P32 * (1 - EPS)], t_k)
            assert max(t_k, lo) <= thr[r] <= max(t_k, hi), (r, thr[r], t_k, lo, hi)
        assert kept[r] == int((x[r] >= thr[r]).sum()), (r, kept[r])


def _check_ids(ids, x, thr, positions, seed, T, gap=1e-3, keep=0.95):
    exp, gaps = NR.draw_over(x, thr, T, seed, SR.TARGET, positions, 0)
    safe = gaps > gap
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(np.asarray(ids)[safe], exp[safe]), (np.asarray(ids)[safe] != exp[safe]).sum()


@pytest.mark.parametrize("tpr", [1, 2])
@pytest.mark.parametrize("Vn", [1000, 4208])
def test_nucleus_t_per_slot_temperature(Vn, tpr):
    """Four request slots with their own (T, K, P): a greedy slot (its filter set, to show that nothing of it is read), an
    unfiltered sampled slot, and K = 50 / P = 0.9 at two temperatures."""
    from dflash_amd import ops
    NQ = 4
    Ts, Ks, Ps = [0.0, 1.3, 0.7, 0.4], [50, 0, 50, 50], [0.9, 1.0, 0.9, 0.9]
    bs = [16, 11, 5, 16] if tpr == 1 else [32, 27, 21, 18]
    g = torch.Generator(device=dev()).manual_seed(Vn + tpr)
    lg = (torch.randn(NQ * tpr, 16, Vn, generator=g, device=dev()) * 2.0).to(BF16)
    x = lg.float().cpu().numpy()
    rec = torch.zeros(NQ * tpr, 8, dtype=torch.int32)
    for t in range(NQ * tpr):
        q, j = divmod(t, tpr)
        rec[t, ops.DYN_BS], rec[t, ops.DYN_POS0] = min(16, bs[q] - 16 * j), 500 + 97 * q
    rec = rec.to(dev())
    seeds = torch.tensor([ops.seed_i64(s) for s in SEEDS], dtype=torch.int64, device=dev())
    inv = torch.tensor([ops.inv_temperature(t) if t > 0 else 0.0 for t in Ts], dtype=torch.float32, device=dev())
    shape = (NQ * tpr, 16)
    ids = torch.full(shape, -1, dtype=torch.int64, device=dev())
    thr = torch.full(shape, -7.0, dtype=torch.float32, device=dev())
    kept = torch.full(shape, -1, dtype=torch.int32, device=dev())
    ops.sample_rows_nucleus(lg, inv_t=inv, seed=seeds, top_k=torch.tensor(Ks, dtype=torch.int32, device=dev()),
                            top_p=torch.tensor(Ps, dtype=torch.float32, device=dev()), dyn=rec, nrows_dyn_word=ops.DYN_BS,
                            pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=tpr, out=ids, thresholds=thr, kept=kept)
    for t in range(NQ * tpr):
        q, j = divmod(t, tpr)
        n, pos0 = int(rec[t, ops.DYN_BS]), 500 + 97 * q + 1 + 16 * j
        sd = int(seeds[q]) & 0xFFFFFFFFFFFFFFFF
        if Ts[q] == 0.0:   # a greedy slot writes nothing: ids and both diagnostics keep the fill
            assert bool((ids[t] == -1).all()) and bool((thr[t] == -7.0).all()) and bool((kept[t] == -1).all())
            continue
        assert int((ids[t, n:] != -1).sum()) == 0 and int((kept[t, n:] != -1).sum()) == 0 and bool((thr[t, n:] == -7.0).all())
        thr_h, kept_h = thr[t, :n].cpu().numpy(), kept[t, :n].cpu().numpy()
        if Ks[q] == 0 and Ps[q] == 1.0:
            assert torch.equal(ids[t, :n], ops.sample_rows(lg[t, :n], seed=sd, temperature=Ts[q], pos0=pos0)), t
            assert np.array_equal(thr_h, x[t, :n].min(axis=1)) and bool((kept_h == Vn).all())
        else:
            _check_thresholds(x[t, :n], thr_h, kept_h, Ks[q], Ps[q], Ts[q])
            _check_ids(ids[t, :n].cpu().numpy(), x[t, :n], thr_h, pos0 + np.arange(n), sd, Ts[q])
