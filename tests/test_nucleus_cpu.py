"""The filtered draw without a GPU: the numpy model (nucleus_ref.py) against a brute-force sort-and-scan, the argument
validation of dfl_sample_rows_nucleus, and the Python-level errors of the top_k / top_p keywords."""
import numpy as np
import pytest

import nucleus_ref as NR
import sampling_ref as SR

T = 0.7


def _row(seed, V, scale):
    return SR.bf16_round(np.random.default_rng(seed).standard_normal(V).astype(np.float32) * scale)


@pytest.mark.parametrize("scale", [2.0, 0.3])
def test_model_matches_the_brute_force_scan(scale):
    for seed in range(4):
        x = _row(seed, 97, scale)
        for K, P in ((0, 1.0), (5, 1.0), (0, 0.9), (5, 0.9), (0, 0.5), (1, 1.0), (97, 1.0), (200, 0.3), (96, 1.0)):
            assert NR.thresholds(x, T, K, P)[2] == NR.threshold_brute(x, T, K, P), (seed, K, P)


def test_ties_at_both_boundaries_are_kept_whole():
    x = np.full(40, -1.0, dtype=np.float32)
    x[:3] = [4.0, 3.0, 3.0]
    x[10:16] = 2.0                      # six equal values straddle the 5th place
    t_k, _, t = NR.thresholds(x, T, 5, 1.0)
    assert t_k == 2.0 and t == 2.0 and int((x >= t).sum()) == 9
    assert NR.threshold_brute(x, T, 5, 1.0) == 2.0
    # top-p: the mass needed ends inside the tie at 3.0 -> both are kept
    w = np.exp((x.astype(np.float64) - 4.0) / 0.7)
    P = float((w[0] + 0.5 * w[1]) / w.sum())
    assert NR.thresholds(x, T, 0, P)[2] == 3.0 == NR.threshold_brute(x, T, 0, P)
    # the argmax is always kept, however small P is
    assert NR.thresholds(x, T, 0, 1e-6)[2] == 4.0
    # top-p applies to what top-k left, renormalised: over {4, 3, 3} the tail -1.0 carries no weight
    P2 = float((w[0] + 1.5 * w[1]) / w[:3].sum())
    assert NR.thresholds(x, T, 3, P2)[2] == 3.0


def test_constant_row_and_k_at_least_v():
    x = np.full(33, 1.5, dtype=np.float32)
    for K, P in ((0, 0.3), (5, 1.0), (5, 0.9), (33, 1.0), (40, 0.5)):
        assert NR.thresholds(x, T, K, P)[2] == 1.5 == NR.threshold_brute(x, T, K, P)
    y = _row(1, 50, 2.0)
    assert NR.thresholds(y, T, 50, 1.0)[2] == y.min() == NR.thresholds(y, T, 57, 1.0)[2] == NR.thresholds(y, T, 0, 1.0)[2]


def test_draw_over_with_everything_kept_is_the_plain_draw():
    x = np.stack([_row(s, 300, 2.0) for s in range(6)])
    pos = np.arange(100, 106)
    ids, gaps = NR.draw_over(x, x.min(axis=1), T, 9, SR.TARGET, pos)
    ref, rg = SR.draw(x, T, 9, SR.TARGET, pos)
    assert np.array_equal(ids, ref) and np.allclose(gaps, rg)
    one, g1 = NR.draw_over(x, x.max(axis=1), T, 9, SR.TARGET, pos)
    assert np.array_equal(one, x.argmax(axis=1)) and np.isinf(g1).all()


def test_entry_point_validates_without_a_gpu():
    from dflash_amd import _lib
    h = _lib.lib()

    def call(logits=1, ld=64, tstride=1024, tiles=1, V=64, row0=0, nrows=16, dyn=None, nword=-1, pword=-1, pbase=0,
             positions=None, padd=0, tpr=1, seeds=None, seed=1, kdev=None, k=0, pdev=None, p=1.0, inv_t=1.0, stream=0,
             extra=0, out=1, ostride=16, ooff=0, thr=None, kept=None):
        return h.dfl_sample_rows_nucleus(logits, ld, tstride, tiles, V, row0, nrows, dyn, nword, pword, pbase, positions,
                                         padd, tpr, seeds, seed, kdev, k, pdev, p, None, inv_t, stream, extra, out, ostride,
                                         ooff, thr, kept, None)

    assert call(tiles=0) == 0                       # nothing to do: no launch
    assert call(logits=None) == -22 and b"null" in h.dfl_last_error()
    assert call(out=None) == -22
    for p in (0.0, -0.1, 1.0001, float("nan")):
        assert call(p=p) == -22, p
    assert b"top_p" in h.dfl_last_error()
    assert call(k=-1) == -22 and b"top_k" in h.dfl_last_error()
    for it in (0.0, -1.0, 2e5):
        assert call(inv_t=it) == -22
    assert call(stream=2) == -22 and b"stream" in h.dfl_last_error()
    assert call(V=0) == -22 and call(V=200000, ld=200000) == -22 and call(ld=32) == -22
    assert call(row0=4, nrows=13) == -22 and call(tpr=3) == -22
    assert call(nword=2) == -22 and call(pword=3) == -22       # a record word without a record


def test_keyword_errors():
    from dflash_amd import ops
    from dflash_amd.batch import _prompt_filters
    from dflash_amd.engine import BatchEngine
    from dflash_amd.generate import resolve_filter
    from dflash_amd.slots import SlotLoop
    import torch
    assert resolve_filter(0, 1.0, T, "torch") is None and resolve_filter(0, 1.0, T, "device") is None
    assert resolve_filter(5, 0.9, 0.0, "torch") is None          # T = 0: accepted, the greedy path runs unchanged
    assert resolve_filter(5, 0.9, T, "device") == dict(top_k=5, top_p=0.9)
    with pytest.raises(ValueError, match="sampler"):
        resolve_filter(5, 1.0, T, "torch")
    with pytest.raises(ValueError, match="sampler"):
        resolve_filter(0, 0.9, T, "torch")
    for bad in (0.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="top_p"):
            resolve_filter(0, bad, T, "device")
        with pytest.raises(ValueError, match="top_p"):
            ops.check_filter(0, bad)
    with pytest.raises(ValueError, match="top_k"):
        resolve_filter(-1, 1.0, 0.0, "device")
    with pytest.raises(ValueError, match="top_k"):
        resolve_filter(2.5, 1.0, T, "device")
    assert _prompt_filters(0, 1.0, 3, T, "device") == ([0, 0, 0], [1.0, 1.0, 1.0], False)
    assert _prompt_filters([0, 5, 0], 0.9, 3, T, "device") == ([0, 5, 0], [0.9, 0.9, 0.9], True)
    assert _prompt_filters([0, 5, 0], 1.0, 3, 0.0, "torch")[2] is False
    with pytest.raises(ValueError, match="sampler"):
        _prompt_filters([0, 5], 1.0, 2, T, "torch")
    with pytest.raises(ValueError):
        _prompt_filters([0, 5], 1.0, 3, T, "device")

    class Dec:
        max_rows, out_len = 400, 400

    eng = BatchEngine.__new__(BatchEngine)        # no GPU here: the engine's queue alone
    eng.dec, eng.temperature, eng.filtering = Dec(), T, False
    eng.loop = SlotLoop(eng.dec, 2, 16)
    ids = torch.zeros(1, 20, dtype=torch.int64)
    assert eng.submit(ids, 10) == 0
    with pytest.raises(ValueError, match="filtering"):
        eng.submit(ids, 10, top_k=5)
    with pytest.raises(ValueError, match="top_p"):
        eng.submit(ids, 10, top_p=0.0)
    eng.filtering = True
    assert eng.submit(ids, 10, top_k=5, top_p=0.5) == 1
