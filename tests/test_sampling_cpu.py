"""The seeded sampler's generator mirror (tests/sampling_ref.py) and its C-ABI entry points, without a GPU."""
import numpy as np

import sampling_ref as SR


def test_philox_known_answers():
    """Random123's published Philox4x32-10 vectors (kat_vectors: zero, all-ones and pi-digit inputs)."""
    def one(ctr, key):
        out = SR.philox4x32_10(*[np.uint32(c) for c in ctr], (key[1] << 32) | key[0])
        return [int(x) for x in out]
    assert one([0, 0, 0, 0], [0, 0]) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    assert one([0xFFFFFFFF] * 4, [0xFFFFFFFF, 0xFFFFFFFF]) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert one([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0]) == \
        [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]


def test_uniform_is_deterministic_and_separates_its_inputs():
    v = np.arange(4096)
    a = SR.uniform(7, SR.TARGET, 100, v)
    assert np.array_equal(a, SR.uniform(7, SR.TARGET, 100, v))
    for other in (SR.uniform(8, SR.TARGET, 100, v), SR.uniform(7, SR.DRAFT, 100, v), SR.uniform(7, SR.TARGET, 101, v),
                  SR.uniform(7, SR.TARGET, 100, v, extra=1), SR.uniform(7, SR.TARGET, 100, v + 4096),
                  SR.uniform(7 + (1 << 32), SR.TARGET, 100, v)):
        assert np.mean(a == other) < 0.01
    # the four columns of a group come from four different words of one call
    assert len(set(a[:4].tolist())) == 4


def test_uniform_stays_strictly_inside_the_unit_interval():
    w = np.array([0, 1, 511, 512, 0x7FFFFFFF, 0xFFFFFDFF, 0xFFFFFE00, 0xFFFFFFFF], dtype=np.uint32)
    u = (w >> np.uint32(9)).astype(np.float32) * np.float32(2.0 ** -23) + np.float32(2.0 ** -24)
    assert u.min() == np.float32(2.0 ** -24) and u.max() == np.float32(1 - 2.0 ** -24)
    assert np.all((u > 0) & (u < 1)) and np.all(np.isfinite(-np.log(-np.log(u))))
    big = SR.uniform(3, SR.TARGET, np.arange(250)[:, None], np.arange(4000)[None, :])
    assert big.dtype == np.float32 and np.all((big > 0) & (big < 1))


def test_uniform_moments_over_a_million_draws():
    u = SR.uniform(12345, SR.TARGET, np.arange(1000)[:, None], np.arange(1000)[None, :]).astype(np.float64)
    assert u.size == 10 ** 6
    assert abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12 / u.size)
    assert abs(u.var() - 1 / 12) < 1e-3
    g = SR.gumbel(12345, SR.TARGET, np.arange(1000)[:, None], np.arange(1000)[None, :]).astype(np.float64)
    assert abs(g.mean() - 0.5772156649) < 0.01 and abs(g.var() - np.pi ** 2 / 6) < 0.03


def test_gumbel_max_draw_follows_softmax():
    """The mirror's draw itself: Gumbel-max over bf16 logits / T is a softmax(logits / T) sample."""
    rng = np.random.default_rng(0)
    logits = SR.bf16_round(rng.normal(0, 1.5, 64).astype(np.float32))
    T, n = 0.7, 40000
    ids, _ = SR.draw(np.repeat(logits[None], n, 0), T, 99, SR.TARGET, np.arange(n))
    p = np.exp(logits.astype(np.float64) * float(SR.inv_t(T)))
    p /= p.sum()
    cnt = np.bincount(ids, minlength=64)
    keep = p * n >= 5
    chi2 = float((((cnt - n * p) ** 2) / (n * p))[keep].sum())
    dof = int(keep.sum()) - 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)


def test_sampling_entry_points_validate_without_gpu():
    from dflash_amd import _lib
    h = _lib.lib()
    assert h.dfl_sample_rows(None, 16, 1, 16, 1, 1.0, 0, 0, None, 0, None, None, None) == -22
    assert b"null" in h.dfl_last_error()
    assert h.dfl_sample_rows(1, 16, 1, 16, 1, 0.0, 0, 0, None, 0, 1, None, None) == -22   # T = inf
    assert h.dfl_sample_rows(1, 16, 1, 16, 1, 1.0, 7, 0, None, 0, 1, None, None) == -22   # unknown stream
    assert h.dfl_gemm_sample(None, None, 16, 32, 0, 16, None, -1, None, None, 0, None, None, 1, 1.0, 0, None, 3, 0, 0,
                             None) == -22
    assert h.dfl_gemm_sample(_lib.Weight(1, None, _lib.W_BF16), None, 16, 32, 0, 16, None, -1, 1, 1, 0, None, None, 1, -1.0, 0, None, 3, 0, 0, None) == -22
