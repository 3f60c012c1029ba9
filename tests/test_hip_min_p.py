"""dfl_min_p_rows alone against the numpy model of min_p_ref.py, bit for bit on the same bits: the
maximum, the two fp32 operations and the comparison, the copies (off, greedy, no finite maximum), the kept counts, the
layout; and the masked rows under the draw."""
import math

import numpy as np
import pytest
import torch

import min_p_ref as MR

pytestmark = pytest.mark.gpu
BF16, I32, I64, F32 = torch.bfloat16, torch.int32, torch.int64, torch.float32
SENT_BITS, SENT = 0x1234, -7
NAN_BITS = 0x7FC0
DYN_BS = 2


def dev():
    return torch.device("cuda", 0)


def to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev()).view(BF16)


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def d(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dt is None else t.to(dt)


def record(bs=16):
    return [0, 0, bs, 0, 0, 0, 0, 0]


def check_rows(x, got, kept, L, invT, rows=None):
    for m in (range(x.shape[0]) if rows is None else rows):
        want, k = MR.process(x[m], L, invT)
        assert np.array_equal(got[m], want), (m, np.nonzero(got[m] != want)[0][:5])
        assert MR.argmax_lowest(got[m]) == MR.argmax_lowest(x[m]), m
        if kept is not None:
            assert int(kept[m]) == k, (m, int(kept[m]), k)


# ------------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("V", [8, 8200, 2048, 151936, 155648])
def test_rows_against_the_model(V):
    """16 rows, host values, ld > V: the columns past V are not written, the raw rows stay, kept is the model's count.
    V = 8200: thread 0 makes a second trip; 155648: the 19th chunk of every thread."""
    from dflash_amd import ops
    rng = np.random.default_rng(V)
    ld = V + 24
    x = MR.case_rows(rng, 16, V)
    x[3, rng.choice(V, min(V, len(MR.SPECIALS)) - 2, replace=False)] = np.array(MR.SPECIALS[2:], dtype=np.uint16)[:max(V - 2, 0)]
    buf = to_bf16(np.full((16, ld), SENT_BITS, dtype=np.uint16))
    buf[:, :V].copy_(to_bf16(x))
    raw = buf.clone()
    obuf = to_bf16(np.full((16, ld), SENT_BITS, dtype=np.uint16))
    kept = torch.full((16,), SENT, dtype=I32, device=dev())
    T, mp = 0.7, 0.05
    out = ops.min_p_rows(buf[:, :V], min_p=mp, temperature=T, out=obuf[:, :V], kept=kept)
    assert out.data_ptr() == obuf.data_ptr()
    assert (bits_of(obuf[:, V:]) == SENT_BITS).all()
    assert torch.equal(buf.view(torch.int16), raw.view(torch.int16))
    k = kept.cpu().numpy()
    check_rows(x, bits_of(out), k, MR.log_min_p(mp), MR.inv_t(T))
    if V >= 2048:
        assert (k < V).all() and (k >= 1).all() and k.min() < V // 4     # the floor cuts through the bulk


def test_row_window_and_the_count_from_the_record():
    """row0 / nrows from the host (kept at kept[2 + m - 3]); then the valid count from a dyn word, row0 = 1."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(9)
    x = MR.case_rows(rng, 16, V)
    L, invT = MR.log_min_p(0.1), MR.inv_t(1.0)
    out = to_bf16(np.full_like(x, SENT_BITS))
    kept = torch.full((16,), SENT, dtype=I32, device=dev())
    ops.min_p_rows(to_bf16(x), min_p=0.1, temperature=1.0, out=out, row0=3, nrows=5, kept=kept, kept_off=2)
    got, k = bits_of(out), kept.cpu().numpy()
    for m in range(16):
        if 3 <= m < 8:
            want, n = MR.process(x[m], L, invT)
            assert np.array_equal(got[m], want) and k[2 + m - 3] == n
        else:
            assert (got[m] == SENT_BITS).all()
    assert (k[:2] == SENT).all() and (k[7:] == SENT).all()
    # two tiles, counts 11 and 0 from the record
    x2 = np.stack([x, MR.case_rows(rng, 16, V)])
    out = to_bf16(np.full_like(x2, SENT_BITS))
    kept = torch.full((2, 16), SENT, dtype=I32, device=dev())
    dyn = d(np.array([record(11), record(0)], dtype=np.int32))
    ops.min_p_rows(to_bf16(x2), min_p=0.1, temperature=1.0, out=out, row0=1, nrows=15, dyn=dyn, nrows_dyn_word=DYN_BS,
                   kept=kept)
    got, k = bits_of(out), kept.cpu().numpy()
    check_rows(x2[0], np.concatenate([got[0]]), None, L, invT, rows=range(1, 11))
    assert (got[0, 0] == SENT_BITS).all() and (got[0, 11:] == SENT_BITS).all() and (got[1] == SENT_BITS).all()
    assert all(k[0, m - 1] == MR.process(x2[0, m], L, invT)[1] for m in range(1, 11))
    assert (k[0, 10:] == SENT).all() and (k[1] == SENT).all()


@pytest.mark.parametrize("tpr", [1, 2])
def test_four_tiles_with_device_values(tpr):
    """Four tiles with (L, invT) per slot from device arrays; an off slot (-inf) and a greedy slot (invT = 0) have their
    rows NaN-prefilled in `out` and must come back as copies reporting V.  tiles_per_req = 2: tiles 2q, 2q + 1 -> slot q."""
    from dflash_amd import ops
    V, T = 2048, 4
    rng = np.random.default_rng(21 + tpr)
    x = np.stack([MR.case_rows(rng, 16, V) for _ in range(T)])
    if tpr == 1:
        L = np.array([math.log(0.2), -np.inf, math.log(0.01), math.log(0.9)], dtype=np.float32)
        invT = np.array([1.0 / 0.7, 1.25, 0.0, 0.5], dtype=np.float32)
    else:   # two slots in use, the other two array entries belong to no tile of this launch
        L = np.array([math.log(0.2), math.log(0.03), 0.5, np.nan], dtype=np.float32)
        invT = np.array([1.0 / 0.7, 2.0, -1.0, np.nan], dtype=np.float32)
    out = to_bf16(np.full_like(x, NAN_BITS))
    kept = torch.full((T, 16), SENT, dtype=I32, device=dev())
    ops.min_p_rows(to_bf16(x), log_min_p=d(L), inv_t=d(invT), out=out, tiles_per_req=tpr, kept=kept)
    got, k = bits_of(out), kept.cpu().numpy()
    for t in range(T):
        q = t // tpr
        check_rows(x[t], got[t], k[t], L[q], invT[q])
    if tpr == 1:
        assert np.array_equal(got[1], x[1]) and np.array_equal(got[2], x[2]) and (k[1:3] == V).all()
        assert (k[0] < V).all() and (k[3] < 64).all()
    else:
        assert not np.array_equal(got[2], MR.process(x[2, 0], L[0], invT[0])[0]) and (k[2] < V).all()
    # every other bit pattern a device array may hold reads as off / greedy: copies
    for Lb, ib in ((0.5, 1.0), (np.nan, 1.0), (np.float32(1e-38), 1.0), (-1.0, -2.0), (-1.0, np.nan), (-1.0, -0.0)):
        o = ops.min_p_rows(to_bf16(x[0]), log_min_p=d(np.array([Lb], dtype=np.float32)),
                           inv_t=d(np.array([ib], dtype=np.float32)), kept=kept[0])
        assert np.array_equal(bits_of(o), x[0]) and (kept[0] == V).all()


def test_in_place():
    from dflash_amd import ops
    V = 8200
    x = MR.case_rows(np.random.default_rng(2), 16, V)
    buf = to_bf16(x)
    out = ops.min_p_rows(buf, min_p=0.2, temperature=0.7, out=buf)
    assert out.data_ptr() == buf.data_ptr()
    check_rows(x, bits_of(buf), None, MR.log_min_p(0.2), MR.inv_t(0.7))


def test_the_exact_boundary():
    """invT = 0.5, L = -2: a column at m - 4 gives d = -2 exactly and is kept; one at m - 4.03125 is dropped."""
    from dflash_amd import ops
    V = 2048
    x = np.full((1, V), 0xC2C8, dtype=np.uint16)      # -100
    x[0, 1000] = MR.to_bits(np.float32(8.0))
    x[0, 7] = MR.to_bits(np.float32(4.0))
    x[0, 2040] = MR.to_bits(np.float32(3.96875))
    kept = torch.full((1,), SENT, dtype=I32, device=dev())
    got = bits_of(ops.min_p_rows(to_bf16(x), log_min_p=d(np.array([-2.0], dtype=np.float32)),
                                 inv_t=d(np.array([0.5], dtype=np.float32)), kept=kept))
    assert got[0, 7] == x[0, 7] and got[0, 2040] == 0xFF80 and got[0, 1000] == x[0, 1000] and int(kept[0]) == 2
    assert np.array_equal(got[0], MR.process(x[0], -2.0, 0.5)[0])
    # a product that rounds: the model's two roundings, not a fused one (the whole neighbourhood of the threshold)
    rng = np.random.default_rng(12)
    y = MR.case_rows(rng, 16, V, scale=1.0)
    for T, mp in ((0.7, 0.3), (0.3, 0.9), (1.9, 0.011)):
        got = bits_of(ops.min_p_rows(to_bf16(y), min_p=mp, temperature=T))
        check_rows(y, got, None, MR.log_min_p(mp), MR.inv_t(T))


def test_ties_and_the_maximum_in_the_last_column():
    from dflash_amd import ops
    V = 8200
    rng = np.random.default_rng(6)
    x = MR.case_rows(rng, 4, V)
    top = MR.to_bits(np.float32(40.0))
    x[0, [3, 8 * 70 + 1, 8 * 1024 + 5, V - 1]] = top      # tied across threads and waves (chunks 0, 70, 1024, 1024)
    x[1, V - 1] = top                                     # the maximum in the last column
    x[2, 0], x[2, 4097] = 0x0000, 0x8000                  # the maximum is zero, in both signs
    x[2, (np.arange(V) != 0) & (np.arange(V) != 4097)] |= 0x8000
    x[2][MR.widen(x[2]) == 0] = 0x8000
    x[2, 0] = 0x0000
    kept = torch.full((4,), SENT, dtype=I32, device=dev())
    got = bits_of(ops.min_p_rows(to_bf16(x), min_p=1.0, temperature=0.7, kept=kept))
    k = kept.cpu().numpy()
    check_rows(x, got, k, 0.0, MR.inv_t(0.7))
    assert k[0] == 4 and k[1] == 1 and got[1, V - 1] == top and (got[1, :V - 1] == 0xFF80).all()
    assert k[2] >= 2 and got[2, 0] == 0x0000 and got[2, 4097] == 0x8000        # bits copied: -0 stays -0


def test_nan_and_infinities():
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(8)
    x = MR.case_rows(rng, 6, V)
    x[0, [5, 900, 901]] = [0x7FC1, 0xFFFF, 0xFF80]        # NaNs keep their bits, -inf stays; the rest is masked
    x[1, 77] = 0x7F80                                     # +inf: no finite maximum, the row is copied
    x[1, 78] = 0x7FC1
    x[2, :] = 0xFF80                                      # all -inf: copied
    x[3, :] = 0x7FC1                                      # all NaN: copied
    x[4, :] = 0xFF80
    x[4, 1500] = 0xC2C8                                   # one finite value among -inf
    x[5, :] = 0x7FC1
    x[5, 3], x[5, 4] = MR.to_bits(np.float32(2.0)), MR.to_bits(np.float32(-30.0))   # two finite values among NaNs
    out = to_bf16(np.full_like(x, SENT_BITS))
    kept = torch.full((6,), SENT, dtype=I32, device=dev())
    ops.min_p_rows(to_bf16(x), min_p=0.5, temperature=1.0, out=out, kept=kept)
    got, k = bits_of(out), kept.cpu().numpy()
    check_rows(x, got, k, MR.log_min_p(0.5), MR.inv_t(1.0))
    assert got[0, 5] == 0x7FC1 and got[0, 900] == 0xFFFF and got[0, 901] == 0xFF80 and k[0] < V - 3
    for m in (1, 2, 3):
        assert np.array_equal(got[m], x[m]) and k[m] == V
    assert k[4] == 1 and got[4, 1500] == 0xC2C8
    assert k[5] == 1 and got[5, 4] == 0xFF80 and (got[5, 5:] == 0x7FC1).all()


@pytest.mark.parametrize("min_p", [0.01, 0.2, 0.9])
def test_random_rows_full_vocabulary(min_p, full_rows):
    """16 x 151936: every element's bits, the counts, and the same bits on every run."""
    from dflash_amd import ops
    x = full_rows(151936)
    kept = torch.full((16,), SENT, dtype=I32, device=dev())
    args = dict(min_p=min_p, temperature=0.7, kept=kept)
    got = bits_of(ops.min_p_rows(to_bf16(x), **args))
    check_rows(x, got, kept.cpu().numpy(), MR.log_min_p(min_p), MR.inv_t(0.7))
    for _ in range(2):                                    # the same bits on every run
        assert np.array_equal(bits_of(ops.min_p_rows(to_bf16(x), **args)), got)


@pytest.fixture(scope="module")
def full_rows():
    cache = {}

    def rows(V):
        if V not in cache:
            cache[V] = MR.case_rows(np.random.default_rng(V), 16, V)
        return cache[V]
    return rows


def test_the_draw_over_the_masked_rows():
    """The masked rows under dfl_sample_rows_nucleus give the ids of the reference draw over the model's masked rows: with
    top_p the nucleus takes its mass over what min_p kept."""
    import sampling_ref as SR
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(31)
    x = MR.case_rows(rng, 16, V, scale=2.0)
    T, mp, seed, pos0 = 0.7, 0.2, 1234, 50
    masked = ops.min_p_rows(to_bf16(x), min_p=mp, temperature=T)
    want_bits = np.stack([MR.process(x[m], MR.log_min_p(mp), MR.inv_t(T))[0] for m in range(16)])
    assert np.array_equal(bits_of(masked), want_bits)
    want_rows = to_bf16(want_bits)
    for flt in (dict(top_k=0, top_p=1.0), dict(top_k=0, top_p=0.9), dict(top_k=3, top_p=1.0)):
        ids = ops.sample_rows_nucleus(masked, seed=seed, temperature=T, pos_base=pos0, **flt)
        ref = ops.sample_rows_nucleus(want_rows, seed=seed, temperature=T, pos_base=pos0, **flt)
        assert torch.equal(ids, ref)
        idn = ids.cpu().numpy()
        for m in range(16):
            assert want_bits[m, idn[m]] != 0xFF80, m      # never a masked column
        if flt == dict(top_k=0, top_p=1.0):               # the host draw over the model's rows (its float64 stands in for
            # the kernel's fp32 fma: rows whose two best perturbed values lie within 1e-3 are not compared)
            host, gaps = SR.draw(MR.widen(want_bits), T, seed, SR.TARGET, np.arange(pos0, pos0 + 16))
            safe = gaps > 1e-3
            assert safe.sum() >= 12 and np.array_equal(idn[safe], host[safe])
    # the floor changes what a plain draw would pick somewhere among 16 rows at min_p = 0.9 (nearly greedy)
    hard = ops.min_p_rows(to_bf16(x), min_p=0.9, temperature=T)
    a = ops.sample_rows_nucleus(hard, seed=seed, temperature=T, pos_base=pos0).cpu().numpy()
    b = ops.sample_rows_nucleus(to_bf16(x), seed=seed, temperature=T, pos_base=pos0).cpu().numpy()
    assert (a != b).any()
    kept = [MR.process(x[m], MR.log_min_p(0.9), MR.inv_t(T))[1] for m in range(16)]
    assert sum(k == 1 for k in kept) >= 8
    assert all(a[m] == MR.argmax_lowest(x[m]) for m in range(16) if kept[m] == 1)   # one column left: the draw is forced
