"""dfl_logprob_rows on the GPU against the NumPy fp64 reference (logprobs_ref.py).  Each test is one
or two launches of 16 rows.

Tolerance, derived (logprobs_ref.tolerance): |kernel - reference| <= 2^-16 + 2^-22 |lse|.  The kernel sums as the issue
fixes it — per thread sequentially in column order (at most 152 terms), the wave's butterfly, 16 wave sums in order — so
the bound is the issue's own."""
import numpy as np
import pytest
import torch

import logprobs_ref as LR

pytestmark = pytest.mark.gpu
BF16, F32, I64, I32 = torch.bfloat16, torch.float32, torch.int64, torch.int32
WIDTHS = [16, 8200, 151936, 155648]
SENT_LP, SENT_ID = -777.0, -555


def dev():
    return torch.device("cuda", 0)


def _sink(slots, length, n_top):
    """A sink whose every entry holds a sentinel, so that an entry the launch must not write shows."""
    from dflash_amd import ops
    s = ops.logprob_sink(slots, length, n_top, dev())
    s.lp.fill_(SENT_LP)
    if n_top:
        s.top_ids.fill_(SENT_ID)
        s.top_lp.fill_(SENT_LP)
    return s


def _launch(x, ids, n_top=8, pos_base=0, length=64, **kw):
    """x float32 [16, V] of bf16-representable values; returns (lp [16], top_ids [16, n], top_lp [16, n]) at the
    positions pos_base + m, and the sink."""
    from dflash_amd import ops
    xg = torch.from_numpy(x).to(dev()).to(BF16)
    s = _sink(1, length, n_top)
    ops.logprob_rows(xg, torch.as_tensor(ids, dtype=I64).to(dev()), s, pos_base=pos_base, **kw)
    torch.cuda.synchronize()
    return s


def _check_rows(x, ids, s, pos, n_top, rows=None):
    """Rows `rows` of x against the reference at positions pos[m] of the sink's row 0; the worst error / bound ratio."""
    lp = s.lp[0].cpu().numpy().astype(np.float64)
    worst = 0.0
    for m in (range(x.shape[0]) if rows is None else rows):
        ref_lse = LR.lse(x[m])
        tol = LR.tolerance(ref_lse)
        ref = LR.logprob(x[m], int(ids[m]))
        got = lp[pos[m]]
        if np.isfinite(ref):
            worst = max(worst, abs(got - ref) / tol)
            assert abs(got - ref) <= tol, (m, got, ref, tol)
        else:
            assert (np.isnan(ref) and np.isnan(got)) or got == ref, (m, got, ref)
        if n_top:
            rid, rlp = LR.top(x[m], n_top)
            gid = s.top_ids[0, pos[m]].cpu().numpy()
            glp = s.top_lp[0, pos[m]].cpu().numpy().astype(np.float64)
            assert np.array_equal(gid, rid), (m, gid, rid)
            fin = np.isfinite(rlp)
            assert (np.abs(glp[fin] - rlp[fin]) <= tol).all(), (m, glp, rlp)
            assert all((np.isnan(a) and np.isnan(b)) or a == b for a, b in zip(glp[~fin], rlp[~fin])), (m, glp, rlp)
    print(f"[logprobs] worst |error| / bound = {worst:.3f}")
    return worst


def _needle_columns(V):
    """Columns where a dropped or doubled column would show: the row's ends, the edges of a 16-byte chunk, of a wave's
    share (64 chunks = 512 columns), of a thread's second chunk (8192), and the last chunk."""
    cols = [0, 7, 8, 511, 512, 8191, 8192, 8199, V - 8, V - 1, 65535, 65536, 8 * 1023, 8 * 1023 + 7, 18 * 8192, 18 * 8192 + 7]
    cols = sorted({c for c in cols if 0 <= c < V})
    return (cols * 16)[:16] if len(cols) < 16 else cols[:16]


@pytest.mark.parametrize("V", WIDTHS)
def test_needle_rows(V):
    """Every column -30 but one at +10: lse = log(e^10 + (V - 1) e^-30) ~ 10, so a kernel that drops the needle's column
    is off by about 28 (lse ~ -30 + log V) and one that counts it twice by log 2."""
    cols = _needle_columns(V)
    x = np.full((16, V), -30.0, dtype=np.float32)
    for m, c in enumerate(cols):
        x[m, c] = 10.0
    ids = np.array(cols)
    ids[1::2] = (ids[1::2] + 1) % V          # odd rows ask for a neighbour of the needle: lp ~ -40
    s = _launch(x, ids, n_top=2)
    _check_rows(x, ids, s, list(range(16)), 2)
    assert (s.top_ids[0, :16, 0].cpu().numpy() == np.array(cols)).all()


@pytest.mark.parametrize("V", WIDTHS)
def test_random_rows_and_top8(V):
    """randn * 4 rounded to bf16.  The top-9 values of every row are made distinct bf16 values (the largest nine get a
    ladder of exactly representable steps), so the top-8 ids are exact."""
    rng = np.random.default_rng(V)
    x = LR.bf16_round(rng.standard_normal((16, V)).astype(np.float32) * 4.0)
    n9 = min(9, V)
    for m in range(16):
        top = np.argsort(-x[m], kind="stable")[:n9]
        x[m, top] = 24.0 - 0.25 * np.arange(n9, dtype=np.float32)    # 24, 23.75, ...: exact in bf16, above every randn * 4
    ids = rng.integers(0, V, size=16)
    ids[0], ids[1] = 0, V - 1
    s = _launch(x, ids, n_top=8)
    _check_rows(x, ids, s, list(range(16)), 8)
    s0 = _launch(x, ids, n_top=0)               # n_top = 0 skips the rounds: same lp bits
    assert torch.equal(s0.lp, s.lp) and s0.top_ids is None


@pytest.mark.parametrize("V", [16, 8200])
def test_special_rows(V):
    """-inf columns, a constant row, a row of +-0, a row with no finite value, exact ties for the top-N."""
    rng = np.random.default_rng(5)
    x = LR.bf16_round(rng.standard_normal((16, V)).astype(np.float32) * 4.0)
    x[0, ::3] = -np.inf                                  # -inf entries contribute 0
    x[1, :] = 1.5                                        # all equal: lp = -log V, top ids 0..7
    x[2, :] = 0.0
    x[2, 1::2] = -0.0                                    # +-0 are one value: top ids 0..7
    x[3, :] = -np.inf                                    # no finite value: lse = -inf, lp = NaN
    x[4, :] = -np.inf
    x[4, V - 1] = -2.0                                   # one finite value: lp = 0 there
    x[5, :] = -3.0
    x[5, [V - 1, 3, V // 2, 9]] = 7.0                    # ties: index order
    x[6, :] = 2.0
    x[6, 5] = -np.inf
    x[7, :8] = np.array([5, 5, 4, 4, 4, 3, 3, 3], dtype=np.float32) + 20.0
    ids = rng.integers(0, V, size=16)
    ids[0], ids[3], ids[4], ids[6] = 0, 2, V - 1, 5      # a -inf column, the all -inf row, the lone value, a -inf column
    s = _launch(x, ids, n_top=8)
    _check_rows(x, ids, s, list(range(16)), 8)
    lp = s.lp[0, :16].cpu().numpy()
    assert lp[0] == -np.inf and np.isnan(lp[3]) and lp[4] == 0.0 and lp[6] == -np.inf
    assert abs(lp[1] + np.log(V)) <= LR.tolerance(np.log(V) + 1.5)
    assert s.top_ids[0, 1].tolist() == list(range(8)) and s.top_ids[0, 2].tolist() == list(range(8))
    assert s.top_ids[0, 5, :4].tolist() == sorted([V - 1, 3, V // 2, 9])
    assert s.top_ids[0, 7].tolist() == list(range(8))
    assert s.top_ids[0, 4, 0].item() == V - 1 and s.top_lp[0, 4, 0].item() == 0.0


def test_every_bit_pattern_is_defined():
    """All 65536 bf16 patterns in one row (NaNs and both infinities among them): nothing traps, the lse is that of the
    finite ones, and the order places +NaN above +inf."""
    from dflash_amd import ops
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16)
    xg = bits.repeat(16, 1).to(dev())
    s = _sink(1, 32, 2)
    ids = torch.full((16,), 0x3F80, dtype=I64, device=dev())      # the pattern of 1.0
    ops.logprob_rows(xg, ids, s)
    torch.cuda.synchronize()
    x = bits.view(torch.int16).to(torch.int32).numpy().astype(np.uint32) << 16
    x = x.view(np.float32)[:65536]
    ref = 1.0 - LR.lse(x)                                         # (lse ~ 3.39e38 ~ the largest bf16: lp ~ -3.39e38)
    got = s.lp[0, 0].item()
    assert abs(got - ref) <= LR.tolerance(LR.lse(x)) and torch.equal(s.lp[0, :16], s.lp[0, :1].expand(16))
    top = s.top_ids[0, 0].tolist()
    assert top == [0x7FFF, 0x7FFE]                                # the NaNs with the sign clear sort first, largest payload first
    assert np.isnan(s.top_lp[0, 0].cpu().numpy()).all()


def test_out_of_range_ids_write_nan_and_rows_past_the_count_write_nothing():
    V = 8200
    x = LR.bf16_round(np.random.default_rng(2).standard_normal((16, V)).astype(np.float32))
    ids = np.arange(16) * 7
    ids[2], ids[3], ids[4] = -1, V, 2 ** 40
    s = _launch(x, ids[4:], n_top=1, row0=4, nrows=9, pos_base=10)   # rows 4..12 write at 14..22; ids indexed from row0
    lp = s.lp[0].cpu().numpy()
    assert np.isnan(lp[14]) and np.isfinite(lp[15:23]).all()
    assert (lp[:14] == SENT_LP).all() and (lp[23:] == SENT_LP).all()
    assert (s.top_ids[0, :14] == SENT_ID).all() and (s.top_ids[0, 23:] == SENT_ID).all()
    x2 = x.copy()
    _check_rows(x2, np.concatenate([np.zeros(4, dtype=np.int64), ids[4:]]), s, [10 + m for m in range(16)], 1,
                rows=range(5, 13))
    s = _launch(x, ids, n_top=0, nrows=5, pos_base=3)
    lp = s.lp[0].cpu().numpy()
    assert np.isnan(lp[5:8]).all() and np.isfinite(lp[3:5]).all()          # ids -1, V and 2^40 at rows 2, 3, 4
    assert (lp[:3] == SENT_LP).all() and (lp[8:] == SENT_LP).all()


def test_positions_past_the_buffer_write_nothing():
    V = 16
    x = LR.bf16_round(np.random.default_rng(3).standard_normal((16, V)).astype(np.float32))
    ids = np.arange(16) % V
    s = _launch(x, ids, n_top=3, pos_base=20, length=28)             # rows 8..15 fall at 28..35: dropped
    lp = s.lp[0].cpu().numpy()
    assert (lp[:20] == SENT_LP).all() and np.isfinite(lp[20:28]).all()
    _check_rows(x, ids, s, [20 + m for m in range(16)], 3, rows=range(8))
    s = _launch(x, ids, n_top=3, pos_base=-4, length=28)             # rows 0..3 fall before the buffer: dropped
    lp = s.lp[0].cpu().numpy()
    assert np.isfinite(lp[:12]).all() and (lp[12:] == SENT_LP).all()
    _check_rows(x, ids, s, [m - 4 for m in range(16)], 3, rows=range(4, 16))


def test_records_slots_and_two_tiles_per_request():
    """Six tiles = three slots of two tiles each; row counts and positions come from the record (words BS and POS0, three
    different POS0), ids with a row stride and an offset; every entry the launch does not own keeps its sentinel."""
    from dflash_amd import ops
    V, n_top, L = 8200, 2, 96
    rng = np.random.default_rng(9)
    x = LR.bf16_round(rng.standard_normal((6, 16, V)).astype(np.float32) * 3.0)
    for t in range(6):
        for m in range(16):
            top = np.argsort(-x[t, m], kind="stable")[:3]
            x[t, m, top] = 20.0 - np.arange(3, dtype=np.float32)
    counts = [16, 5, 16, 0, 9, 0]                       # slot 0: 21 rows, slot 1: 16, slot 2: 9
    pos0 = [30, 30, 7, 7, 55, 55]
    dyn = torch.zeros(6, 8, dtype=I32)
    for t in range(6):
        dyn[t, ops.DYN_BS], dyn[t, ops.DYN_POS0] = counts[t], pos0[t]
    ids = rng.integers(0, V, size=(6, 20))
    xg = torch.from_numpy(x).to(dev()).to(BF16)
    s = _sink(3, L, n_top)
    ops.logprob_rows(xg, torch.from_numpy(ids).to(dev()), s, ids_off=2, dyn=dyn.to(dev()), nrows_dyn_word=ops.DYN_BS,
                     pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=2)
    torch.cuda.synchronize()
    owned = torch.zeros(3, L, dtype=torch.bool)
    for t in range(6):
        q, j = divmod(t, 2)
        for m in range(counts[t]):
            p = LR.position(pos0[t], 1, j, m)
            owned[q, p] = True
            ref = LR.logprob(x[t, m], int(ids[t, 2 + m]))
            assert abs(s.lp[q, p].item() - ref) <= LR.tolerance(LR.lse(x[t, m])), (t, m)
            rid, rlp = LR.top(x[t, m], n_top)
            assert s.top_ids[q, p].tolist() == rid.tolist(), (t, m)
            assert (np.abs(s.top_lp[q, p].cpu().numpy() - rlp) <= LR.tolerance(LR.lse(x[t, m]))).all()
    assert owned.sum().item() == sum(counts)
    assert (s.lp.cpu()[~owned] == SENT_LP).all() and (s.top_ids.cpu()[~owned] == SENT_ID).all()
    assert (s.top_lp.cpu()[~owned] == SENT_LP).all()
    # the sink's slot offset: one tile into row 2 of the same sink
    s2 = _sink(3, L, n_top)
    s2.slot = 2
    ops.logprob_rows(xg[0], torch.from_numpy(ids[0]).to(dev()), s2, ids_off=2, nrows=3, pos_base=40)
    torch.cuda.synchronize()
    assert (s2.lp[:2] == SENT_LP).all() and torch.equal(s2.lp[2, 40:43], s.lp[0, 31:34])


def test_rows_that_do_not_start_on_16_bytes_and_a_row_stride():
    """A view with ld > V whose rows start 2 bytes off a 16-byte boundary: the column-by-column load path."""
    from dflash_amd import ops
    V = 8200
    rng = np.random.default_rng(4)
    x = LR.bf16_round(rng.standard_normal((16, V)).astype(np.float32) * 4.0)
    for m in range(16):
        top = np.argsort(-x[m], kind="stable")[:4]
        x[m, top] = 22.0 - np.arange(4, dtype=np.float32)
    big = torch.full((16, V + 11), 30.0, dtype=BF16, device=dev())   # (what lies outside the row would change every lse)
    big[:, 1:V + 1] = torch.from_numpy(x).to(dev()).to(BF16)
    ids = rng.integers(0, V, size=16)
    s = _sink(1, 32, 3)
    ops.logprob_rows(big[:, 1:V + 1], torch.from_numpy(ids).to(dev()), s)
    torch.cuda.synchronize()
    _check_rows(x, ids, s, list(range(16)), 3)


def test_two_launches_are_bit_equal():
    V = 151936
    rng = np.random.default_rng(6)
    xg = torch.from_numpy(rng.standard_normal((16, V)).astype(np.float32) * 4.0).to(dev()).to(BF16)
    ids = torch.from_numpy(rng.integers(0, V, size=16)).to(dev())
    from dflash_amd import ops
    a, b = _sink(1, 16, 8), _sink(1, 16, 8)
    ops.logprob_rows(xg, ids, a)
    ops.logprob_rows(xg, ids, b)
    torch.cuda.synchronize()
    assert torch.equal(a.lp.view(I32), b.lp.view(I32)) and torch.equal(a.top_ids, b.top_ids)
    assert torch.equal(a.top_lp.view(I32), b.top_lp.view(I32))
    assert torch.isfinite(a.lp).all()
