"""dfl_penalty_count and dfl_penalty_rows alone against the numpy model of penalties_ref.py: the
table exactly, the penalised rows bit for bit (either neighbour where step 3 sits within 1e-6 of a bf16 midpoint, at most
1e-3 of the elements), the argmax ids against the kernel's own rows."""
import numpy as np
import pytest
import torch

import penalties_ref as PR

pytestmark = pytest.mark.gpu
BF16, I32, I64, F32 = torch.bfloat16, torch.int32, torch.int64, torch.float32
SENT_BITS, SENT_ID = 0x1234, -7


def dev():
    return torch.device("cuda", 0)


def to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev()).view(BF16)


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def record(S=0, bs=16, start=0):
    return [S, 0, bs, S, start, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("V", [48, 2048])
def test_count_host_ranges(V):
    """Clear + prompt + output ranges from host values, duplicates, ids outside [0, V), two slots in one launch."""
    from dflash_amd import ops
    rng = np.random.default_rng(V)
    n = 300
    ids = rng.integers(0, V, (2, n)).astype(np.int64)
    ids[:, 10:20] = ids[:, 0:1]                         # duplicates, in the prompt and in the output
    ids[:, 150:170] = ids[:, 149:150]
    ids[0, [5, 120, 130]] = [-1, V, 2 ** 40]            # outside the vocabulary: not counted, never indexed
    ids[1, [7, 140]] = [V + 5, -(2 ** 33)]
    table = torch.full((2, V), 7, dtype=I32, device=dev())          # garbage the clear has to remove
    d_ids = torch.from_numpy(ids).to(dev())
    ops.penalty_count(table, d_ids, lo=0, hi=100, as_prompt=True, clear=True)
    want = np.stack([PR.table_of(ids[s], 100, 100, V) for s in range(2)])
    assert np.array_equal(table.cpu().numpy(), want)
    ops.penalty_count(table, d_ids, lo=100, hi=250)
    ops.penalty_count(table[1:], d_ids[1:], lo=250, hi=10 ** 6)     # one slot; the range is clamped to the ids
    want = np.stack([PR.table_of(ids[0], 100, 250, V), PR.table_of(ids[1], 100, n, V)])
    got = table.cpu().numpy()
    assert np.array_equal(got, want)
    u = got.view(np.uint32)
    if V > 48:   # prompt-only, output-only and mixed entries, and a count of 20 or more
        assert (u == 0x80000000).any() and ((u > 0) & (u < 0x80000000)).any() and (u > 0x80000000).any()
    assert (u & 0x7FFFFFFF).max() >= 20
    # a second prompt pass changes nothing (or), a second output pass counts again (add)
    ops.penalty_count(table, d_ids, lo=0, hi=100, as_prompt=True)
    assert np.array_equal(table.cpu().numpy(), want)


def test_count_record_ranges_and_idle_slot():
    """The range from two words of the slot's length record plus host addends: behind an accept launch, (S, START].  A slot
    whose BS word is 0 is skipped whole — counts and clear — and stays bit-identical."""
    from dflash_amd import ops
    V, n = 2048, 400
    rng = np.random.default_rng(1)
    ids = rng.integers(0, V, (3, n)).astype(np.int64)
    ids[0, 125:130] = ids[0, 121]
    d_ids = torch.from_numpy(ids).to(dev())
    before = rng.integers(0, 9, (3, V)).astype(np.int32)
    before[:, ::3] |= np.int32(-2 ** 31)
    table = torch.from_numpy(before).to(dev())
    dyn = torch.tensor([record(120, 16, 137), record(5, 0, 60), record(300, 9, 301)], dtype=I32, device=dev())
    ops.penalty_count(table, d_ids, dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START, lo=1, hi=1)
    got = table.cpu().numpy()
    assert np.array_equal(got[1], before[1])
    for s, (lo, hi) in ((0, (121, 138)), (2, (301, 302))):
        want = before[s].view(np.uint32).copy()
        np.add.at(want, ids[s, lo:hi], np.uint32(1))
        assert np.array_equal(got[s].view(np.uint32), want), s
    # clear + prompt in the record form: the idle slot keeps its row
    ops.penalty_count(table, d_ids, dyn=dyn, lo_word=ops.DYN_STOP, hi_word=ops.DYN_S, lo=0, hi=0, as_prompt=True, clear=True)
    got2 = table.cpu().numpy()
    assert np.array_equal(got2[1], before[1])
    assert np.array_equal(got2[0], PR.table_of(ids[0], 120, 120, V)) and np.array_equal(got2[2], PR.table_of(ids[2], 300, 300, V))


def test_count_full_vocabulary():
    """V = 151936: a 1024-token prompt with clear, then a 17-token commit."""
    from dflash_amd import ops
    V = 151936
    rng = np.random.default_rng(2)
    ids = rng.integers(0, V, 1100).astype(np.int64)
    ids[1030:1035] = V - 1
    table = torch.full((1, V), -1, dtype=I32, device=dev())
    d_ids = torch.from_numpy(ids).to(dev())
    ops.penalty_count(table, d_ids, lo=0, hi=1024, as_prompt=True, clear=True)
    ops.penalty_count(table, d_ids, lo=1024, hi=1041)
    assert np.array_equal(table[0].cpu().numpy(), PR.table_of(ids, 1024, 1041, V))


# ------------------------------------------------------------------------------------------------------------ the rows
def _case(V, tpr, seed):
    """Two tiles (two slots, or one slot of two tiles): rows with the special patterns in tile 0 and planted exact ties in
    tile 1; a table per slot with prompt-only, output-only and mixed entries; blocks whose tokens repeat inside the block,
    repeat table entries and hold ids outside [0, V)."""
    rng = np.random.default_rng(seed)
    slots = 2 // tpr
    x = np.stack([PR.case_rows(rng, 16, V, specials=True), PR.case_rows(rng, 16, V, specials=False)])
    table = np.stack([PR.case_table(rng, V) for _ in range(slots)])
    block = rng.integers(0, V, (slots, 16 * tpr)).astype(np.int64)
    for q in range(slots):
        hit = np.nonzero(table[q])[0]
        block[q, 2] = block[q, 1]                      # repeats inside the block
        block[q, 9] = block[q, 1]
        block[q, 4] = hit[0]                           # repeats table entries
        block[q, 11] = hit[-1]
        block[q, 12] = hit[-1]
        block[q, 6] = V + 3                            # outside the vocabulary
        block[q, 14] = -2
        if tpr == 2:
            block[q, 17], block[q, 20], block[q, 30] = block[q, 1], -1, block[q, 16]
    # exact ties at the top of tile 1: two untouched columns with one large value, and a column that only ties after
    # its penalty is applied is left to the random rows
    free = [v for v in range(V) if not table[:, v].any() and v not in block][:2]
    x[1][:, free] = 0x41F0                             # 30.0
    return x, table, block


def _expect(x, table, block, params, tpr, counts):
    """want bits, near-midpoint mask: [tiles, 16, V]; rows past a tile's count are not expected to be written."""
    want, near = np.zeros_like(x), np.zeros(x.shape, dtype=bool)
    for t in range(x.shape[0]):
        q, j = divmod(t, tpr)
        r, a, f = params[q]
        for m in range(counts[t]):
            toks = block[q][1:16 * j + m + 1] if block is not None else ()
            seen, c = PR.seen_counts(table[q], toks)
            want[t, m] = PR.penalise(x[t, m], seen, c, r, a, f)
            near[t, m] = PR.near_midpoint(x[t, m], seen, c, r, a, f)
    return want, near


def _check(got, ids, want, near, counts):
    n_el = n_near = 0
    for t in range(got.shape[0]):
        n = counts[t]
        ok = PR.neighbours_ok(got[t, :n], want[t, :n], near[t, :n])
        assert ok.all(), (t, np.argwhere(~ok)[:5], got[t, :n][~ok][:5], want[t, :n][~ok][:5])
        n_el += ok.size
        n_near += int((near[t, :n] & (got[t, :n] != want[t, :n])).sum())
        assert (got[t, n:] == SENT_BITS).all() and (ids[t, n:] == SENT_ID).all(), t       # rows past the count: untouched
        for m in range(n):
            assert ids[t, m] == PR.argmax_lowest(got[t, m]), (t, m)
    assert near.mean() <= 1e-3 and n_near <= 1e-3 * n_el


@pytest.mark.parametrize("V,tpr", [(48, 1), (2048, 1), (2048, 2)])
@pytest.mark.parametrize("form", ["device", "host", "alias"])
def test_rows_against_the_model(V, tpr, form):
    """All 16 rows of two tiles, the second with a record-driven count of 11: device-array or host-scalar parameters, the
    destination beside the source or on top of it."""
    from dflash_amd import ops
    x, table, block = _case(V, tpr, seed=V + tpr)
    slots = 2 // tpr
    params = list(PR.KERNEL_PARAMS[:slots]) if form == "device" else [PR.KERNEL_PARAMS[0]] * slots
    counts = [16, 11]
    dyn = torch.tensor([record(bs=16), record(bs=11)], dtype=I32, device=dev())
    logits = to_bf16(x)
    raw = logits.clone()
    out = logits if form == "alias" else to_bf16(np.full_like(x, SENT_BITS))
    ids = torch.full((2, 16), SENT_ID, dtype=I64, device=dev())
    d_table = torch.from_numpy(table).to(dev())
    d_block = torch.from_numpy(block).to(dev())
    if form == "device":
        kw = {k: torch.tensor([p[i] for p in params], dtype=F32, device=dev())
              for i, k in enumerate(("repetition_penalty", "presence_penalty", "frequency_penalty"))}
    else:
        kw = dict(zip(("repetition_penalty", "presence_penalty", "frequency_penalty"), params[0]))
    ops.penalty_rows(logits, d_table, block=d_block, out=out, dyn=dyn, nrows_dyn_word=ops.DYN_BS, tiles_per_req=tpr,
                     out_ids=ids, **kw)
    got = bits_of(out)
    if form == "alias":     # rows past the count keep the logits: the sentinel of this form
        assert np.array_equal(got[1, 11:], x[1, 11:])
        got[1, 11:] = SENT_BITS
    else:
        assert torch.equal(logits.view(torch.int16), raw.view(torch.int16))         # the raw rows stay
    want, near = _expect(x, table, block, params, tpr, counts)
    _check(got, ids.cpu().numpy(), want, near, counts)
    # the in-block tokens matter: the same rows without the block differ from the model (rows >= 1)
    w0, _ = _expect(x, table, None, params, tpr, counts)
    assert (w0[0, 1:] != want[0, 1:]).any() and np.array_equal(w0[0, 0], want[0, 0])
    # the planted ties win in tile 1, at the lower column
    if V > 48:
        tie = np.nonzero(x[1, 0] == 0x41F0)[0]
        assert len(tie) == 2 and (ids[1, :11].cpu().numpy() == tie[0]).all()


def test_rows_host_row_window_without_block():
    """row0 / nrows from the host and out_off: rows 3..7 of one tile, no block, ids at out_ids[5 + m - 3]; the other rows
    and ids keep their sentinel."""
    from dflash_amd import ops
    V = 2048
    x, table, _ = _case(V, 1, seed=9)
    r, a, f = PR.KERNEL_PARAMS[1]
    out = to_bf16(np.full_like(x[0], SENT_BITS))
    ids = torch.full((16,), SENT_ID, dtype=I64, device=dev())
    ops.penalty_rows(to_bf16(x[0]), torch.from_numpy(table[0]).to(dev()), repetition_penalty=r, presence_penalty=a,
                     frequency_penalty=f, out=out, row0=3, nrows=5, out_ids=ids, out_off=5)
    got, idn = bits_of(out), ids.cpu().numpy()
    seen, c = PR.seen_counts(table[0])
    for m in range(16):
        if 3 <= m < 8:
            ok = PR.neighbours_ok(got[m], PR.penalise(x[0, m], seen, c, r, a, f), PR.near_midpoint(x[0, m], seen, c, r, a, f))
            assert ok.all() and idn[5 + m - 3] == PR.argmax_lowest(got[m])
        else:
            assert (got[m] == SENT_BITS).all()
    assert (idn[:5] == SENT_ID).all() and (idn[10:] == SENT_ID).all()


def test_rows_full_vocabulary_once():
    """V = 151936, rows 0, 1 and 15 of a tile (one launch each), table and block as above."""
    from dflash_amd import ops
    V = 151936
    rng = np.random.default_rng(3)
    x = PR.case_rows(rng, 16, V)
    x[[0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14]] = 0       # (only three rows are read)
    table = PR.case_table(rng, V)
    block = rng.integers(0, V, 16).astype(np.int64)
    block[[3, 7]] = block[1]
    block[5], block[9] = V, np.nonzero(table)[0][5]
    x[0] = PR.case_rows(rng, 1, V)[0]
    r, a, f = PR.KERNEL_PARAMS[0]
    logits = to_bf16(x)
    out = to_bf16(np.full_like(x, SENT_BITS))
    ids = torch.full((16,), SENT_ID, dtype=I64, device=dev())
    d_table, d_block = torch.from_numpy(table).to(dev()), torch.from_numpy(block).to(dev())
    for m in (0, 1, 15):
        ops.penalty_rows(logits, d_table, repetition_penalty=r, presence_penalty=a, frequency_penalty=f, block=d_block,
                         out=out, row0=m, nrows=1, out_ids=ids, out_off=m)
    got, idn = bits_of(out), ids.cpu().numpy()
    n_near = 0
    for m in (0, 1, 15):
        seen, c = PR.seen_counts(table, block[1:m + 1])
        want, near = PR.penalise(x[m], seen, c, r, a, f), PR.near_midpoint(x[m], seen, c, r, a, f)
        ok = PR.neighbours_ok(got[m], want, near)
        assert ok.all(), (m, np.nonzero(~ok)[0][:5])
        assert near.mean() <= 1e-3
        n_near += int((got[m] != want).sum())
        assert idn[m] == PR.argmax_lowest(got[m])
    assert n_near <= 3e-3 * V
    assert (got[2] == SENT_BITS).all() and idn[2] == SENT_ID


@pytest.mark.parametrize("V", [48, 2048])
def test_neutral_parameters_copy_the_rows(V):
    """r = 1, a = 0, f = 0: every row bit for bit, NaNs, infinities and both zeros included, whatever the table and the
    block hold; the ids are those of dfl_argmax (rows without a NaN: its rule for them is not this kernel's)."""
    from dflash_amd import ops
    x, table, block = _case(V, 1, seed=77 + V)
    logits = to_bf16(x)
    ids = torch.full((2, 16), SENT_ID, dtype=I64, device=dev())
    out = ops.penalty_rows(logits, torch.from_numpy(table).to(dev()), block=torch.from_numpy(block).to(dev()), out_ids=ids)
    assert np.array_equal(bits_of(out), x)
    assert torch.equal(ids[1], ops.argmax(logits[1]))
    for m in range(16):
        assert int(ids[0, m]) == PR.argmax_lowest(x[0, m])
    # device values that are not valid read as neutral: r <= 0, r = NaN, r = inf -> 1; a, f not finite -> 0
    bad = dict(repetition_penalty=torch.tensor([-1.0, float("nan")], dtype=F32, device=dev()),
               presence_penalty=torch.tensor([float("inf"), float("nan")], dtype=F32, device=dev()),
               frequency_penalty=torch.tensor([float("nan"), float("-inf")], dtype=F32, device=dev()))
    out2 = ops.penalty_rows(logits, torch.from_numpy(table).to(dev()), block=torch.from_numpy(block).to(dev()), **bad)
    assert np.array_equal(bits_of(out2), x)
    bad["repetition_penalty"] = torch.tensor([0.0, float("inf")], dtype=F32, device=dev())
    assert np.array_equal(bits_of(ops.penalty_rows(logits, torch.from_numpy(table).to(dev()), **bad)), x)


def test_same_bits_on_every_run():
    from dflash_amd import ops
    V = 2048
    x, table, block = _case(V, 2, seed=5)
    r, a, f = PR.KERNEL_PARAMS[0]
    args = (to_bf16(x), torch.from_numpy(table).to(dev()))
    kw = dict(repetition_penalty=r, presence_penalty=a, frequency_penalty=f, block=torch.from_numpy(block).to(dev()),
              tiles_per_req=2)
    first = bits_of(ops.penalty_rows(*args, **kw))
    for _ in range(3):
        assert np.array_equal(bits_of(ops.penalty_rows(*args, **kw)), first)
