"""dfl_logit_bias_rows alone against the numpy model of logit_bias_ref.py, bit for bit: the select
and its one rounding, min_pos against the row's position in both position forms, the argmax ids, the layout."""
import numpy as np
import pytest
import torch

import logit_bias_ref as LR

pytestmark = pytest.mark.gpu
BF16, I32, I64, F32 = torch.bfloat16, torch.int32, torch.int64, torch.float32
SENT_BITS, SENT_ID = 0x1234, -7


def dev():
    return torch.device("cuda", 0)


def to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev()).view(BF16)


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def record(pos0=0, bs=16):
    return [0, 0, bs, pos0, 0, 0, 0, 0]


def d(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dt is None else t.to(dt)


def _plant(x, b, rng):
    """Every special bit pattern under b = 0, b = -0.0, b = -inf, a finite b, a NaN b and a +inf b (V permitting)."""
    V = x.shape[-1]
    n = len(LR.SPECIALS)
    if V < 6 * n:
        return
    cols = rng.choice(V, 6 * n, replace=False).reshape(6, n)
    for k, bv in enumerate((0.0, -0.0, -np.inf, 1.5, np.nan, np.inf)):
        x[..., cols[k]] = np.array(LR.SPECIALS, dtype=np.uint16)
        b[..., cols[k]] = np.float32(bv)


# ------------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("V", [8, 8 * 1031, 2048])
@pytest.mark.parametrize("form", ["device", "host", "alias"])
def test_rows_against_the_model(V, form):
    """Four tiles, four table rows, the last tile with a record-driven count of 11; each tile's rows straddle its slot's
    min_pos (p = min_pos - 1 and p = min_pos in one block); the position from the record's POS0 word plus pos_add
    ("device": min_pos from the device array) or from the host ("host" / "alias": one host min_pos); stop ids inside and
    outside [0, V), one that carries a bias, two in one 8-column chunk; ld > V."""
    from dflash_amd import ops
    rng = np.random.default_rng(V)
    T, ld = 4, V + 24
    x = np.stack([LR.case_rows(rng, 16, V) for _ in range(T)])
    b = np.stack([LR.case_table(rng, V) for _ in range(T)])
    _plant(x[0], b[0], rng)
    stops = np.array([V - 1, V - 2, 3, -1, V, 2 ** 40, 5 % V], dtype=np.int64)      # V-1 and V-2: one chunk
    b[:, 3] = np.float32(2.25)                                                      # a stop id that also has a bias
    b[:, V - 2] = 0.0
    x[:, :, V - 2] = 0x42A0                                                         # 80.0: the raw argmax is a stop id
    counts = [16, 16, 16, 11]
    pos0 = [100, 7, 0, 1000]
    dyn = d(np.array([record(p, c) for p, c in zip(pos0, counts)], dtype=np.int32))
    pos_add = 1
    if form == "device":
        min_pos = [100 + 1 + 6, 0, 40, 1000 + 1 + 10]      # tile 0: rows 0..5 suppressed; tile 1: off; 2: all; 3: rows 0..9
        kw = dict(min_pos=d(np.array(min_pos, dtype=np.int32)), dyn=dyn, nrows_dyn_word=ops.DYN_BS, pos_word=ops.DYN_POS0,
                  pos_add=pos_add)
        pos = lambda t, m: LR.position(t, m, 1, dyn.cpu().numpy(), ops.DYN_POS0, 0, pos_add)
    else:
        min_pos = [57] * T                                  # host form: one value, pos_base = 50 -> rows 0..5 suppressed
        kw = dict(min_pos=57, dyn=dyn, nrows_dyn_word=ops.DYN_BS, pos_base=50, pos_add=pos_add)
        pos = lambda t, m: LR.position(t, m, 1, None, -1, 50, pos_add)
    buf = to_bf16(np.full((T, 16, ld), SENT_BITS, dtype=np.uint16))
    logits = buf[:, :, :V]
    logits.copy_(to_bf16(x))
    raw = buf.clone()
    obuf = buf if form == "alias" else to_bf16(np.full((T, 16, ld), SENT_BITS, dtype=np.uint16))
    out = obuf[:, :, :V]
    ids = torch.full((T, 16), SENT_ID, dtype=I64, device=dev())
    ops.logit_bias_rows(logits, d(b), stop_ids=d(stops), out=out, out_ids=ids, **kw)
    got, idn = bits_of(out), ids.cpu().numpy()
    assert (bits_of(obuf[:, :, V:]) == SENT_BITS).all()                             # the columns past V are not written
    if form != "alias":
        assert torch.equal(buf.view(torch.int16), raw.view(torch.int16))            # the raw rows stay
    seen_on = seen_off = 0
    for t in range(T):
        n = counts[t]
        for m in range(n):
            p = pos(t, m)
            want = LR.process(x[t, m], b[t], p, min_pos[t], stops)
            assert np.array_equal(got[t, m], want), (t, m, np.nonzero(got[t, m] != want)[0][:5])
            assert idn[t, m] == LR.argmax_lowest(want), (t, m)
            seen_on += p < min_pos[t]
            seen_off += p >= min_pos[t]
            if p < min_pos[t]:
                assert got[t, m, V - 1] == 0xFF80 and got[t, m, V - 2] == 0xFF80 and got[t, m, 3] == 0xFF80
                assert idn[t, m] != V - 2
            elif t > 0:                                                             # (tile 0 holds planted +inf logits)
                assert idn[t, m] == V - 2                                           # 80.0 wins once the stop ids are free
        tail = got[t, n:]
        assert (tail == (x[t, n:] if form == "alias" else SENT_BITS)).all() and (idn[t, n:] == SENT_ID).all(), t
    assert seen_on >= 6 and seen_off >= 6
    # the straddle: p = min_pos - 1 and p = min_pos are rows 5 and 6 of tile 0
    assert pos(0, 5) == min_pos[0] - 1 and pos(0, 6) == min_pos[0]


def test_select_and_rounding():
    """One row built column by column: sums that land on bf16 ties (both ways to even), b = 0 / -0.0 on -0.0, NaN payloads
    and +-inf (bit copies), b = -inf on +inf and NaN (-inf), device table values NaN and +inf (read as 0), overflow."""
    from dflash_amd import ops
    cases = [   # (x bits, b, want bits)
        (0x3F80, 2.0 ** -8, 0x3F80),        # 1 + 2^-8: tie between 1.0 and 1.0078125 -> even (down)
        (0x3F81, 2.0 ** -8, 0x3F82),        # 1.0078125 + 2^-8: tie -> even (up)
        (0x3F80, 3 * 2.0 ** -9, 0x3F81),    # above the tie
        (0xBF80, -(2.0 ** -8), 0xBF80),     # the negative tie
        (0x4000, 2.0 ** -7, 0x4000),        # 2 + 2^-7: tie at the next binade -> even
        (0x8000, 0.0, 0x8000), (0x8000, -0.0, 0x8000),
        (0x7FC1, 0.0, 0x7FC1), (0xFFFF, 0.0, 0xFFFF), (0x7F81, 0.0, 0x7F81),
        (0x7F80, 0.0, 0x7F80), (0xFF80, 0.0, 0xFF80),
        (0x7F80, -np.inf, 0xFF80), (0x7FC1, -np.inf, 0xFF80), (0xFFFF, -np.inf, 0xFF80), (0x3F80, -np.inf, 0xFF80),
        (0x3F81, np.nan, 0x3F81), (0x3F81, np.inf, 0x3F81), (0x8000, np.nan, 0x8000), (0x7FC1, np.inf, 0x7FC1),
        (0x7F80, -5.0, 0x7F80), (0xFF80, 5.0, 0xFF80), (0x7FC1, 1.0, 0x7FC1),
        (0x7F7F, 3.0e38, 0x7F80),           # overflow rounds to +inf
        (0x8000, 1.0, 0x3F80), (0x3F80, -1.0, 0x0000), (0x0001, -1.0, 0xBF80),
    ]
    V = 8 * ((len(cases) + 7) // 8)
    x = np.full(V, 0xC2C8, dtype=np.uint16)      # -100: the padding
    b = np.zeros(V, dtype=np.float32)
    want = x.copy()
    for i, (xb, bv, wb) in enumerate(cases):
        x[i], b[i], want[i] = xb, np.float32(bv), wb
    assert np.array_equal(LR.process(x, b), want)                                   # the model agrees with the table above
    got = bits_of(ops.logit_bias_rows(to_bf16(x).view(1, V), d(b)))[0]
    assert np.array_equal(got, want), np.nonzero(got != want)[0]


def test_argmax_ban_tie_and_fully_banned_row():
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(4)
    x = LR.case_rows(rng, 4, V)
    b = np.zeros(V, dtype=np.float32)
    top = [LR.argmax_lowest(x[m]) for m in range(4)]
    b[top[0]] = -np.inf                                  # row 0: the ban removes the raw argmax
    x[1, [1500, 300, 900]] = 0x4270                      # row 1: a three-way tie at 60.0 -> column 300
    x[2, 77], x[2, 78] = 0x41F0, 0x41E0                  # row 2: 30 at 77, 28 + 2.0 at 78: a tie made by the bias -> 77
    b[78] = 2.0
    ids = torch.full((4,), SENT_ID, dtype=I64, device=dev())
    out = bits_of(ops.logit_bias_rows(to_bf16(x), d(b), out_ids=ids))
    idn = ids.cpu().numpy()
    for m in range(4):
        assert np.array_equal(out[m], LR.process(x[m], b)) and idn[m] == LR.argmax_lowest(out[m])
    assert idn[0] != top[0] and idn[1] == 300 and idn[2] == 77
    # a fully banned row is all -inf: column 0; a row of NaNs: 0 too
    ids.fill_(SENT_ID)
    xn = x.copy()
    xn[1] = 0x7FC0
    allb = np.full(V, -np.inf, dtype=np.float32)
    out = bits_of(ops.logit_bias_rows(to_bf16(xn[:1]), d(allb), out_ids=ids[:1]))
    assert (out == 0xFF80).all() and int(ids[0]) == 0
    ops.logit_bias_rows(to_bf16(xn[1:2]), d(np.zeros_like(b)), out_ids=ids[1:2])
    assert int(ids[1]) == 0
    # min_tokens with every other token banned by the stop ids' suppression alone: the stop column itself
    only = np.full(V, -np.inf, dtype=np.float32)
    only[9] = 0.0
    out = bits_of(ops.logit_bias_rows(to_bf16(x[:1]), d(only), min_pos=5, stop_ids=d(np.array([9], dtype=np.int64)),
                                      pos_base=4, out_ids=ids[:1]))
    assert (out == 0xFF80).all() and int(ids[0]) == 0


@pytest.mark.parametrize("form", ["record", "host"])
def test_two_tiles_per_request(form):
    """tiles_per_req = 2: tiles 2q and 2q + 1 take table row q and min_pos[q], and tile j adds 16 j to the position: with
    min_pos inside the second tile, rows of both tiles are suppressed and the rest of the second is free."""
    from dflash_amd import ops
    V, T = 2048, 4
    rng = np.random.default_rng(11)
    x = np.stack([LR.case_rows(rng, 16, V) for _ in range(T)])
    b = np.stack([LR.case_table(rng, V) for _ in range(4)])       # rows 2 and 3 belong to no slot of this launch
    stops = np.array([17, 1040], dtype=np.int64)
    b[:, 17], b[:, 1040] = 0.0, 0.5
    pos0 = [200, 200, 30, 30]                            # a record per tile, both tiles of a request carry its POS0
    dyn_np = np.array([record(p, c) for p, c in zip(pos0, (16, 16, 16, 5))], dtype=np.int32)
    min_pos = [200 + 1 + 16 + 4, 30 + 1 + 3]             # slot 0: tile 0 whole + rows 0..3 of tile 1; slot 1: rows 0..2 of tile 2
    if form == "record":
        kw = dict(dyn=d(dyn_np), nrows_dyn_word=ops.DYN_BS, pos_word=ops.DYN_POS0, pos_add=1)
        pos = lambda t, m: LR.position(t, m, 2, dyn_np, ops.DYN_POS0, 0, 1)
    else:
        dyn_np[:, ops.DYN_POS0] = 200
        min_pos[1] = 200 + 1 + 3
        kw = dict(dyn=d(dyn_np), nrows_dyn_word=ops.DYN_BS, pos_base=200, pos_add=1)
        pos = lambda t, m: LR.position(t, m, 2, None, -1, 200, 1)
    ids = torch.full((T, 16), SENT_ID, dtype=I64, device=dev())
    out = to_bf16(np.full_like(x, SENT_BITS))
    ops.logit_bias_rows(to_bf16(x), d(b), min_pos=d(np.array(min_pos, dtype=np.int32)), stop_ids=d(stops), out=out,
                        tiles_per_req=2, out_ids=ids, **kw)
    got, idn = bits_of(out), ids.cpu().numpy()
    for t, n in enumerate((16, 16, 16, 5)):
        q = t // 2
        for m in range(n):
            want = LR.process(x[t, m], b[q], pos(t, m), min_pos[q], stops)
            assert np.array_equal(got[t, m], want) and idn[t, m] == LR.argmax_lowest(want), (t, m)
        assert (got[t, n:] == SENT_BITS).all() and (idn[t, n:] == SENT_ID).all()
    assert got[1, 3, 17] == 0xFF80 and got[1, 4, 17] == x[1, 4, 17]          # the 16 j: row 3 of tile 1 is p = min_pos - 1
    assert got[0, 15, 17] == 0xFF80 and got[3, 0, 17] == x[3, 0, 17]
    assert not np.array_equal(b[0], b[1])


def test_host_row_window():
    """row0 / nrows from the host and out_off: rows 3..7 of one tile, ids at out_ids[5 + m - 3]; the other rows and ids keep
    their sentinel; the position counts the row's index in the tile, not in the window."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(9)
    x, b = LR.case_rows(rng, 16, V), LR.case_table(rng, V)
    b[40] = 0.0
    stops = np.array([40], dtype=np.int64)
    out = to_bf16(np.full_like(x, SENT_BITS))
    ids = torch.full((16,), SENT_ID, dtype=I64, device=dev())
    ops.logit_bias_rows(to_bf16(x), d(b), min_pos=15, stop_ids=d(stops), pos_base=10, out=out, row0=3, nrows=5,
                        out_ids=ids, out_off=5)
    got, idn = bits_of(out), ids.cpu().numpy()
    for m in range(16):
        if 3 <= m < 8:
            want = LR.process(x[m], b, 10 + m, 15, stops)
            assert np.array_equal(got[m], want) and idn[5 + m - 3] == LR.argmax_lowest(want)
        else:
            assert (got[m] == SENT_BITS).all()
    assert got[4, 40] == 0xFF80 and got[5, 40] == x[5, 40]
    assert (idn[:5] == SENT_ID).all() and (idn[10:] == SENT_ID).all()


def test_full_vocabulary_once():
    """16 x 151936 in one launch: a table with every kind of entry, rows 0..7 before min_pos."""
    from dflash_amd import ops
    V = 151936
    rng = np.random.default_rng(3)
    x, b = LR.case_rows(rng, 16, V), LR.case_table(rng, V)
    _plant(x, b, rng)
    stops = np.array([V - 1, 151643, 151645, V + 7], dtype=np.int64)
    b[151645] = 1.0
    ids = torch.full((16,), SENT_ID, dtype=I64, device=dev())
    out = bits_of(ops.logit_bias_rows(to_bf16(x), d(b), min_pos=108, stop_ids=d(stops), pos_base=100, out_ids=ids))
    idn = ids.cpu().numpy()
    for m in range(16):
        want = LR.process(x[m], b, 100 + m, 108, stops)
        assert np.array_equal(out[m], want), (m, np.nonzero(out[m] != want)[0][:5])
        assert idn[m] == LR.argmax_lowest(want)
    assert out[7, V - 1] == 0xFF80 and out[8, V - 1] != 0xFF80


def test_same_bits_on_every_run_and_refusals():
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(5)
    x, b = np.stack([LR.case_rows(rng, 16, V)] * 2), np.stack([LR.case_table(rng, V)] * 2)
    args, kw = (to_bf16(x), d(b)), dict(min_pos=3, stop_ids=d(np.array([1, 2], dtype=np.int64)))
    first = bits_of(ops.logit_bias_rows(*args, **kw))
    for _ in range(3):
        assert np.array_equal(bits_of(ops.logit_bias_rows(*args, **kw)), first)
    with pytest.raises(RuntimeError):     # more stop ids than one launch takes
        ops.logit_bias_rows(*args, min_pos=3, stop_ids=torch.zeros(65, dtype=I64, device=dev()))
    with pytest.raises(RuntimeError):     # V is not a multiple of 8
        ops.logit_bias_rows(to_bf16(x[0][:, :2044]).contiguous(), d(b[0][:2044]))
