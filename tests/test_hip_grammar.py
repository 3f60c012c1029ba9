"""dfl_grammar_rows and dfl_grammar_advance alone against the numpy model of grammar_ref.py, bit for
bit: the walk through the block's own tokens, live and dead rows, the mask, the argmax ids, the pool's bases, the 64-bit
row offset, the layout; the advance's ranges, idle slots and the sticky -1."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_ref as GR

pytestmark = pytest.mark.gpu
BF16, I16, I32, I64 = torch.bfloat16, torch.int16, torch.int32, torch.int64
SENT_BITS, SENT_ID = 0x1234, -7
BAD, GOOD = 5, 2      # in every test grammar: token 5 is illegal everywhere, token 2 legal everywhere


def dev():
    return torch.device("cuda", 0)


def to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev()).view(BF16)


def bits_of(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def d(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    return t if dt is None else t.to(dt)


def record(s=0, bs=16, start=0):
    return [s, 0, bs, 0, start, 0, 0, 0]


def dfa(rng, S, V):
    nxt = GR.case_dfa(rng, S, V)
    nxt[:, BAD] = -1
    nxt[:, GOOD] = (np.arange(S) + 1) % S
    return nxt


def pool_of(tables, V, spare=2):
    """The tables stacked into one pool with `spare` all-illegal rows in front of each: (pool, bases)."""
    bases, rows, at = [], [], 0
    for t in tables:
        rows.append(np.full((spare, V), -1, np.int16))
        at += spare
        bases.append(at)
        rows.append(t)
        at += len(t)
    return np.concatenate(rows), bases


def state_of(pool, base, state):
    return SimpleNamespace(table=d(pool), base=d(np.asarray(base, np.int32)), state=d(np.asarray(state, np.int32)))


def legal_block(rng, pool, base, s, n, V):
    """n ids: block[0] arbitrary, block[1:] a legal walk from s (a random legal token per step)."""
    blk = [int(rng.integers(0, V))]
    for _ in range(n - 1):
        legal = np.nonzero(pool[base + s] >= 0)[0]
        v = int(rng.choice(legal))
        blk.append(v)
        s = int(pool[base + s, v])
    return blk


def run_rows(x, st, block, *, alias=False, ld_pad=24, **kw):
    """x bits [T, 16, V] through ops.grammar_rows in a padded buffer; returns (out bits, ids, the buffers)."""
    from dflash_amd import ops
    T, _, V = x.shape
    ld = V + ld_pad
    buf = to_bf16(np.full((T, 16, ld), SENT_BITS, dtype=np.uint16))
    logits = buf[:, :, :V]
    logits.copy_(to_bf16(x))
    raw = buf.clone()
    obuf = buf if alias else to_bf16(np.full((T, 16, ld), SENT_BITS, dtype=np.uint16))
    out = obuf[:, :, :V]
    ids = torch.full((T, 16), SENT_ID, dtype=I64, device=dev())
    ops.grammar_rows(logits, st, block=block, out=out, out_ids=ids, **kw)
    torch.cuda.synchronize()
    assert (bits_of(obuf[:, :, V:]) == SENT_BITS).all()                             # the columns past V are not written
    if not alias:
        assert torch.equal(buf.view(I16), raw.view(I16))                            # the raw rows stay
    return bits_of(out), ids.cpu().numpy()


# ------------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("V", [8, 8 * 1024 + 8])
def test_rows_against_the_model(V, alias):
    """Four tiles, three grammars in one pool at non-zero bases — S = 1, S = 3 and S = 300 (states past 255) —, rows 0..15
    each.  The illegal draft token sits at block index 1 (tile 0), 8 (tile 1), 15 (tile 2: an id outside the vocabulary)
    and nowhere (tile 3): rows before it are masked by the state their prefix reaches, rows from it on are copied with
    the raw argmax."""
    rng = np.random.default_rng(V)
    pool, bases = pool_of([dfa(rng, 1, V), dfa(rng, 3, V), dfa(rng, 300, V)], V)
    base = [bases[0], bases[1], bases[2], bases[1]]
    start = [0, 2, 257, 1]
    bad_at = [1, 8, 15, None]
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(4)])
    blocks = np.array([legal_block(rng, pool, base[t], start[t], 16, V) for t in range(4)], dtype=np.int64)
    blocks[0, 1], blocks[1, 8], blocks[2, 15] = BAD, BAD, V + 3
    got, ids = run_rows(x, state_of(pool, base, start), d(blocks), alias=alias)
    for t in range(4):
        z, am, st = GR.rows(x[t], pool, base[t], start[t], blocks[t])
        k = bad_at[t]
        assert ((st >= 0) == (np.arange(16) < (16 if k is None else k))).all(), (t, st)
        assert np.array_equal(got[t], z), (t, np.nonzero((got[t] != z).any(axis=1))[0])
        assert np.array_equal(ids[t], am), t
        for m in range(16):
            if st[m] < 0:
                assert np.array_equal(got[t, m], x[t, m]) and ids[t, m] == GR.argmax_lowest(x[t, m])
            else:
                assert got[t, m, BAD] == 0xFF80 and got[t, m, GOOD] == x[t, m, GOOD]
    assert (GR.rows(x[2], pool, base[2], start[2], blocks[2])[2][:15] > 255).any()   # the walk passes states past 255


def test_rows_full_vocabulary_single_tile():
    """V = 151936 on a single tile: S = 300 at a non-zero base, the illegal token at block index 8."""
    V = 151936
    rng = np.random.default_rng(7)
    pool, bases = pool_of([dfa(rng, 2, V), dfa(rng, 300, V)], V)
    x = GR.case_rows(rng, 16, V)[None]
    blk = np.array([legal_block(rng, pool, bases[1], 299, 16, V)], dtype=np.int64)
    blk[0, 8] = BAD
    got, ids = run_rows(x, state_of(pool, [bases[1]], [299]), d(blk))
    z, am, st = GR.rows(x[0], pool, bases[1], 299, blk[0])
    assert (st[:8] >= 0).all() and (st[8:] < 0).all()
    assert np.array_equal(got[0], z) and np.array_equal(ids[0], am)


def test_only_the_last_column_legal():
    """A state whose only legal column is V - 1, under raw rows whose maximum lies elsewhere: everything else is -inf and
    the argmax is V - 1; an all-illegal state gives an all -inf row and column 0."""
    V = 8 * 1024 + 8
    rng = np.random.default_rng(3)
    t = np.full((3, V), -1, np.int16)
    t[0, V - 1] = 1
    t[1, GOOD] = 2          # state 2: nothing legal
    pool, bases = pool_of([t], V)
    x = GR.case_rows(rng, 16, V)[None]
    x[0, :, 17] = 0x42A0    # 80.0
    x[0, 0, V - 1] = x[0, 1, GOOD] = 0x3F80   # (numbers, whatever case_rows planted there)
    blk = np.array([[0, V - 1, GOOD] + [0] * 13], dtype=np.int64)
    got, ids = run_rows(x, state_of(pool, bases, [0]), d(blk), nrows=3)
    assert (got[0, 0, :V - 1] == 0xFF80).all() and got[0, 0, V - 1] == x[0, 0, V - 1] and ids[0, 0] == V - 1
    assert ids[0, 1] == GOOD
    assert (got[0, 2] == 0xFF80).all() and ids[0, 2] == 0
    assert (got[0, 3:] == SENT_BITS).all() and (ids[0, 3:] == SENT_ID).all()


def test_slots_without_grammar_and_violated_among_live_ones():
    """base = -1 (no grammar) and state = -1 (violated): all their rows are copied with the raw argmax, their neighbours
    are masked; the rows of a tile come from the record (11 and 16), the rest is not written."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(5)
    pool, bases = pool_of([dfa(rng, 3, V)], V)
    base, start = [bases[0], -1, bases[0], bases[0]], [1, 0, -1, 2]
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(4)])
    blocks = np.array([legal_block(rng, pool, bases[0], max(s, 0), 16, V) for s in start], dtype=np.int64)
    counts = [16, 16, 16, 11]
    dyn = d(np.array([record(bs=c) for c in counts], dtype=np.int32))
    got, ids = run_rows(x, state_of(pool, base, start), d(blocks), dyn=dyn, nrows_dyn_word=ops.DYN_BS)
    for t in range(4):
        n = counts[t]
        z, am, st = GR.rows(x[t, :n], pool, base[t], start[t], blocks[t])
        assert (st >= 0).all() == (t in (0, 3)) and ((st < 0).all() or (st >= 0).all())
        assert np.array_equal(got[t, :n], z) and np.array_equal(ids[t, :n], am), t
        if t in (1, 2):
            assert np.array_equal(got[t], x[t])
        assert (got[t, n:] == SENT_BITS).all() and (ids[t, n:] == SENT_ID).all()


def test_single_row_form_and_row0():
    """block = None: no walk, the row is masked by state[q] itself (the first token's form); row0 / nrows pick rows 15 and
    0 alone, each walking its own prefix."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(9)
    pool, bases = pool_of([dfa(rng, 3, V)], V)
    st = state_of(pool, bases, [2])
    x = GR.case_rows(rng, 16, V)
    ids = torch.full((1,), SENT_ID, dtype=I64, device=dev())
    z = ops.grammar_rows(to_bf16(x[:1]), st, out_ids=ids)
    want = GR.mask_row(x[0], pool, bases[0], 2)
    assert np.array_equal(bits_of(z)[0], want) and int(ids[0]) == GR.argmax_lowest(want)
    blk = np.array(legal_block(rng, pool, bases[0], 2, 16, V), dtype=np.int64)
    zw, aw, _ = GR.rows(x, pool, bases[0], 2, blk)
    for m in (0, 15):
        out = to_bf16(np.full((16, V), SENT_BITS, np.uint16))
        ops.grammar_rows(to_bf16(x), st, block=d(blk), out=out, row0=m, nrows=1, out_ids=ids)
        got = bits_of(out)
        assert np.array_equal(got[m], zw[m]) and int(ids[0]) == aw[m]
        assert (np.delete(got, m, axis=0) == SENT_BITS).all()


def test_two_tiles_per_request_are_refused():
    from dflash_amd import ops
    V = 64
    rng = np.random.default_rng(1)
    pool, bases = pool_of([dfa(rng, 2, V)], V)
    x = to_bf16(GR.case_rows(rng, 32, V).reshape(2, 16, V))
    with pytest.raises(NotImplementedError):
        ops.grammar_rows(x, state_of(pool, bases, [0]), block=d(np.zeros(32, np.int64)), tiles_per_req=2)


def test_row_offset_past_2_31_elements():
    """(base + state) * table_stride beyond 2^31 elements: a pool of about 4.3 GB, allocated uninitialised, of which only
    the rows that are read are written.  Rows and advance must address those rows."""
    from dflash_amd import ops
    V, P, base = 151936, 14200, 14000
    assert (base + 136) * V > 2 ** 31
    rng = np.random.default_rng(11)
    t = dfa(rng, 4, V)                                   # relative states 136..139 hold it
    t = np.where(t >= 0, t + 136, -1).astype(np.int16)
    table = torch.empty(P, V, dtype=I16, device=dev())
    table[base + 136:base + 140].copy_(d(t))
    model_pool = np.full((140, V), -1, np.int16)          # the model sees the same rows at base 0
    model_pool[136:140] = t
    st = SimpleNamespace(table=table, base=d(np.array([base], np.int32)), state=d(np.array([137], np.int32)))
    x = GR.case_rows(rng, 4, V)
    blk = np.array(legal_block(rng, model_pool, 0, 137, 4, V), dtype=np.int64)
    ids = torch.full((4,), SENT_ID, dtype=I64, device=dev())
    z = ops.grammar_rows(to_bf16(x), st, block=d(blk), out_ids=ids)
    zw, aw, sw = GR.rows(x, model_pool, 0, 137, blk)
    assert (sw >= 136).all()
    assert np.array_equal(bits_of(z), zw) and np.array_equal(ids.cpu().numpy(), aw)
    ops.grammar_advance(st, d(blk), lo=1, hi=4)
    assert int(st.state[0]) == GR.walk(model_pool, 0, 137, blk[1:4])


# ------------------------------------------------------------------------------------------------------------ the advance
def test_advance():
    """Six slots over ids [6, 40]: ranges (S, START] from the record; an idle slot (BS = 0), a slot without grammar and a
    violated one are left alone; an illegal committed id and an id outside the vocabulary give -1, which a second launch
    over legal ids leaves in place; the host form takes lo / hi themselves and clamps them to the ids."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(13)
    pool, bases = pool_of([dfa(rng, 3, V), dfa(rng, 300, V)], V)
    base = [bases[0], bases[1], bases[1], -1, bases[0], bases[1]]
    start = [1, 290, 5, 0, -1, 7]
    ids = np.array([legal_block(rng, pool, max(b, bases[0]), max(s, 0), 40, V) for b, s in zip(base, start)], dtype=np.int64)
    S, START = [0, 0, 3, 0, 0, 2], [9, 1, 3, 5, 5, 12]              # slot 2: an empty range
    bs = [16, 16, 16, 16, 16, 0]                                    # slot 5: idle
    # the walk of slot s starts at ids[s, S + 1]: make that the legal continuation of its state
    for s in range(6):
        if base[s] >= 0 and start[s] >= 0:
            ids[s, S[s] + 1:] = legal_block(rng, pool, base[s], start[s], 40 - S[s], V)[1:]
    ids[1, 1] = BAD                                                 # slot 1 commits one illegal id
    st = state_of(pool, base, start)
    dyn = d(np.array([record(S[s], bs[s], START[s]) for s in range(6)], dtype=np.int32))
    ops.grammar_advance(st, d(ids), dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START, lo=1, hi=1)
    got = st.state.cpu().numpy()
    want = [GR.advance(pool, base[s], start[s], ids[s, S[s] + 1:START[s] + 1]) if bs[s] else start[s] for s in range(6)]
    assert got.tolist() == want, (got, want)
    assert want[1] == -1 and want[2] == 5 and want[3] == 0 and want[4] == -1 and want[5] == 7 and want[0] >= 0
    assert torch.equal(st.base.cpu(), torch.tensor(base, dtype=I32))
    # -1 stays: the same launch again, slot 1's ids now all legal
    ids[1, 1] = GOOD
    ops.grammar_advance(st, d(ids), dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START, lo=1, hi=1)
    assert int(st.state[1]) == -1
    # the host form, an id outside the vocabulary, the clamp to the ids' length
    st = state_of(pool, [bases[0]] * 3, [0, 0, 0])
    row = np.array([GOOD] * 8, dtype=np.int64)
    three = np.stack([row, row, row])
    three[1, 4], three[2, 7] = V, -1
    ops.grammar_advance(st, d(three), lo=2, hi=100)
    assert st.state.cpu().tolist() == [GR.walk(pool, bases[0], 0, row[2:]), -1, -1]
    st = state_of(pool, [bases[0]] * 3, [0, 0, 0])
    ops.grammar_advance(st, d(three), lo=0, hi=4)                   # the bad ids lie outside [0, 4)
    assert st.state.cpu().tolist() == [GR.walk(pool, bases[0], 0, row[:4])] * 3
