"""dfl_grammar_draft_rows alone ("The draft under the grammar") against the numpy model of
grammar_draft_ref.py, ids array_equal: the row-by-row walk, ties, -inf and NaN, the stop rules, the pool's bases, slots
without grammar, the ban-only and the combined form, the block size from a record, the 64-bit row offset, the layout, and
an eager launch against a graph replay."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_draft_ref as GD
import grammar_ref as GR

pytestmark = pytest.mark.gpu
BF16, I16, I32, I64, F32 = torch.bfloat16, torch.int16, torch.int32, torch.int64, torch.float32
SENT_BITS, SENT_ID = 0x1234, -7


def dev():
    return torch.device("cuda", 0)


def to_bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev()).view(BF16)


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def record(bs=16):
    return [0, 0, bs, 0, 0, 0, 0, 0]


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


def sentinel_blocks(T):
    """Every slot's block on entry: distinct negative ids, so that a row that is not written shows."""
    return SENT_ID - np.arange(T * 16, dtype=np.int64).reshape(T, 16)


def run_pick(x, st, bias, blocks, *, ld_pad=24, blk_pad=3, **kw):
    """x bits [T, 16, V] in a padded buffer, blocks int64 [T, 16] in a padded one, through ops.grammar_draft_rows; returns
    the blocks after it.  The logits, the state and the bias table must come back unchanged."""
    from dflash_amd import ops
    T, _, V = x.shape
    buf = to_bf16(np.full((T, 16, V + ld_pad), SENT_BITS, dtype=np.uint16))
    logits = buf[:, :, :V]
    logits.copy_(to_bf16(x))
    raw = buf.clone()
    bbuf = torch.full((T, 16 + blk_pad), SENT_ID, dtype=I64, device=dev())
    blk = bbuf[:, :16]
    blk.copy_(d(blocks))
    s0 = None if st is None else (st.base.clone(), st.state.clone())
    b = None if bias is None else d(np.asarray(bias, np.float32))
    ops.grammar_draft_rows(logits, st, bias=b, block=blk, **kw)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(I16), raw.view(I16))                          # the logits are only read
    assert (bbuf[:, 16:] == SENT_ID).all()                                    # nothing past a slot's 16 ids
    if st is not None:
        assert torch.equal(st.base, s0[0]) and torch.equal(st.state, s0[1])   # the state is only read
    return blk.cpu().numpy()


def want_of(x, blocks, pool, base, state, bias, ns):
    out = []
    for t in range(len(x)):
        out.append(GD.pick(x[t], ns[t], blocks[t], pool, -1 if base is None else base[t], -1 if state is None else state[t],
                           None if bias is None else bias[t])[0])
    return np.stack(out)


# ------------------------------------------------------------------------------------------------------ against the model
@pytest.mark.parametrize("form", ["grammar", "bias", "both"])
@pytest.mark.parametrize("V", [8, 8200])
def test_pick_against_the_model(V, form):
    """Four tiles over two grammars at different pool bases; tile 1 has no grammar (base = -1) and tile 2 is violated
    (state = -1): grammar-only leaves both untouched, with a bias table tile 1 is picked by its bans alone.  V = 8: one
    chunk, most threads idle; V = 8200: one thread takes a second trip, the row's tail.  Row 0 is never written."""
    rng = np.random.default_rng(V)
    pool, bases = pool_of([GR.case_dfa(rng, 3, V, 0.5), GR.case_dfa(rng, 300, V, 0.5)], V)
    base, state = [bases[0], -1, bases[1], bases[1]], [1, 0, -1, 299]
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(4)])
    bias = None
    if form != "grammar":
        bias = np.where(rng.random((4, V)) < 0.4, -np.inf, rng.standard_normal((4, V)) * 30).astype(np.float32)
        bias[:, V - 1] = 0.0
    blocks = sentinel_blocks(4)
    st = None if form == "bias" else state_of(pool, base, state)
    got = run_pick(x, st, bias, blocks)
    want = want_of(x, blocks, pool if st else None, base if st else None, state if st else None, bias, [16] * 4)
    assert np.array_equal(got, want), np.nonzero(got != want)
    assert np.array_equal(got[:, 0], blocks[:, 0])
    assert np.array_equal(got[2], blocks[2]) == (form != "bias")
    assert np.array_equal(got[1], blocks[1]) == (form == "grammar")
    assert (got[0, 1:] != blocks[0, 1:]).any() and (got[3, 1:] != blocks[3, 1:]).any()


@pytest.mark.parametrize("n", [2, 16])
def test_full_vocabulary(n):
    """V = 151936 on a single tile, S = 300 at a non-zero base; n = 2 is a single pick, the rows behind it stay."""
    V = 151936
    rng = np.random.default_rng(7 + n)
    pool, bases = pool_of([GR.case_dfa(rng, 2, V, 0.5), GR.case_dfa(rng, 300, V, 0.5)], V)
    x = GR.case_rows(rng, 16, V)[None]
    blocks = sentinel_blocks(1)
    got = run_pick(x, state_of(pool, [bases[1]], [299]), None, blocks, nrows=n)
    want, states = GD.pick(x[0], n, blocks[0], pool, bases[1], 299)
    assert np.array_equal(got[0], want) and len(states) == n
    assert np.array_equal(got[0, n:], blocks[0, n:]) and got[0, 0] == blocks[0, 0]
    if n == 16:
        assert max(states) > 255                                         # the walk passes states past 255


def test_block_size_from_the_record():
    """n = dyn[t][DYN_BS]: 16, 0 (an idle slot: nothing written), 5 and 1 (a block without a draft token)."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(5)
    pool, bases = pool_of([GR.case_dfa(rng, 7, V, 0.5)], V)
    ns = [16, 0, 5, 1]
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(4)])
    blocks = sentinel_blocks(4)
    dyn = d(np.array([record(bs=c) for c in ns], dtype=np.int32))
    got = run_pick(x, state_of(pool, [bases[0]] * 4, [0, 1, 2, 3]), None, blocks, dyn=dyn, nrows_dyn_word=ops.DYN_BS)
    want = want_of(x, blocks, pool, [bases[0]] * 4, [0, 1, 2, 3], None, ns)
    assert np.array_equal(got, want)
    assert np.array_equal(got[1], blocks[1]) and np.array_equal(got[3], blocks[3])
    assert (got[2, 1:5] >= 0).all() and np.array_equal(got[2, 5:], blocks[2, 5:])


def test_ties_zeros_inf_nan_and_the_last_column():
    """A hand-written grammar over V = 8200: a state whose only legal column is V - 1; a tie between an illegal column
    and two legal ones (the lowest legal one wins, across threads and waves); +0 against -0; a legal set that is all
    -inf (its lowest column); then a legal set that is all NaN, which stops: the rows behind keep their ids."""
    V = 8200
    t = np.full((6, V), -1, np.int16)
    t[0, V - 1] = 1                      # only the last column
    t[1, [70, 4100, 8199]] = 2           # ties
    t[2, [9, 600]] = 3                   # signed zeros
    t[3, [5, 8192]] = 4                  # all -inf
    t[4, [3, 77]] = 5                    # all NaN: stop
    t[5, :] = 0
    pool, bases = pool_of([t], V)
    rng = np.random.default_rng(3)
    x = GR.f32_to_bf16_bits((rng.standard_normal((16, V)) * 4 - 40).astype(np.float32)).reshape(16, V)
    x[1, 17] = 0x42A0                                                        # 80.0 on an illegal column
    x[2, [12, 70, 4100, 8199]] = 0x42A0                                      # 12 is illegal, 70 the lowest legal
    x[3, :] = 0xBF80
    x[3, 9], x[3, 600] = 0x8000, 0x0000                                      # -0 at 9, +0 at 600: equal, 9 wins
    x[4, [5, 8192]] = 0xFF80
    x[5, [3, 77]] = 0x7FC0
    blocks = sentinel_blocks(1)
    got = run_pick(x[None], state_of(pool, bases, [0]), None, blocks)
    want, states = GD.pick(x, 16, blocks[0], pool, bases[0], 0)
    assert np.array_equal(got[0], want)
    assert got[0, 1:5].tolist() == [V - 1, 70, 9, 5] and states == [0, 1, 2, 3, 4]
    assert np.array_equal(got[0, 5:], blocks[0, 5:])


def test_a_successor_outside_the_pool_stops_behind_its_id():
    """The grammar's last transition points past the pool's end (a pool shorter than the table thinks): that id is
    written, the rows behind it keep theirs.  A start state outside the pool writes nothing."""
    V = 64
    t = np.full((3, V), -1, np.int16)
    t[0, 10], t[1, 20], t[2, 30] = 1, 2, 3                                   # 3 = base + 3 is past the pool
    pool, bases = pool_of([t], V)
    assert bases[0] + 3 == len(pool)
    rng = np.random.default_rng(4)
    x = GR.case_rows(rng, 16, V)[None]
    blocks = sentinel_blocks(1)
    got = run_pick(x, state_of(pool, bases, [0]), None, blocks)
    assert got[0, 1:4].tolist() == [10, 20, 30] and np.array_equal(got[0, 4:], blocks[0, 4:])
    assert np.array_equal(got[0], GD.pick(x[0], 16, blocks[0], pool, bases[0], 0)[0])
    got = run_pick(x, state_of(pool, bases, [3]), None, blocks)
    assert np.array_equal(got, blocks)


def test_ban_only_single_slot_forms():
    """The ban-only form on a 2-D tile of 9 rows with a 1-D block and a 1-D bias row; finite biases are ignored; -inf
    on every column but one leaves that column, whatever its logit."""
    from dflash_amd import ops
    V = 2048
    rng = np.random.default_rng(9)
    x = GR.case_rows(rng, 9, V)
    bias = np.where(rng.random(V) < 0.5, -np.inf, rng.standard_normal(V) * 100).astype(np.float32)
    blk = d(sentinel_blocks(1)[0, :9].copy())
    ops.grammar_draft_rows(to_bf16(x), None, bias=d(bias), block=blk)
    want, _ = GD.pick(x, 9, sentinel_blocks(1)[0, :9], bias=bias)
    assert np.array_equal(blk.cpu().numpy(), want)
    only = np.full(V, -np.inf, np.float32)
    only[1234] = -1000.0
    ops.grammar_draft_rows(to_bf16(x), None, bias=d(only), block=blk, nrows=4)
    assert blk.cpu().numpy()[1:4].tolist() == [1234] * 3 and np.array_equal(blk.cpu().numpy()[4:], want[4:])


def test_refusals():
    from dflash_amd import ops
    V = 64
    rng = np.random.default_rng(1)
    pool, bases = pool_of([GR.case_dfa(rng, 2, V)], V)
    x = to_bf16(GR.case_rows(rng, 32, V).reshape(2, 16, V))
    blk = d(np.zeros((2, 16), np.int64))
    with pytest.raises(NotImplementedError):
        ops.grammar_draft_rows(x, state_of(pool, bases * 2, [0, 0]), block=blk, tiles_per_req=2)
    with pytest.raises(ValueError):
        ops.grammar_draft_rows(x, None, block=blk)
    with pytest.raises(TypeError):
        ops.grammar_draft_rows(x, None, bias=d(np.zeros((2, V), np.float64)), block=blk)


def test_row_offset_past_2_31_elements():
    """(base + state) * table_stride beyond 2^31 elements: a pool of about 4.3 GB, allocated uninitialised, of which only
    the rows that are read are written."""
    V, P, base = 151936, 14200, 14000
    assert (base + 136) * V > 2 ** 31
    rng = np.random.default_rng(11)
    t = GR.case_dfa(rng, 4, V, 0.5)                      # relative states 136..139 hold it
    t = np.where(t >= 0, t + 136, -1).astype(np.int16)
    table = torch.empty(P, V, dtype=I16, device=dev())
    table[base + 136:base + 140].copy_(d(t))
    model_pool = np.full((140, V), -1, np.int16)          # the model sees the same rows at base 0
    model_pool[136:140] = t
    st = SimpleNamespace(table=table, base=d(np.array([base], np.int32)), state=d(np.array([137], np.int32)))
    x = GR.case_rows(rng, 16, V)[None]
    blocks = sentinel_blocks(1)
    got = run_pick(x, st, None, blocks, nrows=5)
    want, states = GD.pick(x[0], 5, blocks[0], model_pool, 0, 137)
    assert min(states) >= 136 and np.array_equal(got[0], want)


def test_eager_and_replayed_launches_give_the_same_bits():
    from dflash_amd import ops
    V = 8200
    rng = np.random.default_rng(13)
    pool, bases = pool_of([GR.case_dfa(rng, 5, V, 0.5), GR.case_dfa(rng, 9, V, 0.5)], V)
    st = state_of(pool, bases, [4, 8])
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(2)])
    bias = np.where(rng.random((2, V)) < 0.3, -np.inf, 0).astype(np.float32)
    logits, b = to_bf16(x), d(bias)
    blocks = sentinel_blocks(2)
    eager, replayed = d(blocks), d(blocks)
    ops.grammar_draft_rows(logits, st, bias=b, block=eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        ops.grammar_draft_rows(logits, st, bias=b, block=replayed)
    replayed.copy_(d(blocks))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager, replayed)
    assert np.array_equal(eager.cpu().numpy(), want_of(x, blocks, pool, bases, [4, 8], bias, [16, 16]))
