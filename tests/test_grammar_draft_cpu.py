"""The grammar-aware draft pick without a GPU ("The draft under the grammar"): the numpy model of
grammar_draft_ref.py against grammar_ref's row rule — a picked block walks the automaton, meets only live verify rows, each
pick is the masked row's argmax, the stop rules, the ban-only form —, the C entry point's refusals and the public keyword."""
import inspect

import numpy as np
import pytest

import grammar_draft_ref as GD
import grammar_ref as GR

SENT = -7


def cases():
    """(x bits [16, V], pool, base, state, n) over case_dfa automata at a non-zero base, NaN, +-inf and +-0 in the rows."""
    out = []
    for seed, (S, V, n) in enumerate([(1, 64, 16), (5, 64, 2), (7, 256, 16), (40, 2048, 11), (3, 8, 16)]):
        rng = np.random.default_rng(seed)
        t = GR.case_dfa(rng, S, V)
        pool = np.concatenate([np.full((3, V), -1, np.int16), t])
        out.append((GR.case_rows(rng, 16, V), pool, 3, int(rng.integers(0, S)), n))
    return out


@pytest.mark.parametrize("case", cases(), ids=lambda c: f"S{c[1].shape[0] - 3}-V{c[1].shape[1]}-n{c[4]}")
def test_picked_block_walks_the_automaton_and_meets_live_rows(case):
    x, pool, base, s0, n = case
    blk0 = np.full(16, SENT, np.int64)
    blk, states = GD.pick(x, n, blk0, pool, base, s0)
    assert blk[0] == SENT and (blk[n:] == SENT).all()                    # row 0 and the rows past n are never written
    assert (blk[1:n] >= 0).all()                                         # case_dfa keeps a legal token in every state
    assert states[0] == s0 and len(states) == n
    # 1. the block walks the automaton from the state
    assert GR.walk(pool, base, s0, blk[1:n]) == states[-1] >= 0
    # 2. every verify row over the picked block is live
    z, am, st = GR.rows(x[:n], pool, base, s0, blk)
    assert (st >= 0).all() and st.tolist() == states
    # 3. the pick of row m is the argmax of the row masked by the state reached over block[1 .. m-1], where that is finite
    finite = 0
    for m in range(1, n):
        zm = GR.mask_row(x[m], pool, base, states[m - 1])
        f = GR.bits_to_f32(zm)
        if np.isfinite(f[~np.isnan(f)].max()):
            assert blk[m] == GR.argmax_lowest(zm), m
            finite += 1
        assert pool[base + states[m - 1], blk[m]] >= 0
    assert finite >= (n - 1) // 2


def test_ties_signed_zero_and_inf():
    V = 16
    pool = np.full((2, V), -1, np.int16)
    pool[0, [3, 5, 9]] = 1
    pool[1, [2, 9]] = 0
    x = np.full((16, V), 0xC000, np.uint16)                              # -2.0
    x[1, [1, 3, 5]] = 0x4000                                             # a tie between an illegal (1) and two legal columns
    x[2, 2], x[2, 9] = 0x0000, 0x8000                                    # +0 and -0: equal, the lowest wins
    x[3, 5], x[3, 9] = 0x8000, 0x0000
    x[3, 3] = 0x7FC0                                                     # a NaN never wins
    x[4, [2, 9]] = 0xFF80                                                # every legal column -inf: the lowest of them
    x[4, 0] = 0x7F80                                                     # +inf on an illegal column
    x[5, 9] = 0x7F80                                                     # +inf on a legal one
    blk, st = GD.pick(x, 6, np.full(16, SENT, np.int64), pool, 0, 0)
    assert blk[:6].tolist() == [SENT, 3, 2, 5, 2, 9] and st == [0, 1, 0, 1, 0, 1]


def test_stop_rules():
    V = 16
    rng = np.random.default_rng(2)
    x = GR.case_rows(rng, 16, V)
    pool = np.full((4, V), -1, np.int16)
    pool[1, 4], pool[2, 6] = 1, 3                                        # a grammar at base 1: 0 -4-> 1 -6-> 3 (outside the pool)
    blk0 = np.arange(100, 116, dtype=np.int64)
    # a successor that leaves the pool: that id is written, the rows behind it keep theirs
    blk, st = GD.pick(x, 16, blk0, pool, 1, 0)
    assert blk.tolist() == [100, 4, 6] + list(range(103, 116)) and st == [0, 1, -1]
    # a violated state, a state outside the pool, no grammar and no bias row: untouched
    for base, s in ((1, -1), (1, 3), (-1, 0)):
        blk, st = GD.pick(x, 16, blk0, pool, base, s)
        assert np.array_equal(blk, blk0)
    assert np.array_equal(GD.pick(x, 16, blk0)[0], blk0)
    # a legal set that is all NaN stops; so does a state with no legal column (here: everything legal is banned)
    x2 = x.copy()
    x2[2, 6] = 0x7FC0
    blk, st = GD.pick(x2, 16, blk0, pool, 1, 0)
    assert blk.tolist() == [100, 4] + list(range(102, 116))
    bias = np.zeros(V, np.float32)
    bias[6] = -np.inf
    blk, st = GD.pick(x, 16, blk0, pool, 1, 0, bias)
    assert blk.tolist() == [100, 4] + list(range(102, 116))
    # n = 2: one pick; n < 2: none
    assert GD.pick(x, 2, blk0, pool, 1, 0)[0].tolist() == [100, 4] + list(range(102, 116))
    assert np.array_equal(GD.pick(x, 1, blk0, pool, 1, 0)[0], blk0)
    # the input block is not modified
    assert blk0.tolist() == list(range(100, 116))


def test_ban_only_is_a_per_row_masked_argmax():
    V = 256
    rng = np.random.default_rng(3)
    x = GR.case_rows(rng, 16, V)
    bias = np.where(rng.random(V) < 0.5, -np.inf, rng.standard_normal(V) * 50).astype(np.float32)   # finite values are ignored
    blk, st = GD.pick(x, 13, np.full(16, SENT, np.int64), bias=bias)
    for m in range(1, 13):
        z = np.where(np.isneginf(bias), GR.NEG_INF, x[m]).astype(np.uint16)
        f = GR.bits_to_f32(z)
        if np.isfinite(f[~np.isnan(f)].max()):
            assert blk[m] == GR.argmax_lowest(z)
        assert not np.isneginf(bias[blk[m]])
    assert (blk[13:] == SENT).all() and blk[0] == SENT
    # rows are independent: any row alone gives the same id
    for m in (1, 7, 12):
        one = np.zeros((2, V), np.uint16)
        one[1] = x[m]
        assert GD.pick(one, 2, np.zeros(2, np.int64), bias=bias)[0][1] == blk[m]
    # with a grammar as well: legal in both
    pool = GR.case_dfa(rng, 4, V, 0.6)
    both, st = GD.pick(x, 16, np.full(16, SENT, np.int64), pool, 0, 2, bias)
    k = len(st) - 1
    assert k >= 1
    for m in range(1, k + 1):
        assert pool[st[m - 1], both[m]] >= 0 and not np.isneginf(bias[both[m]])


# ------------------------------------------------------------------------------------------------------- the C entry point
def test_entry_point_refusals_need_no_gpu():
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(word, *args):
        assert h.dfl_grammar_draft_rows(*args) == -22
        msg = h.dfl_last_error()
        assert b"dfl_grammar_draft_rows:" in msg and word in msg, msg

    ok = dict(logits=256, ld=64, tile_stride=1024, tiles=2, V=64, nrows=16, dyn=None, word=-1, table=256, tstride=64,
              pool=4, base=16, state=16, bias=256, bstride=64, block=16, blkstride=16, stream=None)

    def call(**kw):
        return tuple({**ok, **kw}.values())

    refused(b"null", *call(logits=None))
    refused(b"null", *call(table=None, bias=None))
    refused(b"null", *call(base=None))
    refused(b"V=60", *call(V=60))
    refused(b"V=155656", *call(V=155656, ld=155656, tile_stride=16 * 155656, tstride=155656, bstride=155656))
    refused(b"bad shape", *call(ld=60))
    refused(b"bad shape", *call(logits=264))
    refused(b"bad shape", *call(tile_stride=512))
    refused(b"table_stride", *call(tstride=60))
    refused(b"pool_states=0", *call(pool=0))
    refused(b"bias_stride", *call(bstride=32))
    refused(b"nrows=17", *call(nrows=17))
    refused(b"nrows_dyn_word", *call(word=2))
    refused(b"block_stride", *call(blkstride=8))
    # nothing to launch: no tile, or a block without a draft token
    assert h.dfl_grammar_draft_rows(*call(tiles=0)) == 0
    assert h.dfl_grammar_draft_rows(*call(nrows=1)) == 0


def test_the_source_is_built_and_plain():
    import os

    import helpers as H
    from dflash_amd import build
    assert "grammar_draft.hip" in build.SOURCES
    src = open(os.path.join(H.ROOT, "dflash_amd", "csrc", "grammar_draft.hip")).read()
    assert "atomic" not in src.replace("No atomics", "") and "asm" not in src


# ------------------------------------------------------------------------------------------------------ the public keyword
def test_constrain_draft_is_a_keyword_of_every_entry_and_off_by_default():
    from dflash_amd import batch, engine, generate, model
    fns = [generate.DecodeSession.__init__, generate.run_decode, generate.dflash_generate, generate.dflash_generate_policy,
           model.DFlashDraftModel.spec_generate, batch.BatchedDecoder.__init__, batch.dflash_generate_batch,
           engine.BatchEngine.__init__, engine.dflash_generate_stream]
    for fn in fns:
        p = inspect.signature(fn).parameters
        assert "constrain_draft" in p and p["constrain_draft"].default is False, fn
