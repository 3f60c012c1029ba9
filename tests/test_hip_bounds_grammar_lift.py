"""Bounds of dfl_grammar_lift and dfl_grammar_reach (grammar_lift.hip) inside a guarded arena (tests/arena.py,
tests/bounds_common.py: W, R, S).

Every buffer has exactly its size: the byte DFA [Sc][256], the byte buffer ending on the last token's last byte (the last
token of the vocabulary is made non-empty), the offsets [V + 1], the accepting flags [Sc], the eos ids, adj [S][S],
any_legal [S], the bias row [V].  The pool is [rows][V + 8] int16 with the grammar in the middle: the 8 slack columns and
the rows around it hold the pattern, and must keep it.  V = 8200 = 8 * 1025.  Both lift forms run: the automaton in LDS
(35 states) and read through L2 (266 states).  The launches go to the library directly: ops.grammar_lift makes its own
device buffers."""
import numpy as np
import pytest
import torch

import arena as A
import bounds_common as B
import grammar_lift_common as C
import test_hip_grammar_lift as L

gpu = pytest.mark.gpu
I16, I32, U8, F32 = torch.int16, torch.int32, torch.uint8, torch.float32
V = L.V
BASE, AFTER = 3, 2

COVERS = {
    "dfl_grammar_lift": "test_grammar_lift_bounds",
    "dfl_grammar_reach": "test_grammar_reach_bounds",
}


def _inputs(name):
    g, ref = L.case(name)
    toks = list(g.vocabulary.token_bytes)
    data, off = g.vocabulary.flat()
    if not toks[-1]:                       # the byte buffer must end on the last token's last byte
        from dflash_amd import ByteGrammar, Vocabulary
        toks[-1] = b"a"
        g = ByteGrammar(g, Vocabulary(toks, g.vocabulary.eos_ids))
        ref = g.to_token_dfa().next
        data, off = g.vocabulary.flat()
    assert off[-1] == data.size and off[-1] > off[-2]
    acc = np.zeros(g.num_states, np.uint8)
    acc[list(g.accepting)] = 1
    return g, ref, data, off, acc, np.asarray(g.vocabulary.eos_ids, np.int32)


@gpu
@pytest.mark.parametrize("name", ["regex", "schema"])
def test_grammar_lift_bounds(name):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import _lib
    from dflash_amd.ops import check
    g, ref, data, off, acc, eos = _inputs(name)
    Sc, rows = g.num_states, BASE + g.num_states + AFTER
    plan = [("table", (rows, V + 8), I16, "index"), ("dfa", (Sc, 256), I16, "index"), ("bytes", data.size, U8, "bytes"),
            ("off", V + 1, I32, "index"), ("acc", Sc, U8, "bytes"), ("eos", eos.size, I32, "index")]

    def make(c, which):
        A.poison(c.table, (slice(None), slice(None)), which, "index")
        c.dfa.copy_(torch.from_numpy(g.char_next)), c.bytes.copy_(torch.from_numpy(data.copy()))
        c.off.copy_(torch.from_numpy(off)), c.acc.copy_(torch.from_numpy(acc)), c.eos.copy_(torch.from_numpy(eos))

    def launch(t):
        check(_lib.lib().dfl_grammar_lift(t.table.data_ptr(), V + 8, rows, V, BASE, t.dfa.data_ptr(), Sc, t.bytes.data_ptr(),
                                          data.size, t.off.data_ptr(), t.acc.data_ptr(), t.eos.data_ptr(), eos.size,
                                          torch.cuda.current_stream().cuda_stream), "dfl_grammar_lift")

    def kept(t):                                           # the rows around the grammar and the slack columns: the pattern
        p = t.table[0, 0]
        return torch.stack([(t.table[:BASE] == p).all(), (t.table[BASE + Sc:] == p).all(), (t.table[:, V:] == p).all()])
    c, res = B.check_launch(V + 8, plan, make, launch, [("rows", lambda t: t.table[BASE:BASE + Sc, :V]), ("kept", kept)])
    assert np.array_equal(res["rows"].cpu().numpy(), ref)
    assert bool(res["kept"].all()), res["kept"]


@gpu
@pytest.mark.parametrize("with_bias", [False, True])
def test_grammar_reach_bounds(with_bias):
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import _lib
    from dflash_amd.ops import check
    g, ref = L.case("schema")
    S, rows = g.num_states, BASE + g.num_states + AFTER
    rng = np.random.default_rng(3)
    bias = np.where(rng.random(V) < 0.5, -np.inf, rng.standard_normal(V)).astype(np.float32)
    plan = [("table", (rows, V + 8), I16, "index"), ("bias", V, F32), ("adj", (S, S), U8, "bytes"),
            ("legal", S, U8, "bytes")]

    def make(c, which):
        A.poison(c.table, (slice(None), slice(None)), which, "index")
        c.table[BASE:BASE + S, :V].copy_(torch.from_numpy(ref))
        c.bias.copy_(torch.from_numpy(bias))
        A.poison(c.adj, (slice(None), slice(None)), which), A.poison(c.legal, slice(None), which)

    def launch(t):
        check(_lib.lib().dfl_grammar_reach(t.table.data_ptr(), V + 8, rows, V, BASE, S,
                                           t.bias.data_ptr() if with_bias else None, t.adj.data_ptr(), t.legal.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream), "dfl_grammar_reach")
    c, res = B.check_launch(V + 8, plan, make, launch, ["adj", "legal"])
    want_adj, want_legal = C.reach_model(ref, bias if with_bias else None)
    assert np.array_equal(res["adj"].cpu().numpy(), want_adj) and np.array_equal(res["legal"].cpu().numpy(), want_legal)
