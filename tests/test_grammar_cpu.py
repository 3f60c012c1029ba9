"""Grammar-constrained decoding without a GPU: the numpy model of grammar_ref.py against
transformers' PrefixConstrainedLogitsProcessor, the two TokenDFA constructors against each other on a hand-written byte
automaton, ops.check_grammar's refusals, the pool's bookkeeping, the C entry points' refusals and the public keywords."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import grammar_ref as GR
import helpers as H


# ------------------------------------------------------------------------------------------------------------ the model
def test_model_is_the_hf_prefix_constraint_walked_over_the_sentence():
    """HF's prefix_allowed_tokens_fn sees the sentence so far; walking it through the automaton and returning the
    state's legal tokens is the row rule.  Rows whose sentence holds an illegal token are dead in the model (copied);
    HF is only asked about the live ones."""
    import torch
    from transformers import PrefixConstrainedLogitsProcessor
    rng = np.random.default_rng(0)
    V, S = 64, 5
    pool = GR.case_dfa(rng, S, V)
    x = GR.f32_to_bf16_bits((rng.standard_normal((12, V)) * 4).astype(np.float32)).reshape(12, V)
    sents = []
    for i in range(12):
        s, sent = 2, []
        for _ in range(i % 5):
            v = int(rng.choice(np.nonzero(pool[s] >= 0)[0]))
            sent.append(v)
            s = int(pool[s, v])
        sents.append(sent + [0] * (4 - len(sent)))      # (padded on the right; the function reads its own length)
    lens = [i % 5 for i in range(12)]

    def allowed(batch_id, sent):
        st = GR.walk(pool, 0, 2, sent.tolist()[:lens[batch_id]])
        return np.nonzero(pool[st] >= 0)[0].tolist()

    got = PrefixConstrainedLogitsProcessor(allowed, 1)(torch.tensor(sents), torch.tensor(GR.bits_to_f32(x).copy())).numpy()
    for i in range(12):
        st = GR.walk(pool, 0, 2, sents[i][:lens[i]])
        assert st >= 0
        want = GR.bits_to_f32(GR.mask_row(x[i], pool, 0, st))
        assert np.array_equal(want, got[i])
        z, am, sts = GR.rows(x[i:i + 1], pool, 0, 2, [99] + sents[i][:lens[i]], row0=lens[i])
        assert np.array_equal(GR.bits_to_f32(z[0]), got[i]) and am[0] == int(np.argmax(got[i])) and sts[0] == st


def test_model_dead_rows_argmax_and_base():
    rng = np.random.default_rng(1)
    V = 16
    pool = np.full((6, V), -1, np.int16)
    pool[4, 3], pool[4, 15], pool[5, 15] = 1, 0, 1          # a grammar of two states at base 4
    x = GR.f32_to_bf16_bits(rng.standard_normal((4, V)).astype(np.float32)).reshape(4, V)
    x[:, 7] = 0x42A0
    z, am, st = GR.rows(x, pool, 4, 0, [0, 3, 15, 2])       # 0 -3-> 1 -15-> 1 -2-> dead
    assert st.tolist() == [0, 1, 1, -1]
    assert sorted(np.nonzero(z[0] != 0xFF80)[0]) == [3, 15] and sorted(np.nonzero(z[1] != 0xFF80)[0]) == [15]
    assert am[1] == 15 and np.array_equal(z[3], x[3]) and am[3] == 7
    assert GR.rows(x, pool, -1, 0, [0, 3, 15, 2])[2].tolist() == [-1] * 4          # no grammar: every row dead
    assert GR.rows(x, pool, 4, -1, [0, 3, 15, 2])[2].tolist() == [-1] * 4          # violated: sticky
    assert GR.step(pool, 4, 0, V) == -1 and GR.step(pool, 4, 0, -1) == -1          # ids outside the vocabulary
    assert GR.advance(pool, 4, -1, [3]) == -1 and GR.advance(pool, -1, 0, [3]) == 0 and GR.advance(pool, 4, 0, []) == 0
    nan_row = np.full(V, 0x7FC0, np.uint16)
    assert GR.argmax_lowest(nan_row) == 0 and GR.argmax_lowest(np.full(V, 0xFF80, np.uint16)) == 0
    ids, s = GR.decode_alone(lambda ids: x[len(ids) % 4], pool, 4, 0, [9], 3)
    assert GR.walk(pool, 4, 0, ids[1:]) == s >= 0


# ------------------------------------------------------------------------------------------------------------ TokenDFA
def _number_dfa():
    """Bytes: an optional sign, one or more digits, a terminator ';'.  0: start, 1: after the sign, 2: in the digits,
    3: done (accepting)."""
    cn = np.full((4, 256), -1, dtype=np.int64)
    for s in (0, 1, 2):
        for c in b"0123456789":
            cn[s, c] = 2
    cn[0, ord("-")] = cn[0, ord("+")] = 1
    cn[2, ord(";")] = 3
    return cn, [3]


def _toy_vocab():
    toks = [b"%d" % i for i in range(10)]                           # 0..9
    toks += [b"-", b"+", b";", b"12", b"-7", b"7;", b"-4;", b"1;2", b";;", b"a", b"", b"--", b"9-", b"007"]
    toks += [b"<eos>", b"<pad>"]
    toks += [b"x%d" % i for i in range(64 - len(toks))]
    return toks, toks.index(b"<eos>")


def test_from_bytes_against_from_dict_on_the_number_automaton():
    from dflash_amd import TokenDFA, ops
    cn, acc = _number_dfa()
    toks, eos = _toy_vocab()
    V = len(toks)
    assert V == 64
    got = TokenDFA.from_bytes(cn, acc, toks, [eos], start=0)
    # the same automaton written by hand, token by token: a plain byte walk per (state, token)
    d = {}
    for s in range(4):
        for v, b in enumerate(toks):
            cur = s
            for c in b:
                cur = int(cn[cur, c]) if cur >= 0 else -1
            if b and cur >= 0 and v != eos:
                d.setdefault(s, {})[v] = cur
    d.setdefault(3, {})[eos] = 3
    want = TokenDFA.from_dict(d, V, start=0)
    assert got.next.dtype == np.int16 and got.next.shape == (4, V) and np.array_equal(got.next, want.next)
    ops.check_grammar(got, V)
    t = {b: i for i, b in enumerate(toks)}
    n = got.next
    assert n[0, t[b"-7"]] == 2 and n[0, t[b"7;"]] == 3 and n[0, t[b"-4;"]] == 3     # tokens that straddle states
    assert n[0, t[b"1;2"]] == -1 and n[0, t[b"9-"]] == -1 and n[0, t[b"--"]] == -1  # tokens that die midway
    assert n[0, t[b"007"]] == 2 and n[1, t[b"-"]] == -1 and n[1, t[b"12"]] == 2
    assert (n[:, t[b""]] == -1).all() and (n[:, t[b"a"]] == -1).all()              # empty strings: illegal everywhere
    assert n[:, eos].tolist() == [-1, -1, -1, 3]                                   # EOS in accepting states only
    assert (n[3, :eos] == -1).all() and (n[3, eos + 1:] == -1).all()
    assert got.num_states == 4 and got.vocab_size == V and got.start == 0


def test_from_dict_and_from_bytes_refuse():
    from dflash_amd import TokenDFA
    with pytest.raises(ValueError, match="outside"):
        TokenDFA.from_dict({0: {8: 0}}, 8)
    with pytest.raises(ValueError, match="negative"):
        TokenDFA.from_dict({0: {1: -2}}, 8)
    with pytest.raises(ValueError, match="states"):
        TokenDFA.from_dict({0: {1: 40000}}, 8)
    assert TokenDFA.from_dict({0: {1: 2}}, 8).next.shape == (3, 8)                 # a successor names a state
    cn, acc = _number_dfa()
    with pytest.raises(ValueError, match="256"):
        TokenDFA.from_bytes(cn[:, :100], acc, [b"1"] * 8)
    bad = cn.copy()
    bad[0, 0] = 4
    with pytest.raises(ValueError, match="successor"):
        TokenDFA.from_bytes(bad, acc, [b"1"] * 8)
    with pytest.raises(ValueError, match="eos"):
        TokenDFA.from_bytes(cn, acc, [b"1"] * 8, [8])


def test_check_grammar_refuses():
    import torch
    from dflash_amd import TokenDFA, ops
    ok = TokenDFA.from_dict({0: {1: 1}, 1: {2: 0}}, 8)
    ops.check_grammar(ok, 8)
    ops.check_grammar(ok, 8, torch.zeros(8))
    for nxt in (ok.next.astype(np.int32), ok.next[0], ok.next.tolist(), torch.from_numpy(ok.next)):
        with pytest.raises(ValueError, match="int16 numpy"):
            ops.check_grammar(TokenDFA(nxt), 8)
    with pytest.raises(ValueError, match="states"):
        ops.check_grammar(TokenDFA(np.zeros((0, 8), np.int16)), 8)
    with pytest.raises(ValueError, match="states"):
        ops.check_grammar(TokenDFA(np.zeros((32768, 8), np.int16)), 8)
    with pytest.raises(ValueError, match="columns"):
        ops.check_grammar(ok, 16)
    with pytest.raises(ValueError, match="columns"):
        ops.check_grammar(TokenDFA(np.zeros((1, 12), np.int16)), 12)               # V % 8
    for v in (2, -2):
        bad = ok.next.copy()
        bad[0, 4] = v
        with pytest.raises(ValueError, match="successor"):
            ops.check_grammar(TokenDFA(bad), 8)
    for st in (2, -1, 1.5, None):
        with pytest.raises(ValueError, match="start"):
            ops.check_grammar(TokenDFA(ok.next, st), 8)
    # a reachable state without a legal token; an unreachable one is nobody's business
    dead = TokenDFA.from_dict({0: {1: 1}, 1: {2: 2}}, 8)
    with pytest.raises(ValueError, match="state 2 .*no legal token"):
        ops.check_grammar(dead, 8)
    ops.check_grammar(TokenDFA.from_dict({0: {1: 0}, 1: {2: 2}}, 8), 8)
    # the bias row bans every legal token of a reachable state
    b = torch.zeros(8)
    b[2] = float("-inf")
    with pytest.raises(ValueError, match="state 1 .*banned"):
        ops.check_grammar(ok, 8, b)
    b[1], b[2] = float("-inf"), 0.0
    with pytest.raises(ValueError, match="state 0 .*banned"):
        ops.check_grammar(ok, 8, b)
    with pytest.raises(ValueError, match="shape"):
        ops.check_grammar(ok, 8, torch.zeros(16))


def test_pool_bookkeeping_on_a_cpu_stand_in():
    import torch
    from dflash_amd import TokenDFA, ops
    st = ops.grammar_state(3, 6, 8, "cpu")
    assert st.table.shape == (6, 8) and st.table.dtype == torch.int16 and (st.table == -1).all()
    assert st.base.tolist() == [-1] * 3 and st.state.tolist() == [-1] * 3 and st.used == 0
    ptr = st.table.data_ptr()
    a = TokenDFA.from_dict({0: {1: 1}, 1: {2: 0}}, 8)
    b = TokenDFA.from_dict({0: {3: 1}, 1: {4: 2}, 2: {5: 0}}, 8, start=1)
    assert ops.grammar_load(st, a) == 0 and ops.grammar_load(st, b) == 2 and st.used == 5
    assert np.array_equal(st.table[0:2].numpy(), a.next) and np.array_equal(st.table[2:5].numpy(), b.next)
    assert (st.table[5] == -1).all() and st.table.data_ptr() == ptr
    with pytest.raises(ValueError, match="pool is full"):
        ops.grammar_load(st, a)
    assert st.used == 5
    assert ops.grammar_load(st, TokenDFA.from_dict({0: {1: 0}}, 8)) == 5 and st.used == 6
    with pytest.raises(ValueError, match="no legal token"):
        ops.grammar_load(ops.grammar_state(1, 4, 8, "cpu"), TokenDFA.from_dict({0: {1: 1}}, 8))
    ops.grammar_set(st, 1, 2, b.start)
    ops.grammar_set(st, 2, 0, 0)
    assert st.base.tolist() == [-1, 2, 0] and st.state.tolist() == [-1, 1, 0]
    ops.grammar_set(st, 1, None)
    assert st.base.tolist() == [-1, -1, 0] and st.state.tolist() == [-1, -1, 0]
    for kw in (dict(slot=3, base=0), dict(slot=0, base=6), dict(slot=0, base=4, start=2), dict(slot=0, base=0, start=-1)):
        with pytest.raises(ValueError, match="grammar_set"):
            ops.grammar_set(st, **kw)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.grammar_state(1, 4, 12, "cpu")
    with pytest.raises(TypeError, match="GPU"):
        ops.grammar_advance(st, torch.zeros(3, 4, dtype=torch.long))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def _rows(h, logits=16, out=32, ld=64, tstride=1024, tiles=1, V=64, row0=0, nrows=16, dyn=None, nword=-1, tpr=1, table=48,
          table_stride=64, pool=4, base=64, state=80, block=None, block_stride=0, out_ids=None, out_stride=0, out_off=0):
    return h.dfl_grammar_rows(logits, out, ld, tstride, tiles, V, row0, nrows, dyn, nword, tpr, table, table_stride, pool,
                              base, state, block, block_stride, out_ids, out_stride, out_off, None)


def _adv(h, table=48, table_stride=64, pool=4, V=64, base=64, state=80, slots=0, ids=96, ids_stride=8, ids_len=8, dyn=None,
         lo_word=0, hi_word=0, lo=0, hi=0):
    return h.dfl_grammar_advance(table, table_stride, pool, V, base, state, slots, ids, ids_stride, ids_len, dyn, lo_word,
                                 hi_word, lo, hi, None)


def test_entry_points_refuse_by_name():
    """Small integers stand for pointers: nothing launches."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(call, name, word, **kw):
        assert call(h, **kw) == -22, kw
        err = h.dfl_last_error()
        assert name in err and word in err, (kw, err)

    assert _rows(h, tiles=0) == 0 and _rows(h, nrows=0) == 0 and _adv(h) == 0      # nothing to do
    for name in ("logits", "out", "table", "base", "state"):
        refused(_rows, b"dfl_grammar_rows:", b"null", **{name: None})
    for v in (0, -8, 4, 60, 155656):
        refused(_rows, b"dfl_grammar_rows:", b"V=", V=v, ld=max(v, 64), table_stride=max(v, 64))
        refused(_adv, b"dfl_grammar_advance:", b"V=", V=v, table_stride=max(v, 64))
    for tpr in (0, 3):
        refused(_rows, b"dfl_grammar_rows:", b"tiles_per_req", tpr=tpr)
    refused(_rows, b"dfl_grammar_rows:", b"ld=32", ld=32)
    refused(_rows, b"dfl_grammar_rows:", b"bad shape", logits=18)
    refused(_rows, b"dfl_grammar_rows:", b"tile_stride=512", tiles=2, tstride=512)
    for call, name in ((_rows, b"dfl_grammar_rows:"), (_adv, b"dfl_grammar_advance:")):
        refused(call, name, b"table_stride=32", table_stride=32)
        refused(call, name, b"table_stride=68", table_stride=68)                  # a multiple of 4 is not enough: 8 columns a load
        refused(call, name, b"table_stride", table=24)                            # a pool row off 16 bytes
        refused(call, name, b"pool_states=0", pool=0)
    refused(_rows, b"dfl_grammar_rows:", b"rows [4,17)", row0=4, nrows=13)
    refused(_rows, b"dfl_grammar_rows:", b"nrows_dyn_word=2", nword=2)
    refused(_rows, b"dfl_grammar_rows:", b"nrows_dyn_word=8", nword=8, dyn=16)
    refused(_rows, b"dfl_grammar_rows:", b"negative", out_off=-1)
    for name in ("table", "base", "state", "ids"):
        refused(_adv, b"dfl_grammar_advance:", b"null", **{name: None})
    refused(_adv, b"dfl_grammar_advance:", b"slots=-1", slots=-1)
    refused(_adv, b"dfl_grammar_advance:", b"ids_stride=4", slots=2, ids_stride=4)
    refused(_adv, b"dfl_grammar_advance:", b"lo_word=8", dyn=16, lo_word=8)
    refused(_adv, b"dfl_grammar_advance:", b"hi_word=-1", dyn=16, hi_word=-1)


def test_header_binding_and_sources_agree():
    from dflash_amd import _lib, build
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n in (("dfl_grammar_rows", 22), ("dfl_grammar_advance", 16)):
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SIGNATURES[name][1]) == n
        assert hasattr(_lib.lib(), name)
    assert "grammar.hip" in build.SOURCES
    src = open(os.path.join(H.ROOT, "dflash_amd", "csrc", "grammar.hip")).read()
    assert "atomic" not in src.split("#include")[1]                                # no atomics at all in the code
    import dflash_amd
    assert dflash_amd.TokenDFA is __import__("dflash_amd.grammar", fromlist=["TokenDFA"]).TokenDFA
    assert "TokenDFA" in dflash_amd.__all__


# ------------------------------------------------------------------------------------------------------------ keywords
def test_refusals_that_need_no_launch():
    import torch
    from dflash_amd import DFlashDraftModel, TokenDFA
    from dflash_amd.batch import BatchedDecoder, dflash_generate_batch, dflash_generate_policy_batch
    from dflash_amd.engine import BatchEngine, dflash_generate_stream
    from dflash_amd.generate import DecodeSession, dflash_generate, dflash_generate_policy, run_decode
    from dflash_amd.target import NativeTarget
    model = SimpleNamespace(device=torch.device("cpu"))
    ids = torch.zeros(1, 8, dtype=torch.long)
    kw = dict(mask_token_id=5, max_new_tokens=8, stop_token_ids=[3])
    g = TokenDFA.from_dict({0: {1: 1, 3: 0}, 1: {2: 0}}, 64)
    hf = SimpleNamespace(config=SimpleNamespace(vocab_size=64))             # a wrapped model: no NativeTarget
    for target in (hf, object()):
        with pytest.raises(ValueError, match="NativeTarget"):
            DecodeSession(model, target, ids, max_block_size=16, temperature=0.0, grammar=g, **kw)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(model, hf, ids, 5, 8, 16, [3], grammar=g)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate_policy(model=model, target=hf, input_ids=ids, temperature=0.0, fixed_block_size=8, grammar=g, **kw)
    with pytest.raises(ValueError, match="NativeTarget"):
        run_decode(model, hf, ids, block_size=8, temperature=0.0, clamp_tail=True, grammar=g, **kw)
    native = object.__new__(NativeTarget)       # (the checks come before the target is touched: a stand-in with a vocabulary)
    native.V = 64
    with pytest.raises(ValueError, match="sampler='device'"):
        DecodeSession(model, native, ids, max_block_size=16, temperature=0.7, grammar=g, **kw)
    with pytest.raises(NotImplementedError, match="16 rows"):
        DecodeSession(model, native, ids, max_block_size=24, temperature=0.0, grammar=g, **kw)
    with pytest.raises(NotImplementedError, match="16 rows"):
        dflash_generate_batch(None, native, [ids], 5, 8, 24, [3], grammar=g)
    with pytest.raises(NotImplementedError, match="16 rows"):
        BatchedDecoder(None, native, 1, 64, 64, 5, tiles_per_request=2, grammar_states=4)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchedDecoder(None, native, 1, 64, 64, 5, temperature=0.7, grammar_states=4)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchEngine(None, native, max_rows=64, out_len=64, mask_token_id=5, temperature=0.7, grammar_states=4)
    with pytest.raises(ValueError, match="grammar_states"):
        BatchedDecoder(None, native, 1, 64, 64, 5, grammar_states=-1)
    # a bad automaton, before anything runs; one per prompt
    bad = TokenDFA(np.zeros((2, 60), np.int16))
    with pytest.raises(ValueError, match="columns"):
        dflash_generate_batch(None, native, [ids], 5, 8, 16, [3], grammar=bad)
    with pytest.raises(ValueError, match="columns"):
        dflash_generate_stream(None, native, [ids], 5, 8, 16, [3], grammar=[bad])
    with pytest.raises(ValueError, match="one per prompt"):
        dflash_generate_batch(None, native, [ids, ids, ids], 5, 8, 16, [3], grammar=[g, None])
    with pytest.raises(ValueError, match="one per prompt"):
        dflash_generate_stream(None, native, [ids], 5, 8, 16, [3], grammar=[g, g])
    # a decoder without a pool, a full pool, a handle it did not return
    dec = object.__new__(BatchedDecoder)
    with pytest.raises(ValueError, match="grammar_states > 0"):
        dec.add_grammar(g)
    with pytest.raises(ValueError, match="grammar_states > 0"):
        dec.check_grammar_handle(0)
    assert dec.check_grammar_handle(None) is None
    from dflash_amd import ops
    dec.grammar, dec._grammars = ops.grammar_state(2, 3, 64, "cpu"), []
    assert dec.add_grammar(g) == 0 and dec.check_grammar_handle(0) == (0, g)
    with pytest.raises(ValueError, match="pool is full"):
        dec.add_grammar(g)
    for handle in (1, -1, True, "0", 0.0):
        with pytest.raises(ValueError, match="no handle"):
            dec.check_grammar_handle(handle)
    eng = object.__new__(BatchEngine)
    eng.dec = dec
    assert eng.add_grammar(TokenDFA.from_dict({0: {1: 0}}, 64)) == 1
    with pytest.raises(ValueError, match="no handle"):
        eng.submit(ids, 8, grammar=7)
    # grammar=None is the call without the keyword: nothing above is asked of it
    with pytest.raises(RuntimeError, match="GPU"):
        DecodeSession(model, hf, ids, max_block_size=24, temperature=0.7, grammar=None, **kw)
    # the keyword is where the issue puts it, and nowhere else
    for fn in (DecodeSession.__init__, run_decode, dflash_generate, dflash_generate_policy, DFlashDraftModel.spec_generate,
               dflash_generate_batch, dflash_generate_stream, BatchedDecoder.admit, BatchedDecoder.admit_fused,
               BatchEngine.submit, NativeTarget.verify):
        assert "grammar" in inspect.signature(fn).parameters, fn
    assert "grammar" not in inspect.signature(dflash_generate_policy_batch).parameters
    for cls in (BatchedDecoder, BatchEngine):
        assert inspect.signature(cls.__init__).parameters["grammar_states"].default == 0
