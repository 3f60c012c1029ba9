"""dfl_grammar_lift and dfl_grammar_reach (grammar_lift.hip) against TokenDFA.from_bytes.

ops.grammar_load of a ByteGrammar must leave in the pool, bit for bit, the table its to_token_dfa() holds: the numpy lift
is the reference, unchanged.  V = 8200 = 8 * 1025: thread 0 of a second workgroup makes the trip for the last 8 tokens.
The vocabulary (grammar_lift_common.seeded_vocabulary): ids 0..255 the single bytes, then seeded empty strings, 1..4
bytes, walks of 17..48 bytes of the case's own automaton (beyond the 8 bytes a thread holds in registers), and such walks
whose last byte dies."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grammar_lift_common as C

pytestmark = pytest.mark.gpu
I16, I32, U8, F32 = torch.int16, torch.int32, torch.uint8, torch.float32
V = 8200
SENT = -77                      # what the lift must not overwrite
REGEX = r"(foo|ba+r|[0-9]{1,3}(\.[0-9]+)?|é[a-z]*)( (foo|ba+r|[0-9]+|\w{2,5}ü))*"
SCHEMA = {"type": "object", "required": ["id", "name"], "properties": {
    "id": {"type": "integer"}, "name": {"type": "string", "maxLength": 12},
    "tags": {"type": "array", "items": {"enum": ["a", "bc", None]}, "maxItems": 3},
    "score": {"type": "number"}, "ok": {"type": "boolean"}}}
NESTED = {"type": "object", "required": ["user"], "properties": {
    "user": {"$ref": "#/$defs/user"}, "items": {"type": "array", "minItems": 1, "items": {"$ref": "#/$defs/user"}},
    "kind": {"anyOf": [{"const": "alpha"}, {"type": "integer"}, {"type": "null"}]}},
    "$defs": {"user": {"type": "object", "required": ["name"], "properties": {
        "name": {"type": "string", "minLength": 1, "maxLength": 8}, "age": {"type": "integer"},
        "mail": {"type": "string", "pattern": "[a-z]{1,6}@[a-z]{1,6}\\.(com|org)"}}}}}
_CACHE = {}


def dev():
    return torch.device("cuda", 0)


def case(name):
    """(ByteGrammar, its reference table int16 [Sc, V]) of a named case, made once."""
    if name not in _CACHE:
        from dflash_amd import ByteGrammar, compile_regex, json_schema_regex
        pattern = {"regex": REGEX, "schema": json_schema_regex(SCHEMA), "nested": json_schema_regex(NESTED),
                   "one": "[a-c]*", "slice": "a{16}|a{3}b"}[name]
        dfa = compile_regex(pattern)
        eos = (97, 300, V - 1) if name in ("one", "regex") else (V - 3,)   # 97 = b"a": legal by its own bytes in "one"
        g = ByteGrammar(dfa, C.seeded_vocabulary(dfa, V, seed=len(name) + 40, eos_ids=eos))
        ref = g.to_token_dfa().next
        _CACHE[name] = (g, ref)
    return _CACHE[name]


def state_of(pool_rows, stride=V, used=0):
    """A grammar state over a pool [pool_rows, stride] full of the sentinel; .table is its first V columns."""
    full = torch.full((pool_rows, stride), SENT, dtype=I16, device=dev())
    return SimpleNamespace(table=full[:, :V], base=torch.full((1,), -1, dtype=I32, device=dev()),
                           state=torch.full((1,), -1, dtype=I32, device=dev()), used=used), full


def test_the_vocabulary_holds_every_kind_of_token():
    """On the reference table alone: long tokens that survive, tokens that die on their last byte, empty ones, and
    both launch forms (the automaton in LDS up to 128 states, through L2 above) are all there in numbers."""
    from dflash_amd import TokenDFA
    g, ref = case("regex")
    toks = g.vocabulary.token_bytes
    lens = np.array([len(t) for t in toks])
    assert toks[:256] == [bytes([b]) for b in range(256)] and (lens == 0).sum() > 300 and lens.max() > 40
    assert (ref[:, lens > 16] >= 0).sum() >= 1000, (ref[:, lens > 16] >= 0).sum()
    cut = TokenDFA.from_bytes(g.char_next, g.accepting, [t[:-1] for t in toks]).next
    died_last = ((cut >= 0) & (ref < 0))[:, lens > 1]
    assert died_last.sum() >= 1000, died_last.sum()
    assert died_last[:, lens[lens > 1] > 16].sum() >= 200
    assert case("regex")[0].num_states <= 128 < case("schema")[0].num_states < case("nested")[0].num_states <= 4096
    assert case("one")[0].num_states == 1 and case("slice")[0].num_states == 17    # 16 < 17: a second slice of one state


@pytest.mark.parametrize("name", ["regex", "schema", "nested", "one", "slice"])
def test_lift_is_bit_equal_to_from_bytes(name):
    from dflash_amd import ops
    g, ref = case(name)
    S = g.num_states
    st, full = state_of(S)
    assert ops.grammar_load(st, g) == 0 and st.used == S
    assert torch.equal(st.table.cpu(), torch.from_numpy(ref))
    if name in ("one", "regex"):   # the eos override shows: b"a" walks to a state, the eos rule says otherwise
        acc = np.zeros(S, bool)
        acc[list(g.accepting)] = True
        assert np.array_equal(ref[:, 97], np.where(acc, np.arange(S), -1)) and (g.char_next[:, 97] >= 0).any()
        assert name == "one" or not np.array_equal(ref[:, 97], g.char_next[:, 97])   # (one state: s either way)


def test_base_stride_and_neighbours_are_kept():
    """base > 0 in a pool whose row stride exceeds V: the rows around the grammar and the slack columns keep the
    sentinel; successors are relative to base."""
    from dflash_amd import ops
    g, ref = case("schema")
    S = g.num_states
    st, full = state_of(S + 9, stride=V + 24, used=5)
    assert ops.grammar_load(st, g) == 5 and st.used == 5 + S
    got = full.cpu().numpy()
    assert np.array_equal(got[5:5 + S, :V], ref)
    assert (got[:5] == SENT).all() and (got[5 + S:] == SENT).all() and (got[:, V:] == SENT).all()


def test_row_offset_past_2_31_elements():
    """Three states at V = 151936 lifted to rows past 14200 of a pool that is really allocated (about 4.3 GB,
    uninitialised but for the neighbours): (base + s) * table_stride exceeds 2^31 elements."""
    from dflash_amd import ByteGrammar, Vocabulary, compile_regex, ops
    Vb, P, base = 151936, 14210, 14204
    assert base * Vb > 2 ** 31
    dfa = compile_regex("a(b|cd)*")                       # start, after a / a loop, after c
    assert dfa.num_states == 3
    rng = np.random.default_rng(5)
    toks = [bytes([b]) for b in range(256)]
    toks += [bytes(rng.choice(np.frombuffer(b"abcd", np.uint8), int(rng.integers(1, 7))).tolist()) for _ in range(Vb - 256)]
    g = ByteGrammar(dfa, Vocabulary(toks, eos_ids=(Vb - 1,)))
    ref = g.to_token_dfa().next
    assert (ref >= 0).sum() > 3000
    table = torch.empty(P, Vb, dtype=I16, device=dev())
    table[base - 1].fill_(SENT), table[base + 3].fill_(SENT)
    st = SimpleNamespace(table=table, base=None, state=None, used=base)
    st.base = st.state = torch.full((1,), -1, dtype=I32, device=dev())
    assert ops.grammar_load(st, g) == base
    assert torch.equal(table[base:base + 3].cpu(), torch.from_numpy(ref))
    assert bool((table[base - 1] == SENT).all()) and bool((table[base + 3] == SENT).all())


@pytest.mark.parametrize("with_bias", [False, True])
def test_reach_equals_the_numpy_model(with_bias):
    from dflash_amd import ops
    g, ref = case("nested")
    S = g.num_states
    st, _ = state_of(S + 2, used=2)
    base = ops.grammar_load(st, g)
    bias = None
    if with_bias:
        rng = np.random.default_rng(9)
        bias = np.where(rng.random(V) < 0.6, -np.inf, rng.standard_normal(V)).astype(np.float32)
        bias[:256] = np.where(rng.random(256) < 0.3, -np.inf, 0).astype(np.float32)
    adj, legal = ops.grammar_reach(st, base, S, None if bias is None else torch.from_numpy(bias))
    want_adj, want_legal = C.reach_model(ref, bias)
    assert np.array_equal(adj.cpu().numpy(), want_adj) and np.array_equal(legal.cpu().numpy(), want_legal)
    assert 0 < want_adj.sum() < S * S
    if with_bias:
        assert want_adj.sum() < C.reach_model(ref)[0].sum()       # the bans close transitions


def test_a_reachable_state_without_a_legal_token_is_refused_and_the_rows_cleared():
    """The state behind b"a" accepts only z, and no token spells z: check_grammar's message, from the device's adj; the
    rows read -1 again and `used` has not moved.  Then the bias form: b and c are all that state 1 takes, both banned."""
    from dflash_amd import ByteGrammar, Vocabulary, compile_regex, ops
    voc = Vocabulary([b"a", b"b", b"ab", b"", b"c", b"ba", b"", b""], eos_ids=(7,))
    full = torch.full((6, 8), SENT, dtype=I16, device=dev())
    st = SimpleNamespace(table=full, base=torch.full((1,), -1, dtype=I32, device=dev()),
                         state=torch.full((1,), -1, dtype=I32, device=dev()), used=1)
    g = ByteGrammar(compile_regex("az"), voc)
    with pytest.raises(ValueError, match="state 1 is reachable from start 0 and has no legal token"):
        ops.grammar_load(st, g)
    with pytest.raises(ValueError, match="state 1 is reachable from start 0 and has no legal token"):
        ops.check_grammar(g.to_token_dfa(), 8)                      # (the host's check says the same)
    assert st.used == 1
    got = full.cpu().numpy()
    assert (got[1:4] == -1).all() and (got[0] == SENT).all() and (got[4:] == SENT).all()
    g = ByteGrammar(compile_regex("a(b|c)"), voc)
    bias = torch.zeros(8)
    bias[1] = bias[4] = -float("inf")
    with pytest.raises(ValueError, match="every legal token of reachable state 1 is banned"):
        ops.grammar_load(st, g, bias)
    assert st.used == 1 and bool((full[1:4] == -1).all())
    assert ops.grammar_load(st, g) == 1 and st.used == 1 + g.num_states
    assert torch.equal(full[1:1 + g.num_states].cpu(), torch.from_numpy(g.to_token_dfa().next))


def test_bad_shapes_are_refused_with_nothing_launched():
    """DFL_EINVAL and the entry point's name; small integers stand for pointers, so a launch would fault: none happens."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(name, *args):
        assert getattr(h, name)(*args) == -22, name
        assert (name + ":").encode() in h.dfl_last_error(), h.dfl_last_error()

    #        table stride pool V  base dfa Sc bytes n  off acc eos n_eos stream
    good = [4096, 64, 10, 64, 2, 4096, 8, 16, 100, 16, 16, 16, 1, None]
    for at, bad in ((0, None), (5, None), (7, None), (9, None), (10, None), (11, None), (3, 60), (3, 0), (6, 0), (6, 4097),
                    (4, 3), (4, -1), (1, 56), (1, 60), (0, 4100), (2, 0)):
        args = list(good)
        args[at] = bad
        refused("dfl_grammar_lift", *args)
    #        table stride pool V  base S  bias adj any stream
    good = [4096, 64, 10, 64, 2, 8, None, 16, 16, None]
    for at, bad in ((0, None), (7, None), (8, None), (3, 60), (5, 0), (5, 4097), (4, 3), (4, -1), (1, 56), (0, 4100)):
        args = list(good)
        args[at] = bad
        refused("dfl_grammar_reach", *args)
