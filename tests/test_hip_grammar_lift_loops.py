"""ByteGrammar through the decode loops on the tiny walk target of test_hip_grammar_loops.py (its
helpers imported): a grammar lifted on the device drives the same run as its to_token_dfa() copied from the host.

The vocabulary gives the tiny model's 2048 ids byte strings: 0..255 the single bytes, then seeded strings over the
grammars' alphabets (grammar_lift_common.seeded_vocabulary); id 2040 ends a text.  Both regexes are BOUNDED, so a run
reaches a state where the eos id is all that is legal, and ends on it inside its token budget.

For every run: the ids are torch.equal to the TokenDFA run's; the emitted bytes never kill the regex's automaton; a run
that ended on the eos id spells a full match."""
import pytest
import torch

import grammar_lift_common as C
import helpers as H
import test_hip_grammar_loops as GL

pytestmark = pytest.mark.gpu
V, EOS = GL.V, 2040
REGEX_A = r"[a-f0-9]{20,60}(;[a-f]{1,8}){2}"
REGEX_B = r'\{"k":("[a-z ]{3,40}"|-?[0-9]{1,30})(,"v":\[(true|false)(,(true|false)){0,5}\])?\}'
N_NEW = 120
graphs = GL.graphs
_CACHE = {}


def grammar(which):
    if which not in _CACHE:
        from dflash_amd import ByteGrammar, compile_regex
        dfa = compile_regex({"a": REGEX_A, "b": REGEX_B}[which])
        _CACHE[which] = ByteGrammar(dfa, C.seeded_vocabulary(dfa, V, seed=ord(which), eos_ids=(EOS,)))
    return _CACHE[which]


def check_text(r, n_in, g):
    """The emitted bytes: a prefix the automaton has not died on; a full match where the run ended on the eos id.
    Returns whether it did."""
    ids = GL._ids(r)[n_in:]
    ended = EOS in ids
    body = ids[:ids.index(EOS)] if ended else ids
    s = g.start
    for b in b"".join(g.vocabulary.token_bytes[v] for v in body):
        s = int(g.char_next[s, b])
        assert s >= 0
    assert all(len(g.vocabulary.token_bytes[v]) > 0 for v in body)
    if ended:
        assert s in g.accepting and ids[-1] == EOS
    return ended


def same(a, b):
    assert torch.equal(a.output_ids, b.output_ids) and a.grammar_state == b.grammar_state
    assert list(a.acceptance_lengths) == list(b.acceptance_lengths)


@pytest.mark.parametrize("temperature,constrain_draft", [(0.0, False), (GL.T, False), (0.0, True)])
def test_generate_under_a_lifted_grammar(temperature, constrain_draft, monkeypatch, graphs):
    g = grammar("a")
    kw = dict(temperature=temperature, seed=GL.SEED if temperature >= 1e-5 else None, stop=[EOS], n_new=N_NEW,
              **(dict(constrain_draft=True) if constrain_draft else {}))
    ended = []
    for graph in (False, True):
        lifted = GL._single("generate", monkeypatch, None, graph=graph, grammar=g, **kw)
        copied = GL._single("generate", monkeypatch, None, graph=graph, grammar=g.to_token_dfa(), **kw)
        same(lifted, copied)
        assert (lifted.replayed_cycles > 0) == graph
        ended.append(check_text(lifted, GL.N_IN, g))
    assert all(ended)                                   # the bounded language forces the eos id inside 120 tokens


def test_batch_with_a_grammar_per_prompt(monkeypatch, graphs):
    prompts = [GL._prompt(s, n) for s, n in GL.PROMPTS3]
    gs = [grammar("a"), grammar("b"), None]
    hooks = [lambda blk, start, call: None] * 3
    for graph in (False, True):
        lifted = GL._many("batch", monkeypatch, prompts, hooks, n_new=N_NEW, graph=graph, stop=[EOS], grammar=gs)
        copied = GL._many("batch", monkeypatch, prompts, hooks, n_new=N_NEW, graph=graph, stop=[EOS],
                          grammar=[gs[0].to_token_dfa(), gs[1].to_token_dfa(), None])
        for i in range(3):
            same(lifted[i], copied[i])
        assert check_text(lifted[0], prompts[0].shape[1], gs[0]) and check_text(lifted[1], prompts[1].shape[1], gs[1])
        assert lifted[2].grammar_state is None


def test_engine_lifts_a_grammar_behind_its_capture(monkeypatch, graphs):
    """One slot, one capture: grammar A is lifted before the first cycle, grammar B after the engine has captured its
    cycle, into the same pool (its storage has not moved); a request with a bias row is checked on the loaded rows."""
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    pa, pb = GL._prompt(3, 41), GL._prompt(4, 37)
    ga, gb = grammar("a"), grammar("b")

    def run(a, b):
        eng = BatchEngine(GL._draft_model(cfg), GL._native(), slots=1, max_rows=256, out_len=200,
                          mask_token_id=cfg.mask_token_id, grammar_states=ga.num_states + gb.num_states,
                          stop_token_ids=[EOS], logit_bias=True)
        ptr = eng.dec.grammar.table.data_ptr()
        eng.submit(pa, N_NEW, grammar=eng.add_grammar(a))
        ra = eng.run()[0]
        assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] > 0
        hb = eng.add_grammar(b)
        eng.submit(pb, N_NEW, grammar=hb, banned_token_ids=[ord("q"), ord("7")])
        rb = eng.run()[0]
        assert eng.stats["captures"] == 1 and eng.dec.grammar.table.data_ptr() == ptr
        with pytest.raises(ValueError, match="pool is full"):
            eng.add_grammar(a)
        return ra, rb, eng, hb

    ra, rb, eng, hb = run(ga, gb)
    ca, cb, _, _ = run(ga.to_token_dfa(), gb.to_token_dfa())
    same(ra, ca), same(rb, cb)
    assert check_text(ra, 41, ga) and check_text(rb, 37, gb)
    assert ord("q") not in GL._ids(rb)[37:] and ord("7") not in GL._ids(rb)[37:]
    # every token state 0 of B takes is b"{" or begins with it: with them banned, the admission's check on the loaded
    # rows refuses the request
    opening = [v for v, t in enumerate(gb.vocabulary.token_bytes) if gb.to_token_dfa().next[gb.start, v] >= 0]
    eng.submit(pb, 8, grammar=hb, banned_token_ids=opening)
    with pytest.raises(ValueError, match="every legal token of reachable state 0 is banned"):
        eng.run()


def test_only_a_byte_grammar_reaches_the_new_launches(monkeypatch, graphs):
    """grammar=None and grammar=TokenDFA enqueue neither dfl_grammar_lift nor dfl_grammar_reach (a TokenDFA loads by the
    copy of before); a ByteGrammar enqueues one of each, at the load."""
    from dflash_amd import ops
    calls = []
    for name in ("grammar_lift", "grammar_reach"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, _n=name, **k: (calls.append(_n), _real(*a, **k))[1])
    g = grammar("a")
    GL._single("generate", monkeypatch, None, n_new=8)
    GL._single("generate", monkeypatch, None, n_new=8, grammar=None)
    GL._single("generate", monkeypatch, None, n_new=8, grammar=g.to_token_dfa())
    prompts = [GL._prompt(s, n) for s, n in GL.PROMPTS3]
    GL._many("batch", monkeypatch, prompts, [lambda blk, start, call: None] * 3, n_new=8,
             grammar=[g.to_token_dfa(), None, None])
    assert not calls
    GL._single("generate", monkeypatch, None, n_new=8, grammar=g)
    assert calls == ["grammar_lift", "grammar_reach"]
