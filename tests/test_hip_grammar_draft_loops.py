"""The grammar-aware draft through the decode loops ("The draft under the grammar"): single request,
policy, ragged batch, slot-refill engine — on the tiny walk target of test_hip_grammar_loops.py (helpers copied, not
imported) and a draft model of random weights, whose argmax hits a given token about once in 2048 tries.

The forced chain: a cycle of 37 states with exactly one legal token each.  The target can only emit the chain; a draft
picked under the automaton proposes exactly the chain, so every cycle accepts its whole block, where the plain draft gets
its first token rejected nearly always.  The mixed grammar: every third state is free over the even tokens, the others are
forced; a recording hook compares every cycle's block with the numpy model of grammar_draft_ref.py over the session's own
draft logits.  The emitted ids never depend on the switch."""
import numpy as np
import pytest
import torch

import grammar_draft_ref as GD
import grammar_ref as GR
import helpers as H
import penalties_ref as PR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048
T = 0.7
N_IN = 41
MASK = 2047
NS = 37
_STATE = {}


def dev():
    return torch.device("cuda", 0)


def _walk_target():
    """The greedy-walk target (6 layers, walk seed 8) with lm_head row perm[t] = 0.002 * embedding[t] for a permutation of
    6-cycles over the ids 0..2045 (2046 <-> 2047: the mask id is on no prompt's walk)."""
    if "hf" not in _STATE:
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        torch.manual_seed(11)
        hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev(), dtype=BF16)
        impose_greedy_walk(hf, seed=8)
        order = torch.randperm(V - 2, generator=torch.Generator().manual_seed(8))
        perm = torch.arange(V)
        for i in range(V - 2):
            perm[order[i]] = order[6 * (i // 6) + (i + 1) % 6]
        perm[V - 2], perm[V - 1] = V - 1, V - 2
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(V)
        with torch.no_grad():
            emb = hf.model.embed_tokens.weight.float()
            hf.lm_head.weight.copy_((emb[inv.to(dev())] * 0.002).to(BF16))
        _STATE["hf"] = hf
    return _STATE["hf"]


def _native():
    from dflash_amd import NativeTarget
    return NativeTarget(_walk_target())


def _draft_model(cfg):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return m


def _script(sizes=(8, 12, 16)):
    from dflash_amd.generate import _Fixed
    a, b, c = sizes

    class Script(_Fixed):
        def select(self, cyc):
            return (c, a, b, c, b, a)[cyc % 6]

    s = Script(c)
    s.candidates = tuple(sizes)
    return s


def _prompt(seed=3, n=N_IN):
    return torch.randint(0, 2000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev())


PROMPTS3 = ((3, 41), (4, 37), (5, 45))


def _ids(r):
    return r.output_ids[0].tolist()


# ------------------------------------------------------------------------------------------------------------ the grammars
SEQ = torch.randperm(2000, generator=torch.Generator().manual_seed(37))[:NS].tolist()    # (no mask id among them)
EVEN = list(range(0, V, 2))


def _chain(shift=0):
    """The forced chain: state i has the one legal token SEQ[(i + shift) % 37] and leads to state i + 1 (mod 37)."""
    from dflash_amd import TokenDFA
    return TokenDFA.from_dict({i: {SEQ[(i + shift) % NS]: (i + 1) % NS} for i in range(NS)}, V, 0)


def _mixed():
    """Every third state is free over the even tokens, the others are forced to SEQ[i]; all lead to state i + 1."""
    from dflash_amd import TokenDFA
    key = "mixed"
    if key not in _STATE:
        nxt = np.full((NS, V), -1, dtype=np.int16)
        for i in range(NS):
            if i % 3 == 0:
                nxt[i, EVEN] = (i + 1) % NS
            else:
                nxt[i, SEQ[i]] = (i + 1) % NS
        _STATE[key] = nxt
    return TokenDFA(_STATE[key], start=0)


def _chain_ids(n, shift=0):
    return [SEQ[(i + shift) % NS] for i in range(n)]


# ------------------------------------------------------------------------------------------------------------ the audit
def _raw_rows(ids, n_in):
    hf = _walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    return PR.f32_to_bf16_bits(logits[n_in - 1:len(ids) - 1]).reshape(len(ids) - n_in, V)


def _audit(ids, n_in, g=None, bias=None):
    """T = 0: every emitted token against the teacher-forced row of its prefix — the bans, then the grammar mask by the
    state the emitted prefix reaches — wherever that row's top-2 gap is >= 4 bf16 ulp (the screen of
    test_hip_grammar_loops.py).  Returns (emitted, screen)."""
    x = _raw_rows(ids, n_in)
    got = np.asarray(ids[n_in:])
    want, safe = np.zeros(len(got), dtype=np.int64), np.zeros(len(got), dtype=bool)
    s = 0 if g is None else g.start
    for i in range(len(got)):
        z = x[i] if bias is None else np.where(np.isneginf(bias), GR.NEG_INF, x[i]).astype(np.uint16)
        if g is not None:
            z = GR.mask_row(z, g.next, 0, s)
            s = GR.step(g.next, 0, s, got[i])
            assert s >= 0, (i, got[i])
        want[i], safe[i] = GR.argmax_lowest(z), GR.bf16_ulp_gap(z) >= 4
    print(f"[grammar draft] audit of {len(got)} positions: screen keeps {safe.mean():.3f}")
    assert safe.mean() >= 0.5, safe.mean()
    assert np.array_equal(got[safe], want[safe]), (np.nonzero(safe & (got != want))[0][:8], safe.mean())
    return got, safe


def _same_until_a_near_tie(a, b):
    """Two audited runs of one request: a divergence may only start at a position either screen left out."""
    ga, sa, gb, sb = a[0], a[1], b[0], b[1]
    n = min(len(ga), len(gb))
    diff = np.nonzero(ga[:n] != gb[:n])[0]
    if diff.size:
        assert not (sa[diff[0]] and sb[diff[0]]), diff[0]
    return diff.size == 0


# ------------------------------------------------------------------------------------------------------------ the runs
@pytest.fixture
def graphs():
    """Sessions hold their hipGraphs: collect them with the test, so that no capture state outlives this file's tests."""
    import gc
    yield
    gc.collect()


def _single(kind, monkeypatch, hook=None, *, graph=True, temperature=0.0, seed=None, n_new=100, prompt=None, bs=16, **kw):
    """dflash_generate / dflash_generate_policy (a scripted scheduler over 8 / 12 / 16 rows) on a fresh draft and target."""
    from dflash_amd import dflash_generate, dflash_generate_policy
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    cfg = H.tiny_cfg()
    prompt = _prompt() if prompt is None else prompt
    skw = dict(sampler="device", seed=seed) if temperature >= 1e-5 else {}
    if kind == "generate":
        return dflash_generate(_draft_model(cfg), _native(), prompt, cfg.mask_token_id, n_new, bs, None, temperature,
                               draft_token_hook=hook, **skw, **kw)
    return dflash_generate_policy(model=_draft_model(cfg), target=_native(), input_ids=prompt,
                                  mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, stop_token_ids=None,
                                  temperature=temperature, scheduler=_script(), draft_token_hook=hook, **skw, **kw)


def _many(entry, monkeypatch, prompts, hooks=None, *, temperature=0.0, seeds=None, n_new=80, graph=True, slots=2, **kw):
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import dflash_generate_stream
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    cfg = H.tiny_cfg()
    fn = dflash_generate_batch if entry == "batch" else dflash_generate_stream
    extra = dict(slots=slots) if entry == "stream" else {}
    skw = dict(sampler="device", seed=seeds) if temperature >= 1e-5 else {}
    hook = (lambda i, blk, start, call: hooks[i](blk, start, call)) if hooks else None
    return fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, n_new, 16, None, temperature,
              draft_token_hook=hook, **skw, **extra, **kw)


def _full_blocks(taus, sizes, n_new):
    """Every cycle but the last accepted its whole block: tau == the cycle's block size, `sizes` clamped to what is left
    of the request (the prefill emitted the first of the n_new tokens: the block's slot 0)."""
    left, want = n_new, []
    for i in range(len(taus)):
        want.append(max(1, min(sizes[i % len(sizes)], left)))
        left -= taus[i]
    assert len(taus) >= 3
    assert list(taus[:-1]) == want[:-1], (list(taus), want)


SIZES = dict(generate=(16,), policy=(16, 8, 12, 16, 12, 8), batch=(16,), stream=(16,))


# ------------------------------------------------------------------------------------------------------------ the forced chain
@pytest.mark.parametrize("temperature", [0.0, T])
@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_forced_chain_accepts_every_block(entry, temperature, monkeypatch, graphs):
    """THE test that fails without the feature.  With constrain_draft every cycle's acceptance length is its block size
    (the last cycle excepted: max_new_tokens clamps it) and the ids are the chain, eager and replayed; without it the same
    ids come out at a far smaller mean acceptance length — the random draft proposes the one legal token of 2048 about
    once in 2048 tries, so the plain run commits about one token per cycle: a quarter of the constrained mean is a bound
    with a wide margin on both sides (about 1 against 12 .. 16).
    The policy loop drafts at the request's temperature: at T = 0.7 its draft is sampled, which constrain_draft refuses
    (NotImplementedError) — that combination is checked as the refusal it is."""
    g = _chain()
    n_new = 100
    if entry == "policy" and temperature >= 1e-5:
        with pytest.raises(NotImplementedError, match="greedy draft"):
            _single(entry, monkeypatch, temperature=temperature, seed=5, n_new=16, grammar=g, constrain_draft=True)
        return
    if entry in ("generate", "policy"):
        kw = dict(temperature=temperature, seed=5, n_new=n_new, grammar=g)
        on = [_single(entry, monkeypatch, graph=gr, constrain_draft=True, **kw) for gr in (False, True)]
        off = _single(entry, monkeypatch, graph=True, **kw)
        assert on[1].replayed_cycles > 0 and on[0].replayed_cycles == 0
        groups = [([r], [off], N_IN) for r in on]
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        kw = dict(temperature=temperature, seeds=[5, 6, 7], n_new=n_new, grammar=g)
        on = [_many(entry, monkeypatch, prompts, graph=gr, constrain_draft=True, **kw) for gr in (False, True)]
        off = _many(entry, monkeypatch, prompts, graph=True, **kw)
        groups = [(rs, off, None) for rs in on]
    for rs, offs, _ in groups:
        for r, o in zip(rs, offs):
            n_in = r.num_input_tokens
            assert _ids(r)[n_in:] == _chain_ids(n_new) and _ids(o) == _ids(r)
            assert r.grammar_state == n_new % NS
            _full_blocks(r.acceptance_lengths, SIZES[entry], n_new)
            m_on, m_off = np.mean(r.acceptance_lengths), np.mean(o.acceptance_lengths)
            print(f"[grammar draft] {entry} T={temperature}: mean acceptance length {m_on:.2f} constrained, {m_off:.2f} plain")
            assert 4 * m_off <= m_on, (m_off, m_on)


# ------------------------------------------------------------------------------------------------------------ the mixed grammar
def _bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _recorded_run(monkeypatch, *, graph, g=None, bias=None, n_new=100, **kw):
    """dflash_generate with constrain_draft and a recording hook: per hook call (block size, the slot's state at that
    moment, whether the draft came from a run-ahead launch, the block as the hook saw it, the model's block from the
    session's own draft logits and that state).  Returns (result, records, replayed flags per cycle)."""
    from dflash_amd import generate
    sessions, ahead, recs, flags = [], [False], [], []
    if "reals" not in _STATE:   # (the methods themselves, whatever an earlier call of this function has patched in)
        _STATE["reals"] = (generate.DecodeSession.__init__, generate.DecodeSession._take_ahead,
                           generate.DecodeSession._commit)
    real_init, real_take, real_commit = _STATE["reals"]

    def init(self, *a, **k):
        real_init(self, *a, **k)
        sessions.append(self)

    def take(self, blk):
        ahead[0] = True
        return real_take(self, blk)

    def commit(self, res, bs, start, rows, replayed):
        if bs > 1:   # (a one-row tail cycle has no draft and calls no hook)
            flags.append(bool(replayed))
        return real_commit(self, res, bs, start, rows, replayed)

    monkeypatch.setattr(generate.DecodeSession, "__init__", init)
    monkeypatch.setattr(generate.DecodeSession, "_take_ahead", take)
    monkeypatch.setattr(generate.DecodeSession, "_commit", commit)

    def hook(blk, start, call):
        s = sessions[-1]
        torch.cuda.synchronize()
        x = _bits(s.draft_logits[:16].clone())
        st = int(s.gr.state.item()) if s.gr is not None else -1
        seen = blk[0].cpu().numpy().copy()
        want, _ = GD.pick(x, blk.shape[1], seen, None if g is None else g.next, 0 if g is not None else -1, st, bias)
        recs.append(SimpleRec(blk.shape[1], st, ahead[0], seen, want, x))
        ahead[0] = False

    r = _single("generate", monkeypatch, hook, graph=graph, n_new=n_new, grammar=g, constrain_draft=True, **kw)
    for name, fn in zip(("__init__", "_take_ahead", "_commit"), _STATE["reals"]):
        monkeypatch.setattr(generate.DecodeSession, name, fn)
    return r, recs, flags


class SimpleRec:
    def __init__(self, bs, state, ahead, seen, want, x):
        self.bs, self.state, self.ahead, self.seen, self.want, self.x = bs, state, ahead, seen, want, x


def test_mixed_grammar_blocks_match_the_model_eager_run_ahead_and_replayed(monkeypatch, graphs):
    """Every cycle's block, as the hook sees it, is bit for bit the numpy model's pick over a clone of the session's
    draft logits from the slot's state — for eager, run-ahead and replayed cycles; the ids equal the plain run's up to
    the first near-tie of either run's teacher-forced rows.
    the_run_ahead_pick_reads_the_state_after_the_advance: a run-ahead (or replayed) draft is enqueued behind the accept
    launch of the cycle before; its block must be the model's pick from the state AFTER that cycle's advance, which is
    what the slot holds when the hook runs — and, the grammar's forced tokens differing from state to state, not the
    pick from the state in front of the advance."""
    g = _mixed()
    n_new = 100
    off = _single("generate", monkeypatch, graph=True, n_new=n_new, grammar=g)
    kinds = set()
    for graph in (False, True):
        r, recs, flags = _recorded_run(monkeypatch, graph=graph, g=g, n_new=n_new)
        assert len(recs) == len(flags) >= 3 and len(r.acceptance_lengths) - len(flags) in (0, 1)
        assert (r.replayed_cycles > 0) == graph
        prev = None
        stale = 0
        for c, (rec, replayed) in enumerate(zip(recs, flags)):
            kind = "replayed" if replayed else ("run-ahead" if rec.ahead else "eager")
            kinds.add(kind)
            assert np.array_equal(rec.seen, rec.want), (kind, c, rec.state, rec.seen, rec.want)
            # every draft token is legal where the verify's row will stand: the block walks the automaton
            assert GR.walk(g.next, 0, rec.state, rec.seen[1:rec.bs]) >= 0, (kind, c)
            if kind != "eager":     # the_run_ahead_pick_reads_the_state_after_the_advance
                assert prev is not None and rec.state != prev.state      # (every cycle commits at least one token)
                old, _ = GD.pick(rec.x, rec.bs, rec.seen, g.next, 0, prev.state)
                stale += int(GR.walk(g.next, 0, rec.state, old[1:rec.bs]) < 0)
            prev = rec
        if graph:
            assert stale >= 3, stale       # a pick from the state in front of the advance would have been illegal there
        ua, ub = _audit(_ids(r), N_IN, g), _audit(_ids(off), N_IN, g)
        same = _same_until_a_near_tie(ua, ub)
        print(f"[grammar draft] mixed grammar, graph={graph}: ids equal the plain run's: {same}; mean acceptance length "
              f"{np.mean(r.acceptance_lengths):.2f} constrained, {np.mean(off.acceptance_lengths):.2f} plain")
        assert r.grammar_state == off.grammar_state or not same
    assert kinds == {"eager", "run-ahead", "replayed"}, kinds


def test_mixed_grammar_other_entries_emit_the_plain_ids(monkeypatch, graphs):
    """policy, batch and stream under the mixed grammar at T = 0: the ids of the run without the switch (up to a
    near-tie), at an acceptance length that is no smaller."""
    g = _mixed()
    on = _single("policy", monkeypatch, n_new=80, grammar=g, constrain_draft=True)
    off = _single("policy", monkeypatch, n_new=80, grammar=g)
    pairs = [(on, off)]
    prompts = [_prompt(s, n) for s, n in PROMPTS3]
    for entry in ("batch", "stream"):
        a = _many(entry, monkeypatch, prompts, n_new=60, grammar=g, constrain_draft=True)
        b = _many(entry, monkeypatch, prompts, n_new=60, grammar=g)
        pairs += list(zip(a, b))
    for a, b in pairs:
        n_in = a.num_input_tokens
        _same_until_a_near_tie(_audit(_ids(a), n_in, g), _audit(_ids(b), n_in, g))
        assert np.mean(a.acceptance_lengths) > np.mean(b.acceptance_lengths)


# ------------------------------------------------------------------------------------------------------------ ban-only
def _drafted(monkeypatch, **kw):
    """A plain run's result and the draft tokens its hook saw, cycle by cycle."""
    seen = []
    r = _single("generate", monkeypatch, lambda blk, start, call: seen.append(blk[0, 1:].tolist()), n_new=80, **kw)
    return r, seen


@pytest.mark.parametrize("case", ["even", "drafted"])
def test_ban_only_drafts_no_banned_token(case, monkeypatch, graphs):
    """No grammar.  even: allowed_token_ids = the even tokens.  drafted: banned_token_ids = tokens this draft model does
    propose on this prompt (taken from a run without any ban), so that the plain draft under the same bans still
    proposes banned tokens — the random draft's favourites need not be odd.  With constrain_draft every recorded draft
    token is allowed and is the model's pick, eager and replayed; the ids equal the plain run's up to a near-tie."""
    bias = np.zeros(V, np.float32)
    if case == "even":
        bias[1::2] = -np.inf
        kw = dict(allowed_token_ids=EVEN)
    else:
        proposed = sorted({v for blk in _drafted(monkeypatch)[1] for v in blk if v != MASK})
        assert proposed
        bias[proposed[:64]] = -np.inf
        kw = dict(banned_token_ids=proposed[:64])
    off, plain = _drafted(monkeypatch, **kw)
    hits = sum(int(np.isneginf(bias[blk]).sum()) for blk in plain)
    print(f"[grammar draft] ban-only {case}: the plain draft proposes {hits} banned tokens")
    if case == "drafted":
        assert hits > 0
    for graph in (False, True):
        r, recs, flags = _recorded_run(monkeypatch, graph=graph, bias=bias, n_new=80, **kw)
        assert (r.replayed_cycles > 0) == graph
        for rec in recs:
            assert not np.isneginf(bias[rec.seen[1:rec.bs]]).any() and np.array_equal(rec.seen, rec.want)
        _same_until_a_near_tie(_audit(_ids(r), N_IN, bias=bias), _audit(_ids(off), N_IN, bias=bias))
        assert not np.isneginf(bias[_ids(r)[N_IN:]]).any()
        print(f"[grammar draft] ban-only {case}, graph={graph}: mean acceptance length "
              f"{np.mean(r.acceptance_lengths):.2f} constrained, {np.mean(off.acceptance_lengths):.2f} plain")


# ------------------------------------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("entry", ["batch", "stream"])
def test_a_slot_without_grammar_among_constrained_ones_keeps_its_argmax_draft(entry, monkeypatch, graphs):
    """The prompt without a grammar (and, in the second pass, without bans, in a decoder with a bias table) emits the
    ids at the acceptance lengths of a run without the switch, and its draft blocks are the same."""
    prompts = [_prompt(s, n) for s, n in PROMPTS3]
    for extra in (dict(grammar=[_chain(), None, _mixed()]),
                  dict(grammar=[_chain(), None, None], allowed_token_ids=[None, None, EVEN])):
        blocks = {True: [], False: []}
        outs = {}
        for on in (False, True):
            hooks = [None, lambda blk, start, call, on=on: blocks[on].append(blk[0].tolist()), None]
            hooks = [h or (lambda blk, start, call: None) for h in hooks]
            outs[on] = _many(entry, monkeypatch, prompts, hooks, n_new=50, slots=3, constrain_draft=on, **extra)
        assert _ids(outs[True][1]) == _ids(outs[False][1])
        assert list(outs[True][1].acceptance_lengths) == list(outs[False][1].acceptance_lengths)
        assert blocks[True] == blocks[False] and len(blocks[True]) >= 3
        assert _ids(outs[True][0]) == _ids(outs[False][0])
        assert np.mean(outs[True][0].acceptance_lengths) >= 4 * np.mean(outs[False][0].acceptance_lengths)


def test_engine_one_capture_serves_a_grammar_loaded_later(monkeypatch, graphs):
    """One slot, one capture: chain A is loaded before the first cycle, chain B (other tokens) after the engine has
    captured its cycle; the request under B runs in A's slot by replay and accepts every block."""
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    eng = BatchEngine(_draft_model(cfg), _native(), slots=1, max_rows=256, out_len=200, mask_token_id=cfg.mask_token_id,
                      grammar_states=2 * NS, constrain_draft=True)
    ha = eng.add_grammar(_chain())
    eng.submit(_prompt(3, 41), 60, grammar=ha)
    ra = eng.run()[0]
    assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] > 0
    replayed = eng.stats["replayed_cycles"]
    hb = eng.add_grammar(_chain(shift=11))
    eng.submit(_prompt(4, 37), 60, grammar=hb)
    rb = eng.run()[0]
    assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] > replayed
    assert _ids(ra)[41:] == _chain_ids(60) and _ids(rb)[37:] == _chain_ids(60, shift=11)
    for r in (ra, rb):
        _full_blocks(r.acceptance_lengths, (16,), 60)


# ------------------------------------------------------------------------------------------------------------ off, refusals
@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_constrain_draft_false_changes_nothing(entry, monkeypatch, graphs):
    """constrain_draft=False: the ids and acceptance lengths of the call without the keyword, and no pick launch."""
    from dflash_amd import ops
    calls = []
    real = ops.grammar_draft_rows
    monkeypatch.setattr(ops, "grammar_draft_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    g = _mixed()
    if entry in ("generate", "policy"):
        a = _single(entry, monkeypatch, n_new=60, grammar=g)
        b = _single(entry, monkeypatch, n_new=60, grammar=g, constrain_draft=False)
        pairs = [(a, b)]
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        pairs = list(zip(_many(entry, monkeypatch, prompts, n_new=50, grammar=g),
                         _many(entry, monkeypatch, prompts, n_new=50, grammar=g, constrain_draft=False)))
    for a, b in pairs:
        assert _ids(a) == _ids(b) and list(a.acceptance_lengths) == list(b.acceptance_lengths)
    assert not calls
    _single("generate", monkeypatch, n_new=8, grammar=g, constrain_draft=True)   # (the spy sees real launches)
    assert calls


def test_refusals(monkeypatch, graphs):
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.engine import BatchEngine
    g = _chain()
    cfg = H.tiny_cfg()
    prompts = [_prompt(s, n) for s, n in PROMPTS3]
    # nothing to constrain by: no grammar and no ban (finite biases alone do not ban)
    for kw in (dict(), dict(logit_bias={5: 2.0}), dict(grammar=None, banned_token_ids=[])):
        with pytest.raises(ValueError, match="constrain"):
            _single("generate", monkeypatch, n_new=8, constrain_draft=True, **kw)
    with pytest.raises(ValueError, match="constrain"):
        _single("policy", monkeypatch, n_new=8, constrain_draft=True)
    for entry in ("batch", "stream"):
        with pytest.raises(ValueError, match="constrain"):
            _many(entry, monkeypatch, prompts, n_new=8, constrain_draft=True)
    with pytest.raises(ValueError, match="constrain"):
        BatchedDecoder(_draft_model(cfg), _native(), 2, max_rows=128, out_len=100, mask_token_id=cfg.mask_token_id,
                       constrain_draft=True)
    with pytest.raises(ValueError, match="constrain"):
        BatchEngine(_draft_model(cfg), _native(), slots=2, max_rows=128, out_len=100, mask_token_id=cfg.mask_token_id,
                    constrain_draft=True)
    # a sampled draft
    with pytest.raises(NotImplementedError, match="greedy draft"):
        _single("policy", monkeypatch, temperature=T, seed=1, n_new=8, grammar=g, constrain_draft=True)
    with pytest.raises(NotImplementedError, match="greedy draft"):
        BatchedDecoder(_draft_model(cfg), _native(), 2, max_rows=128, out_len=100, mask_token_id=cfg.mask_token_id,
                       sampler="device", draft_temperature=T, grammar_states=NS, constrain_draft=True)
    # blocks of 17..32 rows: refused as the grammar and the bans refuse them
    with pytest.raises(NotImplementedError, match="16 rows"):
        _single("generate", monkeypatch, n_new=8, bs=24, grammar=g, constrain_draft=True)
    with pytest.raises(NotImplementedError, match="16 rows"):
        _single("generate", monkeypatch, n_new=8, bs=24, allowed_token_ids=EVEN, constrain_draft=True)
    with pytest.raises(NotImplementedError, match="16 rows"):
        BatchedDecoder(_draft_model(cfg), _native(), 1, max_rows=128, out_len=100, mask_token_id=cfg.mask_token_id,
                       tiles_per_request=2, logit_bias=True, constrain_draft=True)
    # a ban is enough
    r = _single("generate", monkeypatch, n_new=8, banned_token_ids=[7], constrain_draft=True)
    assert r.num_output_tokens == 8
