"""Grammar-constrained decoding through the decode loops: single request, policy, ragged batch,
slot-refill engine — on the tiny walk target of test_hip_logit_bias_loops.py (helpers copied, not imported): the lm_head
makes the target walk a permutation of 6-cycles with a logit of about 1.0 on the walk's token and near-zero noise
elsewhere.

The automaton is built from that permutation.  Its state is the last token emitted (2048 states, start = the prompt's
last token).  In a state v with v % mod == rem the walk's own token perm[v] is forbidden and only a fallback set of three
tokens is legal; in every other state perm[v] and the fallback set are legal.  So at T = 0 the run follows the walk until
it enters a restricted state, falls back to the best of the three and resumes from it; at T = 0.7 the draws move between
the walk and the fallback set all the time.

(a) the hard property: the emitted ids walk the automaton without an illegal step, and grammar_state is that walk's end.
(b) the teacher-forced audit of test_hip_logit_bias_loops.py: one HF forward over the emitted ids gives the raw logits
per position, grammar_ref.py the masked row, and every emitted token must be that row's argmax (T = 0) or its seeded draw
(T = 0.7) wherever the row is not a near-tie — the screens and caps of test_hip_penalties_loops.py."""
import numpy as np
import pytest
import torch

import grammar_ref as GR
import helpers as H
import logit_bias_ref as LB
import logprobs_ref as LR
import nucleus_ref as NR
import penalties_ref as PR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048
T = 0.7
N_IN, N_NEW = 41, 120
MASK = 2047
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
        _STATE["hf"], _STATE["perm"] = hf, perm.tolist()
    return _STATE["hf"], _STATE["perm"]


def _native():
    from dflash_amd import NativeTarget
    return NativeTarget(_walk_target()[0])


def _draft_model(cfg):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return m


def _plan():
    return H.make_plan(400, 16, 29)


def _put(blk, toks):
    toks = toks[:blk.shape[1] - 1]
    if toks:
        blk[0, 1:1 + len(toks)] = torch.tensor(toks, dtype=blk.dtype, device=blk.device)


def _walk_hook(perm, plan):
    """Drafts scripted from the RAW walk of the block's first token: plan[call] walk tokens, then a wrong one."""
    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        b, toks = int(blk[0, 0]), []
        for _ in range(k):
            b = perm[b]
            toks.append(b)
        if k + 1 < blk.shape[1]:
            toks.append((perm[b] + 1) % (V - 2))
        _put(blk, toks)
    return hook


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


# ------------------------------------------------------------------------------------------------------------ the grammar
FALLBACK = (100, 104, 107)       # none is 0 mod 3 or 1 mod 4: a fallback token never lands in a restricted state
RULES = ((3, 0), (4, 1))


def _table(mod, rem):
    """next int16 [V, V]: state = the last token; see the module docstring."""
    key = ("tab", mod, rem)
    if key not in _STATE:
        _, perm = _walk_target()
        nxt = np.full((V, V), -1, dtype=np.int16)
        for f in FALLBACK:
            nxt[:, f] = f
        for v in range(V - 2):
            if v % mod != rem:
                nxt[v, perm[v]] = perm[v]
        _STATE[key] = nxt
    return _STATE[key]


def _grammar(prompt, rule=0):
    from dflash_amd import TokenDFA
    return TokenDFA(_table(*RULES[rule]), start=int(prompt[0, -1]))


def _restricted(v, rule=0):
    mod, rem = RULES[rule]
    return v % mod == rem or v >= V - 2


def _walks(ids, n_in, g):
    """(a): the emitted ids walk the automaton from start; returns the states in front of every emitted token and the
    final state."""
    s, before = g.start, []
    for i, v in enumerate(ids[n_in:]):
        before.append(s)
        s = GR.step(g.next, 0, s, v)
        assert s >= 0, (i, v, before[-1])
    return before, s


def _hard(r, n_in, g, n_new=None):
    ids = _ids(r)
    if n_new is not None:
        assert len(ids) == n_in + n_new
    before, end = _walks(ids, n_in, g)
    assert r.grammar_state == end, (r.grammar_state, end)
    return before


def _tape_hook(tape, n_in, g, plan, seen):
    """Drafts scripted from a continuation `tape` (absolute position -> token, a grammar-constrained run): plan[call] of
    its tokens (legal and right), then a wrong one — on even calls an ILLEGAL token (the rows behind it are dead), on odd
    calls a LEGAL but wrong one, followed by legal tokens (the rows behind it are live, in states the tape never
    visits).  seen counts the three kinds."""
    def hook(blk, start, call):
        k = max(0, min(plan[call % len(plan)], blk.shape[1] - 1, len(tape) - start - 2))
        toks = list(tape[start + 1:start + 1 + k])
        seen["right"] += k
        room = blk.shape[1] - 1 - k
        if room > 0 and start + 1 + k < len(tape):
            state = tape[start + k]                                  # the state is the last token
            right = tape[start + 1 + k]
            if call % 2 == 0:
                bad = next(v for v in range(right + 1, right + 9) if g.next[state, v % (V - 2)] < 0) % (V - 2)
                toks.append(bad)
                seen["illegal"] += 1
            else:
                wrong = next(f for f in FALLBACK if f != right)
                toks += [wrong] + [FALLBACK[(call + j) % 3] for j in range(room - 1)]
                seen["legal_wrong"] += 1
        _put(blk, toks)
    return hook


# ------------------------------------------------------------------------------------------------------------ the model
def _raw_rows(ids, n_in):
    hf, _ = _walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    return PR.f32_to_bf16_bits(logits[n_in - 1:len(ids) - 1]).reshape(len(ids) - n_in, V)


def _bias_row(cfg):
    from dflash_amd import ops
    lb = ops.check_logit_bias(V, cfg.get("logit_bias"), None, cfg.get("banned_token_ids"), 0, None)
    return np.zeros(V, np.float32) if lb is None else lb[0].numpy()


def _audit(ids, n_in, g, temperature=0.0, seed=None, pen=None, cfg=None, top_p=1.0):
    """Every emitted token against the model's processed row for its prefix: the bias if `cfg`, the grammar mask by the
    state the emitted prefix reaches, then the penalties if `pen`.  T = 0: the argmax wherever the row's top-2 gap is
    >= 4 bf16 ulp (at least 90 % of the positions).  T = 0.7: the seeded draw wherever its perturbed gap exceeds 0.1 (at
    least 85 %).  Returns (emitted, screen, the model's tokens, raw rows, processed rows)."""
    x = _raw_rows(ids, n_in)
    before, _ = _walks(ids, n_in, g) if g is not None else ([-1] * (len(ids) - n_in), None)
    b = _bias_row(cfg) if cfg else None
    got = np.asarray(ids[n_in:])
    want, safe = np.zeros(len(got), dtype=np.int64), np.zeros(len(got), dtype=bool)
    zs = np.zeros_like(x)
    for i in range(len(got)):
        p = n_in + i
        z = x[i] if b is None else LB.process(x[i], b)
        z = GR.mask_row(z, g.next, 0, before[i]) if g is not None else z
        if pen is not None:
            z = PR.penalise(z, *PR.history(ids, n_in, p, V), *pen)
        zs[i] = z
        if temperature < 1e-5:
            want[i], safe[i] = GR.argmax_lowest(z), GR.bf16_ulp_gap(z) >= 4
        elif top_p < 1.0:
            zf = GR.bits_to_f32(z)
            thr = NR.thresholds(zf, temperature, 0, top_p)[2]
            lo, hi = NR.top_p_thresholds(zf, temperature, [top_p * (1 - 1e-3), top_p * (1 + 1e-3)], float(zf.min()))
            w, gap = NR.draw_over(zf[None], [thr], temperature, seed, SR.TARGET, [p])
            want[i], safe[i] = w[0], gap[0] > 0.1 and lo == hi    # (a nucleus whose edge moves with P (1 +- 1e-3): left out)
        else:
            w, gap = SR.draw(GR.bits_to_f32(z)[None], temperature, seed, SR.TARGET, [p])
            want[i], safe[i] = w[0], gap[0] > 0.1
    print(f"[grammar] audit of {len(got)} positions at T = {temperature}: screen keeps {safe.mean():.3f}")
    assert safe.mean() >= (0.9 if temperature < 1e-5 else 0.85), safe.mean()
    assert np.array_equal(got[safe], want[safe]), (np.nonzero(safe & (got != want))[0][:8], safe.mean())
    return got, safe, want, x, zs


def _spans(r, n_out):
    """Output-index ranges [lo, hi) each cycle committed: index 0 is the prefill's token, every cycle adds its
    acceptance length."""
    out, lo = [], 1
    for tau in r.acceptance_lengths:
        out.append((lo, min(lo + int(tau), n_out)))
        lo += int(tau)
    return out


def _same_until_a_near_tie(a, b):
    """Two audited runs of one request: a divergence may only start at a position either screen left out."""
    ga, sa, gb, sb = a[0], a[1], b[0], b[1]
    n = min(len(ga), len(gb))
    diff = np.nonzero(ga[:n] != gb[:n])[0]
    if diff.size:
        assert not (sa[diff[0]] and sb[diff[0]]), diff[0]


# ------------------------------------------------------------------------------------------------------------ the runs
@pytest.fixture
def graphs():
    """Sessions hold their hipGraphs: collect them with the test, so that no capture state outlives this file's tests."""
    import gc
    yield
    gc.collect()


def _single(kind, monkeypatch, hook, *, graph=True, stop=None, temperature=0.0, seed=None, n_new=N_NEW, prompt=None, bs=16,
            **kw):
    from dflash_amd import dflash_generate, dflash_generate_policy
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    cfg = H.tiny_cfg()
    prompt = _prompt() if prompt is None else prompt
    skw = dict(sampler="device", seed=seed) if temperature >= 1e-5 else {}
    if kind == "generate":
        r = dflash_generate(_draft_model(cfg), _native(), prompt, cfg.mask_token_id, n_new, bs, stop, temperature,
                            draft_token_hook=hook, **skw, **kw)
    else:
        r = dflash_generate_policy(model=_draft_model(cfg), target=_native(), input_ids=prompt,
                                   mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, stop_token_ids=stop,
                                   temperature=temperature, scheduler=_script(), draft_token_hook=hook, **skw, **kw)
    return r


def _many(entry, monkeypatch, prompts, hooks, *, temperature=0.0, seeds=None, n_new=80, graph=True, stop=None, slots=2, **kw):
    """dflash_generate_batch / dflash_generate_stream over `prompts`, hooks[i](blk, start, call) per prompt."""
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import dflash_generate_stream
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    cfg = H.tiny_cfg()
    fn = dflash_generate_batch if entry == "batch" else dflash_generate_stream
    extra = dict(slots=slots) if entry == "stream" else {}
    skw = dict(sampler="device", seed=seeds) if temperature >= 1e-5 else {}
    return fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, n_new, 16, stop, temperature,
              draft_token_hook=lambda i, blk, start, call: hooks[i](blk, start, call), **skw, **extra, **kw)


def _ids(r):
    return r.output_ids[0].tolist()


PROMPTS3 = ((3, 41), (4, 37), (5, 45))
# the seeds of the T = 0.7 runs: chosen, on the reference alone (grammar_ref.decode_alone over the target's rows under
# these grammars), among those whose draws leave the 0.1 screen a margin above its 0.85 cap and enter a restricted state
# often: 0.93 with 20 forced positions of 120 (SEED), 0.96 / 16 and 0.96 / 10 of 80 (SEEDS3, the third prompt has no
# grammar).  At T = 0 the reference's screen keeps every position (58 forced of 120, 16 of 80).
SEED, SEEDS3 = 13, [32, 35, 34]


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("temperature", [0.0, T])
@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_grammar_through_the_loops(entry, temperature, monkeypatch, graphs):
    """Three passes per entry: drafts from the raw walk, eager (its output is a constrained continuation, the tape), then
    drafts scripted from that tape — legal and right, legal but wrong, illegal — eager and replayed.  The batch entries
    run three prompts: two different grammars and one prompt without (two slots in the engine: the third is admitted
    into a finished slot).  Every run has the hard property (a) and passes the audit (b); eager and replayed emit the
    same ids (f); accepted spans cross restricted states and all three kinds of draft occur (c)."""
    _, perm = _walk_target()
    plan = _plan()
    seen = dict(right=0, illegal=0, legal_wrong=0)
    if entry in ("generate", "policy"):
        g = _grammar(_prompt())
        seed = SEED if temperature >= 1e-5 else None
        kw = dict(temperature=temperature, seed=seed, grammar=g)
        a = _single(entry, monkeypatch, _walk_hook(perm, plan), graph=False, **kw)
        b = _single(entry, monkeypatch, _tape_hook(_ids(a), N_IN, g, plan, seen), graph=False, **kw)
        c = _single(entry, monkeypatch, _tape_hook(_ids(a), N_IN, g, plan, seen), graph=True, **kw)
        assert c.replayed_cycles > 0 and b.replayed_cycles == 0
        runs = [(N_IN, seed, g, 0, a, b, c)]
        n_new = N_NEW
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        gs = [_grammar(prompts[0], 0), _grammar(prompts[1], 1), None]
        seeds = SEEDS3 if temperature >= 1e-5 else None
        kw = dict(temperature=temperature, seeds=seeds, grammar=gs)
        n_new = 80

        def tape_hooks(runs_a):
            return [_tape_hook(_ids(r), p.shape[1], gs[i], plan, seen) if gs[i] is not None else _walk_hook(perm, plan)
                    for i, (r, p) in enumerate(zip(runs_a, prompts))]

        a = _many(entry, monkeypatch, prompts, [_walk_hook(perm, plan)] * 3, graph=False, **kw)
        b = _many(entry, monkeypatch, prompts, tape_hooks(a), graph=False, **kw)
        c = _many(entry, monkeypatch, prompts, tape_hooks(a), graph=True, **kw)
        runs = [(p.shape[1], seeds[i] if seeds else None, gs[i], i, a[i], b[i], c[i]) for i, p in enumerate(prompts)]
    crossed = 0
    for n_in, seed, g, rule, ra, rb, rc in runs:
        assert _ids(rc) == _ids(rb) and list(rc.acceptance_lengths) == list(rb.acceptance_lengths)       # (f)
        if g is None:
            assert ra.grammar_state is None and rb.grammar_state is None and rc.grammar_state is None
            continue                                  # (its ids: test_a_slot_without_grammar_among_constrained_ones)
        for r in (ra, rb, rc):
            before = _hard(r, n_in, g, n_new)                                                             # (a)
        ua = _audit(_ids(ra), n_in, g, temperature, seed)                                                 # (b)
        ub = _audit(_ids(rb), n_in, g, temperature, seed)
        _same_until_a_near_tie(ua, ub)
        forced = np.array([i for i, s in enumerate(before) if _restricted(s, rule)])
        assert len(forced) >= 4, len(forced)                          # the grammar bites: states where the walk's token is forbidden
        assert all(_ids(rb)[n_in + i] in FALLBACK for i in forced)
        crossed += len([s for s in _spans(rb, n_new) if s[1] - s[0] >= 2 and ((forced >= s[0]) & (forced < s[1])).any()])
        print(f"[grammar] {entry} T={temperature}: {len(forced)} forced positions, mean tau "
              f"{np.mean(rb.acceptance_lengths):.2f}, screen keeps {ub[1].mean():.3f}")
    print(f"[grammar] {entry} T={temperature}: drafts {seen}, {crossed} accepted spans of >= 2 tokens hold a forced position")
    assert crossed >= 3 and seen["illegal"] >= 4 and seen["legal_wrong"] >= 4 and seen["right"] >= 40   # (c)


def test_the_target_alone_under_the_grammar(monkeypatch, graphs):
    """grammar_ref.decode_alone — the target one token at a time, each row masked by the state so far — against the
    speculative run at T = 0: the same ids up to the first near-tie of either."""
    hf, perm = _walk_target()
    prompt = _prompt()
    g = _grammar(prompt)
    n_new = 48

    def last_row(ids):
        with torch.inference_mode():
            row = hf(torch.tensor([ids], device=dev())).logits[0, -1].float().cpu().numpy()
        return PR.f32_to_bf16_bits(row).reshape(V)

    alone, end = GR.decode_alone(last_row, g.next, 0, g.start, prompt[0].tolist(), n_new)
    r = _single("generate", monkeypatch, _walk_hook(perm, _plan()), n_new=n_new, grammar=g)
    _hard(r, N_IN, g, n_new)
    ua, ur = _audit(alone, N_IN, g), _audit(_ids(r), N_IN, g)
    _same_until_a_near_tie(ua, ur)
    if alone == _ids(r):
        assert r.grammar_state == end


def test_composed_with_bias_penalties_top_p_and_logprobs(monkeypatch, graphs):
    """grammar + logit_bias + penalties + logprobs = 2 at T = 0, and the same with top_p = 0.9 at T = 0.7: the audit
    applies the bias, the grammar mask, the penalties, in that order (and the nucleus at T = 0.7); the hard property
    holds; the logprobs are log_softmax of the RAW teacher-forced rows; eager and replayed emit the same ids."""
    _, perm = _walk_target()
    plan = _plan()
    g = _grammar(_prompt())
    # (biases that keep the three fallback tokens several times the noise apart, seen or unseen, under these penalties: on
    # the reference alone the T = 0 screen keeps 0.99 of 80 positions, the T = 0.7 one 0.95, and the penalties move 63)
    cfg = dict(logit_bias={FALLBACK[0]: 0.5, FALLBACK[1]: 0.8, FALLBACK[2]: 1.3}, banned_token_ids=[MASK, 5])
    PEN = (1.5, 0.3, 0.05)
    pk = dict(repetition_penalty=PEN[0], presence_penalty=PEN[1], frequency_penalty=PEN[2])
    for temperature, extra in ((0.0, {}), (T, dict(top_p=0.9))):
        seed = SEED if temperature >= 1e-5 else None
        seen = dict(right=0, illegal=0, legal_wrong=0)
        kw = dict(temperature=temperature, seed=seed, grammar=g, logprobs=2, n_new=80, **cfg, **pk, **extra)
        a = _single("generate", monkeypatch, _walk_hook(perm, plan), graph=False, **kw)
        b = _single("generate", monkeypatch, _tape_hook(_ids(a), N_IN, g, plan, seen), graph=False, **kw)
        c = _single("generate", monkeypatch, _tape_hook(_ids(a), N_IN, g, plan, seen), graph=True, **kw)
        assert c.replayed_cycles > 0 and _ids(c) == _ids(b)
        for r in (a, b, c):
            _hard(r, N_IN, g, 80)
            assert not {MASK, 5} & set(_ids(r)[N_IN:])
        u = _audit(_ids(b), N_IN, g, temperature, seed, pen=PEN, cfg=cfg, top_p=extra.get("top_p", 1.0))
        x = GR.bits_to_f32(u[3])
        lp = c.logprobs.cpu().numpy()
        for i in range(80):
            assert abs(lp[i] - LR.logprob(x[i], _ids(c)[N_IN + i])) <= 0.05, i
        if temperature < 1e-5:   # the penalties bite on top of bias and grammar
            plain = [GR.argmax_lowest(GR.mask_row(LB.process(u[3][i], _bias_row(cfg)), g.next, 0, s))
                     for i, s in enumerate(_walks(_ids(b), N_IN, g)[0])]
            assert (np.array(plain) != u[2]).sum() >= 3


@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_grammar_none_changes_nothing(entry, monkeypatch, graphs):
    """(e) grammar=None: the ids and acceptance lengths of the call without the keyword, and no grammar launch."""
    from dflash_amd import ops
    calls = []
    for name in ("grammar_rows", "grammar_advance"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
    _, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    if entry in ("generate", "policy"):
        for kw in (dict(), dict(temperature=T, seed=3)):
            a = _single(entry, monkeypatch, hook, n_new=60, **kw)
            b = _single(entry, monkeypatch, hook, n_new=60, grammar=None, **kw)
            assert np.array_equal(_ids(a), _ids(b)) and list(a.acceptance_lengths) == list(b.acceptance_lengths)
            assert b.grammar_state is None
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        a = _many(entry, monkeypatch, prompts, [hook] * 3, n_new=50)
        for gr in (None, [None, None, None]):
            b = _many(entry, monkeypatch, prompts, [hook] * 3, n_new=50, grammar=gr)
            for x, y in zip(a, b):
                assert np.array_equal(_ids(x), _ids(y)) and list(x.acceptance_lengths) == list(y.acceptance_lengths)
                assert y.grammar_state is None
    assert not calls
    _single("generate", monkeypatch, hook, n_new=8, grammar=_grammar(_prompt()))  # (the spy sees real launches)
    assert calls


@pytest.mark.parametrize("entry", ["batch", "stream"])
def test_a_slot_without_grammar_among_constrained_ones(entry, monkeypatch, graphs):
    """The prompt without a grammar in a decoder built with a pool emits the ids of a decoder built without one."""
    _, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    prompts = [_prompt(s, n) for s, n in PROMPTS3]
    plain = _many(entry, monkeypatch, prompts, [hook] * 3, n_new=50, slots=3)
    gs = [_grammar(prompts[0], 0), None, _grammar(prompts[2], 1)]
    out = _many(entry, monkeypatch, prompts, [hook] * 3, n_new=50, slots=3, grammar=gs)
    assert _ids(out[1]) == _ids(plain[1]) and list(out[1].acceptance_lengths) == list(plain[1].acceptance_lengths)
    assert out[1].grammar_state is None
    for i in (0, 2):
        _hard(out[i], prompts[i].shape[1], gs[i], 50)
        assert _ids(out[i]) != _ids(plain[i])


def test_engine_one_capture_serves_grammars_loaded_later(monkeypatch, graphs):
    """One slot, two requests, one capture: grammar A is loaded before the first cycle, grammar B after the engine has
    captured its cycle; request 2 runs in request 1's slot under B, and a third without a grammar gives the ids of a
    fresh engine.  The pool refuses a grammar it has no rows for."""
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    _, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    pa, pb = _prompt(3, 41), _prompt(4, 37)
    ga, gb = _grammar(pa, 0), _grammar(pb, 1)

    def engine(states):
        return BatchEngine(_draft_model(cfg), _native(), slots=1, max_rows=256, out_len=200,
                           mask_token_id=cfg.mask_token_id, grammar_states=states)

    fresh = engine(0)
    fresh.submit(pb, 40, draft_token_hook=hook)
    fresh = fresh.run()[0]
    eng = engine(2 * V)
    ptr = eng.dec.grammar.table.data_ptr()
    ha = eng.add_grammar(ga)
    eng.submit(pa, 40, draft_token_hook=hook, grammar=ha)
    ra = eng.run()[0]
    assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] > 0
    hb = eng.add_grammar(gb)
    with pytest.raises(ValueError, match="pool is full"):
        eng.add_grammar(ga)
    eng.submit(pb, 40, draft_token_hook=hook, grammar=hb)
    eng.submit(pb, 40, draft_token_hook=hook)
    rb, rn = eng.run()
    assert eng.stats["captures"] == 1 and eng.dec.grammar.table.data_ptr() == ptr
    _hard(ra, 41, ga, 40)
    _hard(rb, 37, gb, 40)
    _audit(_ids(rb), 37, gb)
    assert rn.grammar_state is None and _ids(rn) == _ids(fresh)
    with pytest.raises(ValueError, match="grammar_states > 0"):
        engine(0).submit(pa, 8, grammar=0)


def test_refusals(monkeypatch, graphs):
    from dflash_amd import dflash_generate, ops
    cfg = H.tiny_cfg()
    nt = _native()
    g = _grammar(_prompt())
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(_draft_model(cfg), _walk_target()[0], _prompt(), cfg.mask_token_id, 8, 16, None, grammar=g)
    with pytest.raises(ValueError, match="sampler='device'"):
        dflash_generate(_draft_model(cfg), nt, _prompt(), cfg.mask_token_id, 8, 16, None, T, grammar=g)
    with pytest.raises(NotImplementedError, match="16 rows"):
        _single("generate", monkeypatch, None, n_new=8, bs=24, grammar=g)
    # a reachable state whose legal tokens the request's own bias bans all
    with pytest.raises(ValueError, match="banned"):
        _single("generate", monkeypatch, None, n_new=8, grammar=g, banned_token_ids=list(FALLBACK))
    cache = nt.new_cache(128)
    nt.prefill(_prompt(), cache)
    state = ops.grammar_state(1, V, V, dev())
    state.logits = torch.zeros(16, V, dtype=BF16, device=dev())
    with pytest.raises(NotImplementedError, match="16 rows"):
        nt.verify(torch.zeros(24, dtype=torch.long, device=dev()), N_IN, cache, grammar=state)
    with pytest.raises(ValueError, match="seed"):
        nt.verify(torch.zeros(8, dtype=torch.long, device=dev()), N_IN, cache, temperature=T, grammar=state)
