"""Logit bias, allow / ban lists and min_tokens through the decode loops: single request, policy,
ragged batch, slot-refill engine — on the tiny walk target of test_hip_penalties_loops.py (helpers copied, not imported):
the lm_head makes the target walk a permutation of 6-cycles with a logit of about 1.0 on the walk's token and near-zero
noise elsewhere.  Bans and negative biases on walk tokens push the continuation off the walk; a small fallback set with
distinct positive biases (0.40 / 0.55 / 0.70: steps of several times the noise) then wins by far more than 4 bf16 ulp
and the walk resumes from it.

Truth is teacher-forced: one HF forward over the emitted ids gives the raw logits per position, logit_bias_ref.py the
processed row (then penalties_ref.py the penalised one), and every emitted token must be that row's argmax (T = 0) or
its seeded draw (T = 0.7) wherever the row is not a near-tie — the screens and caps of test_hip_penalties_loops.py."""
import numpy as np
import pytest
import torch

import helpers as H
import logit_bias_ref as LB
import logprobs_ref as LR
import penalties_ref as PR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048
T = 0.7
PEN = (1.3, 0.2, 0.25)
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


def _tape_hook(tape, plan):
    """Drafts scripted from a continuation `tape` (absolute position -> token, the processed reference run): plan[call]
    of its tokens, then a wrong one — accepted spans run across the positions where the processing changes the token."""
    def hook(blk, start, call):
        k = max(0, min(plan[call % len(plan)], blk.shape[1] - 1, len(tape) - start - 2))
        toks = list(tape[start + 1:start + 1 + k])
        if k + 1 < blk.shape[1] and start + 1 + k < len(tape):
            toks.append((tape[start + 1 + k] + 1) % (V - 2))
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


# ------------------------------------------------------------------------------------------------------------ the inputs
def _cycle(t):
    """The 6-cycle of the walk from token t: t, perm[t], ..."""
    _, perm = _walk_target()
    out = [t]
    for _ in range(5):
        out.append(perm[out[-1]])
    return out


def _fallback():
    """Three fallback tokens whose 6-cycles are disjoint from one another and from the cycles the test prompts walk."""
    if "fb" not in _STATE:
        lasts = [int(_prompt(s, n)[0, -1]) for s, n in PROMPTS3]
        prot = set()
        for t in lasts:
            prot |= set(_cycle(t))
        fb = []
        for t in range(100, 1900):
            c = set(_cycle(t))
            if not c & prot:
                fb.append(t)
                prot |= c
            if len(fb) == 3:
                break
        _STATE["fb"], _STATE["lasts"], _STATE["prot"] = fb, lasts, prot
    return _STATE["fb"]


def _config():
    """The raw walk of a prompt repeats one 6-cycle, so the configuration is aimed at it: the third token of every
    prompt's continuation is banned (or biased by -2.0), the row falls back to the winner of the fallback set, the walk
    resumes from it, and the third step of the winner's own cycle is banned again — every third position leaves the raw
    argmax.  For the draws at T = 0.7 every third id outside those cycles is banned too, and the mask id."""
    fb = _fallback()
    lasts, prot = _STATE["lasts"], _STATE["prot"]
    bias = {fb[0]: 0.40, fb[1]: 0.55, fb[2]: 0.70}
    banned = [v for v in range(0, V - 2, 3) if v not in prot] + [MASK]
    for k, t in enumerate(lasts):
        c = _cycle(t)[3]                   # output index 2 of that prompt's raw continuation
        if k % 2 == 0:
            banned.append(c)
        else:
            bias[c] = -2.0
    banned.append(_cycle(fb[2])[3])
    bias[_cycle(fb[1])[3]] = -2.0
    return dict(logit_bias=bias, banned_token_ids=banned)


def _fallback_only():
    fb = _fallback()
    return dict(logit_bias={fb[0]: 0.40, fb[1]: 0.55, fb[2]: 0.70}, banned_token_ids=[MASK])


# ------------------------------------------------------------------------------------------------------------ the model
def _raw_rows(ids, n_in):
    hf, _ = _walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    return PR.f32_to_bf16_bits(logits[n_in - 1:len(ids) - 1]).reshape(len(ids) - n_in, V)


def _table(cfg, stop=None):
    """(b fp32 [V], min_tokens) of a configuration, (zeros, 0) when it is neutral."""
    from dflash_amd import ops
    lb = ops.check_logit_bias(V, cfg.get("logit_bias"), cfg.get("allowed_token_ids"), cfg.get("banned_token_ids"),
                              cfg.get("min_tokens", 0), stop)
    return (np.zeros(V, np.float32), 0) if lb is None else (lb[0].numpy(), lb[1])


def _audit(ids, n_in, cfg, temperature=0.0, seed=None, stop=None, pen=None):
    """Every emitted token against the model's processed row for its prefix: bias / bans / allow list / min_tokens, then
    the penalties if `pen`.  T = 0: the argmax wherever the row's top-2 gap is >= 4 bf16 ulp (at least 90 % of the
    positions).  T = 0.7: the seeded draw wherever its perturbed gap exceeds 0.1 (at least 85 %).  Returns (emitted,
    screen, the model's tokens, raw rows, processed rows)."""
    x = _raw_rows(ids, n_in)
    b, mt = _table(cfg, stop)
    min_pos = n_in + mt if mt else 0
    got = np.asarray(ids[n_in:])
    want, safe = np.zeros(len(got), dtype=np.int64), np.zeros(len(got), dtype=bool)
    zs = np.zeros_like(x)
    for i in range(len(got)):
        p = n_in + i
        z = LB.process(x[i], b, p, min_pos, stop or ())
        if pen is not None:
            z = PR.penalise(z, *PR.history(ids, n_in, p, V), *pen)
        zs[i] = z
        if temperature < 1e-5:
            want[i], safe[i] = LB.argmax_lowest(z), LB.bf16_ulp_gap(z) >= 4
        else:
            w, g = SR.draw(LB.bits_to_f32(z)[None], temperature, seed, SR.TARGET, [p])
            want[i], safe[i] = w[0], g[0] > 0.1
    print(f"[logit_bias] audit of {len(got)} positions at T = {temperature}: screen keeps {safe.mean():.3f}")
    assert safe.mean() >= (0.9 if temperature < 1e-5 else 0.85), safe.mean()
    assert np.array_equal(got[safe], want[safe]), (np.nonzero(safe & (got != want))[0][:8], safe.mean())
    return got, safe, want, x, zs


def _moved(u, n_in, temperature=0.0, seed=None):
    """On the reference alone: output indices where the processed row's token (argmax / draw) leaves the raw row's."""
    _, _, want, x, _ = u
    if temperature < 1e-5:
        raw = np.array([LB.argmax_lowest(x[i]) for i in range(len(x))])
    else:
        raw, _ = SR.draw(LB.bits_to_f32(x), temperature, seed, SR.TARGET, np.arange(n_in, n_in + len(x)))
    return np.nonzero(raw != want)[0]


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
    sampled = any(t >= 1e-5 for t in temperature) if isinstance(temperature, list) else temperature >= 1e-5
    skw = dict(sampler="device", seed=seeds) if sampled else {}
    return fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, n_new, 16, stop, temperature,
              draft_token_hook=lambda i, blk, start, call: hooks[i](blk, start, call), **skw, **extra, **kw)


def _ids(r):
    return r.output_ids[0].tolist()


PROMPTS3 = ((3, 41), (4, 37), (5, 45))
# the seeds of the T = 0.7 runs: chosen, on the reference rows alone, among those whose draws leave the 0.1 screen a
# margin above its cap (0.94 - 0.96 here; about one seed in ten lands at or under 0.85 by chance)
SEED, SEEDS3 = 10, [32, 33, 34]


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("temperature", [0.0, T])
@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_teacher_forced_audit(entry, temperature, monkeypatch, graphs):
    """Three passes per entry: drafts from the raw walk, eager (its output is the processed continuation, the tape), then
    drafts scripted from that tape, eager and replayed, so that accepted spans cross the positions the processing
    changes.  All pass the audit and agree up to near-ties; eager and replayed emit the same ids."""
    _, perm = _walk_target()
    plan, cfg = _plan(), _config()
    if entry in ("generate", "policy"):
        seed = SEED if temperature >= 1e-5 else None
        kw = dict(temperature=temperature, seed=seed, **cfg)
        a = _single(entry, monkeypatch, _walk_hook(perm, plan), graph=False, **kw)
        b = _single(entry, monkeypatch, _tape_hook(_ids(a), plan), graph=False, **kw)
        c = _single(entry, monkeypatch, _tape_hook(_ids(a), plan), graph=True, **kw)
        assert c.replayed_cycles > 0 and b.replayed_cycles == 0
        runs = [(N_IN, seed, a, b, c)]
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        seeds = SEEDS3 if temperature >= 1e-5 else None
        kw = dict(temperature=temperature, seeds=seeds, **cfg)
        a = _many(entry, monkeypatch, prompts, [_walk_hook(perm, plan)] * 3, graph=False, **kw)
        b = _many(entry, monkeypatch, prompts, [_tape_hook(_ids(r), plan) for r in a], graph=False, **kw)
        c = _many(entry, monkeypatch, prompts, [_tape_hook(_ids(r), plan) for r in a], graph=True, **kw)
        runs = [(p.shape[1], seeds[i] if seeds else None, a[i], b[i], c[i]) for i, p in enumerate(prompts)]
    banned = set(cfg["banned_token_ids"])
    for n_in, seed, ra, rb, rc in runs:
        n_new = N_NEW if entry in ("generate", "policy") else 80
        assert len(_ids(ra)) == len(_ids(rb)) == n_in + n_new
        assert _ids(rc) == _ids(rb) and list(rc.acceptance_lengths) == list(rb.acceptance_lengths)
        assert not banned & set(_ids(rb)[n_in:])
        ua = _audit(_ids(ra), n_in, cfg, temperature, seed)
        ub = _audit(_ids(rb), n_in, cfg, temperature, seed)
        _same_until_a_near_tie(ua, ub)
        moved = _moved(ub, n_in, temperature, seed)
        crossed = [s for s in _spans(rb, n_new) if s[1] - s[0] >= 2 and ((moved >= s[0]) & (moved < s[1])).any()]
        print(f"[logit_bias] {entry} T={temperature}: {len(moved)} positions leave the raw token, {len(crossed)} accepted "
              f"spans of >= 2 tokens hold one, screen keeps {ub[1].mean():.3f}, mean tau {np.mean(rb.acceptance_lengths):.2f}")
        assert len(moved) >= 10 and len(crossed) >= 3


@pytest.mark.parametrize("entry,temperature", [("generate", 0.0), ("policy", T), ("batch", T), ("stream", 0.0)])
def test_allowed_token_ids(entry, temperature, monkeypatch, graphs):
    """An allow list of some 55 ids (the fallback set with its biases and its next two walk steps among them): every
    emitted id is in the set, and the audit passes."""
    _, perm = _walk_target()
    plan, fb = _plan(), _fallback()
    allowed = sorted(set(range(40, 2000, 43)) | set(fb) | {perm[f] for f in fb} | {perm[perm[f]] for f in fb})
    cfg = dict(allowed_token_ids=allowed, logit_bias={fb[0]: 0.40, fb[1]: 0.55, fb[2]: 0.70})
    seed = SEED if temperature >= 1e-5 else None
    if entry in ("generate", "policy"):
        a = _single(entry, monkeypatch, _walk_hook(perm, plan), temperature=temperature, seed=seed, n_new=60, **cfg)
        b = _single(entry, monkeypatch, _tape_hook(_ids(a), plan), temperature=temperature, seed=seed, n_new=60, **cfg)
        runs = [(N_IN, seed, a, b)]
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        seeds = SEEDS3 if temperature >= 1e-5 else None
        a = _many(entry, monkeypatch, prompts, [_walk_hook(perm, plan)] * 3, temperature=temperature, seeds=seeds, n_new=60, **cfg)
        b = _many(entry, monkeypatch, prompts, [_tape_hook(_ids(r), plan) for r in a], temperature=temperature, seeds=seeds,
                  n_new=60, **cfg)
        runs = [(p.shape[1], seeds[i] if seeds else None, a[i], b[i]) for i, p in enumerate(prompts)]
    for n_in, sd, ra, rb in runs:
        for r in (ra, rb):
            assert len(_ids(r)) == n_in + 60 and set(_ids(r)[n_in:]) <= set(allowed)
        _same_until_a_near_tie(_audit(_ids(ra), n_in, cfg, temperature, sd), _audit(_ids(rb), n_in, cfg, temperature, sd))
        assert max(rb.acceptance_lengths) > 2


@pytest.mark.parametrize("mt", [12, 13])
@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_min_tokens(entry, mt, monkeypatch, graphs):
    """The stop ids: the token the unconstrained run emits at output index 3 — that run ends after 4 tokens — and the
    second walk step behind the fallback winner.  With min_tokens = 12 the suppressed positions fall back to that winner,
    the walk resumes from it and runs into the second stop id every other step: suppressed at the output indices < 12,
    emitted at index 13, where the run ends.  The cycle that commits index 12 holds indices 11 (suppressed) and 12 (free)
    in one accepted block.  min_tokens = 13 gives the same ids from the other side: index 12 is the last suppressed one
    and the stop id comes out at the first free index — a position rule that is off by one either way changes one of
    the two runs."""
    _, perm = _walk_target()
    fb = _fallback()
    cfg = _fallback_only()
    plan = [3, 15, 15, 15]
    prompt = _prompt()

    def run(hook, stop, graph=True, **kw):
        if entry in ("generate", "policy"):
            return _single(entry, monkeypatch, hook, stop=stop, graph=graph, n_new=40, prompt=prompt, **cfg, **kw)
        return _many(entry, monkeypatch, [prompt], [hook], stop=stop, graph=graph, n_new=40, slots=1, **cfg, **kw)[0]

    free = run(_walk_hook(perm, plan), None)
    s1 = _ids(free)[N_IN + 3]
    s2 = perm[perm[fb[2]]]
    stop = [s1, s2]
    assert s2 not in _ids(free)[N_IN:N_IN + 4] and s1 != s2
    short = run(_walk_hook(perm, plan), stop)
    assert _ids(short) == _ids(free)[:N_IN + 4]                                    # without min_tokens: 4 tokens
    a = run(_walk_hook(perm, plan), stop, graph=False, min_tokens=mt)
    b = run(_tape_hook(_ids(a), plan), stop, graph=False, min_tokens=mt)
    c = run(_tape_hook(_ids(a), plan), stop, graph=True, min_tokens=mt)
    for r in (a, b, c):
        new = _ids(r)[N_IN:]
        assert len(new) >= mt and not set(stop) & set(new[:mt])
        hits = [i for i, v in enumerate(new) if v in stop]
        assert hits == [len(new) - 1] and hits[0] >= mt                            # ends at the first stop id after that
        _audit(_ids(r), N_IN, dict(cfg, min_tokens=mt), stop=stop)
    assert _ids(a) == _ids(b) == _ids(c) and list(b.acceptance_lengths) == list(c.acceptance_lengths)
    new = _ids(b)[N_IN:]
    assert new[3] == fb[2] and new[11] == fb[2] and len(new) == 14                 # the suppressed rows fall back
    inside = [s for s in _spans(b, len(new)) if s[0] <= 11 and s[1] >= 13]        # indices 11 and 12 from one block's rows
    assert inside or mt != 12, _spans(b, len(new))


@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_neutral_values_change_nothing(entry, monkeypatch, graphs):
    """Empty / zero / absent values: the ids and acceptance lengths of the run without the keywords, and no
    logit_bias_rows launch."""
    from dflash_amd import ops
    calls = []
    real = ops.logit_bias_rows
    monkeypatch.setattr(ops, "logit_bias_rows", lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
    _, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    neutral = dict(logit_bias={5: 0.0, 9: -0.0}, allowed_token_ids=None, banned_token_ids=[], min_tokens=7)   # no stop ids
    if entry in ("generate", "policy"):
        for kw in (dict(), dict(temperature=T, seed=3)):
            a = _single(entry, monkeypatch, hook, n_new=60, **kw)
            b = _single(entry, monkeypatch, hook, n_new=60, **kw, **neutral)
            assert _ids(a) == _ids(b) and list(a.acceptance_lengths) == list(b.acceptance_lengths)
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        a = _many(entry, monkeypatch, prompts, [hook] * 3, n_new=50)
        b = _many(entry, monkeypatch, prompts, [hook] * 3, n_new=50, **neutral)
        for x, y in zip(a, b):
            assert _ids(x) == _ids(y) and list(x.acceptance_lengths) == list(y.acceptance_lengths)
    assert not calls
    _single("generate", monkeypatch, hook, n_new=8, **_fallback_only())            # (the spy sees a real launch)
    assert calls


@pytest.mark.parametrize("entry", ["batch", "stream"])
def test_mixed_slots(entry, monkeypatch, graphs):
    """Three requests in one ragged group: one biased and banned, one neutral, one with min_tokens.  Each passes its own
    audit; the neutral slot gives the ids of a decoder built without the flag."""
    _, perm = _walk_target()
    plan = _plan()
    prompts = [_prompt(s, n) for s, n in PROMPTS3]
    hooks = [_walk_hook(perm, plan)] * 3
    plain = _many(entry, monkeypatch, prompts, hooks, n_new=60, slots=3)
    stop = [_ids(plain[2])[45 + 3]]
    plain = _many(entry, monkeypatch, prompts, hooks, n_new=60, stop=stop, slots=3)
    assert len(_ids(plain[2])) == 45 + 4
    cfgs = [_config(), {}, dict(_fallback_only(), min_tokens=12)]
    kw = dict(logit_bias=[c.get("logit_bias") for c in cfgs], banned_token_ids=[c.get("banned_token_ids") for c in cfgs],
              min_tokens=[c.get("min_tokens", 0) for c in cfgs])
    a = _many(entry, monkeypatch, prompts, hooks, n_new=60, stop=stop, slots=3, **kw)
    b = _many(entry, monkeypatch, prompts, [_tape_hook(_ids(r), plan) for r in a], n_new=60, stop=stop, slots=3, **kw)
    for i, p in enumerate(prompts):
        n_in = p.shape[1]
        ua = _audit(_ids(a[i]), n_in, cfgs[i], stop=stop)
        ub = _audit(_ids(b[i]), n_in, cfgs[i], stop=stop)
        _same_until_a_near_tie(ua, ub)
    assert _ids(a[1]) == _ids(plain[1]) and list(a[1].acceptance_lengths) == list(plain[1].acceptance_lengths)
    new = _ids(b[2])[45:]
    assert len(new) >= 12 and stop[0] not in new[:12]
    assert len(_moved(_audit(_ids(b[0]), 41, cfgs[0], stop=stop), 41)) >= 5


def test_engine_slot_reuse_starts_from_a_clean_row(monkeypatch, graphs):
    """One slot, two requests: A bans every token B's own run emits (and has the fallback set), B runs afterwards in A's
    slot with neutral values.  B's ids equal those of a fresh engine built without the flag; A never emits a banned id."""
    _, perm = _walk_target()
    plan = _plan()
    pa, pb = _prompt(3, 41), _prompt(4, 37)
    hook = _walk_hook(perm, plan)
    fresh = _many("stream", monkeypatch, [pb], [hook], n_new=40, slots=1)[0]
    b_new = sorted(set(_ids(fresh)[37:]) - set(_fallback()))
    assert len(b_new) >= 6
    cfg_a = dict(_fallback_only())
    cfg_a["banned_token_ids"] = b_new + [MASK]
    out = _many("stream", monkeypatch, [pa, pb], [hook, hook], n_new=40, slots=1,
                logit_bias=[cfg_a["logit_bias"], None], banned_token_ids=[cfg_a["banned_token_ids"], None])
    assert out[0].slot == out[1].slot == 0
    assert _ids(out[1]) == _ids(fresh) and list(out[1].acceptance_lengths) == list(fresh.acceptance_lengths)
    assert not set(cfg_a["banned_token_ids"]) & set(_ids(out[0])[41:])
    _audit(_ids(out[0]), 41, cfg_a)


def test_with_penalties_and_logprobs(monkeypatch, graphs):
    """logit bias + penalties + logprobs = 2: the audit applies the bias, then the penalties, in that order; the
    logprobs are log_softmax of the RAW teacher-forced rows, and the most likely token is the raw argmax even where the
    run emitted another one."""
    _, perm = _walk_target()
    plan, cfg = _plan(), _config()
    pk = dict(repetition_penalty=PEN[0], presence_penalty=PEN[1], frequency_penalty=PEN[2])
    tape = _ids(_single("generate", monkeypatch, _walk_hook(perm, plan), **cfg, **pk))
    r = _single("generate", monkeypatch, _tape_hook(tape, plan), logprobs=2, **cfg, **pk)
    ids = _ids(r)
    assert r.replayed_cycles > 0 and max(r.acceptance_lengths) > 4
    u = _audit(ids, N_IN, cfg, pen=PEN)
    # the order matters on these rows: penalties first, bias second gives other tokens somewhere
    b, _ = _table(cfg)
    swapped = [LB.argmax_lowest(LB.process(PR.penalise(u[3][i], *PR.history(ids, N_IN, N_IN + i, V), *PEN), b))
               for i in range(len(u[2]))]
    bias_only = [LB.argmax_lowest(LB.process(u[3][i], b)) for i in range(len(u[2]))]
    assert (np.array(bias_only) != u[2]).sum() >= 5                                # the penalties bite on top of the bias
    print(f"[logit_bias] with penalties: {(np.array(swapped) != u[2]).sum()} positions depend on the order, "
          f"{(np.array(bias_only) != u[2]).sum()} on the penalties")
    x = LB.bits_to_f32(u[3])
    lp, top = r.logprobs.cpu().numpy(), r.top_logprob_ids.cpu().numpy()
    moved = 0
    for i in range(len(ids) - N_IN):
        assert abs(lp[i] - LR.logprob(x[i], ids[N_IN + i])) <= 0.05, i
        rid, rlp = LR.top(x[i], 2)
        if rlp[0] - rlp[1] > 0.05:
            assert top[i, 0] == rid[0], i
            moved += int(ids[N_IN + i] != rid[0])
    assert moved >= 10


def test_refusals(monkeypatch, graphs):
    from dflash_amd import dflash_generate, ops
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.engine import BatchEngine
    cfg = H.tiny_cfg()
    nt = _native()
    _, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    bias = _fallback_only()
    # a target that is no NativeTarget; T > 0 on the torch sampler; blocks of 17..32 rows, single request and batch
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(_draft_model(cfg), _walk_target()[0], _prompt(), cfg.mask_token_id, 8, 16, None, **bias)
    with pytest.raises(ValueError, match="sampler='device'"):
        dflash_generate(_draft_model(cfg), nt, _prompt(), cfg.mask_token_id, 8, 16, None, T, **bias)
    with pytest.raises(NotImplementedError, match="16 rows"):
        _single("generate", monkeypatch, hook, n_new=8, bs=24, **bias)
    with pytest.raises(NotImplementedError, match="16 rows"):
        BatchedDecoder(_draft_model(cfg), nt, 1, 256, 256, cfg.mask_token_id, tiles_per_request=2, logit_bias=True)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchedDecoder(_draft_model(cfg), nt, 1, 256, 256, cfg.mask_token_id, temperature=T, logit_bias=True)
    cache = nt.new_cache(128)
    nt.prefill(_prompt(), cache)
    state = ops.logit_bias_state(1, V, dev())
    with pytest.raises(NotImplementedError, match="16 rows"):
        nt.verify(torch.zeros(24, dtype=torch.long, device=dev()), N_IN, cache, logit_bias=state)
    with pytest.raises(ValueError, match="seed"):
        nt.verify(torch.zeros(8, dtype=torch.long, device=dev()), N_IN, cache, temperature=T, logit_bias=state)
    # a request with values on a decoder / engine built without the flag; neutral values are no request for it
    dec = BatchedDecoder(_draft_model(cfg), nt, 1, 256, 256, cfg.mask_token_id, stop_token_ids=[7])
    with pytest.raises(ValueError, match="logit_bias=True"):
        dec.admit(0, _prompt(), banned_token_ids=[3])
    with pytest.raises(ValueError, match="logit_bias=True"):
        dec.admit(0, _prompt(), min_tokens=2)
    eng = BatchEngine(_draft_model(cfg), nt, slots=1, max_rows=256, out_len=200, mask_token_id=cfg.mask_token_id)
    with pytest.raises(ValueError, match="logit_bias=True"):
        eng.submit(_prompt(), 8, logit_bias={3: 1.0})
    assert eng.submit(_prompt(), 8, logit_bias={3: 0.0}, banned_token_ids=[], min_tokens=4) == 0
    with pytest.raises(ValueError, match="outside"):
        BatchEngine(_draft_model(cfg), nt, slots=1, max_rows=256, out_len=200, mask_token_id=cfg.mask_token_id,
                    logit_bias=True).submit(_prompt(), 8, banned_token_ids=[V])
