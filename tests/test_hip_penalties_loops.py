"""Repetition / presence / frequency penalties through the decode loops: single request, policy,
ragged batch, slot-refill engine — on the tiny walk target of test_hip_sampling.py (helpers copied, not imported) with its
lm_head rebuilt for a permutation made of cycles of length 6 and scaled so the walk's logit is about 1.0: the walk comes
back to a token every six steps, and the penalties then push the continuation off it.

Truth is teacher-forced: one HF forward over the emitted ids gives the raw logits per position, penalties_ref.py the
penalised row from the emitted prefix, and every emitted token must be that row's argmax (T = 0) or its seeded draw
(T = 0.7) wherever the model's own top-2 gap is not a near-tie."""
import numpy as np
import pytest
import torch

import helpers as H
import logprobs_ref as LR
import penalties_ref as PR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048
T = 0.7
PEN = (1.3, 0.2, 0.25)
N_IN, N_NEW = 41, 120
_STATE = {}


def dev():
    return torch.device("cuda", 0)


def _kw(pen):
    return dict(repetition_penalty=pen[0], presence_penalty=pen[1], frequency_penalty=pen[2])


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
    """Drafts scripted from a continuation `tape` (absolute position -> token, the penalised reference run): plan[call]
    of its tokens, then a wrong one — accepted spans run across the positions where the penalties change the token."""
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


# ------------------------------------------------------------------------------------------------------------ the model
def _raw_rows(ids, n_in):
    hf, _ = _walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    return PR.f32_to_bf16_bits(logits[n_in - 1:len(ids) - 1]).reshape(len(ids) - n_in, V)


def _audit(ids, n_in, pen, temperature=0.0, seed=None):
    """Every emitted token against the model's penalised row for its prefix.  T = 0: the argmax wherever the row's top-2
    gap is >= 4 bf16 ulp (at least 90 % of the positions).  T = 0.7: the seeded draw wherever its perturbed gap exceeds
    0.1 (at least 85 %: the screen of test_hip_nucleus_loops.py).  Returns (emitted, screen, the model's tokens, raw rows)."""
    x = _raw_rows(ids, n_in)
    got = np.asarray(ids[n_in:])
    want, safe = np.zeros(len(got), dtype=np.int64), np.zeros(len(got), dtype=bool)
    for i in range(len(got)):
        p = n_in + i
        z = PR.penalise(x[i], *PR.history(ids, n_in, p, V), *pen)
        if temperature < 1e-5:
            want[i], safe[i] = PR.argmax_lowest(z), PR.bf16_ulp_gap(z) >= 4
        else:
            w, g = SR.draw(PR.bits_to_f32(z)[None], temperature, seed, SR.TARGET, [p])
            want[i], safe[i] = w[0], g[0] > 0.1
    assert safe.mean() >= (0.9 if temperature < 1e-5 else 0.85), safe.mean()
    assert np.array_equal(got[safe], want[safe]), (np.nonzero(safe & (got != want))[0][:8], safe.mean())
    return got, safe, want, x


def _dependence(ids, n_in, pen, x):
    """On the reference alone: positions where the penalised argmax leaves the raw one, and positions where it changes if
    the last <= 15 tokens (what a block holds in front of a row) are left out of the history."""
    changed = blockdep = 0
    for i in range(len(ids) - n_in):
        p = n_in + i
        full = PR.argmax_lowest(PR.penalise(x[i], *PR.history(ids, n_in, p, V), *pen))
        changed += full != PR.argmax_lowest(x[i])
        blockdep += full != PR.argmax_lowest(PR.penalise(x[i], *PR.history(ids, n_in, max(n_in, p - 15), V), *pen))
    return int(changed), int(blockdep)


def _same_until_a_near_tie(a, b):
    """Two audited runs of one request: a divergence may only start at a position either screen left out."""
    (ga, sa, _, _), (gb, sb, _, _) = a, b
    n = min(len(ga), len(gb))
    diff = np.nonzero(ga[:n] != gb[:n])[0]
    if diff.size:
        assert not (sa[diff[0]] and sb[diff[0]]), diff[0]


def _table_ok(table_row, ids_row, n_in, start):
    """The count-once invariant: the row equals a recount of the final ids — prompt flags from [0, n_in), counts from
    [n_in, start]."""
    want = PR.table_of(ids_row.cpu().numpy(), n_in, start + 1, V)
    got = table_row.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


# ------------------------------------------------------------------------------------------------------------ the runs
@pytest.fixture
def made(monkeypatch):
    """Every DecodeSession / BatchedDecoder the entries build, kept for the table invariant — and dropped with the test:
    a session holds its hipGraphs, and graphs left alive would pin the capture state of torch's CUDA generator for the
    test files behind this one."""
    import gc
    from dflash_amd import batch as B, engine as E, generate as G
    made = []
    if not hasattr(G.DecodeSession, "_pen_spy"):
        for mod, name in ((G, "DecodeSession"), (B, "BatchedDecoder")):
            base = getattr(mod, name)

            class Spy(base):
                _pen_spy = True

                def __init__(self, *a, **k):
                    super().__init__(*a, **k)
                    _STATE["made"].append(self)

            Spy.__name__ = name
            monkeypatch.setattr(mod, name, Spy)
            if mod is B:
                monkeypatch.setattr(E, name, Spy)
    _STATE["made"] = made
    yield made
    made.clear()
    _STATE.pop("made", None)
    gc.collect()


def _check_tables(made):
    n = 0
    for o in made:
        if hasattr(o, "pen"):      # a DecodeSession
            if o.pen is not None:
                _table_ok(o.pen.table[0], o.output_ids[0], o.n_in, o.start)
                n += 1
        elif o.penalties:
            for r in range(o.R):
                if o.n_in[r]:
                    _table_ok(o.pen_table[r], o.output_ids[r], o.n_in[r], o.start[r])
                    n += 1
    return n


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


def _many(entry, monkeypatch, prompts, hooks, *, temperature=0.0, seeds=None, n_new=80, **kw):
    """dflash_generate_batch / dflash_generate_stream over `prompts`, hooks[i](blk, start, call) per prompt."""
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import dflash_generate_stream
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    fn = dflash_generate_batch if entry == "batch" else dflash_generate_stream
    extra = dict(slots=2) if entry == "stream" else {}
    sampled = any(t >= 1e-5 for t in temperature) if isinstance(temperature, list) else temperature >= 1e-5
    skw = dict(sampler="device", seed=seeds) if sampled else {}
    return fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, n_new, 16, None, temperature,
              draft_token_hook=lambda i, blk, start, call: hooks[i](blk, start, call), **skw, **extra, **kw)


def _ids(r):
    return r.output_ids[0].tolist()


PROMPTS3 = ((3, 41), (4, 37), (5, 45))


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("temperature", [0.0, T])
@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_teacher_forced_audit(entry, temperature, monkeypatch, made):
    """Two passes per entry: drafts from the raw walk (its output is the penalised continuation, the tape), then drafts
    scripted from that tape, so that accepted spans cross the positions the penalties change.  Both pass the audit and
    agree up to near-ties; the table rows equal a recount of the final ids."""
    _, perm = _walk_target()
    plan = _plan()
    if entry in ("generate", "policy"):
        seed = 5 if temperature >= 1e-5 else None
        a = _single(entry, monkeypatch, _walk_hook(perm, plan), temperature=temperature, seed=seed, **_kw(PEN))
        b = _single(entry, monkeypatch, _tape_hook(_ids(a), plan), temperature=temperature, seed=seed, **_kw(PEN))
        runs = [(N_IN, seed, a, b)]
    else:
        prompts = [_prompt(s, n) for s, n in PROMPTS3]
        seeds = [7, 8, 9] if temperature >= 1e-5 else None
        a = _many(entry, monkeypatch, prompts, [_walk_hook(perm, plan)] * 3, temperature=temperature, seeds=seeds, **_kw(PEN))
        b = _many(entry, monkeypatch, prompts, [_tape_hook(_ids(r), plan) for r in a], temperature=temperature,
                  seeds=seeds, **_kw(PEN))
        runs = [(p.shape[1], seeds[i] if seeds else None, a[i], b[i]) for i, p in enumerate(prompts)]
    for n_in, seed, ra, rb in runs:
        n_new = N_NEW if entry in ("generate", "policy") else 80
        assert len(_ids(ra)) == len(_ids(rb)) == n_in + n_new, "a run drew the mask id: pick another seed"
        ua = _audit(_ids(ra), n_in, PEN, temperature, seed)
        ub = _audit(_ids(rb), n_in, PEN, temperature, seed)
        _same_until_a_near_tie(ua, ub)
        if temperature < 1e-5:
            changed, blockdep = _dependence(_ids(rb), n_in, PEN, ub[3])
            print(f"[penalties] {entry}: {changed} positions leave the raw argmax, {blockdep} depend on the last 15 tokens, "
                  f"screen keeps {ub[1].mean():.3f}, mean tau {np.mean(rb.acceptance_lengths):.2f}")
            assert blockdep >= 5 and changed >= 5
            assert max(rb.acceptance_lengths) > 6        # accepted spans: the in-block history is in play
    assert _check_tables(made) >= 2


@pytest.mark.parametrize("entry", ["generate", "batch"])
def test_cold_draw_runs_over_the_penalised_rows(entry, monkeypatch, made):
    """At T = 0.7 the rows of this target are nearly flat (the walk's token holds 0.2 % of the mass): the draws there
    seldom land on a token the penalties moved.  At T = 0.1 the walk's token holds ~90 %: the draw follows the walk until
    the penalties push it off, and — on the reference alone — at least 5 positions draw another token over the penalised
    row than over the raw one (13 here)."""
    cold, seed = 0.1, 11
    _, perm = _walk_target()
    plan = _plan()
    if entry == "generate":
        a = _single(entry, monkeypatch, _walk_hook(perm, plan), temperature=cold, seed=seed, **_kw(PEN))
        b = _single(entry, monkeypatch, _tape_hook(_ids(a), plan), temperature=cold, seed=seed, **_kw(PEN))
    else:
        a = _many(entry, monkeypatch, [_prompt()], [_walk_hook(perm, plan)], temperature=cold, seeds=[seed], n_new=N_NEW,
                  **_kw(PEN))[0]
        b = _many(entry, monkeypatch, [_prompt()], [_tape_hook(_ids(a), plan)], temperature=cold, seeds=[seed], n_new=N_NEW,
                  **_kw(PEN))[0]
    assert len(_ids(a)) == len(_ids(b)) == N_IN + N_NEW, "a run drew the mask id: pick another seed"
    ua, ub = _audit(_ids(a), N_IN, PEN, cold, seed), _audit(_ids(b), N_IN, PEN, cold, seed)
    _same_until_a_near_tie(ua, ub)
    raw, _ = SR.draw(PR.bits_to_f32(ub[3]), cold, seed, SR.TARGET, np.arange(N_IN, N_IN + N_NEW))
    moved = int((raw != ub[2]).sum())
    print(f"[penalties] {entry} at T = {cold}: {moved} positions draw another token than over the raw rows, screen keeps "
          f"{ub[1].mean():.3f}, mean tau {np.mean(b.acceptance_lengths):.2f}")
    assert moved >= 5 and max(b.acceptance_lengths) > 6
    assert _check_tables(made) == 2


def test_prompt_tokens_count(monkeypatch, made):
    """r = 20 alone, a prompt that ends with a whole 6-cycle: the walk's next tokens are all in the prompt, 1.0 / 20 falls
    below the other logits, so the continuation leaves the walk at once — and does not if the prompt is left out."""
    _, perm = _walk_target()
    cyc = [17]
    for _ in range(5):
        cyc.append(perm[cyc[-1]])
    prompt = torch.cat([_prompt(6, 30), torch.tensor([cyc], device=dev())], dim=1)
    pen = (20.0, 0.0, 0.0)
    r = _single("generate", monkeypatch, _walk_hook(perm, _plan()), prompt=prompt, n_new=40, **_kw(pen))
    ids = _ids(r)
    got, safe, want, x = _audit(ids, 36, pen)
    no_prompt = [PR.argmax_lowest(PR.penalise(x[i], *PR.seen_counts(PR.table_of(ids[36:], 0, i, V)), *pen)) for i in range(6)]
    assert no_prompt[0] == perm[cyc[-1]] == cyc[0] and want[0] != cyc[0] and got[0] != cyc[0]
    assert _check_tables(made) == 1


@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_neutral_values_change_nothing(entry, monkeypatch):
    """r = 1, a = 0, f = 0: the ids and acceptance lengths of the run without the keywords, and no penalty launch."""
    from dflash_amd import ops
    calls = []
    for name in ("penalty_rows", "penalty_count"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _real=real, **k: (calls.append(1), _real(*a, **k))[1])
    _, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    neutral = _kw((1.0, 0.0, 0.0))
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


@pytest.mark.parametrize("kind,temperature", [("generate", 0.0), ("policy", T)])
def test_replay_equals_eager(kind, temperature, monkeypatch, made):
    """DFL_GRAPH=1 against DFL_GRAPH=0: ids and acceptance lengths, the replayed run really replayed; the same with a
    stop id committed inside a replayed cycle.  The table rows of all four runs equal a recount."""
    _, perm = _walk_target()
    plan = _plan()
    seed = 5 if temperature >= 1e-5 else None
    kw = dict(temperature=temperature, seed=seed, **_kw(PEN))
    tape = _ids(_single(kind, monkeypatch, _walk_hook(perm, plan), graph=False, **kw))
    hook = _tape_hook(tape, plan)
    ref = _single(kind, monkeypatch, hook, graph=False, **kw)
    rep = _single(kind, monkeypatch, hook, graph=True, **kw)
    assert _ids(rep) == _ids(ref) and list(rep.acceptance_lengths) == list(ref.acceptance_lengths)
    assert rep.replayed_cycles > 0 and ref.replayed_cycles == 0 and max(ref.acceptance_lengths) > 2
    new = _ids(ref)[N_IN:]
    cands = [i for i in range(len(new) // 2, len(new) - 20) if new.index(new[i]) == i]
    assert cands
    stop = [new[cands[0]]]
    s_ref = _single(kind, monkeypatch, hook, graph=False, stop=stop, **kw)
    s_rep = _single(kind, monkeypatch, hook, graph=True, stop=stop, **kw)
    assert _ids(s_rep) == _ids(s_ref) == _ids(ref)[:N_IN + cands[0] + 1] and s_rep.replayed_cycles > 0
    assert list(s_rep.acceptance_lengths) == list(s_ref.acceptance_lengths)
    assert _check_tables(made) == 5


MIXED = ((1.3, 0.2, 0.25), (1.0, 0.0, 0.0), (1.6, 0.0, 0.1), (1.0, 0.4, 0.3))


@pytest.mark.parametrize("entry,temps", [("batch", [0.0] * 4), ("stream", [0.0, T, T, 0.0])])
def test_requests_with_their_own_values(entry, temps, monkeypatch, made):
    """Four requests, each with its own (r, a, f) — one of them neutral — and, through the engine, its own temperature:
    each passes the audit with its own values; the neutral one emits what its run without the keywords emits; the engine's
    two slots serve two requests each, and every table row equals a recount of the last request it served."""
    _, perm = _walk_target()
    plan = _plan()
    prompts = [_prompt(s, n) for s, n in ((3, 41), (4, 37), (5, 45), (6, 33))]
    seeds = [21, 22, 23, 24]
    pk = dict(repetition_penalty=[p[0] for p in MIXED], presence_penalty=[p[1] for p in MIXED],
              frequency_penalty=[p[2] for p in MIXED])
    mixed_t = any(t != temps[0] for t in temps)
    tv = temps if mixed_t else temps[0]
    a = _many(entry, monkeypatch, prompts, [_walk_hook(perm, plan)] * 4, temperature=tv, seeds=seeds, **pk)
    b = _many(entry, monkeypatch, prompts, [_tape_hook(_ids(r), plan) for r in a], temperature=tv, seeds=seeds, **pk)
    for i, p in enumerate(prompts):
        n_in = p.shape[1]
        assert len(_ids(a[i])) == len(_ids(b[i])) == n_in + 80, "a run drew the mask id: pick another seed"
        ua = _audit(_ids(a[i]), n_in, MIXED[i], temps[i], seeds[i])
        ub = _audit(_ids(b[i]), n_in, MIXED[i], temps[i], seeds[i])
        _same_until_a_near_tie(ua, ub)
    # the neutral request: its plain single-request run (same hook: drafts from the raw walk)
    plain = _single("generate", monkeypatch, _walk_hook(perm, plan), prompt=prompts[1], n_new=80, temperature=temps[1],
                    seed=seeds[1])
    if temps[1] < 1e-5:
        assert _ids(plain) == _ids(a[1]) and list(plain.acceptance_lengths) == list(a[1].acceptance_lengths)
    else:   # (another launch form draws: equal up to a near-tie of the perturbed values)
        _same_until_a_near_tie(_audit(_ids(plain), 37, MIXED[1], temps[1], seeds[1]), _audit(_ids(a[1]), 37, MIXED[1], temps[1], seeds[1]))
    decs = [o for o in made if getattr(o, "penalties", False)]
    assert len(decs) == 2 and _check_tables(made) >= (8 if entry == "batch" else 4)
    if entry == "stream":      # a refilled slot starts from a cleared row: checked by the recount of the slot's last request
        slots_used = [r.slot for r in b]
        assert max(slots_used.count(s) for s in set(slots_used)) >= 2


def test_logprobs_stay_those_of_the_raw_rows(monkeypatch):
    """penalties + logprobs=2: the values are log_softmax of the RAW teacher-forced rows (logprobs_ref.py, the tolerance
    the logprobs loop tests use across two GEMMs), and the most likely token is the raw argmax even where the penalties
    made the run emit another one."""
    _, perm = _walk_target()
    plan = _plan()
    tape = _ids(_single("generate", monkeypatch, _walk_hook(perm, plan), **_kw(PEN)))
    r = _single("generate", monkeypatch, _tape_hook(tape, plan), logprobs=2, **_kw(PEN))
    ids = _ids(r)
    x = PR.bits_to_f32(_raw_rows(ids, N_IN))
    lp, top = r.logprobs.cpu().numpy(), r.top_logprob_ids.cpu().numpy()
    moved = 0
    for i in range(len(ids) - N_IN):
        assert abs(lp[i] - LR.logprob(x[i], ids[N_IN + i])) <= 0.05, i
        rid, rlp = LR.top(x[i], 2)
        if rlp[0] - rlp[1] > 0.05:
            assert top[i, 0] == rid[0], i
            moved += int(ids[N_IN + i] != rid[0])
    assert moved >= 5


def test_refusals(monkeypatch):
    from dflash_amd import dflash_generate, ops
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.engine import BatchEngine
    cfg = H.tiny_cfg()
    nt = _native()
    _, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    # a target that is no NativeTarget; T > 0 on the torch sampler; blocks of 17..32 rows, single request and batch
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(_draft_model(cfg), _walk_target()[0], _prompt(), cfg.mask_token_id, 8, 16, None, **_kw(PEN))
    with pytest.raises(ValueError, match="sampler='device'"):
        dflash_generate(_draft_model(cfg), nt, _prompt(), cfg.mask_token_id, 8, 16, None, T, **_kw(PEN))
    with pytest.raises(NotImplementedError, match="16 rows"):
        _single("generate", monkeypatch, hook, n_new=8, bs=24, **_kw(PEN))
    with pytest.raises(NotImplementedError, match="16 rows"):
        BatchedDecoder(_draft_model(cfg), nt, 1, 256, 256, cfg.mask_token_id, tiles_per_request=2, penalties=True)
    cache = nt.new_cache(128)
    nt.prefill(_prompt(), cache)
    pen = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="16 rows"):
        nt.verify(torch.zeros(24, dtype=torch.long, device=dev()), N_IN, cache, penalties=pen)
    with pytest.raises(ValueError, match="seed"):
        nt.verify(torch.zeros(8, dtype=torch.long, device=dev()), N_IN, cache, temperature=T, penalties=pen)
    # a request with penalties on a decoder / engine built without the flag
    dec = BatchedDecoder(_draft_model(cfg), nt, 1, 256, 256, cfg.mask_token_id)
    with pytest.raises(ValueError, match="penalties=True"):
        dec.admit(0, _prompt(), frequency_penalty=0.1)
    eng = BatchEngine(_draft_model(cfg), nt, slots=1, max_rows=256, out_len=200, mask_token_id=cfg.mask_token_id)
    with pytest.raises(ValueError, match="penalties=True"):
        eng.submit(_prompt(), 8, repetition_penalty=1.2)
    assert eng.submit(_prompt(), 8, repetition_penalty=1.0) == 0       # neutral values are no request for the flag
    with pytest.raises(ValueError, match="repetition_penalty"):
        ops.check_penalties(-1.0)
