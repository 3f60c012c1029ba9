"""top_k / top_p through the decode loops ("Filtered draw"): single request, policy, ragged batch,
slot-refill engine — on the tiny walk target of test_hip_sampling.py (helpers copied, not imported)."""
import numpy as np
import pytest
import torch

import helpers as H
import nucleus_ref as NR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
KP = (20, 0.9)
_STATE = {}


def dev():
    return torch.device("cuda", 0)


def _walk_target(scale=0.62):
    """The greedy-walk target with its lm_head scaled down: the walk's next token keeps probability ~0.75 - 0.8 at
    T = 0.7 instead of ~1, so the draws are genuinely random."""
    if "hf" not in _STATE:
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        torch.manual_seed(11)
        hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev(), dtype=BF16)
        perm = impose_greedy_walk(hf, seed=8)
        with torch.no_grad():
            hf.lm_head.weight.mul_(scale)
        _STATE["hf"], _STATE["perm"] = hf, perm.cpu().tolist()
    return _STATE["hf"], _STATE["perm"]


def _draft_model(cfg):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return m


def _hook(perm, plan, V=2048):
    """Drafts scripted from the walk of the block's first token: plan[call] walk tokens, then a wrong one."""
    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        b = int(blk[0, 0])
        toks = []
        for _ in range(k):
            b = perm[b]
            toks.append(b)
        if k + 1 < blk.shape[1]:
            toks.append((perm[b] + 1) % V)
        if toks:
            blk[0, 1:1 + len(toks)] = torch.tensor(toks, dtype=blk.dtype, device=blk.device)
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


def _prompt(seed=3, n=41):
    return torch.randint(0, 2000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev())


def _plan():
    return H.make_plan(400, 16, 29)


def _run(kind, monkeypatch, *, graph=True, run_ahead=True, stop=None, temperature=T, sampler="device", seed=1, bs=16,
         n_new=120, native=True, prompt=None, **flt):
    from dflash_amd import NativeTarget, dflash_generate, dflash_generate_policy
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("DFL_RUN_AHEAD", "1" if run_ahead else "0")
    hf, perm = _walk_target()
    cfg = H.tiny_cfg()
    target = NativeTarget(hf) if native else hf
    hook = _hook(perm, _plan())
    prompt = _prompt() if prompt is None else prompt
    if kind == "fixed":
        r = dflash_generate(_draft_model(cfg), target, prompt, cfg.mask_token_id, n_new, bs, stop, temperature,
                            draft_token_hook=hook, sampler=sampler, seed=seed, **flt)
    else:
        r = dflash_generate_policy(model=_draft_model(cfg), target=target, input_ids=prompt,
                                   mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, stop_token_ids=stop,
                                   temperature=temperature, scheduler=_script(), draft_token_hook=hook, sampler=sampler,
                                   seed=seed, **flt)
    return r.output_ids[0].tolist(), list(r.acceptance_lengths), r.replayed_cycles


def _bf16_ulp(t):
    return 2.0 ** (np.floor(np.log2(max(abs(float(t)), 1e-30))) - 7)


def _audit(ids, n_in, seed, K, P, gap=0.1, keep=0.85):
    """Teacher-forced: one HF forward over the emitted ids gives the model threshold t per position.  Unscreened: every
    emitted token has x >= t - 4 ulp (a filter that is not applied fails here).  Screened: the token is the model's draw
    wherever that draw is the same over {x >= t - D} and {x >= t + D} and its perturbed gap exceeds `gap`."""
    hf, _ = _walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    pos = np.arange(n_in, len(ids))
    x = SR.bf16_round(logits[pos - 1])
    got = np.asarray(ids)[pos]
    thr = np.array([NR.thresholds(row, T, K, P)[2] for row in x])
    d = 4 * np.array([_bf16_ulp(t) for t in thr])
    assert (x[np.arange(len(pos)), got] >= thr - d).all(), np.nonzero(x[np.arange(len(pos)), got] < thr - d)
    lo, gl = NR.draw_over(x, thr - d, T, seed, SR.TARGET, pos)
    hi, gh = NR.draw_over(x, np.minimum(thr + d, x.max(axis=1)), T, seed, SR.TARGET, pos)
    safe = (lo == hi) & (gl > gap) & (gh > gap)
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(got[safe], lo[safe]), np.nonzero(got[safe] != lo[safe])
    return got, safe


def _walk_hits(ids, n_in):
    perm = _walk_target()[1]
    return float(np.mean([perm[a] == b for a, b in zip(ids[n_in - 1:-1], ids[n_in:])]))


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("entry", ["generate", "policy", "batch", "stream"])
def test_top_k_1_at_t07_reproduces_t0(entry, monkeypatch):
    """K = 1 keeps the argmax alone: the sampled run emits the greedy run's ids and acceptance lengths exactly."""
    from dflash_amd import NativeTarget
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import dflash_generate_stream
    if entry in ("generate", "policy"):
        kind = "fixed" if entry == "generate" else "policy"
        greedy = _run(kind, monkeypatch, temperature=0.0, sampler="torch", seed=None)
        k1 = _run(kind, monkeypatch, top_k=1)
        assert k1[:2] == greedy[:2]
        assert _run(kind, monkeypatch)[0] != greedy[0]        # (the unfiltered T = 0.7 run is not the greedy one)
        return
    monkeypatch.setenv("DFL_GRAPH", "1")
    hf, perm = _walk_target()
    cfg = H.tiny_cfg()
    prompts = [_prompt(3, 41), _prompt(4, 37), _prompt(5, 45)]
    plan = _plan()
    hook = lambda r, blk, start, call: _hook(perm, plan)(blk, start, call)   # noqa: E731
    fn = dflash_generate_batch if entry == "batch" else dflash_generate_stream
    kw = dict(slots=2) if entry == "stream" else {}
    greedy = fn(_draft_model(cfg), NativeTarget(hf), prompts, cfg.mask_token_id, 80, 16, None, 0.0,
                draft_token_hook=hook, **kw)
    k1 = fn(_draft_model(cfg), NativeTarget(hf), prompts, cfg.mask_token_id, 80, 16, None, T, draft_token_hook=hook,
            sampler="device", seed=7, top_k=1, **kw)
    for a, b in zip(greedy, k1):
        assert a.output_ids[0].tolist() == b.output_ids[0].tolist()
        assert list(a.acceptance_lengths) == list(b.acceptance_lengths)


@pytest.mark.parametrize("kind", ["fixed", "policy"])
def test_launch_modes_give_identical_ids_under_a_filter(kind, monkeypatch):
    """DFL_GRAPH=0, replay and DFL_RUN_AHEAD=0 at top_k=20, top_p=0.9: same ids and acceptance lengths, the replayed run
    really replayed; the same with a stop id taken from a replayed cycle."""
    flt = dict(top_k=KP[0], top_p=KP[1])
    ref = _run(kind, monkeypatch, graph=False, **flt)
    rep = _run(kind, monkeypatch, graph=True, **flt)
    noahead = _run(kind, monkeypatch, graph=True, run_ahead=False, **flt)
    assert rep[:2] == ref[:2] and noahead[:2] == ref[:2]
    assert rep[2] > 0 and max(ref[1]) > 2
    _audit(ref[0], 41, 1, *KP)
    # a stop id first emitted well inside the run (cycles there are replays)
    new = ref[0][41:]
    cands = [i for i in range(len(new) // 2, len(new) - 20) if new.index(new[i]) == i]
    assert cands
    stop = [new[cands[0]]]
    s_ref = _run(kind, monkeypatch, graph=False, stop=stop, **flt)
    s_rep = _run(kind, monkeypatch, graph=True, stop=stop, **flt)
    assert s_rep[:2] == s_ref[:2] and s_ref[0] == ref[0][:41 + cands[0] + 1] and s_rep[2] > 0


@pytest.mark.parametrize("mode", ["bs16", "bs24", "bs1", "policy", "hf_target", "batch_bs24"])
def test_teacher_forced_audit_under_a_filter(mode, monkeypatch):
    flt = dict(top_k=KP[0], top_p=KP[1])
    if mode == "bs16":
        ids, _, _ = _run("fixed", monkeypatch, seed=5, **flt)
    elif mode == "bs24":
        ids, _, _ = _run("fixed", monkeypatch, seed=5, bs=24, **flt)
    elif mode == "bs1":
        ids, _, _ = _run("fixed", monkeypatch, seed=5, bs=1, **flt)
    elif mode == "policy":
        ids, _, _ = _run("policy", monkeypatch, seed=5, **flt)
    elif mode == "hf_target":
        ids, _, _ = _run("fixed", monkeypatch, seed=5, native=False, **flt)
    else:   # two tiles per request in the ragged batch (a group of one)
        from dflash_amd import NativeTarget
        from dflash_amd.batch import dflash_generate_batch
        hf, perm = _walk_target()
        cfg = H.tiny_cfg()
        hook = _hook(perm, _plan())
        ids = dflash_generate_batch(_draft_model(cfg), NativeTarget(hf), [_prompt()], cfg.mask_token_id, 120, 24, None, T,
                                    draft_token_hook=lambda r, blk, start, call: hook(blk, start, call), group_size=1,
                                    sampler="device", seed=[5], **flt)[0].output_ids[0].tolist()
    _audit(ids, 41, 5, *KP)


def test_engine_with_per_request_filters(monkeypatch):
    """6 requests through 2 slots, each with its own (K, P): every request passes the audit with its own parameters and
    agrees with its single-request run where both are safe; an unfiltered request admitted into a slot that last held a
    K = 1 request is not greedy (the slot's parameters are re-armed); one capture serves the engine's life."""
    from dflash_amd import NativeTarget
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1")
    hf, perm = _walk_target()
    cfg = H.tiny_cfg()
    kps = [(1, 1.0), (0, 1.0), (20, 0.9), (0, 0.7), (1, 1.0), (0, 1.0)]
    mnt = [40, 100, 60, 220, 30, 80]   # (request 3 outlasts request 4: request 5 then follows request 4 in its slot)
    prompts = [_prompt(10 + i, 37 + i) for i in range(6)]
    seeds = [50 + i for i in range(6)]
    # (the tiny vocabulary holds the mask id: a request that DRAWS it has that token dropped by the reference's trim, and a
    # teacher-forced pass over the trimmed ids cannot place the positions behind it.  The two unfiltered requests take
    # prompts, seeds and lengths under which test_hip_stream.py's unfiltered requests draw none; asserted below)
    prompts[1], seeds[1] = _prompt(4, 37), 2 ** 63 + 9
    prompts[5], seeds[5] = _prompt(7, 45), 35
    plan = _plan()
    eng = BatchEngine(_draft_model(cfg), NativeTarget(hf), slots=2, max_rows=45 + 220 + 48, out_len=45 + 220 + 16,
                      mask_token_id=cfg.mask_token_id, block_size=16, temperature=T, sampler="device", filtering=True)
    for i, p in enumerate(prompts):
        eng.submit(p, mnt[i], seed=seeds[i], draft_token_hook=_hook(perm, plan), top_k=kps[i][0], top_p=kps[i][1])
    res = eng.run()
    assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] > 0
    for i, r in enumerate(res):
        n_in = prompts[i].shape[1]
        ids = r.output_ids[0].tolist()
        assert len(ids) == n_in + mnt[i], f"request {i} drew the mask id: pick another seed"
        got_e, safe_e = _audit(ids, n_in, seeds[i], *kps[i])
        single, _, _ = _run("fixed", monkeypatch, seed=seeds[i], n_new=mnt[i], prompt=prompts[i], top_k=kps[i][0],
                            top_p=kps[i][1])
        assert len(single) == n_in + mnt[i], f"request {i} drew the mask id in its single run: pick another seed"
        got_s, safe_s = _audit(single, n_in, seeds[i], *kps[i])
        diff = np.nonzero(got_e[:len(got_s)] != got_s[:len(got_e)])[0]
        if diff.size:   # a divergence may only start at a screened-out near-tie
            assert not (safe_e[diff[0]] and safe_s[diff[0]]), (i, diff[0])
    # request 5 (unfiltered) follows request 4 (K = 1) in its slot
    assert res[5].slot == res[4].slot and res[4].finished_step <= res[5].admitted_step
    assert 0.3 < _walk_hits(res[5].output_ids[0].tolist(), prompts[5].shape[1]) < 0.95
    assert _walk_hits(res[4].output_ids[0].tolist(), prompts[4].shape[1]) >= 0.97


def test_defaults_change_nothing(monkeypatch):
    """top_k=0, top_p=1.0 give the ids of a call without the keywords, and never reach the new entry point."""
    from dflash_amd import ops
    calls = []
    real = ops.sample_rows_nucleus
    monkeypatch.setattr(ops, "sample_rows_nucleus", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for kind in ("fixed", "policy"):
        assert _run(kind, monkeypatch, n_new=60, top_k=0, top_p=1.0) == _run(kind, monkeypatch, n_new=60)
        assert _run(kind, monkeypatch, n_new=60, temperature=0.0, sampler="torch", seed=None, top_k=5, top_p=0.5) == \
            _run(kind, monkeypatch, n_new=60, temperature=0.0, sampler="torch", seed=None)
    assert not calls
    _run("fixed", monkeypatch, n_new=20, top_k=5)
    assert calls
