"""GPU tests of the slot-refilling ragged batch (dflash_amd.engine, BatchedDecoder.admit_fused, dfl_admit_slot): the
fused admission leaves the device state `admit` leaves, and every request of a refilled batch comes out exactly as
its own single-request run — whichever slot it lands in and whatever ran there before."""
import numpy as np
import pytest
import torch

import helpers as H
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7

MAX_NEW = [12, 96, 20, 150, 30, 8, 120, 40, 16, 64]
# slot 0 runs requests 0 -> 4 -> 6 (long, then a prompt shorter than a tile, then long again), slot 2 runs 2 -> 5 -> 7 -> 8
LENS = [150, 21, 33, 40, 7, 180, 90, 12, 64, 17]


def dev():
    return torch.device("cuda", 0)


_STATE = {}


def _setup(layers=6, seed=5):
    """tests/test_hip_batch.py::_setup: tiny draft + tiny Qwen3 target with the greedy walk."""
    if "greedy" not in _STATE:
        from dflash_amd import DFlashDraftModel, NativeTarget
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        cfg = H.tiny_cfg()
        m = DFlashDraftModel(cfg, device=dev())
        m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
        torch.manual_seed(11)
        hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": layers}, dev(), dtype=BF16)
        perm = impose_greedy_walk(hf, seed=seed)
        _STATE["greedy"] = (cfg, m, hf, NativeTarget(hf), perm)
    return _STATE["greedy"]


def _walk_target(scale=0.62):
    """tests/test_hip_sampling.py::_walk_target: the walk target with its lm_head scaled down (top token p ~ 0.75 - 0.8
    at T = 0.7)."""
    if "soft" not in _STATE:
        from dflash_amd import DFlashDraftModel, NativeTarget
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        cfg = H.tiny_cfg()
        m = DFlashDraftModel(cfg, device=dev())
        m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
        torch.manual_seed(11)
        hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev(), dtype=BF16)
        perm = impose_greedy_walk(hf, seed=8)
        with torch.no_grad():
            hf.lm_head.weight.mul_(scale)
        _STATE["soft"] = (cfg, m, hf, NativeTarget(hf), perm.cpu().tolist())
    return _STATE["soft"]


def _hook_for(G, plan, vocab=2000):
    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % vocab, blk[0, k + 1])
    return hook


def _prompt(P, seed):
    return torch.randint(0, 2000, (1, P), generator=torch.Generator().manual_seed(seed)).to(dev())


def _plan_cycles(max_new, plan, block=16):
    left, call = max_new, 0
    while left > 0:
        bs = max(1, min(block, left))
        left -= min(plan[call], bs - 1) + 1
        call += 1
    return call


def _workload(perm, extra=60):
    from dflash_amd.synthetic import greedy_walk
    prompts = [_prompt(P, 300 + i) for i, P in enumerate(LENS)]
    Gs = [greedy_walk(perm, p, MAX_NEW[i] + extra).to(dev()) for i, p in enumerate(prompts)]
    plans = [H.make_plan(64, 16, 200 + i) for i in range(len(LENS))]
    hooks = [_hook_for(Gs[i], plans[i]) for i in range(len(LENS))]
    return prompts, Gs, plans, hooks


def _singles(cfg, m, nt, prompts, hooks, stop=None):
    from dflash_amd import dflash_generate
    return [dflash_generate(m, nt, prompts[i], cfg.mask_token_id, MAX_NEW[i], 16, stop, 0.0, draft_token_hook=hooks[i])
            for i in range(len(prompts))]


def _engine(cfg, m, nt, slots=4, **kw):
    from dflash_amd.engine import BatchEngine
    need = max(P + n for P, n in zip(LENS, MAX_NEW))
    return BatchEngine(m, nt, slots=slots, max_rows=need + 48, out_len=need + 16, mask_token_id=cfg.mask_token_id, **kw)


def _same(a, b, what):
    assert a.output_ids[0].tolist() == b.output_ids[0].tolist(), what
    assert list(a.acceptance_lengths) == list(b.acceptance_lengths), what
    assert a.num_output_tokens == b.num_output_tokens, what


# ------------------------------------------------------------------------------------------------ fused admission
SLOT_TENSORS = ("output_ids", "block", "dyn_d", "dyn_t", "seeds")


def _slot_state(dec, r):
    st = {k: getattr(dec, k)[r].clone() for k in SLOT_TENSORS}
    st["taps"] = dec.d["taps"][r].clone()
    return st


def _assert_slot_equal(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs"


@pytest.mark.parametrize("P", [1, 7, 16, 17, 33, 200])
@pytest.mark.parametrize("temperature,sampler", [(0.0, "torch"), (T, "device")])
def test_admit_fused_leaves_what_admit_leaves(P, temperature, sampler):
    from dflash_amd.batch import BatchedDecoder
    cfg, m, hf, nt, perm = _setup()

    def mk():
        return BatchedDecoder(m, nt, 3, max_rows=400, out_len=400, mask_token_id=cfg.mask_token_id, temperature=temperature,
                              sampler=sampler)

    A, B, C = mk(), mk(), mk()
    p = _prompt(P, 900 + P)
    before = [_slot_state(B, r) for r in (0, 2)]
    A.admit(1, p, temperature, seed=77)
    B.admit_fused(1, p, temperature, seed=77)
    _assert_slot_equal(_slot_state(A, 1), _slot_state(B, 1), "fresh slot")
    for j, r in enumerate((0, 2)):
        _assert_slot_equal(before[j], _slot_state(B, r), f"slot {r} touched")
    assert B.lm_wp is not None and B.lm_wp.data_ptr() == A.lm_wp.data_ptr() == nt.lm_wp.data_ptr()
    assert B.embed_w is not None and B.embed_w.data_ptr() == A.embed_w.data_ptr()
    assert (B.start[1], B.n_in[1], B.live[1], B.hook_calls[1], B.bs[1]) == (A.start[1], A.n_in[1], A.live[1],
                                                                           A.hook_calls[1], A.bs[1]) == (P, P, True, 0, 16)
    if sampler == "device":
        assert int(B.seeds[1]) == 77
    assert int(B.output_ids[1, P]) == int(B.block[1, 0]) != cfg.mask_token_id
    assert bool((B.output_ids[1, P + 1:] == cfg.mask_token_id).all())

    # dirty slot: a longer request decodes in slot 1 beside two neighbours, then the slot is re-armed for p2
    for D in (A, B):
        D.admit(0, _prompt(40, 1), temperature, seed=5)
        D.admit(2, _prompt(19, 2), temperature, seed=6)
        D.admit(1, _prompt(230, 3), temperature, seed=9)
        for _ in range(3):
            D.cycle()
        D.park(1)
    assert B.start[1] > 230 and int(B.dyn_d[1, 6]) == 3   # (DYN_CYCLE: the slot really ran)
    p2 = _prompt(P, 950 + P)
    before = [_slot_state(B, r) for r in (0, 2)]
    others = [(B.post[r].clone(), B.result[r].clone()) for r in (0, 2)]
    A.admit(1, p2, temperature, seed=78)
    B.admit_fused(1, p2, temperature, seed=78)
    C.admit(1, p2, temperature, seed=78)
    _assert_slot_equal(_slot_state(A, 1), _slot_state(B, 1), "dirty slot, admit against admit_fused")
    _assert_slot_equal(_slot_state(C, 1), _slot_state(B, 1), "dirty slot against a fresh decoder's admit")
    for j, r in enumerate((0, 2)):
        _assert_slot_equal(before[j], _slot_state(B, r), f"slot {r} touched")
        assert torch.equal(B.post[r], others[j][0]) and torch.equal(B.result[r], others[j][1])
    assert not B.post[1].any() and not B.result[1].any()
    assert B.start[1] == P and B.live[1] and B.hook_calls[1] == 0


def test_admit_fused_scope():
    from dflash_amd.batch import BatchedDecoder
    cfg, m, hf, nt, perm = _setup()
    wide = BatchedDecoder(m, nt, 2, max_rows=200, out_len=200, mask_token_id=cfg.mask_token_id, tiles_per_request=2)
    with pytest.raises(NotImplementedError):
        wide.admit_fused(0, _prompt(20, 1))
    dec = BatchedDecoder(m, nt, 2, max_rows=200, out_len=200, mask_token_id=cfg.mask_token_id)
    with pytest.raises(ValueError):
        dec.admit_fused(2, _prompt(20, 1))
    with pytest.raises(ValueError):
        dec.admit_fused(0, _prompt(190, 1))


# ------------------------------------------------------------------------------------------------ the engine, T = 0
def test_refilled_batch_matches_single_request_runs(monkeypatch):
    """Ten requests with their own max_new_tokens and ragged prompts through four slots: ids, acceptance lengths and
    token counts equal each request's dflash_generate run and the greedy walk; 20 group cycles, not the 39 of static
    groups of four."""
    from dflash_amd.engine import dflash_generate_stream
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg, m, hf, nt, perm = _setup()
    prompts, Gs, plans, hooks = _workload(perm)
    singles = _singles(cfg, m, nt, prompts, hooks)
    eng = _engine(cfg, m, nt)
    for i, p in enumerate(prompts):
        eng.submit(p, MAX_NEW[i], draft_token_hook=hooks[i])
    outs = eng.run()
    # the list-in, list-out form: the same engine behind it, sized from the list (three slots here)
    conv = dflash_generate_stream(m, nt, prompts[:6], cfg.mask_token_id, MAX_NEW[:6], 16, None, 0.0, slots=3,
                                  draft_token_hook=lambda i, blk, s, c: hooks[i](blk, s, c))
    for i, (a, b) in enumerate(zip(singles, conv)):
        _same(a, b, f"dflash_generate_stream, request {i}")
    assert [o.request_id for o in outs] == list(range(10))
    for i, (a, b) in enumerate(zip(singles, outs)):
        _same(a, b, f"request {i}")
        assert b.output_ids[0].tolist() == Gs[i][:LENS[i] + MAX_NEW[i]].tolist(), f"request {i}"
        assert b.num_output_tokens == MAX_NEW[i] and b.num_input_tokens == LENS[i]
        assert b.time_to_first_token > 0 and b.time_per_output_token > 0
    cyc = [_plan_cycles(n, plans[i]) for i, n in enumerate(MAX_NEW)]
    assert [len(o.acceptance_lengths) for o in outs] == cyc
    static = sum(max(cyc[g:g + 4]) for g in range(0, 10, 4))
    st = eng.stats
    print("stats", st, "static group cycles", static, "slots", [o.slot for o in outs])
    assert st["group_cycles"] == 20 < static
    assert st["admissions"] == 10 and st["live_slot_cycles"] == sum(cyc)
    assert st["replayed_cycles"] == st["group_cycles"] - 1 and st["captures"] == 1
    # the workload really re-uses slots both ways: long prompt then short one, short then long
    by_slot = {}
    for o in sorted(outs, key=lambda o: o.admitted_step):
        by_slot.setdefault(o.slot, []).append(o.num_input_tokens)
    pairs = [(a, b) for seq in by_slot.values() for a, b in zip(seq, seq[1:])]
    assert any(a >= 100 and b < 16 for a, b in pairs) and any(a < 16 and b >= 64 for a, b in pairs), by_slot


def test_refilled_batch_with_stop_ids(monkeypatch):
    """Stop ids taken from the walks: requests end on a stop at different cycles, their slots are refilled, and every
    output equals the single-request run (cut after the stop id)."""
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg, m, hf, nt, perm = _setup()
    prompts, Gs, plans, hooks = _workload(perm)
    stop = [int(Gs[1][LENS[1] + 50]), int(Gs[3][LENS[3] + 70]), int(Gs[6][LENS[6] + 30])]
    singles = _singles(cfg, m, nt, prompts, hooks, stop=stop)
    eng = _engine(cfg, m, nt, stop_token_ids=stop)
    for i, p in enumerate(prompts):
        eng.submit(p, MAX_NEW[i], draft_token_hook=hooks[i])
    outs = eng.run()
    stopped = []
    for i, (a, b) in enumerate(zip(singles, outs)):
        _same(a, b, f"request {i}")
        new = b.output_ids[0, LENS[i]:].tolist()
        hits = [j for j, x in enumerate(new) if x in stop]
        if hits:
            assert hits == [len(new) - 1], f"request {i}: output not cut after the stop id"
            if len(new) < MAX_NEW[i]:
                stopped.append((i, len(b.acceptance_lengths)))
    assert len(stopped) >= 3 and len({c for _, c in stopped}) >= 3, stopped
    assert {1, 3, 6} <= {i for i, _ in stopped}
    assert eng.stats["admissions"] == 10 and eng.stats["replayed_cycles"] == eng.stats["group_cycles"] - 1


def test_graph_on_and_off_agree_and_capture_once(monkeypatch):
    cfg, m, hf, nt, perm = _setup()
    prompts, Gs, plans, hooks = _workload(perm)
    monkeypatch.setenv("DFL_GRAPH", "0")
    off = _engine(cfg, m, nt)
    assert off.use_graph is False
    for i, p in enumerate(prompts):
        off.submit(p, MAX_NEW[i], draft_token_hook=hooks[i])
    ref = off.run()
    assert off.stats["replayed_cycles"] == 0 and off.dec.graphs is None and off.stats["group_cycles"] == 20

    monkeypatch.setenv("DFL_GRAPH", "1")
    on = _engine(cfg, m, nt)
    assert on.use_graph is True
    on.submit(prompts[0], MAX_NEW[0], draft_token_hook=hooks[0])
    assert on.step() == []                       # the engine's first cycle: eager, then the one capture
    graphs = on.dec.graphs
    held = dict(graphs)
    assert set(held) == {"body", "head", "verify"} and on.stats["captures"] == 1 and on.stats["replayed_cycles"] == 0
    for i in range(1, 10):                       # the second admission comes after the capture
        on.submit(prompts[i], MAX_NEW[i], draft_token_hook=hooks[i])
    got = on.run()
    assert on.dec.graphs is graphs and all(on.dec.graphs[k] is held[k] for k in held)
    assert on.stats["captures"] == 1 and on.stats["admissions"] == 10
    assert on.stats["replayed_cycles"] == on.stats["group_cycles"] - 1
    for i, (a, b) in enumerate(zip(ref, got)):
        _same(a, b, f"request {i}")
        assert b.output_ids[0].tolist() == Gs[i][:LENS[i] + MAX_NEW[i]].tolist()


def test_two_runs_on_one_engine_reuse_caches_and_graphs(monkeypatch):
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg, m, hf, nt, perm = _setup()
    prompts, Gs, plans, hooks = _workload(perm)
    first, second = [0, 1, 2, 3, 4], [5, 6, 7, 8, 9]
    eng = _engine(cfg, m, nt)
    for i in first:
        eng.submit(prompts[i], MAX_NEW[i], draft_token_hook=hooks[i])
    out1 = eng.run()
    dec, graphs, held = eng.dec, eng.dec.graphs, dict(eng.dec.graphs)
    ptrs = [t.data_ptr() for t in (dec.tk, dec.tv, dec.dk, dec.dv, dec.output_ids, dec.d["taps"])]
    for i in second:
        eng.submit(prompts[i], MAX_NEW[i], draft_token_hook=hooks[i])
    out2 = eng.run()
    assert [o.request_id for o in out1] == first and [o.request_id for o in out2] == second
    assert eng.dec is dec and dec.graphs is graphs and all(dec.graphs[k] is held[k] for k in held)
    assert ptrs == [t.data_ptr() for t in (dec.tk, dec.tv, dec.dk, dec.dv, dec.output_ids, dec.d["taps"])]
    assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] == eng.stats["group_cycles"] - 1
    fresh = _engine(cfg, m, nt)
    for i in second:
        fresh.submit(prompts[i], MAX_NEW[i], draft_token_hook=hooks[i])
    ref2 = fresh.run()
    for a, b, i in zip(ref2, out2, second):
        _same(a, b, f"request {i}")
        assert b.output_ids[0].tolist() == Gs[i][:LENS[i] + MAX_NEW[i]].tolist()
    for o, i in zip(out1, first):
        assert o.output_ids[0].tolist() == Gs[i][:LENS[i] + MAX_NEW[i]].tolist()


def test_engine_is_freed_without_a_garbage_collection():
    """Engine, loop and driver form no reference cycle: dropping the engine frees its decoder and hipGraphs at once.
    (Graphs left to the cyclic collector can be destroyed while ANOTHER engine's stream is capturing, which HIP
    refuses and torch turns into an abort; generate.capture_graph pauses the collector for the same reason.)"""
    import gc
    import weakref
    cfg, m, hf, nt, perm = _setup()
    prompts, Gs, plans, hooks = _workload(perm)
    gc.collect()
    gc.disable()
    try:
        eng = _engine(cfg, m, nt, graph=True)
        eng.submit(prompts[2], MAX_NEW[2], draft_token_hook=hooks[2])
        out = eng.run()
        assert eng.stats["captures"] == 1 and out[0].num_output_tokens == MAX_NEW[2]
        refs = [weakref.ref(eng.dec), weakref.ref(eng.dec.graphs["verify"]), weakref.ref(eng.loop)]
        del eng
        assert [r() for r in refs] == [None, None, None]
    finally:
        gc.enable()


# ------------------------------------------------------------------------------------------------ T = 0.7
def _walk_hook(perm, plan, V=2048):
    """tests/test_hip_sampling.py::_hook: drafts scripted from the walk of the block's first token."""
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


def _audit(hf, ids, n_in, seed, gap=0.1, keep=0.90):
    """tests/test_hip_sampling.py::_audit: every emitted token is the target's seeded draw (mirror noise at its
    position) wherever the perturbed top-2 gap exceeds `gap`; at least `keep` of the positions pass the screen."""
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    pos = np.arange(n_in, len(ids))
    exp, gaps = SR.draw(SR.bf16_round(logits[pos - 1]), T, seed, SR.TARGET, pos)
    safe = gaps > gap
    got = np.asarray(ids)[pos]
    print(f"audit: seed {seed} n_in {n_in} positions {len(pos)} kept {safe.mean():.3f}")
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(got[safe], exp[safe]), np.nonzero(got[safe] != exp[safe])
    return got, safe


def _agree_up_to_a_near_tie(a, b, what):
    (ga, sa), (gb, sb) = a, b
    n = min(len(ga), len(gb))
    diff = np.nonzero(ga[:n] != gb[:n])[0]
    if diff.size:   # a divergence may only start at a screened-out near-tie
        assert not (sa[diff[0]] and sb[diff[0]]), (what, diff[0])


def test_sampled_requests_emit_their_own_seeded_draws(monkeypatch):
    """T = 0.7, sampler="device", eight requests through four slots: each passes the teacher-forced audit with its own
    seed and agrees with its single-request run up to the first near-tie; the same request submitted first and
    seventh (another slot, other neighbours, a used slot) passes the same audit."""
    from dflash_amd import dflash_generate
    from dflash_amd.engine import dflash_generate_stream
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg, m, hf, nt, perm = _walk_target()
    lens = [41, 37, 9, 120, 45, 64, 41, 23]
    # (the tiny vocabulary holds the mask id: a request that DRAWS it has that token dropped by the reference's trim,
    # model/dflash.py:269-275, in the single-request run as well, and a teacher-forced pass over the trimmed ids cannot
    # place the positions behind it.  Lengths and seeds are chosen so that no request does; asserted below)
    new = [80, 100, 100, 140, 90, 110, 80, 100]
    pseeds = [3, 4, 5, 6, 7, 8, 3, 9]                # prompt 6 is prompt 0 again
    seeds = [31, 2 ** 63 + 9, 33, 34, 35, 36, 31, 38]
    prompts = [_prompt(P, s) for P, s in zip(lens, pseeds)]
    assert torch.equal(prompts[0], prompts[6])
    plan = H.make_plan(400, 16, 29)
    hook = _walk_hook(perm, plan)
    outs = dflash_generate_stream(m, nt, prompts, cfg.mask_token_id, new, 16, None, T,
                                  draft_token_hook=lambda i, blk, s, c: hook(blk, s, c), sampler="device", seed=seeds)
    assert outs[6].admitted_step > 0 and outs[0].admitted_step == 0   # (the seventh was admitted into a used slot)
    audits = []
    for i, o in enumerate(outs):
        ids = o.output_ids[0].tolist()
        assert len(ids) == lens[i] + new[i] and o.num_output_tokens == new[i], f"request {i} drew the mask id: pick another seed"
        audits.append(_audit(hf, ids, lens[i], seeds[i]))
        single = dflash_generate(m, nt, prompts[i], cfg.mask_token_id, new[i], 16, None, T, draft_token_hook=hook,
                                 sampler="device", seed=seeds[i])
        s_ids = single.output_ids[0].tolist()
        sa = _audit(hf, s_ids, lens[i], seeds[i])
        _agree_up_to_a_near_tie(audits[i], sa, f"request {i} against its single run")
        if np.array_equal(audits[i][0], sa[0]):
            assert list(o.acceptance_lengths) == list(single.acceptance_lengths), f"request {i}"
    _agree_up_to_a_near_tie(audits[0], audits[6], "the same request submitted first and seventh")
    assert max(max(o.acceptance_lengths) for o in outs) > 2   # multi-token acceptance happened
