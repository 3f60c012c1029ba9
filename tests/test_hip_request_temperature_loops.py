"""Per-request temperature through the ragged batch and the slot-refill engine ("Per-request
temperature"): greedy and sampled requests share one decoder, one weight pass and one capture, and each emits what its own
single-request run emits.  Walk target, prompts and hooks of test_hip_stream.py / test_hip_nucleus_loops.py (helpers
copied, with the temperature a parameter)."""
import numpy as np
import pytest
import torch

import helpers as H
import nucleus_ref as NR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_STATE = {}

# The mixed workload: eight requests through four slots.  The sampled (prompt, seed) pairs at T = 0.7 are those of
# test_hip_stream.py::test_sampled_requests_emit_their_own_seeded_draws; request 7 is request 1 again (same prompt, seed
# and T), admitted into a used slot.
TEMPS = [0.0, 0.7, 0.0, 0.5, 0.7, 0.0, 0.5, 0.7]
LENS = [9, 41, 64, 120, 37, 23, 45, 41]
PSEEDS = [5, 3, 8, 6, 4, 9, 7, 3]
SEEDS = [0, 31, 0, 34, 2 ** 63 + 9, 0, 35, 31]
NEW = [100, 80, 110, 140, 100, 100, 90, 80]


def dev():
    return torch.device("cuda", 0)


def _walk_target(scale=0.62):
    """tests/test_hip_stream.py::_walk_target."""
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


def _prompt(P, seed):
    return torch.randint(0, 2000, (1, P), generator=torch.Generator().manual_seed(seed)).to(dev())


def _walk_hook(perm, plan, V=2048):
    """tests/test_hip_stream.py::_walk_hook."""
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


def _audit(hf, ids, n_in, seed, T, gap=0.1, keep=0.90):
    """tests/test_hip_stream.py::_audit with T a parameter: every emitted token is the target's seeded draw at the
    request's own temperature wherever the perturbed top-2 gap exceeds `gap`; at least `keep` of the positions pass."""
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    pos = np.arange(n_in, len(ids))
    exp, gaps = SR.draw(SR.bf16_round(logits[pos - 1]), T, seed, SR.TARGET, pos)
    safe = gaps > gap
    got = np.asarray(ids)[pos]
    print(f"audit: T {T} seed {seed} n_in {n_in} positions {len(pos)} kept {safe.mean():.3f}")
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(got[safe], exp[safe]), np.nonzero(got[safe] != exp[safe])
    return got, safe


def _agree_up_to_a_near_tie(a, b, what):
    (ga, sa), (gb, sb) = a, b
    n = min(len(ga), len(gb))
    diff = np.nonzero(ga[:n] != gb[:n])[0]
    if diff.size:   # a divergence may only start at a screened-out near-tie
        assert not (sa[diff[0]] and sb[diff[0]]), (what, diff[0])


def _plan():
    return H.make_plan(400, 16, 29)


def _single(i, prompts, hook, block=16):
    """Request i's own single-request run at its own temperature."""
    from dflash_amd import dflash_generate
    cfg, m, hf, nt, perm = _walk_target()
    if TEMPS[i] == 0.0:
        return dflash_generate(m, nt, prompts[i], cfg.mask_token_id, NEW[i], block, None, 0.0, draft_token_hook=hook)
    return dflash_generate(m, nt, prompts[i], cfg.mask_token_id, NEW[i], block, None, TEMPS[i], draft_token_hook=hook,
                           sampler="device", seed=SEEDS[i])


def _mixed_engine_run(monkeypatch, graph):
    """The mixed workload through a four-slot engine (made once per graph setting): results and stats."""
    key = ("mixed", graph)
    if key not in _STATE:
        from dflash_amd.engine import BatchEngine
        monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
        cfg, m, hf, nt, perm = _walk_target()
        prompts = [_prompt(P, s) for P, s in zip(LENS, PSEEDS)]
        hook = _walk_hook(perm, _plan())
        need = max(P + n for P, n in zip(LENS, NEW))
        eng = BatchEngine(m, nt, slots=4, max_rows=need + 48, out_len=need + 16, mask_token_id=cfg.mask_token_id,
                          temperature=0.0, sampler="device", request_temperature=True)
        assert eng.use_graph is graph
        for i, p in enumerate(prompts):
            eng.submit(p, NEW[i], seed=SEEDS[i] if TEMPS[i] > 0 else None, draft_token_hook=hook, temperature=TEMPS[i])
        _STATE[key] = (eng.run(), dict(eng.stats), prompts, hook)
    return _STATE[key]


def _check_request(i, out_ids, out_taus, single, hf, n_in, T, seed, what):
    """Greedy: exactly the single run.  Sampled: the audit at its own T and seed, and agreement with the single run up to
    the first near-tie."""
    s_ids = single.output_ids[0].tolist()
    if T == 0.0:
        assert out_ids == s_ids, f"{what}: greedy request {i}"
        assert list(out_taus) == list(single.acceptance_lengths), f"{what}: greedy request {i}"
        return None
    assert len(out_ids) == n_in + NEW[i], f"{what}: request {i} drew the mask id: pick another seed"
    a = _audit(hf, out_ids, n_in, seed, T)
    sa = _audit(hf, s_ids, n_in, seed, T)
    _agree_up_to_a_near_tie(a, sa, f"{what}: request {i} against its single run")
    if np.array_equal(a[0], sa[0]):
        assert list(out_taus) == list(single.acceptance_lengths), f"{what}: request {i}"
    return a


def test_engine_with_mixed_temperatures(monkeypatch):
    """T = [0, 0.7, 0, 0.5, 0.7, 0, 0.5, 0.7] through four slots, replay on: every greedy request equals its
    dflash_generate(T = 0) run exactly (ids and acceptance lengths), every sampled one passes the teacher-forced audit with
    its own seed and T (gap 0.1, at least 0.90 of its positions kept) and agrees with its own single-request run up to the
    first near-tie; request 7, request 1 again admitted into a used slot, agrees with request 1 under the same rule.

    The screen's cap is a condition on the workload, met by the reference alone: the HF target and the numpy mirror over a
    block-size-1 walk per (prompt, seed, T), no kernel of this project involved, keep (gap > 0.1) and never draw the mask id:
        requests 1, 7  (P 41, seed 31, T 0.7, 80 tokens)          0.963
        request 4      (P 37, seed 2^63 + 9, T 0.7, 100 tokens)   0.940
        request 3      (P 120, seed 34, T 0.5, 140 tokens)        1.000
        request 6      (P 45, seed 35, T 0.5, 90 tokens)          1.000
    (lower T only widens the perturbed gaps: T <= 0.7 is the safe side)."""
    cfg, m, hf, nt, perm = _walk_target()
    outs, stats, prompts, hook = _mixed_engine_run(monkeypatch, True)
    assert stats["captures"] == 1 and stats["admissions"] == 8 and stats["replayed_cycles"] == stats["group_cycles"] - 1
    assert outs[7].admitted_step > 0 and outs[1].admitted_step == 0 and torch.equal(prompts[1], prompts[7])
    audits = {}
    for i, o in enumerate(outs):
        audits[i] = _check_request(i, o.output_ids[0].tolist(), o.acceptance_lengths, _single(i, prompts, hook), hf, LENS[i],
                                   TEMPS[i], SEEDS[i], "engine")
    _agree_up_to_a_near_tie(audits[1], audits[7], "the same request submitted second and eighth")
    assert max(max(o.acceptance_lengths) for o in outs) > 2   # multi-token acceptance happened
    # a greedy and a sampled request really shared cycles of one decoder
    assert any(outs[g].admitted_step < outs[s].finished_step and outs[s].admitted_step < outs[g].finished_step
               for g in (0, 2, 5) for s in (1, 3, 4, 6, 7))


def test_graph_on_and_off_agree(monkeypatch):
    """DFL_GRAPH=0 and =1 on the mixed workload: identical ids and acceptance lengths for every request; one capture,
    whose replays span admissions of requests with different temperatures."""
    off, st_off, _, _ = _mixed_engine_run(monkeypatch, False)
    on, st_on, _, _ = _mixed_engine_run(monkeypatch, True)
    assert st_off["replayed_cycles"] == 0 and st_off["captures"] == 0
    assert st_on["captures"] == 1 and st_on["replayed_cycles"] == st_on["group_cycles"] - 1
    for i, (a, b) in enumerate(zip(off, on)):
        assert a.output_ids[0].tolist() == b.output_ids[0].tolist(), f"request {i}"
        assert list(a.acceptance_lengths) == list(b.acceptance_lengths), f"request {i}"
    # admissions after the capture (step 0) brought in both kinds
    late = [i for i, o in enumerate(on) if o.admitted_step > 0]
    assert {TEMPS[i] > 0 for i in late} == {True, False}, late


def test_generate_batch_with_two_tiles_per_request(monkeypatch):
    """dflash_generate_batch(temperature=[0, 0.7]) at block size 24: the greedy prompt equals its T = 0 run, the sampled
    one passes the audit and agrees with its single run up to the first near-tie."""
    from dflash_amd.batch import dflash_generate_batch
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg, m, hf, nt, perm = _walk_target()
    idx = [0, 1]
    prompts = [_prompt(P, s) for P, s in zip(LENS, PSEEDS)]
    hook = _walk_hook(perm, _plan())
    outs = dflash_generate_batch(m, nt, [prompts[i] for i in idx], cfg.mask_token_id, 80, 24, None,
                                 temperature=[TEMPS[i] for i in idx], sampler="device", seed=[SEEDS[i] for i in idx],
                                 draft_token_hook=lambda r, blk, s, c: hook(blk, s, c), hook_block_view=True)
    from dflash_amd import dflash_generate
    for r, i in enumerate(idx):
        kw = dict(sampler="device", seed=SEEDS[i]) if TEMPS[i] > 0 else {}
        single = dflash_generate(m, nt, prompts[i], cfg.mask_token_id, 80, 24, None, TEMPS[i], draft_token_hook=hook, **kw)
        ids = outs[r].output_ids[0].tolist()
        if TEMPS[i] > 0:
            assert len(ids) == LENS[i] + 80, "drew the mask id: pick another seed"
            a = _audit(hf, ids, LENS[i], SEEDS[i], TEMPS[i])
            sa = _audit(hf, single.output_ids[0].tolist(), LENS[i], SEEDS[i], TEMPS[i])
            _agree_up_to_a_near_tie(a, sa, "batch against single, block 24")
        else:
            assert ids == single.output_ids[0].tolist()
            assert list(outs[r].acceptance_lengths) == list(single.acceptance_lengths)


def _bf16_ulp(t):
    return 2.0 ** (np.floor(np.log2(max(abs(float(t)), 1e-30))) - 7)


def _audit_filtered(hf, ids, n_in, seed, T, K, P, gap=0.1, keep=0.85):
    """tests/test_hip_nucleus_loops.py::_audit with T a parameter."""
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


def test_filtering_with_mixed_temperatures(monkeypatch):
    """filtering=True, request_temperature=True: a greedy request with top_k=5 (ignored) and a T = 0.7 request with
    top_k=1 both equal their T = 0 runs; a T = 0.7 request under top_k=20 / top_p=0.9 passes the filtered audit."""
    from dflash_amd import dflash_generate
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg, m, hf, nt, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    prompts = [_prompt(64, 8), _prompt(37, 4), _prompt(41, 3)]
    new = [90, 80, 120]
    eng = BatchEngine(m, nt, slots=3, max_rows=64 + 120 + 48, out_len=64 + 120 + 16, mask_token_id=cfg.mask_token_id,
                      temperature=0.0, sampler="device", filtering=True, request_temperature=True)
    eng.submit(prompts[0], new[0], draft_token_hook=hook, temperature=0.0, top_k=5)
    eng.submit(prompts[1], new[1], seed=12, draft_token_hook=hook, temperature=0.7, top_k=1)
    eng.submit(prompts[2], new[2], seed=5, draft_token_hook=hook, temperature=0.7, top_k=20, top_p=0.9)
    outs = eng.run()
    assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] > 0
    for i in (0, 1):
        g = dflash_generate(m, nt, prompts[i], cfg.mask_token_id, new[i], 16, None, 0.0, draft_token_hook=hook)
        assert outs[i].output_ids[0].tolist() == g.output_ids[0].tolist(), i
        assert list(outs[i].acceptance_lengths) == list(g.acceptance_lengths), i
    ids = outs[2].output_ids[0].tolist()
    assert len(ids) == 41 + new[2], "drew the mask id: pick another seed"
    _audit_filtered(hf, ids, 41, 5, 0.7, 20, 0.9)


@pytest.mark.parametrize("T", [0.0, 0.7])
def test_defaults_change_nothing(T, monkeypatch):
    """request_temperature=False: an engine given the keyword's default and submit(temperature=None | the engine's own)
    emits the ids of an engine built and fed without the new keywords, never reaches the _t entry points, and refuses a
    request temperature of its own."""
    from dflash_amd import ops
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg, m, hf, nt, perm = _walk_target()
    hook = _walk_hook(perm, _plan())
    calls = []
    real_g, real_n = ops.gemm_sample_batch, ops.sample_rows_nucleus
    monkeypatch.setattr(ops, "gemm_sample_batch", lambda *a, **k: (calls.append(k.get("inv_ts")), real_g(*a, **k))[1])
    monkeypatch.setattr(ops, "sample_rows_nucleus", lambda *a, **k: (calls.append(k.get("inv_t")), real_n(*a, **k))[1])
    prompts = [_prompt(41, 3), _prompt(37, 4), _prompt(9, 5)]
    seeds = [31, 2 ** 63 + 9, 33]
    kw = dict(slots=2, max_rows=41 + 60 + 48, out_len=41 + 60 + 16, mask_token_id=cfg.mask_token_id, temperature=T,
              sampler="device")
    runs = []
    for new_kw in (False, True):
        eng = BatchEngine(m, nt, **kw, **(dict(request_temperature=False) if new_kw else {}))
        for i, p in enumerate(prompts):
            extra = dict(temperature=(None, T, None)[i]) if new_kw else {}
            eng.submit(p, 60, seed=seeds[i], draft_token_hook=hook, **extra)
        runs.append(eng.run())
        if new_kw:
            with pytest.raises(ValueError):
                eng.submit(prompts[0], 10, temperature=0.3)
    for a, b in zip(*runs):
        assert a.output_ids[0].tolist() == b.output_ids[0].tolist()
        assert list(a.acceptance_lengths) == list(b.acceptance_lengths)
    assert all(c is None for c in calls) and (len(calls) > 0) == (T > 0)
