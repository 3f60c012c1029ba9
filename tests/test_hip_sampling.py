"""Seeded on-device sampling: the Gumbel-max lm_head epilogue and dfl_sample_rows against the
numpy mirror of the generator, the draw's distribution, and the decode loops at T > 0 and with stop ids on the
replayed path — same ids in every launch mode, and every emitted token the target's own seeded draw."""
import numpy as np
import pytest
import torch

import helpers as H
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7


def dev():
    return torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------- kernels
def _gemm_case(V, K, seed=0):
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(seed)
    W = (torch.randn(V, K, generator=g, device=dev()) * 0.02).to(BF16)
    x = torch.randn(16, K, generator=g, device=dev()).to(BF16)
    ref = torch.cat([x.float() @ W[i:i + 32768].float().T for i in range(0, V, 32768)], dim=1)   # fp32 [16, V]
    return ops.pack_weight(W), x, SR.bf16_round(ref.cpu().numpy())


def _check_vs_mirror(ids, ref_bf16, rows, positions, seed, stream=SR.TARGET, extra=0, gap=1e-3, keep=0.95):
    exp, gaps = SR.draw(ref_bf16[rows], T, seed, stream, positions, extra)
    safe = gaps > gap
    assert safe.mean() >= keep, safe.mean()
    got = np.asarray(ids)
    assert np.array_equal(got[safe], exp[safe]), (got[safe] != exp[safe]).sum()


@pytest.mark.parametrize("V", [4208, 128256, 151936])
def test_gemm_sample_matches_the_mirror_and_the_two_step_draw(V):
    """dfl_gemm_sample (positions from a device record, rows row0..) against numpy, and bit-exact against dfl_sample_rows
    over the logits the same GEMM materialises; tile 1 of a two-tile block (pos_add 17) likewise."""
    from dflash_amd import ops
    K = 4096
    wp, x, ref = _gemm_case(V, K, seed=V)
    ws = ops.argmax_ws(dev())
    rec = torch.tensor([0, 0, 16, 1000, 1000, 0, 0, 0], dtype=torch.int32, device=dev())
    for row0, nrows, pos_add, seed in ((0, 16, 1, 5), (1, 15, 0, 2 ** 40 + 7), (0, 16, 17, 11)):
        ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
        logits = torch.zeros(16, V, dtype=BF16, device=dev())
        ops.gemm_sample(wp, ops.rows_plain(x), V, K, row0, nrows, ws, ids, 0, seed=seed, temperature=T, pos_dyn=rec,
                        pos_word=ops.DYN_POS0, pos_add=pos_add, logits=logits)
        two = ops.sample_rows(logits[row0:row0 + nrows], seed=seed, temperature=T, pos0=1000 + pos_add + row0)
        assert torch.equal(ids[:nrows], two)                               # fused == two-step, bit for bit
        rows = np.arange(row0, row0 + nrows)
        _check_vs_mirror(ids[:nrows].cpu().numpy(), ref, rows, 1000 + pos_add + rows, seed)
        if V == 4208:   # host-side position base and the DRAFT stream (extra = base)
            ids2 = torch.full((16,), -1, dtype=torch.int64, device=dev())
            ops.gemm_sample(wp, ops.rows_plain(x), V, K, row0, nrows, ws, ids2, 0, seed=seed, temperature=T,
                            stream=ops.RNG_DRAFT, pos_base=777, pos_add=pos_add)
            _check_vs_mirror(ids2[:nrows].cpu().numpy(), ref, rows, 777 + pos_add + rows, seed, SR.DRAFT, 777)


@pytest.mark.parametrize("R,tpr", [(1, 1), (2, 1), (3, 1), (4, 1), (2, 2), (4, 2)])
def test_gemm_sample_batch_matches_the_two_step_draw_and_the_mirror(R, tpr):
    """dfl_gemm_sample_batch (ring form): R request tiles with ragged row counts, distinct per-request seeds and
    positions from each tile's record; bit-exact against dfl_sample_rows over the logits the same launch materialises
    (tile j of a two-tile request draws 16 j further on), and against the numpy mirror."""
    from dflash_amd import ops
    V, K = 4208, 4096
    g = torch.Generator(device=dev()).manual_seed(10 * R + tpr)
    W = (torch.randn(V, K, generator=g, device=dev()) * 0.02).to(BF16)
    MT = ops.batch_tiles(R)
    x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    bs = [16, 11, 16, 5][:R] if tpr == 1 else [16, 9, 16, 14][:R]
    rec = torch.zeros(MT, 8, dtype=torch.int32)
    for t in range(R):
        rec[t, ops.DYN_BS], rec[t, ops.DYN_POS0] = bs[t], 500 + 97 * (t // tpr)
    rec = rec.to(dev())
    seeds = torch.tensor([ops.seed_i64(s) for s in (3, 2 ** 63 + 5, 77, 1 << 40)][:MT // tpr], dtype=torch.int64,
                         device=dev())
    ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    logits = torch.zeros(MT, 16, V, dtype=BF16, device=dev())
    gws = torch.zeros(ops.lib().dfl_gemm_batch_ws_bytes(V, K), dtype=torch.uint8, device=dev())
    ops.gemm_sample_batch(ops.pack_weight(W), ops.brows_frag(H.frag_of(x)), R, V, K, 0, 16, gws, ids, 0, rec, seeds=seeds,
                          temperature=T, pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=tpr, nrows_dyn_word=ops.DYN_BS,
                          logits=logits)
    ref = SR.bf16_round((x.float() @ W.float().T).cpu().numpy())   # [MT, 16, V]
    for t in range(R):
        q, j, n = t // tpr, t % tpr, bs[t]
        pos0 = 500 + 97 * q + 1 + 16 * j
        sd = int(seeds[q]) & 0xFFFFFFFFFFFFFFFF
        two = ops.sample_rows(logits[t, :n], seed=sd, temperature=T, pos0=pos0)
        assert torch.equal(ids[t, :n], two), t
        assert int((ids[t, n:] != -1).sum()) == 0   # rows past the tile's valid count are not written
        _check_vs_mirror(ids[t, :n].cpu().numpy(), ref[t], np.arange(n), pos0 + np.arange(n), sd)


def test_sample_rows_explicit_positions_and_margins():
    from dflash_amd import ops
    V = 1000   # not a multiple of 4: the last column group is partial
    g = torch.Generator(device=dev()).manual_seed(1)
    logits = (torch.randn(40, V, generator=g, device=dev()) * 2).to(BF16)
    pos = torch.randint(0, 1 << 30, (40,), generator=g, device=dev(), dtype=torch.int64).to(torch.int32)
    marg = torch.zeros(40, dtype=torch.float32, device=dev())
    ids = ops.sample_rows(logits, seed=3, temperature=T, positions=pos, stream=ops.RNG_DRAFT, extra=9, margins=marg)
    exp, gaps = SR.draw(logits.float().cpu().numpy(), T, 3, SR.DRAFT, pos.cpu().numpy(), 9)
    safe = gaps > 1e-3
    assert safe.mean() >= 0.95 and np.array_equal(ids.cpu().numpy()[safe], exp[safe])
    assert np.allclose(marg.cpu().numpy()[safe], gaps[safe], atol=1e-3)


def _chi2(counts, p, top=8):
    idx = np.argsort(-p)[:top]
    n = counts.sum()
    obs = np.concatenate([counts[idx], [n - counts[idx].sum()]]).astype(np.float64)
    exp = np.concatenate([p[idx], [max(1e-12, 1 - p[idx].sum())]]) * n
    keep = exp > 5
    return float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum()), int(keep.sum()) - 1


def test_draws_follow_softmax_of_the_bf16_logits():
    """>= 20k draws from fixed logits with the positions varied, through dfl_sample_rows and through the fused epilogue,
    against the fp32 softmax(bf16 logits / T)."""
    from dflash_amd import ops
    V, K, n = 256, 256, 20480
    g = torch.Generator(device=dev()).manual_seed(4)
    W = (torch.randn(V, K, generator=g, device=dev()) * 0.15).to(BF16)
    x = torch.randn(1, K, generator=g, device=dev()).to(BF16).expand(16, K).contiguous()
    wp = ops.pack_weight(W)
    ws = ops.argmax_ws(dev())
    lg = torch.zeros(16, V, dtype=BF16, device=dev())
    ids = torch.zeros(n, dtype=torch.int64, device=dev())
    for b in range(n // 16):   # fused: 16 rows per launch, positions 16 b ..
        ops.gemm_sample(wp, ops.rows_plain(x), V, K, 0, 16, ws, ids, 16 * b, seed=21, temperature=T, pos_base=16 * b,
                        logits=lg if b == 0 else None)
    two = ops.sample_rows(lg[0:1].expand(n, V).contiguous(), seed=22, temperature=T, pos0=0)
    p = torch.softmax(lg[0].float() / T, dim=0).double().cpu().numpy()
    for draws in (ids, two):
        counts = np.bincount(draws.cpu().numpy(), minlength=V)
        chi2, dof = _chi2(counts, p)
        assert dof >= 4 and chi2 < dof + 6 * np.sqrt(2 * dof), (chi2, dof)


# ---------------------------------------------------------------------------------------------------------- decode loops
_STATE = {}


def _walk_target(scale=0.62):
    """The greedy-walk target (synthetic.impose_greedy_walk) with its lm_head scaled down: the walk's next token keeps
    probability ~0.75 - 0.8 at T = 0.7 instead of ~1, so the draws are genuinely random."""
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


def _hook(perm, plan, V=2048, log=None):
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
            if log is not None:
                log.append(toks[-1])
        if toks:
            blk[0, 1:1 + len(toks)] = torch.tensor(toks, dtype=blk.dtype, device=blk.device)
    return hook


def _script(sizes=(8, 12, 16)):
    """The policy loop over `sizes` with a scripted choice: the EWMA scheduler picks by measured cycle time, which
    differs between launch modes, and the acceptance lengths are compared cycle by cycle."""
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


def _run(kind, monkeypatch, *, graph=True, run_ahead=True, stop=None, temperature=T, sampler="device", seed=1, bs=16,
         n_new=120, native=True, prompt=None, plan_seed=29, log=None, sizes=(8, 12, 16)):
    from dflash_amd import NativeTarget, dflash_generate, dflash_generate_policy
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    monkeypatch.setenv("DFL_RUN_AHEAD", "1" if run_ahead else "0")
    hf, perm = _walk_target()
    cfg = H.tiny_cfg()
    target = NativeTarget(hf) if native else hf
    hook = _hook(perm, H.make_plan(400, 16, plan_seed), log=log)
    prompt = _prompt() if prompt is None else prompt
    if kind == "fixed":
        r = dflash_generate(_draft_model(cfg), target, prompt, cfg.mask_token_id, n_new, bs, stop, temperature,
                            draft_token_hook=hook, sampler=sampler, seed=seed)
    else:
        r = dflash_generate_policy(model=_draft_model(cfg), target=target, input_ids=prompt,
                                   mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, stop_token_ids=stop,
                                   temperature=temperature, scheduler=_script(sizes), draft_token_hook=hook, sampler=sampler,
                                   seed=seed)
    return r.output_ids[0].tolist(), list(r.acceptance_lengths), r.replayed_cycles


def _audit(ids, n_in, seed, gap=0.1, keep=0.90):
    """Teacher-forced: one HF forward over the emitted sequence; every emitted token must be the target's seeded draw
    (mirror noise at its position) wherever the perturbed top-2 gap exceeds `gap`."""
    hf, _ = _walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    pos = np.arange(n_in, len(ids))
    exp, gaps = SR.draw(SR.bf16_round(logits[pos - 1]), T, seed, SR.TARGET, pos)
    safe = gaps > gap
    got = np.asarray(ids)[pos]
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(got[safe], exp[safe]), np.nonzero(got[safe] != exp[safe])
    return got, safe


@pytest.mark.parametrize("kind", ["fixed", "policy"])
def test_launch_modes_give_identical_ids_at_t07(kind, monkeypatch):
    """DFL_GRAPH=0, replay and DFL_RUN_AHEAD=0 at T = 0.7 with the device sampler: the same ids and acceptance lengths;
    the replayed run really replayed."""
    ref = _run(kind, monkeypatch, graph=False)
    rep = _run(kind, monkeypatch, graph=True)
    noahead = _run(kind, monkeypatch, graph=True, run_ahead=False)
    assert rep[:2] == ref[:2] and noahead[:2] == ref[:2]
    assert rep[2] > 0, rep[2]
    assert max(ref[1]) > 2   # multi-token acceptance happened
    got, _ = _audit(ref[0], 41, 1)
    perm = _walk_target()[1]
    walk_hits = np.mean([perm[a] == b for a, b in zip(ref[0][40:-1], ref[0][41:])])
    assert 0.3 < walk_hits < 0.95, walk_hits   # genuinely random draws, not an argmax in disguise


@pytest.mark.parametrize("mode", ["bs16", "bs24", "policy", "policy_wide", "hf_target", "block1", "batch_bs24"])
def test_teacher_forced_audit_is_lossless(mode, monkeypatch):
    if mode == "bs16":
        ids, _, _ = _run("fixed", monkeypatch, seed=5)
    elif mode == "bs24":
        ids, _, _ = _run("fixed", monkeypatch, seed=5, bs=24)
    elif mode == "policy":
        ids, _, _ = _run("policy", monkeypatch, seed=5)
    elif mode == "policy_wide":   # blocks of 20 / 24 rows: the two-tile verify and the sampled two-tile draft
        ids, _, _ = _run("policy", monkeypatch, seed=5, sizes=(12, 20, 24))
    elif mode == "batch_bs24":    # two tiles per request in the ragged batch (a group of one, as hidden > 4096 runs)
        from dflash_amd import NativeTarget
        from dflash_amd.batch import dflash_generate_batch
        hf, perm = _walk_target()
        cfg = H.tiny_cfg()
        hook = _hook(perm, H.make_plan(400, 16, 29))
        ids = dflash_generate_batch(_draft_model(cfg), NativeTarget(hf), [_prompt()], cfg.mask_token_id, 120, 24, None, T,
                                    draft_token_hook=lambda r, blk, start, call: hook(blk, start, call), group_size=1,
                                    sampler="device", seed=[5])[0].output_ids[0].tolist()
    elif mode == "hf_target":
        ids, _, _ = _run("fixed", monkeypatch, seed=5, native=False, n_new=120)
    else:
        ids, _, _ = _run("fixed", monkeypatch, seed=5, bs=1, n_new=120)
    _audit(ids, 41, 5)


def test_batch_requests_emit_their_single_request_draws(monkeypatch):
    """dflash_generate_batch with 3 prompts and a list of seeds, and dflash_generate_policy_batch at T = 0.7: every
    request passes the teacher-forced audit with its own seed, and request i agrees with the single-request run of the
    same seed on the screened positions — the draw does not depend on the group."""
    from dflash_amd import NativeTarget
    from dflash_amd.batch import dflash_generate_batch, dflash_generate_policy_batch
    monkeypatch.setenv("DFL_GRAPH", "1")
    hf, perm = _walk_target()
    cfg = H.tiny_cfg()
    prompts = [_prompt(3, 41), _prompt(4, 37), _prompt(5, 45)]
    seeds = [31, 2 ** 63 + 9, 33]
    plan = H.make_plan(400, 16, 29)
    hook = lambda r, blk, start, call: _hook(perm, plan)(blk, start, call)   # noqa: E731
    outs = dflash_generate_batch(_draft_model(cfg), NativeTarget(hf), prompts, cfg.mask_token_id, 100, 16, None, T,
                                 draft_token_hook=hook, sampler="device", seed=seeds)
    pol = dflash_generate_policy_batch(model=_draft_model(cfg), target=NativeTarget(hf), input_ids=prompts,
                                       mask_token_id=cfg.mask_token_id, max_new_tokens=100, stop_token_ids=None,
                                       temperature=T, schedulers=[_script() for _ in prompts], draft_token_hook=hook,
                                       sampler="device", seed=seeds)
    for i, p in enumerate(prompts):
        n_in = p.shape[1]
        got_b, safe_b = _audit(outs[i].output_ids[0].tolist(), n_in, seeds[i])
        _audit(pol[i].output_ids[0].tolist(), n_in, seeds[i])
        single, _, _ = _run("fixed", monkeypatch, seed=seeds[i], n_new=100, prompt=p)
        got_s, safe_s = _audit(single, n_in, seeds[i])
        diff = np.nonzero(got_b != got_s)[0]
        if diff.size:   # a divergence may only start at a screened-out near-tie
            assert not (safe_b[diff[0]] and safe_s[diff[0]]), (i, diff[0])


def test_speculative_run_emits_what_the_target_alone_emits(monkeypatch):
    """The token at position p is a function of (target, prefix, seed, p): block 16 and block 1 agree wherever the
    draw is not a near-tie in either run."""
    a, _, _ = _run("fixed", monkeypatch, seed=9, n_new=60)
    b, _, _ = _run("fixed", monkeypatch, seed=9, bs=1, n_new=60)
    ga, sa = _audit(a, 41, 9)
    gb, sb = _audit(b, 41, 9)
    first = np.nonzero(ga != gb)[0]
    if first.size:   # a divergence may only start at a screened-out near-tie
        assert not (sa[first[0]] and sb[first[0]])


def _run_stop(kind, monkeypatch, *, graph, temperature, sampler, seed, stop=None, log=None, n_new=240):
    """run_decode as dflash_generate / dflash_generate_policy call it; returns (ids, taus, per-cycle replayed flags)."""
    from dflash_amd import NativeTarget
    from dflash_amd.generate import run_decode
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    hf, perm = _walk_target()
    cfg = H.tiny_cfg()
    hook = _hook(perm, H.make_plan(400, 16, 29), log=log)
    kw = dict(block_size=16, clamp_tail=True, draft_token_hook=hook, sampler=sampler, seed=seed)
    if kind == "policy":
        kw.update(scheduler=_script(), draft_temperature=temperature, max_block_size=16)
    r = run_decode(_draft_model(cfg), NativeTarget(hf), _prompt(), mask_token_id=cfg.mask_token_id, max_new_tokens=n_new,
                   stop_token_ids=stop, temperature=temperature, **kw)
    return r.output_ids[0].tolist(), list(r.acceptance_lengths), list(r.replayed_flags)


@pytest.mark.parametrize("kind", ["fixed", "policy"])
@pytest.mark.parametrize("temperature", [0.0, T])
def test_stop_ids_on_the_replayed_path(kind, temperature, monkeypatch):
    """Stop ids inside an accepted span, as the bonus token, and in a rejected slot (which must not stop): ids,
    acceptance lengths and the stopping cycle equal DFL_GRAPH=0, and the stopping cycle itself was replayed — the stop
    is caught by the captured accept launch."""
    sampler = "device" if temperature > 0 else "torch"
    seed = 13 if temperature > 0 else None
    rejected = []
    free, taus, flags = _run_stop(kind, monkeypatch, graph=True, temperature=temperature, sampler=sampler, seed=seed,
                                  log=rejected)
    n_in = 41
    starts = n_in + np.concatenate([[0], np.cumsum(taus)[:-1]])   # cycle c commits positions starts[c] + 1 .. + taus[c]
    # a replayed cycle (so: far from the tail clamp) that commits >= 3 tokens whose first occurrence is in that cycle
    cands = [c for c in range(4, len(taus)) if flags[c] and taus[c] >= 3
             and free[n_in:].index(free[starts[c] + 2]) + n_in == starts[c] + 2
             and free[n_in:].index(free[starts[c] + taus[c]]) + n_in == starts[c] + taus[c]]
    assert cands, (taus, flags)
    c = cands[len(cands) // 2]
    cases = {"accepted": (free[starts[c] + 2], c), "bonus": (free[starts[c] + taus[c]], c)}
    never = [t for t in rejected if t not in free]
    assert never
    cases["rejected"] = (never[len(never) // 2], None)
    for name, (tok, cyc) in cases.items():
        eager = _run_stop(kind, monkeypatch, graph=False, temperature=temperature, sampler=sampler, seed=seed, stop=[tok])
        rep = _run_stop(kind, monkeypatch, graph=True, temperature=temperature, sampler=sampler, seed=seed, stop=[tok])
        assert rep[:2] == eager[:2], name
        if name == "rejected":
            assert eager[0] == free, name
            assert sum(rep[2]) > 0
        else:
            first = n_in + free[n_in:].index(tok)
            assert eager[0] == free[:first + 1], name
            assert len(rep[1]) == cyc + 1 and rep[2][cyc], (name, cyc, rep[2][-3:])   # the stopping cycle was replayed


def test_seed_semantics(monkeypatch):
    a = _run("fixed", monkeypatch, seed=100, n_new=60)
    b = _run("fixed", monkeypatch, seed=100, n_new=60)
    c = _run("fixed", monkeypatch, seed=101, n_new=60)
    assert a[:2] == b[:2] and a[0] != c[0]
    torch.manual_seed(77)
    d = _run("fixed", monkeypatch, seed=None, n_new=60)
    torch.manual_seed(77)
    e = _run("fixed", monkeypatch, seed=None, n_new=60)
    torch.manual_seed(78)
    f = _run("fixed", monkeypatch, seed=None, n_new=60)
    assert d[0] == e[0] and d[0] != f[0]
