"""NativeTarget(hf, weight_format="mxfp4") on the GPU ("The target").  "small": hidden 512,
intermediate 768, four layers (the tiny draft taps layer 1; the last layer cannot be tapped) — the 4-bit skinny form sums in
another fp32 order, so stream and copy are compared within the parity bars.  "wide": hidden 2048, intermediate 4096, two
layers — ceil(K / 512) is 4 or 8 for every K, every wave takes its bf16 counterpart's k-steps: compared bit for bit."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16, T = torch.bfloat16, 0.7
DIMS = {"small": {**H.TINY_TARGET, "num_layers": 4, "intermediate_size": 768},
        "wide": dict(vocab_size=4208, hidden_size=2048, num_layers=2, num_heads=16, num_kv_heads=2, head_dim=128,
                     intermediate_size=4096, rope_theta=1e6)}
NAMES = ("ids", "logits", "taps", "K rows", "V rows")
_S = {}


def _case(name, P=37, seed=4):
    """(hf, mxfp4 NativeTarget over it — which overwrites hf's Linear weights —, prompt, its walk, blocks of 16, 7, 20 rows)"""
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk, make_hf_qwen3
    if name not in _S:
        torch.manual_seed(11)
        hf = make_hf_qwen3(DIMS[name], torch.device("cuda", 0), dtype=BF16)
        _S[name] = (hf, impose_greedy_walk(hf, seed=5), NativeTarget(hf, weight_format="mxfp4"))
    hf, perm, t = _S[name]
    prompt = torch.randint(0, 2000, (1, P), generator=H.gen(seed)).cuda()
    G = greedy_walk(perm, prompt, 120).cuda()
    blocks = [torch.cat([G[P:P + good], torch.randint(0, 2000, (bs - good,), generator=H.gen(bs)).cuda()])
              for bs, good in ((16, 9), (7, 7), (20, 13))]
    return hf, t, prompt, G, blocks


def _verify(t, prompt, block, taps=(1,), **kw):
    """Prefill + one verify on a fresh cache: (ids, logits, tap rows, K rows, V rows of the block), cloned."""
    P, bs = prompt.shape[1], block.numel()
    cache = t.new_cache(P + 64)
    t.prefill(prompt, cache, tap_layers=taps)
    logits = torch.zeros(32, t.V, dtype=BF16, device="cuda")
    post, th = t.verify(block, P, cache, tap_layers=taps, logits_out=logits, **kw)
    return post[0].clone(), logits[:bs].clone(), th[:bs].clone(), cache.k[:, :, P:P + bs].clone(), cache.v[:, :, P:P + bs].clone()


@pytest.mark.parametrize("name", ["small", "wide"])
def test_verify_stream_against_its_bf16_copy(name):
    """mxfp4_stream on against off, greedy and T = 0.7 seeded.  wide: everything EQUAL, seeded ids included.  small: within
    helpers.assert_close's bars (3e-2 / 4e-3 of the scale, K/V 3e-2), ids where the copy's logits have a safe margin.  The
    fused draw is the two-step draw over the launch's own logits."""
    from dflash_amd import ops
    _, t, prompt, _, blocks = _case(name)
    for b in blocks:
        for kw in ({}, dict(temperature=T, seed=21)):
            runs = []
            for t.mxfp4_stream in (True, False):
                runs.append(_verify(t, prompt, b, (0,), **kw))
            t.mxfp4_stream = True
            if name == "wide":
                assert all(torch.equal(x, y) for x, y in zip(*runs)), (b.numel(), kw)
            elif not kw:
                for what, x, y in zip(NAMES[1:], runs[0][1:], runs[1][1:]):
                    H.assert_close(f"mxfp4 target stream vs copy, {b.numel()} rows: {what}", x, y,
                                   **(dict(max_rel=H.KV_MAX_REL) if "rows" in what else {}))
                H.assert_ids_match_where_safe(f"mxfp4 target stream vs copy, {b.numel()} rows", runs[0][0], runs[1][1].float())
            if kw and b.numel() <= 16:
                assert torch.equal(runs[0][0], ops.sample_rows(runs[0][1], seed=21, temperature=T, pos0=prompt.shape[1] + 1))


def test_the_copy_is_a_bf16_target_of_the_overwritten_model_and_the_stream_follows_its_hf_forward():
    from dflash_amd import NativeTarget, ops
    hf, t, prompt, _, blocks = _case("small", 33, 9)
    ntb, P = NativeTarget(hf), prompt.shape[1]
    w = hf.state_dict()["model.layers.1.mlp.down_proj.weight"]
    assert torch.equal(ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(w)), w) and ntb.mxfp4_tensors() == ()
    assert len(t.mxfp4_tensors()) == 4 * t.L + 1
    for b in blocks:
        t.mxfp4_stream = False
        copy = _verify(t, prompt, b)
        t.mxfp4_stream = True
        assert all(torch.equal(x, y) for x, y in zip(copy, _verify(ntb, prompt, b)))
        ids, logits, th, _, _ = _verify(t, prompt, b)
        with torch.inference_mode():
            out = hf(torch.cat([prompt[0], b])[None], output_hidden_states=True)
        ref = out.logits[0, P:P + b.numel()]
        H.assert_close(f"mxfp4 target vs HF forward, {b.numel()} rows: logits", logits, ref)
        H.assert_close(f"mxfp4 target vs HF forward, {b.numel()} rows: tap 1", th, out.hidden_states[2][0, P:P + b.numel()])
        H.assert_ids_match_where_safe(f"mxfp4 target vs HF forward, {b.numel()} rows", ids, ref.float())


@pytest.mark.parametrize("name", ["small", "wide"])
def test_which_launch_receives_an_mxfp4_weight(name, monkeypatch):
    from dflash_amd import ops
    _, t, prompt, _, (b16, b7, b20) = _case(name)
    log, P = [], prompt.shape[1]
    for fn in ("gemm_resid", "gemm_silu_mul", "gemm_argmax", "gemm_sample", "gemm_f32_batch", "gemm_silu_mul_batch",
               "gemm_argmax_batch", "gemm_resid_batch", "prefill_gemm_rows", "prefill_gemm_resid", "prefill_gemm_silu"):
        monkeypatch.setattr(ops, fn, lambda wp, *a, _r=getattr(ops, fn), _n=fn, **kw: (
            log.append((_n, isinstance(wp, ops.Mxfp4Weight))), _r(wp, *a, **kw))[1])
    cache = t.new_cache(160)
    t.prefill(prompt, cache)
    assert log and not any(k[1] for k in log)

    def run(block, **kw):
        del log[:]
        cache.length = P
        t.verify(block, P, cache, **kw)
        return set(log)

    rows = {("gemm_resid", True), ("gemm_silu_mul", True)}
    assert run(b16) == rows | {("gemm_argmax", True)}
    assert run(b7, temperature=T, seed=3) == rows | {("gemm_sample", True)}
    assert run(b16, temperature=T, seed=3, top_k=50) == rows | {("gemm_argmax", True)}      # the materialising head
    # the tile paths: gate/up and the greedy head always, o / down only where the K-part launch takes K; T > 0: a bf16 head
    wide = {("gemm_resid_batch", False), ("gemm_f32_batch", name == "wide"), ("gemm_silu_mul_batch", True)}
    assert run(b20) == wide | {("gemm_argmax_batch", True)}
    assert run(b20, temperature=T, seed=3) == wide | {("gemm_argmax_batch", False)}
    t.wide_one_pass = False
    two_pass = run(b20)
    t.wide_one_pass, t.mxfp4_stream = True, False
    off = run(b16) | run(b20) | run(b16, temperature=T, seed=3)
    t.mxfp4_stream = True
    assert not any(k[1] for k in two_pass | off)


def test_loops_commit_the_quantised_targets_walk_on_one_head(monkeypatch):
    """dflash_generate, eager against replayed, greedy and T = 0.7 seeded, with a bf16 and an mxfp4 draft — which takes the
    target's own 4-bit head, its packer never called; dflash_generate_batch at 4 requests returns the single-request ids."""
    from dflash_amd import DFlashDraftModel, dflash_generate, ops
    from dflash_amd.batch import dflash_generate_batch
    cfg = H.tiny_cfg(num_target_layers=4)
    (_, t, *_), cases = _case("small"), [_case("small", P, 40 + i) for i, P in enumerate((33, 7, 50, 21))]
    prompts, Gs = [c[2] for c in cases], [c[3] for c in cases]
    plan = H.make_plan(64, 16, 17)

    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = Gs[0][start + 1:start + k + 1]

    heads, real = [], ops.gemm_argmax
    monkeypatch.setattr(ops, "gemm_argmax", lambda wp, *a, **kw: (heads.append(wp), real(wp, *a, **kw))[1])
    for fmt in ("bf16", "mxfp4"):
        m = DFlashDraftModel(cfg, device="cuda", weight_format=fmt)
        m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
        monkeypatch.setattr(m, "packed_lm_head_mxfp4", lambda *a, **k: pytest.fail("a second 4-bit head was packed"))
        out = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("DFL_GRAPH", mode)
            out[mode] = dflash_generate(m, t, prompts[0], cfg.mask_token_id, 60, 16, None, 0.0, draft_token_hook=hook)
            assert out[mode].output_ids[0].tolist() == Gs[0][:33 + 60].tolist(), (fmt, mode)
            out["s" + mode] = dflash_generate(m, t, prompts[0], cfg.mask_token_id, 40, 16, None, T, draft_token_hook=hook,
                                              sampler="device", seed=5).output_ids[0].tolist()
        assert out["1"].replayed_cycles > 0 and out["0"].acceptance_lengths == out["1"].acceptance_lengths
        assert out["s0"] == out["s1"]
    w4 = [h for h in heads if isinstance(h, ops.Mxfp4Weight)]
    assert w4 and all(h is t.lm_wp4 for h in w4)
    rs = dflash_generate_batch(m, t, prompts, cfg.mask_token_id, 40, 16, None, 0.0)
    assert all(r.output_ids[0].tolist() == G[:p.shape[1] + 40].tolist() for r, p, G in zip(rs, prompts, Gs))
