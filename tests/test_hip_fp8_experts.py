"""FP8 (e4m3) expert weights of a sparse-MoE native target on the GPU ("The experts"):
NativeTarget(expert_format="fp8_e4m3") overwrites the wrapped model's expert tensors with q * scale, keeps the packed bf16
copy of that and a twin of codes and scales, and streams the codes in the <= 16-row verify and in the per-tile branch.

Every bar here is bit-equality.  expert_stream = False runs the bf16 expert kernels on the dequantised copy — the very
launches of a plain bf16 NativeTarget over the overwritten model, so the two are equal by plumbing alone.
expert_stream = True replaces exactly two launches per MoE layer, dfl_moe_gate_up and dfl_moe_down, by their W8 forms,
which are bit-equal to them on q * scale for power-of-two scales (tests/test_hip_fp8_experts_kernels.py derives it; the
scales of quantize_fp8_rows are powers of two); every other launch is the same kernel on the same bytes, so ids, logits,
taps, K/V rows and routing weights are equal, and with them every committed id of every loop."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16, U8, F32 = torch.bfloat16, torch.uint8, torch.float32
_S = {}
NAMES = ("ids", "logits", "taps", "K rows", "V rows")


def dev():
    return torch.device("cuda", 0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _moe_hf(layers=4, E=16, top_k=4, Ie=256, mlp_only=(), dtype=BF16, seed=41, norm_topk=True, hidden=512, heads=4, kv=2):
    """tests/test_hip_moe.py::_moe_hf."""
    tf = pytest.importorskip("transformers")
    cfg = tf.Qwen3MoeConfig(vocab_size=2048, hidden_size=hidden, intermediate_size=2 * hidden, moe_intermediate_size=Ie,
                            num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv, head_dim=128,
                            num_experts=E, num_experts_per_tok=top_k, decoder_sparse_step=1, norm_topk_prob=norm_topk,
                            max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=False,
                            rope_parameters={"rope_type": "default", "rope_theta": 1e6}, mlp_only_layers=list(mlp_only))
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device(dev()):
            m = tf.Qwen3MoeForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    with torch.no_grad():   # the default init leaves the router nearly flat: give the routing something to decide
        for layer in m.model.layers:
            if hasattr(layer.mlp, "gate"):
                layer.mlp.gate.weight.mul_(8.0)
    return m.eval()


KINDS = {"tiny": dict(), "dense1": dict(mlp_only=(1,)),
         "a3b": dict(layers=2, E=128, top_k=8, Ie=768, hidden=2048, heads=32, kv=4, seed=43)}


def _case(name):
    """name -> dict(hf, perm, nt8, before, mlp_only): "tiny" — hidden 512, 16 experts of 256, top-4, 4 layers; "dense1"
    — the same with layer 1 dense (`before`: its state dict as it was before construction); "a3b" — two layers at the
    30B-A3B widths, dropped again by the one test that uses it.  The greedy walk is imposed BEFORE the
    target is constructed; the fp8-expert NativeTarget then overwrites hf's expert tensors.  Shared; tests restore
    every switch they flip."""
    if name not in _S:
        from dflash_amd import NativeTarget
        from dflash_amd.synthetic import impose_greedy_walk
        kw = KINDS[name]
        hf = _moe_hf(**kw)
        perm = impose_greedy_walk(hf, seed=5)
        before = {k: v.clone() for k, v in hf.state_dict().items()} if name == "dense1" else None
        nt8 = NativeTarget(hf, expert_format="fp8_e4m3")
        _S[name] = dict(hf=hf, perm=perm, nt8=nt8, before=before, mlp_only=tuple(kw.get("mlp_only", ())))
    return _S[name]


def _draft():
    from dflash_amd import DFlashDraftModel
    cfg = H.tiny_cfg(num_target_layers=4, target_layer_ids=[0, 2])
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, dtype=BF16))
    return cfg, m


def _hook_for(G, plan, vocab=2000):
    """plan[call] tokens of the walk G, then a wrong one."""
    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % vocab, blk[0, k + 1])
    return hook


def _verify(t, prompt, block, taps):
    """Prefill + one verify on a fresh cache: (ids, logits, tap rows, K rows, V rows of the block) and the routing
    weights of every MoE layer, cloned."""
    P, bs = prompt.shape[1], block.numel()
    cache = t.new_cache(P + 64)
    t.prefill(prompt, cache, tap_layers=taps)
    logits = torch.zeros(32, t.V, dtype=BF16, device=dev())
    t.debug_routing = []
    try:
        post, th = t.verify(block, P, cache, tap_layers=taps, logits_out=logits)
        routing = [(i, w.clone()) for i, w in t.debug_routing]
    finally:
        t.debug_routing = None
    return (post[0].clone(), logits[:bs].clone(), th[:bs].clone(), cache.k[:, :, P:P + bs].clone(),
            cache.v[:, :, P:P + bs].clone()), routing


def _spy(monkeypatch, log):
    """ops.moe_gate_up / ops.moe_down -> log of (name, received codes?)."""
    from dflash_amd import ops
    for name in ("moe_gate_up", "moe_down"):
        real = getattr(ops, name)

        def wrapped(w, *a, _real=real, _name=name, **kw):
            log.append((_name, isinstance(w, ops.Fp8Experts)))
            return _real(w, *a, **kw)
        monkeypatch.setattr(ops, name, wrapped)


# ------------------------------------------------------------------------------------------------ the model itself
def test_the_experts_are_overwritten_with_q_times_scale():
    """After construction both expert tensors of every MoE layer of the CALLER'S model hold dequantize(quantize(original))
    over their flat row views; router, norms, attention, the dense layer and the lm_head are untouched; the twin holds
    codes [E, 2 Ie H] / [E, H Ie] uint8 and scales [E, 2 Ie] / [E, H] fp32, the gate/up scales in the packed tile order."""
    from dflash_amd import ops
    c = _case("dense1")
    hf, nt8, before = c["hf"], c["nt8"], c["before"]
    E, Ie, Hd = nt8.E, nt8.Ie, nt8.H
    assert nt8.expert_format == "fp8_e4m3" and nt8.weight_format == "bf16" and nt8.expert_stream and nt8.layers8 is None
    assert [x is None for x in nt8.experts8] == [False, True, False, False]
    changed = 0
    for k, v in hf.state_dict().items():
        if k.endswith("mlp.experts.gate_up_proj") or k.endswith("mlp.experts.down_proj"):
            q, sc = ops.quantize_fp8_rows(before[k].view(-1, before[k].shape[2]))
            assert torch.equal(v, ops.dequantize_fp8_rows(q, sc).view_as(v)), k
            changed += int(not torch.equal(v, before[k]))
            i = int(k.split(".")[2])
            x8 = nt8.experts8[i]["gu_e" if k.endswith("gate_up_proj") else "down_e"]
            if k.endswith("gate_up_proj"):
                assert x8.wp.shape == (E, 2 * Ie * Hd) and x8.wp.dtype == U8 and (x8.E, x8.N, x8.K) == (E, 2 * Ie, Hd)
                s3 = sc.view(E, 2, Ie // 16, 16).permute(0, 2, 1, 3).reshape(E, 2 * Ie)      # (gate tile p, up tile p)
                assert x8.scale.dtype == F32 and torch.equal(x8.scale, s3)
            else:
                assert x8.wp.shape == (E, Hd * Ie) and x8.wp.dtype == U8 and (x8.E, x8.N, x8.K) == (E, Hd, Ie)
                assert x8.scale.dtype == F32 and torch.equal(x8.scale, sc.view(E, Hd))
        else:
            assert torch.equal(v, before[k]), k
    assert changed == 6                                    # three MoE layers, two tensors each, really quantised
    ts = nt8.fp8_tensors()
    assert len(ts) == 3 * 4 and all(t.is_cuda for t in ts)
    assert nt8.layers[1].get("gu_e8") is None and nt8.layers[0]["gu_e8"] is nt8.experts8[0]["gu_e"]


@pytest.mark.parametrize("name", ["tiny", "dense1"])
def test_the_copy_equals_a_bf16_target_of_the_dequantised_weights(name):
    """expert_stream = False against a plain bf16 NativeTarget built afterwards from the same, now overwritten, model:
    ids, logits, taps and K/V rows bit for bit, at 16 and at 11 rows (pure plumbing; the existing MoE tests anchor that
    path to the HF forward)."""
    from dflash_amd import NativeTarget
    c = _case(name)
    t = c["nt8"]
    ntb = NativeTarget(c["hf"])
    assert ntb.expert_format == "bf16" and ntb.experts8 is None and ntb.fp8_tensors() == ()
    prompt = torch.randint(0, 2000, (1, 33), generator=_gen(9)).to(dev())
    t.expert_stream = False
    try:
        for bs in (16, 11):
            block = torch.randint(0, 2000, (bs,), generator=_gen(bs)).to(dev())
            (a, ra), (b, rb) = _verify(t, prompt, block, [0, 2]), _verify(ntb, prompt, block, [0, 2])
            for x, y, what in zip(a, b, NAMES):
                assert torch.equal(x, y), (bs, what)
            assert len(ra) == len(rb) > 0 and all(i == j and torch.equal(x, y) for (i, x), (j, y) in zip(ra, rb))
    finally:
        t.expert_stream = True


@pytest.mark.parametrize("name", ["tiny", "dense1", "a3b"])
def test_verify_stream_equals_its_bf16_copy_bit_for_bit(name, monkeypatch):
    """expert_stream on against off on one target, verify at 16 and at 11 rows: posterior ids, logits_out, taps, the
    cache's K/V rows and debug_routing are torch.equal (module docstring) — on the tiny model, with a dense layer in
    between, and at the 30B-A3B widths (hidden 2048, 32 / 4 heads, 128 experts of 768, top-8; 2 layers).  The spy shows
    who received codes: both expert launches of every MoE layer when streaming, none otherwise; the dense layer has no
    expert launch at all."""
    c = _case(name)
    t = c["nt8"]
    n_moe = t.L - len(c["mlp_only"])
    log = []
    _spy(monkeypatch, log)
    prompt = torch.randint(0, 2000, (1, 37), generator=_gen(4)).to(dev())
    taps = [0] if name == "a3b" else [0, 2]
    try:
        for bs in (16, 11):
            block = torch.randint(0, 2000, (bs,), generator=_gen(100 + bs)).to(dev())
            runs = {}
            for stream in (True, False):
                t.expert_stream = stream
                del log[:]
                runs[stream] = _verify(t, prompt, block, taps)
                assert log == [("moe_gate_up", stream), ("moe_down", stream)] * n_moe, (stream, log)
            (a, ra), (b, rb) = runs[True], runs[False]
            same = [torch.equal(x, y) for x, y in zip(a, b)]
            print(f"[fp8] experts {name}, {bs} rows: bit-identical {dict(zip(NAMES, same))}")
            assert all(same), (bs, dict(zip(NAMES, same)))
            assert len(ra) == len(rb) == n_moe
            assert all(i == j and torch.equal(x, y) for (i, x), (j, y) in zip(ra, rb))
            assert [i for i, _ in ra] == [i for i in range(t.L) if i not in c["mlp_only"]]
    finally:
        t.expert_stream = True
        if name == "a3b":       # (gigabytes of experts: not kept for the rest of the session)
            del _S[name]


def test_per_tile_branch_streams_the_codes_and_the_shared_pass_does_not(monkeypatch):
    """A 20-row verify (two 16-row tiles): with the shared pass pushed out of reach every tile's two expert launches
    receive the codes; with it (the default from two tiles on) no expert launch of the <= 16-row kind runs at all — the
    grouped kernels read the bf16 copy.  Per-tile stream on equals off bit for bit."""
    c = _case("dense1")
    t = c["nt8"]
    log = []
    _spy(monkeypatch, log)
    prompt = torch.randint(0, 2000, (1, 29), generator=_gen(5)).to(dev())
    block = torch.randint(0, 2000, (20,), generator=_gen(6)).to(dev())
    _verify(t, prompt, block, [0, 2])
    assert log == []
    t.moe_shared_min = 99
    try:
        runs = {}
        for stream in (True, False):
            t.expert_stream = stream
            del log[:]
            runs[stream] = _verify(t, prompt, block, [0, 2])[0]
            assert log == [("moe_gate_up", stream), ("moe_down", stream)] * (2 * 3), (stream, log)
        for x, y, what in zip(runs[True], runs[False], NAMES):
            assert torch.equal(x, y), what
    finally:
        t.moe_shared_min = 2
        t.expert_stream = True


# ------------------------------------------------------------------------------------------------ loops
def _script(sizes=(8, 12, 16)):
    """tests/test_hip_sampling.py::_script: the policy loop with a scripted choice of block size."""
    from dflash_amd.generate import _Fixed
    a, b, c = sizes

    class Script(_Fixed):
        def select(self, cyc):
            return (c, a, b, c, b, a)[cyc % 6]

    s = Script(c)
    s.candidates = tuple(sizes)
    return s


@pytest.fixture(scope="module")
def walk():
    from dflash_amd.synthetic import greedy_walk
    c = _case("tiny")
    lens = (30, 47, 12)
    prompts = [torch.randint(0, 2000, (1, P), generator=_gen(60 + i)).to(dev()) for i, P in enumerate(lens)]
    Gs = [greedy_walk(c["perm"], p, 120).to(dev()) for p in prompts]
    return c["nt8"], prompts, Gs


def test_fp8_expert_greedy_loops_stream_on_equals_off(walk, monkeypatch):
    """dflash_generate eager and by graph replay, the policy loop over 8 / 12 / 16 by graph replay (capture_sizes) and a
    stop id, with the codes streamed and with the bf16 copy: the same committed ids and acceptance lengths — the closed-form
    greedy walk imposed on the model before the target was built."""
    from dflash_amd import dflash_generate, dflash_generate_policy
    nt8, prompts, Gs = walk
    cfg, m = _draft()
    n_new, P, G = 60, 30, Gs[0]
    want = G[:P + n_new].tolist()
    hook = _hook_for(G, H.make_plan(64, 16, 17))
    j = next(j for j in range(25, 55) if int(G[P + j]) not in G[:P + j].tolist())   # a stop id at its first occurrence
    runs = {}
    try:
        for stream in (True, False):
            nt8.expert_stream = stream
            for mode in ("0", "1"):
                monkeypatch.setenv("DFL_GRAPH", mode)
                r = dflash_generate(m, nt8, prompts[0], cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=hook)
                assert r.output_ids[0].tolist() == want, (stream, mode)
                assert (r.replayed_cycles > 0) == (mode == "1"), (stream, mode)
                runs[stream, mode] = r
            p = dflash_generate_policy(model=m, target=nt8, input_ids=prompts[0], mask_token_id=cfg.mask_token_id,
                                       max_new_tokens=n_new, stop_token_ids=None, temperature=0.0, scheduler=_script(),
                                       draft_token_hook=hook)
            assert p.output_ids[0].tolist() == want and p.replayed_cycles > 0, ("policy", stream)
            assert set(p.used_block_sizes) >= {8, 12, 16}
            runs[stream, "policy"] = p
            s = dflash_generate(m, nt8, prompts[0], cfg.mask_token_id, n_new, 16, [int(G[P + j])], 0.0, draft_token_hook=hook)
            assert s.output_ids[0].tolist() == G[:P + j + 1].tolist() and s.replayed_cycles > 0, ("stop", stream)
            runs[stream, "stop"] = s
    finally:
        nt8.expert_stream = True
    for k in ("0", "1", "policy", "stop"):
        assert runs[True, k].acceptance_lengths == runs[False, k].acceptance_lengths, k
    assert max(runs[True, "0"].acceptance_lengths) > 8


def test_fp8_expert_wide_block_and_batch_stream_on_equals_off(walk, monkeypatch):
    """A 20-row block (two tiles: the shared pass on the bf16 copy) and dflash_generate_batch with 3 requests (the
    per-tile expert branch per request): stream on and off commit the walk, with the single-request acceptance lengths."""
    from dflash_amd import dflash_generate
    from dflash_amd.batch import dflash_generate_batch
    nt8, prompts, Gs = walk
    cfg, m = _draft()
    n_new = 50
    lens = [p.shape[1] for p in prompts]
    hooks = [_hook_for(Gs[i], H.make_plan(64, 16, 41 + i)) for i in range(3)]
    bh = lambda i, blk, s, c: hooks[i](blk[:, :min(16, lens[i] + n_new - s)], s, c)  # noqa: E731
    log = []
    _spy(monkeypatch, log)
    acc = {}
    try:
        for stream in (True, False):
            nt8.expert_stream = stream
            r = dflash_generate(m, nt8, prompts[0], cfg.mask_token_id, n_new, 20, None, 0.0,
                                draft_token_hook=_hook_for(Gs[0], H.make_plan(64, 20, 23)))
            assert r.output_ids[0].tolist() == Gs[0][:lens[0] + n_new].tolist() and max(r.acceptance_lengths) > 16, stream
            singles = [dflash_generate(m, nt8, prompts[i], cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=hooks[i])
                       for i in range(3)]
            del log[:]
            rs = dflash_generate_batch(m, nt8, prompts, cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=bh)
            for i, (b, s) in enumerate(zip(rs, singles)):
                assert b.output_ids[0].tolist() == s.output_ids[0].tolist() == Gs[i][:lens[i] + n_new].tolist(), (stream, i)
                assert b.acceptance_lengths == s.acceptance_lengths, (stream, i)
            acc[stream] = [r.acceptance_lengths] + [b.acceptance_lengths for b in rs]
            assert all(got == stream for _, got in log)        # whatever expert launch the batch made took this arm's weights
    finally:
        nt8.expert_stream = True
    assert acc[True] == acc[False]


# ------------------------------------------------------------------------------------------------ one copy, keep-alive
def test_keep_hf_false_with_fp8_experts():
    """keep_hf = False: the overwrite happens before the model is dropped; the verify gives the ids and logits of a
    keep_hf = True target over an identical model."""
    from dflash_amd import NativeTarget
    a = NativeTarget(_moe_hf(seed=47), expert_format="fp8_e4m3")
    b = NativeTarget(_moe_hf(seed=47), expert_format="fp8_e4m3", keep_hf=False)
    assert b.hf is None and b.experts8 is not None and a.hf is not None
    prompt = torch.randint(0, 2000, (1, 41), generator=_gen(3)).to(dev())
    block = torch.randint(0, 2000, (16,), generator=_gen(8)).to(dev())
    (ra, _), (rb, _) = _verify(a, prompt, block, [0, 2]), _verify(b, prompt, block, [0, 2])
    for x, y, what in zip(ra, rb, NAMES):
        assert torch.equal(x, y), what


def test_a_decode_session_keeps_the_expert_codes_alive():
    """fp8_tensors() is non-empty and holds every expert code and scale tensor; the record a capture leaves behind keeps
    each of them alive (the graphs hold their raw addresses)."""
    from dflash_amd.generate import DecodeSession
    c = _case("tiny")
    nt8 = c["nt8"]
    ts = nt8.fp8_tensors()
    assert len(ts) == 4 * 4
    want = {t.data_ptr() for l8 in nt8.experts8 for x8 in l8.values() for t in (x8.wp, x8.scale)}
    assert {t.data_ptr() for t in ts} == want and len(want) == 16
    cfg, m = _draft()
    prompt = torch.randint(0, 2000, (1, 30), generator=_gen(60)).to(dev())
    s = DecodeSession(m, nt8, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=48, max_block_size=16,
                      stop_token_ids=None, temperature=0.0)
    s.prefill()
    s.cycle(16, ahead_ok=True)
    s.capture(16)

    def flat(x):
        if isinstance(x, torch.Tensor):
            yield x
        elif isinstance(x, dict):
            for v in x.values():
                yield from flat(v)
        elif isinstance(x, (tuple, list)):
            for v in x:
                yield from flat(v)

    kept = {id(t) for t in flat(s._fixed.keep)}
    assert all(id(t) in kept for t in ts)
    s.cycle_graph(16)
