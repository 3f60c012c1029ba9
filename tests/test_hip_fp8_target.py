"""An fp8 (e4m3) native target on the GPU ("The target"): the streamed verify against the same
model's dequantised bf16 copy, against a bf16 NativeTarget of q * scale and against the overwritten HF model; which
launch receives which weight; and the decode loops — single request, policy, ragged batch, engine — committing the
quantised target's own greedy continuation, respectively its own seeded draws.

Two width sets.  "small": hidden 512, intermediate 704 — K % 64 == 0 only; at K = 512 the bf16 skinny GEMM gives a wave
one k-step and the W8 form gives eight waves two each, another fp32 order, so stream and copy are compared within the
project's parity bars.  "wide": every K (1024, 2048) a multiple of 1024, compared bit for bit (derivation at the test)."""
import numpy as np
import pytest
import torch

import helpers as H
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
SMALL = {**H.TINY_TARGET, "num_layers": 6, "intermediate_size": 704}
WIDE = dict(vocab_size=4208, hidden_size=1024, num_layers=2, num_heads=8, num_kv_heads=2, head_dim=128,
            intermediate_size=2048, rope_theta=1e6)
_S = {}


def dev():
    return torch.device("cuda", 0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(name):
    """name -> dict(hf, perm, nt8, dims): a walk target (synthetic.impose_greedy_walk) wrapped by an fp8 NativeTarget —
    which overwrites hf's Linear weights with q * scale.  "soft": the small widths with the lm_head scaled by 0.62
    (test_hip_sampling.py::_walk_target), so that draws at T = 0.7 are genuinely random.  Shared; tests restore every
    switch they flip."""
    if name not in _S:
        from dflash_amd import NativeTarget
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        dims = WIDE if name == "wide" else SMALL
        torch.manual_seed(11)
        hf = make_hf_qwen3(dims, dev(), dtype=BF16)
        perm = impose_greedy_walk(hf, seed=8 if name == "soft" else 5)
        if name == "soft":
            with torch.no_grad():
                hf.lm_head.weight.mul_(0.62)
        before = {k: v.clone() for k, v in hf.state_dict().items() if k.endswith("proj.weight") or k == "lm_head.weight"}
        nt8 = NativeTarget(hf, weight_format="fp8_e4m3")
        _S[name] = dict(hf=hf, perm=perm, nt8=nt8, dims=dims, before=before)
    return _S[name]


def _walk(c, prompt, n):
    from dflash_amd.synthetic import greedy_walk
    return greedy_walk(c["perm"], prompt, n).to(dev())


def _draft(fmt="bf16"):
    from dflash_amd import DFlashDraftModel
    cfg = H.tiny_cfg()
    m = DFlashDraftModel(cfg, device=dev(), weight_format=fmt)
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return cfg, m


def _hook_for(G, plan, vocab=2000):
    """plan[call] tokens of the walk G, then a wrong one (tests/test_hip_fp8_batch_model.py)."""
    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % vocab, blk[0, k + 1])
    return hook


# ------------------------------------------------------------------------------------------------ the model itself
def test_the_wrapped_model_is_overwritten_with_q_times_scale():
    """Every Linear weight of the caller's model holds dequantize(quantize(original)) after construction, norms and the
    (untied) embedding are untouched, target.lm_head.weight is the dequantised head, self.layers is its packed bf16
    copy and layers8 / lm_wp8 hold the codes; a second quantisation of the overwritten head gives the same values."""
    from dflash_amd import ops
    c = _case("small")
    hf, nt8 = c["hf"], c["nt8"]
    sd = hf.state_dict()
    assert nt8.weight_format == "fp8_e4m3" and nt8.fp8_stream is True and len(nt8.layers8) == 6
    changed = 0
    for k, w0 in c["before"].items():
        q, sc = ops.quantize_fp8_rows(w0)
        assert torch.equal(sd[k], ops.dequantize_fp8_rows(q, sc)), k
        changed += int(not torch.equal(sd[k], w0))
    assert changed == len(c["before"]) == 6 * 7 + 1
    assert nt8.lm_head.weight is hf.lm_head.weight
    lw, l8 = nt8.layers[2], nt8.layers8[2]
    assert torch.equal(lw["o"], ops.pack_weight(sd["model.layers.2.self_attn.o_proj.weight"]))
    assert isinstance(l8["o"], ops.Fp8Weight) and (l8["o"].N, l8["o"].K) == (512, 512)
    assert (l8["qkv"].N, l8["gu"].N, l8["gu"].K, l8["down"].K) == (1024, 2 * 704, 512, 704)
    assert torch.equal(l8["qkv"].scale[:512], ops.quantize_fp8_rows(c["before"]["model.layers.2.self_attn.q_proj.weight"])[1])
    assert (nt8.lm_wp8.N, nt8.lm_wp8.K) == (2048, 512) and nt8.lm_wp8.scale.data_ptr() % 64 == 0
    assert lw["ln1"].dtype == BF16 and nt8.embed.dtype == BF16
    assert len(nt8.fp8_tensors()) == 2 * (4 * 6 + 1)
    # one quantised model: the draft's packer over the overwritten head holds the same values as the target's codes
    _, m8 = _draft("fp8_e4m3")
    again = ops.quantize_fp8_rows(hf.lm_head.weight)
    assert torch.equal(ops.dequantize_fp8_rows(*again), hf.lm_head.weight)
    assert m8.packed_lm_head_fp8(nt8.lm_head).N == 2048
    # predicates
    assert nt8.streams_fp8(16) and nt8.streams_fp8(20) and nt8.streams_fp8_tiles()
    nt8.fp8_stream = False
    assert not nt8.streams_fp8(16) and not nt8.streams_fp8_tiles() and nt8.tile_layers(True) is nt8.layers
    nt8.fp8_stream = True
    assert all(isinstance(nt8.tile_layers(True)[0][k], ops.Fp8Weight) for k in ("qkv", "o", "gu", "down"))
    assert isinstance(nt8.tile_layers(False)[0]["qkv"], torch.Tensor)
    assert nt8.tile_layers(False)[2]["ln2"] is lw["ln2"] and nt8.tile_layers(False)[2]["gu"] is l8["gu"]


def test_tied_embeddings_hold_the_dequantised_head():
    from transformers import Qwen3Config, Qwen3ForCausalLM
    from dflash_amd import NativeTarget, ops
    cfg = Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=256, num_hidden_layers=1, num_attention_heads=2,
                      num_key_value_heads=1, head_dim=128, max_position_embeddings=4096, rms_norm_eps=1e-6,
                      rope_parameters={"rope_type": "default", "rope_theta": 1e6}, tie_word_embeddings=True,
                      attention_bias=False)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        torch.manual_seed(3)
        with torch.device(dev()):
            hf = Qwen3ForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    assert hf.lm_head.weight.data_ptr() == hf.model.embed_tokens.weight.data_ptr()
    with torch.no_grad():
        hf.lm_head.weight.mul_(50.0)     # (HF's init std 0.02: spread the rows over more than the subnormal codes)
    w0 = hf.lm_head.weight.detach().clone()
    deq = ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(w0))
    assert not torch.equal(deq, w0)
    nt8 = NativeTarget(hf, weight_format="fp8_e4m3")
    assert torch.equal(hf.model.embed_tokens.weight, deq) and torch.equal(hf.lm_head.weight, deq)
    assert torch.equal(nt8.embed, deq) and torch.equal(nt8.model.embed_tokens.weight, deq)
    assert nt8.streams_fp8(16) and nt8.streams_fp8_tiles()    # (widths of 256: the least the batch W8 forms take)


def _verify(t, prompt, block, taps, **kw):
    """Prefill + one verify on a fresh cache: (ids, logits, tap rows, K rows, V rows of the block), cloned."""
    P, bs = prompt.shape[1], block.numel()
    cache = t.new_cache(P + 64)
    t.prefill(prompt, cache, tap_layers=taps)
    logits = torch.zeros(32, t.V, dtype=BF16, device=dev())
    post, th = t.verify(block, P, cache, tap_layers=taps, logits_out=logits, **kw)
    return (post[0].clone(), logits[:bs].clone(), th[:bs].clone(), cache.k[:, :, P:P + bs].clone(),
            cache.v[:, :, P:P + bs].clone())


def _blocks(c, P=37, seed=4):
    """A prompt and three blocks of its walk (16, 7 and 20 rows; slots past a few walk tokens are random ids)."""
    prompt = torch.randint(0, 2000, (1, P), generator=_gen(seed)).to(dev())
    G = _walk(c, prompt, 40)
    out = []
    for bs, good in ((16, 9), (7, 7), (20, 13)):
        b = G[P:P + bs].clone()
        b[good:] = torch.randint(0, 2000, (bs - good,), generator=_gen(bs)).to(dev())
        out.append(b)
    return prompt, out


NAMES = ("ids", "logits", "taps", "K rows", "V rows")


def test_verify_stream_against_its_bf16_copy_small_widths():
    """fp8_stream on against off, blocks of 16, 7 and 20 rows, greedy and sampled: taps, K/V rows and logits within
    helpers.assert_close's default bars, ids where the copy's logits have a safe margin.  Not bit-identical (K = 512:
    other k-steps per wave in the two skinny forms; K = 704: 22 k-steps, 11 pairs)."""
    from dflash_amd import ops
    c = _case("small")
    t = c["nt8"]
    prompt, blocks = _blocks(c)
    taps = [0, 2, 4]
    for b in blocks:
        runs = []
        for stream in (True, False):
            t.fp8_stream = stream
            runs.append(_verify(t, prompt, b, taps))
        t.fp8_stream = True
        (ia, la, ta, ka, va), (ib, lb, tb, kb, vb) = runs
        n = b.numel()
        H.assert_close(f"fp8 target stream vs copy, {n} rows: logits", la, lb)
        H.assert_close(f"fp8 target stream vs copy, {n} rows: taps", ta, tb)
        H.assert_close(f"fp8 target stream vs copy, {n} rows: K", ka, kb, max_rel=H.KV_MAX_REL)
        H.assert_close(f"fp8 target stream vs copy, {n} rows: V", va, vb, max_rel=H.KV_MAX_REL)
        H.assert_ids_match_where_safe(f"fp8 target stream vs copy, {n} rows", ia, lb.float())
        assert torch.equal(la.float().gather(1, ia[:, None])[:, 0], la.float().amax(-1)), "ids: the maxima of the launch's logits"
        # the sampled head: the fused draw is the two-step draw over the same launch's logits
        s = _verify(t, prompt, b, taps, temperature=T, seed=21)
        assert torch.equal(s[1], la), "the sampled launch materialises the greedy launch's logits"
        assert torch.equal(s[0], ops.sample_rows(s[1], seed=21, temperature=T, pos0=prompt.shape[1] + 1)), n


def test_verify_stream_equals_its_bf16_copy_bit_for_bit_at_k_1024():
    """hidden 1024, q width 1024, intermediate 2048: stream and copy are EQUAL, bit for bit — ids, logits, taps, K/V.
    Derivation.  Single-request kernels (gemm_body): a wave's share is nfr = ceil(KS / 16) k-steps, rounded up to even in
    the W8 form; KS = 32 or 64 gives nfr = 2 or 4 in both, so wave w takes k-steps w * nfr .. in both, accumulates them in
    ascending order through the same MFMA, and the 16 partial sums meet in LDS in wave order in both.  The K-part form
    (k_gemm_b: the 20-row block's o_proj and down_proj): nfr = KS / 8 = 4 or 8, even, the same argument.  The ring form
    (gate/up at KQ = 4: KPC = 2 k-steps of every chunk per wave, one pair; lm_head at KQ = 1): the same k-steps per
    wave by construction.  In every form the W8 sum is the bf16 form's sum of q * scale with the power-of-two scale
    factored out, which commutes with every fp32 rounding (no subnormals at these magnitudes), and is multiplied back in
    front of the first rounding of the epilogue.  q/k/v of the 20-row block reads the bf16 copy in both."""
    from dflash_amd import ops
    c = _case("wide")
    t = c["nt8"]
    assert (t.H, t.q_dim, t.I) == (1024, 1024, 2048) and all(k % 1024 == 0 for k in (t.H, t.q_dim, t.I))
    prompt, blocks = _blocks(c, P=29, seed=6)
    for b in blocks:
        for kw in ({}, dict(temperature=T, seed=5)):
            runs = []
            for stream in (True, False):
                t.fp8_stream = stream
                runs.append(_verify(t, prompt, b, [0], **kw))
            t.fp8_stream = True
            if kw and b.numel() > 16:   # (on the bf16 kernels a wide verify at T > 0 draws from a buffer of its own and
                runs[1] = runs[1][:1] + (greedy_copy_logits,) + runs[1][2:]   # leaves logits_out alone: the greedy run's)
            greedy_copy_logits = runs[1][1]
            same = [torch.equal(x, y) for x, y in zip(*runs)]
            print(f"[fp8] wide target, {b.numel()} rows, {kw or 'greedy'}: bit-identical {dict(zip(NAMES, same))}")
            assert all(same), (b.numel(), kw, dict(zip(NAMES, same)))
            if kw:
                ids, lg = runs[0][0], runs[0][1]
                assert torch.equal(ids, ops.sample_rows(lg, seed=5, temperature=T, pos0=prompt.shape[1] + 1))


@pytest.mark.parametrize("name", ["small", "wide"])
def test_the_copy_equals_a_bf16_target_of_the_dequantised_weights(name):
    """fp8_stream = False against a plain bf16 NativeTarget built from the HF model that now holds q * scale: bit for
    bit — prefill logits, ids, logits, taps, K/V."""
    from dflash_amd import NativeTarget
    c = _case(name)
    t = c["nt8"]
    ntb = NativeTarget(c["hf"])
    assert ntb.weight_format == "bf16" and ntb.layers8 is None and ntb.lm_wp8 is None and ntb.fp8_tensors() == ()
    assert not ntb.streams_fp8(16) and not ntb.streams_fp8_tiles() and ntb.tile_layers(True) is ntb.layers
    prompt, blocks = _blocks(c, P=33, seed=9)
    taps = [0] if name == "wide" else [1, 3]
    t.fp8_stream = False
    try:
        for b in blocks:
            for x, y, what in zip(_verify(t, prompt, b, taps), _verify(ntb, prompt, b, taps), NAMES):
                assert torch.equal(x, y), (b.numel(), what)
        ca, cb = t.new_cache(96), ntb.new_cache(96)
        assert torch.equal(t.prefill(prompt, ca).logits, ntb.prefill(prompt, cb).logits)
    finally:
        t.fp8_stream = True


def test_verify_against_the_overwritten_hf_model():
    """The streamed verify against the wrapped model's own forward (it holds q * scale): logits and tapped hidden rows
    within the default bars, ids where the HF logits have a safe margin; prefill="hf" gives the same first token."""
    from dflash_amd import NativeTarget
    c = _case("small")
    t, hf = c["nt8"], c["hf"]
    prompt, blocks = _blocks(c, P=41, seed=12)
    taps = [0, 2, 4]
    P = prompt.shape[1]
    for b in blocks[:2]:
        ids, logits, th, _, _ = _verify(t, prompt, b, taps)
        with torch.inference_mode():
            out = hf(torch.cat([prompt[0], b])[None], output_hidden_states=True)
        n = b.numel()
        ref = out.logits[0, P:P + n]
        H.assert_close(f"fp8 target vs HF forward, {n} rows: logits", logits, ref)
        H.assert_ids_match_where_safe(f"fp8 target vs HF forward, {n} rows", ids, ref.float())
        for j, l in enumerate(taps):
            H.assert_close(f"fp8 target vs HF forward, {n} rows: tap {l}", th[:, j * t.H:(j + 1) * t.H],
                           out.hidden_states[l + 1][0, P:P + n])
    ca = t.new_cache(96)
    first = t.prefill(prompt, ca).logits.argmax(-1)
    th_ = NativeTarget(hf, prefill="hf", weight_format="fp8_e4m3")     # (a second quantisation: the same values)
    cb = th_.new_cache(96)
    assert torch.equal(th_.prefill(prompt, cb).logits.argmax(-1), first)
    assert torch.equal(th_.lm_head.weight, t.lm_head.weight)


# ------------------------------------------------------------------------------------------------ routing
_SINGLE = ("gemm_resid", "gemm_silu_mul", "gemm_argmax", "gemm_sample", "gemm_f32")
_BATCH = ("gemm_f32_batch", "gemm_silu_mul_batch", "gemm_argmax_batch", "gemm_resid_batch", "gemm_sample_batch")
_PREFILL = ("prefill_gemm_rows", "prefill_gemm_resid", "prefill_gemm_silu")


class _Log(list):
    phase = None

    def kinds(self, phase=None):
        return {(e[1], e[2]) for e in self if phase is None or e[0] == phase}


def _record(monkeypatch, log):
    from dflash_amd import ops
    for name in _SINGLE + _BATCH + _PREFILL:
        real = getattr(ops, name)

        def wrapped(wp, *a, _real=real, _name=name, **kw):
            log.append((log.phase, _name, isinstance(wp, ops.Fp8Weight), wp))
            return _real(wp, *a, **kw)
        monkeypatch.setattr(ops, name, wrapped)


def test_fp8_target_routing(monkeypatch):
    """Which launch receives the codes.  Streamed: every GEMM of verify (q/k/v, o, gate/up, down, greedy / sampled /
    materialising head), of _verify_wide (all but q/k/v as finished rows) and of the batch verify (q/k/v parts
    included), sampled heads too.  The bf16 copy: prefill, attn_impl="fused", fuse_oproj, two-pass wide blocks, the
    candidate loop, and everything with fp8_stream off."""
    from dflash_amd import ops
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.candidates import NativeCandidateVerifier
    c = _case("small")
    t = c["nt8"]
    prompt, (b16, b7, b20) = _blocks(c)
    P, L = prompt.shape[1], t.L
    log = _Log()
    _record(monkeypatch, log)
    cache = t.new_cache(160)
    t.prefill(prompt, cache, tap_layers=[0, 2])
    assert log.kinds() == {(n, False) for n in _PREFILL} | {("gemm_argmax", False)}

    def run(block, **kw):
        del log[:]
        cache.crop(P)
        cache.length = P
        t.verify(block, P, cache, tap_layers=[0, 2], **kw)
        return log.kinds()

    assert run(b16) == {("gemm_resid", True), ("gemm_silu_mul", True), ("gemm_argmax", True)}
    assert [e[1] for e in log].count("gemm_resid") == 3 * L and log[-1][3] is t.lm_wp8
    assert run(b7, temperature=T, seed=3) == {("gemm_resid", True), ("gemm_silu_mul", True), ("gemm_sample", True)}
    assert run(b16, temperature=T, seed=3, top_k=50) == {("gemm_resid", True), ("gemm_silu_mul", True), ("gemm_argmax", True)}
    wide = {("gemm_resid_batch", False), ("gemm_f32_batch", True), ("gemm_silu_mul_batch", True)}
    assert run(b20) == wide | {("gemm_argmax_batch", True)}
    assert run(b20, temperature=T, seed=3) == wide | {("gemm_sample_batch", True)}
    assert run(b20, temperature=T, seed=3, top_p=0.9) == wide | {("gemm_argmax_batch", True)}
    # ---- the bf16 copy
    t.fp8_stream = False
    assert not any(k[1] for k in run(b16) | run(b20) | run(b16, temperature=T, seed=3))
    t.fp8_stream = True
    t.wide_one_pass = False
    assert run(b20) == {("gemm_resid", False), ("gemm_silu_mul", False), ("gemm_argmax", False)}
    t.wide_one_pass = True
    t.fuse_oproj = True
    try:
        assert run(b16) == {("gemm_resid", False), ("gemm_silu_mul", False), ("gemm_argmax", False)}
        t.raise_if_failed()
    finally:
        t.fuse_oproj = False
    t.attn_impl = "fused"
    try:
        assert run(b16) == {("gemm_f32", False), ("gemm_resid", False), ("gemm_silu_mul", False), ("gemm_argmax", False)}
    finally:
        t.attn_impl = "head"
    del log[:]
    cands = torch.stack([b16, b16.roll(1), b16.flip(0)])
    cands[:, 0] = b16[0]
    cache.length = P
    NativeCandidateVerifier(t, 2).verify(cands, P, cache, [0, 2])
    assert log.kinds() and not any(k[1] for k in log.kinds())
    # ---- the ragged batch: a bf16 draft beside the fp8 target
    cfg, m = _draft()
    prompts = [prompt, torch.randint(0, 2000, (1, 21), generator=_gen(6)).to(dev())]

    def cycle(dec):
        del log[:]
        for log.phase, fn in (("draft", dec.draft), ("verify", dec.verify)):
            fn()
        dec.accept()
        return log.kinds("draft"), log.kinds("verify")

    dec = BatchedDecoder(m, t, 2, max_rows=160, out_len=160, mask_token_id=cfg.mask_token_id)
    assert dec.qkv_parts
    for r in range(2):
        dec.admit(r, prompts[r])
    draft, verify = cycle(dec)
    assert not any(k[1] for k in draft)
    assert verify == {("gemm_f32_batch", True), ("gemm_silu_mul_batch", True), ("gemm_argmax_batch", True)}
    assert [e[1] for e in log if e[0] == "verify"].count("gemm_f32_batch") == 3 * L
    t.fp8_stream = False
    assert not any(k[1] for k in cycle(dec)[1])
    t.fp8_stream = True
    for kw, adm in ((dict(temperature=T, sampler="device"), (T, T)),
                    (dict(temperature=T, sampler="device", request_temperature=True), (0.0, T))):
        dec = BatchedDecoder(m, t, 2, max_rows=160, out_len=160, mask_token_id=cfg.mask_token_id, **kw)
        for r in range(2):
            dec.admit(r, prompts[r], adm[r], seed=5 + r)
        _, verify = cycle(dec)
        assert verify == {("gemm_f32_batch", True), ("gemm_silu_mul_batch", True), ("gemm_sample_batch", True)}, kw
    # two tiles per request: q/k/v leaves finished rows (the copy), everything else streams
    dec = BatchedDecoder(m, t, 2, max_rows=200, out_len=200, mask_token_id=cfg.mask_token_id, tiles_per_request=2)
    for r in range(2):
        dec.admit(r, prompts[r])
    _, verify = cycle(dec)
    assert verify == {("gemm_resid_batch", False), ("gemm_f32_batch", True), ("gemm_silu_mul_batch", True),
                      ("gemm_argmax_batch", True)}


# ------------------------------------------------------------------------------------------------ loops, greedy
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
    """The small fp8 target, five ragged prompts and their walks — each checked to BE the quantised target's own greedy
    continuation by one teacher-forced forward of the overwritten HF model."""
    c = _case("small")
    lens = (33, 7, 50, 21, 40)
    prompts = [torch.randint(0, 2000, (1, P), generator=_gen(40 + i)).to(dev()) for i, P in enumerate(lens)]
    Gs = [_walk(c, p, 150) for p in prompts]
    with torch.inference_mode():
        for p, G in zip(prompts, Gs):
            nxt = c["hf"](G[None, :-1]).logits[0].argmax(-1)
            assert torch.equal(nxt[p.shape[1] - 1:], G[p.shape[1]:])
    return c["nt8"], prompts, Gs


def test_fp8_target_greedy_loop_is_lossless_and_replays(walk, monkeypatch):
    """dflash_generate with scripted acceptance on the fp8 target: the committed ids are the quantised target's own
    greedy continuation; DFL_GRAPH=1 equals DFL_GRAPH=0 id for id, with replayed cycles (the captured graphs hold the fp8
    launches); the same under a policy schedule over block sizes 8, 12 and 16, and with a stop id."""
    from dflash_amd import dflash_generate, dflash_generate_policy
    nt8, prompts, Gs = walk
    cfg, m = _draft()
    n_new, P, G = 120, 33, Gs[0]
    want = G[:P + n_new].tolist()
    hook = _hook_for(G, H.make_plan(64, 16, 17))
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DFL_GRAPH", mode)
        r = dflash_generate(m, nt8, prompts[0], cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=hook)
        assert r.output_ids[0].tolist() == want, mode
        runs[mode] = r
        p = dflash_generate_policy(model=m, target=nt8, input_ids=prompts[0], mask_token_id=cfg.mask_token_id,
                                   max_new_tokens=n_new, stop_token_ids=None, temperature=0.0, scheduler=_script(),
                                   draft_token_hook=hook)
        assert p.output_ids[0].tolist() == want, ("policy", mode)
        runs["policy", mode] = p
        j = next(j for j in range(57, 100) if int(G[P + j]) not in G[:P + j].tolist())   # its first occurrence
        s = dflash_generate(m, nt8, prompts[0], cfg.mask_token_id, n_new, 16, [int(G[P + j])], 0.0, draft_token_hook=hook)
        assert s.output_ids[0].tolist() == G[:P + j + 1].tolist(), ("stop", mode)
        runs["stop", mode] = s
    assert runs["1"].replayed_cycles > 0 and runs["0"].replayed_cycles == 0 and runs["policy", "1"].replayed_cycles > 0
    assert runs["stop", "1"].replayed_cycles > 0
    for k in ("", "policy", "stop"):
        a, b = (runs["0"], runs["1"]) if not k else (runs[k, "0"], runs[k, "1"])
        assert a.acceptance_lengths == b.acceptance_lengths, k
    assert max(runs["0"].acceptance_lengths) > 8
    # no hook (random draft weights: nearly every draft token rejected), and a 20-row block run: still the walk
    r = dflash_generate(m, nt8, prompts[0], cfg.mask_token_id, 40, 16, None, 0.0)
    assert r.output_ids[0].tolist() == G[:P + 40].tolist()
    r = dflash_generate(m, nt8, prompts[0], cfg.mask_token_id, 70, 20, None, 0.0,
                        draft_token_hook=_hook_for(G, H.make_plan(64, 20, 23)))
    assert r.output_ids[0].tolist() == G[:P + 70].tolist() and max(r.acceptance_lengths) > 16


def test_fp8_target_with_fp8_draft_shares_one_head(walk, monkeypatch):
    """fp8 target and fp8 draft: lossless, and ONE e4m3 copy of the lm_head serves both — the draft's greedy unmask is
    launched with the target's own code tensor and the draft's packer is never called."""
    from dflash_amd import dflash_generate, ops
    from dflash_amd.batch import dflash_generate_batch
    nt8, prompts, Gs = walk
    cfg, m8 = _draft("fp8_e4m3")
    calls = []
    real = m8.packed_lm_head_fp8
    monkeypatch.setattr(m8, "packed_lm_head_fp8", lambda *a, **k: calls.append(1) or real(*a, **k))
    log = _Log()
    _record(monkeypatch, log)
    monkeypatch.setenv("DFL_GRAPH", "0")
    hook = _hook_for(Gs[0], H.make_plan(64, 16, 17))
    r = dflash_generate(m8, nt8, prompts[0], cfg.mask_token_id, 60, 16, None, 0.0, draft_token_hook=hook)
    assert r.output_ids[0].tolist() == Gs[0][:33 + 60].tolist()
    heads = [e[3] for e in log if e[1] == "gemm_argmax" and e[2]]
    assert heads and all(h.wp is nt8.lm_wp8.wp and h.scale is nt8.lm_wp8.scale for h in heads)
    del log[:]
    rs = dflash_generate_batch(m8, nt8, prompts[:2], cfg.mask_token_id, 40, 16, None, 0.0)
    for i, r in enumerate(rs):
        assert r.output_ids[0].tolist() == Gs[i][:prompts[i].shape[1] + 40].tolist(), i
    heads = [e[3] for e in log if e[1] == "gemm_argmax_batch"]
    assert heads and all(isinstance(h, ops.Fp8Weight) and h.wp is nt8.lm_wp8.wp for h in heads)
    assert not calls


def test_fp8_target_batch_and_engine_return_the_single_request_ids(walk):
    """dflash_generate_batch with three ragged requests and BatchEngine under refill (five requests, three slots), replay
    on and off: every request returns what its own single-request run returns — the quantised target's walk — with the
    single run's acceptance lengths."""
    from dflash_amd import dflash_generate
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import BatchEngine
    nt8, prompts, Gs = walk
    cfg, m = _draft()
    n_new = [60, 45, 70, 30, 50]
    lens = [p.shape[1] for p in prompts]
    hooks = [_hook_for(Gs[i], H.make_plan(64, 16, 17 + i)) for i in range(5)]
    single = [dflash_generate(m, nt8, prompts[i], cfg.mask_token_id, 60, 16, None, 0.0, draft_token_hook=hooks[i])
              for i in range(3)]
    bh = lambda i, blk, s, c: hooks[i](blk[:, :min(16, lens[i] + 60 - s)], s, c)  # noqa: E731
    rs = dflash_generate_batch(m, nt8, prompts[:3], cfg.mask_token_id, 60, 16, None, 0.0, draft_token_hook=bh)
    for i, (r, s) in enumerate(zip(rs, single)):
        assert r.output_ids[0].tolist() == s.output_ids[0].tolist() == Gs[i][:lens[i] + 60].tolist(), i
        assert r.acceptance_lengths == s.acceptance_lengths, i
    outs = {}
    for graph in (False, True):
        eng = BatchEngine(m, nt8, slots=3, max_rows=50 + 70 + 48, out_len=50 + 70 + 16, mask_token_id=cfg.mask_token_id,
                          graph=graph)
        for i, p in enumerate(prompts):
            eng.submit(p, n_new[i], draft_token_hook=hooks[i])
        res = eng.run()
        assert (eng.stats["replayed_cycles"] > 0) == graph and eng.stats["admissions"] == 5
        for i, r in enumerate(res):
            assert r.output_ids[0].tolist() == Gs[i][:lens[i] + n_new[i]].tolist(), (graph, i)
        outs[graph] = res
    for a, b in zip(outs[False], outs[True]):
        assert a.acceptance_lengths == b.acceptance_lengths


# ------------------------------------------------------------------------------------------------ loops, T > 0
def _soft_hook(perm, plan, V=2048):
    """tests/test_hip_sampling.py::_hook: plan[call] tokens of the walk of the block's first token, then a wrong one."""
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


def _audit(hf, ids, n_in, seed, temperature=T, gap=0.1, keep=0.90):
    """tests/test_hip_sampling.py::_audit (its gap and keep) over the fp8 target's logits — one forward of the HF model
    that holds q * scale: every emitted token is that model's seeded draw wherever the perturbed top-2 gap exceeds gap."""
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    pos = np.arange(n_in, len(ids))
    exp, gaps = SR.draw(SR.bf16_round(logits[pos - 1]), temperature, seed, SR.TARGET, pos)
    safe = gaps > gap
    got = np.asarray(ids)[pos]
    print(f"[fp8] audit: T {temperature} seed {seed} positions {len(pos)} kept {safe.mean():.3f}")
    assert safe.mean() >= keep, safe.mean()
    assert np.array_equal(got[safe], exp[safe]), np.nonzero(got[safe] != exp[safe])
    return got, safe


def _prompt(seed=3, n=41):
    return torch.randint(0, 2000, (1, n), generator=_gen(seed)).to(dev())


@pytest.mark.parametrize("bs", [16, 24])
def test_fp8_target_sampled_loop_passes_the_teacher_forced_audit(bs, monkeypatch):
    """T = 0.7, sampler="device", the walk target with the softened head: every emitted token is the fp8 target's own
    seeded draw (audit of test_hip_sampling.py, gap 0.1, keep 0.90); replay equals eager id for id; the draws are
    random, not an argmax in disguise.  bs = 24: the two-tile verify, whose head is the sampled e4m3 ring."""
    from dflash_amd import dflash_generate
    c = _case("soft")
    perm = c["perm"].cpu().tolist()
    cfg, m = _draft()
    hook = _soft_hook(perm, H.make_plan(400, 16, 29))
    outs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DFL_GRAPH", mode)
        r = dflash_generate(m, c["nt8"], _prompt(), cfg.mask_token_id, 120, bs, None, T, draft_token_hook=hook,
                            sampler="device", seed=5)
        outs[mode] = r
    ids = outs["0"].output_ids[0].tolist()
    assert outs["1"].output_ids[0].tolist() == ids and outs["0"].acceptance_lengths == outs["1"].acceptance_lengths
    assert bs > 16 or outs["1"].replayed_cycles > 0
    assert max(outs["0"].acceptance_lengths) > 2
    _audit(c["hf"], ids, 41, 5)
    hits = np.mean([perm[a] == b for a, b in zip(ids[40:-1], ids[41:])])
    assert 0.3 < hits < 0.95, hits


def test_fp8_target_mixed_temperatures_in_one_batch(monkeypatch):
    """One greedy and two sampled requests (T = 0.7, 0.5) in one ragged batch on the fp8 target, per-request temperature:
    the greedy one returns exactly its single-request run, the sampled ones pass the audit at their own T and seed and
    agree with their single runs up to the first near-tie."""
    from dflash_amd import dflash_generate
    from dflash_amd.batch import dflash_generate_batch
    monkeypatch.setenv("DFL_GRAPH", "1")
    c = _case("soft")
    nt8, perm = c["nt8"], c["perm"].cpu().tolist()
    cfg, m = _draft()
    temps, seeds, lens, pseeds = [0.0, 0.7, 0.5], [0, 31, 34], [23, 41, 37], [9, 3, 6]
    prompts = [_prompt(s, n) for s, n in zip(pseeds, lens)]
    hook = _soft_hook(perm, H.make_plan(400, 16, 29))
    rs = dflash_generate_batch(m, nt8, prompts, cfg.mask_token_id, 90, 16, None, temps,
                               draft_token_hook=lambda i, blk, s, cyc: hook(blk, s, cyc), hook_block_view=True,
                               sampler="device", seed=seeds)
    for i, r in enumerate(rs):
        ids = r.output_ids[0].tolist()
        if temps[i] == 0.0:
            s = dflash_generate(m, nt8, prompts[i], cfg.mask_token_id, 90, 16, None, 0.0, draft_token_hook=hook)
            assert ids == s.output_ids[0].tolist() and r.acceptance_lengths == s.acceptance_lengths
            continue
        s = dflash_generate(m, nt8, prompts[i], cfg.mask_token_id, 90, 16, None, temps[i], draft_token_hook=hook,
                            sampler="device", seed=seeds[i])
        assert len(ids) == lens[i] + 90
        (ga, sa), (gb, sb) = _audit(c["hf"], ids, lens[i], seeds[i], temps[i]), _audit(c["hf"], s.output_ids[0].tolist(),
                                                                                      lens[i], seeds[i], temps[i])
        n = min(len(ga), len(gb))
        diff = np.nonzero(ga[:n] != gb[:n])[0]
        if diff.size:   # a divergence may only start at a screened-out near-tie
            assert not (sa[diff[0]] and sb[diff[0]]), (i, diff[0])
