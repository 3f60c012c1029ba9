"""Prompt logprobs on the GPU: dfl_prefill_logprobs against the fp64 log_softmax of the fp64 product
of the same bf16 operands, and prefill(prompt_logprobs=True) / score / dflash_generate on tiny dense and sparse-MoE targets.

Bars.  Exact family (integer logits, |z| <= 256: the bf16 rounding and the order of the sums cannot matter): the bar of
dfl_logprob_rows on the same row arithmetic, logprobs_ref.tolerance = 2^-16 + 2^-22 |lse|.  randn / model family: each
logit is off by at most 2^-9 |z| (its one bf16 rounding) plus the fp32 accumulation error, out combines two such terms:
|out - ref| <= 2^-8 max|z_ref| + 1e-4.  Every case prints its worst |error| / bar (DESIGN.md records them)."""
import functools

import pytest
import torch

import helpers as H
import logprobs_ref as LR

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
SHAPES = [(15, 256, 256), (17, 4208, 256), (130, 4208, 512), (129, 2048, 4096)]
SENTINEL = -7.0


def dev():
    return torch.device("cuda", 0)


FLAT = (1, 2, 6, 9, 12, 19, 27)   # classes without a peak: integer logits in [-16, 16], the LSE is a real sum over V columns
SPLITS = ["one", "uneven", "default", "all"]


def _cmax(q, V):       # the column of class q's maximum; class 3's sits in the last column block
    return V - 2 if q == 3 else (q * 131 + 7) % V


def _nsplit(split, rows, V):
    """1; 5 strips (33 column blocks: 6 or 7 each, 16: 3 or 4 — strips > 0 of several blocks, c0 / c1 not dividing evenly;
    the 2 blocks of V = 256 allow 2); ops' default; one strip per column block."""
    from dflash_amd import ops
    ncb = (V + 127) // 128
    return dict(one=1, uneven=min(5, ncb), default=ops.prefill_logprobs_nsplit(rows, V), all=ncb)[split]


@functools.lru_cache(maxsize=None)
def _case(rows, V, K, family):
    """(packed W, frag16 rows, targets, fp64 reference [rows], fp64 lse [rows], max |z|), built once per shape.
    exact: z[m][v] = noise (|.| <= 16) + S[v][m % 32], S = 100 (class 8: 230, a single column ~200 above the rest) at
    _cmax, 40 at a column ~60 below it; the classes of FLAT have no S at all, so their LSE is a sum that every column
    counts in (a lost tile shows at the tight bar).  Targets by m % 6: column 0, the last real column, the maximum, the
    column ~60 below it (FLAT: 64 + class columns behind the maximum), -1, V."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(rows + V + K)
    m = torch.arange(rows, device=dev())
    if family == "exact":
        W, X = torch.zeros(V, K, device=dev()), torch.zeros(rows, K, device=dev())
        W[:, :8] = torch.randint(-2, 3, (V, 8), generator=g, device=dev()).float()
        X[:, :8] = torch.randint(-1, 2, (rows, 8), generator=g, device=dev()).float()
        X[m, 16 + m % 32] = 1.0
        for q in set(range(32)) - set(FLAT):
            W[_cmax(q, V), 16 + q] = 230.0 if q == 8 else 100.0
            W[(_cmax(q, V) + 64 + q) % V, 16 + q] = 40.0
    else:
        W, X = torch.randn(V, K, generator=g, device=dev()) * 0.05, torch.randn(rows, K, generator=g, device=dev())
    Wb, Xb = W.to(BF16), X.to(BF16)
    z = Xb.to(F64) @ Wb.to(F64).T
    cm = z.argmax(-1)
    tg = torch.stack([torch.zeros_like(m), torch.full_like(m, V - 1), cm, (cm + 64 + m % 32) % V, torch.full_like(m, -1),
                      torch.full_like(m, V)])[m % 6, m].contiguous()
    lse = torch.logsumexp(z, -1)
    ok = (tg >= 0) & (tg < V)
    ref = torch.where(ok, z.gather(1, tg.clamp(0, V - 1)[:, None])[:, 0] - lse, torch.full_like(lse, float("nan")))
    if family == "exact":
        assert float(z.abs().max()) <= 256 and torch.equal(z, z.round())
        assert abs(float(lse[8] - z[8].max())) < 1e-12 and int(tg[8]) == int(cm[8])   # row 8: the LSE IS its target column
    xf = torch.zeros(ops.prefill_rows_padded(rows) * K, dtype=BF16, device=dev())
    ops.prefill_pack_rows(Xb, rows, K, xf)
    return ops.pack_weight(Wb), xf, tg, ref, lse, float(z.abs().max())


def _launch(wp, xf, rows, V, K, tg, nsplit):
    from dflash_amd import ops
    out = torch.full((rows + 5,), SENTINEL, dtype=F32, device=dev())
    ws = torch.full((nsplit * ops.prefill_rows_padded(rows) * 4,), float("nan"), dtype=F32, device=dev())
    ops.check(ops.lib().dfl_prefill_logprobs(wp.data_ptr(), xf.data_ptr(), rows, V, K, tg.data_ptr(), nsplit, ws.data_ptr(),
                                             out.data_ptr(), torch.cuda.current_stream().cuda_stream), "dfl_prefill_logprobs")
    assert torch.all(out[rows:] == SENTINEL), "rows >= rows written"
    return out[:rows].to(F64)


def _check(name, got, ref, bar):
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), (name, "NaN exactly where the target is outside [0, V)")
    err = (got - ref).abs()[~nan]
    worst = float((err / bar[~nan]).max())
    print(f"[prompt_logprobs] {name}: worst |error| / bar = {worst:.3f} (max |error| {float(err.max()):.3e})")
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("rows,V,K", SHAPES, ids=lambda v: str(v))
def test_kernel_exact_family_matches_fp64(rows, V, K, split):
    wp, xf, tg, ref, lse, _ = _case(rows, V, K, "exact")
    nsplit = _nsplit(split, rows, V)
    got = _launch(wp, xf, rows, V, K, tg, nsplit)
    _check(f"exact {rows}x{V}x{K} nsplit={nsplit}", got, ref, LR.tolerance(lse))


@pytest.mark.parametrize("split", SPLITS)
def test_kernel_randn_k4096_matches_fp64(split):
    rows, V, K = SHAPES[3]
    wp, xf, tg, ref, _, zmax = _case(rows, V, K, "randn")
    nsplit = _nsplit(split, rows, V)
    got = _launch(wp, xf, rows, V, K, tg, nsplit)
    _check(f"randn {rows}x{V}x{K} nsplit={nsplit}", got, ref, torch.full_like(ref, 2.0 ** -8 * zmax + 1e-4))


# ---------------------------------------------------------------- the model path
@functools.lru_cache(maxsize=None)
def _target(kind):
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import make_hf_qwen3
    torch.manual_seed(11)
    if kind == "dense":
        return NativeTarget(make_hf_qwen3({**H.TINY_TARGET, "hidden_size": 256, "num_layers": 2, "vocab_size": 4208}, dev()))
    if kind == "walk":                                                        # the draft of helpers.tiny_cfg fits this one
        return NativeTarget(make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev()))
    import transformers as tf
    cfg = tf.Qwen3MoeConfig(vocab_size=2048, hidden_size=512, intermediate_size=1024, moe_intermediate_size=256,
                            num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                            num_experts=16, num_experts_per_tok=4, decoder_sparse_step=1, norm_topk_prob=True,
                            max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=False,
                            rope_parameters={"rope_type": "default", "rope_theta": 1e6}, mlp_only_layers=[])
    cfg._attn_implementation = "sdpa"
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        with torch.device(dev()):
            hf = tf.Qwen3MoeForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    nt = NativeTarget(hf)
    assert nt.is_moe and nt.native_prefill
    return nt


@pytest.mark.parametrize("P", [2, 17, 130])
@pytest.mark.parametrize("kind", ["dense", "moe"])
def test_prefill_prompt_logprobs_and_score(kind, P):
    from dflash_amd import ops
    nt = _target(kind)
    V, Hd = nt.V, nt.H
    ids = torch.randint(0, V, (1, P), generator=torch.Generator().manual_seed(P)).to(dev())
    c_off, c_on = nt.new_cache(P + 16), nt.new_cache(P + 16)
    off = nt.prefill(ids, c_off, tap_layers=[0])
    on = nt.prefill(ids, c_on, tap_layers=[0], prompt_logprobs=True)
    assert not hasattr(off, "prompt_logprobs") and on.prompt_logprobs.shape == (P - 1,) and on.prompt_logprobs.dtype == F32
    assert torch.equal(on.logits, off.logits) and torch.equal(on.hidden_states[1], off.hidden_states[1])
    assert torch.equal(c_on.k, c_off.k) and torch.equal(c_on.v, c_off.v)
    # the fp64 reference from the prefill's own final-normed rows (the tiles the launch read)
    xn = H.unpack_tiles(nt._pf["xf"][:ops.prefill_rows_padded(P) * Hd], P, Hd).clone()
    hrows = nt._pf["h"][:ops.prefill_rows_padded(P)].clone()
    W = nt.lm_head.weight.detach().to(BF16)
    z = xn[:P - 1].to(F64) @ W.to(F64).T
    ref = (z - torch.logsumexp(z, -1, keepdim=True)).gather(1, ids[0, 1:, None])[:, 0]
    bar = torch.full_like(ref, 2.0 ** -8 * float(z.abs().max()) + 1e-4)
    _check(f"{kind} P={P} prefill", on.prompt_logprobs.to(F64), ref, bar)
    assert torch.equal(nt.score(ids), on.prompt_logprobs)                    # bit for bit
    # the last entry against dfl_logprob_rows on the materialised logits of row P - 2's tile
    t0 = (P - 2) // 16 * 16
    rows = hrows[t0:t0 + 16]
    lg = torch.zeros(16, V, dtype=BF16, device=dev())
    ops.gemm_argmax(nt.lm_wp, ops.rows_normed(rows, rows.float().pow(2).sum(-1).contiguous(), 1, nt.norm, nt.eps), V, Hd, 0, 16,
                    nt.ws["argmax_ws"], torch.zeros(16, dtype=torch.int64, device=dev()), 0, logits=lg)
    sink = ops.logprob_sink(1, 16, 0, dev())
    tok = torch.zeros(16, dtype=torch.int64, device=dev())
    tok[P - 2 - t0] = ids[0, P - 1]
    ops.logprob_rows(lg, tok, sink)
    _check(f"{kind} P={P} last entry vs dfl_logprob_rows", on.prompt_logprobs[-1:].to(F64), sink.lp[0, P - 2 - t0:P - 1 - t0].to(F64),
           bar[:1])


def test_generate_carries_prompt_logprobs():
    from dflash_amd import DFlashDraftModel, dflash_generate
    nt, cfg = _target("walk"), H.tiny_cfg()
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    ids = torch.randint(0, 2000, (1, 41), generator=torch.Generator().manual_seed(3)).to(dev())
    a = dflash_generate(m, nt, ids, cfg.mask_token_id, 24, 16, None, 0.0)
    b = dflash_generate(m, nt, ids, cfg.mask_token_id, 24, 16, None, 0.0, prompt_logprobs=True)
    assert a.prompt_logprobs is None and torch.equal(a.output_ids, b.output_ids)
    assert torch.equal(b.prompt_logprobs, nt.score(ids)) and torch.isfinite(b.prompt_logprobs).all()
