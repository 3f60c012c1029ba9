"""One model-level check per odd GQA group, with nothing scripted between the kernels and the comparison: NativeTarget at
(10, 2) (Qwen3 layout) and (6, 2) (Llama layout) against the HF forward, and the DFlashDraftModel forward at (10, 2) —
a single request and a ragged batch of three — against the oracle's plain torch forward on the same weights.  Tiny
widths (hidden 384 / 512, 2 or 3 layers, vocabulary 2048); bars: helpers.assert_close at its defaults, KV_MAX_REL for cache rows.
The only other place a non-power-of-two group ran, test_hidden_5120_runs_through_the_ragged_batch_kernels, overwrites
the drafted tokens by its hook, so a wrong draft attention passed there."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048


def dev():
    return torch.device("cuda", 0)


def _qwen3(heads, layers=3, seed=11):
    from dflash_amd.synthetic import make_hf_qwen3
    torch.manual_seed(seed)
    return make_hf_qwen3({**H.TINY_TARGET, "num_layers": layers, "num_heads": heads[0], "num_kv_heads": heads[1]}, dev(), dtype=BF16)


def _llama(heads, layers=3):
    """hidden 384: HF wants the hidden size a multiple of the head count (6)."""
    tf = pytest.importorskip("transformers")
    cfg = tf.LlamaConfig(vocab_size=V, hidden_size=384, intermediate_size=1024, num_hidden_layers=layers,
                         num_attention_heads=heads[0], num_key_value_heads=heads[1], head_dim=128, rms_norm_eps=1e-5,
                         max_position_embeddings=4096, tie_word_embeddings=False, attention_bias=False, mlp_bias=False,
                         rope_parameters={"rope_type": "default", "rope_theta": 500000.0})
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(3)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        with torch.device(dev()):
            return tf.LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(prev)


@pytest.mark.parametrize("bs", [16, 24])
@pytest.mark.parametrize("family,heads", [("qwen3", (10, 2)), ("llama", (6, 2))], ids=["qwen3-G5", "llama-G3"])
def test_native_target_odd_group_matches_hf_forward(family, heads, bs):
    """prefill (dfl_prefill_qk_rope / dfl_prefill_attn at hq = 1) and verify (dfl_attn_head, one and two query tiles) of a
    G = 5 and a G = 3 target against the HF forward: last-row prefill logits, every verify logit row, two taps, K / V of
    every layer (3 layers: the last one cannot be tapped)."""
    from transformers import DynamicCache
    from dflash_amd import NativeTarget
    hf = _qwen3(heads) if family == "qwen3" else _llama(heads)
    nt = NativeTarget(hf)
    assert (nt.layers[0]["q_norm"] is None) == (family == "llama") and nt.native_prefill and nt.attn_impl == "head"
    Hd = hf.config.hidden_size
    g = torch.Generator().manual_seed(40 + bs + heads[0])
    P, taps, tag = 45, [0, 1], f"{family} ({heads[0]},{heads[1]}) bs {bs}"
    prompt = torch.randint(0, 2000, (1, P), generator=g).to(dev())
    block = torch.randint(0, 2000, (1, bs), generator=g).to(dev())
    cache = nt.new_cache(128)
    out0 = nt.prefill(prompt, cache)
    logits = torch.zeros(32, V, dtype=BF16, device=dev())
    post, th = nt.verify(block[0], P, cache, tap_layers=taps, logits_out=logits)
    rc = DynamicCache()
    with torch.inference_mode():
        ref0 = hf(prompt, past_key_values=rc, use_cache=True)
        ref = hf(block, position_ids=torch.arange(P, P + bs, device=dev())[None], past_key_values=rc, use_cache=True,
                 output_hidden_states=True)
    rl = ref.logits[0].float()
    H.assert_close(f"{tag} prefill logits (last row)", out0.logits[0, -1:], ref0.logits[0, -1:])
    H.assert_close(f"{tag} verify logits", logits[:bs], rl)
    assert post.shape == (1, bs) and torch.equal(post[0], torch.argmax(logits[:bs], dim=-1))
    H.assert_ids_match_where_safe(f"{tag} verify ids", post[0], rl)
    for j, l in enumerate(taps):
        H.assert_close(f"{tag} verify tap {l}", th[:bs, j * Hd:(j + 1) * Hd], ref.hidden_states[l + 1][0])
    for li in range(3):
        H.assert_close(f"{tag} K layer {li}", cache.k[li][:, :P + bs], rc.layers[li].keys[0], max_rel=H.KV_MAX_REL)
        H.assert_close(f"{tag} V layer {li}", cache.v[li][:, :P + bs], rc.layers[li].values[0], max_rel=H.KV_MAX_REL)
    assert cache.get_seq_length() == P + bs


# ---------------------------------------------------------------- the draft at (10, 2)
def _draft_cfg():
    return H.tiny_cfg(num_attention_heads=10, num_key_value_heads=2)


def _draft(cfg):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    assert m.attn_impl == "head"
    return m


def _oracle_logits(cfg, ocache, th, emb, ids, lm, start):
    """The oracle's draft forward on the CPU (bf16, sdpa) over the context rows th and the block ids -> fp32 logits of
    block rows 1.. ."""
    from oracle import dflash_oracle as O
    pos = torch.arange(ocache.get_seq_length(), start + ids.shape[1])[None]
    hid = O.draft_forward(H.draft_weights(cfg, seed=3, dtype=BF16), H.oracle_cfg(cfg, "sdpa"), position_ids=pos,
                          noise_embedding=emb[ids], target_hidden=th, cache=ocache)
    ocache.crop(start)
    return torch.nn.functional.linear(hid[:, 1:], lm).float()[0]


def test_draft_odd_group_matches_oracle():
    """DFlashDraftModel at (10, 2): two draft cycles (a 50-row context through prefill_context + the last 16 rows, then 9
    rows on the grown cache) through draft_block + draft_tokens: the block's logits against the oracle's, ids equal where
    the oracle's margin allows, the draft cache's K / V rows against the oracle's cache."""
    from oracle import dflash_oracle as O
    cfg = _draft_cfg()
    m = _draft(cfg)
    g = torch.Generator().manual_seed(77)
    Hd = cfg.hidden_size
    lm = (torch.randn(V, Hd, generator=g) * 0.05).to(BF16)
    emb = (torch.randn(V, Hd, generator=g) * 0.05).to(BF16)
    P, tau, bs = 50, 9, 16
    steps = [((torch.randn(1, n, cfg.fc_in, generator=g) * 1.5).to(BF16), torch.randint(0, V, (1, bs), generator=g), start)
             for n, start in ((P, P), (tau, P + tau))]
    ocache = O.ListKVCache()
    cache = m.new_cache(256)
    lm_wp = m.packed_lm_head(lm.to(dev()))
    for th, ids, start in steps:
        ref_logits = _oracle_logits(cfg, ocache, th, emb, ids, lm, start)
        ctx = th[0].to(dev())
        S = cache.get_seq_length()
        if ctx.shape[0] > 16:
            head = ctx.shape[0] - 16
            m.prefill_context(cache, ctx[:head], S)
            ctx, S = ctx[head:], S + head
        blk = ids.to(dev()).clone()
        frag = m.draft_block(cache, th_rows=ctx, tau=ctx.shape[0], bs=bs, pos0=S, block_ids=blk[0], embed=emb.to(dev()))
        logits = torch.zeros(16, V, dtype=BF16, device=dev())
        m.draft_tokens(frag, lm_wp, bs, blk[0], logits=logits)
        H.assert_close(f"(10,2) draft logits start {start}", logits[1:bs], ref_logits)
        H.assert_ids_match_where_safe(f"(10,2) draft ids start {start}", blk[0, 1:], ref_logits, min_safe=0)
        for li in range(cfg.num_hidden_layers):
            H.assert_close(f"(10,2) draft K layer {li} start {start}", cache.k[li][:, :start], ocache.k[li][0], max_rel=H.KV_MAX_REL)
            H.assert_close(f"(10,2) draft V layer {li} start {start}", cache.v[li][:, :start], ocache.v[li][0], max_rel=H.KV_MAX_REL)


def test_draft_odd_group_ragged_batch_matches_oracle():
    """The same draft in a ragged batch of R = 3 (prompts of 45, 9 and 70 tokens: dfl_kv_append_batch and
    dfl_attn_head_batch_f32 at (10, 2)) behind a (10, 2) target: after the admissions, ONE batched draft forward whose
    lm_head launch also writes its logits; every request's block logits against the oracle's forward over that request's
    tapped rows and block.  No hook runs: the block ids compared are the kernels' own."""
    from oracle import dflash_oracle as O
    from dflash_amd import NativeTarget
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.generate import _taps
    cfg = _draft_cfg()
    m = _draft(cfg)
    hf = _qwen3((10, 2), layers=cfg.num_target_layers)
    nt = NativeTarget(hf)
    lens = (45, 9, 70)
    prompts = [torch.randint(0, 2000, (1, P), generator=torch.Generator().manual_seed(7 + i)).to(dev()) for i, P in enumerate(lens)]
    dec = BatchedDecoder(m, nt, 3, max_rows=200, out_len=200, mask_token_id=cfg.mask_token_id)
    for r, p in enumerate(prompts):
        dec.admit(r, p)
    # the greedy lm_head launch of the draft writes its logits wherever this buffer is set (the constrained draft's)
    dec._cd_logits = torch.zeros(dec.MT, 16, V, dtype=BF16, device=dev())
    dec.draft()
    torch.cuda.synchronize()
    emb, lm = hf.model.embed_tokens.weight.detach().cpu(), hf.lm_head.weight.detach().cpu()
    for r, (P, p) in enumerate(zip(lens, prompts)):
        out = nt.prefill(p, nt.new_cache(128), output_hidden_states=True, tap_layers=m.target_layer_ids)
        th = _taps(out.hidden_states, m.target_layer_ids).cpu()          # [1, P, fc_in]
        ids = dec.block[r:r + 1].cpu()
        assert int(ids[0, 0]) == int(dec.output_ids[r, P]) and ids.shape == (1, 16)
        start_ids = ids.clone()
        start_ids[0, 1:] = cfg.mask_token_id                             # what the forward embedded
        ref_logits = _oracle_logits(cfg, O.ListKVCache(), th, emb, start_ids, lm, P)
        H.assert_close(f"(10,2) batch draft logits r{r} P{P}", dec._cd_logits[r, 1:16], ref_logits)
        H.assert_ids_match_where_safe(f"(10,2) batch draft ids r{r} P{P}", ids[0, 1:], ref_logits, min_safe=0)
