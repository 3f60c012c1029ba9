"""GPU parity of the host-side mirror (DFlashDraftModel.forward / spec_generate,
dflash_generate, dflash_generate_policy) against the reference-generated golden
vectors and the oracle."""
import json
import os

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
E2E = json.load(open(os.path.join(H.GOLDEN, "e2e.json")))


def dev():
    return torch.device("cuda", 0)


def make_model(cfg, seed=3):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=seed, dtype=BF16))
    return m


# Draft hidden states vs the reference's bf16 output.  Tolerance: the
# reference's own bf16 backends differ from fp32 and from each other by ~2e-2 abs at
# unit-scale outputs; we require max-abs <= 4e-2 of the output scale against the bf16
# golden and a mean-abs an order of magnitude below that.
@pytest.mark.parametrize("tag,cfgf", [("tiny_bf16_eager", H.tiny_cfg), ("tiny_bf16_sdpa", H.tiny_cfg),
                                      ("mid_bf16_sdpa", H.mid_cfg),
                                      ("tiny_bf16_sdpa_wide", H.tiny_cfg)])   # blocks of 17..32 rows (golden G8)
def test_forward_matches_reference_vectors(tag, cfgf):
    z = np.load(os.path.join(H.GOLDEN, f"draft_forward_{tag}.npz"))
    cfg = cfgf()
    m = make_model(cfg)
    cache = m.new_cache(int(z["prompt_len"]) + 200)
    g, ctx_rows = torch.Generator().manual_seed(int(z["seed"])), int(z["prompt_len"])   # the generator's inputs
    for c, (bs, tau_next) in enumerate(z["steps"].tolist()):
        start = int(z[f"start{c}"])
        th, ne = (t.to(dev()) for t in H.draft_forward_inputs(cfg, BF16, g, ctx_rows, bs))
        ctx_rows = tau_next
        pos = torch.arange(cache.get_seq_length(), start + bs, device=dev()).unsqueeze(0)
        hid = m(target_hidden=th, noise_embedding=ne, position_ids=pos, past_key_values=cache, use_cache=True,
                is_causal=False)
        cache.crop(start)
        H.assert_close(f"{tag} hidden cycle {c}", hid, torch.from_numpy(z[f"hid{c}"]))
    n = cache.get_seq_length()
    for li in (0, cfg.num_hidden_layers - 1):
        for name, buf in (("k", cache.k), ("v", cache.v)):
            ref = torch.from_numpy(z[f"{name}_l{li}"])[0]          # [kv, n, 128]
            assert ref.shape[1] == n
            H.assert_close(f"{tag} cache {name} layer {li}", buf[li][:, :n], ref, max_rel=H.KV_MAX_REL)


def ops_pack(w):
    from dflash_amd import ops
    return ops.pack_weight(w)


def _scripted(g, cfg, dtype=BF16):
    base = H.tiny_target(dtype=dtype, device=dev())
    total = len(g["prompt"]) + g["max_new_tokens"]
    tape = H.make_tape(total + 64, cfg.vocab_size, g["tape_seed"], forbid=(cfg.mask_token_id,))
    t = H.ScriptedTarget(base, tape, H.make_plan(64, cfg.block_size, g["plan_seed"]))
    t.script_lm_head = False   # the product takes the real lm_head weight; agreement comes via the hook
    return t


def test_spec_generate_matches_reference_ids():
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    for key in ("spec", "spec_stop"):
        g = E2E[f"bf16_sdpa/{key}"]
        tgt = _scripted(g, cfg)
        ids = m.spec_generate(target=tgt, input_ids=torch.tensor([g["prompt"]], device=dev()),
                              max_new_tokens=g["max_new_tokens"], stop_token_ids=g.get("stop_token_ids"),
                              temperature=0.0, draft_token_hook=tgt.draft_token_hook)
        assert ids[0].tolist() == g["ids"], key
        assert [v["acc"] for v in tgt.verify_log] == [v["acc"] for v in g["verify"]]
        assert [v["start"] for v in tgt.verify_log] == [v["start"] for v in g["verify"]]


def test_dflash_generate_matches_reference_ids():
    from dflash_amd import dflash_generate
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    for key in ("gen_bs1", "gen_bs12", "gen_bs16", "gen_steps2"):
        g = E2E[f"bf16_sdpa/{key}"]
        tgt = _scripted(g, cfg)
        r = dflash_generate(m, tgt, torch.tensor([g["prompt"]], device=dev()), cfg.mask_token_id,
                            g["max_new_tokens"], g["block_size"], None, 0.0, collect_profile=(key == "gen_bs16"),
                            draft_steps=g["draft_steps"], draft_token_hook=tgt.draft_token_hook)
        assert r.output_ids[0].tolist() == g["ids"], key
        assert r.acceptance_lengths == g["acceptance_lengths"], key
        assert r.num_output_tokens == g["num_output_tokens"]
        if key == "gen_bs16":
            ps = r.profile_summary
            assert ps["profiled_cycles"] == len(g["acceptance_lengths"])
            assert ps["draft_decode_s"] > 0 and ps["target_decode_s"] > 0
            assert abs(ps["draft_share_decode"] + ps["target_share_decode"] - 1.0) < 1e-6


class _Replay:
    """Scheduler stand-in replaying the block sizes the reference's scheduler chose
    (they depend on wall-clock there)."""

    def __init__(self, chosen, candidates):
        self.chosen, self.candidates = chosen, candidates
        self.tau_hat, self.cycle_hat, self.score_hat = {}, {}, {}
        self.current = self.adl_target_k = self.adl_target_bs = max(candidates)
        self.adl_lgen_hat = self.adl_lacc_hat = None
        self.updates = []

    def select(self, cyc):
        return self.chosen[min(cyc, len(self.chosen) - 1)]

    def update(self, **kw):
        self.updates.append(kw)


def test_dflash_generate_policy_matches_reference_ids():
    from dflash_amd import dflash_generate_policy
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    g = E2E["bf16_sdpa/policy"]
    tgt = _scripted(g, cfg)
    sch = _Replay(g["chosen_block_sizes"], [8, 12, 16])
    r = dflash_generate_policy(model=m, target=tgt, input_ids=torch.tensor([g["prompt"]], device=dev()),
                               mask_token_id=cfg.mask_token_id, max_new_tokens=g["max_new_tokens"],
                               stop_token_ids=g["stop_token_ids"], temperature=0.0, scheduler=sch,
                               draft_token_hook=tgt.draft_token_hook)
    assert r.output_ids[0].tolist() == g["ids"]
    assert r.acceptance_lengths == g["acceptance_lengths"]
    assert r.used_block_sizes == g["used_block_sizes"]
    assert [u["l_gen"] for u in sch.updates] == g["l_gen"]
    assert [t["chosen_block_size"] for t in r.cycle_trace] == g["chosen_block_sizes"]


def test_natural_run_is_lossless_on_gpu():
    """No scripting: whatever the draft proposes, the committed ids are the target's own
    greedy continuation (fp32 target so near-ties cannot flip between a 1-token and a
    16-token forward)."""
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    g = E2E["f32_eager/natural"]
    tgt = H.tiny_target(dtype=torch.float32, device=dev())
    prompt = torch.tensor([g["prompt"]], device=dev())
    ids = m.spec_generate(target=tgt, input_ids=prompt, max_new_tokens=g["max_new_tokens"], stop_token_ids=None,
                          temperature=0.0)
    cache = tgt.new_cache()
    ar = prompt.clone()
    out = tgt(ar, past_key_values=cache, logits_to_keep=1)
    for _ in range(g["max_new_tokens"]):
        nxt = out.logits[:, -1:].argmax(-1)
        ar = torch.cat([ar, nxt], dim=1)
        out = tgt(nxt, past_key_values=cache)
    assert ids[0].tolist() == ar[0].tolist()
    assert ids[0].tolist() == g["ids"]      # and equals the reference's CPU run


def test_draft_tokens_match_oracle_tiny():
    """Draft argmax ids of one cycle vs the oracle run on the CPU with the same weights
    (bf16, sdpa): logits within tolerance, ids equal wherever the oracle's top-2 margin
    exceeds it (SURVEY.md §7 'margin-screened')."""
    from oracle import dflash_oracle as O
    cfg = H.mid_cfg()
    w = H.draft_weights(cfg, dtype=BF16)
    m = make_model(cfg)
    g = torch.Generator().manual_seed(77)
    V, Hd = cfg.vocab_size, cfg.hidden_size
    lm = (torch.randn(V, Hd, generator=g) * 0.05).to(BF16)
    emb = (torch.randn(V, Hd, generator=g) * 0.05).to(BF16)
    P, tau, bs = 50, 9, 16
    th0 = (torch.randn(1, P, cfg.fc_in, generator=g) * 1.5).to(BF16)
    th1 = (torch.randn(1, tau, cfg.fc_in, generator=g) * 1.5).to(BF16)
    ids0 = torch.randint(0, V, (1, bs), generator=g)
    ids1 = torch.randint(0, V, (1, bs), generator=g)
    oc = H.oracle_cfg(cfg, "sdpa")
    ocache = O.ListKVCache()
    cache = m.new_cache(256)
    lm_wp = m.packed_lm_head(lm.to(dev()))
    for th, ids, start in ((th0, ids0, P), (th1, ids1, P + tau)):
        pos = torch.arange(ocache.get_seq_length(), start + bs)[None]
        hid = O.draft_forward(w, oc, position_ids=pos, noise_embedding=emb[ids], target_hidden=th, cache=ocache)
        ocache.crop(start)
        ref_logits = torch.nn.functional.linear(hid[:, 1:], lm).float()[0]
        # product
        ctx = th[0].to(dev())
        S = cache.get_seq_length()
        if ctx.shape[0] > 16:
            head = ctx.shape[0] - 16
            m.prefill_context(cache, ctx[:head], S)
            ctx, S = ctx[head:], S + head
        blk = ids.to(dev()).clone()
        frag = m.draft_block(cache, th_rows=ctx, tau=ctx.shape[0], bs=bs, pos0=S, block_ids=blk[0],
                             embed=emb.to(dev()))
        logits = torch.zeros(16, V, dtype=BF16, device=dev())
        m.draft_tokens(frag, lm_wp, bs, blk[0], logits=logits)
        H.assert_close(f"mid draft logits start {start}", logits[1:bs], ref_logits)
        H.assert_ids_match_where_safe(f"mid draft ids start {start}", blk[0, 1:], ref_logits, min_agree=0.8)


# ------------------------------------------------------------------ native target verify
def _tiny_hf(dtype=BF16, layers=6):
    from dflash_amd.synthetic import make_hf_qwen3
    torch.manual_seed(11)
    return make_hf_qwen3({**H.TINY_TARGET, "num_layers": layers}, dev(), dtype=dtype)


def test_native_verify_matches_hf_forward():
    """Same block through the wrapped HF model and through the kernels: logits, tapped
    hidden rows and the appended K/V agree within the bf16 tolerance of DESIGN.md §2."""
    from transformers import DynamicCache
    from dflash_amd import NativeTarget
    hf = _tiny_hf()
    nt = NativeTarget(hf)
    g = torch.Generator().manual_seed(2)
    prompt = torch.randint(0, 2000, (1, 45), generator=g).to(dev())
    block = torch.randint(0, 2000, (1, 16), generator=g).to(dev())
    taps = [1, 3]
    cache = nt.new_cache(128)
    out0 = nt.prefill(prompt, cache)
    logits = torch.zeros(16, 2048, dtype=BF16, device=dev())
    post, th = nt.verify(block[0], 45, cache, tap_layers=taps, logits_out=logits)
    # reference: HF forward over prompt then block
    rc = DynamicCache()
    hf(prompt, past_key_values=rc, use_cache=True)
    ref = hf(block, position_ids=torch.arange(45, 61, device=dev())[None], past_key_values=rc, use_cache=True,
             output_hidden_states=True)
    rl = ref.logits[0].float()
    H.assert_close("tiny verify logits", logits, rl)
    assert torch.equal(post[0], torch.argmax(logits, dim=-1))
    H.assert_ids_match_where_safe("tiny verify ids", post[0], rl)
    for j, l in enumerate(taps):
        H.assert_close(f"tiny verify tap {l}", th[:16, j * 512:(j + 1) * 512], ref.hidden_states[l + 1][0])
    for li in (0, 5):
        H.assert_close(f"tiny verify K layer {li}", cache.k[li][:, :61], rc.layers[li].keys[0], max_rel=H.KV_MAX_REL)
        H.assert_close(f"tiny verify V layer {li}", cache.v[li][:, :61], rc.layers[li].values[0], max_rel=H.KV_MAX_REL)
    assert cache.get_seq_length() == 61
    assert out0.logits.shape[1] == 1


def test_native_target_end_to_end_lossless_walk():
    """A large-margin synthetic target (dflash_amd.synthetic.impose_greedy_walk): the
    committed ids are its closed-form greedy walk through the native verify AND through
    the plain HF verify, with scripted acceptance lengths reproduced exactly."""
    from dflash_amd import NativeTarget, dflash_generate
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=5)
    prompt = torch.randint(0, 2000, (1, 33), generator=torch.Generator().manual_seed(4)).to(dev())
    n_new = 80
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = H.make_plan(64, 16, 17)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)       # the tail cycle's block is clamped
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % 2000, blk[0, k + 1])

    runs = {}
    for name, tgt in (("hf", hf), ("native", NativeTarget(hf))):
        r = dflash_generate(m, tgt, prompt, cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=hook)
        runs[name] = r
        assert r.output_ids[0].tolist() == G[:33 + n_new].tolist(), name
    assert runs["hf"].acceptance_lengths == runs["native"].acceptance_lengths
    exp = []
    tot, c = 0, 0
    while tot < n_new:
        t = min(plan[c] + 1, n_new - tot)
        exp.append(t)
        tot += t
        c += 1
    assert runs["native"].acceptance_lengths == exp


def test_round1_attention_stage_over_several_verifies():
    """NativeTarget(attn_impl="fused") — the round-1 stage that reads S / tau / pos0 from the cache's length record —
    over MANY verifies of one cache with an unchanged block size: the record must be rewritten every call (a record
    left at the first cycle's start position gives wrong RoPE / append rows from the second verify on).  Committed ids
    = the target's greedy walk, acceptance lengths = the 'head' stage's."""
    from dflash_amd import NativeTarget, dflash_generate
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=8)
    prompt = torch.randint(0, 2000, (1, 37), generator=torch.Generator().manual_seed(12)).to(dev())
    n_new = 90
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = H.make_plan(64, 16, 23)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % 2000, blk[0, k + 1])

    runs = {}
    for impl in ("head", "fused"):
        r = dflash_generate(m, NativeTarget(hf, attn_impl=impl), prompt, cfg.mask_token_id, n_new, 16, None, 0.0,
                            draft_token_hook=hook)
        assert r.output_ids[0].tolist() == G[:37 + n_new].tolist(), impl
        assert len(r.acceptance_lengths) > 5
        runs[impl] = r
    assert runs["head"].acceptance_lengths == runs["fused"].acceptance_lengths
    # and verify by verify on one cache: posterior ids and appended K rows of the two stages, three blocks in a row
    res = {}
    for impl in ("head", "fused"):
        tgt = NativeTarget(hf, attn_impl=impl)
        cache = tgt.new_cache(256)
        tgt.prefill(G[None, :30], cache)
        posts = []
        for c in range(3):
            s0 = 30 + 16 * c
            post, _ = tgt.verify(G[s0:s0 + 16].contiguous(), s0, cache)
            posts.append(post.clone())
        res[impl] = (posts, cache.k[2][:, :78].clone())
    for a, b in zip(res["head"][0], res["fused"][0]):
        assert torch.equal(a, b)
    H.assert_close("K rows layer 2 over three verifies, fused vs head", res["fused"][1], res["head"][1], max_rel=H.KV_MAX_REL)


def test_fused_attention_oproj_launch_is_equivalent():
    """fuse_oproj = True (dfl_attn_head_oproj: attention stage + o_proj in one launch, opt-in because it measured
    slower): the native verify's posterior ids and taps and the draft's block tokens agree with the two-launch
    path within the usual tolerances, the lossless walk still holds, and no launch raised its failure flag."""
    from dflash_amd import NativeTarget, dflash_generate
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=6)
    prompt = torch.randint(0, 2000, (1, 41), generator=torch.Generator().manual_seed(9)).to(dev())
    G = greedy_walk(perm, prompt, 120).to(dev())
    outs = {}
    for fuse in (False, True):
        m = make_model(cfg)
        m.fuse_oproj = fuse
        tgt = NativeTarget(hf)
        tgt.fuse_oproj = fuse
        r = dflash_generate(m, tgt, prompt, cfg.mask_token_id, 72, 16, None, 0.0)
        assert r.output_ids[0].tolist() == G[:41 + 72].tolist(), fuse
        outs[fuse] = r
        if fuse:
            assert int(tgt.ws["sync"].abs().sum()) == 0 and int(m._ws["sync"].abs().sum()) == 0
    assert outs[True].output_ids.tolist() == outs[False].output_ids.tolist()
    # one verify pass, state by state
    ids = G[:41][None]
    res = {}
    for fuse in (False, True):
        tgt = NativeTarget(hf)
        tgt.fuse_oproj = fuse
        cache = tgt.new_cache(256)
        tgt.prefill(ids[:, :30], cache)
        post, taps = tgt.verify(ids[0, 30:41].contiguous(), 30, cache, tap_layers=[1, 2])
        tgt.raise_if_failed()
        res[fuse] = (post.clone(), taps[:11].clone(), cache.k[3][:, :41].clone())
    assert torch.equal(res[True][0], res[False][0])
    H.assert_close("taps, one launch vs two", res[True][1], res[False][1])
    H.assert_close("K rows layer 3, one launch vs two", res[True][2], res[False][2], max_rel=H.KV_MAX_REL)


def test_accept_result_in_pinned_memory_equals_device_buffer(monkeypatch):
    """The loop's per-cycle hand-over: the accept kernel's 16-byte store into pinned host memory, polled by the host
    (default), against a device buffer read back with .tolist() (DFL_HOST_RESULT=0) — same ids, same acceptance
    lengths; and the block the kernel re-arms for the next cycle is what the reference slices out of output_ids
    (model/dflash.py:235)."""
    from dflash_amd import NativeTarget, dflash_generate
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=8)
    prompt = torch.randint(0, 2000, (1, 29), generator=torch.Generator().manual_seed(12)).to(dev())
    G = greedy_walk(perm, prompt, 100).to(dev())
    plan = H.make_plan(64, 16, 5)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000

    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DFL_HOST_RESULT", mode)
        m = make_model(cfg)
        r = dflash_generate(m, NativeTarget(hf), prompt, cfg.mask_token_id, 60, 16, None, 0.0, draft_token_hook=hook)
        assert r.output_ids[0].tolist() == G[:29 + 60].tolist(), mode
        runs[mode] = r
    assert runs["1"].acceptance_lengths == runs["0"].acceptance_lengths
    monkeypatch.setenv("DFL_HOST_RESULT", "1")
    s = DecodeSession(make_model(cfg), NativeTarget(hf), prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=40,
                      max_block_size=16, stop_token_ids=None, temperature=0.0, draft_token_hook=hook)
    assert s.result.is_pinned()
    s.prefill()
    for _ in range(3):
        s.cycle(16)
        assert torch.equal(s.block[0], s.output_ids[0, s.start:s.start + 16])


def test_temperature_path_with_sharp_logits():
    """T = 0.7 (BASELINE config 4's sampling path): softmax + torch.multinomial on the
    posterior, acceptance on the device.  With the scripted target's +-10 logits the
    draw is deterministic, so the ids equal the T = 0 golden run."""
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    g = E2E["bf16_sdpa/spec"]
    tgt = _scripted(g, cfg)
    torch.manual_seed(0)
    ids = m.spec_generate(target=tgt, input_ids=torch.tensor([g["prompt"]], device=dev()),
                          max_new_tokens=g["max_new_tokens"], stop_token_ids=None, temperature=0.7,
                          draft_token_hook=tgt.draft_token_hook)
    assert ids[0].tolist() == g["ids"]


def test_from_pretrained_checkpoint_dir(tmp_path):
    """HF checkpoint directory (config.json with block_size /
    num_target_layers / dflash_config + sharded *.safetensors with the reference's key
    names) loads into the same packed weights as load_state_dict."""
    from safetensors.torch import save_file
    from dflash_amd import DFlashDraftModel
    cfg = H.tiny_cfg()
    sd = H.draft_weights(cfg, dtype=BF16)
    keys = sorted(sd)
    save_file({k: sd[k] for k in keys[:len(keys) // 2]}, str(tmp_path / "model-00001-of-00002.safetensors"))
    save_file({k: sd[k] for k in keys[len(keys) // 2:]}, str(tmp_path / "model-00002-of-00002.safetensors"))
    hf_cfg = {"architectures": ["DFlashDraftModel"], "hidden_size": 512, "num_hidden_layers": 2,
              "num_attention_heads": 4, "num_key_value_heads": 2, "head_dim": 128, "intermediate_size": 1024,
              "vocab_size": 2048, "rms_norm_eps": 1e-6, "rope_theta": 1000000.0, "max_position_embeddings": 40960,
              "attention_bias": False, "block_size": 16, "num_target_layers": 6, "torch_dtype": "bfloat16",
              "dflash_config": {"mask_token_id": 2047, "target_layer_ids": [1, 3]}}
    (tmp_path / "config.json").write_text(json.dumps(hf_cfg))
    a = DFlashDraftModel.from_pretrained(str(tmp_path), device=dev())
    b = make_model(cfg)
    assert (a.block_size, a.mask_token_id, a.target_layer_ids) == (16, 2047, [1, 3])
    assert torch.equal(a.w["fc"], b.w["fc"])
    for la, lb in zip(a.w["layers"], b.w["layers"]):
        for k in la:
            assert torch.equal(la[k], lb[k]), k


@pytest.mark.parametrize("rope", [{"rope_type": "default", "rope_theta": 500000.0},
                                  {"rope_type": "llama3", "rope_theta": 500000.0, "factor": 8.0, "low_freq_factor": 1.0,
                                   "high_freq_factor": 4.0, "original_max_position_embeddings": 32}])
def test_native_target_llama_style(rope):
    """BASELINE config 4's target family (Llama-3.1: no per-head q/k norm, "llama3" RoPE
    frequency scaling — made active at test positions by a small original context):
    NativeTarget verify vs the HF forward."""
    tf = pytest.importorskip("transformers")
    from transformers import DynamicCache
    from dflash_amd import NativeTarget
    cfg = tf.LlamaConfig(vocab_size=2048, hidden_size=512, intermediate_size=1024, num_hidden_layers=4,
                         num_attention_heads=4, num_key_value_heads=2, head_dim=128, rms_norm_eps=1e-5,
                         max_position_embeddings=4096, tie_word_embeddings=False, attention_bias=False,
                         mlp_bias=False, rope_parameters=dict(rope))
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(3)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        with torch.device(dev()):
            hf = tf.LlamaForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    nt = NativeTarget(hf)
    assert nt.layers[0]["q_norm"] is None
    g = torch.Generator().manual_seed(8)
    prompt = torch.randint(0, 2000, (1, 29), generator=g).to(dev())
    block = torch.randint(0, 2000, (1, 12), generator=g).to(dev())
    cache = nt.new_cache(64)
    nt.prefill(prompt, cache)
    logits = torch.zeros(16, 2048, dtype=BF16, device=dev())
    post, taps = nt.verify(block[0], 29, cache, tap_layers=[1], logits_out=logits)
    rc = DynamicCache()
    hf(prompt, past_key_values=rc, use_cache=True)
    ref = hf(block, position_ids=torch.arange(29, 41, device=dev())[None], past_key_values=rc, use_cache=True,
             output_hidden_states=True)
    rl = ref.logits[0].float()
    tag = rope["rope_type"]
    H.assert_close(f"llama-style {tag} logits", logits[:12], rl)
    H.assert_close(f"llama-style {tag} tap", taps[:12, :512], ref.hidden_states[2][0])
    assert torch.equal(post[0], torch.argmax(logits[:12], dim=-1))
    for li in (0, 3):    # K rows carry the RoPE: scaled frequencies included
        H.assert_close(f"llama-style {tag} K layer {li}", cache.k[li][:, :41], rc.layers[li].keys[0], max_rel=H.KV_MAX_REL)


def test_qwen3_4b_geometry_matches_oracle():
    """Qwen3-4B's geometry (BASELINE configs[0]): q_dim = heads x 128 = 1024 != hidden 640 here
    (4096 != 2560 there), FFN not a multiple of 1024, hidden % 512 != 0 — the o_proj / qkv
    shapes no other fixture has.  Three draft cycles with cache against the CPU oracle on the same
    seeded weights; then the native target verify at the same geometry against the HF forward."""
    from oracle import dflash_oracle as O
    from dflash_amd import DFlashDraftModel
    from dflash_amd.config import DFlashConfig
    cfg = DFlashConfig(hidden_size=640, num_hidden_layers=2, num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                       intermediate_size=2432, vocab_size=3072, num_target_layers=6, block_size=16, rope_theta=1e6,
                       mask_token_id=3071)
    assert cfg.q_dim != cfg.hidden_size
    w = H.draft_weights(cfg, seed=21, dtype=BF16)
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(w)
    oc = H.oracle_cfg(cfg, "sdpa")
    g = torch.Generator().manual_seed(9)
    ocache = O.ListKVCache()
    cache = m.new_cache(256)
    start = 37
    for c, (ctx, bs, tau_next) in enumerate(((37, 16, 5), (5, 16, 16), (16, 12, 3))):
        th = (torch.randn(1, ctx, cfg.fc_in, generator=g) * 1.5).to(BF16)
        ne = (torch.randn(1, bs, cfg.hidden_size, generator=g) * 0.05).to(BF16)
        pos = torch.arange(ocache.get_seq_length(), start + bs)[None]
        ref = O.draft_forward(w, oc, position_ids=pos, noise_embedding=ne, target_hidden=th, cache=ocache)
        ocache.crop(start)
        got = m(target_hidden=th.to(dev()), noise_embedding=ne.to(dev()), position_ids=pos.to(dev()),
                past_key_values=cache, use_cache=True, is_causal=False)
        cache.crop(start)
        H.assert_close(f"4B-geometry draft hidden cycle {c}", got, ref)
        start += tau_next
    n = cache.get_seq_length()
    for li in range(cfg.num_hidden_layers):
        H.assert_close(f"4B-geometry draft K layer {li}", cache.k[li][:, :n], ocache.k[li][0], max_rel=H.KV_MAX_REL)
        H.assert_close(f"4B-geometry draft V layer {li}", cache.v[li][:, :n], ocache.v[li][0], max_rel=H.KV_MAX_REL)


    # ---- target side: a 4-layer HF Qwen3 of the same geometry through NativeTarget.verify
    from transformers import DynamicCache
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import make_hf_qwen3
    torch.manual_seed(13)
    hf = make_hf_qwen3(dict(vocab_size=3072, hidden_size=640, num_layers=4, num_heads=8, num_kv_heads=2, head_dim=128,
                            intermediate_size=2432, rope_theta=1e6), dev())
    nt = NativeTarget(hf)
    prompt = torch.randint(0, 3000, (1, 50), generator=g).to(dev())
    block = torch.randint(0, 3000, (1, 16), generator=g).to(dev())
    tc = nt.new_cache(128)
    nt.prefill(prompt, tc)
    logits = torch.zeros(16, 3072, dtype=BF16, device=dev())
    post, taps = nt.verify(block[0], 50, tc, tap_layers=[0, 2], logits_out=logits)
    rc = DynamicCache()
    hf(prompt, past_key_values=rc, use_cache=True)
    refo = hf(block, position_ids=torch.arange(50, 66, device=dev())[None], past_key_values=rc, use_cache=True,
              output_hidden_states=True)
    H.assert_close("4B-geometry verify logits", logits, refo.logits[0])
    for j, li in enumerate((0, 2)):
        H.assert_close(f"4B-geometry verify tap {li}", taps[:16, j * 640:(j + 1) * 640], refo.hidden_states[li + 1][0])


def test_full_size_draft_cycle_matches_oracle():
    """BASELINE.json's full shapes (Qwen3-8B-DFlash-b16: H 4096, 5 layers, 32/8 heads,
    FFN 12288, 5 taps): a prompt-context cycle and a steady cycle of the draft forward
    against the CPU oracle with the same seeded weights; then the fused lm_head+argmax on
    a 151936-row head against the oracle's logits (margin-screened ids)."""
    from oracle import dflash_oracle as O
    from dflash_amd.config import DFlashConfig, QWEN3_8B_DRAFT
    torch.set_num_threads(max(8, torch.get_num_threads()))
    cfg = DFlashConfig(**QWEN3_8B_DRAFT)
    w = H.draft_weights(cfg, seed=11, dtype=BF16)
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(w)
    oc = H.oracle_cfg(cfg, "sdpa")
    g = torch.Generator().manual_seed(5)
    ocache = O.ListKVCache()
    cache = m.new_cache(256)
    start = 40
    for c, (ctx, bs, tau_next) in enumerate(((40, 16, 7), (7, 16, 16))):
        th = (torch.randn(1, ctx, cfg.fc_in, generator=g) * 1.5).to(BF16)
        ne = (torch.randn(1, bs, cfg.hidden_size, generator=g) * 0.05).to(BF16)
        pos = torch.arange(ocache.get_seq_length(), start + bs)[None]
        ref = O.draft_forward(w, oc, position_ids=pos, noise_embedding=ne, target_hidden=th, cache=ocache)
        ocache.crop(start)
        got = m(target_hidden=th.to(dev()), noise_embedding=ne.to(dev()), position_ids=pos.to(dev()),
                past_key_values=cache, use_cache=True, is_causal=False)
        cache.crop(start)
        H.assert_close(f"8B draft hidden cycle {c}", got, ref)
        start += tau_next
    # lm_head at full vocabulary on the last cycle's hidden rows
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.02).to(BF16)
    ref_logits = torch.nn.functional.linear(ref[0, 1:], lm).float()
    wp = m.packed_lm_head(lm.to(dev()))
    ids = torch.zeros(16, dtype=torch.long, device=dev())
    logits = torch.zeros(16, cfg.vocab_size, dtype=BF16, device=dev())
    m.draft_tokens(m._src["final"], wp, 16, ids, logits=logits)
    H.assert_close("8B draft logits (V = 151936)", logits[1:], ref_logits)
    # random weights: the top-2 margin of a 151936-way argmax is a few bf16 ulps, so the screen
    # (margin > 3 % of the logit scale) keeps few rows; it must keep some, and those must agree
    H.assert_ids_match_where_safe("8B draft ids", ids[1:], ref_logits, margin_rel=3e-2, min_agree=0.6)


def test_full_size_draft_at_the_bench_operating_point():
    """VERDICT r3 next #5a: the 8B-shaped draft exactly where bench.py runs it — cycle 0 with a 1024-row prompt context
    (through `_prefill_context_rows`: the prompt's tapped states projected into the draft cache at once) and two steady
    cycles at S ~ 1024..1040 (tau = 7, then 16) — against `oracle.draft_forward` on the same seeded weights: hidden
    rows of every cycle, the cached K/V rows of layers 0 and 4 over the whole 1k prefix, and the 151936-way greedy ids
    on margin-screened rows.  (The bench's `lossless_fraction` cannot see the draft: its hook overwrites the ids.)"""
    from oracle import dflash_oracle as O
    from dflash_amd.config import DFlashConfig, QWEN3_8B_DRAFT
    from dflash_amd import DFlashDraftModel
    torch.set_num_threads(max(8, torch.get_num_threads()))
    cfg = DFlashConfig(**QWEN3_8B_DRAFT)
    w = H.draft_weights(cfg, seed=11, dtype=BF16)
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(w)
    oc = H.oracle_cfg(cfg, "sdpa")
    g = torch.Generator().manual_seed(15)
    ocache = O.ListKVCache()
    cache = m.new_cache(1024 + 128)
    start = 1024
    refs = []
    for c, (ctx, bs, tau_next) in enumerate(((1024, 16, 7), (7, 16, 16), (16, 16, 4))):
        th = (torch.randn(1, ctx, cfg.fc_in, generator=g) * 1.5).to(BF16)
        ne = (torch.randn(1, bs, cfg.hidden_size, generator=g) * 0.05).to(BF16)
        pos = torch.arange(ocache.get_seq_length(), start + bs)[None]
        ref = O.draft_forward(w, oc, position_ids=pos, noise_embedding=ne, target_hidden=th, cache=ocache)
        ocache.crop(start)
        got = m(target_hidden=th.to(dev()), noise_embedding=ne.to(dev()), position_ids=pos.to(dev()),
                past_key_values=cache, use_cache=True, is_causal=False)
        cache.crop(start)
        H.assert_close(f"8B draft @ S~1k hidden cycle {c} (ctx {ctx})", got, ref)
        refs.append(ref)
        start += tau_next
    n = cache.get_seq_length()
    assert n == ocache.get_seq_length() == 1024 + 7 + 16
    for li in (0, 4):
        H.assert_close(f"8B draft @ S~1k K layer {li}", cache.k[li][:, :n], ocache.k[li][0], max_rel=H.KV_MAX_REL)
        H.assert_close(f"8B draft @ S~1k V layer {li}", cache.v[li][:, :n], ocache.v[li][0], max_rel=H.KV_MAX_REL)
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.02).to(BF16)
    ref_logits = torch.nn.functional.linear(refs[-1][0, 1:], lm).float()
    wp = m.packed_lm_head(lm.to(dev()))
    ids = torch.zeros(16, dtype=torch.long, device=dev())
    logits = torch.zeros(16, cfg.vocab_size, dtype=BF16, device=dev())
    m.draft_tokens(m._src["final"], wp, 16, ids, logits=logits)
    H.assert_close("8B draft @ S~1k logits (V = 151936)", logits[1:], ref_logits)
    H.assert_ids_match_where_safe("8B draft @ S~1k ids", ids[1:], ref_logits, margin_rel=3e-2, min_agree=0.6)


def test_true_qwen3_4b_shapes_with_tied_embeddings():
    """VERDICT r3 next #5b: BASELINE configs[0] at its real widths — hidden 2560, FFN 9728, q_dim 4096 != hidden, 5 taps
    (fc: 12800 -> 2560) — and with TIED embeddings (Qwen3-4B: lm_head.weight is embed_tokens.weight, so the draft's
    noise rows and its unmask logits come from one tensor, model/dflash.py:237-238): a prompt-context cycle and a steady
    cycle of the draft forward vs the oracle, block rows embedded from the tied table by the product's own gather, the
    151936-way logits / ids through the same table."""
    from oracle import dflash_oracle as O
    from dflash_amd.config import DFlashConfig, QWEN3_4B_DRAFT
    from dflash_amd import DFlashDraftModel
    torch.set_num_threads(max(8, torch.get_num_threads()))
    cfg = DFlashConfig(**QWEN3_4B_DRAFT)
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.q_dim, cfg.fc_in) == (2560, 9728, 4096, 12800)
    w = H.draft_weights(cfg, seed=19, dtype=BF16)
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(w)
    oc = H.oracle_cfg(cfg, "sdpa")
    g = torch.Generator().manual_seed(23)
    tied = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.05).to(BF16)   # embed_tokens.weight IS lm_head.weight
    tied_d = tied.to(dev())
    ocache = O.ListKVCache()
    cache = m.new_cache(256)
    start = 70
    for c, (ctx, bs, tau_next) in enumerate(((70, 16, 9), (9, 16, 16))):
        th = (torch.randn(1, ctx, cfg.fc_in, generator=g) * 1.5).to(BF16)
        blk = torch.randint(0, cfg.vocab_size, (bs,), generator=g)
        blk[1:] = cfg.mask_token_id
        ne = tied[blk][None]                               # target.model.embed_tokens(block), model/dflash.py:237
        pos = torch.arange(ocache.get_seq_length(), start + bs)[None]
        ref = O.draft_forward(w, oc, position_ids=pos, noise_embedding=ne, target_hidden=th, cache=ocache)
        ocache.crop(start)
        got = m(target_hidden=th.to(dev()), noise_embedding=tied_d[blk.to(dev())][None], position_ids=pos.to(dev()),
                past_key_values=cache, use_cache=True, is_causal=False)
        cache.crop(start)
        H.assert_close(f"Qwen3-4B widths draft hidden cycle {c}", got, ref)
        start += tau_next
    n = cache.get_seq_length()
    for li in (0, cfg.num_hidden_layers - 1):
        H.assert_close(f"Qwen3-4B widths draft K layer {li}", cache.k[li][:, :n], ocache.k[li][0], max_rel=H.KV_MAX_REL)
    ref_logits = torch.nn.functional.linear(ref[0, 1:], tied).float()       # target.lm_head == the embedding table
    wp = m.packed_lm_head(tied_d)
    ids = torch.zeros(16, dtype=torch.long, device=dev())
    logits = torch.zeros(16, cfg.vocab_size, dtype=BF16, device=dev())
    m.draft_tokens(m._src["final"], wp, 16, ids, logits=logits)
    H.assert_close("Qwen3-4B widths tied-table logits (V = 151936)", logits[1:], ref_logits)
    H.assert_ids_match_where_safe("Qwen3-4B widths tied-table ids", ids[1:], ref_logits, margin_rel=3e-2, min_agree=0.6)


def test_long_prefix_many_key_splits():
    """Prefix far beyond the bench's 1k (S = 9000: the key-split count saturates at
    max_splits, every split walks many tiles): native verify vs the HF forward."""
    from transformers import DynamicCache
    from dflash_amd import NativeTarget
    hf = _tiny_hf(layers=2)
    nt = NativeTarget(hf, max_splits=8)
    g = torch.Generator().manual_seed(12)
    P = 9000
    prompt = torch.randint(0, 2000, (1, P), generator=g).to(dev())
    block = torch.randint(0, 2000, (1, 16), generator=g).to(dev())
    cache = nt.new_cache(P + 64)
    nt.prefill(prompt, cache)
    logits = torch.zeros(16, 2048, dtype=BF16, device=dev())
    nt.verify(block[0], P, cache, logits_out=logits)
    rc = DynamicCache()
    hf(prompt, past_key_values=rc, use_cache=True)
    ref = hf(block, position_ids=torch.arange(P, P + 16, device=dev())[None], past_key_values=rc, use_cache=True)
    H.assert_close("S = 9000 verify logits", logits, ref.logits[0])


def test_harness_options_on_native_target():
    """The harness-level options of benchmark.py / benchmark_dynamic_schedule.py on the native
    verify: per-cycle profile (benchmark.py:99-240), draft_steps = 2 (:112-142), the block-size
    scheduler loop with T > 0 draft sampling (benchmark_dynamic_schedule.py:321-379) and the
    bs = 1 baseline — all must commit the target's own greedy walk."""
    from dflash_amd import EWMAPerformanceScheduler, NativeTarget, dflash_generate, dflash_generate_policy
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=5)
    nt = NativeTarget(hf)
    prompt = torch.randint(0, 2000, (1, 27), generator=torch.Generator().manual_seed(14)).to(dev())
    n_new = 50
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    want = G[:27 + n_new].tolist()
    r = dflash_generate(m, nt, prompt, cfg.mask_token_id, n_new, 16, None, 0.0, collect_profile=True)
    assert r.output_ids[0].tolist() == want
    ps = r.profile_summary
    assert ps["profiled_cycles"] == len(r.acceptance_lengths) and ps["draft_decode_s"] > 0 and ps["target_decode_s"] > 0
    assert abs(ps["draft_share_decode"] + ps["target_share_decode"] - 1.0) < 1e-6
    r2 = dflash_generate(m, nt, prompt, cfg.mask_token_id, n_new, 16, None, 0.0, draft_steps=2)
    assert r2.output_ids[0].tolist() == want
    r1 = dflash_generate(m, nt, prompt, cfg.mask_token_id, n_new, 1, None, 0.0)   # bs = 1: plain target AR
    assert r1.output_ids[0].tolist() == want and r1.acceptance_lengths == [1] * n_new
    sched = EWMAPerformanceScheduler(candidates=[8, 12, 16], scheduler_mode="ewma", warmup_cycles=3, ewma_alpha=0.25,
                                     switch_margin=0.03, required_streak=2, cooldown_cycles=2, probe_interval=5,
                                     low_accept_threshold=0.2, low_accept_streak=3, adl_rho=0.3, adl_delta=1.0,
                                     adl_k_min=8, adl_k_max=16, adl_neighborhood=4)
    torch.manual_seed(0)
    rp = dflash_generate_policy(model=m, target=nt, input_ids=prompt, mask_token_id=cfg.mask_token_id,
                                max_new_tokens=n_new, stop_token_ids=None, temperature=0.7, scheduler=sched)
    assert rp.output_ids[0].tolist() == want          # margin ~70: the T = 0.7 posterior draw is the argmax
    assert set(rp.used_block_sizes) <= {8, 12, 16} | set(range(1, 17)) and len(rp.cycle_trace) == len(rp.acceptance_lengths)


# ------------------------------------------------------------------ blocks of 17..32 rows (golden G8)
WIDE = json.load(open(os.path.join(H.GOLDEN, "e2e_wide.json")))


def _scripted_wide(g, cfg):
    base = H.tiny_target(dtype=BF16, device=dev())
    total = len(g["prompt"]) + g["max_new_tokens"]
    tape = H.make_tape(total + 64, cfg.vocab_size, g["tape_seed"], forbid=(cfg.mask_token_id,))
    t = H.ScriptedTarget(base, tape, H.make_plan(64, g["plan_bs"], g["plan_seed"]))
    t.script_lm_head = False
    return t


def test_wide_blocks_match_reference_ids():
    """Block sizes 20 / 24 / 32 (results.md:11-16, run_block_sweep.sh) and a {12, 20, 24} schedule
    (benchmark_dynamic_schedule.py:44-51 takes any candidate >= 2): committed ids, acceptance lengths (up to 32)
    and used block sizes equal the reference's runs."""
    from dflash_amd import dflash_generate, dflash_generate_policy
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    for key in ("gen_bs20", "gen_bs24", "gen_bs32"):
        g = WIDE[f"bf16_sdpa/{key}"]
        tgt = _scripted_wide(g, cfg)
        r = dflash_generate(m, tgt, torch.tensor([g["prompt"]], device=dev()), cfg.mask_token_id,
                            g["max_new_tokens"], g["block_size"], None, 0.0, draft_token_hook=tgt.draft_token_hook)
        assert r.output_ids[0].tolist() == g["ids"], key
        assert r.acceptance_lengths == g["acceptance_lengths"], key
        assert max(r.acceptance_lengths) > 16
    g = WIDE["bf16_sdpa/policy_wide"]
    tgt = _scripted_wide(g, cfg)
    sch = _Replay(g["chosen_block_sizes"], g["candidates"])
    r = dflash_generate_policy(model=m, target=tgt, input_ids=torch.tensor([g["prompt"]], device=dev()),
                               mask_token_id=cfg.mask_token_id, max_new_tokens=g["max_new_tokens"],
                               stop_token_ids=None, temperature=0.0, scheduler=sch,
                               draft_token_hook=tgt.draft_token_hook)
    assert r.output_ids[0].tolist() == g["ids"]
    assert r.acceptance_lengths == g["acceptance_lengths"] and r.used_block_sizes == g["used_block_sizes"]
    with pytest.raises(ValueError):      # 33 rows: rejected before the prefill runs
        dflash_generate(m, tgt, torch.tensor([g["prompt"]], device=dev()), cfg.mask_token_id, 8, 33, None, 0.0)


@pytest.mark.parametrize("one_pass", [True, False])
@pytest.mark.parametrize("bs", [17, 24, 32])
def test_native_verify_wide_block_matches_hf_forward(bs, one_pass):
    """The native verify on two 16-row tiles against the HF forward: logits of all bs rows, taps, appended K/V.
    one_pass: both tiles through the ragged-batch GEMMs (one pass over the weights, the default); else one launch
    per tile of every single-request GEMM.  Both query tiles share the attention launch either way."""
    from transformers import DynamicCache
    from dflash_amd import NativeTarget
    hf = _tiny_hf()
    nt = NativeTarget(hf)
    nt.wide_one_pass = one_pass
    g = torch.Generator().manual_seed(40 + bs)
    P = 45
    prompt = torch.randint(0, 2000, (1, P), generator=g).to(dev())
    block = torch.randint(0, 2000, (1, bs), generator=g).to(dev())
    taps = [1, 3]
    cache = nt.new_cache(128)
    nt.prefill(prompt, cache)
    logits = torch.zeros(32, 2048, dtype=BF16, device=dev())
    post, th = nt.verify(block[0], P, cache, tap_layers=taps, logits_out=logits)
    rc = DynamicCache()
    with torch.inference_mode():
        hf(prompt, past_key_values=rc, use_cache=True)
        ref = hf(block, position_ids=torch.arange(P, P + bs, device=dev())[None], past_key_values=rc, use_cache=True,
                 output_hidden_states=True)
    rl = ref.logits[0].float()
    H.assert_close(f"bs {bs} verify logits", logits[:bs], rl)
    assert post.shape == (1, bs) and torch.equal(post[0], torch.argmax(logits[:bs], dim=-1))
    H.assert_ids_match_where_safe(f"bs {bs} verify ids", post[0], rl)
    for j, l in enumerate(taps):
        H.assert_close(f"bs {bs} verify tap {l}", th[:bs, j * 512:(j + 1) * 512], ref.hidden_states[l + 1][0])
    for li in (0, 5):
        H.assert_close(f"bs {bs} verify K layer {li}", cache.k[li][:, :P + bs], rc.layers[li].keys[0], max_rel=H.KV_MAX_REL)
        H.assert_close(f"bs {bs} verify V layer {li}", cache.v[li][:, :P + bs], rc.layers[li].values[0], max_rel=H.KV_MAX_REL)
    assert cache.get_seq_length() == P + bs


@pytest.mark.parametrize("bs,tau", [(24, 9), (32, 16), (17, 0)])
def test_wide_draft_one_pass_equals_two_passes(bs, tau):
    """Draft forward of a 17..32-row block: one pass over the weights (ragged-batch GEMMs, R = 2) against the
    single-request GEMMs run once per 16-row tile — hidden states, appended K/V and the drafted tokens."""
    cfg = H.tiny_cfg()
    g = torch.Generator().manual_seed(7 * bs + tau)
    P = 70
    th = torch.randn(1, tau, cfg.fc_in, generator=g).to(BF16).to(dev())
    ne = torch.randn(1, bs, cfg.hidden_size, generator=g).to(BF16).to(dev())
    ctx0 = torch.randn(P, cfg.fc_in, generator=g).to(BF16).to(dev())
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g) * 0.05).to(BF16).to(dev())
    emb = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=g)).to(BF16).to(dev())
    ids = torch.randint(0, cfg.vocab_size, (bs,), generator=g).to(dev())
    outs = {}
    for one_pass in (True, False):
        m = make_model(cfg)
        m.wide_one_pass = one_pass
        cache = m.new_cache(P + 64)
        m.prefill_context(cache, ctx0, 0)
        pos = torch.arange(P, P + tau + bs, device=dev()).unsqueeze(0)
        hid = m(target_hidden=th, noise_embedding=ne, position_ids=pos, past_key_values=cache, use_cache=True)
        kv = (cache.k[1][:, :P + tau + bs].clone(), cache.v[1][:, :P + tau + bs].clone())
        # the loop's form: token ids + embedding table in, drafted ids out
        cache2 = m.new_cache(P + 64)
        m.prefill_context(cache2, ctx0, 0)
        blk = ids.clone()
        logits = torch.zeros(32, cfg.vocab_size, dtype=BF16, device=dev())
        with torch.inference_mode():
            rows = m.draft_block(cache2, th_rows=th[0] if tau else None, tau=tau, bs=bs, pos0=P, block_ids=blk, embed=emb)
            m.draft_tokens(rows, ops_pack(lm), bs, blk, logits=logits)
        assert torch.equal(blk[1:], torch.argmax(logits[1:bs], dim=-1)) and blk[0] == ids[0]
        outs[one_pass] = (hid.clone(), kv, logits[1:bs].clone(), blk.clone())
    a, b = outs[True], outs[False]
    H.assert_close(f"wide draft hidden bs {bs}", a[0], b[0])
    H.assert_close(f"wide draft K bs {bs}", a[1][0], b[1][0], max_rel=H.KV_MAX_REL)
    H.assert_close(f"wide draft V bs {bs}", a[1][1], b[1][1], max_rel=H.KV_MAX_REL)
    H.assert_close(f"wide draft logits bs {bs}", a[2], b[2])
    H.assert_ids_match_where_safe(f"wide draft ids bs {bs}", a[3][1:], b[2].float(), min_safe=1)


@pytest.mark.parametrize("one_pass", [True, False])
def test_native_verify_wide_block_temperature_path(one_pass):
    """T = 0.7 on a 24-row block (the materialised-logits branch of the wide verify, softmax + multinomial on 24 rows
    of device logits): with the large-margin synthetic target the draw is its argmax, so the posterior equals the
    T = 0 posterior — which is the closed-form greedy walk."""
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=21)
    P, bs = 40, 24
    prompt = torch.randint(0, 2000, (1, P), generator=torch.Generator().manual_seed(5)).to(dev())
    G = greedy_walk(perm, prompt, bs + 8).to(dev())
    nt = NativeTarget(hf)
    nt.wide_one_pass = one_pass
    posts = []
    for T in (0.0, 0.7):
        cache = nt.new_cache(128)
        nt.prefill(prompt, cache)
        torch.manual_seed(3)
        post, _ = nt.verify(G[P:P + bs].contiguous(), P, cache, temperature=T)
        posts.append(post[0].clone())
    assert torch.equal(posts[0], G[P + 1:P + bs + 1])          # next-token ids of the walk
    assert torch.equal(posts[1], posts[0])


def test_native_target_wide_blocks_lossless_walk():
    """bs = 24 and a {12, 20, 24} schedule end to end on the NATIVE verify: the committed ids are the target's
    closed-form greedy walk, with scripted acceptance lengths up to 24."""
    from dflash_amd import EWMAPerformanceScheduler, NativeTarget, dflash_generate, dflash_generate_policy
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=5)
    nt = NativeTarget(hf)
    prompt = torch.randint(0, 2000, (1, 33), generator=torch.Generator().manual_seed(4)).to(dev())
    n_new = 120
    G = greedy_walk(perm, prompt, n_new + 64).to(dev())
    plan = H.make_plan(64, 24, 23)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % 2000, blk[0, k + 1])

    r = dflash_generate(m, nt, prompt, cfg.mask_token_id, n_new, 24, None, 0.0, draft_token_hook=hook)
    assert r.output_ids[0].tolist() == G[:33 + n_new].tolist()
    assert max(r.acceptance_lengths) == 24 and r.acceptance_lengths[:4] == [1, 24, 2, 23]
    sched = EWMAPerformanceScheduler(candidates=[12, 20, 24], scheduler_mode="ewma", warmup_cycles=3, ewma_alpha=0.25,
                                     switch_margin=0.03, required_streak=2, cooldown_cycles=2, probe_interval=5,
                                     low_accept_threshold=0.2, low_accept_streak=3, adl_rho=0.3, adl_delta=1.0,
                                     adl_k_min=8, adl_k_max=24, adl_neighborhood=4)
    rp = dflash_generate_policy(model=m, target=nt, input_ids=prompt, mask_token_id=cfg.mask_token_id,
                                max_new_tokens=n_new, stop_token_ids=None, temperature=0.0, scheduler=sched,
                                draft_token_hook=hook)
    assert rp.output_ids[0].tolist() == G[:33 + n_new].tolist()
    assert set(rp.used_block_sizes) & {20, 24}


@pytest.mark.parametrize("P", [17, 64, 100, 128, 300, 1000])
def test_wide_context_prefill_equals_group_prefill(P):
    """The prompt's context rows at once on the prefill kernels (P >= 128) / through the 64-row passes of the ragged-batch
    GEMMs (model/dflash.py:73-85 at ctx = P) vs the 16-row-group path: the same K/V rows in every layer (V up to the
    rounding of a different K-split order, K likewise after its RoPE), within tolerance of the oracle on the CPU."""
    from oracle import dflash_oracle as O
    cfg = H.tiny_cfg()
    m = make_model(cfg)
    g = torch.Generator().manual_seed(P)
    th = (torch.randn(1, P, cfg.fc_in, generator=g) * 1.5).to(BF16)
    ca, cb = m.new_cache(P + 64), m.new_cache(P + 64)
    m.wide_prefill = True
    m.prefill_context(ca, th[0].to(dev()), 5)
    m.wide_prefill = False
    m.prefill_context(cb, th[0].to(dev()), 5)
    m.wide_prefill = True
    assert ca.get_seq_length() == cb.get_seq_length() == P
    if P >= 128:      # ca took the prompt-length kernels: the 64-row passes are the third form
        cc = m.new_cache(P + 64)
        m.rows_prefill = False
        m.prefill_context(cc, th[0].to(dev()), 5)
        m.rows_prefill = True
        for li in range(cfg.num_hidden_layers):
            H.assert_close(f"64-row passes K l{li} P{P}", cc.k[li][:, :P], cb.k[li][:, :P], max_rel=2 ** -6, mean_rel=1e-3)
            H.assert_close(f"64-row passes V l{li} P{P}", cc.v[li][:, :P], cb.v[li][:, :P], max_rel=2 ** -6, mean_rel=1e-3)
    for li in range(cfg.num_hidden_layers):
        H.assert_close(f"wide prefill K l{li} P{P}", ca.k[li][:, :P], cb.k[li][:, :P], max_rel=2 ** -6, mean_rel=1e-3)
        H.assert_close(f"wide prefill V l{li} P{P}", ca.v[li][:, :P], cb.v[li][:, :P], max_rel=2 ** -6, mean_rel=1e-3)
    assert int(torch.count_nonzero(ca.k[:, :, P:])) == 0 and int(torch.count_nonzero(ca.v[:, :, P:])) == 0
    if P <= 300:   # and against the oracle: K/V of the context rows as the reference caches them (positions 5..)
        w = H.draft_weights(cfg, dtype=BF16)
        oc = H.oracle_cfg(cfg, "sdpa")
        oc_cache = O.ListKVCache()
        ne = torch.zeros(1, 1, cfg.hidden_size, dtype=BF16)
        O.draft_forward(w, oc, position_ids=torch.arange(5, 5 + P + 1)[None], noise_embedding=ne, target_hidden=th,
                        cache=oc_cache)
        for li in range(cfg.num_hidden_layers):
            H.assert_close(f"wide prefill vs oracle K l{li}", ca.k[li][:, :P], oc_cache.k[li][0][:, :P], max_rel=H.KV_MAX_REL)
            H.assert_close(f"wide prefill vs oracle V l{li}", ca.v[li][:, :P], oc_cache.v[li][0][:, :P], max_rel=H.KV_MAX_REL)


def test_graph_replayed_cycles_equal_eager_cycles():
    """DecodeSession.capture / cycle_graph: the steady-state cycle replayed from two hipGraphs —
    [verify + accept], [the next cycle's draft + lm_head], every length from the device records the accept kernel keeps
    (dfl_accept_commit with dyn_t) — commits the same ids with the same acceptance lengths as eager cycles, including an
    eager cycle in the middle (its accept keeps the target's record too) and the eager tail."""
    from dflash_amd import NativeTarget
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=8)
    prompt = torch.randint(0, 2000, (1, 41), generator=torch.Generator().manual_seed(3)).to(dev())
    n_new = 150
    G = greedy_walk(perm, prompt, n_new + 60).to(dev())
    plan = H.make_plan(64, 16, 29)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000

    def run(graph):
        s = DecodeSession(make_model(cfg), NativeTarget(hf), prompt, mask_token_id=cfg.mask_token_id,
                          max_new_tokens=n_new, max_block_size=16, stop_token_ids=None, temperature=0.0,
                          draft_token_hook=hook)
        s.prefill()
        taus, replayed = [], 0
        for i in range(64):
            if s.start >= s.max_length:
                break
            bs = min(16, s.max_length - s.start)
            if graph and i == 2:
                s.capture(16)
            if graph and i >= 2 and i != 5 and bs == 16:
                replayed += int(s._graph_ok(16))
                r = s.cycle_graph(16)
            else:
                r = s.cycle(bs, ahead_ok=bs == 16)
            taus.append(r.tau)
        return s.finish()[0].tolist(), taus, replayed

    ids_e, taus_e, _ = run(False)
    ids_g, taus_g, replayed = run(True)
    assert ids_e == G[:41 + n_new].tolist()
    assert ids_g == ids_e and taus_g == taus_e
    assert replayed >= 8, replayed      # most steady-state cycles really went through the graphs


def test_captured_graphs_survive_a_replaced_rope_table():
    """the captured launches hold raw pointers into the draft model's / target's RoPE tables, which
    `_rope_tab` REPLACES when another caller on the same shared target needs more positions.  The session keeps the
    captured tensors alive, notices the new table (`_graph_ok`), runs that cycle eagerly and captures again: ids and
    acceptance lengths stay those of the eager loop."""
    from dflash_amd import NativeTarget
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=8)
    prompt = torch.randint(0, 2000, (1, 41), generator=torch.Generator().manual_seed(3)).to(dev())
    n_new = 150
    G = greedy_walk(perm, prompt, n_new + 60).to(dev())
    plan = H.make_plan(64, 16, 29)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000

    nt, m = NativeTarget(hf), make_model(cfg)
    s = DecodeSession(m, nt, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, max_block_size=16,
                      stop_token_ids=None, temperature=0.0, draft_token_hook=hook)
    s.prefill()
    taus, replayed, recaptured = [], 0, 0
    for i in range(64):
        if s.start >= s.max_length:
            break
        bs = min(16, s.max_length - s.start)
        if i == 2:
            s.capture(16)
            old = (nt._rope[0], m._rope[0])
        if i == 5:      # another caller needs a longer table: both owners allocate a new one, the old is released by them
            need = 4 * nt._rope[0].shape[0]
            nt._rope_tab(need)
            m._rope_tab(need)
            assert nt._rope[0].data_ptr() != old[0].data_ptr() and m._rope[0].data_ptr() != old[1].data_ptr()
            del old
            junk = [torch.full((1 << 16,), float("nan"), dtype=BF16, device=dev()) for _ in range(8)]   # reuse freed blocks
        if i >= 2 and bs == 16:
            if getattr(s, "_graph_bs", None) is None and s._ahead == 16:
                s.capture(16)
                recaptured += 1
            replayed += int(s._graph_ok(16))
            r = s.cycle_graph(16)
        else:
            r = s.cycle(bs, ahead_ok=bs == 16)
        taus.append(r.tau)
    assert s.finish()[0].tolist() == G[:41 + n_new].tolist()
    assert recaptured == 1 and replayed >= 6, (recaptured, replayed)
    del junk


def test_generate_loop_with_graph_replay_env(monkeypatch):
    """DFL_GRAPH=1: dflash_generate replays its steady-state cycles from the captured graphs — same ids, same acceptance
    lengths as the eager loop (model/dflash.py:235-268 per cycle either way)."""
    from dflash_amd import NativeTarget, dflash_generate
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=5)
    prompt = torch.randint(0, 2000, (1, 33), generator=torch.Generator().manual_seed(4)).to(dev())
    n_new = 120
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = H.make_plan(64, 16, 17)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000

    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DFL_GRAPH", mode)
        r = dflash_generate(make_model(cfg), NativeTarget(hf), prompt, cfg.mask_token_id, n_new, 16, None, 0.0,
                            draft_token_hook=hook)
        assert r.output_ids[0].tolist() == G[:33 + n_new].tolist(), mode
        runs[mode] = r
    assert runs["0"].acceptance_lengths == runs["1"].acceptance_lengths
    assert runs["1"].replayed_cycles > 0 and runs["0"].replayed_cycles == 0


class _ScriptedSizes:
    """A scheduler with the attributes run_decode's cycle trace reads (dflash_amd/scheduler.py) that walks a fixed list of
    block sizes: the measured cycle time cannot change what the two runs of a test do."""

    def __init__(self, sizes, candidates):
        self.sizes, self.candidates = list(sizes), sorted(candidates)
        self.current = self.candidates[-1]
        self.tau_hat = dict.fromkeys(self.candidates)
        self.cycle_hat = dict.fromkeys(self.candidates)
        self.score_hat = dict.fromkeys(self.candidates)
        self.adl_lgen_hat = self.adl_lacc_hat = None
        self.adl_target_k = self.adl_target_bs = self.candidates[-1]
        self.seen = []

    def select(self, cyc):
        self.current = self.sizes[cyc % len(self.sizes)]
        return self.current

    def update(self, **kw):
        self.seen.append((kw["effective_bs"], kw["tau"]))


def test_policy_loop_by_graph_replay_equals_the_eager_policy_loop(monkeypatch):
    """The dynamic-schedule loop (benchmark_dynamic_schedule.py:319-379) with one pair of hipGraphs per candidate size
    (DecodeSession.capture_sizes / cycle_sized; DFL_GRAPH=1): ids, acceptance lengths and the sizes used equal the eager
    loop's, through size changes every cycle, the clamped tail (sizes that were never captured) and cycle 0."""
    from dflash_amd import NativeTarget
    from dflash_amd.generate import dflash_generate_policy
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=6)
    prompt = torch.randint(0, 2000, (1, 37), generator=torch.Generator().manual_seed(8)).to(dev())
    n_new = 171
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = H.make_plan(96, 16, 23)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000

    sizes = [16, 8, 12, 12, 16, 8, 8, 12]
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("DFL_GRAPH", mode)
        sched = _ScriptedSizes(sizes, (8, 12, 16))
        r = dflash_generate_policy(model=make_model(cfg), target=NativeTarget(hf), input_ids=prompt,
                                   mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, stop_token_ids=None, temperature=0.0,
                                   scheduler=sched, draft_token_hook=hook)
        assert r.output_ids[0].tolist() == G[:37 + n_new].tolist(), mode
        runs[mode] = (r, sched)
    a, b = runs["0"], runs["1"]
    assert a[0].acceptance_lengths == b[0].acceptance_lengths and a[0].used_block_sizes == b[0].used_block_sizes
    assert a[1].seen == b[1].seen and len(set(a[0].used_block_sizes)) >= 3
    assert b[0].replayed_cycles > 0 and a[0].replayed_cycles == 0


def test_cycle_sized_replays_and_falls_back():
    """DecodeSession.cycle_sized: replayed for captured sizes, eager for the others (and when events are recorded), and a
    session may go back and forth between cycle(), cycle_sized() and sizes freely."""
    from dflash_amd import NativeTarget
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    cfg = H.tiny_cfg()
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=9)
    prompt = torch.randint(0, 2000, (1, 29), generator=torch.Generator().manual_seed(5)).to(dev())
    n_new = 160
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = H.make_plan(96, 16, 31)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000

    s = DecodeSession(make_model(cfg), NativeTarget(hf), prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=n_new,
                      max_block_size=16, stop_token_ids=None, temperature=0.0, draft_token_hook=hook)
    s.prefill()
    s.cycle(16)
    s.capture_sizes((8, 16))
    seq = [16, 8, 10, 16, 16, 8, 5, 8, 16, 12, 8]      # 10, 5, 12 were not captured: eager
    replayed, i, taus = 0, 0, []
    while s.start < s.max_length:
        bs = min(seq[i % len(seq)], s.max_length - s.start)
        if i % 4 == 3:
            r = s.cycle(bs)                        # an eager cycle in between
        else:
            replayed += int(s._sized_ok(bs))
            r = s.cycle_sized(bs)
        taus.append(r.tau)
        assert 1 <= r.tau <= bs
        i += 1
    assert s.finish()[0].tolist() == G[:29 + n_new].tolist()
    assert replayed >= 8, replayed


def _replay_case(seed, n_prompt, n_new, plan):
    """The tiny target with a known greedy walk G, a prompt, and the hook that scripts plan[call] agreeing draft tokens."""
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=seed)
    prompt = torch.randint(0, 2000, (1, n_prompt), generator=torch.Generator().manual_seed(seed)).to(dev())
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000
    return hf, prompt, G, hook


def test_fresh_session_has_its_replay_state():
    """Every replay attribute exists from __init__ on: nothing is captured, nothing can be replayed, no AttributeError."""
    from dflash_amd import NativeTarget
    from dflash_amd.generate import DecodeSession
    cfg = H.tiny_cfg()
    hf, prompt, _, hook = _replay_case(7, 30, 48, H.make_plan(16, 16, 3))
    s = DecodeSession(make_model(cfg), NativeTarget(hf), prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=48,
                      max_block_size=16, stop_token_ids=None, temperature=0.0, draft_token_hook=hook)
    assert s._graph_bs is None
    assert s._graph_ok(16) is False and s._sized_ok(16) is False
    assert s.replay_uncovered((16,), ahead=True) is None and s.replay_uncovered((8, 16)) is None


@pytest.mark.parametrize("case", ["torch_sampler_at_T", "mask_id_among_stop_ids"])
def test_uncovered_session_raises_graph_not_covered(case):
    """A session the graphs do not cover says why (replay_uncovered) and raises GraphNotCovered from both captures, with
    every state precondition met (a cycle has run); dflash_generate runs such a request with eager cycles only."""
    from dflash_amd import NativeTarget, dflash_generate
    from dflash_amd.generate import DecodeSession, GraphNotCovered
    cfg = H.tiny_cfg()
    hf, prompt, _, hook = _replay_case(7, 30, 48, H.make_plan(64, 16, 3))
    kw = (dict(stop_token_ids=None, temperature=0.7, sampler="torch") if case == "torch_sampler_at_T"
          else dict(stop_token_ids=[cfg.mask_token_id], temperature=0.0))
    m, nt = make_model(cfg), NativeTarget(hf)
    s = DecodeSession(m, nt, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=48, max_block_size=16,
                      draft_token_hook=hook, **kw)
    s.prefill()
    s.cycle(16, ahead_ok=True)
    for sizes, ahead in (((16,), True), ((8, 16), False)):
        why = s.replay_uncovered(sizes, ahead=ahead)
        assert isinstance(why, str) and why, (sizes, why)
    with pytest.raises(GraphNotCovered):
        s.capture(16)
    with pytest.raises(GraphNotCovered):
        s.capture_sizes((8, 16))
    assert s._graph_bs is None and not s._sized_ok(16)
    if case == "torch_sampler_at_T":
        r = dflash_generate(m, nt, prompt, cfg.mask_token_id, 48, 16, None, 0.7, draft_token_hook=hook, sampler="torch")
        assert r.replayed_cycles == 0 and len(r.acceptance_lengths) > 0


def test_capture_failure_other_than_coverage_propagates(monkeypatch):
    """run_decode answers GraphNotCovered with eager cycles and nothing else: an error raised inside a capture (here a
    host-side stub in place of capture_graph; no launch is made to fail) leaves dflash_generate as it is."""
    import dflash_amd.generate as gen
    from dflash_amd import NativeTarget, dflash_generate
    cfg = H.tiny_cfg()
    hf, prompt, _, hook = _replay_case(7, 30, 48, H.make_plan(64, 16, 3))

    def boom(fn):
        raise RuntimeError("boom")

    monkeypatch.setenv("DFL_GRAPH", "1")
    monkeypatch.setattr(gen, "capture_graph", boom)
    with pytest.raises(RuntimeError, match="boom") as e:
        dflash_generate(make_model(cfg), NativeTarget(hf), prompt, cfg.mask_token_id, 48, 16, None, 0.0,
                        draft_token_hook=hook)
    assert not isinstance(e.value, gen.GraphNotCovered)
    torch.cuda.synchronize()


def test_replay_forms_agree_under_both_result_modes(monkeypatch):
    """The hand-over's two branches — pinned host memory polled on the cycle counter (DFL_HOST_RESULT=1, the default)
    and a device buffer read with .tolist() (=0) — under cycle_graph and under cycle_sized: ids are the greedy walk and
    the acceptance lengths are the same in both modes, with cycles really replayed in each."""
    from dflash_amd import NativeTarget
    from dflash_amd.generate import DecodeSession
    cfg = H.tiny_cfg()
    n_new = 40
    plan = [0, 1, 2, 0, 1, 0, 3, 1] * 5   # short acceptances: several cycles start early enough to be replayed (_graph_ok)
    hf, prompt, G, hook = _replay_case(11, 31, n_new, plan)
    m, nt = make_model(cfg), NativeTarget(hf)

    def run(form):
        s = DecodeSession(m, nt, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, max_block_size=16,
                          stop_token_ids=None, temperature=0.0, draft_token_hook=hook)
        s.prefill()
        taus, replayed, i = [], 0, 0
        while s.start < s.max_length:
            left = s.max_length - s.start
            if form == "fixed":
                if i == 2:
                    s.capture(16)
                bs = min(16, left)
                r = s.cycle_graph(16) if (i >= 2 and bs == 16) else s.cycle(bs, ahead_ok=bs == 16)
            else:
                if i == 1:
                    s.capture_sizes((8, 16))
                bs = min((16, 8)[i % 2], left)
                r = s.cycle_sized(bs) if i >= 1 else s.cycle(bs)
            taus.append(r.tau)
            replayed += int(r.replayed)
            i += 1
        assert s.finish()[0].tolist() == G[:31 + n_new].tolist(), form
        return taus, replayed

    runs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DFL_HOST_RESULT", mode)
        for form in ("fixed", "sized"):
            taus, replayed = runs[mode, form] = run(form)
            assert replayed >= 3, (mode, form, replayed)
    for form in ("fixed", "sized"):
        assert runs["0", form][0] == runs["1", form][0], form
