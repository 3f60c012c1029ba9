"""e4m3 KV cache on the GPU (csrc/attn_head_kv8.hip): dfl_kv_quant_rows bit for bit against the host rule, dfl_attn_head_kv8
against fp64 attention over the dequantised cache, and a kv_format="fp8_e4m3" target as one model: the same outputs however
the tokens are cut into prefill and blocks, and a speculative loop that emits the target's own greedy continuation."""
import functools

import pytest
import torch

import attn_keys_ref as R
import helpers as H
from kv8_rows import edge_rows

pytestmark = pytest.mark.gpu
BF16, U8 = torch.bfloat16, torch.uint8
NAN = float("nan")
NAN_CODE = 0x7F   # e4m3fn NaN: a stale cache byte that must never reach a product


def dev():
    return torch.device("cuda", 0)


# ---------------------------------------------------------------- dfl_kv_quant_rows
@pytest.mark.parametrize("row0", [0, 5])
@pytest.mark.parametrize("P", [1, 17, 33])
def test_kv_quant_rows_equals_the_host_rule(P, row0):
    """Codes, scales and the written-back rows bit-equal to ops.quantize_kv_rows / dequantize_kv_rows on the host, the edge
    rows of the CPU test among them; cache rows outside [row0, row0 + P) and source rows >= P untouched."""
    from dflash_amd import ops
    n_kv, rows, src_rows = 2, 44, 40
    g = torch.Generator().manual_seed(P + row0)
    src = [(torch.randn(n_kv, src_rows, 128, generator=g) * torch.exp2(torch.randint(-9, 9, (n_kv, src_rows, 1), generator=g))).to(BF16)
           for _ in range(2)]
    e = edge_rows()
    for i in range(P):   # K head 0 and V head 1 carry the edge rows
        src[0][0, i], src[1][1, i] = e[i % 8], e[(i + 3) % 8]
    codes = [torch.full((n_kv, rows, 128), NAN_CODE, dtype=U8, device=dev()) for _ in range(2)]
    scales = [torch.full((n_kv, rows), NAN, device=dev()) for _ in range(2)]
    got = [s.to(dev()) for s in src]
    ops.kv_quant_rows(got[0], got[1], P, codes[0], codes[1], scales[0], scales[1], row0)
    for t in range(2):
        q, s = ops.quantize_kv_rows(src[t][:, :P])
        c, sc = codes[t].cpu(), scales[t].cpu()
        assert torch.equal(c[:, row0:row0 + P], q) and torch.equal(sc[:, row0:row0 + P], s), t
        assert torch.equal(got[t].cpu()[:, :P].view(torch.int16), ops.dequantize_kv_rows(q, s).view(torch.int16)), t
        assert torch.equal(got[t].cpu()[:, P:].view(torch.int16), src[t][:, P:].view(torch.int16)), t
        out = torch.ones(rows, dtype=torch.bool)
        out[row0:row0 + P] = False
        assert bool((c[:, out] == NAN_CODE).all()) and bool(torch.isnan(sc[:, out]).all()), t


# ---------------------------------------------------------------- dfl_attn_head_kv8
@functools.lru_cache(maxsize=None)
def _tables():
    cos, sin = R.rope_tables_identity(2048)
    return cos.to(dev()), sin.to(dev())


@functools.lru_cache(maxsize=4)
def _keys(S, n_q, n_kv, bs):
    """q, and K / V rows whose row j is multiplied by 2^((5j + phase) mod 13 - 6), K and V at different phases: a scale
    taken from a neighbouring key or from the other tensor is off by a factor.  Returns q, the rows as the Linear would
    give them, what the cache must hold for ALL of them, and the fp64 result over the dequantised rows."""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(31 * S + n_q + bs)
    n = S + bs
    j = torch.arange(n)
    q = torch.randn(bs, n_q, 128, generator=g).to(BF16)
    raw = [(torch.randn(n_kv, n, 128, generator=g) * torch.exp2(((5 * j + ph) % 13 - 6).float())[None, :, None]).to(BF16)
           for ph in (0, 4)]
    quant = [ops.quantize_kv_rows(x) for x in raw]
    deq = [ops.dequantize_kv_rows(*qs) for qs in quant]
    ref, _ = R.attention_ref(q, deq[0], deq[1], R.decode_visibility(S, 0, bs, True))
    return q, raw, quant, deq, ref


def _block_rows(q, k_new, v_new, tiles):
    bs, n_q, n_kv = q.shape[0], q.shape[1], k_new.shape[0]
    x = torch.zeros(16 * tiles, (n_q + 2 * n_kv) * 128, dtype=BF16)
    x[:bs] = torch.cat([q.reshape(bs, -1), k_new.transpose(0, 1).reshape(bs, -1), v_new.transpose(0, 1).reshape(bs, -1)], dim=1)
    return x.to(dev())


@pytest.mark.parametrize("n_q,n_kv", [(2, 2), (8, 2)])
@pytest.mark.parametrize("old_splits", [1, 8])
@pytest.mark.parametrize("S", [0, 1, 31, 32, 33, 261, 529])
def test_attn_head_kv8_against_fp64_over_the_dequantised_cache(S, old_splits, n_q, n_kv):
    """bs 1 and 16 (one query tile) and 20 (two), lengths as immediates and from dyn with the launch sized 40 keys above
    the record.  old_splits: how many splits the cached keys may get (max_splits = old_splits + 1: the new rows are a split
    of their own, and with max_splits = 1 no launch of this family attends a cached key) — one split at S = 529 is a wave
    walking three tiles.  Bar: max-abs error <= 2^-6 of the fp64 result's largest value, the bar test_hip_attn_keys.py
    holds dfl_attn_head to.  Append: cache rows [S, S + bs) bit-equal to ops.quantize_kv_rows of the rows the bf16
    dfl_attn_head appends from the same inputs; rows beyond untouched, rows < S unchanged."""
    from dflash_amd import ops
    cos, sin = _tables()
    for bs in (1, 16, 20):
        tiles = 1 if bs <= 16 else 2
        q, raw, quant, deq, ref = _keys(S, n_q, n_kv, bs)
        xq = _block_rows(q, raw[0][:, S:], raw[1][:, S:], tiles)
        rows = (S + bs + 40 + 16 + 3) // 4 * 4
        qd = n_q * 128
        common = dict(xq=xq, q_col=0, k_col=qd, v_col=qd + n_kv * 128, n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None,
                      eps=1e-6, cos_tab=cos, sin_tab=sin, scale=R.SCALE, causal=True, tau=0, bs=bs, pos0=S,
                      max_splits=old_splits + 1, q_tiles=tiles, out_tile_stride=16 * qd)
        # the rows the bf16 stage appends from the same inputs (its cache holds the dequantised prefix)
        kb, vb = (torch.full((n_kv, rows, 128), NAN, dtype=BF16, device=dev()) for _ in range(2))
        kb[:, :S], vb[:, :S] = deq[0][:, :S].to(dev()), deq[1][:, :S].to(dev())
        ws = ops.attn_head_ws(n_q, old_splits + 1, tiles, dev())
        ops.attn_head(**common, kcache=kb, vcache=vb, S=S, ws=ws, out_frag=torch.zeros(tiles, 16 * qd, dtype=BF16, device=dev()))
        want = [ops.quantize_kv_rows(x[:, S:S + bs].cpu()) for x in (kb, vb)]
        for use_dyn in (False, True):
            codes = [torch.full((n_kv, rows, 128), NAN_CODE, dtype=U8, device=dev()) for _ in range(2)]
            scales = [torch.full((n_kv, rows), NAN, device=dev()) for _ in range(2)]
            for t in range(2):
                codes[t][:, :S], scales[t][:, :S] = quant[t][0][:, :S].to(dev()), quant[t][1][:, :S].to(dev())
            dyn = None
            if use_dyn:
                dyn = torch.zeros(8, dtype=torch.int32, device=dev())
                ops.set_dyn(dyn, S, 0, bs, S)
            out = torch.full((tiles, 16 * qd), NAN, dtype=BF16, device=dev())
            ops.attn_head_kv8(**common, kcache=codes[0], vcache=codes[1], k_scale=scales[0], v_scale=scales[1],
                              S=S + 40 if use_dyn else S, dyn=dyn, ws=ws, out_frag=out)
            got = torch.cat([H.unfrag(t, qd) for t in out])[:bs].reshape(bs, n_q, 128).cpu()
            name = f"S={S} bs={bs} dyn={use_dyn}"
            assert torch.isfinite(got.float()).all(), name
            err = float((got.double() - ref).abs().max() / ref.abs().max())
            print(f"[kv8] attn_head_kv8 ({n_q},{n_kv}) old_splits={old_splits} {name}: max-abs error {err:.3e} of scale")
            assert err <= 2.0 ** -6, (name, err)
            for t in range(2):
                c, sc = codes[t].cpu(), scales[t].cpu()
                assert torch.equal(c[:, S:S + bs], want[t][0]) and torch.equal(sc[:, S:S + bs], want[t][1]), (name, t)
                assert torch.equal(c[:, :S], quant[t][0][:, :S]) and torch.equal(sc[:, :S], quant[t][1][:, :S]), (name, t)
                assert bool((c[:, S + bs:] == NAN_CODE).all()) and bool(torch.isnan(sc[:, S + bs:]).all()), (name, t)


@pytest.mark.parametrize("S", [0, 33])
def test_attn_head_kv8_at_max_splits_1(S):
    """max_splits = 1 leaves no split for cached keys: admitted at S = 0 with immediate lengths (and right), refused with
    cached keys (dfl_attn_head would attend none of them)."""
    from dflash_amd import ops
    n_q, n_kv, bs, qd = 2, 2, 16, 256
    cos, sin = _tables()
    q, raw, quant, deq, ref = _keys(S, n_q, n_kv, bs)
    rows = (S + 16 + 3) // 4 * 4
    codes = [torch.zeros(n_kv, rows, 128, dtype=U8, device=dev()) for _ in range(2)]
    scales = [torch.ones(n_kv, rows, device=dev()) for _ in range(2)]
    out = torch.zeros(1, 16 * qd, dtype=BF16, device=dev())
    call = lambda: ops.attn_head_kv8(      # noqa: E731
        xq=_block_rows(q, raw[0][:, S:], raw[1][:, S:], 1), q_col=0, k_col=qd, v_col=qd + n_kv * 128, n_q=n_q, n_kv=n_kv,
        q_norm_w=None, k_norm_w=None, eps=1e-6, cos_tab=cos, sin_tab=sin, kcache=codes[0], vcache=codes[1], k_scale=scales[0],
        v_scale=scales[1], scale=R.SCALE, causal=True, S=S, bs=bs, pos0=S, ws=ops.attn_head_ws(n_q, 1, 1, dev()), max_splits=1,
        out_frag=out)
    if S:
        with pytest.raises(Exception, match="max_splits >= 2"):
            call()
        return
    call()
    got = H.unfrag(out[0], qd)[:bs].reshape(bs, n_q, 128).cpu()
    assert float((got.double() - ref).abs().max() / ref.abs().max()) <= 2.0 ** -6


# ---------------------------------------------------------------- the target
DIMS = {**H.TINY_TARGET, "num_layers": 6, "intermediate_size": 704}   # (the small fp8-target of test_hip_fp8_target.py)
TAPS = [1, 3]


@functools.lru_cache(maxsize=None)
def _targets():
    """One walk model (synthetic.impose_greedy_walk) under a bf16-cache and an e4m3-cache NativeTarget."""
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
    torch.manual_seed(11)
    hf = make_hf_qwen3(DIMS, dev(), dtype=BF16)
    impose_greedy_walk(hf, seed=5)
    return NativeTarget(hf), NativeTarget(hf, kv_format="fp8_e4m3")


@functools.lru_cache(maxsize=None)
def _peaky_targets():
    """The same widths at HF's random init with every q_norm weight times 4: scores of standard deviation ~4, so a softmax
    rests on a few keys and a K / V row moved by e4m3's step moves the layer's output at first order (under the walk
    model's wide margins, and with flat softmaxes, it does not: profiles/kv8_tests.txt)."""
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import make_hf_qwen3
    torch.manual_seed(11)
    hf = make_hf_qwen3(DIMS, dev(), dtype=BF16)
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if n.endswith("q_norm.weight"):
                p.mul_(4)
    return NativeTarget(hf), NativeTarget(hf, kv_format="fp8_e4m3")


def _three_ways(t, ids, P):
    """(taps, logits) of rows P .. P + 15 from (a) a verify of 16 after a prefill of P, (b) verifies of 7 then 9, and, taps
    only, (c) a prefill of P + 16."""
    def run(cuts):
        cache = t.new_cache(P + 64)
        t.prefill(ids[:, :P], cache, tap_layers=TAPS)
        taps, logits, at = [], [], P
        for n in cuts:
            lo = torch.zeros(32, t.V, dtype=BF16, device=dev())
            _, th = t.verify(ids[0, at:at + n], at, cache, tap_layers=TAPS, logits_out=lo)
            taps.append(th[:n].float().clone())
            logits.append(lo[:n].float().clone())
            at += n
        return torch.cat(taps), torch.cat(logits)
    a, b = run((16,)), run((7, 9))
    hs = t.prefill(ids[:, :P + 16], t.new_cache(P + 64), tap_layers=TAPS).hidden_states
    c = torch.cat([hs[l + 1][0, P:P + 16] for l in TAPS], dim=1).float()
    return a, b, c


def _worst(a, b, c):
    d = lambda x, y: float((x - y).abs().max() / x.abs().max())   # noqa: E731
    return max(d(a[0], b[0]), d(a[0], c), d(b[0], c)), d(a[1], b[1])


@pytest.mark.parametrize("P", [45, 130])
def test_kv8_target_does_not_depend_on_the_partition(P):
    """The e4m3-cache target's taps and logits of 16 rows, three ways (_three_ways), lie as close together as the bf16-cache
    target's do, where only the accumulation order differs: at most four times the bf16 target's worst relative distance
    (measured in the same test).  A stage that attended new rows unquantised, or a prefill that attended the unrounded
    scratch, would move K / V by e4m3's 2^-4 relative step.  Model: hidden 512, 6 layers, q_norm weights x 4
    (_peaky_targets).  Measured there (profiles/kv8_tests.txt), taps: bf16 2.2e-2 / 3.3e-2 (P = 45 / 130), e4m3 5.6e-2 /
    3.4e-2, and with a prefill that attends the unrounded scratch 1.9e-1 / 3.2e-1 — 8.6 and 9.7 times the bf16 distance,
    outside the bound.  (On the walk model the same fault stayed inside it: 1.0 and 2.0 times.)
    Also here: the rows the prefill attended — the last layer's scratch — ARE the cache's rows dequantised, bit for bit."""
    from dflash_amd import ops
    t16, t8 = _peaky_targets()
    ids = torch.randint(0, 2000, (1, P + 16), generator=torch.Generator().manual_seed(P)).to(dev())
    base, got = _worst(*_three_ways(t16, ids, P)), _worst(*_three_ways(t8, ids, P))
    print(f"[kv8] partition P={P}: taps bf16 {base[0]:.3e} e4m3 {got[0]:.3e}; logits bf16 {base[1]:.3e} e4m3 {got[1]:.3e}")
    assert got[0] <= 4 * base[0] and got[1] <= 4 * base[1], (base, got)
    cache = t8.new_cache(P + 16)
    t8.prefill(ids[:, :P], cache)
    for scratch, codes, scale in ((t8._pf["kv8_k"], cache.k, cache.k_scale), (t8._pf["kv8_v"], cache.v, cache.v_scale)):
        want = ops.dequantize_kv_rows(codes[-1, :, :P], scale[-1, :, :P])
        assert torch.equal(scratch[:, :P].view(torch.int16), want.view(torch.int16))


def test_kv8_wide_block_in_two_passes_and_refusals():
    """A 20-row block with wide_one_pass off (every GEMM once per tile, one attention launch with two query tiles) against
    the one-pass form: as close as the bf16-cache target's two forms are, times four.  Then what such a target refuses."""
    from dflash_amd.candidates import NativeCandidateVerifier
    t16, t8 = _peaky_targets()
    P = 45
    ids = torch.randint(0, 2000, (1, P + 20), generator=torch.Generator().manual_seed(7)).to(dev())

    def dist(t):
        outs = []
        for one_pass in (True, False):
            t.wide_one_pass = one_pass
            cache = t.new_cache(P + 64)
            t.prefill(ids[:, :P], cache, tap_layers=TAPS)
            lo = torch.zeros(32, t.V, dtype=BF16, device=dev())
            _, th = t.verify(ids[0, P:], P, cache, tap_layers=TAPS, logits_out=lo)
            outs.append((th[:20].float().clone(), lo[:20].float().clone()))
        t.wide_one_pass = True
        return [float((a - b).abs().max() / a.abs().max()) for a, b in zip(*outs)]

    base, got = dist(t16), dist(t8)
    print(f"[kv8] wide block, one pass vs two: taps / logits bf16 {base} e4m3 {got}")
    assert got[0] <= 4 * base[0] and got[1] <= 4 * base[1], (base, got)
    with pytest.raises(NotImplementedError, match="NativeCandidateVerifier"):
        NativeCandidateVerifier(t8, len(TAPS))
    cache = t8.new_cache(P + 64)
    try:
        t8.prefill_attn = "sdpa"
        with pytest.raises(NotImplementedError, match="sdpa"):
            t8.prefill(ids[:, :P], cache)
        t8.prefill_attn = "native"
        t8.prefill(ids[:, :P], cache)
        t8.fuse_oproj = True
        with pytest.raises(NotImplementedError, match="fuse_oproj"):
            t8.verify(ids[0, P:P + 16], P, cache)
    finally:
        t8.prefill_attn, t8.fuse_oproj = "native", False


def test_kv8_target_greedy_loop_is_lossless_and_replays(monkeypatch):
    """dflash_generate on the e4m3-cache target with scripted acceptance emits the ids of that target's own block-size-1
    greedy continuation — eager and replayed (DFL_GRAPH), at block sizes 16 and 24."""
    from dflash_amd import DFlashDraftModel, dflash_generate
    _, t8 = _targets()
    P, n_new = 33, 90
    prompt = torch.randint(0, 2000, (1, P), generator=torch.Generator().manual_seed(40)).to(dev())
    cache = t8.new_cache(P + n_new + 8)
    G = prompt[0].tolist() + [int(t8.prefill(prompt, cache).logits[0, -1].argmax())]
    for at in range(P, P + n_new - 1):
        post, _ = t8.verify(torch.tensor(G[-1:], device=dev()), at, cache)
        G.append(int(post[0, 0]))
    Gt = torch.tensor(G + [0] * 32, device=dev())
    cfg = H.tiny_cfg()
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))

    def hook_for(plan):
        def hook(blk, start, call):
            k = min(plan[call % len(plan)], blk.shape[1] - 1)
            blk[0, 1:k + 1] = Gt[start + 1:start + k + 1]
        return hook

    for bs in (16, 24):
        runs = {}
        for mode in ("0", "1"):
            monkeypatch.setenv("DFL_GRAPH", mode)
            runs[mode] = dflash_generate(m, t8, prompt, cfg.mask_token_id, n_new, bs, None, 0.0,
                                         draft_token_hook=hook_for(H.make_plan(64, bs, 17)))
            assert runs[mode].output_ids[0].tolist() == G, (bs, mode)
        assert runs["0"].acceptance_lengths == runs["1"].acceptance_lengths and max(runs["0"].acceptance_lengths) > 8
        if bs == 16:
            assert runs["1"].replayed_cycles > 0 and runs["0"].replayed_cycles == 0
