"""FP8 (e4m3) weight streaming on the GPU: the W8 skinny GEMM kernels against torch on exact
operands and against fp64 on the dequantised weights, the fp8 draft model against its own bf16 fallback copy and
against a bf16 model loaded with q * scale, and the decode loops' losslessness with an fp8 draft."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def dev():
    return torch.device("cuda", 0)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def unfrag(frag, K):
    return frag.view(K // 8, 16, 8).permute(1, 0, 2).reshape(16, K)


def to_frag(ops, x):   # x [16, K] bf16 on the GPU, every row packed as it is (NaN rows included)
    out = torch.empty(16 * x.shape[1], dtype=BF16, device=x.device)
    ops.pack_rows(x, 16, out)
    return out


def codes_of(w):
    """e4m3 codes of values that e4m3 holds exactly (small integers)."""
    q = w.float().to(F8)
    assert torch.equal(q.float(), w.float())
    return q.view(torch.uint8).contiguous()


def int_weight(ops, N, K, g, lo=-8, hi=8):
    """Integer weight rows in [lo, hi] with the scales 2^((n % 5) - 2): (Fp8Weight, dequantised fp64 [N, K])."""
    w = torch.randint(lo, hi + 1, (N, K), generator=g).float()
    scale = torch.tensor([2.0 ** ((n % 5) - 2) for n in range(N)])
    return ops.pack_weight_fp8(codes_of(w).to(dev()), scale.to(dev())), w.double() * scale.double()[:, None]


# ------------------------------------------------------------------ 3. every code
def test_every_e4m3_code_converts_exactly(ops):
    """A [16, 64] weight whose 1024 entries run through all 254 finite e4m3 codes (subnormals and both zeros included),
    scale 1, one-hot activation rows selecting 16 k's per launch: the logits of dfl_gemm_argmax (e4m3) are the codes'
    values in bf16, bit for bit — the conversion and the byte layout.  (Code 0x80: the K-sum of +0 products and one -0
    is +0 in IEEE arithmetic, so a zero is compared as a zero, every other value by its bits.)"""
    finite = torch.tensor([c for c in range(256) if (c & 0x7F) != 0x7F], dtype=torch.uint8)
    assert finite.numel() == 254
    q = finite[(torch.arange(1024) * 37 + 11) % 254].view(16, 64).contiguous()   # 37 is coprime to 254: all codes appear
    assert torch.unique(q).numel() == 254
    val = q.view(F8).float()
    w8 = ops.pack_weight_fp8(q.to(dev()), torch.ones(16, device=dev()))
    ws = ops.argmax_ws(dev())
    for j in range(4):
        x = torch.zeros(16, 64, dtype=BF16)
        x[torch.arange(16), 16 * j + torch.arange(16)] = 1.0
        logits = torch.full((16, 16), float("nan"), dtype=BF16, device=dev())
        ids = torch.zeros(16, dtype=torch.long, device=dev())
        ops.gemm_argmax(w8, ops.rows_plain(x.to(dev())), 16, 64, 0, 16, ws, ids, 0, logits=logits)
        want = val[:, 16 * j:16 * j + 16].t().contiguous().to(BF16)           # logits[m][n] = W[n][16 j + m]
        got = logits.cpu()
        nz = want != 0
        assert torch.equal(got.view(torch.int16)[nz], want.view(torch.int16)[nz]), j
        assert torch.all(got[~nz] == 0), j
        assert torch.equal(ids.cpu(), want.float().argmax(-1)), j


# ------------------------------------------------------------------ 4. exact integers through gemm_resid
RESID_SHAPES = [(16, 64, 16), (48, 192, 5), (256, 512, 16), (4480, 4096, 16), (256, 12288, 7)]


@pytest.mark.parametrize("add_residual", [False, True])
@pytest.mark.parametrize("N,K,rows", RESID_SHAPES)
def test_gemm_resid_fp8_exact_ints(ops, N, K, rows, add_residual):
    """Weights in [-8, 8], activations in [-4, 4], scales 2^((n % 5) - 2): every sum is exact in fp32 (< 2^24 at
    K = 12288), so h, tap and the sums of squares equal torch's — fragment layout, pairs per wave (nfr rounded up),
    waves without a share, half tiles (no ss_out) and whole tiles (ss_out), the chunked form.  Rows >= `rows` of the
    frag source are NaN: a frag source is not masked, but no valid row may see them."""
    g = gen(N + K + rows)
    w8, wd = int_weight(ops, N, K, g)
    x = torch.randint(-4, 5, (16, K), generator=g).float()
    xp = x.clone()
    xp[rows:] = float("nan")
    h0 = torch.randint(-64, 65, (16, N + 16), generator=g).to(BF16)
    h = h0.to(dev())
    tap = torch.zeros(16, 3 * N, dtype=BF16, device=dev())
    ss = torch.zeros(N, device=dev()) if add_residual else None    # (sums of squares keep whole tiles: no halves)
    ops.gemm_resid(w8, to_frag(ops, xp.to(BF16).to(dev())), N, K, h[:, :N], add_residual=add_residual, ss_out=ss,
                   tap=tap[:, N:2 * N])
    lin = (x.double() @ wd.t()).float().to(BF16)                   # exact sum, scaled, one rounding
    ref = (h0[:, :N].float() + lin.float()).to(BF16) if add_residual else lin
    assert torch.equal(h[:rows, :N].cpu(), ref[:rows])
    assert torch.equal(h[:, N:].cpu(), h0[:, N:])                   # nothing beyond column N
    assert torch.equal(tap[:rows, N:2 * N].cpu(), ref[:rows])
    assert torch.count_nonzero(tap[:, :N]) == 0 and torch.count_nonzero(tap[:, 2 * N:]) == 0
    if ss is not None:
        want = ref[:rows].double().pow(2).view(rows, N // 16, 16).sum(-1).t()      # [tile][row]
        got = ss.view(N // 16, 16)[:, :rows].cpu().double()
        assert torch.allclose(got, want, rtol=2e-6, atol=0)       # 16 fp32 terms in the DPP order


def test_gemm_resid_fp8_row_count_from_dyn_word(ops):
    """Plain rows with the valid count in a dyn word, 4096 -> 512: rows >= dyn[TAU] hold NaN and count as zero."""
    N, K, rows = 512, 4096, 7
    g = gen(77)
    w8, wd = int_weight(ops, N, K, g)
    x = torch.randint(-4, 5, (16, K), generator=g).float()
    xp = x.clone()
    xp[rows:] = float("nan")
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, 0, rows, 16, 0)
    h = torch.full((16, N), 7.0, dtype=BF16, device=dev())
    ss = torch.zeros(N, device=dev())
    ops.gemm_resid(w8, ops.rows_plain(xp.to(BF16).to(dev()), ops.DYN_TAU), N, K, h, add_residual=False, ss_out=ss, dyn=dyn)
    ref = (x.double() @ wd.t()).float().to(BF16)
    assert torch.equal(h[:rows].cpu(), ref[:rows]) and torch.count_nonzero(h[rows:]) == 0
    want = ref[:rows].double().pow(2).view(rows, N // 16, 16).sum(-1).t()
    assert torch.allclose(ss.view(N // 16, 16)[:, :rows].cpu().double(), want, rtol=2e-6, atol=0)
    assert torch.count_nonzero(ss.view(N // 16, 16)[:, rows:]) == 0


def test_gemm_resid_fp8_normalised_source(ops):
    """4096 -> 512 from the residual stream + sums of squares (the RMSNorm in the GEMM's prologue) against the oracle's
    rms_norm and fp64 on the dequantised weights; the bar of test_gemm_row_sources_and_resid_epilogue for this source
    (1-ulp flips of the normalised inputs: 2e-2 / 1e-3 of the scale)."""
    from oracle.dflash_oracle import rms_norm
    N, K, bs = 512, 4096, 11
    g = gen(78)
    w = (torch.randn(N, K, generator=g) * 0.03).to(BF16)
    q, sc = ops.quantize_fp8_rows(w.to(dev()))
    wd = ops.dequantize_fp8_rows(q, sc).cpu().double()
    hrows = (torch.randn(16, K, generator=g) * 0.7).to(BF16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16)
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, 0, 7, bs, 0)
    ss0 = hrows.float().pow(2).sum(-1).to(dev())
    out = torch.zeros(16, N, dtype=BF16, device=dev())
    ops.gemm_resid(ops.pack_weight_fp8(q, sc), ops.rows_normed(hrows.to(dev()), ss0, 1, nw.to(dev()), 1e-6, ops.DYN_BS),
                   N, K, out, add_residual=False, dyn=dyn)
    ref = (rms_norm(hrows, nw, 1e-6).double() @ wd.t()).float()
    d = (out[:bs].cpu().float() - ref[:bs]).abs()
    print(f"[fp8] normalised source: max {float(d.max() / ref.abs().max()):.3e} mean {float(d.mean() / ref.abs().max()):.3e}")
    assert d.max() <= 2e-2 * ref.abs().max() and d.mean() <= 1e-3 * ref.abs().max()
    assert torch.count_nonzero(out[bs:]) == 0


# ------------------------------------------------------------------ 5. SiLU
def _gateup(ops, wg, sg, wu, su):
    return ops.pack_weight_gateup_fp8(codes_of(wg).to(dev()), sg.to(dev()), codes_of(wu).to(dev()), su.to(dev()))


def test_gemm_silu_mul_fp8_exact_ints(ops):
    """Integer operands at (I 64, K 512), distinct scales for gate rows (2^((n % 5) - 2)) and up rows (2^(1 - n % 3)):
    a gate / up mix-up in the packed scale order would show.  Bar of test_gemm_silu_mul_exact_ints (__expf vs exp)."""
    I, K = 64, 512
    g = gen(7)
    wg = torch.randint(-8, 9, (I, K), generator=g).float()
    wu = torch.randint(-8, 9, (I, K), generator=g).float()
    sg = torch.tensor([2.0 ** ((n % 5) - 2) for n in range(I)])
    su = torch.tensor([2.0 ** (1 - (n % 3)) for n in range(I)])
    x = torch.zeros(16, K, dtype=BF16)
    x[:, :8] = torch.randint(-1, 2, (16, 8), generator=g).to(BF16)
    act = torch.empty(16 * I, dtype=BF16, device=dev())
    ops.gemm_silu_mul(_gateup(ops, wg, sg, wu, su), to_frag(ops, x.to(dev())), I, K, act)
    gl = ((x.double() @ wg.double().t()) * sg.double()).float().to(BF16).float()
    ul = ((x.double() @ wu.double().t()) * su.double()).float().to(BF16).float()
    ref = (torch.nn.functional.silu(gl).to(BF16).float() * ul).to(BF16).float()
    got = unfrag(act, I).float().cpu()
    assert (got - ref).abs().max() <= 2 ** -7 * max(1.0, float(ref.abs().max()))


def test_gemm_silu_mul_fp8_random(ops):
    """Random bf16 at (I 2560, K 1024) through the normalised-source-free path against fp64 on the dequantised weights
    with the same rounding points; bar of test_gemm_silu_mul: 2^-6 of the scale, under 5 % of elements differing."""
    I, K = 2560, 1024
    g = gen(6)
    wg = (torch.randn(I, K, generator=g) * 0.05).to(BF16).to(dev())
    wu = (torch.randn(I, K, generator=g) * 0.11).to(BF16).to(dev())     # another amax: other scales than the gate rows'
    x = torch.randn(16, K, generator=g).to(BF16).to(dev())
    (qg, sg), (qu, su) = ops.quantize_fp8_rows(wg), ops.quantize_fp8_rows(wu)
    assert not torch.equal(sg, su)
    act = torch.empty(16 * I, dtype=BF16, device=dev())
    ops.gemm_silu_mul(ops.pack_weight_gateup_fp8(qg, sg, qu, su), to_frag(ops, x), I, K, act)
    got = unfrag(act, I).float()
    gl = (x.double() @ ops.dequantize_fp8_rows(qg, sg).double().t()).float().to(BF16)
    ul = (x.double() @ ops.dequantize_fp8_rows(qu, su).double().t()).float().to(BF16)
    ref = (torch.nn.functional.silu(gl.float()).to(BF16).float() * ul.float()).to(BF16).float()
    H.assert_close("fp8 silu_mul (2560, 1024) vs fp64 on q*scale", got, ref, max_rel=2 ** -6)
    assert ((got - ref).abs() > 0).float().mean() < 0.05


# ------------------------------------------------------------------ 6. argmax
@pytest.mark.parametrize("V,K,bs,row0", [(2048, 512, 16, 0), (4096 + 16 * 7, 1024, 12, 1)])
def test_gemm_argmax_fp8_exact_ints(ops, V, K, bs, row0):
    """Integer operands: ids (first index on ties, of which integers give many), logits and top-2 margins are exact."""
    g = gen(V)
    w8, wd = int_weight(ops, V, K, g)
    x = torch.randint(-4, 5, (16, K), generator=g).float()
    ids = torch.full((16,), -1, dtype=torch.long, device=dev())
    margins = torch.full((16,), -1.0, device=dev())
    logits = torch.zeros(16, V, dtype=BF16, device=dev())
    xf = to_frag(ops, x.to(BF16).to(dev()))
    ops.gemm_argmax(w8, xf, V, K, row0, bs - row0, ops.argmax_ws(dev()), ids, row0, logits=logits, margins=margins)
    ref = (x.double() @ wd.t()).float().to(BF16)
    assert torch.equal(logits[row0:bs].cpu(), ref[row0:bs])
    assert torch.equal(ids[row0:bs].cpu(), ref[row0:bs].float().argmax(-1))
    top2 = ref[row0:bs].float().topk(2, dim=-1).values
    assert torch.equal(margins[row0:bs].cpu(), top2[:, 0] - top2[:, 1])
    assert (ids[:row0] == -1).all() and (ids[bs:] == -1).all()
    ids2 = torch.full((16,), -1, dtype=torch.long, device=dev())     # the fused path (no logits written): the same ids
    ops.gemm_argmax(w8, xf, V, K, row0, bs - row0, ops.argmax_ws(dev()), ids2, row0)
    assert torch.equal(ids, ids2)


def test_gemm_argmax_fp8_tie_across_workgroups_after_scaling(ops):
    """Two columns in different workgroups that tie only AFTER scaling (integer 1 at scale 2 in column 5, integer 4 at
    scale 0.5 in column 1000): the first index wins with margin 0; unscaled, column 1000 would."""
    V, K = 2048, 512
    w = torch.full((V, K), -1.0)
    scale = torch.ones(V)
    w[5, :], scale[5] = 1.0, 2.0
    w[1000, :], scale[1000] = 4.0, 0.5
    x = torch.zeros(16, K)
    x[:, 0] = torch.arange(1, 17).float()
    w8 = ops.pack_weight_fp8(codes_of(w).to(dev()), scale.to(dev()))
    ids = torch.full((16,), -1, dtype=torch.long, device=dev())
    margins = torch.full((16,), -1.0, device=dev())
    ops.gemm_argmax(w8, to_frag(ops, x.to(BF16).to(dev())), V, K, 0, 16, ops.argmax_ws(dev()), ids, 0, margins=margins)
    assert ids.tolist() == [5] * 16 and torch.count_nonzero(margins) == 0


def test_gemm_argmax_fp8_full_vocabulary(ops):
    """(V 151936, K 4096), random data: ids against fp64 logits of the dequantised weights, where the margin is safe."""
    V, K = 151936, 4096
    gd = torch.Generator(device=dev()).manual_seed(9)
    w = (torch.randn(V, K, generator=gd, device=dev()) * 0.02).to(BF16)
    x = torch.randn(16, K, generator=gd, device=dev()).to(BF16)
    q, sc = ops.quantize_fp8_rows(w)
    del w
    ids = torch.full((16,), -1, dtype=torch.long, device=dev())
    logits = torch.zeros(16, V, dtype=BF16, device=dev())
    ops.gemm_argmax(ops.pack_weight_fp8(q, sc), to_frag(ops, x), V, K, 1, 15, ops.argmax_ws(dev()), ids, 1, logits=logits)
    ref = torch.empty(16, V, dtype=torch.float64, device=dev())
    for n0 in range(0, V, 16384):    # fp64 in slabs: the dequantised slab alone is 0.5 GB
        sl = slice(n0, min(V, n0 + 16384))
        ref[:, sl] = x.double() @ ops.dequantize_fp8_rows(q[sl], sc[sl]).double().t()
    H.assert_close("fp8 lm_head logits (V = 151936) vs fp64 on q*scale", logits[1:], ref[1:].float(), max_rel=2 ** -7)
    assert torch.equal(ids[1:], torch.argmax(logits[1:], dim=-1))
    H.assert_ids_match_where_safe("fp8 lm_head ids", ids[1:], ref[1:].float(), margin_rel=3e-2)


# ------------------------------------------------------------------ 7. random data through gemm_resid
@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 12288)])
def test_gemm_resid_fp8_random(ops, N, K):
    """fp64 on the dequantised weights, then the bf16 rounding: identical rounding points and another fp32 order, so
    the outputs differ by 1-ulp flips only — max-abs <= one bf16 ulp of the output scale, under 5 % of elements."""
    gd = torch.Generator(device=dev()).manual_seed(N + K)
    w = (torch.randn(N, K, generator=gd, device=dev()) * 0.03).to(BF16)
    x = torch.randn(16, K, generator=gd, device=dev()).to(BF16)
    q, sc = ops.quantize_fp8_rows(w)
    h = torch.zeros(16, N, dtype=BF16, device=dev())
    ops.gemm_resid(ops.pack_weight_fp8(q, sc), to_frag(ops, x), N, K, h, add_residual=False)
    ref = (x.double() @ ops.dequantize_fp8_rows(q, sc).double().t()).float().to(BF16).float()
    scale = float(ref.abs().max())
    ulp = 2.0 ** (torch.tensor(scale).log2().floor().item() - 7)       # bf16: 8 significant bits
    d = (h.float() - ref).abs()
    H.assert_close(f"fp8 gemm_resid ({N}, {K}) vs fp64 on q*scale", h, ref, max_rel=2 ** -7)
    assert float(d.max()) <= ulp, (float(d.max()), ulp)
    assert (d > 0).float().mean() < 0.05


# ------------------------------------------------------------------ 8 - 11. model and loops
def make_model(cfg, weight_format="bf16", sd=None, seed=3):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev(), weight_format=weight_format)
    m.load_state_dict(sd if sd is not None else H.draft_weights(cfg, seed=seed, dtype=BF16))
    return m


def run_cycles(m, cfg, taus, seed, lm=None, bs=16):
    """`len(taus)` draft cycles through forward() on a fresh cache: hidden rows per cycle, the cache, draft ids."""
    g = gen(seed)
    cache = m.new_cache(sum(taus) + 64)
    start, outs, ids_all = taus[0], [], []
    for c, tau in enumerate(taus):
        th = (torch.randn(1, tau, cfg.fc_in, generator=g) * 1.5).to(BF16).to(dev())
        ne = (torch.randn(1, bs, cfg.hidden_size, generator=g) * 0.05).to(BF16).to(dev())
        pos = torch.arange(cache.get_seq_length(), start + bs, device=dev())[None]
        outs.append(m(target_hidden=th, noise_embedding=ne, position_ids=pos, past_key_values=cache, use_cache=True))
        if lm is not None and bs <= 16:
            ids = torch.zeros(16, dtype=torch.long, device=dev())
            wp = m.packed_lm_head_fp8(lm) if m.streams_fp8(bs) else m.packed_lm_head(lm)
            m.draft_tokens(m._src["final"], wp, bs, ids)
            ids_all.append(ids[1:bs].clone())
        cache.crop(start)
        if c + 1 < len(taus):
            start += taus[c + 1]
    return outs, cache, ids_all


def compare_runs(name, a, b, cfg, lm_deq=None):
    """Parity bar of DESIGN.md section 2 between two runs of run_cycles; returns whether everything was bit-identical."""
    (oa, ca, ia), (ob, cb, ib) = a, b
    same = True
    for c, (x, y) in enumerate(zip(oa, ob)):
        H.assert_close(f"{name} hidden cycle {c}", x, y)
        same &= torch.equal(x, y)
    n = ca.get_seq_length()
    assert n == cb.get_seq_length()
    for li in (0, cfg.num_hidden_layers - 1):
        H.assert_close(f"{name} K layer {li}", ca.k[li][:, :n], cb.k[li][:, :n], max_rel=H.KV_MAX_REL)
        H.assert_close(f"{name} V layer {li}", ca.v[li][:, :n], cb.v[li][:, :n], max_rel=H.KV_MAX_REL)
        same &= torch.equal(ca.k[li][:, :n], cb.k[li][:, :n]) and torch.equal(ca.v[li][:, :n], cb.v[li][:, :n])
    for c, (x, y) in enumerate(zip(ia, ib)):
        ref_logits = torch.nn.functional.linear(ob[c][0, 1:].float(), lm_deq.float())
        H.assert_ids_match_where_safe(f"{name} ids cycle {c} (stream)", x, ref_logits, margin_rel=3e-2, min_safe=0)
        H.assert_ids_match_where_safe(f"{name} ids cycle {c} (copy)", y, ref_logits, margin_rel=3e-2, min_safe=0)
        same &= torch.equal(x, y)
    print(f"[fp8] {name}: bit-identical = {same}")
    return same


def test_fp8_stream_equals_its_bf16_copy_tiny():
    """weight_format="fp8_e4m3", fp8_stream True against False on the same model, six cycles with tau in {1, 7, 16}:
    hidden rows, cached K/V of the first and last layer, draft ids — within the project's parity bar (3e-2 / 4e-3 of
    the scale, ids where safe).  Both paths multiply the same values; they differ only in the fp32 order where the W8
    form rounds a wave's share up to a pair of k-steps (K = 512: one k-step per wave in bf16, two per wave on eight
    waves in W8), so they are NOT bit-identical here.  Achieved on MI355X: hidden rows max 5.8e-3 / mean 3.5e-4 of the
    scale (three of six cycles bit-identical), cached K/V max 2.3e-4, ids equal on every margin-screened row."""
    from dflash_amd import ops
    cfg = H.tiny_cfg()
    m = make_model(cfg, "fp8_e4m3")
    assert m.w8 is not None and m.streams_fp8(16) and not m.streams_fp8(17)
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=gen(2)) * 0.05).to(BF16).to(dev())
    lm_deq = ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(lm))
    taus = [1, 7, 16, 1, 7, 16]
    a = run_cycles(m, cfg, taus, 5, lm)
    m.fp8_stream = False
    assert not m.streams_fp8(16)
    b = run_cycles(m, cfg, taus, 5, lm_deq)    # the copy's lm_head: the dequantised values, in bf16
    compare_runs("fp8 stream vs copy (tiny)", a, b, cfg, lm_deq)


def test_fp8_stream_equals_its_bf16_copy_8b_widths():
    """8B widths, one layer, S = 1024: the production nfr = 8 and chunked launch forms under the model code.  Every K
    here is a multiple of 1024, so both forms give every wave the same k-steps and the same fp32 order: measured
    bit-identical on MI355X (hidden rows and cached K/V), and asserted so."""
    from dflash_amd.config import DFlashConfig, QWEN3_8B_DRAFT
    cfg = DFlashConfig(**{**QWEN3_8B_DRAFT, "num_hidden_layers": 1})
    m = make_model(cfg, "fp8_e4m3", seed=11)
    g = gen(3)
    ctx = (torch.randn(1024, cfg.fc_in, generator=g) * 1.5).to(BF16).to(dev())
    th = (torch.randn(1, 16, cfg.fc_in, generator=g) * 1.5).to(BF16).to(dev())
    ne = (torch.randn(1, 16, cfg.hidden_size, generator=g) * 0.05).to(BF16).to(dev())
    runs = []
    for stream in (True, False):
        m.fp8_stream = stream
        cache = m.new_cache(1024 + 64)
        m.prefill_context(cache, ctx, 0)
        pos = torch.arange(1024, 1024 + 32, device=dev())[None]
        out = m(target_hidden=th, noise_embedding=ne, position_ids=pos, past_key_values=cache, use_cache=True)
        cache.crop(1024 + 16)
        runs.append(([out], cache, []))
    assert compare_runs("fp8 stream vs copy (8B widths, S = 1024)", runs[0], runs[1], cfg)


def _dequantised_state_dict(cfg, sd):
    from dflash_amd import ops
    out = {}
    for k, v in sd.items():
        if v.dim() == 2 and k in cfg.state_dict_shapes():
            out[k] = ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(v.to(dev()).to(BF16))).cpu()
        else:
            out[k] = v
    return out


def test_fp8_model_copy_equals_a_bf16_model_of_the_dequantised_weights():
    """self.w of an fp8 model holds q * scale: with fp8_stream off it computes, bit for bit, what a bf16 model loaded
    with q * scale as its state dict computes — one quantised model on every path."""
    cfg = H.tiny_cfg()
    sd = H.draft_weights(cfg, seed=3, dtype=BF16)
    m8 = make_model(cfg, "fp8_e4m3", sd=sd)
    m8.fp8_stream = False
    mb = make_model(cfg, "bf16", sd=_dequantised_state_dict(cfg, sd))
    assert mb.w8 is None
    taus = [7, 16, 1]
    (oa, ca, _), (ob, cb, _) = run_cycles(m8, cfg, taus, 8), run_cycles(mb, cfg, taus, 8)
    for x, y in zip(oa, ob):
        assert torch.equal(x, y)
    n = ca.get_seq_length()
    assert torch.equal(ca.k[:, :, :n], cb.k[:, :, :n]) and torch.equal(ca.v[:, :, :n], cb.v[:, :, :n])
    # and a 20-row block (the wide path reads self.w on either model)
    (oa, _, _), (ob, _, _) = run_cycles(m8, cfg, [9, 4], 9, bs=20), run_cycles(mb, cfg, [9, 4], 9, bs=20)
    for x, y in zip(oa, ob):
        assert torch.equal(x, y)


def _tiny_hf(dtype=BF16, layers=6):
    from dflash_amd.synthetic import make_hf_qwen3
    torch.manual_seed(11)
    return make_hf_qwen3({**H.TINY_TARGET, "num_layers": layers}, dev(), dtype=dtype)


def _walk_case(n_new):
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    hf = _tiny_hf()
    perm = impose_greedy_walk(hf, seed=5)
    prompt = torch.randint(0, 2000, (1, 33), generator=gen(4)).to(dev())
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = H.make_plan(64, 16, 17)

    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 2000

    return hf, prompt, G, hook


def test_fp8_draft_is_lossless_and_replays(monkeypatch):
    """spec_generate and dflash_generate with the fp8 draft on the tiny native target, scripted acceptance: the
    committed ids are the target's greedy walk, as the bf16 draft's are; DFL_GRAPH=1 equals DFL_GRAPH=0 id for id with
    replayed cycles (the captured graphs hold the fp8 launches); and WITHOUT the hook (random weights: nearly every
    draft token is rejected) the ids are still the walk."""
    from dflash_amd import NativeTarget, dflash_generate
    cfg = H.tiny_cfg()
    n_new = 120
    hf, prompt, G, hook = _walk_case(n_new)
    want = G[:33 + n_new].tolist()
    runs = {}
    for fmt in ("bf16", "fp8_e4m3"):
        for mode in ("0", "1") if fmt != "bf16" else ("0",):
            monkeypatch.setenv("DFL_GRAPH", mode)
            m = make_model(cfg, fmt)
            r = dflash_generate(m, NativeTarget(hf), prompt, cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=hook)
            assert r.output_ids[0].tolist() == want, (fmt, mode)
            runs[fmt, mode] = r
    assert runs["fp8_e4m3", "1"].replayed_cycles > 0 and runs["fp8_e4m3", "0"].replayed_cycles == 0
    assert (runs["fp8_e4m3", "0"].acceptance_lengths == runs["fp8_e4m3", "1"].acceptance_lengths
            == runs["bf16", "0"].acceptance_lengths)
    monkeypatch.setenv("DFL_GRAPH", "0")
    m8 = make_model(cfg, "fp8_e4m3")
    ids = m8.spec_generate(target=NativeTarget(hf), input_ids=prompt, max_new_tokens=n_new, stop_token_ids=None,
                           temperature=0.0, draft_token_hook=hook)
    assert ids[0, :33 + n_new].tolist() == want
    # no hook: rejection on nearly every cycle
    for mode in ("0", "1"):
        monkeypatch.setenv("DFL_GRAPH", mode)
        r = dflash_generate(make_model(cfg, "fp8_e4m3"), NativeTarget(hf), prompt, cfg.mask_token_id, 48, 16, None, 0.0)
        assert r.output_ids[0].tolist() == G[:33 + 48].tolist(), mode
    ids = m8.spec_generate(target=NativeTarget(hf), input_ids=prompt, max_new_tokens=48, stop_token_ids=None,
                           temperature=0.0)
    assert ids[0, :33 + 48].tolist() == G[:33 + 48].tolist()


def test_fp8_fallback_paths_match_their_twin():
    """Paths without an fp8 kernel run on the dequantised copy whatever fp8_stream says: a 20-row block, a sampled draft
    (sampler="device", T = 0.7: the bf16 lm_head draws) and the ragged batch with two requests."""
    from dflash_amd import NativeTarget, dflash_generate
    from dflash_amd.batch import dflash_generate_batch
    cfg = H.tiny_cfg()
    m = make_model(cfg, "fp8_e4m3")
    # a 20-row block
    a = run_cycles(m, cfg, [9, 4, 16], 12, bs=20)
    m.fp8_stream = False
    b = run_cycles(m, cfg, [9, 4, 16], 12, bs=20)
    compare_runs("fp8 model, 20-row block", a, b, cfg)
    # a sampled draft: the committed tokens are the target's seeded draws, whatever the draft proposes
    hf, prompt, G, hook = _walk_case(64)
    outs = []
    for stream in (True, False):
        m.fp8_stream = stream
        r = dflash_generate(m, NativeTarget(hf), prompt, cfg.mask_token_id, 48, 16, None, 0.7, sampler="device", seed=5)
        outs.append(r.output_ids[0].tolist())
    assert outs[0] == outs[1]
    # the ragged batch, two requests
    prompts = [prompt, torch.randint(0, 2000, (1, 21), generator=gen(6)).to(dev())]
    outs = []
    for stream in (True, False):
        m.fp8_stream = stream
        rs = dflash_generate_batch(m, NativeTarget(hf), prompts, cfg.mask_token_id, 40, 16, None, 0.0)
        outs.append([r.output_ids[0].tolist() for r in rs])
    assert outs[0] == outs[1] and outs[0][0] == G[:33 + 40].tolist()
    from dflash_amd import DFlashDraftModel
    with pytest.raises(ValueError):
        DFlashDraftModel(cfg, device=dev(), weight_format="int4")
