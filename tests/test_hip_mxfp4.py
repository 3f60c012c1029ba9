"""MXFP4 weight streaming on the GPU: the W4 skinny GEMM kernels (k_gemm_w4) against torch on exact
operands, against fp64 on the dequantised weights and, bit for bit, against the bf16 launch on the dequantised matrix
where both forms give every wave the same k-steps; the mxfp4 draft model against its own bf16 copy and against a bf16
model loaded with the dequantised weights; the decode loops' losslessness with an mxfp4 draft.

Which K are bit-identical to the bf16 launch: the bf16 form gives a wave ceil(K / 512) k-steps, the W4 form that number
rounded up to a multiple of 4, and the K-chunked form (K > 4096) 4 per chunk in both.  The shares — and with them the
fp32 order of every sum — are the same exactly when ceil(K / 512) is 4 or 8, i.e. K in {1664 .. 2048} or {3712 .. 4096}
(multiples of 128), and at every K > 4096.  All 8B widths (4096, 12288, 20480) are among them."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16, U8 = torch.bfloat16, torch.uint8


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


def first_argmax(lg):
    m = lg.max(dim=-1, keepdim=True).values
    idx = torch.arange(lg.shape[-1], device=lg.device).expand_as(lg)
    return torch.where(lg == m, idx, lg.shape[-1]).min(dim=-1).values


def same_k_steps(K):
    """Whether the bf16 and the W4 launch give every wave the same k-steps at this K (the module docstring)."""
    return K % 128 == 0 and (K > 4096 or -(-K // 512) in (4, 8))


def grid_codes(N, K, g, scale_of_block=lambda b: 126 + b % 3):
    """Random e2m1 codes with the block scales 2^-1, 2^0, 2^1 for blocks b % 3 of every row (they vary WITHIN a row):
    (codes [N, K/2], scale codes [N, K/32], the dequantised values as fp64 [N, K]).  Multiples of 1/4 up to 12."""
    from dflash_amd import ops
    codes = torch.randint(0, 256, (N, K // 2), generator=g).to(U8)
    sc = torch.tensor([scale_of_block(b) for b in range(K // 32)], dtype=U8).repeat(N, 1)
    return codes, sc, ops.dequantize_mxfp4_rows(codes, sc).double()


def grid_weight(ops, N, K, g):
    codes, sc, wd = grid_codes(N, K, g)
    return ops.pack_weight_mxfp4(codes.to(dev()), sc.to(dev())), wd


# ------------------------------------------------------------------ every code
def test_every_e2m1_code_converts_exactly_under_every_scale(ops):
    """A [16, 128] weight in which every block of 32 holds all 16 e2m1 codes (code = (5 k + n) % 16) and the four blocks
    of a row carry four different scale codes out of {7, 126, 127, 128, 140, 247}; one-hot activation rows select 16 k's
    per launch.  The logits of dfl_gemm_argmax are the weights in bf16, bit for bit (a zero is compared as a zero: the
    K-sum of +0 products and one -0 is +0) and the ids torch's first argmax: the nibble order inside a byte, the order
    of the conversion's byte select and the order of the scale bytes inside a dword."""
    SC = [7, 126, 127, 128, 140, 247]
    n, k = torch.arange(16)[:, None], torch.arange(128)[None, :]
    code = ((5 * k + n) % 16).to(U8)
    sc = torch.tensor([[SC[(4 * r + b) % 6] for b in range(4)] for r in range(16)], dtype=U8)
    pairs = {(int(code[r, c]), int(sc[r, c // 32])) for r in range(16) for c in range(128)}
    assert len(pairs) == 16 * 6
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    val = ops.dequantize_mxfp4_rows(codes, sc)
    lut = torch.tensor(list(ops.E2M1_VALUES) + [-v for v in ops.E2M1_VALUES], dtype=torch.float64)
    assert torch.equal(val.double(), lut[code.long()] * torch.exp2(sc.double() - 127).repeat_interleave(32, dim=1))
    w4 = ops.pack_weight_mxfp4(codes.to(dev()), sc.to(dev()))
    ws = ops.argmax_ws(dev())
    for j in range(8):
        x = torch.zeros(16, 128, dtype=BF16)
        x[torch.arange(16), 16 * j + torch.arange(16)] = 1.0
        logits = torch.full((16, 16), float("nan"), dtype=BF16, device=dev())
        ids = torch.zeros(16, dtype=torch.long, device=dev())
        ops.gemm_argmax(w4, ops.rows_plain(x.to(dev())), 16, 128, 0, 16, ws, ids, 0, logits=logits)
        want = val[:, 16 * j:16 * j + 16].t().contiguous()             # logits[m][n] = W[n][16 j + m]
        got = logits.cpu()
        nz = want != 0
        assert torch.equal(got.view(torch.int16)[nz], want.view(torch.int16)[nz]), j
        assert torch.all(got[~nz] == 0), j
        assert torch.equal(ids.cpu(), first_argmax(want.float())), j


# ------------------------------------------------------------------ exact sums through gemm_resid
RESID_SHAPES = [(16, 128, 16), (48, 384, 5), (256, 512, 16), (4480, 4096, 16), (256, 12288, 7)]


@pytest.mark.parametrize("add_residual", [False, True])
@pytest.mark.parametrize("N,K,rows", RESID_SHAPES)
def test_gemm_resid_mxfp4_exact(ops, N, K, rows, add_residual):
    """Weights on the e2m1 grid times 2^-1 / 2^0 / 2^1 by block (multiples of 1/4 up to 12), activations in [-4, 4]:
    every sum is exact in fp32 (a multiple of 1/4 below 2^22 at K = 12288), so h, tap and the sums of squares equal
    torch's — one word per lane with fifteen waves without a share (K = 128), nfr rounded up and half tiles (48 x 384),
    whole plus half tiles (4480), the chunked form (12288).  Rows >= `rows` of the frag source are NaN: a frag source
    is not masked, but no valid row may see them."""
    g = gen(N + K + rows)
    w4, wd = grid_weight(ops, N, K, g)
    x = torch.randint(-4, 5, (16, K), generator=g).float()
    xp = x.clone()
    xp[rows:] = float("nan")
    h0 = torch.randint(-64, 65, (16, N + 16), generator=g).to(BF16)
    h = h0.to(dev())
    tap = torch.zeros(16, 3 * N, dtype=BF16, device=dev())
    ss = torch.zeros(N, device=dev()) if add_residual else None    # (sums of squares keep whole tiles: no halves)
    ops.gemm_resid(w4, to_frag(ops, xp.to(BF16).to(dev())), N, K, h[:, :N], add_residual=add_residual, ss_out=ss,
                   tap=tap[:, N:2 * N])
    lin = (x.double() @ wd.t()).float().to(BF16)                   # exact sum, one rounding
    ref = (h0[:, :N].float() + lin.float()).to(BF16) if add_residual else lin
    assert torch.equal(h[:rows, :N].cpu(), ref[:rows])
    assert torch.equal(h[:, N:].cpu(), h0[:, N:])                   # nothing beyond column N
    assert torch.equal(tap[:rows, N:2 * N].cpu(), ref[:rows])
    assert torch.count_nonzero(tap[:, :N]) == 0 and torch.count_nonzero(tap[:, 2 * N:]) == 0
    if ss is not None:
        want = ref[:rows].double().pow(2).view(rows, N // 16, 16).sum(-1).t()      # [tile][row]
        got = ss.view(N // 16, 16)[:, :rows].cpu().double()
        assert torch.allclose(got, want, rtol=2e-6, atol=0)       # 16 fp32 terms in the DPP order


def test_gemm_resid_mxfp4_row_count_from_dyn_word(ops):
    """Plain rows with the valid count in a dyn word, 4096 -> 512: rows >= dyn[TAU] hold NaN and count as zero."""
    N, K, rows = 512, 4096, 7
    g = gen(77)
    w4, wd = grid_weight(ops, N, K, g)
    x = torch.randint(-4, 5, (16, K), generator=g).float()
    xp = x.clone()
    xp[rows:] = float("nan")
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, 0, rows, 16, 0)
    h = torch.full((16, N), 7.0, dtype=BF16, device=dev())
    ss = torch.zeros(N, device=dev())
    ops.gemm_resid(w4, ops.rows_plain(xp.to(BF16).to(dev()), ops.DYN_TAU), N, K, h, add_residual=False, ss_out=ss, dyn=dyn)
    ref = (x.double() @ wd.t()).float().to(BF16)
    assert torch.equal(h[:rows].cpu(), ref[:rows]) and torch.count_nonzero(h[rows:]) == 0
    want = ref[:rows].double().pow(2).view(rows, N // 16, 16).sum(-1).t()
    assert torch.allclose(ss.view(N // 16, 16)[:, :rows].cpu().double(), want, rtol=2e-6, atol=0)
    assert torch.count_nonzero(ss.view(N // 16, 16)[:, rows:]) == 0


def test_gemm_resid_mxfp4_normalised_source(ops):
    """4096 -> 512 from the residual stream + sums of squares (the RMSNorm in the GEMM's prologue) against the oracle's
    rms_norm and fp64 on the dequantised weights; the bar of test_gemm_row_sources_and_resid_epilogue for this source
    (1-ulp flips of the normalised inputs: 2e-2 / 1e-3 of the scale)."""
    from oracle.dflash_oracle import rms_norm
    N, K, bs = 512, 4096, 11
    g = gen(78)
    w = (torch.randn(N, K, generator=g) * 0.03).to(BF16)
    q = ops.quantize_mxfp4_rows(w.to(dev()))
    wd = ops.dequantize_mxfp4_rows(*q).cpu().double()
    hrows = (torch.randn(16, K, generator=g) * 0.7).to(BF16)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(BF16)
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, 0, 7, bs, 0)
    ss0 = hrows.float().pow(2).sum(-1).to(dev())
    out = torch.zeros(16, N, dtype=BF16, device=dev())
    ops.gemm_resid(ops.pack_weight_mxfp4(*q), ops.rows_normed(hrows.to(dev()), ss0, 1, nw.to(dev()), 1e-6, ops.DYN_BS),
                   N, K, out, add_residual=False, dyn=dyn)
    ref = (rms_norm(hrows, nw, 1e-6).double() @ wd.t()).float()
    d = (out[:bs].cpu().float() - ref[:bs]).abs()
    print(f"[mxfp4] normalised source: max {float(d.max() / ref.abs().max()):.3e} mean {float(d.mean() / ref.abs().max()):.3e}")
    assert d.max() <= 2e-2 * ref.abs().max() and d.mean() <= 1e-3 * ref.abs().max()
    assert torch.count_nonzero(out[bs:]) == 0


# ------------------------------------------------------------------ SiLU
def test_gemm_silu_mul_mxfp4_exact(ops):
    """Grid operands at (I 64, K 512) with DISTINCT block scales in the gate tile (2^-3, 2^-2, 2^-1 by block) and the up
    tile (2^1, 2^0 by block) of every pair, activations in {-1, 0, 1} on columns of four different blocks: a gate / up
    mix-up in the packed scale order, or a scale byte taken from another k-step, would show.  The gate and up sums are
    exact; bar of test_gemm_silu_mul_exact_ints (__expf vs exp)."""
    I, K = 64, 512
    g = gen(7)
    gc, gs, wg = grid_codes(I, K, g, lambda b: 124 + b % 3)
    uc, us, wu = grid_codes(I, K, g, lambda b: 128 - b % 2)
    assert not torch.equal(gs, us)
    cols = torch.tensor([0, 1, 40, 41, 80, 81, 120, 500])
    x = torch.zeros(16, K, dtype=BF16)
    x[:, cols] = torch.randint(-1, 2, (16, 8), generator=g).to(BF16)
    act = torch.empty(16 * I, dtype=BF16, device=dev())
    w4 = ops.pack_weight_gateup_mxfp4(gc.to(dev()), gs.to(dev()), uc.to(dev()), us.to(dev()))
    ops.gemm_silu_mul(w4, to_frag(ops, x.to(dev())), I, K, act)
    gl = (x.double() @ wg.t()).float().to(BF16).float()
    ul = (x.double() @ wu.t()).float().to(BF16).float()
    ref = (torch.nn.functional.silu(gl).to(BF16).float() * ul).to(BF16).float()
    got = unfrag(act, I).float().cpu()
    assert float(ref.abs().max()) > 1
    assert (got - ref).abs().max() <= 2 ** -7 * max(1.0, float(ref.abs().max()))


def test_gemm_silu_mul_mxfp4_random(ops):
    """Random bf16 at (I 2560, K 1024) against fp64 on the dequantised weights with the same rounding points; bar of
    test_gemm_silu_mul: 2^-6 of the scale, under 5 % of elements differing."""
    I, K = 2560, 1024
    g = gen(6)
    wg = (torch.randn(I, K, generator=g) * 0.05).to(BF16).to(dev())
    wu = (torch.randn(I, K, generator=g) * 0.11).to(BF16).to(dev())     # another amax: other scales than the gate rows'
    x = torch.randn(16, K, generator=g).to(BF16).to(dev())
    qg, qu = ops.quantize_mxfp4_rows(wg), ops.quantize_mxfp4_rows(wu)
    assert not torch.equal(qg[1], qu[1])
    act = torch.empty(16 * I, dtype=BF16, device=dev())
    ops.gemm_silu_mul(ops.pack_weight_gateup_mxfp4(*qg, *qu), to_frag(ops, x), I, K, act)
    got = unfrag(act, I).float()
    gl = (x.double() @ ops.dequantize_mxfp4_rows(*qg).double().t()).float().to(BF16)
    ul = (x.double() @ ops.dequantize_mxfp4_rows(*qu).double().t()).float().to(BF16)
    ref = (torch.nn.functional.silu(gl.float()).to(BF16).float() * ul.float()).to(BF16).float()
    H.assert_close("mxfp4 silu_mul (2560, 1024) vs fp64 on dq", got, ref, max_rel=2 ** -6)
    assert ((got - ref).abs() > 0).float().mean() < 0.05


# ------------------------------------------------------------------ argmax
@pytest.mark.parametrize("V,K,bs,row0", [(2048, 512, 16, 0), (4096 + 16 * 7, 1024, 12, 1)])
def test_gemm_argmax_mxfp4_exact(ops, V, K, bs, row0):
    """Grid operands: ids (first index on ties), logits and top-2 margins are exact."""
    g = gen(V)
    w4, wd = grid_weight(ops, V, K, g)
    x = torch.randint(-4, 5, (16, K), generator=g).float()
    ids = torch.full((16,), -1, dtype=torch.long, device=dev())
    margins = torch.full((16,), -1.0, device=dev())
    logits = torch.zeros(16, V, dtype=BF16, device=dev())
    xf = to_frag(ops, x.to(BF16).to(dev()))
    ops.gemm_argmax(w4, xf, V, K, row0, bs - row0, ops.argmax_ws(dev()), ids, row0, logits=logits, margins=margins)
    ref = (x.double() @ wd.t()).float().to(BF16)
    assert torch.equal(logits[row0:bs].cpu(), ref[row0:bs])
    assert torch.equal(ids[row0:bs].cpu(), first_argmax(ref[row0:bs].float()))
    top2 = ref[row0:bs].float().topk(2, dim=-1).values
    assert torch.equal(margins[row0:bs].cpu(), top2[:, 0] - top2[:, 1])
    assert (ids[:row0] == -1).all() and (ids[bs:] == -1).all()
    ids2 = torch.full((16,), -1, dtype=torch.long, device=dev())     # the fused path (no logits written): the same ids
    ops.gemm_argmax(w4, xf, V, K, row0, bs - row0, ops.argmax_ws(dev()), ids2, row0)
    assert torch.equal(ids, ids2)


def test_gemm_argmax_mxfp4_tie_across_workgroups_after_the_block_scales(ops):
    """Two columns in different workgroups that tie only AFTER their block scales (code 1.0 under 2^1 in column 5, code
    4.0 under 2^-1 in column 1000, every other weight -1): the first index wins with margin 0; by the codes alone,
    column 1000 would."""
    V, K = 2048, 512
    code = torch.full((V, K), 10, dtype=U8)          # -1.0
    sc = torch.full((V, K // 32), 127, dtype=U8)
    code[5], sc[5] = 2, 128
    code[1000], sc[1000] = 6, 126
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    x = torch.zeros(16, K)
    x[:, 0] = torch.arange(1, 17).float()
    w4 = ops.pack_weight_mxfp4(codes.to(dev()), sc.to(dev()))
    ids = torch.full((16,), -1, dtype=torch.long, device=dev())
    margins = torch.full((16,), -1.0, device=dev())
    ops.gemm_argmax(w4, to_frag(ops, x.to(BF16).to(dev())), V, K, 0, 16, ops.argmax_ws(dev()), ids, 0, margins=margins)
    assert ids.tolist() == [5] * 16 and torch.count_nonzero(margins) == 0


def test_gemm_argmax_mxfp4_full_vocabulary(ops):
    """(V 151936, K 4096), random data: ids against fp64 logits of the dequantised weights, where the margin is safe."""
    V, K = 151936, 4096
    gd = torch.Generator(device=dev()).manual_seed(9)
    w = (torch.randn(V, K, generator=gd, device=dev()) * 0.02).to(BF16)
    x = torch.randn(16, K, generator=gd, device=dev()).to(BF16)
    codes, sc = ops.quantize_mxfp4_rows(w)
    del w
    ids = torch.full((16,), -1, dtype=torch.long, device=dev())
    logits = torch.zeros(16, V, dtype=BF16, device=dev())
    ops.gemm_argmax(ops.pack_weight_mxfp4(codes, sc), to_frag(ops, x), V, K, 1, 15, ops.argmax_ws(dev()), ids, 1, logits=logits)
    ref = torch.empty(16, V, dtype=torch.float64, device=dev())
    for n0 in range(0, V, 16384):    # fp64 in slabs: the dequantised slab alone is 0.5 GB
        sl = slice(n0, min(V, n0 + 16384))
        ref[:, sl] = x.double() @ ops.dequantize_mxfp4_rows(codes[sl], sc[sl]).double().t()
    H.assert_close("mxfp4 lm_head logits (V = 151936) vs fp64 on dq", logits[1:], ref[1:].float(), max_rel=2 ** -7)
    assert torch.equal(ids[1:], torch.argmax(logits[1:], dim=-1))
    H.assert_ids_match_where_safe("mxfp4 lm_head ids", ids[1:], ref[1:].float(), margin_rel=3e-2)


# ------------------------------------------------------------------ random data through gemm_resid, and bit identity
def _random_case(ops, N, K, seed):
    gd = torch.Generator(device=dev()).manual_seed(seed)
    w = (torch.randn(N, K, generator=gd, device=dev()) * 0.03).to(BF16)
    x = torch.randn(16, K, generator=gd, device=dev()).to(BF16)
    q = ops.quantize_mxfp4_rows(w)
    return q, ops.dequantize_mxfp4_rows(*q), x


@pytest.mark.parametrize("N,K", [(4096, 4096), (4096, 12288)])
def test_gemm_resid_mxfp4_random(ops, N, K):
    """fp64 on the dequantised weights, then the bf16 rounding: identical rounding points and another fp32 order, so
    the outputs differ by 1-ulp flips only — max-abs <= one bf16 ulp of the output scale, under 5 % of elements."""
    q, dq, x = _random_case(ops, N, K, N + K)
    h = torch.zeros(16, N, dtype=BF16, device=dev())
    ops.gemm_resid(ops.pack_weight_mxfp4(*q), to_frag(ops, x), N, K, h, add_residual=False)
    ref = (x.double() @ dq.double().t()).float().to(BF16).float()
    scale = float(ref.abs().max())
    ulp = 2.0 ** (torch.tensor(scale).log2().floor().item() - 7)       # bf16: 8 significant bits
    d = (h.float() - ref).abs()
    H.assert_close(f"mxfp4 gemm_resid ({N}, {K}) vs fp64 on dq", h, ref, max_rel=2 ** -7)
    assert float(d.max()) <= ulp, (float(d.max()), ulp)
    assert (d > 0).float().mean() < 0.05


def test_same_k_steps_rule():
    """(no launch) the K at which the two forms share out the k-steps alike: every 8B width, not the tiny ones."""
    assert all(same_k_steps(K) for K in (2048, 4096, 3712, 1664, 4224, 12288, 20480))
    assert not any(same_k_steps(K) for K in (128, 384, 512, 1024, 1536, 2176, 3584))
    for K in range(128, 4097, 128):
        bf, w4 = -(-(K // 32) // 16), (-(-(K // 32) // 16) + 3) & ~3
        assert same_k_steps(K) == (bf == w4), K


@pytest.mark.parametrize("N,K", [(6144, 4096), (4096, 12288), (4096, 20480), (512, 2048), (512, 1024)])
def test_gemm_resid_mxfp4_against_the_bf16_launch(ops, N, K):
    """The W4 launch against the bf16 launch on the dequantised matrix (the same bf16 fragments into the same MFMAs):
    bit-identical h and sums of squares wherever same_k_steps(K) — the 8B widths of qkv / o (4096), down (12288) and fc
    (20480) among them; at K = 1024 the waves' shares differ (2 k-steps on 16 waves against 4 on 8) and the parity bar of
    DESIGN.md section 2 holds."""
    q, dq, x = _random_case(ops, N, K, N + K + 1)
    xf = to_frag(ops, x)
    h0 = (torch.randn(16, N, generator=gen(N)) * 0.5).to(BF16).to(dev())
    outs = []
    for wt in (ops.pack_weight_mxfp4(*q), ops.pack_weight(dq)):
        h, ss = h0.clone(), torch.zeros(N, device=dev())
        ops.gemm_resid(wt, xf, N, K, h, add_residual=True, ss_out=ss)
        outs.append((h, ss))
    (h4, s4), (hb, sb) = outs
    mx, _ = H.assert_close(f"mxfp4 vs bf16 launch on dq ({N}, {K})", h4, hb)
    if same_k_steps(K):
        assert torch.equal(h4, hb) and torch.equal(s4, sb)
    else:
        print(f"[mxfp4] ({N}, {K}): other k-steps per wave, max error {mx:.3e} of the scale")


def test_gemm_silu_and_argmax_mxfp4_against_the_bf16_launch_8b_width(ops):
    """K = 4096 (8 k-steps per wave in both forms): gate/up + SiLU at I = 1024 and the lm_head logits, ids and margins at
    V = 8192 + 112 equal the bf16 launch's on the dequantised matrices, bit for bit."""
    K, I, V = 4096, 1024, 8192 + 112
    qg, dg, x = _random_case(ops, I, K, 31)
    qu, du, _ = _random_case(ops, I, K, 32)
    xf = to_frag(ops, x)
    acts = []
    for wt in (ops.pack_weight_gateup_mxfp4(*qg, *qu), ops.pack_weight_gateup(dg, du)):
        act = torch.empty(16 * I, dtype=BF16, device=dev())
        ops.gemm_silu_mul(wt, xf, I, K, act)
        acts.append(act)
    assert torch.equal(acts[0].view(torch.int16), acts[1].view(torch.int16))
    q, dq, _ = _random_case(ops, V, K, 33)
    res = []
    for wt in (ops.pack_weight_mxfp4(*q), ops.pack_weight(dq)):
        ids = torch.full((16,), -1, dtype=torch.long, device=dev())
        mg = torch.full((16,), -1.0, device=dev())
        lg = torch.zeros(16, V, dtype=BF16, device=dev())
        ops.gemm_argmax(wt, xf, V, K, 1, 15, ops.argmax_ws(dev()), ids, 1, logits=lg, margins=mg)
        res.append((ids, mg, lg))
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ model and loops
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
            wp = m.packed_lm_head_mxfp4(lm) if m.streams_mxfp4(bs) else m.packed_lm_head(lm)
            m.draft_tokens(m._src["final"], wp, bs, ids)
            ids_all.append(ids[1:bs].clone())
        cache.crop(start)
        if c + 1 < len(taus):
            start += taus[c + 1]
    return outs, cache, ids_all


def compare_runs(name, a, b, cfg, lm_deq=None):
    """Parity bar of DESIGN.md section 2 between two runs of run_cycles; returns (everything bit-identical, worst max
    error of the hidden rows)."""
    (oa, ca, ia), (ob, cb, ib) = a, b
    same, worst = True, 0.0
    for c, (x, y) in enumerate(zip(oa, ob)):
        worst = max(worst, H.assert_close(f"{name} hidden cycle {c}", x, y)[0])
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
    print(f"[mxfp4] {name}: bit-identical = {same}, worst hidden max error {worst:.3e}")
    return same, worst


def test_mxfp4_stream_equals_its_bf16_copy_tiny():
    """weight_format="mxfp4", mxfp4_stream True against False on the same model, six cycles with tau in {1, 7, 16}: hidden
    rows, cached K/V of the first and last layer, draft ids — within the project's parity bar (3e-2 / 4e-3 of the scale,
    ids where safe).  Both paths multiply the same values; at the tiny widths (K = 512, 1024, 2560) the W4 form rounds a
    wave's share up to four k-steps, so the fp32 order differs and bit identity is not guaranteed (achieved on MI355X:
    no bf16 rounding moved — hidden rows, cached K/V and ids identical in all six cycles, max error 0)."""
    from dflash_amd import ops
    cfg = H.tiny_cfg()
    m = make_model(cfg, "mxfp4")
    assert m.w4 is not None and m.w8 is None and m.streams_mxfp4(16) and not m.streams_mxfp4(17)
    assert all(isinstance(m.w4["layers"][0][k], ops.Mxfp4Weight) for k in ("qkv", "o", "gu", "down"))
    assert isinstance(m.w4["fc"], ops.Mxfp4Weight) and isinstance(m.w4["kv_all"], ops.Mxfp4Weight)
    assert m.row_layers(16)[0]["gu"] is m.w4["layers"][0]["gu"] and m.row_layers(17)[0]["gu"] is m.w["layers"][0]["gu"]
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=gen(2)) * 0.05).to(BF16).to(dev())
    lm_deq = ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(lm))
    taus = [1, 7, 16, 1, 7, 16]
    a = run_cycles(m, cfg, taus, 5, lm)
    m.mxfp4_stream = False
    assert not m.streams_mxfp4(16) and m.row_layers(16)[0]["gu"] is m.w["layers"][0]["gu"]
    b = run_cycles(m, cfg, taus, 5, lm_deq)    # the copy's lm_head: the dequantised values, in bf16
    compare_runs("mxfp4 stream vs copy (tiny)", a, b, cfg, lm_deq)


def test_mxfp4_stream_equals_its_bf16_copy_8b_widths():
    """8B widths, one layer, S = 1024: the production nfr = 8 and chunked launch forms under the model code.  Every K
    here (4096, 12288, 20480) gives every wave the same k-steps in both forms (same_k_steps), hence the same fp32 order:
    bit-identical hidden rows and cached K/V, asserted."""
    from dflash_amd.config import DFlashConfig, QWEN3_8B_DRAFT
    cfg = DFlashConfig(**{**QWEN3_8B_DRAFT, "num_hidden_layers": 1})
    assert all(same_k_steps(k) for k in (cfg.hidden_size, cfg.intermediate_size, cfg.fc_in, cfg.q_dim))
    m = make_model(cfg, "mxfp4", seed=11)
    g = gen(3)
    ctx = (torch.randn(1024, cfg.fc_in, generator=g) * 1.5).to(BF16).to(dev())
    th = (torch.randn(1, 16, cfg.fc_in, generator=g) * 1.5).to(BF16).to(dev())
    ne = (torch.randn(1, 16, cfg.hidden_size, generator=g) * 0.05).to(BF16).to(dev())
    runs = []
    for stream in (True, False):
        m.mxfp4_stream = stream
        cache = m.new_cache(1024 + 64)
        m.prefill_context(cache, ctx, 0)
        pos = torch.arange(1024, 1024 + 32, device=dev())[None]
        out = m(target_hidden=th, noise_embedding=ne, position_ids=pos, past_key_values=cache, use_cache=True)
        cache.crop(1024 + 16)
        runs.append(([out], cache, []))
    assert compare_runs("mxfp4 stream vs copy (8B widths, S = 1024)", runs[0], runs[1], cfg)[0]


def _dequantised_state_dict(cfg, sd):
    from dflash_amd import ops
    out = {}
    for k, v in sd.items():
        if v.dim() == 2 and k in cfg.state_dict_shapes():
            out[k] = ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(v.to(dev()).to(BF16))).cpu()
        else:
            out[k] = v
    return out


def test_mxfp4_model_copy_equals_a_bf16_model_of_the_dequantised_weights():
    """self.w of an mxfp4 model holds the dequantised values: with mxfp4_stream off it computes, bit for bit, what a bf16
    model loaded with them as its state dict computes (stream_format="bf16": the same plain launches) — one quantised
    model on every path."""
    from dflash_amd import DFlashDraftModel
    cfg = H.tiny_cfg()
    sd = H.draft_weights(cfg, seed=3, dtype=BF16)
    m4 = make_model(cfg, "mxfp4", sd=sd)
    m4.mxfp4_stream = False
    mb = DFlashDraftModel(cfg, device=dev(), stream_format="bf16").load_state_dict(_dequantised_state_dict(cfg, sd))
    assert mb.w4 is None and mb.w8 is None
    taus = [7, 16, 1]
    (oa, ca, _), (ob, cb, _) = run_cycles(m4, cfg, taus, 8), run_cycles(mb, cfg, taus, 8)
    for x, y in zip(oa, ob):
        assert torch.equal(x, y)
    n = ca.get_seq_length()
    assert torch.equal(ca.k[:, :, :n], cb.k[:, :, :n]) and torch.equal(ca.v[:, :, :n], cb.v[:, :, :n])


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


def test_mxfp4_draft_is_lossless_and_replays(monkeypatch):
    """dflash_generate and spec_generate with the mxfp4 draft on the tiny native target: under scripted acceptance the
    committed ids are the target's greedy walk with the bf16 draft's acceptance lengths, eager (DFL_GRAPH=0) and with
    replayed cycles (DFL_GRAPH=1: the captured graphs hold the W4 launches, lossless_fraction 1.0); WITHOUT the hook
    (random weights: nearly every draft token is rejected) the ids are still the walk."""
    from dflash_amd import NativeTarget, dflash_generate
    cfg = H.tiny_cfg()
    n_new = 96
    hf, prompt, G, hook = _walk_case(n_new)
    want = G[:33 + n_new].tolist()
    runs = {}
    for fmt in ("bf16", "mxfp4"):
        for mode in ("0", "1") if fmt != "bf16" else ("0",):
            monkeypatch.setenv("DFL_GRAPH", mode)
            m = make_model(cfg, fmt)
            r = dflash_generate(m, NativeTarget(hf), prompt, cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=hook)
            assert r.output_ids[0].tolist() == want, (fmt, mode)
            runs[fmt, mode] = r
    assert runs["mxfp4", "1"].replayed_cycles > 0 and runs["mxfp4", "0"].replayed_cycles == 0
    assert (runs["mxfp4", "0"].acceptance_lengths == runs["mxfp4", "1"].acceptance_lengths
            == runs["bf16", "0"].acceptance_lengths)
    match = sum(a == b for a, b in zip(runs["mxfp4", "1"].output_ids[0].tolist(), want)) / len(want)
    assert match == 1.0
    monkeypatch.setenv("DFL_GRAPH", "0")
    m4 = make_model(cfg, "mxfp4")
    ids = m4.spec_generate(target=NativeTarget(hf), input_ids=prompt, max_new_tokens=n_new, stop_token_ids=None,
                           temperature=0.0, draft_token_hook=hook)
    assert ids[0, :33 + n_new].tolist() == want
    for mode in ("0", "1"):     # no hook: rejection on nearly every cycle
        monkeypatch.setenv("DFL_GRAPH", mode)
        r = dflash_generate(make_model(cfg, "mxfp4"), NativeTarget(hf), prompt, cfg.mask_token_id, 48, 16, None, 0.0)
        assert r.output_ids[0].tolist() == G[:33 + 48].tolist(), mode


def test_mxfp4_fallback_paths_equal_the_bf16_model_of_the_dequantised_weights():
    """Paths without a 4-bit kernel read self.w whatever mxfp4_stream says, i.e. they compute what a bf16 model loaded
    with the dequantised weights computes: a 24-row block (hidden rows bit for bit), a sampled draft (sampler="device",
    T = 0.7) and the ragged batch with two requests (ids)."""
    from dflash_amd import DFlashDraftModel, NativeTarget, dflash_generate
    from dflash_amd.batch import dflash_generate_batch
    cfg = H.tiny_cfg()
    sd = H.draft_weights(cfg, seed=3, dtype=BF16)
    m4 = make_model(cfg, "mxfp4", sd=sd)
    mb = DFlashDraftModel(cfg, device=dev(), stream_format="bf16").load_state_dict(_dequantised_state_dict(cfg, sd))
    (oa, ca, _), (ob, cb, _) = run_cycles(m4, cfg, [9, 4, 16], 12, bs=24), run_cycles(mb, cfg, [9, 4, 16], 12, bs=24)
    for x, y in zip(oa, ob):
        assert torch.equal(x, y)
    n = ca.get_seq_length()
    assert torch.equal(ca.k[:, :, :n], cb.k[:, :, :n]) and torch.equal(ca.v[:, :, :n], cb.v[:, :, :n])
    hf, prompt, G, hook = _walk_case(64)
    outs = [dflash_generate(m, NativeTarget(hf), prompt, cfg.mask_token_id, 48, 16, None, 0.7, sampler="device",
                            seed=5) for m in (m4, mb)]
    assert outs[0].output_ids[0].tolist() == outs[1].output_ids[0].tolist()    # the target's seeded draws, either draft
    prompts = [prompt, torch.randint(0, 2000, (1, 21), generator=gen(6)).to(dev())]
    res = []
    for m in (m4, mb):
        rs = dflash_generate_batch(m, NativeTarget(hf), prompts, cfg.mask_token_id, 40, 16, None, 0.0)
        res.append(([r.output_ids[0].tolist() for r in rs], [r.acceptance_lengths for r in rs]))
    assert res[0] == res[1] and res[0][0][0] == G[:33 + 40].tolist()
