"""The two expert launches on e4m3 codes — dfl_moe_gate_up and dfl_moe_down with an e4m3 descriptor (csrc/moe.hip, k_moe_gate_up<true>,
k_moe_down<CT, 16, true>) — against their bf16 siblings on the dequantised weights (bit for bit) and against exact
arithmetic in torch ("The experts").

Why (a) is bit-equality.  A code c is an e4m3 value, exactly representable in bf16, and a scale s = 2^k of
quantize_fp8_rows is a power of two, so the dequantised weight w = c * s is exact in bf16 as well.  The W8 kernels keep,
per wave, the k-steps the bf16 kernels multiply and their order, and the same LDS reduction over the 16 waves.  Scaling
every A operand of a row by 2^k scales every product, every MFMA partial sum and every fp32 addition of that row's sum by
2^k without touching a rounding (no overflow or underflow in range here: |c| <= 448, 2^-20 < s < 1), so the bf16 launch
holds S16 = s * S8 exactly, where S8 is the W8 launch's fp32 sum over the codes.  The W8 epilogue multiplies S8 by s (exact)
in front of the first rounding point — rbf(S8 * s) = rbf(S16) for gate/up; (acc * s) * wr for down, the same `x * wr`
meeting the same running sum as the bf16 form's acc16 * wr — and everything behind that point is the same code on the
same bits.

Inactive experts' activations are pre-filled with NaN and must stay NaN (never written: gate/up; never read: down), and
inactive experts' codes are 0x7F (e4m3 NaN), so that a stray read shows in the sums."""
import pytest
import torch


pytestmark = pytest.mark.gpu
BF16, F32, U8, F8 = torch.bfloat16, torch.float32, torch.uint8, torch.float8_e4m3fn
SCALES = (1.0, 1.5, 0.75, 2.0 ** -3)


def dev():
    return torch.device("cuda", 0)


def _tie_free_logits(rows, E, g):
    """As test_hip_moe._tie_free_logits: bf16 logits with no two equal values in a row."""
    pool = torch.unique((torch.randn(20000, generator=g) * 3).to(BF16))
    assert pool.numel() >= E
    return torch.stack([pool[torch.randperm(pool.numel(), generator=g)[:E]] for _ in range(rows)])


def _int_codes(shape, lim, g):
    """Random integers in [-lim, lim] as (values fp32, e4m3 codes uint8), on the device."""
    vals = torch.arange(-lim, lim + 1, dtype=F32)
    lut = vals.to(F8).view(U8)
    assert torch.equal(lut.view(F8).float(), vals)                 # small integers are e4m3 values
    idx = torch.randint(0, 2 * lim + 1, shape, generator=g, device=dev())
    return vals.to(dev())[idx], lut.to(dev())[idx]


def _pick_scales(shape, g):
    return torch.tensor(SCALES, device=dev())[torch.randint(0, len(SCALES), shape, generator=g, device=dev())]


def _rows_of(act_e, I):
    """One expert's frag16 activation tile [I/8][16][8] -> rows [16, I]."""
    return act_e.view(I // 8, 16, 8).permute(1, 0, 2).reshape(16, I)


def _frag_rows(a):
    """a [..., 16, I] bf16 rows -> [..., 16*I] frag16."""
    *lead, m, I = a.shape
    return a.reshape(-1, m, I // 8, 8).permute(0, 2, 1, 3).reshape(*lead, m * I).contiguous()


def _active_list(E, k, g):
    on = torch.zeros(E, dtype=torch.bool, device=dev())
    on[torch.randperm(E, generator=g, device=dev())[:k]] = True
    lst = torch.zeros(E, dtype=torch.int32, device=dev())
    lst[:k] = on.nonzero()[:, 0].to(torch.int32)
    return on, lst, torch.tensor([k], dtype=torch.int32, device=dev())


def _poison(x8, on):
    """Inactive experts' codes -> 0x7F (e4m3 NaN)."""
    x8.wp[~on] = 0x7F
    return x8


GU_SHAPES = [(8, 16, 64, 3, 16), (8, 48, 1088, 5, 11), (16, 768, 2048, 12, 16), (128, 768, 2048, None, 16)]
GU_IDS = ["one-pair-K64", "KS34-11rows", "576-items", "30b-a3b-routed"]


@pytest.mark.parametrize("E,I,K,nact,rows", GU_SHAPES, ids=GU_IDS)
def test_moe_gate_up_fp8(E, I, K, nact, rows):
    """dfl_moe_gate_up (e4m3) at: one pair where only wave 0 has k-steps (a single 16-byte load); KS = 34 (wave 8 holds
    two k-steps, waves 9..15 none) with 11 valid rows through `dyn`; 576 items > 2 x 256 workgroups (both buffers, the
    loop's second trip); the 30B-A3B geometry routed by dfl_moe_route on tie-free logits.
    (a) power-of-two scales: bit-equal to ops.moe_gate_up on the packed dequantised weights (module docstring).
    (b) integer codes |q| <= 4, integer activations |x| <= 2, per-row scales from {1, 1.5, 0.75, 2^-3}: the gate and up
    sums are exact (|sum| <= 4 * 2 * 2048 = 2^14, times 1.5: 16 bits), so `act` is bf16(silu(bf16(sum_g s_g))) *
    bf16(sum_u s_u) up to the kernel's __expf — the activation bar of test_expert_kernels_at_30b_a3b_shapes: 2e-2 of the
    tile's largest value."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(E + I + K)
    dyn = None
    if rows < 16:
        dyn = torch.zeros(8, dtype=torch.int32, device=dev())
        ops.set_dyn(dyn, 0, 0, rows, 0)
    word = ops.DYN_BS if dyn is not None else -1
    if nact is None:
        cg = torch.Generator().manual_seed(30)
        wt = torch.zeros(16, E, dtype=BF16, device=dev())
        active = torch.zeros(E, dtype=torch.int32, device=dev())
        lst = torch.zeros(E, dtype=torch.int32, device=dev())
        n = torch.zeros(1, dtype=torch.int32, device=dev())
        ops.moe_route(_tie_free_logits(16, E, cg).to(dev()), E, 8, True, wt, active, lst, n)
        on = active != 0
        assert 60 <= int(n) <= 100, int(n)
    else:
        on, lst, n = _active_list(E, nact, g)

    def launch(w):
        act = torch.full((E, 16 * I), float("nan"), dtype=BF16, device=dev())
        ops.moe_gate_up(w, xf, E, I, K, act, lst, n, dyn=dyn, valid_word=word)
        assert torch.isnan(act[~on].float()).all() and torch.isfinite(act[on].float()).all()
        return act

    # ---- (a) bit-equality with the bf16 kernel on q * scale
    w = (torch.randn(E, 2 * I, K, generator=g, device=dev()) * 0.03).to(BF16)
    q, sc = ops.quantize_fp8_rows(w.view(-1, K))
    m, _ = torch.frexp(sc)
    assert torch.all(m == 0.5)
    deq = ops.dequantize_fp8_rows(q, sc).view(E, 2 * I, K)
    x8 = _poison(ops.pack_experts_fp8(q.view(E, 2 * I, K), sc.view(E, 2 * I), gateup=True), on)
    assert x8.wp.shape == (E, 2 * I * K) and x8.scale.shape == (E, 2 * I)
    gu_p = torch.stack([ops.pack_weight_gateup(deq[e, :I].contiguous(), deq[e, I:].contiguous()) for e in range(E)])
    xf = torch.empty(16 * K, dtype=BF16, device=dev())
    ops.pack_rows(torch.randn(16, K, generator=g, device=dev()).to(BF16), 16, xf)
    a8, a16 = launch(x8), launch(gu_p)
    assert torch.equal(a8.view(torch.int16), a16.view(torch.int16))
    del w, q, deq, gu_p, x8

    # ---- (b) exact sums against torch
    qv, qc = _int_codes((E, 2 * I, K), 4, g)
    sc = _pick_scales((E, 2 * I), g)
    x8 = _poison(ops.pack_experts_fp8(qc, sc, gateup=True), on)
    x = torch.randint(-2, 3, (16, K), generator=g, device=dev()).float()
    ops.pack_rows(x.to(BF16), 16, xf)
    x[rows:] = 0
    a8 = launch(x8)
    worst = 0.0
    for e in on.nonzero()[:, 0].tolist():
        s = (x.double() @ qv[e].double().T) * sc[e].double()               # exact: integers, then a 2-bit scale
        assert torch.equal(s, s.float().double())
        gate, up = s.float().to(BF16).chunk(2, dim=-1)
        ref = (torch.nn.functional.silu(gate.float()).to(BF16).float() * up.float()).to(BF16).float()
        got = _rows_of(a8[e], I).float()
        assert torch.equal(got[rows:], torch.zeros_like(got[rows:]))        # masked rows: silu(0) * 0
        assert float(ref.abs().max()) > 0
        err = float((got - ref).abs().max() / ref.abs().max())
        assert err <= 2e-2, (e, err)                                        # (a NaN fails this too)
        worst = max(worst, err)
    print(f"[parity] moe_gate_up_fp8 E {E} I {I} K {K}: worst activation error {worst:.3e} of the tile's largest value")
    assert worst <= 2e-2, worst


def _down_case(E, N, I, nsplit, g, n_on=None):
    """Routing of 16 rows: top-8 with the last 8 experts idle (test_moe_down_at_the_target_grid), or — n_on — every
    row on the same n_on experts.  -> (selection mask [16, E], active mask, list, count)."""
    sel = torch.zeros(16, E, dtype=torch.bool, device=dev())
    if n_on is None:
        for m in range(16):
            sel[m, torch.randperm(E - 8, generator=g, device=dev())[:8]] = True
    else:
        sel[:, torch.randperm(E - 8, generator=g, device=dev())[:n_on]] = True
    on = sel.any(dim=0)
    k = int(on.sum())
    lst = torch.zeros(E, dtype=torch.int32, device=dev())
    lst[:k] = on.nonzero()[:, 0].to(torch.int32)
    return sel, on, lst, torch.tensor([k], dtype=torch.int32, device=dev())


DOWN_SHAPES = [(1, 2048, 768, None), (4, 2048, 768, None), (4, 2064, 768, None), (4, 64, 64, None), (2, 64, 832, None),
               (4, 64, 128, 3)]
DOWN_IDS = ["ns1-N2048-two-tile", "ns4-N2048-two-tile", "ns4-N2064-one-tile", "ns4-one-chunk-of-two", "ns2-KSe26",
            "ns4-3-active-empty-share"]


@pytest.mark.parametrize("nsplit,N,I,n_on", DOWN_SHAPES, ids=DOWN_IDS)
def test_moe_down_fp8(nsplit, N, I, n_on):
    """dfl_moe_down (e4m3) at E 128 with top-8 on 16 rows and the last 8 experts idle: the two-tile form (N % 32 == 0) under
    1 and 4 shares, the one-tile form (N = 2064), one chunk of two k-steps (I = 64), KSe = 26 (the last chunk two
    k-steps), and 3 active experts under 4 shares (one share is empty and must still be written as zeros).
    (a) power-of-two scales: every share of `out` bit-equal to ops.moe_down on the dequantised weights.
    (b) integer activations |a| <= 4, integer codes |q| <= 4, routing weights from {0.25, 0.5, 1}, scales from
    {1, 1.5, 0.75, 2^-3}: every term is a multiple of 2^-5 and a row's sum stays under 8 * 16 * I * 1.5 < 2^18 — dyadic
    rationals of under 24 bits, so every partial sum is exact in fp32 in any order, and out.sum(0) equals the fp64
    einsum of test_moe_down_at_the_target_grid with the scale applied, bit for bit (the budget is asserted on the
    reference: ref == ref.float())."""
    from dflash_amd import ops
    E = 128
    g = torch.Generator(device=dev()).manual_seed(N + I + nsplit)
    sel, on, lst, n = _down_case(E, N, I, nsplit, g, n_on)

    def launch(w, act, wt):
        out = torch.full((nsplit, 16, N), float("nan"), dtype=F32, device=dev())
        ops.moe_down(w, act, wt, lst, n, E, N, I, nsplit, out)
        assert torch.isfinite(out).all()
        return out

    # ---- (a)
    w = (torch.randn(E, N, I, generator=g, device=dev()) * 0.03).to(BF16)
    q, sc = ops.quantize_fp8_rows(w.view(-1, I))
    m, _ = torch.frexp(sc)
    assert torch.all(m == 0.5)
    deq = ops.dequantize_fp8_rows(q, sc).view(E, N, I)
    x8 = _poison(ops.pack_experts_fp8(q.view(E, N, I), sc.view(E, N), gateup=False), on)
    assert x8.wp.shape == (E, N * I) and x8.scale.shape == (E, N)
    dn_p = torch.stack([ops.pack_weight(deq[e].contiguous()) for e in range(E)])
    act = _frag_rows(torch.randn(E, 16, I, generator=g, device=dev()).to(BF16))
    act[~on] = float("nan")
    wt = torch.where(sel, torch.rand(16, E, generator=g, device=dev()) + 0.01, torch.zeros((), device=dev())).to(BF16)
    o8, o16 = launch(x8, act, wt), launch(dn_p, act, wt)
    assert torch.equal(o8.view(torch.int32), o16.view(torch.int32))
    if n_on is not None:                                       # 3 experts over 4 shares: the last share is empty
        assert int(n) == n_on and torch.equal(o8[n_on:], torch.zeros_like(o8[n_on:]))
    del w, q, deq, dn_p, x8

    # ---- (b)
    qv, qc = _int_codes((E, N, I), 4, g)
    sc = _pick_scales((E, N), g)
    x8 = _poison(ops.pack_experts_fp8(qc, sc, gateup=False), on)
    a = torch.randint(-4, 5, (E, 16, I), generator=g, device=dev()).float()
    act = _frag_rows(a.to(BF16))
    act[~on] = float("nan")
    wsel = torch.tensor([0.25, 0.5, 1.0], device=dev())[torch.randint(0, 3, (16, E), generator=g, device=dev())]
    wt = torch.where(sel, wsel, torch.zeros((), device=dev())).to(BF16)
    o8 = launch(x8, act, wt)
    ref = torch.zeros(16, N, dtype=torch.float64, device=dev())
    for e in on.nonzero()[:, 0].tolist():                      # the einsum "emi,eni->emn", one active expert at a time
        y = (a[e].double() @ qv[e].double().T) * sc[e].double()[None, :]
        ref += wt[:, e].double()[:, None] * y
    assert torch.equal(ref, ref.float().double())              # the bit budget: the reference is an fp32 number
    assert float(ref.abs().max()) > 0
    assert torch.equal(o8.sum(0), ref.float())
    if n_on is not None:
        assert torch.equal(o8[n_on:], torch.zeros_like(o8[n_on:]))


def test_fp8_expert_ops_refuse_mismatched_shapes():
    """ops.moe_gate_up / ops.moe_down with an Fp8Experts whose dimensions are not the launch's: an error, no launch."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(1)
    _, qc = _int_codes((4, 32, 64), 2, g)
    x8 = ops.pack_experts_fp8(qc, torch.ones(4, 32, device=dev()), gateup=True)
    z = torch.zeros(4, dtype=torch.int32, device=dev())
    with pytest.raises(ValueError, match="fp8 experts"):
        ops.moe_gate_up(x8, torch.zeros(16 * 64, dtype=BF16, device=dev()), 4, 32, 64, torch.zeros(4, 16 * 32, dtype=BF16, device=dev()),
                        z, z[:1])
    with pytest.raises(ValueError, match="fp8 experts"):
        ops.moe_down(x8, torch.zeros(4, 16 * 64, dtype=BF16, device=dev()), torch.zeros(16, 4, dtype=BF16, device=dev()), z, z[:1],
                     4, 64, 64, 2, torch.zeros(2, 16, 64, device=dev()))
