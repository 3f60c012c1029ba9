"""dfl_moe_gate_up / dfl_moe_down on MXFP4 codes (csrc/moe_w4.hip) against their bf16 siblings on the dequantised weights,
bit for bit — e2m1 * 2^n is exact in bf16 and the block scale rides in the conversion, so the same bf16 fragments meet the
same MFMAs in the same order — and against exact arithmetic in fp64 ("The experts").  Inactive
experts carry scale code 0xFF (NaN in e8m0) and NaN activations throughout, so that a stray read shows."""
import pytest
import torch

from test_hip_fp8_experts_kernels import _active_list, _down_case, _frag_rows, _rows_of, _tie_free_logits, dev

pytestmark = pytest.mark.gpu
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8


def _experts(ops, codes, scales, on, gateup):
    """-> (Mxfp4Experts, inactive experts' scales poisoned; packed bf16 experts of the dequantised weights; those as fp64)."""
    E, N, _ = codes.shape
    deq = ops.dequantize_mxfp4_rows(codes.view(E * N, -1), scales.view(E * N, -1)).view(E, N, -1)
    x4 = ops.pack_experts_mxfp4(codes, scales, gateup=gateup)
    x4.sc[~on] = 0xFF
    if gateup:
        wp = torch.stack([ops.pack_weight_gateup(deq[e, :N // 2].contiguous(), deq[e, N // 2:].contiguous()) for e in range(E)])
    else:
        wp = torch.stack([ops.pack_weight(deq[e].contiguous()) for e in range(E)])
    return x4, wp, deq.double()


def _quantised(ops, E, N, K, g):
    w = (torch.randn(E * N, K, generator=g, device=dev()) * 0.03).to(BF16)
    q, sc = ops.quantize_mxfp4_rows(w)
    return q.view(E, N, -1), sc.view(E, N, -1)


def _random_codes(E, N, K, g):
    """Every e2m1 code under block scales 0.5, 1 and 2: weights that are multiples of 0.25, at most 12."""
    return (torch.randint(0, 256, (E, N, K // 2), generator=g, device=dev(), dtype=torch.int32).to(U8),
            torch.randint(126, 129, (E, N, K // 32), generator=g, device=dev(), dtype=torch.int32).to(U8))


GU_SHAPES = [(8, 16, 128, 3, 16), (8, 48, 1152, 5, 11), (16, 1152, 2048, 8, 16), (128, 768, 2048, None, 16)]
GU_IDS = ["K128-one-word-one-pair", "K1152-nine-waves-11rows-odd-npp", "more-items-than-workgroups", "30b-a3b-routed"]


@pytest.mark.parametrize("E,I,K,nact,rows", GU_SHAPES, ids=GU_IDS)
def test_moe_gate_up_mxfp4(E, I, K, nact, rows):
    """K = 128 (one word: waves 1..15 idle) with ONE pair per expert (a two-pair form's tail); K = 1152 (nine waves), 11 valid
    rows through `dyn`, three pairs per expert; K = 2048 with 8 x 72 pairs (more items than 256 workgroups in either form);
    the 30B-A3B geometry routed by dfl_moe_route.  (a) quantised Gaussian weights and rows: bit-equal to the bf16 launch.
    (b) every code under scales {0.5, 1, 2}, integer |x| <= 2: products are multiples of 0.25 and a sum stays under 24 * 2048
    < 2^16 — 18 bits, exact in fp32 in any order — so `act` is bf16(silu(bf16(sum_g))) * bf16(sum_u) up to the kernel's
    __expf: the 2e-2 activation bar of helpers.assert_close, of the tile's largest value."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(E + I + K)
    dyn = None
    if rows < 16:
        dyn = torch.zeros(8, dtype=torch.int32, device=dev())
        ops.set_dyn(dyn, 0, 0, rows, 0)
    if nact is None:
        wt, active, lst = torch.zeros(16, E, dtype=BF16, device=dev()), *torch.zeros(2, E, dtype=torch.int32, device=dev())
        n = torch.zeros(1, dtype=torch.int32, device=dev())
        ops.moe_route(_tie_free_logits(16, E, torch.Generator().manual_seed(30)).to(dev()), E, 8, True, wt, active, lst, n)
        on = active != 0
        assert 60 <= int(n) <= 100, int(n)
    else:
        on, lst, n = _active_list(E, nact, g)
    xf = torch.empty(16 * K, dtype=BF16, device=dev())

    def launch(w):
        act = torch.full((E, 16 * I), float("nan"), dtype=BF16, device=dev())
        ops.moe_gate_up(w, xf, E, I, K, act, lst, n, dyn=dyn, valid_word=ops.DYN_BS if dyn is not None else -1)
        assert torch.isnan(act[~on].float()).all() and torch.isfinite(act[on].float()).all()
        return act

    x4, wp, _ = _experts(ops, *_quantised(ops, E, 2 * I, K, g), on, True)
    ops.pack_rows(torch.randn(16, K, generator=g, device=dev()).to(BF16), 16, xf)
    assert torch.equal(launch(x4).view(torch.int16), launch(wp).view(torch.int16))
    del x4, wp

    x4, wp, deq = _experts(ops, *_random_codes(E, 2 * I, K, g), on, True)
    x = torch.randint(-2, 3, (16, K), generator=g, device=dev()).float()
    ops.pack_rows(x.to(BF16), 16, xf)
    x[rows:] = 0
    a4 = launch(x4)
    assert torch.equal(a4.view(torch.int16), launch(wp).view(torch.int16))
    worst = 0.0
    for e in on.nonzero()[:, 0].tolist():
        s = x.double() @ deq[e].T
        assert torch.equal(s, s.float().double())                            # the bit budget: fp32 numbers
        gate, up = s.float().to(BF16).chunk(2, dim=-1)
        ref = (torch.nn.functional.silu(gate.float()).to(BF16).float() * up.float()).to(BF16).float()
        got = _rows_of(a4[e], I).float()
        assert torch.equal(got[rows:], torch.zeros_like(got[rows:]))          # masked rows: silu(0) * 0
        worst = max(worst, float((got - ref).abs().max() / ref.abs().max()))
    print(f"[parity] moe_gate_up_mxfp4 E {E} I {I} K {K}: worst activation error {worst:.3e} of the tile's largest value")
    assert worst <= 2e-2, worst


DOWN_SHAPES = [(1, 2048, 768, None), (4, 2048, 768, None), (4, 2080, 128, None), (4, 2064, 128, None), (2, 64, 896, None),
               (4, 64, 128, 3)]
DOWN_IDS = ["ns1-N2048-widest", "ns4-N2048-widest", "ns4-N2080-two-tile-one-chunk", "ns4-N2064-one-tile-one-chunk",
            "ns2-seven-chunks", "ns4-3-active-empty-share"]


@pytest.mark.parametrize("nsplit,N,I,n_on", DOWN_SHAPES, ids=DOWN_IDS)
def test_moe_down_mxfp4(nsplit, N, I, n_on):
    """E 128, top-8 on 16 rows, the last 8 experts idle: the widest form (N % 64 == 0 serves two and four column tiles alike)
    under 1 and 4 shares; N = 2080 (two tiles, not four) and N = 2064 (one tile) at one chunk (I = 128); seven chunks; 3
    active experts under 4 shares (the empty share is zeros).  (a) quantised Gaussian weights: every share bit-equal to the
    bf16 launch.  (b) every code under scales {0.5, 1, 2}, integer |a| <= 4, routing weights from {0.25, 0.5, 1}: terms are
    multiples of 2^-4, a row's sum stays under 8 * 896 * 48 < 2^19 — 23 bits, exact in fp32 in any order — so out.sum(0)
    equals the fp64 sum bit for bit (the budget is asserted on the reference)."""
    from dflash_amd import ops
    E = 128
    g = torch.Generator(device=dev()).manual_seed(N + I + nsplit)
    sel, on, lst, n = _down_case(E, N, I, nsplit, g, n_on)

    def launch(w, act, wt):
        out = torch.full((nsplit, 16, N), float("nan"), dtype=F32, device=dev())
        ops.moe_down(w, act, wt, lst, n, E, N, I, nsplit, out)
        assert torch.isfinite(out).all()
        if n_on is not None:                                       # 3 experts over 4 shares: the last share is empty
            assert int(n) == n_on and torch.equal(out[n_on:], torch.zeros_like(out[n_on:]))
        return out

    x4, wp, _ = _experts(ops, *_quantised(ops, E, N, I, g), on, False)
    act = _frag_rows(torch.randn(E, 16, I, generator=g, device=dev()).to(BF16))
    act[~on] = float("nan")
    wt = torch.where(sel, torch.rand(16, E, generator=g, device=dev()) + 0.01, torch.zeros((), device=dev())).to(BF16)
    assert torch.equal(launch(x4, act, wt).view(torch.int32), launch(wp, act, wt).view(torch.int32))
    del x4, wp

    x4, wp, deq = _experts(ops, *_random_codes(E, N, I, g), on, False)
    a = torch.randint(-4, 5, (E, 16, I), generator=g, device=dev()).float()
    act = _frag_rows(a.to(BF16))
    act[~on] = float("nan")
    wsel = torch.tensor([0.25, 0.5, 1.0], device=dev())[torch.randint(0, 3, (16, E), generator=g, device=dev())]
    wt = torch.where(sel, wsel, torch.zeros((), device=dev())).to(BF16)
    o4 = launch(x4, act, wt)
    assert torch.equal(o4.view(torch.int32), launch(wp, act, wt).view(torch.int32))
    ref = torch.zeros(16, N, dtype=torch.float64, device=dev())
    for e in on.nonzero()[:, 0].tolist():
        ref += wt[:, e].double()[:, None] * (a[e].double() @ deq[e].T)
    assert torch.equal(ref, ref.float().double()) and float(ref.abs().max()) > 0
    assert torch.equal(o4.sum(0), ref.float())
