"""dfl_moe_grouped_gate_up / dfl_moe_grouped_down on MXFP4 expert codes (csrc/moe_w4_shared.hip: k_moe_w4_shared), what the
shared MoE pass of an mxfp4-expert target launches — on dfl_prefill_moe_route's work lists, judged by check_plan.
(a) torch.equal with the bf16 launch of the same entry point on the dequantised weights over the same plan: e2m1 * 2^n
    is exact in bf16, and the kernel keeps the bf16 form's k-steps and their order into every accumulator.
(b) fp64 on small-integer activations.  A product is a multiple of 2^-11 (gate/up: scale codes 117..121, |x| <= 2,
    K <= 2176: |sum| < 2^9, 20 bits) or of 2^-10 (down: scale codes 118 / 119, |a| <= 2, I <= 768: 16 bits, times an 8-bit
    routing weight: 24) — every sum is exact in fp32 in any order (asserted), so the down rows match bit for bit and the
    gate/up activations stand inside the 2e-2 bar of tests/test_hip_fp8_experts_kernels.py (the kernel's __expf).
(c) outputs are pre-filled with NaN: nothing is written beyond the items' tiles, every row of them is.
Idle experts hold arbitrary codes under scale code 0xFF (e8m0 NaN); the bf16 arm's idle experts are NaN."""
import pytest
import torch

import test_hip_fp8_experts_shared_kernels as F

pytestmark = pytest.mark.gpu
BF16, F64, U8 = torch.bfloat16, torch.float64, torch.uint8


def _experts4(ops, E, N, K, gateup, on, g, lo, hi):
    """Random e2m1 codes, scale codes lo..hi -> (Mxfp4Experts with the idle experts' scales 0xFF, dequantised bf16 [E, N, K])."""
    codes = torch.randint(0, 256, (E, N, K // 2), generator=g, device=F.dev()).to(U8)
    scales = torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, device=F.dev()).to(U8)
    deq = ops.dequantize_mxfp4_rows(codes.view(E * N, -1), scales.view(E * N, -1)).view(E, N, K)
    x4 = ops.pack_experts_mxfp4(codes, scales, gateup=gateup)
    x4.sc[~on] = 0xFF
    assert x4.sc.data_ptr() % 64 == 0
    return x4, deq


def _plan(sc, st):
    n_tiles = st["n_items"][1]
    owner = torch.zeros(n_tiles * 16, dtype=torch.long, device=F.dev())
    for e, t0, nt in st["items"]:
        owner[t0 * 16:(t0 + nt) * 16] = e
    return n_tiles, sc["src_row"][:n_tiles * 16].long(), owner


def _check_gate_up(ops, kind, I, K, rows_per_item, g, sc=None):
    sc, pe, pw, st, on = F._route(ops, kind, K, I, rows_per_item, g, sc)
    E, P = sc["E"], pe.shape[0]
    n_tiles, srow, owner = _plan(sc, st)
    x4, deq = _experts4(ops, E, 2 * I, K, True, on, g, 117, 121)
    gu_p = F._pack_bf16(ops, deq, True, on)
    xf = F._x_tiles(ops, torch.randn(P, K, generator=g, device=F.dev()).to(BF16))
    F._gather(ops, xf, sc, P, K, n_tiles)
    a4 = F._gate_up(ops, x4, xf, sc, K, n_tiles, gather=True)                       # (c) inside
    for w, gather in ((gu_p, True), (x4, False), (gu_p, False)):
        assert torch.equal(F._bits(a4), F._bits(F._gate_up(ops, w, xf, sc, K, n_tiles, gather=gather))), (type(w), gather)
    assert bool((a4[srow < 0] == 0).all()) and float(a4.float().abs().max()) > 0
    x = torch.randint(-2, 3, (P, K), generator=g, device=F.dev()).float()
    xf = F._x_tiles(ops, x.to(BF16))
    F._gather(ops, xf, sc, P, K, n_tiles)
    xg = torch.where((srow >= 0)[:, None], x[srow.clamp_min(0)], torch.zeros((), device=F.dev()))
    for gather in (True, False):
        got = F._gate_up(ops, x4, xf, sc, K, n_tiles, gather=gather).float()
        for e in on.nonzero()[:, 0].tolist():
            m = owner == e
            s = xg[m].double() @ deq[e].double().T
            assert torch.equal(s, s.float().double())
            gate, up = s.float().to(BF16).chunk(2, dim=-1)
            ref = (torch.nn.functional.silu(gate.float()).to(BF16).float() * up.float()).to(BF16).float()
            err = float((got[m] - ref).abs().max() / ref.abs().max())
            print(f"[parity] grouped gate/up W4 {kind} I {I} K {K} expert {e} gather {gather}: {err:.3e}")
            assert float(ref.abs().max()) > 0 and err <= 2e-2, (e, gather, err)
    return sc


def _check_down(ops, kind, N, I, rows_per_item, g, sc=None):
    sc, pe, pw, st, on = F._route(ops, kind, N, I, rows_per_item, g, sc)
    E, P, top_k = sc["E"], pe.shape[0], sc["top_k"]
    n_tiles, srow, owner = _plan(sc, st)
    row_w = sc["row_w"][:n_tiles * 16].clone()

    def set_act(rows):                                           # the tiles beyond n_tiles hold NaN
        a = torch.full((sc["act_g"].numel() // I, I), float("nan"), dtype=BF16, device=F.dev())
        a[:n_tiles * 16] = rows
        sc["act_g"].copy_(F._pack_tiles(a))

    x4, deq = _experts4(ops, E, N, I, False, on, g, 117, 121)
    set_act(torch.randn(n_tiles * 16, I, generator=g, device=F.dev()).to(BF16))
    o4 = F._down(ops, x4, sc, N, n_tiles)                                           # (c) inside
    assert torch.equal(F._bits(o4), F._bits(F._down(ops, F._pack_bf16(ops, deq, False, on), sc, N, n_tiles)))
    assert bool((o4[srow < 0] == 0).all()) and float(o4.abs().max()) > 0
    x4, deq = _experts4(ops, E, N, I, False, on, g, 118, 119)
    a = torch.randint(-2, 3, (n_tiles * 16, I), generator=g, device=F.dev()).float()
    set_act(a.to(BF16))
    o4 = F._down(ops, x4, sc, N, n_tiles)
    ref = torch.zeros(n_tiles * 16, N, dtype=F64, device=F.dev())
    for e in on.nonzero()[:, 0].tolist():
        m = owner == e
        ref[m] = row_w[m].double()[:, None] * (a[m].double() @ deq[e].double().T)
    assert torch.equal(ref, ref.float().double()) and float(ref.abs().max()) > 0     # the bit budget of (b)
    assert torch.equal(o4, ref.float()), "out32 differs from the fp64 reference"
    pos = sc["posmap"][:P, :top_k].long()
    assert torch.equal(o4[pos], ref.float()[pos])                # every routed pair finds its row
    return sc


@pytest.mark.parametrize("rows_per_item", [64, 128])
@pytest.mark.parametrize("I,K", [(128, 128), (192, 384), (384, 640), (128, 2176)],
                         ids=["K128-prologue-only", "I192-K384-12-pairs-odd-words", "I384-K640-ring-wraps", "K2176-above-2048"])
def test_grouped_gate_up_mxfp4(I, K, rows_per_item):
    """The "skew" routing: an expert over two items of 4 + 3 tiles (64) / one of 7 in two passes (128), an expert with one
    tile of 5 rows, an expert without rows; from src_row and from the gathered copy.  12 pairs: a last workgroup with
    four idle waves."""
    from dflash_amd import ops
    _check_gate_up(ops, "skew", I, K, rows_per_item, torch.Generator(device=F.dev()).manual_seed(I + K + rows_per_item))


@pytest.mark.parametrize("rows_per_item", [64, 128])
@pytest.mark.parametrize("N,I", [(128, 128), (384, 384), (128, 384)], ids=["N128-I128-one-word", "N384-I384", "N128-I384-three-words"])
def test_grouped_down_mxfp4(N, I, rows_per_item):
    """The same routing for the down projection: 4 and 12 column units (workgroups with idle waves), K of 1 and 3 words."""
    from dflash_amd import ops
    _check_down(ops, "skew", N, I, rows_per_item, torch.Generator(device=F.dev()).manual_seed(N + I + rows_per_item))


@pytest.mark.parametrize("rows_per_item", [64, 128])
def test_grouped_mxfp4_on_a_reused_scratch(rows_per_item):
    """P = 100, then P = 40 with another idle expert, on one scratch: the second plan stands on its own."""
    from dflash_amd import ops
    g = torch.Generator(device=F.dev()).manual_seed(44 + rows_per_item)
    sc = _check_gate_up(ops, "skew", 128, 128, rows_per_item, g)
    first = int(sc["n_items"][1])
    sc = _check_gate_up(ops, "second", 128, 128, rows_per_item, g, sc=sc)
    assert int(sc["n_items"][1]) < first
    sc = _check_down(ops, "skew", 128, 128, rows_per_item, g, sc=sc)
    _check_down(ops, "second", 128, 128, rows_per_item, g, sc=sc)


def test_grouped_mxfp4_at_the_operating_point():
    """E 128, top-8, 64 rows, hidden 2048, experts of 768: a 30B-A3B layer's shared pass, rows_per_item as the scratch picks."""
    from dflash_amd import ops
    g = torch.Generator(device=F.dev()).manual_seed(30)
    _check_gate_up(ops, "a3b", 768, 2048, None, g)
    _check_down(ops, "a3b", 2048, 768, None, g)
