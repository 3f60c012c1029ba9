"""FP8 (e4m3) draft weights in the ragged batch on the GPU ("The batch forms"): the W8 forms of the
ring kernel (gate/up + SiLU*up, lm_head + argmax) and of the register-resident K-part GEMM against torch on exact
operands and, bit for bit, against their bf16 siblings on the dequantised copy."""
import pytest
import torch

import fp8_batch_cases as FC
import helpers as H

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32


def dev():
    return torch.device("cuda", 0)


def _gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _ints(shape, g):
    """int8 in [-2, 2] on the device: every product and every fp32 sum of up to 2^20 of them is exact"""
    return torch.randint(-2, 3, shape, generator=g, device=dev(), dtype=torch.int8)


_LUT = [0xC0, 0xB8, 0x00, 0x38, 0x40]   # e4m3 codes of -2, -1, 0, 1, 2


def _codes(w_int):
    return torch.tensor(_LUT, dtype=torch.uint8, device=w_int.device)[(w_int.long() + 2)]


def _bf16_steps(a, b):
    def line(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def _pow2(n, period, e0):
    """fp32 [n]: 2^(e0 + i % period)"""
    return torch.exp2((torch.arange(n, device=dev()) % period + e0).float())


def _frag(x):
    from dflash_amd import ops
    return ops.brows_frag(H.frag_of(x))


# ---------------------------------------------------------------- ring form, gate/up + SiLU * up
def _silu_ref(x, gate_sum_scaled, up_sum_scaled):
    gb, ub = gate_sum_scaled.to(BF16).float(), up_sum_scaled.to(BF16).float()
    return (torch.nn.functional.silu(gb).to(BF16).float() * ub).to(BF16)


@pytest.mark.parametrize("R,I,K", FC.SILU_CASES, ids=[FC.case_id(c) for c in FC.SILU_CASES])
def test_ring_silu_fp8_exact_ints(R, I, K):
    """Integer codes and activations in [-2, 2]: the gate and up sums are exact integers, and so are their products with
    the scales below (powers of two that differ between gate and up and from row to row; then 1.5 * 2^-5 / 0.75: a
    3-bit factor on an 11-bit integer), so the output is torch's at torch's rounding points up to the SiLU's exp — the
    bars of test_ring_gemm_silu_mul_batch's integer kinds: at most 2 bf16 steps, at most 1e-3 of the elements off."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _gen(R + I + K)
    dyn = H.dyn_records([(0, 16)] * MT, MT, dev())
    ws = ops.gemm_batch_ws(2 * I, K, dev())
    gate, up, x = _ints((I, K), g), _ints((I, K), g), _ints((MT, 16, K), g).to(BF16)
    gs, us = x.float().view(MT * 16, K) @ gate.float().T, x.float().view(MT * 16, K) @ up.float().T   # exact
    for kind, sg, su in (("pow2", _pow2(I, 5, -7), _pow2(I, 3, -1)),
                         ("3-bit", torch.full((I,), 1.5 * 2 ** -5, device=dev()), torch.full((I,), 0.75, device=dev()))):
        w8 = ops.pack_weight_gateup_fp8(_codes(gate), sg, _codes(up), su)
        act = torch.full((MT, 16 * I), float("nan"), dtype=BF16, device=dev())
        ops.gemm_silu_mul_batch(w8, _frag(x), R, I, K, act, ws, dyn)
        want = _silu_ref(x, gs * sg[None], us * su[None]).view(MT, 16, I)
        for r in range(R):
            got = H.unfrag(act[r], I)
            assert not torch.isnan(got.float()).any(), (kind, r)
            d = _bf16_steps(got, want[r])
            off = float((d > 0).float().mean())
            print(f"[parity] fp8 ring silu {kind} R{R} I{I} K{K} r{r}: max {int(d.max())} bf16 steps, {off:.2e} off")
            assert int(d.max()) <= 2 and off <= 1e-3, (kind, r, int(d.max()), off)


@pytest.mark.parametrize("R,I,K", FC.SILU_CASES, ids=[FC.case_id(c) for c in FC.SILU_CASES])
def test_ring_silu_fp8_equals_the_bf16_ring_on_the_copy(R, I, K):
    """Random data quantised by quantize_fp8_rows: the W8 launch equals the bf16 ring launch on the dequantised copy
    bit for bit.  Derivable: both forms give every wave the same k-steps in the same order, and a power-of-two row
    scale commutes with every fp32 rounding (random normal data stays far from the denormal range)."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _gen(3 * R + I + K)
    dyn = H.dyn_records([(0, 16)] * MT, MT, dev())
    ws = ops.gemm_batch_ws(2 * I, K, dev())
    gate = (torch.randn(I, K, generator=g, device=dev()) * 0.05).to(BF16)
    up = (torch.randn(I, K, generator=g, device=dev()) * 0.05).to(BF16)
    x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    (qg, sg), (qu, su) = ops.quantize_fp8_rows(gate), ops.quantize_fp8_rows(up)
    outs = []
    for wp in (ops.pack_weight_gateup_fp8(qg, sg, qu, su),
               ops.pack_weight_gateup(ops.dequantize_fp8_rows(qg, sg), ops.dequantize_fp8_rows(qu, su))):
        act = torch.full((MT, 16 * I), float("nan"), dtype=BF16, device=dev())
        ops.gemm_silu_mul_batch(wp, _frag(x), R, I, K, act, ws, dyn)
        outs.append(act)
    assert not torch.isnan(outs[0].float()).any()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


# ---------------------------------------------------------------- ring form, lm_head + argmax
LM_BS = {1: [16], 2: [16, 1], 3: [16, 5, 1], 4: [16, 9, 1, 13]}   # rows per request: ragged, one with a single row


def _first_argmax(lg):
    m = lg.max(dim=-1, keepdim=True).values
    idx = torch.arange(lg.shape[-1], device=lg.device).expand_as(lg)
    return torch.where(lg == m, idx, lg.shape[-1]).min(dim=-1).values


def _forced_ties(V, x0):
    """Weight rows (ints, scale) that give rows 1..6 of request 0 their maximum — the largest logit a column can reach,
    2 sum|x| — at exactly two columns each: inside a lane's four columns, across the column groups of a tile, across
    workgroups, across waves of a workgroup (upp >= 2), across passes (npass >= 2), and a tie that exists only after
    scaling: the LOWER column holds sign(x) at scale 2, the higher one 2 sign(x) at scale 1."""
    f = FC.argmax_form(4, V)
    gx, upp, npass = f["gx"], f["upp"], f["npass"]

    def tile(b, p, uu):
        t = b + (p * upp + uu) * gx
        assert t < V // 16, (b, p, uu)
        return t
    u = min(1, upp - 1)
    pairs = {1: ((16 * tile(3, 0, 0) + 5, 2, 1.0), (16 * tile(3, 0, 0) + 6, 2, 1.0)),
             2: ((16 * tile(1, 0, 0) + 13, 2, 1.0), (16 * tile(1, 0, 0) + 6, 2, 1.0)),
             3: ((16 * tile(5, 0, u) + 7, 2, 1.0), (16 * tile(6, 0, u) + 7, 2, 1.0)),
             6: ((16 * tile(9, 0, 0) + 3, 1, 2.0), (16 * tile(11, 0, 0) + 3, 2, 1.0))}
    if upp >= 2:
        pairs[4] = ((16 * tile(2, 0, 0) + 14, 2, 1.0), (16 * tile(2, 0, 1) + 14, 2, 1.0))
    if npass >= 2:
        pairs[5] = ((16 * tile(4, 0, u) + 9, 2, 1.0), (16 * tile(4, npass - 1, u) + 9, 2, 1.0))
    rows = {}
    for m, cols in pairs.items():
        for c, mult, sc in cols:
            assert c not in rows
            rows[c] = ((mult * torch.sign(x0[m].float())).to(torch.int8), sc)
    return pairs, rows


@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("R,V,K", FC.ARGMAX_CASES, ids=[FC.case_id(c) for c in FC.ARGMAX_CASES])
def test_ring_argmax_fp8_exact_ties(R, V, K, row0):
    """Integer codes, scales 1 / 0.5 / 0.25 by row: the bf16 logits are known exactly, so the ids must be the first
    maximum of the reference logits through every merge (lane, column groups, waves, workgroups, passes), with the
    forced ties of _forced_ties; the logits, where asked for, equal the reference bit for bit; rows outside a tile's
    count keep the prefilled sentinel."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _gen(V + K + R)
    x = _ints((MT, 16, K), g).to(BF16)
    w = _ints((V, K), g)
    scale = _pow2(V, 3, -2)
    pairs, rows = _forced_ties(V, x[0])
    for c, (row, sc) in rows.items():
        w[c], scale[c] = row, sc
    bss = LM_BS[R] + [0] * (MT - R)
    dyn = H.dyn_records([(0, b) for b in bss], MT, dev())
    w8 = ops.pack_weight_fp8(_codes(w), scale)
    ws = ops.gemm_batch_ws(V, K, dev())
    ref_bf = ((x.view(MT * 16, K).float() @ w.float().T) * scale[None]).view(MT, 16, V).to(BF16)   # exact before the rounding
    del w
    runs = []
    for with_logits in (False, True):
        ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
        logits = torch.full((MT, 16, V), 3.0, dtype=BF16, device=dev()) if with_logits else None
        ops.gemm_argmax_batch(w8, _frag(x), R, V, K, row0, 16 - row0, ws, ids, row0, dyn, nrows_dyn_word=ops.DYN_BS,
                              logits=logits)
        runs.append((ids, logits))
    (ids0, _), (ids1, logits) = runs
    for m, ((a, _, _), (b, _, _)) in pairs.items():
        top = ref_bf[0, m].float()
        assert top[a] == top[b] == top.max() and int((top == top.max()).sum()) == 2, m
        assert int(ids0[0, m]) == min(a, b), (m, a, b, int(ids0[0, m]))
    for r in range(MT):
        n = max(bss[r] - row0, 0)
        for ids in (ids0, ids1):
            assert torch.all(ids[r, :row0] == -1) and torch.all(ids[r, row0 + n:] == -1), r
        if n == 0:
            assert torch.all(logits[r] == 3.0), r
            continue
        lg = ref_bf[r, row0:row0 + n]
        want = _first_argmax(lg.float())
        assert torch.equal(ids0[r, row0:row0 + n], want), (r, ids0[r].tolist(), want.tolist())
        assert torch.equal(ids1[r, row0:row0 + n], want), r
        assert torch.equal(logits[r, row0:row0 + n], lg), r
        assert torch.all(logits[r, :row0] == 3.0) and torch.all(logits[r, row0 + n:] == 3.0), r


@pytest.mark.parametrize("R,V,K", FC.ARGMAX_CASES, ids=[FC.case_id(c) for c in FC.ARGMAX_CASES])
def test_ring_argmax_fp8_equals_the_bf16_ring_on_the_copy(R, V, K):
    """Random data: ids, and the logits when they are asked for, equal the bf16 ring launch on the dequantised copy."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _gen(V + K + 100 * R)
    x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    w = (torch.randn(V, K, generator=g, device=dev()) * 0.05).to(BF16)
    q, sc = ops.quantize_fp8_rows(w)
    del w
    bss = LM_BS[R] + [0] * (MT - R)
    dyn = H.dyn_records([(0, b) for b in bss], MT, dev())
    ws = ops.gemm_batch_ws(V, K, dev())
    outs = []
    for wp in (ops.pack_weight_fp8(q, sc), ops.pack_weight(ops.dequantize_fp8_rows(q, sc))):
        for with_logits in (False, True):
            ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
            logits = torch.full((MT, 16, V), 3.0, dtype=BF16, device=dev()) if with_logits else None
            ops.gemm_argmax_batch(wp, _frag(x), R, V, K, 1, 15, ws, ids, 1, dyn, nrows_dyn_word=ops.DYN_BS, logits=logits)
            outs.append((ids, logits))
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[1][0], outs[3][0]) and torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[1][1].view(torch.int16), outs[3][1].view(torch.int16))
    assert int(outs[0][0][0, 1:].min()) >= 0 and int(outs[0][0].max()) < V


# ---------------------------------------------------------------- register-resident form, fp32 K parts
def _f32_run(ops, wp, x, R, N, K, dyn):
    MT, ks = ops.batch_tiles(R), ops.batch_ksplit(K)
    out = torch.full((ks, MT * 16, N), float("nan"), dtype=F32, device=dev())
    ops.gemm_f32_batch(wp, _frag(x), R, N, K, out, dyn)
    return out.view(ks, MT, 16, N)[:, :R]


@pytest.mark.parametrize("R,N,K", FC.F32_CASES, ids=[FC.case_id(c) for c in FC.F32_CASES])
def test_gemm_f32_batch_fp8_exact_ints(R, N, K):
    """Integer codes and activations, power-of-two scales by row: every K part is the exact scaled sum over its own
    k-steps (part c: the 8 * nfr k-steps from c times that many), and the parts add up to x @ (q * scale)^T exactly."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    f = FC.f32_form(R, N, K)
    assert f["ksplit"] == ops.batch_ksplit(K)
    g = _gen(R + N + K)
    x, w = _ints((MT, 16, K), g).to(BF16), _ints((N, K), g)
    scale = _pow2(N, 5, -2)
    dyn = H.dyn_records([(0, 16)] * MT, MT, dev())
    out = _f32_run(ops, ops.pack_weight_fp8(_codes(w), scale), x, R, N, K, dyn)
    wd = w.float() * scale[:, None]
    assert torch.equal(out.sum(0), x[:R].float() @ wd.T)
    span = 8 * f["nfr"] * 32
    for c in range(f["ksplit"]):
        k0, k1 = min(c * span, K), min((c + 1) * span, K)
        assert torch.equal(out[c], x[:R, :, k0:k1].float() @ wd[:, k0:k1].T), c


@pytest.mark.parametrize("R,N,K", FC.F32_CASES, ids=[FC.case_id(c) for c in FC.F32_CASES])
def test_gemm_f32_batch_fp8_random(R, N, K):
    """Random data.  Where the bf16 form's share per wave is even, both forms give every wave the same k-steps: every
    part equals the bf16 launch on the dequantised copy bit for bit.  K = 2560 (5 k-steps per wave in bf16, 6 in W8):
    the summed parts lie within the fp32 summation bound K * 2^-24 * (|x| @ |q * scale|^T) of fp64, elementwise."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _gen(7 * R + N + K)
    x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    w = (torch.randn(N, K, generator=g, device=dev()) * 0.05).to(BF16)
    q, sc = ops.quantize_fp8_rows(w)
    deq = ops.dequantize_fp8_rows(q, sc)
    dyn = H.dyn_records([(0, 16)] * MT, MT, dev())
    got = _f32_run(ops, ops.pack_weight_fp8(q, sc), x, R, N, K, dyn)
    assert torch.isfinite(got).all()
    if FC.f32_form(R, N, K, w8=False)["nfr"] % 2 == 0:
        assert torch.equal(got, _f32_run(ops, ops.pack_weight(deq), x, R, N, K, dyn))
    else:
        assert K == 2560
        ref = x[:R].double() @ deq.double().T
        bound = K * 2.0 ** -24 * (x[:R].double().abs() @ deq.double().abs().T)
        err = (got.sum(0).double() - ref).abs()     # (the parts summed in fp32, as the next launch does)
        print(f"[parity] fp8 f32 parts R{R} N{N} K{K}: worst error {float((err / bound).max()):.3f} of the bound")
        assert torch.all(err <= bound)
