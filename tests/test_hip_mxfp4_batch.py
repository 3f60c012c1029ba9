"""MXFP4 draft weights in the ragged batch on the GPU ("The batch forms"): the 4-bit ring kernel
(gate/up + SiLU * up, lm_head + argmax) and the 4-bit K-part GEMM, bit for bit against their bf16 siblings on the
dequantised weights, and against fp64 on operands whose every partial sum is exact in fp32."""
import pytest
import torch

import fp8_batch_cases as FC
import helpers as H
from arena import Arena
from test_hip_fp8_batch import LM_BS, _bf16_steps, _first_argmax, _forced_ties, _frag, _gen, _silu_ref

pytestmark = pytest.mark.gpu
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8

# (R, I, K).  The 4-bit plan is the bf16 ring's (fp8_batch_cases.silu_form: 3 or 4 units of FOUR waves per workgroup and
# pass): I = 64 fewer units than a workgroup's slots, 1024 one unit per workgroup, 12288 / 16384 one pass of 3 / 4 units,
# 14336 a tail workgroup, 17408 several passes with a tail.  K = 256: one chunk, fewer than the look-ahead; 384: a partial
# last chunk (one word of two); 1152: 9 chunks, the ring (5 or 9 slots) wraps.
SILU4 = [(1, 64, 256), (3, 1024, 384), (2, 8192, 256), (4, 12288, 1152), (4, 14336, 256), (2, 16384, 384), (4, 17408, 256),
         (1, 1024, 1152), (3, 64, 1152), (2, 64, 384), (4, 64, 384)]
ARGMAX4 = [(1, 2048, 256), (4, 4208, 384), (3, 69632, 256), (4, 151936, 512), (2, 4208, 512)]
F32_4 = [(1, 64, 1024), (4, 512, 4096), (3, 4112, 1024), (4, 256, 12288), (2, 64, 32768)]


def dev():
    return torch.device("cuda", 0)


def _nibbles(shape, g):
    """one e2m1 code per element over all 15 values (no -0)"""
    n = torch.randint(0, 15, shape, generator=g, device=dev(), dtype=U8)
    return torch.where(n >= 8, n + 1, n)


def _bytes(nib):
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()


def _scales(n, k, g, lo, hi):
    """e8m0 codes of 2^lo .. 2^hi, varying per block and column"""
    return torch.randint(127 + lo, 128 + hi, (n, k // 32), generator=g, device=dev(), dtype=U8)


def _x_ints(MT, K, g):
    return torch.randint(-2, 3, (MT, 16, K), generator=g, device=dev(), dtype=torch.int8).to(BF16)


def _quant(n, k, g):
    from dflash_amd import ops
    return ops.quantize_mxfp4_rows((torch.randn(n, k, generator=g, device=dev()) * 0.05).to(BF16))


def _exact(x, deq, granule):
    """fp64 x @ deq^T, after asserting that every partial sum is a multiple of `granule` below 2^24 of them"""
    xd, wd = x.double().reshape(-1, x.shape[-1]), deq.double()
    assert float((xd.abs() @ wd.abs().T).max()) / granule < 2 ** 24
    return xd @ wd.T


# ---------------------------------------------------------------- ring form, gate/up + SiLU * up
def _silu_run(ops, wp, x, R, I, K):
    MT = ops.batch_tiles(R)
    act = torch.full((MT, 16 * I), float("nan"), dtype=BF16, device=dev())
    ops.gemm_silu_mul_batch(wp, _frag(x), R, I, K, act, ops.gemm_batch_ws(2 * I, K, dev()), H.dyn_records([(0, 16)] * MT, MT, dev()))
    return act


@pytest.mark.parametrize("R,I,K", SILU4, ids=[FC.case_id(c) for c in SILU4])
def test_ring_silu_mxfp4_equals_the_bf16_ring_on_the_dequantised_matrix(R, I, K):
    from dflash_amd import ops
    g = _gen(3 * R + I + K)
    (qg, sg), (qu, su) = _quant(I, K, g), _quant(I, K, g)
    x = torch.randn(ops.batch_tiles(R), 16, K, generator=g, device=dev()).to(BF16)
    got = _silu_run(ops, ops.pack_weight_gateup_mxfp4(qg, sg, qu, su), x, R, I, K)
    want = _silu_run(ops, ops.pack_weight_gateup(ops.dequantize_mxfp4_rows(qg, sg), ops.dequantize_mxfp4_rows(qu, su)), x, R, I, K)
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("R,I,K", SILU4[:7], ids=[FC.case_id(c) for c in SILU4[:7]])
def test_ring_silu_mxfp4_exact_ints(R, I, K):
    """All 15 e2m1 values under block scales 2^0 .. 2^3, activations in [-2, 2]: every partial sum is a multiple of 0.5
    below 2^24 of them, so the gate and up sums are exact and the output is torch's up to the SiLU's exp — the bars of
    test_ring_silu_fp8_exact_ints (the same epilogue code): at most 2 bf16 steps, at most 1e-3 of the elements off."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _gen(R + I + K)
    qg, qu = _bytes(_nibbles((I, K), g)), _bytes(_nibbles((I, K), g))
    sg, su = _scales(I, K, g, 0, 3), _scales(I, K, g, 0, 3)
    x = _x_ints(MT, K, g)
    gs = _exact(x, ops.dequantize_mxfp4_rows(qg, sg), 0.5).float()
    us = _exact(x, ops.dequantize_mxfp4_rows(qu, su), 0.5).float()
    want = _silu_ref(x, gs, us).view(MT, 16, I)
    act = _silu_run(ops, ops.pack_weight_gateup_mxfp4(qg, sg, qu, su), x, R, I, K)
    for r in range(R):
        got = H.unfrag(act[r], I)
        assert not torch.isnan(got.float()).any(), r
        d = _bf16_steps(got, want[r])
        off = float((d > 0).float().mean())
        print(f"[parity] mxfp4 ring silu R{R} I{I} K{K} r{r}: max {int(d.max())} bf16 steps, {off:.2e} off")
        assert int(d.max()) <= 2 and off <= 1e-3, (r, int(d.max()), off)


# ---------------------------------------------------------------- ring form, lm_head + argmax
def _argmax_run(ops, wp, x, R, V, K, row0, with_logits):
    MT = ops.batch_tiles(R)
    bss = LM_BS[R] + [0] * (MT - R)
    ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    logits = torch.full((MT, 16, V), 3.0, dtype=BF16, device=dev()) if with_logits else None
    ops.gemm_argmax_batch(wp, _frag(x), R, V, K, row0, 16 - row0, ops.gemm_batch_ws(V, K, dev()), ids, row0,
                          H.dyn_records([(0, b) for b in bss], MT, dev()), nrows_dyn_word=ops.DYN_BS, logits=logits)
    return ids, logits, bss


@pytest.mark.parametrize("R,V,K", ARGMAX4, ids=[FC.case_id(c) for c in ARGMAX4])
def test_ring_argmax_mxfp4_equals_the_bf16_ring_on_the_dequantised_head(R, V, K):
    from dflash_amd import ops
    g = _gen(V + K + 100 * R)
    q, sc = _quant(V, K, g)
    x = torch.randn(ops.batch_tiles(R), 16, K, generator=g, device=dev()).to(BF16)
    w4, wb = ops.pack_weight_mxfp4(q, sc), ops.pack_weight(ops.dequantize_mxfp4_rows(q, sc))
    for with_logits in (False, True):
        got, want = (_argmax_run(ops, wp, x, R, V, K, 1, with_logits) for wp in (w4, wb))
        assert torch.equal(got[0], want[0])
        assert int(got[0][0, 1:].min()) >= 0 and int(got[0].max()) < V
        if with_logits:
            assert torch.equal(got[1].view(torch.int16), want[1].view(torch.int16))


@pytest.mark.parametrize("row0", [0, 1])
@pytest.mark.parametrize("R,V,K", ARGMAX4[:4], ids=[FC.case_id(c) for c in ARGMAX4[:4]])
def test_ring_argmax_mxfp4_exact_ties(R, V, K, row0):
    """All 15 e2m1 values under block scales 2^-3 .. 2^0 (|w| <= 6, multiples of 2^-4), activations in [-2, 2]: the logits
    are bf16(fp64 sum) exactly, so the ids are the first maximum of the reference through every merge (lane, column groups,
    waves, workgroups, passes).  test_hip_fp8_batch's forced ties, each at the largest logit a column can reach, 6 sum|x|:
    6 sign(x) at scale 1, and — the tie that exists only after scaling — 3 sign(x) at scale 2.  Rows outside a tile's count
    keep the prefilled sentinel."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _gen(V + K + R)
    x = _x_ints(MT, K, g)
    nib, sc = _nibbles((V, K), g), _scales(V, K, g, -3, 0)
    pairs, rows = _forced_ties(V, x[0])
    for c, (row, s) in rows.items():   # row = mult * sign(x) with mult * s == 2
        mag = 7 if s == 1.0 else 5     # e2m1 codes of 6 and 3
        sgn = torch.sign(row.float())
        nib[c] = torch.where(sgn > 0, mag, torch.where(sgn < 0, mag | 8, 0)).to(U8)
        sc[c] = 127 if s == 1.0 else 128
    q = _bytes(nib)
    ref_bf = _exact(x, ops.dequantize_mxfp4_rows(q, sc), 2.0 ** -4).view(MT, 16, V).to(BF16)
    w4 = ops.pack_weight_mxfp4(q, sc)
    (ids0, _, bss), (ids1, logits, _) = (_argmax_run(ops, w4, x, R, V, K, row0, wl) for wl in (False, True))
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
        assert torch.equal(ids0[r, row0:row0 + n], want) and torch.equal(ids1[r, row0:row0 + n], want), r
        assert torch.equal(logits[r, row0:row0 + n], lg), r
        assert torch.all(logits[r, :row0] == 3.0) and torch.all(logits[r, row0 + n:] == 3.0), r


# ---------------------------------------------------------------- register-resident form, fp32 K parts
def _f32_run(ops, wp, x, R, N, K):
    MT, ks = ops.batch_tiles(R), ops.batch_ksplit(K)
    out = torch.full((ks, MT * 16, N), float("nan"), dtype=F32, device=dev())
    ops.gemm_f32_batch(wp, _frag(x), R, N, K, out, H.dyn_records([(0, 16)] * MT, MT, dev()))
    return out.view(ks, MT, 16, N)[:, :R]


@pytest.mark.parametrize("R,N,K", F32_4, ids=[FC.case_id(c) for c in F32_4])
def test_gemm_f32_batch_mxfp4(R, N, K):
    """Integers (all 15 values, block scales 2^0 .. 2^3): every K part is the exact sum over its own k-steps — part c the
    8 * nfr k-steps from c times that many.  Random codes: every part equals the bf16 launch on the dequantised matrix."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    f = FC.f32_form(R, N, K, w8=False)
    assert f["nfr"] % 4 == 0 and ops.mxfp4_parts_ok(K)
    g = _gen(R + N + K)
    q, sc, x = _bytes(_nibbles((N, K), g)), _scales(N, K, g, 0, 3), _x_ints(MT, K, g)
    deq = ops.dequantize_mxfp4_rows(q, sc)
    out = _f32_run(ops, ops.pack_weight_mxfp4(q, sc), x, R, N, K)
    span = 8 * f["nfr"] * 32
    for c in range(f["ksplit"]):
        k0, k1 = min(c * span, K), min((c + 1) * span, K)
        want = _exact(x[:R, :, k0:k1], deq[:, k0:k1], 0.5).view(R, 16, N)
        assert torch.equal(out[c].double(), want), c
    q, sc = _quant(N, K, g)
    x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    got = _f32_run(ops, ops.pack_weight_mxfp4(q, sc), x, R, N, K)
    assert torch.isfinite(got).all()
    assert torch.equal(got, _f32_run(ops, ops.pack_weight(ops.dequantize_mxfp4_rows(q, sc)), x, R, N, K))


# ---------------------------------------------------------------- every form inside a guarded arena
@pytest.mark.parametrize("form", ["silu", "argmax", "f32"])
def test_mxfp4_batch_forms_stay_inside_their_buffers(form):
    """Weights, activations, workspace and outputs at exactly their declared sizes between guard bands: no band is written,
    and the result does not depend on what the bands hold (guard patterns A and B)."""
    from dflash_amd import ops
    R, K = 3, 384 if form != "f32" else 1024
    N = 4208 if form == "argmax" else 272
    MT = ops.batch_tiles(R)
    g = _gen(17)
    q, sc = _quant(2 * N if form == "silu" else N, K, g)
    blob = (ops.pack_weight_gateup_mxfp4(q[:N], sc[:N], q[N:], sc[N:]) if form == "silu" else ops.pack_weight_mxfp4(q, sc)).data
    wsb = int(ops.gemm_batch_ws(2 * N, K, dev()).numel())
    plan = [("w", blob.numel(), U8), ("x", (MT, 16 * K), BF16), ("ws", wsb, U8), ("dyn", (MT, 8), torch.int32),
            ("act", (MT, 16 * N), BF16), ("ids", (MT, 16), torch.int64), ("logits", (MT, 16, N), BF16),
            ("out", (ops.batch_ksplit(K), MT * 16, N), F32)]
    ar = Arena(Arena.bytes_for([torch.Size([s] if isinstance(s, int) else s).numel() * 8 for _, s, _ in plan]), dev())
    b = {n: ar.take(n, s, d, kind="index" if d in (torch.int32, torch.int64) else "float") for n, s, d in plan}
    x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    w4 = ops.Mxfp4Weight(b["w"], 2 * N if form == "silu" else N, K)
    res = []
    for which in ("A", "B"):
        ar.fill_guards(which)
        b["w"].copy_(blob)
        b["x"].copy_(H.frag_of(x))
        b["ws"].zero_()
        b["dyn"].copy_(H.dyn_records([(0, 16)] * R + [(0, 0)] * (MT - R), MT, dev()))
        b["act"].fill_(1.0), b["ids"].fill_(-1), b["logits"].fill_(3.0), b["out"].fill_(float("nan"))
        src = ops.brows_frag(b["x"])
        if form == "silu":
            ops.gemm_silu_mul_batch(w4, src, R, N, K, b["act"], b["ws"], b["dyn"])
        elif form == "argmax":
            ops.gemm_argmax_batch(w4, src, R, N, K, 0, 16, b["ws"], b["ids"], 0, b["dyn"], nrows_dyn_word=ops.DYN_BS, logits=b["logits"])
        else:
            ops.gemm_f32_batch(w4, src, R, N, K, b["out"], b["dyn"])
        torch.cuda.synchronize()
        ar.check()
        res.append([b[n][:R].clone() if n != "out" else b[n][:, :R * 16].clone() for n in ("act", "ids", "logits", "out")])
    for a1, a2 in zip(*res):
        assert torch.equal(a1.view(torch.uint8), a2.view(torch.uint8))
    assert torch.all(b["ids"][R:] == -1) and torch.all(b["logits"][R:] == 3.0)
