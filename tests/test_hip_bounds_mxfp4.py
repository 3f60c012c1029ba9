"""Bounds of the three launches that take a DFL_W_MXFP4 weight (k_gemm_w4 of gemm_skinny.hip), each inside a guarded arena
(tests/arena.py, tests/bounds_common.py: the properties W, R and S).

The weight blob is an arena view of exactly the documented size, N * K / 2 bytes of codes and N * K / 32 bytes of block
scales: a scale request past the last (column, 128-k group) dword, or a 16-byte word read past the codes, would land in the
guard — under one pattern a NaN-free garbage scale, under the other another one — and change the result.  The shapes are
the small launch-form shapes of test_hip_bounds_gemm.py at K a multiple of 128 (256; 4224 = 33 words for the K-chunked
form, whose last chunk holds one word).  Small-integer operands (exact in e2m1 under a power-of-two block scale) make every
sum exact: the values are compared with torch bit for bit."""
import pytest
import torch

import arena as A
import bounds_common as B
import helpers as H
import test_hip_bounds_gemm as G
import test_hip_skinny_gemm as SG

gpu = pytest.mark.gpu
BF16, F32, I32, I64, U8 = B.BF16, B.F32, B.I32, B.I64, B.U8
BS = G.BS

COVERS = {
    "dfl_gemm_resid": "test_gemm_resid_mxfp4_bounds",
    "dfl_gemm_silu_mul": "test_gemm_silu_mul_mxfp4_bounds",
    "dfl_gemm_argmax": "test_gemm_argmax_mxfp4_bounds",
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def blob_bytes(N, K):
    return N * K // 2 + N * K // 32


def _quantise_exactly(ops, w):
    q = ops.quantize_mxfp4_rows(w)
    assert torch.equal(ops.dequantize_mxfp4_rows(*q), w)
    return q


# (N, K, source, add_residual, ss_out, tap, valid rows)
RESID = [
    (128, 256, "frag", True, False, False, 16),        # all halves
    (128, 256, "rows", False, False, False, 1),        # all halves, rows 1..15 of the source dead
    (4112, 256, "rows", True, False, True, 7),         # 256 whole + 1 in halves
    (2064, 256, "normed", False, False, False, 5),     # whole tiles on 129 workgroups, the norm in the prologue
    (6144, 256, "normed", True, True, True, 7),        # ss_out: two whole tiles per workgroup, + tap
    (256, 4224, "rows", True, True, True, 3),          # K-chunked: 33 words, three chunks, the last of one word
    (256, 4224, "frag", False, False, False, 16),
]


def _resid_id(c):
    N, K, kind, add, ss, tap, nv = c
    return f"N{N}-K{K}-{SG.form_id(SG.resid_plan(N, K, ss))}-{kind}-nv{nv}" + "".join(
        s for s, on in (("-add", add), ("-ss", ss), ("-tap", tap)) if on)


def test_mxfp4_bounds_cases_reach_the_forms():
    """(no GPU) the shapes reach the forms of resid_plan named above, at K % 128 == 0."""
    plans = {(N, K, bool(ss)): SG.resid_plan(N, K, ss) for N, K, _, _, ss, _, _ in RESID}
    assert plans[(128, 256, False)] == dict(gx=16, whole=0, half=8, nch=1)
    assert plans[(4112, 256, False)] == dict(gx=256, whole=256, half=1, nch=1)
    assert plans[(2064, 256, False)] == dict(gx=129, whole=129, half=0, nch=1)
    assert plans[(6144, 256, True)] == dict(gx=192, whole=384, half=0, nch=1)
    assert plans[(256, 4224, True)]["nch"] == 3 and 4224 // 32 - 2 * 64 == 4 and all(K % 128 == 0 for _, K, *_ in RESID)


@gpu
@pytest.mark.parametrize("case", RESID, ids=[_resid_id(c) for c in RESID])
def test_gemm_resid_mxfp4_bounds(ops, case):
    """dfl_gemm_resid on an Mxfp4Weight.  W: h_io columns past N, tap columns outside the slice; R: dead source rows, their
    partial sums and everything around the weight blob under both patterns; sizes exact.  Values: torch, bit for bit."""
    N, K, kind, add, want_ss, want_tap, nv = case
    ld, ldt = N + 48, N + 80
    w = B.small_ints((N, K), N + K)
    w4 = ops.pack_weight_mxfp4(*_quantise_exactly(ops, w))
    assert w4.data.numel() == blob_bytes(N, K)
    plan = ([("wp", blob_bytes(N, K), U8, "bytes")] + G._source_plan(kind, K, K // 16)
            + [("h", (16, ld), BF16), ("dyn", 8, I32, "index")]
            + ([("tap", (16, ldt), BF16)] if want_tap else []) + ([("ss_out", N, F32)] if want_ss else []))
    c = B.Case(max(K, ldt), plan)
    wt = ops.Mxfp4Weight(c.wp, N, K)
    src = G._Src(ops, c, kind, K, BS, nv, seed=N + K + nv)
    h0 = SG._distinct_resid(ld)

    def make(which):
        c.wp.copy_(w4.data)
        src.fill(which)
        G._dyn_fill(c.dyn, nv)
        c.h.copy_(h0)
        if want_tap:
            c.tap.fill_(5.0)
        if want_ss:
            c.ss_out.fill_(float("nan"))

    def launch():
        ops.gemm_resid(wt, src.src, N, K, c.h, add_residual=add, ss_out=c.ss_out if want_ss else None,
                       tap=c.tap[:, 40:40 + N] if want_tap else None, dyn=c.dyn)

    def outs():
        o = {"h": c.h}
        if want_tap:
            o["tap"] = c.tap
        if want_ss:
            o["ss_out"] = c.ss_out
        return o
    res = c.run(make, launch, outs)
    lin = (src.xs @ w.float().T).to(BF16)
    want = (h0[:, :N].float() + lin.float()).to(BF16) if add else lin
    assert torch.equal(res["h"][:, :N], want) and torch.equal(res["h"][:, N:], h0[:, N:])
    if want_tap:
        assert torch.equal(res["tap"][:, 40:40 + N], want)
        assert torch.all(res["tap"][:, :40] == 5.0) and torch.all(res["tap"][:, 40 + N:] == 5.0)
    if want_ss:
        torch.testing.assert_close(res["ss_out"], SG._ss_ref(want), rtol=2e-6, atol=0)


# (I, K, source, valid rows): an uneven last workgroup (257 pairs on 129 workgroups), one pair per workgroup
SILU = [(4112, 256, "normed", 11), (128, 256, "rows", 1), (528, 256, "frag", 16)]


@gpu
@pytest.mark.parametrize("I,K,kind,nv", SILU, ids=[f"I{I}-K{K}-{k}-nv{nv}" for I, K, k, nv in SILU])
def test_gemm_silu_mul_mxfp4_bounds(ops, I, K, kind, nv):
    """dfl_gemm_silu_mul on an Mxfp4Weight in gate/up tile order: the blob at exactly 2 I K / 2 + 2 I K / 32 bytes, the
    frag16 output at exactly 16 * I elements."""
    g = B.cuda_gen(I + K)
    up = torch.randint(-2, 3, (I, K), generator=g, device=B.dev(), dtype=torch.int8).to(BF16)
    gate = torch.randint(-2, 3, (I, K), generator=g, device=B.dev(), dtype=torch.int8).to(BF16) * 2 ** -6
    w4 = ops.pack_weight_gateup_mxfp4(*_quantise_exactly(ops, gate), *_quantise_exactly(ops, up))
    assert w4.data.numel() == blob_bytes(2 * I, K)
    c = B.Case(max(K, I), [("wp", blob_bytes(2 * I, K), U8, "bytes")] + G._source_plan(kind, K, K // 16)
               + [("act", 16 * I, BF16), ("dyn", 8, I32, "index")])
    wt = ops.Mxfp4Weight(c.wp, 2 * I, K)
    src = G._Src(ops, c, kind, K, BS, nv, seed=I + K + nv)

    def make(which):
        c.wp.copy_(w4.data)
        src.fill(which)
        G._dyn_fill(c.dyn, nv)
        c.act.fill_(float("nan"))
    res = c.run(make, lambda: ops.gemm_silu_mul(wt, src.src, I, K, c.act, c.dyn), lambda: {"act": c.act})
    got, want = H.unfrag(res["act"], I), SG._silu_ref(src.xs, gate, up)
    d = SG._bf16_ulps(got, want)
    assert int(d.max()) <= 2 and float((d > 0).float().mean()) <= 1e-3          # the bar of test_gemm_silu_mul_exact
    assert torch.count_nonzero(got[nv:].float()) == 0


# (V, K, source, row0, valid rows): 256 whole tiles + 1 in halves, 256 workgroups of two tiles, all halves
ARG = [(4112, 256, "normed", 0, 11), (8192, 256, "rows", 1, 9), (528, 256, "frag", 1, 13)]


@gpu
@pytest.mark.parametrize("V,K,kind,row0,nv", ARG, ids=[f"V{V}-K{K}-{k}-row{r}-nv{nv}" for V, K, k, r, nv in ARG])
def test_gemm_argmax_mxfp4_bounds(ops, V, K, kind, row0, nv):
    """dfl_gemm_argmax on an Mxfp4Weight: the workspace at exactly dfl_argmax_ws_bytes() and holding the pattern, row0 > 0
    with the row count from the record, the logits at exactly [16][V], ids / margins outside their range untouched.
    S: the same ids, margins and logits on a four times larger workspace."""
    w = B.small_ints((V, K), V + K)
    w4 = ops.pack_weight_mxfp4(*_quantise_exactly(ops, w))
    off = 3
    c = B.Case(max(K, V), [("wp", blob_bytes(V, K), U8, "bytes")] + G._source_plan(kind, K, K // 16)
               + [("ws", ops.lib().dfl_argmax_ws_bytes(), U8, "bytes"), ("ids", 24, I64, "index"), ("mg", 24, F32),
                  ("logits", (16, V), BF16), ("dyn", 8, I32, "index")])
    wt = ops.Mxfp4Weight(c.wp, V, K)
    src = G._Src(ops, c, kind, K, BS, nv, seed=V + K + nv)

    def make(which):
        c.wp.copy_(w4.data)
        src.fill(which)
        G._dyn_fill(c.dyn, nv)
        A.poison(c.ws, slice(None), which, kind="bytes")      # ws needs no zeroing: whatever it holds must not matter
        c.ids.fill_(-7)
        c.mg.fill_(-7.0)
        c.logits.fill_(3.0)

    def launch_with(ws):
        ops.gemm_argmax(wt, src.src, V, K, row0, 16 - row0, ws, c.ids, off, dyn=c.dyn, nrows_dyn_word=BS, logits=c.logits,
                        margins=c.mg)
    outs = lambda: {"ids": c.ids, "mg": c.mg, "logits": c.logits}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    n = nv - row0
    ref = (src.xs @ w.float().T).to(BF16)
    assert torch.equal(res["logits"][row0:nv], ref[row0:nv])
    assert torch.all(res["logits"][:row0] == 3.0) and torch.all(res["logits"][nv:] == 3.0)
    assert torch.all(res["ids"][:off] == -7) and torch.all(res["ids"][off + n:] == -7)
    assert torch.all(res["mg"][:off] == -7) and torch.all(res["mg"][off + n:] == -7)
    assert torch.equal(res["ids"][off:off + n], B.first_argmax(ref[row0:nv].float()))
    top2 = ref[row0:nv].float().topk(2, dim=-1).values
    assert torch.equal(res["mg"][off:off + n], top2[:, 0] - top2[:, 1])
