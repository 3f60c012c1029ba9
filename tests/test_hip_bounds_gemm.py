"""Bounds of the single-request GEMM launches (gemm_skinny.hip, gemm_rows.h) and the one-time packers, each inside a
guarded arena (tests/arena.py, tests/bounds_common.py: the properties W, R and S).

Every buffer is an arena view of exactly the size the header states: the packed weight at the packer's output size, the
e4m3 scale vector at N floats, the mode-2 partial sums at nss * 16 floats, the fp32 output of dfl_gemm_f32 at
[ksplit][mt * 16][N], the argmax workspace at dfl_argmax_ws_bytes().  Rows at or past the valid count of a plain or
normalised source (and their partial sums) carry the guard pattern: NaN in one run, 1.0 in the other.

Shapes are the smallest that reach each launch form of plan_tiles / resid_plan / silu_plan / grid_x_for
(test_hip_skinny_gemm.py holds those host rules; the forms depend on tile and k-step counts only, so K = 256 does).
Small-integer operands make every sum exact: the values are compared with torch bit for bit."""
import pytest
import torch

import arena as A
import bounds_common as B
import helpers as H
import test_hip_skinny_gemm as SG

gpu = pytest.mark.gpu
BF16, F32, I32, I64, U8 = B.BF16, B.F32, B.I32, B.I64, B.U8
TAU, BS = 1, 2

COVERS = {
    "dfl_gemm_resid": "test_gemm_resid_bounds",
    "dfl_gemm_f32": "test_gemm_f32_bounds",
    "dfl_gemm_silu_mul": "test_gemm_silu_mul_bounds",
    "dfl_gemm_argmax": "test_gemm_argmax_sample_bounds",
    "dfl_gemm_sample": "test_gemm_argmax_sample_bounds",
    "dfl_pack_weight": "test_packers_bounds",
    "dfl_pack_weight_gateup": "test_packers_bounds",
    "dfl_pack_weight_fp8": "test_packers_bounds",
    "dfl_pack_weight_gateup_fp8": "test_packers_bounds",
    "dfl_pack_rows": "test_pack_rows_and_records_bounds",
    "dfl_set_dyn": "test_pack_rows_and_records_bounds",
    "dfl_set_dyn2": "test_pack_rows_and_records_bounds",
    "dfl_embed_rows": "test_embed_rows_bounds",
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


# ---------------------------------------------------------------- operands inside the arena
def _weight_plan(fmt, N, K, x13_bytes=0):
    if fmt == "bf16":
        return [("wp", N * K, BF16)]
    if fmt == "e4m3":
        return [("wp", N * K, U8, "bytes"), ("wscale", N, F32)]
    return [("wp", x13_bytes, U8, "bytes")]


def _weight(ops, c, fmt, wp_bf16, w, N, K):
    """Fill the case's weight views from the packed bf16 weight `wp_bf16` of `w` and return what the wrappers take.  The
    e4m3 codes of small integers with a power-of-two scale dequantise to the same integers."""
    if fmt == "bf16":
        c.wp.copy_(wp_bf16)
        return c.wp
    if fmt == "x13":
        c.wp.copy_(c.x13.data)
        return ops.Bf16x13Weight(c.wp, N, K)
    c.wp.copy_(c.w8.wp)
    c.wscale.copy_(c.w8.scale)
    return ops.Fp8Weight(c.wp, c.wscale, N, K)


def _prepack(ops, fmt, wp_bf16, w, N, K, gateup=None):
    """(the x13 / e4m3 forms packed outside the arena once, and the byte size the arena view must have)"""
    ns = type("P", (), {})()
    ns.x13 = ns.w8 = None
    nb = 0
    if fmt == "x13":
        ns.x13, report = ops.pack_weight_bf16x13(wp_bf16, N, K)
        assert ns.x13 is not None, report
        nb = ns.x13.data.numel()
        assert nb == (N // 16) * (K // 128) * 3328 + (N // 16) * (16 if K <= 4096 else K // 128) * 8     # quads, then the meta pairs
    elif fmt == "e4m3":
        if gateup is None:
            q, s = ops.quantize_fp8_rows(w)
            ns.w8 = ops.pack_weight_fp8(q, s)
            assert torch.equal(ops.dequantize_fp8_rows(q, s), w)
        else:
            (gq, gs), (uq, us) = ops.quantize_fp8_rows(gateup[0]), ops.quantize_fp8_rows(gateup[1])
            ns.w8 = ops.pack_weight_gateup_fp8(gq, gs, uq, us)
    return ns, nb


def _source_plan(kind, K, nss):
    if kind == "frag":
        return [("xf", 16 * K, BF16)]
    if kind == "rows":
        return [("xr", (16, K), BF16)]
    return [("xr", (16, K), BF16), ("ss", nss * 16, F32), ("nw", K, BF16)]


class _Src:
    """A row source in arena views: frag16 at exactly 16 * K elements, plain rows at exactly 16 rows, the mode-2 partial
    sums at exactly nss * 16 floats.  fill(which) rewrites them; rows at or past nv hold the pattern."""

    def __init__(self, ops, c, kind, K, vw, nv, seed, nss=None):
        self.c, self.kind, self.nv = c, kind, nv
        nss = nss or K // 16
        if kind == "normed":
            self.h, self.ssv, self.nwv, xn = SG._normed(K, seed, nss)
            self.xs = xn.float().clone()
            self.src = ops.rows_normed(c.xr, c.ss, nss, c.nw, 0.0, vw)
        else:
            self.x = B.small_ints((16, K), seed)
            self.xs = self.x.float().clone()
            self.src = ops.rows_frag(c.xf) if kind == "frag" else ops.rows_plain(c.xr, vw)
        if kind != "frag":
            self.xs[nv:] = 0

    def fill(self, which):
        c, nv = self.c, self.nv
        if self.kind == "frag":
            c.xf.copy_(B.frag16(self.x))
            return
        c.xr.copy_(self.h if self.kind == "normed" else self.x)
        A.poison(c.xr, (slice(nv, None), slice(None)), which)
        if self.kind == "normed":
            c.ss.copy_(self.ssv)
            c.nw.copy_(self.nwv)
            A.poison(c.ss.view(-1, 16), (slice(None), slice(nv, None)), which)       # slot j * 16 + m of a dead row m


def _dyn_fill(d, nv):
    d.zero_()
    d[TAU] = nv
    d[BS] = nv


# ---------------------------------------------------------------- dfl_gemm_resid
# (N, K, source, format, add_residual, ss_out, tap, valid rows): the forms of resid_plan, the three sources, the formats
RESID = [
    (128, 256, "frag", "bf16", True, False, False, 16),        # all halves
    (128, 256, "rows", "e4m3", False, False, False, 1),        # all halves, rows 1..15 of the source dead
    (4112, 256, "rows", "bf16", True, False, True, 7),         # 256 whole + 1 in halves
    (2064, 256, "normed", "bf16", False, False, False, 5),     # whole tiles on 129 workgroups, the norm in the prologue
    (6144, 256, "normed", "bf16", True, True, True, 7),        # ss_out: two whole tiles per workgroup, + tap
    (6144, 256, "frag", "e4m3", True, True, False, 16),
    (256, 4160, "rows", "bf16", True, True, True, 3),          # K-chunked: 130 k-steps, three chunks, the last of 2
    (256, 4160, "frag", "bf16", False, False, False, 16),
    (128, 6144, "frag", "x13", True, True, True, 16),          # the 13-bit K-chunked form (three whole chunks)
    (128, 6144, "rows", "x13", False, False, False, 9),
]


def _resid_id(c):
    N, K, kind, fmt, add, ss, tap, nv = c
    p = SG.resid_plan(N, K, ss)
    return f"N{N}-K{K}-{SG.form_id(p)}-{kind}-{fmt}-nv{nv}" + "".join(
        s for s, on in (("-add", add), ("-ss", ss), ("-tap", tap)) if on)


def test_resid_bounds_cases_reach_the_forms():
    """(no GPU) the shapes above reach every form of resid_plan the issue of this test names."""
    plans = {(N, K, bool(ss)): SG.resid_plan(N, K, ss) for N, K, _, _, _, ss, _, _ in RESID}
    assert plans[(128, 256, False)] == dict(gx=16, whole=0, half=8, nch=1)
    assert plans[(4112, 256, False)] == dict(gx=256, whole=256, half=1, nch=1)
    assert plans[(2064, 256, False)] == dict(gx=129, whole=129, half=0, nch=1)
    assert plans[(6144, 256, True)] == dict(gx=192, whole=384, half=0, nch=1)
    assert plans[(256, 4160, True)]["nch"] == 3 and 4160 // 32 - 2 * 64 == 2
    assert plans[(128, 6144, True)]["nch"] == 3 and {k for _, _, k, *_ in RESID} == {"frag", "rows", "normed"}


@gpu
@pytest.mark.parametrize("case", RESID, ids=[_resid_id(c) for c in RESID])
def test_gemm_resid_bounds(ops, case):
    """dfl_gemm_resid.  W: h_io columns past N, tap columns outside the slice and (without a residual) nothing but zeros in
    dead rows; R: dead source rows and their partial sums under both patterns; sizes exact.  Values: torch, bit for bit."""
    N, K, kind, fmt, add, want_ss, want_tap, nv = case
    ld, ldt = N + 48, N + 80
    w = B.small_ints((N, K), N + K)
    wp0 = ops.pack_weight(w)
    pre, nb = _prepack(ops, fmt, wp0, w, N, K)
    plan = (_weight_plan(fmt, N, K, nb) + _source_plan(kind, K, K // 16) + [("h", (16, ld), BF16), ("dyn", 8, I32, "index")]
            + ([("tap", (16, ldt), BF16)] if want_tap else []) + ([("ss_out", N, F32)] if want_ss else []))
    c = B.Case(max(K, ldt), plan)
    c.x13, c.w8 = pre.x13, pre.w8
    wt = _weight(ops, c, fmt, wp0, w, N, K)
    src = _Src(ops, c, kind, K, BS, nv, seed=N + K + nv)
    h0 = SG._distinct_resid(ld)

    def make(which):
        _weight(ops, c, fmt, wp0, w, N, K)
        src.fill(which)
        _dyn_fill(c.dyn, nv)
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


# ---------------------------------------------------------------- dfl_gemm_f32
# (N, K, mt, ksplit, sources): ksplit at pick_ksplit_min and above; the output exactly [ksplit][mt * 16][N]
F32C = [(2064, 256, 1, 1, ("rows",)), (2064, 256, 1, 2, ("normed",)), (128, 256, 2, 1, ("frag", "rows")),
        (256, 4160, 2, 3, ("rows", "frag")), (256, 4160, 1, 2, ("frag",)), (256, 4160, 2, 4, ("frag", "rows"))]


@gpu
@pytest.mark.parametrize("N,K,mt,ksplit,kinds", F32C,
                         ids=[f"N{N}-K{K}-mt{mt}-ks{ks}-{'+'.join(k)}" for N, K, mt, ks, k in F32C])
def test_gemm_f32_bounds(ops, N, K, mt, ksplit, kinds):
    """dfl_gemm_f32: the fp32 partial sums of every K part, the output sized exactly ksplit * mt * 16 * N floats.  The parts
    sum to torch's exact product; rows past the count are zero in every part."""
    assert ksplit >= ops.min_ksplit(K, mt)
    w = B.small_ints((N, K), N + K + mt)
    wp0 = ops.pack_weight(w)
    nv = 7
    plans = [("wp", N * K, BF16), ("out", (ksplit, mt * 16, N), F32), ("dyn", 8, I32, "index")]
    for i, kind in enumerate(kinds):
        plans += [(f"{n}{i}",) + tuple(rest) for n, *rest in _source_plan(kind, K, K // 16)]
    c = B.Case(max(K, N), plans)
    srcs = []
    for i, kind in enumerate(kinds):
        v = type("V", (), {})()
        for n in ("xf", "xr", "ss", "nw"):
            if hasattr(c, f"{n}{i}"):
                setattr(v, n, getattr(c, f"{n}{i}"))
        srcs.append(_Src(ops, v, kind, K, BS, nv, seed=N + 3 * i + ksplit))

    def make(which):
        c.wp.copy_(wp0)
        for s in srcs:
            s.fill(which)
        _dyn_fill(c.dyn, nv)
        c.out.fill_(float("nan"))

    def launch():
        ops.gemm_f32(c.wp, srcs[0].src, srcs[1].src if mt == 2 else None, mt, N, K, ksplit, c.out, c.dyn)
    res = c.run(make, launch, lambda: {"out": c.out})
    for i, s in enumerate(srcs):
        assert torch.equal(res["out"][:, 16 * i:16 * i + 16].sum(0), s.xs @ w.float().T), (i, kinds[i])
        if kinds[i] != "frag":
            assert torch.count_nonzero(res["out"][:, 16 * i + nv:16 * i + 16]) == 0


# ---------------------------------------------------------------- dfl_gemm_silu_mul
# (I, K, source, format, valid rows): an uneven last workgroup (257 pairs on 129 workgroups: the last walks one), one
# pair per workgroup, and the 13-bit UNC launch at the smallest K the layout covers
SILU = [(4112, 256, "normed", "bf16", 11), (4112, 256, "frag", "e4m3", 16), (128, 256, "rows", "bf16", 1),
        (528, 2048, "frag", "x13", 16), (528, 2048, "normed", "x13", 11), (64, 2048, "rows", "x13", 3)]


def test_silu_bounds_cases_reach_the_forms():
    p = SG.silu_plan(4112)
    assert p == dict(gx=129, npairs=257, per_wg=2) and 257 % 129 != 0       # I / 16 = 203 k + r generalised: uneven
    assert SG.silu_plan(128)["per_wg"] == 1 and SG.silu_plan(528) == dict(gx=33, npairs=33, per_wg=1)


@gpu
@pytest.mark.parametrize("I,K,kind,fmt,nv", SILU, ids=[f"I{I}-K{K}-{k}-{f}-nv{nv}" for I, K, k, f, nv in SILU])
def test_gemm_silu_mul_bounds(ops, I, K, kind, fmt, nv):
    """dfl_gemm_silu_mul: the frag16 output at exactly 16 * I elements.  The 13-bit cases run k_gemm_w13<EPI_SILU, *>'s UNC
    item loop, whose request past the last item must read nothing that reaches the result."""
    g = B.cuda_gen(I + K)
    up = torch.randint(-2, 3, (I, K), generator=g, device=B.dev(), dtype=torch.int8).to(BF16)
    gate = torch.randint(-2, 3, (I, K), generator=g, device=B.dev(), dtype=torch.int8).to(BF16) * 2 ** -6
    wp0 = ops.pack_weight_gateup(gate, up)
    pre, nb = _prepack(ops, fmt, wp0, None, 2 * I, K, gateup=(gate, up))
    c = B.Case(max(K, I), _weight_plan(fmt, 2 * I, K, nb) + _source_plan(kind, K, K // 16)
               + [("act", 16 * I, BF16), ("dyn", 8, I32, "index")])
    c.x13, c.w8 = pre.x13, pre.w8
    wt = _weight(ops, c, fmt, wp0, None, 2 * I, K)
    src = _Src(ops, c, kind, K, BS, nv, seed=I + K + nv)

    def make(which):
        _weight(ops, c, fmt, wp0, None, 2 * I, K)
        src.fill(which)
        _dyn_fill(c.dyn, nv)
        c.act.fill_(float("nan"))
    res = c.run(make, lambda: ops.gemm_silu_mul(wt, src.src, I, K, c.act, c.dyn), lambda: {"act": c.act})
    got, want = H.unfrag(res["act"], I), SG._silu_ref(src.xs, gate, up)
    d = SG._bf16_ulps(got, want)
    assert int(d.max()) <= 2 and float((d > 0).float().mean()) <= 1e-3          # the bar of test_gemm_silu_mul_exact
    assert torch.count_nonzero(got[nv:].float()) == 0


# ---------------------------------------------------------------- dfl_gemm_argmax / dfl_gemm_sample
# (V, K, source, format, row0, valid rows): V = 4112 (256 whole tiles + 1 in halves), 8192 (256 workgroups of two tiles),
# 528 at K = 2048 for the 13-bit form (all halves)
ARG = [(4112, 256, "normed", "bf16", 0, 11), (4112, 256, "frag", "e4m3", 1, 16), (8192, 256, "rows", "bf16", 1, 9),
       (528, 2048, "frag", "x13", 1, 13)]


ARG_RUNS = [c + (s,) for c in ARG for s in (False, True) if not (s and c[3] == "x13")]   # dfl_gemm_sample takes no 13-bit weight


@gpu
@pytest.mark.parametrize("V,K,kind,fmt,row0,nv,sample", ARG_RUNS,
                         ids=[f"{'sample' if s else 'argmax'}-V{V}-K{K}-{k}-{f}-row{r}-nv{nv}" for V, K, k, f, r, nv, s in ARG_RUNS])
def test_gemm_argmax_sample_bounds(ops, V, K, kind, fmt, row0, nv, sample):
    """dfl_gemm_argmax and dfl_gemm_sample: the workspace at exactly dfl_argmax_ws_bytes(), row0 > 0 with the row count
    from the record, the logits buffer at exactly [16][V] (the single-request form has no logits stride; the batch form,
    test_hip_bounds_batch.py, has), ids / margins outside [out_off, out_off + rows) untouched, a workspace that is NOT
    zeroed (the header asks for none: it holds the pattern).
    S: the same ids, margins and logits on a four times larger workspace."""
    w = B.small_ints((V, K), V + K)
    wp0 = ops.pack_weight(w)
    pre, nb = _prepack(ops, fmt, wp0, w, V, K)
    off = 3
    c = B.Case(max(K, V), _weight_plan(fmt, V, K, nb) + _source_plan(kind, K, K // 16)
               + [("ws", ops.lib().dfl_argmax_ws_bytes(), U8, "bytes"), ("ids", 24, I64, "index"), ("mg", 24, F32),
                  ("logits", (16, V), BF16), ("dyn", 8, I32, "index")])
    c.x13, c.w8 = pre.x13, pre.w8
    wt = _weight(ops, c, fmt, wp0, w, V, K)
    src = _Src(ops, c, kind, K, BS, nv, seed=V + K + nv)

    def make(which):
        _weight(ops, c, fmt, wp0, w, V, K)
        src.fill(which)
        _dyn_fill(c.dyn, nv)
        A.poison(c.ws, slice(None), which, kind="bytes")      # ws needs no zeroing: whatever it holds must not matter
        c.ids.fill_(-7)
        c.mg.fill_(-7.0)
        c.logits.fill_(3.0)

    def launch_with(ws):
        kw = dict(dyn=c.dyn, nrows_dyn_word=BS, logits=c.logits, margins=c.mg)
        if sample:
            ops.gemm_sample(wt, src.src, V, K, row0, 16 - row0, ws, c.ids, off, seed=5, temperature=0.7, pos_base=11, **kw)
        else:
            ops.gemm_argmax(wt, src.src, V, K, row0, 16 - row0, ws, c.ids, off, **kw)
    outs = lambda: {"ids": c.ids, "mg": c.mg, "logits": c.logits}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    n = nv - row0
    ref = (src.xs @ w.float().T).to(BF16)
    assert torch.equal(res["logits"][row0:nv], ref[row0:nv])
    assert torch.all(res["logits"][:row0] == 3.0) and torch.all(res["logits"][nv:] == 3.0)
    assert torch.all(res["ids"][:off] == -7) and torch.all(res["ids"][off + n:] == -7)
    assert torch.all(res["mg"][:off] == -7) and torch.all(res["mg"][off + n:] == -7)
    ids = res["ids"][off:off + n]
    assert int(ids.min()) >= 0 and int(ids.max()) < V
    if not sample:
        assert torch.equal(ids, B.first_argmax(ref[row0:nv].float()))
        top2 = ref[row0:nv].float().topk(2, dim=-1).values
        assert torch.equal(res["mg"][off:off + n], top2[:, 0] - top2[:, 1])


# ---------------------------------------------------------------- the packers
@gpu
@pytest.mark.parametrize("N,K", [(16, 64), (4112, 256)], ids=lambda v: str(v))
def test_packers_bounds(ops, N, K):
    """dfl_pack_weight / _gateup / _fp8 / _gateup_fp8 as launches of their own: sources of exactly N * K elements, outputs of
    exactly the packed size.  The grid-stride loop of 2048 x 256 threads over N / 16 * K / 32 * 64 words must stop at the
    last word (N = 16, K = 64: 128 words for half a million threads).  Values: the packed layout by plain indexing."""
    lib, st = ops.lib(), torch.cuda.current_stream().cuda_stream
    w, u = B.small_ints((N, K), N + K, -100, 100), B.small_ints((N, K), N + K + 1, -100, 100)
    q = torch.randint(0, 256, (N, K), generator=B.cuda_gen(N), device=B.dev(), dtype=torch.int32).to(U8)
    q2 = torch.randint(0, 256, (N, K), generator=B.cuda_gen(N + 1), device=B.dev(), dtype=torch.int32).to(U8)
    c = B.Case(K, [("w", (N, K), BF16), ("u", (N, K), BF16), ("wp", N * K, BF16), ("wgu", 2 * N * K, BF16),
                   ("q", (N, K), U8, "bytes"), ("q2", (N, K), U8, "bytes"), ("wp8", N * K, U8, "bytes"),
                   ("wgu8", 2 * N * K, U8, "bytes")])

    def make(which):
        c.w.copy_(w), c.u.copy_(u), c.q.copy_(q), c.q2.copy_(q2)
        c.wp.fill_(float("nan")), c.wgu.fill_(float("nan")), c.wp8.fill_(0x7F), c.wgu8.fill_(0x7F)

    def launch():
        p = lambda t: t.data_ptr()      # noqa: E731
        ops.check(lib.dfl_pack_weight(p(c.w), p(c.wp), N, K, st), "dfl_pack_weight")
        ops.check(lib.dfl_pack_weight_gateup(p(c.w), p(c.u), p(c.wgu), N, K, st), "dfl_pack_weight_gateup")
        ops.check(lib.dfl_pack_weight_fp8(p(c.q), p(c.wp8), N, K, st), "dfl_pack_weight_fp8")
        ops.check(lib.dfl_pack_weight_gateup_fp8(p(c.q), p(c.q2), p(c.wgu8), N, K, st), "dfl_pack_weight_gateup_fp8")
    res = c.run(make, launch, lambda: {"wp": c.wp, "wgu": c.wgu, "wp8": c.wp8, "wgu8": c.wgu8})

    def packed(x):       # [N][K] -> [N/16][K/32][64 lanes][8]: lane l = column l & 15, k group l >> 4
        return x.view(N // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(N // 16, -1)

    def packed8(x):      # [N][K] codes -> [N/16][K/64][64 lanes][16 B]: bytes 0-7 of k = 64 j + 8 kq, 8-15 of 32 further
        return x.view(N // 16, 16, K // 64, 2, 4, 8).permute(0, 2, 4, 1, 3, 5).reshape(N // 16, -1)
    assert torch.equal(res["wp"].view(N // 16, -1), packed(w))
    assert torch.equal(res["wgu"].view(N // 16, 2, -1), torch.stack([packed(w), packed(u)], dim=1))
    assert torch.equal(res["wp8"].view(N // 16, -1), packed8(q))
    assert torch.equal(res["wgu8"].view(N // 16, 2, -1), torch.stack([packed8(q), packed8(q2)], dim=1))


# ---------------------------------------------------------------- dfl_pack_rows, dfl_set_dyn, dfl_set_dyn2
@gpu
def test_pack_rows_and_records_bounds(ops):
    """dfl_pack_rows from 5 rows of a 16-row buffer with a stride above K (rows past the count: the pattern, their
    fragments zero), into exactly 16 * K elements; dfl_set_dyn / dfl_set_dyn2 into exactly 8 / 16 words."""
    K, ld, nv = 96, 104, 5
    x = B.small_ints((16, ld), 9, -50, 50)
    c = B.Case(ld, [("x", (16, ld), BF16), ("xf", 16 * K, BF16), ("dyn", 8, I32, "index"), ("d1", 8, I32, "index"),
                    ("d2", 16, I32, "index")])

    def make(which):
        c.x.copy_(x)
        A.poison(c.x, [(slice(nv, None), slice(None)), (slice(None), slice(K, None))], which)
        c.dyn.zero_()
        c.dyn[TAU] = nv
        c.xf.fill_(float("nan"))
        c.d1.fill_(-9), c.d2.fill_(-9)

    def launch():
        ops.pack_rows(c.x[:, :K], 16, c.xf, c.dyn, TAU)
        ops.set_dyn(c.d1, 100, 3, 16, 97)
        ops.set_dyn2(c.d2, 100, 20, 27, 80)
    res = c.run(make, launch, lambda: {"xf": c.xf, "d1": c.d1, "d2": c.d2})
    want = x[:, :K].clone()
    want[nv:] = 0
    assert torch.equal(H.unfrag(res["xf"], K), want)
    assert res["d1"].tolist() == [100, 3, 16, 97, 100, 0, 0, 0]
    assert res["d2"].tolist() == [100, 16, 16, 80, 100, 0, 0, 0, 100, 4, 11, 80, 100, 0, 0, 0]


@gpu
def test_embed_rows_bounds(ops):
    """dfl_embed_rows: the table at exactly [V][H] with the last row in use, ids past the count holding the pattern
    (0 / 1: valid rows, never a wild address), h_out rows past the count untouched, ss_out at exactly 16 floats."""
    V, Hd, nv = 40, 72, 6
    emb = B.small_ints((V, Hd), 4, -9, 9)
    ids = torch.tensor([V - 1, 0, 17, V - 1, 3, 22] + [5] * 10, device=B.dev())
    c = B.Case(Hd, [("emb", (V, Hd), BF16), ("ids", 16, I64, "index"), ("h", (16, Hd), BF16), ("ss", 16, F32),
                    ("dyn", 8, I32, "index")])

    def make(which):
        c.emb.copy_(emb)
        c.ids.copy_(ids)
        A.poison(c.ids, slice(nv, None), which)
        c.dyn.zero_()
        c.dyn[TAU] = nv
        c.h.fill_(-3.0)
        c.ss.fill_(float("nan"))
    res = c.run(make, lambda: ops.embed_rows(c.emb, c.ids, c.h, Hd, c.ss, c.dyn, TAU), lambda: {"h": c.h, "ss": c.ss})
    assert torch.equal(res["h"][:nv], emb[ids[:nv]]) and torch.all(res["h"][nv:] == -3.0)
    want_ss = torch.zeros(16, device=B.dev())
    want_ss[:nv] = emb[ids[:nv]].float().pow(2).sum(1)
    assert torch.equal(res["ss"], want_ss)
