"""Bounds of the ragged-batch launches (gemm_batch.hip, gemm_ring.h, the batch row kernels) inside a guarded arena
(tests/arena.py, tests/bounds_common.py: W, R, S).

Both implementations of each fused GEMM run: the ring form (frag16 sources) and k_gemm_b (plain-row sources), at R = 1, 3
(one compiled tile is empty) and 4, with dfl_batch_ksplit(K) of 1 (K = 256) and 2 (K = 2048 + 64).  Every buffer holds
exactly dfl_batch_tiles(R) requests; the unused request tiles hold the guard pattern and their length records stay zero,
as the header requires.  `ws` is an arena view of exactly dfl_gemm_batch_ws_bytes(N, K): its 1 KiB of tickets zeroed, the
candidates and slabs behind them filled with the pattern (the header asks for zeroed tickets only).  Small-integer
operands: the values are compared with torch exactly."""
import pytest
import torch

import arena as A
import bounds_common as B
import helpers as H
import test_hip_batch_kernels as BK
import test_hip_skinny_gemm as SG

gpu = pytest.mark.gpu
BF16, F32, I32, I64, U8 = B.BF16, B.F32, B.I32, B.I64, B.U8
TAU, BS, POS0 = 1, 2, 3
WS_TICKETS = 1024                     # gemm_batch.hip: 256 arrival tickets in front of the workspace

COVERS = {
    "dfl_gemm_f32_batch": "test_gemm_f32_batch_bounds",
    "dfl_gemm_resid_batch": "test_gemm_resid_batch_bounds",
    "dfl_gemm_silu_mul_batch": "test_gemm_silu_mul_batch_bounds",
    "dfl_gemm_argmax_batch": "test_gemm_argmax_sample_batch_bounds",
    "dfl_gemm_sample_batch": "test_gemm_argmax_sample_batch_bounds",
    "dfl_norm_frag_batch": "test_norm_frag_batch_bounds",
    "dfl_embed_rows_batch": "test_embed_rows_batch_bounds",
    "dfl_kv_append_batch": "test_kv_append_batch_bounds",
}

# (R, K): K = 2112 is 66 k-steps in two parts of 40 + 26
RK = [(1, 256), (3, 256), (4, 2112), (3, 2112)]
BSS = {1: [16], 3: [16, 5, 1], 4: [16, 9, 1, 13]}        # valid rows per request of a plain-row source / live rows


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def test_batch_bounds_cases_reach_both_k_splits():
    """(no GPU: host code of the library) dfl_batch_ksplit gives the two K of the cases 1 and 2 parts, dfl_batch_tiles
    compiles R = 1 as 2 tiles and R = 3 as 4, and the workspace formula is WS_HEAD plus the K-part slabs."""
    from dflash_amd import ops
    L = ops.lib()
    assert [L.dfl_batch_ksplit(K) for _, K in RK] == [1, 1, 2, 2] and 2112 % 64 == 0
    assert [L.dfl_batch_tiles(R) for R in (1, 2, 3, 4)] == [2, 2, 4, 4]
    head = WS_TICKETS + 256 * 16 * 4 * 16 * 8
    assert L.dfl_gemm_batch_ws_bytes(272, 2112) == head + 2 * 17 * 4 * 256 * 4
    assert L.dfl_gemm_batch_ws_bytes(272, 256) == head + 1 * 17 * 4 * 256 * 4


class _BSrc:
    """Request tiles in arena views: frag [MT][16 K] (all 16 rows of a live request valid) or rows [MT][16][K] with the
    valid count in the BS word.  Unused tiles and dead rows hold the pattern."""

    def __init__(self, ops, c, kind, R, MT, K, seed):
        self.c, self.kind, self.R, self.MT = c, kind, R, MT
        self.x = B.small_ints((MT, 16, K), seed)
        self.nv = [16] * R if kind == "frag" else BSS[R]
        self.xs = self.x.float().clone()
        for r in range(R):
            self.xs[r, self.nv[r]:] = 0
        self.src = ops.brows_frag(c.xf) if kind == "frag" else ops.brows_plain(c.xr, BS)

    @staticmethod
    def plan(kind, MT, K):
        return [("xf", (MT, 16 * K), BF16)] if kind == "frag" else [("xr", (MT, 16, K), BF16)]

    def fill(self, which):
        c = self.c
        if self.kind == "frag":
            for r in range(self.R):
                c.xf[r].copy_(B.frag16(self.x[r]))
            A.poison(c.xf, slice(self.R, None), which)
        else:
            c.xr.copy_(self.x)
            for r in range(self.R):
                A.poison(c.xr, (r, slice(self.nv[r], None)), which)
            A.poison(c.xr, slice(self.R, None), which)
        c.dyn.zero_()
        for r in range(self.R):
            c.dyn[r, BS] = self.nv[r]
            c.dyn[r, TAU] = self.nv[r]


def _w8_plan(N, K):
    """An e4m3 weight in arena views: the codes at exactly N * K bytes, the scale vector at exactly N floats (256-byte
    aligned, so the 64-byte alignment the batch forms ask of it holds)."""
    return [("wp8", N * K, U8, "bytes"), ("wscale", N, F32)]


def _w8(ops, c, w8):
    c.wp8.copy_(w8.wp), c.wscale.copy_(w8.scale)
    return ops.Fp8Weight(c.wp8, c.wscale, w8.N, w8.K)


def _ws_fill(ws, which):
    A.poison(ws, slice(WS_TICKETS, None), which, kind="bytes")
    ws[:WS_TICKETS].zero_()


def _tickets_left_zero(ws):
    assert int(ws[:WS_TICKETS].to(torch.int32).sum()) == 0, "arrival tickets not left at zero"


# ---------------------------------------------------------------- dfl_gemm_f32_batch
F32B = [(R, K, kind, "bf16") for R, K in RK for kind in ("frag", "rows")] + [(3, 256, "rows", "e4m3"), (4, 2112, "frag", "e4m3")]


@gpu
@pytest.mark.parametrize("R,K,kind,fmt", F32B, ids=[f"R{R}-K{K}-{k}-{f}" for R, K, k, f in F32B])
def test_gemm_f32_batch_bounds(ops, R, K, kind, fmt):
    """out is exactly [ksplit][tiles * 16][N] floats; the parts of a live request sum to torch's exact product.  e4m3
    (k_gemm_b<.., W8>): small integers quantise exactly, the scale vector is exactly N floats."""
    N, MT, ks = 272, ops.batch_tiles(R), ops.batch_ksplit(K)
    w = B.small_ints((N, K), N + K + R)
    wp0 = ops.pack_weight(w)
    w8 = ops.pack_weight_fp8(*ops.quantize_fp8_rows(w)) if fmt == "e4m3" else None
    c = B.Case(max(K, N), (_w8_plan(N, K) if w8 else [("wp", N * K, BF16)])
               + [("out", (ks, MT * 16, N), F32), ("dyn", (MT, 8), I32, "index")] + _BSrc.plan(kind, MT, K))
    src = _BSrc(ops, c, kind, R, MT, K, seed=R + K)
    wt = _w8(ops, c, w8) if w8 else c.wp

    def make(which):
        _w8(ops, c, w8) if w8 else c.wp.copy_(wp0)
        src.fill(which)
        c.out.fill_(float("nan"))
    res = c.run(make, lambda: ops.gemm_f32_batch(wt, src.src, R, N, K, c.out, c.dyn), lambda: {"out": c.out[:, :R * 16]})
    assert torch.equal(res["out"].sum(0).view(R, 16, N), src.xs[:R] @ w.float().T)


# ---------------------------------------------------------------- dfl_gemm_resid_batch
@gpu
@pytest.mark.parametrize("kind", ["frag", "rows"])
@pytest.mark.parametrize("R,K", RK, ids=[f"R{R}-K{K}" for R, K in RK])
def test_gemm_resid_batch_bounds(ops, R, K, kind):
    """h_io / tap with row strides above N, ss_out of exactly N floats per request, ws of exactly
    dfl_gemm_batch_ws_bytes(N, K); S: the same bits on a four times larger zeroed workspace."""
    N, MT = 272, ops.batch_tiles(R)
    ld, ldt = N + 48, N + 80
    w = B.small_ints((N, K), N + K + R)
    wp0 = ops.pack_weight(w)
    c = B.Case(max(K, ldt), [("wp", N * K, BF16), ("h", (MT, 16, ld), BF16), ("tap", (MT, 16, ldt), BF16),
                             ("ss", (MT, N), F32), ("ws", ops.lib().dfl_gemm_batch_ws_bytes(N, K), U8, "bytes"),
                             ("dyn", (MT, 8), I32, "index")] + _BSrc.plan(kind, MT, K))
    src = _BSrc(ops, c, kind, R, MT, K, seed=R + K + 1)
    h0 = torch.stack([SG._distinct_resid(ld)] * MT)

    def make(which):
        c.wp.copy_(wp0)
        src.fill(which)
        c.h.copy_(h0)
        c.tap.fill_(5.0)
        c.ss.fill_(float("nan"))
        _ws_fill(c.ws, which)

    def launch_with(ws):
        ops.gemm_resid_batch(c.wp, src.src, R, N, K, c.h, add_residual=True, ws=ws, dyn=c.dyn, ss_out=c.ss,
                             tap=c.tap[:, :, 40:40 + N])
    outs = lambda: {"h": c.h[:R], "tap": c.tap[:R], "ss": c.ss[:R]}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs)
    _tickets_left_zero(c.ws)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    want = (h0[:R, :, :N].float() + (src.xs[:R] @ w.float().T).to(BF16).float()).to(BF16)
    assert torch.equal(res["h"][:, :, :N], want) and torch.equal(res["h"][:, :, N:], h0[:R, :, N:])
    assert torch.equal(res["tap"][:, :, 40:40 + N], want)
    assert torch.all(res["tap"][:, :, :40] == 5.0) and torch.all(res["tap"][:, :, 40 + N:] == 5.0)
    for r in range(R):
        torch.testing.assert_close(res["ss"][r], SG._ss_ref(want[r]), rtol=2e-6, atol=0)


# ---------------------------------------------------------------- dfl_gemm_silu_mul_batch
SILUB = [(R, K, kind, "bf16") for R, K in RK for kind in ("frag", "rows")] + [(3, 256, "frag", "e4m3"), (4, 2112, "frag", "e4m3")]


@gpu
@pytest.mark.parametrize("R,K,kind,fmt", SILUB,
                         ids=[f"R{R}-K{K}-{'ring' if k == 'frag' else 'slab'}-{f}" for R, K, k, f in SILUB])
def test_gemm_silu_mul_batch_bounds(ops, R, K, kind, fmt):
    """act is exactly [tiles][16 I]; the ring form (frag16 sources) and k_gemm_b (plain rows, K parts met in ws slabs);
    e4m3 runs the W8 ring form with the gate / up scales of exactly 2 I floats."""
    I, MT = 272, ops.batch_tiles(R)
    g = B.cuda_gen(I + K + R)
    up = torch.randint(-2, 3, (I, K), generator=g, device=B.dev(), dtype=torch.int8).to(BF16)
    gate = torch.randint(-2, 3, (I, K), generator=g, device=B.dev(), dtype=torch.int8).to(BF16) * 2 ** -6
    wp0 = ops.pack_weight_gateup(gate, up)
    w8 = ops.pack_weight_gateup_fp8(*ops.quantize_fp8_rows(gate), *ops.quantize_fp8_rows(up)) if fmt == "e4m3" else None
    c = B.Case(max(K, I), (_w8_plan(2 * I, K) if w8 else [("wp", 2 * I * K, BF16)])
               + [("act", (MT, 16 * I), BF16), ("dyn", (MT, 8), I32, "index"),
                  ("ws", ops.lib().dfl_gemm_batch_ws_bytes(2 * I, K), U8, "bytes")] + _BSrc.plan(kind, MT, K))
    src = _BSrc(ops, c, kind, R, MT, K, seed=R + K + 2)
    wt = _w8(ops, c, w8) if w8 else c.wp

    def make(which):
        _w8(ops, c, w8) if w8 else c.wp.copy_(wp0)
        src.fill(which)
        c.act.fill_(float("nan"))
        _ws_fill(c.ws, which)

    def launch_with(ws):
        ops.gemm_silu_mul_batch(wt, src.src, R, I, K, c.act, ws, c.dyn)
    outs = lambda: {"act": c.act[:R]}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs)
    _tickets_left_zero(c.ws)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    for r in range(R):
        got, want = H.unfrag(res["act"][r], I), BK._silu_ref(src.xs[r], gate, up)
        d = BK._bf16_ulps(got, want)
        assert int(d.max()) <= 2 and float((d > 0).float().mean()) <= 1e-3, r      # test_ring_gemm_silu_mul_batch's bar
        assert torch.count_nonzero(got[src.nv[r]:].float()) == 0, r


# ---------------------------------------------------------------- dfl_gemm_argmax_batch / dfl_gemm_sample_batch
# (R, V, K, form, sample): V = 4208 has 7 ring workgroups with a second unit; the slab form is k_gemm_b (argmax only)
LM8 = [(3, 528, 256, "ring8", False), (4, 528, 2112, "ring8", True)]      # e4m3: the W8 ring forms, scales of exactly V floats
LM = [(1, 4208, 256, "ring", False), (3, 4208, 256, "ring", False), (4, 528, 2112, "ring", False),
      (3, 528, 256, "slab", False), (4, 528, 2112, "slab", False),
      (1, 4208, 256, "ring", True), (4, 528, 2112, "ring", True), (3, 528, 256, "ring", True)]


@gpu
@pytest.mark.parametrize("R,V,K,form,sample", LM + LM8,
                         ids=[f"{'sample' if s else 'argmax'}-R{R}-V{V}-K{K}-{f}" for R, V, K, f, s in LM + LM8])
def test_gemm_argmax_sample_batch_bounds(ops, R, V, K, form, sample):
    """row0 = 1 with the row counts from the records (a request with bs = 1 has no live row), ids at out_off of rows of
    exactly 20 ids, a logits output whose request stride (16 * (V + 8)) lies above 16 * V: the 8 trailing columns' worth of
    slack per request keeps its sentinel.  seeds / inv_ts hold exactly one entry per tile."""
    MT, off, ROW0 = ops.batch_tiles(R), 2, 1
    kind = "frag" if form.startswith("ring") else "rows"
    lstride = 16 * (V + 8)
    w = B.small_ints((V, K), V + K + R)
    wp0 = ops.pack_weight(w)
    w8 = ops.pack_weight_fp8(*ops.quantize_fp8_rows(w)) if form == "ring8" else None
    c = B.Case(max(K, V), (_w8_plan(V, K) if w8 else [("wp", V * K, BF16)]) + [("ids", (MT, 20), I64, "index"), ("logits", (MT, lstride), BF16),
                           ("ws", ops.lib().dfl_gemm_batch_ws_bytes(V, K), U8, "bytes"), ("dyn", (MT, 8), I32, "index"),
                           ("seeds", MT, I64, "index"), ("inv_ts", MT, F32)] + _BSrc.plan(kind, MT, K))
    src = _BSrc(ops, c, kind, R, MT, K, seed=R + K + 3)
    live = BSS[R]

    def make(which):
        _w8(ops, c, w8) if w8 else c.wp.copy_(wp0)
        src.fill(which)
        for r in range(R):
            c.dyn[r, BS] = live[r]
            c.dyn[r, POS0] = 100 + r
        c.ids.fill_(-1)
        c.logits.fill_(3.0)
        c.seeds.copy_(torch.arange(7, 7 + MT))
        c.inv_ts.copy_(torch.tensor([1.25, 0.0, 2.0, 0.5][:MT]))      # slot 1: greedy
        _ws_fill(c.ws, which)
    lg = torch.as_strided(c.logits, (MT, 16, V), (lstride, V, 1))

    def launch_with(ws):
        lib, st = ops.lib(), torch.cuda.current_stream().cuda_stream
        wd = ops._w(_w8(ops, c, w8) if w8 else c.wp, V, K, "wp")
        if sample:
            ops.check(lib.dfl_gemm_sample_batch(wd, src.src.ref, R, V, K, ROW0, 16 - ROW0, c.dyn.data_ptr(), BS, ws.data_ptr(),
                                                c.ids.data_ptr(), 20, off, c.logits.data_ptr(), lstride, c.seeds.data_ptr(),
                                                c.inv_ts.data_ptr(), 0.0, 0, POS0, 0, 1, st), "dfl_gemm_sample_batch")
        else:
            ops.check(lib.dfl_gemm_argmax_batch(wd, src.src.ref, R, V, K, ROW0, 16 - ROW0, c.dyn.data_ptr(), BS, ws.data_ptr(),
                                                c.ids.data_ptr(), 20, off, c.logits.data_ptr(), lstride, st),
                      "dfl_gemm_argmax_batch")
    outs = lambda: {"ids": c.ids[:R], "logits": c.logits[:R]}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    ref = (src.x.float() @ w.float().T).to(BF16)      # (frag rows are all valid; a plain-row source counts rows < bs)
    got_lg = torch.as_strided(res["logits"], (R, 16, V), (lstride, V, 1))
    for r in range(R):
        n = max(live[r] - ROW0, 0)
        assert torch.all(res["ids"][r, :off] == -1) and torch.all(res["ids"][r, off + n:] == -1), r
        assert torch.equal(got_lg[r, ROW0:ROW0 + n], ref[r, ROW0:ROW0 + n]), r
        assert torch.all(got_lg[r, :ROW0] == 3.0) and torch.all(got_lg[r, ROW0 + n:] == 3.0), r
        assert torch.all(res["logits"][r, 16 * V:] == 3.0), r
        ids = res["ids"][r, off:off + n]
        if n and (not sample or r == 1):
            assert torch.equal(ids, B.first_argmax(ref[r, ROW0:ROW0 + n].float())), r
        assert n == 0 or (int(ids.min()) >= 0 and int(ids.max()) < V), r
    del lg


# ---------------------------------------------------------------- one workspace shared by several (N, K)
@gpu
def test_gemm_batch_ws_shared_across_shapes(ops):
    """The sharing rule tile_stack.gemm_ws relies on: ONE workspace of the maximum of dfl_gemm_batch_ws_bytes over the
    (N, K) of a layer, used by launches of each shape in turn (slab gate/up at K = 2112, resid at another N, slab argmax),
    twice over: every launch leaves the tickets the next one needs at zero, whatever the other shape left in the slabs."""
    R, K, I, N, V = 3, 2112, 160, 272, 528
    MT = ops.batch_tiles(R)
    shapes = [(2 * I, K), (N, I), (V, K)]
    wsb = max(ops.lib().dfl_gemm_batch_ws_bytes(n, k) for n, k in shapes)
    assert len({ops.lib().dfl_gemm_batch_ws_bytes(n, k) for n, k in shapes}) == 3
    g = B.cuda_gen(5)
    ri = lambda *s: torch.randint(-2, 3, s, generator=g, device=B.dev(), dtype=torch.int8).to(BF16)      # noqa: E731
    gate, up, wd, wl = ri(I, K) * 2 ** -6, ri(I, K), ri(N, I), ri(V, K)
    wgu0, wd0, wl0 = ops.pack_weight_gateup(gate, up), ops.pack_weight(wd), ops.pack_weight(wl)
    c = B.Case(K, [("wgu", 2 * I * K, BF16), ("wd", N * I, BF16), ("wl", V * K, BF16), ("act", (MT, 16 * I), BF16),
                   ("h", (MT, 16, N), BF16), ("ids", (MT, 16), I64, "index"), ("ws", wsb, U8, "bytes"),
                   ("dyn", (MT, 8), I32, "index")] + _BSrc.plan("rows", MT, K))
    src = _BSrc(ops, c, "rows", R, MT, K, seed=77)

    def make(which):
        c.wgu.copy_(wgu0), c.wd.copy_(wd0), c.wl.copy_(wl0)
        src.fill(which)
        c.act.fill_(float("nan"))
        c.h.zero_()
        c.ids.fill_(-1)
        _ws_fill(c.ws, which)

    def launch_with(ws):
        for _ in range(2):
            ops.gemm_silu_mul_batch(c.wgu, src.src, R, I, K, c.act, ws, c.dyn)
            ops.gemm_resid_batch(c.wd, ops.brows_frag(c.act), R, N, I, c.h, add_residual=False, ws=ws, dyn=c.dyn)
            ops.gemm_argmax_batch(c.wl, src.src, R, V, K, 0, 16, ws, c.ids, 0, c.dyn, nrows_dyn_word=BS)
    outs = lambda: {"act": c.act[:R], "h": c.h[:R], "ids": c.ids[:R]}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs)
    _tickets_left_zero(c.ws)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    for r in range(R):
        act = H.unfrag(res["act"][r], I)
        H.assert_close(f"shared ws resid r{r}", res["h"][r], act.float() @ wd.float().T)
        n = src.nv[r]
        assert torch.equal(res["ids"][r, :n], B.first_argmax((src.xs[r, :n] @ wl.float().T).to(BF16).float())), r
        assert torch.all(res["ids"][r, n:] == -1), r


# ---------------------------------------------------------------- dfl_norm_frag_batch
@gpu
@pytest.mark.parametrize("R,Hd,nsplit", [(1, 72, 1), (3, 4104, 2), (4, 8200, 3)], ids=lambda v: str(v))
def test_norm_frag_batch_bounds(ops, R, Hd, nsplit):
    """h of exactly R requests (only r < R is touched), the parts laid out for dfl_batch_tiles(R) tile slots, the part
    rows of dead rows holding the pattern ("loaded but ignored"), frag of exactly R x 16 H.  Dead rows: frag zero, h and
    tap untouched.  The three compiled widths (H <= 4096, <= 8192, above)."""
    from oracle.dflash_oracle import rms_norm
    MT = ops.batch_tiles(R)
    nvs = BSS.get(R, [16])
    ldt = Hd + 16
    g = B.cuda_gen(R + Hd)
    h0 = (torch.randn(R, 16, Hd, generator=g, device=B.dev()) * 0.7).to(BF16)
    part0 = torch.randn(nsplit, MT * 16, Hd, generator=g, device=B.dev()) * 0.3
    nw = (1 + 0.1 * torch.randn(Hd, generator=g, device=B.dev())).to(BF16)
    c = B.Case(ldt, [("h", (R, 16, Hd), BF16), ("part", (nsplit, MT * 16, Hd), F32), ("tap", (R, 16, ldt), BF16),
                     ("nw", Hd, BF16), ("frag", (R, 16 * Hd), BF16), ("dyn", (R, 8), I32, "index")])

    def make(which):
        c.h.copy_(h0), c.part.copy_(part0), c.nw.copy_(nw)
        c.tap.fill_(5.0)
        c.frag.fill_(float("nan"))
        c.dyn.zero_()
        pv = c.part.view(nsplit, MT, 16, Hd)
        for r in range(R):
            c.dyn[r, BS] = nvs[r]
            A.poison(pv, (slice(None), r, slice(nvs[r], None)), which)
        A.poison(pv, (slice(None), slice(R, None)), which)
    res = c.run(make, lambda: ops.norm_frag_batch(c.h, R, c.nw, 1e-6, c.frag, c.dyn, BS, part=c.part, N=Hd, nsplit=nsplit,
                                                  tap=c.tap[:, :, 8:8 + Hd]),
                lambda: {"h": c.h, "tap": c.tap, "frag": c.frag})
    assert torch.all(res["tap"][:, :, :8] == 5.0) and torch.all(res["tap"][:, :, 8 + Hd:] == 5.0)
    for r in range(R):
        nv = nvs[r]
        s = torch.zeros(16, Hd, device=B.dev())
        for k in range(nsplit):
            s = s + part0[k, r * 16:r * 16 + 16]
        want = (h0[r].float() + s.to(BF16).float()).to(BF16)
        assert torch.equal(res["h"][r, :nv], want[:nv]) and torch.equal(res["h"][r, nv:], h0[r, nv:]), r
        assert torch.equal(res["tap"][r, :nv, 8:8 + Hd], want[:nv]) and torch.all(res["tap"][r, nv:] == 5.0), r
        fr = H.unfrag(res["frag"][r], Hd)
        assert torch.count_nonzero(fr[nv:].float()) == 0, r
        H.assert_close(f"norm_frag_batch r{r}", fr[:nv], rms_norm(want[:nv], nw, 1e-6), max_rel=2 ** -6, mean_rel=H.MEAN_REL)


# ---------------------------------------------------------------- dfl_embed_rows_batch
@gpu
@pytest.mark.parametrize("R", [1, 3, 4])
def test_embed_rows_batch_bounds(ops, R):
    """The table at exactly [V][H] with its last row in use, ids rows of exactly 16 with the pattern past the count, h_out
    and ss_out of exactly R requests."""
    V, Hd = 40, 72
    nvs = BSS[R]
    emb = B.small_ints((V, Hd), 4, -9, 9)
    ids = torch.randint(0, V, (R, 16), generator=B.cuda_gen(R), device=B.dev())
    ids[:, 0] = V - 1
    c = B.Case(Hd, [("emb", (V, Hd), BF16), ("ids", (R, 16), I64, "index"), ("h", (R, 16, Hd), BF16), ("ss", (R, 16), F32),
                    ("dyn", (R, 8), I32, "index")])

    def make(which):
        c.emb.copy_(emb), c.ids.copy_(ids)
        c.dyn.zero_()
        for r in range(R):
            c.dyn[r, BS] = nvs[r]
            A.poison(c.ids, (r, slice(nvs[r], None)), which)
        c.h.fill_(-3.0)
        c.ss.fill_(float("nan"))
    res = c.run(make, lambda: ops.embed_rows_batch(c.emb, c.ids, R, c.h, Hd, c.ss, c.dyn, BS), lambda: {"h": c.h, "ss": c.ss})
    for r in range(R):
        nv = nvs[r]
        assert torch.equal(res["h"][r, :nv], emb[ids[r, :nv]]) and torch.all(res["h"][r, nv:] == -3.0), r
        want = torch.zeros(16, device=B.dev())
        want[:nv] = emb[ids[r, :nv]].float().pow(2).sum(1)
        assert torch.equal(res["ss"][r], want), r


# ---------------------------------------------------------------- dfl_kv_append_batch
@gpu
@pytest.mark.parametrize("tpr", [1, 2], ids=["tiles1", "tiles2"])
def test_kv_append_batch_bounds(ops, tpr):
    """Caches of exactly cache_rows rows per (request, layer, head) with one request's appended rows ending on the last
    row and another's running one row past it: that row is "silently not stored", so the rows behind the cache (the next
    head's first row, or the guard behind the last head) keep their bits.  Rotation tables of exactly max_pos rows with a
    position at max_pos - 1 and positions past it (clamped: the K row equals the one rotated at max_pos - 1).  The fp32
    parts hold the pattern in rows at or past a tile's tau."""
    from dflash_amd.model import _rope_tables
    L, n_kv, rows, T = 2, 2, 48, 4
    nreq = T // tpr
    kd = n_kv * 128
    ld = L * 2 * kd
    max_pos = 60
    # tile: (S, tau, pos0).  Tile 0 reaches position max_pos - 1 with its last row; tile 1 fills the cache to its last row
    # and runs one row past it; tile 2 is idle; tile 3 rotates past max_pos.  (Tiles 2 q, 2 q + 1 share a cache at
    # tiles_per_req = 2: their rows do not overlap.)
    tiles = [(8, 16, max_pos - 16), (rows - 4, 5, 10), (7, 0, 7), (3, 7, max_pos - 2)]
    g = B.cuda_gen(tpr)
    parts0 = torch.randn(2, T * 16, ld, generator=g, device=B.dev())
    kw = (1 + 0.1 * torch.randn(L, 128, generator=g, device=B.dev())).to(BF16)
    kc0 = torch.randn(nreq, L, n_kv, rows, 128, generator=g, device=B.dev()).to(BF16)
    cos, sin = _rope_tables(128, 1e6, max_pos, B.dev())
    c = B.Case(ld, [("parts", (2, T * 16, ld), F32), ("kw", (L, 128), BF16), ("kc", (nreq, L, n_kv, rows, 128), BF16),
                    ("vc", (nreq, L, n_kv, rows, 128), BF16), ("cos", (max_pos, 64), BF16), ("sin", (max_pos, 64), BF16),
                    ("dyn", (T, 8), I32, "index")])

    def make(which):
        c.parts.copy_(parts0), c.kw.copy_(kw), c.kc.copy_(kc0), c.vc.copy_(kc0), c.cos.copy_(cos), c.sin.copy_(sin)
        c.dyn.zero_()
        for t, (S, tau, pos0) in enumerate(tiles):
            c.dyn[t, 0], c.dyn[t, TAU], c.dyn[t, POS0] = S, tau, pos0
            A.poison(c.parts, (slice(None), slice(t * 16 + tau, t * 16 + 16)), which)
    res = c.run(make, lambda: BK._kv_call(ops, c.parts, T, ld, kd, L, n_kv, c.kw, c.cos, c.sin, c.kc, c.vc, c.dyn, tpr=tpr),
                lambda: {"kc": c.kc, "vc": c.vc})
    lin = parts0.sum(0).to(BF16).cpu()
    vexp, touched = kc0.clone(), torch.zeros(nreq, L, n_kv, rows, dtype=torch.bool, device=B.dev())
    for t, (S, tau, pos0) in enumerate(tiles):
        q = t // tpr
        for ly in range(L):
            x = lin[t * 16:t * 16 + tau, ly * 2 * kd:(ly + 1) * 2 * kd]
            n = min(tau, rows - S)                       # rows at or past cache_rows are dropped
            if n <= 0:
                continue
            vexp[q, ly, :, S:S + n] = x[:n, kd:].reshape(n, n_kv, 128).transpose(0, 1).to(B.dev())
            touched[q, ly, :, S:S + n] = True
            kref = torch.cat([BK._rope_ref(x[i:i + 1, :kd].reshape(1, n_kv, 128), kw[ly].cpu(), min(pos0 + i, max_pos - 1))
                              for i in range(n)], dim=1)
            BK._assert_rope_bar(f"kv_append bounds tile {t} layer {ly}", res["kc"][q, ly, :, S:S + n].cpu(), kref)
    assert torch.equal(res["vc"], vexp)
    assert torch.equal(res["kc"][~touched], kc0[~touched])
