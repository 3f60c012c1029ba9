"""Bounds of the sparse-MoE launches (moe.hip, moe_route.h, the MoE half of prefill.hip) and of the dense prefill
launches (prefill.hip) inside a guarded arena (tests/arena.py, tests/bounds_common.py: W, R, S).

Decode MoE: rlog with ld at its minimum (E padded to 16), wt / active / list sized by E exactly, the experts' weights
back to back with the LAST expert active (its weights end the buffer), 5 valid rows of 16.  E = 2, 24 and 200 (no
multiple of the padding), top_k = 1 and 8.
Prefill MoE: the scratch dict of dflash_amd.ops.prefill_moe_scratch rebuilt from arena views of exactly the sizes the
wrapper computes from dfl_prefill_moe_max_tiles / _max_items / dfl_prefill_rows_padded, at the plans that make them tight
(one expert takes every row; every expert takes one row) and both rows_per_item.
Dense prefill: row buffers of exactly dfl_prefill_rows_padded(P) rows, caches of exactly P rows, P = 1, 17 and 129.

Each chain of launches runs under both guard patterns and once more on ordinary torch allocations holding the same
bytes, whose outputs must be bit-equal (bounds_common.check_launch)."""
import pytest
import torch

import arena as A
import bounds_common as B
import helpers as H

gpu = pytest.mark.gpu
BF16, F32, I32, I64, U8 = B.BF16, B.F32, B.I32, B.I64, B.U8
BS = 2

COVERS = {
    "dfl_moe_router": "test_moe_decode_bounds",
    "dfl_moe_route": "test_moe_decode_bounds",
    "dfl_moe_gate_up": "test_moe_decode_bounds",
    "dfl_gemm_silu_mul_experts": "test_moe_decode_bounds",
    "dfl_moe_down": "test_moe_decode_bounds",
    "dfl_prefill_gemm_rows": "test_prefill_dense_bounds",
    "dfl_prefill_gemm_resid": "test_prefill_dense_bounds",
    "dfl_prefill_gemm_silu": "test_prefill_dense_bounds",
    "dfl_prefill_norm_pack": "test_prefill_dense_bounds",
    "dfl_prefill_pack_rows": "test_prefill_dense_bounds",
    "dfl_prefill_qk_rope": "test_prefill_dense_bounds",
    "dfl_prefill_attn": "test_prefill_dense_bounds",
    "dfl_prefill_moe_route": "test_prefill_moe_bounds",
    "dfl_prefill_moe_gather": "test_prefill_moe_bounds",
    "dfl_prefill_moe_gemm_silu": "test_prefill_moe_bounds",
    "dfl_prefill_moe_gemm_down": "test_prefill_moe_bounds",
    "dfl_prefill_moe_combine": "test_prefill_moe_bounds",
    "dfl_moe_grouped_gate_up": "test_prefill_moe_bounds",
    "dfl_moe_grouped_down": "test_prefill_moe_bounds",
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def _randn(g, *shape, s=1.0):
    return (torch.randn(*shape, generator=g, device=B.dev()) * s).to(BF16)


# ---------------------------------------------------------------- the decode MoE chain
@gpu
@pytest.mark.parametrize("E,top_k,nan_row", [(2, 1, None), (24, 8, None), (200, 8, None), (8, 8, 2), (2, 1, 2), (24, 8, 4)],
                         ids=lambda v: str(v))
def test_moe_decode_bounds(ops, E, top_k, nan_row):
    """dfl_moe_router (norm + gate Linear + routing in one launch), dfl_moe_route on the logits it left, dfl_moe_gate_up,
    dfl_gemm_silu_mul_experts and dfl_moe_down, on the rows of one tile with 5 valid rows.  The outputs of inactive experts
    keep their sentinels; rows at or past the count route nowhere.
    nan_row: one VALID hidden row is NaN throughout (under both patterns): its logits are NaN and it routes to experts
    0 .. top_k - 1 with NaN weights (test_hip_moe.py::test_moe_route_nan_row_and_edges) — at E = 8 / top-8 onto the last
    expert, at E = 2 / top-1 beside it; the scan and the list write must stay inside the E-sized wt / active / list, the
    other rows route as always, and the NaN stays in that row of the expert sums."""
    K, I, N, nv, nsplit = 256, 64, 256, 5, 2
    Ep = -(-E // 16) * 16
    g = B.cuda_gen(E)
    h0, nw0 = _randn(g, 16, K + 8), (1 + 0.1 * torch.randn(K, generator=g, device=B.dev())).to(BF16)
    wr = _randn(g, Ep, K, s=0.05)
    wr[E:] = 0
    wr[E - 1] = torch.sign(h0[0, :K].float()).to(BF16) * 0.02 * nw0.sign()         # row 0 routes to the LAST expert (a logit of ~4)
    if nan_row is not None:
        h0[nan_row] = float("nan")
    ok = [m for m in range(nv) if m != nan_row]                                    # the valid rows that hold numbers
    wr0 = ops.pack_weight(wr)
    wgu0 = torch.stack([ops.pack_weight_gateup(_randn(g, I, K, s=0.06), _randn(g, I, K, s=0.06)) for _ in range(E)])
    wd0 = torch.stack([ops.pack_weight(_randn(g, N, I, s=0.1)) for _ in range(E)])
    ix = "index"
    plan = [("h", (16, K + 8), BF16), ("nw", K, BF16), ("xn", 16 * K, BF16), ("wr", Ep * K, BF16), ("rlog", (16, Ep), BF16),
            ("wt", (16, E), BF16), ("active", E, I32, ix), ("lst", E, I32, ix), ("n_act", 1, I32, ix), ("ticket", 1, I32, ix),
            ("wt2", (16, E), BF16), ("active2", E, I32, ix), ("lst2", E, I32, ix), ("n_act2", 1, I32, ix),
            ("dyn", 8, I32, ix), ("wgu", (E, 2 * I * K), BF16), ("wd", (E, N * I), BF16), ("act", (E, 16 * I), BF16),
            ("act2", (E, 16 * I), BF16), ("out", (nsplit, 16, N), F32)]

    def make(c, which):
        c.h.copy_(h0), c.nw.copy_(nw0), c.wr.copy_(wr0), c.wgu.copy_(wgu0), c.wd.copy_(wd0)
        A.poison(c.h, [(slice(nv, None), slice(None)), (slice(None), slice(K, None))], which)
        c.dyn.zero_()
        c.dyn[BS] = nv
        c.ticket.zero_()
        c.xn.fill_(float("nan")), c.rlog.fill_(-7.0), c.wt.fill_(-7.0), c.wt2.fill_(-7.0)
        for n in ("active", "lst", "n_act", "active2", "lst2", "n_act2"):
            getattr(c, n).fill_(-7)
        c.act.fill_(-7.0), c.act2.fill_(-7.0), c.out.fill_(float("nan"))

    def launch(t):
        ops.moe_router(h=t.h[:, :K], norm_w=t.nw, eps=1e-6, xn=t.xn, wp_router=t.wr, K=K, E=E, top_k=top_k, norm_topk=True,
                       rlog=t.rlog, wt=t.wt, active=t.active, lst=t.lst, n_active=t.n_act, ticket=t.ticket, dyn=t.dyn, dyn_word=BS)
        ops.moe_route(t.rlog, E, top_k, True, t.wt2, t.active2, t.lst2, t.n_act2, dyn=t.dyn, dyn_word=BS)
        ops.moe_gate_up(t.wgu, t.xn, E, I, K, t.act, t.lst, t.n_act, dyn=t.dyn, valid_word=BS)
        ops.gemm_silu_mul_experts(t.wgu, t.xn, E, I, K, t.act2, t.lst, t.n_act, dyn=t.dyn)
        ops.moe_down(t.wd, t.act, t.wt, t.lst, t.n_act, E, N, I, nsplit, t.out)
    # list entries at or past n_active are left as they were; the logits of rows at or past the count are unspecified
    outs = ["xn", ("rlog", lambda t: t.rlog[:nv]), "wt", "active", "n_act", "ticket", "wt2", "active2", "n_act2", "act", "act2",
            "out", ("lst", lambda t: t.lst[:int(t.n_act)]), ("lst2", lambda t: t.lst2[:int(t.n_act2)])]
    c, res = B.check_launch(K + 8, plan, make, launch, outs)
    n = int(res["n_act"])
    lst = res["lst"].tolist()
    assert 1 <= n <= min(E, nv * top_k) and lst == sorted(lst) and lst[-1] == E - 1 and int(res["ticket"]) == 0
    assert res["lst2"].tolist() == lst and torch.equal(A.bits(res["wt2"]), A.bits(res["wt"]))      # (bits: a NaN row's weights)
    assert torch.equal(res["active2"], res["active"])
    wt = res["wt"].float()
    assert torch.count_nonzero(wt[nv:]) == 0 and torch.all((wt[ok] > 0).sum(1) == top_k)
    torch.testing.assert_close(wt[ok].sum(1), torch.ones(len(ok), device=B.dev()), rtol=0, atol=2e-2)
    xn = H.unfrag(res["xn"], K)
    assert torch.isfinite(xn[ok].float()).all() and torch.count_nonzero(xn[nv:].float()) == 0
    on = torch.zeros(E, dtype=torch.bool, device=B.dev())
    on[lst] = True
    acts = torch.stack([H.unfrag(a, I) for a in res["act"]]).float()      # [E, 16, I]
    acts2 = torch.stack([H.unfrag(a, I) for a in res["act2"]]).float()
    for a, au in ((res["act"], acts), (res["act2"], acts2)):
        assert torch.all(a[~on] == -7.0) and torch.isfinite(au[on][:, ok]).all() and torch.count_nonzero(au[on][:, nv:]) == 0
    H.assert_close("moe_gate_up vs gemm_silu_mul_experts", acts[on][:, ok], acts2[on][:, ok], max_rel=2e-2, mean_rel=2e-3)
    if nan_row is not None:      # the NaN row: NaN weights on experts 0 .. top_k - 1 only, NaN in its row of every sum
        assert torch.isnan(wt[nan_row, :top_k]).all() and torch.count_nonzero(wt[nan_row, top_k:]) == 0
        assert all(e in lst for e in range(top_k)) and torch.isnan(xn[nan_row].float()).all()
        assert torch.isnan(acts[on][:, nan_row]).all() and torch.isnan(res["out"].sum(0)[nan_row]).all()
        assert torch.isfinite(res["out"][:, ok]).all()
    wdm = wd0.view(E, N // 16, I // 32, 4, 16, 8).permute(0, 1, 4, 2, 3, 5).reshape(E, N, I).float()      # unpack dfl_pack_weight
    want = torch.zeros(16, N, device=B.dev())
    for e in lst:
        want[ok] += wt[ok][:, e, None] * (acts[e][ok] @ wdm[e].T)
    H.assert_close("moe_down bounds", res["out"].sum(0)[ok], want[ok], max_rel=2e-2, mean_rel=2e-3)


# ---------------------------------------------------------------- the prefill MoE chain
def _scratch_plan(ops, P, Hd, I, E, top_k, rcols):
    """The members of dflash_amd.ops.prefill_moe_scratch, at the sizes that wrapper computes."""
    L = ops.lib()
    mt, mi = int(L.dfl_prefill_moe_max_tiles(P, top_k, E)), int(L.dfl_prefill_moe_max_items(P, top_k, E))
    ix = "index"
    return mt, mi, [("rlog", (ops.prefill_rows_padded(P), rcols), BF16), ("pair_e", (P, 8), I32, ix), ("posmap", (P, 8), I32, ix),
                    ("pair_w", (P, 8), F32), ("cnt", E, I32, ix), ("tile_off", E, I32, ix), ("src_row", mt * 16, I32, ix),
                    ("items", 3 * mi, I32, ix), ("n_items", 2, I32, ix), ("xg", mt * 16 * Hd, BF16), ("act_g", mt * 16 * I, BF16),
                    ("row_w", mt * 16, F32), ("out32", (mt * 16, Hd), F32), ("zeros", 512, BF16)]


SC_NAMES = ("rlog", "pair_e", "posmap", "pair_w", "cnt", "tile_off", "src_row", "items", "n_items", "xg", "act_g", "row_w", "out32",
            "zeros")


@gpu
@pytest.mark.parametrize("rpi", [64, 128], ids=["rpi64", "rpi128"])
@pytest.mark.parametrize("plan_kind,P,E,top_k", [("one-expert", 130, 8, 1), ("one-row-each", 8, 8, 1), ("spread", 33, 8, 8)],
                         ids=lambda v: str(v))
def test_prefill_moe_bounds(ops, plan_kind, P, E, top_k, rpi):
    """ops.prefill_moe_mlp (router GEMM, dfl_prefill_moe_route, _gather, _gemm_silu, _gemm_down, _combine) and the two
    dfl_moe_grouped_* launches (gathering in the kernel's addresses) on a scratch of arena views.  one-expert: every row
    routes to the LAST expert (its weights end the buffer; ceil(P / 16) tiles of the max_tiles = ceil(P k / 16) + E);
    one-row-each: P = E rows, each to its own expert: E items and E tiles, one short of max_items = ceil(P k / 64) + E and
    of max_tiles, the most any plan of these P k pairs can take.  S: every member of the scratch again as torch.zeros of
    four times its size (max_tiles / max_items still the library's figures): the same bits."""
    Hd, I, rcols = 128, 64, 128
    Pp = ops.prefill_rows_padded(P)
    g = B.cuda_gen(P + E)
    x0 = _randn(g, P, Hd)
    wr = torch.zeros(rcols, Hd, dtype=BF16, device=B.dev())
    if plan_kind == "one-expert":
        wr[E - 1] = 0.0
        wr[:E - 1] = -1.0 * torch.sign(x0[0]).abs()              # (all logits of the other experts equal; the last is 0)
        x0 = x0.abs()
    elif plan_kind == "one-row-each":
        x0 = torch.zeros(P, Hd, dtype=BF16, device=B.dev())
        for r in range(P):
            x0[r, r] = 4.0
            wr[r, r] = 4.0
    else:
        wr[:E] = _randn(g, E, Hd, s=0.3)
    wr0 = ops.pack_weight(wr)
    gu0 = torch.stack([ops.pack_weight_gateup(_randn(g, I, Hd, s=0.1), _randn(g, I, Hd, s=0.1)) for _ in range(E)])
    dn0 = torch.stack([ops.pack_weight(_randn(g, Hd, I, s=0.1)) for _ in range(E)])
    h0 = _randn(g, P, Hd + 8)
    mt, mi, splan = _scratch_plan(ops, P, Hd, I, E, top_k, rcols)
    plan = splan + [("x", (P, Hd), BF16), ("xf", Pp * Hd, BF16), ("wr", rcols * Hd, BF16), ("gu", (E, 2 * I * Hd), BF16),
                    ("dn", (E, Hd * I), BF16), ("h", (P, Hd + 8), BF16), ("tap", (P, Hd), BF16), ("act2", mt * 16 * I, BF16),
                    ("out2", (mt * 16, Hd), F32)]

    def make(c, which):
        c.x.copy_(x0), c.wr.copy_(wr0), c.gu.copy_(gu0), c.dn.copy_(dn0), c.h.copy_(h0)
        A.poison(c.h, (slice(None), slice(Hd, None)), which)
        for n in SC_NAMES:                                       # a scratch "reused" from anything: the pattern everywhere
            A.poison(getattr(c, n), slice(None), which)
        c.zeros.zero_()
        c.xf.fill_(float("nan")), c.tap.fill_(-7.0)
        A.poison(c.act2, slice(None), which), A.poison(c.out2, slice(None), which)

    def launch(t):
        sc = dict(P=P, H=Hd, I=I, E=E, top_k=top_k, max_tiles=mt, max_items=mi, rows_per_item=rpi, **{n: getattr(t, n) for n in SC_NAMES})
        ops.prefill_pack_rows(t.x, P, Hd, t.xf)
        ops.prefill_moe_mlp(t.wr, t.gu, t.dn, t.xf, P, Hd, I, E, top_k, True, t.h[:, :Hd], sc, tap=t.tap)
        sc2 = dict(sc, act_g=t.act2, out32=t.out2)
        ops.moe_grouped_gate_up(t.gu, t.xf, sc2, Hd, gather=True)
        ops.moe_grouped_down(t.dn, sc2, Hd)
    outs = [("h", lambda t: t.h[:, :Hd]), "tap", ("pair_e", lambda t: t.pair_e[:P, :top_k]), ("pair_w", lambda t: t.pair_w[:P, :top_k]),
            ("cnt", lambda t: t.cnt[:E]), ("tile_off", lambda t: t.tile_off[:E]), ("n_items", lambda t: t.n_items[:2])]
    # posmap / src_row / items / out32 are the plan's internals: WHICH gathered row of its expert a pair gets is decided by
    # the order integer atomics land in and differs from run to run; what they add up to (h) does not.  They are checked
    # below on the state the last launch left, for consistency with each other.
    c, res = B.check_launch(Hd + 8, plan, make, launch, outs, ws_names=SC_NAMES)
    n_items, n_tiles = res["n_items"].tolist()
    assert 1 <= n_items <= mi and 1 <= n_tiles <= mt, (n_items, mi, n_tiles, mt)
    cnt = res["cnt"].tolist()
    assert sum(cnt) == P * top_k
    if plan_kind == "one-expert":
        assert cnt == [0] * (E - 1) + [P] and n_tiles == -(-P // 16)
    if plan_kind == "one-row-each":
        assert cnt == [1] * E and n_items == E == mi - 1 and n_tiles == E == mt - 1
    assert torch.isfinite(res["h"].float()).all() and torch.equal(res["tap"], res["h"])
    assert torch.all(c.h[:, Hd:].view(torch.int16) == A.pattern_scalar(BF16, "float", "A"))      # (the last fill) columns past H
    make(c, "A")
    launch(c)
    torch.cuda.synchronize()
    c.arena.check()
    src = c.src_row[:16 * n_tiles]
    assert int(src.max()) < P and int((src >= 0).sum()) == P * top_k
    assert sorted(src[src >= 0].tolist()) == sorted(list(range(P)) * top_k)          # every (row, slot) pair gathered once
    pm = c.posmap[:, :top_k]
    assert int(pm.min()) >= 0 and int(pm.max()) < 16 * n_tiles and pm.unique().numel() == P * top_k
    assert torch.equal(src[pm.long()], torch.arange(P, device=B.dev(), dtype=I32)[:, None].expand(P, top_k))
    # the work list: (expert, first gathered tile, tiles) per item, in tile order, covering the gathered tiles exactly once,
    # each expert's items spanning ceil(cnt / 16) tiles from its tile_off, none longer than rows_per_item
    items = c.items[:3 * n_items].view(n_items, 3).tolist()
    assert torch.all(c.items[3 * n_items:] == A.pattern_scalar(I32, "index", "A")), "items past n_items written"
    nxt, per_e = 0, [0] * E
    toff = res["tile_off"].tolist()
    for e, t0, nt in sorted(items, key=lambda it: it[1]):
        assert 0 <= e < E and t0 == nxt and 1 <= nt <= rpi // 16 and t0 >= toff[e], (e, t0, nt)
        nxt, per_e[e] = t0 + nt, per_e[e] + nt
    assert nxt == n_tiles and per_e == [-(-n // 16) for n in cnt]
    live = src >= 0
    assert torch.isfinite(c.out32[:16 * n_tiles][live]).all()
    H.assert_close("grouped gate/up + down, gathered in the kernel", c.out2[:16 * n_tiles][live], c.out32[:16 * n_tiles][live],
                   max_rel=1e-6, mean_rel=1e-7)


# ---------------------------------------------------------------- the dense prefill chain
@gpu
@pytest.mark.parametrize("P", [1, 17, 129])
def test_prefill_dense_bounds(ops, P):
    """pack_rows / norm_pack -> gemm_rows (q | k | v) -> qk_rope -> attn -> gemm_resid (+ tap) and gemm_silu, with row
    buffers of exactly dfl_prefill_rows_padded(P) rows, caches of exactly P rows, rotation tables of exactly max_pos rows
    with the last prompt rows at or past max_pos (clamped).  Rows at or past P of every row buffer keep their sentinels."""
    from dflash_amd.model import _rope_tables
    Hd, I, n_q, n_kv = 128, 128, 2, 1
    qd, N = n_q * 128, (n_q + 2 * n_kv) * 128
    Pp = ops.prefill_rows_padded(P)
    pos0 = 5
    max_pos = pos0 + P - (2 if P > 2 else 0)
    g = B.cuda_gen(P)
    rows0, nw0 = _randn(g, P, Hd + 8), (1 + 0.1 * torch.randn(Hd, generator=g, device=B.dev())).to(BF16)
    wqkv0 = ops.pack_weight(_randn(g, N, Hd, s=0.1))
    wo0, wgu0 = ops.pack_weight(_randn(g, Hd, qd, s=0.06)), ops.pack_weight_gateup(_randn(g, I, Hd, s=0.1), _randn(g, I, Hd, s=0.1))
    qw0, kw0 = (1 + 0.1 * torch.randn(128, generator=g, device=B.dev())).to(BF16), (1 + 0.1 * torch.randn(128, generator=g, device=B.dev())).to(BF16)
    cos0, sin0 = _rope_tables(128, 1e6, max_pos, B.dev())
    h0 = _randn(g, Pp, Hd + 8)
    plan = [("rows", (P, Hd + 8), BF16), ("nw", Hd, BF16), ("xf", Pp * Hd, BF16), ("xp", Pp * Hd, BF16), ("wqkv", N * Hd, BF16),
            ("qkv", (Pp, N), BF16), ("qw", 128, BF16), ("kw", 128, BF16), ("cos", (max_pos, 64), BF16), ("sin", (max_pos, 64), BF16),
            ("kc", (n_kv, P, 128), BF16), ("vc", (n_kv, P, 128), BF16), ("af", Pp * qd, BF16), ("wo", Hd * qd, BF16),
            ("h", (Pp, Hd + 8), BF16), ("tap", (P, Hd + 8), BF16), ("wgu", 2 * I * Hd, BF16), ("act", Pp * I, BF16)]

    def make(c, which):
        c.rows.copy_(rows0), c.nw.copy_(nw0), c.wqkv.copy_(wqkv0), c.qw.copy_(qw0), c.kw.copy_(kw0), c.cos.copy_(cos0)
        c.sin.copy_(sin0), c.wo.copy_(wo0), c.wgu.copy_(wgu0), c.h.copy_(h0)
        A.poison(c.rows, (slice(None), slice(Hd, None)), which)
        c.xf.fill_(float("nan")), c.xp.fill_(float("nan")), c.qkv.fill_(-7.0), c.kc.fill_(-7.0), c.vc.fill_(-7.0)
        c.af.zero_()                                              # the padding tiles of a GEMM operand hold zero fragments
        c.tap.fill_(-7.0), c.act.fill_(-7.0)

    def launch(t):
        ops.prefill_pack_rows(t.rows[:, :Hd], P, Hd, t.xp)
        ops.prefill_norm_pack(t.rows[:, :Hd], P, Hd, t.nw, 1e-6, t.xf)
        ops.prefill_gemm_rows(t.wqkv, t.xf, P, N, Hd, t.qkv)
        ops.prefill_qk_rope(t.qkv, P, 0, qd, qd + n_kv * 128, n_q, n_kv, t.qw, t.kw, 1e-6, t.cos, t.sin, pos0, t.kc, t.vc, 0)
        ops.prefill_attn(t.qkv, P, 0, t.kc, t.vc, n_q, n_kv, 128 ** -0.5, t.af)
        ops.prefill_gemm_resid(t.wo, t.af, P, Hd, qd, t.h[:, :Hd], tap=t.tap[:, :Hd])
        ops.prefill_gemm_silu(t.wgu, t.xp, P, I, Hd, t.act)
    c, res = B.check_launch(N, plan, make, launch, ["xf", "xp", "qkv", "kc", "vc", "af", "h", "tap", "act"])
    assert torch.equal(H.unpack_tiles(res["xp"], P, Hd), rows0[:, :Hd])
    assert torch.count_nonzero(H.unpack_tiles(res["xp"], Pp, Hd)[P:].float()) == 0       # every padded tile written: zeros
    assert torch.count_nonzero(H.unpack_tiles(res["xf"], Pp, Hd)[P:].float()) == 0
    assert torch.all(res["qkv"][P:] == -7.0) and torch.isfinite(res["qkv"][:P].float()).all()        # rows >= P never stored
    assert torch.equal(res["h"][P:], h0[P:]) and torch.equal(res["h"][:, Hd:], h0[:, Hd:])
    assert torch.equal(res["tap"][:, :Hd], res["h"][:P, :Hd]) and torch.all(res["tap"][:, Hd:] == -7.0)
    assert torch.isfinite(res["kc"].float()).all() and torch.all(res["kc"] != -7.0)
    v = res["qkv"][:P, qd + n_kv * 128:].reshape(P, n_kv, 128).transpose(0, 1)
    assert torch.equal(res["vc"], v)
    lin = H.unpack_tiles(res["xf"], P, Hd).float() @ wqkv0.view(N // 16, Hd // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(N, Hd).float().T
    H.assert_close("prefill gemm_rows bounds (v columns)", res["qkv"][:P, qd + n_kv * 128:], lin[:, qd + n_kv * 128:], max_rel=2e-2, mean_rel=2e-3)
    act = H.unpack_tiles(res["act"], Pp, I)
    assert torch.isfinite(act[:P].float()).all()
