"""Bounds of the attention launches (attn_block.hip, attn_head.hip) and dfl_qknorm_rope_append inside a guarded arena
(tests/arena.py, tests/bounds_common.py: W, R, S).

Exact sizes: every workspace at its *_ws_bytes (n_cand / R times the per-block figure for the candidate and batch forms,
DFL_ATTN_OPROJ_SYNC_WORDS for the o_proj tail's sync words), caches of exactly cache_rows rows with the appended rows
ending on the last one, rotation tables of exactly max_pos rows with the last new row at position max_pos - 1 or past it
(clamped: "no read past the tables").  Don't-care regions under both patterns: cache rows at or past the key count, table
rows past the last position used, Linear rows at or past bs / tau, the split partials of every workspace (only the
arrival tickets are zeroed, as the header asks).

Key counts: S = 0, 32, 31, 33, and one count above the split threshold of the case's max_splits, where the old-key splits
reach max_splits - 1 and the workspace is used to its last split (attn_keys_ref.head_form is the host rule).
Values: fp32 softmax attention over the oracle's RMSNorm + RoPE, at the bars of test_hip_batch_kernels.py."""
import pytest
import torch

import arena as A
import attn_keys_ref as KR
import bounds_common as B
import helpers as H
import test_hip_batch_kernels as BK

gpu = pytest.mark.gpu
BF16, F32, I32, I64, U8 = B.BF16, B.F32, B.I32, B.I64, B.U8
N_Q, N_KV = 4, 2
QD, KD = N_Q * 128, N_KV * 128
LD = QD + 2 * KD
SCALE = 128 ** -0.5

COVERS = {
    "dfl_attn_head": "test_attn_head_bounds",
    "dfl_attn_head_oproj": "test_attn_head_oproj_bounds",
    "dfl_attn_head_cand": "test_attn_head_cand_bounds",
    "dfl_attn_head_batch": "test_attn_batch_bounds",
    "dfl_attn_head_batch_f32": "test_attn_batch_bounds",
    "dfl_attn_fused_batch": "test_attn_batch_bounds",
    "dfl_attn_fused": "test_attn_fused_bounds",
    "dfl_block_attn": "test_qknorm_rope_append_and_block_attn_bounds",
    "dfl_qknorm_rope_append": "test_qknorm_rope_append_and_block_attn_bounds",
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def test_attn_bounds_cases_fill_the_last_split():
    """(no GPU) 769 cached keys at max_splits = 4: 25 tiles want 4 old-key splits, the workspace allows 3 = max_splits - 1,
    on the head, the two-tile and the o_proj kernels."""
    assert KR.head_form(N_Q, N_KV, 769, 16, 4)["ns"] == 3 and -(-25 // 8) == 4
    assert KR.head_form(N_Q, N_KV, 769, 32, 4, q_tiles=2) == dict(kernel="head2", ns=3, tiles_per_wave=2)
    assert KR.head_form(N_Q, N_KV, 769, 16, 4, oproj=True)["ns"] == 3
    assert KR.head_form(N_Q, N_KV, 32, 16, 4)["ns"] == 1 and KR.head_form(N_Q, N_KV, 0, 16, 4)["ns"] == 0
    # the pair kernel needs more tiles than 8 x the workgroup budget: 4 candidates from 3841 keys, 3 requests from 5121
    assert KR.head_form(N_Q, N_KV, 3900, 16, 4, n_cand=4) == dict(kernel="pair", ns=3, tiles_per_wave=6)
    assert KR.head_form(N_Q, N_KV, 5200, 16, 4, n_cand=3, dyn=True)["kernel"] == "pair"
    assert KR.head_form(N_Q, N_KV, 769, 16, 4, n_cand=4)["kernel"] == "head1"


# ---------------------------------------------------------------- the reference
def _norm_rope(x, w, positions, max_pos):
    """x [rows, heads, 128] bf16 (CPU) -> [heads, rows, 128]: the oracle's RMSNorm + RoPE, row i at min(position, max_pos - 1)."""
    return torch.cat([BK._rope_ref(x[i:i + 1], w, min(int(p), max_pos - 1)) for i, p in enumerate(positions)], dim=1)


def _reference(blk, ctx, kc0, vc0, S, tau, bs, pos0, causal, qw, kw, max_pos):
    """blk [>= bs, LD], ctx [>= tau, LD] bf16 Linear rows (q | k | v), kc0 / vc0 [N_KV, rows, 128]: (out fp32 [bs, N_Q, 128],
    the new K rows bf16 [N_KV, tau + bs, 128], the new V rows)."""
    blk, ctx = blk[:bs].cpu(), (ctx[:tau].cpu() if tau else blk[:0].cpu())
    new = torch.cat([ctx, blk])
    pos = [pos0 + i for i in range(tau + bs)]
    q = _norm_rope(blk[:, :QD].reshape(bs, N_Q, 128), qw.cpu(), pos[tau:], max_pos)
    k = _norm_rope(new[:, QD:QD + KD].reshape(tau + bs, N_KV, 128), kw.cpu(), pos, max_pos)
    v = new[:, QD + KD:].reshape(tau + bs, N_KV, 128).transpose(0, 1).contiguous()
    G = N_Q // N_KV
    keys = torch.cat([kc0[:, :S].cpu(), k], dim=1).float().repeat_interleave(G, dim=0)
    vals = torch.cat([vc0[:, :S].cpu(), v], dim=1).float().repeat_interleave(G, dim=0)
    sc = torch.einsum("hqd,hkd->hqk", q.float(), keys) * SCALE
    vis = KR.decode_visibility(S, tau, bs, causal)
    sc = sc.masked_fill(~vis[None], float("-inf"))
    return torch.einsum("hqk,hkd->qhd", torch.softmax(sc, dim=-1), vals), k, v


class _Data:
    """Random operands of one block on one cache, kept outside the arena and copied in by fill()."""

    def __init__(self, seed, rows, max_pos, qt=1):
        g = B.cuda_gen(seed)
        rn = lambda *s: torch.randn(*s, generator=g, device=B.dev())      # noqa: E731
        self.blk, self.ctx = rn(16 * qt, LD).to(BF16), rn(32, LD).to(BF16)
        self.kc0, self.vc0 = rn(N_KV, rows, 128).to(BF16), rn(N_KV, rows, 128).to(BF16)
        self.qw, self.kw = (1 + 0.1 * rn(128)).to(BF16), (1 + 0.1 * rn(128)).to(BF16)
        from dflash_amd.model import _rope_tables
        self.cos, self.sin = _rope_tables(128, 1e6, max_pos, B.dev())


def _fill_common(c, d, which, S, tau, bs, last_pos):
    """Caches (rows at or past S: the pattern), tables (rows past the last position used: the pattern), norm weights."""
    c.kc.copy_(d.kc0), c.vc.copy_(d.vc0), c.cos.copy_(d.cos), c.sin.copy_(d.sin), c.qw.copy_(d.qw), c.kw.copy_(d.kw)
    A.poison(c.kc, (slice(None), slice(S, None)), which)
    A.poison(c.vc, (slice(None), slice(S, None)), which)
    A.poison(c.cos, slice(last_pos + 1, None), which)
    A.poison(c.sin, slice(last_pos + 1, None), which)


def _head_ws_fill(ws, which, n_q, ms, qt, n_blocks=1):
    """dfl_attn_head's workspace, per block: [rows * 130 floats of partials | n_q tickets | pad]: the partials hold the
    pattern, the tickets zero."""
    per = ws.numel() // n_blocks
    part = ms * n_q * qt * 16 * 130 * 4
    v = ws.view(n_blocks, per)
    A.poison(v, (slice(None), slice(0, part)), which, kind="bytes")
    v[:, part:].zero_()


def _check_new_rows(res, d, S, n_new, k, v, name):
    """W on the caches: the appended rows (V bit-exact, K at the RoPE bar), every other row as it was filled."""
    assert torch.equal(res["vc"][:, S:S + n_new].cpu(), v[:, :n_new]), name
    BK._assert_rope_bar(f"{name} K rows", res["kc"][:, S:S + n_new].cpu(), k[:, :n_new])


def _cache_plan(rows, max_pos):
    return [("kc", (N_KV, rows, 128), BF16), ("vc", (N_KV, rows, 128), BF16), ("cos", (max_pos, 64), BF16),
            ("sin", (max_pos, 64), BF16), ("qw", 128, BF16), ("kw", 128, BF16)]


# ---------------------------------------------------------------- dfl_attn_head
# (S, tau, bs, q_tiles, dyn bound or None, causal, position of the last new row relative to max_pos - 1)
HEAD = [(0, 3, 16, 1, None, False, 0), (32, 0, 16, 1, None, True, -5), (31, 5, 11, 1, 31, False, 2), (33, 0, 16, 1, 40, True, 0),
        (769, 16, 16, 1, None, False, 0), (769, 0, 16, 1, 769, True, 3), (33, 32, 32, 2, None, False, 0),
        (769, 0, 17, 2, 769, True, -1), (0, 0, 16, 1, 64, True, 0)]


@gpu
@pytest.mark.parametrize("S,tau,bs,qt,bound,causal,over", HEAD,
                         ids=[f"S{S}-tau{t}-bs{b}-qt{q}-{'imm' if bd is None else f'dyn{bd}'}-{'causal' if c else 'full'}-pos{o:+d}"
                              f"-{KR.head_form_id(N_Q, N_KV, S if bd is None else bd, b, 4, q_tiles=q, dyn=bd is not None)}"
                              for S, t, b, q, bd, c, o in HEAD])
def test_attn_head_bounds(ops, S, tau, bs, qt, bound, causal, over):
    """dfl_attn_head at max_splits = 4: the cache is exactly S + tau + bs rows (the appended rows end on its last row), the
    tables exactly max_pos rows, ws exactly dfl_attn_head_ws_bytes(n_q, 4, q_tiles)."""
    ms, n_new = 4, tau + bs
    rows = (S if bound is None else max(S, bound)) + n_new
    pos0 = 50
    max_pos = pos0 + n_new - over           # the last new row sits at max_pos - 1 + over
    d = _Data(S + tau + bs, rows, max_pos, qt)
    wsb = ops.lib().dfl_attn_head_ws_bytes(N_Q, ms, qt)
    c = B.Case(LD, _cache_plan(rows, max_pos) + [("xq", (16 * qt, LD), BF16), ("xc", (32, LD), BF16),
                                                 ("out", (qt, 16 * QD), BF16), ("ws", wsb, U8, "bytes"),
                                                 ("dyn", 8, I32, "index")])

    def make(which):
        _fill_common(c, d, which, S, tau, bs, min(pos0 + n_new - 1, max_pos - 1))
        c.xq.copy_(d.blk), c.xc.copy_(d.ctx)
        A.poison(c.xq, slice(bs, None), which)
        A.poison(c.xc, slice(tau, None), which)
        c.out.fill_(float("nan"))
        c.dyn.copy_(torch.tensor([S, tau, bs, pos0, pos0 + tau, 0, 0, 0], dtype=I32))
        _head_ws_fill(c.ws, which, N_Q, ms, qt)

    def launch_with(ws):
        ops.attn_head(xq=c.xq, q_col=0, k_col=QD, v_col=QD + KD, xc=c.xc if tau else None, ck_col=QD, cv_col=QD + KD, n_q=N_Q,
                      n_kv=N_KV, q_norm_w=c.qw, k_norm_w=c.kw, eps=1e-6, cos_tab=c.cos, sin_tab=c.sin, kcache=c.kc, vcache=c.vc,
                      scale=SCALE, causal=causal, S=S if bound is None else bound, tau=tau, bs=bs, pos0=pos0,
                      dyn=None if bound is None else c.dyn, ws=ws, max_splits=ms, out_frag=c.out, q_tiles=qt,
                      out_tile_stride=16 * QD if qt == 2 else 0)
    # rows of the output at or past bs, and cache rows the launch does not append, are compared as filled
    outs = lambda: {"out": c.out, "kc": c.kc[:, :S + n_new], "vc": c.vc[:, :S + n_new]}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs, finite=False)
    assert int(c.ws[ms * N_Q * qt * 16 * 130 * 4:].to(I32).sum()) == 0, "tickets not left at zero"
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    ref, k, v = _reference(d.blk, d.ctx, d.kc0, d.vc0, S, tau, bs, pos0, causal, d.qw, d.kw, max_pos)
    got = torch.cat([H.unfrag(t, QD) for t in res["out"]])[:bs].view(bs, N_Q, 128)
    assert torch.isfinite(got.float()).all()
    H.assert_close("attn_head bounds out", got, ref, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
    _check_new_rows(res, d, S, n_new, k, v, "attn_head bounds")
    assert torch.equal(res["kc"][:, :S], d.kc0[:, :S]) and torch.equal(res["vc"][:, :S], d.vc0[:, :S])
    if bound is not None and bound > S:      # the rows between the record's end and the bound's: never stored to
        tail = torch.cat([c.kc[:, S + n_new:], c.vc[:, S + n_new:]])
        assert torch.all(tail.view(torch.int16) == A.pattern_scalar(BF16, "float", "A"))      # (the last fill)


# ---------------------------------------------------------------- dfl_attn_head_oproj
@gpu
@pytest.mark.parametrize("S,tau,causal", [(0, 3, False), (33, 0, True), (769, 16, False)],
                         ids=lambda v: str(v))
def test_attn_head_oproj_bounds(ops, S, tau, causal):
    """dfl_attn_head_oproj: sync at exactly DFL_ATTN_OPROJ_SYNC_WORDS words (zeroed, left zero), h_io with a row stride
    above H, ss_out of exactly H floats, the o_proj weight at exactly H * q_dim elements."""
    ms, bs, Hd = 4, 11, 272
    n_new, pos0 = tau + bs, 7
    rows, max_pos, ldh = S + n_new, pos0 + n_new, Hd + 24
    d = _Data(S + tau, rows, max_pos)
    wo = B.small_ints((Hd, QD), S + 1) * 2 ** -5
    wp0 = ops.pack_weight(wo)
    h0 = (torch.randn(16, ldh, generator=B.cuda_gen(S), device=B.dev())).to(BF16)
    c = B.Case(LD, _cache_plan(rows, max_pos) + [("xq", (16, LD), BF16), ("xc", (32, LD), BF16), ("out", 16 * QD, BF16),
                                                 ("ws", ops.lib().dfl_attn_head_ws_bytes(N_Q, ms, 1), U8, "bytes"),
                                                 ("wo", Hd * QD, BF16), ("h", (16, ldh), BF16), ("ss", Hd, F32),
                                                 ("sync", ops.ATTN_OPROJ_SYNC_WORDS, I32, "index")])

    def make(which):
        _fill_common(c, d, which, S, tau, bs, max_pos - 1)
        c.xq.copy_(d.blk), c.xc.copy_(d.ctx), c.wo.copy_(wp0), c.h.copy_(h0)
        A.poison(c.xq, slice(bs, None), which)
        A.poison(c.xc, slice(tau, None), which)
        c.out.fill_(float("nan")), c.ss.fill_(float("nan"))
        c.sync.zero_()
        _head_ws_fill(c.ws, which, N_Q, ms, 1)

    def launch_with(ws):
        ops.attn_head_oproj(xq=c.xq, q_col=0, k_col=QD, v_col=QD + KD, xc=c.xc if tau else None, ck_col=QD, cv_col=QD + KD,
                            n_q=N_Q, n_kv=N_KV, q_norm_w=c.qw, k_norm_w=c.kw, eps=1e-6, cos_tab=c.cos, sin_tab=c.sin,
                            kcache=c.kc, vcache=c.vc, scale=SCALE, causal=causal, S=S, tau=tau, bs=bs, pos0=pos0, ws=ws,
                            max_splits=ms, attn_frag=c.out, wo=c.wo, H=Hd, h_io=c.h, ss_out=c.ss, sync=c.sync)
    outs = lambda: {"out": c.out, "h": c.h, "ss": c.ss, "kc": c.kc, "vc": c.vc, "sync": c.sync}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs, finite=False)
    assert int(res["sync"].abs().sum()) == 0
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    ref, k, v = _reference(d.blk, d.ctx, d.kc0, d.vc0, S, tau, bs, pos0, causal, d.qw, d.kw, max_pos)
    attn = H.unfrag(res["out"], QD)
    H.assert_close("attn_head_oproj bounds attn", attn[:bs].view(bs, N_Q, 128), ref, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
    assert torch.count_nonzero(attn[bs:].float()) == 0                   # rows >= bs are written as zeros
    _check_new_rows(res, d, S, n_new, k, v, "attn_head_oproj bounds")
    want = (h0[:, :Hd].float() + (attn.float() @ wo.float().T).to(BF16).float()).to(BF16)
    H.assert_close("attn_head_oproj bounds h", res["h"][:, :Hd], want, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
    assert torch.equal(res["h"][:, Hd:], h0[:, Hd:])


# ---------------------------------------------------------------- dfl_attn_head_cand
@gpu
@pytest.mark.parametrize("S,bs,qt", [(33, 16, 1), (769, 11, 1), (769, 27, 2), (0, 16, 1), (3900, 16, 1)], ids=lambda v: str(v))
def test_attn_head_cand_bounds(ops, S, bs, qt):
    """dfl_attn_head_cand with n_cand = 4: ws exactly 4 x dfl_attn_head_ws_bytes, the staging area exactly
    [4][n_kv][bs][128] (out_rows = bs), the shared cache of exactly S rows and read-only.  The per-candidate strides of
    ws, out, k_out / v_out are all at work; candidates differ, so a stride one block off shows in the values."""
    C, ms, pos_over = 4, 4, 1
    max_pos = S + bs - pos_over              # the last block row rotates past the tables: clamped
    rows = max(S, 1)
    ds = [_Data(100 * cnd + S, rows, max_pos, qt) for cnd in range(C)]
    d = ds[0]
    c = B.Case(LD, _cache_plan(rows, max_pos) + [("xq", (C * qt, 16, LD), BF16), ("out", (C * qt, 16 * QD), BF16),
                                                 ("k_out", (C, N_KV, bs, 128), BF16), ("v_out", (C, N_KV, bs, 128), BF16),
                                                 ("ws", C * ops.lib().dfl_attn_head_ws_bytes(N_Q, ms, qt), U8, "bytes")])

    def make(which):
        _fill_common(c, d, which, S, 0, bs, max_pos - 1)
        for cnd in range(C):
            c.xq[cnd * qt:(cnd + 1) * qt].copy_(ds[cnd].blk.view(qt, 16, LD))
        A.poison(c.xq.view(C, qt * 16, LD), (slice(None), slice(bs, None)), which)
        c.out.fill_(float("nan")), c.k_out.fill_(float("nan")), c.v_out.fill_(float("nan"))
        _head_ws_fill(c.ws, which, N_Q, ms, qt, n_blocks=C)

    def launch_with(ws):
        ops.attn_head_cand(xq=c.xq, q_col=0, k_col=QD, v_col=QD + KD, n_q=N_Q, n_kv=N_KV, q_norm_w=c.qw, k_norm_w=c.kw, eps=1e-6,
                           cos_tab=c.cos, sin_tab=c.sin, kcache=c.kc, vcache=c.vc, scale=SCALE, S=S, bs=bs, ws=ws,
                           max_splits=ms, out_frag=c.out, k_out=c.k_out, v_out=c.v_out, q_tiles=qt)
    outs = lambda: {"out": c.out, "k_out": c.k_out, "v_out": c.v_out, "kc": c.kc[:, :S], "vc": c.vc[:, :S]}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs, finite=False)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    assert torch.equal(res["kc"], d.kc0[:, :S]) and torch.equal(res["vc"], d.vc0[:, :S])
    for cnd in range(C):
        ref, k, v = _reference(ds[cnd].blk, None, d.kc0, d.vc0, S, 0, bs, S, True, d.qw, d.kw, max_pos)
        got = torch.cat([H.unfrag(t, QD) for t in res["out"][cnd * qt:(cnd + 1) * qt]])[:bs].view(bs, N_Q, 128)
        H.assert_close(f"attn_head_cand bounds c{cnd}", got, ref, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
        assert torch.equal(res["v_out"][cnd].cpu(), v), cnd
        BK._assert_rope_bar(f"attn_head_cand bounds K c{cnd}", res["k_out"][cnd].cpu(), k)


# ---------------------------------------------------------------- the ragged-batch forms
# (form, lens, bss, q_tiles): R = 3 requests, buffers of exactly 3; 5200 keys put the f32 case on the pair kernel
BATCH = [("f32", (33, 0, 5200), (16, 5, 16), 1), ("bf16", (32, 769, 31), (16, 7, 16), 1), ("bf16", (33, 769, 0), (17, 32, 25), 2),
         ("fused", (33, 0, 769), (16, 5, 12), 1)]


@gpu
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("form,lens,bss,qt", BATCH, ids=[f"{f}-S{'_'.join(map(str, ln))}-qt{q}" for f, ln, _, q in BATCH])
def test_attn_batch_bounds(ops, form, lens, bss, qt, causal):
    """dfl_attn_head_batch_f32 / dfl_attn_head_batch / dfl_attn_fused_batch: ws of exactly R x the per-request figure (the
    fused form: dfl_attn_fused_batch_ws_bytes(R, ...)), caches [R][L = 1][n_kv][rows][128] where the longest request's new
    rows end on its last row, records and outputs of exactly R requests."""
    R, ms = len(lens), 4
    rows = max(s + b for s, b in zip(lens, bss))
    max_pos = rows                           # the longest request's last row sits at max_pos - 1
    nparts = 2 if form != "bf16" else 1
    ds = [_Data(10 * r + lens[r] + qt, rows, max_pos, qt) for r in range(R)]
    lib = ops.lib()
    wsb = (lib.dfl_attn_fused_batch_ws_bytes(R, N_Q, N_KV, ms) if form == "fused" else R * lib.dfl_attn_head_ws_bytes(N_Q, ms, qt))
    xplan = [("xq", (R * qt, 16, LD), BF16)] if form == "bf16" else [("parts", (nparts, R * 16, LD), F32)]
    c = B.Case(LD, [("kc", (R, 1, N_KV, rows, 128), BF16), ("vc", (R, 1, N_KV, rows, 128), BF16), ("cos", (max_pos, 64), BF16),
                    ("sin", (max_pos, 64), BF16), ("qw", 128, BF16), ("kw", 128, BF16), ("out", (R * qt, 16 * QD), BF16),
                    ("ws", wsb, U8, "bytes"), ("dyn", (R, 8), I32, "index")] + xplan)
    g = B.cuda_gen(sum(lens))
    split = [torch.randn(R * 16, LD, generator=g, device=B.dev()) for _ in range(nparts - 1)]
    d0 = ds[0]

    def make(which):
        c.cos.copy_(d0.cos), c.sin.copy_(d0.sin), c.qw.copy_(d0.qw), c.kw.copy_(d0.kw)
        c.dyn.zero_()
        for r in range(R):
            c.kc[r, 0].copy_(ds[r].kc0), c.vc[r, 0].copy_(ds[r].vc0)
            A.poison(c.kc, (r, 0, slice(None), slice(lens[r], None)), which)
            A.poison(c.vc, (r, 0, slice(None), slice(lens[r], None)), which)
            c.dyn[r, 0], c.dyn[r, 2], c.dyn[r, 3], c.dyn[r, 4] = lens[r], bss[r], lens[r], lens[r]
            if form == "bf16":
                c.xq[r * qt:(r + 1) * qt].copy_(ds[r].blk.view(qt, 16, LD))
                A.poison(c.xq.view(R, qt * 16, LD), (r, slice(bss[r], None)), which)
            else:     # fp32 parts whose bf16 sum is the Linear row: part 1 random, part 0 the rest (bf16(p0 + p1) == row)
                rowsl = slice(r * 16, r * 16 + 16)
                if nparts == 2:
                    c.parts[1, rowsl].copy_(split[0][rowsl])
                    c.parts[0, rowsl].copy_(ds[r].blk.float() - split[0][rowsl])
                else:
                    c.parts[0, rowsl].copy_(ds[r].blk.float())
                A.poison(c.parts, (slice(None), slice(r * 16 + bss[r], r * 16 + 16)), which)
        c.out.fill_(float("nan"))
        if form == "fused":
            tk = R * lib.dfl_attn_ws_bytes(N_Q, ms)
            A.poison(c.ws, slice(0, tk), which, kind="bytes")
            c.ws[tk:].zero_()
        else:
            _head_ws_fill(c.ws, which, N_Q, ms, qt, n_blocks=R)

    def launch_with(ws):
        common = dict(q_col=0, k_col=QD, v_col=QD + KD, R=R, n_q=N_Q, n_kv=N_KV, q_norm_w=c.qw, k_norm_w=c.kw, eps=1e-6,
                      cos_tab=c.cos, sin_tab=c.sin, kcache=c.kc, vcache=c.vc, layer=0, scale=SCALE, causal=causal, dyn=c.dyn,
                      kv_len_max=rows, ws=ws, max_splits=ms, out_frag=c.out)
        if form == "f32":
            ops.attn_head_batch_f32(qkv_parts=c.parts, nparts=nparts, MT=R, ld=LD, **common)
        elif form == "bf16":
            ops.attn_head_batch(xq=c.xq, q_tiles=qt, **common)
        else:
            ops.attn_fused_batch(qkv=c.parts, nsplit=nparts, split_stride=R * 16 * LD, ld=LD, **common)
    outs = lambda: {"out": c.out, **{f"kc{r}": c.kc[r, 0, :, :lens[r] + bss[r]] for r in range(R)},      # noqa: E731
                    **{f"vc{r}": c.vc[r, 0, :, :lens[r] + bss[r]] for r in range(R)}}
    res = c.run(make, lambda: launch_with(c.ws), outs, finite=False)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    for r in range(R):
        S, bs = lens[r], bss[r]
        if form == "bf16":
            blk = ds[r].blk
        else:      # what the kernel sees: bf16(part 0 + part 1)
            blk = ((ds[r].blk.float() - split[0][r * 16:r * 16 + 16]) + split[0][r * 16:r * 16 + 16]).to(BF16) if nparts == 2 else ds[r].blk
        ref, k, v = _reference(blk, None, ds[r].kc0, ds[r].vc0, S, 0, bs, S, causal, d0.qw, d0.kw, max_pos)
        got = torch.cat([H.unfrag(t, QD) for t in res["out"][r * qt:(r + 1) * qt]])[:bs].view(bs, N_Q, 128)
        assert torch.isfinite(got.float()).all(), r
        H.assert_close(f"attn batch bounds {form} r{r}", got, ref, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
        assert torch.equal(res[f"vc{r}"][:, S:].cpu(), v), r
        BK._assert_rope_bar(f"attn batch bounds {form} K r{r}", res[f"kc{r}"][:, S:].cpu(), k)
        assert torch.equal(res[f"kc{r}"][:, :S], ds[r].kc0[:, :S]) and torch.equal(res[f"vc{r}"][:, :S], ds[r].vc0[:, :S]), r
        tail = torch.cat([c.kc[r, 0, :, S + bs:], c.vc[r, 0, :, S + bs:]])
        assert torch.all(tail.view(torch.int16) == A.pattern_scalar(BF16, "float", "A")), f"r{r}: rows past the new ones written"


# ---------------------------------------------------------------- dfl_attn_fused
@gpu
@pytest.mark.parametrize("S,tau,bs,causal,over", [(0, 3, 16, False, 0), (33, 0, 11, True, 2), (769, 16, 16, False, 0),
                                                  (40, 5, 16, True, 0)], ids=lambda v: str(v))
def test_attn_fused_bounds(ops, S, tau, bs, causal, over):
    """dfl_attn_fused at max_splits = 2 (every case with more than 64 keys uses both splits): ws at exactly
    dfl_attn_fused_ws_bytes, the partial buffer exactly [2][32][ld], the cache exactly S + tau + bs rows."""
    ms, n_new, pos0 = 2, tau + bs, 9
    rows, max_pos = S + n_new, pos0 + n_new - over
    d = _Data(S + tau + 3, rows, max_pos)
    lin = torch.cat([d.ctx[:16], d.blk])
    p1 = torch.randn(32, LD, generator=B.cuda_gen(S), device=B.dev())
    c = B.Case(LD, _cache_plan(rows, max_pos) + [("parts", (2, 32, LD), F32), ("out", 16 * QD, BF16), ("dyn", 8, I32, "index"),
                                                 ("ws", ops.lib().dfl_attn_fused_ws_bytes(N_Q, N_KV, ms), U8, "bytes")])
    tk = ops.lib().dfl_attn_ws_bytes(N_Q, ms)

    def make(which):
        _fill_common(c, d, which, S, tau, bs, min(pos0 + n_new - 1, max_pos - 1))
        c.parts[1].copy_(p1), c.parts[0].copy_(lin.float() - p1)
        A.poison(c.parts, [(slice(None), slice(tau, 16)), (slice(None), slice(16 + bs, 32))], which)
        c.out.fill_(float("nan"))
        c.dyn.copy_(torch.tensor([S, tau, bs, pos0, pos0 + tau, 0, 0, 0], dtype=I32))
        A.poison(c.ws, slice(0, tk), which, kind="bytes")
        c.ws[tk:].zero_()

    def launch_with(ws):
        ops.attn_fused(qkv=c.parts, nsplit=2, split_stride=32 * LD, ld=LD, q_col=0, k_col=QD, v_col=QD + KD, ctx_row0=0,
                       blk_row0=16, n_q=N_Q, n_kv=N_KV, q_norm_w=c.qw, k_norm_w=c.kw, eps=1e-6, cos_tab=c.cos, sin_tab=c.sin,
                       kcache=c.kc, vcache=c.vc, scale=SCALE, dyn=c.dyn, kv_len_max=rows, ws=ws, max_splits=ms, out_frag=c.out,
                       causal=causal)
    outs = lambda: {"out": c.out, "kc": c.kc, "vc": c.vc}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs, finite=False)
    assert int(c.ws[tk:].to(I32).sum()) == 0, "tickets not left at zero"
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    seen = ((lin.float() - p1) + p1).to(BF16)
    ref, k, v = _reference(seen[16:], seen[:16], d.kc0, d.vc0, S, tau, bs, pos0, causal, d.qw, d.kw, max_pos)
    got = H.unfrag(res["out"], QD)[:bs].view(bs, N_Q, 128)
    H.assert_close("attn_fused bounds out", got, ref, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
    _check_new_rows(res, d, S, n_new, k, v, "attn_fused bounds")
    assert torch.equal(res["kc"][:, :S], d.kc0[:, :S]) and torch.equal(res["vc"][:, :S], d.vc0[:, :S])


# ---------------------------------------------------------------- dfl_qknorm_rope_append + dfl_block_attn
@gpu
@pytest.mark.parametrize("S,tau,bs,causal,long_by", [(0, 3, 16, False, 0), (33, 0, 11, True, 1), (769, 16, 16, False, 0),
                                                     (31, 5, 16, True, 1)], ids=lambda v: str(v))
def test_qknorm_rope_append_and_block_attn_bounds(ops, S, tau, bs, causal, long_by):
    """dfl_qknorm_rope_append into caches of exactly cache_rows rows — with long_by = 1 the block is ONE ROW TOO LONG for
    the cache: that row "is silently not stored" (the guard behind the last head's rows, and the first row of the next
    head, keep their bits; q_out is still written) — and tables of exactly max_pos rows whose last row serves the rows
    at or past max_pos.  Then dfl_block_attn over the rows that fit, ws at exactly dfl_attn_ws_bytes(n_q, 2)."""
    ms, n_new, pos0 = 2, tau + bs, 21
    rows = S + n_new - long_by
    max_pos = pos0 + n_new - 2               # the last two new rows rotate with the last table row
    d = _Data(S + bs, rows, max_pos)
    lin = torch.cat([d.ctx[:16], d.blk])
    p1 = torch.randn(32, LD, generator=B.cuda_gen(S + 1), device=B.dev())
    c = B.Case(LD, _cache_plan(rows, max_pos) + [("parts", (2, 32, LD), F32), ("q", (N_Q, 16, 128), BF16), ("out", 16 * QD, BF16),
                                                 ("dyn", 8, I32, "index"), ("dyn2", 8, I32, "index"),
                                                 ("ws", ops.lib().dfl_attn_ws_bytes(N_Q, ms), U8, "bytes")])
    bs_fit = bs - long_by                    # block rows that have a cache row

    def make(which):
        _fill_common(c, d, which, S, tau, bs, max_pos - 1)
        c.parts[1].copy_(p1), c.parts[0].copy_(lin.float() - p1)
        A.poison(c.parts, [(slice(None), slice(tau, 16)), (slice(None), slice(16 + bs, 32))], which)
        c.q.fill_(float("nan")), c.out.fill_(float("nan"))
        c.dyn.copy_(torch.tensor([S, tau, bs, pos0, pos0 + tau, 0, 0, 0], dtype=I32))
        c.dyn2.copy_(torch.tensor([S, tau, bs_fit, pos0, pos0 + tau, 0, 0, 0], dtype=I32))
        A.poison(c.ws, slice(None), which, kind="bytes")          # dfl_block_attn's workspace needs no zeroing

    def launch_with(ws):
        ops.qknorm_rope_append(qkv=c.parts, nsplit=2, split_stride=32 * LD, ld=LD, q_col=0, k_col=QD, v_col=QD + KD, ctx_row0=0,
                               blk_row0=16, n_q=N_Q, n_kv=N_KV, q_norm_w=c.qw, k_norm_w=c.kw, eps=1e-6, cos_tab=c.cos,
                               sin_tab=c.sin, q_out=c.q, kcache=c.kc, vcache=c.vc, dyn=c.dyn)
        ops.block_attn(q=c.q, kcache=c.kc, vcache=c.vc, n_q=N_Q, n_kv=N_KV, scale=SCALE, dyn=c.dyn2, kv_len_max=rows, ws=ws,
                       max_splits=ms, out_frag=c.out, causal=causal)
    outs = lambda: {"q": c.q[:, :bs], "out": c.out, "kc": c.kc, "vc": c.vc}      # noqa: E731
    res = c.run(make, lambda: launch_with(c.ws), outs, finite=False)
    c.same_on_big_workspaces(make, launch_with, ["ws"], outs, res)
    seen = ((lin.float() - p1) + p1).to(BF16)
    ref, k, v = _reference(seen[16:], seen[:16], d.kc0, d.vc0, S, tau, bs_fit, pos0, causal, d.qw, d.kw, max_pos)
    _check_new_rows(res, d, S, n_new - long_by, k, v, "qknorm_rope_append bounds")
    assert torch.equal(res["kc"][:, :S], d.kc0[:, :S]) and torch.equal(res["vc"][:, :S], d.vc0[:, :S])
    qref = _norm_rope(seen[16:16 + bs, :QD].cpu().reshape(bs, N_Q, 128), d.qw.cpu(), [pos0 + tau + j for j in range(bs)], max_pos)
    BK._assert_rope_bar("qknorm_rope_append bounds q", res["q"].cpu(), qref)
    got = H.unfrag(res["out"], QD)[:bs_fit].view(bs_fit, N_Q, 128)
    H.assert_close("block_attn bounds out", got, ref, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
