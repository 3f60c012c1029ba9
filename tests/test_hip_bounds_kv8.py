"""Bounds of the e4m3 KV cache launches (attn_head_kv8.hip) inside a guarded arena (tests/arena.py, tests/bounds_common.py:
W, R, S): every buffer exactly as large as the header says, the appended rows ending on the cache's last row."""
import pytest
import torch

import arena as A
import attn_keys_ref as KR
import bounds_common as B
import helpers as H

gpu = pytest.mark.gpu
BF16, F32, I32, U8 = B.BF16, B.F32, B.I32, B.U8
N_Q, N_KV = 4, 2
QD, KD = N_Q * 128, N_KV * 128
LD = QD + 2 * KD

COVERS = {"dfl_attn_head_kv8": "test_attn_head_kv8_bounds", "dfl_kv_quant_rows": "test_kv_quant_rows_bounds"}


@gpu
@pytest.mark.parametrize("P,row0", [(1, 0), (17, 3), (33, 0)])
def test_kv_quant_rows_bounds(P, row0):
    """Source rows exactly [n_kv][P][128], codes and scales exactly row0 + P rows."""
    from dflash_amd import ops
    rows = row0 + P
    g = B.cuda_gen(P)
    src = [torch.randn(N_KV, P, 128, generator=g, device=B.dev()).to(BF16) for _ in range(2)]
    plan = [("kr", (N_KV, P, 128), BF16), ("vr", (N_KV, P, 128), BF16), ("kc", (N_KV, rows, 128), U8, "bytes"),
            ("vc", (N_KV, rows, 128), U8, "bytes"), ("ks", (N_KV, rows), F32), ("vs", (N_KV, rows), F32)]

    def make(c, which):
        c.kr.copy_(src[0]), c.vr.copy_(src[1])
        for t in (c.kc, c.vc, c.ks, c.vs):
            A.poison(t, slice(None), which)

    B.check_launch(128, plan, make, lambda t: ops.kv_quant_rows(t.kr, t.vr, P, t.kc, t.vc, t.ks, t.vs, row0),
                            ["kr", "vr", ("kc", lambda t: t.kc[:, row0:]), ("vc", lambda t: t.vc[:, row0:]),
                             ("ks", lambda t: t.ks[:, row0:]), ("vs", lambda t: t.vs[:, row0:])])


# (S, bs, q_tiles, dyn bound or None): S + bs (the bound's: bound + bs) is a multiple of 4 — the cache ends on the last new row
HEAD8 = [(0, 16, 1, None), (32, 16, 1, None), (33, 11, 1, 41), (769, 19, 2, 769), (0, 16, 1, 64)]


@gpu
@pytest.mark.parametrize("S,bs,qt,bound", HEAD8, ids=[f"S{S}-bs{b}-qt{q}-{'imm' if bd is None else f'dyn{bd}'}" for S, b, q, bd in HEAD8])
def test_attn_head_kv8_bounds(S, bs, qt, bound):
    """dfl_attn_head_kv8 at max_splits = 4: codes and scales exactly (bound or S) + bs rows, the tables exactly pos0 + bs
    rows, ws exactly dfl_attn_head_ws_bytes; rows at or past S hold the pattern (the clamped scale loads read some of
    them: nothing of it may reach the result)."""
    from dflash_amd import ops
    ms, pos0 = 4, 50
    rows = (S if bound is None else bound) + bs
    assert rows % 4 == 0
    g = B.cuda_gen(S + bs)
    blk = torch.randn(16 * qt, LD, generator=g, device=B.dev()).to(BF16)
    old = [ops.quantize_kv_rows(torch.randn(N_KV, S, 128, generator=g, device=B.dev()).to(BF16)) for _ in range(2)]
    cos, sin = (t.to(B.dev()) for t in KR.rope_tables_identity(pos0 + bs))
    wsb = ops.lib().dfl_attn_head_ws_bytes(N_Q, ms, qt)
    plan = [("kc", (N_KV, rows, 128), U8, "bytes"), ("vc", (N_KV, rows, 128), U8, "bytes"), ("ks", (N_KV, rows), F32),
            ("vs", (N_KV, rows), F32), ("cos", (pos0 + bs, 64), BF16), ("sin", (pos0 + bs, 64), BF16), ("xq", (16 * qt, LD), BF16),
            ("out", (qt, 16 * QD), BF16), ("ws", wsb, U8, "bytes"), ("dyn", 8, I32, "index")]

    def make(c, which):
        for t, o in ((c.kc, old[0][0]), (c.vc, old[1][0]), (c.ks, old[0][1]), (c.vs, old[1][1])):
            A.poison(t, slice(None), which)
            t[:, :S] = o
        c.cos.copy_(cos), c.sin.copy_(sin), c.xq.copy_(blk)
        A.poison(c.xq, slice(bs, None), which)
        c.out.fill_(float("nan"))
        c.dyn.copy_(torch.tensor([S, 0, bs, pos0, pos0, 0, 0, 0], dtype=I32))
        A.poison(c.ws, slice(0, ms * N_Q * qt * 16 * 130 * 4), which, kind="bytes")
        c.ws[ms * N_Q * qt * 16 * 130 * 4:].zero_()

    def launch(t):
        ops.attn_head_kv8(xq=t.xq, q_col=0, k_col=QD, v_col=QD + KD, n_q=N_Q, n_kv=N_KV, q_norm_w=None, k_norm_w=None, eps=1e-6,
                          cos_tab=t.cos, sin_tab=t.sin, kcache=t.kc, vcache=t.vc, k_scale=t.ks, v_scale=t.vs, scale=KR.SCALE,
                          causal=True, S=S if bound is None else bound, bs=bs, pos0=pos0, dyn=None if bound is None else t.dyn,
                          ws=t.ws, max_splits=ms, out_frag=t.out, q_tiles=qt, out_tile_stride=16 * QD if qt == 2 else 0)

    part = lambda n: (n, lambda t: getattr(t, n)[:, :S + bs])      # noqa: E731
    c, res = B.check_launch(LD, plan, make, launch, ["out", part("kc"), part("vc"), part("ks"), part("vs")], ws_names=("ws",))
    got = torch.cat([H.unfrag(t, QD) for t in res["out"]])[:bs]
    assert torch.isfinite(got.float()).all()
    for i, n in enumerate("kv"):      # (what the appended rows must hold: tests/test_hip_kv8.py)
        assert torch.equal(res[n + "c"][:, :S], old[i][0]) and torch.equal(res[n + "s"][:, :S], old[i][1]), n
