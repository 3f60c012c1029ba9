"""Bounds of dfl_prefill_logprobs (prompt_logprobs.hip) inside a guarded arena (tests/arena.py, tests/bounds_common.py: W,
R, S): x_frag of exactly dfl_prefill_rows_padded(rows) rows, the packed head of exactly V x K, targets and out of exactly
`rows` entries, ws of exactly nsplit x rows_padded x 4 floats — at a V whose last column block is partly masked (its
clamped weight requests end the head's buffer) and rows that leave a partial tile and a partial 128-row block."""
import pytest
import torch

import arena as A
import bounds_common as B

gpu = pytest.mark.gpu
COVERS = {"dfl_prefill_logprobs": "test_prefill_logprobs_bounds"}


@gpu
@pytest.mark.parametrize("rows,V,K", [(17, 4208, 256), (130, 4208, 512)], ids=lambda v: str(v))
def test_prefill_logprobs_bounds(rows, V, K):
    from dflash_amd import ops
    Pp, nsplit = ops.prefill_rows_padded(rows), ops.prefill_logprobs_nsplit(rows, V)
    g = B.cuda_gen(rows)
    x0 = torch.randn(rows, K, generator=g, device=B.dev()).to(B.BF16)
    w0 = ops.pack_weight((torch.randn(V, K, generator=g, device=B.dev()) * 0.05).to(B.BF16))
    tg0 = torch.randint(0, V, (rows,), generator=g, device=B.dev())
    tg0[0], tg0[rows - 1], tg0[1] = V - 1, 0, V                     # the last real column; the first; one outside: NaN
    plan = [("x", (rows, K), B.BF16), ("xf", Pp * K, B.BF16), ("wp", V * K, B.BF16), ("tg", rows, B.I64, "index"),
            ("ws", nsplit * Pp * 4, B.F32), ("out", rows, B.F32)]

    def make(c, which):
        c.x.copy_(x0), c.wp.copy_(w0), c.tg.copy_(tg0)
        c.xf.fill_(float("nan")), c.out.fill_(-7.0)
        A.poison(c.ws, slice(None), which)                         # a workspace "reused" from anything

    def launch(t):
        ops.prefill_pack_rows(t.x, rows, K, t.xf)
        ops.check(ops.lib().dfl_prefill_logprobs(t.wp.data_ptr(), t.xf.data_ptr(), rows, V, K, t.tg.data_ptr(), nsplit,
                                                 t.ws.data_ptr(), t.out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                  "dfl_prefill_logprobs")
    c, res = B.check_launch(K, plan, make, launch, ["out"], ws_names=("ws",))
    out = res["out"]
    assert torch.isnan(out[1]) and torch.isfinite(out[[0] + list(range(2, rows))]).all() and (out[2:] < 0).all()
