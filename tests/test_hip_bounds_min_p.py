"""Bounds of dfl_min_p_rows (min_p.hip) inside a guarded arena (tests/arena.py, tests/bounds_common.py: W, R, S).

The layout of the verify-row cases of test_hip_bounds_rows.py: three tiles [3][16][V] with a row stride of V + 8 (the 8
slack columns hold the pattern), in and out alike; tile 0 full, tile 1 ragged (the row count from its record, row0 = 1),
tile 2 idle.  V = 8200 = 8 * 1025: thread 0 makes a second trip.  The per-slot L and invT arrays and the kept counts have
exactly their sizes.  The launch runs under both guard patterns and once more on ordinary torch allocations holding the
same bytes, whose outputs must be bit-equal (bounds_common.check_launch)."""
import math

import numpy as np
import pytest
import torch

import arena as A
import bounds_common as B
import min_p_ref as MR

gpu = pytest.mark.gpu
BF16, F32, I32 = B.BF16, B.F32, B.I32
BS = 2
T = 3                                   # tiles = request slots
NV = (16, 7, 0)                         # rows per tile (the record's BS word)
V = 8200

COVERS = {
    "dfl_min_p_rows": "test_min_p_rows_bounds",
}


@gpu
def test_min_p_rows_bounds():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops
    lg = (torch.randn(T, 16, V, generator=B.cuda_gen(V), device=B.dev()) * 3).to(BF16)
    L = [float(np.float32(math.log(0.2))), float(np.float32(math.log(0.01))), -1.0]
    invT = [1.25, 0.8, 2.0]
    plan = [("logits", (T, 16, V + 8), BF16), ("out", (T, 16, V + 8), BF16), ("dyn", (T, 8), I32, "index"),
            ("L", T, F32), ("inv_t", T, F32), ("kept", (T, 16), I32, "index")]

    def make(c, which):
        c.logits[:, :, :V].copy_(lg)
        A.poison(c.logits, (slice(None), slice(None), slice(V, None)), which)
        for t in range(T):
            A.poison(c.logits, (t, slice(NV[t], None)), which)
        c.dyn.zero_()
        for t in range(T):
            c.dyn[t, BS] = NV[t]
        c.L.copy_(torch.tensor(L)), c.inv_t.copy_(torch.tensor(invT))
        c.out.fill_(-7.0), c.kept.fill_(-7)

    def launch(t):
        ops.min_p_rows(t.logits[:, :, :V], log_min_p=t.L, inv_t=t.inv_t, out=t.out[:, :, :V], row0=1, nrows=15, dyn=t.dyn,
                       nrows_dyn_word=BS, kept=t.kept, kept_off=1)
    c, res = B.check_launch(V + 8, plan, make, launch, ["out", "kept"])
    bits = lg.view(torch.int16).cpu().numpy().view(np.uint16)
    got = res["out"].contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    for t in range(T):
        hi = 1 + max(NV[t] - 1, 0)
        assert torch.all(res["out"][t, :1] == -7.0) and torch.all(res["out"][t, max(NV[t], 1):] == -7.0), t
        assert torch.all(res["out"][t, :, V:] == -7.0), t
        assert torch.all(res["kept"][t, :1] == -7) and torch.all(res["kept"][t, hi:] == -7), t
        for m in range(1, NV[t]):
            want, kept = MR.process(bits[t, m], L[t], invT[t])
            assert np.array_equal(got[t, m, :V], want) and int(res["kept"][t, m]) == kept and 1 <= kept < V, (t, m)
