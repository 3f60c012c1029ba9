"""Bounds of dfl_grammar_draft_sample_rows (grammar_draft.hip, the noise form) inside a guarded arena (tests/arena.py,
tests/bounds_common.py: W, R, S).

The layout of test_hip_bounds_min_p.py: three tiles [3][16][V] of logits with a row stride of V + 8 (the 8 slack columns
hold the pattern); tile 0 full, tile 1 ragged (the row count from its record), tile 2 idle.  V = 8200 = 8 * 1025: thread
0 makes a second trip.  The pool is exactly [pool_states][V + 8] int16 and slot 1's grammar ends on its LAST row; the
bias table, the records, base / state, the seeds and the per-slot invT (slot 1 at 0: the plain pick) have exactly their
sizes, a block row exactly 16 ids.  The launch runs under both guard patterns and once more on ordinary torch allocations
holding the same bytes, whose outputs must be bit-equal (bounds_common.check_launch); the ids are the numpy model's."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import arena as A
import bounds_common as B
import couple_draft_ref as CD
import grammar_ref as GR

gpu = pytest.mark.gpu
BF16, F32, I32, I64, I16 = B.BF16, B.F32, B.I32, B.I64, torch.int16
BS, START = 2, 4                        # words of a length record (ops.DYN_BS, ops.DYN_START)
T = 3
NV = (16, 7, 0)
V = 8200
SEEDS = (11, -(1 << 62) + 5, 3)
INV_T = (1.25, 0.0, 2.0)
STARTS = (40, 1039, 7)

COVERS = {
    "dfl_grammar_draft_sample_rows": "test_grammar_draft_sample_rows_bounds",
}


@gpu
def test_grammar_draft_sample_rows_bounds():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops
    assert (ops.DYN_BS, ops.DYN_START) == (BS, START)
    rng = np.random.default_rng(V)
    x = np.stack([GR.case_rows(rng, 16, V) for _ in range(T)])
    pool, bases = 7, (0, 4, -1)
    tab = np.full((pool, V), -1, np.int16)
    tab[0:4] = GR.case_dfa(rng, 4, V, 0.4)
    tab[4:7] = GR.case_dfa(rng, 3, V, 0.4)
    bias = np.where(rng.random((T, V)) < 0.3, -np.inf, rng.standard_normal((T, V))).astype(np.float32)
    blk0 = -7 - np.arange(T * 16, dtype=np.int64).reshape(T, 16)
    state0 = (1, 2, 0)                   # slot 1 starts on the pool's last row
    lg = torch.from_numpy(x.view(np.int16)).to(B.dev()).view(BF16)
    plan = [("logits", (T, 16, V + 8), BF16), ("dyn", (T, 8), I32, "index"), ("table", (pool, V + 8), I16, "index"),
            ("base", T, I32, "index"), ("state", T, I32, "index"), ("bias", (T, V + 8), F32),
            ("block", (T, 16), I64, "index"), ("seeds", T, I64, "index"), ("inv_t", T, F32)]

    def make(c, which):
        c.logits[:, :, :V].copy_(lg)
        A.poison(c.logits, (slice(None), slice(None), slice(V, None)), which)
        for t in range(T):
            A.poison(c.logits, (t, slice(NV[t], None)), which)
        c.dyn.zero_()
        for t in range(T):
            c.dyn[t, BS], c.dyn[t, START] = NV[t], STARTS[t]
        c.table[:, :V].copy_(torch.from_numpy(tab))
        c.table[:, V:].fill_(-1 if which == "A" else 0)
        c.base.copy_(torch.tensor(bases, dtype=I32)), c.state.copy_(torch.tensor(state0, dtype=I32))
        c.bias[:, :V].copy_(torch.from_numpy(bias))
        A.poison(c.bias, (slice(None), slice(V, None)), which)
        c.block.copy_(torch.from_numpy(blk0))
        c.seeds.copy_(torch.tensor(SEEDS, dtype=I64)), c.inv_t.copy_(torch.tensor(INV_T))

    def launch(t):
        st = SimpleNamespace(table=t.table[:, :V], base=t.base, state=t.state, used=pool)
        ops.grammar_draft_sample_rows(t.logits[:, :, :V], st, bias=t.bias[:, :V], block=t.block, dyn=t.dyn,
                                      nrows_dyn_word=BS, seeds=t.seeds, inv_ts=t.inv_t, pos_dyn_word=START)
    c, res = B.check_launch(V + 8, plan, make, launch, ["block", "state"])
    got = res["block"].cpu().numpy()
    assert res["state"].tolist() == list(state0)                              # only read
    for t in range(T):
        want, _, gaps = CD.pick(x[t], NV[t], blk0[t], seed=SEEDS[t], inv_t=np.float32(INV_T[t]), pos0=STARTS[t],
                                pool=tab, base=bases[t], state=state0[t], bias=bias[t])
        assert all(g > 1e-4 for g in gaps), (t, gaps)                         # (the inputs: no pick rests on a logf rounding)
        assert np.array_equal(got[t], want), (t, got[t], want)
        assert got[t, 0] == blk0[t, 0] and np.array_equal(got[t, max(NV[t], 1):], blk0[t, max(NV[t], 1):])
    assert (got[0, 1:] >= 0).all() and (got[1, 1:7] >= 0).all() and np.array_equal(got[2], blk0[2])
