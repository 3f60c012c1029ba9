"""Bounds of dfl_stop_seq_rows (stop_seq.hip) inside a guarded arena (tests/arena.py, tests/bounds_common.py: W, R, S).

Every array has exactly its size: block / posterior [3][16] with a row stride of 16, output_ids [3][24], the records
[3][8], the tables [3][8][16] / [3][8] / [3] / [3] and hit [3][2].  Slot 0 is a request whose `start` (2) is smaller than
the longest sequence (16): a read below the row's start would land in the guard in front of output_ids.  Slot 1 is idle,
all its rows hold the pattern.  Slot 2 sits on the last row of every table, its `start` on the last id of its row, its
block fully accepted (lane 15 reads the last id of block and posterior) and its match straddles `start`.  Everything the
header calls unread — block and posterior rows past the block size, ids past `start`, table ids past a sequence's length
— holds the pattern.  The launch runs under both guard patterns and once more on ordinary torch allocations holding the
same bytes, whose outputs must be bit-equal (bounds_common.check_launch); the outputs are then compared with the model."""
from types import SimpleNamespace

import pytest
import torch

import arena as A
import bounds_common as B
import stop_seq_ref as SR

gpu = pytest.mark.gpu
I32, I64 = B.I32, B.I64
S, W, N = 3, 16, 24

COVERS = {
    "dfl_stop_seq_rows": "test_stop_seq_rows_bounds",
}

LONG = list(range(100, 116))
SLOTS = [
    # start = 2 < 16: prompt of 1, block of 5 with 3 accepted; [41, 42] ends at position 4; the 16-id sequences cannot fit
    dict(out=[10, 11, 40], start=2, bs=5, block=[40, 41, 42, 43, 44], post=[41, 42, 43, 50, 51],
         seqs=[LONG, [12] * 16, [41, 42]] + [LONG] * 5, first_pos=1, min_end=0),
    dict(out=[], start=7, bs=0, block=[], post=[], seqs=[[41]], first_pos=0, min_end=0),
    # start = 23 = N - 1: 8 ids of LONG behind start, 8 ahead; all 16 rows accepted
    dict(out=[20] * 16 + LONG[:8], start=23, bs=16, block=[LONG[7]] + LONG[8:] + [60] * 7, post=LONG[8:] + [60] * 7 + [61],
         seqs=[[61, 61]] * 7 + [LONG], first_pos=16, min_end=31),
]


@gpu
def test_stop_seq_rows_bounds():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops
    plan = [("block", (S, W), I64, "index"), ("post", (S, W), I64, "index"), ("out", (S, N), I64, "index"),
            ("dyn", (S, 8), I32, "index"), ("seq_ids", (S, 8, 16), I32, "index"), ("seq_len", (S, 8), I32, "index"),
            ("first_pos", S, I32, "index"), ("min_end", S, I32, "index"), ("hit", (S, 2), I32, "index")]

    def make(c, which):
        for name in ("block", "post", "out", "seq_ids"):      # everything unread holds the pattern
            A.poison(getattr(c, name), slice(None), which)
        c.dyn.zero_(), c.seq_len.zero_(), c.hit.fill_(-1)
        for s, t in enumerate(SLOTS):
            for name in ("block", "post", "out"):
                v = torch.tensor(t[name], dtype=I64)
                getattr(c, name)[s, :len(t[name])] = v.to(c.block.device)
            c.dyn[s] = torch.tensor([3, 4, t["bs"], 5, t["start"], 0, 6, 7], dtype=I32)
            for k, q in enumerate(t["seqs"]):
                c.seq_ids[s, k, :len(q)] = torch.tensor(q, dtype=I32).to(c.block.device)
                c.seq_len[s, k] = len(q)
            c.first_pos[s], c.min_end[s] = t["first_pos"], t["min_end"]

    def launch(t):
        st = SimpleNamespace(seq_ids=t.seq_ids, seq_len=t.seq_len, first_pos=t.first_pos, min_end=t.min_end, hit=t.hit)
        ops.stop_seq_rows(t.block, t.post, t.out, t.dyn, st)

    c, res = B.check_launch(128, plan, make, launch, ["dyn", "hit"])
    # the model, on rows whose unread parts hold a value no sequence has
    dyn = [[3, 4, t["bs"], 5, t["start"], 0, 6, 7] for t in SLOTS]
    tables = [dict(seqs=t["seqs"], first_pos=t["first_pos"], min_end=t["min_end"], hit=[-1, -1]) for t in SLOTS]
    pad = lambda x, n: list(x) + [-5] * (n - len(x))      # noqa: E731
    SR.launch([pad(t["block"], W) for t in SLOTS], [pad(t["post"], W) for t in SLOTS], [pad(t["out"], N) for t in SLOTS],
              dyn, tables)
    assert res["dyn"].tolist() == dyn and res["hit"].tolist() == [t["hit"] for t in tables]
    assert res["hit"].tolist() == [[4, 2], [-1, -1], [31, 7]] and [d[SR.STOP] for d in dyn] == [1, 0, 1]
