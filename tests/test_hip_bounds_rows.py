"""Bounds of the row kernels (rows.hip, accept.hip, candidates.hip, nucleus.hip, logprobs.hip, penalties.hip,
logit_bias.hip, grammar.hip, grammar_draft.hip) inside a guarded arena (tests/arena.py, tests/bounds_common.py: W, R, S).

Layout of the verify-row launches: three tiles [3][16][V] with a logits row stride of V + 8 (the 8 slack columns hold the
pattern); tile 0 full, tile 1 ragged (the row count from its record, row0 = 1), tile 2 idle.  V is a multiple of 8 just
above a multiple of a 256- or 1024-thread workgroup's 8-element chunks (2056 = 8 * 257, 8200 = 8 * 1025).  Per-slot tables
are exactly [slots][stride] with stride = V + 8 and the last slot in use; the integer records and id lists are `index`
buffers (their guards hold 0 / 1: valid ids, never a wild address).

Each launch runs under both guard patterns and once more on ordinary torch allocations holding the same bytes, whose
outputs must be bit-equal (bounds_common.check_launch); the integer records are compared with records_ref's model."""
from types import SimpleNamespace

import pytest
import torch

import arena as A
import bounds_common as B
import records_ref as RR

gpu = pytest.mark.gpu
BF16, F32, I32, I64, U8, I16 = B.BF16, B.F32, B.I32, B.I64, B.U8, torch.int16
S_, TAU, BS, POS0, START = 0, 1, 2, 3, 4
T = 3                                   # tiles = request slots
NV = (16, 7, 0)                         # rows per tile (the record's BS word)
VS = (2056, 8200)

COVERS = {
    "dfl_sample_rows_nucleus": "test_sample_rows_nucleus_bounds",
    "dfl_logprob_rows": "test_logprob_rows_bounds",
    "dfl_penalty_count": "test_penalty_bounds",
    "dfl_penalty_rows": "test_penalty_bounds",
    "dfl_logit_bias_rows": "test_logit_bias_rows_bounds",
    "dfl_grammar_rows": "test_grammar_bounds",
    "dfl_grammar_advance": "test_grammar_bounds",
    "dfl_grammar_draft_rows": "test_grammar_bounds",
    "dfl_argmax": "test_argmax_sample_rows_topk_bounds",
    "dfl_sample_rows": "test_argmax_sample_rows_topk_bounds",
    "dfl_topk_rows": "test_argmax_sample_rows_topk_bounds",
    "dfl_candidate_select": "test_candidate_select_bounds",
    "dfl_accept_commit": "test_accept_commit_bounds",
    "dfl_accept_commit_batch": "test_accept_commit_batch_bounds",
    "dfl_admit_slot": "test_admit_slot_bounds",
    "dfl_norm_pack": "test_norm_pack_bounds",
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def _logits(V, seed):
    return (torch.randn(T, 16, V, generator=B.cuda_gen(seed), device=B.dev()) * 3).to(BF16)


def _fill_logits(c, lg, which, V):
    """c.logits [T][16][V + 8]: the data, the slack columns and the rows at or past each tile's count under the pattern."""
    c.logits[:, :, :V].copy_(lg)
    A.poison(c.logits, (slice(None), slice(None), slice(V, None)), which)
    for t in range(T):
        A.poison(c.logits, (t, slice(NV[t], None)), which)


def _fill_dyn(c, pos0=(40, 90, 5)):
    c.dyn.zero_()
    for t in range(T):
        c.dyn[t, BS], c.dyn[t, POS0], c.dyn[t, START] = NV[t], pos0[t], pos0[t]


def _rows_written(t, row0=1):
    """out index range [lo, hi) of tile t for row0 = 1, out_off = 1: rows row0 .. NV[t]."""
    return 1, 1 + max(NV[t] - row0, 0)


# ---------------------------------------------------------------- dfl_sample_rows_nucleus
@gpu
@pytest.mark.parametrize("V", VS)
def test_sample_rows_nucleus_bounds(ops, V):
    """Per-slot seeds / top_k / top_p / invT of exactly T entries (slot 2: greedy, slot 1: top_k on), outputs of exactly
    [T][16]: entries outside a tile's rows, and all of an idle or greedy slot, keep their sentinels."""
    lg = _logits(V, V)
    plan = [("logits", (T, 16, V + 8), BF16), ("dyn", (T, 8), I32, "index"), ("seeds", T, I64, "index"), ("top_k", T, I32, "index"),
            ("top_p", T, F32), ("inv_t", T, F32), ("out", (T, 16), I64, "index"), ("thr", (T, 16), F32), ("kept", (T, 16), I32, "index")]

    def make(c, which):
        _fill_logits(c, lg, which, V)
        _fill_dyn(c)
        c.seeds.copy_(torch.tensor([11, 12, 13])), c.top_k.copy_(torch.tensor([0, 5, 3], dtype=I32))
        c.top_p.copy_(torch.tensor([0.9, 1.0, 0.5])), c.inv_t.copy_(torch.tensor([1.25, 0.8, 2.0]))
        c.out.fill_(-7), c.thr.fill_(-7.0), c.kept.fill_(-7)

    def launch(t):
        ops.sample_rows_nucleus(t.logits[:, :, :V], top_k=t.top_k, top_p=t.top_p, seed=t.seeds, row0=1, nrows=15, dyn=t.dyn,
                                nrows_dyn_word=BS, pos_word=POS0, inv_t=t.inv_t, out=t.out, out_off=1, thresholds=t.thr,
                                kept=t.kept)
    c, res = B.check_launch(V + 8, plan, make, launch, ["out", "thr", "kept"])
    for t in range(T):
        lo, hi = _rows_written(t)
        ids = res["out"][t]
        assert torch.all(ids[:lo] == -7) and torch.all(ids[hi:] == -7) and torch.all(res["kept"][t, hi:] == -7), t
        assert hi == lo or (int(ids[lo:hi].min()) >= 0 and int(ids[lo:hi].max()) < V), t
        assert torch.isfinite(res["thr"][t, lo:hi]).all() and torch.all(res["thr"][t, hi:] == -7.0), t
        if t == 1 and hi > lo:
            assert int(res["kept"][t, lo:hi].max()) <= 5 + 8          # top_k = 5 plus ties at the threshold


# ---------------------------------------------------------------- dfl_logprob_rows
@gpu
@pytest.mark.parametrize("V", VS)
def test_logprob_rows_bounds(ops, V):
    """The sinks are exactly [T][lp_len] (and x n_top); tile 1's positions run past lp_len: dropped, nothing behind the
    sinks is written.  ids rows of exactly 16; an id past a tile's count is never read as a column."""
    lg, n_top, lp_len = _logits(V, V + 1), 3, 48
    ids0 = torch.randint(0, V, (T, 16), generator=B.cuda_gen(V), device=B.dev())
    ids0[0, 1] = V - 1
    plan = [("logits", (T, 16, V + 8), BF16), ("dyn", (T, 8), I32, "index"), ("ids", (T, 16), I64, "index"),
            ("lp", (T, lp_len), F32), ("top_ids", (T, lp_len, n_top), I64, "index"), ("top_lp", (T, lp_len, n_top), F32)]

    def make(c, which):
        _fill_logits(c, lg, which, V)
        _fill_dyn(c, pos0=(20, lp_len - 4, 5))
        c.ids.copy_(ids0)
        for t in range(T):
            A.poison(c.ids, (t, slice(max(NV[t], 1), None)), which)
        c.lp.fill_(-7.0), c.top_ids.fill_(-7), c.top_lp.fill_(-7.0)

    def launch(t):
        sink = SimpleNamespace(lp=t.lp, top_ids=t.top_ids, top_lp=t.top_lp, n_top=n_top, slot=0)
        ops.logprob_rows(t.logits[:, :, :V], t.ids, sink, ids_off=1, row0=1, nrows=15, dyn=t.dyn, nrows_dyn_word=BS,
                         pos_word=POS0, pos_add=1)
    c, res = B.check_launch(V + 8, plan, make, launch, ["lp", "top_ids", "top_lp"])
    # tile 0: rows 1..15 at positions 20 + 1 + m; tile 1: rows 1..6 at 44 + 1 + m, those >= 48 dropped; tile 2: none
    written = torch.zeros(T, lp_len, dtype=torch.bool)
    written[0, 22:37] = True
    written[1, 46:48] = True
    got = (res["lp"] != -7.0).cpu()
    assert torch.equal(got, written), (got.nonzero().tolist())
    x = lg[0, 1:16].float()
    want = x.gather(1, ids0[0, 1:16, None])[:, 0] - torch.logsumexp(x, dim=-1)
    torch.testing.assert_close(res["lp"][0, 22:37], want, rtol=0, atol=2e-5 * float(want.abs().max()) + 1e-5)
    assert int(res["top_ids"][0, 22:37].min()) >= 0 and int(res["top_ids"][0, 22:37].max()) < V
    assert torch.all(res["top_ids"][~written] == -7) and torch.all(res["top_lp"][~written] == -7.0)


# ---------------------------------------------------------------- dfl_penalty_count + dfl_penalty_rows
@gpu
@pytest.mark.parametrize("V", VS)
def test_penalty_bounds(ops, V):
    """The table is exactly [T][V + 8] int32 (columns [V, V + 8) hold the pattern and keep it), the id lists exactly
    [T][ids_len] with the counted range clamped to it, r / a / f of exactly T entries, the last slot in use by the count
    (its record is live there).  Then the penalised rows, in place of nothing: a separate out of the logits' strides."""
    lg, n = _logits(V, V + 2), 24
    ids0 = torch.randint(0, V, (T, n), generator=B.cuda_gen(V + 1), device=B.dev())
    ids0[:, 3] = V - 1
    ids0[:, 4] = V + 5                                  # outside the vocabulary: not counted, never indexed
    blk0 = torch.randint(0, V, (T, 16), generator=B.cuda_gen(V + 2), device=B.dev())
    plan = [("logits", (T, 16, V + 8), BF16), ("out", (T, 16, V + 8), BF16), ("dyn", (T, 8), I32, "index"),
            ("cdyn", (T, 8), I32, "index"), ("table", (T, V + 8), I32, "index"), ("ids", (T, n), I64, "index"),
            ("block", (T, 16), I64, "index"), ("r", T, F32), ("a", T, F32), ("f", T, F32), ("out_ids", (T, 16), I64, "index")]

    def make(c, which):
        _fill_logits(c, lg, which, V)
        _fill_dyn(c)
        c.table.zero_()
        A.poison(c.table, (slice(None), slice(V, None)), which)
        c.ids.copy_(ids0), c.block.copy_(blk0)
        c.cdyn.zero_()                                   # ids (S, START] + 1: slot 0 counts 1..9, slot 1 is idle, slot 2
        for s, (lo, hi, bs) in enumerate(((0, 9, 16), (2, 8, 0), (15, 40, 4))):     # runs past ids_len: clamped
            c.cdyn[s, S_], c.cdyn[s, START], c.cdyn[s, BS] = lo, hi, bs
        c.r.copy_(torch.tensor([1.5, 1.0, 2.0])), c.a.copy_(torch.tensor([0.25, 0.0, 1.0])), c.f.copy_(torch.tensor([0.125, 0.5, 0.0]))
        c.out.fill_(-7.0), c.out_ids.fill_(-7)

    def launch(t):
        tab = t.table[:, :V]
        ops.penalty_count(tab, t.ids, lo=0, hi=6, as_prompt=True, clear=True)
        ops.penalty_count(tab, t.ids, lo=1, hi=1, dyn=t.cdyn, lo_word=S_, hi_word=START)
        ops.penalty_rows(t.logits[:, :, :V], tab, repetition_penalty=t.r, presence_penalty=t.a, frequency_penalty=t.f,
                         block=t.block, out=t.out[:, :, :V], row0=1, nrows=15, dyn=t.dyn, nrows_dyn_word=BS, out_ids=t.out_ids,
                         out_off=1)
    c, res = B.check_launch(V + 8, plan, make, launch, [("table", lambda t: t.table[:, :V]), "out", "out_ids"])
    want = torch.zeros(T, V, dtype=torch.int64)
    for s, (lo, hi, live) in enumerate(((1, 10, True), (0, 0, False), (16, n, True))):
        for v in ids0[s, :6].tolist():
            if v < V:
                want[s, v] |= 1 << 31
        for v in (ids0[s, lo:hi].tolist() if live else []):
            if v < V:
                want[s, v] += 1
    assert torch.equal(res["table"].cpu().to(torch.int64) & 0xFFFFFFFF, want)
    assert torch.all(c.table[:, V:] == A.pattern_scalar(I32, "index", "A"))          # (the last fill) clear = 1 stops at V
    for t in range(T):
        lo, hi = _rows_written(t)
        assert torch.all(res["out"][t, :1] == -7.0) and torch.all(res["out"][t, max(NV[t], 1):] == -7.0), t
        assert torch.all(res["out"][t, :, V:] == -7.0), t
        assert torch.all(res["out_ids"][t, :lo] == -7) and torch.all(res["out_ids"][t, hi:] == -7), t
        if hi > lo:
            rows = res["out"][t, 1:NV[t], :V].float()
            assert torch.isfinite(rows).all() and torch.equal(res["out_ids"][t, lo:hi], B.first_argmax(rows)), t


# ---------------------------------------------------------------- dfl_logit_bias_rows
@gpu
@pytest.mark.parametrize("V", VS)
def test_logit_bias_rows_bounds(ops, V):
    """The bias table exactly [T][V + 8] fp32 (slack columns under the pattern), min_pos of exactly T entries, a stop list
    with an id outside [0, V) ("ignored and never indexed")."""
    lg = _logits(V, V + 3)
    bias0 = torch.zeros(T, V, device=B.dev())
    bias0[:, 5], bias0[:, V - 1], bias0[1, 9] = 2.5, float("-inf"), -1.0
    plan = [("logits", (T, 16, V + 8), BF16), ("out", (T, 16, V + 8), BF16), ("dyn", (T, 8), I32, "index"),
            ("bias", (T, V + 8), F32), ("min_pos", T, I32, "index"), ("stops", 3, I64, "index"), ("out_ids", (T, 16), I64, "index")]

    def make(c, which):
        _fill_logits(c, lg, which, V)
        _fill_dyn(c)
        c.bias[:, :V].copy_(bias0)
        A.poison(c.bias, (slice(None), slice(V, None)), which)
        c.min_pos.copy_(torch.tensor([45, 0, 99], dtype=I32)), c.stops.copy_(torch.tensor([7, V + 3, -2]))
        c.out.fill_(-7.0), c.out_ids.fill_(-7)

    def launch(t):
        ops.logit_bias_rows(t.logits[:, :, :V], t.bias[:, :V], min_pos=t.min_pos, stop_ids=t.stops, out=t.out[:, :, :V], row0=1,
                            nrows=15, dyn=t.dyn, nrows_dyn_word=BS, pos_word=POS0, pos_add=1, out_ids=t.out_ids, out_off=1)
    c, res = B.check_launch(V + 8, plan, make, launch, ["out", "out_ids"])
    for t in range(T):
        lo, hi = _rows_written(t)
        assert torch.all(res["out"][t, :1] == -7.0) and torch.all(res["out"][t, max(NV[t], 1):] == -7.0), t
        assert torch.all(res["out"][t, :, V:] == -7.0) and torch.all(res["out_ids"][t, hi:] == -7), t
        for m in range(1, NV[t]):
            x, z = lg[t, m].float(), res["out"][t, m, :V].float()
            want = torch.where(bias0[t] == 0, x, (x + bias0[t]).to(BF16).float())
            if 40 + 1 + m < 45 and t == 0:               # below min_pos: the stop id inside the vocabulary is banned
                want[7] = float("-inf")
            assert torch.equal(z, want), (t, m)


# ---------------------------------------------------------------- dfl_grammar_rows / _advance / _draft_rows
@gpu
@pytest.mark.parametrize("V", VS)
def test_grammar_bounds(ops, V):
    """The pool is exactly [pool_states][V + 8] int16; slot 1's grammar ends on the pool's LAST row and is walked into it;
    slot 0's has a successor at or past pool_states ("reads as violated and is never indexed": a read of that row would
    land in the guard behind the pool).  base / state of exactly T entries, block rows of exactly 16 ids."""
    lg = _logits(V, V + 4)
    pool, bases, nst = 7, (0, 4, -1), (4, 3, 0)
    g = B.cuda_gen(V + 5)
    tab0 = torch.full((pool, V), -1, dtype=I16, device=B.dev())
    for b, n in zip(bases[:2], nst[:2]):
        nxt = torch.randint(-1, n, (n, V), generator=g, device=B.dev()).to(I16)
        tab0[b:b + n] = nxt
    blk0 = torch.randint(0, V, (T, 16), generator=g, device=B.dev())
    # slot 0: token blk0[0, 1] in state 0 leads to successor 9: base + 9 >= pool_states, violated from row 2 on
    tab0[0, blk0[0, 1]] = 9
    # slot 1: its block walks 0 -> 2 (pool row 6, the last) and stays legal there
    tab0[4, blk0[1, 1]] = 2
    tab0[6, blk0[1, 2:7]] = 2
    bias0 = torch.zeros(T, V, device=B.dev())
    bias0[:, 11] = float("-inf")
    ids0 = torch.randint(0, V, (T, 12), generator=g, device=B.dev())
    plan = [("logits", (T, 16, V + 8), BF16), ("out", (T, 16, V + 8), BF16), ("dyn", (T, 8), I32, "index"),
            ("cdyn", (T, 8), I32, "index"), ("table", (pool, V + 8), I16, "index"), ("base", T, I32, "index"),
            ("state", T, I32, "index"), ("state2", T, I32, "index"), ("block", (T, 16), I64, "index"),
            ("dblock", (T, 16), I64, "index"), ("bias", (T, V + 8), F32), ("ids", (T, 12), I64, "index"),
            ("out_ids", (T, 16), I64, "index")]

    def make(c, which):
        _fill_logits(c, lg, which, V)
        _fill_dyn(c)
        c.table[:, :V].copy_(tab0)
        c.table[:, V:].fill_(-1 if which == "A" else 0)           # the slack columns: two patterns of the table's own type
        c.base.copy_(torch.tensor(bases, dtype=I32)), c.state.zero_(), c.state2.zero_()
        c.block.copy_(blk0), c.dblock.copy_(blk0), c.ids.copy_(ids0)
        c.bias[:, :V].copy_(bias0)
        A.poison(c.bias, (slice(None), slice(V, None)), which)
        c.cdyn.zero_()
        for s, (lo, hi, bs) in enumerate(((0, 5, 16), (1, 30, 4), (2, 6, 0))):
            c.cdyn[s, S_], c.cdyn[s, START], c.cdyn[s, BS] = lo, hi, bs
        c.out.fill_(-7.0), c.out_ids.fill_(-7)

    def launch(t):
        st = SimpleNamespace(table=t.table[:, :V], base=t.base, state=t.state, used=pool)
        ops.grammar_rows(t.logits[:, :, :V], st, block=t.block, out=t.out[:, :, :V], row0=1, nrows=15, dyn=t.dyn,
                         nrows_dyn_word=BS, out_ids=t.out_ids, out_off=1)
        ops.grammar_draft_rows(t.logits[:, :, :V], st, bias=t.bias[:, :V], block=t.dblock, dyn=t.dyn, nrows_dyn_word=BS)
        st2 = SimpleNamespace(table=t.table[:, :V], base=t.base, state=t.state2, used=pool)
        ops.grammar_advance(st2, t.ids, lo=1, hi=1, dyn=t.cdyn, lo_word=S_, hi_word=START)
    c, res = B.check_launch(V + 8, plan, make, launch, ["out", "out_ids", "dblock", "state2", "state"])
    tab = tab0.cpu().to(torch.int64)
    for t in range(T):
        lo, hi = _rows_written(t)
        assert torch.all(res["out"][t, :1] == -7.0) and torch.all(res["out"][t, max(NV[t], 1):] == -7.0), t
        assert torch.all(res["out"][t, :, V:] == -7.0) and torch.all(res["out_ids"][t, hi:] == -7), t
        s = 0
        for m in range(1, NV[t]):
            if s >= 0:
                s = int(tab[bases[t] + s, int(blk0[t, m])]) if bases[t] >= 0 else -1
                if s >= 0 and bases[t] + s >= pool:
                    s = -1
            x = lg[t, m].float()
            want = torch.where(tab[bases[t] + s] < 0, torch.full_like(x, float("-inf")).cpu(), x.cpu()) if s >= 0 else x.cpu()
            assert torch.equal(res["out"][t, m, :V].float().cpu(), want), (t, m, s)
        assert int(res["dblock"][t, 0]) == int(blk0[t, 0]) and torch.equal(res["dblock"][t, max(NV[t], 1):], blk0[t, max(NV[t], 1):]), t
    assert torch.equal(res["state"], torch.zeros(T, dtype=I32, device=B.dev()))          # only read by the two row launches
    for s, (lo, hi, live) in enumerate(((1, 6, True), (2, 12, True), (0, 0, False))):
        st = 0
        for v in (ids0[s, lo:hi].tolist() if live and bases[s] >= 0 else []):
            if st >= 0:
                st = int(tab[bases[s] + st, v])
                st = -1 if st >= 0 and bases[s] + st >= pool else st
        assert int(res["state2"][s]) == st, s


# ---------------------------------------------------------------- dfl_argmax, dfl_sample_rows, dfl_topk_rows
@gpu
@pytest.mark.parametrize("V", [1003, 8200])
def test_argmax_sample_rows_topk_bounds(ops, V):
    """Materialised logits of exactly [rows][V - V % 8] (dfl_argmax, bf16 and fp32) and [rows][ld] with ld = V + 3 (dfl_sample_rows,
    dfl_topk_rows: V = 1003 is no multiple of 8 and ld = 1006 puts odd rows on an unaligned start); row 2 has its eight
    largest values inside one aligned 8-element vector, row 3 its maximum in the last column.  Outputs sized exactly."""
    rows, ld, Va = 5, V + 3, V - V % 8
    lg = (torch.randn(rows, V, generator=B.cuda_gen(V), device=B.dev()) * 2).to(BF16)
    lg[2, 64:72] = torch.arange(20, 28, device=B.dev()).to(BF16)
    lg[3, V - 1] = 30.0
    plan = [("lb", (rows, Va), BF16), ("lf", (rows, Va), F32), ("ls", (rows, ld), BF16), ("ids_b", rows, I64, "index"),
            ("ids_f", rows, I64, "index"), ("pos", rows, I32, "index"), ("sid", rows, I64, "index"), ("smg", rows, F32),
            ("val", (rows, 8), F32), ("idx", (rows, 8), I32, "index"), ("lse", rows, F32)]

    def make(c, which):
        c.lb.copy_(lg[:, :Va]), c.lf.copy_(lg[:, :Va].float()), c.ls[:, :V].copy_(lg)
        A.poison(c.ls, (slice(None), slice(V, None)), which)
        c.pos.copy_(torch.tensor([3, 9, 4, 100, 7], dtype=I32))
        for n in ("ids_b", "ids_f", "sid", "idx"):
            getattr(c, n).fill_(-7)
        c.smg.fill_(-7.0), c.val.fill_(-7.0), c.lse.fill_(-7.0)

    def launch(t):
        lb, st = ops.lib(), torch.cuda.current_stream().cuda_stream
        ops.check(lb.dfl_argmax(t.lb.data_ptr(), 0, rows, Va, t.ids_b.data_ptr(), st), "dfl_argmax")
        ops.check(lb.dfl_argmax(t.lf.data_ptr(), 1, rows, Va, t.ids_f.data_ptr(), st), "dfl_argmax")
        if V % 8 == 0:
            ops.sample_rows(t.ls[:, :V], seed=5, temperature=0.8, positions=t.pos, out=t.sid, margins=t.smg)
        ops.check(lb.dfl_topk_rows(t.ls.data_ptr(), ld, rows, V, 8, t.val.data_ptr(), t.idx.data_ptr(), t.lse.data_ptr(), st),
                  "dfl_topk_rows")
    c, res = B.check_launch(ld, plan, make, launch, ["ids_b", "ids_f", "sid", "smg", "val", "idx", "lse"])
    assert torch.equal(res["ids_b"], B.first_argmax(lg[:, :Va].float())) and torch.equal(res["ids_f"], res["ids_b"])
    tv, ti = lg.float().topk(8, dim=-1)
    assert torch.equal(res["val"], tv) and res["idx"][2].tolist() == list(range(71, 63, -1))
    torch.testing.assert_close(res["lse"], torch.logsumexp(lg.float(), dim=-1), rtol=1e-5, atol=1e-5)
    if V % 8 == 0:
        assert int(res["sid"].min()) >= 0 and int(res["sid"].max()) < V and torch.isfinite(res["smg"]).all()


# ---------------------------------------------------------------- dfl_candidate_select
@gpu
@pytest.mark.parametrize("bs,start,n_cand", [(16, 10, 4), (63, 5, 8), (32, 40, 3)], ids=lambda v: str(v))
def test_candidate_select_bounds(ops, bs, start, n_cand):
    """blocks / posterior of exactly [n_cand][bs], scores of exactly n_cand, output_ids of exactly output_len ids with the
    winner's commit running past it (start + acc + 1 >= output_len: clipped), result of exactly 12 words, dyn of 8."""
    out_len = start + bs // 2                       # the full-accept winner's tokens do not fit
    g = torch.Generator().manual_seed(bs)
    post = torch.randint(0, 1000, (n_cand, bs), generator=g)
    blocks = torch.randint(0, 1000, (n_cand, bs), generator=g)
    win = n_cand - 1
    blocks[win, 1:] = post[win, :-1]                # the last candidate accepts everything
    blocks[0, 1:3] = post[0, :2]
    plan = [("blocks", (n_cand, bs), I64, "index"), ("post", (n_cand, bs), I64, "index"), ("scores", n_cand, F32),
            ("out", out_len, I64, "index"), ("dyn", 8, I32, "index"), ("stops", 2, I64, "index"), ("result", 12, I32, "index")]

    def make(c, which):
        c.blocks.copy_(blocks), c.post.copy_(post)
        c.scores.copy_(torch.linspace(-1.0, 1.0, n_cand))
        c.out.fill_(-7)
        c.dyn.copy_(torch.tensor([start - 3, 3, bs, start - 3, start, 0, 4, 77], dtype=I32))
        c.stops.copy_(torch.tensor([1001, 1002])), c.result.fill_(-7)

    def launch(t):
        ops.candidate_select(t.blocks, t.post, t.scores, bs, t.out, t.dyn, t.stops, t.result)
    c, res = B.check_launch(bs, plan, make, launch, ["out", "dyn", "result"])
    want_out, dyn = [-7] * out_len, [start - 3, 3, bs, start - 3, start, 0, 4, 77]
    acc = RR.single_cycle(blocks[win].tolist(), post[win].tolist(), bs, want_out, out_len, dyn, {1001, 1002})
    assert acc == bs - 1 and res["out"].tolist() == want_out and res["dyn"].tolist() == dyn
    r = res["result"].tolist()
    assert r[:4] == [acc, start + acc + 1, 0, win] and r[4] == 2 and r[4 + win] == acc and all(x == -1 for x in r[4 + n_cand:])


# ---------------------------------------------------------------- dfl_accept_commit
@gpu
@pytest.mark.parametrize("bs,rearm_n", [(16, 16), (63, 64), (5, 1)], ids=lambda v: str(v))
def test_accept_commit_bounds(ops, bs, rearm_n):
    """block / posterior of exactly bs ids, output_ids of exactly output_len with the commit clipped at it, result of
    exactly 4 words, the re-armed block of exactly rearm_n ids, both records of exactly 8 words."""
    start = 9
    out_len = start + bs - 2
    g = torch.Generator().manual_seed(bs)
    post = torch.randint(0, 1000, (bs,), generator=g)
    block = torch.randint(0, 1000, (bs,), generator=g)
    block[1:] = post[:-1]
    plan = [("block", bs, I64, "index"), ("post", bs, I64, "index"), ("out", out_len, I64, "index"), ("dyn", 8, I32, "index"),
            ("dyn_t", 8, I32, "index"), ("stops", 2, I64, "index"), ("result", 4, I32, "index"), ("nb", rearm_n, I64, "index")]
    d0, dt0 = [start - 2, 2, bs, start - 2, start, 0, 3, 55], [1, 2, bs, 3, 4, 0, 3, 66]

    def make(c, which):
        c.block.copy_(block), c.post.copy_(post), c.out.fill_(-7), c.nb.fill_(-7), c.result.fill_(-7)
        c.dyn.copy_(torch.tensor(d0, dtype=I32)), c.dyn_t.copy_(torch.tensor(dt0, dtype=I32))
        c.stops.copy_(torch.tensor([int(post[bs - 1]), 2000]))

    def launch(t):
        ops.accept_commit(t.block, t.post, bs, t.out, t.dyn, stop_ids=t.stops, result=t.result, rearm=(t.nb, rearm_n, 999),
                          dyn_t=t.dyn_t)
    c, res = B.check_launch(64, plan, make, launch, ["out", "dyn", "dyn_t", "result", "nb"])
    want_out, dyn, dyn_t, result, nb = [-7] * out_len, list(d0), list(dt0), [-7] * 4, [-7] * rearm_n
    RR.single_cycle(block.tolist(), post.tolist(), bs, want_out, out_len, dyn, {int(post[bs - 1]), 2000}, result, nb, rearm_n,
                    999, dyn_t)
    assert (res["out"].tolist(), res["dyn"].tolist(), res["dyn_t"].tolist()) == (want_out, dyn, dyn_t)
    assert res["result"].tolist() == result and res["nb"].tolist() == nb and dyn[RR.STOP] == 1


# ---------------------------------------------------------------- dfl_accept_commit_batch
@gpu
@pytest.mark.parametrize("tpr", [1, 2], ids=["tiles1", "tiles2"])
def test_accept_commit_batch_bounds(ops, tpr):
    """R = 3 requests (one idle: no word of its slot is read or written), every buffer of exactly R rows: block / posterior
    [R][16 tpr], output_ids [R][output_len] with a commit clipped at it, the per-request and per-tile records."""
    R, w = 3, 16 * tpr
    out_len = 40
    bss, starts = (w, 0, w - 3), (out_len - 6, 7, 11)
    g = torch.Generator().manual_seed(tpr)
    post = torch.randint(0, 1000, (R, w), generator=g)
    block = torch.randint(0, 1000, (R, w), generator=g)
    block[0, 1:] = post[0, :-1]
    block[2, 1:4] = post[2, :3]
    dd0 = [[starts[r] - 1, 1, bss[r], starts[r] - 1, starts[r], 0, 2, 40 + r] for r in range(R)]
    dt0 = [[5, 6, 7, 8, 9, 0, 2, 50 + r] for r in range(R)]
    tl0 = [[60 + i] * 8 for i in range(R * tpr)]
    plan = [("block", (R, w), I64, "index"), ("post", (R, w), I64, "index"), ("out", (R, out_len), I64, "index"),
            ("dd", (R, 8), I32, "index"), ("dt", (R, 8), I32, "index"), ("ddt", (R * tpr, 8), I32, "index"),
            ("dtt", (R * tpr, 8), I32, "index"), ("stops", 1, I64, "index"), ("result", (R, 4), I32, "index"),
            ("nb", (R, w), I64, "index")]

    def make(c, which):
        c.block.copy_(block), c.post.copy_(post), c.out.fill_(-7), c.nb.fill_(-7), c.result.fill_(-7)
        A.poison(c.block, 1, which), A.poison(c.post, 1, which)            # the idle request's rows: none is read
        c.dd.copy_(torch.tensor(dd0, dtype=I32)), c.dt.copy_(torch.tensor(dt0, dtype=I32))
        c.ddt.copy_(torch.tensor(tl0, dtype=I32)), c.dtt.copy_(torch.tensor(tl0, dtype=I32))
        c.stops.fill_(3000)

    def launch(t):
        ops.accept_commit_batch(t.block, t.post, R, t.out, t.dd, t.dt, t.stops, t.result, rearm_mask_id=999, tiles_per_req=tpr,
                                dyn_d_tiles=t.ddt, dyn_t_tiles=t.dtt, next_block=t.nb)
    c, res = B.check_launch(64, plan, make, launch, ["out", "dd", "dt", "ddt", "dtt", "result", "nb"])
    out, dd, dt = [[-7] * out_len for _ in range(R)], [list(x) for x in dd0], [list(x) for x in dt0]
    ddt, dtt = [list(x) for x in tl0], [list(x) for x in tl0]
    result, nb = [[-7] * 4 for _ in range(R)], [[-7] * w for _ in range(R)]
    RR.batch_cycle(R, block.tolist(), post.tolist(), out, out_len, dd, dt, {3000}, result, nb, 999, tpr,
                   ddt if tpr == 2 else None, dtt if tpr == 2 else None)
    assert res["out"].tolist() == out and res["dd"].tolist() == dd and res["dt"].tolist() == dt
    assert res["result"].tolist() == result and res["nb"].tolist() == nb
    assert res["ddt"].tolist() == ddt and res["dtt"].tolist() == dtt


# ---------------------------------------------------------------- dfl_admit_slot
@gpu
@pytest.mark.parametrize("P,n_tail", [(40, 16), (9, 9), (20, 0)], ids=lambda v: str(v))
def test_admit_slot_bounds(ops, P, n_tail):
    """The LAST slot of three: every per-slot buffer is exactly [3][...], so whatever the launch writes one slot too far
    lands in a guard; the tail rows are exactly n_tail rows of a wider buffer; the other slots keep their bits."""
    slots, r, out_len, blk_w, fc = 3, 2, 64, 16, 72
    prompt = torch.randint(0, 1000, (P,), generator=torch.Generator().manual_seed(P))
    tail = B.small_ints((max(n_tail, 1), fc + 8), P, -50, 50)
    plan = [("prompt", P, I64, "index"), ("first", 1, I64, "index"), ("out", (slots, out_len), I64, "index"),
            ("block", (slots, blk_w), I64, "index"), ("post", (slots, blk_w), I64, "index"), ("result", (slots, 4), I32, "index"),
            ("tail", (max(n_tail, 1), fc + 8), BF16), ("taps", (slots, 16, fc), BF16), ("dd", (slots, 8), I32, "index"),
            ("dt", (slots, 8), I32, "index"), ("seeds", slots, I64, "index")]

    def make(c, which):
        c.prompt.copy_(prompt), c.first.fill_(321), c.tail.copy_(tail)
        A.poison(c.tail, (slice(None), slice(fc, None)), which)
        for n in ("out", "block", "post", "result", "dd", "dt", "seeds"):
            getattr(c, n).fill_(-7)
        c.taps.fill_(-7.0)

    def launch(t):
        ops.admit_slot(r, t.prompt, t.first, t.out, t.block, t.post, t.result, t.tail[:n_tail, :fc], t.taps, t.dd, t.dt, 11, 999,
                       seeds=t.seeds, seed=-5)
    c, res = B.check_launch(fc + 8, plan, make, launch, ["out", "block", "post", "result", "taps", "dd", "dt", "seeds"])
    out, blk, post, result = [-7] * out_len, [-7] * blk_w, [-7] * blk_w, [-7] * 4
    dd, dt, seeds = [-7] * 8, [-7] * 8, [-7] * slots
    RR.admit(prompt.tolist(), 321, out, out_len, blk, post, blk_w, result, n_tail, dd, dt, 11, 999, seeds, r, -5)
    for name, want in (("out", out), ("block", blk), ("post", post), ("result", result), ("dd", dd), ("dt", dt)):
        assert res[name][r].tolist() == want, name
        assert torch.all(res[name][:r] == -7), name
    assert res["seeds"].tolist() == seeds
    assert torch.equal(res["taps"][r, :n_tail], tail[:n_tail, :fc]) and torch.count_nonzero(res["taps"][r, n_tail:].float()) == 0
    assert torch.all(res["taps"][:r] == -7.0)


# ---------------------------------------------------------------- dfl_norm_pack
@gpu
@pytest.mark.parametrize("Hd,mode", [(72, "embed"), (4104, "resid"), (16384, "part")], ids=lambda v: str(v))
def test_norm_pack_bounds(ops, Hd, mode):
    """dfl_norm_pack with 6 valid rows: the parts exactly [2][row_off + 16][H] with the rows past the count under the
    pattern, the embedding table exactly [V][H] with its last row in use, h_out exactly [16][H], h_out2 a column slice of a
    wider buffer, frag exactly 16 H."""
    from oracle.dflash_oracle import rms_norm
    nv, V, row_off = 6, 24, 16
    g = B.cuda_gen(Hd)
    part0 = torch.randn(2, row_off + 16, Hd, generator=g, device=B.dev()) * 0.3
    resid0 = (torch.randn(16, Hd, generator=g, device=B.dev()) * 0.7).to(BF16)
    emb0 = (torch.randn(V, Hd, generator=g, device=B.dev()) * 0.7).to(BF16)
    nw0 = (1 + 0.1 * torch.randn(Hd, generator=g, device=B.dev())).to(BF16)
    ids0 = torch.tensor([V - 1, 0, 5, V - 1, 7, 3] + [2] * 10, device=B.dev())
    plan = [("part", (2, row_off + 16, Hd), F32), ("resid", (16, Hd), BF16), ("emb", (V, Hd), BF16), ("ids", 16, I64, "index"),
            ("nw", Hd, BF16), ("h", (16, Hd), BF16), ("h2", (16, Hd + 16), BF16), ("frag", 16 * Hd, BF16), ("dyn", 8, I32, "index")]

    def make(c, which):
        c.part.copy_(part0), c.resid.copy_(resid0), c.emb.copy_(emb0), c.ids.copy_(ids0), c.nw.copy_(nw0)
        A.poison(c.part, (slice(None), slice(row_off + nv, None)), which)
        A.poison(c.resid, slice(nv, None), which)
        A.poison(c.ids, slice(nv, None), which)
        c.h.fill_(-7.0), c.h2.fill_(-7.0), c.frag.fill_(float("nan"))
        c.dyn.zero_()
        c.dyn[BS] = nv

    def launch(t):
        kw = dict(norm_w=t.nw, frag=t.frag, H=Hd, eps=1e-6, h_out=t.h, h_out2=t.h2[:, 8:8 + Hd], ld2=Hd + 16, dyn=t.dyn, dyn_word=BS)
        if mode == "embed":
            ops.norm_pack(embed=t.emb, ids=t.ids, **kw)
        elif mode == "resid":
            ops.norm_pack(resid_in=t.resid, part=t.part, nsplit=2, part_split=(row_off + 16) * Hd, ldp=Hd, row_off=row_off, **kw)
        else:
            ops.norm_pack(part=t.part, nsplit=2, part_split=(row_off + 16) * Hd, ldp=Hd, row_off=row_off, **kw)
    import helpers as H
    c, res = B.check_launch(Hd + 16, plan, make, launch, ["h", "h2", "frag"])
    v = (part0[0, row_off:row_off + nv] + part0[1, row_off:row_off + nv]).to(BF16)
    want = {"embed": emb0[ids0[:nv]], "resid": (resid0[:nv].float() + v.float()).to(BF16), "part": v}[mode]
    assert torch.equal(res["h"][:nv], want) and torch.equal(res["h2"][:nv, 8:8 + Hd], want)
    assert torch.all(res["h2"][:, :8] == -7.0) and torch.all(res["h2"][:, 8 + Hd:] == -7.0)
    fr = H.unfrag(res["frag"], Hd)
    assert torch.count_nonzero(fr[nv:].float()) == 0
    H.assert_close(f"norm_pack bounds {mode}", fr[:nv], rms_norm(want, nw0, 1e-6), max_rel=2 ** -6, mean_rel=H.MEAN_REL)
