"""dfl_stop_seq_rows alone against the pure-Python model of stop_seq_ref.py: the length records and
the hit records are compared exactly, and nothing else the launch is handed may change."""
import random

import pytest
import torch

import stop_seq_ref as SR

gpu = pytest.mark.gpu
I32, I64 = torch.int32, torch.int64
MASK = 99
W = 32            # block / posterior row width
N = 96            # ids per slot


def dev():
    return torch.device("cuda", 0)


def slot(out, block, post, seqs, *, bs=None, first_pos=0, min_end=0, hit=(-1, -1), stop=0, start=None):
    """One slot of a launch: `out` the committed ids (positions 0 .. start; start defaults to their last), block /
    posterior rows, the slot's sequences.  bs: the record's block size (default: the block's length)."""
    start = len(out) - 1 if start is None else start
    bs = len(block) if bs is None else bs
    return dict(out=list(out), block=list(block), post=list(post), seqs=[list(s) for s in seqs], bs=bs, start=start,
                first_pos=first_pos, min_end=min_end, hit=list(hit), stop=stop)


def run(slots, host_bs=None):
    """Launch over `slots` and compare with the model; returns (dyn, hit) as lists."""
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops
    S = len(slots)
    block = torch.full((S, W), 7, dtype=I64)
    post = torch.full((S, W), 8, dtype=I64)
    out = torch.full((S, N), MASK, dtype=I64)
    dyn = torch.zeros(S, 8, dtype=I32)
    for s, c in enumerate(slots):
        block[s, :len(c["block"])] = torch.tensor(c["block"], dtype=I64)
        post[s, :len(c["post"])] = torch.tensor(c["post"], dtype=I64)
        out[s, :len(c["out"])] = torch.tensor(c["out"], dtype=I64)
        # (every word but START / BS / STOP holds a value of its own: the launch may write none of them)
        dyn[s] = torch.tensor([11 + s, 12, c["bs"], 13, c["start"], c["stop"], 14 + s, 15], dtype=I32)
    st = ops.stop_seq_state(S, dev())
    for s, c in enumerate(slots):
        ops.stop_seq_set(st, s, c["seqs"], first_pos=c["first_pos"], min_end=c["min_end"])
        st.hit[s] = torch.tensor(c["hit"], dtype=I32)
    g = [t.to(dev()) for t in (block, post, out, dyn)]
    before = [t.clone() for t in (g[0], g[1], g[2], st.seq_ids, st.seq_len, st.first_pos, st.min_end)]
    ops.stop_seq_rows(g[0], g[1], g[2], g[3], st, bs=host_bs, slots=S)
    torch.cuda.synchronize()
    # the model on the same rows (the whole W-wide rows: what the strides let a record's block size reach)
    ref_dyn = dyn.tolist()
    tables = [dict(seqs=c["seqs"], first_pos=c["first_pos"], min_end=c["min_end"], hit=list(c["hit"])) for c in slots]
    SR.launch(block.tolist(), post.tolist(), out.tolist(), ref_dyn, tables, bs=host_bs)
    got_dyn, got_hit = g[3].cpu().tolist(), st.hit.cpu().tolist()
    assert got_dyn == ref_dyn, (got_dyn, ref_dyn)
    assert got_hit == [t["hit"] for t in tables], (got_hit, [t["hit"] for t in tables])
    for a, b in zip(before, (g[0], g[1], g[2], st.seq_ids, st.seq_len, st.first_pos, st.min_end)):
        assert torch.equal(a, b), "the launch wrote an input"
    return got_dyn, got_hit


def one(*a, host_bs=None, **kw):
    dyn, hit = run([slot(*a, **kw)], host_bs=host_bs)
    return dyn[0][SR.STOP], hit[0]


# the cycle most cases share: positions 0..5 committed (prompt of 3, start = 5), block of 8 whose first four draft tokens
# are accepted (acc = 4): committed now are positions 6..10 = 21 22 23 24 (block[1..4]) and 30 (posterior[4], the bonus)
OUT = [1, 2, 3, 10, 11, 20]
BLOCK = [20, 21, 22, 23, 24, 25, 26, 27]
POST = [21, 22, 23, 24, 30, 31, 32, 33]


@gpu
def test_sequence_wholly_inside_one_commit():
    assert one(OUT, BLOCK, POST, [[22, 23]], first_pos=3) == (1, [8, 0])
    assert one(OUT, BLOCK, POST, [[21, 22, 23, 24, 30]], first_pos=3) == (1, [10, 0])
    assert one(OUT, BLOCK, POST, [[22, 24]], first_pos=3) == (0, [-1, -1])


@gpu
@pytest.mark.parametrize("behind", range(1, 16))
def test_sequence_straddling_start(behind):
    """`behind` ids of a 16-id sequence are in output_ids already (the last of them at `start`), the rest is committed now."""
    seq = list(range(40, 56))
    ahead = 16 - behind
    prompt = [1, 2, 3]
    out = prompt + [5] * 4 + seq[:behind]
    block = [out[-1]] + seq[behind:] + [60] * 15       # 31 rows: the block's tail is accepted too
    post = block[1:] + [61]
    stop, hit = one(out, block[:W], post[:W], [[9], seq], bs=W, first_pos=3)
    assert (stop, hit) == (1, [len(out) - 1 + ahead, 1])


@gpu
def test_sequence_ending_on_the_bonus_token():
    assert one(OUT, BLOCK, POST, [[24, 30]], first_pos=3) == (1, [10, 0])
    assert one(OUT, BLOCK, POST, [[30]], first_pos=3) == (1, [10, 0])


@gpu
def test_rejected_draft_tokens_never_match():
    """block[5..] were rejected: a sequence that completes only through them must not match (an implementation that
    scans the draft block instead of the commit fails here), nor one through the posterior rows behind the bonus."""
    for seq in ([25], [24, 25], [23, 24, 25, 26], [26, 27], [31], [30, 31], [24, 31]):
        assert one(OUT, BLOCK, POST, [seq], first_pos=3) == (0, [-1, -1]), seq
    # nothing accepted at all: only the bonus token is committed
    assert one(OUT, BLOCK, [50] + POST[1:], [[21]], first_pos=3) == (0, [-1, -1])
    assert one(OUT, BLOCK, [50] + POST[1:], [[20, 50]], first_pos=3) == (1, [6, 0])


@gpu
def test_window_may_not_begin_inside_the_prompt():
    seq = [3, 10, 11, 20, 21]                  # begins at position 2, one token inside the prompt of 3
    assert one(OUT, BLOCK, POST, [seq], first_pos=3) == (0, [-1, -1])
    assert one(OUT, BLOCK, POST, [seq[1:]], first_pos=3) == (1, [6, 0])     # the same window one position later
    assert one(OUT, BLOCK, POST, [seq], first_pos=2) == (1, [6, 0])


@gpu
def test_min_end():
    assert one(OUT, BLOCK, POST, [[22, 23]], first_pos=3, min_end=9) == (0, [-1, -1])    # one above the match end
    assert one(OUT, BLOCK, POST, [[22, 23]], first_pos=3, min_end=8) == (1, [8, 0])      # exactly at it
    # a later occurrence past min_end still counts
    assert one(OUT, [20, 21, 22, 21, 22, 0, 0, 0], [21, 22, 21, 22, 30, 0, 0, 0], [[21, 22]], first_pos=3,
               min_end=8) == (1, [9, 0])


@gpu
def test_ties_and_order():
    # two sequences ending on the same position: the lower index
    assert one(OUT, BLOCK, POST, [[22, 23], [23]], first_pos=3) == (1, [8, 0])
    assert one(OUT, BLOCK, POST, [[23], [22, 23]], first_pos=3) == (1, [8, 0])
    assert one(OUT, BLOCK, POST, [[5], [21, 22, 23], [23]], first_pos=3) == (1, [8, 1])
    # two matches in one commit: the smaller end, whatever the index
    assert one(OUT, BLOCK, POST, [[24], [22]], first_pos=3) == (1, [7, 1])
    assert one(OUT, BLOCK, POST, [[30], [21, 22, 23, 24], [20, 21]], first_pos=3) == (1, [6, 2])


@gpu
def test_first_hit_sticks():
    assert one(OUT, BLOCK, POST, [[22, 23]], first_pos=3, hit=(4, 5), stop=1) == (1, [4, 5])
    # stopped by a stop id before (no hit yet): the sequence is recorded, the word stays 1
    assert one(OUT, BLOCK, POST, [[22, 23]], first_pos=3, stop=1) == (1, [8, 0])
    # a half-written record is no "none yet"
    assert one(OUT, BLOCK, POST, [[22, 23]], first_pos=3, hit=(-1, 3)) == (1, [-1, 3])


@gpu
def test_idle_and_empty_slots_are_untouched():
    slots = [slot(OUT, BLOCK, POST, [[22, 23]], bs=0, first_pos=3, hit=(-7, -9)),           # idle: the record's BS is 0
             slot(OUT, BLOCK, POST, [], first_pos=3, hit=(-7, -9)),                         # no sequences
             slot(OUT, BLOCK, POST, [[22, 23]], first_pos=3)]
    dyn, hit = run(slots)
    assert [d[SR.STOP] for d in dyn] == [0, 0, 1] and hit == [[-7, -9], [-7, -9], [8, 0]]
    # a host block size of 0: nothing is launched
    dyn, hit = run(slots, host_bs=0)
    assert [d[SR.STOP] for d in dyn] == [0, 0, 0] and hit == [[-7, -9], [-7, -9], [-1, -1]]


@gpu
@pytest.mark.parametrize("bs", [1, 16, 32])
@pytest.mark.parametrize("from_record", [False, True])
def test_block_sizes(bs, from_record):
    """bs = 1: acc = 0, the one committed token is posterior[0]; 16 and 32: everything accepted, the sequence ends on the
    last draft token and on the bonus."""
    out = [1, 2, 3, 50]
    block = [50] + list(range(100, 100 + bs - 1))
    post = block[1:] + [77]
    host = None if from_record else bs
    rec = bs if from_record else 5                      # (a host value overrides the record's)
    last = 3 + bs
    assert one(out, block, post, [[77]], bs=rec, host_bs=host, first_pos=3) == (1, [last, 0])
    if bs > 1:
        assert one(out, block, post, [[block[-1]]], bs=rec, host_bs=host, first_pos=3) == (1, [last - 1, 0])
        assert one(out, block, post, [block[-2:] + [77]], bs=rec, host_bs=host, first_pos=3) == (1, [last, 0])
    assert one(out, block, post, [[78]], bs=rec, host_bs=host, first_pos=3) == (0, [-1, -1])


@gpu
def test_four_slots_four_tables():
    slots = [slot(OUT, BLOCK, POST, [[22, 23], [30]], first_pos=3),
             slot([4, 4, 4, 4, 9], [9, 1, 2, 3], [1, 2, 5, 6], [[2, 3], [2, 5]], first_pos=2),
             slot(OUT, BLOCK, POST, [[25]], first_pos=3),
             slot([6] * 20, [6] * 16, [6] * 16, [[6] * 16, [6] * 15], first_pos=16, min_end=30)]
    dyn, hit = run(slots)
    assert [d[SR.STOP] for d in dyn] == [1, 1, 0, 1]
    assert hit == [[8, 0], [7, 1], [-1, -1], [30, 1]]


@gpu
def test_length_one_sequence_is_a_stop_id():
    """The stop word the accept launch gives for an id as a stop id = the one it carries for the same id as a sequence."""
    from dflash_amd import ops
    for tok in (22, 30, 25, 31, 20):          # accepted, the bonus, rejected, behind the bonus, block[0] (committed before)
        words = []
        for as_seq in (False, True):
            block = torch.tensor(BLOCK, dtype=I64, device=dev())
            post = torch.tensor(POST, dtype=I64, device=dev())
            out = torch.full((N,), MASK, dtype=I64, device=dev())
            out[:len(OUT)] = torch.tensor(OUT, dtype=I64)
            dyn = torch.tensor([0, 0, 8, 0, 5, 0, 0, 0], dtype=I32, device=dev())
            res = torch.zeros(4, dtype=I32, device=dev())
            stop_ids = None
            if as_seq:
                st = ops.stop_seq_state(1, dev())
                ops.stop_seq_set(st, 0, [[tok]], first_pos=3)
                ops.stop_seq_rows(block, post, out, dyn, st, bs=8)
            else:
                stop_ids = torch.tensor([tok], dtype=I64, device=dev())
            ops.accept_commit(block, post, 8, out, dyn, stop_ids, res)
            torch.cuda.synchronize()
            assert res.tolist()[:2] == [4, 10]
            words.append((int(dyn[SR.STOP]), int(res[2])))
        # (block[0] is the one difference: the accept launch tests it again every cycle, the sequence launch tested it in
        # the cycle — or the admission — that committed it)
        assert words[0] == words[1] or tok == 20, (tok, words)
        assert words[1] == ((1, 1) if tok in (22, 30) else (0, 0)), (tok, words)


def random_slots(seed=20, n=256):
    rng = random.Random(seed)
    slots = []
    for _ in range(n):
        n_in = rng.randint(1, 5)
        start = n_in + rng.randint(0, 10)
        out = [rng.randrange(4) for _ in range(start + 1)]
        bs = rng.randint(1, 16)
        block = [out[-1]] + [rng.randrange(4) for _ in range(bs - 1)]
        post = [block[i + 1] if i + 1 < bs and rng.random() < 0.75 else rng.randrange(4) for i in range(bs)]
        seqs = [[rng.randrange(4) for _ in range(rng.randint(1, 4))] for _ in range(rng.randint(1, 3))]
        min_end = rng.choice([0, 0, start + rng.randint(0, 4)])
        slots.append(slot(out, block, post, seqs, first_pos=n_in, min_end=min_end))
    return slots


@gpu
def test_random_cases():
    slots = random_slots()
    hits = 0
    for c in slots:   # the model alone, before any launch: hits and misses are both common
        hits += SR.match(c["block"], c["post"], c["out"], c["start"], c["bs"], c["seqs"], c["first_pos"],
                         c["min_end"]) is not None
    assert len(slots) == 256 and hits >= 64 and len(slots) - hits >= 64, hits
    for i in range(0, 256, 64):      # four launches of 64 slots, every slot with a table of its own
        run(slots[i:i + 64])
