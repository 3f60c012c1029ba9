"""The plain-Python record model (records_ref.py) checked before it judges any kernel: against the reference's accept
goldens, against itself across its three forms, and against the literal records BatchedDecoder.admit writes."""
import json
import os

import pytest

import helpers as H
import records_ref as RR

GOLD = json.load(open(os.path.join(H.GOLDEN, "accept.json")))


def _pair(bs, acc, base=100):
    """block / posterior whose first mismatch sits at `acc`, with the positions after it matching again."""
    block = [base + i for i in range(bs)]
    post = [block[i + 1] if i + 1 < bs else base + 900 for i in range(bs)]
    if acc < bs - 1:
        post[acc] = base + 500
    return block, post


def test_accept_reproduces_all_goldens():
    assert len(GOLD) == 17
    for c in GOLD:
        out = [9999] * len(c["out"])
        acc, ns, hit = RR.accept(c["block"], c["posterior"], c["bs"], c["start"], out, len(out), ())
        assert (acc, ns, hit, out) == (c["acc"], c["new_start"], False, c["out"])


def test_accept_clips_and_still_counts():
    block, post = _pair(8, 5)
    out = [-1] * 12
    acc, ns, hit = RR.accept(block, post, 8, 9, out, 11, (post[5],))     # 7 tokens from 9: only 9, 10 fit
    assert (acc, ns, hit) == (5, 15, True)                              # the clipped bonus token still stops
    assert out == [-1] * 9 + block[:2] + [-1]
    assert RR.accept(block, post, 8, 0, [-1] * 12, 12, (post[6], block[7]))[2] is False   # rejected ids do not stop


@pytest.mark.parametrize("bs", range(1, 33))
def test_tile_shares_and_forms_agree(bs):
    for acc in range(bs):
        block, post = _pair(bs, acc)
        start = 40 + bs
        # single form (+ _rearm_t's dyn_t)
        dyn = [901, 902, bs, 903, start, 0, 4, 907]
        dyn_t1 = [911, 912, 913, 914, 915, 916, 917, 918]
        res1, out1, nb1 = [-1] * 4, [-5] * 120, [-9] * 40
        assert RR.single_cycle(block, post, bs, out1, 120, dyn, (), res1, nb1, 32, 7, dyn_t1) == acc
        # batch form on one request, with per-tile records
        dd, dt = [[901, 902, bs, 903, start, 0, 4, 907]], [[911, 912, 913, 914, 915, 916, 917, 918]]
        res, out, nb = [[-1] * 4], [[-5] * 120], [[-9] * 40]
        ddt = [[100 * j + w for w in range(8)] for j in (1, 2)]
        dtt = [[100 * j + w for w in range(8)] for j in (3, 4)]
        assert RR.batch_cycle(1, [block], [post], out, 120, dd, dt, (), res, nb, 7, 2, ddt, dtt) == [acc]
        assert dd[0] == dyn and res[0] == res1 and out[0] == out1 and nb[0] == nb1
        for w in (RR.S, RR.TAU, RR.POS0, RR.START):
            assert dt[0][w] == dyn_t1[w]
        assert dt[0][RR.BS] == bs and dt[0][RR.STOP] == dyn[RR.STOP] and dt[0][RR.CYCLE] == dyn[RR.CYCLE] == 5
        assert dt[0][7] == 918 and dyn_t1[RR.BS:RR.BS + 1] + dyn_t1[5:] == [913, 916, 917, 918]
        # the tiles' shares add up, tile 1 starts 16 rows after tile 0
        assert ddt[0][RR.TAU] + ddt[1][RR.TAU] == acc + 1 == dyn[RR.TAU]
        assert dtt[0][RR.BS] + dtt[1][RR.BS] == bs
        assert ddt[1][RR.S] == ddt[0][RR.S] + 16 == start + 16 and ddt[1][RR.POS0] == ddt[0][RR.POS0] + 16
        assert all(0 <= t[RR.TAU] <= 16 for t in ddt) and all(0 <= t[RR.BS] <= 16 for t in dtt)
        for j in range(2):
            assert ddt[j][RR.START] == dtt[j][RR.S] == dtt[j][RR.POS0] == dtt[j][RR.START] == start + acc + 1
            assert dtt[j][RR.TAU] == 0
            assert [ddt[j][w] for w in (2, 5, 6, 7)] == [100 * (j + 1) + w for w in (2, 5, 6, 7)]     # not named: kept
            assert [dtt[j][w] for w in (5, 6, 7)] == [100 * (j + 3) + w for w in (5, 6, 7)]
        # one tile per request with the per-tile records being the per-request ones: nothing changes
        if bs <= 16:
            dd2, dt2 = [[901, 902, bs, 903, start, 0, 4, 907]], [[911, 912, 913, 914, 915, 916, 917, 918]]
            RR.batch_cycle(1, [block], [post], [[-5] * 120], 120, dd2, dt2, (), None, None, 7, 1, dd2, dt2)
            assert dd2 == dd and dt2 == dt


def test_idle_request_changes_nothing():
    dd, dt = [[1, 2, 0, 3, 4, 5, 6, 7]], [[8, 9, 10, 11, 12, 13, 14, 15]]
    res, out, nb, tl = [[-1] * 4], [[-5] * 20], [[-9] * 16], [[-3] * 8, [-4] * 8]
    assert RR.batch_cycle(1, [[5] * 16], [[5] * 16], out, 20, dd, dt, (5,), res, nb, 7, 1, tl[:1], tl[1:]) == [None]
    assert (dd, dt, res, out, nb, tl) == ([[1, 2, 0, 3, 4, 5, 6, 7]], [[8, 9, 10, 11, 12, 13, 14, 15]], [[-1] * 4],
                                          [[-5] * 20], [[-9] * 16], [[-3] * 8, [-4] * 8])


@pytest.mark.parametrize("P", [1, 7, 16, 17, 200])
def test_admit_equals_the_batched_decoder_records(P):
    """The two literal records of BatchedDecoder.admit (dflash_amd/batch.py), copied here as data."""
    BW, n_tail = 16, min(16, P)
    Sd = P - n_tail
    want_d = [Sd, n_tail, BW, Sd, P, 0, 0, 0]
    want_t = [P, 0, BW, P, P, 0, 0, 0]
    prompt = list(range(50, 50 + P))
    out, blk, post, res = [-1] * (P + 9), [-2] * 20, [-3] * 20, [-4] * 5
    dd, dt, seeds = [91] * 8, [92] * 8, [5, 6, 7]
    rows = RR.admit(prompt, 4242, out, P + 6, blk, post, 16, res, n_tail, dd, dt, BW, 99, seeds, 1, 31337)
    assert dd == want_d and dt == want_t
    assert out == prompt + [4242] + [99] * 5 + [-1] * 3
    assert blk == [4242] + [99] * 15 + [-2] * 4 and post == [0] * 16 + [-3] * 4 and res == [0] * 4 + [-4]
    assert seeds == [5, 31337, 7] and rows == list(range(n_tail)) + [None] * (16 - n_tail)


def test_setters():
    rec = [9] * 8
    RR.set_dyn(rec, 40, 3, 16, 37)
    assert rec == [40, 3, 16, 37, 40, 0, 0, 0]
    recs = [9] * 18
    RR.set_dyn2(recs, 5, 17, 32, 7)
    assert recs == [5, 16, 16, 7, 24, 0, 0, 0, 5, 1, 16, 7, 24, 0, 0, 0, 9, 9]
    RR.set_dyn2(recs, 5, 16, 5, 7)
    assert recs[:16] == [5, 16, 5, 7, 23, 0, 0, 0, 5, 0, 0, 7, 23, 0, 0, 0]
