"""Slot refill of the ragged batch without a GPU: the scheduling decisions (dflash_amd.slots.SlotLoop) driven by a fake
decoder, the host-side mirror of the workload tests/test_hip_stream.py runs, and the capacity check of submit()."""
import math

import pytest

import helpers as H

MAX_NEW = [12, 96, 20, 150, 30, 8, 120, 40, 16, 64]
CYCLES = [2, 13, 4, 19, 4, 2, 13, 5, 2, 7]


def _plan_cycles(max_new, plan, block=16):
    """Mirror of the decode loop's rule: a cycle commits min(plan[call], bs - 1) + 1 tokens, bs = max(1, min(block, left))."""
    left, call = max_new, 0
    while left > 0:
        bs = max(1, min(block, left))
        left -= min(plan[call], bs - 1) + 1
        call += 1
    return call


def _static(cycles, group):
    return sum(max(cycles[g:g + group]) for g in range(0, len(cycles), group))


class FakeDecoder:
    """The driver protocol of dflash_amd.slots with no device behind it.  A request's payload is either an int (it
    commits ONE token per cycle, so max_new_tokens = its cycle count) or an acceptance plan (it commits
    min(plan[call], bs - 1) + 1 tokens per cycle, what the scripted hooks of the GPU tests make the real decoder do)."""

    def __init__(self, slots):
        self.req = [None] * slots
        self.live = [False] * slots
        self.bs = [16] * slots
        self.calls = [0] * slots
        self.start = [0] * slots
        self.log = []          # (event, slot, rid)
        self.occupancy = []    # rids per slot at every cycle
        self.pending = False

    def admit(self, slot, request):
        assert self.req[slot] is None and not self.live[slot], "slot holds two requests"
        self.req[slot], self.live[slot], self.calls[slot], self.start[slot] = request, True, 0, request.n_in
        self.bs[slot] = 16
        self.log.append(("admit", slot, request.rid))

    def set_block_size(self, slot, bs):
        assert self.live[slot]
        self.bs[slot] = bs

    def park(self, slot):
        self.live[slot] = False
        self.log.append(("park", slot, self.req[slot].rid))

    def retire(self, slot, request):
        assert self.req[slot] is request and not self.live[slot]
        self.req[slot] = None
        self.log.append(("retire", slot, request.rid))

    def ahead_pending(self):
        return self.pending

    def cycle(self, ahead_ok):
        assert any(self.live), "a cycle with no live slot"
        self.occupancy.append([r.rid if r is not None and self.live[s] else None for s, r in enumerate(self.req)])
        out = []
        for s, r in enumerate(self.req):
            if not self.live[s]:
                out.append(None)
                continue
            left = r.max_len - self.start[s]
            assert self.bs[s] == max(1, min(16, left)), "tail clamp"
            plan = r.payload
            n = 1 if isinstance(plan, int) else min(plan[self.calls[s]], self.bs[s] - 1) + 1
            self.calls[s] += 1
            self.start[s] += n
            out.append((n, self.start[s], False))
        return out


def _loop(slots, **kw):
    from dflash_amd.slots import SlotLoop
    dec = FakeDecoder(slots)
    return SlotLoop(dec, slots, 16, **kw), dec


def _check_run(loop, dec, done, cycles):
    n = len(cycles)
    assert [r.rid for r in done] == list(range(n))                               # results in submission order
    assert [len(r.taus) for r in done] == cycles
    admits = [e for e in dec.log if e[0] == "admit"]
    assert [e[2] for e in admits] == list(range(n))                              # admitted once each, in submission order
    assert sorted(e[2] for e in dec.log if e[0] == "retire") == list(range(n))   # finished once each
    assert loop.stats["admissions"] == n
    assert loop.stats["live_slot_cycles"] == sum(cycles)
    assert loop.stats["group_cycles"] == len(dec.occupancy)
    for occ in dec.occupancy:
        rids = [x for x in occ if x is not None]
        assert len(rids) == len(set(rids))                                       # no request in two slots
    assert loop.idle


def test_refill_runs_the_workload_in_20_group_cycles():
    loop, dec = _loop(4)
    for c in CYCLES:
        loop.submit(10, c, payload=c)   # one token per cycle: c cycles
    done = loop.run()
    _check_run(loop, dec, done, CYCLES)
    static = _static(CYCLES, 4)
    assert static == 39
    assert loop.stats["group_cycles"] == 20 < static
    assert loop.stats["group_cycles"] >= max(math.ceil(sum(CYCLES) / 4), max(CYCLES))
    # the first free slot takes the next request: 4 and 5 follow 0 and 2 into their slots
    assert [e[1:] for e in dec.log if e[0] == "admit"][:6] == [(0, 0), (1, 1), (2, 2), (3, 3), (0, 4), (2, 5)]


def test_plan_mirror_pins_the_workload():
    cyc = [_plan_cycles(n, H.make_plan(64, 16, 200 + i)) for i, n in enumerate(MAX_NEW)]
    assert cyc == CYCLES and sum(cyc) == 71
    loop, dec = _loop(4)
    for i, n in enumerate(MAX_NEW):
        loop.submit(5 + 3 * i, n, payload=H.make_plan(64, 16, 200 + i))
    done = loop.run()
    _check_run(loop, dec, done, CYCLES)
    assert [r.start - r.n_in for r in done] == MAX_NEW   # (the tail clamp ends every request exactly at its length)
    assert loop.stats["group_cycles"] == 20 and _static(cyc, 4) == 39


@pytest.mark.parametrize("slots", [1, 2, 3])
def test_fewer_slots(slots):
    loop, dec = _loop(slots)
    for c in CYCLES:
        loop.submit(3, c, payload=c)
    done = loop.run()
    _check_run(loop, dec, done, CYCLES)
    g = loop.stats["group_cycles"]
    assert max(math.ceil(sum(CYCLES) / slots), max(CYCLES)) <= g <= _static(CYCLES, slots)
    if slots == 1:
        assert g == sum(CYCLES)


def test_fewer_requests_than_slots_and_empty_queue():
    loop, dec = _loop(4)
    assert loop.idle and loop.step() == [] and loop.run() == []
    assert loop.stats["group_cycles"] == 0 and dec.log == []
    for c in (3, 5):
        loop.submit(7, c, payload=c)
    done = loop.run()
    _check_run(loop, dec, done, [3, 5])
    assert loop.stats["group_cycles"] == 5
    assert all(occ[2] is None and occ[3] is None for occ in dec.occupancy)


def test_requests_submitted_while_others_run():
    loop, dec = _loop(2)
    loop.submit(4, 6, payload=6)
    assert loop.step() == [] and loop.step() == []
    loop.submit(4, 2, payload=2)          # a slot is free: admitted at the next step, runs beside request 0
    loop.submit(4, 3, payload=3)          # waits for a slot
    fin = loop.step()
    assert fin == [] and dec.occupancy[-1] == [0, 1]
    fin = loop.step()
    assert [r.rid for r in fin] == [1] and dec.occupancy[-1] == [0, 1]
    done = fin + loop.run()
    assert sorted(r.rid for r in done) == [0, 1, 2]
    assert [e[1:] for e in dec.log if e[0] == "admit"] == [(0, 0), (1, 1), (1, 2)]
    assert loop.stats["group_cycles"] == 7 and loop.stats["live_slot_cycles"] == 11
    # a second queue after the first drained: same loop, same slots
    loop.submit(4, 1, payload=1)
    assert [r.rid for r in loop.run()] == [3] and loop.stats["admissions"] == 4


def test_zero_new_tokens_finishes_at_admission():
    loop, dec = _loop(2)
    loop.submit(9, 0, payload=1)
    loop.submit(9, 2, payload=2)
    done = loop.run()
    assert [len(r.taus) for r in done] == [0, 2] and loop.stats["group_cycles"] == 2


def test_no_admission_between_a_run_ahead_draft_and_its_verify():
    loop, dec = _loop(2)
    loop.submit(4, 100, payload=100)
    real_cycle = dec.cycle
    seen = []

    def cycle(ahead_ok):
        seen.append(ahead_ok)
        out = real_cycle(ahead_ok)
        dec.pending = ahead_ok          # the decoder drafts the next cycle ahead when it may
        return out

    dec.cycle = cycle
    loop.step()
    assert seen == [True] and dec.pending
    loop.submit(4, 50, payload=50)      # arrives while the run-ahead draft is in flight
    loop.step()
    assert dec.occupancy[-1] == [0, None], "admitted between the run-ahead draft and its verify"
    assert seen[-1] is False and not dec.pending       # (a request waits for a free slot: no further run-ahead)
    loop.step()
    assert dec.occupancy[-1] == [0, 1]
    # stop ids: any cycle may end a request, so never ahead
    loop2, dec2 = _loop(2, may_stop=True)
    loop2.submit(4, 100, payload=100)
    seen2 = []
    rc2 = dec2.cycle
    dec2.cycle = lambda a: (seen2.append(a), rc2(a))[1]
    loop2.step()
    assert seen2 == [False]


def test_submit_rejects_what_cannot_fit_before_touching_the_decoder():
    from dflash_amd.engine import BatchEngine, check_fit
    check_fit(100, 50, 100 + 50 + 48, 100 + 50 + 16)
    with pytest.raises(ValueError, match="max_rows"):
        check_fit(100, 50, 100 + 50 + 47, 1000)
    with pytest.raises(ValueError, match="out_len"):
        check_fit(100, 50, 1000, 100 + 50 + 15)
    with pytest.raises(ValueError):
        check_fit(0, 5, 1000, 1000)

    class Boom:
        max_rows, out_len = 198, 166

        def __getattr__(self, name):
            raise AssertionError(f"submit touched the decoder ({name})")

    from dflash_amd.slots import SlotLoop
    eng = BatchEngine.__new__(BatchEngine)       # no GPU here: the engine's queue over a decoder that must not be reached
    eng.dec = Boom()
    eng.loop = SlotLoop(eng.dec, 4, 16)
    import torch
    assert eng.submit(torch.zeros(1, 100, dtype=torch.int64), 50) == 0
    with pytest.raises(ValueError):
        eng.submit(torch.zeros(1, 101, dtype=torch.int64), 50)
    with pytest.raises(ValueError):
        eng.submit(torch.zeros(100, dtype=torch.int64), 5)
    assert len(eng.loop.queue) == 1


def test_engine_scope():
    from dflash_amd.engine import BatchEngine, dflash_generate_stream
    with pytest.raises(NotImplementedError):
        BatchEngine(None, None, max_rows=100, out_len=100, mask_token_id=0, block_size=24)
    with pytest.raises(NotImplementedError):
        dflash_generate_stream(None, None, [], 0, 8, 17, None)
    with pytest.raises(ValueError):
        BatchEngine(None, None, max_rows=100, out_len=100, mask_token_id=0, temperature=0.7, sampler="torch", graph=True)


def test_admit_slot_validates_without_gpu():
    """dfl_admit_slot rejects bad arguments before any launch.  The entry point checks the scalars first and the
    pointers last, and every scalar case below ALSO passes a null pointer, so no call here can reach a launch."""
    from dflash_amd import _lib
    h = _lib.lib()
    ok = dict(r=0, n=4, P=5, out_stride=64, out_len=64, blk_w=16, ld=1024, n_tail=5, fc_in=1024, bs=16)

    def call(null="prompt", **kw):
        k = {**ok, **kw}
        p = lambda name: None if name == null else 16   # noqa: E731  (never dereferenced: validation only)
        return h.dfl_admit_slot(k["r"], k["n"], p("prompt"), k["P"], p("first"), p("out"), k["out_stride"], k["out_len"],
                                p("block"), p("post"), k["blk_w"], p("result"), p("tail"), k["ld"], k["n_tail"], p("taps"),
                                k["fc_in"], p("dyn_d"), p("dyn_t"), k["bs"], None, 0, 0, None)

    for name in ("prompt", "first", "out", "block", "post", "result", "tail", "taps", "dyn_d", "dyn_t"):
        assert call(null=name) == -22, name
        assert b"null" in h.dfl_last_error()
    for kw, text in ((dict(r=4), b"slot"), (dict(r=-1), b"slot"), (dict(P=64), b"does not fit"), (dict(P=0), b"does not fit"),
                     (dict(n_tail=17), b"n_tail"), (dict(n_tail=-1), b"n_tail"), (dict(n_tail=6), b"n_tail"),
                     (dict(fc_in=1020), b"fc_in"), (dict(bs=17), b"bs=")):
        assert call(**kw) == -22, kw
        assert text in h.dfl_last_error(), (kw, h.dfl_last_error())
