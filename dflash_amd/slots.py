"""Slot scheduling of the refilling ragged batch (dflash_amd.engine): which queued request goes into which slot at
which step, when a block is clamped, when a slot frees.  Pure Python, no torch, no GPU: the decoder is reached through
a small driver protocol, so the decisions can be driven by a fake decoder on the CPU.

Driver protocol (BatchEngine's adapter over BatchedDecoder, or a fake):
    admit(slot, request)            prefill `request` into `slot`; afterwards its start is request.n_in
    set_block_size(slot, bs)        tail clamp of a live slot
    cycle(ahead_ok) -> list         one group cycle; per slot None (idle) or (tau, new_start, stop)
    park(slot)                      the slot's request has ended: the slot does no work until re-admitted
    retire(slot, request)           the request's results can be collected (called once, before the slot is reused)
    ahead_pending() -> bool         a run-ahead draft of the NEXT cycle is already enqueued: no admission until its
                                    verify has run
"""
from __future__ import annotations

from collections import deque
from typing import Any, Optional


class Request:
    """One queued / running / finished request as the scheduler sees it."""

    __slots__ = ("rid", "n_in", "max_new_tokens", "max_len", "payload", "slot", "start", "taus", "stopped", "done",
                 "admitted_step", "finished_step")

    def __init__(self, rid: int, n_in: int, max_new_tokens: int, payload: Any = None):
        self.rid, self.n_in, self.max_new_tokens, self.payload = rid, n_in, max_new_tokens, payload
        self.max_len = n_in + max_new_tokens
        self.slot: Optional[int] = None
        self.start = n_in
        self.taus: list = []
        self.stopped = self.done = False
        self.admitted_step = self.finished_step = None


class SlotLoop:
    """First come, first served refill of `slots` decoder slots.

    step() is one group cycle: requests submitted since the last step are admitted into free slots, every live slot's
    block is clamped to what its request has left (bs = max(1, min(block_size, left)), benchmark.py:104-105), the
    driver runs one cycle, requests that ended (stop id, length) are parked and retired, and every free slot is
    filled from the queue in submission order, lowest slot first.

    may_stop: stop ids are set, so any cycle may end a request (no run-ahead draft then); stop_always: the mask id is
    itself a stop id, every request ends after one cycle (the rule of dflash_generate_batch)."""

    def __init__(self, driver, slots: int, block_size: int = 16, may_stop: bool = False, stop_always: bool = False,
                 stats: Optional[dict] = None):
        if slots < 1:
            raise ValueError("slots >= 1")
        if block_size < 1:
            raise ValueError("block_size >= 1")
        self.driver, self.slots, self.block_size = driver, slots, block_size
        self.may_stop, self.stop_always = may_stop, stop_always
        self.queue: deque = deque()
        self.slot_req: list = [None] * slots
        self.next_rid = 0
        self.steps = 0
        self.stats = stats if stats is not None else {}   # (the caller's dict: the engine keeps its counters beside these)
        for k in ("group_cycles", "live_slot_cycles", "admissions"):
            self.stats.setdefault(k, 0)

    # ------------------------------------------------------------------ queue
    def submit(self, n_in: int, max_new_tokens: int, payload: Any = None) -> Request:
        if n_in < 1 or max_new_tokens < 0:
            raise ValueError("a request has a prompt of at least one id and max_new_tokens >= 0")
        req = Request(self.next_rid, n_in, max_new_tokens, payload)
        self.next_rid += 1
        self.queue.append(req)
        return req

    @property
    def idle(self) -> bool:
        return not self.queue and all(r is None for r in self.slot_req)

    def live_slots(self) -> list:
        return [s for s, r in enumerate(self.slot_req) if r is not None]

    # ------------------------------------------------------------------ decisions
    def clamp(self, req: Request) -> int:
        return max(1, min(self.block_size, req.max_len - req.start))

    def ahead_ok(self) -> bool:
        """The existing run-ahead rule (dflash_generate_batch): the next cycle runs with the same live requests and
        block sizes — no stop ids, nobody within two blocks of its end — and, here, nothing waits for a free slot."""
        if self.may_stop or self.stop_always:
            return False
        if self.queue and any(r is None for r in self.slot_req):
            return False
        return all(r.start + 2 * self.block_size <= r.max_len for r in self.slot_req if r is not None)

    def _finish(self, slot: int, req: Request, finished: list) -> None:
        req.done, req.finished_step, req.slot = True, self.steps, slot
        self.driver.park(slot)
        self.driver.retire(slot, req)
        self.slot_req[slot] = None
        finished.append(req)

    def _fill(self, finished: list) -> None:
        if self.driver.ahead_pending():   # never between a run-ahead draft and its verify
            return
        while self.queue:
            free = [s for s, r in enumerate(self.slot_req) if r is None]
            if not free:
                return
            slot, req = free[0], self.queue.popleft()
            self.slot_req[slot] = req
            req.slot, req.admitted_step = slot, self.steps
            self.driver.admit(slot, req)
            self.stats["admissions"] += 1
            if req.start >= req.max_len:   # nothing to generate
                self._finish(slot, req, finished)

    # ------------------------------------------------------------------ one group cycle
    def step(self) -> list:
        finished: list = []
        self._fill(finished)
        live = self.live_slots()
        if not live:
            return finished
        for s in live:
            self.driver.set_block_size(s, self.clamp(self.slot_req[s]))
        out = self.driver.cycle(self.ahead_ok())
        self.steps += 1
        self.stats["group_cycles"] += 1
        self.stats["live_slot_cycles"] += len(live)
        for s in live:
            req = self.slot_req[s]
            tau, new_start, stop = out[s]
            req.taus.append(tau)
            req.start = new_start
            req.stopped = bool(stop)
            if stop or self.stop_always or req.start >= req.max_len:
                self._finish(s, req, finished)
        self._fill(finished)
        return finished

    def run(self) -> list:
        """Drain the queue; the requests that finished, in submission order."""
        done: list = []
        while not self.idle:
            done.extend(self.step())
        return sorted(done, key=lambda r: r.rid)

