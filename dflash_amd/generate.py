"""Decode loops over the HIP hot path, with the reference's call signatures and
return fields:

* `dflash_generate`        — benchmark.py:44-251 (fixed block, tail clamp,
                             block_size==1 baseline, draft_steps, per-cycle profile)
* `dflash_generate_policy` — benchmark_dynamic_schedule.py:260-434 (block size from
                             `EWMAPerformanceScheduler` every cycle)
* `DFlashDraftModel.spec_generate` (model.py) — model/dflash.py:192-277

All three drive a `DecodeSession` (prefill once, then `cycle()` per block), which
bench.py also steps directly.  Per cycle the host enqueues: draft forward + fused
lm_head/argmax (kernels), the caller's target forward (PyTorch-ROCm, outside the
path), the posterior argmax kernel and the accept/commit kernel; the only
device->host read is the 4-int accept result the loop needs to slice the
target's hidden states and roll its cache back.
"""
from __future__ import annotations

import gc
import os
import time
from types import SimpleNamespace
from typing import Callable, NamedTuple, Optional

import torch

from . import ops
from .logits_stage import LogitsStage, check_features, draw_rows as _draw_rows
from .utils import extract_context_feature, sample

_TABLES = {}
MAX_BLOCK = 32  # rows per block the kernels take: two 16-row tiles


def cuda_time() -> float:
    torch.cuda.synchronize()
    return time.perf_counter()


def capture_graph(fn) -> "torch.cuda.CUDAGraph":
    """Capture fn()'s launches into a hipGraph WITHOUT `torch.cuda.graph()`'s preamble.  That context manager calls
    `torch.cuda.empty_cache()` before it begins a capture: every block in torch's caching allocator goes back to the
    driver — with a NativeTarget(keep_hf=False) that is the ~17 GB of the wrapped model's dropped weights — and the driver
    clears released VRAM in the background, on the GPU, for the next few hundred milliseconds.  Every kernel that runs
    meanwhile is 2 - 4 % slower (measured, round 4: DESIGN.md section 5, profiles/r4_graph_ab.txt; rounds 2 - 3 read this
    as "kernels are slower once a graph exists").  Nothing here needs the cache emptied: the launches allocate nothing."""
    g = torch.cuda.CUDAGraph()
    cur = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    # No garbage collection while the stream captures: a collection that frees an unreachable hipGraph (a dropped
    # session or decoder held in a reference cycle) destroys it inside the capture, which HIP refuses ("operation not
    # permitted when stream is capturing") and torch turns into an abort.  torch.cuda.graph() collects before it begins
    # for the same reason; pausing the collector for the ~300 launches of a capture needs no collection here.
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.stream(side):
            g.capture_begin()
            try:
                fn()
            finally:
                g.capture_end()
    finally:
        if gc_was_on:
            gc.enable()
    cur.wait_stream(side)
    return g


class GraphNotCovered(ValueError):
    """capture / capture_sizes: this session, or the state it is in, is not one the graphs cover.  run_decode answers it
    with eager cycles; anything else a capture raises is a failure and propagates."""


class _Replay(NamedTuple):
    """What a capture leaves behind, for the fixed-size form and for the caller-sized form alike."""
    graphs: dict   # block size -> ([draft + lm_head] graph, [verify + accept] graph)
    bound: int     # upper bound of S / start the captured launches were sized for
    rope: tuple    # addresses of the draft model's and the target's RoPE tables at capture time
    keep: tuple    # every tensor whose address sits in the launches and that the session does not own otherwise


def _new_target_cache(target):
    if hasattr(target, "new_cache"):
        return target.new_cache()
    from transformers import DynamicCache  # the reference's choice (model/dflash.py:214)
    return DynamicCache()


def _taps(hidden_states, layer_ids):
    """extract_context_feature (model/utils.py:16-25); the kernels take bf16 rows, which
    is what a bf16 target (the reference's dtype, benchmark.py:404) already returns."""
    t = extract_context_feature(hidden_states, layer_ids)
    return t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)


def _bf16_table(w, dev):
    if w.dtype == torch.bfloat16 and w.device == dev and w.is_contiguous():
        return w.detach()
    key = (w.data_ptr(), tuple(w.shape), w._version)
    if key not in _TABLES:
        _TABLES.clear()
        _TABLES[key] = w.detach().to(device=dev, dtype=torch.bfloat16).contiguous()
    return _TABLES[key]


SAMPLERS = ("torch", "device")


def resolve_seed(sampler: str, seed: Optional[int], needed: bool = True) -> Optional[int]:
    """sampler="device" without a seed draws one from torch's default generator, so that torch.manual_seed still
    governs reproducibility — only when a draw needs it (`needed`: T > 0), so a greedy run leaves the caller's RNG alone;
    sampler="torch" takes no seed (it draws on the caller's torch RNG)."""
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler={sampler!r}: one of {SAMPLERS}")
    if sampler == "torch":
        if seed is not None:
            raise ValueError("seed needs sampler='device' (sampler='torch' draws on the caller's torch RNG)")
        return None
    if not needed:
        return None if seed is None else int(seed) & 0xFFFFFFFFFFFFFFFF
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def resolve_filter(top_k, top_p, temperature: float, sampler: str) -> Optional[dict]:
    """Validate (top_k, top_p); the keywords of the filtered draw ("Filtered draw") if a filter is on
    and the run samples, else None: at T = 0 the argmax is always kept, so the greedy path runs unchanged."""
    on = ops.check_filter(top_k, top_p)
    if not on or temperature < 1e-5:
        return None
    if sampler != "device":
        raise ValueError("top_k / top_p at T > 0 need sampler='device' (sampler='torch' is the reference's unfiltered "
                         "multinomial)")
    return dict(top_k=int(top_k), top_p=float(top_p))


def check_couple_draft(couple_draft, temperature: float, draft_temperature: Optional[float], sampler: str) -> float:
    """Validate couple_draft against the request and return the draft temperature to run with
    (0.0: a greedy draft).  A coupled draft shares the target's seeded noise: sampler="torch" has none at T > 0, and a
    draft temperature of its own contradicts invT = the target's."""
    dt = 0.0 if draft_temperature is None else float(draft_temperature)
    if not couple_draft:
        return dt
    if draft_temperature is not None and dt != float(temperature):
        raise ValueError(f"couple_draft draws the draft at the target's temperature: draft_temperature={draft_temperature!r} "
                         f"differs from temperature={temperature!r}")
    if temperature >= 1e-5 and sampler != "device":
        raise ValueError("couple_draft at T > 0 needs sampler='device' (sampler='torch' has no seeded noise to share)")
    return dt


def _trim(output_ids, max_length, mask_token_id, stop_token_ids, n_in, stop_hit=None):
    """model/dflash.py:269-275.  stop_hit (the stop sequences' (e, k, L, include) of _stop_hit, or None): see _kept_cols."""
    if stop_hit is not None:
        return output_ids[:, _kept_cols(output_ids, max_length, mask_token_id, stop_token_ids, n_in, stop_hit)]
    output_ids = output_ids[:, :max_length]
    output_ids = output_ids[:, output_ids[0] != mask_token_id]
    if stop_token_ids is not None:
        st = torch.tensor(stop_token_ids, device=output_ids.device)
        idx = torch.isin(output_ids[0][n_in:], st).nonzero(as_tuple=True)[0]
        if idx.numel() > 0:
            output_ids = output_ids[:, : n_in + idx[0] + 1]
    return output_ids


def _kept_cols(output_ids, max_length, mask_token_id, stop_token_ids, n_in, stop_hit=None, which=None):
    """The columns of output_ids that _trim keeps, as indices: what trims a per-position buffer exactly as the ids.
    stop_hit = (e, k, L, include): a stop sequence of L ids (index k) matched with its last id at position e (DESIGN.md
    section 22).  The cut is at the earlier of the first stop id and e; where the sequence decides (e is kept and not
    behind the first stop id), include=False drops the window's L ids too and `which` (a list, optional) receives k."""
    cols = (output_ids[0, :max_length] != mask_token_id).nonzero(as_tuple=True)[0]
    cut = None
    if stop_token_ids is not None:
        st = torch.tensor(stop_token_ids, device=output_ids.device)
        idx = torch.isin(output_ids[0, cols][n_in:], st).nonzero(as_tuple=True)[0]
        if idx.numel() > 0:
            cut = n_in + int(idx[0]) + 1
    if stop_hit is not None and cols.numel() > 0:
        e, k, L, include = stop_hit
        if 0 <= e <= int(cols[-1]) and (cut is None or e <= int(cols[cut - 1])):
            cut = int((cols <= (e if include else e - L)).sum())
            if which is not None:
                which.append(k)
    return cols if cut is None else cols[:cut]


def _stop_hit(state, slot: int, seqs, include: bool):
    """The slot's hit record read back as _kept_cols takes it (with the ids, at the end of the request), or None."""
    if state is None or not seqs:
        return None
    e, k = state.hit[slot].tolist()
    return (e, k, len(seqs[k]), bool(include)) if e >= 0 and 0 <= k < len(seqs) else None


def logprob_fields(sink, row: int, cols: torch.Tensor) -> dict:
    """The three result fields of a request whose generated tokens sit at positions `cols` of the sink's row: logprobs
    fp32 [n], top_logprob_ids int64 [n, N], top_logprobs fp32 [n, N] (N = 0: empty second axis)."""
    n, N = cols.numel(), sink.n_top
    dev = sink.lp.device
    return dict(logprobs=sink.lp[row, cols].clone(),
                top_logprob_ids=sink.top_ids[row, cols].clone() if N else torch.empty(n, 0, dtype=torch.long, device=dev),
                top_logprobs=sink.top_lp[row, cols].clone() if N else torch.empty(n, 0, dtype=torch.float32, device=dev))


NO_LOGPROBS = dict(logprobs=None, top_logprob_ids=None, top_logprobs=None)


def _vocab_of(target) -> int:
    """The vocabulary the logit-bias keywords are validated against: a NativeTarget's V, else the wrapped model's
    config.vocab_size (only to tell neutral values from a request such a target cannot serve)."""
    v = getattr(target, "V", None)
    if v is None:
        v = getattr(getattr(target, "config", None), "vocab_size", None)
    if v is None:
        raise ValueError("logit_bias / allowed_token_ids / banned_token_ids / min_tokens need a dflash_amd.NativeTarget "
                         "(the kernel reads the verify's materialised logits)")
    return int(v)


def first_token_stop(state, slot: int, ids_row: torch.Tensor, n_in: int, dyn_row: Optional[torch.Tensor] = None) -> bool:
    """The first new token (position n_in of ids_row, produced by admission before any accept launch runs) against the
    slot's stop sequences: dfl_stop_seq_rows over a one-row block — a record of its own with START = n_in - 1, whose one
    committed token is the "posterior" ids_row[n_in] — so a length-1 sequence equal to the first token stops the request
    as a stop id does.  dyn_row (the ragged batch: the slot's draft-form record): the stop word is ORed into it on the
    device and nothing is read back (returns False); None: the stop word is read back and returned."""
    rec = torch.zeros(8, dtype=torch.int32, device=ids_row.device)
    rec[ops.DYN_START] = n_in - 1
    one = SimpleNamespace(seq_ids=state.seq_ids[slot:slot + 1], seq_len=state.seq_len[slot:slot + 1],
                          first_pos=state.first_pos[slot:slot + 1], min_end=state.min_end[slot:slot + 1],
                          hit=state.hit[slot:slot + 1])
    first = ids_row[n_in:n_in + 1]
    ops.stop_seq_rows(first, first, ids_row, rec, one, bs=1)
    if dyn_row is not None:
        dyn_row[ops.DYN_STOP] |= rec[ops.DYN_STOP]
        return False
    return bool(rec[ops.DYN_STOP].item())


class DecodeSession:
    """State of one request between cycles (what the reference keeps in local
    variables of its while-loop, model/dflash.py:206-233)."""

    def __init__(self, model, target, input_ids: torch.Tensor, *, mask_token_id: int, max_new_tokens: int,
                 max_block_size: int, stop_token_ids, temperature: float, draft_temperature: Optional[float] = None,
                 draft_token_hook: Optional[Callable] = None, sampler: str = "torch", seed: Optional[int] = None,
                 top_k: int = 0, top_p: float = 1.0, logprobs: Optional[int] = None, repetition_penalty: float = 1.0,
                 presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None,
                 banned_token_ids=None, min_tokens: int = 0, grammar=None, constrain_draft: bool = False, min_p=None,
                 couple_draft: bool = False, stop_sequences=None, include_stop_sequence: bool = True):
        from .target import NativeTarget
        # stop_sequences: multi-token stops matched on the device by one launch in front of every
        # accept launch; None / empty: the launches of before, nothing allocated.  Bad values are refused first
        self.stop_seqs = (ops.check_stop_sequences(stop_sequences, _vocab_of(target), mask_token_id)
                          if stop_sequences is not None else None)
        self.include_stop = bool(include_stop_sequence)
        self._min_tokens = int(min_tokens) if self.stop_seqs else 0
        # couple_draft: at T > 0 every draft token is the argmax of the DRAFT's logits under the
        # noise the TARGET's verify will draw that position with (stream TARGET, the request's seed, the target's invT).
        # The draft then counts as greedy everywhere below — run-ahead, constrain_draft, the fixed-size capture — and only
        # its head launch differs.  At T = 0, or off: every launch is the one enqueued without the keyword
        draft_temperature = check_couple_draft(couple_draft, temperature, draft_temperature, sampler)
        self.couple = bool(couple_draft) and temperature >= 1e-5
        if self.couple:
            draft_temperature = 0.0
        # The row processors on the TARGET's rows (logits_stage.LogitsStage has the order and the DESIGN.md sections).
        # Bad values are refused first; min_p at T = 0 keeps the maximum and is off; every feature at its neutral value
        # leaves every launch below the one enqueued without the keyword
        mp = ops.check_min_p(min_p) if temperature >= 1e-5 else (ops.check_min_p(min_p) and None)
        lb = None
        if not (logit_bias is None and allowed_token_ids is None and banned_token_ids is None and min_tokens == 0):
            lb = ops.check_logit_bias(_vocab_of(target), logit_bias, allowed_token_ids, banned_token_ids, min_tokens,
                                      stop_token_ids)
        pen = ops.check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
        # logprobs = N (None: off): per position of output_ids the log-probability of the committed token and the top N
        # alternatives
        self.logprobs = ops.check_logprobs(logprobs)
        on = dict(min_p=mp is not None, grammar=grammar is not None, logit_bias=lb is not None, penalties=pen is not None,
                  logprobs=self.logprobs is not None)
        check_features([f for f, v in on.items() if v], native=isinstance(target, NativeTarget),
                       sampling=temperature >= 1e-5, seeded=sampler == "device", wide=int(max_block_size) > 16)
        dev = model.device
        if not input_ids.is_cuda:
            raise RuntimeError("dflash_amd: input_ids must be on the GPU")
        if input_ids.shape[0] != 1:
            raise NotImplementedError("batch = 1 per call, as in the reference; shard requests over ranks")
        if not 1 <= int(max_block_size) <= MAX_BLOCK:
            raise ValueError(f"block size {max_block_size}: the gfx950 kernels take blocks of 1..{MAX_BLOCK} rows "
                             f"(two 16-row tiles); checked here, before the target prefill runs")
        self.model, self.target, self.dev = model, target, dev
        self.input_ids = input_ids
        self.mask_token_id, self.temperature = mask_token_id, temperature
        self.draft_temperature, self.hook = draft_temperature, draft_token_hook
        # sampler="device": T > 0 draws are seeded Gumbel-max draws on the device — the target's in
        # its lm_head epilogue (stream TARGET), the draft's likewise (stream DRAFT); None where a draw is greedy
        self.sampler = sampler
        self.seed = resolve_seed(sampler, seed, needed=temperature >= 1e-5 or draft_temperature >= 1e-5)
        self._tseed = self.seed if (self.seed is not None and temperature >= 1e-5) else None
        self._dseed = self.seed if (self.seed is not None and draft_temperature >= 1e-5) else None
        self._couple = dict(seed=self._tseed, temperature=temperature) if self.couple else None
        self._cseed = (torch.tensor([ops.seed_i64(self._tseed)], dtype=torch.long, device=dev) if self.couple else None)
        # top_k / top_p restrict the TARGET's draw (the draft's own draw stays unfiltered: the target's draw alone
        # decides what is emitted); None: the fused unfiltered epilogue
        self._filter = resolve_filter(top_k, top_p, temperature, sampler)
        # T > 0 cycles can be replayed only with the device sampler (the torch draw consumes host RNG state)
        self.replay_sampling_ok = sampler == "device" or (temperature < 1e-5 and draft_temperature < 1e-5)
        self.stop_token_ids = stop_token_ids
        self.max_bs = max_block_size
        self.n_in = input_ids.shape[1]
        self.max_length = self.n_in + max_new_tokens
        self.output_ids = torch.full((1, self.max_length + self.max_bs), mask_token_id, dtype=torch.long, device=dev)
        self.position_ids = torch.arange(self.output_ids.shape[1], device=dev).unsqueeze(0)
        self.native = isinstance(target, NativeTarget)
        self.tcache = (target.new_cache(self.max_length + 2 * self.max_bs) if self.native
                       else _new_target_cache(target))
        self.use_draft = self.max_bs > 1
        self.dcache = model.new_cache(self.max_length + 2 * self.max_bs) if self.use_draft else None
        self.dyn = self.dcache.dyn if self.dcache is not None else torch.zeros(8, dtype=torch.int32, device=dev)
        self.embed_w = _bf16_table(target.model.embed_tokens.weight, dev)
        self.lm_wp = model.packed_lm_head(target.lm_head) if self.use_draft else None
        if self.native and self.lm_wp is not None:
            target.share_lm_head(self.lm_wp)  # one packed copy serves draft unmask and target posterior
        # an fp8 draft model: the DRAFT's greedy unmask streams an e4m3 copy of the lm_head — the fp8 target's own codes
        # where it has them (ONE e4m3 copy serves both), else packed here (a bf16 target keeps its bf16 one)
        self.lm_wp8 = None
        if self.use_draft and getattr(model, "w8", None) is not None:
            self.lm_wp8 = getattr(target, "lm_wp8", None) if self.native else None
            if self.lm_wp8 is None:
                self.lm_wp8 = model.packed_lm_head_fp8(target.lm_head)
        elif self.use_draft and getattr(model, "w4", None) is not None:   # an mxfp4 draft: its own 4-bit copy of the head
            self.lm_wp8 = model.packed_lm_head_mxfp4(target.lm_head)
        self.stop_t = torch.tensor(stop_token_ids, dtype=torch.long, device=dev) if stop_token_ids else None
        # the stop sequences' tables and hit record, slot 0 of a state of its own (None: off); written in prefill()
        self.sq = ops.stop_seq_state(1, dev) if self.stop_seqs else None
        self._hit = None   # the hit record as finish() read it: (e, k, L, include) or None
        self.stop_sequence = None
        # the row processors' state and buffers, slot 0 of a stage of its own (None: nothing is on, and verify is called
        # without it); the slot's values go in with the first token (prefill).  A grammar's pool is exactly the
        # automaton's rows at base 0, validated against the bias row: a reachable state whose legal tokens are all banned
        # is refused here
        self.stage, self._vkw = None, {}
        if any(on.values()) or (self.native and self._filter is not None):
            if grammar is not None:
                ops.check_grammar(grammar, target.V, None if lb is None else lb[0])
            self.stage = LogitsStage(1, target.V, dev, tiles=2 if self.max_bs > 16 else 1, out_len=self.output_ids.shape[1],
                                     logprobs=self.logprobs, penalties=pen is not None, logit_bias=lb is not None,
                                     grammar_states=grammar.num_states if grammar is not None else 0,
                                     min_p=mp is not None, filtering=self._filter is not None,
                                     sampling=temperature >= 1e-5, stop_ids=self.stop_t)
            self._vkw = dict(stage=self.stage)
            self._gr_start = int(grammar.start) if grammar is not None else None
            self._admit = dict(penalties=pen, min_p=mp, flt=self._filter,
                               bias=(lb[0], self.n_in + lb[1] if lb[1] else 0) if lb is not None else None,
                               grammar=(self.stage.load_grammar(grammar, lb[0] if lb is not None and ops.is_byte_grammar(grammar)
                                                                 else None), self._gr_start)
                               if grammar is not None else None)
        # what the session's own code and its observers read of the stage: the logprob sink, the penalty table, the
        # grammar state (None each where the feature is off)
        st = self.stage
        self.lp, self.gr = (st.lp, st.gr) if st is not None else (None, None)
        self.pen = SimpleNamespace(table=st.pen_table) if st is not None and st.pen_table is not None else None
        # the reference scans the whole buffer, mask slots included (model/dflash.py:265-268)
        self.stop_always = stop_token_ids is not None and mask_token_id in stop_token_ids
        # the accept result {acc, new start, stop, cycle}: pinned host memory the kernel writes with one 16-byte store and
        # this thread polls (no blit kernel, no interrupt-driven wake); DFL_HOST_RESULT=0: a device buffer + .tolist()
        self.poll_result = os.environ.get("DFL_HOST_RESULT", "1") != "0"
        self.result = (torch.zeros(4, dtype=torch.int32).pin_memory() if self.poll_result
                       else torch.zeros(4, dtype=torch.int32, device=dev))
        self._res_np = self.result.numpy() if self.poll_result else None
        self.block = torch.empty(1, self.max_bs, dtype=torch.long, device=dev)
        self._dyn_bs = None   # block size for which the draft cache's length record is already armed (see _draft)
        # run-ahead draft (DFL_RUN_AHEAD=0 turns it off): the NEXT cycle's draft forward is enqueued right behind the
        # accept kernel, before the host has read the acceptance length — every length it needs is in the device record
        # the accept kernel has just written — so the GPU does not idle through the host's turnaround (result poll,
        # bookkeeping, ~30 launches: 0.04-0.08 ms per cycle).  _ahead = block size of a draft already in flight.
        self.run_ahead = os.environ.get("DFL_RUN_AHEAD", "1") != "0"
        self._ahead = None
        self._ahead_ev = None
        self._armed = False   # True: the accept kernel has written the next cycle's block (bonus token + mask ids)
        # hipGraph replay (capture / capture_sizes): one _Replay per form, None until captured or after a table moved
        self._fixed = None    # one block size, the next cycle's draft running ahead (cycle_graph)
        self._sized = None    # one pair of graphs per caller-chosen block size (cycle_sized)
        self.start = self.n_in
        self.target_hidden = None
        self.hook_calls = 0
        self.stopped = False
        self.events = None  # set to a dict to have cycle() record (start, end) event pairs per phase
        self.record_events = True  # False: record nothing new, but still hand a run-ahead draft's pairs to self.events
        self.host_times = None  # a list: cycle() appends (seconds enqueueing launches, seconds polling for the result)
        self.draft_logits = None  # set to a bf16 [32, V] buffer to have the draft's logits materialised into it
        # constrain_draft: every greedy draft head below materialises its logits and dfl_grammar_draft_rows re-picks the
        # block's draft tokens under the automaton and the bans ("The draft under the grammar").
        # Off: every launch is the one enqueued without the keyword.  Only the bans of the bias row are read, and only
        # where it has one: a row of finite biases alone leaves nothing to constrain by
        self.constrain = bool(constrain_draft)
        if self.constrain:
            if draft_temperature >= 1e-5:
                raise NotImplementedError("constrain_draft takes a greedy draft (a sampled draft draws in the head launch's "
                                          "epilogue, before the pick)")
            bans = lb is not None and bool(torch.isneginf(lb[0]).any())
            if grammar is None and not bans:
                raise ValueError("constrain_draft needs something to constrain by: a grammar, allowed_token_ids, "
                                 "banned_token_ids or a logit_bias of -inf")
            self._cd_bias = self.stage.lb.bias if bans else None
            self.draft_logits = torch.zeros(16, target.V, dtype=torch.bfloat16, device=dev)
        # the tapped rows live here from a verify to the next draft (own buffer: several
        # sessions may be interleaved on one NativeTarget)
        self.taps_buf = (torch.zeros(32, len(model.target_layer_ids) * model.config.hidden_size, dtype=torch.bfloat16,
                                     device=dev) if (self.native and self.use_draft) else None)

    @torch.inference_mode()
    def prefill(self) -> None:
        """model/dflash.py:218-229."""
        if self.native:
            out = self.target.prefill(self.input_ids, self.tcache, output_hidden_states=self.use_draft,
                                      tap_layers=self.model.target_layer_ids if self.use_draft else None)
        else:
            out = self.target(self.input_ids, position_ids=self.position_ids[:, :self.n_in],
                              past_key_values=self.tcache, use_cache=True, logits_to_keep=1,
                              output_hidden_states=self.use_draft)
        self.output_ids[:, :self.n_in] = self.input_ids
        if self.stage is not None:   # the first new token through the stage's chain, from the prompt's last-row logits
            self.stage.admit(0, out.logits[0, -1:], self.output_ids, self.n_in, temperature=self.temperature,
                             seed=self._tseed, first=self.output_ids[0, self.n_in:self.n_in + 1], **self._admit)
        elif self._tseed is not None:   # the first new token draws position n_in
            self.output_ids[:, self.n_in:self.n_in + 1] = _draw_rows(out.logits[:, -1:], self.temperature, self._tseed,
                                                                     self.n_in, self._filter)
        else:
            self.output_ids[:, self.n_in:self.n_in + 1] = sample(out.logits, self.temperature)
        if self.use_draft:
            self.target_hidden = _taps(out.hidden_states, self.model.target_layer_ids)
        if self.sq is not None:
            ops.stop_seq_set(self.sq, 0, self.stop_seqs, first_pos=self.n_in,
                             min_end=self.n_in + self._min_tokens if self._min_tokens > 0 else 0)
            self.stopped = first_token_stop(self.sq, 0, self.output_ids[0], self.n_in)

    def _stop_seq(self, blk_row, post_row, bs) -> None:
        """Directly in front of an accept launch: the slot's stop sequences over what that launch is about to commit."""
        if self.sq is not None:
            ops.stop_seq_rows(blk_row, post_row, self.output_ids[0], self.dyn, self.sq, bs=bs)

    def _mark(self, key, which):
        if self.events is not None and self.record_events:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.events.setdefault(key, [None, None])[which] = e

    def _lm8(self):
        """The e4m3 (an mxfp4 draft: the 4-bit) lm_head for the draft's greedy unmask, or None (a bf16 model, or fp8_stream /
        mxfp4_stream switched off)."""
        if isinstance(self.lm_wp8, ops.Mxfp4Weight):
            return self.lm_wp8 if self.model.mxfp4_stream else None
        return self.lm_wp8 if self.model.fp8_stream else None

    def _constrain_draft(self, bs, start: Optional[int] = None) -> None:
        """Right behind a greedy draft head launch, in front of the hook: block[1:bs] re-picked row by row from the head's
        materialised logits, each the best token that is legal in the state reached over the picks before it.  The
        slot's state is read, never written: it moves in the stage's commit alone.
        A coupled draft: the noise form — the perturbed maximum over the legal columns, slot j under the noise of position
        START + j (the draft record's word, as the head launch read it; `start`: the host value, where no record is armed)."""
        if not self.constrain:
            return
        if self.couple:
            ops.grammar_draft_sample_rows(self.draft_logits[:16], self.gr, bias=self._cd_bias, block=self.block[0], nrows=bs,
                                          seeds=self._cseed, temperature=self.temperature, dyn=self.dcache.dyn,
                                          pos_dyn_word=-1 if start is not None else ops.DYN_START,
                                          pos_base=0 if start is None else int(start))
        else:
            ops.grammar_draft_rows(self.draft_logits[:16], self.gr, bias=self._cd_bias, block=self.block[0], nrows=bs)

    def _draft_ahead(self, bs) -> None:
        """The draft forward of the cycle AFTER the one whose accept kernel has just been enqueued (model/dflash.py:237-247
        of the next loop iteration): lengths from the device record, context rows = the verify's tap buffer (valid count
        = the record's tau), block = what the accept kernel re-armed.  Upper bounds for the host-side checks only."""
        m = self.model
        ev = None
        if self.events is not None and self.record_events:   # the caller times the phases: this draft's pairs belong to the NEXT cycle
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        hid = m.draft_block(self.dcache, th_rows=self.taps_buf[:16], tau=16, bs=bs, pos0=self.start + self.max_bs,
                            block_ids=self.block[0], embed=self.embed_w, dyn_ready=True, s_bound=self.start + self.max_bs)
        if ev:
            ev[2].record()
        _draft_ids(m, hid, self.lm_wp, bs, self.block[:, :bs], 0.0, self.draft_logits, dyn=self.dcache.dyn,
                   lm_wp8=self._lm8(), couple=self._couple)
        # (cycle() enqueues this draft behind the stage's commit: the state the pick reads is the one AFTER the advance
        # over what the accept launch has just committed — the state the next verify's rows start from)
        self._constrain_draft(bs)
        if ev:
            ev[3].record()
            ev[1].record()
        self._ahead, self._ahead_ev = bs, ev

    def _call_hook(self, blk) -> None:
        if self.hook is not None:
            self.hook(blk, self.start, self.hook_calls)
        self.hook_calls += 1

    def _take_ahead(self, blk) -> None:
        """This cycle's draft was enqueued behind the previous cycle's accept kernel: only the host's bookkeeping is left."""
        self._ahead = None
        self.dcache.length = self.start           # rows kept (S) + this cycle's context rows (tau) = the new start
        self._dyn_bs = None
        if self.events is not None and self._ahead_ev:   # its event pairs were recorded by the cycle that enqueued it
            e = self._ahead_ev
            self.events["draft"], self.events["lm_head"] = [e[0], e[1]], [e[2], e[3]]
        self._call_hook(blk)

    def _draft(self, blk, bs, draft_steps):
        m = self.model
        ctx = self.target_hidden[0]
        if draft_steps == 1 and self._ahead == bs:
            return self._take_ahead(blk)
        # (a run-ahead draft of another block size is simply abandoned: it touched scratch buffers, the draft tokens of
        # the block and the draft cache rows this forward writes again — the length record is the accept kernel's)
        self._ahead = None
        if draft_steps == 1:
            S = self.dcache.get_seq_length()
            head_rows = max(0, ctx.shape[0] - 16)
            if ctx.shape[0] > 16:  # cycle 0: the prompt's context rows, 16 at a time
                head = ctx.shape[0] - 16
                m.prefill_context(self.dcache, ctx[:head], S)
                ctx, S = ctx[head:], S + head
            # steady state: the accept kernel of the previous cycle wrote S, tau, pos0 and start of THIS forward into
            # the draft cache's record (dfl_accept_commit); only a changed block size or a context head needs new words
            ready = self._dyn_bs == bs and head_rows == 0
            hid = m.draft_block(self.dcache, th_rows=ctx, tau=ctx.shape[0], bs=bs, pos0=S, block_ids=blk[0],
                                embed=self.embed_w, dyn_ready=ready)
            self._dyn_bs = None   # until the accept of this cycle has re-armed the record
            self._mark("lm_head", 0)
            _draft_ids(m, hid, self.lm_wp, bs, blk, self.draft_temperature, self.draft_logits, seed=self._dseed,
                       dyn=self.dcache.dyn, start=self.start, lm_wp8=self._lm8(), couple=self._couple)
            self._constrain_draft(bs)
            self._mark("lm_head", 1)
            return self._call_hook(blk)
        # benchmark.py:112-142: k full passes, each re-embedding the whole block, no draft
        # cache, positions rebuilt as [start-ctx_len, start+bs)
        ctx_len = ctx.shape[0]
        for _ in range(draft_steps):
            tmp = m.new_cache(ctx_len + bs)
            p0 = max(0, self.start - ctx_len)
            c2 = ctx
            if ctx_len > 16:
                m.prefill_context(tmp, ctx[:ctx_len - 16], p0)
                c2, p0 = ctx[ctx_len - 16:], p0 + ctx_len - 16
            hid = m.draft_block(tmp, th_rows=c2, tau=c2.shape[0], bs=bs, pos0=p0, block_ids=blk[0],
                                embed=self.embed_w, append=False)
            _draft_ids(m, hid, self.lm_wp, bs, blk, 0.0, self.draft_logits if self.constrain else None,
                       start=self.start, lm_wp8=self._lm8(), couple=self._couple)   # (no record: the host's start)
            self._constrain_draft(bs, start=self.start)
            self._call_hook(blk)

    @torch.inference_mode()
    def cycle(self, bs: int, *, draft_steps: int = 1, want_hidden: Optional[bool] = None,
              after_draft: Optional[Callable] = None, ahead_ok: bool = False) -> SimpleNamespace:
        """One pass of model/dflash.py:235-268 with block size `bs` (>= 1).  ahead_ok: the caller promises that the next
        cycle uses the same block size whenever the tail allows it (fixed-size loops): its draft may be enqueued early."""
        t_call = time.perf_counter() if self.host_times is not None else 0.0
        start = self.start
        blk = self.block[:, :bs]
        if not self._armed:   # model/dflash.py:235; afterwards dfl_accept_commit (re-arming) leaves the same ids in self.block
            blk.copy_(self.output_ids[:, start:start + bs])
        if bs > 1:
            ahead = draft_steps == 1 and self._ahead == bs
            if not ahead:
                self._mark("draft", 0)
            self._draft(blk, bs, draft_steps)
            if not ahead:
                self._mark("draft", 1)
            if after_draft is not None:
                after_draft(blk)
        if want_hidden is None:
            want_hidden = self.use_draft
        # ---- target verify (outside the path; model/dflash.py:249-255)
        self._mark("target", 0)
        taps = None
        if self.native:
            posterior, taps = self.target.verify(
                blk[0], start, self.tcache, temperature=self.temperature,
                tap_layers=self.model.target_layer_ids if (want_hidden and self.use_draft) else (),
                taps_out=self.taps_buf, seed=self._tseed, **self._vkw)
            self._mark("target", 1)
        else:
            out = self.target(blk, position_ids=self.position_ids[:, start:start + bs],
                              past_key_values=self.tcache, use_cache=True, output_hidden_states=want_hidden)
            self._mark("target", 1)
            if self._tseed is not None:   # verify row j predicts position start + j + 1
                posterior = _draw_rows(out.logits, self.temperature, self._tseed, start + 1, self._filter)
            else:
                posterior = sample(out.logits, self.temperature)
        # ---- accept scan + commit + bookkeeping on the device (:258-268)
        if not (bs > 1 and draft_steps == 1):
            # (after a cached draft forward the record already holds start = pos0 + tau: either draft_block's
            # dfl_set_dyn2 wrote it — which also clears the stop / cycle words — or, on the dyn_ready steady state, the
            # previous cycle's accept kernel did.  STOP is sticky and CYCLE keeps counting across steady-state cycles:
            # a stopped session is terminal, run_decode leaves the loop on it)
            ops.set_dyn(self.dyn, 0, 0, bs, start)  # start word = pos0 + tau = start
        self._arm_result()
        post0 = posterior[0].contiguous()
        self._stop_seq(blk[0], post0, bs)
        ops.accept_commit(blk[0], post0, bs, self.output_ids[0], self.dyn, self.stop_t,
                          self.result, rearm=(self.block[0], self.max_bs, self.mask_token_id),
                          dyn_t=self.tcache.dyn if (self.native and self._fixed is not None) else None)
        if self.stage is not None:
            self.stage.commit(self.output_ids, self.dyn)
        self._armed = True
        # the record now holds the next draft forward's S / tau / pos0 / start — if that cycle was a cached draft cycle
        # on this record (bs > 1, one draft step) and keeps the block size
        self._dyn_bs = bs if (bs > 1 and draft_steps == 1 and self.use_draft) else None
        # run-ahead: the next cycle's draft goes out now if it is likely to be a draft cycle of the same block size —
        # no tail clamp even if every token of this block is accepted, no caller-driven block size (a scheduler picks the
        # next size only after this cycle's result: `ahead_ok`).  A stop token committed by this cycle ends the request:
        # its run-ahead draft is simply abandoned (it wrote scratch buffers and draft cache rows nobody reads again)
        if (ahead_ok and self.run_ahead and self._dyn_bs == bs and self.native and want_hidden
                and getattr(self.model, "attn_impl", "head") == "head"   # (the round-1 stage takes no device-driven lengths)
                and not self.stop_always and self.draft_temperature < 1e-5 and bs <= 16
                and start + 2 * bs <= self.max_length and start + self.max_bs + 16 + bs <= self.dcache.max_rows):
            self._draft_ahead(bs)
        res = self._await_result(t_call)
        rows = None
        if want_hidden and self.use_draft:
            rows = taps if self.native else _taps(out.hidden_states, self.model.target_layer_ids)[0]
        return self._commit(res, bs, start, rows, replayed=False)

    # ------------------------------------------------------------------ the cycle's one device->host hand-over
    def _arm_result(self) -> None:
        # before the accept launch or its replay: the cycle counter (>= 1 once written) is the kernel's LAST store,
        # behind a release
        if self.poll_result:
            self._res_np[3] = -1

    def _await_result(self, t_call: float) -> list:
        """After the cycle's last enqueue: wait for the accept result {acc, new start, stop, cycle} and return it."""
        t_enq = time.perf_counter() if self.host_times is not None else 0.0
        if self.poll_result:   # pinned memory, polled on the word written last
            t0 = time.perf_counter()
            while self._res_np[3] == -1:
                if time.perf_counter() - t0 > 0.05:   # a long verify: stop burning the core, block on the stream
                    torch.cuda.current_stream().synchronize()
                    if self._res_np[3] == -1:
                        raise RuntimeError("dfl_accept_commit: the result never arrived in host memory")
            res = self._res_np.tolist()   # words 0..2 were stored before the counter was released: read them now
        else:
            res = self.result.tolist()  # device->host copy (synchronises the stream)
        if self.host_times is not None:   # host share of the cycle: launches enqueued, then waiting for the GPU
            self.host_times.append((t_enq - t_call, time.perf_counter() - t_enq))
        return res

    def _commit(self, res: list, bs: int, start: int, rows: Optional[torch.Tensor], replayed: bool) -> SimpleNamespace:
        """The host's bookkeeping of an accepted block (model/dflash.py:258-268).  rows: the verify's tapped hidden rows
        [>= tau, :], the next draft's context; None: the caller asked for none."""
        tau = res[0] + 1
        self.start = start + tau
        self.tcache.crop(self.start)
        if rows is not None:
            self.target_hidden = rows[None, :tau]
        self.stopped = bool(self.stop_always or res[2])   # (a replayed session never has stop_always)
        return SimpleNamespace(tau=tau, bs=bs, start=start, stop=self.stopped, replayed=replayed)

    # ------------------------------------------------------------------ hipGraph replay: coverage and capture
    def replay_uncovered(self, sizes, ahead: bool = False) -> Optional[str]:
        """None if this session's cycles can be replayed from hipGraphs at every block size in `sizes`, else the reason
        why not.  ahead: the fixed-size form (capture / cycle_graph), whose draft runs ahead of the accept result."""
        sizes = sorted({int(b) for b in sizes})
        if not self.native:
            return "needs a NativeTarget"
        if not self.use_draft:
            return "needs a draft (block size > 1)"
        if (self.target.attn_impl != "head" or self.target.fuse_oproj
                or getattr(self.model, "attn_impl", "head") != "head"):
            return "needs the plain 'head' attention stage on target and draft (the launches take device-driven lengths)"
        if not self.replay_sampling_ok:
            return "needs T = 0 or sampler='device' (the torch draw consumes host RNG state)"
        if self.stop_always:
            return "needs no mask id among the stop ids"
        if not sizes or sizes[0] < 2 or sizes[-1] > 16:
            return "needs block sizes in 2..16"
        # The one asymmetry: the fixed form's draft is the NEXT cycle's, enqueued before the host has this cycle's result,
        # and a run-ahead draft is only ever greedy or coupled (cycle() launches none at a draft temperature: capture()'s
        # `_ahead == bs` could never hold; a coupled draft reads START from the record the accept launch re-armed).
        # The sized form drafts inside its own cycle, after the host has written the records, so its draft may sample
        # (the draw takes the block start from the record's START word).
        if ahead and self.draft_temperature >= 1e-5:
            return "needs a greedy draft (the next cycle's draft runs ahead of the accept result)"
        if self._replay_bound(sizes[-1]) < self.start:
            return "the caches leave no room for a replayed cycle"
        return None

    def _replay_bound(self, top: int) -> int:
        # upper bound of S / start for replays of up to `top` block rows: it sizes key splits and RoPE tables and must
        # pass the launchers' capacity checks
        return min(self.max_length, self.dcache.max_rows - 16 - top, self.tcache.max_rows - top)

    def _capture_pairs(self, sizes, fixed: bool = False) -> _Replay:
        """Per block size the graphs of [draft forward + lm_head] and [target verify + accept], every length from the
        two device records the accept kernel keeps; `bound` stands in for S / start on the host side.  fixed: the one
        size of capture(), whose accept kernel keeps the target cache's record from here on."""
        m, t, tl = self.model, self.target, self.model.target_layer_ids
        bound = self._replay_bound(max(sizes))
        m._rope_tab(bound + 64 + 64)   # both tables long enough for every replayed cycle before an address is captured
        t._rope_tab(bound + 64 + 64)
        if fixed:   # the target cache's record: block form for the cycle about to run
            ops.set_dyn2(self.tcache.dyn, self.start, 0, sizes[0], self.start)
            self.tcache._dyn_bs = sizes[0]
        torch.cuda.synchronize(self.dev)

        def draft(bs):   # (a sampled draft takes the block start from the draft record's START word)
            hid = m.draft_block(self.dcache, th_rows=self.taps_buf[:16], tau=16, bs=bs, pos0=bound, block_ids=self.block[0],
                                embed=self.embed_w, dyn_ready=True, s_bound=bound)
            _draft_ids(m, hid, self.lm_wp, bs, self.block[:, :bs], self.draft_temperature, self.draft_logits,
                       seed=self._dseed, dyn=self.dcache.dyn, lm_wp8=self._lm8(), couple=self._couple)
            self._constrain_draft(bs)

        def verify_accept(bs):   # (a T > 0 draw takes its positions from the target record's POS0 word: fresh every replay)
            post, _ = t.verify(self.block[0, :bs], bound, self.tcache, temperature=self.temperature, tap_layers=tl,
                               taps_out=self.taps_buf, dyn_lengths=True, seed=self._tseed, **self._vkw)
            post0 = post[0].contiguous()
            self._stop_seq(self.block[0, :bs], post0, bs)
            ops.accept_commit(self.block[0, :bs], post0, bs, self.output_ids[0], self.dyn, self.stop_t,
                              self.result, rearm=(self.block[0], self.max_bs, self.mask_token_id), dyn_t=self.tcache.dyn)
            if self.stage is not None:
                self.stage.commit(self.output_ids, self.dyn)

        graphs = {bs: (capture_graph(lambda: draft(bs)), capture_graph(lambda: verify_accept(bs))) for bs in sizes}
        # The graphs hold RAW device pointers: keep alive every tensor whose address they hold and that this session does
        # not own through another attribute — the RoPE tables, the shared workspaces of draft model and target
        return _Replay(graphs, bound, (m._rope[0].data_ptr(), t._rope[0].data_ptr()),
                       (m._rope, t._rope, getattr(m, "ws", None), getattr(t, "ws", None), getattr(t, "_taps", None),
                        self.lm_wp, self.lm_wp8, self.embed_w, getattr(t, "lm_wp", None),
                        t.fp8_tensors() if self.native else (),    # (an fp8 target's codes and scale vectors)
                        self.stage,    # (the row processors' state and every buffer their launches read or write)
                        self.sq))      # (the stop sequences' tables and hit record)

    def _tables_moved(self, rec: _Replay) -> bool:
        """A shared draft model / NativeTarget replaces its RoPE table when another caller needs more positions
        (`_rope_tab`), and sessions may interleave on one target.  The record keeps the captured tensors alive, so a
        replay stays memory-safe; a differing pointer only says the owner has moved on to a larger table (same first
        rows): the caller drops the graphs, runs this cycle eagerly and captures again, not to pin the old table for ever."""
        m, t = self.model, self.target
        return m._rope is None or t._rope is None or (m._rope[0].data_ptr(), t._rope[0].data_ptr()) != rec.rope

    # ------------------------------------------------------------------ replay of the steady-state cycle, fixed block size
    @property
    def _graph_bs(self) -> Optional[int]:   # the block size capture() holds graphs for (its record's one key), or None
        return next(iter(self._fixed.graphs)) if self._fixed is not None else None

    def _graph_ok(self, bs: int) -> bool:
        """A cycle that can be replayed: the captured block size, no tail clamp even if every token of this block and the
        next is accepted, and the previous cycle left this cycle's draft enqueued (run-ahead)."""
        r = self._fixed
        if not (r is not None and bs in r.graphs and self._ahead == bs
                and (self.events is None or not self.record_events)   # (a dict that only takes a run-ahead draft's pairs is fine)
                and self.start + 2 * bs <= self.max_length and self.start + bs <= r.bound):
            return False
        if self._tables_moved(r):
            self._fixed = None
            return False
        return True

    @torch.inference_mode()
    def capture(self, bs: int) -> None:
        """Capture the steady-state cycle of block size bs (2..16) into two hipGraphs: [target verify + accept] and
        [draft forward + lm_head of the NEXT cycle].  Every length the launches need is in the device records the
        accept kernel keeps (dfl_accept_commit with dyn_t: the draft cache's record and the target cache's block-form
        record), so one capture serves every cycle; the attention launches size their key splits for the caches'
        capacity.  Call after at least one cycle(bs, ahead_ok=True).  The host then spends two graph launches and one poll
        per cycle instead of ~215 ctypes calls.  Raises GraphNotCovered for a session or a state
        the graphs do not cover (replay_uncovered)."""
        why = self.replay_uncovered((bs,), ahead=True)
        if why is None and self._ahead != bs:
            why = "run one cycle(bs, ahead_ok=True) first (the next draft must be in flight)"
        if why is not None:
            raise GraphNotCovered(f"capture: {why}")
        self._fixed = self._capture_pairs((bs,), fixed=True)

    @torch.inference_mode()
    def cycle_graph(self, bs: int) -> SimpleNamespace:
        """One pass of model/dflash.py:235-268 by graph replay; falls back to cycle(bs, ahead_ok=True) where the cycle
        cannot be replayed (tail of the request, events being recorded)."""
        if not self._graph_ok(bs):
            return self.cycle(bs, ahead_ok=True)
        t_call = time.perf_counter() if self.host_times is not None else 0.0
        start = self.start
        self._take_ahead(self.block[:, :bs])   # the draft of THIS cycle is in flight already (run-ahead)
        draft_next, verify = self._fixed.graphs[bs]
        self._arm_result()
        verify.replay()
        self._armed = True
        self._dyn_bs = bs
        draft_next.replay()          # the NEXT cycle's draft, behind the accept kernel
        self._ahead, self._ahead_ev = bs, None
        return self._commit(self._await_result(t_call), bs, start, self.taps_buf, replayed=True)

    # ------------------------------------------------------------------ hipGraph replay with a caller-chosen block size
    @torch.inference_mode()
    def capture_sizes(self, sizes) -> None:
        """One pair of hipGraphs per block size in `sizes` (2..16 each) for loops whose caller picks the size every cycle —
        the policy loop of benchmark_dynamic_schedule.py:319-379: [draft forward + lm_head] and [target verify + accept],
        every launch taking its lengths from the two device records.  cycle_sized() writes those records from the host's
        own bookkeeping (two 64-thread launches) and replays the pair; there is no run-ahead draft, since the next block's
        size is only known once the scheduler has seen this cycle's result.  Call after at least one draft cycle.  Raises
        GraphNotCovered for a session or a state the graphs do not cover (replay_uncovered)."""
        sizes = sorted({int(b) for b in sizes})
        why = self.replay_uncovered(sizes)
        if why is None and not self._armed:
            why = "run one cycle first"
        if why is not None:
            raise GraphNotCovered(f"capture_sizes: {why}")
        self._sized = self._capture_pairs(sizes)
        self.tcache.crop(self.start)     # (verify's host-side bookkeeping ran with the bound)

    def _sized_ok(self, bs: int) -> bool:
        r = self._sized
        if not (r is not None and bs in r.graphs and self._armed
                and (self.events is None or not self.record_events) and self.target_hidden is not None
                and self.target_hidden.shape[1] <= 16 and self.start + bs <= min(self.max_length, r.bound)):
            return False
        if self._tables_moved(r):
            self._sized = None
            return False
        return True

    @torch.inference_mode()
    def cycle_sized(self, bs: int, *, after_draft: Optional[Callable] = None) -> SimpleNamespace:
        """One pass of model/dflash.py:235-268 with the caller's block size by graph replay (capture_sizes); falls back
        to cycle(bs) where the cycle cannot be replayed (a size that was not captured — the clamped tail —, events being
        recorded, cycle 0's prompt-length context)."""
        if not self._sized_ok(bs):
            return self.cycle(bs, after_draft=after_draft)
        t_call = time.perf_counter() if self.host_times is not None else 0.0
        start = self.start
        tau_c = int(self.target_hidden.shape[1])
        S = self.dcache.get_seq_length()
        # the two length records, exactly as the eager launches would write them (model.draft_block, NativeTarget.verify)
        ops.set_dyn2(self.dcache.dyn, S, tau_c, bs, S)
        ops.set_dyn2(self.tcache.dyn, start, 0, bs, start)
        self.tcache._dyn_bs = bs
        self._ahead = None
        dg, vg = self._sized.graphs[bs]
        dg.replay()
        self.dcache.length = S + tau_c
        blk = self.block[:, :bs]
        self._call_hook(blk)
        if after_draft is not None:
            after_draft(blk)
        self._arm_result()
        vg.replay()
        self._armed = True
        self._dyn_bs = bs
        res = self._await_result(t_call)
        self.tcache.length = start + bs   # (the replayed verify wrote bs rows; the host's counter follows before the crop)
        return self._commit(res, bs, start, self.taps_buf, replayed=True)

    def finish(self) -> torch.Tensor:
        """The returned ids; with stop sequences the hit record is read here, once, and `stop_sequence` set: the index of
        the sequence that ended the request, None where it ended otherwise."""
        self._hit = _stop_hit(self.sq, 0, self.stop_seqs, self.include_stop)
        if self._hit is None:
            return _trim(self.output_ids, self.max_length, self.mask_token_id, self.stop_token_ids, self.n_in)
        which = []
        cols = _kept_cols(self.output_ids, self.max_length, self.mask_token_id, self.stop_token_ids, self.n_in, self._hit,
                          which)
        self.stop_sequence = which[0] if which else None
        return self.output_ids[:, cols]

    def finish_logprobs(self) -> dict:
        """The result fields logprobs / top_logprob_ids / top_logprobs, trimmed exactly as finish() trims the ids (all
        None with logprobs off)."""
        if self.lp is None:
            return dict(NO_LOGPROBS)
        cols = _kept_cols(self.output_ids, self.max_length, self.mask_token_id, self.stop_token_ids, self.n_in, self._hit)
        return logprob_fields(self.lp, 0, cols[self.n_in:])

    def finish_grammar(self, output_ids: torch.Tensor) -> Optional[int]:
        """The result field grammar_state: the automaton's state after the generated tokens finish() returned, walked by
        dfl_grammar_advance from start; -1 where one of them is illegal or the slot's own state was violated; None with
        the grammar off.  (The slot's own state runs on over what an accept launch committed behind a stop id, behind a
        matched stop sequence or past max_length — tokens the trim drops, which dfl_penalty_count and dfl_grammar_advance
        still count — so it is not the state after what is returned.)"""
        if self.gr is None:
            return None
        if int(self.gr.state.item()) < 0:
            return -1
        g = SimpleNamespace(table=self.gr.table, base=self.gr.base,
                            state=torch.full((1,), self._gr_start, dtype=torch.int32, device=self.dev))
        ops.grammar_advance(g, output_ids[0].contiguous(), lo=self.n_in, hi=output_ids.shape[1])
        return int(g.state.item())


@torch.inference_mode()
def run_decode(model, target, input_ids: torch.Tensor, *, mask_token_id: int, max_new_tokens: int,
               block_size: int, stop_token_ids, temperature: float, clamp_tail: bool,
               draft_steps: int = 1, collect_profile: bool = False, scheduler=None,
               draft_temperature: Optional[float] = None, draft_token_hook: Optional[Callable] = None,
               max_block_size: Optional[int] = None, sampler: str = "torch", seed: Optional[int] = None,
               top_k: int = 0, top_p: float = 1.0, logprobs: Optional[int] = None, repetition_penalty: float = 1.0,
               presence_penalty: float = 0.0, frequency_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None,
               banned_token_ids=None, min_tokens: int = 0, grammar=None,
               constrain_draft: bool = False, min_p=None, couple_draft: bool = False, stop_sequences=None,
               include_stop_sequence: bool = True) -> SimpleNamespace:
    s = DecodeSession(model, target, input_ids, mask_token_id=mask_token_id, max_new_tokens=max_new_tokens,
                      max_block_size=max_block_size or block_size, stop_token_ids=stop_token_ids,
                      temperature=temperature, draft_temperature=draft_temperature,
                      draft_token_hook=draft_token_hook, sampler=sampler, seed=seed, top_k=top_k, top_p=top_p,
                      logprobs=logprobs, repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                      frequency_penalty=frequency_penalty, logit_bias=logit_bias, allowed_token_ids=allowed_token_ids,
                      banned_token_ids=banned_token_ids, min_tokens=min_tokens, grammar=grammar,
                      constrain_draft=constrain_draft, min_p=min_p, couple_draft=couple_draft,
                      stop_sequences=stop_sequences, include_stop_sequence=include_stop_sequence)
    t_prefill = cuda_time()
    s.prefill()
    time_to_first_token = cuda_time() - t_prefill

    decode_start = cuda_time()
    taus, used_bs, cycle_trace, lgens = [], [], [], []
    draft_prefill = True
    # Steady-state cycles are replayed from hipGraphs where the graphs cover the session (replay_uncovered: asked here
    # and again by the capture, for the state it finds); DFL_GRAPH=0: eager launches.  GraphNotCovered from a capture
    # means eager cycles for the rest of the request; any other error is a real failure and leaves this call
    sizes = (block_size,) if scheduler is None else tuple(getattr(scheduler, "candidates", ()))
    replay = os.environ.get("DFL_GRAPH", "1") != "0" and s.replay_uncovered(sizes, ahead=scheduler is None) is None
    cyc = replayed = 0
    replayed_flags = []
    while s.start < s.max_length and not s.stopped:   # (stopped before a cycle: the first token ended a stop sequence)
        cycle_t0 = cuda_time() if scheduler is not None else None
        if collect_profile:
            s.events = {}
            s._mark("cycle", 0)
        chosen = block_size if scheduler is None else scheduler.select(cyc)
        remaining = s.max_length - s.start
        bs = max(1, min(chosen, remaining)) if (clamp_tail or scheduler is not None) else chosen
        lg = [float(bs)]

        def after_draft(blk, lg=lg, bs=bs):
            nonlocal draft_prefill, decode_start
            # EOS-aware generated length of the policy loop (benchmark_dynamic_schedule.py:344-349)
            if scheduler is not None and s.stop_t is not None:
                pos = torch.isin(blk[0, 1:], s.stop_t).nonzero(as_tuple=True)[0]
                if pos.numel() > 0:
                    lg[0] = float(min(int(pos[0].item()) + 1, bs))
            if draft_prefill:
                # the TPOT clock restarts right after the FIRST draft call and before that cycle's target
                # forward (benchmark.py:145-147, benchmark_dynamic_schedule.py:352-354): it drops the
                # prompt-context projection, not cycle 0's verify
                draft_prefill = False
                decode_start = cuda_time()

        # hidden states: always in spec_generate / the policy loop, only for bs > 1 in the
        # harness form (benchmark.py:157)
        want_hidden = s.use_draft if (scheduler is not None or not clamp_tail) else bs > 1
        gen_before = s.start - s.n_in
        start_idx = s.start
        # fixed-size loops replay their steady-state cycles from two hipGraphs (DecodeSession.capture): the host's share
        # of a cycle drops from ~2.3 ms to ~0.2 ms at the same GPU time.  Stop ids ride along in
        # the captured accept launch; T > 0 needs the device sampler
        per_cycle = replay and draft_steps == 1 and not collect_profile and want_hidden and not draft_prefill
        if per_cycle and scheduler is None and bs == block_size and s._ahead == bs:
            if s._graph_bs is None:
                try:
                    s.capture(bs)
                except GraphNotCovered:
                    replay = False
            r = s.cycle_graph(bs)
        elif per_cycle and scheduler is not None:
            # the policy loop by replay: one pair of graphs per candidate size (DecodeSession.capture_sizes, which needs
            # a cycle to have run: `not draft_prefill` says one has, and every cycle leaves the session armed)
            if s._sized is None:
                try:
                    s.capture_sizes(sizes)
                except GraphNotCovered:
                    replay = False
            r = s.cycle_sized(bs, after_draft=after_draft)
        else:
            # (collect_profile: no run-ahead draft — its event pairs would be recorded during cycle N and handed to
            # cycle N + 1, outside that cycle's [cycle0, cycle1] marks; benchmark.py:149-160 times each phase inside its
            # own cycle)
            r = s.cycle(bs, draft_steps=draft_steps, want_hidden=want_hidden, after_draft=after_draft,
                        ahead_ok=scheduler is None and draft_steps == 1 and not collect_profile)
        taus.append(r.tau)
        used_bs.append(bs)
        lgens.append(lg[0])
        replayed += int(r.replayed)
        replayed_flags.append(r.replayed)
        if scheduler is not None:
            cycle_s = cuda_time() - cycle_t0
            scheduler.update(tau=r.tau, cycle_s=cycle_s, effective_bs=bs, cycle_idx=cyc, l_gen=lg[0])
            cycle_trace.append({
                "cycle_idx": cyc, "start_idx": int(start_idx), "block_size": int(bs),
                "chosen_block_size": int(chosen), "tau": int(r.tau), "l_gen": float(lg[0]),
                "acceptance_ratio": float(r.tau / max(1, bs)), "cycle_s": float(cycle_s),
                "tau_hat": scheduler.tau_hat.get(bs), "cycle_hat": scheduler.cycle_hat.get(bs),
                "score_hat": scheduler.score_hat.get(bs), "current_block_size": int(scheduler.current),
                "adl_lgen_hat": scheduler.adl_lgen_hat, "adl_lacc_hat": scheduler.adl_lacc_hat,
                "adl_target_k": int(scheduler.adl_target_k), "adl_target_bs": int(scheduler.adl_target_bs)})
        elif collect_profile:
            s._mark("cycle", 1)
            cycle_trace.append({"cycle_idx": cyc, "generated_tokens_before": int(gen_before),
                                "effective_block_size": int(bs), "tau": int(r.tau),
                                "acceptance_ratio": float(r.tau / max(1, bs)), "_events": s.events})
        s.events = None
        cyc += 1
        if r.stop:
            break

    output_ids = s.finish()
    for m in (model, target):   # opt-in fused launches leave a flag instead of hanging when their wait runs out
        if getattr(m, "fuse_oproj", False):
            m.raise_if_failed()
    num_output_tokens = output_ids.shape[1] - s.n_in
    total_decode_time = cuda_time() - decode_start
    profile_summary = None
    if collect_profile and scheduler is None:
        profile_summary = _resolve_profile(cycle_trace, time_to_first_token, total_decode_time)
    return SimpleNamespace(output_ids=output_ids, num_input_tokens=s.n_in, num_output_tokens=num_output_tokens,
                           time_to_first_token=time_to_first_token,
                           time_per_output_token=total_decode_time / max(1, num_output_tokens),
                           acceptance_lengths=taus, used_block_sizes=used_bs, l_gen=lgens,
                           cycle_trace=cycle_trace, profile_summary=profile_summary, replayed_cycles=replayed,
                           replayed_flags=replayed_flags,
                           seed=s.seed, grammar_state=s.finish_grammar(output_ids), stop_sequence=s.stop_sequence,
                           **s.finish_logprobs())


def _draft_ids(model, hid_frag, lm_wp, bs, blk, draft_temperature, keep_logits=None, seed=None, dyn=None, start=None,
               lm_wp8=None, couple=None):
    """blk[0, 1:bs] <- draft tokens.  Greedy (every loop but the policy one at T>0):
    fused lm_head GEMM + argmax.  benchmark_dynamic_schedule.py:342 samples the draft
    with the temperature: then the logits are materialised by the same GEMM and the
    reference's softmax + multinomial is applied to them.  keep_logits (bf16 [16 * tiles, V]): the caller's
    buffer for the materialised logits (the multi-candidate loop builds its candidates from them).
    seed (sampler="device"): the seeded draw of the same GEMM's epilogue instead (stream DRAFT: slot j of the block that
    starts at `start` draws position start + j, extra = start); dyn: the draft cache's record, whose START word holds
    that start on the device (what a captured graph reads).
    lm_wp8 (an fp8 draft model): the e4m3 lm_head, taken by the greedy unmask — of a block of <= 16 rows, or of a
    17..32-row block that went through the tile stack; a sampled draft keeps the bf16 copy.
    couple (dict(seed, temperature): the request's seed and the TARGET's temperature): the coupled
    draw — the same epilogue on stream TARGET, slot j under the noise verify row j - 1 will draw position start + j with;
    the bf16 head, as every sampled draft."""
    if couple is not None:
        model.draft_tokens(hid_frag, lm_wp, bs, blk[0], logits=keep_logits,
                           sample=dict(seed=couple["seed"], temperature=couple["temperature"], dyn=dyn, start=start,
                                       stream=ops.RNG_TARGET))
        return
    if draft_temperature < 1e-5:
        from .model import WideRows
        wide = isinstance(hid_frag, WideRows)   # (both tiles in one ragged-batch lm_head pass)
        # (an mxfp4 draft's 4-bit head: the single 16-row tile only — streams_fp8_tiles() is False for it)
        wp = lm_wp8 if lm_wp8 is not None and (model.streams_fp8_tiles() if wide else bs <= 16) else lm_wp
        model.draft_tokens(hid_frag, wp, bs, blk[0], logits=keep_logits)
        return
    if seed is not None:
        model.draft_tokens(hid_frag, lm_wp, bs, blk[0], logits=keep_logits,
                           sample=dict(seed=seed, temperature=draft_temperature, dyn=dyn, start=start))
        return
    V = model.config.vocab_size
    logits = keep_logits
    if logits is None:
        logits = torch.empty(16 * ((bs + 15) // 16), V, dtype=torch.bfloat16, device=model.device)
    model.draft_tokens(hid_frag, lm_wp, bs, blk[0], logits=logits)
    blk[:, 1:bs] = sample(logits[1:bs].unsqueeze(0), draft_temperature)


def _resolve_profile(cycle_trace, ttft, decode_wall):
    """benchmark.py:208-240: turn the recorded event pairs into seconds."""
    torch.cuda.synchronize()
    tot = {"draft": 0.0, "target": 0.0, "cycle": 0.0}
    for row in cycle_trace:
        ev = row.pop("_events")
        for k in tot:
            pair = ev.get(k)
            s = pair[0].elapsed_time(pair[1]) / 1000.0 if pair and pair[0] is not None and pair[1] is not None else 0.0
            row[f"{k}_s"] = float(s)
            tot[k] += s
    den = max(1e-12, tot["draft"] + tot["target"])
    return {"target_prefill_s": float(ttft), "target_decode_s": float(tot["target"]),
            "draft_decode_s": float(tot["draft"]), "cycle_decode_s_sum": float(tot["cycle"]),
            "decode_wall_s": float(decode_wall), "profiled_cycles": int(len(cycle_trace)),
            "draft_share_decode": float(tot["draft"] / den), "target_share_decode": float(tot["target"] / den)}


def dflash_generate(model, target, input_ids: torch.Tensor, mask_token_id: int, max_new_tokens: int,
                    block_size: int, stop_token_ids, temperature: float = 0.0, collect_profile: bool = False,
                    draft_steps: int = 1, draft_token_hook=None, sampler: str = "torch",
                    seed: Optional[int] = None, top_k: int = 0, top_p: float = 1.0,
                    logprobs: Optional[int] = None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                    frequency_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
                    min_tokens: int = 0, grammar=None, constrain_draft: bool = False, min_p=None,
                    couple_draft: bool = False, stop_sequences=None, include_stop_sequence: bool = True) -> SimpleNamespace:
    """benchmark.py:44-55 signature; returns the namespace of :242-251 (+ replayed_cycles).
    stop_sequences (None: off, the launches of before; up to 8 sequences of 1..16 token ids, a bare int counting as a
    sequence of one): the request ends with the first committed token that completes one of them — matched on the device
    in front of every accept launch, over committed tokens only, across cycle boundaries, never inside the prompt and
    not before min_tokens tokens are out.  include_stop_sequence (True, as stop ids stay in the
    output; False: the matched ids are cut off too, the OpenAI behaviour).  The result's `stop_sequence` is the index of
    the sequence that ended the request, None where it ended otherwise.  Any target, native or wrapped.
    couple_draft (False: off, the launches of before; at T > 0 needs sampler="device", else ValueError; at T = 0 it does
    nothing): every draft token is picked under the noise the target's verify will draw that position with — Gumbel-max
    coupling, DESIGN.md section 20.  The emitted ids do not change (the target's draw decides every token as before),
    only the acceptance lengths.  The draft's head reads the bf16 lm_head for this launch, also in an fp8 / mxfp4 draft.
    With constrain_draft the pick under the automaton is the perturbed maximum over the legal tokens.
    min_p (None / 0: off; a float in (0, 1]; needs a NativeTarget and sampler="device" at T > 0, does nothing at T = 0):
    the target's draw keeps token v only if p_v >= min_p * p_max on its tempered, processed distribution — one launch
    directly in front of every target draw, behind the logit bias, the grammar and the penalties; top_p takes its mass
    over what min_p kept; blocks of up to 32 rows.  The draft's proposals stay unfiltered.
    grammar (a dflash_amd.TokenDFA or ByteGrammar; None: off; needs a NativeTarget, blocks of <= 16 rows, and sampler="device" at
    T > 0): the emitted tokens walk the automaton from its start state — every verify row is masked by the state its
    own prefix of the block reaches, between the logit bias and the penalties.  The result's
    `grammar_state` is the state after the returned tokens (-1: violated; None when off).  The draft's proposals stay
    unconstrained unless constrain_draft is set.
    constrain_draft (False: off, the launches of before; needs a grammar or a ban — allowed_token_ids, banned_token_ids,
    a logit_bias of -inf —, else ValueError; a greedy draft): each draft token is the draft's best choice among the
    tokens the request could emit at that point of the block — one launch behind the draft's head picks row by row
    under the automaton and the bans ("The draft under the grammar").  The emitted ids do not
    change, only the acceptance lengths.
    logit_bias ({id: bias}, finite or -inf) / allowed_token_ids / banned_token_ids / min_tokens (None / None / None / 0:
    off; need a NativeTarget, blocks of <= 16 rows, and sampler="device" at T > 0): the OpenAI / vLLM controls on the
    target's logits, applied before the penalties; no stop id is emitted before min_tokens tokens are out (DESIGN.md
    section 14).  The draft's proposals stay unprocessed.
    repetition_penalty r / presence_penalty a / frequency_penalty f (1.0 / 0.0 / 0.0: off; need a NativeTarget, blocks of
    <= 16 rows, and sampler="device" at T > 0): the vLLM / OpenAI penalties on the target's logits, history = the prompt
    and everything emitted so far, the draft tokens in front of a verify row included.  The draft's
    proposals stay unpenalised.
    logprobs (None: off; needs a NativeTarget): 0 adds the field `logprobs` fp32 [num_output_tokens], the
    log-probability of every generated token under the target's RAW distribution (log_softmax of its logits at T = 1,
    unfiltered, whatever temperature and filter drew the token); 1..8 add `top_logprob_ids` / `top_logprobs`
    [num_output_tokens, N], the N most likely tokens at each position.  Off: the fields are None.
    sampler="device": T > 0 draws are seeded on the device — the same seed gives the same tokens
    however the request runs, and the cycles can be replayed from hipGraphs; seed=None draws one from torch's RNG.
    top_k / top_p (0 / 1.0: off) restrict the target's seeded draw (section 8, "Filtered draw"); sampler="device" only."""
    if getattr(model, "wide_hidden", False):
        if grammar is not None:
            raise NotImplementedError("grammar: hidden_size > 4096 runs through the ragged batch, which takes no grammar")
        return _generate_wide_hidden(model, target, input_ids, mask_token_id, max_new_tokens, block_size, stop_token_ids,
                                     temperature, collect_profile, draft_steps, draft_token_hook, sampler, seed, top_k, top_p,
                                     logprobs, (repetition_penalty, presence_penalty, frequency_penalty),
                                     dict(logit_bias=logit_bias, allowed_token_ids=allowed_token_ids,
                                          banned_token_ids=banned_token_ids, min_tokens=min_tokens),
                                     constrain_draft=constrain_draft, min_p=min_p, couple_draft=couple_draft,
                                     stop_sequences=stop_sequences, include_stop_sequence=include_stop_sequence)
    r = run_decode(model, target, input_ids, mask_token_id=mask_token_id, max_new_tokens=max_new_tokens,
                   block_size=block_size, stop_token_ids=stop_token_ids, temperature=temperature, clamp_tail=True,
                   stop_sequences=stop_sequences, include_stop_sequence=include_stop_sequence, draft_steps=draft_steps, collect_profile=collect_profile, draft_token_hook=draft_token_hook,
                   sampler=sampler, seed=seed, top_k=top_k, top_p=top_p, logprobs=logprobs,
                   repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                   frequency_penalty=frequency_penalty, logit_bias=logit_bias, allowed_token_ids=allowed_token_ids,
                   banned_token_ids=banned_token_ids, min_tokens=min_tokens, grammar=grammar,
                   constrain_draft=constrain_draft, min_p=min_p, couple_draft=couple_draft)
    return SimpleNamespace(output_ids=r.output_ids, num_input_tokens=r.num_input_tokens,
                           num_output_tokens=r.num_output_tokens, time_to_first_token=r.time_to_first_token,
                           time_per_output_token=r.time_per_output_token, acceptance_lengths=r.acceptance_lengths,
                           cycle_trace=r.cycle_trace, profile_summary=r.profile_summary,
                           replayed_cycles=r.replayed_cycles, logprobs=r.logprobs, top_logprob_ids=r.top_logprob_ids,
                           top_logprobs=r.top_logprobs, grammar_state=r.grammar_state, stop_sequence=r.stop_sequence)


def _generate_wide_hidden(model, target, input_ids, mask_token_id, max_new_tokens, block_size, stop_token_ids, temperature,
                          collect_profile=False, draft_steps=1, draft_token_hook=None, sampler="torch",
                          seed=None, top_k=0, top_p=1.0, logprobs=None, penalties=(1.0, 0.0, 0.0),
                          bias=None, constrain_draft=False, min_p=None, couple_draft=False, stop_sequences=None,
                          include_stop_sequence=True) -> SimpleNamespace:
    """hidden_size > 4096: the request runs as a group of ONE through the ragged-batch kernels (their GEMMs cut K over
    workgroups; the single-request kernels keep a whole K = hidden row slice per workgroup).  Same loop semantics
    (benchmark.py:44-251, tail clamp included); no per-cycle profile, one draft step per cycle."""
    from .batch import dflash_generate_batch
    from .target import NativeTarget
    if not isinstance(target, NativeTarget):
        raise NotImplementedError("hidden_size > 4096: wrap the target in dflash_amd.NativeTarget (the draft forward and the "
                                  "verify share the ragged-batch launches)")
    if collect_profile or draft_steps != 1:
        raise NotImplementedError("hidden_size > 4096: no per-cycle profile and one draft step per cycle")
    hook = (lambda r, blk, start, call: draft_token_hook(blk, start, call)) if draft_token_hook else None
    return dflash_generate_batch(model, target, [input_ids], mask_token_id, max_new_tokens, block_size, stop_token_ids,
                                 temperature, draft_token_hook=hook, group_size=1, hook_block_view=True, sampler=sampler,
                                 seed=None if seed is None else [seed], top_k=top_k, top_p=top_p, logprobs=logprobs,
                                 repetition_penalty=penalties[0], presence_penalty=penalties[1],
                                 frequency_penalty=penalties[2], **_one_prompt_bias(bias),
                                 constrain_draft=constrain_draft, min_p=min_p, couple_draft=couple_draft,
                                 stop_sequences=stop_sequences, include_stop_sequence=include_stop_sequence)[0]


def _one_prompt_bias(bias) -> dict:
    """A single request's logit-bias keywords in the per-prompt form dflash_generate_batch takes (lists are values
    there: one per prompt)."""
    if not bias:
        return {}
    return dict(logit_bias=[bias["logit_bias"]], allowed_token_ids=[bias["allowed_token_ids"]],
                banned_token_ids=[bias["banned_token_ids"]], min_tokens=bias["min_tokens"])


def dflash_generate_policy(*, model, target, input_ids: torch.Tensor, mask_token_id: int, max_new_tokens: int,
                           stop_token_ids, temperature: float, fixed_block_size: Optional[int] = None,
                           scheduler=None, draft_token_hook=None, sampler: str = "torch",
                           seed: Optional[int] = None, top_k: int = 0, top_p: float = 1.0,
                           logprobs: Optional[int] = None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                           frequency_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
                           min_tokens: int = 0, grammar=None, constrain_draft: bool = False,
                           min_p=None, couple_draft: bool = False, stop_sequences=None,
                           include_stop_sequence: bool = True) -> SimpleNamespace:
    """benchmark_dynamic_schedule.py:260-272 signature; returns the namespace of :425-434 (+ replayed_cycles).
    stop_sequences / include_stop_sequence: as dflash_generate (the field `stop_sequence`).
    couple_draft: as dflash_generate; here it REPLACES this loop's own draw on the DRAFT stream (whose acceptance,
    sum p_i q_i, is the lowest of the three drafts), and constrain_draft then works at T > 0.
    min_p: as dflash_generate (the target's draw; the draft's own draw stays unfiltered).
    grammar: as dflash_generate (the target's rows; the draft's own draw stays unconstrained; `grammar_state`).
    constrain_draft: as dflash_generate; this loop drafts at the request's temperature, so it needs temperature = 0
    (NotImplementedError for a sampled draft).
    logprobs: as dflash_generate (the fields logprobs / top_logprob_ids / top_logprobs; None when off).
    sampler / seed: as dflash_generate; the draft's own T > 0 draw uses the same seed on a stream of its own.
    top_k / top_p: as dflash_generate (the target's draw; the draft's own draw stays unfiltered).
    repetition_penalty / presence_penalty / frequency_penalty: as dflash_generate (the target's rows; the draft's own
    draw stays unpenalised).  logit_bias / allowed_token_ids / banned_token_ids / min_tokens: likewise."""
    if fixed_block_size is None and scheduler is None:
        raise ValueError("Either fixed_block_size or scheduler must be provided.")
    max_bs = fixed_block_size if fixed_block_size is not None else max(scheduler.candidates)
    sched = scheduler if fixed_block_size is None else _Fixed(fixed_block_size)
    r = run_decode(model, target, input_ids, mask_token_id=mask_token_id, max_new_tokens=max_new_tokens,
                   block_size=max_bs, stop_token_ids=stop_token_ids, temperature=temperature, clamp_tail=True,
                   scheduler=sched, draft_temperature=temperature, max_block_size=max_bs,
                   stop_sequences=stop_sequences, include_stop_sequence=include_stop_sequence,
                   draft_token_hook=draft_token_hook, sampler=sampler, seed=seed, top_k=top_k, top_p=top_p,
                   logprobs=logprobs, repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                   frequency_penalty=frequency_penalty, logit_bias=logit_bias, allowed_token_ids=allowed_token_ids,
                   banned_token_ids=banned_token_ids, min_tokens=min_tokens, grammar=grammar,
                   constrain_draft=constrain_draft, min_p=min_p, couple_draft=couple_draft)
    if fixed_block_size is not None:
        for row in r.cycle_trace:
            for k in ("tau_hat", "cycle_hat", "score_hat", "current_block_size", "adl_lgen_hat", "adl_lacc_hat",
                      "adl_target_k", "adl_target_bs"):
                row[k] = None
    return SimpleNamespace(output_ids=r.output_ids, num_input_tokens=r.num_input_tokens,
                           num_output_tokens=r.num_output_tokens, time_to_first_token=r.time_to_first_token,
                           time_per_output_token=r.time_per_output_token, acceptance_lengths=r.acceptance_lengths,
                           used_block_sizes=r.used_block_sizes, cycle_trace=r.cycle_trace,
                           replayed_cycles=r.replayed_cycles, logprobs=r.logprobs, top_logprob_ids=r.top_logprob_ids,
                           top_logprobs=r.top_logprobs, grammar_state=r.grammar_state, stop_sequence=r.stop_sequence)


class _Fixed:
    """fixed_block_size path of dflash_generate_policy: a scheduler that never moves."""
    candidates = ()
    tau_hat = cycle_hat = score_hat = {}
    adl_lgen_hat = adl_lacc_hat = None

    def __init__(self, bs):
        self.bs = bs
        self.candidates = (bs,)
        self.current = self.adl_target_k = self.adl_target_bs = bs

    def select(self, cyc):
        return self.bs

    def update(self, **_):
        pass
