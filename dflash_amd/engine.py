"""A ragged batch that stays full: `BatchEngine` owns ONE `BatchedDecoder` (one set of caches, workspaces and
hipGraphs) for its whole life and re-admits the next queued prompt into a slot as soon as its request ends, instead of
running static groups until their slowest request is done (`dflash_generate_batch`).  DESIGN.md section 9.

Contract, the one `dflash_generate_batch` states: request i emits exactly what `dflash_generate(model, target,
prompt_i, ..., max_new_tokens_i, ...)` emits — ids, acceptance lengths, token count — whichever slot it lands in,
whenever it is admitted and whatever ran in that slot before; with sampler="device" at T > 0 under the terms of
DESIGN.md section 8.  The scheduling decisions live in `dflash_amd.slots.SlotLoop` (pure Python)."""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Callable, Optional, Sequence, Union

import torch

from . import ops
from .batch import (MAX_GROUP, BatchedDecoder, _load_grammars, _pool_rows, _prompt_bias, _prompt_filters,
                    _prompt_grammars, _prompt_min_p, _prompt_penalties, _prompt_seeds, _prompt_stop_sequences,
                    _prompt_temperatures)
from .generate import NO_LOGPROBS, _kept_cols, _trim, cuda_time, logprob_fields
from .logits_stage import check_features
from .slots import SlotLoop

BLOCK_ROWS = 16   # rows of a slot's tile: the margins below are the ones dflash_generate_batch sizes its decoder with


def check_fit(P: int, max_new_tokens: int, max_rows: int, out_len: int) -> None:
    """ValueError unless a prompt of P ids with max_new_tokens fits a decoder of max_rows cache rows and out_len ids
    (no torch, no GPU: `submit` calls it before anything is launched)."""
    if P < 1 or max_new_tokens < 0:
        raise ValueError("a request has a prompt of at least one id and max_new_tokens >= 0")
    if P + max_new_tokens + 3 * BLOCK_ROWS > max_rows:
        raise ValueError(f"request does not fit: P + max_new_tokens + {3 * BLOCK_ROWS} = "
                         f"{P + max_new_tokens + 3 * BLOCK_ROWS} > max_rows = {max_rows}")
    if P + max_new_tokens + BLOCK_ROWS > out_len:
        raise ValueError(f"request does not fit: P + max_new_tokens + {BLOCK_ROWS} = "
                         f"{P + max_new_tokens + BLOCK_ROWS} > out_len = {out_len}")


class _DecoderDriver:
    """The driver protocol of dflash_amd.slots over one BatchedDecoder.  It holds no reference to the engine or the
    loop: an engine that goes out of scope is freed at once, graphs included, not by a later garbage collection —
    which, if it ran inside another engine's capture, would destroy a hipGraph while a stream is capturing."""

    def __init__(self, dec: BatchedDecoder, stats: dict, use_graph: bool, temperature: float, stop_token_ids):
        self.dec, self.stats, self.use_graph = dec, stats, use_graph
        self.temperature, self.stop_token_ids = temperature, stop_token_ids
        self.hooks = [None] * dec.R
        self.guard = None

    def _captured_state(self) -> tuple:
        """Addresses a captured launch reads that a prefill could in principle move."""
        d, m, t = self.dec, self.dec.model, self.dec.target
        return (m._rope[0].data_ptr(), m._rope[1].data_ptr(), t._rope[0].data_ptr(), t._rope[1].data_ptr(),
                d.lm_wp.data_ptr(), d.lm_wp8.wp.data_ptr() if d.lm_wp8 is not None else 0, d.embed_w.data_ptr(),
                t.embed.data_ptr()) + tuple(x.data_ptr() for x in t.fp8_tensors())   # (an fp8 target's codes and scales)

    def admit(self, slot: int, req) -> None:
        p = req.payload
        t0 = cuda_time()
        ids = p.input_ids if p.input_ids.is_cuda else p.input_ids.to(self.dec.dev)
        bias = dict(p.bias)
        if p.stop_sequences:   # (no stop sequence matches before min_tokens tokens are out, bias keywords or not)
            bias.setdefault("min_tokens", p.min_tokens)
        self.dec.admit_fused(slot, ids, p.temperature, seed=p.seed, top_k=p.top_k, top_p=p.top_p,
                             repetition_penalty=p.penalties[0], presence_penalty=p.penalties[1],
                             frequency_penalty=p.penalties[2], **bias, grammar=p.grammar, min_p=p.min_p,
                             stop_sequences=p.stop_sequences)
        t1 = cuda_time()
        p.ttft, p.t_admitted = t1 - t0, t1
        self.stats["admit_s"] += t1 - t0
        self.hooks[slot] = p.hook

    def set_block_size(self, slot: int, bs: int) -> None:
        self.dec.set_block_size(slot, bs)

    def park(self, slot: int) -> None:
        self.dec.park(slot)

    def ahead_pending(self) -> bool:
        return self.dec._ahead

    def _hook(self, r: int, blk: torch.Tensor, start: int, call: int) -> None:
        h = self.hooks[r]
        if h is not None:
            h(blk[:, :max(1, self.dec.bs[r])], start, call)

    def cycle(self, ahead_ok: bool) -> list:
        d = self.dec
        hook = self._hook if any(h is not None for h in self.hooks) else None
        if d.graphs is not None:
            # (no admission of this engine can move them; a larger decoder on the same models can)
            if self._captured_state() != self.guard:
                raise RuntimeError("a buffer the captured graphs read has moved (RoPE table, lm_head, embedding)")
            out = d.cycle_graph(hook)
            self.stats["replayed_cycles"] += 1
        else:
            out = d.cycle(hook, ahead_ok=ahead_ok and not self.use_graph)
            if self.use_graph:   # the one capture of the engine's life: every length is read from the device records
                d.capture()
                self.stats["captures"] += 1
                self.guard = self._captured_state()
        return [None if o is None else (o[0], d.start[r], o[1]) for r, o in enumerate(out)]

    def retire(self, slot: int, req) -> None:
        d, p = self.dec, req.payload
        # (the slot's hit record is read here, with the ids: the next admission rewrites it)
        hit, which = d.stop_hit(slot, p.include_stop), []
        cols = _kept_cols(d.output_ids[slot:slot + 1], req.max_len, d.mask_id, self.stop_token_ids, req.n_in, hit, which)
        ids = _trim(d.output_ids[slot:slot + 1], req.max_len, d.mask_id, self.stop_token_ids, req.n_in, hit).clone()
        n_out = ids.shape[1] - req.n_in
        decode_s = cuda_time() - p.t_admitted
        self.hooks[slot] = None
        # logprobs: the positions the ids keep, [n_in, n_in + n_out) of the slot's row — each written by THIS request (its
        # admission, then the cycle that committed the position), so nothing of the slot's previous request shows
        lpf = NO_LOGPROBS if d.lp is None else logprob_fields(d.lp, slot, cols[req.n_in:])
        p.result = SimpleNamespace(output_ids=ids, num_input_tokens=req.n_in, num_output_tokens=n_out,
                                   time_to_first_token=p.ttft, time_per_output_token=decode_s / max(1, n_out),
                                   acceptance_lengths=req.taus, cycle_trace=[], profile_summary=None,
                                   request_id=req.rid, slot=slot, admitted_step=req.admitted_step,
                                   finished_step=req.finished_step,
                                   grammar_state=d.grammar_state_of(slot, ids[0], req.n_in),
                                   stop_sequence=which[0] if which else None, **lpf)


class BatchEngine:
    """submit() queues requests, step() runs one group cycle and refills free slots, run() drains the queue.

    graph: None = replay unless DFL_GRAPH=0 (the rule of run_decode); True / False force it.  With replay the first
    cycle runs eagerly, the decoder is captured ONCE and every later cycle of the engine's life is a replay, across
    admissions.  A precondition of the capture that does not hold raises here, nothing is swallowed."""

    filtering, request_temperature, temperature, penalties, logit_bias = False, False, 0.0, False, False
    min_p = False

    def __init__(self, model, target, *, slots: int = MAX_GROUP, max_rows: int, out_len: int, mask_token_id: int,
                 block_size: int = 16, stop_token_ids=None, temperature: float = 0.0, sampler: str = "torch",
                 graph: Optional[bool] = None, filtering: bool = False, request_temperature: bool = False,
                 logprobs: Optional[int] = None, penalties: bool = False, logit_bias: bool = False,
                 grammar_states: int = 0, constrain_draft: bool = False, min_p: bool = False,
                 couple_draft: bool = False, stop_sequences: bool = False):
        """stop_sequences: as BatchedDecoder takes it — requests may carry their own stop sequences (submit), matched on
        the device in front of every accept launch; results carry `stop_sequence`.
        filtering / request_temperature / logprobs / penalties / logit_bias / grammar_states / constrain_draft / min_p /
        couple_draft:
        as BatchedDecoder takes them — what requests may carry (submit); fixed here because they fix the one captured
        launch sequence of the engine's life (logits_stage.LogitsStage has the row processors' order and the DESIGN.md
        sections).  A slot's values are rewritten whole on every admission and read by address by the captured launches:
        nothing of the slot's previous request survives, and requests at the neutral values emit the same ids.
        logprobs = N: every result carries logprobs / top_logprob_ids / top_logprobs; there is no per-request switch.
        grammar_states = N: add_grammar loads a TokenDFA into the pool and returns the handle submit takes; the pool's
        address is fixed, so the one capture serves grammars loaded later; results carry `grammar_state`.
        request_temperature: greedy and sampled requests share the weight pass and the capture; needs sampler='device';
        `temperature` is then the default of submit."""
        if not 1 <= block_size <= 32:
            raise ValueError("block_size is 1..32")
        if block_size > BLOCK_ROWS:
            raise NotImplementedError("the engine takes blocks of 1..16 rows (one tile per request); blocks of 17..32 rows "
                                      "run through dflash_generate_batch")
        if not 1 <= slots <= MAX_GROUP:
            raise ValueError(f"slots is 1..{MAX_GROUP}")
        sampled_on_host = temperature >= 1e-5 and sampler != "device"
        if graph is None:
            graph = os.environ.get("DFL_GRAPH", "1") != "0" and not sampled_on_host
        elif graph and sampled_on_host:
            raise ValueError("graph=True at T > 0 needs sampler='device': torch.multinomial on the caller's RNG stream "
                             "cannot be captured")
        self.use_graph = bool(graph)
        self.dec = BatchedDecoder(model, target, slots, max_rows=max_rows, out_len=out_len, mask_token_id=mask_token_id,
                                  stop_token_ids=stop_token_ids, temperature=temperature, sampler=sampler,
                                  filtering=filtering, request_temperature=request_temperature, logprobs=logprobs,
                                  penalties=penalties, logit_bias=logit_bias, grammar_states=grammar_states,
                                  constrain_draft=constrain_draft, min_p=min_p, couple_draft=couple_draft,
                                  stop_sequences=stop_sequences)
        self.min_p = bool(min_p)
        self.filtering, self.temperature, self.penalties = bool(filtering), float(temperature), bool(penalties)
        self.logit_bias = bool(logit_bias)
        self.request_temperature = bool(request_temperature)
        self.stats = dict(group_cycles=0, live_slot_cycles=0, admissions=0, replayed_cycles=0, admit_s=0.0, captures=0,
                          graph=self.use_graph)
        driver = _DecoderDriver(self.dec, self.stats, self.use_graph, float(temperature), stop_token_ids)
        stop_always = stop_token_ids is not None and mask_token_id in stop_token_ids
        self.loop = SlotLoop(driver, slots, block_size, may_stop=stop_token_ids is not None or bool(stop_sequences),
                             stop_always=stop_always,
                             stats=self.stats)
        self._pending: list = []   # results of requests finished since the last run()

    def submit(self, input_ids: torch.Tensor, max_new_tokens: int, *, seed: Optional[int] = None,
               draft_token_hook: Optional[Callable] = None, top_k: int = 0, top_p: float = 1.0,
               temperature: Optional[float] = None, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
               frequency_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
               min_tokens: int = 0, grammar=None, min_p=None, stop_sequences=None,
               include_stop_sequence: bool = True) -> int:
        """Queue a request; returns its id (ids count up in submission order).  draft_token_hook(block_view, start,
        call): `call` counts from 0 at the request's admission; the view has the cycle's block size.
        top_k / top_p: the request's own filter on its T > 0 draws (an engine built with filtering=True); accepted and
        ignored on a request whose own temperature is 0.
        temperature: the request's own (None: the engine's); a value that differs from the engine's needs an engine built
        with request_temperature=True.
        repetition_penalty / presence_penalty / frequency_penalty: the request's own (an engine built with
        penalties=True; 1.0 / 0.0 / 0.0: off).
        logit_bias / allowed_token_ids / banned_token_ids / min_tokens: the request's own (an engine built with
        logit_bias=True; None / None / None / 0: off), validated here.
        grammar: a handle add_grammar returned (None: no grammar; an engine built with grammar_states > 0).
        min_p: the request's own (None / 0: off; an engine built with min_p=True, else ValueError); it does nothing on a
        request whose own temperature is 0.
        stop_sequences: the request's own (None: none; an engine built with stop_sequences=True, else ValueError),
        validated here; a request's own stop IDS are sequences of length 1.  include_stop_sequence=False cuts the matched
        ids off the result as well."""
        seqs = None if stop_sequences is None else self.dec.check_stop_sequences(stop_sequences)
        mp = ops.check_min_p(min_p)
        if grammar is not None:   # (raises on a handle this engine did not return, and on an engine without a pool)
            self.dec.check_grammar_handle(grammar)
        pen = ops.check_penalties(repetition_penalty, presence_penalty, frequency_penalty)
        bias = dict(logit_bias=logit_bias, allowed_token_ids=allowed_token_ids, banned_token_ids=banned_token_ids,
                    min_tokens=min_tokens)
        if (logit_bias is None and allowed_token_ids is None and banned_token_ids is None and min_tokens == 0) \
                or self.dec.check_bias(**bias) is None:   # (raises on a bad value, and on a request an unflagged engine cannot serve)
            bias = {}
        if input_ids.dim() != 2 or input_ids.shape[0] != 1:
            raise ValueError("submit: input_ids must be a [1, P] tensor")
        T = self.temperature if temperature is None else float(temperature)
        if T != self.temperature and not self.request_temperature:
            raise ValueError("submit: a temperature other than the engine's needs an engine built with "
                             "request_temperature=True")
        on = dict(min_p=mp is not None, penalties=pen is not None, filter=ops.check_filter(top_k, top_p) and T >= 1e-5)
        check_features([f for f, v in on.items() if v], where="submit: ", sampling=T >= 1e-5, owner="engine",
                       seeded=mp is None or T < 1e-5 or self.dec.sampler == "device",   # (the rest: at the admission)
                       built=dict(min_p=self.min_p, penalties=self.penalties, filter=self.filtering))
        check_fit(input_ids.shape[1], int(max_new_tokens), self.dec.max_rows, self.dec.out_len)
        req = self.loop.submit(input_ids.shape[1], int(max_new_tokens),
                               SimpleNamespace(input_ids=input_ids, seed=seed, hook=draft_token_hook, result=None,
                                               ttft=0.0, t_admitted=0.0, top_k=int(top_k), top_p=float(top_p),
                                               temperature=T, penalties=pen or (1.0, 0.0, 0.0), bias=bias,
                                               grammar=grammar, min_p=mp, stop_sequences=seqs,
                                               include_stop=bool(include_stop_sequence), min_tokens=int(min_tokens)))
        return req.rid

    def add_grammar(self, dfa) -> int:
        """Load a TokenDFA, or a ByteGrammar (lifted on the device), into the engine's pool; the
        handle submit(..., grammar=handle) takes.  ValueError when the pool is full or the engine was built with
        grammar_states = 0."""
        return self.dec.add_grammar(dfa)

    @torch.inference_mode()
    def step(self) -> list:
        """One group cycle; the result namespaces of the requests that finished on it."""
        done = [r.payload.result for r in self.loop.step()]
        self._pending.extend(done)
        return done

    @torch.inference_mode()
    def run(self) -> list:
        """Drain the queue.  Returns the results of every request finished since the last run(), in submission order."""
        while not self.loop.idle:
            self.step()
        out, self._pending = sorted(self._pending, key=lambda r: r.request_id), []
        return out


@torch.inference_mode()
def dflash_generate_stream(model, target, input_ids: Sequence[torch.Tensor], mask_token_id: int,
                           max_new_tokens: Union[int, Sequence[int]], block_size: int, stop_token_ids,
                           temperature=0.0, *, slots: int = MAX_GROUP, draft_token_hook: Optional[Callable] = None,
                           sampler: str = "torch", seed=None, top_k=0, top_p=1.0,
                           logprobs: Optional[int] = None, repetition_penalty=1.0, presence_penalty=0.0,
                           frequency_penalty=0.0, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
                           min_tokens=0, grammar=None, constrain_draft: bool = False, min_p=None,
                           couple_draft: bool = False, stop_sequences=None,
                           include_stop_sequence: bool = True) -> list:
    """`dflash_generate_batch` with slot refill: one namespace per prompt with the fields of benchmark.py:242-251, each
    request emitting what its own `dflash_generate` run emits.  max_new_tokens: one int or one per prompt.
    draft_token_hook(request_index, block_view, start, call).  seed as in dflash_generate_batch (an int s gives prompt i
    the seed s + i).  time_to_first_token is the request's own admission; time_per_output_token its own decode wall
    time, admission to last token, over its tokens.  top_k / top_p: a scalar or one value per prompt.
    temperature: one float, or one value per prompt (values that differ: sampler="device", an engine built with
    request_temperature=True).  logprobs: as dflash_generate, for every prompt.
    repetition_penalty / presence_penalty / frequency_penalty: a scalar or one value per prompt.
    logit_bias / allowed_token_ids / banned_token_ids / min_tokens: one value for every prompt, or a sequence with one
    value (or None) per prompt.
    grammar: one TokenDFA for every prompt, or a sequence with one (or None) per prompt.
    constrain_draft: as dflash_generate_batch.  couple_draft: likewise.
    min_p: a scalar, or one value (or None) per prompt.
    stop_sequences / include_stop_sequence: as dflash_generate_batch."""
    stops = _prompt_stop_sequences(stop_sequences, len(input_ids), target, mask_token_id)
    dfas = _prompt_grammars(grammar, len(input_ids))
    for d in {id(d): d for d in dfas if d is not None}.values():
        ops.check_grammar(d, target.V)
    n = len(input_ids)
    mnt = [int(max_new_tokens)] * n if isinstance(max_new_tokens, int) else [int(x) for x in max_new_tokens]
    if len(mnt) != n:
        raise ValueError("one max_new_tokens per prompt")
    if block_size > BLOCK_ROWS:
        raise NotImplementedError("dflash_generate_stream takes blocks of 1..16 rows; 17..32-row blocks run through "
                                  "dflash_generate_batch")
    temps, per_request = _prompt_temperatures(temperature, n, sampler)
    seeds = _prompt_seeds(sampler, seed, n, any(t >= 1e-5 for t in temps))
    top_ks, top_ps, filtering = _prompt_filters(top_k, top_p, n, temps, sampler)
    min_ps, min_p_on = _prompt_min_p(min_p, n, temps, sampler)
    pens, penalties = _prompt_penalties(repetition_penalty, presence_penalty, frequency_penalty, n)
    biases, logit_bias_on = _prompt_bias(target, logit_bias, allowed_token_ids, banned_token_ids, min_tokens, n,
                                         stop_token_ids)
    need = max([p.shape[1] + k for p, k in zip(input_ids, mnt)] + [1])
    eng = BatchEngine(model, target, slots=max(1, min(slots, max(n, 1))), max_rows=need + 3 * BLOCK_ROWS,
                      out_len=need + BLOCK_ROWS, mask_token_id=mask_token_id, block_size=block_size,
                      stop_token_ids=stop_token_ids, temperature=max(temps, default=0.0), sampler=sampler, filtering=filtering,
                      request_temperature=per_request, logprobs=logprobs, penalties=penalties, logit_bias=logit_bias_on,
                      grammar_states=_pool_rows(dfas), constrain_draft=constrain_draft, min_p=min_p_on,
                      couple_draft=couple_draft, stop_sequences=any(s is not None for s in stops))
    handles = _load_grammars(eng, dfas)
    for i, p in enumerate(input_ids):
        hook = (lambda blk, start, call, i=i: draft_token_hook(i, blk, start, call)) if draft_token_hook else None
        eng.submit(p, mnt[i], seed=seeds[i], draft_token_hook=hook, top_k=top_ks[i], top_p=top_ps[i],
                   temperature=temps[i], repetition_penalty=pens[i][0], presence_penalty=pens[i][1],
                   frequency_penalty=pens[i][2], **biases[i], grammar=handles[i],
                   min_p=min_ps[i] if min_p_on else None, stop_sequences=stops[i],
                   include_stop_sequence=include_stop_sequence)
    return eng.run()
