"""Ragged batch of requests on one GPU: R <= 4 requests advance one decode cycle together
and share every weight byte of the draft forward, the lm_head and the target verify
(BASELINE.json configs[2]: 32 requests over 8 GPUs = 4 per GPU).

The reference has no batched form of the path: `spec_generate` is batch-1 by construction
(model/dflash.py:206-211,258) and its "batched" harness is a Python loop over prompts
(benchmark_batched.py:212-243, benchmark.py:445-470).  `dflash_generate_batch` therefore
keeps that contract — a list of prompts in, one `dflash_generate` namespace per prompt out,
each identical to what the single-request loop returns for that prompt — and changes only
how the cycles are executed: per cycle ONE pass over the weights for all live requests
(dfl_*_batch kernels), per-request lengths S / tau / start held on the device (`dyn`),
per-request preallocated KV caches, one device->host read of R x 4 ints.

Needs the native target (`dflash_amd.NativeTarget`): the HF forward cannot take requests
of different lengths without padding masks, which is exactly the cost this path removes.
Sparse-MoE targets (round 3): attention and the dense projections run batched, the expert
MLP per request (`NativeTarget.moe_mlp_tiles`).
"""
from __future__ import annotations

import os

from types import SimpleNamespace
from typing import Callable, Optional, Sequence

import torch

from . import ops
from .generate import (NO_LOGPROBS, _bf16_table, _draw_rows, _kept_cols, _stop_hit, _taps, _trim, capture_graph, check_couple_draft,
                       first_token_stop,
                       cuda_time, logprob_fields, resolve_seed)
from .logits_stage import LogitsStage, check_features
from .model import DFlashDraftModel
from .target import NativeTarget
from .tile_stack import TileStack, gemm_ws
from .utils import sample

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
MAX_GROUP = 4


class _View:
    """One request's slice of the group caches, with the fields the single-request
    prefill code expects (DFlashKVCache / TargetKVCache)."""

    def __init__(self, k, v, dyn, max_rows):
        self.k, self.v, self.dyn, self.max_rows, self.length = k, v, dyn, max_rows, 0

    def get_seq_length(self, layer_idx: int = 0) -> int:
        return self.length


class BatchedDecoder:
    """Device state and per-cycle launch sequence of one group of R <= 4 requests."""

    def __init__(self, model: DFlashDraftModel, target: NativeTarget, n_requests: int, max_rows: int,
                 out_len: int, mask_token_id: int, stop_token_ids=None, max_splits: int = 32,
                 temperature: float = 0.0, tiles_per_request: int = 1, sampler: str = "torch",
                 draft_temperature: float = 0.0, filtering: bool = False, request_temperature: bool = False,
                 logprobs: Optional[int] = None, penalties: bool = False, logit_bias: bool = False,
                 grammar_states: int = 0, constrain_draft: bool = False, min_p: bool = False,
                 couple_draft: bool = False, stop_sequences: bool = False):
        """stop_sequences (fixed here: it fixes the captured launch sequence): dfl_stop_seq_rows directly in front of every
        accept launch, over every slot's own table of stop sequences (admit(..., stop_sequences=...); DESIGN.md section
        22).  Off: the launches of before, nothing allocated, and a request that carries sequences is refused.
        filtering / logprobs / penalties / logit_bias / grammar_states / min_p: which row processors the verify runs
        between its head launch and the posterior (logits_stage.LogitsStage has the order, what each reads and the
        DESIGN.md sections).  Fixed here: they fix the captured launch sequence and the addresses it reads.  Requests
        carry their own values (admit); a slot at the neutral values gets the ids of a decoder built without the
        feature, and a greedy decoder enqueues neither min_p nor a draw.  grammar_states = N: a pool of N automaton rows
        that add_grammar fills.
        constrain_draft (fixed here for the same reason; needs grammar_states > 0 or logit_bias, one tile per request and
        a greedy draft): the draft's head launch materialises its logits and ONE dfl_grammar_draft_rows launch over all
        tiles re-picks every slot's draft tokens under its automaton and its bans ("The draft under
        the grammar").  A slot without a grammar and without bans keeps its argmax ids.
        couple_draft (fixed here for the same reason; sampler="device" where anything samples): the draft's head launch is
        dfl_gemm_sample_batch on stream TARGET with each slot's seed and the TARGET's invT (the per-slot array with
        request_temperature: a greedy slot keeps the plain argmax), position base = the draft record's START word — every
        slot's draft token j is picked under the noise the verify draws that position with.  The
        bf16 lm_head for this launch, also in an fp8 draft.  With constrain_draft the pick is the noise form.  A decoder
        in which nothing samples enqueues the launches of before."""
        logprobs = ops.check_logprobs(logprobs)
        draft_temperature = check_couple_draft(couple_draft, temperature, draft_temperature if draft_temperature >= 1e-5
                                               else None, sampler)
        self.couple = bool(couple_draft) and (temperature >= 1e-5 or bool(request_temperature))
        if self.couple:
            draft_temperature = 0.0   # the draft counts as greedy below: only its head launch differs
        grammar_states = int(grammar_states)
        if grammar_states < 0:
            raise ValueError(f"grammar_states must be >= 0 (0: off), got {grammar_states}")
        on = dict(min_p=min_p, grammar=grammar_states, logit_bias=logit_bias, penalties=penalties, filter=filtering)
        check_features([f for f, v in on.items() if v], sampling=temperature >= 1e-5, seeded=sampler == "device",
                       wide=tiles_per_request != 1)
        if constrain_draft:
            if not (grammar_states or logit_bias):
                raise ValueError("constrain_draft needs something to constrain by: a decoder built with grammar_states > 0 "
                                 "or logit_bias=True")
            if tiles_per_request != 1:
                raise NotImplementedError("constrain_draft takes blocks of <= 16 rows (tiles_per_request = 1)")
            if draft_temperature >= 1e-5:
                raise NotImplementedError("constrain_draft takes a greedy draft (a sampled draft draws in the head "
                                          "launch's epilogue, before the pick)")
        if not isinstance(target, NativeTarget):
            raise TypeError("BatchedDecoder needs a dflash_amd.NativeTarget (see module docstring)")
        if tiles_per_request not in (1, 2):
            raise ValueError("tiles_per_request is 1 (blocks of <= 16 rows) or 2 (blocks of <= 32 rows)")
        if not 1 <= n_requests * tiles_per_request <= MAX_GROUP:
            raise ValueError(f"a group holds 1..{MAX_GROUP} sixteen-row tiles (requests x tiles_per_request)")
        if tiles_per_request == 2 and temperature >= 1e-5 and sampler != "device":
            raise NotImplementedError("blocks of more than 16 rows in the ragged batch sample at T > 0 with sampler='device' only")
        if draft_temperature >= 1e-5 and sampler != "device":
            raise NotImplementedError("a sampled draft in the ragged batch needs sampler='device'")
        resolve_seed(sampler, None, needed=False)   # (validates the name)
        if request_temperature and sampler != "device":
            raise ValueError("request_temperature needs sampler='device': a slot's temperature is read by the seeded draw "
                             "on the device")
        if model.w is None:
            raise RuntimeError("draft weights not loaded")
        c, t = model.config, target
        if c.hidden_size != t.H:
            raise ValueError("draft and target hidden sizes differ")
        self.model, self.target, self.cfg = model, target, c
        # Blocks of 17..32 rows (benchmark.py's block-size sweep): a request takes TPR = 2 consecutive 16-row tiles of every
        # per-tile launch (GEMMs, norms, embedding, context K/V append), one cache, one slot of the attention / accept
        # launches.  Two kinds of length records then: per REQUEST (dyn_d / dyn_t: attention, accept) and per TILE (dyn_dt /
        # dyn_tt: valid rows of each tile), both kept by dfl_accept_commit_batch.  TPR = 1: the same tensors.
        self.TPR = TPR = tiles_per_request
        self.R, self.NT = n_requests, n_requests * TPR
        self.MT = ops.batch_tiles(self.NT)
        self.BW = 16 * TPR                    # slots of a request's block
        NREQ = self.MT // TPR                 # request slots of the caches / id buffers
        self.dev = dev = model.device
        self.max_rows, self.out_len, self.mask_id = int(max_rows), int(out_len), int(mask_token_id)
        self.max_splits = max_splits
        self.temperature = float(temperature)
        self.draft_temperature = float(draft_temperature)
        # sampler="device": T > 0 draws are seeded on the device, one seed per request slot in a
        # device array, so that a captured graph and a re-admitted slot keep working
        self.sampler = sampler
        self._logits = None
        R, MT, H, I = self.R, self.MT, c.hidden_size, c.intermediate_size
        z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=dev)  # noqa: E731

        # ---- lengths (device): draft form and block form, see dfl_accept_commit_batch
        self.dyn_d, self.dyn_t = z(MT, 8, dt=I32), z(MT, 8, dt=I32)
        self.dyn_dt, self.dyn_tt = (self.dyn_d, self.dyn_t) if TPR == 1 else (z(MT, 8, dt=I32), z(MT, 8, dt=I32))
        # ---- caches [request][layer][kv head][row][128]
        Ld, Lt = c.num_hidden_layers, t.L
        self.dk, self.dv = z(NREQ, Ld, c.num_key_value_heads, max_rows, 128), z(NREQ, Ld, c.num_key_value_heads, max_rows, 128)
        self.tk, self.tv = z(NREQ, Lt, t.n_kv, max_rows, 128), z(NREQ, Lt, t.n_kv, max_rows, 128)
        # ---- ids
        self.block = torch.full((NREQ, self.BW), self.mask_id, dtype=I64, device=dev)
        self.post = z(NREQ, self.BW, dt=I64)
        self.ids_tmp = z(MT, 16, dt=I64)      # TPR = 2: the draft's ids of every tile row (row 0 of tile 0 is not a draft token)
        self.result = z(MT, 4, dt=I32)
        self.seeds = z(NREQ, dt=I64)
        # filtering (fixed here: it fixes the captured launch sequence): the verify materialises its logits and
        # dfl_sample_rows_nucleus draws under each slot's top_k / top_p (0 / 1.0: that slot's plain draw, same ids as the
        # fused epilogue's); at T = 0 the argmax is always kept and the greedy path runs unchanged
        # request_temperature (fixed here for the same reason): every slot draws at its own invT, read by address from
        # inv_ts beside its seed; 0 is a greedy slot ("Per-request temperature").  `temperature` is
        # then only the default of admit(): the verify runs the _t launch forms whatever it is.
        self.request_temperature = bool(request_temperature)
        self.inv_ts = z(NREQ, dt=F32) if self.request_temperature else None
        sampling = self.temperature >= 1e-5 or self.request_temperature
        self.filtering = bool(filtering) and sampling
        self.stop_t = torch.tensor(stop_token_ids, dtype=I64, device=dev) if stop_token_ids else None
        # the row processors' state and buffers, one slot per request slot, values read by address (None: nothing is on);
        # the flags say what the decoder was built with (admit refuses a request that asks for more)
        self.penalties, self.logit_bias, self.min_p = bool(penalties), bool(logit_bias), bool(min_p)
        self.stage, self.grammar, self.lp = None, None, None
        if self.filtering or logprobs is not None or penalties or logit_bias or grammar_states or min_p:
            self.stage = LogitsStage(NREQ, target.V, dev, tiles=MT, device_values=True, out_len=out_len, logprobs=logprobs,
                                     penalties=penalties, logit_bias=logit_bias, grammar_states=grammar_states,
                                     min_p=min_p, filtering=filtering, sampling=sampling,
                                     stop_ids=self.stop_t)
            self.grammar, self.lp, self._grammars = self.stage.gr, self.stage.lp, []
            self.pen_table = self.stage.pen_table   # (None without penalties)
            if self.stage.materialises:   # where every head launch of such a decoder materialises its logits
                self._logits = self.stage.raw.view(MT, 16, target.V)
        # constrain_draft: the draft head's materialised logits, read by the pick launch right behind it
        self.constrain_draft = bool(constrain_draft)
        self._cd_logits = z(MT, 16, target.V) if self.constrain_draft else None
        self.output_ids = torch.full((NREQ, out_len), self.mask_id, dtype=I64, device=dev)
        self.stop_token_ids = list(stop_token_ids) if stop_token_ids else None
        # stop sequences: one table row and one hit record per request slot, read by address (None: off)
        self.sq = ops.stop_seq_state(NREQ, dev) if stop_sequences else None
        self.stop_seqs = [None] * NREQ   # host mirror: the slot's sequences as admitted (the trim needs their lengths)
        # ---- draft scratch
        self.nqkv_d = c.q_dim + 2 * c.kv_dim
        self.nkv_all = Ld * 2 * c.kv_dim
        ks = ops.batch_ksplit
        self.d = dict(ctxh=z(MT, 16, H), ss_emb=z(MT, 16, dt=F32),
                      part_kv=z(ks(H) * MT * 16 * self.nkv_all, dt=F32), taps=z(MT, 16, c.fc_in))
        # context K/V weights of all layers as ONE packed weight: the k/v column tiles of each
        # layer's packed qkv, concatenated (tile-major layout: a plain cat of tile ranges)
        L = model.w["layers"]
        self.kv_all = torch.cat([lw["qkv"][c.q_dim * H:] for lw in L]).contiguous()
        self.k_norm_all = torch.stack([lw["k_norm"] for lw in L]).contiguous()
        # ---- target scratch
        self.t = dict(ss_emb=z(MT, 16, dt=F32))
        # ---- shared workspace (launches are stream-ordered) and the two stacks: their rows, sums and row sources
        # (normalised operands come from dfl_norm_frag_batch: at 4 tiles the in-GEMM norm of the
        # single-request path, replicated in every workgroup, costs more than that launch)
        self.gws = gemm_ws(H, (c.vocab_size, t.V, 2 * I, 2 * t.I, self.nqkv_d, t.nqkv), (H, I, t.I, c.fc_in, c.q_dim), dev)
        sd = TileStack(H=H, q_dim=c.q_dim, I=I, nqkv=self.nqkv_d, eps=c.rms_norm_eps, MT=MT, gws=self.gws, part_qkv=True)
        st = TileStack(H=H, q_dim=t.q_dim, I=t.I, nqkv=t.nqkv, eps=t.eps, MT=MT, gws=self.gws, part_qkv=True,
                       moe_nsplit=t.moe_nsplit if getattr(t, "is_moe", False) else 0)
        self.src_taps = ops.brows_plain(self.d["taps"], ops.DYN_TAU)
        # round 2: the attention stage on finished bf16 q/k/v rows (dfl_attn_head_batch); "fused" keeps the round-1 stage
        self.attn_impl = getattr(model, "attn_impl", "head")
        if TPR == 2 and self.attn_impl != "head":
            raise NotImplementedError("blocks of more than 16 rows need the 'head' attention stage")
        # round 4: the q/k/v projection leaves fp32 K-part sums and the attention launch sums them while it loads its rows
        # (dfl_attn_head_batch_f32) — blocks of <= 16 rows, <= 2 K parts (hidden <= 4096); otherwise the round-3 form
        # (finished bf16 rows: slabs + ticket + combine inside the GEMM)
        self.qkv_parts = tiles_per_request == 1 and ops.batch_ksplit(H) <= 2
        # what the attention launch of a model side takes (_attend); the workspaces are one per model: the arrival
        # tickets sit behind the partials, whose size depends on n_q
        self.side_d = SimpleNamespace(
            stack=sd, q_dim=c.q_dim, kv_dim=c.kv_dim, n_q=c.num_attention_heads, n_kv=c.num_key_value_heads,
            scale=c.head_dim ** -0.5, causal=False, k=self.dk, v=self.dv, rope=model._rope_tab,
            aws=ops.attn_fused_batch_ws(MT, c.num_attention_heads, c.num_key_value_heads, max_splits, dev),
            hws=ops.attn_head_batch_ws(MT, c.num_attention_heads, max_splits, dev, q_tiles=TPR))
        self.side_t = SimpleNamespace(
            stack=st, q_dim=t.q_dim, kv_dim=t.kv_dim, n_q=t.n_q, n_kv=t.n_kv, scale=128 ** -0.5, causal=True, k=self.tk,
            v=self.tv, rope=t._rope_tab, aws=ops.attn_fused_batch_ws(MT, t.n_q, t.n_kv, max_splits, dev),
            hws=ops.attn_head_batch_ws(MT, t.n_q, max_splits, dev, q_tiles=TPR))
        self.lm_wp = None
        self.lm_wp8 = None
        self.embed_w = None
        # ---- host mirror of the lengths
        self.start = [0] * R
        self.n_in = [0] * R
        self.live = [False] * R
        self.hook_calls = [0] * R
        self.bs = [self.BW] * R
        self.events = None  # set to a dict to have cycle() record (start, end) event pairs per phase
        self._ahead, self._ahead_ev = False, None   # a run-ahead draft is in flight (cycle(ahead_ok=True))
        self.run_ahead = os.environ.get("DFL_RUN_AHEAD", "1") != "0"
        self.graphs = None   # capture(): the three hipGraphs of a cycle

    def _mark(self, key, which):
        if self.events is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.events.setdefault(key, [None, None])[which] = e

    def _lm8(self):
        """The e4m3 lm_head of the greedy draft head, or None where the draft does not stream its codes; packed on first
        use (0.6 GB at 8B shapes: not for a model that never reads it)."""
        if not self.model.streams_fp8_tiles():
            return None
        if self.lm_wp8 is None:   # (an fp8 target's own codes where it has them: one e4m3 copy serves both)
            self.lm_wp8 = getattr(self.target, "lm_wp8", None) or self.model.packed_lm_head_fp8(self.target.lm_head)
        return self.lm_wp8

    def _t_head(self):
        """The verify's lm_head: an fp8 target that streams takes its e4m3 codes, else the shared packed bf16 copy."""
        return self.target.lm_wp8 if self.target.streams_fp8_tiles() else self.lm_wp

    # ------------------------------------------------------------------ admission
    def _admit_prefill(self, r: int, input_ids: torch.Tensor, temperature: float, seed: Optional[int], top_k=0,
                       top_p=1.0, penalties=(1.0, 0.0, 0.0), bias=None, grammar=None, min_p=None):
        """The launches both admissions share: target prefill into slot r's cache, the first token, the prompt's context
        rows into the draft cache except the last <= 16.  Returns (P, first token [1, 1] on the device, tapped rows
        [P, fc_in], the seed written for the slot or None)."""
        m, t = self.model, self.target
        gr = self.check_grammar_handle(grammar)
        pen = ops.check_penalties(*penalties)
        lb = self.check_bias(**bias) if bias else None
        if gr is not None and lb is not None:   # a reachable state whose legal tokens this request's bias bans all
            if ops.is_byte_grammar(gr[1]):   # a ByteGrammar: its table exists on the device only
                ops.grammar_reach_check(self.grammar, gr[0], gr[1].num_states, gr[1].start, lb[0])
            else:
                ops.check_grammar(gr[1], t.V, lb[0])
        flt = None
        if ops.check_filter(top_k, top_p) and temperature >= 1e-5:
            flt = dict(top_k=int(top_k), top_p=float(top_p))
        mp = ops.check_min_p(min_p)
        on = dict(min_p=mp is not None, grammar=gr is not None, logit_bias=lb is not None, penalties=pen is not None,
                  filter=flt is not None)
        check_features([f for f, v in on.items() if v], where="admit: ", sampling=temperature >= 1e-5,
                       seeded=self.sampler == "device",
                       built=dict(min_p=self.min_p, penalties=self.penalties, filter=self.filtering))
        if input_ids.shape[0] != 1 or not input_ids.is_cuda:
            raise ValueError("admit: input_ids must be a [1, P] GPU tensor")
        P = input_ids.shape[1]
        if P + 2 * self.BW > self.max_rows or P + 1 > self.out_len:
            raise ValueError("admit: prompt does not fit the group's caches")
        if self.lm_wp is None:
            self.lm_wp = m.packed_lm_head(t.lm_head)
            t.share_lm_head(self.lm_wp)
            # an fp8 draft that streams: its greedy unmask takes an e4m3 copy of the lm_head (an fp8 target's own codes,
            # else packed here beside the bf16 one the target keeps)
            self._lm8()
            self.embed_w = _bf16_table(t.model.embed_tokens.weight, self.dev)
        tc = _View(self.tk[r], self.tv[r], None, self.max_rows)
        out = t.prefill(input_ids, tc, output_hidden_states=True, tap_layers=self.model.target_layer_ids)
        sd = None
        if self.sampler == "device" and (temperature >= 1e-5 or self.temperature >= 1e-5):
            sd = resolve_seed("device", seed)
        if self.stage is not None:   # the slot's values, rewritten whatever ran in the slot before, and the first token
            first = self.stage.admit(r, out.logits[0, -1:], input_ids, P, temperature=temperature, seed=sd, penalties=pen,
                                     bias=(lb[0], P + lb[1] if lb[1] else 0) if lb else None,
                                     grammar=(gr[0], gr[1].start) if gr else None, min_p=mp, flt=flt)
        elif sd is not None and temperature >= 1e-5:
            first = _draw_rows(out.logits[:, -1:], temperature, sd, P)
        else:
            first = sample(out.logits[:, -1:], temperature)
        if self.request_temperature:   # the slot's invT for every later token; 0: greedy
            self.inv_ts[r:r + 1].fill_(ops.inv_temperature(temperature) if temperature >= 1e-5 else 0.0)
        th = _taps(out.hidden_states, m.target_layer_ids)[0]          # [P, fc_in]
        n_tail = min(16, P)
        dc = _View(self.dk[r], self.dv[r], torch.zeros(8, dtype=I32, device=self.dev), self.max_rows)
        if P > n_tail:
            m.prefill_context(dc, th[:P - n_tail], 0)
        return P, first, th, sd

    def check_bias(self, logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_tokens=0):
        """ops.check_logit_bias of one request's values against this decoder's vocabulary and stop ids: None (neutral),
        or (b fp32 [V] on the host, min_tokens).  Values that are not neutral need a decoder built with logit_bias=True."""
        if logit_bias is None and allowed_token_ids is None and banned_token_ids is None and min_tokens == 0:
            return None
        lb = ops.check_logit_bias(self.target.V, logit_bias, allowed_token_ids, banned_token_ids, min_tokens,
                                  self.stop_token_ids)
        if lb is not None and not self.logit_bias:
            raise ValueError("logit_bias / allowed_token_ids / banned_token_ids / min_tokens need a decoder built with "
                             "logit_bias=True")
        return lb

    def check_stop_sequences(self, stop_sequences):
        """ops.check_stop_sequences of one request's value against this decoder's vocabulary and mask id: None (none), or
        the list of lists.  A request that carries sequences needs a decoder built with stop_sequences=True."""
        if stop_sequences is None:
            return None
        seqs = ops.check_stop_sequences(stop_sequences, self.target.V, self.mask_id)
        if seqs is not None and getattr(self, "sq", None) is None:
            raise ValueError("stop_sequences need a decoder built with stop_sequences=True")
        return seqs

    def _admit_stop(self, r: int, P: int, seqs, min_tokens) -> None:
        """Behind the slot's records: its table rows rewritten whole (nothing of the previous request survives), then the
        first token — produced before any accept launch runs — through the same launch over a one-row block
        (generate.first_token_stop), its stop word ORed into the slot's draft-form record on the device."""
        self.stop_seqs[r] = seqs
        if self.sq is None:
            return
        mt = int(min_tokens) if seqs else 0
        ops.stop_seq_set(self.sq, r, seqs, first_pos=P, min_end=P + mt if mt > 0 else 0)
        if seqs:
            first_token_stop(self.sq, r, self.output_ids[r], P, dyn_row=self.dyn_d[r])

    def stop_hit(self, r: int, include: bool = True):
        """Slot r's hit record as _trim / _kept_cols take it (read with the ids, at the end of the request), or None."""
        return _stop_hit(self.sq, r, self.stop_seqs[r], include)

    grammar = None   # (the state of a decoder built with grammar_states > 0)

    def add_grammar(self, dfa) -> int:
        """Validate a TokenDFA (ops.check_grammar) and copy its table into the pool's next free rows — a ByteGrammar is lifted
        there on the device instead (ops.grammar_load); returns the handle
        admit takes.  ValueError when the decoder was built without a pool or the pool is full.  The pool's address is
        fixed, so a captured cycle serves grammars loaded after the capture."""
        if self.grammar is None:
            raise ValueError("add_grammar needs a decoder built with grammar_states > 0")
        if ops.is_byte_grammar(dfa) and dfa.num_states > ops.LIFT_MAX_STATES:   # too large to lift: the host's table
            dfa = dfa.to_token_dfa()
        base = ops.grammar_load(self.grammar, dfa)
        self._grammars.append((base, dfa))
        return len(self._grammars) - 1

    def check_grammar_handle(self, handle):
        """(base, dfa) of a handle add_grammar returned; None for None."""
        if handle is None:
            return None
        if self.grammar is None:
            raise ValueError("grammar needs a decoder built with grammar_states > 0")
        if isinstance(handle, bool) or not isinstance(handle, int) or not 0 <= handle < len(self._grammars):
            raise ValueError(f"grammar: {handle!r} is no handle add_grammar returned")
        return self._grammars[handle]

    def grammar_state_of(self, r: int, ids: torch.Tensor, n_in: int):
        """The result field grammar_state of slot r's request: the state after the generated tokens ids[n_in:] (1-D, as
        returned), walked by dfl_grammar_advance from the grammar's start; -1 where one is illegal or the slot's own state
        was violated; None when the slot has no grammar (DecodeSession.finish_grammar has the reasons)."""
        if self.grammar is None:
            return None
        base, st = int(self.grammar.base[r]), int(self.grammar.state[r])
        if base < 0:
            return None
        if st < 0:
            return -1
        start = next(d.start for b, d in self._grammars if b == base)
        g = SimpleNamespace(table=self.grammar.table, base=self.grammar.base[r:r + 1],
                            state=torch.full((1,), int(start), dtype=I32, device=self.dev))
        ops.grammar_advance(g, ids.contiguous(), lo=n_in, hi=ids.shape[0])
        return int(g.state.item())

    @torch.inference_mode()
    def admit(self, r: int, input_ids: torch.Tensor, temperature: float = 0.0, seed: Optional[int] = None,
              top_k: int = 0, top_p: float = 1.0, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
              frequency_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
              min_tokens: int = 0, grammar=None, min_p=None, stop_sequences=None) -> None:
        """Prefill request r (model/dflash.py:218-229): target prefill through the wrapped
        model, K/V into the group cache, first token sampled, the prompt's context rows
        projected into the draft cache except the last <= 16, which become the first
        cycle's context tile.  seed (sampler="device"): the request's seed (None: one from torch's RNG).
        temperature: of the first token; of every later token too in a decoder built with request_temperature=True
        (otherwise those are drawn at the decoder's).
        top_k / top_p: the request's filter (a decoder built with filtering=True), written into the slot's device words.
        repetition_penalty / presence_penalty / frequency_penalty: the request's penalties (a decoder built with
        penalties=True), likewise; the slot's table row is cleared and re-counted from this prompt.
        logit_bias / allowed_token_ids / banned_token_ids / min_tokens: the request's own (a decoder built with
        logit_bias=True); the slot's whole bias row and min_pos are rewritten.
        grammar: a handle add_grammar returned (None: no grammar, the slot's rows pass unmasked); the slot's base and
        state are rewritten.
        min_p: the request's own (None / 0: off; a decoder built with min_p=True, else ValueError); the slot's
        ln(min_p) is rewritten.
        stop_sequences: the request's own (None: none; a decoder built with stop_sequences=True, else ValueError); the
        slot's table rows and hit record are rewritten.  A request's own stop IDS are sequences of length 1 given here."""
        seqs = self.check_stop_sequences(stop_sequences)
        P, first, th, sd = self._admit_prefill(r, input_ids, temperature, seed, top_k, top_p,
                                               (repetition_penalty, presence_penalty, frequency_penalty),
                                               dict(logit_bias=logit_bias, allowed_token_ids=allowed_token_ids,
                                                    banned_token_ids=banned_token_ids, min_tokens=min_tokens), grammar,
                                               min_p)
        self.output_ids[r].fill_(self.mask_id)
        self.output_ids[r, :P] = input_ids[0]
        if sd is not None:
            self.seeds[r] = ops.seed_i64(sd)
        self.output_ids[r, P:P + 1] = first[0]
        n_tail = min(16, P)
        t0, BW = r * self.TPR, self.BW
        self.d["taps"][t0:t0 + self.TPR].zero_()
        self.d["taps"][t0, :n_tail] = th[P - n_tail:]      # (the tail rows fit the request's first tile)
        self.block[r].fill_(self.mask_id)
        self.block[r, 0:1] = first[0]
        S = P - n_tail
        self.dyn_d[r] = torch.tensor([S, n_tail, BW, S, P, 0, 0, 0], dtype=I32)
        self.dyn_t[r] = torch.tensor([P, 0, BW, P, P, 0, 0, 0], dtype=I32)
        if self.TPR == 2:
            for j in range(2):
                self.dyn_dt[t0 + j] = torch.tensor([S + 16 * j, n_tail if j == 0 else 0, 0, S + 16 * j, P, 0, 0, 0], dtype=I32)
                self.dyn_tt[t0 + j] = torch.tensor([P, 0, 16, P, P, 0, 0, 0], dtype=I32)
        self.start[r], self.n_in[r], self.live[r], self.hook_calls[r], self.bs[r] = P, P, True, 0, BW
        self._admit_stop(r, P, seqs, min_tokens)

    @torch.inference_mode()
    def admit_fused(self, r: int, input_ids: torch.Tensor, temperature: float = 0.0, seed: Optional[int] = None,
                    top_k: int = 0, top_p: float = 1.0, repetition_penalty: float = 1.0, presence_penalty: float = 0.0,
                    frequency_penalty: float = 0.0, logit_bias=None, allowed_token_ids=None, banned_token_ids=None,
                    min_tokens: int = 0, grammar=None, min_p=None, stop_sequences=None) -> None:
        """`admit` with the slot re-armed by ONE launch (dfl_admit_slot) instead of a dozen small writes: ids, first
        token, block, context tile, both length records and the seed are written on the device from device-resident
        inputs, so that after the prefill launches the admission reads nothing back and copies nothing from the host —
        the other slots' cycle in flight is not waited for.  Leaves the device state `admit` leaves (and post / result
        of the slot cleared).  Blocks of <= 16 rows (tiles_per_request = 1)."""
        if self.TPR != 1:
            raise NotImplementedError("admit_fused re-arms one 16-row tile per request; use admit() with tiles_per_request=2")
        if not 0 <= r < self.R:
            raise ValueError(f"admit_fused: slot {r} outside 0..{self.R - 1}")
        seqs = self.check_stop_sequences(stop_sequences)
        P, first, th, sd = self._admit_prefill(r, input_ids, temperature, seed, top_k, top_p,
                                               (repetition_penalty, presence_penalty, frequency_penalty),
                                               dict(logit_bias=logit_bias, allowed_token_ids=allowed_token_ids,
                                                    banned_token_ids=banned_token_ids, min_tokens=min_tokens), grammar,
                                               min_p)
        n_tail = min(16, P)
        ops.admit_slot(r, input_ids[0].contiguous(), first.reshape(1), self.output_ids, self.block, self.post, self.result,
                       th[P - n_tail:], self.d["taps"], self.dyn_d, self.dyn_t, self.BW, self.mask_id,
                       seeds=self.seeds if sd is not None else None, seed=ops.seed_i64(sd) if sd is not None else 0)
        self.start[r], self.n_in[r], self.live[r], self.hook_calls[r], self.bs[r] = P, P, True, 0, self.BW
        self._admit_stop(r, P, seqs, min_tokens)

    def park(self, r: int) -> None:
        """Request r is finished: its tile stays in the launches but does no work."""
        self.live[r] = False
        self.dyn_d[r, ops.DYN_TAU:ops.DYN_BS + 1] = 0
        self.dyn_t[r, ops.DYN_BS] = 0
        if self.TPR == 2:
            self.dyn_dt[2 * r:2 * r + 2, ops.DYN_TAU:ops.DYN_BS + 1] = 0
            self.dyn_tt[2 * r:2 * r + 2, ops.DYN_BS] = 0

    def set_block_size(self, r: int, bs: int) -> None:
        """Tail clamp (benchmark.py:104-105): a host write only when the size changes."""
        if bs != self.bs[r]:
            self.dyn_d[r, ops.DYN_BS] = bs
            self.dyn_t[r, ops.DYN_BS] = bs
            if self.TPR == 2:
                self.dyn_tt[2 * r, ops.DYN_BS] = min(bs, 16)
                self.dyn_tt[2 * r + 1, ops.DYN_BS] = max(0, bs - 16)
            self.bs[r] = bs

    # ------------------------------------------------------------------ one cycle
    def _kv_len_max(self) -> int:
        return max([self.start[r] for r in range(self.R) if self.live[r]] + [1]) + self.BW

    def draft(self) -> None:
        """Draft forward + lm_head + greedy unmask for every live request
        (model/dflash.py:237-247): block[r, 1:bs] <- argmax."""
        self._draft_body(self._kv_len_max())
        self._mark("lm_head", 0)
        self._draft_head()
        self._mark("lm_head", 1)

    def _attend(self, sd, kvmax: int):
        """The attention launch of one model side (side_d / side_t) as TileStack.run takes it, and the q/k/v form it
        reads.  Per-request records (self.dyn_t) steer the 'head' stages, per-tile ones the fused stage."""
        st, MT = sd.stack, self.MT
        cos, sin = sd.rope(kvmax + 64)
        kw = dict(q_col=0, k_col=sd.q_dim, v_col=sd.q_dim + sd.kv_dim, n_q=sd.n_q, n_kv=sd.n_kv, eps=st.eps, cos_tab=cos,
                  sin_tab=sin, kcache=sd.k, vcache=sd.v, scale=sd.scale, causal=sd.causal, kv_len_max=kvmax,
                  max_splits=self.max_splits, out_frag=st.attn)
        nsp = ops.batch_ksplit(st.H)
        if self.attn_impl != "head":
            return "parts", lambda i, lw: ops.attn_fused_batch(
                qkv=st.part_qkv, nsplit=nsp, split_stride=MT * 16 * st.nqkv, ld=st.nqkv, R=self.NT, q_norm_w=lw["q_norm"],
                k_norm_w=lw["k_norm"], layer=i, dyn=self.dyn_tt, ws=sd.aws, **kw)
        if self.qkv_parts:   # the parts meet in the attention launch's row loads (round 4)
            return "parts", lambda i, lw: ops.attn_head_batch_f32(
                qkv_parts=st.part_qkv, nparts=nsp, MT=MT, ld=st.nqkv, R=self.R, q_norm_w=lw["q_norm"],
                k_norm_w=lw["k_norm"], layer=i, dyn=self.dyn_t, ws=sd.hws, **kw)
        return "rows", lambda i, lw: ops.attn_head_batch(
            xq=st.xq, R=self.R, q_norm_w=lw["q_norm"], k_norm_w=lw["k_norm"], layer=i, dyn=self.dyn_t, ws=sd.hws,
            q_tiles=self.TPR, **kw)

    def _draft_body(self, kvmax: int) -> None:
        m, c, d, st, MT = self.model, self.cfg, self.d, self.side_d.stack, self.MT
        R, TPR = self.NT, self.TPR                 # R: 16-row tiles of the per-tile launches
        dyn_d, dyn_t = self.dyn_dt, self.dyn_tt    # per-tile records (the per-request ones when TPR = 1)
        H = c.hidden_size
        cos, sin = m._rope_tab(kvmax + 64)
        ops.embed_rows_batch(self.embed_w, self.block.view(-1, 16), R, st.h, H, d["ss_emb"], dyn_t, ops.DYN_BS)
        # context rows: fc, then K/V of all layers appended to the draft caches
        eps = c.rms_norm_eps
        ops.gemm_resid_batch(m.w["fc"], self.src_taps, R, H, c.fc_in, d["ctxh"], add_residual=False, ws=self.gws,
                             dyn=dyn_d)
        ops.norm_frag_batch(d["ctxh"], R, m.w["hidden_norm"], eps, st.xn, dyn_d, ops.DYN_TAU)
        # an fp8 draft: the context K/V weights and the layers' gate/up, o, down — and q/k/v where
        # it leaves K parts — stream their e4m3 codes; fc (a plain-row source) reads the dequantised copy
        fp8 = m.streams_fp8_tiles()
        ops.gemm_f32_batch(m.w8["kv_all"] if fp8 else self.kv_all, st.src["xn"], R, self.nkv_all, H, d["part_kv"], dyn_d)
        ops.kv_append_batch(kv=d["part_kv"], nsplit=ops.batch_ksplit(H), split_stride=MT * 16 * self.nkv_all,
                            ld=self.nkv_all, k_col=0, v_col=c.kv_dim, col_layer_stride=2 * c.kv_dim,
                            n_layers=c.num_hidden_layers, R=R, n_kv=c.num_key_value_heads, k_norm_w=self.k_norm_all,
                            eps=c.rms_norm_eps, cos_tab=cos, sin_tab=sin, kcache=self.dk, vcache=self.dv, dyn=dyn_d,
                            tiles_per_req=TPR)
        qkv, attend = self._attend(self.side_d, kvmax)   # block rows
        st.run(m.tile_layers(qkv_parts=qkv == "parts"), R, dyn_t, attend, qkv=qkv)

    def _draft_head(self) -> None:
        m, c, R = self.model, self.cfg, self.NT
        self.side_d.stack.finish(m.w["norm"])   # last down_proj + final norm
        s = self.side_d.stack.src
        if self.couple:   # coupled draft: slot j under the noise the verify draws position START + j with (section 20)
            row0, out, off = (1, self.block, 1) if self.TPR == 1 else (0, self.ids_tmp, 0)
            inv = dict(inv_ts=self.inv_ts) if self.request_temperature else dict(temperature=self.temperature)
            ops.gemm_sample_batch(self.lm_wp, s["xn"], R, c.vocab_size, c.hidden_size, row0, 16 - row0, self.gws, out, off,
                                  self.dyn_tt, seeds=self.seeds, stream=ops.RNG_TARGET, pos_word=ops.DYN_START, pos_add=0,
                                  tiles_per_req=self.TPR, nrows_dyn_word=ops.DYN_BS, logits=self._cd_logits, **inv)
            if self.TPR == 2:
                self.block[:, 1:].copy_(self.ids_tmp.view(-1, self.BW)[:, 1:])
            if self.constrain_draft:   # the noise form of the pick below: the perturbed maximum over the legal columns
                ops.grammar_draft_sample_rows(self._cd_logits[:R], self.grammar,
                                              bias=self.stage.lb.bias if self.logit_bias else None, block=self.block,
                                              dyn=self.dyn_tt, nrows_dyn_word=ops.DYN_BS, seeds=self.seeds,
                                              pos_dyn_word=ops.DYN_START, **inv)
        elif self.draft_temperature >= 1e-5:   # sampled draft (policy loop): slot j of the block draws start + j
            row0, out, off = (1, self.block, 1) if self.TPR == 1 else (0, self.ids_tmp, 0)
            ops.gemm_sample_batch(self.lm_wp, s["xn"], R, c.vocab_size, c.hidden_size, row0, 16 - row0, self.gws, out, off,
                                  self.dyn_tt, seeds=self.seeds, temperature=self.draft_temperature, stream=ops.RNG_DRAFT,
                                  pos_word=ops.DYN_START, pos_add=0, tiles_per_req=self.TPR, nrows_dyn_word=ops.DYN_BS)
            if self.TPR == 2:
                self.block[:, 1:].copy_(self.ids_tmp.view(-1, self.BW)[:, 1:])
        elif self.TPR == 1:
            lm = self._lm8() or self.lm_wp
            ops.gemm_argmax_batch(lm, s["xn"], R, c.vocab_size, c.hidden_size, 1, 15, self.gws, self.block, 1,
                                  self.dyn_tt, nrows_dyn_word=ops.DYN_BS, logits=self._cd_logits)
            if self.constrain_draft:
                # every slot's block[1:BS] re-picked under its automaton and its bans, from the state dfl_grammar_advance
                # left behind the last accept launch (a run-ahead head is enqueued behind _accept_launch: the new state);
                # in front of the hook.  A slot with base < 0 and a bias row without bans keeps the argmax ids
                ops.grammar_draft_rows(self._cd_logits[:R], self.grammar, bias=self.stage.lb.bias if self.logit_bias else None,
                                       block=self.block, dyn=self.dyn_tt, nrows_dyn_word=ops.DYN_BS)
        else:   # row 0 of a request's SECOND tile is a draft row: all 16 rows of every tile, row 0 of the block dropped here
            lm = self._lm8() or self.lm_wp
            ops.gemm_argmax_batch(lm, s["xn"], R, c.vocab_size, c.hidden_size, 0, 16, self.gws, self.ids_tmp, 0,
                                  self.dyn_tt, nrows_dyn_word=ops.DYN_BS)
            self.block[:, 1:].copy_(self.ids_tmp.view(-1, self.BW)[:, 1:])

    def verify(self, kvmax: Optional[int] = None) -> None:
        """Target verify of every live request's block (model/dflash.py:249-257, T = 0):
        post[r] <- the target's greedy tokens, taps[r] <- the tapped layers' hidden rows."""
        t, st, R, MT, H = self.target, self.side_t.stack, self.NT, self.MT, self.cfg.hidden_size
        TPR, dyn_t, s = self.TPR, self.dyn_tt, st.src    # (R: tiles, dyn_t: per-tile records, see _draft_body)
        kvmax = kvmax or self._kv_len_max()
        ops.embed_rows_batch(t.embed, self.block.view(-1, 16), R, st.h, H, self.t["ss_emb"], dyn_t, ops.DYN_BS)
        qkv, attend = self._attend(self.side_t, kvmax)
        # (a sparse-MoE layer: the requests share attention and projections; routing and expert weights are per request)
        # (an fp8 target, DESIGN.md section 10 "The target": o, gate/up, down — and q/k/v where it leaves K parts — and
        # every head below stream its e4m3 codes; q/k/v as finished rows reads the dequantised copy)
        st.run(t.tile_layers(qkv_parts=qkv == "parts"), R, dyn_t, attend, qkv=qkv, taps=self.d["taps"],
               tap_layers=self.model.target_layer_ids, moe=t.moe_mlp_tiles)
        st.finish(t.norm)
        lm = self._t_head()
        stage = self.stage
        lg = self._logits if self.lp is not None else None   # logprobs: every head below materialises its logits
        # tile j row m of a slot predicts (and, if accepted, commits at) position POS0 + 16 j + m + 1
        where = dict(dyn=dyn_t, nrows_dyn_word=ops.DYN_BS, pos=dict(pos_word=ops.DYN_POS0, pos_add=1), tiles_per_req=TPR)
        if stage is not None and stage.processes:
            # materialise, then the stage's launches over every slot's rows at its own values; a greedy slot keeps the
            # argmax ids the launches before the draw wrote
            ops.gemm_argmax_batch(lm, s["xn"], R, t.V, H, 0, 16, self.gws, self.post.view(-1, 16), 0, dyn_t,
                                  nrows_dyn_word=ops.DYN_BS, logits=self._logits)
            draw = None
            if self.request_temperature or self.temperature >= 1e-5:
                draw = dict(seed=self.seeds, **(dict(inv_t=self.inv_ts) if self.request_temperature
                                                else dict(temperature=self.temperature)))
            stage.rows(self._logits[:R], self.block, self.post.view(-1, 16), draw=draw, **where)
        elif self.request_temperature:   # the fused draw at each slot's own invT; a greedy slot takes the plain argmax
            ops.gemm_sample_batch(lm, s["xn"], R, t.V, H, 0, 16, self.gws, self.post.view(-1, 16), 0, dyn_t,
                                  seeds=self.seeds, inv_ts=self.inv_ts, pos_word=ops.DYN_POS0, pos_add=1,
                                  tiles_per_req=TPR, nrows_dyn_word=ops.DYN_BS, logits=lg)
        elif self.temperature < 1e-5:
            ops.gemm_argmax_batch(lm, s["xn"], R, t.V, H, 0, 16, self.gws, self.post.view(-1, 16), 0, dyn_t,
                                  nrows_dyn_word=ops.DYN_BS, logits=lg)
        elif self.sampler == "device":   # the seeded draw in the lm_head epilogue: tile j row m -> start + 16 j + m + 1
            ops.gemm_sample_batch(lm, s["xn"], R, t.V, H, 0, 16, self.gws, self.post.view(-1, 16), 0, dyn_t,
                                  seeds=self.seeds, temperature=self.temperature, pos_word=ops.DYN_POS0, pos_add=1,
                                  tiles_per_req=TPR, nrows_dyn_word=ops.DYN_BS, logits=lg)
        else:
            # T > 0 (model/utils.py:30-34): the same GEMM materialises the bf16 logits and the
            # reference's own softmax + torch.multinomial draws the posterior (caller's RNG stream;
            # one draw over all requests' rows, so the stream differs from R sequential runs)
            if self._logits is None:
                self._logits = torch.zeros(MT, 16, t.V, dtype=BF16, device=self.dev)
            ops.gemm_argmax_batch(lm, s["xn"], R, t.V, H, 0, 16, self.gws, self.post, 0, dyn_t,
                                  nrows_dyn_word=ops.DYN_BS, logits=self._logits)
            self.post[:R] = sample(self._logits[:R], self.temperature)
        if self.lp is not None:   # behind whichever branch wrote the posterior, before the accept launch moves POS0
            stage.logprobs(self._logits[:R], self.post.view(-1, 16), **where)

    def _accept_launch(self) -> None:
        if self.sq is not None:   # every slot's stop sequences over what the accept launch is about to commit
            ops.stop_seq_rows(self.block, self.post, self.output_ids, self.dyn_d, self.sq, slots=self.R)
        ops.accept_commit_batch(self.block, self.post, self.R, self.output_ids, self.dyn_d, self.dyn_t, self.stop_t,
                                self.result, rearm_mask_id=self.mask_id, tiles_per_req=self.TPR,
                                dyn_d_tiles=self.dyn_dt, dyn_t_tiles=self.dyn_tt)
        if self.stage is not None:
            self.stage.commit(self.output_ids, self.dyn_d, self.R)

    def accept(self, launch: bool = True) -> list:
        """Acceptance scan + commit + rollback bookkeeping of all requests (:258-268) and
        the cycle's one device->host read.  Returns per request (tau, stop) or None."""
        if launch:
            self._accept_launch()
        res = self.result[:self.R].tolist()
        out = []
        for r in range(self.R):
            if not self.live[r]:
                out.append(None)
                continue
            self.start[r] = res[r][1]
            out.append((res[r][0] + 1, bool(res[r][2])))
        return out

    # ------------------------------------------------------------------ hipGraph
    @torch.inference_mode()
    def capture(self) -> None:
        """Capture the cycle's launch sequence (~300 kernels) into three hipGraphs: draft body,
        lm_head + unmask, verify + accept.  Every length the kernels need is read from `dyn`
        on the device, so one capture serves every cycle; the key-split count of the attention
        launches is fixed at the cache capacity (splits past a request's keys are empty).
        The host then spends three graph launches per cycle instead of ~300 ctypes calls."""
        kv = self.max_rows
        self.model._rope_tab(kv + 64)
        self.target._rope_tab(kv + 64)
        torch.cuda.synchronize(self.dev)
        self.graphs = {}
        for name, fn in (("body", lambda: self._draft_body(kv)), ("head", self._draft_head),
                         ("verify", lambda: (self.verify(kv), self._accept_launch()))):
            self.graphs[name] = capture_graph(fn)   # (not torch.cuda.graph(): its empty_cache(), see generate.capture_graph)

    @torch.inference_mode()
    def cycle_graph(self, draft_token_hook: Optional[Callable] = None) -> list:
        """`cycle` through the captured graphs (call `capture()` once after the first eager
        cycle).  Note the capture itself replays nothing: state only advances here."""
        g = self.graphs
        self._mark("draft", 0)
        g["body"].replay()
        self._mark("lm_head", 0)
        g["head"].replay()
        self._mark("lm_head", 1)
        self._mark("draft", 1)
        if draft_token_hook is not None:
            for r in range(self.R):
                if self.live[r]:
                    draft_token_hook(r, self.block[r:r + 1], self.start[r], self.hook_calls[r])
                    self.hook_calls[r] += 1
        self._mark("target", 0)
        g["verify"].replay()
        self._mark("target", 1)
        return self.accept(launch=False)

    @torch.inference_mode()
    def cycle(self, draft_token_hook: Optional[Callable] = None, after_draft: Optional[Callable] = None,
              ahead_ok: bool = False) -> list:
        """One decode cycle of every live request.  draft_token_hook(r, block_row, start,
        call): test/bench instrumentation for scripted acceptance, as in DecodeSession.
        ahead_ok: the caller promises that the NEXT cycle runs with the same block sizes and the same live requests
        (no tail clamp, no request ending on this cycle's result): its draft forward — every length it needs is in the
        device records the accept kernel writes — is then enqueued behind this cycle's accept kernel, before the host
        reads the result, and the GPU does not idle through the host's turnaround."""
        if self._ahead:
            self._ahead = False
            if self.events is not None and self._ahead_ev:
                e = self._ahead_ev
                self.events["draft"], self.events["lm_head"] = [e[0], e[1]], [e[2], e[3]]
        else:
            self._mark("draft", 0)
            self.draft()
            self._mark("draft", 1)
        if after_draft is not None:
            after_draft()
        if draft_token_hook is not None:
            for r in range(self.R):
                if self.live[r]:
                    draft_token_hook(r, self.block[r:r + 1], self.start[r], self.hook_calls[r])
                    self.hook_calls[r] += 1
        self._mark("target", 0)
        self.verify()
        self._mark("target", 1)
        if not (ahead_ok and self.run_ahead):
            return self.accept()
        self._accept_launch()
        ev = None
        if self.events is not None:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
        self._draft_body(self._kv_len_max() + self.BW)   # (the new starts are at most a block further)
        if ev:
            ev[2].record()
        self._draft_head()
        if ev:
            ev[3].record()
            ev[1].record()
        self._ahead, self._ahead_ev = True, ev
        return self.accept(launch=False)


def _prompt_seeds(sampler: str, seed, n: int, sampling: bool) -> list:
    """One seed per prompt: an int s gives prompt i the seed s + i; a sequence gives its own; None draws them."""
    resolve_seed(sampler, None, needed=False)
    if sampler != "device" or not sampling:
        if seed is not None and sampler != "device":
            raise ValueError("seed needs sampler='device' (sampler='torch' draws on the caller's torch RNG)")
        return [None] * n
    if seed is None:
        return [resolve_seed("device", None) for _ in range(n)]
    if isinstance(seed, int):
        return [seed + i for i in range(n)]
    seeds = [int(x) for x in seed]
    if len(seeds) != n:
        raise ValueError("one seed per prompt")
    return seeds


def _prompt_temperatures(temperature, n: int, sampler: str):
    """(temperature per prompt, whether the prompts need a decoder built with request_temperature=True) from one float or
    one value per prompt.  A scalar or equal values run the single-temperature path; values that differ need
    sampler='device'."""
    if isinstance(temperature, (int, float)):
        return [float(temperature)] * n, False
    ts = [float(t) for t in temperature]
    if len(ts) != n:
        raise ValueError("temperature: one float or one value per prompt")
    mixed = any(t != ts[0] for t in ts)
    if mixed and sampler != "device":
        raise ValueError("per-prompt temperatures that differ need sampler='device'")
    return ts, mixed


def _prompt_filters(top_k, top_p, n: int, temperature, sampler: str):
    """(top_k per prompt, top_p per prompt, whether any prompt filters a sampled draw) from scalars or sequences;
    temperature: one float, or the list _prompt_temperatures returns."""
    ks = [top_k] * n if isinstance(top_k, int) else list(top_k)
    ps = [top_p] * n if isinstance(top_p, (int, float)) else list(top_p)
    if len(ks) != n or len(ps) != n:
        raise ValueError("top_k / top_p: a scalar or one value per prompt")
    on = [ops.check_filter(k, p) for k, p in zip(ks, ps)]
    ts = [temperature] * n if isinstance(temperature, (int, float)) else list(temperature)
    filtering = any(o and t >= 1e-5 for o, t in zip(on, ts))
    if filtering and sampler != "device":
        raise ValueError("top_k / top_p at T > 0 need sampler='device' (sampler='torch' is the reference's unfiltered "
                         "multinomial)")
    return [int(k) for k in ks], [float(p) for p in ps], filtering


def _prompt_min_p(min_p, n: int, temperature, sampler: str):
    """(min_p per prompt: a float in (0, 1] or None, whether any prompt floors a sampled draw) from None, a scalar or one
    value (or None) per prompt; temperature: one float, or the list _prompt_temperatures returns."""
    if min_p is None or isinstance(min_p, (bool, int, float)) or not hasattr(min_p, "__len__"):
        mps = [min_p] * n
    else:
        mps = list(min_p)
        if len(mps) != n:
            raise ValueError("min_p: a scalar or one value per prompt")
    mps = [ops.check_min_p(v) for v in mps]
    ts = [temperature] * n if isinstance(temperature, (int, float)) else list(temperature)
    on = any(v is not None and t >= 1e-5 for v, t in zip(mps, ts))
    if on and sampler != "device":
        raise ValueError("min_p at T > 0 needs sampler='device' (sampler='torch' is the reference's multinomial over the "
                         "raw logits)")
    return mps, on


def _prompt_stop_sequences(stop_sequences, n: int, target, mask_token_id: int) -> list:
    """The stop sequences per prompt (ops.check_stop_sequences: a list of lists of ints, or None) from None, one list of
    sequences for every prompt, or a list of n entries each of which is None or a list of SEQUENCES (its first element
    is itself a list / tuple / tensor).  A flat list of n lists of ids is therefore one list for every prompt.  target.V
    is read only where sequences are given."""
    def is_seq(v):
        return isinstance(v, (list, tuple)) or (torch.is_tensor(v) and v.dim() >= 1)

    if stop_sequences is None:
        return [None] * n
    vals, V = list(stop_sequences), target.V
    per_prompt = len(vals) == n and any(v is None or (is_seq(v) and len(v) > 0 and is_seq(v[0])) for v in vals) \
        and all(v is None or is_seq(v) for v in vals)
    if not per_prompt:
        vals = [vals] * n
    return [ops.check_stop_sequences(v, V, mask_token_id) for v in vals]


def _prompt_penalties(repetition_penalty, presence_penalty, frequency_penalty, n: int):
    """((r, a, f) per prompt, whether any prompt is not neutral) from scalars or one value per prompt."""
    cols = []
    for v in (repetition_penalty, presence_penalty, frequency_penalty):
        col = [float(v)] * n if isinstance(v, (int, float)) else [float(x) for x in v]
        if len(col) != n:
            raise ValueError("repetition_penalty / presence_penalty / frequency_penalty: a scalar or one value per prompt")
        cols.append(col)
    pens = list(zip(*cols))
    return pens, any(ops.check_penalties(*p) is not None for p in pens)


def _prompt_bias(target, logit_bias, allowed_token_ids, banned_token_ids, min_tokens, n: int, stop_token_ids):
    """(the four keywords per prompt as dicts, whether any prompt is not neutral; target.V is read only for a prompt whose
    keywords are given).  logit_bias: None or one mapping for every prompt, or a sequence of n (mapping or None).
    allowed_token_ids / banned_token_ids: None or one sequence of ids for every prompt, or a sequence of n (sequence of
    ids or None).  min_tokens: an int, or one per prompt."""
    from collections.abc import Mapping

    def is_id(v):
        return isinstance(v, int) or (torch.is_tensor(v) and v.dim() == 0) or (hasattr(v, "__index__")
                                                                             and not hasattr(v, "__len__"))

    def per_prompt(v, one, name):
        if one(v):
            return [v] * n
        v = list(v)
        if len(v) != n:
            raise ValueError(f"{name}: one value, or one per prompt")
        return v

    lbs = per_prompt(logit_bias, lambda v: v is None or isinstance(v, Mapping), "logit_bias")
    ids_one = lambda v: v is None or all(is_id(x) for x in v)  # noqa: E731
    als = per_prompt(allowed_token_ids, ids_one, "allowed_token_ids")
    bns = per_prompt(banned_token_ids, ids_one, "banned_token_ids")
    mts = per_prompt(min_tokens, lambda v: not hasattr(v, "__len__"), "min_tokens")
    kws = [dict(logit_bias=lbs[i], allowed_token_ids=als[i], banned_token_ids=bns[i], min_tokens=mts[i]) for i in range(n)]
    on = False
    for kw in kws:
        if not (kw["logit_bias"] is None and kw["allowed_token_ids"] is None and kw["banned_token_ids"] is None
                and kw["min_tokens"] == 0):
            on = ops.check_logit_bias(target.V, stop_token_ids=stop_token_ids, **kw) is not None or on
    return kws, on


def _prompt_grammars(grammar, n: int) -> list:
    """One TokenDFA (or None) per prompt: None or one TokenDFA for every prompt, or a sequence of n (TokenDFA or None)."""
    if grammar is None or hasattr(grammar, "next") or hasattr(grammar, "char_next"):
        return [grammar] * n
    g = list(grammar)
    if len(g) != n:
        raise ValueError("grammar: one TokenDFA, or one per prompt")
    return g


def _load_grammars(dec, dfas) -> list:
    """The handles of `dfas` (TokenDFA or None each) in decoder / engine `dec`, every distinct automaton loaded once."""
    seen, out = {}, []
    for d in dfas:
        if d is not None and id(d) not in seen:
            seen[id(d)] = dec.add_grammar(d)
        out.append(None if d is None else seen[id(d)])
    return out


def _pool_rows(dfas) -> int:
    """The pool rows the distinct (validated) automata among `dfas` need (0: none given)."""
    return sum(int(d.num_states) for d in {id(d): d for d in dfas if d is not None}.values())


@torch.inference_mode()
def dflash_generate_batch(model: DFlashDraftModel, target: NativeTarget, input_ids: Sequence[torch.Tensor],
                          mask_token_id: int, max_new_tokens: int, block_size: int, stop_token_ids,
                          temperature=0.0, draft_token_hook: Optional[Callable] = None,
                          group_size: int = MAX_GROUP, hook_block_view: bool = False, sampler: str = "torch",
                          seed=None, top_k=0, top_p=1.0, logprobs: Optional[int] = None, repetition_penalty=1.0,
                          presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None, allowed_token_ids=None,
                          banned_token_ids=None, min_tokens=0, grammar=None, constrain_draft: bool = False,
                          min_p=None, couple_draft: bool = False, stop_sequences=None,
                          include_stop_sequence: bool = True) -> list:
    """`dflash_generate` (benchmark.py:44-251) for a list of prompts: requests run in
    groups of `group_size` <= 4 (<= 2 with block sizes of 17..32 rows) that share the weight stream; returns one namespace per
    prompt with the fields of benchmark.py:242-251 (timing fields are the group's).
    draft_token_hook(request_index, block, start, call).
    sampler="device": seeded draws on the device; seed is an int s (prompt i gets s + i), one seed
    per prompt, or None (one per prompt from torch's RNG).  Request i then emits what dflash_generate(..., seed=its seed)
    emits, however the group is formed.
    top_k / top_p: a scalar, or one value per prompt (0 / 1.0: off), as in dflash_generate.
    temperature: one float, or one value per prompt; values that differ need sampler="device" and run every group through
    a decoder built with request_temperature=True ("Per-request temperature").
    logprobs: as dflash_generate, for every prompt (the fields logprobs / top_logprob_ids / top_logprobs; None when off).
    repetition_penalty / presence_penalty / frequency_penalty: as dflash_generate; a scalar, or one value per prompt.
    The decoders are built with penalties=True when any prompt is not neutral (blocks of <= 16 rows).
    logit_bias / allowed_token_ids / banned_token_ids / min_tokens: as dflash_generate; one value for every prompt, or a
    sequence with one value (or None) per prompt.  The decoders are built with logit_bias=True when any prompt is not
    neutral (blocks of <= 16 rows).
    grammar: as dflash_generate; one TokenDFA for every prompt, or a sequence with one (or None) per prompt.  Each group's
    decoder gets a pool of exactly its prompts' automata (blocks of <= 16 rows); the results carry `grammar_state`.
    constrain_draft: as dflash_generate (ValueError when no prompt has a grammar or a not-neutral logit-bias keyword); a
    prompt without a grammar and without bans keeps its argmax draft.
    min_p: as dflash_generate; a scalar, or one value (or None) per prompt.  The decoders are built with min_p=True when
    any prompt floors a sampled draw (blocks of up to 32 rows); a prompt at 0 gets the ids of a run without it.
    couple_draft: as dflash_generate, for every prompt at its own temperature (a prompt at 0 keeps its greedy draft).
    stop_sequences / include_stop_sequence: as dflash_generate; one list of sequences for every prompt, or a list with one
    list (or None) per prompt.  The decoders are built with stop_sequences=True when any prompt carries one; the
    results carry `stop_sequence`."""
    stops = _prompt_stop_sequences(stop_sequences, len(input_ids), target, mask_token_id)
    stops_on = any(s is not None for s in stops)
    logprobs = ops.check_logprobs(logprobs)
    dfas = _prompt_grammars(grammar, len(input_ids))
    for d in {id(d): d for d in dfas if d is not None}.values():
        ops.check_grammar(d, target.V)
    if _pool_rows(dfas) and block_size > 16:
        raise NotImplementedError("grammar takes blocks of <= 16 rows")
    pens, penalties = _prompt_penalties(repetition_penalty, presence_penalty, frequency_penalty, len(input_ids))
    biases, logit_bias_on = _prompt_bias(target, logit_bias, allowed_token_ids, banned_token_ids, min_tokens,
                                         len(input_ids), stop_token_ids)
    if constrain_draft and not (_pool_rows(dfas) or logit_bias_on):
        raise ValueError("constrain_draft needs something to constrain by: a grammar, allowed_token_ids, banned_token_ids "
                         "or a logit_bias")
    if constrain_draft and block_size > 16:
        raise NotImplementedError("constrain_draft takes blocks of <= 16 rows")
    temps, per_request = _prompt_temperatures(temperature, len(input_ids), sampler)
    seeds = _prompt_seeds(sampler, seed, len(input_ids), any(t >= 1e-5 for t in temps))
    top_ks, top_ps, filtering = _prompt_filters(top_k, top_p, len(input_ids), temps, sampler)
    min_ps, min_p_on = _prompt_min_p(min_p, len(input_ids), temps, sampler)
    if not 1 <= block_size <= 32:
        raise NotImplementedError("the batched loop takes blocks of 1..16 rows (one tile per request) or 17..32 rows (two)")
    if penalties and block_size > 16:
        raise NotImplementedError("penalties take blocks of <= 16 rows")
    if logit_bias_on and block_size > 16:
        raise NotImplementedError("logit_bias / allowed_token_ids / banned_token_ids / min_tokens take blocks of <= 16 rows")
    tpr = 1 if block_size <= 16 else 2      # blocks of 17..32 rows: a request takes two of the group's four tiles
    group_size = min(group_size, MAX_GROUP // tpr)
    n = len(input_ids)
    results = [None] * n
    for g0 in range(0, n, group_size):
        idx = list(range(g0, min(n, g0 + group_size)))
        prompts = [input_ids[i] for i in idx]
        pmax = max(p.shape[1] for p in prompts)
        max_len = [p.shape[1] + max_new_tokens for p in prompts]
        dec = BatchedDecoder(model, target, len(idx), max_rows=pmax + max_new_tokens + 3 * 16 * tpr,
                             out_len=pmax + max_new_tokens + 16 * tpr, mask_token_id=mask_token_id,
                             stop_token_ids=stop_token_ids, temperature=max(temps[i] for i in idx), tiles_per_request=tpr,
                             sampler=sampler, filtering=filtering, request_temperature=per_request, logprobs=logprobs,
                             penalties=penalties, logit_bias=logit_bias_on, min_p=min_p_on,
                             grammar_states=_pool_rows([dfas[i] for i in idx]),
                             # (a group none of whose prompts has anything to constrain by runs the plain launches)
                             constrain_draft=bool(constrain_draft) and bool(logit_bias_on or _pool_rows([dfas[i] for i in idx])),
                             couple_draft=couple_draft, stop_sequences=stops_on)
        handles = _load_grammars(dec, [dfas[i] for i in idx])
        t0 = cuda_time()
        for r, p in enumerate(prompts):
            pr, pa, pf = pens[idx[r]]
            dec.admit(r, p, temps[idx[r]], seed=seeds[idx[r]], top_k=top_ks[idx[r]], top_p=top_ps[idx[r]],
                      repetition_penalty=pr, presence_penalty=pa, frequency_penalty=pf, **biases[idx[r]],
                      grammar=handles[r], min_p=min_ps[idx[r]] if min_p_on else None, stop_sequences=stops[idx[r]])
        ttft = cuda_time() - t0
        taus = [[] for _ in idx]
        # (hook_block_view: the hook sees the block as the single-request loop hands it over, bs slots; default: the
        # request's whole 16- / 32-slot row)
        hook = ((lambda r, blk, start, call: draft_token_hook(idx[r], blk[:, :max(1, dec.bs[r])] if hook_block_view else blk,
                                                              start, call)) if draft_token_hook else None)
        t1 = cuda_time()
        clock = [t1]
        first = True
        stop_always = stop_token_ids is not None and mask_token_id in stop_token_ids
        for r in range(len(idx)):   # nothing to generate
            if dec.start[r] >= max_len[r]:
                dec.park(r)
        while any(dec.live):
            for r in range(len(idx)):  # tail clamp (benchmark.py:104-105)
                if dec.live[r]:
                    dec.set_block_size(r, max(1, min(block_size, max_len[r] - dec.start[r])))
            # run-ahead draft: only while no live request can finish or hit its tail clamp on this cycle's result
            ahead = (stop_token_ids is None and not stops_on and not stop_always
                     and all(dec.start[r] + 2 * block_size <= max_len[r] for r in range(len(idx)) if dec.live[r]))
            if first:   # the clock restarts after the first draft, before its verify (benchmark.py:145-147)
                first = False
                out = dec.cycle(hook, after_draft=lambda: clock.__setitem__(0, cuda_time()), ahead_ok=ahead)
                t1 = clock[0]
            else:
                out = dec.cycle(hook, ahead_ok=ahead)
            for r, o in enumerate(out):
                if o is None:
                    continue
                taus[r].append(o[0])
                if o[1] or stop_always or dec.start[r] >= max_len[r]:
                    dec.park(r)
        decode_s = cuda_time() - t1
        for r, i in enumerate(idx):
            hit, which = dec.stop_hit(r, include_stop_sequence), []
            ids = _trim(dec.output_ids[r:r + 1], max_len[r], mask_token_id, stop_token_ids, dec.n_in[r], hit)
            n_out = ids.shape[1] - dec.n_in[r]
            cols = _kept_cols(dec.output_ids[r:r + 1], max_len[r], mask_token_id, stop_token_ids, dec.n_in[r], hit, which)
            lpf = NO_LOGPROBS if dec.lp is None else logprob_fields(dec.lp, r, cols[dec.n_in[r]:])
            results[i] = SimpleNamespace(output_ids=ids.clone(), num_input_tokens=dec.n_in[r], num_output_tokens=n_out,
                                         time_to_first_token=ttft, time_per_output_token=decode_s / max(1, n_out),
                                         acceptance_lengths=taus[r], cycle_trace=[], profile_summary=None,
                                         grammar_state=dec.grammar_state_of(r, ids[0], dec.n_in[r]),
                                         stop_sequence=which[0] if which else None, **lpf)
        del dec
    return results


@torch.inference_mode()
def dflash_generate_policy_batch(*, model: DFlashDraftModel, target: NativeTarget, input_ids: Sequence[torch.Tensor],
                                 mask_token_id: int, max_new_tokens: int, stop_token_ids, temperature: float,
                                 schedulers: Sequence, draft_token_hook: Optional[Callable] = None,
                                 group_size: int = MAX_GROUP, sampler: str = "torch", seed=None, stop_sequences=None,
                                 include_stop_sequence: bool = True) -> list:
    """`dflash_generate_policy` (benchmark_dynamic_schedule.py:260-434) for a list of prompts, the requests of a group
    sharing the weight stream: every request has its OWN scheduler (schedulers[i], e.g. an EWMAPerformanceScheduler) and
    therefore its own block size per cycle — the kernels read each request's size from its length record, so a group
    may mix 8-, 12- and 16-row blocks in one pass over the weights.  Returns one namespace per prompt with the fields of
    :425-434.  The cycle time a scheduler is fed is the GROUP's cycle wall time (what its request actually waited).
    Block sizes <= 16 (one tile per request); T = 0 (the reference samples the draft with T too, :342 — a per-request
    RNG stream over a shared launch has no counterpart in it): both raise NotImplementedError otherwise — except with
    sampler="device" (seed as in dflash_generate_batch), whose per-request seeded draws of target AND draft are what
    dflash_generate_policy(..., sampler="device") draws for that request.
    stop_sequences / include_stop_sequence: as dflash_generate_batch (the field `stop_sequence`)."""
    stops = _prompt_stop_sequences(stop_sequences, len(input_ids), target, mask_token_id)
    stops_on = any(s is not None for s in stops)
    if temperature >= 1e-5 and sampler != "device":
        raise NotImplementedError("the batched policy loop samples at T > 0 with sampler='device' only; or run the requests "
                                  "through dflash_generate_policy")
    seeds = _prompt_seeds(sampler, seed, len(input_ids), temperature >= 1e-5)
    T = temperature if sampler == "device" else 0.0
    n = len(input_ids)
    if len(schedulers) != n:
        raise ValueError("one scheduler per prompt")
    for sc in schedulers:
        if max(sc.candidates) > 16:
            raise NotImplementedError("the batched kernels take blocks of at most 16 rows")
    results = [None] * n
    stop_t = None
    for g0 in range(0, n, group_size):
        idx = list(range(g0, min(n, g0 + group_size)))
        prompts = [input_ids[i] for i in idx]
        scheds = [schedulers[i] for i in idx]
        pmax = max(p.shape[1] for p in prompts)
        max_len = [p.shape[1] + max_new_tokens for p in prompts]
        dec = BatchedDecoder(model, target, len(idx), max_rows=pmax + max_new_tokens + 3 * 16,
                             out_len=pmax + max_new_tokens + 16, mask_token_id=mask_token_id,
                             stop_token_ids=stop_token_ids, temperature=T, sampler=sampler, draft_temperature=T,
                             stop_sequences=stops_on)
        stop_t = dec.stop_t
        t0 = cuda_time()
        for r, p in enumerate(prompts):
            dec.admit(r, p, T, seed=seeds[idx[r]], stop_sequences=stops[idx[r]])
        ttft = cuda_time() - t0
        R = len(idx)
        taus, used, traces, cyc = [[] for _ in idx], [[] for _ in idx], [[] for _ in idx], [0] * R
        hook = (lambda r, blk, start, call: draft_token_hook(idx[r], blk, start, call)) if draft_token_hook else None
        stop_always = stop_token_ids is not None and mask_token_id in stop_token_ids
        for r in range(R):
            if dec.start[r] >= max_len[r]:
                dec.park(r)
        t1 = cuda_time()
        clock = [t1]
        first = True
        while any(dec.live):
            chosen, bs, lgen, start_idx = [0] * R, [0] * R, [0.0] * R, list(dec.start)
            for r in range(R):
                if dec.live[r]:
                    chosen[r] = scheds[r].select(cyc[r])
                    bs[r] = max(1, min(chosen[r], max_len[r] - dec.start[r]))
                    dec.set_block_size(r, bs[r])
                    lgen[r] = float(bs[r])

            def after_draft(first_now=first):
                # EOS-aware generated length (benchmark_dynamic_schedule.py:344-349)
                if stop_t is not None:
                    for r in range(R):
                        if dec.live[r] and bs[r] > 1:
                            pos = torch.isin(dec.block[r, 1:bs[r]], stop_t).nonzero(as_tuple=True)[0]
                            if pos.numel() > 0:
                                lgen[r] = float(min(int(pos[0].item()) + 1, bs[r]))
                if first_now:   # the TPOT clock restarts after the first draft (benchmark_dynamic_schedule.py:352-354)
                    clock[0] = cuda_time()

            c0 = cuda_time()
            out = dec.cycle(hook, after_draft=after_draft)
            cycle_s = cuda_time() - c0
            if first:
                first, t1 = False, clock[0]
            for r, o in enumerate(out):
                if o is None:
                    continue
                sc = scheds[r]
                tau = o[0]
                taus[r].append(tau)
                used[r].append(bs[r])
                sc.update(tau=tau, cycle_s=cycle_s, effective_bs=bs[r], cycle_idx=cyc[r], l_gen=lgen[r])
                traces[r].append({
                    "cycle_idx": cyc[r], "start_idx": int(start_idx[r]), "block_size": int(bs[r]),
                    "chosen_block_size": int(chosen[r]), "tau": int(tau), "l_gen": float(lgen[r]),
                    "acceptance_ratio": float(tau / max(1, bs[r])), "cycle_s": float(cycle_s),
                    "tau_hat": sc.tau_hat.get(bs[r]), "cycle_hat": sc.cycle_hat.get(bs[r]),
                    "score_hat": sc.score_hat.get(bs[r]), "current_block_size": int(sc.current),
                    "adl_lgen_hat": sc.adl_lgen_hat, "adl_lacc_hat": sc.adl_lacc_hat,
                    "adl_target_k": int(sc.adl_target_k), "adl_target_bs": int(sc.adl_target_bs)})
                cyc[r] += 1
                if o[1] or stop_always or dec.start[r] >= max_len[r]:
                    dec.park(r)
        decode_s = cuda_time() - t1
        for r, i in enumerate(idx):
            hit, which = dec.stop_hit(r, include_stop_sequence), []
            ids = dec.output_ids[r:r + 1][:, _kept_cols(dec.output_ids[r:r + 1], max_len[r], mask_token_id, stop_token_ids,
                                                        dec.n_in[r], hit, which)]
            n_out = ids.shape[1] - dec.n_in[r]
            results[i] = SimpleNamespace(output_ids=ids.clone(), num_input_tokens=dec.n_in[r], num_output_tokens=n_out,
                                         time_to_first_token=ttft, time_per_output_token=decode_s / max(1, n_out),
                                         acceptance_lengths=taus[r], used_block_sizes=used[r], cycle_trace=traces[r],
                                         stop_sequence=which[0] if which else None)
        del dec
    return results
