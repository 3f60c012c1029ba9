"""`LogitsStage` — everything between the verify's lm_head launch and its posterior ids, in ONE place: the row processors
of DESIGN.md sections 8 and 12 - 15 and 18, their state, their buffers and their order.  A `DecodeSession` holds one for
its single request (slot 0), a `BatchedDecoder` one for its request slots; `NativeTarget.verify`, `_verify_wide` and
`BatchedDecoder.verify` hand it the raw rows their head launch materialised.  Nothing enabled: no stage (None), nothing
enqueued, nothing allocated.

The order, and what each step reads (every step is one launch over all rows handed in; row m of a block predicts position
POS0 + m + 1):

  head launch     materialises the raw rows (the caller's; `raw` is where, unless the caller has a buffer of its own)
  logit bias      raw rows + the slot's bias row; stop ids -> -inf while the position is < min_pos          (section 14)
  grammar         those rows, masked by the state the slot's state reaches over block[1 .. m]; the state is read (15)
  penalties       those rows, by the slot's table row plus the block's own block[1 .. m]                         (13)
                  — each of the three writes a buffer of its own and the rows' argmax into the posterior: what a greedy
                  slot keeps.  Masking commutes with both neighbours: neither turns -inf finite
  min_p           sampling only, directly in front of the draw: columns below min_p x the top probability -> -inf  (18)
  draw            sampling only: dfl_sample_rows_nucleus over the last of those rows, at the slot's seed / top_k /
                  top_p (0 / 1.0: the plain seeded draw, the ids of the fused epilogue)          (8, "Filtered draw")
  logprobs        log_softmax of the RAW rows at the posterior ids, T = 1, unfiltered, whatever drew the token    (12)
  — behind the accept launch (`commit`): penalty_count, then grammar_advance, over output_ids(S, START] of the record.

The first token (`admit`) takes the same steps on the prompt's last-row logits, which predict position P: bias, grammar
(start state, no walk), clear the table row and count the prompt, penalise, min_p, draw or argmax, count the token,
advance the state, logprobs of the raw row.

What is enabled is fixed at construction: it fixes the launch sequence a hipGraph captures, and every buffer a captured
launch reads keeps its address for the stage's life (a buffer is made on first use, which is always an eager cycle).
Per-slot values are host values in a session's stage (`device_values=False`: one request, written once) and device
arrays read by address in a decoder's (rewritten on every admission, neutral where the request has none).
`check_features` holds the refusals every entry point shares."""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import torch

from . import ops
from .utils import sample

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32

# feature -> (how the refusals name it, the verb's plural form, the flag a decoder / engine is built with)
FEATURES = dict(min_p=("min_p", False, "min_p=True"),
                grammar=("grammar", False, "grammar_states > 0"),
                logit_bias=("logit_bias / allowed_token_ids / banned_token_ids / min_tokens", True, "logit_bias=True"),
                penalties=("penalties", True, "penalties=True"),
                filter=("top_k / top_p", True, "filtering=True (and sampler='device')"),
                logprobs=("logprobs", False, "logprobs=N"))
NARROW = ("grammar", "logit_bias", "penalties")   # the processors that read block[1 .. m]: one 16-row tile per request


def check_features(on, *, where: str = "", native: bool = True, sampling: bool = False, seeded: bool = True,
                   wide: bool = False, built: Optional[dict] = None, owner: str = "decoder") -> None:
    """The refusals of the features in `on` (keys of FEATURES), before anything touches the GPU.  built: feature -> whether
    the `owner` (a decoder or an engine) was built with it (a request's features only); native: the target is a
    NativeTarget; sampling: the draw is at T > 0, seeded: by the device sampler (sampler='device' / seed=...); wide:
    blocks of 17..32 rows."""
    for f, (name, plural, flag) in FEATURES.items():
        if f not in on:
            continue
        s = "" if plural else "s"
        if built is not None and not built.get(f, True):
            raise ValueError(f"{where}{name} need{s} {'an' if owner[0] in 'aeiou' else 'a'} {owner} built with {flag}")
        if not native and f != "filter":
            raise ValueError(f"{where}{name} need{s} a dflash_amd.NativeTarget (the kernel reads the verify's materialised "
                             f"logits)")
        if sampling and not seeded and f != "logprobs":
            raise ValueError(f"{where}{name} at T > 0 need{s} the seeded draw (sampler='device', seed=...): "
                             f"sampler='torch' is the reference's multinomial over the raw logits")
        if wide and f in NARROW:
            raise NotImplementedError(f"{where}{name} take{s} blocks of <= 16 rows (the 17..32-row verify is not covered)")


def draw_rows(logits: torch.Tensor, temperature: float, seed: int, pos0: int, flt: Optional[dict] = None) -> torch.Tensor:
    """The device sampler over materialised logits [1, T, V]: row j draws position pos0 + j (stream TARGET); flt: the
    top_k / top_p of the filtered draw, one launch per 16-row tile."""
    _, t, v = logits.shape
    rows = logits.reshape(t, v)
    if flt is None:
        return ops.sample_rows(rows, seed=seed, temperature=temperature, pos0=pos0).view(1, t)
    out = torch.empty(t, dtype=torch.long, device=logits.device)
    for r0 in range(0, t, 16):
        ops.sample_rows_nucleus(rows[r0:r0 + 16], seed=seed, temperature=temperature, pos_base=pos0 + r0, out=out[r0:r0 + 16],
                                **flt)
    return out.view(1, t)


class LogitsStage:
    def __init__(self, slots: int, V: int, device, *, tiles: int = 1, device_values: bool = False, out_len: int = 0,
                 logprobs: Optional[int] = None, penalties: bool = False, logit_bias: bool = False,
                 grammar_states: int = 0, min_p: bool = False, filtering: bool = False, sampling: bool = False,
                 stop_ids: Optional[torch.Tensor] = None):
        """slots request slots, `tiles` 16-row tiles in all.  sampling: the owner draws at T > 0 (a greedy owner enqueues
        neither min_p nor a draw; min_p then only keeps the slots' values).  stop_ids: the accept launch's list, which
        the logit bias suppresses under min_tokens."""
        self.slots, self.V, self.device, self.tiles, self.device_values = slots, V, device, tiles, device_values
        self._bufs, self._on = {}, None
        self.stop = stop_ids
        self.lp = ops.logprob_sink(slots, out_len, logprobs, device) if logprobs is not None else None
        # penalties: one table row per slot (bit 31: seen in the prompt, bits 0..30: occurrences in the output) and the
        # three values
        self.pen_table = ops.penalty_state(slots, V, device) if penalties else None
        self.pen = [1.0, 0.0, 0.0]
        if penalties and device_values:
            self.pen = [torch.ones(slots, dtype=F32, device=device), torch.zeros(slots, dtype=F32, device=device),
                        torch.zeros(slots, dtype=F32, device=device)]
        # logit bias: one dense fp32 row and one min_pos per slot, rewritten whole on every admission
        self.lb = ops.logit_bias_state(slots, V, device) if logit_bias else None
        # grammar: the pool (its storage never moves: one capture serves every grammar loaded later), base / state per slot
        self.gr = ops.grammar_state(slots, grammar_states, V, device) if grammar_states else None
        # min_p: the host value, or one fp32 ln(min_p) per slot (-inf: off); min_p_on: the launch is enqueued at all
        self.min_p, self.min_p_on = bool(min_p), bool(min_p) and sampling
        self.mp = None
        if self.min_p and device_values:
            self.mp = torch.full((slots,), float("-inf"), dtype=F32, device=device)
        # the draw's filter: host values, or one top_k / top_p per slot (0 / 1.0: that slot's plain draw)
        self.filtering = bool(filtering) and sampling
        self.top_k, self.top_p = 0, 1.0
        if device_values:
            self.top_k, self.top_p = torch.zeros(slots, dtype=I32, device=device), torch.ones(slots, dtype=F32, device=device)

    @classmethod
    def of_keywords(cls, V: int, temperature: float, *, top_k=0, top_p=1.0, logprobs=None, penalties=None, logit_bias=None,
                    grammar=None, min_p=None) -> Optional["LogitsStage"]:
        """The stage of a NativeTarget.verify called with the keywords instead: logprobs an ops.logprob_sink; penalties
        (.table, .r, .a, .f), logit_bias (an ops.logit_bias_state with .stop) and grammar (an ops.grammar_state) the
        state objects a caller keeps itself.  None when nothing is asked.  Values are validated, nothing is allocated."""
        mp = ops.check_min_p(min_p) if temperature >= 1e-5 else (ops.check_min_p(min_p) and None)
        flt = ops.check_filter(top_k, top_p) and temperature >= 1e-5
        if not flt and mp is None and logprobs is None and penalties is None and logit_bias is None and grammar is None:
            return None
        st = cls(1, V, None, tiles=2, min_p=mp is not None, filtering=flt, sampling=temperature >= 1e-5)
        st.lp, st.lb, st.gr, st.mp = logprobs, logit_bias, grammar, mp
        if flt:
            st.top_k, st.top_p = int(top_k), float(top_p)
        if penalties is not None:
            st.pen_table, st.pen = getattr(penalties, "table", penalties), [getattr(penalties, k, None) for k in "raf"]
        st.stop = getattr(logit_bias, "stop", None)
        return st

    # ------------------------------------------------------------------ what is on
    @property
    def on(self) -> list:
        """The enabled features, as check_features names them (fixed once asked: a verify asks every cycle)."""
        if self._on is None:
            flags = dict(min_p=self.min_p_on, grammar=self.gr is not None, logit_bias=self.lb is not None,
                         penalties=self.pen_table is not None, filter=self.filtering, logprobs=self.lp is not None)
            self._on = [f for f, v in flags.items() if v]
        return self._on

    @property
    def processes(self) -> bool:
        """Whether the posterior comes from this stage's launches (else from the head launch's own epilogue, and the
        stage only reads the raw rows for logprobs)."""
        return (self.lb is not None or self.gr is not None or self.pen_table is not None or self.min_p_on
                or self.filtering)

    @property
    def materialises(self) -> bool:
        return self.processes or self.lp is not None

    def check_block(self, bs: int, temperature: float, seed, logits_out) -> None:
        """The refusals of one verify: blocks of <= 16 rows for the processors that read the block, the seeded draw at
        T > 0, and a logits_out the masked rows can be laid out like."""
        check_features(self.on, where="NativeTarget.verify: ", sampling=temperature >= 1e-5, seeded=seed is not None,
                       wide=bs > 16)
        if self.min_p_on and logits_out is not None and (logits_out.dim() != 2 or logits_out.stride(0) != self.V):
            raise ValueError("min_p needs logits_out with a row stride of V: the masked rows go to a buffer of the "
                             "stage's own, laid out like the rows they are made from")

    # ------------------------------------------------------------------ buffers
    def _buf(self, name: str, like: Optional[torch.Tensor] = None, tile: int = 0) -> torch.Tensor:
        """bf16 [tiles * 16, V], made on first use and kept; `like`: the view of it laid out like those rows, from
        16-row tile `tile` on (kept too: a cycle looks it up)."""
        key = (name, tile, None if like is None else like.shape)
        b = self._bufs.get(key)
        if b is None:
            if name not in self._bufs:
                self._bufs[name] = torch.zeros(16 * self.tiles, self.V, dtype=BF16, device=self.device)
            b = self._bufs[name]
            if like is not None:
                b = b[16 * tile:16 * tile + like.numel() // self.V].view(like.shape)
            self._bufs[key] = b
        return b

    @property
    def raw(self) -> torch.Tensor:
        """Where the head launch materialises the raw rows when the caller has no buffer of its own."""
        return self._buf("raw")

    # ------------------------------------------------------------------ admission
    def load_grammar(self, dfa, bias_row=None) -> int:
        """ops.grammar_load into the pool: the base `admit` takes (validated against the request's bias row, if any)."""
        return ops.grammar_load(self.gr, dfa, bias_row)

    def admit(self, slot: int, row: torch.Tensor, prompt: torch.Tensor, P: int, *, temperature: float, seed,
              first: Optional[torch.Tensor] = None, penalties=None, bias=None, grammar=None, min_p=None,
              flt: Optional[dict] = None) -> torch.Tensor:
        """Slot's values — penalties (r, a, f), bias (row, min_pos), grammar (base, start state), min_p, flt (top_k /
        top_p); None: neutral — then the first token from `row`, the prompt's last-row logits [1, V], which predict
        position P.  prompt: ids whose [.., :P] are the prompt's.  first: the int64 [1] view of position P in `prompt`
        (a session: the processors write their argmax there, and the draw lands there) or None (the token is returned
        alone and counted from its own tensor).  seed: None for a greedy or host-drawn token.  Returns ids [1, 1]."""
        one = slice(slot, slot + 1)
        sampled = seed is not None and temperature >= 1e-5
        z = raw = row.to(BF16).contiguous()
        wrote = False
        if self.lb is not None:   # the slot's whole row and min_pos are rewritten, whatever ran in the slot before
            ops.logit_bias_set(self.lb, slot, bias[0] if bias else None, bias[1] if bias else 0)
            z = ops.logit_bias_rows(z, self.lb.bias[one], min_pos=self.lb.min_pos[one], stop_ids=self.stop, pos_base=P,
                                    **(dict(out_ids=first) if first is not None else {}))
            wrote = first is not None
        g1 = None
        if self.gr is not None:   # base and state likewise (no grammar: -1 / -1, the rows pass unmasked); no walk
            ops.grammar_set(self.gr, slot, grammar[0] if grammar else None, grammar[1] if grammar else 0)
            g1 = SimpleNamespace(table=self.gr.table, base=self.gr.base[one], state=self.gr.state[one])
            z = ops.grammar_rows(z, g1, **(dict(out_ids=first) if first is not None else {}))
            wrote = first is not None
        if self.pen_table is not None:   # the slot's table row starts from the prompt alone
            r, a, f = penalties or (1.0, 0.0, 0.0)
            tab = self.pen_table[one]
            ops.penalty_count(tab, prompt, lo=0, hi=P, as_prompt=True, clear=True)
            z = ops.penalty_rows(z, tab, repetition_penalty=r, presence_penalty=a, frequency_penalty=f,
                                 **(dict(out_ids=first) if first is not None else {}))
            wrote = first is not None
            if self.device_values:
                for t, v in zip(self.pen, (r, a, f)):
                    t[one].fill_(v)
            else:
                self.pen = [r, a, f]
        if self.min_p:
            if self.device_values:
                self.mp[one].fill_(ops.min_p_log(min_p))
            else:
                self.mp = min_p
            if min_p is not None and sampled:   # the floor directly in front of the draw; filters off: the plain draw
                z = ops.min_p_rows(z, min_p=min_p, temperature=temperature)
                flt = flt or dict(top_k=0, top_p=1.0)
        if self.device_values:   # the slot's filter, re-armed on every admission (0 / 1.0: off)
            self.top_k[one].fill_(flt["top_k"] if flt else 0)
            self.top_p[one].fill_(flt["top_p"] if flt else 1.0)
        elif flt:
            self.top_k, self.top_p = flt["top_k"], flt["top_p"]
        tok = None if first is None else first.view(1, 1)
        if sampled:
            tok = draw_rows(z.unsqueeze(0), temperature, seed, P, flt)
        elif not wrote:
            tok = sample(z.unsqueeze(0), temperature)
        if first is not None and tok.data_ptr() != first.data_ptr():
            first.copy_(tok[0])
        ids, lo = (prompt, P) if first is not None else (tok.reshape(1, 1), 0)
        if self.pen_table is not None:   # the first token is output
            ops.penalty_count(tab, ids, lo=lo, hi=lo + 1)
        if g1 is not None:
            ops.grammar_advance(g1, ids, lo=lo, hi=lo + 1)
        if self.lp is not None:   # from the raw row: nothing is read back
            ops.logprob_rows(raw, first if first is not None else tok.reshape(1),
                             SimpleNamespace(**{**vars(self.lp), "slot": slot}), pos_base=P)
        return tok

    # ------------------------------------------------------------------ the block chain
    def rows(self, raw: torch.Tensor, block, post: torch.Tensor, *, draw: Optional[dict], pos: dict, tile: int = 0,
             nrows: Optional[int] = None, dyn=None, nrows_dyn_word: int = -1, tiles_per_req: int = 1) -> None:
        """The processors and the draw over the rows a head launch has just materialised: raw [<= 16, V] (one tile) or
        [tiles, 16, V]; block: the block ids ([slots, >= 16] or 1-D); post: where the ids go, laid out like the rows'
        tiles.  draw: None (greedy: the last processor's argmax stays) or seed= with temperature= / inv_t=.  pos: the
        pos_word / pos_base / pos_add of row 0.  Rows of a tile: nrows, else dyn[t][nrows_dyn_word] (a host row count
        goes to the host-value launches alone, as it always has).  tile: which 16-row tile of the stage's buffers."""
        size = dict(nrows=nrows, dyn=dyn, nrows_dyn_word=nrows_dyn_word)
        own = dict(nrows=nrows) if nrows is not None else size
        z = raw
        if self.lb is not None:
            z = ops.logit_bias_rows(z, self.lb.bias, min_pos=self.lb.min_pos, stop_ids=self.stop,
                                    out=self._buf("bias", raw, tile), out_ids=post, **size, **pos)
        if self.gr is not None:
            z = ops.grammar_rows(z, self.gr, block=block, out=self._buf("grammar", raw, tile), out_ids=post, **size)
        if self.pen_table is not None:
            r, a, f = self.pen
            z = ops.penalty_rows(z, self.pen_table, repetition_penalty=r, presence_penalty=a, frequency_penalty=f,
                                 block=block, out=self._buf("penalties", raw, tile), out_ids=post, **own)
        if draw is None:
            return
        tkw = {k: v for k, v in draw.items() if k != "seed"}
        if self.min_p_on:
            mp = dict(log_min_p=self.mp) if self.device_values else dict(min_p=self.mp)
            z = ops.min_p_rows(z, out=self._buf("min_p", raw, tile), tiles_per_req=tiles_per_req, **mp, **tkw, **own)
        ops.sample_rows_nucleus(z, top_k=self.top_k, top_p=self.top_p, tiles_per_req=tiles_per_req, out=post, **draw,
                                **size, **pos)

    def logprobs(self, raw: torch.Tensor, ids: torch.Tensor, *, pos: dict, nrows: Optional[int] = None, dyn=None,
                 nrows_dyn_word: int = -1, tiles_per_req: int = 1) -> None:
        """Behind whichever launch wrote the posterior, before the accept launch moves POS0: the sink's rows."""
        if self.lp is not None:
            ops.logprob_rows(raw, ids, self.lp, nrows=nrows, dyn=dyn, nrows_dyn_word=nrows_dyn_word,
                             tiles_per_req=tiles_per_req, **pos)

    # ------------------------------------------------------------------ commit
    def commit(self, output_ids: torch.Tensor, dyn: torch.Tensor, slots: Optional[int] = None) -> None:
        """Right behind an accept launch: what it committed, output_ids(S, START] of the draft record(s) it has just
        written, goes into the penalty table and steps the grammar state — once per cycle, eager or replayed; a parked
        slot is idle.  slots: the first `slots` (None: all)."""
        if self.pen_table is not None:
            ops.penalty_count(self.pen_table[:slots], output_ids, dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START,
                              lo=1, hi=1)
        if self.gr is not None:
            ops.grammar_advance(self.gr, output_ids, slots=slots, dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START,
                                lo=1, hi=1)
