"""Token automata for grammar-constrained decoding.

A TokenDFA is a dense table next int16 [S, V]: next[s, v] >= 0 is the state after token v in state s, -1 means v is
illegal in s.  End of text is part of the table: a stop id is legal exactly in the accepting states (its successor is any
state).  Host-side numpy only; ops.grammar_load copies a table into the device pool the kernels read.

Structured outputs: a Vocabulary holds the byte string of every token id, a ByteGrammar a byte
automaton (dflash_amd.regex, dflash_amd.json_schema) over one.  A ByteGrammar goes wherever a TokenDFA does;
ops.grammar_load lifts it to the token table on the device, so that table is never built here.
"""
from __future__ import annotations

from typing import Iterable, Mapping, Sequence

import numpy as np

MAX_STATES = 32767


class TokenDFA:
    """TokenDFA(next, start=0): next int16 [S, V] (1 <= S <= 32767, V % 8 == 0), -1 = illegal.  The array is kept as
    given (no copy of an int16 C-contiguous array); ops.check_grammar validates it."""

    def __init__(self, next, start: int = 0):
        self.next = next
        self.start = start

    @property
    def num_states(self) -> int:
        return int(self.next.shape[0])

    @property
    def vocab_size(self) -> int:
        return int(self.next.shape[1])

    @classmethod
    def from_dict(cls, transitions: Mapping[int, Mapping[int, int]], V: int, start: int = 0) -> "TokenDFA":
        """{state: {token: next_state}} (the shape of an outlines-style index) over a vocabulary of V.  The states are
        0 .. the largest one named, as a key or as a successor; a state without an entry has no legal token."""
        V = int(V)
        names = [int(start)]
        for s, row in transitions.items():
            names.append(int(s))
            names.extend(int(n) for n in row.values())
        if min(names) < 0:
            raise ValueError(f"dflash_amd: TokenDFA.from_dict: state {min(names)} is negative")
        S = max(names) + 1
        if S > MAX_STATES:
            raise ValueError(f"dflash_amd: TokenDFA.from_dict: {S} states, at most {MAX_STATES}")
        nxt = np.full((S, V), -1, dtype=np.int16)
        for s, row in transitions.items():
            for v, n in row.items():
                v = int(v)
                if not 0 <= v < V:
                    raise ValueError(f"dflash_amd: TokenDFA.from_dict: token {v} outside [0, {V})")
                nxt[int(s), v] = int(n)
        return cls(nxt, int(start))

    @classmethod
    def from_bytes(cls, char_next, accepting: Iterable[int], token_bytes: Sequence[bytes], eos_ids: Iterable[int] = (),
                   start: int = 0) -> "TokenDFA":
        """Lift a byte-level DFA over a vocabulary's byte strings.  char_next int [Sc, 256], -1 = dead; token v is legal in
        state s iff walking token_bytes[v] from s never dies, and its successor is where the walk ends.  eos_ids are legal
        in the accepting states only (successor: the state itself); empty byte strings are illegal everywhere."""
        cn = np.asarray(char_next)
        if cn.ndim != 2 or cn.shape[1] != 256 or cn.shape[0] < 1 or not np.issubdtype(cn.dtype, np.integer):
            raise ValueError("dflash_amd: TokenDFA.from_bytes: char_next is an integer array [Sc, 256]")
        Sc, V = cn.shape[0], len(token_bytes)
        if Sc > MAX_STATES:
            raise ValueError(f"dflash_amd: TokenDFA.from_bytes: {Sc} states, at most {MAX_STATES}")
        if cn.min() < -1 or cn.max() >= Sc:
            raise ValueError(f"dflash_amd: TokenDFA.from_bytes: char_next has a successor outside [-1, {Sc})")
        # one more row, the dead state, absorbs every byte: the walk needs no branch
        ext = np.full((Sc + 1, 256), Sc, dtype=np.int64)
        ext[:Sc] = np.where(cn < 0, Sc, cn)
        lens = np.fromiter((len(b) for b in token_bytes), dtype=np.int64, count=V)
        L = int(lens.max()) if V else 0
        padded = np.zeros((V, max(L, 1)), dtype=np.int64)
        for v, b in enumerate(token_bytes):
            if b:
                padded[v, :len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
        cur = np.broadcast_to(np.arange(Sc, dtype=np.int64)[:, None], (Sc, V)).copy()
        for i in range(L):   # all states x all tokens at once, one byte position per step
            step = ext[cur, padded[None, :, i]]
            cur = np.where((i < lens)[None, :], step, cur)
        cur[:, lens == 0] = Sc
        nxt = np.where(cur == Sc, -1, cur).astype(np.int16)
        acc = np.zeros(Sc, dtype=bool)
        acc[np.asarray(sorted(int(a) for a in accepting), dtype=np.int64)] = True
        for e in eos_ids:
            e = int(e)
            if not 0 <= e < V:
                raise ValueError(f"dflash_amd: TokenDFA.from_bytes: eos id {e} outside [0, {V})")
            nxt[:, e] = np.where(acc, np.arange(Sc), -1).astype(np.int16)
        return cls(nxt, int(start))


def _bytes_to_unicode() -> dict:
    """The byte -> printable character table of GPT-2's byte-level BPE (public: openai/gpt-2 encoder.py)."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    table, n = {}, 0
    for b in range(256):
        if b in keep:
            table[b] = chr(b)
        else:
            table[b] = chr(256 + n)
            n += 1
    return table


class Vocabulary:
    """Vocabulary(token_bytes, eos_ids=()): the byte string of every token id (empty: the token is illegal everywhere, as
    TokenDFA.from_bytes treats it) and the ids that end a text.  The host list is kept; device_buffers(device) makes, once
    per device, the two buffers dfl_grammar_lift reads: the byte strings back to back (uint8) and their offsets (int32
    [V + 1])."""

    def __init__(self, token_bytes: Sequence[bytes], eos_ids: Iterable[int] = ()):
        self.token_bytes = [bytes(b) for b in token_bytes]
        V = len(self.token_bytes)
        self.eos_ids = tuple(int(e) for e in eos_ids)
        for e in self.eos_ids:
            if not 0 <= e < V:
                raise ValueError(f"dflash_amd: Vocabulary: eos id {e} outside [0, {V})")
        if sum(len(b) for b in self.token_bytes) >= 1 << 31:
            raise ValueError("dflash_amd: Vocabulary: the byte strings exceed 2 GiB")
        self._device = {}

    def __len__(self) -> int:
        return len(self.token_bytes)

    def flat(self):
        """(bytes uint8 [sum of lengths, at least 1], offsets int32 [V + 1]) as numpy arrays."""
        lens = np.fromiter((len(b) for b in self.token_bytes), dtype=np.int64, count=len(self.token_bytes))
        off = np.zeros(len(lens) + 1, dtype=np.int32)
        np.cumsum(lens, out=off[1:])
        data = np.frombuffer(b"".join(self.token_bytes) or b"\0", dtype=np.uint8)
        return data, off

    def device_buffers(self, device):
        import torch
        key = str(torch.device(device))
        if key not in self._device:
            data, off = self.flat()
            self._device[key] = (torch.from_numpy(data.copy()).to(device), torch.from_numpy(off).to(device),
                                 torch.tensor(self.eos_ids or (0,), dtype=torch.int32, device=device))
        return self._device[key]

    @classmethod
    def from_tokenizer(cls, tok, vocab_size: int = None, eos_ids: Iterable[int] = None) -> "Vocabulary":
        """A GPT-2-style byte-level BPE tokenizer (Qwen, Llama-3): the bytes-to-unicode table inverted over
        tok.get_vocab(), padded to vocab_size (the model's V) with empty strings; added / special tokens get empty
        strings.  eos_ids: default tok.eos_token_id.  A token that is not spelled in the table's characters means another
        kind of tokenizer: ValueError."""
        if not hasattr(tok, "get_vocab"):
            raise ValueError("dflash_amd: Vocabulary.from_tokenizer: the tokenizer has no get_vocab()")
        back = {c: b for b, c in _bytes_to_unicode().items()}
        vocab = tok.get_vocab()
        added = set(getattr(tok, "get_added_vocab", dict)()) | set(getattr(tok, "all_special_tokens", ()) or ())
        n = max(vocab.values(), default=-1) + 1
        V = n if vocab_size is None else int(vocab_size)
        if V < n:
            raise ValueError(f"dflash_amd: Vocabulary.from_tokenizer: vocab_size {V} below the tokenizer's {n} ids")
        out = [b""] * V
        for text, i in vocab.items():
            if text in added:
                continue
            try:
                out[i] = bytes(back[c] for c in text)
            except KeyError:
                raise ValueError(f"dflash_amd: Vocabulary.from_tokenizer: token {i} ({text!r}) is not byte-level BPE "
                                 f"(only GPT-2-style byte-level tokenizers are supported)") from None
        if eos_ids is None:
            e = getattr(tok, "eos_token_id", None)
            eos_ids = () if e is None else (e,)
        return cls(out, eos_ids)


class ByteGrammar:
    """ByteGrammar(byte_dfa, vocabulary): a byte automaton (dflash_amd.regex.ByteDFA, or anything with char_next /
    accepting / start) over a Vocabulary.  Taken wherever a TokenDFA is; ops.grammar_load lifts it to the token table on
    the device (dfl_grammar_lift).  to_token_dfa() is TokenDFA.from_bytes of the same inputs: the
    reference, and the loading path above 4096 states."""

    def __init__(self, byte_dfa, vocabulary: Vocabulary):
        cn = np.asarray(byte_dfa.char_next)
        if cn.ndim != 2 or cn.shape[1] != 256 or cn.shape[0] < 1 or not np.issubdtype(cn.dtype, np.integer):
            raise ValueError("dflash_amd: ByteGrammar: char_next is an integer array [Sc, 256]")
        if cn.shape[0] > MAX_STATES:
            raise ValueError(f"dflash_amd: ByteGrammar: {cn.shape[0]} states, at most {MAX_STATES}")
        if cn.min() < -1 or cn.max() >= cn.shape[0]:
            raise ValueError(f"dflash_amd: ByteGrammar: char_next has a successor outside [-1, {cn.shape[0]})")
        self.char_next = np.ascontiguousarray(cn, dtype=np.int16)
        self.accepting = tuple(sorted(int(a) for a in byte_dfa.accepting))
        if self.accepting and not 0 <= self.accepting[0] <= self.accepting[-1] < cn.shape[0]:
            raise ValueError("dflash_amd: ByteGrammar: an accepting state is no state")
        self.start = int(byte_dfa.start)
        self.vocabulary = vocabulary
        self._dfa = None

    @property
    def num_states(self) -> int:
        return int(self.char_next.shape[0])

    @property
    def vocab_size(self) -> int:
        return len(self.vocabulary)

    def to_token_dfa(self) -> TokenDFA:
        if self._dfa is None:
            self._dfa = TokenDFA.from_bytes(self.char_next, self.accepting, self.vocabulary.token_bytes,
                                            self.vocabulary.eos_ids, self.start)
        return self._dfa


def compile_grammar(*, regex: str = None, json_schema: dict = None, vocabulary: Vocabulary,
                    whitespace_pattern: str = "[ ]?", max_states: int = 4096) -> ByteGrammar:
    """A ByteGrammar from a regular expression or a JSON schema (exactly one of them)."""
    from .json_schema import json_schema_regex
    from .regex import compile_regex
    if (regex is None) == (json_schema is None):
        raise ValueError("dflash_amd: compile_grammar: give exactly one of regex and json_schema")
    if json_schema is not None:
        regex = json_schema_regex(json_schema, whitespace_pattern=whitespace_pattern)
    return ByteGrammar(compile_regex(regex, max_states=max_states), vocabulary)
