"""Token automata for grammar-constrained decoding.

A TokenDFA is a dense table next int16 [S, V]: next[s, v] >= 0 is the state after token v in state s, -1 means v is
illegal in s.  End of text is part of the table: a stop id is legal exactly in the accepting states (its successor is any
state).  Host-side numpy only; ops.grammar_load copies a table into the device pool the kernels read.
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
