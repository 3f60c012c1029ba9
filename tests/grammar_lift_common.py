"""Shared by the structured-output tests: seeded vocabularies over a byte automaton, random walks
to an accepting state, and the numpy models of dfl_grammar_reach's outputs.  The reference table of every case is
ByteGrammar.to_token_dfa(), which is TokenDFA.from_bytes."""
import numpy as np


def live_bytes(dfa, s):
    return np.nonzero(dfa.char_next[s] >= 0)[0]


def walk_bytes(dfa, rng, s, n):
    """Up to n bytes of a random walk from state s that never dies (shorter where a state has no way on)."""
    out = []
    for _ in range(n):
        ok = live_bytes(dfa, s)
        if not ok.size:
            break
        b = int(rng.choice(ok))
        out.append(b)
        s = int(dfa.char_next[s, b])
    return bytes(out), s


def accepted_text(dfa, rng, max_len=200):
    """A byte string the automaton accepts: a random walk that, from max_len / 2 on, heads for the nearest accepting
    state.  (Every state of a trimmed automaton reaches one.)"""
    S = dfa.num_states
    dist = np.full(S, 1 << 30)
    dist[list(dfa.accepting)] = 0
    for _ in range(S):
        nxt = dfa.char_next
        via = np.where(nxt >= 0, dist[np.where(nxt < 0, 0, nxt)], 1 << 30).min(axis=1) + 1
        new = np.minimum(dist, via)
        if np.array_equal(new, dist):
            break
        dist = new
    assert dist.max() < 1 << 30, "the automaton is not trimmed"
    s, out = dfa.start, []
    while True:
        if s in dfa.accepting and (len(out) >= max_len // 2 or rng.random() < 0.3 or not live_bytes(dfa, s).size):
            return bytes(out)
        ok = live_bytes(dfa, s)
        if len(out) >= max_len // 2:   # head home
            ok = np.array([b for b in ok if dist[dfa.char_next[s, b]] < dist[s]] or ok)
        b = int(rng.choice(ok))
        out.append(b)
        s = int(dfa.char_next[s, b])


def seeded_vocabulary(dfa, V, seed, eos_ids=()):
    """token_bytes of V ids over the byte automaton `dfa`: 0..255 the single bytes; the rest seeded — empty strings, 1..4
    bytes (from the automaton's own alphabet or any), walks of 17..48 bytes from a random state (long walks that
    survive), and such walks with the last byte replaced by one that dies."""
    rng = np.random.default_rng(seed)
    alphabet = np.nonzero((dfa.char_next >= 0).any(axis=0))[0]
    toks = [bytes([b]) for b in range(256)]
    S = dfa.num_states
    while len(toks) < V:
        kind = rng.random()
        if kind < 0.08:
            toks.append(b"")
        elif kind < 0.45:
            n = int(rng.integers(1, 5))
            src = alphabet if rng.random() < 0.8 else np.arange(256)
            toks.append(bytes(int(b) for b in rng.choice(src, n)))
        else:
            s = int(rng.integers(S))
            w, _ = walk_bytes(dfa, rng, s, int(rng.integers(17, 49)))
            if kind < 0.75 or len(w) < 2:
                toks.append(w if w else b"")
            else:       # the state in front of the last byte, and a byte that dies there
                at = s
                for b in w[:-1]:
                    at = int(dfa.char_next[at, b])
                dead = np.nonzero(dfa.char_next[at] < 0)[0]
                toks.append(w[:-1] + bytes([int(rng.choice(dead))]) if dead.size else w)
    from dflash_amd import Vocabulary
    return Vocabulary(toks, eos_ids)


def reach_model(table, bias=None):
    """(adj uint8 [S, S], any_legal uint8 [S]) of a token table int16 [S, V] under a bias row (fp32 [V], -inf: banned)."""
    S = table.shape[0]
    legal = table >= 0
    open_ = legal if bias is None else legal & (bias > -np.inf)[None, :]
    adj = np.zeros((S, S), np.uint8)
    for s in range(S):
        adj[s, np.unique(table[s][open_[s]])] = 1
    return adj, legal.any(axis=1).astype(np.uint8)
