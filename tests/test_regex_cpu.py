"""dflash_amd.regex against Python's `re`: the DFA's verdict on a string equals
re.compile(p, re.ASCII).fullmatch(s) is not None — on every string up to length 5 over the pattern's own small alphabet
plus a foreign character, and on seeded random walks of the DFA to an accepting state with one-byte edits of them."""
import itertools
import re

import numpy as np
import pytest

import grammar_lift_common as C
from dflash_amd import ByteDFA, TokenDFA, compile_regex, ops
from dflash_amd.json_schema import INTEGER, NUMBER, STRING

# (pattern, alphabet): the alphabet is the pattern's own characters of interest plus one foreign to it
PATTERNS = [
    ("abc", "abcx"), ("(a|b)*abb", "abx"), ("a*", "ab"), ("a+b?", "abx"), ("a?b+c*", "abcx"),
    ("a{3}", "ab"), ("a{2,}", "ab"), ("a{1,3}b", "abx"), ("(ab){2,3}", "abx"), ("(a{1,2}b){0,2}c", "abcx"),
    ("((a|b){2}c){1,2}", "abcx"), ("a|bc|", "abcx"), ("(?:ab|c)+", "abcx"), ("^ab$", "abx"), ("a{,2}b", "abx"),
    ("x{1}y{0}z", "xyz"), ("[abc]+", "abcd"), ("[a-c]x", "abcdx"), ("[^a]", "ab\né"), ("[^a-c\\d]+", "ad1x"),
    ("[]a]+", "]ab"), ("[a\\]-]+", "a]-x"), ("[\\w-]+", "a_-+"), ("[^\\W\\d]", "a1_ "), ("[\\s,]*", " ,\tx"),
    (".", "a\né"), ("a.c", "abc\n"), (".*b", "ab\n"), ("\\d+", "01a"), ("\\D", "1aé"), ("\\w+", "aZ_9-"), ("\\W", "a- é"),
    ("\\s\\S", " a\t"), ("\\n\\t\\\\", "\n\t\\x"), ("\\.\\*\\(\\)\\[", ".*()[x"), ("\\x41\\u00e9+", "Aéx"),
    ("é+x", "éxe"), ("[α-ω]+", "αβωa"), ("日本(語|人)?", "日本語人x"), ("[^é]é", "éab"), ("😀|a", "😀ab"),
    ("a{2}{", "a{x"), ("{a}", "{a}x"),
    (STRING, "\"\\aun\x01"), (INTEGER, "-01x"), (NUMBER, "-0.e+1"),
]
IDS = [f"{i}:{p[:18]}" for i, (p, _) in enumerate(PATTERNS)]


def verdicts_agree(dfa, rx, s):
    got, want = dfa.matches(s.encode("utf-8")), rx.fullmatch(s) is not None
    assert got == want, (rx.pattern, s, got, want)


@pytest.mark.parametrize("pattern,alphabet", PATTERNS, ids=IDS)
def test_every_short_string_over_the_alphabet(pattern, alphabet):
    dfa, rx = compile_regex(pattern), re.compile(pattern, re.ASCII)
    alphabet = sorted(set(alphabet))[:6]
    for n in range(6):
        for t in itertools.product(alphabet, repeat=n):
            verdicts_agree(dfa, rx, "".join(t))


@pytest.mark.parametrize("pattern,alphabet", PATTERNS, ids=IDS)
def test_random_walks_to_acceptance_and_their_one_byte_edits(pattern, alphabet):
    dfa, rx = compile_regex(pattern), re.compile(pattern, re.ASCII)
    rng = np.random.default_rng(len(pattern))
    edits = 0
    for _ in range(12):
        text = C.accepted_text(dfa, rng, max_len=40)
        assert dfa.matches(text)
        assert rx.fullmatch(text.decode("utf-8")) is not None, (pattern, text)     # accepted => well-formed UTF-8
        for _ in range(6):
            b = bytearray(text)
            kind = rng.integers(3) if b else 1
            at = int(rng.integers(len(b) + (kind == 1)))
            if kind == 0:
                b[at] = int(rng.integers(256))
            elif kind == 1:
                b.insert(at, int(rng.choice(np.frombuffer(alphabet.encode(), np.uint8))))
            else:
                del b[at]
            try:
                s = bytes(b).decode("utf-8")
            except UnicodeDecodeError:
                assert not dfa.matches(bytes(b)), (pattern, bytes(b))               # ill-formed UTF-8 is never accepted
                continue
            verdicts_agree(dfa, rx, s)
            edits += 1
    assert edits >= 3           # (the rest were ill-formed UTF-8, checked above: most edits of multi-byte texts)


@pytest.mark.parametrize("pattern,alphabet", PATTERNS, ids=IDS)
def test_trimmed_deterministic_and_numbered_from_the_start(pattern, alphabet):
    a, b = compile_regex(pattern), compile_regex(pattern)
    assert isinstance(a, ByteDFA) and a.char_next.dtype == np.int16 and a.char_next.shape[1] == 256 and a.start == 0
    assert np.array_equal(a.char_next, b.char_next) and a.accepting == b.accepting
    S = a.num_states
    assert a.char_next.min() >= -1 and a.char_next.max() < S and a.accepting
    alive = np.zeros(S, bool)                                   # every state reaches an accepting one
    alive[list(a.accepting)] = True
    for _ in range(S):
        alive |= ((a.char_next >= 0) & alive[np.where(a.char_next < 0, 0, a.char_next)]).any(axis=1)
    assert alive.all()
    order, seen = [0], {0}                                      # BFS order from the start over bytes 0..255
    for s in order:
        for t in a.char_next[s][a.char_next[s] >= 0].tolist():
            if t not in seen:
                seen.add(t)
                order.append(t)
    assert order == list(range(S))


def test_state_counts_of_textbook_automata():
    assert compile_regex("(a|b)*abb").num_states == 4
    assert compile_regex("(a|b)*a(a|b)(a|b)").num_states == 8        # the third symbol from the end: 2^3
    assert compile_regex("(0|1(01*0)*1)*").num_states == 3           # binary multiples of three: the remainders
    assert compile_regex("(0|1(01*0)*1)+").num_states == 4           # non-empty: the start is a state of its own
    assert compile_regex("a{16}").num_states == 17 and compile_regex("[a-c]*").num_states == 1
    assert compile_regex("(a|b)*abb").accepting == (3,)


REFUSED = [("(a)\\1", "backreference"), ("(?P<n>a)(?P=n)", "named group"), ("(?P=n)", "backreference"),
           ("(?=a)a", "lookaround"), ("(?!a)b", "lookaround"), ("(?<=a)b", "lookaround"), ("(?<!a)b", "lookaround"),
           ("a*?", "lazy"), ("a+?", "lazy"), ("a??", "lazy"), ("a{1,2}?", "lazy"), ("a*+", "possessive"), ("a++", "possessive"),
           ("(?i)a", "inline flag"), ("(?s:a)", "inline flag"), ("(?<n>a)", "named group"), ("a\\b", "\\\\b"), ("\\Ba", "\\\\B"),
           ("a^b", "anchor"), ("a$b", "anchor"), ("\\Aa", "escape \\\\A"), ("a\\Z", "escape \\\\Z"), ("\\pL", "escape \\\\p")]


@pytest.mark.parametrize("pattern,name", REFUSED, ids=[p for p, _ in REFUSED])
def test_unsupported_constructs_are_refused_by_name(pattern, name):
    with pytest.raises(ValueError, match="regex: .*" + name + ".*not supported"):
        compile_regex(pattern)


@pytest.mark.parametrize("pattern", ["(a", "a)", "[a", "*a", "a**", "a{3,1}", "[b-a]", "\\", "\\xZ1", "\\ud800"])
def test_malformed_patterns_are_refused(pattern):
    with pytest.raises(ValueError, match="dflash_amd: regex"):
        compile_regex(pattern)


def test_empty_language_and_max_states():
    with pytest.raises(ValueError, match="empty language"):
        compile_regex("[^\\d\\D]")
    with pytest.raises(ValueError, match="empty language"):
        compile_regex("a[^\\w\\W]b|[^\\s\\S]")
    with pytest.raises(ValueError, match="max_states = 64"):
        compile_regex("(a|b)*a(a|b){9}", max_states=64)                  # 2^10 subsets
    assert compile_regex("(a|b)*a(a|b){9}", max_states=2048).num_states == 1024
    with pytest.raises(ValueError, match="max_states"):
        compile_regex("a", max_states=0)


def test_byte_dfa_round_trips_through_from_bytes_and_check_grammar():
    """A toy vocabulary of 16 tokens: the lifted table steps exactly as the byte walk does, and check_grammar takes it."""
    from dflash_amd import ByteGrammar, Vocabulary
    dfa = compile_regex("(ab|é)+c?")
    toks = [b"a", b"b", b"ab", b"c", "é".encode(), b"\xc3", b"\xa9", b"abab", b"bc", b"", b"x", b"ca", b"abc", b"ba", b"", b""]
    t = TokenDFA.from_bytes(dfa.char_next, dfa.accepting, toks, eos_ids=(15,), start=dfa.start)
    ops.check_grammar(t, 16)
    for s in range(dfa.num_states):
        for v, tok in enumerate(toks[:15]):
            at = s
            for b in tok:
                at = int(dfa.char_next[at, b]) if at >= 0 else -1
            assert t.next[s, v] == (at if tok else -1)
        assert t.next[s, 15] == (s if s in dfa.accepting else -1)
    g = ByteGrammar(dfa, Vocabulary(toks, eos_ids=(15,)))
    assert (g.num_states, g.vocab_size, g.start) == (dfa.num_states, 16, 0)
    assert np.array_equal(g.to_token_dfa().next, t.next)
    ops.check_grammar(g, 16)                                            # the host-side checks of a ByteGrammar
    with pytest.raises(ValueError, match="vocabulary has 16 tokens"):
        ops.check_grammar(g, 24)
