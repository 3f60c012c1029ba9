"""What loading a grammar costs: the host lift and copy against the device lift.

V = 151936 over a SYNTHETIC byte-level vocabulary — no real tokenizer is available: ids 0..255 are the single bytes, the
rest seeded strings with a BPE-like length distribution (1..16 bytes, mode 3..5, half of them with a leading space,
mostly lower-case letters, some digits, JSON punctuation and two-byte UTF-8).  Three automata: a short regex, a JSON
schema with five mixed properties, a regex that compiles to more than 1000 states.  Per automaton, in one process, after
a warm-up of each path, alternating, 5 repeats each (median, min .. max), wall clock around a device synchronisation:

  host:    ByteGrammar.to_token_dfa() (TokenDFA.from_bytes, numpy) + ops.grammar_load of the TokenDFA (check_grammar on
           the host, the copy of Sc x V x 2 bytes)
  device:  ops.grammar_load of the ByteGrammar: the byte DFA's copy, dfl_grammar_lift, dfl_grammar_reach, the readback of
           adj / any_legal and the search over them (the vocabulary's device buffers exist: once per vocabulary)

The claim checked per automaton: the slowest device repeat beats the fastest host repeat.  Beside it: the lift launch
alone (HIP events, 5 launches) against the time merely to write Sc x V x 2 bytes at 8 TB/s, the reach launch alone, and
the pattern's compile time on the host.

    timeout -k 10 1100 python scripts/bench_grammar_lift.py
"""
from __future__ import annotations

import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import ByteGrammar, Vocabulary, _lib, compile_regex, json_schema_regex, ops  # noqa: E402

V = 151936
REPEATS = 5
SHORT = r"(yes|no|maybe)( [a-z]+){0,3}\."
SCHEMA = {"type": "object", "required": ["id", "name"], "properties": {
    "id": {"type": "integer"}, "name": {"type": "string", "maxLength": 12},
    "tags": {"type": "array", "items": {"enum": ["a", "bc", None]}, "maxItems": 3},
    "score": {"type": "number"}, "ok": {"type": "boolean"}}}
LARGE = r"[a-z0-9]{1,600}@[a-z]{1,480}\.(com|org|net)"


def synthetic_vocabulary(seed: int = 0) -> Vocabulary:
    rng = np.random.default_rng(seed)
    lengths = np.arange(1, 17)
    weight = np.array([2, 8, 15, 17, 15, 12, 10, 7, 5, 3, 2, 1.5, 1, 0.7, 0.5, 0.3])
    letters = np.frombuffer(b"etaoinshrdlcumwfgypbvkjxqz", np.uint8)
    letter_w = np.linspace(3.0, 0.3, letters.size)
    other = np.frombuffer(b"0123456789{}[]\":,.-_@ \n", np.uint8)
    toks = [bytes([b]) for b in range(256)]
    n = V - 256
    lens = rng.choice(lengths, n, p=weight / weight.sum())
    for L in lens.tolist():
        kind = rng.random()
        if kind < 0.06:                                     # a two-byte UTF-8 character or two
            t = "".join(chr(int(c)) for c in rng.integers(0xC0, 0x250, max(L // 2, 1))).encode("utf-8")
        elif kind < 0.22:
            t = bytes(rng.choice(other, L).tolist())
        else:
            body = bytes(rng.choice(letters, L, p=letter_w / letter_w.sum()).tolist())
            t = (b" " + body[1:]) if rng.random() < 0.5 and L > 1 else body
        toks.append(t)
    return Vocabulary(toks, eos_ids=(V - 1,))


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    dev = torch.device("cuda", 0)
    t0 = time.perf_counter()
    voc = synthetic_vocabulary()
    lens = np.array([len(t) for t in voc.token_bytes])
    print(json.dumps({"vocabulary": "SYNTHETIC (256 single bytes + seeded strings, BPE-like lengths)", "V": V,
                      "bytes": int(lens.sum()), "mean_len": round(float(lens.mean()), 2), "max_len": int(lens.max()),
                      "build_s": round(time.perf_counter() - t0, 2)}), flush=True)
    t0 = time.perf_counter()
    voc.device_buffers(dev)
    torch.cuda.synchronize()
    print(json.dumps({"vocabulary_to_device_ms": round(1e3 * (time.perf_counter() - t0), 2)}), flush=True)
    for name, pattern in (("short_regex", SHORT), ("json_schema_5", json_schema_regex(SCHEMA)), ("large_regex", LARGE)):
        t0 = time.perf_counter()
        dfa = compile_regex(pattern)
        compile_ms = 1e3 * (time.perf_counter() - t0)
        g = ByteGrammar(dfa, voc)
        Sc = g.num_states
        st = ops.grammar_state(1, Sc, V, dev)

        def host():
            st.used = 0
            torch.cuda.synchronize()
            t = time.perf_counter()
            tdfa = ByteGrammar(dfa, voc).to_token_dfa()      # (a fresh one: to_token_dfa keeps its result)
            t_lift = time.perf_counter()
            ops.grammar_load(st, tdfa)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t), 1e3 * (t_lift - t), tdfa

        def device():
            st.used = 0
            torch.cuda.synchronize()
            t = time.perf_counter()
            ops.grammar_load(st, g)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)

        _, _, tdfa = host()                                   # warm-up of each, and the tables compared once
        want = st.table.clone()
        device()
        equal = bool(torch.equal(st.table, want))
        hs, hl, ds = [], [], []
        for _ in range(REPEATS):
            h, l, _ = host()
            hs.append(h), hl.append(l)
            ds.append(device())
            print(f"# {name}: host {hs[-1]:.1f} ms, device {ds[-1]:.2f} ms", flush=True)
        lift_us, reach_us = [], []
        data, off, eos = voc.device_buffers(dev)              # the launch alone: its inputs are on the device already
        dfa_t = torch.from_numpy(g.char_next).to(dev)
        acc = np.zeros(Sc, np.uint8)
        acc[list(g.accepting)] = 1
        acc_t = torch.from_numpy(acc).to(dev)
        for _ in range(REPEATS):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            ops.check(_lib.lib().dfl_grammar_lift(st.table.data_ptr(), V, Sc, V, 0, dfa_t.data_ptr(), Sc, data.data_ptr(),
                                                  data.numel(), off.data_ptr(), acc_t.data_ptr(), eos.data_ptr(), 1,
                                                  torch.cuda.current_stream().cuda_stream), "dfl_grammar_lift")
            e[1].record()
            ops.grammar_reach(st, 0, Sc)
            e[2].record()
            torch.cuda.synchronize()
            lift_us.append(1e3 * e[0].elapsed_time(e[1])), reach_us.append(1e3 * e[1].elapsed_time(e[2]))
        print(json.dumps({"automaton": name, "states": Sc, "table_MB": round(Sc * V * 2 / 1e6, 1),
                          "compile_ms": round(compile_ms, 1), "tables_equal": equal,
                          "host_ms": spread(hs), "of_which_from_bytes_ms": spread(hl), "device_ms": spread(ds),
                          "claim_slowest_device_beats_fastest_host": max(ds) < min(hs),
                          "speedup_median": round(statistics.median(hs) / statistics.median(ds), 1),
                          "lift_launch_us": spread(lift_us), "reach_launch_us": spread(reach_us),
                          "write_floor_us_at_8TBps": round(Sc * V * 2 / 8e12 * 1e6, 2)}), flush=True)
        del st, want, tdfa


if __name__ == "__main__":
    main()
