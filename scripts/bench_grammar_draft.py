"""What the grammar-aware draft costs and returns ("The draft under the grammar").

1. The dfl_grammar_draft_rows launch at 16 x 151936 (a 64-state automaton, half of every state's columns legal): n = 16,
   n = 2, the ban-only form and both together, beside dfl_grammar_rows on the same rows for scale.  The logits rotate
   through enough buffers to exceed L2 and the 256 MB MALL, so every launch reads HBM; HIP events around blocks of
   launches, the arms alternating, min .. max over the blocks.
3. The single-request cycle (Qwen3-8B shapes, prefix 1024, block 16, T = 0, replayed) under a grammar with
   constrain_draft off / on.  The hook scripts the same accepted tokens into both arms after the pick, so the difference
   is the cost of materialising the draft's logits plus the pick launch.
4. The four-request ragged cycle (prompts 1024 / 768 / 512 / 896, replayed), off / on, scripted likewise.
5. The gain: a mixed grammar (a cycle of 37 states, every third free over the even tokens, the others forced) at the
   same shapes with random weights and NO scripting hook: mean acceptance length and accepted tokens per second, off / on.

    timeout -k 10 900 python scripts/bench_grammar_draft.py [--parts 1,3,4,5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import TokenDFA, ops  # noqa: E402
from scripts.bench_grammar import _on_grammar  # noqa: E402
from scripts.bench_logprobs import _hook, timed  # noqa: E402


def part_launch(dev):
    V, S = 151936, 64
    g = torch.Generator(device=dev).manual_seed(V)
    rng = np.random.default_rng(V)
    nbuf = (320 << 20) // (16 * V * 2) + 1          # > 256 MB MALL + L2
    lg = (torch.randn(nbuf, 16, V, generator=g, device=dev) * 2).to(torch.bfloat16)
    out = torch.empty(16, V, dtype=torch.bfloat16, device=dev)
    post = torch.zeros(16, dtype=torch.int64, device=dev)
    nxt = np.where(rng.random((S, V)) < 0.5, rng.integers(0, S, (S, V)), -1).astype(np.int16)
    st = ops.grammar_state(1, S, V, dev)
    ops.grammar_set(st, 0, ops.grammar_load(st, TokenDFA(nxt, 0)), 0)
    block = torch.zeros(16, dtype=torch.int64, device=dev)
    ops.grammar_draft_rows(lg[0], st, block=block)   # (a legal walk for the verify-side launch beside it)
    walk = block.clone()
    bias = torch.zeros(V, dtype=torch.float32, device=dev)
    bias[torch.from_numpy(rng.random(V) < 0.5).to(dev)] = float("-inf")
    arms = {
        "grammar_draft_rows_n16": lambda i: ops.grammar_draft_rows(lg[i % nbuf], st, block=block),
        "grammar_draft_rows_n2": lambda i: ops.grammar_draft_rows(lg[i % nbuf], st, block=block, nrows=2),
        "grammar_draft_rows_ban_only_n16": lambda i: ops.grammar_draft_rows(lg[i % nbuf], None, bias=bias, block=block),
        "grammar_draft_rows_both_n16": lambda i: ops.grammar_draft_rows(lg[i % nbuf], st, bias=bias, block=block),
        "grammar_rows_16": lambda i: ops.grammar_rows(lg[i % nbuf], st, block=walk, out=out, out_ids=post),
    }
    print(json.dumps({"part": 1, "V": V, "rows": 16, "buffers": nbuf, "us": timed(arms)}), flush=True)
    del lg


def part_cycle(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, 1024), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = bench.tau_plan(2 + warmup, steps, bs, seed=100)
    need = sum(k + 1 for k in plan[:warmup + steps + 2]) + 2 * bs
    G = greedy_walk(perm, prompt, need + 2 * bs).to(dev)
    dfa = _on_grammar(G, V)
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need,
                              max_block_size=bs, stop_token_ids=None, temperature=0.0, draft_token_hook=_hook(G, plan, V),
                              grammar=dfa, constrain_draft=arm == "on")
            s.prefill()
            s.cycle(bs)
            for _ in range(1 + warmup):
                s.cycle(bs, ahead_ok=True)
            s.capture(bs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tau = [s.cycle_graph(bs).tau for _ in range(steps)]
            torch.cuda.synchronize()
            res.setdefault(arm, []).append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
            taus[arm] = round(sum(tau) / len(tau), 3)
            del s
    print(json.dumps({"part": 3, "single_request_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v} for k, v in res.items()},
                      "mean_tau": taus, "steps": steps, "prefix": 1024, "block": bs}), flush=True)


def part_batch(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.synthetic import greedy_walk
    dev, bs, lens = draft.device, 16, (1024, 768, 512, 896)
    prompts = [torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(10 + i)).to(dev)
               for i, P in enumerate(lens)]
    plans = [bench.tau_plan(2 + warmup, steps, bs, seed=200 + i) for i in range(4)]
    need = max(sum(k + 1 for k in p[:warmup + steps + 3]) for p in plans) + 3 * bs
    Gs = [greedy_walk(perm, p, need + 2 * bs).to(dev) for p in prompts]
    hooks = [_hook(Gs[i], plans[i], V) for i in range(4)]
    hook = lambda r, blk, start, call: hooks[r](blk, start, call)   # noqa: E731
    dfa = _on_grammar(torch.cat(Gs), V)
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            dec = BatchedDecoder(draft, target, 4, max_rows=max(lens) + need + 64, out_len=max(lens) + need + 32,
                                 mask_token_id=cfg.mask_token_id, grammar_states=4, constrain_draft=arm == "on")
            h = dec.add_grammar(dfa)
            for r, p in enumerate(prompts):
                dec.admit(r, p, grammar=h)
            for _ in range(1 + warmup):
                dec.cycle(hook)
            dec.capture()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tau = [sum(o[0] for o in dec.cycle_graph(hook)) for _ in range(steps)]
            torch.cuda.synchronize()
            res.setdefault(arm, []).append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
            taus[arm] = round(sum(tau) / (4 * len(tau)), 3)
            del dec
    print(json.dumps({"part": 4, "four_request_ragged_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v}
                                                                   for k, v in res.items()},
                      "mean_tau": taus, "steps": steps, "prompts": lens, "block": bs}), flush=True)


def mixed_grammar(V, states=37):
    """A cycle of `states` states: every third is free over the even tokens, the others have one legal token each."""
    seq = torch.randperm(V - 1000, generator=torch.Generator().manual_seed(states))[:states].tolist()
    nxt = np.full((states, V), -1, dtype=np.int16)
    for i in range(states):
        if i % 3 == 0:
            nxt[i, 0::2] = (i + 1) % states
        else:
            nxt[i, seq[i]] = (i + 1) % states
    return TokenDFA(nxt, 0)


def part_gain(target, draft, cfg, V, steps, warmup, runs):
    from dflash_amd.generate import DecodeSession
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, 1024), generator=torch.Generator().manual_seed(1)).to(dev)
    dfa = mixed_grammar(V)
    need = (2 + warmup + steps) * bs + 2 * bs
    res, taus, rate, ids = {}, {}, {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need,
                              max_block_size=bs, stop_token_ids=None, temperature=0.0, grammar=dfa,
                              constrain_draft=arm == "on")
            s.prefill()
            s.cycle(bs)
            for _ in range(1 + warmup):
                s.cycle(bs, ahead_ok=True)
            s.capture(bs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tau = [s.cycle_graph(bs).tau for _ in range(steps)]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res.setdefault(arm, []).append(round(1e3 * dt / steps, 4))
            rate.setdefault(arm, []).append(round(sum(tau) / dt, 1))
            taus[arm] = round(sum(tau) / len(tau), 3)
            ids[arm] = s.output_ids[0, 1024:s.start + 1].tolist()     # (what has been committed so far)
            del s
    n = min(len(ids["on"]), len(ids["off"]))
    diff = [i for i in range(n) if ids["on"][i] != ids["off"][i]]
    # (token i is emitted in state i % 37; a forced state has one legal token, so the arms can part only in a free state,
    # at a near-tie among the target's 75968 legal logits there)
    first = None if not diff else {"index": diff[0], "state": diff[0] % 37, "free_state": (diff[0] % 37) % 3 == 0}
    print(json.dumps({"part": 5, "mixed_grammar_cycle_ms": {k: {"min": min(v), "max": max(v)} for k, v in res.items()},
                      "accepted_tokens_per_s": {k: {"min": min(v), "max": max(v)} for k, v in rate.items()},
                      "mean_tau": taus, "ids_compared": n, "ids_equal": not diff, "first_difference": first, "steps": steps,
                      "prefix": 1024, "block": bs}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,3,4,5")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=4)
    a = ap.parse_args()
    parts = {int(x) for x in a.parts.split(",") if x}
    dev = torch.device("cuda", 0)
    if 1 in parts:
        part_launch(dev)
    if parts & {3, 4, 5}:
        import bench   # (the workload builders only; bench.py itself is not run)
        spec = bench.workload_spec("qwen3-8b")
        args = SimpleNamespace(target_layers=0, hf_verify=False, hf_prefill=False, attn_impl="head", fuse_oproj=False)
        target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
        if 3 in parts:
            part_cycle(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)
        if 4 in parts:
            part_batch(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)
        if 5 in parts:
            part_gain(target, draft, cfg, meta["V"], a.steps, a.warmup, a.runs)


if __name__ == "__main__":
    main()
