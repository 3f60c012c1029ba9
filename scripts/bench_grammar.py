"""What grammar-constrained decoding costs.

1. The dfl_grammar_rows launch at 16 x 151936 (a 64-state automaton, half of every state's columns legal, the block a
   legal walk), beside dfl_logit_bias_rows and dfl_penalty_rows on the same rows; then row 0 alone (no walk) and row 15
   alone (15 dependent steps in front of the dense pass), and dfl_grammar_advance alone (4 slots, 16 committed ids).
   The logits rotate through enough buffers to exceed L2 and the 256 MB MALL, so every launch reads HBM; HIP events
   around blocks of launches, the arms alternating, min .. max over the blocks.
3. The single-request cycle (Qwen3-8B shapes, prefix 1024, block 16, T = 0, replayed) with the grammar off / on.
4. The four-request ragged cycle (prompts 1024 / 768 / 512 / 896, replayed) with the pool and the grammars off / on.
The on arm's automaton has four states that every legal token steps round and forbids 1000 ids the scripted walk never
visits: both arms accept the same tokens.

    timeout -k 10 900 python scripts/bench_grammar.py [--parts 1,3,4]
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
from scripts.bench_logprobs import _hook, timed  # noqa: E402

PEN = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.25)


def part_launch(dev):
    V, S = 151936, 64
    g = torch.Generator(device=dev).manual_seed(V)
    rng = np.random.default_rng(V)
    nbuf = (320 << 20) // (16 * V * 2) + 1          # > 256 MB MALL + L2
    lg = (torch.randn(nbuf, 16, V, generator=g, device=dev) * 2).to(torch.bfloat16)
    out = torch.empty(16, V, dtype=torch.bfloat16, device=dev)
    post = torch.zeros(16, dtype=torch.int64, device=dev)
    nxt = np.where(rng.random((S, V)) < 0.5, rng.integers(0, S, (S, V)), -1).astype(np.int16)
    dfa = TokenDFA(nxt, 0)
    st = ops.grammar_state(4, S, V, dev)
    base = ops.grammar_load(st, dfa)
    for slot in range(4):
        ops.grammar_set(st, slot, base, slot)
    blocks = np.zeros((4, 16), dtype=np.int64)
    for slot in range(4):                           # legal walks: every row of the tile is live
        s = slot
        for i in range(1, 16):
            blocks[slot, i] = rng.choice(np.nonzero(nxt[s] >= 0)[0])
            s = nxt[s, blocks[slot, i]]
    blocks = torch.from_numpy(blocks).to(dev)
    block = blocks[0].contiguous()
    pick = torch.randperm(V, generator=torch.Generator().manual_seed(V))[:3000].tolist()
    b, _ = ops.check_logit_bias(V, {v: (2.0 if i % 2 else -2.0) for i, v in enumerate(pick[:2000])}, None, pick[2000:])
    lb = ops.logit_bias_state(1, V, dev)
    ops.logit_bias_set(lb, 0, b, 0)
    ids = torch.randint(0, V, (1, 1200), generator=g, device=dev)
    table = ops.penalty_state(1, V, dev)
    ops.penalty_count(table, ids, lo=0, hi=1024, as_prompt=True, clear=True)
    ops.penalty_count(table, ids, lo=1024, hi=1200)
    one = torch.zeros(1, dtype=torch.int64, device=dev)
    arms = {
        "grammar_rows": lambda i: ops.grammar_rows(lg[i % nbuf], st, block=block, out=out, out_ids=post),
        "logit_bias_rows": lambda i: ops.logit_bias_rows(lg[i % nbuf], lb.bias, out=out, out_ids=post, pos_base=100),
        "penalty_rows": lambda i: ops.penalty_rows(lg[i % nbuf], table, block=block, out=out, out_ids=post, **PEN),
        "grammar_rows_in_place": lambda i: ops.grammar_rows(lg[i % nbuf], st, block=block, out=lg[i % nbuf]),
    }
    print(json.dumps({"part": 1, "V": V, "rows": 16, "buffers": nbuf, "us": timed(arms)}), flush=True)
    lg[:] = (torch.randn(nbuf, 16, V, generator=g, device=dev) * 2).to(torch.bfloat16)   # (the in-place arm masked them)
    arms = {
        "grammar_rows_row0_alone": lambda i: ops.grammar_rows(lg[i % nbuf], st, block=block, out=out, row0=0, nrows=1,
                                                              out_ids=one),
        "grammar_rows_row15_alone": lambda i: ops.grammar_rows(lg[i % nbuf], st, block=block, out=out, row0=15, nrows=1,
                                                               out_ids=one),
        "logit_bias_rows_row0_alone": lambda i: ops.logit_bias_rows(lg[i % nbuf], lb.bias, out=out, row0=0, nrows=1,
                                                                    out_ids=one, pos_base=100),
        "logit_bias_rows_row15_alone": lambda i: ops.logit_bias_rows(lg[i % nbuf], lb.bias, out=out, row0=15, nrows=1,
                                                                     out_ids=one, pos_base=100),
    }
    print(json.dumps({"part": 1, "V": V, "rows": 1, "us": timed(arms)}), flush=True)
    # the advance: 4 slots, 16 committed ids each, the state put back by a host-side fill outside the timed launches' cost
    # (a violated state would end the walk early: the blocks are legal walks, so every launch does its 15 steps)
    dyn = torch.tensor([[0, 0, 16, 0, 15, 0, 0, 0]] * 4, dtype=torch.int32, device=dev)
    start = st.state.clone()

    def advance(i):
        st.state.copy_(start)
        ops.grammar_advance(st, blocks, dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START, lo=1, hi=1)

    print(json.dumps({"part": 1, "slots": 4, "ids": 15,
                      "us": timed({"state_copy_alone": lambda i: st.state.copy_(start), "copy_plus_grammar_advance": advance})}),
          flush=True)
    del lg


def _on_grammar(G, V):
    """The on arm's automaton for a scripted walk G: four states every legal token steps round; 1000 ids the walk never
    visits are illegal everywhere."""
    walk = set(G.tolist())
    free = [v for v in range(V) if v not in walk][:1000]
    nxt = np.repeat(((np.arange(4, dtype=np.int16) + 1) % 4)[:, None], V, axis=1)
    nxt[:, free] = -1
    return TokenDFA(np.ascontiguousarray(nxt), 0)


def part_cycle(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, 1024), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = bench.tau_plan(2 + warmup, steps, bs, seed=100)
    need = sum(k + 1 for k in plan[:warmup + steps + 2]) + 2 * bs
    G = greedy_walk(perm, prompt, need + 2 * bs).to(dev)
    dfa = _on_grammar(G, V)
    res, taus, states = {}, {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need,
                              max_block_size=bs, stop_token_ids=None, temperature=0.0, draft_token_hook=_hook(G, plan, V),
                              grammar=dfa if arm == "on" else None)
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
            states[arm] = s.finish_grammar(s.finish())
            del s
    print(json.dumps({"part": 3, "single_request_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v} for k, v in res.items()},
                      "mean_tau": taus, "grammar_state": states, "steps": steps, "prefix": 1024, "block": bs}), flush=True)


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
                                 mask_token_id=cfg.mask_token_id, grammar_states=4 if arm == "on" else 0)
            h = dec.add_grammar(dfa) if arm == "on" else None
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,3,4")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=4)
    a = ap.parse_args()
    parts = {int(x) for x in a.parts.split(",") if x}
    dev = torch.device("cuda", 0)
    if 1 in parts:
        part_launch(dev)
    if parts & {3, 4}:
        import bench   # (the workload builders only; bench.py itself is not run)
        spec = bench.workload_spec("qwen3-8b")
        args = SimpleNamespace(target_layers=0, hf_verify=False, hf_prefill=False, attn_impl="head", fuse_oproj=False)
        target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
        if 3 in parts:
            part_cycle(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)
        if 4 in parts:
            part_batch(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)


if __name__ == "__main__":
    main()
