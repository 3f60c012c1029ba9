"""What stop sequences cost.

1. The dfl_stop_seq_rows launch alone at 1 and 4 slots, block 16, every slot with eight sequences of 16 ids that never
   match (every lane walks all eight tables), beside dfl_grammar_advance and dfl_penalty_count over the same 16 committed
   ids in the same process: points of comparison, not a bar.  HIP events around blocks of 64 launches, the arms
   alternating, median of 8 blocks (min .. max).
2. The replayed single-request cycle (Qwen3-8B shapes, prefix 1024, block 16, T = 0) without / with eight stop sequences
   of 16 ids, the arms alternating.
3. The four-request ragged cycle (prompts 1024 / 768 / 512 / 896, replayed), the decoder built without / with
   stop_sequences=True and every slot carrying eight sequences of 16, the arms alternating.
No sequence matches: both arms run the same cycles and accept the same tokens.

    timeout -k 10 900 python scripts/bench_stop_seq.py [--parts 1,2,3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import ops  # noqa: E402
from scripts.bench_logprobs import _hook, timed  # noqa: E402


def never(V):
    """Eight sequences of 16 ids out of the top 1000 ids, which no prompt and no walk of the workload holds."""
    return [[V - 1 - 16 * k - j for j in range(16)] for k in range(8)]


def part_launch(dev):
    V, n = 151936, 2048
    for slots in (1, 4):
        g = torch.Generator(device=dev).manual_seed(slots)
        ids = torch.randint(0, V - 1000, (slots, n), generator=g, device=dev)
        block = ids[:, 1024:1040].contiguous()
        post = torch.cat([block[:, 1:], ids[:, 1040:1041]], dim=1).contiguous()      # everything accepted: 16 end positions
        dyn = torch.zeros(slots, 8, dtype=torch.int32, device=dev)
        dyn[:, ops.DYN_BS], dyn[:, ops.DYN_START], dyn[:, ops.DYN_S] = 16, 1024, 1008
        st = ops.stop_seq_state(slots, dev)
        for s in range(slots):
            ops.stop_seq_set(st, s, never(V), first_pos=512)
        table = ops.penalty_state(slots, V, dev)
        gr = ops.grammar_state(slots, 1, V, dev)
        from dflash_amd import TokenDFA
        import numpy as np
        base = ops.grammar_load(gr, TokenDFA(np.zeros((1, V), dtype=np.int16), 0))
        for s in range(slots):
            ops.grammar_set(gr, s, base, 0)
        arms = {
            "stop_seq_rows": lambda i: ops.stop_seq_rows(block, post, ids, dyn, st),
            "grammar_advance": lambda i: ops.grammar_advance(gr, ids, dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START,
                                                             lo=1, hi=1),
            "penalty_count": lambda i: ops.penalty_count(table, ids, dyn=dyn, lo_word=ops.DYN_S, hi_word=ops.DYN_START,
                                                         lo=1, hi=1),
        }
        print(json.dumps({"part": 1, "slots": slots, "block": 16, "sequences": "8 x 16", "us": timed(arms, blocks=8)}),
              flush=True)
        assert int(dyn[:, ops.DYN_STOP].sum()) == 0 and bool((st.hit == -1).all())


def part_cycle(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, 1024), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = bench.tau_plan(2 + warmup, steps, bs, seed=100)
    need = sum(k + 1 for k in plan[:warmup + steps + 2]) + 2 * bs
    G = greedy_walk(perm, prompt, need + 2 * bs).to(dev)
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need,
                              max_block_size=bs, stop_token_ids=None, temperature=0.0, draft_token_hook=_hook(G, plan, V),
                              stop_sequences=never(V) if arm == "on" else None)
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
            assert not s.stopped
            del s
    print(json.dumps({"part": 2, "single_request_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v} for k, v in res.items()},
                      "mean_tau": taus, "steps": steps, "prefix": 1024, "block": bs, "T": 0.0, "sequences": "8 x 16"}),
          flush=True)


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
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            dec = BatchedDecoder(draft, target, 4, max_rows=max(lens) + need + 64, out_len=max(lens) + need + 32,
                                 mask_token_id=cfg.mask_token_id, stop_sequences=arm == "on")
            for r, p in enumerate(prompts):
                dec.admit(r, p, **(dict(stop_sequences=never(V)) if arm == "on" else {}))
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
    print(json.dumps({"part": 3, "four_request_ragged_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v}
                                                                   for k, v in res.items()},
                      "mean_tau": taus, "steps": steps, "prompts": lens, "block": bs, "T": 0.0, "sequences": "8 x 16"}),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=4)
    a = ap.parse_args()
    parts = {int(x) for x in a.parts.split(",") if x}
    dev = torch.device("cuda", 0)
    if 1 in parts:
        part_launch(dev)
    if parts & {2, 3}:
        import bench   # (the workload builders only; bench.py itself is not run)
        spec = bench.workload_spec("qwen3-8b")
        args = SimpleNamespace(target_layers=0, hf_verify=False, hf_prefill=False, attn_impl="head", fuse_oproj=False)
        target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
        if 2 in parts:
            part_cycle(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)
        if 3 in parts:
            part_batch(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)


if __name__ == "__main__":
    main()
