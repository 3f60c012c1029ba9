"""What min_p costs.

1. The dfl_min_p_rows launch at 16 x 151936 and 16 x 128256 (a slot at 0.1, and an off slot's plain copy), beside
   dfl_logit_bias_rows and dfl_sample_rows_nucleus (top_p = 0.9, and filters off) on the same rows in the same process:
   points of comparison, not a bar.  The logits rotate through enough buffers to exceed L2 and the 256 MB MALL, so every
   launch reads HBM; HIP events around blocks of launches, the arms alternating, median of 5 blocks (min .. max).
2. The single-request cycle (Qwen3-8B shapes, prefix 1024, block 16, T = 0.7, top_p = 0.9, replayed) without / with
   min_p = 0.1, the arms alternating.
3. The four-request ragged cycle (prompts 1024 / 768 / 512 / 896, replayed) at T = 0.7 and top_p = 0.9, the decoder built
   without / with min_p (every slot at 0.1), the arms alternating.
The walk target's margin is ~80: both arms accept the same tokens.

    timeout -k 10 900 python scripts/bench_min_p.py [--parts 1,2,3]
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

T, TOP_P, MIN_P = 0.7, 0.9, 0.1


def part_launch(dev):
    for V in (151936, 128256):
        g = torch.Generator(device=dev).manual_seed(V)
        nbuf = (320 << 20) // (16 * V * 2) + 1          # > 256 MB MALL + L2
        lg = (torch.randn(nbuf, 16, V, generator=g, device=dev) * 2).to(torch.bfloat16)
        out = torch.empty(16, V, dtype=torch.bfloat16, device=dev)
        post = torch.zeros(16, dtype=torch.int64, device=dev)
        kept = torch.zeros(16, dtype=torch.int32, device=dev)
        pick = torch.randperm(V, generator=torch.Generator().manual_seed(V))[:3000].tolist()
        b, _ = ops.check_logit_bias(V, {v: (2.0 if i % 2 else -2.0) for i, v in enumerate(pick[:2000])}, None, pick[2000:])
        st = ops.logit_bias_state(1, V, dev)
        ops.logit_bias_set(st, 0, b, 0)
        arms = {
            "min_p_rows": lambda i: ops.min_p_rows(lg[i % nbuf], min_p=MIN_P, temperature=T, out=out, kept=kept),
            "min_p_rows_off_slot_copy": lambda i: ops.min_p_rows(lg[i % nbuf], min_p=0, temperature=T, out=out),
            "logit_bias_rows": lambda i: ops.logit_bias_rows(lg[i % nbuf], st.bias, out=out, out_ids=post, pos_base=100),
            "sample_rows_nucleus_top_p": lambda i: ops.sample_rows_nucleus(lg[i % nbuf], temperature=T, top_p=TOP_P, seed=7,
                                                                           pos_base=100, out=post),
            "sample_rows_nucleus_filters_off": lambda i: ops.sample_rows_nucleus(lg[i % nbuf], temperature=T, seed=7,
                                                                                 pos_base=100, out=post),
        }
        print(json.dumps({"part": 1, "V": V, "rows": 16, "buffers": nbuf, "us": timed(arms, blocks=5)}), flush=True)
        del lg


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
                              max_block_size=bs, stop_token_ids=None, temperature=T, draft_token_hook=_hook(G, plan, V),
                              sampler="device", seed=11, top_p=TOP_P, min_p=MIN_P if arm == "on" else None)
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
    print(json.dumps({"part": 2, "single_request_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v} for k, v in res.items()},
                      "mean_tau": taus, "steps": steps, "prefix": 1024, "block": bs, "T": T, "top_p": TOP_P, "min_p": MIN_P}),
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
                                 mask_token_id=cfg.mask_token_id, temperature=T, sampler="device", filtering=True,
                                 min_p=arm == "on")
            for r, p in enumerate(prompts):
                dec.admit(r, p, T, seed=20 + r, top_p=TOP_P, **(dict(min_p=MIN_P) if arm == "on" else {}))
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
                      "mean_tau": taus, "steps": steps, "prompts": lens, "block": bs, "T": T, "top_p": TOP_P, "min_p": MIN_P}),
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
