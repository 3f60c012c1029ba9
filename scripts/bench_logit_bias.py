"""What logit bias / allow and ban lists / min_tokens cost.

1. The dfl_logit_bias_rows launch at 16 x 151936 and 16 x 128256 (a table with 2000 biases and 1000 bans; with and without
   two suppressed stop ids; in place), beside dfl_penalty_rows on the same rows, which moves the same bytes.  The logits
   rotate through enough buffers to exceed L2 and the 256 MB MALL, so every launch reads HBM; HIP events around blocks of
   launches, the arms alternating, min .. max over the blocks.
3. The single-request cycle (Qwen3-8B shapes, prefix 1024, block 16, T = 0, replayed) with the keywords off / on.
4. The four-request ragged cycle (prompts 1024 / 768 / 512 / 896, replayed) with the flag and the keywords off / on.
The on arm biases 2000 ids by +-2.0 (the walk target's margin is ~80), bans 1000 ids the scripted walk never visits and
suppresses two stop ids it never visits for the whole run (min_tokens = 10^6): both arms accept the same tokens.

    timeout -k 10 900 python scripts/bench_logit_bias.py [--parts 1,3,4]
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

PEN = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.25)


def part_launch(dev):
    for V in (151936, 128256):
        g = torch.Generator(device=dev).manual_seed(V)
        nbuf = (320 << 20) // (16 * V * 2) + 1          # > 256 MB MALL + L2
        lg = (torch.randn(nbuf, 16, V, generator=g, device=dev) * 2).to(torch.bfloat16)
        out = torch.empty(16, V, dtype=torch.bfloat16, device=dev)
        post = torch.zeros(16, dtype=torch.int64, device=dev)
        pick = torch.randperm(V, generator=torch.Generator().manual_seed(V))[:3000].tolist()
        b, _ = ops.check_logit_bias(V, {v: (2.0 if i % 2 else -2.0) for i, v in enumerate(pick[:2000])}, None, pick[2000:])
        st = ops.logit_bias_state(1, V, dev)
        ops.logit_bias_set(st, 0, b, 0)
        stop = torch.tensor([V - 5, V - 901], dtype=torch.int64, device=dev)
        ids = torch.randint(0, V, (1, 1200), generator=g, device=dev)
        table = ops.penalty_state(1, V, dev)
        ops.penalty_count(table, ids, lo=0, hi=1024, as_prompt=True, clear=True)
        ops.penalty_count(table, ids, lo=1024, hi=1200)
        block = ids[0, 1100:1116].contiguous()
        arms = {
            "logit_bias_rows": lambda i: ops.logit_bias_rows(lg[i % nbuf], st.bias, out=out, out_ids=post, pos_base=100),
            "logit_bias_rows_stop_suppressed": lambda i: ops.logit_bias_rows(lg[i % nbuf], st.bias, min_pos=10 ** 6,
                                                                             stop_ids=stop, out=out, out_ids=post, pos_base=100),
            "logit_bias_rows_in_place": lambda i: ops.logit_bias_rows(lg[i % nbuf], st.bias, out=lg[i % nbuf], pos_base=100),
            "penalty_rows": lambda i: ops.penalty_rows(lg[i % nbuf], table, block=block, out=out, out_ids=post, **PEN),
        }
        print(json.dumps({"part": 1, "V": V, "rows": 16, "buffers": nbuf, "us": timed(arms)}), flush=True)
        del lg


def _on_keywords(G, V):
    """The on arm's keywords for a scripted walk G: nothing the walk emits is touched by more than 2.0."""
    walk = set(G.tolist())
    free = [v for v in range(V) if v not in walk]
    return dict(logit_bias={v: (2.0 if i % 2 else -2.0) for i, v in enumerate(range(0, 4000, 2))},
                banned_token_ids=free[:1000], min_tokens=10 ** 6), free[1000:1002]


def part_cycle(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, 1024), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = bench.tau_plan(2 + warmup, steps, bs, seed=100)
    need = sum(k + 1 for k in plan[:warmup + steps + 2]) + 2 * bs
    G = greedy_walk(perm, prompt, need + 2 * bs).to(dev)
    on, stop = _on_keywords(G, V)
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need,
                              max_block_size=bs, stop_token_ids=stop, temperature=0.0, draft_token_hook=_hook(G, plan, V),
                              **(on if arm == "on" else {}))
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
    on, stop = _on_keywords(torch.cat(Gs), V)
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("off", "on") if rep % 2 == 0 else ("on", "off")):
            dec = BatchedDecoder(draft, target, 4, max_rows=max(lens) + need + 64, out_len=max(lens) + need + 32,
                                 mask_token_id=cfg.mask_token_id, stop_token_ids=stop, logit_bias=arm == "on")
            for r, p in enumerate(prompts):
                dec.admit(r, p, **(on if arm == "on" else {}))
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
