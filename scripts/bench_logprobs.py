"""What `logprobs=` costs.

1. The dfl_logprob_rows launch at 16 x 151936 and 16 x 128256 for n_top 0 and 8, beside dfl_sample_rows_nucleus
   (k_sample_rows_nucleus, top_k 50 / top_p 0.9) at the same shape: both read the same row once.  The logits rotate
   through enough buffers to exceed L2 and the 256 MB MALL, so every launch reads HBM; HIP events around blocks of
   launches, the arms alternating, min .. max over the blocks.
2. The lm_head launch (16 rows, K = 4096) with and without `logits=`.
3. The single-request cycle (Qwen3-8B shapes, prefix 1024, block 16, T = 0, replayed) with logprobs off / 0 / 8.
4. The four-request ragged cycle (prompts 1024 / 768 / 512 / 896, replayed) with logprobs off / 0 / 8.

    timeout -k 10 900 python scripts/bench_logprobs.py [--parts 1,2,3,4]
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


def timed(launch: dict, blocks: int = 8, per: int = 64) -> dict:
    """launch: name -> f(i), i counting launches (it picks the rotated buffer).  us per launch: min .. max over blocks."""
    res = {k: [] for k in launch}
    for f in launch.values():
        for i in range(8):
            f(i)
    names = list(launch)
    for rep in range(blocks):
        for k in (names if rep % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(per):
                launch[k](rep * per + i)
            b.record()
            b.synchronize()
            res[k].append(1e3 * a.elapsed_time(b) / per)
    return {k: {"min": round(min(v), 2), "median": round(sorted(v)[len(v) // 2], 2), "max": round(max(v), 2)}
            for k, v in res.items()}


def part_launch(dev):
    for V in (151936, 128256):
        g = torch.Generator(device=dev).manual_seed(V)
        nbuf = (320 << 20) // (16 * V * 2) + 1          # > 256 MB MALL + L2
        lg = (torch.randn(nbuf, 16, V, generator=g, device=dev) * 2).to(torch.bfloat16)
        ids = torch.randint(0, V, (16,), generator=g, device=dev)
        out = torch.zeros(16, dtype=torch.int64, device=dev)
        s0, s8 = ops.logprob_sink(1, 64, 0, dev), ops.logprob_sink(1, 64, 8, dev)
        arms = {
            "logprob_rows_n0": lambda i: ops.logprob_rows(lg[i % nbuf], ids, s0, pos_base=7),
            "logprob_rows_n8": lambda i: ops.logprob_rows(lg[i % nbuf], ids, s8, pos_base=7),
            "nucleus_k50_p0.9": lambda i: ops.sample_rows_nucleus(lg[i % nbuf], seed=1, temperature=0.7, top_k=50, top_p=0.9,
                                                                  pos_base=7, out=out),
            "nucleus_off": lambda i: ops.sample_rows_nucleus(lg[i % nbuf], seed=1, temperature=0.7, pos_base=7, out=out),
        }
        print(json.dumps({"part": 1, "V": V, "rows": 16, "buffers": nbuf, "us": timed(arms)}), flush=True)
        del lg


def part_head(dev):
    K = 4096
    for V in (151936, 128256):
        g = torch.Generator(device=dev).manual_seed(V)
        wp = ops.pack_weight((torch.randn(V, K, generator=g, device=dev) * 0.02).to(torch.bfloat16))
        src, ws = ops.rows_plain(torch.randn(16, K, generator=g, device=dev).to(torch.bfloat16)), ops.argmax_ws(dev)
        ids = torch.zeros(16, dtype=torch.int64, device=dev)
        buf = torch.zeros(16, V, dtype=torch.bfloat16, device=dev)
        s8 = ops.logprob_sink(1, 64, 8, dev)
        print(json.dumps({"part": 2, "V": V, "K": K, "us": timed({
            "gemm_argmax": lambda i: ops.gemm_argmax(wp, src, V, K, 0, 16, ws, ids, 0),
            "gemm_argmax_logits": lambda i: ops.gemm_argmax(wp, src, V, K, 0, 16, ws, ids, 0, logits=buf),
            "gemm_argmax_logits+logprob_rows_n8": lambda i: (ops.gemm_argmax(wp, src, V, K, 0, 16, ws, ids, 0, logits=buf),
                                                             ops.logprob_rows(buf, ids, s8, pos_base=7)),
        }, per=32)}), flush=True)
        del wp


def _hook(G, plan, V):
    def hook(blk, start, call):   # k agreeing tokens of the walk, then one that is not (bench.py's scripted acceptance)
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        if k > 0:
            blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % (V - 1000)
    return hook


def part_cycle(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, 1024), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = bench.tau_plan(2 + warmup, steps, bs, seed=100)
    need = sum(k + 1 for k in plan[:warmup + steps + 2]) + 2 * bs
    G = greedy_walk(perm, prompt, need + 2 * bs).to(dev)
    res = {}
    for rep in range(runs):
        for arm in ((None, 0, 8) if rep % 2 == 0 else (8, 0, None)):
            s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need,
                              max_block_size=bs, stop_token_ids=None, temperature=0.0, draft_token_hook=_hook(G, plan, V),
                              logprobs=arm)
            s.prefill()
            s.cycle(bs)
            for _ in range(1 + warmup):
                s.cycle(bs, ahead_ok=True)
            s.capture(bs)
            torch.cuda.synchronize()
            taus = []
            t0 = time.perf_counter()
            for _ in range(steps):
                taus.append(s.cycle_graph(bs).tau)
            torch.cuda.synchronize()
            res.setdefault(str(arm), []).append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
            del s
    print(json.dumps({"part": 3, "single_request_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v} for k, v in res.items()},
                      "steps": steps, "prefix": 1024, "block": bs}), flush=True)


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
    res = {}
    for rep in range(runs):
        for arm in ((None, 0, 8) if rep % 2 == 0 else (8, 0, None)):
            dec = BatchedDecoder(draft, target, 4, max_rows=max(lens) + need + 64, out_len=max(lens) + need + 32,
                                 mask_token_id=cfg.mask_token_id, logprobs=arm)
            for r, p in enumerate(prompts):
                dec.admit(r, p)
            for _ in range(1 + warmup):
                dec.cycle(hook)
            dec.capture()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                dec.cycle_graph(hook)
            torch.cuda.synchronize()
            res.setdefault(str(arm), []).append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
            del dec
    print(json.dumps({"part": 4, "four_request_ragged_cycle_ms": {k: {"min": min(v), "max": max(v), "all": v}
                                                                   for k, v in res.items()},
                      "steps": steps, "prompts": lens, "block": bs}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3,4")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    parts = {int(x) for x in a.parts.split(",") if x}
    dev = torch.device("cuda", 0)
    if 1 in parts:
        part_launch(dev)
    if 2 in parts:
        part_head(dev)
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
