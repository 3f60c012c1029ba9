"""Same-box A/B of the two T > 0 samplers on BASELINE configs[3]'s workload (Llama-3.1-8B shapes, T = 0.7, prefix 1024,
block 16, bench.py's scripted acceptance): sampler="torch" with eager cycles — what bench.py runs, its replay needs
T < 1e-5 — against sampler="device" with the cycles replayed from hipGraphs; the arm
"device_filtered" is the device arm with top_k=50, top_p=0.9 (the materialise + dfl_sample_rows_nucleus path; the plain
device arm's launch sequence is the one from before that path existed).  The arms alternate,
`--runs` timed runs each, on one set of models in one process; one JSON line per run, then a summary line.

    timeout -k 10 900 python scripts/sampler_ab.py --runs 3 --steps 48
    timeout -k 10 900 python scripts/sampler_ab.py --runs 3 --steps 48 --arms device,device_filtered
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
import bench  # noqa: E402  (the workload builders only; bench.py itself is not run)


def one_run(arm, draft, target, cfg, perm, V, P, steps, warmup, temperature, seed):
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = bench.tau_plan(2 + warmup, steps, bs, seed=100)
    need = sum(k + 1 for k in plan[:warmup + steps + 2]) + 2 * bs
    G = greedy_walk(perm, prompt, need + 2 * bs).to(dev)

    def hook(blk, start, call):   # k agreeing tokens of the walk, then one that is not (bench.py's scripted acceptance)
        k = min(plan[call], blk.shape[1] - 1)
        if k > 0:
            blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % (V - 1000)

    device = arm in ("device", "device_filtered")
    flt = dict(top_k=50, top_p=0.9) if arm == "device_filtered" else {}
    s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need, max_block_size=bs,
                      stop_token_ids=None, temperature=temperature, draft_token_hook=hook,
                      sampler="device" if device else "torch", seed=seed if device else None, **flt)
    s.prefill()
    s.cycle(bs)
    for _ in range(1 + warmup):
        s.cycle(bs, ahead_ok=True)
    if device:
        s.capture(bs)
    torch.cuda.synchronize()
    s.host_times = []
    taus = []
    t0 = time.perf_counter()
    for _ in range(steps):
        taus.append((s.cycle_graph(bs) if device else s.cycle(bs, ahead_ok=True)).tau)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ht = s.host_times
    return {"arm": arm, "ms_per_cycle": 1e3 * dt / steps, "mean_tau": sum(taus) / len(taus),
            "host_enqueue_ms": 1e3 * sum(a for a, _ in ht) / len(ht), "host_wait_ms": 1e3 * sum(b for _, b in ht) / len(ht),
            "tokens_per_s": sum(taus) / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--prefix", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--arms", default="torch,device", help="comma list: run only these arms (a profiler run takes one)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    spec = bench.workload_spec("llama31-8b")
    args = SimpleNamespace(target_layers=0, hf_verify=False, hf_prefill=False, attn_impl="head", fuse_oproj=False)
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    T = spec["temperature"]
    rows = []
    arms = [x for x in a.arms.split(",") if x]
    for i in range(a.runs):
        for arm in (arms if i % 2 == 0 else arms[::-1]):
            r = one_run(arm, draft, target, cfg, perm, meta["V"], a.prefix, a.steps, a.warmup, T, a.seed)
            r["run"] = i
            rows.append(r)
            print(json.dumps(r), flush=True)
    summ = {}
    for arm in arms:
        ms = sorted(r["ms_per_cycle"] for r in rows if r["arm"] == arm)
        summ[arm] = {"ms_per_cycle_median": ms[len(ms) // 2], "ms_per_cycle_all": ms,
                     "host_enqueue_ms_median": sorted(r["host_enqueue_ms"] for r in rows if r["arm"] == arm)[len(ms) // 2]}
    print(json.dumps({"summary": summ, "temperature": T, "workload": "llama31-8b", "prefix": a.prefix, "steps": a.steps}))


if __name__ == "__main__":
    main()
