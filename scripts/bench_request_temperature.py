"""Cost of the per-request temperature ("Per-request temperature"), one process, arms alternating.

  lm_head   the ring-form lm_head at four request tiles, K = 4096, V = 151936 / 128256: dfl_gemm_sample_batch (inv_ts given) with
            (i) uniform sampled inv_ts, (ii) mixed (sampled, greedy, sampled, greedy), (iii) all greedy, against
            dfl_gemm_sample_batch at one host invT and dfl_gemm_argmax_batch; median of 10 blocks of 50 launches (GEMM plus finish kernel),
            the order of the arms rotating from block to block, and each arm's own spread over its blocks
  cycle     scripts/stream_ab.py's steady four-request cycle on Qwen3-8B shapes, every request at T = 0.7 with
            sampler="device": an engine built with request_temperature=True against one built without it

    timeout -k 10 600 python scripts/bench_request_temperature.py > profiles/request_temperature_ab.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from dflash_amd import ops  # noqa: E402

T = 0.7


def frag16(x: torch.Tensor) -> torch.Tensor:
    """[MT, 16, K] rows -> the frag16 operand layout, through the library's own packer."""
    MT, _, K = x.shape
    out = torch.empty(MT, 16 * K, dtype=torch.bfloat16, device=x.device)
    for t in range(MT):
        ops.pack_rows(x[t], 16, out[t])
    return out


def part_lm_head(dev):
    K, R = 4096, 4
    for V in (151936, 128256):
        g = torch.Generator(device=dev).manual_seed(V)
        wp = ops.pack_weight((torch.randn(V, K, generator=g, device=dev) * 0.02).to(torch.bfloat16))
        src = ops.brows_frag(frag16(torch.randn(R, 16, K, generator=g, device=dev).to(torch.bfloat16)))
        gws = torch.zeros(ops.lib().dfl_gemm_batch_ws_bytes(V, K), dtype=torch.uint8, device=dev)
        ids = torch.zeros(R, 16, dtype=torch.int64, device=dev)
        rec = torch.tensor([[0, 0, 16, 1000 + 97 * t, 1000, 0, 0, 0] for t in range(R)], dtype=torch.int32, device=dev)
        seeds = torch.arange(1, R + 1, dtype=torch.int64, device=dev)
        it = ops.inv_temperature(T)
        inv = {"t_uniform": [it] * 4, "t_mixed": [it, 0.0, it, 0.0], "t_greedy": [0.0] * 4}
        inv = {k: torch.tensor(v, dtype=torch.float32, device=dev) for k, v in inv.items()}
        kw = dict(seeds=seeds, pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=1, nrows_dyn_word=ops.DYN_BS)
        launch = {"argmax": lambda: ops.gemm_argmax_batch(wp, src, R, V, K, 0, 16, gws, ids, 0, rec, nrows_dyn_word=ops.DYN_BS),
                  "sample": lambda: ops.gemm_sample_batch(wp, src, R, V, K, 0, 16, gws, ids, 0, rec, temperature=T, **kw)}
        for name, arr in inv.items():
            launch[name] = lambda arr=arr: ops.gemm_sample_batch(wp, src, R, V, K, 0, 16, gws, ids, 0, rec, inv_ts=arr, **kw)
        names = list(launch)
        res = {k: [] for k in names}
        for _ in range(20):
            for k in names:
                launch[k]()
        for rep in range(10):
            for k in names[rep % len(names):] + names[:rep % len(names)]:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(50):
                    launch[k]()
                b.record()
                b.synchronize()
                res[k].append(1e3 * a.elapsed_time(b) / 50)
        med = {k: statistics.median(v) for k, v in res.items()}
        print(json.dumps({"part": "lm_head", "V": V, "K": K, "tiles": R, "us_median": med,
                          "us_spread": {k: max(v) - min(v) for k, v in res.items()}, "us_all": res,
                          "t_uniform_minus_sample_us": med["t_uniform"] - med["sample"],
                          "t_greedy_minus_argmax_us": med["t_greedy"] - med["argmax"]}), flush=True)


def part_cycle(dev, runs, steps=24, warm=4):
    import bench
    import stream_ab as S
    from types import SimpleNamespace
    from dflash_amd.engine import BatchEngine
    from dflash_amd.synthetic import greedy_walk
    spec = bench.workload_spec("qwen3-8b")
    args = SimpleNamespace(target_layers=0, hf_verify=False, hf_prefill=False, attn_impl="head", fuse_oproj=False)
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    V, BS, P = meta["V"], S.BS, 1024
    new = (steps + warm + 4) * BS * 2
    prompts = [torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(1 + r)).to(dev) for r in range(4)]
    plans = [bench.tau_plan(2 + warm, steps, BS, seed=100 + r, extra=2 * (steps + warm)) for r in range(4)]
    Gs = [greedy_walk(perm, p, new + 2 * BS).to(dev) for p in prompts]
    hooks = [S.make_hook(Gs[r], plans[r], V) for r in range(4)]
    rows = {"engine": [], "engine_request_temperature": []}
    for r in range(runs):
        for form in (list(rows) if r % 2 == 0 else list(rows)[::-1]):
            flag = form != "engine"
            eng = BatchEngine(draft, target, slots=4, max_rows=P + new + 3 * BS, out_len=P + new + BS,
                              mask_token_id=cfg.mask_token_id, temperature=T, sampler="device", request_temperature=flag)
            for i, p in enumerate(prompts):
                eng.submit(p, new, seed=11 + i, draft_token_hook=hooks[i], **(dict(temperature=T) if flag else {}))
            eng.step()
            for _ in range(warm):
                eng.step()
            t0 = S.sync_time()
            for _ in range(steps):
                eng.step()
            ms = 1e3 * (S.sync_time() - t0) / steps
            assert eng.stats["captures"] == 1 and eng.stats["replayed_cycles"] == steps + warm
            rows[form].append(ms)
            print(json.dumps({"part": "cycle", "form": form, "run": r, "ms_per_group_cycle": ms}), flush=True)
            eng = None
    print(json.dumps({"part": "cycle", "summary": True, "T": T, "ms_median": {k: statistics.median(v) for k, v in rows.items()},
                      "ms_spread": {k: max(v) - min(v) for k, v in rows.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="lm_head,cycle")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    for name in a.part.split(","):
        if name == "lm_head":
            part_lm_head(dev)
        else:
            part_cycle(dev, a.runs)


if __name__ == "__main__":
    main()
