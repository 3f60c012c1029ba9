"""Same-box A/B of the FP8 (e4m3) draft weights against the bf16 draft in the RAGGED BATCH ("The
batch forms"), Qwen3-8B shapes, one process, both forms alternating after a warm-up of each; median of `--runs` repeats
with the spread (min .. max) shown.

Parts (each prints JSON lines):
  gemm     per-launch device time of the six draft launches of a batch cycle that have an fp8 form — kv_all, q/k/v parts,
           o_proj, down_proj (dfl_gemm_f32_batch), gate/up (ring, SiLU) and lm_head (ring, argmax) — at 4 request tiles
           and at 2, bf16 against fp8; the weights rotate through > 600 MB of distinct buffers so that no launch is
           served from the Infinity Cache; bytes / time against 8 TB/s
  cycle    bench.py's `batch4` workload (bench.batched_leg: four requests, scripted acceptance, hipGraph replay) with the
           bf16 draft and with the fp8 draft on the SAME bf16 target: ms per group cycle by wall clock over the replayed
           steps, and the draft phase / the lm_head launch pair from the event pairs of the instrumented cycles
  lm_head  `--part lm_head --launches K`: K launches of the fp8 ring lm_head at 4 tiles and nothing else, for a counter run
           of its own (rocprofv3 --pmc FETCH_SIZE -- python scripts/bench_fp8_batch.py --part lm_head)

    timeout -k 10 900 python scripts/bench_fp8_batch.py --runs 5 > profiles/fp8_batch_ab.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload builders only; bench.py itself is not run)

from dflash_amd import ops  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
H, I, V, L, Q, KV = 4096, 12288, 151936, 5, 4096, 1024


def out(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def time_launches(fn, n_buf):
    """device microseconds per launch over one pass through the n_buf weight buffers"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n_buf):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n_buf * 1e3


def weights(N, K, n_buf, dev):
    """n_buf packed weights of N x K per form with arbitrary finite contents (the time does not depend on the values)"""
    b16 = [torch.randn(N * K, device=dev, dtype=F32).to(BF16) for _ in range(n_buf)]
    f8 = []
    for _ in range(n_buf):
        codes = torch.randint(0, 0x78, (N * K,), device=dev, dtype=torch.uint8)     # finite, positive
        f8.append(ops.Fp8Weight(codes, torch.full((N,), 2.0 ** -9, device=dev), N, K))
    return b16, f8


def part_gemm(dev, runs):
    for R in (4, 2):
        MT = ops.batch_tiles(R)
        dyn = torch.zeros(MT, 8, dtype=torch.int32, device=dev)
        dyn[:, ops.DYN_TAU], dyn[:, ops.DYN_BS] = 16, 16

        def frag(K):
            return ops.brows_frag(torch.randn(MT, 16 * K, device=dev).to(BF16))

        part = torch.zeros(ops.batch_ksplit(I) * MT * 16 * max(H, L * 2 * KV, Q + 2 * KV), dtype=F32, device=dev)
        act = torch.zeros(MT, 16 * I, dtype=BF16, device=dev)
        ids = torch.zeros(MT, 16, dtype=torch.long, device=dev)
        gws = ops.gemm_batch_ws(max(V, 2 * I), H, dev)

        def f32(N, K):
            return lambda w, x=frag(K): ops.gemm_f32_batch(w, x, R, N, K, part, dyn)

        cases = [   # (name, N, K, launch(w))
            ("kv_all", L * 2 * KV, H, f32(L * 2 * KV, H)),
            ("qkv_parts", Q + 2 * KV, H, f32(Q + 2 * KV, H)),
            ("o_proj", H, Q, f32(H, Q)),
            ("gate_up", 2 * I, H, lambda w, x=frag(H): ops.gemm_silu_mul_batch(w, x, R, I, H, act, gws, dyn)),
            ("down_proj", H, I, f32(H, I)),
            ("lm_head", V, H, lambda w, x=frag(H): ops.gemm_argmax_batch(w, x, R, V, H, 1, 15, gws, ids, 1, dyn,
                                                                          nrows_dyn_word=ops.DYN_BS)),
        ]
        for name, N, K, launch in cases:
            n_buf = max(2, int(600e6 // (N * K)) + 1)
            b16, f8 = weights(N, K, n_buf, dev)
            forms = {"bf16": b16, "fp8": f8}
            for wl in forms.values():        # warm-up of each form
                time_launches(lambda i: launch(wl[i]), n_buf)
            us = {"bf16": [], "fp8": []}
            for _ in range(runs):            # alternating
                for f, wl in forms.items():
                    us[f].append(time_launches(lambda i: launch(wl[i]), n_buf))
            mb, m8 = med(us["bf16"]), med(us["fp8"])
            # faster by more than the spread: the slowest fp8 repeat beats the fastest bf16 repeat
            out(part="gemm", tiles=R, gemm=name, N=N, K=K, buffers=n_buf, bf16_us=mb, fp8_us=m8,
                bf16_frac_of_8TBps=N * K * 2 / (mb["median"] * 1e-6) / 8e12,
                fp8_frac_of_8TBps=N * K / (m8["median"] * 1e-6) / 8e12, fp8_over_bf16=m8["median"] / mb["median"],
                faster_beyond_spread=m8["max"] < mb["min"])
            del b16, f8, forms
            torch.cuda.empty_cache()


def part_cycle(dev, runs, steps, warmup):
    from dflash_amd import DFlashDraftModel
    args = SimpleNamespace(steps=steps, warmup=warmup, prefix=1024, temperature=None, schedule=None, event_every=4,
                           target_layers=0, hf_verify=False, hf_prefill=False, eager=False, attn_impl="head",
                           fuse_oproj=False, full=False, workload="qwen3-8b")
    spec = bench.workload_spec("qwen3-8b")
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    g = torch.Generator(device=dev).manual_seed(0)       # bench.build_models' draft weights, drawn again
    sd = {k: (torch.randn(s, generator=g, device=dev, dtype=F32) * 0.02).to(BF16)
          if len(s) == 2 else torch.ones(s, device=dev, dtype=BF16) for k, s in cfg.state_dict_shapes().items()}
    draft8 = DFlashDraftModel(cfg, device=dev, weight_format="fp8_e4m3")
    draft8.load_state_dict(sd)
    del sd
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert draft8.streams_fp8_tiles() and not draft.streams_fp8_tiles()
    forms = {"bf16": draft, "fp8": draft8}
    for d in forms.values():             # warm-up of each form
        bench.batched_leg(args, 0, dev, d, target, perm, cfg, meta, 4)
    cyc, drf, lm = {"bf16": [], "fp8": []}, {"bf16": [], "fp8": []}, {"bf16": [], "fp8": []}
    for _ in range(runs):
        for f, d in forms.items():
            r = bench.batched_leg(args, 0, dev, d, target, perm, cfg, meta, 4)
            assert r["lossless_fraction"] == 1.0, (f, r["lossless_fraction"])
            cyc[f].append(1e3 * r["dt"] / r["steps"])
            drf[f].append(r["hot_path"]["draft_plus_lm_head_ms_per_cycle"])
            lm[f].append(r["roofline"]["avg_ms"])
    for what, d in (("ms_per_group_cycle", cyc), ("draft_phase_ms_event_pair", drf), ("lm_head_ms_event_pair", lm)):
        mb, m8 = med(d["bf16"]), med(d["fp8"])
        out(part="cycle", requests=4, what=what, steps=steps, bf16=mb, fp8=m8, fp8_over_bf16=m8["median"] / mb["median"],
            faster_beyond_spread=m8["max"] < mb["min"], lossless_fraction=1.0)


def part_lm_head(dev, launches):
    R, MT = 4, 4
    dyn = torch.zeros(MT, 8, dtype=torch.int32, device=dev)
    dyn[:, ops.DYN_BS] = 16
    _, f8 = weights(V, H, 2, dev)
    x = ops.brows_frag(torch.randn(MT, 16 * H, device=dev).to(BF16))
    ids = torch.zeros(MT, 16, dtype=torch.long, device=dev)
    gws = ops.gemm_batch_ws(V, H, dev)
    for i in range(launches):
        ops.gemm_argmax_batch(f8[i % 2], x, R, V, H, 1, 15, gws, ids, 1, dyn, nrows_dyn_word=ops.DYN_BS)
    torch.cuda.synchronize()
    out(part="lm_head", tiles=R, launches=launches, algorithmic_bytes_per_launch=V * H)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gemm", "cycle", "lm_head", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--launches", type=int, default=8)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.part in ("gemm", "all"):
        part_gemm(dev, a.runs)
    if a.part in ("cycle", "all"):
        part_cycle(dev, a.runs, a.steps, a.warmup)
    if a.part == "lm_head":
        part_lm_head(dev, a.launches)
