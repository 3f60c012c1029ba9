"""Same-box A/B of the MXFP4 draft weights against the bf16 and the e4m3 draft in the RAGGED BATCH (DESIGN.md section 17,
"The batch forms"), after scripts/bench_fp8_batch.py, whose timing helpers it uses.  One JSON line per result.

  gemm     per-launch device time of the six draft launches of a batch cycle at the 8B shapes, at 4 request tiles and at
           2: bf16 / fp8 / mxfp4 alternating in one process after a warm-up of each, the weights rotating through
           > 600 MB of distinct buffers per form; median of --runs with min .. max.  `beats_fp8_beyond_spread`: the slowest
           mxfp4 repeat beats the fastest fp8 repeat of the same run.
  cycle    bench.py's batched leg (4 requests, prefix 1024, graph replay) with the three drafts on the SAME bf16 target: ms
           per group cycle by wall clock, the draft phase and the lm_head by event pairs; lossless_fraction is asserted.

    timeout -k 10 900 python scripts/bench_mxfp4_batch.py --runs 5 > profiles/mxfp4_batch_ab.txt
"""
from __future__ import annotations

import argparse
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_fp8_batch as F8  # noqa: E402  (puts the repository root on the path and imports bench)

from dflash_amd import ops  # noqa: E402

bench, out, med, time_launches = F8.bench, F8.out, F8.med, F8.time_launches
BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
H, I, V, L, Q, KV = F8.H, F8.I, F8.V, F8.L, F8.Q, F8.KV
FORMS = ("bf16", "fp8", "mxfp4")
BYTES = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1 / 32}


def weights4(N, K, n_buf, dev):
    """n_buf Mxfp4Weights of N x K: random codes under scale codes 118 .. 121 (the time does not depend on the values)"""
    w4 = []
    for _ in range(n_buf):
        blob = torch.randint(0, 256, (N * K // 2 + N * K // 32,), device=dev, dtype=U8)
        blob[N * K // 2:] = torch.randint(118, 122, (N * K // 32,), device=dev, dtype=U8)
        w4.append(ops.Mxfp4Weight(blob, N, K))
    return w4


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

        cases = [("kv_all", L * 2 * KV, H, f32(L * 2 * KV, H)), ("qkv_parts", Q + 2 * KV, H, f32(Q + 2 * KV, H)),
                 ("o_proj", H, Q, f32(H, Q)),
                 ("gate_up", 2 * I, H, lambda w, x=frag(H): ops.gemm_silu_mul_batch(w, x, R, I, H, act, gws, dyn)),
                 ("down_proj", H, I, f32(H, I)),
                 ("lm_head", V, H, lambda w, x=frag(H): ops.gemm_argmax_batch(w, x, R, V, H, 1, 15, gws, ids, 1, dyn,
                                                                               nrows_dyn_word=ops.DYN_BS))]
        for name, N, K, launch in cases:
            n_buf = max(2, int(600e6 // (N * K)) + 1)
            b16, f8 = F8.weights(N, K, n_buf, dev)
            forms = {"bf16": b16, "fp8": f8, "mxfp4": weights4(N, K, n_buf, dev)}
            for wl in forms.values():        # warm-up of each form
                time_launches(lambda i: launch(wl[i]), n_buf)
            us = {f: [] for f in FORMS}
            for _ in range(runs):            # alternating
                for f, wl in forms.items():
                    us[f].append(time_launches(lambda i: launch(wl[i]), n_buf))
            m = {f: med(us[f]) for f in FORMS}
            out(part="gemm", tiles=R, gemm=name, N=N, K=K, buffers=n_buf, us=m,
                frac_of_8TBps={f: N * K * BYTES[f] / (m[f]["median"] * 1e-6) / 8e12 for f in FORMS},
                mxfp4_over_bf16=m["mxfp4"]["median"] / m["bf16"]["median"], mxfp4_over_fp8=m["mxfp4"]["median"] / m["fp8"]["median"],
                beats_fp8_beyond_spread=m["mxfp4"]["max"] < m["fp8"]["min"], beats_bf16_beyond_spread=m["mxfp4"]["max"] < m["bf16"]["min"])
            del b16, f8, forms
            torch.cuda.empty_cache()


def part_cycle(dev, runs, steps, warmup):
    from dflash_amd import DFlashDraftModel
    args = SimpleNamespace(steps=steps, warmup=warmup, prefix=1024, temperature=None, schedule=None, event_every=4,
                           target_layers=0, hf_verify=False, hf_prefill=False, eager=False, attn_impl="head",
                           fuse_oproj=False, full=False, workload="qwen3-8b")
    spec = bench.workload_spec("qwen3-8b")
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    forms = {"bf16": draft}
    for f, fmt in (("fp8", "fp8_e4m3"), ("mxfp4", "mxfp4")):
        g = torch.Generator(device=dev).manual_seed(0)       # bench.build_models' draft weights, drawn again
        sd = {k: (torch.randn(s, generator=g, device=dev, dtype=F32) * 0.02).to(BF16)
              if len(s) == 2 else torch.ones(s, device=dev, dtype=BF16) for k, s in cfg.state_dict_shapes().items()}
        forms[f] = DFlashDraftModel(cfg, device=dev, weight_format=fmt).load_state_dict(sd)
        del sd
        torch.cuda.empty_cache()
    assert forms["mxfp4"].streams_mxfp4_tiles() and forms["fp8"].streams_fp8_tiles()
    for d in forms.values():             # warm-up of each form
        bench.batched_leg(args, 0, dev, d, target, perm, cfg, meta, 4)
    cyc, drf, lm = ({f: [] for f in FORMS} for _ in range(3))
    for _ in range(runs):
        for f, d in forms.items():
            r = bench.batched_leg(args, 0, dev, d, target, perm, cfg, meta, 4)
            assert r["lossless_fraction"] == 1.0, (f, r["lossless_fraction"])
            cyc[f].append(1e3 * r["dt"] / r["steps"])
            drf[f].append(r["hot_path"]["draft_plus_lm_head_ms_per_cycle"])
            lm[f].append(r["roofline"]["avg_ms"])
    for what, d in (("ms_per_group_cycle", cyc), ("draft_phase_ms_event_pair", drf), ("lm_head_ms_event_pair", lm)):
        m = {f: med(d[f]) for f in FORMS}
        out(part="cycle", requests=4, what=what, steps=steps, ms=m, mxfp4_over_bf16=m["mxfp4"]["median"] / m["bf16"]["median"],
            mxfp4_over_fp8=m["mxfp4"]["median"] / m["fp8"]["median"], beats_fp8_beyond_spread=m["mxfp4"]["max"] < m["fp8"]["min"],
            lossless_fraction=1.0)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gemm", "cycle", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.part in ("gemm", "all"):
        part_gemm(dev, a.runs)
    if a.part in ("cycle", "all"):
        part_cycle(dev, a.runs, a.steps, a.warmup)
