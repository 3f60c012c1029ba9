"""Same-box A/B of an MXFP4 native target against the fp8 and the bf16 target ("The target"),
Qwen3-8B shapes, prefix 1024, one process, the three forms alternating after a warm-up of each; median of `--runs` repeats
with the spread (min .. max) shown.  The claim under test is against the fp8 arm of the same run: the slowest mxfp4
repeat below the fastest fp8 repeat (`mxfp4_below_fp8_beyond_spread`).

Parts (each prints JSON lines):
  gemm     per-launch device time of the verify's launches at one 16-row tile in the row-source and epilogue forms the
           verify uses — q/k/v, o_proj, gate/up, down_proj (with the tap copy), the greedy head (dfl_gemm_argmax) and the
           sampled head (dfl_gemm_sample; the 4-bit form is k_gemm_s_w4); the weights rotate through > 600 MB of distinct
           buffers so that no launch is served from the Infinity Cache; bytes / time against 8 TB/s
  cycle    bench.py's N = 1 workload (bench.single_leg: DecodeSession, scripted acceptance, hipGraph replay) and its
           `batch4` workload (bench.batched_leg: four requests) with the SAME bf16 draft on a bf16, an fp8 and an mxfp4
           NativeTarget built from the same seeded weights: ms per cycle by wall clock, the verify phase from the event
           pairs of the instrumented cycles, and lossless_fraction (committed ids == the target's own greedy walk)

    timeout -k 10 1100 python scripts/bench_mxfp4_target.py --runs 5 > profiles/mxfp4_target_ab.txt
"""
from __future__ import annotations

import argparse
import gc
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

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
H, I, V, Q, KV = 4096, 12288, 151936, 4096, 1024
T = 0.7
FORMS = ("bf16", "fp8", "mxfp4")
BYTES = {"bf16": 2.0, "fp8": 1.0, "mxfp4": 0.5 + 1 / 32}     # streamed per weight (fp8: + 4 bytes per row, not counted)


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
    forms = {f: [] for f in FORMS}
    for _ in range(n_buf):
        forms["bf16"].append(torch.randn(N * K, device=dev, dtype=F32).to(BF16))
        codes = torch.randint(0, 0x78, (N * K,), device=dev, dtype=U8)     # finite, positive
        forms["fp8"].append(ops.Fp8Weight(codes, torch.full((N,), 2.0 ** -9, device=dev), N, K))
        blob = torch.randint(0, 256, (N * K // 2 + N * K // 32,), device=dev, dtype=U8)
        blob[N * K // 2:] = 118                                            # block scales 2^-9: scale codes inside 7..247
        forms["mxfp4"].append(ops.Mxfp4Weight(blob, N, K))
    return forms


def ab(name, N, K, launch, dev, runs):
    n_buf = max(2, int(600e6 // (N * K // 2)) + 1)       # > 600 MB of the SMALLEST form's bytes
    forms = weights(N, K, n_buf, dev)
    for wl in forms.values():        # warm-up of each form
        time_launches(lambda i: launch(wl[i]), n_buf)
    us = {f: [] for f in FORMS}
    for _ in range(runs):            # alternating
        for f, wl in forms.items():
            us[f].append(time_launches(lambda i: launch(wl[i]), n_buf))
    m = {f: med(us[f]) for f in FORMS}
    out(part="gemm", gemm=name, N=N, K=K, buffers=n_buf, us=m,
        frac_of_8TBps={f: N * K * BYTES[f] / (m[f]["median"] * 1e-6) / 8e12 for f in FORMS},
        mxfp4_over_fp8=m["mxfp4"]["median"] / m["fp8"]["median"], mxfp4_over_bf16=m["mxfp4"]["median"] / m["bf16"]["median"],
        mxfp4_below_fp8_beyond_spread=m["mxfp4"]["max"] < m["fp8"]["min"])
    del forms
    torch.cuda.empty_cache()


def part_gemm(dev, runs):
    dyn = torch.zeros(8, dtype=torch.int32, device=dev)
    ops.set_dyn(dyn, 1024, 16, 16, 1024)

    def normed(K):
        h = torch.randn(16, K, device=dev).to(BF16)
        return ops.rows_normed(h, torch.rand(K, device=dev) * 16, K // 16, torch.ones(K, device=dev, dtype=BF16), 1e-6,
                               ops.DYN_BS)

    def frag(K):
        return ops.rows_frag(torch.randn(16 * K, device=dev).to(BF16))

    hbuf = torch.zeros(16, Q + 2 * KV, dtype=BF16, device=dev)
    tap = torch.zeros(16, H, dtype=BF16, device=dev)
    ss = torch.zeros(H, device=dev)
    act = torch.zeros(16 * I, dtype=BF16, device=dev)
    ids = torch.zeros(16, dtype=torch.long, device=dev)
    aws = ops.argmax_ws(dev)
    cases = [   # (name, N, K, launch(w)): the forms NativeTarget.verify launches
        ("qkv", Q + 2 * KV, H, lambda w, x=normed(H): ops.gemm_resid(w, x, Q + 2 * KV, H, hbuf, add_residual=False, dyn=dyn)),
        ("o_proj", H, Q, lambda w, x=frag(Q): ops.gemm_resid(w, x, H, Q, hbuf[:, :H], add_residual=True, ss_out=ss, dyn=dyn)),
        ("gate_up", 2 * I, H, lambda w, x=normed(H): ops.gemm_silu_mul(w, x, I, H, act, dyn)),
        ("down_proj", H, I, lambda w, x=frag(I): ops.gemm_resid(w, x, H, I, hbuf[:, :H], add_residual=True, ss_out=ss, tap=tap, dyn=dyn)),
        ("lm_head_greedy", V, H, lambda w, x=normed(H): ops.gemm_argmax(w, x, V, H, 0, 16, aws, ids, 0, dyn=dyn)),
        ("lm_head_sampled", V, H, lambda w, x=normed(H): ops.gemm_sample(w, x, V, H, 0, 16, aws, ids, 0, seed=5, temperature=T,
                                                                         pos_dyn=dyn, pos_word=ops.DYN_POS0, pos_add=1, dyn=dyn)),
    ]
    for name, N, K, launch in cases:
        ab(name, N, K, launch, dev, runs)


def build_targets(args, spec, dev):
    """bench.build_models' bf16 target and draft, and an fp8 and an mxfp4 NativeTarget over the same seeded HF weights."""
    from dflash_amd import NativeTarget
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    forms = {"bf16": target}
    for f, fmt in (("fp8", "fp8_e4m3"), ("mxfp4", "mxfp4")):
        torch.manual_seed(0)                                     # (as build_models: the same HF init and the same walk)
        hf, p2 = bench.make_hf_target(spec, dev, meta["layers"])
        assert torch.equal(p2, perm)
        forms[f] = NativeTarget(hf, attn_impl="head", keep_hf=False, prefill="native", weight_format=fmt)
        del hf
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    t4 = forms["mxfp4"]
    assert t4.streams_mxfp4(16) and t4.streams_mxfp4_tiles() and forms["fp8"].streams_fp8(16) and not target.streams_mxfp4(16)
    packed = sum(w.numel() * 2 for lw in t4.layers for k, w in lw.items() if k in ("qkv", "o", "gu", "down")) + V * H * 2
    codes = sum(t.numel() for t in t4.mxfp4_tensors())
    out(part="cycle", packed_bf16_bytes=packed, mxfp4_blob_bytes=codes, mxfp4_target_over_bf16_target_bytes=(packed + codes) / packed)
    return forms, draft, cfg, perm, meta


def part_cycle(dev, runs, steps, warmup):
    args = SimpleNamespace(steps=steps, warmup=warmup, prefix=1024, temperature=None, schedule=None, event_every=4,
                           target_layers=0, hf_verify=False, hf_prefill=False, eager=False, attn_impl="head",
                           fuse_oproj=False, full=False, workload="qwen3-8b")
    spec = bench.workload_spec("qwen3-8b")
    forms, draft, cfg, perm, meta = build_targets(args, spec, dev)
    legs = {1: lambda t: bench.single_leg(args, spec, 0, dev, t, draft, cfg, perm, meta),
            4: lambda t: bench.batched_leg(args, 0, dev, draft, t, perm, cfg, meta, 4)}
    for n, leg in legs.items():
        for t in forms.values():             # warm-up of each form
            leg(t)
        cyc, ver, drf, loss = ({f: [] for f in FORMS} for _ in range(4))
        for _ in range(runs):
            for f, t in forms.items():
                r = leg(t)
                loss[f].append(r["lossless_fraction"])
                cyc[f].append(1e3 * r["dt"] / (r["cycles"] if n == 1 else r["steps"]))
                ver[f].append(r["hot_path"]["target_verify_ms_per_cycle"])
                drf[f].append(r["hot_path"]["draft_plus_lm_head_ms_per_cycle"])
        for what, d in (("ms_per_cycle", cyc), ("verify_phase_ms_event_pair", ver), ("draft_phase_ms_event_pair", drf)):
            m = {f: med(d[f]) for f in FORMS}
            out(part="cycle", requests=n, what=what, steps=steps, ms=m, mxfp4_over_fp8=m["mxfp4"]["median"] / m["fp8"]["median"],
                mxfp4_over_bf16=m["mxfp4"]["median"] / m["bf16"]["median"],
                mxfp4_below_fp8_beyond_spread=m["mxfp4"]["max"] < m["fp8"]["min"],
                lossless_fraction={f: min(v) for f, v in loss.items()})


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
