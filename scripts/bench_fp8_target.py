"""Same-box A/B of an FP8 (e4m3) native target against the bf16 target ("The target"), Qwen3-8B
shapes, prefix 1024, one process, both forms alternating after a warm-up of each; median of `--runs` repeats with the
spread (min .. max) shown.  The reference of every comparison is the bf16 arm of the same run.

Parts (each prints JSON lines):
  gemm     per-launch device time of the verify's launches at one 16-row tile in the row-source and epilogue forms the
           verify uses — q/k/v, o_proj, gate/up, down_proj (with the tap copy), the greedy head (dfl_gemm_argmax) and the
           sampled head (dfl_gemm_sample) — and of the sampled ring head at 4 request tiles (dfl_gemm_sample_batch, uniform
           and per-request temperature), bf16 against fp8; the weights rotate through > 600 MB of distinct buffers so
           that no launch is served from the Infinity Cache; bytes / time against 8 TB/s
  cycle    bench.py's N = 1 workload (bench.single_leg: DecodeSession, scripted acceptance, hipGraph replay) and its
           `batch4` workload (bench.batched_leg: four requests) with the SAME bf16 draft on a bf16 NativeTarget and on an
           fp8 NativeTarget built from the same seeded weights: ms per cycle by wall clock, the verify phase from the event
           pairs of the instrumented cycles, and lossless_fraction (committed ids == the target's own greedy walk)
  head     `--part head --launches K`: K launches of the sampled fp8 head (one tile) and K of the sampled fp8 ring head
           (4 tiles) and nothing else, for a counter run of its own
           (rocprofv3 --pmc FETCH_SIZE -- python scripts/bench_fp8_target.py --part head)

    timeout -k 10 900 python scripts/bench_fp8_target.py --runs 5 > profiles/fp8_target_ab.txt
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

BF16, F32 = torch.bfloat16, torch.float32
H, I, V, Q, KV = 4096, 12288, 151936, 4096, 1024
T = 0.7


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


def ab(name, N, K, launch, dev, runs, **tag):
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
    out(part="gemm", gemm=name, N=N, K=K, buffers=n_buf, bf16_us=mb, fp8_us=m8,
        bf16_frac_of_8TBps=N * K * 2 / (mb["median"] * 1e-6) / 8e12, fp8_frac_of_8TBps=N * K / (m8["median"] * 1e-6) / 8e12,
        fp8_over_bf16=m8["median"] / mb["median"], faster_beyond_spread=m8["max"] < mb["min"], **tag)
    del b16, f8, forms
    torch.cuda.empty_cache()


def ring_inputs(dev, R=4):
    MT = ops.batch_tiles(R)
    dyn = torch.zeros(MT, 8, dtype=torch.int32, device=dev)
    dyn[:, ops.DYN_BS], dyn[:, ops.DYN_POS0] = 16, 1024
    x = ops.brows_frag(torch.randn(MT, 16 * H, device=dev).to(BF16))
    ids = torch.zeros(MT, 16, dtype=torch.long, device=dev)
    seeds = torch.arange(3, 3 + MT, dtype=torch.int64, device=dev)
    inv = torch.tensor([ops.inv_temperature(t) if t > 0 else 0.0 for t in (0.7, 0.0, 1.3, 0.4)][:MT], dtype=F32, device=dev)
    return R, dyn, x, ids, seeds, inv, ops.gemm_batch_ws(V, H, dev)


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
        ab(name, N, K, launch, dev, runs, tiles=1)
    R, rdyn, x, rids, seeds, inv, gws = ring_inputs(dev)
    kw = dict(seeds=seeds, pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=1, nrows_dyn_word=ops.DYN_BS)
    ab("lm_head_sampled_ring", V, H, lambda w: ops.gemm_sample_batch(w, x, R, V, H, 0, 16, gws, rids, 0, rdyn, temperature=T, **kw),
       dev, runs, tiles=4)
    ab("lm_head_sampled_ring_per_request_T", V, H,
       lambda w: ops.gemm_sample_batch(w, x, R, V, H, 0, 16, gws, rids, 0, rdyn, inv_ts=inv, **kw), dev, runs, tiles=4)


def build_targets(args, spec, dev):
    """bench.build_models' bf16 target and draft, and an fp8 NativeTarget over the same seeded HF weights."""
    from dflash_amd import NativeTarget
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    torch.manual_seed(0)                                     # (as build_models: the same HF init and the same walk)
    hf, perm8 = bench.make_hf_target(spec, dev, meta["layers"])
    assert torch.equal(perm8, perm)
    target8 = NativeTarget(hf, attn_impl="head", keep_hf=False, prefill="native", weight_format="fp8_e4m3")
    del hf
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    assert target8.streams_fp8(16) and target8.streams_fp8_tiles() and not target.streams_fp8(16)
    codes = sum(t.numel() * t.element_size() for t in target8.fp8_tensors())
    packed = sum(w.numel() * 2 for lw in target8.layers for k, w in lw.items() if k in ("qkv", "o", "gu", "down")) + V * H * 2
    out(part="cycle", note="target quantised on " + ("the device" if ops.fp8_cast_on_device(dev) else "the host"),
        packed_bf16_bytes=packed, e4m3_code_and_scale_bytes=codes, fp8_target_over_bf16_target_bytes=(packed + codes) / packed)
    return {"bf16": target, "fp8": target8}, draft, cfg, perm, meta


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
        cyc, ver, drf, loss = ({"bf16": [], "fp8": []} for _ in range(4))
        for _ in range(runs):
            for f, t in forms.items():
                r = leg(t)
                loss[f].append(r["lossless_fraction"])
                cyc[f].append(1e3 * r["dt"] / (r["cycles"] if n == 1 else r["steps"]))
                ver[f].append(r["hot_path"]["target_verify_ms_per_cycle"])
                drf[f].append(r["hot_path"]["draft_plus_lm_head_ms_per_cycle"])
        for what, d in (("ms_per_cycle", cyc), ("verify_phase_ms_event_pair", ver), ("draft_phase_ms_event_pair", drf)):
            mb, m8 = med(d["bf16"]), med(d["fp8"])
            out(part="cycle", requests=n, what=what, steps=steps, bf16=mb, fp8=m8, fp8_over_bf16=m8["median"] / mb["median"],
                saved_ms=mb["median"] - m8["median"], faster_beyond_spread=m8["max"] < mb["min"],
                lossless_fraction={f: min(v) for f, v in loss.items()})


def part_head(dev, launches):
    dyn = torch.zeros(8, dtype=torch.int32, device=dev)
    ops.set_dyn(dyn, 1024, 16, 16, 1024)
    _, f8 = weights(V, H, 2, dev)
    h = torch.randn(16, H, device=dev).to(BF16)
    x = ops.rows_normed(h, torch.rand(H, device=dev) * 16, H // 16, torch.ones(H, device=dev, dtype=BF16), 1e-6, ops.DYN_BS)
    ids = torch.zeros(16, dtype=torch.long, device=dev)
    aws = ops.argmax_ws(dev)
    for i in range(launches):
        ops.gemm_sample(f8[i % 2], x, V, H, 0, 16, aws, ids, 0, seed=5, temperature=T, pos_dyn=dyn, pos_word=ops.DYN_POS0,
                        pos_add=1, dyn=dyn)
    R, rdyn, xr, rids, seeds, inv, gws = ring_inputs(dev)
    for i in range(launches):
        ops.gemm_sample_batch(f8[i % 2], xr, R, V, H, 0, 16, gws, rids, 0, rdyn, seeds=seeds, temperature=T,
                              pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=1, nrows_dyn_word=ops.DYN_BS)
    torch.cuda.synchronize()
    out(part="head", launches_each=launches, kernels=["k_gemm_s_w8 (one tile)", "dfl_k_gemm_r<4,1,1,16,2,EPI_SAMPLE,W8> (4 tiles)"],
        algorithmic_bytes_per_launch=V * H)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gemm", "cycle", "head", "all"], default="all")
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
    if a.part == "head":
        part_head(dev, a.launches)
