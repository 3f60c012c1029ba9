"""Same-box A/B of FP8 (e4m3) expert weights on the sparse-MoE native target ("The experts"),
Qwen3-Coder-30B-A3B shapes (BASELINE configs[4]), one process, both arms alternating after a warm-up of each; median of
`--runs` repeats with the spread (min .. max) shown.  The reference of every comparison is the bf16 arm of the same run:
`expert_stream = False` on the SAME fp8-expert target — the same values, streamed as 2-byte weights — so one target
serves both arms and 61 GB of experts need not exist twice.

Parts (each prints JSON lines):
  experts  per-launch device time of k_moe_gate_up and k_moe_down (nsplit 4, as the target launches it) at the 30B-A3B
           geometry (128 experts of 768 x 2048) with ~46 and ~80 active experts, bf16 against fp8; the launches rotate
           through the layers' own expert tensors (48 layers: > 30 GB per form), so that none is served from the Infinity
           Cache; bytes / time against 8 TB/s.  Run alone (`--part experts`) the part makes `--layers` layers of expert
           tensors of its own with arbitrary finite contents, for a counter run:
               rocprofv3 --pmc FETCH_SIZE -- python scripts/bench_fp8_experts.py --part experts --layers 8 --runs 1
  cycle    bench.py's `qwen3-30b-a3b` workload (bench.single_leg: DecodeSession, scripted acceptance, the policy loop
           over block sizes 8 / 12 / 16 by hipGraph replay): ms per cycle by wall clock, the verify phase from the event
           pairs of the instrumented cycles, lossless_fraction (committed ids == the target's own greedy walk) and the
           block sizes used

    timeout -k 10 1100 python scripts/bench_fp8_experts.py --runs 5 > profiles/fp8_experts_ab.txt
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload builders only; bench.py itself is not run)

import dflash_amd  # noqa: E402
from dflash_amd import ops  # noqa: E402

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
E, IE, H, NSPLIT = 128, 768, 2048, 4


def out(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def synthetic_layers(n, dev):
    """n layers of expert tensors per form with arbitrary finite contents (the time does not depend on the values)"""
    layers = []
    for _ in range(n):
        lw = {}
        for key, rows, k in (("gu_e", 2 * IE, H), ("down_e", H, IE)):
            lw[key] = torch.randn(E, rows * k, device=dev, dtype=F32).mul_(0.03).to(BF16)
            codes = torch.randint(0, 0x78, (E, rows * k), device=dev, dtype=U8)          # finite, positive
            lw[key + "8"] = ops.Fp8Experts(codes, torch.full((E, rows), 2.0 ** -9, device=dev), E, rows, k)
        layers.append(lw)
    return layers


def part_experts(dev, runs, layers):
    n_l = len(layers)
    g = torch.Generator(device=dev).manual_seed(0)
    xf = torch.randn(16 * H, generator=g, device=dev).to(BF16)
    act = (torch.randn(E, 16 * IE, generator=g, device=dev) * 0.1).to(BF16)
    part = torch.zeros(NSPLIT, 16, H, dtype=F32, device=dev)
    for n_act in (46, 80):
        on = torch.randperm(E, generator=g, device=dev)[:n_act].sort().values
        lst = torch.zeros(E, dtype=torch.int32, device=dev)
        lst[:n_act] = on.to(torch.int32)
        n = torch.tensor([n_act], dtype=torch.int32, device=dev)
        wt = torch.zeros(16, E, dtype=BF16, device=dev)
        wt[:, on] = torch.rand(16, n_act, generator=g, device=dev).to(BF16)
        launches = {
            "k_moe_gate_up": (lambda w: ops.moe_gate_up(w, xf, E, IE, H, act, lst, n), "gu_e", 2 * IE * H, 2 * IE),
            "k_moe_down": (lambda w: ops.moe_down(w, act, wt, lst, n, E, H, IE, NSPLIT, part), "down_e", H * IE, H),
        }
        for name, (launch, key, weights, rows) in launches.items():
            forms = {"bf16": [lw[key] for lw in layers], "fp8": [lw[key + "8"] for lw in layers]}

            def one_pass(wl):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for w in wl:
                    launch(w)
                e.record()
                torch.cuda.synchronize()
                return s.elapsed_time(e) / n_l * 1e3
            for wl in forms.values():          # warm-up of each form
                one_pass(wl)
            us = {"bf16": [], "fp8": []}
            for _ in range(runs):              # alternating
                for f, wl in forms.items():
                    us[f].append(one_pass(wl))
            mb, m8 = med(us["bf16"]), med(us["fp8"])
            b16, b8 = n_act * weights * 2, n_act * (weights + rows * 4)
            out(part="experts", kernel=name, active_experts=n_act, layers_rotated=n_l, bf16_us=mb, fp8_us=m8,
                bf16_bytes=b16, fp8_bytes_with_scales=b8, bf16_frac_of_8TBps=b16 / (mb["median"] * 1e-6) / 8e12,
                fp8_frac_of_8TBps=b8 / (m8["median"] * 1e-6) / 8e12, fp8_over_bf16=m8["median"] / mb["median"],
                faster_beyond_spread=m8["max"] < mb["min"])


def build(args, spec, dev):
    """bench.build_models' target and draft, the target built with expert_format="fp8_e4m3" (the builder looks
    NativeTarget up in the package at call time)."""
    real = dflash_amd.NativeTarget
    dflash_amd.NativeTarget = functools.partial(real, expert_format="fp8_e4m3")
    try:
        target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    finally:
        dflash_amd.NativeTarget = real
    assert target.expert_format == "fp8_e4m3" and target.experts8 is not None and target.hf is None
    packed = sum(lw[k].numel() * 2 for lw in target.layers for k in ("gu_e", "down_e"))
    codes = sum(t.numel() * t.element_size() for t in target.fp8_tensors())
    out(part="cycle", note="experts quantised on " + ("the device" if ops.fp8_cast_on_device(dev) else "the host"),
        layers=target.L, packed_bf16_expert_bytes=packed, e4m3_code_and_scale_bytes=codes,
        fp8_experts_over_bf16_experts_bytes=(packed + codes) / packed)
    return target, draft, cfg, perm, meta


def part_cycle(args, spec, dev, runs, built):
    target, draft, cfg, perm, meta = built
    arms = {"bf16": False, "fp8": True}

    def leg(stream):
        target.expert_stream = stream
        try:
            return bench.single_leg(args, spec, 0, dev, target, draft, cfg, perm, meta)
        finally:
            target.expert_stream = True
    for stream in arms.values():              # warm-up of each arm
        leg(stream)
    cyc, ver, loss, used = ({"bf16": [], "fp8": []} for _ in range(4))
    for _ in range(runs):
        for f, stream in arms.items():
            r = leg(stream)
            loss[f].append(r["lossless_fraction"])
            cyc[f].append(1e3 * r["dt"] / r["cycles"])
            ver[f].append(r["hot_path"]["target_verify_ms_per_cycle"])
            used[f].append(r.get("used_block_sizes"))
    for what, d in (("ms_per_cycle", cyc), ("verify_phase_ms_event_pair", ver)):
        mb, m8 = med(d["bf16"]), med(d["fp8"])
        out(part="cycle", what=what, steps=args.steps, bf16=mb, fp8=m8, fp8_over_bf16=m8["median"] / mb["median"],
            saved_ms=mb["median"] - m8["median"], faster_beyond_spread=m8["max"] < mb["min"],
            lossless_fraction={f: min(v) for f, v in loss.items()}, used_block_sizes={f: v[-1] for f, v in used.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["experts", "cycle", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--layers", type=int, default=0, help="target layers (0: the workload's 48); --part experts: layers of "
                                                           "synthetic expert tensors to rotate through")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.part == "experts":
        part_experts(dev, a.runs, synthetic_layers(a.layers or 48, dev))
    else:
        args = SimpleNamespace(steps=a.steps, warmup=a.warmup, prefix=1024, temperature=None, schedule=None, event_every=4,
                               target_layers=a.layers, hf_verify=False, hf_prefill=False, eager=False, attn_impl="head",
                               fuse_oproj=False, full=False, workload="qwen3-30b-a3b")
        spec = bench.workload_spec("qwen3-30b-a3b")
        built = build(args, spec, dev)
        if a.part == "all":
            part_experts(dev, a.runs, [{k: lw[k] for k in ("gu_e", "down_e", "gu_e8", "down_e8")} for lw in built[0].layers])
        part_cycle(args, spec, dev, a.runs, built)
