"""Same-box A/B of MXFP4 expert weights on the sparse-MoE native target ("The experts"), Qwen3-Coder-
30B-A3B shapes (BASELINE configs[4]): one process, the arms alternating after a warm-up of each; median of `--runs`
repeats with the spread (min .. max).

Parts (each prints JSON lines):
  experts  per-launch device time of the gate/up and the down launch (128 experts of 768 x 2048, ~46 and ~80 active) on
           bf16, e4m3 and MXFP4 weights, plus the forms the library does not ship: gate/up with one and with two pairs
           per LDS meeting, down with 2 and with 4 column tiles per workgroup (4 shares, and 8 shares for 4 tiles: the
           grid of 256 workgroups).  The forms come from two builds of csrc/moe_w4.hip made here into build/mxfp4_ab/
           (-DDFL_MOE_W4_GU_PAIRS=1 -DDFL_MOE_W4_DOWN_CT=2, and =2 / =4) and called through their own handles.  The
           launches rotate through `--layers` layers of expert tensors of their own (arbitrary finite contents), so that
           none is served from the Infinity Cache.
  cycle    bench.py's `qwen3-30b-a3b` workload on a NativeTarget(expert_format=F) for F in --formats, expert_stream
           off (the bf16 copy of the same values) against on: ms per cycle, the verify phase, lossless_fraction.

    timeout -k 10 1100 python scripts/bench_mxfp4_experts.py --runs 5 > profiles/mxfp4_experts_ab.txt
"""
from __future__ import annotations

import argparse
import ctypes as C
import functools
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload builders only; bench.py itself is not run)

import dflash_amd  # noqa: E402
from dflash_amd import _lib, ops  # noqa: E402
from dflash_amd.build import CSRC, EXTRA_FLAGS, FLAGS, _hipcc  # noqa: E402

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
E, IE, H = 128, 768, 2048


def out(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def form_lib(pairs: int, ct: int):
    """csrc/moe.hip + moe_w4.hip + dfl_common.hip with the two W4 forms chosen at compile time, as a library of its own."""
    d = os.path.join(ROOT, "build", "mxfp4_ab")
    so = os.path.join(d, f"libmoe_w4_p{pairs}_ct{ct}.so")
    srcs = [os.path.join(CSRC, f) for f in ("moe.hip", "moe_w4.hip", "dfl_common.hip")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        os.makedirs(d, exist_ok=True)
        subprocess.run([_hipcc(), *FLAGS, *EXTRA_FLAGS["moe_w4.hip"], "-shared", f"-DDFL_MOE_W4_GU_PAIRS={pairs}",
                        f"-DDFL_MOE_W4_DOWN_CT={ct}", "-o", so, *srcs], check=True)
    h = C.CDLL(so)
    for name in ("dfl_moe_gate_up", "dfl_moe_down", "dfl_last_error"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


class through:
    """ops' launches through another library handle for the length of a `with`."""

    def __init__(self, handle):
        self.h = handle

    def __enter__(self):
        self.real, ops.lib = ops.lib, (lambda: self.h) if self.h is not None else ops.lib

    def __exit__(self, *a):
        ops.lib = self.real


def synthetic_layers(n, dev):
    layers = []
    for _ in range(n):
        lw = {}
        for key, rows, k in (("gu_e", 2 * IE, H), ("down_e", H, IE)):
            lw[key] = torch.randn(E, rows * k, device=dev, dtype=F32).mul_(0.03).to(BF16)
            codes = torch.randint(0, 0x78, (E, rows * k), device=dev, dtype=U8)          # finite, positive
            lw[key + "8"] = ops.Fp8Experts(codes, torch.full((E, rows), 2.0 ** -9, device=dev), E, rows, k)
            lw[key + "4"] = ops.Mxfp4Experts(torch.randint(0, 256, (E, rows * k // 2), device=dev, dtype=U8),
                                             torch.full((E, rows * k // 32), 120, device=dev, dtype=U8), E, rows, k)
        layers.append(lw)
    return layers


def part_experts(dev, runs, layers):
    n_l = len(layers)
    p1c2, p2c4 = form_lib(1, 2), form_lib(2, 4)
    g = torch.Generator(device=dev).manual_seed(0)
    xf = torch.randn(16 * H, generator=g, device=dev).to(BF16)
    act = (torch.randn(E, 16 * IE, generator=g, device=dev) * 0.1).to(BF16)
    part = torch.zeros(8, 16, H, dtype=F32, device=dev)
    for n_act in (46, 80):
        on = torch.randperm(E, generator=g, device=dev)[:n_act].sort().values
        lst = torch.zeros(E, dtype=torch.int32, device=dev)
        lst[:n_act] = on.to(torch.int32)
        n = torch.tensor([n_act], dtype=torch.int32, device=dev)
        wt = torch.zeros(16, E, dtype=BF16, device=dev)
        wt[:, on] = torch.rand(16, n_act, generator=g, device=dev).to(BF16)
        gu = lambda w: ops.moe_gate_up(w, xf, E, IE, H, act, lst, n)                                   # noqa: E731
        down = lambda ns: (lambda w: ops.moe_down(w, act, wt, lst, n, E, H, IE, ns, part))             # noqa: E731
        # arm -> (launch, layer key, library handle (None: the shipped library))
        kernels = {
            "gate_up": {"bf16": (gu, "gu_e", None), "fp8": (gu, "gu_e8", None), "mxfp4": (gu, "gu_e4", None),
                        "mxfp4_one_pair": (gu, "gu_e4", p1c2), "mxfp4_two_pairs": (gu, "gu_e4", p2c4)},
            "down": {"bf16": (down(4), "down_e", None), "fp8": (down(4), "down_e8", None), "mxfp4": (down(4), "down_e4", None),
                     "mxfp4_ct2_ns4": (down(4), "down_e4", p1c2), "mxfp4_ct4_ns4": (down(4), "down_e4", p2c4),
                     "mxfp4_ct4_ns8": (down(8), "down_e4", p2c4)},
        }
        for kname, arms in kernels.items():
            def one_pass(arm):
                launch, key, handle = arms[arm]
                with through(handle):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    for lw in layers:
                        launch(lw[key])
                    e.record()
                    torch.cuda.synchronize()
                return s.elapsed_time(e) / n_l * 1e3
            for arm in arms:                   # warm-up of each arm
                one_pass(arm)
            us = {arm: [] for arm in arms}
            for _ in range(runs):              # alternating
                for arm in arms:
                    us[arm].append(one_pass(arm))
            m = {arm: med(v) for arm, v in us.items()}
            out(part="experts", kernel=kname, active_experts=n_act, layers_rotated=n_l, us=m,
                mxfp4_over_bf16=m["mxfp4"]["median"] / m["bf16"]["median"], mxfp4_over_fp8=m["mxfp4"]["median"] / m["fp8"]["median"],
                slowest_mxfp4_beats_fastest_fp8=m["mxfp4"]["max"] < m["fp8"]["min"],
                slowest_mxfp4_beats_fastest_bf16=m["mxfp4"]["max"] < m["bf16"]["min"])


def part_cycle(args, spec, dev, runs, fmt):
    real = dflash_amd.NativeTarget
    dflash_amd.NativeTarget = functools.partial(real, expert_format=fmt)
    try:
        target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    finally:
        dflash_amd.NativeTarget = real
    assert target.expert_format == fmt
    arms = {"bf16_copy": False, fmt: True}

    def leg(stream):
        target.expert_stream = stream
        try:
            return bench.single_leg(args, spec, 0, dev, target, draft, cfg, perm, meta)
        finally:
            target.expert_stream = True
    for stream in arms.values():
        leg(stream)
    cyc, ver, loss = ({a: [] for a in arms} for _ in range(3))
    for _ in range(runs):
        for a, stream in arms.items():
            r = leg(stream)
            loss[a].append(r["lossless_fraction"])
            cyc[a].append(1e3 * r["dt"] / r["cycles"])
            ver[a].append(r["hot_path"]["target_verify_ms_per_cycle"])
    for what, d in (("ms_per_cycle", cyc), ("verify_phase_ms_event_pair", ver)):
        m = {a: med(v) for a, v in d.items()}
        out(part="cycle", expert_format=fmt, what=what, steps=args.steps, layers=target.L, ms=m,
            codes_over_copy=m[fmt]["median"] / m["bf16_copy"]["median"], faster_beyond_spread=m[fmt]["max"] < m["bf16_copy"]["min"],
            lossless_fraction={a: min(v) for a, v in loss.items()})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["experts", "cycle", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--layers", type=int, default=0, help="experts: layers of synthetic expert tensors to rotate through (0: 24); "
                                                           "cycle: target layers (0: the workload's 48)")
    ap.add_argument("--formats", default="fp8_e4m3,mxfp4")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.part in ("experts", "all"):
        part_experts(dev, a.runs, synthetic_layers(a.layers or 24, dev))
        torch.cuda.empty_cache()
    if a.part in ("cycle", "all"):
        args = SimpleNamespace(steps=a.steps, warmup=a.warmup, prefix=1024, temperature=None, schedule=None, event_every=4,
                               target_layers=a.layers if a.part == "cycle" else 0, hf_verify=False, hf_prefill=False, eager=False,
                               attn_impl="head", fuse_oproj=False, full=False, workload="qwen3-30b-a3b")
        spec = bench.workload_spec("qwen3-30b-a3b")
        for fmt in a.formats.split(","):
            part_cycle(args, spec, dev, a.runs, fmt)
            torch.cuda.empty_cache()
