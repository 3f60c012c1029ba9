"""Same-box A/B of the lossless 13-bit expert gate/up stream (dfl_moe_gate_up on DFL_W_BF16X13; DESIGN.md section 11,
"The experts") at the Qwen3-Coder-30B-A3B geometry (BASELINE configs[4]: 128 experts of 2 x 768 x 2048 per layer), one
process, both arms alternating after a warm-up of each; median of `--runs` repeats with the spread (min .. max) shown.
Both arms stream the SAME weights: the packed bf16 tensor and its twin (ops.pack_weight_bf16x13 of it).

Prints JSON lines:
  pack     seconds to pack one layer's expert-tall matrix (196608 x 2048) on the device, over all layers, and the bytes
  experts  per-launch device time of k_moe_gate_up with ~46 and ~80 active experts, bf16 against 13-bit; the launches
           rotate through `--layers` layers' own expert tensors (48: 38.7 GB bf16, 31.4 GB of twins), so that nothing is
           served from L2 or the Infinity Cache; bytes / time against 8 TB/s; `kind_on` = the rule of ops.X13_KINDS: the
           slowest 13-bit repeat beats the fastest bf16 repeat.
For a counter run of its own (nothing traced alongside), a few launches of each form:
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- python scripts/bench_bf16x13_experts.py --layers 4 --runs 1

    timeout -k 10 900 python scripts/bench_bf16x13_experts.py --runs 5 > profiles/bf16x13_experts_ab.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import ops  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
E, IE, H = 128, 768, 2048


def out(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def make_layers(n, dev):
    """n layers of packed expert gate/up tensors (randn * 0.03: the time does not depend on the values) and their twins."""
    layers, secs = [], []
    for _ in range(n):
        wp = torch.randn(E, 2 * IE * H, device=dev, dtype=F32).mul_(0.03).to(BF16)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        w13, rep = ops.pack_weight_bf16x13(wp, E * 2 * IE, H)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        assert w13 is not None, rep
        layers.append((wp, w13))
    wp, w13 = layers[0]
    out(part="pack", layers=n, seconds_per_layer=med(secs), bf16_bytes_per_layer=wp.numel() * 2,
        x13_bytes_per_layer=w13.data.numel(), x13_over_bf16=w13.data.numel() / (wp.numel() * 2))
    return layers


def part_experts(dev, runs, layers):
    n_l = len(layers)
    g = torch.Generator(device=dev).manual_seed(0)
    xf = torch.randn(16 * H, generator=g, device=dev).to(BF16)
    act = torch.zeros(E, 16 * IE, dtype=BF16, device=dev)
    forms = {"bf16": [l[0] for l in layers], "x13": [l[1] for l in layers]}
    verdict = []
    for n_act in (46, 80):
        on = torch.randperm(E, generator=g, device=dev)[:n_act].sort().values
        lst = torch.zeros(E, dtype=torch.int32, device=dev)
        lst[:n_act] = on.to(torch.int32)
        n = torch.tensor([n_act], dtype=torch.int32, device=dev)

        def one_pass(wl):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for w in wl:
                ops.moe_gate_up(w, xf, E, IE, H, act, lst, n)
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / n_l * 1e3
        for wl in forms.values():          # warm-up of each form
            one_pass(wl)
        us = {f: [] for f in forms}
        for _ in range(runs):              # alternating
            for f, wl in forms.items():
                us[f].append(one_pass(wl))
        mb, m13 = med(us["bf16"]), med(us["x13"])
        b16 = n_act * 2 * IE * H * 2
        b13 = n_act * (2 * IE * H * 13 // 8 + 2 * IE // 16 * 16 * 8)
        verdict.append(m13["max"] < mb["min"])
        out(part="experts", kernel="k_moe_gate_up", active_experts=n_act, layers_rotated=n_l, bf16_us=mb, x13_us=m13,
            bf16_bytes=b16, x13_bytes_with_meta=b13, bytes_ratio=b13 / b16, bf16_frac_of_8TBps=b16 / (mb["median"] * 1e-6) / 8e12,
            x13_frac_of_8TBps=b13 / (m13["median"] * 1e-6) / 8e12, x13_over_bf16=m13["median"] / mb["median"],
            slowest_x13_beats_fastest_bf16=verdict[-1])
    out(part="experts", kind_on=all(verdict), shipped=ops.X13_KINDS["experts_gateup"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=48, help="layers of expert tensors to rotate through")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    part_experts(dev, a.runs, make_layers(a.layers, dev))
