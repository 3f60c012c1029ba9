"""Same-box A/B of the lossless 13-bit bf16 weight stream against the plain packed bf16 form, per
launch, Qwen3-8B shapes, one process, both forms alternating after a warm-up of each; median of `--runs` repeats with
the spread (min .. max).  After scripts/bench_fp8_target.py --part gemm.

  gemm   gate/up + SiLU (dfl_gemm_silu_mul, 24576 x 4096) and the greedy lm_head (dfl_gemm_argmax, 151936 x 4096) at one
         16-row tile with the normalised row source the verify uses.  The weights are randn * 0.02 matrices — what the
         packer sees at load — and every launch reads another buffer of a rotation of more than 256 MiB per form, so
         that none is served from the Infinity Cache.  A form is kept for a matrix kind only if its slowest repeat beats
         the plain form's fastest (`keep`).
  pmc    `--part pmc --launches K`: K launches of each form of each kind and nothing else, for a counter run of its own
         (rocprofv3 --pmc FETCH_SIZE -- python scripts/bench_bf16x13.py --part pmc)

    timeout -k 10 600 python scripts/bench_bf16x13.py --runs 5
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

from dflash_amd import ops  # noqa: E402

BF16 = torch.bfloat16
H, I, V = 4096, 12288, 151936


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


def forms_of(N, K, n_buf, dev, gateup):
    """n_buf distinct buffers per form of ONE randn * 0.02 matrix (the time does not depend on which buffer holds what)"""
    if gateup:
        g, u = (torch.randn(N // 2, K, device=dev) * 0.02).to(BF16), (torch.randn(N // 2, K, device=dev) * 0.02).to(BF16)
        wp = ops.pack_weight_gateup(g, u)
        del g, u
    else:
        w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
        wp = ops.pack_weight(w)
        del w
    w13, report = ops.pack_weight_bf16x13(wp, N, K)
    assert w13 is not None, report
    b16 = [wp] + [wp.clone() for _ in range(n_buf - 1)]
    x13 = [w13] + [ops.Bf16x13Weight(w13.data.clone(), N, K) for _ in range(n_buf - 1)]
    return b16, x13, report


def cases(dev):
    dyn = torch.zeros(8, dtype=torch.int32, device=dev)
    ops.set_dyn(dyn, 1024, 16, 16, 1024)
    h = torch.randn(16, H, device=dev).to(BF16)
    x = ops.rows_normed(h, torch.rand(H, device=dev) * 16, H // 16, torch.ones(H, device=dev, dtype=BF16), 1e-6, ops.DYN_BS)
    act = torch.zeros(16 * I, dtype=BF16, device=dev)
    ids = torch.zeros(16, dtype=torch.long, device=dev)
    aws = ops.argmax_ws(dev)
    return [("gate_up", "gateup", 2 * I, H, lambda w: ops.gemm_silu_mul(w, x, I, H, act, dyn)),
            ("lm_head_greedy", "lm_head", V, H, lambda w: ops.gemm_argmax(w, x, V, H, 0, 16, aws, ids, 0, dyn=dyn))]


def part_gemm(dev, runs):
    for name, kind, N, K, launch in cases(dev):
        n_buf = max(2, int(600e6 // (N * K)) + 1)     # > 256 MiB per form in rotation
        b16, x13, report = forms_of(N, K, n_buf, dev, kind == "gateup")
        forms = {"bf16": b16, "bf16x13": x13}
        for wl in forms.values():        # warm-up of each form
            time_launches(lambda i: launch(wl[i]), n_buf)
        us = {f: [] for f in forms}
        for _ in range(runs):            # alternating
            for f, wl in forms.items():
                us[f].append(time_launches(lambda i: launch(wl[i]), n_buf))
        mb, mx = med(us["bf16"]), med(us["bf16x13"])
        nbytes = {"bf16": N * K * 2, "bf16x13": x13[0].data.numel()}
        out(part="gemm", gemm=name, kind=kind, N=N, K=K, buffers=n_buf, packer=report, bf16_us=mb, bf16x13_us=mx,
            bf16_TBps=nbytes["bf16"] / mb["median"] / 1e6, bf16x13_TBps=nbytes["bf16x13"] / mx["median"] / 1e6,
            bytes_ratio=nbytes["bf16x13"] / nbytes["bf16"], time_ratio=mx["median"] / mb["median"],
            keep=mx["max"] < mb["min"])
        del b16, x13, forms
        torch.cuda.empty_cache()


def part_pmc(dev, launches):
    for name, kind, N, K, launch in cases(dev):
        b16, x13, _ = forms_of(N, K, 2, dev, kind == "gateup")
        for wl in (b16, x13):
            for i in range(launches):
                launch(wl[i % 2])
        torch.cuda.synchronize()
        out(part="pmc", gemm=name, launches_per_form=launches, bf16_bytes=N * K * 2, bf16x13_bytes=x13[0].data.numel())
        del b16, x13
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gemm", "pmc"], default="gemm")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--launches", type=int, default=4)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    if args.part == "gemm":
        part_gemm(dev, args.runs)
    else:
        part_pmc(dev, args.launches)
