"""Same-box A/B of the K-chunked 13-bit bf16 weight stream ("down_proj and fc") against the plain
packed bf16 form, per launch of dfl_gemm_resid, one process, both forms alternating after a warm-up of each; median of
`--runs` repeats with the spread (min .. max).  After scripts/bench_bf16x13.py.

  gemm   down_proj at 4096 x 12288 (Qwen3-8B), 4096 x 14336 (Llama-3.1-8B) and 2048 x 6144 (the 30B-A3B draft): a frag16
         source, the residual add, sums of squares out — the launch of the layer loop; fc at 4096 x 20480: plain rows with
         the row count from the dyn record, no residual add — the draft's launch.  The weights are randn * 0.02 matrices
         and every launch reads another buffer of a rotation of more than 256 MiB per form, so that none is served from
         the Infinity Cache.  A KIND is kept (ops.X13_KINDS) only if the 13-bit form's slowest repeat beats the plain
         form's fastest at every shape of that kind (`keep` per shape).
  pmc    `--part pmc --launches K`: K launches of each form of each shape and nothing else, for a counter run of its own
         (rocprofv3 --pmc FETCH_SIZE -- python scripts/bench_bf16x13_down.py --part pmc)

    timeout -k 10 600 python scripts/bench_bf16x13_down.py --runs 5
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
SHAPES = [("down_proj", "down", 4096, 12288), ("down_proj", "down", 4096, 14336), ("down_proj", "down", 2048, 6144),
          ("fc", "fc", 4096, 20480)]


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


def forms_of(N, K, n_buf, dev):
    """n_buf distinct buffers per form of ONE randn * 0.02 matrix (the time does not depend on which buffer holds what)"""
    w = (torch.randn(N, K, device=dev) * 0.02).to(BF16)
    wp = ops.pack_weight(w)
    del w
    w13, report = ops.pack_weight_bf16x13(wp, N, K)
    assert w13 is not None, report
    b16 = [wp] + [wp.clone() for _ in range(n_buf - 1)]
    x13 = [w13] + [ops.Bf16x13Weight(w13.data.clone(), N, K) for _ in range(n_buf - 1)]
    return b16, x13, report


def launcher(kind, N, K, dev):
    dyn = torch.zeros(8, dtype=torch.int32, device=dev)
    ops.set_dyn(dyn, 1024, 16, 16, 1024)
    rows = torch.randn(16, K, device=dev).to(BF16)
    h = torch.zeros(16, N, dtype=BF16, device=dev)
    ss = torch.zeros(N, dtype=torch.float32, device=dev)
    if kind == "fc":
        x = ops.rows_plain(rows, ops.DYN_TAU)
        return lambda w: ops.gemm_resid(w, x, N, K, h, add_residual=False, ss_out=ss, dyn=dyn)
    frag = torch.empty(16 * K, dtype=BF16, device=dev)
    ops.pack_rows(rows, 16, frag)
    x = ops.rows_frag(frag)
    return lambda w: ops.gemm_resid(w, x, N, K, h, add_residual=True, ss_out=ss, dyn=dyn)


def part_gemm(dev, runs):
    keep = {}
    for name, kind, N, K in SHAPES:
        launch = launcher(kind, N, K, dev)
        n_buf = max(2, int(600e6 // (N * K)) + 1)     # > 256 MiB per form in rotation
        b16, x13, report = forms_of(N, K, n_buf, dev)
        forms = {"bf16": b16, "bf16x13": x13}
        for wl in forms.values():        # warm-up of each form
            time_launches(lambda i: launch(wl[i]), n_buf)
        us = {f: [] for f in forms}
        for _ in range(runs):            # alternating
            for f, wl in forms.items():
                us[f].append(time_launches(lambda i: launch(wl[i]), n_buf))
        mb, mx = med(us["bf16"]), med(us["bf16x13"])
        nbytes = {"bf16": N * K * 2, "bf16x13": x13[0].data.numel()}
        k = mx["max"] < mb["min"]
        keep[kind] = keep.get(kind, True) and k
        out(part="gemm", gemm=name, kind=kind, N=N, K=K, buffers=n_buf, packer=report, bf16_us=mb, bf16x13_us=mx,
            bf16_TBps=nbytes["bf16"] / mb["median"] / 1e6, bf16x13_TBps=nbytes["bf16x13"] / mx["median"] / 1e6,
            bytes_ratio=nbytes["bf16x13"] / nbytes["bf16"], time_ratio=mx["median"] / mb["median"], keep=k)
        del b16, x13, forms
        torch.cuda.empty_cache()
    out(part="gemm", keep_kind=keep)


def part_pmc(dev, launches):
    for name, kind, N, K in SHAPES:
        launch = launcher(kind, N, K, dev)
        b16, x13, _ = forms_of(N, K, 2, dev)
        for wl in (b16, x13):
            for i in range(launches):
                launch(wl[i % 2])
        torch.cuda.synchronize()
        out(part="pmc", gemm=name, N=N, K=K, launches_per_form=launches, bf16_bytes=N * K * 2,
            bf16x13_bytes=x13[0].data.numel())
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
