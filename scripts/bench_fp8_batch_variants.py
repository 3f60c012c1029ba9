"""Builds of the library that differ in a compile-time choice of the fp8 ragged-batch kernels ("The
batch forms": the look-ahead A of the W8 ring forms — the W8_A_* constants of csrc/gemm_batch.hip —, where k_gemm_b's
W8 form requests its scales), interleaved in ONE process on one box: the tree's library and every `--lib NAME=PATH`
loaded side by side, the six fp8 launches of a batch cycle at 4 request tiles and at 2, 8B shapes, a warm-up of each
build, then `--runs` alternating repeats; device µs per launch, median with min .. max, one JSON line per (launch, build).

    python scripts/bench_fp8_batch_variants.py --lib deeper=/path/libdflash_hip_A3.so --lib deepest=/path/..._A4.so
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import _lib, ops  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
H, I, V, L, Q, KV = 4096, 12288, 151936, 5, 4096, 1024
NAMES = ("dfl_gemm_f32_batch", "dfl_gemm_silu_mul_batch", "dfl_gemm_argmax_batch", "dfl_last_error")


def load(path):
    h = C.CDLL(path)
    for name in NAMES:
        fn = getattr(h, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return h


def timed(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(n):
        fn(i)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="NAME=PATH of another build")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    libs = {"tree": _lib.lib()}
    for spec in a.lib:
        name, path = spec.split("=", 1)
        libs[name] = load(path)
    st = torch.cuda.current_stream().cuda_stream
    for R in (4, 2):
        MT = ops.batch_tiles(R)
        dyn = torch.zeros(MT, 8, dtype=torch.int32, device=dev)
        dyn[:, ops.DYN_TAU], dyn[:, ops.DYN_BS] = 16, 16
        part = torch.zeros(ops.batch_ksplit(I) * MT * 16 * max(H, L * 2 * KV, Q + 2 * KV), dtype=F32, device=dev)
        act = torch.zeros(MT, 16 * I, dtype=BF16, device=dev)
        ids = torch.zeros(MT, 16, dtype=torch.long, device=dev)
        gws = ops.gemm_batch_ws(max(V, 2 * I), H, dev)
        for gemm, N, K in (("kv_all", L * 2 * KV, H), ("qkv_parts", Q + 2 * KV, H), ("o_proj", H, Q), ("gate_up", 2 * I, H),
                           ("down_proj", H, I), ("lm_head", V, H)):
            x = ops.brows_frag(torch.randn(MT, 16 * K, device=dev).to(BF16))
            n_buf = max(2, int(600e6 // (N * K)) + 1)
            ws = [(torch.randint(0, 0x78, (N * K,), device=dev, dtype=torch.uint8), torch.full((N,), 2.0 ** -9, device=dev))
                  for _ in range(n_buf)]

            def launch(h, i):
                w = _lib.Weight(ws[i][0].data_ptr(), ws[i][1].data_ptr(), _lib.W_E4M3)
                if gemm == "gate_up":
                    rc = h.dfl_gemm_silu_mul_batch(w, x.ref, R, I, K, act.data_ptr(), act.stride(0), gws.data_ptr(),
                                                   dyn.data_ptr(), st)
                elif gemm == "lm_head":
                    rc = h.dfl_gemm_argmax_batch(w, x.ref, R, V, K, 1, 15, dyn.data_ptr(), ops.DYN_BS, gws.data_ptr(),
                                                 ids.data_ptr(), ids.stride(0), 1, None, 0, st)
                else:
                    rc = h.dfl_gemm_f32_batch(w, x.ref, R, N, K, part.data_ptr(), dyn.data_ptr(), st)
                assert rc == 0, h.dfl_last_error()

            for h in libs.values():          # warm-up of each build
                timed(lambda i: launch(h, i), n_buf)
            us = {k: [] for k in libs}
            for _ in range(a.runs):          # alternating
                for k, h in libs.items():
                    us[k].append(timed(lambda i: launch(h, i), n_buf))
            for k in libs:
                print(json.dumps(dict(part="variants", tiles=R, gemm=gemm, N=N, K=K, build=k,
                                      us=dict(median=round(statistics.median(us[k]), 2), min=round(min(us[k]), 2),
                                              max=round(max(us[k]), 2)))), flush=True)
            del ws
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
