"""lm_head launch cost of the seeded draw: dfl_gemm_sample against dfl_gemm_argmax on the same weights and rows (16 rows,
K = 4096, V = 151936 / 128256), alternating blocks of launches timed with HIP events; the GEMM plus its finish kernel.
Then dfl_sample_rows over 1 and 16 materialised rows (the prefill's first token, a two-tile or HF-target verify).

    timeout -k 10 300 python scripts/bench_gemm_sample.py
"""
from __future__ import annotations

import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dflash_amd import ops  # noqa: E402


def main():
    dev, K = torch.device("cuda", 0), 4096
    for V in (151936, 128256):
        g = torch.Generator(device=dev).manual_seed(V)
        wp = ops.pack_weight((torch.randn(V, K, generator=g, device=dev) * 0.02).to(torch.bfloat16))
        x = torch.randn(16, K, generator=g, device=dev).to(torch.bfloat16)
        src, ws = ops.rows_plain(x), ops.argmax_ws(dev)
        ids = torch.zeros(16, dtype=torch.int64, device=dev)
        rec = torch.tensor([0, 0, 16, 1000, 1000, 0, 0, 0], dtype=torch.int32, device=dev)
        launch = {"argmax": lambda: ops.gemm_argmax(wp, src, V, K, 1, 15, ws, ids, 0),
                  "sample": lambda: ops.gemm_sample(wp, src, V, K, 1, 15, ws, ids, 0, seed=1, temperature=0.7,
                                                    pos_dyn=rec, pos_word=ops.DYN_POS0, pos_add=1)}
        res = {k: [] for k in launch}
        for _ in range(20):
            launch["argmax"]()
            launch["sample"]()
        for rep in range(10):
            for k in (("argmax", "sample") if rep % 2 == 0 else ("sample", "argmax")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(50):
                    launch[k]()
                b.record()
                b.synchronize()
                res[k].append(1e3 * a.elapsed_time(b) / 50)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        print(json.dumps({"V": V, "K": K, "rows": 15, "us_median": med, "us_all": res,
                          "sample_over_argmax": med["sample"] / med["argmax"] - 1.0}), flush=True)
        lg = torch.randn(16, V, generator=g, device=dev).to(torch.bfloat16)
        for rows in (1, 16):
            for _ in range(5):
                ops.sample_rows(lg[:rows], seed=1, temperature=0.7, pos0=7)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(50):
                ops.sample_rows(lg[:rows], seed=1, temperature=0.7, pos0=7)
            b.record()
            b.synchronize()
            print(json.dumps({"V": V, "sample_rows": rows, "us": 1e3 * a.elapsed_time(b) / 50}), flush=True)


if __name__ == "__main__":
    main()
