"""Cost of the filtered draw: dfl_sample_rows_nucleus against dfl_sample_rows (k_sample_rows) over the same materialised
logits, 1 and 16 rows at V = 128256 and 151936, randn * 2 rows at T = 0.7; blocks of 50 launches timed with HIP events,
the arms alternating, median of 10 blocks.  Then the lm_head launch with and without its logits written (the filtered
verify materialises them; the fused draw does not).

    timeout -k 10 300 python scripts/bench_nucleus.py
"""
from __future__ import annotations

import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dflash_amd import ops  # noqa: E402


def timed(launch: dict, blocks: int = 10, per: int = 50) -> dict:
    res = {k: [] for k in launch}
    for f in launch.values():
        for _ in range(5):
            f()
    names = list(launch)
    for rep in range(blocks):
        for k in (names if rep % 2 == 0 else names[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per):
                launch[k]()
            b.record()
            b.synchronize()
            res[k].append(1e3 * a.elapsed_time(b) / per)
    return {k: round(sorted(v)[len(v) // 2], 2) for k, v in res.items()}


def main():
    dev, K, T = torch.device("cuda", 0), 4096, 0.7
    for V in (128256, 151936):
        g = torch.Generator(device=dev).manual_seed(V)
        lg = (torch.randn(16, V, generator=g, device=dev) * 2).to(torch.bfloat16)
        for rows in (1, 16):
            out = torch.zeros(rows, dtype=torch.int64, device=dev)
            x = lg[:rows]
            arms = {"sample_rows": lambda: ops.sample_rows(x, seed=1, temperature=T, pos0=7, out=out)}
            for name, (k, p) in {"off": (0, 1.0), "k50": (50, 1.0), "p0.9": (0, 0.9), "k50_p0.9": (50, 0.9),
                                 "k1": (1, 1.0)}.items():
                arms["nucleus_" + name] = (lambda k=k, p=p: ops.sample_rows_nucleus(x, seed=1, temperature=T, top_k=k,
                                                                                    top_p=p, pos_base=7, out=out))
            print(json.dumps({"V": V, "rows": rows, "us_median": timed(arms)}), flush=True)
        wp = ops.pack_weight((torch.randn(V, K, generator=g, device=dev) * 0.02).to(torch.bfloat16))
        xr = torch.randn(16, K, generator=g, device=dev).to(torch.bfloat16)
        src, ws = ops.rows_plain(xr), ops.argmax_ws(dev)
        ids = torch.zeros(16, dtype=torch.int64, device=dev)
        buf = torch.zeros(16, V, dtype=torch.bfloat16, device=dev)
        print(json.dumps({"V": V, "lm_head_16_rows_us_median": timed({
            "gemm_sample": lambda: ops.gemm_sample(wp, src, V, K, 0, 16, ws, ids, 0, seed=1, temperature=T, pos_base=7),
            "gemm_argmax_logits": lambda: ops.gemm_argmax(wp, src, V, K, 0, 16, ws, ids, 0, logits=buf),
            "gemm_argmax_logits+nucleus_k50_p0.9": lambda: (
                ops.gemm_argmax(wp, src, V, K, 0, 16, ws, ids, 0, logits=buf),
                ops.sample_rows_nucleus(buf, seed=1, temperature=T, top_k=50, top_p=0.9, pos_base=7, out=ids))})}),
            flush=True)


if __name__ == "__main__":
    main()
