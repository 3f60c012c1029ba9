"""Same-box A/B of the attention stage on a bf16 and on an e4m3 KV cache, Qwen3-8B shapes (32 query
heads, 8 kv heads, head_dim 128), block of 16 rows, one process, the two forms alternating after a warm-up of each; median
of `--runs` repeats with the spread (min .. max) shown.  Each prints JSON lines.  Launch sequences are captured into a
hipGraph once and replayed between the two timing events, so the figures are device time, not the host's enqueue time.

  attn     device time per launch of dfl_attn_head (bf16 cache) against dfl_attn_head_kv8 at S = 1024, 8192 and 32768; the
           launches rotate through enough distinct layer caches (> 600 MB of the e4m3 form) that none is served from the
           Infinity Cache; cache bytes read per launch / time against 8 TB/s
  quant    dfl_kv_quant_rows on one layer's K / V scratch at P = 1024 and 4096: the launch the e4m3 prefill adds per layer
  prefill  the whole native prefill of an 8B-shaped target (36 layers) at P = 1024 and 4096 with a bf16 and an e4m3 cache:
           ms per layer, and what the scratch + dfl_kv_quant_rows add to it
  verify   the N = 1 verify of 16 rows (greedy, replayed from a graph, lengths from the device record) at S = 1024 and
           32768, bf16 and mxfp4 weights, bf16 against e4m3 cache (the cache holds arbitrary finite rows: the time does not
           depend on the values)
  capacity rows of context per GB of cache, both formats

The V path: the attn part once on the library as built and once with DFL_LIB_PATH pointing at a
library whose attn_head_kv8.hip was compiled with -DDFL_KV8_V_CODES=0, same box, back to back, each against its own bf16 arm.

    timeout -k 10 500 python scripts/bench_kv8.py --runs 5 > profiles/kv8_ab.txt
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import ops  # noqa: E402
from dflash_amd.model import _rope_tables  # noqa: E402

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
NQ, NKV, MS = 32, 8, 32
ROW_BYTES = {"bf16": 2 * 128 * 2, "e4m3": 2 * (128 + 4)}   # K and V of one (row, kv head)


def out(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return dict(median=round(statistics.median(xs), 4), min=round(min(xs), 4), max=round(max(xs), 4), n=len(xs))


def captured(fn, n):
    """fn(0) .. fn(n - 1) once eagerly, then captured into a graph: returns replay() -> device microseconds per call."""
    for i in range(n):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(n):
            fn(i)

    def replay(reps=1):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            g.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / (n * reps) * 1e3
    return replay


def attn(dev, runs):
    g = torch.Generator(device=dev).manual_seed(1)
    qd, kd = NQ * 128, NKV * 128
    xq = torch.randn(16, qd + 2 * kd, device=dev, generator=g).to(BF16)
    nw = torch.ones(128, dtype=BF16, device=dev)
    ws = ops.attn_head_ws(NQ, MS, 1, dev)
    frag = torch.zeros(16 * qd, dtype=BF16, device=dev)
    for S in (1024, 8192, 32768):
        rows = S + 64
        L = max(4, min(300, -(-600_000_000 // (NKV * rows * ROW_BYTES["e4m3"]))))
        cos, sin = _rope_tables(128, 1e6, rows + 64, dev)
        kb = torch.randn(L, NKV, rows, 128, device=dev, generator=g).to(BF16)
        vb = torch.randn(L, NKV, rows, 128, device=dev, generator=g).to(BF16)
        k8, v8 = torch.empty(L, NKV, rows, 128, dtype=U8, device=dev), torch.empty(L, NKV, rows, 128, dtype=U8, device=dev)
        ks, vs = torch.empty(L, NKV, rows, dtype=F32, device=dev), torch.empty(L, NKV, rows, dtype=F32, device=dev)
        for i in range(L):   # (the bf16 arm reads the dequantised values: both arms compute the same attention)
            ops.kv_quant_rows(kb[i], vb[i], rows, k8[i], v8[i], ks[i], vs[i], 0)
        kw = dict(xq=xq, q_col=0, k_col=qd, v_col=qd + kd, n_q=NQ, n_kv=NKV, q_norm_w=nw, k_norm_w=nw, eps=1e-6, cos_tab=cos,
                  sin_tab=sin, scale=128 ** -0.5, causal=True, S=S, tau=0, bs=16, pos0=S, ws=ws, max_splits=MS, out_frag=frag)
        arms = {"bf16": lambda i: ops.attn_head(**kw, kcache=kb[i], vcache=vb[i]),
                "e4m3": lambda i: ops.attn_head_kv8(**kw, kcache=k8[i], vcache=v8[i], k_scale=ks[i], v_scale=vs[i])}
        us = {a: [] for a in arms}
        rp = {a: captured(fn, L) for a, fn in arms.items()}
        for a in arms:
            rp[a]()
        for _ in range(runs):
            for a in arms:
                us[a].append(rp[a]())
        for a in arms:
            m = med(us[a])
            gb = NKV * S * ROW_BYTES[a] / 1e9
            out(part="attn", S=S, cache=a, us_per_launch=m, cache_mb=round(gb * 1e3, 2), layers_rotated=L,
                frac_of_8tbs=round(gb / (m["median"] * 1e-6) / 8e3, 3))
        out(part="attn", S=S, e4m3_over_bf16=round(statistics.median(us["e4m3"]) / statistics.median(us["bf16"]), 3),
            e4m3_below_bf16_beyond_spread=max(us["e4m3"]) < min(us["bf16"]))
        del kb, vb, k8, v8, ks, vs
        torch.cuda.empty_cache()


def quant(dev, runs):
    for P in (1024, 4096):
        L = 16
        kb, vb = (torch.randn(L, NKV, P, 128, device=dev).to(BF16) for _ in range(2))
        k8, v8 = (torch.empty(NKV, P, 128, dtype=U8, device=dev) for _ in range(2))
        ks, vs = (torch.empty(NKV, P, dtype=F32, device=dev) for _ in range(2))
        rp = captured(lambda i: ops.kv_quant_rows(kb[i], vb[i], P, k8, v8, ks, vs, 0), L)
        rp()
        out(part="quant", P=P, us_per_layer=med([rp() for _ in range(runs)]), scratch_mb=round(2 * NKV * P * 256 / 1e6, 1))


def _target(dev, weight_format, kv_format):
    import bench  # (the workload builders only; bench.py itself is not run)
    from dflash_amd import NativeTarget
    spec = bench.workload_spec("qwen3-8b")
    torch.manual_seed(0)
    hf, _ = bench.make_hf_target(spec, dev, spec["target"]["num_layers"])
    t = NativeTarget(hf, keep_hf=False, weight_format=weight_format, kv_format=kv_format)
    del hf
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return t


def prefill(dev, runs, ts):
    for P in (1024, 4096):
        ids = torch.randint(0, 100000, (1, P), device=dev)
        ms = {}
        for fmt in ops.KV_FORMATS:
            t = ts[fmt]
            cache = t.new_cache(P + 64)
            xs = []
            for r in range(runs + 1):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                t.prefill(ids, cache, output_hidden_states=False)
                e.record()
                torch.cuda.synchronize()
                if r:
                    xs.append(s.elapsed_time(e) / t.L)
            ms[fmt] = med([round(x, 4) for x in xs])
        out(part="prefill", P=P, ms_per_layer=ms, added_us_per_layer=round(1e3 * (ms["fp8_e4m3"]["median"] - ms["bf16"]["median"]), 1),
            added_frac=round(ms["fp8_e4m3"]["median"] / ms["bf16"]["median"] - 1, 4))


def verify(dev, runs, ts, weights):
    blk = torch.randint(0, 100000, (16,), device=dev)
    for S in (1024, 32768):
        rp = {}
        for fmt in ops.KV_FORMATS:
            t = ts[fmt]
            cache = t.new_cache(S + 64)
            if fmt == "bf16":
                cache.k.normal_(), cache.v.normal_()
            else:
                cache.k.random_(0, 120), cache.v.random_(0, 120)   # (finite codes; the scales are ones)
            cache.length = S
            ops.set_dyn2(cache.dyn, S, 0, 16, S)
            rp[fmt] = (captured(lambda i, c=cache, t=t: t.verify(blk, S, c, dyn_lengths=True), 1), cache)
        ms = {f: [] for f in rp}
        for _ in range(runs):
            for f in rp:
                ms[f].append(rp[f][0](4) / 1e3)
        m = {f: med([round(x, 4) for x in v]) for f, v in ms.items()}
        out(part="verify", weights=weights, S=S, ms_per_verify=m, e4m3_over_bf16=round(m["fp8_e4m3"]["median"] / m["bf16"]["median"], 4),
            e4m3_below_bf16_beyond_spread=m["fp8_e4m3"]["max"] < m["bf16"]["min"])
        del rp
        gc.collect()
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parts", default="attn,quant,prefill,verify,capacity")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    parts = a.parts.split(",")
    if "attn" in parts:
        attn(dev, a.runs)
    if "quant" in parts:
        quant(dev, a.runs)
    for wf in ("bf16", "mxfp4"):   # (the same seeded weights under a target per cache format)
        if "verify" in parts or ("prefill" in parts and wf == "bf16"):
            ts = {kv: _target(dev, wf, kv) for kv in ops.KV_FORMATS}
            if "prefill" in parts and wf == "bf16":
                prefill(dev, a.runs, ts)
            if "verify" in parts:
                verify(dev, a.runs, ts, wf)
            del ts
            gc.collect()
            torch.cuda.empty_cache()
    if "capacity" in parts:   # Qwen3-8B: 36 layers x 8 kv heads
        out(part="capacity", rows_per_gb={k: int(1e9 // (36 * NKV * b)) for k, b in ROW_BYTES.items()},
            bytes_per_token={k: 36 * NKV * b for k, b in ROW_BYTES.items()})


if __name__ == "__main__":
    main()
