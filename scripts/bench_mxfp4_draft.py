"""Same-box A/B of the MXFP4 draft weights against the FP8 (e4m3) and the bf16 draft, Qwen3-8B
shapes, one process, all three forms alternating after a warm-up of each; median of `--runs` repeats with the spread
(min .. max) shown.  Everything here is at EQUAL (scripted) acceptance length: what a 4-bit draft does to the acceptance
length of a trained checkpoint is not measured.

Parts (each prints JSON lines):
  gemm     per-launch device time of the seven draft GEMMs (fc, kv_all, qkv, o_proj, gate/up, down_proj, lm_head) in the
           row-source and epilogue forms the draft cycle launches, bf16 / fp8 / mxfp4; the weights rotate through
           > 600 MB of distinct buffers so that no launch is served from the Infinity Cache; bytes / time against 8 TB/s.
           The claim: on lm_head and gate/up the slowest mxfp4 repeat beats the fastest fp8 repeat (mxfp4_beats_fp8).
  cycle    bench.py's N = 1 workload (bench.single_leg: DecodeSession, scripted acceptance, hipGraph replay) with the
           bf16, the fp8 and the mxfp4 draft on the SAME bf16 target: ms per cycle, the draft forward + lm_head share of a
           cycle from the event pairs of the instrumented cycles, lossless_fraction.

    timeout -k 10 900 python scripts/bench_mxfp4_draft.py --runs 5 > profiles/mxfp4_draft_ab.txt
"""
from __future__ import annotations

import argparse
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

BF16 = torch.bfloat16
H, I, V, L, FC_IN, Q, KV = 4096, 12288, 151936, 5, 5 * 4096, 4096, 1024


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


def weights(N, K, n_buf, dev, gateup=False):
    """n_buf packed weights of N x K per form with arbitrary finite contents (the time does not depend on the values)"""
    b16 = [torch.randn(N * K // 2, device=dev, dtype=torch.float32).view(BF16)[:N * K].contiguous() for _ in range(n_buf)]
    f8 = []
    for _ in range(n_buf):
        codes = torch.randint(0, 0x78, (N * K,), device=dev, dtype=torch.uint8)     # finite, positive
        f8.append(ops.Fp8Weight(codes, torch.full((N,), 2.0 ** -9, device=dev), N, K))
    f4 = []
    for _ in range(n_buf):     # any code bytes under the block scale 2^-9: finite everywhere
        data = torch.randint(0, 256, (N * K // 2 + N * K // 32,), device=dev, dtype=torch.uint8)
        data[N * K // 2:] = 118
        f4.append(ops.Mxfp4Weight(data, N, K))
    return b16, f8, f4


def part_gemm(dev, runs):
    dyn = torch.zeros(8, dtype=torch.int32, device=dev)
    ops.set_dyn(dyn, 0, 16, 16, 0)

    def normed(K):
        h = torch.randn(16, K, device=dev).to(BF16)
        return ops.rows_normed(h, torch.rand(K, device=dev) * 16, K // 16, torch.ones(K, device=dev, dtype=BF16), 1e-6,
                               ops.DYN_BS)

    def frag(K):
        return ops.rows_frag(torch.randn(16 * K, device=dev).to(BF16))

    hbuf = torch.zeros(16, max(H, L * 2 * KV, Q + 2 * KV), dtype=BF16, device=dev)
    ss = torch.zeros(H, device=dev)
    act = torch.zeros(16 * I, dtype=BF16, device=dev)
    ids = torch.zeros(16, dtype=torch.long, device=dev)
    aws = ops.argmax_ws(dev)
    th = torch.randn(16, FC_IN, device=dev).to(BF16)
    cases = [   # (name, N, K, launch(w))
        ("fc", H, FC_IN, lambda w, x=ops.rows_plain(th, ops.DYN_TAU): ops.gemm_resid(w, x, H, FC_IN, hbuf[:, :H], add_residual=False, ss_out=ss, dyn=dyn)),
        ("kv_all", L * 2 * KV, H, lambda w, x=normed(H): ops.gemm_resid(w, x, L * 2 * KV, H, hbuf[:, :L * 2 * KV], add_residual=False, dyn=dyn)),
        ("qkv", Q + 2 * KV, H, lambda w, x=normed(H): ops.gemm_resid(w, x, Q + 2 * KV, H, hbuf[:, :Q + 2 * KV], add_residual=False, dyn=dyn)),
        ("o_proj", H, Q, lambda w, x=frag(Q): ops.gemm_resid(w, x, H, Q, hbuf[:, :H], add_residual=True, ss_out=ss, dyn=dyn)),
        ("gate_up", 2 * I, H, lambda w, x=normed(H): ops.gemm_silu_mul(w, x, I, H, act, dyn)),
        ("down_proj", H, I, lambda w, x=frag(I): ops.gemm_resid(w, x, H, I, hbuf[:, :H], add_residual=True, ss_out=ss, dyn=dyn)),
        ("lm_head", V, H, lambda w, x=normed(H): ops.gemm_argmax(w, x, V, H, 1, 15, aws, ids, 1, dyn=dyn)),
    ]
    for name, N, K, launch in cases:
        n_buf = max(2, int(600e6 // (N * K)) + 1)
        b16, f8, f4 = weights(N, K, n_buf, dev)
        forms = {"bf16": b16, "fp8": f8, "mxfp4": f4}
        for wl in forms.values():        # warm-up of each form
            time_launches(lambda i: launch(wl[i]), n_buf)
        us = {f: [] for f in forms}
        for _ in range(runs):            # alternating
            for f, wl in forms.items():
                us[f].append(time_launches(lambda i: launch(wl[i]), n_buf))
        mb, m8, m4 = med(us["bf16"]), med(us["fp8"]), med(us["mxfp4"])
        frac = lambda nbytes, m: nbytes / (m["median"] * 1e-6) / 8e12      # noqa: E731
        # faster by more than the spread: the slowest mxfp4 repeat beats the fastest fp8 (bf16) repeat
        out(part="gemm", gemm=name, N=N, K=K, buffers=n_buf, bf16_us=mb, fp8_us=m8, mxfp4_us=m4,
            bf16_frac_of_8TBps=frac(N * K * 2, mb), fp8_frac_of_8TBps=frac(N * K, m8),
            mxfp4_frac_of_8TBps=frac(N * K // 2 + N * K // 32, m4), fp8_over_bf16=m8["median"] / mb["median"],
            mxfp4_over_bf16=m4["median"] / mb["median"], mxfp4_over_fp8=m4["median"] / m8["median"],
            mxfp4_beats_fp8=m4["max"] < m8["min"], mxfp4_beats_bf16=m4["max"] < mb["min"])
        del b16, f8, f4, forms
        torch.cuda.empty_cache()


def part_cycle(dev, runs, steps, warmup):
    from dflash_amd import DFlashDraftModel
    args = SimpleNamespace(steps=steps, warmup=warmup, prefix=1024, temperature=None, schedule=None, event_every=4,
                           target_layers=0, hf_verify=False, hf_prefill=False, eager=False, attn_impl="head",
                           fuse_oproj=False, full=False, workload="qwen3-8b")
    spec = bench.workload_spec("qwen3-8b")
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    g = torch.Generator(device=dev).manual_seed(0)       # bench.build_models' draft weights, drawn again
    sd = {k: (torch.randn(s, generator=g, device=dev, dtype=torch.float32) * 0.02).to(BF16)
          if len(s) == 2 else torch.ones(s, device=dev, dtype=BF16) for k, s in cfg.state_dict_shapes().items()}
    draft8 = DFlashDraftModel(cfg, device=dev, weight_format="fp8_e4m3")
    draft8.load_state_dict(sd)
    draft4 = DFlashDraftModel(cfg, device=dev, weight_format="mxfp4")
    draft4.load_state_dict(sd)
    del sd
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    out(part="cycle", note="quantised on " + ("the device" if ops.fp8_cast_on_device(dev) else "the host"))
    forms = {"bf16": draft, "fp8": draft8, "mxfp4": draft4}
    for d in forms.values():             # warm-up of each form
        bench.single_leg(args, spec, 0, dev, target, d, cfg, perm, meta)
    cyc, drf, lm = ({f: [] for f in forms} for _ in range(3))
    for _ in range(runs):
        for f, d in forms.items():
            r = bench.single_leg(args, spec, 0, dev, target, d, cfg, perm, meta)
            assert r["lossless_fraction"] == 1.0, (f, r["lossless_fraction"])
            cyc[f].append(1e3 * r["dt"] / r["cycles"])
            drf[f].append(r["hot_path"]["draft_plus_lm_head_ms_per_cycle"])
            e = r["roofline"]["also"][0] if "also" in r["roofline"] else r["roofline"]
            lm[f].append(e["avg_ms"])
    for what, d in (("ms_per_cycle", cyc), ("draft_plus_lm_head_ms", drf), ("lm_head_ms_event_pair", lm)):
        mb, m8, m4 = med(d["bf16"]), med(d["fp8"]), med(d["mxfp4"])
        out(part="cycle", what=what, steps=steps, bf16=mb, fp8=m8, mxfp4=m4, fp8_over_bf16=m8["median"] / mb["median"],
            mxfp4_over_bf16=m4["median"] / mb["median"], mxfp4_over_fp8=m4["median"] / m8["median"],
            mxfp4_beats_fp8=m4["max"] < m8["min"], lossless_fraction=1.0, acceptance="scripted, equal in all three arms")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gemm", "cycle", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.part in ("gemm", "all"):
        part_gemm(dev, a.runs)
    if a.part in ("cycle", "all"):
        part_cycle(dev, a.runs, a.steps, a.warmup)
