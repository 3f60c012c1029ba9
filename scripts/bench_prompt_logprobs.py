"""What prompt logprobs cost, at Qwen3-8B head shapes (H = 4096, V = 151936), P in {128, 1024, 4096}.

(a) the new launch pair: dfl_prefill_logprobs over P - 1 rows (strips + finish), no logits written;
(b) the same numbers from the entry points that existed before, built HERE and nowhere in the library:
    dfl_prefill_gemm_rows into a 128-row x V bf16 slab, then dfl_logprob_rows per 16-row tile of it, slab by slab.
The two arms alternate in one process after a warm-up of each; HIP events around each sample; median of 5 with min .. max.
The 1.24 GB head exceeds L2 and the 256 MB MALL: every pass streams it from HBM.
Then the native prefill of a target with the same widths at 2 and 4 layers, prompt_logprobs off and on: the per-layer and
fixed parts give the 36-layer prefill the launch is a fraction of (extrapolated: the line says so).

    timeout -k 10 900 python scripts/bench_prompt_logprobs.py [--P 128,1024,4096] [--no-prefill]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import ops  # noqa: E402

BF16 = torch.bfloat16
H, V = 4096, 151936


def sample(f, per: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(per):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / per


def alternate(arms: dict, per: dict, n: int = 5) -> dict:
    for f in arms.values():       # warm-up of each arm: code objects, workspaces
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in arms}
    for rep in range(n):
        for k in (list(arms) if rep % 2 == 0 else list(arms)[::-1]):
            res[k].append(sample(arms[k], per[k]))
    return res


def fmt(xs) -> str:
    return f"{statistics.median(xs):9.3f} ms (min {min(xs):.3f} .. max {max(xs):.3f}, n={len(xs)})"


def head_ab(P: int, wp: torch.Tensor, dev) -> float:
    rows, Pp = P - 1, ops.prefill_rows_padded(P - 1)
    g = torch.Generator(device=dev).manual_seed(P)
    x = torch.randn(rows, H, generator=g, device=dev).to(BF16)
    xf = torch.zeros(Pp * H, dtype=BF16, device=dev)
    ops.prefill_pack_rows(x, rows, H, xf)
    tg = torch.randint(0, V, (rows,), generator=g, device=dev)
    out_a = torch.empty(rows, dtype=torch.float32, device=dev)
    slab = torch.zeros(128, V, dtype=BF16, device=dev)
    sink = ops.logprob_sink(1, Pp, 0, dev)
    tg_pad = torch.zeros(Pp, dtype=torch.int64, device=dev)
    tg_pad[:rows] = tg

    def arm_a():
        ops.prefill_logprobs(wp, xf, rows, V, H, tg, out_a)

    def arm_b():
        for s0 in range(0, rows, 128):
            n = min(128, rows - s0)
            ops.prefill_gemm_rows(wp, xf[s0 * H:], n, V, H, slab)
            for t0 in range(0, n, 16):
                ops.logprob_rows(slab[t0:t0 + 16], tg_pad[s0 + t0:s0 + t0 + 16], sink, nrows=min(16, n - t0), pos_base=s0 + t0)

    res = alternate(dict(a=arm_a, b=arm_b), dict(a=4 if P <= 128 else 1, b=1))
    diff = float((out_a - sink.lp[0, :rows]).abs().max())
    ma, mb = statistics.median(res["a"]), statistics.median(res["b"])
    tf = 2.0 * rows * V * H / (ma * 1e-3) / 1e12
    print(f"P={P:5d} rows={rows:5d} nsplit={ops.prefill_logprobs_nsplit(rows, V):4d}")
    print(f"   (a) dfl_prefill_logprobs              {fmt(res['a'])}   {tf:6.1f} TFLOP/s bf16 MFMA (2 rows V K / t)")
    print(f"   (b) gemm_rows slab + logprob_rows     {fmt(res['b'])}   (b)/(a) = {mb / ma:.2f}   max |a - b| = {diff:.2e}")
    print(f"       logits (b) would hold at once: {128 * V * 2 / 1e6:.0f} MB slab (P x V: {P * V * 2 / 1e6:.0f} MB); "
          f"(a) workspace {ops.prefill_logprobs_nsplit(rows, V) * Pp * 16 / 1e6:.2f} MB", flush=True)
    return ma


def prefill_ab(Ps, head_ms: dict, dev) -> None:
    from dflash_amd import NativeTarget
    from dflash_amd.config import QWEN3_8B_TARGET
    from dflash_amd.synthetic import make_hf_qwen3
    t = {}
    for L in (2, 4):
        torch.manual_seed(21)
        nt = NativeTarget(make_hf_qwen3({**QWEN3_8B_TARGET, "num_layers": L}, dev), keep_hf=False)
        for P in Ps:
            ids = torch.randint(0, V, (1, P), generator=torch.Generator().manual_seed(P)).to(dev)
            cache = nt.new_cache(P + 16)
            res = alternate(dict(off=lambda: nt.prefill(ids, cache, output_hidden_states=False),
                                 on=lambda: nt.prefill(ids, cache, output_hidden_states=False, prompt_logprobs=True)),
                            dict(off=1, on=1))
            t[L, P] = res
            print(f"prefill L={L} P={P:5d}: off {fmt(res['off'])}   on {fmt(res['on'])}", flush=True)
        del nt
        torch.cuda.empty_cache()
    for P in Ps:
        m2, m4 = statistics.median(t[2, P]["off"]), statistics.median(t[4, P]["off"])
        layer = (m4 - m2) / 2
        full = m2 - 2 * layer + 36 * layer
        on = statistics.median(t[4, P]["on"]) - m4
        print(f"P={P:5d}: per layer {layer:.3f} ms, 36-layer prefill {full:.2f} ms (extrapolated from 2 and 4 layers); "
              f"prompt_logprobs adds {on:.3f} ms in the prefill (norm_pack + launch pair; the launch alone {head_ms[P]:.3f} ms) "
              f"= {100 * on / full:.1f} % of it")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", default="128,1024,4096")
    ap.add_argument("--no-prefill", action="store_true")
    a = ap.parse_args()
    Ps = [int(p) for p in a.P.split(",")]
    dev = torch.device("cuda", 0)
    print(f"device: {torch.cuda.get_device_name(0)}; H={H} V={V}; head {V * H * 2 / 1e9:.2f} GB bf16")
    g = torch.Generator(device=dev).manual_seed(1)
    w = torch.empty(V, H, dtype=BF16, device=dev)
    for r0 in range(0, V, 16384):       # (in pieces: no 2.5 GB fp32 temporary)
        w[r0:r0 + 16384] = (torch.randn(min(16384, V - r0), H, generator=g, device=dev) * 0.02).to(BF16)
    wp = ops.pack_weight(w)
    del w
    head_ms = {P: head_ab(P, wp, dev) for P in Ps}
    del wp
    torch.cuda.empty_cache()
    if not a.no_prefill:
        prefill_ab(Ps, head_ms, dev)


if __name__ == "__main__":
    main()
