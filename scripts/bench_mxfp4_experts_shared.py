"""Same-box A/B of MXFP4 expert weights in the SHARED MoE pass over 2..4 tiles (NativeTarget._moe_mlp_shared; DESIGN.md
section 17, "The shared pass"), Qwen3-Coder-30B-A3B geometry (128 experts of 768 x 2048, top-8), one process, the arms
alternating after a warm-up of each; median of `--runs` repeats with the spread (min .. max).  After
scripts/bench_fp8_experts_shared.py, whose helpers it uses.

Parts (each prints JSON lines):
  launches  device time of a layer's two grouped launches at R = 2 and R = 4 tiles of 16 rows on one routed work list per
            R (rows and router logits random), three arms: the bf16 copy, e4m3 codes (k_pgemm's W8 form), MXFP4 codes
            (csrc/moe_w4_shared.hip).  The launches rotate through `--layers` layers of expert tensors made here, so that
            none is served from the Infinity Cache; code + scale bytes of the active experts / time against 8 TB/s.
            The shipping rule: the slowest mxfp4 repeat beats the fastest bf16 repeat at both tile counts.
  pass      the whole shared pass of a layer on an mxfp4-expert target, expert_stream off (the copy) against on
  cycle     four requests of 16 rows on that target at prefix 1024 through BatchedDecoder by hipGraph replay, one capture
            per arm: the verify + accept graph by event pairs and the whole cycle by wall clock, copy against codes

    timeout -k 10 900 python scripts/bench_mxfp4_experts_shared.py --runs 5 > profiles/mxfp4_experts_shared_ab.txt
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_fp8_experts_shared import E, H, IE, TOP_K, device_us, med, out  # noqa: E402

from dflash_amd import ops  # noqa: E402

BF16, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32


def alternate(runs, arms, one):
    """one(arm) -> a time; a warm-up of each arm, then `runs` repeats alternating."""
    for arm in arms:
        one(arm)
    t = {arm: [] for arm in arms}
    for _ in range(runs):
        for arm in arms:
            t[arm].append(one(arm))
    return {arm: med(v) for arm, v in t.items()}


def synthetic_layers(n, dev):
    """n layers of expert tensors in the three forms, arbitrary finite contents (the time does not depend on the values)"""
    layers = []
    for _ in range(n):
        lw = {}
        for key, rows, k in (("gu_e", 2 * IE, H), ("down_e", H, IE)):
            lw[key, "bf16"] = torch.randn(E, rows * k, device=dev, dtype=F32).mul_(0.03).to(BF16)
            lw[key, "fp8"] = ops.Fp8Experts(torch.randint(0, 0x78, (E, rows * k), device=dev, dtype=U8),
                                            torch.full((E, rows), 2.0 ** -9, device=dev), E, rows, k)
            lw[key, "mxfp4"] = ops.Mxfp4Experts(torch.randint(0, 256, (E, rows * k // 2), device=dev, dtype=U8),
                                                torch.randint(117, 122, (E, rows * k // 32), device=dev, dtype=U8), E, rows, k)
        layers.append(lw)
    return layers


def part_launches(dev, runs, n_layers, tiles):
    layers = synthetic_layers(n_layers, dev)
    arms = ("bf16", "fp8", "mxfp4")
    g = torch.Generator(device=dev).manual_seed(0)
    xn = torch.randn(4, 16 * H, generator=g, device=dev).to(BF16)
    sc = ops.prefill_moe_scratch(64, H, IE, E, TOP_K, 128, dev)
    for R in tiles:
        P = 16 * R
        sc["rlog"][:P, :E] = torch.randn(P, E, generator=g, device=dev).to(BF16)
        ops.prefill_moe_route(sc["rlog"], P, sc, True)
        ops.moe_grouped_gate_up(layers[0]["gu_e", "bf16"], xn, sc, H, gather=True)   # act_g of this work list, for the down launches
        n_act, n_items, n_tiles = int((sc["cnt"] > 0).sum()), int(sc["n_items"][0]), int(sc["n_items"][1])
        launches = {"grouped gate/up": (lambda w: ops.moe_grouped_gate_up(w, xn, sc, H, gather=True), "gu_e", 2 * IE * H, 2 * IE),
                    "grouped down": (lambda w: ops.moe_grouped_down(w, sc, H), "down_e", H * IE, H)}
        for name, (launch, key, weights, rows) in launches.items():
            t = alternate(runs, arms, lambda arm: device_us(lambda: [launch(lw[key, arm]) for lw in layers], n_layers))
            nbytes = {"bf16": n_act * weights * 2, "fp8": n_act * (weights + rows * 4), "mxfp4": n_act * (weights // 2 + weights // 32)}
            out(part="launches", launch=name, tiles=R, rows_per_item=sc["rows_per_item"], active_experts=n_act, work_items=n_items,
                gathered_tiles=n_tiles, layers_rotated=n_layers, us=t, weight_bytes=nbytes,
                frac_of_8TBps={a: nbytes[a] / (t[a]["median"] * 1e-6) / 8e12 for a in arms},
                mxfp4_over_bf16=t["mxfp4"]["median"] / t["bf16"]["median"], mxfp4_over_fp8=t["mxfp4"]["median"] / t["fp8"]["median"],
                slowest_mxfp4_beats_fastest_bf16=t["mxfp4"]["max"] < t["bf16"]["min"],
                slowest_mxfp4_beats_fastest_fp8=t["mxfp4"]["max"] < t["fp8"]["min"])


def build(n_layers, dev):
    """scripts/bench_moe_batch.py's target (random-init Qwen3MoeForCausalLM at the 30B-A3B widths) with mxfp4 experts, and
    its two-layer draft."""
    from transformers import Qwen3MoeConfig, Qwen3MoeForCausalLM

    from dflash_amd import DFlashDraftModel, NativeTarget
    from dflash_amd.config import DFlashConfig
    from dflash_amd.synthetic import make_draft_state_dict
    cfg = Qwen3MoeConfig(vocab_size=151936, hidden_size=H, intermediate_size=6144, moe_intermediate_size=IE,
                         num_hidden_layers=n_layers, num_attention_heads=32, num_key_value_heads=4, head_dim=128,
                         num_experts=E, num_experts_per_tok=TOP_K, decoder_sparse_step=1, norm_topk_prob=True,
                         max_position_embeddings=40960, rms_norm_eps=1e-6, tie_word_embeddings=False,
                         rope_parameters={"rope_type": "default", "rope_theta": 1e7}, mlp_only_layers=[])
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(0)
    torch.set_default_dtype(BF16)
    with torch.device(dev):
        hf = Qwen3MoeForCausalLM(cfg).eval()
    torch.set_default_dtype(F32)
    nt = NativeTarget(hf, expert_format="mxfp4", keep_hf=False)
    del hf
    assert nt.experts4 is not None and nt.moe_shared_pass and nt.moe_shared_min == 2
    dcfg = DFlashConfig(hidden_size=H, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=4, head_dim=128,
                        intermediate_size=6144, vocab_size=151936, num_target_layers=n_layers, block_size=16, rope_theta=1e7,
                        mask_token_id=151669)
    m = DFlashDraftModel(dcfg, device=dev)
    m.load_state_dict(make_draft_state_dict(dcfg, seed=3, dtype=BF16))
    out(part="build", layers=nt.L)
    return nt, m, dcfg


def part_pass(dev, runs, nt, tiles):
    g = torch.Generator(device=dev).manual_seed(1)
    xn = torch.randn(4, 16 * H, generator=g, device=dev).to(BF16)
    part = torch.zeros(4 * 16 * H, dtype=F32, device=dev)
    for R in tiles:
        dyn = torch.zeros(4, 8, dtype=I32, device=dev)
        dyn[:R, ops.DYN_BS] = 16

        def one(arm):
            nt.expert_stream = arm == "codes"
            try:
                return device_us(lambda: [nt._moe_mlp_shared(lw, R, 4, dyn, xn, part) for lw in nt.layers], nt.L)
            finally:
                nt.expert_stream = True
        t = alternate(runs, ("copy", "codes"), one)
        out(part="pass", what="whole shared pass of a layer, us", tiles=R, layers_rotated=nt.L, us=t,
            codes_over_copy=t["codes"]["median"] / t["copy"]["median"], saved_us=t["copy"]["median"] - t["codes"]["median"],
            slowest_codes_beats_fastest_copy=t["codes"]["max"] < t["copy"]["min"])


def part_cycle(dev, runs, nt, m, dcfg, prefix, reps=10):
    from dflash_amd.batch import BatchedDecoder
    R = 4
    dec = BatchedDecoder(m, nt, R, max_rows=prefix + 1024, out_len=prefix + 1024, mask_token_id=dcfg.mask_token_id)
    for r in range(R):
        dec.admit(r, torch.randint(0, 151000, (1, prefix), generator=torch.Generator().manual_seed(1 + r)).to(dev))
    dec.cycle()
    graphs = {}
    for arm in ("copy", "codes"):             # one capture per arm: the graphs hold the launches of that arm
        nt.expert_stream = arm == "codes"
        dec.capture()
        graphs[arm] = dec.graphs
    nt.expert_stream = True

    def verify(arm):
        g = graphs[arm]["verify"]
        return device_us(lambda: [g.replay() for _ in range(reps)], reps) * 1e-3

    def cycle(arm):
        dec.graphs = graphs[arm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            dec.cycle_graph()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3
    for what, one in (("verify + accept graph, ms (event pair)", verify), ("whole four-request cycle, ms (wall clock)", cycle)):
        t = alternate(runs, ("copy", "codes"), one)
        out(part="cycle", what=what, requests=R, prefix=prefix, layers=nt.L, ms=t,
            codes_over_copy=t["codes"]["median"] / t["copy"]["median"], saved_ms=t["copy"]["median"] - t["codes"]["median"],
            slowest_codes_beats_fastest_copy=t["codes"]["max"] < t["copy"]["min"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["launches", "pass", "cycle", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=48, help="target layers (48: the 30B-A3B depth) of the pass and the cycle")
    ap.add_argument("--launch-layers", type=int, default=12, help="layers of expert tensors the launches part rotates through")
    ap.add_argument("--tiles", type=str, default="2,4")
    ap.add_argument("--prefix", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tiles = [int(t) for t in a.tiles.split(",")]
    if a.part in ("cycle", "all") and a.layers < 5:
        ap.error("the cycle part needs --layers >= 5 (the draft taps target layers 1 .. layers - 3)")
    if a.part in ("launches", "all"):
        with torch.inference_mode():
            part_launches(dev, a.runs, a.launch_layers, tiles)
    if a.part != "launches":
        nt, m, dcfg = build(a.layers, dev)       # (outside inference mode: the packers key on tensor versions)
        with torch.inference_mode():
            if a.part in ("pass", "all"):
                part_pass(dev, a.runs, nt, tiles)
            if a.part in ("cycle", "all"):
                part_cycle(dev, a.runs, nt, m, dcfg, a.prefix)
