"""Same-box A/B of FP8 (e4m3) expert weights in the SHARED MoE pass over 2..4 tiles (NativeTarget._moe_mlp_shared; DESIGN.md
section 10, "The experts"), Qwen3-Coder-30B-A3B geometry (128 experts of 768 x 2048, top-8), one process, both arms
alternating after a warm-up of each; median of `--runs` repeats with the spread (min .. max).  The bf16 arm of every
comparison is `expert_stream = False` on the SAME fp8-expert target: the same values as 2-byte weights through the bf16
form of the grouped kernel, i.e. the launches the shared pass made before it could take codes.

Parts (each prints JSON lines):
  launches  device time of each of a layer's two grouped launches (ops.moe_grouped_gate_up with the gather in its
            addresses, ops.moe_grouped_down) at R = 2 and R = 4 tiles of 16 rows, on one routed work list per R; the
            launches rotate through the layers' own expert tensors, so that none is served from the Infinity Cache;
            bytes / time against 8 TB/s.  `--synthetic`: no model — `--layers` layers of expert tensors with arbitrary
            finite contents and a random routing; what a counter run takes:
                rocprofv3 --pmc FETCH_SIZE -- python scripts/bench_fp8_experts_shared.py --part launches --synthetic \
                    --layers 4 --runs 1 --tiles 4
  pass      the whole shared pass of a layer (router GEMM, routing + plan, the two grouped launches, combine) at R = 2 and 4,
            rotating through the target's layers
  cycle     four requests of 16 rows on that target at prefix 1024 through BatchedDecoder (scripts/bench_moe_batch.py's
            set-up), by hipGraph replay, one capture per arm: the verify + accept graph by event pairs, and the whole
            cycle (draft body, draft head, verify + accept) by wall clock

    timeout -k 10 900 python scripts/bench_fp8_experts_shared.py --runs 5 > profiles/fp8_experts_shared_ab.txt
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

BF16, F32, U8, I32 = torch.bfloat16, torch.float32, torch.uint8, torch.int32
E, IE, H, TOP_K = 128, 768, 2048, 8
ARMS = {"bf16": False, "fp8": True}


def out(**kw):
    print(json.dumps(kw), flush=True)


def med(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def alternate(runs, one):
    """one(arm) -> a time; a warm-up of each arm, then `runs` repeats alternating."""
    for arm in ARMS:
        one(arm)
    t = {arm: [] for arm in ARMS}
    for _ in range(runs):
        for arm in ARMS:
            t[arm].append(one(arm))
    return med(t["bf16"]), med(t["fp8"])


def device_us(fn, n):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def synthetic_layers(n, dev):
    """n layers of expert tensors per form with arbitrary finite contents (the time does not depend on the values)"""
    layers = []
    for _ in range(n):
        lw = {}
        for key, rows, k in (("gu_e", 2 * IE, H), ("down_e", H, IE)):
            lw[key] = torch.randn(E, rows * k, device=dev, dtype=F32).mul_(0.03).to(BF16)
            codes = torch.randint(0, 0x78, (E, rows * k), device=dev, dtype=U8)          # finite, positive
            lw[key + "8"] = ops.Fp8Experts(codes, torch.full((E, rows), 2.0 ** -9, device=dev), E, rows, k)
        layers.append(lw)
    return layers


def part_launches(dev, runs, layers, tiles):
    n_l = len(layers)
    g = torch.Generator(device=dev).manual_seed(0)
    xn = torch.randn(4, 16 * H, generator=g, device=dev).to(BF16)
    sc = ops.prefill_moe_scratch(64, H, IE, E, TOP_K, 128, dev)
    for R in tiles:
        P = 16 * R
        sc["rlog"][:P, :E] = torch.randn(P, E, generator=g, device=dev).to(BF16)
        ops.prefill_moe_route(sc["rlog"], P, sc, True)
        ops.moe_grouped_gate_up(layers[0]["gu_e"], xn, sc, H, gather=True)     # act_g of this work list, for the down launches
        n_act, n_items, n_tiles = int((sc["cnt"] > 0).sum()), int(sc["n_items"][0]), int(sc["n_items"][1])
        launches = {
            "grouped gate/up": (lambda w: ops.moe_grouped_gate_up(w, xn, sc, H, gather=True), "gu_e", 2 * IE * H, 2 * IE),
            "grouped down": (lambda w: ops.moe_grouped_down(w, sc, H), "down_e", H * IE, H),
        }
        for name, (launch, key, weights, rows) in launches.items():
            forms = {"bf16": [lw[key] for lw in layers], "fp8": [lw[key + "8"] for lw in layers]}
            mb, m8 = alternate(runs, lambda arm: device_us(lambda: [launch(w) for w in forms[arm]], n_l))
            b16, b8 = n_act * weights * 2, n_act * (weights + rows * 4)
            out(part="launches", launch=name, tiles=R, rows_per_item=sc["rows_per_item"], active_experts=n_act,
                work_items=n_items, gathered_tiles=n_tiles, layers_rotated=n_l, bf16_us=mb, fp8_us=m8, bf16_weight_bytes=b16,
                fp8_code_and_scale_bytes=b8, bf16_frac_of_8TBps=b16 / (mb["median"] * 1e-6) / 8e12,
                fp8_frac_of_8TBps=b8 / (m8["median"] * 1e-6) / 8e12, fp8_over_bf16=m8["median"] / mb["median"],
                slowest_fp8_beats_fastest_bf16=m8["max"] < mb["min"])


def build(n_layers, dev):
    """scripts/bench_moe_batch.py's target (random-init Qwen3MoeForCausalLM at the 30B-A3B widths) with fp8 experts, and
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
    nt = NativeTarget(hf, expert_format="fp8_e4m3", keep_hf=False)
    del hf
    assert nt.experts8 is not None and nt.moe_shared_pass and nt.moe_shared_min == 2
    dcfg = DFlashConfig(hidden_size=H, num_hidden_layers=2, num_attention_heads=32, num_key_value_heads=4, head_dim=128,
                        intermediate_size=6144, vocab_size=151936, num_target_layers=n_layers, block_size=16, rope_theta=1e7,
                        mask_token_id=151669)
    m = DFlashDraftModel(dcfg, device=dev)
    m.load_state_dict(make_draft_state_dict(dcfg, seed=3, dtype=BF16))
    packed = sum(lw[k].numel() * 2 for lw in nt.layers for k in ("gu_e", "down_e"))
    codes = sum(t.numel() * t.element_size() for t in nt.fp8_tensors())
    out(part="build", layers=nt.L, packed_bf16_expert_bytes=packed, e4m3_code_and_scale_bytes=codes)
    return nt, m, dcfg


def part_pass(dev, runs, nt, tiles):
    g = torch.Generator(device=dev).manual_seed(1)
    xn = torch.randn(4, 16 * H, generator=g, device=dev).to(BF16)
    part = torch.zeros(4 * 16 * H, dtype=F32, device=dev)
    for R in tiles:
        dyn = torch.zeros(4, 8, dtype=I32, device=dev)
        dyn[:R, ops.DYN_BS] = 16

        def one(arm):
            nt.expert_stream = ARMS[arm]
            try:
                return device_us(lambda: [nt._moe_mlp_shared(lw, R, 4, dyn, xn, part) for lw in nt.layers], nt.L)
            finally:
                nt.expert_stream = True
        mb, m8 = alternate(runs, one)
        sc = nt._moe_sh["sc"]
        out(part="pass", what="whole shared pass of a layer, us", tiles=R, rows_per_item=sc["rows_per_item"],
            active_experts_last_layer=int((sc["cnt"] > 0).sum()), layers_rotated=nt.L, bf16_us=mb, fp8_us=m8,
            fp8_over_bf16=m8["median"] / mb["median"], saved_us=mb["median"] - m8["median"],
            slowest_fp8_beats_fastest_bf16=m8["max"] < mb["min"])


def part_cycle(dev, runs, nt, m, dcfg, prefix, reps=10):
    from dflash_amd.batch import BatchedDecoder
    R = 4
    dec = BatchedDecoder(m, nt, R, max_rows=prefix + 1024, out_len=prefix + 1024, mask_token_id=dcfg.mask_token_id)
    for r in range(R):
        dec.admit(r, torch.randint(0, 151000, (1, prefix), generator=torch.Generator().manual_seed(1 + r)).to(dev))
    dec.cycle()
    graphs = {}
    for arm, stream in ARMS.items():          # one capture per arm: the graphs hold the launches of that arm
        nt.expert_stream = stream
        dec.capture()
        graphs[arm] = dec.graphs
    nt.expert_stream = True
    # how far these prompts' rows spread over the experts: one eager verify, the active experts of every layer's work list
    active, real = [], ops.prefill_moe_route

    def counted(rlog, P, sc, norm_topk=True):
        real(rlog, P, sc, norm_topk)
        active.append(int((sc["cnt"] > 0).sum()))
    ops.prefill_moe_route = counted
    try:
        dec.verify()
    finally:
        ops.prefill_moe_route = real
    out(part="cycle", what="active experts per layer in the four requests' shared pass", **med(active))

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
        mb, m8 = alternate(runs, one)
        out(part="cycle", what=what, requests=R, prefix=prefix, layers=nt.L, bf16=mb, fp8=m8,
            fp8_over_bf16=m8["median"] / mb["median"], saved_ms=mb["median"] - m8["median"],
            slowest_fp8_beats_fastest_bf16=m8["max"] < mb["min"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["launches", "pass", "cycle", "all"], default="all")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=48, help="target layers (48: the 30B-A3B depth); the launches and the pass "
                                                             "rotate through them")
    ap.add_argument("--tiles", type=str, default="2,4")
    ap.add_argument("--prefix", type=int, default=1024)
    ap.add_argument("--synthetic", action="store_true", help="--part launches on expert tensors made here, no model")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    tiles = [int(t) for t in a.tiles.split(",")]
    if a.part in ("cycle", "all") and a.layers < 5:
        ap.error("the cycle part needs --layers >= 5 (the draft taps target layers 1 .. layers - 3)")
    if a.synthetic:
        if a.part != "launches":
            ap.error("--synthetic goes with --part launches")
        part_launches(dev, a.runs, synthetic_layers(a.layers, dev), tiles)
    else:
        nt, m, dcfg = build(a.layers, dev)
        with torch.inference_mode():
            if a.part in ("launches", "all"):
                part_launches(dev, a.runs, [{k: lw[k] for k in ("gu_e", "down_e", "gu_e8", "down_e8")} for lw in nt.layers], tiles)
            if a.part in ("pass", "all"):
                part_pass(dev, a.runs, nt, tiles)
            if a.part in ("cycle", "all"):
                part_cycle(dev, a.runs, nt, m, dcfg, a.prefix)
