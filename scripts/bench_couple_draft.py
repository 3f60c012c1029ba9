"""What the coupled draft costs, and what the coupling does to the match rate of a draw.

1. The pick launch under a grammar at 16 x 151936 (a 64-state automaton, half of every state's columns legal):
   dfl_grammar_draft_rows beside dfl_grammar_draft_sample_rows, the logits rotating through more buffers than L2 and the
   256 MB MALL hold; HIP events around blocks of launches, the arms alternating.
2. The single-request cycle (Qwen3-8B shapes, prefix 1024, block 16, T = 0.7, sampler="device", replayed): a greedy draft
   against a coupled one.  The hook scripts the same draft tokens into both arms behind the head launch and the emitted
   ids do not depend on the draft, so both arms accept the same lengths: the difference is the head launch (the plain
   bf16 k_gemm_s with its Philox epilogue where the greedy head streams its 13-bit twin).
3. Four ragged requests (prompts 1024 / 768 / 512 / 896, T = 0.7, replayed), greedy against coupled, scripted likewise.
   Parts 2 and 3: the two arms alternate in one process; median of --runs (5), min .. max.
4. Acceptance of the DRAW, not of a checkpoint: logits pairs target = X W, draft = (X + sigma E) W through the real head
   launches (V = 2048, K = 512; 1024 positions), the target's seeded draw against a greedy draft, a draft drawn on its
   own stream and a coupled draft, at T = 0.7 and 1.0, beside the closed forms (mean over the rows of p[argmax q],
   sum p q and sum_i 1 / sum_j max(p_j / p_i, q_j / q_i)) of the materialised logits.

    timeout -k 10 900 python scripts/bench_couple_draft.py [--parts 1,2,3,4] [--out profiles/couple_draft_ab.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dflash_amd import TokenDFA, ops  # noqa: E402
from scripts.bench_logprobs import _hook, timed  # noqa: E402

T = 0.7
OUT = None


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    if OUT is not None:
        OUT.write(line + "\n")
        OUT.flush()


def stats(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "all": v}


def part_launch(dev):
    V, S = 151936, 64
    g = torch.Generator(device=dev).manual_seed(V)
    rng = np.random.default_rng(V)
    nbuf = (320 << 20) // (16 * V * 2) + 1          # > 256 MB MALL + L2
    lg = (torch.randn(nbuf, 16, V, generator=g, device=dev) * 2).to(torch.bfloat16)
    nxt = np.where(rng.random((S, V)) < 0.5, rng.integers(0, S, (S, V)), -1).astype(np.int16)
    st = ops.grammar_state(1, S, V, dev)
    ops.grammar_set(st, 0, ops.grammar_load(st, TokenDFA(nxt, 0)), 0)
    block = torch.zeros(16, dtype=torch.int64, device=dev)
    bias = torch.zeros(V, dtype=torch.float32, device=dev)
    bias[torch.from_numpy(rng.random(V) < 0.5).to(dev)] = float("-inf")
    seeds = torch.tensor([7], dtype=torch.int64, device=dev)
    kw = dict(seeds=seeds, temperature=T, pos_base=1024)
    arms = {
        "plain_n16": lambda i: ops.grammar_draft_rows(lg[i % nbuf], st, block=block),
        "noise_n16": lambda i: ops.grammar_draft_sample_rows(lg[i % nbuf], st, block=block, **kw),
        "plain_both_n16": lambda i: ops.grammar_draft_rows(lg[i % nbuf], st, bias=bias, block=block),
        "noise_both_n16": lambda i: ops.grammar_draft_sample_rows(lg[i % nbuf], st, bias=bias, block=block, **kw),
        "noise_ban_only_n16": lambda i: ops.grammar_draft_sample_rows(lg[i % nbuf], None, bias=bias, block=block, **kw),
    }
    emit({"part": 1, "V": V, "rows": 16, "buffers": nbuf, "us": timed(arms)})
    del lg


def part_cycle(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk
    bs, dev = 16, draft.device
    prompt = torch.randint(0, V - 1000, (1, 1024), generator=torch.Generator().manual_seed(1)).to(dev)
    plan = bench.tau_plan(2 + warmup, steps, bs, seed=100)
    need = sum(k + 1 for k in plan[:warmup + steps + 2]) + 2 * bs
    G = greedy_walk(perm, prompt, need + 2 * bs).to(dev)
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("greedy", "coupled") if rep % 2 == 0 else ("coupled", "greedy")):
            s = DecodeSession(draft, target, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=need,
                              max_block_size=bs, stop_token_ids=None, temperature=T, sampler="device", seed=11,
                              draft_token_hook=_hook(G, plan, V), couple_draft=arm == "coupled")
            s.prefill()
            s.cycle(bs)
            for _ in range(1 + warmup):
                s.cycle(bs, ahead_ok=True)
            s.capture(bs)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tau = [s.cycle_graph(bs).tau for _ in range(steps)]
            torch.cuda.synchronize()
            res.setdefault(arm, []).append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
            taus.setdefault(arm, []).append(round(sum(tau) / len(tau), 3))
            del s
    emit({"part": 2, "single_request_cycle_ms": {k: stats(v) for k, v in res.items()}, "mean_tau": taus, "steps": steps,
          "prefix": 1024, "block": bs, "temperature": T})


def part_batch(bench, target, draft, cfg, perm, V, steps, warmup, runs):
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.synthetic import greedy_walk
    dev, bs, lens = draft.device, 16, (1024, 768, 512, 896)
    prompts = [torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(10 + i)).to(dev)
               for i, P in enumerate(lens)]
    plans = [bench.tau_plan(2 + warmup, steps, bs, seed=200 + i) for i in range(4)]
    need = max(sum(k + 1 for k in p[:warmup + steps + 3]) for p in plans) + 3 * bs
    Gs = [greedy_walk(perm, p, need + 2 * bs).to(dev) for p in prompts]
    hooks = [_hook(Gs[i], plans[i], V) for i in range(4)]
    hook = lambda r, blk, start, call: hooks[r](blk, start, call)   # noqa: E731
    res, taus = {}, {}
    for rep in range(runs):
        for arm in (("greedy", "coupled") if rep % 2 == 0 else ("coupled", "greedy")):
            dec = BatchedDecoder(draft, target, 4, max_rows=max(lens) + need + 64, out_len=max(lens) + need + 32,
                                 mask_token_id=cfg.mask_token_id, temperature=T, sampler="device",
                                 couple_draft=arm == "coupled")
            for r, p in enumerate(prompts):
                dec.admit(r, p, T, seed=21 + r)
            for _ in range(1 + warmup):
                dec.cycle(hook)
            dec.capture()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tau = [sum(o[0] for o in dec.cycle_graph(hook)) for _ in range(steps)]
            torch.cuda.synchronize()
            res.setdefault(arm, []).append(round(1e3 * (time.perf_counter() - t0) / steps, 4))
            taus.setdefault(arm, []).append(round(sum(tau) / (4 * len(tau)), 3))
            del dec
    emit({"part": 3, "four_request_ragged_cycle_ms": {k: stats(v) for k, v in res.items()}, "mean_tau": taus, "steps": steps,
          "prompts": lens, "block": bs, "temperature": T})


def part_acceptance(dev):
    """The draw itself, through dfl_gemm_argmax / dfl_gemm_sample as the draft head and the verify head launch them."""
    V, K, launches, seed = 2048, 512, 64, 12345
    g = torch.Generator(device=dev).manual_seed(3)
    W = (torch.randn(V, K, generator=g, device=dev) * 0.09).to(torch.bfloat16)   # logits of std ~2
    wp = ops.pack_weight(W)
    ws = ops.argmax_ws(dev)
    rows = []
    for temp in (0.7, 1.0):
        for sigma in (0.0, 0.1, 0.3, 1.0):
            hit = {"greedy": 0, "own_noise": 0, "coupled": 0}
            closed = {"greedy": 0.0, "own_noise": 0.0, "coupled": 0.0}
            n = 0
            for b in range(launches):
                x = torch.randn(16, K, generator=g, device=dev)
                xt, xd = x.to(torch.bfloat16), (x + sigma * torch.randn(16, K, generator=g, device=dev)).to(torch.bfloat16)
                start = 100 + 16 * b
                ids = {k: torch.zeros(16, dtype=torch.int64, device=dev) for k in ("target", "greedy", "own_noise", "coupled")}
                lt, ld = (torch.zeros(16, V, dtype=torch.bfloat16, device=dev) for _ in range(2))
                # verify row r draws position start + r + 1; draft row r stands for block slot r + 1: the same position
                ops.gemm_sample(wp, ops.rows_plain(xt), V, K, 0, 16, ws, ids["target"], 0, seed=seed, temperature=temp,
                                pos_base=start, pos_add=1, logits=lt)
                ops.gemm_argmax(wp, ops.rows_plain(xd), V, K, 0, 16, ws, ids["greedy"], 0, logits=ld)
                ops.gemm_sample(wp, ops.rows_plain(xd), V, K, 0, 16, ws, ids["own_noise"], 0, seed=seed, temperature=temp,
                                stream=ops.RNG_DRAFT, pos_base=start, pos_add=1)
                ops.gemm_sample(wp, ops.rows_plain(xd), V, K, 0, 16, ws, ids["coupled"], 0, seed=seed, temperature=temp,
                                stream=ops.RNG_TARGET, pos_base=start, pos_add=1)
                for k in hit:
                    hit[k] += int((ids[k] == ids["target"]).sum())
                p = torch.softmax(lt.double() / temp, dim=1)
                q = torch.softmax(ld.double() / temp, dim=1)
                closed["greedy"] += float(p.gather(1, ids["greedy"][:, None]).sum())
                closed["own_noise"] += float((p * q).sum())
                for r in range(16):   # sum_i 1 / sum_j max(p_j / p_i, q_j / q_i)
                    den = torch.maximum(p[r][None, :] / p[r][:, None], q[r][None, :] / q[r][:, None]).sum(dim=1)
                    closed["coupled"] += float((1.0 / den).sum())
                n += 16
            rows.append({"T": temp, "sigma": sigma, "draws": n,
                         "match_rate": {k: round(v / n, 4) for k, v in hit.items()},
                         "closed_form": {k: round(v / n, 4) for k, v in closed.items()}})
    emit({"part": 4, "V": V, "K": K, "acceptance_of_the_draw": rows})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="1,2,3,4")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "couple_draft_ab.txt"))
    a = ap.parse_args()
    parts = {int(x) for x in a.parts.split(",") if x}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    OUT = open(a.out, "w")
    dev = torch.device("cuda", 0)
    if 4 in parts:
        part_acceptance(dev)
    if 1 in parts:
        part_launch(dev)
    if parts & {2, 3}:
        import bench   # (the workload builders only; bench.py itself is not run)
        spec = bench.workload_spec("qwen3-8b")
        args = SimpleNamespace(target_layers=0, hf_verify=False, hf_prefill=False, attn_impl="head", fuse_oproj=False)
        target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
        if 2 in parts:
            part_cycle(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)
        if 3 in parts:
            part_batch(bench, target, draft, cfg, perm, meta["V"], a.steps, a.warmup, a.runs)
    OUT.close()


if __name__ == "__main__":
    main()
