"""Same-box A/B of the slot-refilling engine (dflash_amd.engine) against static groups of four (dflash_generate_batch)
on Qwen3-8B shapes: bench.py's synthetic weights, prompts of 960..1088 ids, block 16, scripted acceptance (mean 7.3),
T = 0, one process, the two forms alternating `--runs` times after a warm-up of each.

Workload: 32 requests with ONE max_new_tokens (256: the static form has no per-request length) and a spread of lengths
that comes from stop ids placed in the scripted walks: request i stops after L_i = 16 + (i * 37) % 241 new tokens
(16..256, mean ~136; every L_i <= 256), its stop id being the walk's token at that offset.  The stop list is the union
of the 32 ids (the walk is one cycle through the vocabulary, so no request meets another's id within 256 tokens: checked).

Parts (each prints JSON lines, then one summary line):
  throughput   accepted tokens per second over the whole list, engine against static groups; counted and timed ratio
  admission    admit against admit_fused for P = 64, 1024: device-synchronised wall time, target prefill excluded
  cycle        steady per-cycle time of a full engine against the bare four-request cycle (BatchedDecoder.cycle_graph),
               at two cache capacities (the captured attention launches size their key splits by max_rows)
  trace        `--part trace --form admit|fused --admissions K`: K admissions and nothing else, for a profiler run of its
               own (rocprofv3 --kernel-trace --memory-copy-trace --stats -- python scripts/stream_ab.py --part trace ...);
               the per-admission copy and kernel counts are the difference of a K = 16 and a K = 8 run over 8

    timeout -k 10 900 python scripts/stream_ab.py --runs 3 > profiles/stream_ab.txt
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the workload builders only; bench.py itself is not run)

BS = 16


def out(**kw):
    print(json.dumps(kw), flush=True)


def sync_time():
    torch.cuda.synchronize()
    return time.perf_counter()


def make_hook(G, plan, V):
    def hook(blk, start, call):   # k agreeing tokens of the walk, then one that is not (bench.py's scripted acceptance)
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        if k > 0:
            blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % (V - 1000)
    return hook


def workload(perm, V, dev, n=32, max_new=256, prefix=1024):
    from dflash_amd.synthetic import greedy_walk
    lens = [prefix - 64 + (i * 29) % 129 for i in range(n)]
    stops_at = [16 + (i * 37) % 241 for i in range(n)]
    prompts = [torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(500 + i)).to(dev)
               for i, P in enumerate(lens)]
    walks = [greedy_walk(perm, p, max_new + 2 * BS) for p in prompts]
    stop = [int(w[P + L - 1]) for w, P, L in zip(walks, lens, stops_at)]
    for i, (w, P, L) in enumerate(zip(walks, lens, stops_at)):   # request i meets no stop id before its own
        first = next(j for j, x in enumerate(w[P:P + max_new].tolist()) if x in stop)
        assert first == L - 1, (i, first, L)
    plans = [bench.tau_plan(0, 48, BS, seed=700 + i) for i in range(n)]
    Gs = [w.to(dev) for w in walks]
    hooks = [make_hook(Gs[i], plans[i], V) for i in range(n)]
    return SimpleNamespace(prompts=prompts, lens=lens, stops_at=stops_at, stop=stop, hooks=hooks, Gs=Gs, max_new=max_new, n=n)


def check(w, outs):
    for i, o in enumerate(outs):
        assert o.num_output_tokens == w.stops_at[i], (i, o.num_output_tokens, w.stops_at[i])
        assert o.output_ids[0].tolist() == w.Gs[i][:w.lens[i] + w.stops_at[i]].tolist(), i


def part_throughput(a, draft, target, cfg, perm, V, dev):
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import BatchEngine
    w = workload(perm, V, dev, prefix=a.prefix)
    need = max(w.lens) + w.max_new
    eng = BatchEngine(draft, target, slots=4, max_rows=need + 3 * BS, out_len=need + BS, mask_token_id=cfg.mask_token_id,
                      stop_token_ids=w.stop)

    def static():
        t0 = sync_time()
        outs = dflash_generate_batch(draft, target, w.prompts, cfg.mask_token_id, w.max_new, BS, w.stop, 0.0,
                                     draft_token_hook=lambda i, blk, s, c: w.hooks[i](blk, s, c), hook_block_view=True)
        dt = sync_time() - t0
        cyc = [len(o.acceptance_lengths) for o in outs]
        return outs, dt, dict(group_cycles=sum(max(cyc[g:g + 4]) for g in range(0, w.n, 4)), live_slot_cycles=sum(cyc))

    def refill():
        before = dict(eng.stats)
        t0 = sync_time()
        for i, p in enumerate(w.prompts):
            eng.submit(p, w.max_new, draft_token_hook=w.hooks[i])
        outs = eng.run()
        dt = sync_time() - t0
        st = {k: eng.stats[k] - before[k] for k in ("group_cycles", "live_slot_cycles", "admissions", "replayed_cycles", "admit_s")}
        return outs, dt, st

    rows = {"static": [], "engine": []}
    for name, fn in (("static", static), ("engine", refill)):   # warm-up of each form (the engine's one capture is here)
        outs, dt, st = fn()
        check(w, outs)
        out(part="throughput", form=name, run="warmup", seconds=dt, **st)
    for r in range(a.runs):
        for name, fn in ((("static", static), ("engine", refill)) if r % 2 == 0 else (("engine", refill), ("static", static))):
            outs, dt, st = fn()
            check(w, outs)
            tok = sum(o.num_output_tokens for o in outs)
            rows[name].append(dict(tokens_per_s=tok / dt, seconds=dt, **st))
            out(part="throughput", form=name, run=r, tokens=tok, tokens_per_s=tok / dt, seconds=dt,
                occupancy=st["live_slot_cycles"] / (4 * st["group_cycles"]), **st)
            if name == "engine":
                by_len = {}
                for o in outs:
                    by_len.setdefault(o.num_input_tokens // 32 * 32, []).append(1e3 * o.time_to_first_token)
                out(part="throughput", form="engine", run=r,
                    admission_ms_by_prompt_length={k: round(statistics.median(v), 3) for k, v in sorted(by_len.items())})
    med = lambda name, key: statistics.median(x[key] for x in rows[name])   # noqa: E731
    spread = lambda name: (max(x["tokens_per_s"] for x in rows[name]) - min(x["tokens_per_s"] for x in rows[name])) / med(name, "tokens_per_s")   # noqa: E731
    out(part="throughput", summary=True, requests=w.n, max_new_tokens=w.max_new, mean_new_tokens=sum(w.stops_at) / w.n,
        static_tokens_per_s=med("static", "tokens_per_s"), engine_tokens_per_s=med("engine", "tokens_per_s"),
        timed_ratio=med("engine", "tokens_per_s") / med("static", "tokens_per_s"),
        counted_ratio=rows["static"][0]["group_cycles"] / rows["engine"][0]["group_cycles"],
        static_group_cycles=rows["static"][0]["group_cycles"], engine_group_cycles=rows["engine"][0]["group_cycles"],
        engine_admit_s=med("engine", "admit_s"), engine_seconds=med("engine", "seconds"), static_seconds=med("static", "seconds"),
        spread_static=spread("static"), spread_engine=spread("engine"), engine_captures=eng.stats["captures"])


def part_admission(a, draft, target, cfg, perm, V, dev, reps=7):
    from dflash_amd.batch import BatchedDecoder
    for P in (64, 1024):
        dec = BatchedDecoder(draft, target, 4, max_rows=P + 256, out_len=P + 256, mask_token_id=cfg.mask_token_id)
        prompt = torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(9)).to(dev)
        forms = {"prefill_only": lambda: dec._admit_prefill(1, prompt, 0.0, None), "admit": lambda: dec.admit(1, prompt),
                 "admit_fused": lambda: dec.admit_fused(1, prompt)}
        times = {k: [] for k in forms}
        with torch.inference_mode():
            for k, fn in forms.items():
                fn()
            for r in range(reps):
                for k, fn in (list(forms.items()) if r % 2 == 0 else list(forms.items())[::-1]):
                    t0 = sync_time()
                    fn()
                    times[k].append(1e3 * (sync_time() - t0))
        m = {k: statistics.median(v) for k, v in times.items()}
        out(part="admission", P=P, reps=reps, total_ms=m, rearm_ms={k: m[k] - m["prefill_only"] for k in ("admit", "admit_fused")},
            spread_ms={k: max(v) - min(v) for k, v in times.items()})
        del dec


def part_trace(a, draft, target, cfg, perm, V, dev):
    from dflash_amd.batch import BatchedDecoder
    P = a.prefix
    dec = BatchedDecoder(draft, target, 4, max_rows=P + 256, out_len=P + 256, mask_token_id=cfg.mask_token_id)
    prompt = torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(9)).to(dev)
    fn = dec.admit if a.form == "admit" else dec.admit_fused
    K = a.admissions
    for _ in range(K):
        fn(1, prompt)
    torch.cuda.synchronize()
    out(part="trace", form=a.form, admissions=K, P=P)


def part_cycle(a, draft, target, cfg, perm, V, dev, steps=24, warm=4):
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.engine import BatchEngine
    from dflash_amd.synthetic import greedy_walk
    P, new = a.prefix, (steps + warm + 4) * BS * 2
    prompts = [torch.randint(0, V - 1000, (1, P), generator=torch.Generator().manual_seed(1 + r)).to(dev) for r in range(4)]
    plans = [bench.tau_plan(2 + warm, steps, BS, seed=100 + r, extra=2 * (steps + warm)) for r in range(4)]
    Gs = [greedy_walk(perm, p, new + 2 * BS).to(dev) for p in prompts]
    hooks = [make_hook(Gs[r], plans[r], V) for r in range(4)]
    for max_rows in (P + new + 3 * BS, 8192):
        rows = {"decoder": [], "engine": []}
        for r in range(a.runs):
            for form in (("decoder", "engine") if r % 2 == 0 else ("engine", "decoder")):
                if form == "decoder":   # the four-request cycle as bench.py's batch4 leg runs it
                    dec = BatchedDecoder(draft, target, 4, max_rows=max_rows, out_len=P + new + BS, mask_token_id=cfg.mask_token_id)
                    with torch.inference_mode():
                        for i, p in enumerate(prompts):
                            dec.admit(i, p)
                    hk = lambda i, blk, s, c: hooks[i](blk, s, c)   # noqa: E731
                    dec.cycle(hk)
                    dec.capture()
                    step = lambda: dec.cycle_graph(hk)   # noqa: E731
                else:
                    eng = BatchEngine(draft, target, slots=4, max_rows=max_rows, out_len=P + new + BS,
                                      mask_token_id=cfg.mask_token_id)
                    for i, p in enumerate(prompts):
                        eng.submit(p, new, draft_token_hook=hooks[i])
                    eng.step()
                    step = eng.step
                for _ in range(warm):
                    step()
                t0 = sync_time()
                for _ in range(steps):
                    step()
                ms = 1e3 * (sync_time() - t0) / steps
                rows[form].append(ms)
                out(part="cycle", form=form, run=r, max_rows=max_rows, ms_per_cycle=ms)
                dec = eng = step = None
        out(part="cycle", summary=True, max_rows=max_rows, decoder_ms=statistics.median(rows["decoder"]),
            engine_ms=statistics.median(rows["engine"]), spread_decoder_ms=max(rows["decoder"]) - min(rows["decoder"]),
            spread_engine_ms=max(rows["engine"]) - min(rows["engine"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--prefix", type=int, default=1024)
    ap.add_argument("--part", default="throughput,admission,cycle", help="comma list of throughput, admission, cycle, trace")
    ap.add_argument("--form", choices=["admit", "fused"], default="fused", help="--part trace: which admission to run")
    ap.add_argument("--admissions", type=int, default=8, help="--part trace: admissions to run (two runs with different "
                    "counts give the per-admission figures by difference)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    spec = bench.workload_spec("qwen3-8b")
    args = SimpleNamespace(target_layers=0, hf_verify=False, hf_prefill=False, attn_impl="head", fuse_oproj=False)
    target, draft, cfg, perm, meta = bench.build_models(args, spec, 0, dev)
    out(part="setup", argv=sys.argv[1:], workload="qwen3-8b", prefix=a.prefix, block=BS, runs=a.runs,
        graph=os.environ.get("DFL_GRAPH", "1") != "0")
    parts = dict(throughput=part_throughput, admission=part_admission, cycle=part_cycle, trace=part_trace)
    for name in a.part.split(","):
        parts[name](a, draft, target, cfg, perm, meta["V"], dev)


if __name__ == "__main__":
    main()
