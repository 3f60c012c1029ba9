"""min_p through the decode loops: single request, policy, a 24-row block, ragged batch, slot-refill
engine — on the tiny walk target of test_hip_penalties_loops.py (helpers copied, not imported).

Truth is teacher-forced: one HF forward over the emitted ids gives the raw rows, min_p_ref.py the masked row, and every
emitted token must be the seeded draw over that row (sampling_ref.draw) wherever the screen holds: the draw's perturbed
gap exceeds 0.1 and no finite column lies within 4 bf16 ulp of the min_p threshold (the HF rows and the kernels' rows
differ by a rounding, which may move such a column across the floor).

On the reference alone (autoregressive on a CPU, T = 0.7, 120 new tokens, seed 5; profiles/min_p_tests.txt):
  min_p = 0.5   exactly 1 column kept in every row, screen keeps 1.000: the run is the greedy walk
  min_p = 0.3   mean 1.05 kept (max 4), screen keeps 0.983, 2 rows with a column at the threshold
  min_p <= 0.1  every column kept, screen keeps 0.875: the run without min_p
  0.20 - 0.27 leave a column at the threshold in most rows of this target and are not audited.
Caps: >= 0.95 of the positions screened in at 0.5 and 0.3, >= 0.85 at <= 0.1 (the plain draw's cap elsewhere).  Every audit
compares the ids first; the caps are asserted last in each test (_caps_hold).

The default prompt at seed 5 is audited at 0.5 only.  At 0.3 its reference run on the GPU's HF rows settles on 6-cycles in
which 15 of 120 rows hold a column within 4 bf16 ulp of the floor (maximum 0.9844, floor 0.843 below it, columns at 0.1426
/ 0.1387) and the screen keeps 0.867, below the cap, whatever emits the ids (on a CPU's HF rows, which differ by a rounding
of the maximum, it keeps 0.983).  The 0.3 cases therefore run on prompts chosen on the reference alone for a walk that keeps
clear of the floor (P03 below; the batch and engine cases likewise), with the caps as stated."""
import numpy as np
import pytest
import torch

import helpers as H
import logit_bias_ref as LB
import min_p_ref as MR
import nucleus_ref as NR
import penalties_ref as PR
import sampling_ref as SR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048
T = 0.7
N_IN, N_NEW = 41, 120
SEED = 5
_STATE = {}


def dev():
    return torch.device("cuda", 0)


def _walk_target():
    """The greedy-walk target (6 layers, walk seed 8) with lm_head row perm[t] = 0.002 * embedding[t] for a permutation of
    6-cycles over the ids 0..2045 (2046 <-> 2047: the mask id is on no prompt's walk)."""
    if "hf" not in _STATE:
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        torch.manual_seed(11)
        hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev(), dtype=BF16)
        impose_greedy_walk(hf, seed=8)
        order = torch.randperm(V - 2, generator=torch.Generator().manual_seed(8))
        perm = torch.arange(V)
        for i in range(V - 2):
            perm[order[i]] = order[6 * (i // 6) + (i + 1) % 6]
        perm[V - 2], perm[V - 1] = V - 1, V - 2
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(V)
        with torch.no_grad():
            emb = hf.model.embed_tokens.weight.float()
            hf.lm_head.weight.copy_((emb[inv.to(dev())] * 0.002).to(BF16))
        _STATE["hf"], _STATE["perm"] = hf, perm.tolist()
    return _STATE["hf"], _STATE["perm"]


def _native():
    from dflash_amd import NativeTarget
    return NativeTarget(_walk_target()[0])


def _draft_model(cfg):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return m


def _plan():
    return H.make_plan(400, 16, 29)


def _put(blk, toks):
    if toks:
        blk[0, 1:1 + len(toks)] = torch.tensor(toks, dtype=blk.dtype, device=blk.device)


def _walk_hook(perm, plan):
    """Drafts scripted from the RAW walk of the block's first token: plan[call] walk tokens, then a wrong one."""
    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        b, toks = int(blk[0, 0]), []
        for _ in range(k):
            b = perm[b]
            toks.append(b)
        if k + 1 < blk.shape[1]:
            toks.append((perm[b] + 1) % (V - 2))
        _put(blk, toks)
    return hook


def _script(sizes=(8, 12, 16)):
    from dflash_amd.generate import _Fixed
    a, b, c = sizes

    class Script(_Fixed):
        def select(self, cyc):
            return (c, a, b, c, b, a)[cyc % 6]

    s = Script(c)
    s.candidates = tuple(sizes)
    return s


def _prompt(seed=3, n=N_IN):
    return torch.randint(0, 2000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev())


def _cycle(t):
    _, perm = _walk_target()
    out = [t]
    for _ in range(5):
        out.append(perm[out[-1]])
    return out


def _fallback():
    """Three fallback tokens whose 6-cycles are disjoint from one another and from the cycles the test prompts walk (the
    set test_hip_logit_bias_loops.py uses)."""
    if "fb" not in _STATE:
        prot = set()
        for s, n in ((3, 41), (4, 37), (5, 45)):
            prot |= set(_cycle(int(_prompt(s, n)[0, -1])))
        fb = []
        for t in range(100, 1900):
            c = set(_cycle(t))
            if not c & prot:
                fb.append(t)
                prot |= c
            if len(fb) == 3:
                break
        _STATE["fb"] = fb
    return _STATE["fb"]


# ------------------------------------------------------------------------------------------------------------ the model
def _raw_rows(ids, n_in):
    hf, _ = _walk_target()
    with torch.inference_mode():
        logits = hf(torch.tensor([ids], device=dev())).logits[0].float().cpu().numpy()
    return PR.f32_to_bf16_bits(logits[n_in - 1:len(ids) - 1]).reshape(len(ids) - n_in, V)


def _near_threshold(zbits, L, invT):
    """A finite column within 4 bf16 ulp (of its own size) of the floor."""
    x = MR.widen(zbits)
    m = MR.row_max(x)
    with np.errstate(invalid="ignore", over="ignore"):
        dd = ((x - m).astype(np.float32) * invT).astype(np.float32)
        ulp = np.abs(x) * 2.0 ** -7 + 1e-30
        return bool((np.isfinite(x) & (x != m) & (np.abs(dd - L) <= 4 * ulp * invT)).any())   # (the maximum is kept by rule)


def _cap(min_p):
    return 0.85 if (min_p or 0) <= 0.1 else 0.95


def _audit(ids, n_in, min_p, seed, *, temperature=T, cap=None, bias=None, pen=None, top_p=1.0):
    """Every emitted token against the seeded draw over the model's row for its prefix: logit bias, penalties, min_p, then
    top_p over what min_p kept.  Returns (emitted, screen, kept per row)."""
    x = _raw_rows(ids, n_in)
    L, invT = MR.log_min_p(min_p), MR.inv_t(temperature)
    got = np.asarray(ids[n_in:])
    want, safe, kept = np.zeros(len(got), dtype=np.int64), np.zeros(len(got), dtype=bool), np.zeros(len(got), dtype=np.int64)
    for i in range(len(got)):
        p = n_in + i
        z = x[i]
        if bias is not None:
            z = LB.process(z, bias, p, 0, ())
        if pen is not None:
            z = PR.penalise(z, *PR.history(ids, n_in, p, V), *pen)
        near = np.isfinite(L) and _near_threshold(z, L, invT)
        zb, kept[i] = MR.process(z, L, invT)
        xm = MR.widen(zb)[None]
        if top_p < 1.0:   # the nucleus screen: the same draw over the nuclei of P (1 + eps) and P (1 - eps).  4 bf16 ulp of a
            # logit of size <= 1 move a column's share of the mass by at most 4 * 2^-8 / T = 2.2 %: eps = 0.025.  (The
            # threshold +- 4 ulp of test_hip_nucleus_loops.py is for rows of thousands of columns: over the 2..4 that min_p
            # leaves here, "threshold + 4 ulp" drops the nucleus' last member and screens out every row that draws it)
            tlo, thi = NR.top_p_thresholds(xm[0], temperature, [top_p * 1.025, top_p * 0.975], float("-inf"))
            lo, gl = NR.draw_over(xm, [tlo], temperature, seed, SR.TARGET, [p])
            hi, gh = NR.draw_over(xm, [thi], temperature, seed, SR.TARGET, [p])
            want[i], ok = lo[0], lo[0] == hi[0] and gl[0] > 0.1 and gh[0] > 0.1
        else:
            w, g = SR.draw(xm, temperature, seed, SR.TARGET, [p])
            want[i], ok = w[0], g[0] > 0.1
        safe[i] = bool(ok) and not near
    cap = _cap(min_p) if cap is None else cap
    print(f"[min_p] audit of {len(got)} positions at min_p = {min_p}: screen keeps {safe.mean():.3f} (cap {cap}), "
          f"kept mean {kept.mean():.2f} max {kept.max()}")
    assert np.array_equal(got[safe], want[safe]), (np.nonzero(safe & (got != want))[0][:8], safe.mean())
    _STATE.setdefault("shares", []).append((min_p, float(safe.mean()), cap))      # asserted by _caps_hold, last in each test
    return got, safe, kept


def _caps_hold():
    """The share of positions each audit of this test screened in, against its cap — asserted after everything else, so
    that a screen that drops too many positions does not hide what the comparisons of the test say."""
    low = [s for s in _STATE.get("shares", []) if s[1] < s[2]]
    assert not low, f"(min_p, share of positions screened in, cap): {low}"


def _same_until_a_near_tie(a, b):
    """Two audited runs of one request: a divergence may only start at a position either screen left out."""
    ga, sa, gb, sb = a[0], a[1], b[0], b[1]
    n = min(len(ga), len(gb))
    diff = np.nonzero(ga[:n] != gb[:n])[0]
    if diff.size:
        assert not (sa[diff[0]] and sb[diff[0]]), diff[0]


# ------------------------------------------------------------------------------------------------------------ the runs
@pytest.fixture(autouse=True)
def graphs():
    """Sessions hold their hipGraphs: collect them with the test, so that no capture state outlives this file's tests."""
    import gc
    _STATE["shares"] = []
    yield
    gc.collect()


def _single(kind, monkeypatch, hook, *, graph=True, temperature=T, seed=SEED, n_new=N_NEW, prompt=None, bs=16, **kw):
    from dflash_amd import dflash_generate, dflash_generate_policy
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    cfg = H.tiny_cfg()
    prompt = _prompt() if prompt is None else prompt
    skw = dict(sampler="device", seed=seed) if temperature >= 1e-5 else {}
    if kind == "generate":
        return dflash_generate(_draft_model(cfg), _native(), prompt, cfg.mask_token_id, n_new, bs, None, temperature,
                               draft_token_hook=hook, **skw, **kw)
    return dflash_generate_policy(model=_draft_model(cfg), target=_native(), input_ids=prompt,
                                  mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, stop_token_ids=None,
                                  temperature=temperature, scheduler=_script(), draft_token_hook=hook, **skw, **kw)


def _ids(r):
    return r.output_ids[0].tolist()


def _hook():
    return _walk_hook(_walk_target()[1], _plan())


def _full(r, n_in=N_IN, n_new=N_NEW):
    ids = _ids(r)
    assert len(ids) == n_in + n_new, "a run drew the mask id: pick another seed"
    return ids


# ------------------------------------------------------------------------------------------------------------ tests
def test_half_is_the_greedy_walk(monkeypatch):
    """min_p = 0.5 at T = 0.7 leaves one column in every row of this target: the ids of the T = 0 run, exactly."""
    greedy = _full(_single("generate", monkeypatch, _hook(), temperature=0.0))
    r = _single("generate", monkeypatch, _hook(), min_p=0.5)
    assert _full(r) == greedy and r.replayed_cycles > 0
    got, safe, kept = _audit(_ids(r), N_IN, 0.5, SEED)
    assert (kept == 1).all()
    plain = _full(_single("generate", monkeypatch, _hook()))
    assert plain != greedy                                   # (the draws at T = 0.7 do leave the walk without the floor)
    _caps_hold()


# min_p = 0.3 is audited on a prompt chosen on the REFERENCE alone (the HF forward on the GPU, min_p_ref, sampling_ref; no
# kernel of the project; profiles/min_p_tests.txt): its walk keeps clear of the floor (the screen keeps 0.975 of 120
# positions at seed 5) and still has rows in which the floor leaves several columns (5 rows, up to 30 columns).  On the
# default prompt the same reference run meets, every six positions, rows with a column within 4 bf16 ulp of the floor: the
# screen keeps 0.867 there, below the cap, whatever emits the ids.
P03 = (22, 43)


def _single03(kind, monkeypatch, hook, **kw):
    return _single(kind, monkeypatch, hook, prompt=_prompt(*P03), min_p=0.3, **kw)


def _audit03(r):
    a = _audit(_full(r, P03[1]), P03[1], 0.3, SEED)
    assert (a[2] > 1).sum() >= 3                     # the floor is in play: rows that keep more than the maximum
    return a


def test_block_16_against_block_1_eager_against_replayed(monkeypatch):
    """min_p = 0.3: a scripted draft in blocks of 16 against block size 1 (no draft at all); eager against replayed."""
    ref = _single03("generate", monkeypatch, _hook(), graph=False)
    rep = _single03("generate", monkeypatch, _hook(), graph=True)
    one = _single03("generate", monkeypatch, _hook(), graph=False, bs=1)
    assert _ids(rep) == _ids(ref) and list(rep.acceptance_lengths) == list(ref.acceptance_lengths)
    assert rep.replayed_cycles > 0 and ref.replayed_cycles == 0 and max(ref.acceptance_lengths) > 6
    _same_until_a_near_tie(_audit03(ref), _audit03(one))
    assert set(one.acceptance_lengths) == {1}
    _caps_hold()


def test_policy_loop(monkeypatch):
    ref = _single03("policy", monkeypatch, _hook(), graph=False)
    rep = _single03("policy", monkeypatch, _hook(), graph=True)
    assert _ids(rep) == _ids(ref) and rep.replayed_cycles > 0
    _same_until_a_near_tie(_audit03(rep), _audit03(_single03("generate", monkeypatch, _hook())))
    _caps_hold()


def test_a_24_row_block(monkeypatch):
    long_hook = _walk_hook(_walk_target()[1], [23, 18, 7, 21])             # accepted spans reach into the second tile
    wide = _single03("generate", monkeypatch, long_hook, bs=24)
    _same_until_a_near_tie(_audit03(wide), _audit03(_single03("generate", monkeypatch, _hook())))
    assert max(wide.acceptance_lengths) > 16
    half = _single("generate", monkeypatch, long_hook, min_p=0.5, bs=24)
    assert _full(half) == _full(_single("generate", monkeypatch, long_hook, temperature=0.0, bs=24))
    assert max(half.acceptance_lengths) > 16
    _caps_hold()


MIXED = (0, 0.3, 0.5, 1.0)
PROMPTS4 = ((3, 41), P03, (4, 37), (6, 33))           # (0.3 goes to the prompt and seed audited above)
SEEDS4 = [21, SEED, 22, 24]


def test_batch_with_per_prompt_values(monkeypatch):
    """Four prompts with (0, 0.3, 0.5, 1.0): each passes the audit with its own value and agrees with its own
    single-request run (exactly where the floor leaves one column: 0.5 and 1.0 are that prompt's greedy run)."""
    from dflash_amd.batch import dflash_generate_batch
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    prompts = [_prompt(s, n) for s, n in PROMPTS4]
    hook = _hook()
    out = dflash_generate_batch(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, 80, 16, None, T,
                                draft_token_hook=lambda i, blk, start, call: hook(blk, start, call), sampler="device",
                                seed=SEEDS4, min_p=list(MIXED))
    for i, p in enumerate(prompts):
        n_in = p.shape[1]
        ids = _full(out[i], n_in, 80)
        a = _audit(ids, n_in, MIXED[i], SEEDS4[i])
        one = _single("generate", monkeypatch, hook, prompt=p, n_new=80, seed=SEEDS4[i], min_p=MIXED[i])
        _same_until_a_near_tie(a, _audit(_full(one, n_in, 80), n_in, MIXED[i], SEEDS4[i]))
        if MIXED[i] >= 0.5:
            greedy = _single("generate", monkeypatch, hook, prompt=p, n_new=80, temperature=0.0)
            assert ids == _ids(one) == _ids(greedy), i
    assert _ids(out[0]) != _ids(_single("generate", monkeypatch, hook, prompt=prompts[0], n_new=80, temperature=0.0))
    _caps_hold()


def _engine(monkeypatch, graph, values, flag=True, slots=3, n_new=60):
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    cfg = H.tiny_cfg()
    prompts = [_prompt(10 + i, 35 + i) for i in range(len(values))]
    eng = BatchEngine(_draft_model(cfg), _native(), slots=slots, max_rows=48 + n_new + 48, out_len=48 + n_new + 16,
                      mask_token_id=cfg.mask_token_id, block_size=16, temperature=T, sampler="device", **(
                          dict(min_p=True) if flag else {}))
    for i, p in enumerate(prompts):
        kw = {} if values[i] is None else dict(min_p=values[i])
        eng.submit(p, n_new, seed=60 + i, draft_token_hook=_hook(), **kw)
    res = eng.run()
    return prompts, res, eng.stats


def test_engine_under_refill(monkeypatch):
    """Six prompts over three slots, each with its own min_p: a slot's L is rewritten on every admission (a request at 0
    behind one at 0.5 in the same slot is not greedy); replay on and off emit the same ids; one capture serves the engine."""
    values = [0.5, 0.3, 0, 0, 1.0, 0.5]
    prompts, res, stats = _engine(monkeypatch, True, values)
    _, eager, st0 = _engine(monkeypatch, False, values)
    assert stats["captures"] == 1 and stats["replayed_cycles"] > 0 and st0["replayed_cycles"] == 0
    for i, r in enumerate(res):
        n_in = prompts[i].shape[1]
        ids = _full(r, n_in, 60)
        assert ids == _ids(eager[i]), i
        _, _, kept = _audit(ids, n_in, values[i], 60 + i)
        assert values[i] != 0.5 or (kept == 1).all(), i
        assert values[i] != 0 or (kept == V).all(), i
    slots_used = [r.slot for r in res]
    assert max(slots_used.count(s) for s in set(slots_used)) >= 2
    by_slot = {s: [i for i, r in enumerate(res) if r.slot == s] for s in set(slots_used)}
    assert any(values[a] != values[b] for idx in by_slot.values() for a, b in zip(idx, idx[1:]))
    _caps_hold()


def test_all_slots_at_zero_is_the_engine_without_the_flag(monkeypatch):
    values = [0, None, 0.0, 0]
    _, with_flag, _ = _engine(monkeypatch, True, values, flag=True, slots=2, n_new=40)
    _, without, _ = _engine(monkeypatch, True, [None] * 4, flag=False, slots=2, n_new=40)
    for a, b in zip(with_flag, without):
        assert _ids(a) == _ids(b) and list(a.acceptance_lengths) == list(b.acceptance_lengths)


# the combined case: logit bias -> penalties -> min_p -> top_p.  Penalties and min_p were chosen on the reference alone
# (the HF forward on the GPU and the numpy models, no kernel of the project; profiles/min_p_tests.txt): r = 1.1 and a = 0.05
# move the walk's token, once seen, from ~1.0 to ~0.86, and min_p = 0.65 puts the floor 0.30 below the maximum — in the gaps
# of the fallback set's +0.40 / +0.55 / +0.70, whichever the maximum is.  70 of 120 rows keep 2 or 3 columns and the draw
# is not forced; 3 rows have a column at the floor.  Without a frequency penalty the levels do not drift from row to row
# across the floor.  The reference's screen keeps 0.967 on this prompt (0.95 .. 0.967 on three prompts); the cap is the
# plain draw's, 0.85.
COMBO_PEN = (1.1, 0.05, 0.0)
COMBO_MIN_P = 0.65
COMBO_CAP = 0.85


def test_with_top_p_penalties_and_a_logit_bias(monkeypatch):
    from dflash_amd import ops
    fb = _fallback()
    mask = H.tiny_cfg().mask_token_id
    cfg = dict(logit_bias={fb[0]: 0.40, fb[1]: 0.55, fb[2]: 0.70}, banned_token_ids=[mask])
    kw = dict(min_p=COMBO_MIN_P, top_p=0.9, repetition_penalty=COMBO_PEN[0], presence_penalty=COMBO_PEN[1],
              frequency_penalty=COMBO_PEN[2], **cfg)
    bias = ops.check_logit_bias(V, cfg["logit_bias"], None, cfg["banned_token_ids"], 0, None)[0].numpy()
    akw = dict(cap=COMBO_CAP, bias=bias, pen=COMBO_PEN, top_p=0.9)
    ref = _single("generate", monkeypatch, _hook(), graph=False, **kw)
    rep = _single("generate", monkeypatch, _hook(), graph=True, **kw)
    assert _full(rep) == _full(ref) and rep.replayed_cycles > 0
    a = _audit(_ids(ref), N_IN, COMBO_MIN_P, SEED, **akw)
    assert ((a[2] >= 2) & (a[2] <= 4)).sum() >= 10 and mask not in _ids(ref)[N_IN:]      # the draw is not forced
    one = _single("generate", monkeypatch, _hook(), graph=False, bs=1, **kw)
    _same_until_a_near_tie(a, _audit(_full(one), N_IN, COMBO_MIN_P, SEED, **akw))
    _caps_hold()


def test_off_and_greedy_launch_nothing(monkeypatch):
    """min_p None / 0 launches no min_p_rows anywhere; T = 0 with min_p = 0.3 launches none either; 0.3 at T = 0.7 does."""
    from dflash_amd import ops
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import dflash_generate_stream
    calls = []
    real = ops.min_p_rows
    monkeypatch.setattr(ops, "min_p_rows", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    hook = _hook()
    cfg = H.tiny_cfg()
    prompts = [_prompt(s, n) for s, n in PROMPTS4[:2]]
    many = dict(draft_token_hook=lambda i, blk, start, call: hook(blk, start, call))
    for kind in ("generate", "policy"):
        base = _ids(_single(kind, monkeypatch, hook, n_new=40))
        for mp in (None, 0) if kind == "generate" else (0.0,):
            assert _ids(_single(kind, monkeypatch, hook, n_new=40, min_p=mp)) == base
        g = _ids(_single(kind, monkeypatch, hook, n_new=40, temperature=0.0))
        assert _ids(_single(kind, monkeypatch, hook, n_new=40, temperature=0.0, min_p=0.3)) == g
    assert _ids(_single("generate", monkeypatch, hook, n_new=40, bs=24, min_p=0)) == \
        _ids(_single("generate", monkeypatch, hook, n_new=40, bs=24))
    for fn in (dflash_generate_batch, dflash_generate_stream):
        base = fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, 30, 16, None, T, sampler="device", seed=[1, 2], **many)
        off = fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, 30, 16, None, T, sampler="device", seed=[1, 2],
                 min_p=[0, None], **many)
        assert [_ids(r) for r in off] == [_ids(r) for r in base]
        g0 = fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, 30, 16, None, 0.0, **many)
        g1 = fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, 30, 16, None, 0.0, min_p=0.3, **many)
        assert [_ids(r) for r in g1] == [_ids(r) for r in g0]
    assert not calls
    _single("generate", monkeypatch, hook, n_new=8, min_p=0.3)                      # (the spy sees a real launch)
    assert calls
