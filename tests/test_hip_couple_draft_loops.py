"""The coupled draft through the decode loops, on the soft walk target of test_hip_sampling.py
(helpers copied into couple_draft_common.py) and a draft model of random weights.

Such a draft's distribution has nothing to do with the target's, so coupling buys no acceptance here (the closed form of
section 20 says so for a q far from p); what these tests hold is the contract — every cycle's draft ids are the
reference's coupled draw over the session's own draft logits at p = start + j, in eager, run-ahead and replayed cycles —
and that nothing emitted changes.  The prompts, seeds and temperatures are those of test_hip_sampling.py and
test_hip_request_temperature_loops.py, whose audits keep >= 0.90 of the positions (the emitted ids do not depend on the
draft)."""
import numpy as np
import pytest
import torch

import couple_draft_common as C
import couple_draft_ref as CD
import grammar_ref as GR
import helpers as H
import sampling_ref as SR

pytestmark = pytest.mark.gpu
T = 0.7
V = 2048
N_IN = 41


@pytest.fixture(autouse=True)
def graphs():
    """Sessions, decoders and engines hold their hipGraphs, captured under inference mode: collect them with every test, so
    that no capture state outlives it (a graph captured later OUTSIDE inference mode, as tests/test_hip_grammar_draft.py
    does, fails while one of them is alive: the generator's capture words would be inference tensors)."""
    import gc
    yield
    gc.collect()


def _ids(r):
    return r.output_ids[0].tolist()


def _check_draft_ids(recs, seed, temperature=T, screen=1e-3, keep=0.95):
    """Every hook call: block[1:bs] is the coupled draw over the clone of the draft logits at p = start + j, wherever the
    draw's top-2 gap exceeds the screen.  The check tells the coupled draw from its two neighbours: the DRAFT-stream draw
    and the draw one position off each differ from it on at least a tenth of the slots (where they differ, the block
    holds the coupled id, not theirs)."""
    n = hits = own_diff = off_diff = 0
    for c, rec in enumerate(recs):
        x = GR.bits_to_f32(rec.x)
        want, gaps = CD.draw(x, temperature, seed, rec.start, rec.bs)
        safe = gaps[1:] > screen
        assert np.array_equal(rec.seen[1:rec.bs][safe], want[1:][safe]), (c, rec.start, rec.bs, rec.ahead)
        own, _ = CD.draw(x, temperature, seed, rec.start, rec.bs, stream=SR.DRAFT)
        off, _ = CD.draw(x, temperature, seed, rec.start + 1, rec.bs)
        n, hits = n + len(safe), hits + int(safe.sum())
        own_diff += int((own[1:] != want[1:])[safe].sum())
        off_diff += int((off[1:] != want[1:])[safe].sum())
    assert n and hits >= keep * n, (hits, n)
    assert own_diff >= 0.1 * n and off_diff >= 0.1 * n, (own_diff, off_diff, n)


# ------------------------------------------------------------------------------------------------------------ launch forms
def test_draft_ids_in_eager_run_ahead_and_replayed_cycles(monkeypatch):
    """Fixed loop, block 16, T = 0.7: the draft ids of every cycle against the reference; eager (with run-ahead), replayed
    and no-run-ahead runs give identical ids and acceptance lengths; the replayed run replayed, run-ahead drafts were
    taken, and against couple_draft=False the emitted ids agree up to a screened-out near-tie."""
    runs = {}
    for name, (graph, ahead) in dict(eager=(False, True), replayed=(True, True), noahead=(True, False)).items():
        r, recs, flags = C.recorded_run(monkeypatch, graph=graph, run_ahead=ahead, seed=5, n_new=100, couple_draft=True)
        _check_draft_ids(recs, 5)
        runs[name] = (r, recs, flags)
    ref = runs["eager"][0]
    for name in ("replayed", "noahead"):
        assert _ids(runs[name][0]) == _ids(ref) and runs[name][0].acceptance_lengths == ref.acceptance_lengths, name
    assert runs["replayed"][0].replayed_cycles > 0 and any(runs["replayed"][2])
    assert ref.replayed_cycles == 0 and any(rec.ahead for rec in runs["eager"][1])     # a run-ahead draft really was taken
    assert not any(rec.ahead for rec in runs["noahead"][1])
    off, _, _ = C.recorded_run(monkeypatch, seed=5, n_new=100)
    C.same_until_a_near_tie(C.audit(_ids(ref), N_IN, 5), C.audit(_ids(off), N_IN, 5), "coupled against greedy draft")


def test_policy_loop_draft_ids_and_replay(monkeypatch):
    """The policy loop (sizes 8 / 12 / 16 scripted): couple_draft replaces its DRAFT-stream draw; eager and replayed
    (capture_sizes) runs give the same ids and acceptance lengths, every cycle's draft the reference's coupled draw."""
    ra, recs_a, _ = C.recorded_run(monkeypatch, kind="policy", graph=False, seed=5, n_new=100, couple_draft=True)
    rb, recs_b, flags = C.recorded_run(monkeypatch, kind="policy", graph=True, seed=5, n_new=100, couple_draft=True)
    _check_draft_ids(recs_a, 5)
    _check_draft_ids(recs_b, 5)
    assert _ids(ra) == _ids(rb) and ra.acceptance_lengths == rb.acceptance_lengths
    assert rb.replayed_cycles > 0 and {rec.bs for rec in recs_b} >= {8, 12, 16}
    C.audit(_ids(ra), N_IN, 5)


# ------------------------------------------------------------------------------------------------------------ losslessness
@pytest.mark.parametrize("mode", ["bs16", "bs24", "policy"])
def test_single_request_audit_is_lossless(mode, monkeypatch):
    """couple_draft=True at T = 0.7: the teacher-forced audit with gap 0.1 keeps >= 0.90 and every kept position is the
    target's own seeded draw; against couple_draft=False with the same seed a divergence starts only at a near-tie."""
    kw = dict(bs16=dict(bs=16), bs24=dict(bs=24), policy=dict(kind="policy"))[mode]
    on, recs, _ = C.recorded_run(monkeypatch, seed=5, n_new=120, couple_draft=True, **kw)
    off, _, _ = C.recorded_run(monkeypatch, seed=5, n_new=120, **kw)
    if mode == "bs24":
        _check_draft_ids(recs, 5)          # two tiles: the host's start, the second tile 16 positions further on
    C.same_until_a_near_tie(C.audit(_ids(on), N_IN, 5), C.audit(_ids(off), N_IN, 5), mode)


REQS = ((3, 41, 0.7, 31), (5, 9, 0.0, 0), (6, 120, 0.5, 34))      # prompt seed, length, temperature, seed


def test_batch_with_per_request_temperatures_is_lossless(monkeypatch):
    """dflash_generate_batch, three prompts at T = 0.7 / 0 / 0.5 (one decoder with request_temperature): the sampled
    requests pass the audit at their own temperature and agree with the run without the keyword up to a near-tie; the
    greedy request emits the ids of the run without it.  (The heads' per-slot noise is test_hip_couple_draft.py's.)"""
    from dflash_amd.batch import dflash_generate_batch
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    prompts = [C.prompt(s, n) for s, n, _, _ in REQS]
    temps, seeds = [r[2] for r in REQS], [r[3] for r in REQS]
    seen = []
    outs = {}
    for on in (True, False):
        hook = (lambda i, blk, start, call: seen.append((i, int(start), blk[0].cpu().numpy().copy()))) if on else None
        outs[on] = dflash_generate_batch(C.draft_model(cfg), C.native(), prompts, cfg.mask_token_id, 80, 16, None, temps,
                                         sampler="device", seed=seeds, couple_draft=on, draft_token_hook=hook)
    for i, (_, n_in, t, sd) in enumerate(REQS):
        a, b = _ids(outs[True][i]), _ids(outs[False][i])
        if t == 0.0:
            assert a == b, i
        else:
            C.same_until_a_near_tie(C.audit(a, n_in, sd, t), C.audit(b, n_in, sd, t), i)
    assert {i for i, _, _ in seen} == {0, 1, 2}


def test_engine_under_refill_is_lossless(monkeypatch):
    """dflash_generate_stream with two slots and three prompts at T = 0.7 (the third is admitted into a freed slot, the
    cycles replayed from the engine's one capture): every request passes the audit and agrees with the run without the
    keyword up to a near-tie."""
    from dflash_amd.engine import dflash_generate_stream
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    lens = [(3, 41), (4, 37), (5, 45)]
    prompts = [C.prompt(s, n) for s, n in lens]
    seeds = [31, 2 ** 63 + 9, 33]
    outs = {on: dflash_generate_stream(C.draft_model(cfg), C.native(), prompts, cfg.mask_token_id, [60, 30, 60], 16, None, T,
                                       slots=2, sampler="device", seed=seeds, couple_draft=on) for on in (True, False)}
    for i, (_, n_in) in enumerate(lens):
        C.same_until_a_near_tie(C.audit(_ids(outs[True][i]), n_in, seeds[i]), C.audit(_ids(outs[False][i]), n_in, seeds[i]), i)


# ------------------------------------------------------------------------------------------------------------ with a grammar
NS = 37
SEQ = torch.randperm(2000, generator=torch.Generator().manual_seed(37))[:NS].tolist()
EVEN = list(range(0, V, 2))


def _mixed():
    """tests/test_hip_grammar_draft_loops.py::_mixed: every third state is free over the even tokens, the others are
    forced to SEQ[i]; all lead to state i + 1."""
    from dflash_amd import TokenDFA
    nxt = np.full((NS, V), -1, dtype=np.int16)
    for i in range(NS):
        if i % 3 == 0:
            nxt[i, EVEN] = (i + 1) % NS
        else:
            nxt[i, SEQ[i]] = (i + 1) % NS
    return TokenDFA(nxt, start=0)


@pytest.mark.parametrize("kind", ["fixed", "policy"])
def test_grammar_with_constrained_coupled_draft(kind, monkeypatch):
    """grammar= with constrain_draft=True and couple_draft=True at T = 0.7 (the policy loop too: its draft counts as
    greedy now): the emitted ids walk the automaton; every cycle's block, eager, run-ahead and replayed, is the noise-form
    reference's pick over the session's draft logits from the slot's state at p = start + m; the forced states are
    proposed exactly, so the acceptance lengths are far above those of the unconstrained coupled draft."""
    g = _mixed()
    kinds = set()
    res = {}
    for graph in (False, True):
        r, recs, flags = C.recorded_run(monkeypatch, kind=kind, graph=graph, seed=5, n_new=80, grammar=g,
                                        constrain_draft=True, couple_draft=True)
        assert r.grammar_state is not None and r.grammar_state >= 0
        assert GR.walk(g.next, 0, g.start, _ids(r)[N_IN:]) == r.grammar_state
        assert len(recs) >= 3
        for c, rec in enumerate(recs):
            blk0 = rec.seen.copy()
            want, _, gaps = CD.pick(rec.x, rec.bs, blk0, seed=5, inv_t=SR.inv_t(T), pos0=rec.start, pool=g.next, base=0,
                                    state=rec.state)
            ok = np.ones(rec.bs, bool)
            for m, gap in enumerate(gaps, start=1):       # behind a near-tie the walk may part: compare up to it
                if gap <= 1e-3:
                    ok[m:] = False
                    break
            assert np.array_equal(rec.seen[:rec.bs][ok], want[:rec.bs][ok]), (c, rec.state, rec.ahead)
            assert GR.walk(g.next, 0, rec.state, rec.seen[1:rec.bs]) >= 0, c
        kinds |= {"replayed" if f else ("run-ahead" if rec.ahead else "eager") for rec, f in zip(recs, flags)}
        res[graph] = r
    assert _ids(res[False]) == _ids(res[True]) and res[False].acceptance_lengths == res[True].acceptance_lengths
    assert res[True].replayed_cycles > 0
    assert kinds >= ({"eager", "run-ahead", "replayed"} if kind == "fixed" else {"eager", "replayed"}), kinds
    plain, _, _ = C.recorded_run(monkeypatch, kind=kind, seed=5, n_new=80, grammar=g, couple_draft=True)
    assert np.mean(res[True].acceptance_lengths) > 1.5 * np.mean(plain.acceptance_lengths)
    assert GR.walk(g.next, 0, g.start, _ids(plain)[N_IN:]) >= 0
