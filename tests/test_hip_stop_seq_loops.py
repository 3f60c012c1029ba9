"""Stop sequences through the decode loops: single request, policy, spec_generate on a wrapped
target, ragged batch and slot-refill engine — on the tiny walk target of test_hip_sampling.py (helpers copied, not
imported), draft_token_hook scripting the acceptance.

Truth is the run's own free continuation: a run without stops gives the ids; a sequence is cut out of them at a place
where it occurs for the first time (searched on the host, windows inside the prompt excluded); the run with
stop_sequences must emit exactly the prefix up to and including it, on the cycle that commits it."""
import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048
T = 0.7
N_IN = 41
_STATE = {}


def dev():
    return torch.device("cuda", 0)


def _walk_target(scale=0.62):
    """The greedy-walk target (synthetic.impose_greedy_walk) with its lm_head scaled down: the walk's next token keeps
    probability ~0.75 - 0.8 at T = 0.7 instead of ~1, so the draws are genuinely random."""
    if "hf" not in _STATE:
        from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
        torch.manual_seed(11)
        hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev(), dtype=BF16)
        perm = impose_greedy_walk(hf, seed=8)
        with torch.no_grad():
            hf.lm_head.weight.mul_(scale)
        _STATE["hf"], _STATE["perm"] = hf, perm.cpu().tolist()
    return _STATE["hf"], _STATE["perm"]


def _native():
    from dflash_amd import NativeTarget
    return NativeTarget(_walk_target()[0])


def _draft_model(cfg):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return m


def _hook(plan=None):
    """Drafts scripted from the walk of the block's first token: plan[call] walk tokens, then a wrong one."""
    perm = _walk_target()[1]
    plan = H.make_plan(400, 16, 29) if plan is None else plan

    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        b = int(blk[0, 0])
        toks = []
        for _ in range(k):
            b = perm[b]
            toks.append(b)
        if k + 1 < blk.shape[1]:
            toks.append((perm[b] + 1) % V)
        if toks:
            blk[0, 1:1 + len(toks)] = torch.tensor(toks, dtype=blk.dtype, device=blk.device)
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


@pytest.fixture
def graphs():
    """Sessions hold their hipGraphs: collect them with the test, so that no capture state outlives this file's tests."""
    import gc
    yield
    gc.collect()


def _run(kind, monkeypatch, *, graph, temperature=0.0, n_new=160, **kw):
    """run_decode as dflash_generate / dflash_generate_policy call it."""
    from dflash_amd.generate import run_decode
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    cfg = H.tiny_cfg()
    skw = dict(sampler="device", seed=13) if temperature >= 1e-5 else {}
    if kind == "policy":
        skw.update(scheduler=_script(), draft_temperature=temperature, max_block_size=16)
    r = run_decode(_draft_model(cfg), _native(), _prompt(), mask_token_id=cfg.mask_token_id, max_new_tokens=n_new,
                   stop_token_ids=None, temperature=temperature, block_size=16, clamp_tail=True, draft_token_hook=_hook(),
                   **skw, **kw)
    r.ids = r.output_ids[0].tolist()
    return r


def first_end(ids, seq, n_in):
    """The end position of the first window of ids that equals seq and does not begin inside the prompt, or None."""
    L = len(seq)
    for e in range(n_in + L - 1, len(ids)):
        if ids[e - L + 1:e + 1] == list(seq):
            return e
    return None


def absent(ids, n_in):
    """A two-id sequence of the run's own tokens that never occurs in it."""
    for a in ids[n_in:]:
        for b in ids[n_in:]:
            if first_end(ids, [a, b], n_in) is None:
                return [a, b]
    raise AssertionError("no absent pair")


# ------------------------------------------------------------------------------------------------------------ one request
@pytest.mark.parametrize("kind, temperature", [("fixed", 0.0), ("fixed", T), ("policy", T)])
def test_mid_block_bonus_and_across_cycles(kind, temperature, monkeypatch, graphs):
    """A sequence that ends mid-block, one that ends on the bonus token and one that begins in the cycle before: the ids
    are the free run's prefix up to and including it, eager and replayed runs agree in ids and in the number of
    cycles, the stopping cycle is the one that commits the sequence's last id, and it was replayed."""
    free = _run(kind, monkeypatch, graph=True, temperature=temperature)
    ids, taus, flags = free.ids, list(free.acceptance_lengths), list(free.replayed_flags)
    assert free.stop_sequence is None and len(ids) == N_IN + 160
    starts = N_IN + np.concatenate([[0], np.cumsum(taus)[:-1]])   # cycle c commits positions starts[c] + 1 .. + taus[c]
    decoy = absent(ids, N_IN)

    def cases_of(c):
        s, t = int(starts[c]), int(taus[c])
        return {"mid": (ids[s + 1:s + 3], s + 2), "bonus": (ids[s + t - 2:s + t + 1], s + t),
                "across": (ids[s - 1:s + 2], s + 1)}

    ok = [c for c in range(4, len(taus)) if flags[c] and taus[c] >= 4
          and all(first_end(ids, q, N_IN) == e for q, e in cases_of(c).values())]
    assert ok, (taus, flags)
    c = ok[len(ok) // 2]
    for name, (seq, e) in cases_of(c).items():
        kw = dict(temperature=temperature, stop_sequences=[decoy, seq])
        eager = _run(kind, monkeypatch, graph=False, **kw)
        rep = _run(kind, monkeypatch, graph=True, **kw)
        assert eager.ids == ids[:e + 1], name
        assert rep.ids == eager.ids and list(rep.acceptance_lengths) == list(eager.acceptance_lengths), name
        assert len(rep.acceptance_lengths) == c + 1 and rep.replayed_flags[c], (name, c, rep.replayed_flags[-3:])
        assert eager.stop_sequence == 1 and rep.stop_sequence == 1, name
    # the matched ids cut off as well; logprobs follow the ids' columns
    seq, e = cases_of(c)["bonus"]
    for include in (True, False):
        r = _run(kind, monkeypatch, graph=True, temperature=temperature, stop_sequences=[seq], include_stop_sequence=include,
                 logprobs=1)
        n_out = e + 1 - N_IN - (0 if include else len(seq))
        assert r.ids == ids[:N_IN + n_out] and r.stop_sequence == 0 and r.num_output_tokens == n_out
        assert r.logprobs.shape == (n_out,) and r.top_logprob_ids.shape == (n_out, 1)
        assert bool(torch.isfinite(r.logprobs).all())


def test_first_token_and_min_tokens(monkeypatch, graphs):
    """A length-1 sequence equal to the first new token stops the request before any cycle runs, as a stop id does; with
    min_tokens the same id stops at its first occurrence at or behind the minimum."""
    free = _run("fixed", monkeypatch, graph=True, n_new=60)
    first = free.ids[N_IN]
    r = _run("fixed", monkeypatch, graph=True, n_new=60, stop_sequences=[first])
    assert r.ids == free.ids[:N_IN + 1] and r.stop_sequence == 0 and list(r.acceptance_lengths) == []
    r = _run("fixed", monkeypatch, graph=True, n_new=60, stop_sequences=[[first]], include_stop_sequence=False)
    assert r.ids == free.ids[:N_IN] and r.stop_sequence == 0
    # a pair whose first occurrence ends at output index 9: min_tokens = 9 still allows it (9 tokens are out before its
    # last id), min_tokens = 11 does not, and the run goes on to the end (the pair occurs once)
    seq = free.ids[N_IN + 8:N_IN + 10]
    assert first_end(free.ids, seq, N_IN) == N_IN + 9 and first_end(free.ids[N_IN + 10:], seq, 0) is None
    r = _run("fixed", monkeypatch, graph=True, n_new=60, stop_sequences=[seq], min_tokens=9)
    assert r.ids == free.ids[:N_IN + 10] and r.stop_sequence == 0
    r = _run("fixed", monkeypatch, graph=True, n_new=60, stop_sequences=[seq], min_tokens=11)
    assert r.ids == free.ids and r.stop_sequence is None


def test_spec_generate_with_the_hf_target(monkeypatch, graphs):
    """The launch never reads the logits: a wrapped transformers model will do."""
    hf, _ = _walk_target()
    cfg = H.tiny_cfg()
    m = _draft_model(cfg)
    free = m.spec_generate(hf, _prompt(), 60, None, 0.0, draft_token_hook=_hook())[0].tolist()
    seq = free[N_IN + 20:N_IN + 23]
    e = first_end(free, seq, N_IN)
    assert e == N_IN + 22
    got = m.spec_generate(hf, _prompt(), 60, None, 0.0, draft_token_hook=_hook(), stop_sequences=[seq])[0].tolist()
    assert got == free[:e + 1]
    got = m.spec_generate(hf, _prompt(), 60, None, 0.0, draft_token_hook=_hook(), stop_sequences=[seq],
                          include_stop_sequence=False)[0].tolist()
    assert got == free[:e - 2]


def test_the_multi_candidate_loop_refuses(graphs):
    from dflash_amd.candidates import dflash_generate_candidate_solutions
    cfg = H.tiny_cfg()
    with pytest.raises(NotImplementedError, match="stop_sequences"):
        dflash_generate_candidate_solutions(_draft_model(cfg), _native(), _prompt(), cfg.mask_token_id, 20, 16, None,
                                            stop_sequences=[[5, 6]])


# ------------------------------------------------------------------------------------------------------------ the launches
class Recorder:
    """In place of dflash_amd._lib._lib: every C entry called is appended to .names and forwarded."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*a):
            self.names.append(name)
            return fn(*a)
        return call

    def take(self):
        out, self.names = self.names, []
        return out


@pytest.fixture
def rec():
    from dflash_amd import _lib
    real = _lib.lib()
    r = Recorder(real)
    _lib._lib = r
    try:
        yield r
    finally:
        _lib._lib = real


STOP = "dfl_stop_seq_rows"


def _without(names):
    return [n for n in names if n != STOP]


def test_launch_sequence_of_a_session(rec, graphs):
    """Off (None, or an empty list): not one launch more.  On: the first token's one-row launch in prefill(), then
    exactly one launch per cycle, directly in front of the accept launch — and nothing else changes."""
    from dflash_amd.generate import DecodeSession
    cfg = H.tiny_cfg()
    runs = {}
    for name, seqs in (("off", None), ("empty", []), ("on", [[5, 6, 7], [8]])):
        s = DecodeSession(_draft_model(cfg), _native(), _prompt(), mask_token_id=cfg.mask_token_id, max_new_tokens=60,
                          max_block_size=16, stop_token_ids=None, temperature=0.0, stop_sequences=seqs)
        rec.take()
        s.prefill()
        first = rec.take()
        s.cycle(16, ahead_ok=True)      # (with the next cycle's draft running ahead)
        s.cycle(16, ahead_ok=True)
        torch.cuda.synchronize()
        runs[name] = (first, rec.take())
        assert (s.sq is None) == (name != "on")
    for name in ("off", "empty"):
        assert STOP not in runs[name][0] + runs[name][1]
        assert runs[name] == runs["off"]
    first, cyc = runs["on"]
    assert first.count(STOP) == 1 and _without(first) == runs["off"][0]
    assert cyc.count(STOP) == 2 and _without(cyc) == runs["off"][1]
    assert all(cyc[i + 1] == "dfl_accept_commit" for i, n in enumerate(cyc) if n == STOP)
    assert all(cyc[i - 1] == STOP for i, n in enumerate(cyc) if n == "dfl_accept_commit")


def test_launch_sequence_of_a_decoder(rec, graphs):
    from dflash_amd.batch import BatchedDecoder
    cfg = H.tiny_cfg()
    runs = {}
    for flag in (False, True):
        dec = BatchedDecoder(_draft_model(cfg), _native(), 2, 256, 200, cfg.mask_token_id, stop_sequences=flag)
        rec.take()
        dec.admit(0, _prompt(3, 41), stop_sequences=[[5, 6]] if flag else None)
        dec.admit_fused(1, _prompt(4, 37))
        adm = rec.take()
        dec.cycle()
        dec.cycle(ahead_ok=True)
        torch.cuda.synchronize()
        runs[flag] = (adm, rec.take())
    assert STOP not in runs[False][0] + runs[False][1]
    adm, cyc = runs[True]
    assert adm.count(STOP) == 1 and _without(adm) == runs[False][0]      # (the slot without sequences checks no first token)
    assert cyc.count(STOP) == 2 and _without(cyc) == runs[False][1]
    assert all(cyc[i + 1] == "dfl_accept_commit_batch" for i, n in enumerate(cyc) if n == STOP)
    assert all(cyc[i - 1] == STOP for i, n in enumerate(cyc) if n == "dfl_accept_commit_batch")


# ------------------------------------------------------------------------------------------------------------ many requests
PROMPTS = ((3, 41), (4, 37), (5, 45), (6, 39))


def _many(entry, monkeypatch, prompts, *, temperature=0.0, n_new=80, **kw):
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import dflash_generate_stream
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    fn = dflash_generate_batch if entry == "batch" else dflash_generate_stream
    extra = dict(slots=2) if entry == "stream" else {}
    skw = dict(sampler="device", seed=[31 + i for i in range(len(prompts))]) if temperature >= 1e-5 else {}
    hook = _hook()
    return fn(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, n_new, 16, None, temperature,
              draft_token_hook=lambda i, blk, start, call: hook(blk, start, call), **skw, **extra, **kw)


def _pick(ids, n_in, at, L=3):
    """A sequence of L ids of the run's own, the first from output index `at` on whose first occurrence is there."""
    for a in range(at, len(ids) - n_in - L):
        seq = ids[n_in + a:n_in + a + L]
        if first_end(ids, seq, n_in) == n_in + a + L - 1:
            return seq, n_in + a + L - 1
    raise AssertionError("no first occurrence")


@pytest.mark.parametrize("temperature", [0.0, T])
def test_batch_with_one_list_per_prompt(temperature, monkeypatch, graphs):
    """Every request stops on its own sequence; a request without one runs to the end."""
    prompts = [_prompt(s, n) for s, n in PROMPTS[:3]]
    free = [r.output_ids[0].tolist() for r in _many("batch", monkeypatch, prompts, temperature=temperature)]
    picks = [_pick(free[0], 41, 12), _pick(free[1], 37, 30, L=2), None]
    # (request 1 also carries request 0's sequence behind its own: it must stop on ITS table's first match)
    stops = [[picks[0][0]], [picks[1][0], picks[0][0]], None]
    out = _many("batch", monkeypatch, prompts, temperature=temperature, stop_sequences=stops)
    for i, (r, p) in enumerate(zip(out, picks)):
        ids = r.output_ids[0].tolist()
        if p is None:
            assert ids == free[i] and r.stop_sequence is None, i
        else:
            assert ids == free[i][:p[1] + 1] and r.stop_sequence == 0, i
    # one list for every prompt, cut off: only request 0's continuation holds the sequence
    out = _many("batch", monkeypatch, prompts, temperature=temperature, stop_sequences=[picks[0][0]],
                include_stop_sequence=False, logprobs=0)
    assert out[0].output_ids[0].tolist() == free[0][:picks[0][1] - 2] and out[0].stop_sequence == 0
    assert out[0].logprobs.shape == (picks[0][1] - 2 - 41,)
    for i in (1, 2):
        assert out[i].output_ids[0].tolist() == free[i] and out[i].stop_sequence is None


def test_policy_batch(monkeypatch, graphs):
    """dflash_generate_policy_batch, every request with a scheduler and a table of its own."""
    from dflash_amd.batch import dflash_generate_policy_batch
    monkeypatch.setenv("DFL_GRAPH", "1")
    cfg = H.tiny_cfg()
    prompts = [_prompt(s, n) for s, n in PROMPTS[:2]]
    hook = _hook()

    def run(**kw):
        return dflash_generate_policy_batch(model=_draft_model(cfg), target=_native(), input_ids=prompts,
                                            mask_token_id=cfg.mask_token_id, max_new_tokens=80, stop_token_ids=None,
                                            temperature=0.0, schedulers=[_script() for _ in prompts],
                                            draft_token_hook=lambda i, blk, start, call: hook(blk, start, call), **kw)

    free = [r.output_ids[0].tolist() for r in run()]
    picks = [_pick(free[0], 41, 25), _pick(free[1], 37, 9, L=4)]
    out = run(stop_sequences=[[p[0]] for p in picks], include_stop_sequence=False)
    for i, (r, (seq, e)) in enumerate(zip(out, picks)):
        assert r.output_ids[0].tolist() == free[i][:e + 1 - len(seq)] and r.stop_sequence == 0, i


def test_engine_refill_starts_from_a_clean_table(monkeypatch, graphs):
    """Four requests in two slots.  Requests 0 and 2 share a prompt, 1 and 3 another: request 0 stops early on sequence A,
    so request 2 is refilled into ITS slot and — with the same continuation — runs through A to its own, later sequence
    B; request 3 carries no sequence and emits what an engine built without the flag emits."""
    a, b = _prompt(3, 41), _prompt(4, 37)
    prompts = [a, b, a.clone(), b.clone()]
    free = _many("stream", monkeypatch, prompts)
    ids = [r.output_ids[0].tolist() for r in free]
    assert ids[0] == ids[2] and ids[1] == ids[3]
    A, eA = _pick(ids[0], 41, 6)
    B, eB = _pick(ids[0], 41, 45)
    C, eC = _pick(ids[1], 37, 40, L=2)
    out = _many("stream", monkeypatch, prompts, stop_sequences=[[A], [C], [[9, 9], B], None])
    got = [r.output_ids[0].tolist() for r in out]
    assert got[0] == ids[0][:eA + 1] and out[0].stop_sequence == 0
    assert got[1] == ids[1][:eC + 1] and out[1].stop_sequence == 0
    assert out[2].slot == out[0].slot and out[2].admitted_step > 0          # refilled into request 0's slot
    assert got[2] == ids[0][:eB + 1] and out[2].stop_sequence == 1          # not stopped by A, its predecessor's sequence
    assert np.array_equal(np.asarray(got[3]), np.asarray(ids[3])) and out[3].stop_sequence is None
    assert out[3].slot == out[1].slot
