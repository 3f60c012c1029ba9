"""The verify's logits chain as ONE stage (dflash_amd/logits_stage.py): which launches a prefill, an
admission and a cycle enqueue, and in which order, for every feature alone, for all six together and for none — in a
DecodeSession and in a BatchedDecoder — read off a recorder in front of the library's C entries; and all six together,
eager against replayed.  On the tiny walk target of test_hip_min_p_loops.py (helpers copied, not imported).

What the emitted ids ARE is audited by the per-feature *_loops.py files against their CPU references; this file pins the
order, which they cannot see: two processors swapped, or one enqueued twice, still emits plausible ids."""
import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
V = 2048
T = 0.7
SEED = 5
_STATE = {}

# the entries the chain is made of, single-request and ragged-batch names of the head and the accept launch
HEAD, HEAD_B, DRAWN, DRAWN_B = "dfl_gemm_argmax", "dfl_gemm_argmax_batch", "dfl_gemm_sample", "dfl_gemm_sample_batch"
ACCEPT, ACCEPT_B = "dfl_accept_commit", "dfl_accept_commit_batch"
BIAS, GRAMMAR, PENALTY, MIN_P, DRAW, LOGPROB = ("dfl_logit_bias_rows", "dfl_grammar_rows", "dfl_penalty_rows",
                                                "dfl_min_p_rows", "dfl_sample_rows_nucleus", "dfl_logprob_rows")
COUNT, ADVANCE = "dfl_penalty_count", "dfl_grammar_advance"
EIGHT = (BIAS, GRAMMAR, PENALTY, MIN_P, DRAW, LOGPROB, COUNT, ADVANCE)
CHAIN = EIGHT + (HEAD, HEAD_B, DRAWN, DRAWN_B, ACCEPT, ACCEPT_B)
FEATURES = ("penalties", "logit_bias", "grammar", "min_p", "filter", "logprobs")


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
        if toks:
            blk[0, 1:1 + len(toks)] = torch.tensor(toks, dtype=blk.dtype, device=blk.device)
    return hook


def _hook():
    return _walk_hook(_walk_target()[1], H.make_plan(400, 16, 29))


def _prompt(seed=3, n=41):
    return torch.randint(0, 2000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev())


def _fallback():
    """Three tokens off the walks of the test prompts (the set test_hip_min_p_loops.py biases)."""
    if "fb" not in _STATE:
        _, perm = _walk_target()

        def cycle(t):
            out = [t]
            for _ in range(5):
                out.append(perm[out[-1]])
            return set(out)

        prot = set()
        for s, n in ((3, 41), (4, 37), (5, 45)):
            prot |= cycle(int(_prompt(s, n)[0, -1]))
        fb = []
        for t in range(100, 1900):
            if not cycle(t) & prot:
                fb.append(t)
                prot |= cycle(t)
            if len(fb) == 3:
                break
        _STATE["fb"] = fb
    return _STATE["fb"]


def _any_token():
    """A one-state automaton that allows every id."""
    from dflash_amd import TokenDFA
    return TokenDFA(np.zeros((1, V), dtype=np.int16), 0)


# ------------------------------------------------------------------------------------------------------------ the recorder
class Recorder:
    """In place of dflash_amd._lib._lib (what every importer reaches through _lib.lib()): every C entry called is appended
    to .calls as (name, arguments) and forwarded."""

    def __init__(self, real):
        self._real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*a):
            self.calls.append((name, a))
            return fn(*a)
        return call

    def take(self):
        out, self.calls = self.calls, []
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


def names_after_head(calls, head):
    """The chain's entries from the last `head` launch on."""
    names = [n for n, _ in calls if n in CHAIN]
    last = max(i for i, n in enumerate(names) if n == head)
    return names[last:]


# ------------------------------------------------------------------------------------------------------------ the settings
def feature_kwargs(on, slot=0):
    """The request's keywords for the features in `on`: COMBO_* of test_with_top_p_penalties_and_a_logit_bias in slot 0,
    other values in the other slots."""
    fb, mask = _fallback(), H.tiny_cfg().mask_token_id
    kw = {}
    if "penalties" in on:
        kw.update(repetition_penalty=(1.1, 1.3)[slot], presence_penalty=(0.05, 0.0)[slot], frequency_penalty=(0.0, 0.1)[slot])
    if "logit_bias" in on:
        kw.update(logit_bias={fb[0]: 0.40, fb[1]: 0.55, fb[2]: 0.70} if slot == 0 else {fb[1]: -0.5},
                  banned_token_ids=[mask])
    if "min_p" in on:
        kw.update(min_p=(0.65, 0.3)[slot])
    if "filter" in on:
        kw.update(**(dict(top_p=0.9) if slot == 0 else dict(top_k=5)))
    return kw


def expected(on, temperature, batch=False):
    """(first-token chain, cycle chain from the verify's head launch on) of the features in `on`: the sub-lists of the
    all-on order."""
    sampling = temperature >= 1e-5
    rows = [e for f, e in (("logit_bias", BIAS), ("grammar", GRAMMAR), ("penalties", PENALTY)) if f in on]
    mp = [MIN_P] if sampling and "min_p" in on else []
    flt = sampling and "filter" in on
    lp = [LOGPROB] if "logprobs" in on else []
    count = [COUNT] if "penalties" in on else []
    adv = [ADVANCE] if "grammar" in on else []
    first = []
    for e in rows:   # the table row is cleared and the prompt counted in front of the penalised rows
        first += count + [e] if e == PENALTY else [e]
    first += mp + ([DRAW] if mp or flt else []) + count + adv + lp   # (the plain first draw is dfl_sample_rows: not listed)
    processed = bool(rows or mp or flt)
    head = (HEAD_B if batch else HEAD) if processed or not sampling else (DRAWN_B if batch else DRAWN)
    cycle = [head] + rows + mp + ([DRAW] if sampling and processed else []) + lp + [ACCEPT_B if batch else ACCEPT] + count + adv
    return first, cycle


def run_session(rec, on, temperature, bs=8):
    """prefill() and one eager cycle(bs) of a DecodeSession with the features in `on`; the two recordings."""
    from dflash_amd.generate import DecodeSession
    cfg = H.tiny_cfg()
    kw = dict(sampler="device", seed=SEED) if temperature >= 1e-5 else {}
    kw.update(feature_kwargs(on))
    if "grammar" in on:
        kw.update(grammar=_any_token())
    if "logprobs" in on:
        kw.update(logprobs=2)
    s = DecodeSession(_draft_model(cfg), _native(), _prompt(), mask_token_id=cfg.mask_token_id, max_new_tokens=40,
                      max_block_size=16, stop_token_ids=None, temperature=temperature, **kw)
    rec.take()
    s.prefill()
    first = rec.take()
    s.cycle(bs)
    torch.cuda.synchronize()
    return first, rec.take(), s


def run_decoder(rec, on, temperature, request_temperature=False):
    """Two admissions and one eager cycle() of a BatchedDecoder of 2 requests with the features in `on`, the slots' values
    differing; the recordings."""
    from dflash_amd.batch import BatchedDecoder
    cfg = H.tiny_cfg()
    sampling = temperature >= 1e-5
    dec = BatchedDecoder(_draft_model(cfg), _native(), 2, 256, 200, cfg.mask_token_id, temperature=temperature,
                         sampler="device" if sampling else "torch", request_temperature=request_temperature,
                         filtering="filter" in on, logprobs=2 if "logprobs" in on else None, penalties="penalties" in on,
                         logit_bias="logit_bias" in on, grammar_states=1 if "grammar" in on else 0, min_p="min_p" in on)
    handle = dec.add_grammar(_any_token()) if "grammar" in on else None
    admits = []
    for r, (p, t) in enumerate(((_prompt(3, 41), temperature), (_prompt(4, 37), 0.5 if request_temperature else temperature))):
        rec.take()
        dec.admit(r, p, t, seed=SEED + r if sampling else None, grammar=handle, **feature_kwargs(on, r))
        admits.append(rec.take())
    dec.cycle()
    torch.cuda.synchronize()
    return admits, rec.take(), dec


# ------------------------------------------------------------------------------------------------------------ the tests
def test_order_single_request_everything_on(rec):
    first, cycle, _ = run_session(rec, FEATURES, T)
    assert names_after_head(cycle, HEAD) == [HEAD, BIAS, GRAMMAR, PENALTY, MIN_P, DRAW, LOGPROB, ACCEPT, COUNT, ADVANCE]
    assert names_after_head(first, HEAD)[1:] == [BIAS, GRAMMAR, COUNT, PENALTY, MIN_P, DRAW, COUNT, ADVANCE, LOGPROB]
    assert (names_after_head(first, HEAD)[1:], names_after_head(cycle, HEAD)) == expected(FEATURES, T)


def test_order_ragged_batch_everything_on(rec):
    admits, cycle, dec = run_decoder(rec, FEATURES, T, request_temperature=True)
    assert names_after_head(cycle, HEAD_B) == [HEAD_B, BIAS, GRAMMAR, PENALTY, MIN_P, DRAW, LOGPROB, ACCEPT_B, COUNT, ADVANCE]
    for a in admits:
        assert names_after_head(a, HEAD)[1:] == [BIAS, GRAMMAR, COUNT, PENALTY, MIN_P, DRAW, COUNT, ADVANCE, LOGPROB]
    assert all(dec.live)


@pytest.mark.parametrize("temperature", [T, 0.0])
@pytest.mark.parametrize("feature", FEATURES)
def test_each_feature_alone(rec, feature, temperature):
    """The feature's sub-list of the all-on order, in the session and in the decoder.  At T = 0 min_p and the filter
    enqueue nothing, and logprobs alone keeps the plain dfl_gemm_argmax, its logits materialised."""
    want_first, want_cycle = expected((feature,), temperature)
    first, cycle, _ = run_session(rec, (feature,), temperature)
    assert names_after_head(first, HEAD)[1:] == want_first
    assert names_after_head(cycle, HEAD if want_cycle[0] == HEAD else DRAWN) == want_cycle
    if feature == "logprobs" and temperature < 1e-5:
        head_args = [a for n, a in cycle if n == HEAD][-1]
        assert want_cycle[0] == HEAD and head_args[11] is not None      # (the 12th argument: where the logits go)
    want_first, want_cycle = expected((feature,), temperature, batch=True)
    admits, cycle, _ = run_decoder(rec, (feature,), temperature)
    assert [names_after_head(a, HEAD)[1:] for a in admits] == [want_first] * 2
    assert names_after_head(cycle, want_cycle[0]) == want_cycle


@pytest.mark.parametrize("temperature", [T, 0.0])
def test_no_feature_enqueues_none_of_it(rec, temperature):
    first, cycle, s = run_session(rec, (), temperature)
    assert not [n for n, _ in first + cycle if n in EIGHT] and getattr(s, "stage", None) is None
    admits, cycle, dec = run_decoder(rec, (), temperature)
    assert not [n for n, _ in admits[0] + admits[1] + cycle if n in EIGHT] and getattr(dec, "stage", None) is None and dec._logits is None


# all six on, 60 new tokens, eager against replayed
def _all_on():
    kw = feature_kwargs(FEATURES)
    return dict(sampler="device", logprobs=2, grammar=_any_token(), **kw)


def _same_result(a, b):
    assert a.output_ids[0].tolist() == b.output_ids[0].tolist() and a.grammar_state == b.grammar_state == 0
    for f in ("logprobs", "top_logprobs"):
        assert torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32)), f
    assert torch.equal(a.top_logprob_ids, b.top_logprob_ids) and torch.isfinite(a.logprobs).all()


def test_all_six_eager_is_replayed(monkeypatch):
    from dflash_amd import dflash_generate
    cfg = H.tiny_cfg()
    out = []
    for graph in ("0", "1"):
        monkeypatch.setenv("DFL_GRAPH", graph)
        out.append(dflash_generate(_draft_model(cfg), _native(), _prompt(), cfg.mask_token_id, 60, 16, None, T,
                                   draft_token_hook=_hook(), seed=SEED, **_all_on()))
    _same_result(*out)
    assert out[0].replayed_cycles == 0 and out[1].replayed_cycles > 0
    assert out[0].num_output_tokens == 60


def test_all_six_eager_is_replayed_in_the_stream(monkeypatch):
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.engine import dflash_generate_stream
    cfg = H.tiny_cfg()
    replays = []
    real = BatchedDecoder.cycle_graph
    monkeypatch.setattr(BatchedDecoder, "cycle_graph", lambda self, *a: (replays.append(1), real(self, *a))[1])
    hook = _hook()
    out = []
    for graph in ("0", "1"):
        monkeypatch.setenv("DFL_GRAPH", graph)
        n0 = len(replays)
        out.append(dflash_generate_stream(_draft_model(cfg), _native(), [_prompt(3, 41), _prompt(4, 37)], cfg.mask_token_id,
                                          60, 16, None, T, draft_token_hook=lambda i, blk, start, call: hook(blk, start, call),
                                          seed=SEED, **_all_on()))
        assert (len(replays) > n0) == (graph == "1")
    for a, b in zip(*out):
        _same_result(a, b)
