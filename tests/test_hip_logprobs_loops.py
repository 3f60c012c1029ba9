"""`logprobs=` through the decode loops: single request (fixed and policy, eager and replayed),
wide blocks, MoE and fp8 targets, the ragged batch and the slot-refill engine — on the tiny walk target of
test_hip_sampling.py (helpers copied, not imported).

Truth needs no tolerance on the GEMM: the kernel's numbers are checked against the NumPy fp64 reference applied to the
very logits buffer the kernel read, within logprobs_ref.tolerance (2^-16 + 2^-22 |lse|)."""
import numpy as np
import pytest
import torch

import helpers as H
import logprobs_ref as LR

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
T = 0.7
_STATE = {}


def dev():
    return torch.device("cuda", 0)


def _walk_target(scale=0.62):
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
    if "nt" not in _STATE:
        _STATE["nt"] = NativeTarget(_walk_target()[0])
    return _STATE["nt"]


def _draft_model(cfg):
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return m


def _hook(perm, plan, V=2048):
    """Drafts scripted from the walk of the block's first token: plan[call] walk tokens, then a wrong one."""
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


def _prompt(seed=3, n=41):
    return torch.randint(0, 2000, (1, n), generator=torch.Generator().manual_seed(seed)).to(dev())


def _plan():
    return H.make_plan(400, 16, 29)


def _run(kind, monkeypatch, *, graph=True, stop=None, temperature=0.0, sampler="torch", seed=None, bs=16, n_new=90, **kw):
    from dflash_amd import dflash_generate, dflash_generate_policy
    monkeypatch.setenv("DFL_GRAPH", "1" if graph else "0")
    _, perm = _walk_target()
    cfg = H.tiny_cfg()
    hook = _hook(perm, _plan())
    if kind == "fixed":
        return dflash_generate(_draft_model(cfg), _native(), _prompt(), cfg.mask_token_id, n_new, bs, stop, temperature,
                               draft_token_hook=hook, sampler=sampler, seed=seed, **kw)
    return dflash_generate_policy(model=_draft_model(cfg), target=_native(), input_ids=_prompt(),
                                  mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, stop_token_ids=stop,
                                  temperature=temperature, scheduler=_script(), draft_token_hook=hook, sampler=sampler,
                                  seed=seed, **kw)


def _fields_shape(r, N):
    n = r.num_output_tokens
    assert r.logprobs.shape == (n,) and r.logprobs.dtype == torch.float32
    assert r.top_logprob_ids.shape == (n, N) and r.top_logprobs.shape == (n, N)
    assert torch.isfinite(r.logprobs).all() and (r.logprobs <= 0).all()
    if N:
        assert torch.isfinite(r.top_logprobs).all() and (r.top_logprob_ids >= 0).all()
        assert (r.top_logprobs[:, :-1] >= r.top_logprobs[:, 1:]).all()       # value descending
        assert (r.top_logprobs[:, 0] >= r.logprobs).all()                     # nothing beats the most likely token


def _same_fields(a, b):
    return (torch.equal(a.logprobs.view(torch.int32), b.logprobs.view(torch.int32))
            and torch.equal(a.top_logprob_ids, b.top_logprob_ids)
            and torch.equal(a.top_logprobs.view(torch.int32), b.top_logprobs.view(torch.int32)))


def _check_against(logits_rows, ids, got_lp, got_ids=None, got_tlp=None):
    """Rows of the logits buffer the kernel read (bf16, on the device) -> the reference; compared with what the sink holds."""
    x = logits_rows.float().cpu().numpy()
    ids = ids.cpu().tolist()
    got_lp = got_lp.cpu().numpy().astype(np.float64)
    for m in range(x.shape[0]):
        tol = LR.tolerance(LR.lse(x[m]))
        assert abs(got_lp[m] - LR.logprob(x[m], ids[m])) <= tol, (m, got_lp[m], LR.logprob(x[m], ids[m]), tol)
        if got_ids is not None:
            n = got_ids.shape[1]
            rid, rlp = LR.top(x[m], n + 1)
            vals = x[m][rid]
            gid = got_ids[m].cpu().numpy()
            # ids are exact where the reference's top n + 1 values are distinct; always: the same VALUES in the same order
            if len(set(vals.tolist())) == n + 1:
                assert np.array_equal(gid, rid[:n]), (m, gid, rid)
            assert np.array_equal(x[m][gid], vals[:n]), (m, gid, rid)
            assert (np.abs(got_tlp[m].cpu().numpy() - rlp[:n]) <= tol).all(), m


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("mode", ["greedy", "sampled", "filtered"])
def test_logprobs_leave_the_committed_ids_alone(mode, monkeypatch):
    kw = dict(greedy={}, sampled=dict(temperature=T, sampler="device", seed=5),
              filtered=dict(temperature=T, sampler="device", seed=5, top_k=20, top_p=0.9))[mode]
    off = _run("fixed", monkeypatch, **kw)
    assert off.logprobs is None and off.top_logprob_ids is None and off.top_logprobs is None
    for N in (0, 3):
        on = _run("fixed", monkeypatch, logprobs=N, **kw)
        assert torch.equal(on.output_ids, off.output_ids)
        assert list(on.acceptance_lengths) == list(off.acceptance_lengths) and on.replayed_cycles > 0
        _fields_shape(on, N)
    if mode == "greedy":   # the committed token is the most likely one: its logprob is the top entry
        assert torch.equal(on.top_logprob_ids[:, 0], on.output_ids[0, on.num_input_tokens:])
        assert torch.equal(on.top_logprobs[:, 0], on.logprobs)
    elif mode == "sampled":   # raw distribution: a sampled run commits tokens that are not the most likely ones
        assert (on.top_logprob_ids[:, 0] != on.output_ids[0, on.num_input_tokens:]).any()


@pytest.mark.parametrize("kind", ["fixed", "policy"])
@pytest.mark.parametrize("mode", ["greedy", "filtered"])
def test_eager_and_replayed_runs_are_bit_equal(kind, mode, monkeypatch):
    kw = {} if mode == "greedy" else dict(temperature=T, sampler="device", seed=9, top_k=20, top_p=0.9)
    eager = _run(kind, monkeypatch, graph=False, logprobs=4, **kw)
    rep = _run(kind, monkeypatch, graph=True, logprobs=4, **kw)
    assert eager.replayed_cycles == 0 and rep.replayed_cycles > 0 and max(rep.acceptance_lengths) > 2
    assert torch.equal(eager.output_ids, rep.output_ids)
    assert _same_fields(eager, rep)
    _fields_shape(rep, 4)


def _drive(bs, n_new, stop=None, N=3, temperature=0.0, plan=None, **kw):
    """A DecodeSession cycle by cycle: after each cycle the reference over the logits buffer the kernel read, rows < tau,
    against the session's buffer at start + 1 .. start + tau; position n_in after the prefill.  Returns the session and
    what was accumulated per position."""
    from dflash_amd.generate import DecodeSession
    _, perm = _walk_target()
    cfg = H.tiny_cfg()
    nt = _native()
    prompt = _prompt()
    s = DecodeSession(_draft_model(cfg), nt, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=n_new,
                      max_block_size=bs, stop_token_ids=stop, temperature=temperature,
                      draft_token_hook=_hook(perm, plan or _plan()), logprobs=N, **kw)
    s.prefill()
    n_in = s.n_in
    t0 = (n_in - 1) // 16 * 16
    _check_against(nt._pf["logits"][n_in - 1 - t0:n_in - t0], s.output_ids[0, n_in:n_in + 1], s.lp.lp[0, n_in:n_in + 1],
                   s.lp.top_ids[0, n_in:n_in + 1], s.lp.top_lp[0, n_in:n_in + 1])
    acc = {n_in: (s.lp.lp[0, n_in].item(), s.lp.top_ids[0, n_in].tolist())}
    taus = []
    while s.start < s.max_length:
        b = max(1, min(bs, s.max_length - s.start))
        r = s.cycle(b)
        torch.cuda.synchronize()
        lo, hi = r.start + 1, r.start + r.tau + 1
        _check_against(nt._nuc_logits[:r.tau], s.output_ids[0, lo:hi], s.lp.lp[0, lo:hi], s.lp.top_ids[0, lo:hi],
                       s.lp.top_lp[0, lo:hi])
        for p in range(lo, hi):
            acc[p] = (s.lp.lp[0, p].item(), s.lp.top_ids[0, p].tolist())
        taus.append(r.tau)
        if r.stop:
            break
    return s, acc, taus


@pytest.mark.parametrize("mode", ["greedy", "stop", "sampled"])
def test_session_values_are_the_reference_over_the_logits_the_kernel_read(mode):
    stop, kw = None, {}
    if mode == "stop":      # a token the greedy run emits well inside it
        s0, _, _ = _drive(16, 70)
        new = s0.finish()[0, s0.n_in:].tolist()
        stop = [next(t for i, t in enumerate(new) if i > 30 and new.index(t) == i)]
    if mode == "sampled":
        kw = dict(temperature=T, sampler="device", seed=3)
    s, acc, taus = _drive(16, 70, stop=stop, **kw)
    assert max(taus) > 2 and min(taus) == 1
    ids = s.finish()
    f = s.finish_logprobs()
    n_out = ids.shape[1] - s.n_in
    assert f["logprobs"].shape == (n_out,) and f["top_logprob_ids"].shape == (n_out, 3)
    if mode == "stop":
        assert n_out < 70 and ids[0, -1].item() == stop[0]
    else:
        assert n_out == 70
    assert f["logprobs"].tolist() == [acc[s.n_in + i][0] for i in range(n_out)]
    assert f["top_logprob_ids"].tolist() == [acc[s.n_in + i][1] for i in range(n_out)]


def test_wide_block_of_24_rows():
    """bs = 24 runs _verify_wide: two tiles of one request (tiles_per_req = 2), rows 16..23 from the second tile."""
    s, acc, taus = _drive(24, 100, plan=H.make_plan(64, 24, 29))
    assert max(taus) > 16, taus          # (a cycle whose committed rows reach into the second tile)
    f = s.finish_logprobs()
    assert f["logprobs"].tolist() == [acc[s.n_in + i][0] for i in range(100)]


def _verify_once(nt, bs=16, P=37, N=2, **kw):
    """One prefill + one verify of a random block on `nt`: the sink against the launch's own logits_out and posterior."""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(7)
    prompt = torch.randint(0, 2000, (1, P), generator=g).to(dev())
    block = torch.randint(0, 2000, (bs,), generator=g).to(dev())
    cache = nt.new_cache(P + 64)
    nt.prefill(prompt, cache)
    logits = torch.zeros(32, nt.V, dtype=BF16, device=dev())
    sink = ops.logprob_sink(1, P + 64, N, dev())
    post, _ = nt.verify(block, P, cache, logits_out=logits, logprobs=sink, **kw)
    torch.cuda.synchronize()
    assert torch.isnan(sink.lp[0, :P + 1]).all() and torch.isnan(sink.lp[0, P + bs + 1:]).all()
    _check_against(logits[:bs], post[0], sink.lp[0, P + 1:P + bs + 1], sink.top_ids[0, P + 1:P + bs + 1],
                   sink.top_lp[0, P + 1:P + bs + 1])
    ref, _ = nt.verify(block, P, cache, logits_out=torch.zeros_like(logits), **kw)
    assert torch.equal(ref, post)


def test_moe_target_one_cycle():
    tf = pytest.importorskip("transformers")
    from dflash_amd import NativeTarget
    cfg = tf.Qwen3MoeConfig(vocab_size=2048, hidden_size=512, intermediate_size=1024, moe_intermediate_size=256,
                            num_hidden_layers=3, num_attention_heads=4, num_key_value_heads=2, head_dim=128,
                            num_experts=16, num_experts_per_tok=4, decoder_sparse_step=1, norm_topk_prob=True,
                            max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=False,
                            rope_parameters={"rope_type": "default", "rope_theta": 1e6}, mlp_only_layers=[])
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(41)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        with torch.device(dev()):
            hf = tf.Qwen3MoeForCausalLM(cfg).eval()
    finally:
        torch.set_default_dtype(prev)
    nt = NativeTarget(hf)
    assert nt.is_moe
    _verify_once(nt)
    _verify_once(nt, bs=9, temperature=T, seed=4)


def test_fp8_target_one_cycle():
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import impose_greedy_walk, make_hf_qwen3
    torch.manual_seed(11)
    hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 3, "intermediate_size": 704}, dev(), dtype=BF16)
    impose_greedy_walk(hf, seed=8)
    nt = NativeTarget(hf, weight_format="fp8_e4m3")
    assert nt.streams_fp8(16)
    _verify_once(nt)
    _verify_once(nt, temperature=T, seed=4, top_k=20, top_p=0.9)
    _verify_once(nt, bs=24)


def _batch_run(captured, N=2, n_cycles=7):
    """Three requests of different prompt lengths, cycle by cycle: every live slot against its own rows of dec._logits.
    Returns per slot the values at its committed positions."""
    from dflash_amd.batch import BatchedDecoder
    _, perm = _walk_target()
    cfg = H.tiny_cfg()
    prompts = [_prompt(3, 41), _prompt(4, 23), _prompt(5, 50)]
    dec = BatchedDecoder(_draft_model(cfg), _native(), 3, max_rows=50 + 16 * n_cycles + 64, out_len=50 + 16 * n_cycles + 32,
                         mask_token_id=cfg.mask_token_id, logprobs=N)
    for r, p in enumerate(prompts):
        dec.admit(r, p)
    hooks = [_hook(perm, H.make_plan(64, 16, 31 + r)) for r in range(3)]
    hook = lambda r, blk, start, call: hooks[r](blk, start, call)   # noqa: E731
    torch.cuda.synchronize()
    for r, p in enumerate(prompts):       # the first token's value, written by the admission
        P = p.shape[1]
        assert torch.isfinite(dec.lp.lp[r, P]) and torch.isnan(dec.lp.lp[r, :P]).all() and torch.isnan(dec.lp.lp[r, P + 1:]).all()
        assert dec.lp.top_ids[r, P, 0].item() == dec.output_ids[r, P].item()        # greedy: the most likely token
    for c in range(n_cycles):
        starts = list(dec.start)
        if captured and c == 1:
            dec.capture()
        out = dec.cycle_graph(hook) if (captured and c >= 1) else dec.cycle(hook)
        torch.cuda.synchronize()
        for r, (tau, _) in enumerate(out):
            lo, hi = starts[r] + 1, starts[r] + tau + 1
            _check_against(dec._logits[r, :tau], dec.output_ids[r, lo:hi], dec.lp.lp[r, lo:hi], dec.lp.top_ids[r, lo:hi],
                           dec.lp.top_lp[r, lo:hi])
    assert max(dec.start[r] - prompts[r].shape[1] for r in range(3)) > 3 * n_cycles
    return [(dec.output_ids[r, :dec.start[r] + 1].clone(), dec.lp.lp[r, prompts[r].shape[1]:dec.start[r] + 1].clone(),
             dec.lp.top_ids[r, prompts[r].shape[1]:dec.start[r] + 1].clone()) for r in range(3)]


def test_batched_decoder_eager_and_captured():
    eager, cap = _batch_run(False), _batch_run(True)
    for (ia, la, ta), (ib, lb, tb) in zip(eager, cap):
        assert torch.equal(ia, ib) and torch.equal(la.view(torch.int32), lb.view(torch.int32)) and torch.equal(ta, tb)
        assert torch.isfinite(la).all()


def test_generate_batch_fields_match_the_single_request_run(monkeypatch):
    """dflash_generate_batch(logprobs=N): same ids as without, fields of the right length; a request's values agree with
    its own dflash_generate run (another GEMM, so within bf16 logit noise — loosely; the ids exactly)."""
    from dflash_amd.batch import dflash_generate_batch
    monkeypatch.setenv("DFL_GRAPH", "1")
    _, perm = _walk_target()
    cfg = H.tiny_cfg()
    prompts = [_prompt(3, 41), _prompt(4, 23)]
    hook = lambda r, blk, start, call: _hook(perm, _plan())(blk, start, call)   # noqa: E731
    off = dflash_generate_batch(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, 40, 16, None, draft_token_hook=hook)
    on = dflash_generate_batch(_draft_model(cfg), _native(), prompts, cfg.mask_token_id, 40, 16, None, draft_token_hook=hook,
                               logprobs=2)
    for a, b in zip(off, on):
        assert a.logprobs is None and torch.equal(a.output_ids, b.output_ids)
        _fields_shape(b, 2)
        assert torch.equal(b.top_logprob_ids[:, 0], b.output_ids[0, b.num_input_tokens:])


def test_engine_refill_shows_nothing_of_the_slots_previous_request(monkeypatch):
    """Two slots, five prompts.  Every result's fields have its own length; the buffers are filled with a sentinel after
    the engine's first cycle, so any entry a result shows that its own request did not write would be the sentinel —
    and each result equals the same request's run through a fresh engine of one slot."""
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", "1")
    _, perm = _walk_target()
    cfg = H.tiny_cfg()
    prompts = [_prompt(10 + i, 20 + 5 * i) for i in range(5)]
    mnt = [30, 70, 25, 40, 35]
    SENT = -12345.0

    def engine(slots):
        return BatchEngine(_draft_model(cfg), _native(), slots=slots, max_rows=45 + 70 + 48, out_len=45 + 70 + 16,
                           mask_token_id=cfg.mask_token_id, block_size=16, logprobs=2)

    eng = engine(2)
    for i, p in enumerate(prompts):
        eng.submit(p, mnt[i], draft_token_hook=_hook(perm, H.make_plan(64, 16, 50 + i)))
    first = eng.step()
    assert not first
    torch.cuda.synchronize()
    keep = [(s, r.n_in, r.start) for s, r in enumerate(eng.loop.slot_req)]
    saved = [(eng.dec.lp.lp[s, a:b + 1].clone(), eng.dec.lp.top_ids[s, a:b + 1].clone(), eng.dec.lp.top_lp[s, a:b + 1].clone())
             for s, a, b in keep]
    eng.dec.lp.lp.fill_(SENT)
    eng.dec.lp.top_ids.fill_(-777)
    eng.dec.lp.top_lp.fill_(SENT)
    for (s, a, b), (l, ti, tl) in zip(keep, saved):    # what the two live requests have committed so far stays
        eng.dec.lp.lp[s, a:b + 1], eng.dec.lp.top_ids[s, a:b + 1], eng.dec.lp.top_lp[s, a:b + 1] = l, ti, tl
    res = eng.run()
    assert len(res) == 5 and eng.stats["captures"] == 1 and eng.stats["admissions"] == 5
    slots_used = [r.slot for r in res]
    assert max(slots_used.count(s) for s in set(slots_used)) >= 2        # a slot served at least two requests
    for i, r in enumerate(res):
        assert r.num_output_tokens == mnt[i]
        _fields_shape(r, 2)                                             # (finite, <= 0: no sentinel, no NaN)
        assert (r.top_logprob_ids != -777).all() and (r.top_logprobs != SENT).all()
        assert torch.equal(r.top_logprob_ids[:, 0], r.output_ids[0, r.num_input_tokens:])
    # the same requests alone in a one-slot engine: the same ids and, the rows being computed alike, the same values
    solo = engine(1)
    for i in (1, 4):
        solo.submit(prompts[i], mnt[i], draft_token_hook=_hook(perm, H.make_plan(64, 16, 50 + i)))
    for i, r in zip((1, 4), solo.run()):
        assert torch.equal(r.output_ids, res[i].output_ids)
        assert torch.allclose(r.logprobs, res[i].logprobs, atol=0.05)
