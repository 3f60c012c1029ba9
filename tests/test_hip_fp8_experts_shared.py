"""FP8 (e4m3) expert weights in the shared MoE pass over 2..4 tiles ("The experts"): from two tiles
on NativeTarget.moe_mlp_tiles takes _moe_mlp_shared — blocks of 17..32 rows, the ragged batch, the engine, the candidate
verifier — and with expert codes and expert_stream set its two grouped launches (ops.moe_grouped_gate_up,
ops.moe_grouped_down) stream the codes instead of the dequantised bf16 copy.

Every bar here is bit-equality.  expert_stream = True replaces exactly the weight operand of two launches per MoE layer
by codes and scales; the W8 form of the grouped kernel is bit-equal to the bf16 form on q * scale for power-of-two scales
(tests/test_hip_fp8_experts_shared_kernels.py derives it; the scales of quantize_fp8_rows are powers of two).  Every other
launch is the same kernel on the same bytes, so ids, logits, taps and K/V rows are equal, and with them every committed
id of every loop.

The models are those of tests/test_hip_fp8_experts.py (hidden 512, 16 experts of 256, top-4, 4 layers, once with a dense
layer in between: the 64-row item form) and one of two layers at hidden 2560 with 8 experts of 128, top-6 (hidden > 2048:
the per-tile gate/up has no code form there, the grouped one has; few experts: the 128-row item form)."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_S = {}
NAMES = ("ids", "logits", "taps", "K rows", "V rows")
GROUPED = ("moe_grouped_gate_up", "moe_grouped_down")


def dev():
    return torch.device("cuda", 0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _moe_hf(layers=4, E=16, top_k=4, Ie=256, mlp_only=(), seed=41, hidden=512, heads=4, kv=2):
    """tests/test_hip_fp8_experts.py::_moe_hf."""
    tf = pytest.importorskip("transformers")
    cfg = tf.Qwen3MoeConfig(vocab_size=2048, hidden_size=hidden, intermediate_size=2 * hidden, moe_intermediate_size=Ie,
                            num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv, head_dim=128,
                            num_experts=E, num_experts_per_tok=top_k, decoder_sparse_step=1, norm_topk_prob=True,
                            max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=False,
                            rope_parameters={"rope_type": "default", "rope_theta": 1e6}, mlp_only_layers=list(mlp_only))
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        with torch.device(dev()):
            m = tf.Qwen3MoeForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    with torch.no_grad():   # the default init leaves the router nearly flat: give the routing something to decide
        for layer in m.model.layers:
            if hasattr(layer.mlp, "gate"):
                layer.mlp.gate.weight.mul_(8.0)
    return m.eval()


KINDS = {"tiny": dict(), "dense1": dict(mlp_only=(1,)),
         "h2560": dict(layers=2, E=8, top_k=6, Ie=128, hidden=2560, seed=44)}


def _case(name):
    """name -> dict(hf, perm, nt8, mlp_only); the greedy walk is imposed BEFORE the fp8-expert target is constructed
    (which overwrites hf's expert tensors with q * scale).  Shared; tests restore every switch they flip."""
    if name not in _S:
        from dflash_amd import NativeTarget
        from dflash_amd.synthetic import impose_greedy_walk
        kw = KINDS[name]
        hf = _moe_hf(**kw)
        perm = impose_greedy_walk(hf, seed=5)
        nt8 = NativeTarget(hf, expert_format="fp8_e4m3")
        assert nt8.moe_shared_pass and nt8.moe_shared_min == 2 and nt8.expert_stream
        _S[name] = dict(hf=hf, perm=perm, nt8=nt8, mlp_only=tuple(kw.get("mlp_only", ())))
    return _S[name]


def _draft():
    from dflash_amd import DFlashDraftModel
    cfg = H.tiny_cfg(num_target_layers=4, target_layer_ids=[0, 2])
    m = DFlashDraftModel(cfg, device=dev())
    m.load_state_dict(H.draft_weights(cfg, dtype=BF16))
    return cfg, m


def _hook_for(G, plan, vocab=2000):
    """plan[call] tokens of the walk G, then a wrong one."""
    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % vocab, blk[0, k + 1])
    return hook


def _verify(t, prompt, block, taps):
    """Prefill + one verify on a fresh cache: (ids, logits, tap rows, K rows, V rows of the block), cloned."""
    P, bs = prompt.shape[1], block.numel()
    cache = t.new_cache(P + 64)
    t.prefill(prompt, cache, tap_layers=taps)
    logits = torch.zeros(32, t.V, dtype=BF16, device=dev())
    post, th = t.verify(block, P, cache, tap_layers=taps, logits_out=logits)
    return (post[0].clone(), logits[:bs].clone(), th[:bs].clone(), cache.k[:, :, P:P + bs].clone(),
            cache.v[:, :, P:P + bs].clone())


def _spy(monkeypatch, log):
    """The two grouped launches and the two per-tile ones -> log of (name, received codes?, the weight)."""
    from dflash_amd import ops
    for name in GROUPED + ("moe_gate_up", "moe_down"):
        real = getattr(ops, name)

        def wrapped(w, *a, _real=real, _name=name, **kw):
            log.append((_name, isinstance(w, ops.Fp8Experts), w))
            return _real(w, *a, **kw)
        monkeypatch.setattr(ops, name, wrapped)


def _expect(t, mlp_only, stream, passes=1):
    """The log of `passes` shared passes over every MoE layer: both grouped launches, with the layer's own codes (stream)
    or its own bf16 copy."""
    want = []
    for _ in range(passes):
        for i, lw in enumerate(t.layers):
            if i not in mlp_only:
                want += [(GROUPED[0], stream, lw["gu_e8"] if stream else lw["gu_e"]),
                         (GROUPED[1], stream, lw["down_e8"] if stream else lw["down_e"])]
    return want


def _same_log(log, want):
    return len(log) == len(want) and all(a[0] == b[0] and a[1] == b[1] and a[2] is b[2] for a, b in zip(log, want))


# ------------------------------------------------------------------------------------------------ one verify
@pytest.mark.parametrize("name", ["tiny", "dense1", "h2560"])
def test_wide_verify_streams_the_codes_and_equals_the_copy(name, monkeypatch):
    """A 20-row and a 32-row verify (two tiles: the shared pass) with expert_stream on against off: posterior ids,
    logits_out, taps and the cache's K/V rows are torch.equal.  The spy: under expert_stream the shared pass handed BOTH
    grouped launches of every MoE layer that layer's Fp8Experts — gate/up too at hidden 2560, where the per-tile branch
    still reads the copy — and the bf16 tensors otherwise; no per-tile expert launch ran; the dense layer has none."""
    c = _case(name)
    t = c["nt8"]
    assert (t.H > 2048) == (name == "h2560")
    log = []
    _spy(monkeypatch, log)
    prompt = torch.randint(0, 2000, (1, 29), generator=_gen(5)).to(dev())
    taps = [0] if name == "h2560" else [0, 2]
    try:
        for bs in (20, 32):
            block = torch.randint(0, 2000, (bs,), generator=_gen(100 + bs)).to(dev())
            runs = {}
            for stream in (True, False):
                t.expert_stream = stream
                del log[:]
                runs[stream] = _verify(t, prompt, block, taps)
                assert _same_log(log, _expect(t, c["mlp_only"], stream)), (bs, stream, [(a, b) for a, b, _ in log])
            same = [torch.equal(x, y) for x, y in zip(runs[True], runs[False])]
            print(f"[fp8] shared pass {name}, {bs} rows: bit-identical {dict(zip(NAMES, same))}")
            assert all(same), (bs, dict(zip(NAMES, same)))
    finally:
        t.expert_stream = True
    sc = t._moe_sh["sc"]
    assert sc["rows_per_item"] == (128 if name == "h2560" else 64)


def test_the_per_tile_branch_still_runs_and_equals_the_shared_pass(monkeypatch):
    """moe_shared_pass = False on a 20-row verify: the per-tile branch runs (its two launches per tile and MoE layer, on
    the codes), no grouped launch does, and the posterior ids equal the shared pass's.  At hidden 2560 the per-tile
    gate/up is dfl_gemm_silu_mul_experts on the copy (no spy entry) and the down projection takes the codes."""
    for name in ("dense1", "h2560"):
        c = _case(name)
        t = c["nt8"]
        n_moe = t.L - len(c["mlp_only"])
        log = []
        _spy(monkeypatch, log)
        prompt = torch.randint(0, 2000, (1, 29), generator=_gen(5)).to(dev())
        block = torch.randint(0, 2000, (20,), generator=_gen(6)).to(dev())
        taps = [0] if name == "h2560" else [0, 2]
        shared = _verify(t, prompt, block, taps)
        assert {e[0] for e in log} == set(GROUPED)
        t.moe_shared_pass = False
        try:
            del log[:]
            tiles = _verify(t, prompt, block, taps)
            per_tile = [("moe_down", True)] if name == "h2560" else [("moe_gate_up", True), ("moe_down", True)]
            assert [e[:2] for e in log] == per_tile * (2 * n_moe), [e[:2] for e in log]
        finally:
            t.moe_shared_pass = True
        assert torch.equal(shared[0], tiles[0])


# ------------------------------------------------------------------------------------------------ the ragged batch
@pytest.fixture(scope="module")
def walk():
    from dflash_amd.synthetic import greedy_walk
    c = _case("tiny")
    lens = (30, 47, 12, 25, 38, 19)
    prompts = [torch.randint(0, 2000, (1, P), generator=_gen(60 + i)).to(dev()) for i, P in enumerate(lens)]
    Gs = [greedy_walk(c["perm"], p, 240).to(dev()) for p in prompts]
    return c["nt8"], prompts, Gs


@pytest.mark.parametrize("R", [3, 4])
def test_batch_cycles_stream_on_equals_off_eager_and_replayed(walk, R, monkeypatch):
    """BatchedDecoder — what dflash_generate_batch drives — with 3 and with 4 requests, eight cycles launched kernel by kernel
    and eight replayed from the captured graphs, expert_stream on against off: the same acceptance lengths, committed
    ids, posterior ids, tapped rows and target K/V rows, and the committed ids are the walk.  The captured verify holds the
    code launches (the spy sees them during the capture)."""
    from dflash_amd.batch import BatchedDecoder
    nt8, prompts, Gs = walk
    cfg, m = _draft()
    hooks = [_hook_for(Gs[i], H.make_plan(64, 16, 17 + i)) for i in range(R)]
    hook = lambda r, b, s, c: hooks[r](b, s, c)  # noqa: E731
    log = []
    _spy(monkeypatch, log)
    runs = {}
    try:
        for stream in (True, False):
            nt8.expert_stream = stream
            for use_graph in (False, True):
                dec = BatchedDecoder(m, nt8, R, max_rows=320, out_len=320, mask_token_id=cfg.mask_token_id)
                for r in range(R):
                    dec.admit(r, prompts[r])
                del log[:]
                taus = [dec.cycle(hook)]
                assert _same_log(log, _expect(nt8, (), stream)), (stream, [(a, b) for a, b, _ in log])
                if use_graph:
                    del log[:]
                    dec.capture()
                    assert _same_log(log, _expect(nt8, (), stream)), (stream, "capture")
                    del log[:]
                for _ in range(8):
                    taus.append((dec.cycle_graph if use_graph else dec.cycle)(hook))
                if use_graph:
                    assert log == []                       # replays launch nothing from the host
                torch.cuda.synchronize()
                runs[stream, use_graph] = (taus, list(dec.start), dec.output_ids.clone(), dec.post.clone(),
                                           dec.d["taps"].clone(), dec.tk.clone(), dec.tv.clone())
                for r in range(R):
                    n = dec.start[r]
                    assert torch.equal(dec.output_ids[r, :n + 1], Gs[r][:n + 1]), (stream, use_graph, r)
                del dec
    finally:
        nt8.expert_stream = True
    ref = runs[False, False]
    assert max(t[0] for cyc in ref[0] for t in cyc if t is not None) > 8
    for key, run in runs.items():
        assert run[0] == ref[0] and run[1] == ref[1] and torch.equal(run[2], ref[2]), key
    # rows bit for bit between the two arms of one launch form (a replayed attention launch splits its keys at the
    # cache capacity, an eager one at the request's length: their rows agree to rounding only)
    for use_graph in (False, True):
        for x, y, what in zip(runs[True, use_graph][2:], runs[False, use_graph][2:],
                              ("output ids", "posterior ids", "taps", "K rows", "V rows")):
            assert torch.equal(x, y), (use_graph, what)


def test_generate_batch_stream_on_equals_off(walk):
    """dflash_generate_batch with 3 and with 4 requests: every request commits its walk with the same acceptance lengths
    in both arms."""
    from dflash_amd.batch import dflash_generate_batch
    nt8, prompts, Gs = walk
    cfg, m = _draft()
    n_new = 40
    lens = [p.shape[1] for p in prompts]
    hooks = [_hook_for(Gs[i], H.make_plan(64, 16, 41 + i)) for i in range(4)]
    bh = lambda i, blk, s, c: hooks[i](blk[:, :min(16, lens[i] + n_new - s)], s, c)  # noqa: E731
    acc = {}
    try:
        for stream in (True, False):
            nt8.expert_stream = stream
            for R in (3, 4):
                rs = dflash_generate_batch(m, nt8, prompts[:R], cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=bh)
                for i, r in enumerate(rs):
                    assert r.output_ids[0].tolist() == Gs[i][:lens[i] + n_new].tolist(), (stream, R, i)
                acc[stream, R] = [r.acceptance_lengths for r in rs]
    finally:
        nt8.expert_stream = True
    assert acc[True, 3] == acc[False, 3] and acc[True, 4] == acc[False, 4]


def test_engine_with_four_slots_and_an_admission_in_mid_run(walk, monkeypatch):
    """BatchEngine with four slots and six requests of unequal lengths (two are admitted into slots that finished while
    the others run), eager and by graph replay: every request returns its walk, with the same acceptance lengths under
    expert_stream on and off.  The engine's expert launches are the grouped ones, on this arm's weights."""
    from dflash_amd.engine import BatchEngine
    nt8, prompts, Gs = walk
    cfg, m = _draft()
    n_new = [60, 25, 70, 30, 45, 50]
    lens = [p.shape[1] for p in prompts]
    hooks = [_hook_for(Gs[i], H.make_plan(64, 16, 17 + i)) for i in range(6)]
    log = []
    _spy(monkeypatch, log)
    outs = {}
    try:
        for stream in (True, False):
            nt8.expert_stream = stream
            for graph in (False, True):
                eng = BatchEngine(m, nt8, slots=4, max_rows=50 + 70 + 48, out_len=50 + 70 + 16,
                                  mask_token_id=cfg.mask_token_id, graph=graph)
                for i, p in enumerate(prompts):
                    eng.submit(p, n_new[i], draft_token_hook=hooks[i])
                del log[:]
                res = eng.run()
                assert (eng.stats["replayed_cycles"] > 0) == graph and eng.stats["admissions"] == 6
                assert set(GROUPED) <= {e[0] for e in log} and all(e[1] == stream for e in log), (stream, graph)
                for i, r in enumerate(res):
                    assert r.output_ids[0].tolist() == Gs[i][:lens[i] + n_new[i]].tolist(), (stream, graph, i)
                outs[stream, graph] = [r.acceptance_lengths for r in res]
                del eng
    finally:
        nt8.expert_stream = True
    assert outs[True, False] == outs[False, False] == outs[True, True] == outs[False, True]


# ------------------------------------------------------------------------------------------------ candidates
@pytest.mark.parametrize("name", ["tiny", "h2560"])
def test_candidate_verifier_streams_the_codes_and_equals_the_copy(name, monkeypatch):
    """NativeCandidateVerifier at C = 3 (three tiles through moe_mlp_tiles: the shared pass): posterior ids, every
    candidate's tapped rows and staged K/V rows with expert_stream on equal those with it off; the grouped launches
    received the codes, respectively the copy."""
    from dflash_amd.candidates import NativeCandidateVerifier
    c = _case(name)
    t = c["nt8"]
    taps = [0] if name == "h2560" else [0, 2]
    prompt = torch.randint(0, 2000, (1, 33), generator=_gen(8)).to(dev())
    b16 = torch.randint(0, 2000, (16,), generator=_gen(9)).to(dev())
    cands = torch.stack([b16, b16.roll(1), b16.flip(0)])
    cands[:, 0] = b16[0]
    P = prompt.shape[1]
    cache = t.new_cache(P + 64)
    t.prefill(prompt, cache, tap_layers=taps)
    ver = NativeCandidateVerifier(t, len(taps))
    log = []
    _spy(monkeypatch, log)
    runs = {}
    try:
        for stream in (True, False):
            t.expert_stream = stream
            del log[:]
            cache.length = P
            post = ver.verify(cands, P, cache, taps)
            assert _same_log(log, _expect(t, c["mlp_only"], stream)), (stream, [(a, b) for a, b, _ in log])
            runs[stream] = (post.clone(), torch.stack([ver.cand_taps(i, 16) for i in range(3)]).clone(),
                            ver.stage_k[:, :3, :, :16].clone(), ver.stage_v[:, :3, :, :16].clone())
    finally:
        t.expert_stream = True
    for x, y, what in zip(runs[True], runs[False], ("posterior ids", "taps", "K rows", "V rows")):
        assert torch.equal(x, y), what
    assert not torch.equal(runs[True][0][0], runs[True][0][2])          # (three different candidates went through)
