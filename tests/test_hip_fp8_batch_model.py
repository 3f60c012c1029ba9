"""An fp8 (e4m3) draft in the ragged batch, the engine and wide blocks ("The batch forms"): the
streamed launches against the same model's dequantised copy, which launch receives which weight, and the loops'
losslessness.  Tiny widths: every K (512, 1024) gives the W8 and the bf16 K-part GEMM the same even share per wave, so
stream and copy are compared bit for bit."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def dev():
    return torch.device("cuda", 0)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _model(fmt="fp8_e4m3"):
    from dflash_amd import DFlashDraftModel
    cfg = H.tiny_cfg()
    m = DFlashDraftModel(cfg, device=dev(), weight_format=fmt)
    m.load_state_dict(H.draft_weights(cfg, seed=3, dtype=BF16))
    return cfg, m


@pytest.fixture(scope="module")
def walk():
    """The tiny native target with an imposed greedy walk, six prompts and their walks (shared, never modified)."""
    from dflash_amd import NativeTarget
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk, make_hf_qwen3
    torch.manual_seed(11)
    hf = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 6}, dev(), dtype=BF16)
    perm = impose_greedy_walk(hf, seed=5)
    lens = (33, 7, 50, 21, 40, 18)
    prompts = [torch.randint(0, 2000, (1, P), generator=_gen(40 + i)).to(dev()) for i, P in enumerate(lens)]
    Gs = [greedy_walk(perm, p, 140).to(dev()) for p in prompts]
    return NativeTarget(hf), prompts, Gs


def _hook_for(G, plan, vocab=2000):
    def hook(blk, start, call):
        k = min(plan[call], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            w = G[start + k + 1]
            blk[0, k + 1] = torch.where(blk[0, k + 1] == w, (w + 1) % vocab, blk[0, k + 1])
    return hook


# ---------------------------------------------------------------- stream against copy
@pytest.mark.parametrize("R", [2, 4])
def test_fp8_batch_draft_phase_equals_the_copy(walk, R):
    """fp8_stream True against False on one fp8 model: two cycles of a ragged batch of R requests; after each draft phase
    the drafted blocks, the draft caches and the hidden tiles are equal bit for bit."""
    from dflash_amd.batch import BatchedDecoder
    nt, prompts, _ = walk
    cfg, m = _model()
    snaps = []
    for stream in (True, False):
        m.fp8_stream = stream
        assert m.streams_fp8_tiles() == stream
        dec = BatchedDecoder(m, nt, R, max_rows=160, out_len=160, mask_token_id=cfg.mask_token_id)
        for r in range(R):
            dec.admit(r, prompts[r])
        s = []
        for _ in range(2):
            dec.draft()
            s.append((dec.block.clone(), dec.dk.clone(), dec.dv.clone(), dec.side_d.stack.h.clone(), dec.side_d.stack.xn.clone()))
            dec.verify()
            dec.accept()
        snaps.append(s)
    same = [all(torch.equal(a, b) for a, b in zip(x, y)) for x, y in zip(*snaps)]
    print(f"[fp8] ragged batch of {R}, stream vs copy: bit-identical per cycle = {same}")
    for c, (x, y) in enumerate(zip(*snaps)):
        for name, a, b in zip(("block", "K cache", "V cache", "hidden tiles", "final-normed tiles"), x, y):
            assert torch.equal(a, b), (c, name)
        assert (x[0][:R, 1:] != cfg.mask_token_id).all()


@pytest.mark.parametrize("bs", [20, 32])
def test_fp8_wide_block_equals_the_copy(bs):
    """A 20- and a 32-row block through forward() (the tile stack, R = 2) and draft_tokens(WideRows) with the e4m3
    lm_head against the dequantised one: hidden rows, cached K/V and ids equal bit for bit."""
    from dflash_amd import ops
    from dflash_amd.model import WideRows
    cfg, m = _model()
    lm = (torch.randn(cfg.vocab_size, cfg.hidden_size, generator=_gen(2)) * 0.05).to(BF16).to(dev())
    lm8 = m.packed_lm_head_fp8(lm)
    lm_copy = ops.pack_weight(ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(lm)))
    g = _gen(bs)
    th = (torch.randn(1, 9, cfg.fc_in, generator=g) * 1.5).to(BF16).to(dev())
    ne = (torch.randn(1, bs, cfg.hidden_size, generator=g) * 0.05).to(BF16).to(dev())
    outs = []
    for stream in (True, False):
        m.fp8_stream = stream
        cache = m.new_cache(9 + bs + 64)
        pos = torch.arange(0, 9 + bs, device=dev())[None]
        hid = m(target_hidden=th, noise_embedding=ne, position_ids=pos, past_key_values=cache, use_cache=True)
        ids = torch.full((32,), -1, dtype=torch.long, device=dev())
        m.draft_tokens(WideRows(m._wide.src["xn"], cache.dyn[:16].view(2, 8)), lm8 if stream else lm_copy, bs, ids)
        n = cache.get_seq_length()
        outs.append((hid, cache.k[:, :, :n].clone(), cache.v[:, :, :n].clone(), ids))
    same = [torch.equal(a, b) for a, b in zip(*outs)]
    print(f"[fp8] {bs}-row block, stream vs copy: bit-identical (hidden, K, V, ids) = {same}")
    assert all(same)
    assert int(outs[0][3][1:bs].min()) >= 0 and torch.all(outs[0][3][bs:] == -1)


# ---------------------------------------------------------------- routing
def _record_weights(monkeypatch, log):
    from dflash_amd import ops
    for name in ("gemm_f32_batch", "gemm_silu_mul_batch", "gemm_argmax_batch", "gemm_resid_batch", "gemm_sample_batch"):
        real = getattr(ops, name)

        def wrapped(wp, x, R, N, K, *a, _real=real, _name=name, **kw):
            log.append((log.phase, _name, N, K, isinstance(wp, ops.Fp8Weight)))
            return _real(wp, x, R, N, K, *a, **kw)
        monkeypatch.setattr(ops, name, wrapped)


class _Log(list):
    phase = None


def test_fp8_batch_routing(walk, monkeypatch):
    """Which launch of a cycle receives the codes: the draft side's context K/V, q/k/v parts, o_proj, gate/up, down_proj
    and greedy lm_head take an Fp8Weight; fc, every launch of the verify and a sampled draft head never do; with
    fp8_stream off nothing does."""
    from dflash_amd.batch import BatchedDecoder
    nt, prompts, _ = walk
    cfg, m = _model()
    log = _Log()
    _record_weights(monkeypatch, log)
    H_, I, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    nqkv, nkv_all = cfg.q_dim + 2 * cfg.kv_dim, L * 2 * cfg.kv_dim

    def cycle(dec):
        del log[:]
        for log.phase, fn in (("draft", dec.draft), ("verify", dec.verify)):
            fn()
        dec.accept()
        return [e[1:] for e in log if e[0] == "draft"], [e[1:] for e in log if e[0] == "verify"]

    dec = BatchedDecoder(m, nt, 2, max_rows=160, out_len=160, mask_token_id=cfg.mask_token_id)
    assert dec.qkv_parts
    for r in range(2):
        dec.admit(r, prompts[r])
    draft, verify = cycle(dec)
    layer = [("gemm_f32_batch", nqkv, H_, True), ("gemm_f32_batch", H_, cfg.q_dim, True),
             ("gemm_silu_mul_batch", I, H_, True), ("gemm_f32_batch", H_, I, True)]
    assert draft == ([("gemm_resid_batch", H_, cfg.fc_in, False), ("gemm_f32_batch", nkv_all, H_, True)] + layer * L
                     + [("gemm_argmax_batch", cfg.vocab_size, H_, True)])
    assert verify and not any(e[3] for e in verify)
    m.fp8_stream = False
    draft, verify = cycle(dec)
    assert len(draft) == 3 + 4 * L and not any(e[3] for e in draft + verify)
    m.fp8_stream = True
    # a sampled draft head keeps the bf16 lm_head; the layers still stream
    dec = BatchedDecoder(m, nt, 2, max_rows=160, out_len=160, mask_token_id=cfg.mask_token_id, temperature=0.7,
                         sampler="device", draft_temperature=0.7)
    for r in range(2):
        dec.admit(r, prompts[r], 0.7, seed=5 + r)
    draft, verify = cycle(dec)
    assert draft[-1] == ("gemm_sample_batch", cfg.vocab_size, H_, False) and draft[2:-1] == layer * L
    assert not any(e[3] for e in verify)
    # two tiles per request: q/k/v leaves finished rows (the bf16 copy), everything else streams, the lm_head too
    dec = BatchedDecoder(m, nt, 2, max_rows=200, out_len=200, mask_token_id=cfg.mask_token_id, tiles_per_request=2)
    for r in range(2):
        dec.admit(r, prompts[r])
    draft, verify = cycle(dec)
    assert draft[2:6] == [("gemm_resid_batch", nqkv, H_, False)] + layer[1:]
    assert draft[-1] == ("gemm_argmax_batch", cfg.vocab_size, H_, True) and not any(e[3] for e in verify)


def test_fp8_wide_block_routing(monkeypatch):
    from dflash_amd import ops
    cfg, m = _model()
    log = _Log()
    _record_weights(monkeypatch, log)
    g = _gen(1)
    th = (torch.randn(1, 9, cfg.fc_in, generator=g) * 1.5).to(BF16).to(dev())
    ne = (torch.randn(1, 20, cfg.hidden_size, generator=g) * 0.05).to(BF16).to(dev())
    for stream in (True, False):
        m.fp8_stream = stream
        del log[:]
        m(target_hidden=th, noise_embedding=ne, position_ids=torch.arange(0, 29, device=dev())[None],
          past_key_values=m.new_cache(128), use_cache=True)
        kinds = {(e[1], e[4]) for e in log}
        assert kinds == {("gemm_resid_batch", False), ("gemm_f32_batch", stream), ("gemm_silu_mul_batch", stream)}
    assert isinstance(m.tile_layers(qkv_parts=False)[0]["gu"], torch.Tensor)
    m.fp8_stream = True
    lw = m.tile_layers(qkv_parts=True)[0]
    assert all(isinstance(lw[k], ops.Fp8Weight) for k in ("qkv", "o", "gu", "down")) and lw["ln1"] is m.w["layers"][0]["ln1"]
    assert isinstance(m.tile_layers(qkv_parts=False)[0]["qkv"], torch.Tensor)
    assert m.streams_fp8_tiles() and m.streams_fp8(16) and not m.streams_fp8(17)


# ---------------------------------------------------------------- loops
def test_fp8_batch_loop_is_lossless(walk):
    """dflash_generate_batch with the fp8 draft, scripted acceptance: the committed ids are the target's greedy walk and
    the acceptance lengths the bf16 draft's."""
    from dflash_amd.batch import dflash_generate_batch
    nt, prompts, Gs = walk
    n_new, n = 60, 4
    lens = [p.shape[1] for p in prompts]
    hooks = [_hook_for(Gs[i], H.make_plan(64, 16, 17 + i)) for i in range(n)]
    bh = lambda i, blk, s, c: hooks[i](blk[:, :min(16, lens[i] + n_new - s)], s, c)  # noqa: E731
    runs = {}
    for fmt in ("bf16", "fp8_e4m3"):
        cfg, m = _model(fmt)
        runs[fmt] = dflash_generate_batch(m, nt, prompts[:n], cfg.mask_token_id, n_new, 16, None, 0.0, draft_token_hook=bh)
        for i, r in enumerate(runs[fmt]):
            assert r.output_ids[0].tolist() == Gs[i][:lens[i] + n_new].tolist(), (fmt, i)
    for a, b in zip(runs["bf16"], runs["fp8_e4m3"]):
        assert a.acceptance_lengths == b.acceptance_lengths
    # no hook: random draft weights, nearly every draft token rejected; still the walk
    cfg, m = _model()
    for i, r in enumerate(dflash_generate_batch(m, nt, prompts[:2], cfg.mask_token_id, 24, 16, None, 0.0)):
        assert r.output_ids[0].tolist() == Gs[i][:lens[i] + 24].tolist(), i


def test_fp8_engine_replays_and_refills(walk):
    """BatchEngine with the fp8 draft, six requests over four slots: lossless under refill, and graph replay on equals
    off id for id with replayed cycles (the captured graphs hold the fp8 launches)."""
    from dflash_amd.engine import BatchEngine
    nt, prompts, Gs = walk
    cfg, m = _model()
    n_new = [40, 25, 60, 30, 45, 20]
    outs = {}
    for graph in (False, True):
        eng = BatchEngine(m, nt, slots=4, max_rows=50 + 60 + 48, out_len=50 + 60 + 16, mask_token_id=cfg.mask_token_id,
                          graph=graph)
        for i, p in enumerate(prompts):
            eng.submit(p, n_new[i], draft_token_hook=_hook_for(Gs[i], H.make_plan(64, 16, 17 + i)))
        res = eng.run()
        assert (eng.stats["replayed_cycles"] > 0) == graph and eng.stats["admissions"] == 6
        outs[graph] = res
        for i, r in enumerate(res):
            assert r.output_ids[0].tolist() == Gs[i][:prompts[i].shape[1] + n_new[i]].tolist(), (graph, i)
    for a, b in zip(outs[False], outs[True]):
        assert a.acceptance_lengths == b.acceptance_lengths


def test_fp8_wide_blocks_are_lossless(walk):
    """Blocks of 20 rows through dflash_generate with the fp8 draft: the tile stack streams the codes, the committed ids
    are the walk, with the bf16 draft's acceptance lengths."""
    from dflash_amd import dflash_generate
    nt, prompts, Gs = walk
    n_new = 70
    taus = {}
    for fmt in ("bf16", "fp8_e4m3"):
        cfg, m = _model(fmt)
        r = dflash_generate(m, nt, prompts[0], cfg.mask_token_id, n_new, 20, None, 0.0,
                            draft_token_hook=_hook_for(Gs[0], H.make_plan(64, 20, 23)))
        assert r.output_ids[0].tolist() == Gs[0][:33 + n_new].tolist(), fmt
        taus[fmt] = r.acceptance_lengths
    assert taus["bf16"] == taus["fp8_e4m3"]
