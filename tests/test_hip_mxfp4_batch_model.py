"""An mxfp4 draft on the tile-stack paths ("The batch forms"): which launch takes which weight, wide
blocks and the ragged batch with mxfp4_stream on against off, and the batch / engine loops under scripted acceptance."""
import pytest
import torch

import helpers as H
from test_hip_mxfp4 import _walk_case, dev, gen, make_model, run_cycles

pytestmark = pytest.mark.gpu


def _batch_hook(hook):
    return lambda r, blk, start, call: hook(blk, start, call)


def test_which_launch_takes_which_weight(monkeypatch):
    """Tiny widths: gate/up (ring) and down_proj (K = 1024) the 4-bit twins, o_proj and q/k/v (K = 512: 2 k-steps per wave)
    and the context K/V the bf16 copy; the batch's greedy draft head the 4-bit lm_head, the verify's the bf16 one."""
    from dflash_amd import NativeTarget, ops
    from dflash_amd.batch import dflash_generate_batch
    cfg = H.tiny_cfg()
    m = make_model(cfg, "mxfp4")
    assert (cfg.hidden_size, cfg.intermediate_size) == (512, 1024) and m.streams_mxfp4_tiles()
    for parts in (False, True):
        for lw, l4, lb in zip(m.tile_layers(qkv_parts=parts), m.w4["layers"], m.w["layers"]):
            assert lw["gu"] is l4["gu"] and lw["down"] is l4["down"] and lw["o"] is lb["o"] and lw["qkv"] is lb["qkv"]
    assert m.kv_all_tiles() is None
    m.mxfp4_stream = False
    assert m.tile_layers(qkv_parts=True) is m.w["layers"]
    m.mxfp4_stream = True
    heads, real = [], ops.gemm_argmax_batch
    monkeypatch.setattr(ops, "gemm_argmax_batch", lambda wp, *a, **k: (heads.append(type(wp)), real(wp, *a, **k))[1])
    hf, prompt, G, _ = _walk_case(24)
    dflash_generate_batch(m, NativeTarget(hf), [prompt, prompt], cfg.mask_token_id, 24, 16, None, 0.0)
    assert ops.Mxfp4Weight in heads and torch.Tensor in heads


@pytest.mark.parametrize("bs", [20, 32])
def test_wide_blocks_stream_on_equals_off(bs):
    cfg = H.tiny_cfg()
    m = make_model(cfg, "mxfp4")
    outs = []
    for on in (True, False):
        m.mxfp4_stream = on
        o, c, _ = run_cycles(m, cfg, [9, 4, 16], 12, bs=bs)
        n = c.get_seq_length()
        outs.append((o, c.k[:, :, :n].clone(), c.v[:, :, :n].clone()))
    for x, y in zip(outs[0][0], outs[1][0]):
        assert torch.equal(x, y)
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2])


def test_three_request_batch_stream_on_equals_off():
    """No hook: every acceptance length is decided by the draft's own tokens, i.e. by the draft phase's bits."""
    from dflash_amd import NativeTarget
    from dflash_amd.batch import dflash_generate_batch
    cfg = H.tiny_cfg()
    hf, prompt, G, _ = _walk_case(40)
    prompts = [prompt] + [torch.randint(0, 2000, (1, n), generator=gen(6 + n)).to(dev()) for n in (21, 40)]
    res = []
    for on in (True, False):
        m = make_model(cfg, "mxfp4")
        m.mxfp4_stream = on
        rs = dflash_generate_batch(m, NativeTarget(hf), prompts, cfg.mask_token_id, 40, 16, None, 0.0)
        res.append(([r.output_ids[0].tolist() for r in rs], [r.acceptance_lengths for r in rs]))
    assert res[0] == res[1] and res[0][0][0] == G[:33 + 40].tolist()


@pytest.mark.parametrize("graph", ["0", "1"])
def test_batch_and_engine_are_lossless_under_scripted_acceptance(monkeypatch, graph):
    """Committed ids are the target's greedy walk, with the bf16 draft's acceptance lengths: dflash_generate_batch over
    three requests, and BatchEngine with three requests through two slots (a refill), eager and with replayed cycles."""
    from dflash_amd import NativeTarget
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.engine import BatchEngine
    monkeypatch.setenv("DFL_GRAPH", graph)
    cfg = H.tiny_cfg()
    n_new = [48, 30, 40]
    hf, prompt, G, hook = _walk_case(max(n_new))
    runs = {}
    for fmt in ("bf16", "mxfp4"):
        rs = dflash_generate_batch(make_model(cfg, fmt), NativeTarget(hf), [prompt] * 3, cfg.mask_token_id, n_new[0], 16, None,
                                   0.0, draft_token_hook=_batch_hook(hook))
        eng = BatchEngine(make_model(cfg, fmt), NativeTarget(hf), slots=2, max_rows=33 + 48 + 48, out_len=33 + 48 + 16,
                          mask_token_id=cfg.mask_token_id, block_size=16, temperature=0.0)
        for n in n_new:
            eng.submit(prompt, n, draft_token_hook=hook)
        re = eng.run()
        if fmt == "mxfp4" and graph == "1":
            assert eng.stats["replayed_cycles"] > 0
        for r in rs:
            assert r.output_ids[0].tolist() == G[:33 + n_new[0]].tolist(), fmt
        for r, n in zip(re, n_new):
            assert r.output_ids[0].tolist() == G[:33 + n].tolist(), (fmt, n)
        runs[fmt] = [r.acceptance_lengths for r in list(rs) + list(re)]
    assert runs["mxfp4"] == runs["bf16"]
