"""An fp8 (e4m3) native target, the parts that need no GPU ("The target"): the quantiser's fixed
point that lets one quantised model live in two representations, NativeTarget.check_config under both weight formats,
and the two sampled fp8 entry points' declarations and argument validation."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

import helpers as H

BF16, F8 = torch.bfloat16, torch.float8_e4m3fn


def _edge_rows():
    """Rows whose largest code lands on 224 after rounding — the edge where a second quantisation halves the scale —
    beside ordinary rows, an all-zero row and rows of one magnitude only."""
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(24, 128, generator=g, dtype=torch.float64) * torch.logspace(-3, 3, 24, dtype=torch.float64)[:, None])
    w = w.to(BF16)
    w[2] = 0
    for r, (amax, s) in enumerate(((225.0, 1.0), (226.0, 2.0 ** -9), (231.0, 2.0 ** 5), (224.0, 1.0), (448.0, 4.0),
                                   (449.0, 1.0)), start=8):
        # amax / scale in (224, 232]: e4m3 has a step of 16 there, so the largest magnitude rounds DOWN onto 224
        row = (torch.rand(128, generator=g, dtype=torch.float64) * 200 - 100)
        row[5] = -amax
        w[r] = (row * s).to(BF16)
    return w


def test_requantising_the_dequantised_rows_keeps_every_value():
    """quantize(dequantize(quantize(w))) dequantises to the same bf16 values: the fp8 target overwrites the wrapped
    model's weights with q * scale, and whoever quantises those again — packed_lm_head_fp8 of the overwritten head, a
    second NativeTarget over the same model — holds the same model.  Where the largest code is 224 the second scale is
    half the first and the codes are doubled: other codes, the same values."""
    from dflash_amd import ops
    w = _edge_rows()
    q1, s1 = ops.quantize_fp8_rows(w)
    d1 = ops.dequantize_fp8_rows(q1, s1)
    q2, s2 = ops.quantize_fp8_rows(d1)
    d2 = ops.dequantize_fp8_rows(q2, s2)
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))
    top = q1.view(F8).float().abs().amax(dim=1)
    edge = top == 224.0
    assert int(edge.sum()) >= 3, top.tolist()
    assert torch.equal(s2[edge], s1[edge] / 2) and torch.all(q2.view(F8).float().abs().amax(dim=1)[edge] == 448.0)
    keep = ~edge & (top > 0)
    assert torch.equal(s2[keep], s1[keep]) and torch.equal(q2[keep], q1[keep])
    q3, s3 = ops.quantize_fp8_rows(d2)       # and from there on the codes are a fixed point too
    assert torch.equal(q3, q2) and torch.equal(s3, s2)


def _cfg(**over):
    base = dict(hidden_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128, intermediate_size=2048,
                num_hidden_layers=2, vocab_size=4208, attention_bias=False, mlp_bias=False)
    return SimpleNamespace(**{**base, **over})


def test_check_config_under_both_formats():
    """fp8 refuses, before any device work: an unknown format (ValueError), a sparse-MoE target and widths that are no
    multiple of 64 (NotImplementedError); bf16 accepts the same configs."""
    from dflash_amd import NativeTarget
    NativeTarget.check_config(_cfg())
    NativeTarget.check_config(_cfg(), "bf16")
    NativeTarget.check_config(_cfg(), "fp8_e4m3")
    for fmt in ("int4", "fp8", "FP8_E4M3", None):
        with pytest.raises(ValueError, match="weight_format"):
            NativeTarget.check_config(_cfg(), fmt)
    moe = _cfg(num_experts=128, num_experts_per_tok=8, moe_intermediate_size=768)
    NativeTarget.check_config(moe)
    with pytest.raises(NotImplementedError, match="MoE"):
        NativeTarget.check_config(moe, "fp8_e4m3")
    for bad in (dict(hidden_size=1056), dict(intermediate_size=2080), dict(hidden_size=1024 + 32, intermediate_size=2048)):
        NativeTarget.check_config(_cfg(**bad))
        with pytest.raises(NotImplementedError, match="% 64"):
            NativeTarget.check_config(_cfg(**bad), "fp8_e4m3")
    # what bf16 refuses, fp8 refuses too (the format check comes on top)
    for fmt in ("bf16", "fp8_e4m3"):
        with pytest.raises(NotImplementedError, match="head_dim"):
            NativeTarget.check_config(_cfg(head_dim=64), fmt)


def test_constructor_refuses_before_any_device_work():
    """The constructor runs check_config first: with a config-only stand-in for the model (no weights, no device) the
    refusals above come out of NativeTarget(...) itself."""
    from dflash_amd import NativeTarget
    fake = SimpleNamespace(config=_cfg(num_experts=64, num_experts_per_tok=4, moe_intermediate_size=512))
    with pytest.raises(NotImplementedError, match="MoE"):
        NativeTarget(fake, weight_format="fp8_e4m3")
    with pytest.raises(ValueError, match="weight_format"):
        NativeTarget(SimpleNamespace(config=_cfg()), weight_format="e5m2")
    with pytest.raises(NotImplementedError, match="% 64"):
        NativeTarget(SimpleNamespace(config=_cfg(intermediate_size=2080)), weight_format="fp8_e4m3")


# ---------------------------------------------------------------------------------------------- the C ABI
SAMPLED = ("dfl_gemm_sample", "dfl_gemm_sample_batch")
PACKERS = {"dfl_pack_weight_fp8", "dfl_pack_weight_gateup_fp8"}   # another element type, nothing chosen at launch


def test_sampled_entry_points_take_a_descriptor_and_no_fp8_launch_is_declared():
    from dflash_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dfl_[a-z0-9_]+)\s*\(", txt))
    handle = _lib.lib()
    for n in SAMPLED:
        assert n in names and n in _lib.SIGNATURES and isinstance(getattr(handle, n), C._CFuncPtr), n
        assert _lib.SIGNATURES[n][1][0] is C.POINTER(_lib.Weight), n     # the e4m3 lm_head arrives in the descriptor
        assert re.search(r"\b" + n + r"\s*\(\s*const\s+dfl_weight\s*\*", txt), n
    assert {n for n in names | set(_lib.SIGNATURES) if n.endswith("_fp8")} == PACKERS
    assert not any(hasattr(handle, n + "_fp8") for n in SAMPLED)
    assert handle.dfl_version() == 1
    assert re.search(r"#define\s+DFL_ABI_VERSION\s+1\b", txt)


def test_sampled_fp8_entry_points_validate_without_gpu():
    """Small integers stand for pointers; every call is refused with -22 and its own name before anything launches."""
    from dflash_amd import _lib
    h = _lib.lib()
    x = _lib.Rows()
    x.frag, x.mode, x.valid_word = 64, 0, -1
    xb = _lib.RowsBatch()
    xb.r0, xb.frag_stride = x, 16 * 512

    def refused(name, *args, text=None):
        assert getattr(h, name)(*args) == -22, (name, args)
        err = h.dfl_last_error()
        assert (name + ":").encode() in err, (name, err)
        if text:
            assert text in err, (name, err)

    f = C.c_float

    def w8(wp, sc):
        return _lib.Weight(wp, sc, _lib.W_E4M3)
    # ---- dfl_gemm_sample({wp8, wscale, e4m3}, x, V, K, row0, nrows, dyn, word, ws, ids, off, logits, margins, seed, inv_t,
    #                      stream, pos_dyn, pos_word, pos_base, pos_add, hip stream)
    def one(wp=64, sc=64, V=64, K=512, row0=0, nrows=16, ws=64, ids=64, inv_t=1.4, stream=0, pos_dyn=None, pos_word=3):
        return (w8(wp, sc), C.byref(x), V, K, row0, nrows, None, -1, ws, ids, 0, None, None, 5, f(inv_t), stream, pos_dyn,
                pos_word, 0, 1, None)
    refused("dfl_gemm_sample", *one(wp=None), text=b"null")
    refused("dfl_gemm_sample", *one(sc=None), text=b"null")
    refused("dfl_gemm_sample", *one(ids=None), text=b"null")
    refused("dfl_gemm_sample", *one(K=544), text=b"K%64")
    refused("dfl_gemm_sample", *one(V=72), text=b"%16")
    refused("dfl_gemm_sample", *one(inv_t=0.0), text=b"inv_t")
    refused("dfl_gemm_sample", *one(stream=2), text=b"stream")
    refused("dfl_gemm_sample", *one(pos_dyn=64, pos_word=8), text=b"pos_word")
    assert h.dfl_gemm_sample(*one(row0=4, nrows=13)) == -22
    assert h.dfl_gemm_sample(*one(K=8192)) == -22          # beyond 4096: the head needs finished sums

    # ---- dfl_gemm_sample_batch({wp8, wscale, e4m3}, x, R, V, K, row0, nrows, dyn, word, ws, ids, stride, off, logits,
    #                            lstride, seeds, inv_ts, inv_t, stream, pos_word, pos_add, tiles_per_req, hip stream)
    def ring(wp=64, sc=64, src=xb, R=2, V=64, K=512, dyn=64, seeds=64, inv_ts=None, inv_t=1.4, stream=0, pos_word=3, tpr=1):
        return (w8(wp, sc), C.byref(src) if src is not None else None, R, V, K, 0, 16, dyn, 2, 64, 64, 16, 0, None, 0, seeds,
                inv_ts, f(inv_t), stream, pos_word, 1, tpr, None)
    refused("dfl_gemm_sample_batch", *ring(wp=None), text=b"null")
    refused("dfl_gemm_sample_batch", *ring(sc=None), text=b"null")
    refused("dfl_gemm_sample_batch", *ring(src=None), text=b"null")
    refused("dfl_gemm_sample_batch", *ring(seeds=None), text=b"null")
    refused("dfl_gemm_sample_batch", *ring(dyn=None), text=b"null")
    refused("dfl_gemm_sample_batch", *ring(sc=68), text=b"64-byte aligned")
    refused("dfl_gemm_sample_batch", *ring(K=288), text=b"K%64")
    refused("dfl_gemm_sample_batch", *ring(K=192), text=b"K >= 256")
    refused("dfl_gemm_sample_batch", *ring(R=0), text=b"R")
    refused("dfl_gemm_sample_batch", *ring(R=5), text=b"R")
    refused("dfl_gemm_sample_batch", *ring(V=72), text=b"%16")
    refused("dfl_gemm_sample_batch", *ring(inv_t=0.0), text=b"inv_t")
    refused("dfl_gemm_sample_batch", *ring(stream=3), text=b"stream")
    refused("dfl_gemm_sample_batch", *ring(tpr=3), text=b"tiles_per_req")
    refused("dfl_gemm_sample_batch", *ring(R=3, tpr=2), text=b"tiles_per_req")
    rows = _lib.Rows()                      # plain rows (mode 1): the ring takes frag16 only, and there is no slab form
    rows.rows, rows.ld, rows.mode, rows.valid_word = 64, 512, 1, -1
    pb = _lib.RowsBatch()
    pb.r0, pb.rows_stride = rows, 16 * 512
    refused("dfl_gemm_sample_batch", *ring(src=pb), text=b"ring form")
    xb.frag_stride = 16 * 512 + 4           # a fragment stride that is no multiple of 8
    refused("dfl_gemm_sample_batch", *ring(), text=b"ring form")
