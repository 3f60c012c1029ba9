"""MXFP4 in the ragged-batch GEMMs without a GPU ("The batch forms"): every refusal of the C ABI —
nothing is launched, the pointers are small integers — the K rule of the K-part launch, and the model's routing."""
import ctypes as C

import pytest
import torch

import helpers as H
from dflash_amd import ops

W4_BASE, SCALE = 4096, 4096 + 64 * 256 // 2   # "pointers": codes, and a 64-byte aligned scale region


def _abi():
    from dflash_amd import _lib
    h = _lib.lib()
    xb = _lib.RowsBatch()
    xb.r0.frag, xb.r0.mode, xb.r0.valid_word, xb.frag_stride = 16, 0, -1, 4096 * 16
    return _lib, h, xb


def _calls(_lib, xb, scale=SCALE, R=2, K=256, x=None):
    """the three entry points on a 64 x K weight, each with everything valid but what the arguments change"""
    w = _lib.Weight(W4_BASE, scale, _lib.W_MXFP4)
    x = C.byref(xb) if x is None else x
    return {"dfl_gemm_silu_mul_batch": (w, x, R, 64, K, 16, 1024, 16, 16, None),
            "dfl_gemm_f32_batch": (w, x, R, 64, K, 16, 16, None),
            "dfl_gemm_argmax_batch": (w, x, R, 64, K, 0, 16, 16, 2, 16, 16, 16, 0, None, 0, None)}


RING = ("dfl_gemm_silu_mul_batch", "dfl_gemm_argmax_batch")
# what changes, which entry points refuse it, a word of the message
REFUSALS = [("null scale", dict(scale=None), None, b"format 3"),
            ("misaligned scale", dict(scale=SCALE + 32), None, b"64-byte aligned"),
            ("K % 128", dict(K=320), None, b"128"),
            ("R = 5", dict(R=5), None, b"R"),
            ("K < 256", dict(K=128), RING, b"256"),
            ("nfr % 4", dict(K=512), ("dfl_gemm_f32_batch",), b"multiple of 4"),
            ("nfr % 4 above one part", dict(K=2560), ("dfl_gemm_f32_batch",), b"multiple of 4")]


@pytest.mark.parametrize("what,change,names,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_abi_refusals(what, change, names, word):
    _lib, h, xb = _abi()
    for name, args in _calls(_lib, xb, **change).items():
        if names is None or name in names:
            assert getattr(h, name)(*args) == -22, (what, name)
            err = h.dfl_last_error()
            assert (name + ":").encode() in err and word in err, (what, name, err)


def test_abi_refuses_plain_rows_in_the_ring_forms_and_the_sampled_head():
    _lib, h, xb = _abi()
    xb.r0.frag, xb.r0.rows, xb.r0.ld, xb.r0.mode, xb.rows_stride = None, 16, 256, 1, 16 * 256
    for name, args in _calls(_lib, xb).items():
        if name in RING:
            assert getattr(h, name)(*args) == -22 and b"frag16" in h.dfl_last_error(), name
    _lib, h, xb = _abi()
    w = _lib.Weight(W4_BASE, SCALE, _lib.W_MXFP4)
    assert h.dfl_gemm_sample_batch(w, C.byref(xb), 2, 64, 256, 0, 16, 16, 2, 16, 16, 16, 0, None, 0, 16, None, 1.0, 1, 0, 0, 1,
                                   None) == -22
    assert b"dfl_gemm_sample_batch:" in h.dfl_last_error() and b"format 3" in h.dfl_last_error()


@pytest.mark.parametrize("K,ok", [(512, False), (1024, True), (2560, False), (3072, False), (4096, True), (5120, False),
                                  (12288, True)])
def test_mxfp4_parts_ok_is_the_nfr_rule(K, ok):
    ks = K // 32
    parts = -(-ks // 64)
    assert ops.mxfp4_parts_ok(K) is ok and ok == (-(-ks // (8 * parts)) % 4 == 0)


def test_streams_mxfp4_tiles_path_table():
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(H.tiny_cfg(), device="cpu", weight_format="mxfp4")
    assert not m.streams_mxfp4_tiles()                      # nothing loaded
    m.w4 = {"layers": []}
    assert m.streams_mxfp4_tiles() and not m.streams_fp8_tiles()
    m.fuse_oproj = True                                     # (the single-request path's condition only)
    assert m.streams_mxfp4_tiles() and not m.streams_mxfp4(16)
    for attr, off in (("mxfp4_stream", False), ("attn_impl", "fused"), ("wide_hidden", True)):
        keep = getattr(m, attr)
        setattr(m, attr, off)
        assert not m.streams_mxfp4_tiles(), attr
        setattr(m, attr, keep)
    assert not DFlashDraftModel(H.tiny_cfg(), device="cpu").streams_mxfp4_tiles()


def test_tile_layers_routes_per_matrix():
    """gu always; o / down / qkv the 4-bit twin where the K-part launch takes the matrix's K, else the bf16 copy; an e4m3
    twin as before."""
    e = torch.empty(0, dtype=torch.uint8)
    layers = [{"qkv": 1, "o": 2, "gu": 3, "down": 4, "ln1": 5}]
    t4 = {"qkv": ops.Mxfp4Weight(e, 768, 512), "o": ops.Mxfp4Weight(e, 512, 512), "gu": ops.Mxfp4Weight(e, 2048, 512),
          "down": ops.Mxfp4Weight(e, 512, 1024)}
    assert ops.tile_layers(layers, [t4], False, {}) == [{"qkv": 1, "o": 2, "gu": t4["gu"], "down": t4["down"], "ln1": 5}]
    t4k = {**t4, "qkv": ops.Mxfp4Weight(e, 768, 2048), "o": ops.Mxfp4Weight(e, 512, 4096)}
    assert ops.tile_layers(layers, [t4k], True, {}) == [{"qkv": t4k["qkv"], "o": t4k["o"], "gu": t4["gu"], "down": t4["down"],
                                                         "ln1": 5}]
    assert ops.tile_layers(layers, [t4k], False, {})[0]["qkv"] == 1
    t8 = {"qkv": "q8", "o": "o8", "gu": "g8", "down": "d8"}
    assert ops.tile_layers(layers, [t8], True, {}) == [{"qkv": "q8", "o": "o8", "gu": "g8", "down": "d8", "ln1": 5}]
