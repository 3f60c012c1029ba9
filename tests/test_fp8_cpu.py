"""FP8 (e4m3) draft weights, the parts that need no GPU: the row quantiser's contract and the new entry points'
argument validation.  The launches take the codes as a Weight(wp, scale, W_E4M3) descriptor."""
import ctypes as C
import os
import re

import pytest
import torch

import helpers as H

BF16 = torch.bfloat16
FP8_PACKERS = ["dfl_pack_weight_fp8", "dfl_pack_weight_gateup_fp8"]


def _rows():
    g = torch.Generator().manual_seed(31)
    w = (torch.randn(40, 256, generator=g, dtype=torch.float64) * torch.logspace(-6, 6, 40, dtype=torch.float64)[:, None])
    w = w.to(BF16)
    w[3] = 0                                                       # an all-zero row
    w[5] = (torch.randn(256, generator=g, dtype=torch.float64) * 0.01).to(BF16)
    w[5, 77] = 3.0e38                                              # one huge outlier: everything else underflows
    tiny = torch.arange(256, dtype=torch.int16).view(BF16).clone()  # bf16 subnormals (and +0): bit patterns 0 .. 255
    tiny[1::2] = -tiny[1::2]
    w[6] = tiny
    return w


def test_quantize_fp8_rows_contract():
    from dflash_amd import ops
    w = _rows()
    q, scale = ops.quantize_fp8_rows(w)
    assert q.dtype == torch.uint8 and q.shape == w.shape and scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    assert not ((q & 0x7F) == 0x7F).any(), "a NaN code"
    qv = q.view(torch.float8_e4m3fn).to(torch.float64)
    assert float(qv.abs().max()) <= 448.0
    mant, _ = torch.frexp(scale)
    assert torch.all(mant == 0.5) and torch.all(scale > 0), "every scale is a power of two"
    assert float(scale[3]) == 1.0 and torch.count_nonzero(q[3] & 0x7F) == 0
    # the rule itself: the smallest power of two that brings the row's largest magnitude within 448
    amax = w.double().abs().amax(dim=1)
    nz = amax > 0
    assert torch.all(amax[nz] / scale.double()[nz] <= 448.0) and torch.all(amax[nz] / scale.double()[nz] > 224.0)
    x = w.double() / scale.double()[:, None]
    normal = x.abs() >= 2.0 ** -6
    rel = ((qv - x).abs() / x.abs().clamp_min(1e-300))[normal]
    assert float(rel.max()) <= 2.0 ** -4
    assert float((qv - x).abs()[~normal].max()) <= 2.0 ** -10       # i.e. |q * scale - w| <= scale * 2^-10
    deq = qv * scale.double()[:, None]
    assert torch.equal(deq.float().to(BF16).double(), deq), "q * scale is exactly representable in bf16"
    assert torch.equal(ops.dequantize_fp8_rows(q, scale).double(), deq)
    # the outlier row keeps its outlier and the sign pattern of what survives
    assert float(deq[5, 77]) == pytest.approx(3.0e38, rel=2.0 ** -4)
    assert torch.all((deq[6] == 0) | (torch.sign(deq[6]) == torch.sign(w[6].double())))


def test_quantize_fp8_rows_is_idempotent_in_value():
    """One quantised model: the dequantised weights are a fixed point — quantising them again reproduces the same
    VALUES exactly (a row whose largest magnitude rounded down into the next binade gets half the scale and twice the
    codes), so a bf16 model loaded with q * scale computes what the fp8 model's fallback copy computes."""
    from dflash_amd import ops
    q, scale = ops.quantize_fp8_rows(_rows())
    d1 = ops.dequantize_fp8_rows(q, scale)
    d2 = ops.dequantize_fp8_rows(*ops.quantize_fp8_rows(d1))
    assert torch.equal(d1, d2)


def _declared():
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(dfl_[a-z0-9_]+)\s*\(", txt))


def test_fp8_entry_points_are_declared_bound_and_exported():
    from dflash_amd import _lib
    names = _declared()
    handle = _lib.lib()
    for n in FP8_PACKERS + ["dfl_gemm_resid", "dfl_gemm_silu_mul", "dfl_gemm_argmax"]:
        assert n in names, f"{n} missing from include/dflash_hip.h"
        assert n in _lib.SIGNATURES, f"{n} missing from SIGNATURES"
        assert isinstance(getattr(handle, n), C._CFuncPtr)
    # one launch name per operation: the weight's format travels in the descriptor that takes the packed weight's place
    for n in ("dfl_gemm_resid", "dfl_gemm_silu_mul", "dfl_gemm_argmax"):
        assert _lib.SIGNATURES[n][1][0] is C.POINTER(_lib.Weight), n
        assert n + "_fp8" not in names and n + "_fp8" not in _lib.SIGNATURES, n
    for n in ("dfl_pack_weight", "dfl_pack_weight_gateup"):   # the packers stay: another element type, nothing chosen at launch
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[n + "_fp8"]


def test_fp8_entry_points_validate_without_gpu():
    """Null pointers, K % 64 != 0 and N % 16 != 0 are refused with -22 and the entry point's own name; small integers
    stand for pointers, nothing launches."""
    from dflash_amd import _lib
    h = _lib.lib()
    x = _lib.Rows()
    x.frag, x.mode, x.valid_word = 16, 0, -1
    xr = C.byref(x)

    def w8(wp, scale):
        return _lib.Weight(wp, scale, _lib.W_E4M3)

    def refused(name, *args, text=None):
        assert getattr(h, name)(*args) == -22, (name, args)
        err = h.dfl_last_error()
        assert (name + ":").encode() in err, (name, err)
        if text:
            assert text in err, (name, err)

    for N, K, text in ((16, 64, b"null"), (16, 96, b"K%64"), (24, 64, b"%16"), (16, 32, b"K%64")):
        p = None if text == b"null" else 16
        refused("dfl_pack_weight_fp8", p, 16, N, K, None, text=text)
        refused("dfl_pack_weight_gateup_fp8", 16, p, 16, N, K, None, text=text)
        refused("dfl_gemm_resid", w8(16, p), xr, N, K, 16, N, 0, None, 0, None, None, None, text=text)
        refused("dfl_gemm_silu_mul", w8(16, p), xr, N, K, 16, None, None, text=text)
        refused("dfl_gemm_argmax", w8(16, p), xr, N, K, 0, 16, None, -1, 16, 16, 0, None, None, None, None, None, text=text)
    # a missing weight / output pointer, and a missing row source
    refused("dfl_gemm_resid", w8(None, 16), xr, 16, 64, 16, 16, 0, None, 0, None, None, None, text=b"null")
    refused("dfl_gemm_resid", w8(16, 16), xr, 16, 64, None, 16, 0, None, 0, None, None, None, text=b"null")
    refused("dfl_gemm_resid", w8(16, 16), None, 16, 64, 16, 16, 0, None, 0, None, None, None, text=b"null")
    refused("dfl_gemm_silu_mul", w8(16, 16), xr, 16, 64, None, None, None, text=b"null")
    refused("dfl_gemm_argmax", w8(16, 16), xr, 16, 64, 0, 16, None, -1, None, 16, 0, None, None, None, None, None, text=b"null")
    # a normalised source beyond K = 4096 (the chunked form takes none), as the bf16 sibling
    assert h.dfl_gemm_silu_mul(w8(16, 16), xr, 16, 8192, 16, None, None) == -22


def test_weight_format_is_validated():
    from dflash_amd import DFlashDraftModel
    with pytest.raises(ValueError, match="weight_format"):
        DFlashDraftModel(H.tiny_cfg(), device="cpu", weight_format="int4")
    assert DFlashDraftModel(H.tiny_cfg(), device="cpu").weight_format == "bf16"
    m = DFlashDraftModel(H.tiny_cfg(), device="cpu", weight_format="fp8_e4m3")
    assert m.weight_format == "fp8_e4m3" and m.fp8_stream is True and m.w8 is None
    with pytest.raises(NotImplementedError):   # K = 544 is no multiple of 64
        DFlashDraftModel(H.tiny_cfg(intermediate_size=544), device="cpu", weight_format="fp8_e4m3")
