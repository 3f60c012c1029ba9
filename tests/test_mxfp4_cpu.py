"""MXFP4 weights without a GPU: the quantiser's properties, the packers against a plainly written
unpacker of the documented DFL_W_MXFP4 layout, the C ABI's refusals (small integers for pointers: nothing launches), and
the draft model's format option and path table."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import helpers as H
from dflash_amd import ops

BF16, U8 = torch.bfloat16, torch.uint8
GRID = torch.tensor(ops.E2M1_VALUES)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bits(x):
    return x.contiguous().view(torch.int16)


def _matrices():
    """Random bf16 [N, K] matrices: plain, scaled by 2^+-40, with all-zero blocks and with a wide spread inside a row."""
    g = gen(1)
    base = torch.randn(48, 384, generator=g) * 0.05
    spread = base * torch.exp2(torch.randint(-12, 13, (48, 384), generator=g).float())
    holes = base.clone()
    holes[3, 32:64] = 0
    holes[17] = 0
    return {"plain": base.to(BF16), "up40": (base * 2.0 ** 40).to(BF16), "down40": (base * 2.0 ** -40).to(BF16),
            "holes": holes.to(BF16), "spread": spread.to(BF16)}


@pytest.mark.parametrize("name", ["plain", "up40", "down40", "holes", "spread"])
def test_quantiser_properties(name):
    w = _matrices()[name]
    n, k = w.shape
    codes, sc = ops.quantize_mxfp4_rows(w)
    assert codes.dtype == U8 and sc.dtype == U8 and codes.shape == (n, k // 2) and sc.shape == (n, k // 32)
    assert int(sc.min()) >= 7 and int(sc.max()) <= 247
    dq = ops.dequantize_mxfp4_rows(codes, sc)
    assert dq.dtype == BF16 and dq.shape == w.shape
    # exact in bf16: the double-precision value of code * 2^e survives the bf16 rounding unchanged
    c = torch.stack([codes & 15, codes >> 4], dim=2).view(n, k).long()
    mag, neg = GRID.double()[c & 7], (c & 8) != 0
    scale = torch.exp2(sc.double() - 127).repeat_interleave(32, dim=1)
    val = torch.where(neg, -mag, mag) * scale
    assert torch.equal(dq.double(), val)
    # the scale rule: 2^ceil(log2(amax / 6)), exponent 0 for an all-zero block
    amax = w.double().abs().view(n, k // 32, 32).amax(dim=2)
    e = sc.double() - 127
    live = amax > 0
    assert torch.all(e[~live] == 0)
    assert torch.all(6 * torch.exp2(e[live]) >= amax[live]) and torch.all(6 * torch.exp2(e[live] - 1) < amax[live])
    # |w - dq| <= half the e2m1 spacing at that magnitude, times the block scale; nothing saturates (the ceil rule)
    a = (w.double() / scale).abs()
    assert float(a.max()) <= 6.0
    spacing = torch.where(a < 2, 0.5, torch.where(a < 4, 1.0, 2.0))
    assert torch.all((w.double() - val).abs() <= spacing / 2 * scale)
    # the block maximum is never clamped: it lies in (3, 6] scales and its code is that of the nearest grid point
    assert torch.all(mag.view(n, k // 32, 32).amax(dim=2)[live] >= 3.0)
    # value idempotence, bit for bit
    dq2 = ops.dequantize_mxfp4_rows(*ops.quantize_mxfp4_rows(dq))
    assert torch.equal(bits(dq2), bits(dq))


def test_quantiser_ties_go_to_the_even_code_and_zero_is_positive():
    """Block maximum 6 (scale 1): the midpoints .25 .75 1.25 1.75 2.5 3.5 5 round to codes 0 2 2 4 4 6 6."""
    w = torch.zeros(1, 32)
    w[0, :9] = torch.tensor([6.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -0.25])
    codes, sc = ops.quantize_mxfp4_rows(w.to(BF16))
    c = torch.stack([codes & 15, codes >> 4], dim=2).view(-1)
    assert sc.tolist() == [[127]] and c[:9].tolist() == [7, 0, 2, 2, 4, 4, 6, 6, 0]
    codes, _ = ops.quantize_mxfp4_rows((-w).to(BF16))
    c = torch.stack([codes & 15, codes >> 4], dim=2).view(-1)
    assert c[:9].tolist() == [15, 0, 10, 10, 12, 12, 14, 14, 0]


def test_quantiser_exponent_clamp():
    """Blocks beyond 6 * 2^120 are clamped at +-6 by the exponent clamp alone; blocks below 2^-120 keep exponent -120."""
    w = torch.zeros(2, 32)
    w[0, 0], w[0, 1] = 2.0 ** 127, -(2.0 ** 124)
    w[1, 0], w[1, 1] = 2.0 ** -126, 2.0 ** -121
    codes, sc = ops.quantize_mxfp4_rows(w.to(BF16))
    assert sc.view(-1).tolist() == [247, 7]
    dq = ops.dequantize_mxfp4_rows(codes, sc).double()
    assert dq[0, 0] == 6 * 2.0 ** 120 and dq[0, 1] == -6 * 2.0 ** 120
    assert dq[1, 0] == 0 and dq[1, 1] == 2.0 ** -121


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_quantiser_refuses_non_finite_input(bad):
    w = torch.ones(16, 128, dtype=BF16)
    w[5, 77] = bad
    with pytest.raises(ValueError, match="non-finite"):
        ops.quantize_mxfp4_rows(w)


# ---------------------------------------------------------------- the packers against the documented layout
def unpack_reference(data, N, K):
    """The DFL_W_MXFP4 layout read back element by element, as include/dflash_hip.h words it: codes [N/16][K/128][64
    lanes][16 B], lane l = column 16 t + (l & 15), kq = l >> 4, dword d = k-step 4 j + d, its 8 codes those of k = 128 j +
    32 d + 8 kq .., low nibble first; scales [N/16][K/128][16 columns][4 B] at byte N * K / 2, byte d = k-step 4 j + d."""
    b = data.tolist()
    codes = [[0] * K for _ in range(N)]
    scales = [[0] * (K // 32) for _ in range(N)]
    for t in range(N // 16):
        for j in range(K // 128):
            for lane in range(64):
                n, kq = 16 * t + (lane & 15), lane >> 4
                word = ((t * (K // 128) + j) * 64 + lane) * 16
                for d in range(4):
                    for i in range(8):
                        byte = b[word + 4 * d + i // 2]
                        codes[n][128 * j + 32 * d + 8 * kq + i] = (byte >> 4) if i & 1 else (byte & 15)
            for col in range(16):
                for d in range(4):
                    scales[16 * t + col][4 * j + d] = b[N * K // 2 + ((t * (K // 128) + j) * 16 + col) * 4 + d]
    return torch.tensor(codes, dtype=U8), torch.tensor(scales, dtype=U8)


def _random_codes(N, K, seed):
    g = gen(seed)
    codes = torch.randint(0, 256, (N, K // 2), generator=g).to(U8)
    scales = torch.randint(7, 248, (N, K // 32), generator=g).to(U8)
    return codes, scales


def _nibbles(codes):
    return torch.stack([codes & 15, codes >> 4], dim=2).view(codes.shape[0], -1)


@pytest.mark.parametrize("N", [16, 48])
@pytest.mark.parametrize("K", [128, 384])
def test_pack_weight_mxfp4_layout(N, K):
    codes, scales = _random_codes(N, K, N + K)
    w4 = ops.pack_weight_mxfp4(codes, scales)
    assert isinstance(w4, ops.Mxfp4Weight) and (w4.N, w4.K) == (N, K)
    assert w4.data.dtype == U8 and w4.data.numel() == N * K // 2 + N * K // 32
    c, s = unpack_reference(w4.data, N, K)
    assert torch.equal(c, _nibbles(codes)) and torch.equal(s, scales)


@pytest.mark.parametrize("I", [16, 48])
@pytest.mark.parametrize("K", [128, 384])
def test_pack_weight_gateup_mxfp4_layout(I, K):
    """Tiles interleaved (gate tile p, up tile p) as dfl_pack_weight_gateup, scales in the same tile order."""
    gc, gs = _random_codes(I, K, I + K)
    uc, us = _random_codes(I, K, I + K + 1)
    w4 = ops.pack_weight_gateup_mxfp4(gc, gs, uc, us)
    assert (w4.N, w4.K) == (2 * I, K) and w4.data.numel() == 2 * I * K // 2 + 2 * I * K // 32
    c, s = unpack_reference(w4.data, 2 * I, K)
    for p in range(I // 16):
        rows = slice(16 * p, 16 * p + 16)
        assert torch.equal(c[32 * p:32 * p + 16], _nibbles(gc)[rows]) and torch.equal(s[32 * p:32 * p + 16], gs[rows])
        assert torch.equal(c[32 * p + 16:32 * p + 32], _nibbles(uc)[rows]) and torch.equal(s[32 * p + 16:32 * p + 32], us[rows])


def test_packers_refuse_other_shapes():
    codes, scales = _random_codes(16, 128, 3)
    with pytest.raises(ValueError):
        ops.pack_weight_mxfp4(codes[:8], scales[:8])               # N % 16
    with pytest.raises(ValueError):
        ops.pack_weight_mxfp4(codes[:, :32], scales[:, :2])        # K = 64
    with pytest.raises(ValueError):
        ops.pack_weight_mxfp4(codes, scales[:, :3])
    with pytest.raises(ValueError):
        ops.quantize_mxfp4_rows(torch.zeros(16, 48, dtype=BF16))   # K % 32


# ---------------------------------------------------------------- the C ABI's refusals
def test_abi_refuses_mxfp4_where_no_kernel_takes_it():
    """-22 and the entry point's name in dfl_last_error, nothing launched: DFL_W_MXFP4 into entry points without a W4
    form; with a scale pointer; with K = 192."""
    from dflash_amd import _lib
    h = _lib.lib()
    assert _lib.W_MXFP4 == 3

    def refused(name, *args):
        assert getattr(h, name)(*args) == -22, name
        assert (name + ":").encode() in h.dfl_last_error(), (name, h.dfl_last_error())

    w4 = lambda scale=None: _lib.Weight(4096, scale, _lib.W_MXFP4)      # noqa: E731
    rows = _lib.Rows()
    rows.frag, rows.mode, rows.valid_word = 16, 0, -1
    xb = _lib.RowsBatch()
    xb.r0.frag, xb.r0.mode, xb.frag_stride = 16, 0, 4096 * 16
    refused("dfl_gemm_sample", w4(), C.byref(rows), 64, 128, 0, 16, None, -1, 16, 16, 0, None, None, 1, 1.0, 0, None, 0, 0,
            0, None)
    assert b"format 3" in h.dfl_last_error()
    refused("dfl_gemm_silu_mul_batch", w4(), C.byref(xb), 2, 64, 256, 16, 1024, 16, 16, None)
    assert b"format 3" in h.dfl_last_error()
    refused("dfl_gemm_f32_batch", w4(), C.byref(xb), 2, 64, 256, 16, None, None)
    refused("dfl_gemm_argmax_batch", w4(), C.byref(xb), 2, 64, 256, 0, 16, 16, 2, 16, 16, 16, 0, None, 0, None)
    refused("dfl_moe_gate_up", w4(), 16, 4, 64, 2048, 16, 16, 16, None, -1, None)
    assert b"format 3" in h.dfl_last_error()
    refused("dfl_moe_down", w4(), 64 * 2048, 16, 1024, 16, 16, 16, 4, 2048, 64, 1, 16, None)
    refused("dfl_moe_grouped_gate_up", w4(), 2 * 64 * 256, 16, 16, 16, 4, 64, 256, 16, 16, None, 16, None)
    refused("dfl_moe_grouped_down", w4(), 64 * 256, 16, 16, 16, 4, 256, 64, 16, 16, 16, None)
    assert b"format 3" in h.dfl_last_error()
    # the three entry points that take it: a scale pointer, K = 192
    resid = lambda w, K: refused("dfl_gemm_resid", w, C.byref(rows), 16, K, 16, 16, 0, None, 0, None, None, None)   # noqa: E731
    silu = lambda w, K: refused("dfl_gemm_silu_mul", w, C.byref(rows), 16, K, 16, None, None)                      # noqa: E731
    arg = lambda w, K: refused("dfl_gemm_argmax", w, C.byref(rows), 16, K, 0, 16, None, -1, 16, 16, 0, None, None,  # noqa: E731
                               None, None, None)
    for call in (resid, silu, arg):
        call(w4(4096), 128)
        assert b"scale" in h.dfl_last_error()
        call(w4(), 192)
        assert b"128" in h.dfl_last_error()
    resid(w4(4096), 8192)        # (the K-chunked form)
    assert b"scale" in h.dfl_last_error()
    resid(w4(), 8192 + 64)
    assert b"128" in h.dfl_last_error()


# ---------------------------------------------------------------- the model's option and path table
def test_weight_format_option():
    from dflash_amd import DFlashDraftModel
    from dflash_amd.model import WEIGHT_FORMATS
    assert "mxfp4" in WEIGHT_FORMATS
    with pytest.raises(ValueError, match="weight_format"):
        DFlashDraftModel(H.tiny_cfg(), device="cpu", weight_format="mxfp6")
    m = DFlashDraftModel(H.tiny_cfg(), device="cpu", weight_format="mxfp4")
    assert m.weight_format == "mxfp4" and m.mxfp4_stream is True and m.w4 is None and m.w8 is None
    assert m.x13 is False                                   # stream_format is ignored: the 13-bit twins are for bf16 weights
    assert DFlashDraftModel(H.tiny_cfg(), device="cpu").weight_format == "bf16"      # off by default
    with pytest.raises(NotImplementedError, match="128"):
        DFlashDraftModel(H.tiny_cfg(intermediate_size=1088), device="cpu", weight_format="mxfp4")   # % 64 but not % 128
    DFlashDraftModel(H.tiny_cfg(intermediate_size=1088), device="cpu", weight_format="fp8_e4m3")     # (e4m3 takes it)


def test_the_target_takes_no_mxfp4():
    from dflash_amd import NativeTarget
    with pytest.raises(ValueError, match="weight_format"):
        NativeTarget.check_config(SimpleNamespace(), weight_format="mxfp4")


def test_streams_mxfp4_path_table():
    """True only for: an mxfp4 model with mxfp4_stream, one 16-row tile, attn_impl "head", no fuse_oproj, no wide hidden."""
    from dflash_amd import DFlashDraftModel
    m = DFlashDraftModel(H.tiny_cfg(), device="cpu", weight_format="mxfp4")
    assert not m.streams_mxfp4(16)                          # nothing loaded
    m.w4 = {"layers": []}
    assert m.streams_mxfp4(1) and m.streams_mxfp4(16) and not m.streams_mxfp4(17) and not m.streams_mxfp4(32)
    assert not m.streams_fp8(16) and not m.streams_fp8_tiles()
    for attr, off in (("mxfp4_stream", False), ("attn_impl", "fused"), ("fuse_oproj", True), ("wide_hidden", True)):
        keep = getattr(m, attr)
        setattr(m, attr, off)
        assert not m.streams_mxfp4(16), attr
        setattr(m, attr, keep)
        assert m.streams_mxfp4(16)
    b = DFlashDraftModel(H.tiny_cfg(), device="cpu")
    b.w4 = None
    assert not b.streams_mxfp4(16)


def test_row_layers_hands_over_the_four_twins():
    layers = [{"qkv": 1, "o": 2, "gu": 3, "down": 4, "ln1": 5}]
    twins = [{"qkv": "q4", "o": "o4", "gu": "g4", "down": "d4"}]
    out = ops.row_layers(layers, twins, [None], True, {})
    assert out == [{"qkv": "q4", "o": "o4", "gu": "g4", "down": "d4", "ln1": 5}]
