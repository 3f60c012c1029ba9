"""The K-chunked form of the 13-bit bf16 weight stream (DFL_W_BF16X13 at K a multiple of 2048 above 4096; DESIGN.md
section 11, "down_proj and fc") without a GPU: the packer against a NumPy decoder written from the format's description
— the meta pair of item (tile t, chunk c, wave w) at index (t * nch + c) * 16 + w — the unchanged bytes at K = 2048 /
4096, dfl_gemm_resid's refusals, the packer's account of every matrix the GPU tests stream
(tests/bf16x13_chunked_cases.py) and ops.row_layers with the down twins."""
import ctypes as C

import numpy as np
import pytest
import torch

import bf16x13_chunked_cases as XC
from test_bf16x13_cpu import QUAD, bits, decode, rand_w, to_packed

BF16 = torch.bfloat16


def decode_chunked(data: np.ndarray, N: int, K: int) -> np.ndarray:
    """The format at K > 4096 -> the packed bf16 bit patterns, uint16 [N/16][K/32][64][8].  The quads are those of the
    K <= 4096 form; what differs is the meta block: [N/16][nch][16] pairs, nch = K / 2048, and a patch word's k-step
    counts inside the item's ONE quad."""
    nt, KS, nch = N // 16, K // 32, K // 2048
    Q = KS // 4
    qb = nt * Q * QUAD
    assert K > 4096 and K % 2048 == 0 and data.dtype == np.uint8 and data.size == qb + nt * nch * 16 * 8
    quads = data[:qb].reshape(nt, Q, QUAD)
    meta = data[qb:].view(np.uint32).reshape(nt * nch * 16, 2)
    base = meta[:, 0].reshape(nt, nch * 16)
    assert (base == base[:, :1]).all() and (base <= 112).all()      # one base per tile, repeated per (chunk, wave)
    hb = base[:, 0].astype(np.uint16).reshape(nt, 1, 1, 1)
    low = [quads[:, :, p * 1024:(p + 1) * 1024].reshape(nt, Q, 64, 2, 8) for p in (0, 1)]
    nib = quads[:, :, 2048:3072].reshape(nt, Q, 64, 4, 4)
    sgn = quads[:, :, 3072:].reshape(nt, Q, 64, 4)
    out = np.zeros((nt, Q, 4, 64, 8), np.uint16)
    for f in range(4):
        lo = low[f >> 1][:, :, :, f & 1, :].astype(np.uint16)
        code = np.concatenate([nib[:, :, :, f, :] & 15, nib[:, :, :, f, :] >> 4], axis=-1).astype(np.uint16)
        sign = np.stack([(sgn[:, :, :, j % 4] >> (2 * f + j // 4)) & 1 for j in range(8)], axis=-1).astype(np.uint16)
        out[:, :, f] = lo | (np.where(code == 0, 0, hb + code).astype(np.uint16) << 8) | (sign << 15)
    for t in range(nt):
        for c in range(nch):
            for w in range(16):
                pw = int(meta[(t * nch + c) * 16 + w, 1])
                if pw >> 31:
                    assert (pw >> 28) & 7 < 4                       # a k-step of the quad
                    out[t, 16 * c + w, (pw >> 28) & 7, (pw >> 22) & 63, (pw >> 19) & 7] = pw & 0xffff
    return out.reshape(nt, KS, 64, 8)


@pytest.mark.parametrize("N,K", [(32, 6144), (48, 8192)])
def test_random_matrices_round_trip(N, K):
    from dflash_amd import ops
    w = rand_w(N, K, 7 + K)
    wi = w.view(torch.int16)
    top = int((wi[:16] & 0x7fff).max()) >> 8
    below = ((top - 15) << 8) | 0x5a
    planted = [(0, 0, 0, 0), (0, K // 2048 - 1, 15, 127), (1, 1, 7, 40), (N // 16 - 1, K // 2048 - 1, 0, 64)]
    for t, c, wv, off in planted:                                   # one below-window element in four items
        wi[16 * t + 3, (16 * c + wv) * 128 + off] = below
    wp = to_packed(w)
    w13, rep = ops.pack_weight_bf16x13(wp, N, K, tiles_per_pass=2)  # (several passes, the last one short at 3 tiles)
    assert w13 is not None and rep == {"items": N // 16 * (K // 128), "patched": len(planted), "refused": 0}
    assert w13.data.numel() == N * K * 13 // 8 + N // 16 * (K // 128) * 8
    got = decode_chunked(w13.data.numpy(), N, K)
    assert np.array_equal(got.reshape(-1), bits(wp)), "the 13-bit form does not reproduce the packed bf16 weight"
    # the patch words sit where the item map says: pair (t * nch + c) * 16 + w
    nch = K // 2048
    meta = w13.data.numpy()[N // 16 * (K // 128) * QUAD:].view(np.uint32).reshape(-1, 2)
    assert sorted(np.nonzero(meta[:, 1] >> 31)[0].tolist()) == sorted((t * nch + c) * 16 + wv for t, c, wv, _ in planted)


def test_two_exceptions_in_one_chunked_item_refuse_and_in_two_items_do_not():
    from dflash_amd import ops
    N, K = 32, 6144
    w = rand_w(N, K, 5)
    wi = w.view(torch.int16)
    below = (((int((wi[:16] & 0x7fff).max()) >> 8) - 15) << 8) | 0x11
    wi[1, 128 * 17 + 3] = below
    wi[2, 128 * 33 + 3] = below            # the same wave (1), another chunk: its own item
    w13, rep = ops.pack_weight_bf16x13(to_packed(w), N, K)
    assert w13 is not None and rep["patched"] == 2 and rep["refused"] == 0
    wi[5, 128 * 17 + 100] = below          # a second one in (tile 0, chunk 1, wave 1)
    w13, rep = ops.pack_weight_bf16x13(to_packed(w), N, K)
    assert w13 is None and rep["refused"] == 1 and rep["patched"] == 1
    w2 = rand_w(N, K, 6)
    XC.plant_refusal(w2, 1, 2, 9)
    assert ops.pack_weight_bf16x13(to_packed(w2), N, K)[0] is None


@pytest.mark.parametrize("K", [2048, 4096])
def test_the_single_pass_layout_is_unchanged(K):
    """K = 2048 / 4096: the bytes the parent's layout description gives — decoded by the existing NumPy decoder (meta
    [N/16][16]) — and the sizes and item counts as they were."""
    from dflash_amd import ops
    N = 48
    w = rand_w(N, K, K)
    wi = w.view(torch.int16)
    below = (((int((wi[16:32] & 0x7fff).max()) >> 8) - 15) << 8) | 0x5a
    wi[16, K // 16 * 3 + 5] = below
    wp = to_packed(w)
    w13, rep = ops.pack_weight_bf16x13(wp, N, K)
    assert rep == {"items": N // 16 * 16, "patched": 1, "refused": 0}
    assert w13.data.numel() == N * K * 13 // 8 + N // 16 * 16 * 8
    assert np.array_equal(decode(w13.data.numpy(), N, K).reshape(-1), bits(wp))
    meta = w13.data.numpy()[N // 16 * (K // 128) * QUAD:].view(np.uint32).reshape(N // 16, 16, 2)
    assert [a.tolist() for a in np.nonzero(meta[:, :, 1] >> 31)] == [[1], [3]]
    assert (int(meta[1, 3, 1]) >> 28) & 7 == (K // 16 * 3 + 5) // 32 - 3 * (K // 512)


def test_covers_and_value_errors():
    from dflash_amd import ops
    for K in (6144, 8192, 12288, 14336, 20480):
        assert ops.bf16x13_covers(32, K)
    for K in (5120, 6144 + 128, 512, 4096 + 2048 - 32):
        assert not ops.bf16x13_covers(32, K)
        with pytest.raises(ValueError):
            ops.pack_weight_bf16x13(torch.zeros(32 * K, dtype=BF16), 32, K)
        assert ops.bf16x13_twin(torch.zeros(32 * K, dtype=BF16), 32, K, "down") is None    # before the twin table
    assert not ops.bf16x13_covers(24, 6144)
    assert "down" in ops.X13_KINDS and "fc" in ops.X13_KINDS


def test_gemm_resid_refusals():
    from dflash_amd import _lib
    h = _lib.lib()
    rows = _lib.Rows()
    rows.frag, rows.mode, rows.valid_word = 16, 0, -1
    W13 = _lib.W_BF16X13

    def refused(text, w, N, K, h_io=16):
        assert h.dfl_gemm_resid(w, C.byref(rows), N, K, h_io, N, 0, None, 0, None, None, None) == -22
        err = h.dfl_last_error()
        assert b"dfl_gemm_resid:" in err and text in err, err

    refused(b"no scale", _lib.Weight(4096, 4096, W13), 16, 6144)
    for K in (5120, 4096, 2048, 6144 + 128):       # like every K the chunked layout does not cover
        refused(b"unknown weight format 2", _lib.Weight(4096, None, W13), 16, K)
    refused(b"null", _lib.Weight(None, None, W13), 16, 6144)
    refused(b"null", _lib.Weight(4096, None, W13), 16, 6144, h_io=None)


@pytest.mark.parametrize("N,K", XC.SHAPES)
def test_generated_cases_are_in_format_by_the_packers_account(N, K):
    """Every matrix the GPU file streams: nothing refused, exactly the planted patches — one in every (chunk, wave) item
    of the patch tiles, which are the tiles some workgroups walk first and second — and at least five bases (two or
    three tiles: one per tile)."""
    from dflash_amd import ops
    case = XC.chunked_case(N, K)
    nt, nq, nch = N // 16, K // 128, K // 2048
    tiles, zero_tile, edge_tile = XC.layout_for(N)
    assert case.patch_tiles == tiles and len(case.patches) == len(tiles) * nq
    assert sorted({(p.tile, p.wave) for p in case.patches}) == [(t, q) for t in tiles for q in range(nq)]
    plan = XC.plan_resid(N)
    firsts, seconds = {p[0] for p in plan}, {p[1] for p in plan if len(p) > 1}
    assert set(tiles) & firsts and (not seconds or set(tiles) & seconds)
    if N == 4112:
        assert len(plan) == 129 and plan[0] == [0, 129] and plan[128] == [128] and tiles == [0, 1, 64, 128, 129, 130, 193]
    wp = to_packed(case.w)
    w13, rep = ops.pack_weight_bf16x13(wp, N, K)
    assert w13 is not None and rep == {"items": nt * nq, "patched": len(case.patches), "refused": 0}
    data = w13.data.numpy()
    assert np.array_equal(decode_chunked(data, N, K).reshape(-1), bits(wp))
    meta = data[nt * nq * QUAD:].view(np.uint32).reshape(nt, nch, 16, 2)
    assert len(np.unique(meta[:, 0, 0, 0])) >= min(5, nt)          # (two or three tiles: a base of its own for each)
    if zero_tile is not None:
        assert (meta[zero_tile, :, :, 0] == 0).all()
    for p in case.patches:                          # the word of each item, field by field
        pw = int(meta[p.tile, p.wave // 16, p.wave % 16, 1])
        assert pw >> 31 and ((pw >> 28) & 7, (pw >> 22) & 63, (pw >> 19) & 7, pw & 0xffff) == (p.kstep, p.lane, p.element, p.bits)
        assert p.col == p.wave * 128 + p.kstep * 32 + (p.lane >> 4) * 8 + p.element and p.row == 16 * p.tile + (p.lane & 15)
    wb = bits(case.w)
    for row, col, v in case.edges:
        assert wb[row, col] == v and row // 16 == edge_tile
    # successive chunks of one wave differ in k-step, element and lane
    by = {(p.tile, p.wave): p for p in case.patches}
    for t in tiles:
        for wv in range(16):
            seq = [by[(t, 16 * c + wv)] for c in range(nch)]
            assert len({(s.kstep, s.element, s.lane) for s in seq}) == nch


def test_row_layers_with_and_without_down_twins():
    from dflash_amd import ops
    layers = [dict(qkv=f"qkv.{i}", o=f"o.{i}", gu=f"gu.{i}", down=f"down.{i}", ln1=f"ln1.{i}") for i in range(4)]
    gu13 = ["gu13.0", None, "gu13.2", None]
    down13 = ["down13.0", "down13.1", None, None]
    got = ops.row_layers(layers, None, gu13, False, {}, down13)
    assert got[0] == dict(layers[0], gu="gu13.0", down="down13.0") and got[1] == dict(layers[1], down="down13.1")
    assert got[2] == dict(layers[2], gu="gu13.2") and got[3] is layers[3]
    assert layers[0]["down"] == "down.0" and layers[1]["down"] == "down.1"
    # without: the five-argument call, and None, as before
    for plain in (ops.row_layers(layers, None, gu13, False, {}), ops.row_layers(layers, None, gu13, False, {}, None)):
        assert plain[0] == dict(layers[0], gu="gu13.0") and plain[1] is layers[1] and plain[3] is layers[3]
    # e4m3 ignores the 13-bit twins
    l8 = [dict(qkv=f"q8.{i}", o=f"o8.{i}", gu=f"g8.{i}", down=f"d8.{i}") for i in range(4)]
    codes = ops.row_layers(layers, l8, gu13, True, {}, down13)
    assert all(c["down"] == f"d8.{i}" and c["gu"] == f"g8.{i}" for i, c in enumerate(codes))


def test_model_row_layers_with_and_without_down13():
    """DFlashDraftModel.row_layers hands down13 on, and answers for an object that has none."""
    from dflash_amd.model import DFlashDraftModel
    m = object.__new__(DFlashDraftModel)   # (no device: only what row_layers reads)
    L = [dict(qkv=f"qkv.{i}", o=f"o.{i}", gu=f"gu.{i}", down=f"down.{i}") for i in range(2)]
    m.w, m.w8, m.gu13, m._row_layers = {"layers": L}, None, [None, "gu13.1"], {}
    m.fp8_stream, m.attn_impl, m.fuse_oproj, m.wide_hidden = False, "head", False, False
    assert m.row_layers(16) == [L[0], dict(L[1], gu="gu13.1")]
    m.down13, m._row_layers = ["down13.0", None], {}
    assert m.row_layers(16) == [dict(L[0], down="down13.0"), dict(L[1], gu="gu13.1")]
