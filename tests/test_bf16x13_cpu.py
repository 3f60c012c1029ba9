"""The lossless 13-bit bf16 weight stream (DFL_W_BF16X13) without a GPU: the packer against a
NumPy decoder written from the format's description, the entry points' refusals, the auto -> bf16 fall-back, and the
packer's account of every matrix the GPU tests stream (tests/bf16x13_cases.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

BF16 = torch.bfloat16
QUAD = 3328


def to_packed(w: torch.Tensor) -> torch.Tensor:
    """[N, K] bf16 -> the packed bf16 layout [N/16][K/32][64 lanes][8] (flat): lane l = column l & 15, k group l >> 4."""
    n, k = w.shape
    return w.view(n // 16, 16, k // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1).contiguous()


def to_packed_gateup(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    i, k = gate.shape
    g, u = to_packed(gate).view(i // 16, -1), to_packed(up).view(i // 16, -1)
    return torch.stack([g, u], dim=1).reshape(-1).contiguous()


def decode(data: np.ndarray, N: int, K: int) -> np.ndarray:
    """The format as the header states it -> the packed bf16 bit patterns, uint16 [N/16][K/32][64][8]."""
    nt, KS = N // 16, K // 32
    Q, nfr = KS // 4, KS // 16
    qb = nt * Q * QUAD
    assert data.dtype == np.uint8 and data.size == qb + nt * 16 * 8
    quads = data[:qb].reshape(nt, Q, QUAD)
    meta = data[qb:].view(np.uint32).reshape(nt, 16, 2)
    assert (meta[:, :, 0] == meta[:, :1, 0]).all() and (meta[:, :, 0] <= 112).all()   # one base per tile
    hb = meta[:, 0, 0].astype(np.uint16).reshape(nt, 1, 1, 1)
    low = [quads[:, :, p * 1024:(p + 1) * 1024].reshape(nt, Q, 64, 2, 8) for p in (0, 1)]
    nib = quads[:, :, 2048:3072].reshape(nt, Q, 64, 4, 4)
    sgn = quads[:, :, 3072:].reshape(nt, Q, 64, 4)
    out = np.zeros((nt, Q, 4, 64, 8), np.uint16)
    for f in range(4):
        lo = low[f >> 1][:, :, :, f & 1, :].astype(np.uint16)
        code = np.concatenate([nib[:, :, :, f, :] & 15, nib[:, :, :, f, :] >> 4], axis=-1).astype(np.uint16)
        sign = np.stack([(sgn[:, :, :, j % 4] >> (2 * f + j // 4)) & 1 for j in range(8)], axis=-1).astype(np.uint16)
        h7 = np.where(code == 0, 0, hb + code).astype(np.uint16)
        out[:, :, f] = lo | (h7 << 8) | (sign << 15)
    out = out.reshape(nt, KS, 64, 8)
    for t, w in zip(*np.nonzero(meta[:, :, 1] >> 31)):
        pw = int(meta[t, w, 1])
        out[t, w * nfr + ((pw >> 28) & 7), (pw >> 22) & 63, (pw >> 19) & 7] = pw & 0xffff
    return out


def bits(t: torch.Tensor) -> np.ndarray:
    return t.view(torch.int16).numpy().view(np.uint16)


def from_bits(v: int) -> torch.Tensor:
    return torch.tensor([v if v < 32768 else v - 65536], dtype=torch.int16).view(BF16)[0]


def rand_w(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, k, generator=g) * 0.02).to(BF16)


def roundtrip(wp, N, K):
    from dflash_amd import ops
    w13, rep = ops.pack_weight_bf16x13(wp, N, K, tiles_per_pass=3)   # (several passes, the last one short)
    assert w13 is not None and rep["refused"] == 0, rep
    assert w13.data.numel() == N * K * 13 // 8 + N // 16 * 16 * 8
    got = decode(w13.data.numpy(), N, K)
    assert np.array_equal(got.reshape(-1), bits(wp)), "the 13-bit form does not reproduce the packed bf16 weight"
    return rep


@pytest.mark.parametrize("K", [2048, 4096])
def test_random_matrices_round_trip(K):
    rep = roundtrip(to_packed(rand_w(80, K, 1)), 80, K)
    assert rep["items"] == 5 * 16
    gate, up = rand_w(48, K, 2), rand_w(48, K, 3) * 64     # (gate and up tiles six binades apart: a base per packed tile)
    roundtrip(to_packed_gateup(gate, up), 96, K)


def test_planted_values_round_trip():
    K = 4096
    w = rand_w(64, K, 4)
    top = int(bits(w[:16].contiguous()).max() & 0x7fff) >> 8           # tile 0's largest H & 0x7f
    hb = top - 15
    assert hb >= 1
    cases = {"+0": 0x0000, "-0": 0x8000, "denormal": 0x0001, "-denormal": 0x807f, "exponent 1": 0x0080,
             "-exponent 1": 0x80ff, "top binade": (top << 8) | 0xff, "-top binade": 0x8000 | (top << 8) | 0x80,
             "lowest window binade": ((hb + 1) << 8) | 0x00, "-lowest window binade": 0x8000 | ((hb + 1) << 8) | 0x7f}
    # the first and the last k-step of a wave's share (wave 0: columns 0..255, wave 15: 3840..4095), lanes 0 and 63
    spots = [(0, 0), (15, 3840 + 7 * 32 + 31), (0, 7 * 32 + 24), (15, 3840), (5, 100)]
    for i, (name, v) in enumerate(cases.items()):
        r, c = spots[i % len(spots)]
        w[r, (c + 8 * (i // len(spots))) % K] = from_bits(v)
    w[16:32] = 0                                                       # an all-zero tile: base 0, every code 0
    w[32:48] = w[32:48] * 2.0 ** -100                                  # a tile deep down the exponent range
    w[48:64] = w[48:64] * 2.0 ** 124                                   # a tile at the top of the range, and in it
    w[48, 5] = from_bits(0x7f7f)                                       # the largest finite bf16: base 112
    w[49, 6] = from_bits((0x7f7f >> 8) - 14 << 8)                      # ... and the lowest binade of ITS window
    rep = roundtrip(to_packed(w), 64, K)
    assert rep["patched"] == 0


def test_one_below_window_element_is_patched_exactly():
    for K in (2048, 4096):
        w = rand_w(32, K, 5)
        top = int(bits(w[16:].contiguous()).max() & 0x7fff) >> 8
        low = 0x8000 | ((top - 15) << 8) | 0x55                        # nonzero, one step below the window
        w[16 + 15, K - 1] = from_bits(low)                             # tile 1, wave 15, last k-step, lane 63, element 7
        w[3, 0] = from_bits(low)                                       # tile 0, wave 0, first k-step, lane 3, element 0
        rep = roundtrip(to_packed(w), 32, K)
        assert rep["patched"] == 2 and rep["refused"] == 0


def _generated_cases():
    import bf16x13_cases as X
    return ([("argmax", V, K, ext) for V, K in X.ARGMAX_SHAPES for ext in (False, True)]
            + [("silu", I, K, False) for I, K in X.SILU_SHAPES])


@pytest.mark.parametrize("kind,n,K,extreme", _generated_cases())
def test_generated_cases_are_in_format_by_the_packers_account(kind, n, K, extreme):
    """What keeps the GPU tests over tests/bf16x13_cases.py honest: every matrix they stream is in format by the PACKER's
    account — nothing refused, exactly the planted patches, each patch word naming the planted (k-step, lane, element,
    bits) — it decodes back bit for bit, its tiles have many bases, the items a workgroup walks one after the other have
    different ones, and the planted patches cover the classes the kernel's decode distinguishes."""
    import bf16x13_cases as X
    from dflash_amd import ops
    case = X.argmax_case(n, K, extreme) if kind == "argmax" else X.silu_case(n, K)
    N, nfr = case.N, K // 512
    wp = to_packed(case.w)
    w13, rep = ops.pack_weight_bf16x13(wp, N, K)
    assert w13 is not None and rep["refused"] == 0, rep
    assert rep["patched"] == len(case.patches) == 16 * len(case.patch_tiles), rep
    data = w13.data.numpy()
    assert np.array_equal(decode(data, N, K).reshape(-1), bits(wp)), "the 13-bit form does not reproduce the weight"
    meta = data[N // 16 * (K // 128) * QUAD:].view(np.uint32).reshape(N // 16, 16, 2)
    hb = meta[:, 0, 0].astype(int)
    assert len(set(hb.tolist())) >= 5 + 2 * extreme, sorted(set(hb.tolist()))
    assert hb[X.ZERO_TILE] == 0 and (not extreme or (hb[X.TOP_TILE] == 112 and hb[X.DEEP_TILE] == 0))
    wb = bits(case.w)
    for r, c, v in case.edges:
        assert wb[r, c] == v
    # the patch words against the table
    assert int((meta[:, :, 1] >> 31).sum()) == len(case.patches)
    for p in case.patches:
        pw = int(meta[p.tile, p.wave, 1])
        assert (pw >> 31, (pw >> 28) & 7, (pw >> 22) & 63, (pw >> 19) & 7, pw & 0xffff) == (1, p.kstep, p.lane, p.element, p.bits)
        assert wb[p.row, p.col] == p.bits and (p.row, p.col) == (16 * p.tile + (p.lane & 15),
                                                                 (p.wave * nfr + p.kstep) * 32 + (p.lane >> 4) * 8 + p.element)
        assert 1 <= (p.bits >> 8) & 0x7f <= hb[p.tile] and p.bits & 0x7fff, "not a nonzero element below the window"
    # the classes
    P = case.patches
    assert {p.kstep for p in P} == set(range(nfr)) and {p.element for p in P} == set(range(8))
    assert {0, 63} <= {p.lane for p in P} and {(p.lane >> 3) & 1 for p in P} == {0, 1}
    assert {0, 15} <= {p.wave for p in P} and len({p.wave for p in P} - {0, 15}) >= 2
    assert {p.bits >> 15 for p in P} == {0, 1}
    plan = X.plan_argmax(n) if kind == "argmax" else X.plan_silu(n)
    ptiles = set(case.patch_tiles)
    longest = max(len(items) for items in plan)
    for pos in range(longest):     # a patched tile at every position of a workgroup's sequence: first, second, third ...
        assert any(len(items) > pos and items[pos][0] in ptiles for items in plan), pos
    for items in plan:
        if all(t in ptiles for t, _ in items):      # the workgroups the patches sit in: a base per item
            assert all(hb[a[0]] != hb[b[0]] for a, b in zip(items, items[1:])), items
    differ = sum(all(hb[a[0]] != hb[b[0]] for a, b in zip(items, items[1:])) for items in plan)
    assert differ >= 0.8 * len(plan)
    halved = {t for items in plan for t, half in items if half >= 0}
    for t in halved & ptiles:                        # a halved tile: patches in both halves
        assert {(p.lane >> 3) & 1 for p in P if p.tile == t} == {0, 1}
    if kind == "argmax" and n != 8192:
        assert halved & ptiles
    if kind == "silu":
        assert {p.tile & 1 for p in P} == {0, 1}     # gate tiles and up tiles
        assert hb[0] != hb[1]


def test_model_helpers_of_the_generated_cases():
    """What the mixed-model session test does to a model's gate/up: tile shifts leave the matrix in format with a base
    per tile (and are undone exactly by the down columns' powers); plant_refusal makes the packer refuse it."""
    import bf16x13_cases as X
    from dflash_amd import ops
    K = 2048
    gate, up, down = rand_w(112, K, 9), rand_w(112, K, 10), rand_w(64, 112, 11)
    g0, u0, d0 = gate.clone(), up.clone(), down.clone()
    X.apply_tile_shifts(gate, up, down)
    s = torch.tensor(X.SHIFTS, dtype=torch.float64)
    t = torch.arange(112) // 16 * 2
    assert torch.equal(gate.double(), g0.double() * torch.exp2(s[t % 7]).view(-1, 1))
    assert torch.equal(up.double(), u0.double() * torch.exp2(s[(t + 1) % 7]).view(-1, 1))
    assert torch.equal(down.double(), d0.double() * torch.exp2(-s[t % 7] - s[(t + 1) % 7]).view(1, -1))
    w13, rep = ops.pack_weight_bf16x13(to_packed_gateup(gate, up), 224, K)
    assert w13 is not None and rep == {"items": 224, "patched": 0, "refused": 0}
    meta = w13.data.numpy()[224 // 16 * (K // 128) * QUAD:].view(np.uint32).reshape(14, 16, 2)
    assert len(set(meta[:, 0, 0].tolist())) >= 5 and all(meta[t, 0, 0] != meta[t + 1, 0, 0] for t in range(13))
    X.plant_refusal(gate, 4, 3)
    w13, rep = ops.pack_weight_bf16x13(to_packed_gateup(gate, up), 224, K)
    assert w13 is None and rep == {"items": 224, "patched": 0, "refused": 1}


def test_two_below_window_elements_in_one_item_refuse_the_matrix():
    from dflash_amd import ops
    K = 4096
    w = rand_w(32, K, 6)
    top = int(bits(w[:16].contiguous()).max() & 0x7fff) >> 8
    low = from_bits(((top - 15) << 8) | 0x01)
    w[0, 3], w[7, 200] = low, low                                      # both in tile 0, wave 0 (columns 0..255)
    w[1, 300] = low                                                    # wave 1: one exception, fine on its own
    w13, rep = ops.pack_weight_bf16x13(to_packed(w), 32, K)
    assert w13 is None and rep == {"items": 32, "patched": 1, "refused": 1}
    # auto -> bf16: the twin of a refused matrix is None (the caller keeps streaming plain bf16), and so is the twin of a
    # shape the layout does not cover or of a kind that is switched off
    wp = to_packed(w)
    assert ops.bf16x13_twin(wp, 32, K, "gateup") is None
    assert ops.bf16x13_report()["kept_bf16"] >= 1 and ops.bf16x13_report()["refused_items"] >= 1
    good = to_packed(rand_w(32, 512, 7))
    assert ops.bf16x13_twin(good, 32, 512, "gateup") is None
    assert not ops.bf16x13_covers(32, 512) and not ops.bf16x13_covers(24, 4096) and ops.bf16x13_covers(32, 2048)
    fine = to_packed(rand_w(32, 2048, 8))
    twin = ops.bf16x13_twin(fine, 32, 2048, "lm_head")
    assert isinstance(twin, ops.Bf16x13Weight) and ops.bf16x13_twin(fine, 32, 2048, "lm_head") is twin   # packed once
    with pytest.raises(ValueError):
        ops.pack_weight_bf16x13(good, 32, 512)
    with pytest.raises(ValueError):
        ops.check_stream_format("fp8")
    assert ops.check_stream_format("auto") and not ops.check_stream_format("bf16")


def test_models_fall_back_to_bf16_where_the_layout_does_not_apply():
    """stream_format="auto" on shapes the layout does not cover (hidden 512) keeps plain bf16 everywhere; an unknown
    value is refused before anything is built."""
    import helpers as H
    from dflash_amd.model import DFlashDraftModel
    from dflash_amd.target import NativeTarget
    with pytest.raises(ValueError, match="stream_format"):
        DFlashDraftModel(H.tiny_cfg(), device="cpu", stream_format="x13")
    with pytest.raises(ValueError, match="stream_format"):
        NativeTarget(None, stream_format="13")          # (refused before the model is looked at)
    m = DFlashDraftModel(H.tiny_cfg(), device="cpu")
    assert m.stream_format == "auto"
    assert DFlashDraftModel(H.tiny_cfg(), device="cpu", stream_format="bf16").stream_format == "bf16"


def test_entry_points_refuse_what_the_format_does_not_cover():
    from dflash_amd import _lib
    h = _lib.lib()
    rows = _lib.Rows()
    rows.frag, rows.mode, rows.valid_word = 16, 0, -1
    x = _lib.RowsBatch()
    x.r0.frag, x.r0.mode, x.frag_stride = 16, 0, 4096 * 16
    W13 = _lib.W_BF16X13
    assert W13 == 2

    def refused(name, text, *args):
        assert getattr(h, name)(*args) == -22, name
        err = h.dfl_last_error()
        assert (name + ":").encode() in err and text in err, (name, err)

    silu = lambda w, I, K: (w, C.byref(rows), I, K, 16, None, None)                      # noqa: E731
    argmax = lambda w, V, K: (w, C.byref(rows), V, K, 0, 16, None, -1, 16, 16, 0, None, None, None, None, None)  # noqa: E731
    # the format with a scale vector
    refused("dfl_gemm_silu_mul", b"no scale", *silu(_lib.Weight(4096, 4096, W13), 64, 4096))
    refused("dfl_gemm_argmax", b"no scale", *argmax(_lib.Weight(4096, 4096, W13), 64, 4096))
    # a K, i.e. a share per wave, that the quads do not cover
    for K in (512, 1024, 3072, 4096 - 128):
        refused("dfl_gemm_silu_mul", b"K = 2048 and K = 4096", *silu(_lib.Weight(4096, None, W13), 64, K))
        refused("dfl_gemm_argmax", b"K = 2048 and K = 4096", *argmax(_lib.Weight(4096, None, W13), 64, K))
    refused("dfl_gemm_silu_mul", b"null", *silu(_lib.Weight(None, None, W13), 64, 4096))
    # every other entry point keeps refusing the format
    smp = (C.byref(rows), 64, 4096, 0, 16, None, -1, 16, 16, 0, None, None, 1, 1.0, 0, None, 0, 0, 0, None)
    refused("dfl_gemm_sample", b"unknown weight format 2", _lib.Weight(4096, None, W13), *smp)
    refused("dfl_gemm_resid", b"unknown weight format 2", _lib.Weight(4096, None, W13), C.byref(rows), 16, 4096, 16, 16, 0,
            None, 0, None, None, None)
    refused("dfl_gemm_f32_batch", b"unknown weight format 2", _lib.Weight(4096, None, W13), C.byref(x), 2, 64, 4096, 16, None,
            None)
    refused("dfl_gemm_silu_mul_batch", b"unknown weight format 2", _lib.Weight(4096, None, W13), C.byref(x), 2, 64, 4096, 16,
            0, 16, None, None)
    refused("dfl_gemm_argmax_batch", b"unknown weight format 2", _lib.Weight(4096, None, W13), C.byref(x), 2, 64, 4096, 0,
            16, 16, 0, 16, 16, 16, 0, None, 0, None)
