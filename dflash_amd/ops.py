"""torch-tensor wrappers over the C-ABI (one function per entry point).

torch owns device memory and the stream; these wrappers only validate and pass
raw pointers.  Everything raises on a non-CUDA tensor — there is no host path.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from ._lib import W_BF16, W_BF16X13, W_E4M3, W_MXFP4, Rows, Weight, check, lib

BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64
DYN_S, DYN_TAU, DYN_BS, DYN_POS0, DYN_START, DYN_STOP, DYN_CYCLE = range(7)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor], dtype=None, name="tensor") -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"dflash_amd: {name} must be a GPU tensor (got {t.device}); there is no CPU path")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"dflash_amd: {name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"dflash_amd: {name} must be contiguous")
    return t.data_ptr()


# ---- one-time packing -----------------------------------------------------
def pack_weight(w: torch.Tensor) -> torch.Tensor:
    """[N, K] bf16 row-major -> packed weight (flat bf16 tensor of N*K)."""
    n, k = w.shape
    out = torch.empty(n * k, dtype=BF16, device=w.device)
    check(lib().dfl_pack_weight(_p(w, BF16, "w"), _p(out), n, k, _stream()), "dfl_pack_weight")
    return out


def pack_weight_gateup(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    i, k = gate.shape
    assert up.shape == gate.shape
    out = torch.empty(2 * i * k, dtype=BF16, device=gate.device)
    check(lib().dfl_pack_weight_gateup(_p(gate, BF16, "gate"), _p(up, BF16, "up"), _p(out), i, k, _stream()),
          "dfl_pack_weight_gateup")
    return out


# ---- fp8 (OCP e4m3fn) weights: one byte per weight, one power-of-two scale per output row ----
U8 = torch.uint8
FP8_MAX = 448.0   # largest finite e4m3fn value


class Fp8Weight(NamedTuple):
    """A packed e4m3 weight (pack_weight_fp8 / pack_weight_gateup_fp8) and its fp32 scales in packed tile order.
    gemm_resid / gemm_silu_mul / gemm_argmax take one in place of a packed bf16 weight."""
    wp: torch.Tensor      # uint8 [N * K], layout [N/16][K/64][64 lanes][16 B]
    scale: torch.Tensor   # fp32 [N]
    N: int
    K: int


_fp8_cast_on_device = {}


def fp8_cast_on_device(device) -> bool:
    """Whether this torch build casts fp32 -> float8_e4m3fn on `device` as the host does (probed once per device over
    every rounding boundary of the format: all midpoints between neighbouring codes and the codes themselves)."""
    device = torch.device(device)
    if device.type == "cpu":
        return True
    key = str(device)
    if key not in _fp8_cast_on_device:
        codes = torch.arange(256, dtype=U8)
        v = codes.view(torch.float8_e4m3fn).float()
        v = v[torch.isfinite(v)].sort().values
        probe = torch.cat([v, (v[1:] + v[:-1]) / 2])
        try:
            got = probe.to(device).to(torch.float8_e4m3fn).view(U8).cpu()
            ok = bool(torch.equal(got, probe.to(torch.float8_e4m3fn).view(U8)))
        except (RuntimeError, TypeError, NotImplementedError):
            ok = False
        _fp8_cast_on_device[key] = ok
    return _fp8_cast_on_device[key]


def quantize_fp8_rows(w: torch.Tensor):
    """[N, K] weight -> (q uint8 [N, K] e4m3fn codes, scale fp32 [N]): scale[n] = 2^ceil(log2(amax_n / 448)) (1 for an
    all-zero row), q = round-to-nearest-even of clamp(w / scale, +-448).  w / scale is exact (a power of two), the cast
    never sees a value beyond 448 and so never yields NaN, and q * scale is exactly representable in bf16.
    Runs on w's device; a torch build whose device cast to float8_e4m3fn is missing or differs quantises on the host."""
    assert w.dim() == 2
    dev = w.device
    if not fp8_cast_on_device(dev):
        q, scale = quantize_fp8_rows(w.cpu())
        return q.to(dev), scale.to(dev)
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    m, e = torch.frexp(amax / FP8_MAX)                 # amax / 448 = m * 2^e, m in [0.5, 1)
    e = torch.where(m == 0.5, e - 1, e)                # ceil(log2(.)): an exact power of two is its own ceiling
    scale = torch.ldexp(torch.ones_like(amax), e)
    scale = torch.where(amax / scale > FP8_MAX, scale * 2, scale)   # (a quotient rounded down onto a power of two)
    scale = torch.where(amax == 0, torch.ones_like(scale), scale)
    x = (wf / scale[:, None]).clamp_(-FP8_MAX, FP8_MAX)
    q = x.to(torch.float8_e4m3fn).view(U8)
    return q.contiguous(), scale.contiguous()


def dequantize_fp8_rows(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """q * scale as bf16 [N, K] (exact for quantize_fp8_rows' output)."""
    return (q.view(torch.float8_e4m3fn).float() * scale[:, None].float()).to(BF16)


def pack_weight_fp8(q: torch.Tensor, scale: torch.Tensor) -> Fp8Weight:
    """q uint8 [N, K] e4m3 codes (row-major), scale fp32 [N] -> Fp8Weight.  N % 16 == 0, K % 64 == 0."""
    n, k = q.shape
    assert scale.numel() == n
    out = torch.empty(n * k, dtype=U8, device=q.device)
    check(lib().dfl_pack_weight_fp8(_p(q, U8, "q"), _p(out), n, k, _stream()), "dfl_pack_weight_fp8")
    return Fp8Weight(out, scale.to(device=q.device, dtype=F32).contiguous(), n, k)


def pack_weight_gateup_fp8(gate_q: torch.Tensor, gate_scale: torch.Tensor, up_q: torch.Tensor,
                           up_scale: torch.Tensor) -> Fp8Weight:
    """gate / up codes [I, K] and scales [I] -> one Fp8Weight of 2I rows, tiles (and scales, 16 at a time) interleaved
    (gate tile p, up tile p) as pack_weight_gateup."""
    i, k = gate_q.shape
    assert up_q.shape == gate_q.shape and gate_scale.numel() == i and up_scale.numel() == i
    out = torch.empty(2 * i * k, dtype=U8, device=gate_q.device)
    check(lib().dfl_pack_weight_gateup_fp8(_p(gate_q, U8, "gate_q"), _p(up_q, U8, "up_q"), _p(out), i, k, _stream()),
          "dfl_pack_weight_gateup_fp8")
    sc = torch.stack([gate_scale.to(F32).view(i // 16, 16), up_scale.to(F32).view(i // 16, 16)], dim=1)
    return Fp8Weight(out, sc.reshape(-1).to(gate_q.device).contiguous(), 2 * i, k)


class Fp8Experts(NamedTuple):
    """One MoE layer's expert weights of one kind as e4m3 codes (pack_experts_fp8): expert e's packed codes in row e.
    moe_gate_up / moe_down and moe_grouped_gate_up / moe_grouped_down take one in place of the packed bf16 [E, .] tensor."""
    wp: torch.Tensor      # uint8 [E, N * K]: per expert pack_weight_gateup_fp8's (gate/up, N = 2I) or pack_weight_fp8's layout
    scale: torch.Tensor   # fp32 [E, N], in that layout's tile order
    E: int
    N: int                # output rows per expert: 2 * I (gate/up) or the hidden width (down)
    K: int


def pack_experts_fp8(q: torch.Tensor, scale: torch.Tensor, gateup: bool) -> Fp8Experts:
    """q uint8 [E, N, K] codes and scale fp32 [E, N] (quantize_fp8_rows of the [E * N, K] view) -> Fp8Experts.
    gateup: N = 2I with rows 0 .. I-1 the gate and I .. 2I-1 the up projection (HF's fused gate_up_proj), packed with
    their tiles interleaved; else a plain [N, K] weight per expert (down_proj).  One expert at a time, as the bf16 path."""
    e, n, k = q.shape
    assert scale.shape == (e, n) and q.dtype == U8
    wp = torch.empty(e, n * k, dtype=U8, device=q.device)
    sc = torch.empty(e, n, dtype=F32, device=q.device)
    for j in range(e):
        if gateup:
            i = n // 2
            w8 = pack_weight_gateup_fp8(q[j, :i].contiguous(), scale[j, :i], q[j, i:].contiguous(), scale[j, i:])
        else:
            w8 = pack_weight_fp8(q[j].contiguous(), scale[j])
        wp[j].copy_(w8.wp)
        sc[j].copy_(w8.scale)
    return Fp8Experts(wp, sc, e, n, k)


def quantize_keep_fp8(m: torch.Tensor):
    """The load step of an fp8 model for one Linear weight [N, K]: (q * scale as bf16 — what the bf16 kernels and the
    rest of the model compute with —, (q, scale) for pack_weight_fp8 / pack_layer_fp8)."""
    q, sc = quantize_fp8_rows(m)
    return dequantize_fp8_rows(q, sc), (q, sc)


def pack_layer_fp8(l8: dict) -> dict:
    """A dense layer's (codes, scales) by projection — q, k, v, o, gate, up, down — -> its four Fp8Weights, laid out as
    the layer's packed bf16 weights are: q/k/v as one matrix, gate/up interleaved."""
    return {"qkv": pack_weight_fp8(torch.cat([l8[k][0] for k in "qkv"]), torch.cat([l8[k][1] for k in "qkv"])),
            "o": pack_weight_fp8(*l8["o"]), "gu": pack_weight_gateup_fp8(*l8["gate"], *l8["up"]),
            "down": pack_weight_fp8(*l8["down"])}


def tile_layers(layers: list, layers8: list, qkv_parts: bool, cache: dict) -> list:
    """The layer dicts TileStack.run takes where it streams e4m3 codes: `layers` with gu / o / down — and qkv, where the
    caller runs qkv="parts" — replaced by their twins in layers8.  Built once per form and kept in `cache`."""
    if qkv_parts not in cache:
        keys = ("gu", "o", "down") + (("qkv",) if qkv_parts else ())
        cache[qkv_parts] = [{**lw, **{k: l8[k] for k in keys}} for lw, l8 in zip(layers, layers8)]
    return cache[qkv_parts]


def row_layers(layers: list, layers8, gu13: list, fp8: bool, cache: dict, down13=None) -> list:
    """The layer dicts RowStack.run takes — the one format choice of the single-request path.  fp8: `layers` with qkv / o /
    gu / down replaced by their quantised twins in layers8 (an fp8 model's e4m3 codes, an mxfp4 model's 4-bit ones); else with gu / down replaced by their 13-bit twins where gu13[i] /
    down13[i] is not None (a layer with neither, an MoE layer among them, passes through as it is).  Built once per form
    and kept in `cache`."""
    if fp8 not in cache:
        if fp8:
            cache[fp8] = [{**lw, **{k: l8[k] for k in ("qkv", "o", "gu", "down")}} for lw, l8 in zip(layers, layers8)]
        else:
            twins = [{k: v for k, v in (("gu", g), ("down", d)) if v is not None}
                     for g, d in zip(gu13, down13 or [None] * len(layers))]
            cache[fp8] = [{**lw, **tw} if tw else lw for lw, tw in zip(layers, twins)]
    return cache[fp8]


# ---- bf16x13: the packed bf16 weight in 13 bits per element, losslessly ----
X13_QUAD_BYTES = 3328   # four k-steps of one 16-column tile: L0, L1, NB (1024 B each) and SG (256 B); csrc/gemm_rows.h
STREAM_FORMATS = ("auto", "bf16")
# Which matrix kinds stream_format="auto" packs: each kept only where its slowest repeat beat the plain form's fastest
# (profiles/bf16x13_ab.txt, part 1); "experts_gateup" — an MoE layer's experts as one tall matrix, dfl_moe_gate_up — by
# the same rule at 46 AND at 80 active experts (profiles/bf16x13_experts_ab.txt, part 1: 40.6 < 45.6 us, 63.5 < 74.9 us);
# "down" and "fc" — the K-chunked form of gemm_resid, K a multiple of 2048 above 4096 — by profiles/bf16x13_down_ab.txt,
# part 1: down kept at 4096 x 12288, 4096 x 14336 and 2048 x 6144; fc (4096 x 20480: 0.99 x, the spreads overlap) NOT kept
X13_KINDS = {"gateup": True, "lm_head": True, "experts_gateup": True, "down": True, "fc": False}


class Bf16x13Weight(NamedTuple):
    """A packed bf16 weight re-coded by pack_weight_bf16x13: gemm_silu_mul / gemm_argmax (K = 2048 or 4096), gemm_resid
    (K a multiple of 2048 above 4096) — and moe_gate_up, for an MoE layer's experts as one tall matrix — take one in
    place of the packed bf16 tensor and compute the same bits from 13/16 of the bytes."""
    data: torch.Tensor    # uint8: [N/16][K/128] quads of X13_QUAD_BYTES, then int32 [N/16][items per tile][2] {base, patch}
    N: int
    K: int


def bf16x13_covers(N: int, K: int) -> bool:
    """The layout holds whole quads of four k-steps per wave: 16 waves x 4 or x 8 k-steps in one pass, or — the K-chunked
    form of gemm_resid — whole chunks of 16 waves x 4 k-steps above that."""
    return N > 0 and N % 16 == 0 and (K in (2048, 4096) or (K > 4096 and K % 2048 == 0))


def pack_weight_bf16x13(wp: torch.Tensor, N: int, K: int, tiles_per_pass: int = 256):
    """wp: the packed bf16 weight of N x K (pack_weight, or pack_weight_gateup with N = 2I: its tiles are already
    interleaved, and every packed tile — a gate tile, an up tile — gets a base of its own).
    Returns (Bf16x13Weight or None, report).  Per packed tile hb = max(0, max(H & 0x7f) - 15) with H the bf16's high
    byte; an element keeps its low byte, its sign and a code c (0: H & 0x7f == 0; 1..15: H & 0x7f == hb + c).  A nonzero
    element below the window (H & 0x7f in 1..hb) is an exception: ONE per item is carried exactly in that item's patch
    word; a second one refuses the matrix (None: the caller keeps plain bf16).  An item is what one wave holds in flight
    at a time: (tile, wave) — K / 16 elements per column — at K <= 4096, and (tile, chunk, wave) — one quad — in the
    K-chunked form above that; its meta pair is pair (tile * nch + chunk) * 16 + wave, nch = K / 2048 chunks (1 at
    K <= 4096).  report = {"items": items, "patched": items with a patch word, "refused": items with two or more
    exceptions}.
    Plain tensor ops on wp's device (CPU included), `tiles_per_pass` tiles at a time; runs once at load."""
    if not bf16x13_covers(N, K):
        raise ValueError(f"dflash_amd: bf16x13 covers K = 2048, 4096 or a multiple of 2048 above, and N % 16 == 0 (N={N} K={K})")
    if wp.dtype != BF16 or wp.numel() != N * K:
        raise ValueError("dflash_amd: pack_weight_bf16x13 takes the packed bf16 weight of N * K elements")
    nt, KS, dev = N // 16, K // 32, wp.device
    Q = KS // 4
    nit, isz = (16, KS // 16 * 512) if K <= 4096 else (Q, 4 * 512)   # items per tile, elements per item
    src = wp.view(torch.int16).view(nt, KS, 64, 8)
    qbytes = nt * Q * X13_QUAD_BYTES
    data = torch.empty(qbytes + nt * nit * 8, dtype=U8, device=dev)
    quads, meta = data[:qbytes].view(nt, Q, X13_QUAD_BYTES), data[qbytes:].view(I32).view(nt, nit, 2)
    rsh = torch.arange(8, dtype=I32, device=dev).view(1, 1, 4, 1, 2, 1)   # r = 2 f + g
    patched = refused = 0
    for t0 in range(0, nt, tiles_per_pass):
        wi = src[t0:t0 + tiles_per_pass].to(I32) & 0xffff
        T = wi.shape[0]
        lo, h7, sign = (wi & 0xff).to(U8), (wi >> 8) & 0x7f, wi >> 15
        hb = (h7.amax(dim=(1, 2, 3)) - 15).clamp_(min=0)
        c = h7 - hb.view(T, 1, 1, 1)
        exc = (h7 != 0) & (c < 1)
        c = torch.where(c < 1, torch.zeros_like(c), c)             # (h7 == 0 lies below hb + 1 as well)
        # exceptions per item: item i of a tile owns its k-steps i * isz / 512 ..
        ex = exc.view(T, nit, isz)
        cnt = ex.sum(dim=2)
        refused += int((cnt > 1).sum())
        patched += int((cnt == 1).sum())
        idx = ex.to(I32).argmax(dim=2)                             # (the first one: the only one where cnt == 1)
        raw = wi.view(T, nit, isz).gather(2, idx.unsqueeze(2)).squeeze(2)
        word = ((8 + idx // 512) << 28) | (((idx // 8) % 64) << 22) | ((idx % 8) << 19) | raw      # int64
        word = torch.where(cnt == 1, word - (1 << 32), torch.zeros_like(word)).to(I32)             # bit 31: the sign
        meta[t0:t0 + T, :, 0] = hb.to(I32).view(T, 1)
        meta[t0:t0 + T, :, 1] = word
        lq = lo.view(T, Q, 4, 64, 8)
        cq = c.view(T, Q, 4, 64, 8)
        nb = (cq[..., :4] | (cq[..., 4:] << 4)).to(U8)              # byte b = c[b] | c[b + 4] << 4
        sg = (sign.view(T, Q, 4, 64, 2, 4) << rsh).sum(dim=(2, 4)).to(U8)   # [T, Q, 64, 4]: bit r of byte b
        out = quads[t0:t0 + T]
        out[:, :, 0:1024] = lq[:, :, 0:2].permute(0, 1, 3, 2, 4).reshape(T, Q, 1024)
        out[:, :, 1024:2048] = lq[:, :, 2:4].permute(0, 1, 3, 2, 4).reshape(T, Q, 1024)
        out[:, :, 2048:3072] = nb.permute(0, 1, 3, 2, 4).reshape(T, Q, 1024)
        out[:, :, 3072:3328] = sg.reshape(T, Q, 256)
    report = {"items": nt * nit, "patched": patched, "refused": refused}
    if refused:
        return None, report
    return Bf16x13Weight(data, N, K), report


_x13_twins = {}   # data_ptr of a packed bf16 tensor -> (weak reference to it, N, K, its Bf16x13Weight or None, report)


def bf16x13_twin(wp: torch.Tensor, N: int, K: int, kind: str):
    """The 13-bit twin stream_format="auto" streams in place of the packed bf16 tensor `wp`, or None where plain bf16
    stays: a kind the measurement did not keep (X13_KINDS), a shape the layout does not cover, a matrix the packer refused.
    Packed once per tensor — draft and target share one lm_head twin as they share the packed head — and kept while the
    tensor lives."""
    import weakref
    if not X13_KINDS[kind] or not bf16x13_covers(N, K):
        return None
    if kind in ("down", "fc") and K <= 4096:   # gemm_resid takes the K-chunked form only (dfl_gemm_resid)
        return None
    key = wp.data_ptr()
    hit = _x13_twins.get(key)
    if hit is None or hit[0]() is not wp or hit[1:3] != (N, K):
        for k in [k for k, v in _x13_twins.items() if v[0]() is None]:
            del _x13_twins[k]
        twin, report = pack_weight_bf16x13(wp, N, K)
        hit = _x13_twins[key] = (weakref.ref(wp), N, K, twin, report)
    return hit[3]


def bf16x13_report() -> dict:
    """What the live twins came to: matrices packed, matrices kept as plain bf16 because the packer refused them, and the
    patched / refused (tile, wave) items over all of them."""
    live = [v for v in _x13_twins.values() if v[0]() is not None]
    return {"packed": sum(v[3] is not None for v in live), "kept_bf16": sum(v[3] is None for v in live),
            "patched_items": sum(v[4]["patched"] for v in live), "refused_items": sum(v[4]["refused"] for v in live)}


# ---- mxfp4: OCP Microscaling e2m1 codes with one e8m0 scale per 32 consecutive k of a row ----
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)   # magnitudes of codes 0..7; bit 3 of a code is the sign
MX_BLOCK = 32
MX_EXP_MIN, MX_EXP_MAX = -120, 120     # scale codes 7..247 (code = exponent + 127)


class Mxfp4Weight(NamedTuple):
    """A packed MXFP4 weight (pack_weight_mxfp4 / pack_weight_gateup_mxfp4): gemm_resid / gemm_silu_mul / gemm_argmax
    take one in place of a packed bf16 weight (K % 128 == 0)."""
    data: torch.Tensor    # uint8: codes [N/16][K/128][64 lanes][16 B], then e8m0 scales [N/16][K/128][16 columns][4 B]
    N: int
    K: int


def quantize_mxfp4_rows(w: torch.Tensor):
    """[N, K] weight (K % 32 == 0) -> (codes uint8 [N, K/2], scale_codes uint8 [N, K/32]).  Per block of 32 consecutive k
    of a row: scale = 2^e, e = ceil(log2(amax / 6)) clamped to [-120, 120] (0 for an all-zero block), scale code e + 127;
    q = round-to-nearest-even of w / scale onto the e2m1 grid {0, .5, 1, 1.5, 2, 3, 4, 6} with sign (a value that rounds to
    zero is stored as +0).  The ceil rule keeps amax / scale <= 6: nothing is clamped at +-6 except by the exponent clamp.
    Element 2 i of a row is the LOW nibble of byte i.  Thresholds, no cast to a torch fp4 type; runs on w's device."""
    if w.dim() != 2 or w.shape[1] % MX_BLOCK:
        raise ValueError(f"dflash_amd: quantize_mxfp4_rows takes [N, K] with K % {MX_BLOCK} == 0, got {tuple(w.shape)}")
    wf = w.detach().float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("dflash_amd: quantize_mxfp4_rows: the weight holds a non-finite value")
    n, k = wf.shape
    blk = wf.view(n, k // MX_BLOCK, MX_BLOCK)
    amax = blk.abs().amax(dim=2)
    # amax = m * 2^ea with m in [0.5, 1): 6 * 2^e >= amax  <=>  2^(e - ea) >= m / 6, and m / 6 <= 1/8 exactly when m <= 0.75
    m, ea = torch.frexp(amax)
    e = torch.where(m <= 0.75, ea - 3, ea - 2)
    e = torch.where(amax == 0, torch.zeros_like(e), e).clamp_(MX_EXP_MIN, MX_EXP_MAX)
    a = torch.ldexp(blk.abs(), -e.unsqueeze(2))        # |w| / scale, exact (a power of two)
    # round to nearest, ties to the even code: midpoints .25 .75 1.25 1.75 2.5 3.5 5 between codes 0..7
    mag = ((a > 0.25).to(U8) + (a >= 0.75).to(U8) + (a > 1.25).to(U8) + (a >= 1.75).to(U8) + (a > 2.5).to(U8)
           + (a >= 3.5).to(U8) + (a > 5.0).to(U8))
    code = torch.where((blk < 0) & (mag != 0), mag | 8, mag).view(n, k // 2, 2)
    codes = (code[..., 0] | (code[..., 1] << 4)).contiguous()
    return codes, (e + 127).to(U8).contiguous()


def dequantize_mxfp4_rows(codes: torch.Tensor, scale_codes: torch.Tensor) -> torch.Tensor:
    """e2m1 value * 2^(scale code - 127) as bf16 [N, K]: exact (at most two significant bits, exponents -121 .. 122)."""
    n, k2 = codes.shape
    c = torch.stack([codes & 15, codes >> 4], dim=2).view(n, 2 * k2).long()
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=F32, device=codes.device)
    e = (scale_codes.to(I32) - 127).repeat_interleave(MX_BLOCK, dim=1)
    return torch.ldexp(lut[c], e).to(BF16)


def _mxfp4_check(codes, scale_codes):
    n, k = codes.shape[0], codes.shape[1] * 2
    if codes.dtype != U8 or scale_codes.dtype != U8 or tuple(scale_codes.shape) != (n, k // MX_BLOCK) or n % 16 or k % 128:
        raise ValueError(f"dflash_amd: mxfp4 codes uint8 [N, K/2] and scale codes uint8 [N, K/32] with N % 16 == 0 and "
                         f"K % 128 == 0 (got {tuple(codes.shape)}, {tuple(scale_codes.shape)})")
    return n, k


def pack_weight_mxfp4(codes: torch.Tensor, scale_codes: torch.Tensor) -> Mxfp4Weight:
    """quantize_mxfp4_rows' output for an [N, K] weight -> Mxfp4Weight in the DFL_W_MXFP4 layout (include/dflash_hip.h):
    a byte permutation, tensor ops on the codes' device.  N % 16 == 0, K % 128 == 0; N * K / 2 + N * K / 32 bytes."""
    n, k = _mxfp4_check(codes, scale_codes)
    # row byte 64 j + 16 d + 4 kq + b holds k = 128 j + 32 d + 8 kq + 2 b ..: [t][column][j][d][kq][b] -> [t][j][kq][column][d][b]
    cp = codes.view(n // 16, 16, k // 128, 4, 4, 4).permute(0, 2, 4, 1, 3, 5).reshape(-1)
    sp = scale_codes.view(n // 16, 16, k // 128, 4).permute(0, 2, 1, 3).reshape(-1)    # [t][j][column][d]
    return Mxfp4Weight(torch.cat([cp, sp]).contiguous(), n, k)


def pack_weight_gateup_mxfp4(gate_codes: torch.Tensor, gate_scales: torch.Tensor, up_codes: torch.Tensor,
                             up_scales: torch.Tensor) -> Mxfp4Weight:
    """gate / up codes [I, K/2] and scale codes [I, K/32] -> one Mxfp4Weight of 2I rows, tiles interleaved (gate tile p, up
    tile p) as pack_weight_gateup, codes and scales alike."""
    i, k = _mxfp4_check(gate_codes, gate_scales)
    if (i, k) != _mxfp4_check(up_codes, up_scales):
        raise ValueError("dflash_amd: gate and up must have one shape")

    def weave(g, u):
        return torch.stack([g.view(i // 16, 16, -1), u.view(i // 16, 16, -1)], dim=1).reshape(2 * i, -1)

    return pack_weight_mxfp4(weave(gate_codes, up_codes), weave(gate_scales, up_scales))


def quantize_keep_mxfp4(m: torch.Tensor):
    """The load step of an mxfp4 model for one Linear weight [N, K]: (the dequantised values as bf16 — what every path
    without a 4-bit kernel computes with —, (codes, scale codes) for pack_weight_mxfp4 / pack_layer_mxfp4)."""
    q = quantize_mxfp4_rows(m)
    return dequantize_mxfp4_rows(*q), q


def pack_layer_mxfp4(l4: dict) -> dict:
    """A dense layer's (codes, scale codes) by projection — q, k, v, o, gate, up, down — -> its four Mxfp4Weights, laid
    out as the layer's packed bf16 weights are: q/k/v as one matrix, gate/up interleaved."""
    return {"qkv": pack_weight_mxfp4(torch.cat([l4[k][0] for k in "qkv"]), torch.cat([l4[k][1] for k in "qkv"])),
            "o": pack_weight_mxfp4(*l4["o"]), "gu": pack_weight_gateup_mxfp4(*l4["gate"], *l4["up"]),
            "down": pack_weight_mxfp4(*l4["down"])}


def check_stream_format(stream_format: str) -> bool:
    """True for "auto" (the 13-bit twins where they apply), False for "bf16"."""
    if stream_format not in STREAM_FORMATS:
        raise ValueError(f"stream_format must be one of {STREAM_FORMATS}, got {stream_format!r}")
    return stream_format == "auto"


def _w(wp, N: int, K: int, name: str) -> Weight:
    """The dfl_weight of a launch: a packed bf16 tensor, or an Fp8Weight / a Bf16x13Weight / an Mxfp4Weight of the launch's
    N x K (the C side refuses a format the entry point does not take).  Read
    on the host during the call only; the caller's references keep the tensors alive."""
    if isinstance(wp, Bf16x13Weight):
        if (wp.N, wp.K) != (N, K):
            raise ValueError(f"dflash_amd: {name} is a bf16x13 weight of {wp.N} x {wp.K}, the launch asks for {N} x {K}")
        return Weight(_p(wp.data, U8, name), None, W_BF16X13)
    if isinstance(wp, Mxfp4Weight):
        if (wp.N, wp.K) != (N, K):
            raise ValueError(f"dflash_amd: {name} is an mxfp4 weight of {wp.N} x {wp.K}, the launch asks for {N} x {K}")
        return Weight(_p(wp.data, U8, name), None, W_MXFP4)
    if not isinstance(wp, Fp8Weight):
        return Weight(_p(wp, BF16, name), None, W_BF16)
    if (wp.N, wp.K) != (N, K):
        raise ValueError(f"dflash_amd: {name} is an fp8 weight of {wp.N} x {wp.K}, the launch asks for {N} x {K}")
    return Weight(_p(wp.wp, U8, name), _p(wp.scale, F32, name + ".scale"), W_E4M3)


def _we(wp, E: int, N: int, K: int, name: str):
    """_w for one MoE layer's experts: packed bf16 [E, .] or an Fp8Experts of E x N x K.  Returns the descriptor and the
    tensor whose rows are the experts (its stride(0): bf16 elements, or bytes of codes, between them)."""
    if not isinstance(wp, Fp8Experts):
        assert wp.dim() == 2 and wp.is_contiguous()
        return Weight(_p(wp, BF16, name), None, W_BF16), wp
    if (wp.E, wp.N, wp.K) != (E, N, K):
        raise ValueError(f"dflash_amd: {name} holds fp8 experts of {wp.E} x {wp.N} x {wp.K}, the launch asks for "
                         f"{E} x {N} x {K}")
    return Weight(_p(wp.wp, U8, name), _p(wp.scale, F32, name + ".scale"), W_E4M3), wp.wp


# ---- per-cycle ------------------------------------------------------------------
def set_dyn(dyn: torch.Tensor, S: int, tau: int, bs: int, pos0: int) -> None:
    check(lib().dfl_set_dyn(_p(dyn, I32, "dyn"), S, tau, bs, pos0, _stream()), "dfl_set_dyn")


def set_dyn2(dyn: torch.Tensor, S: int, tau: int, bs: int, pos0: int) -> None:
    """dyn int32 [>= 16]: one record per 16-row tile of a block of up to 32 rows."""
    assert dyn.numel() >= 16
    check(lib().dfl_set_dyn2(_p(dyn, I32, "dyn"), S, tau, bs, pos0, _stream()), "dfl_set_dyn2")


def pack_rows(x: torch.Tensor, rows: int, out_frag: torch.Tensor, dyn=None, dyn_word=0) -> None:
    """x: [rows(+), K] bf16 with unit inner stride -> frag16 (out_frag has 16*K elements)."""
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == BF16 and x.is_cuda
    k = x.shape[1]
    assert out_frag.numel() >= 16 * k
    check(lib().dfl_pack_rows(x.data_ptr(), x.stride(0), rows, k, _p(out_frag, BF16, "out_frag"),
                              _p(dyn, I32, "dyn"), dyn_word, _stream()), "dfl_pack_rows")


# ---- row sources (dfl_rows): where a GEMM's 16-row activation tile comes from ---------
import ctypes as _C


class RowSource:
    """Keeps the ctypes struct and the tensors it points into alive together."""

    def __init__(self, struct: Rows, *keep):
        self.struct, self.keep = struct, keep

    @property
    def ref(self):
        return _C.byref(self.struct)


def rows_frag(frag: torch.Tensor) -> RowSource:
    """frag16 fragments written by a producer kernel."""
    return RowSource(Rows(_p(frag, BF16, "frag"), None, 0, None, 0, None, 0.0, -1, 0), frag)


def _readable16(rows: torch.Tensor) -> torch.Tensor:
    """The kernels load all 16 rows of a tile before they know how many are valid (the lengths
    arrive by a scalar load they do not wait for): the storage behind `rows` must cover 16
    rows.  A view of a 16-row buffer does; a shorter tensor is copied into a padded one."""
    need = (15 * rows.stride(0) + rows.shape[1]) * rows.element_size()
    have = rows.untyped_storage().nbytes() - rows.storage_offset() * rows.element_size()
    if rows.shape[0] >= 16 or have >= need:
        return rows
    pad = torch.zeros(16, rows.shape[1], dtype=rows.dtype, device=rows.device)
    pad[:rows.shape[0]] = rows
    return pad


def rows_plain(rows: torch.Tensor, valid_word: int = -1) -> RowSource:
    """bf16 rows [<=16, K] (unit inner stride); rows >= dyn[valid_word] count as zero."""
    assert rows.is_cuda and rows.dtype == BF16 and rows.dim() == 2 and rows.stride(1) == 1
    rows = _readable16(rows)
    return RowSource(Rows(None, rows.data_ptr(), rows.stride(0), None, 0, None, 0.0, valid_word, 1), rows)


def rows_normed(rows: torch.Tensor, ss: torch.Tensor, nss: int, norm_w: torch.Tensor, eps: float,
                valid_word: int = -1) -> RowSource:
    """the residual stream + partial sums of squares: the GEMM applies the RMSNorm itself."""
    assert rows.is_cuda and rows.dtype == BF16 and rows.dim() == 2 and rows.stride(1) == 1
    assert ss.numel() >= nss * 16
    rows = _readable16(rows)
    return RowSource(Rows(None, rows.data_ptr(), rows.stride(0), _p(ss, F32, "ss"), nss, _p(norm_w, BF16, "norm_w"),
                          eps, valid_word, 2), rows, ss, norm_w)


def _src(x) -> RowSource:
    return x if isinstance(x, RowSource) else rows_frag(x)


def gemm_f32(wp, x0, x1, mt: int, N: int, K: int, ksplit: int, out: torch.Tensor, dyn=None) -> None:
    """x0/x1: RowSource, or a frag16 tensor."""
    assert out.numel() >= ksplit * mt * 16 * N
    s0, s1 = _src(x0), (_src(x1) if x1 is not None else None)
    check(lib().dfl_gemm_f32(_p(wp, BF16, "wp"), s0.ref, s1.ref if s1 is not None else None, mt, N, K, ksplit,
                             _p(out, F32, "out"), _p(dyn, I32, "dyn"), _stream()), "dfl_gemm_f32")


def min_ksplit(K: int, mt: int) -> int:
    per = 16 * (8 if mt == 1 else 4) * 32
    return (K + per - 1) // per


def pick_ksplit(N: int, K: int, mt: int) -> int:
    """K split for dfl_gemm_f32 that fills the 256 CUs evenly: work units = column tiles x
    K chunks, dealt to <= 256 workgroups of equal load, preferring >= 2 tiles per workgroup
    (the next tile's weights are prefetched under the current one).  Measured on MI355X
    (scripts/bench_gemm.py): every shape runs ~3.6 us + bytes / 6.5 TB/s for any split
    near this choice, so the picker only has to avoid the unbalanced ones."""
    ntiles, ks_steps = N // 16, K // 32
    best, best_score = None, None
    for ks in range(min_ksplit(K, mt), 17):
        nfr = -(-ks_steps // (16 * ks))
        if nfr < 2 and ks > min_ksplit(K, mt):
            break
        gx_max = max(1, 256 // ks)
        per_wg = -(-ntiles // gx_max)
        fill = (ntiles * ks) / (256.0 * per_wg)           # busy fraction of the chip over the launch
        score = (round(min(fill, 1.0), 3), min(per_wg, 2), -ks)
        if best_score is None or score > best_score:
            best, best_score = ks, score
    return best


def gemm_silu_mul(wp_gu, x, I: int, K: int, act_frag: torch.Tensor, dyn=None) -> None:
    assert act_frag.numel() >= 16 * I
    check(lib().dfl_gemm_silu_mul(_w(wp_gu, 2 * I, K, "wp_gu"), _src(x).ref, I, K, _p(act_frag, BF16, "act"),
                                  _p(dyn, I32, "dyn"), _stream()), "dfl_gemm_silu_mul")


def argmax_ws(device) -> torch.Tensor:
    return torch.empty(lib().dfl_argmax_ws_bytes(), dtype=torch.uint8, device=device)


def gemm_argmax(wp, x, V: int, K: int, row0: int, nrows: int, ws, out_ids: torch.Tensor, out_off: int = 0,
                dyn=None, nrows_dyn_word: int = -1, logits: Optional[torch.Tensor] = None,
                margins: Optional[torch.Tensor] = None, events=None) -> None:
    """margins: optional fp32 tensor indexed like out_ids: top-1 minus top-2 logit per row.
    events: (start, end) torch.cuda.Event pair (enable_timing, already recorded once so that their handles exist),
    recorded right around the GEMM launch itself."""
    if logits is not None:
        assert logits.numel() >= 16 * V
    if margins is not None:
        assert margins.numel() >= out_off + nrows
    ev_start, ev_end = (None, None) if events is None else (events[0].cuda_event, events[1].cuda_event)
    check(lib().dfl_gemm_argmax(_w(wp, V, K, "wp"), _src(x).ref, V, K, row0, nrows, _p(dyn, I32, "dyn"), nrows_dyn_word,
                                _p(ws), _p(out_ids, I64, "out_ids"), out_off, _p(logits, BF16, "logits"),
                                _p(margins, F32, "margins"), ev_start, ev_end, _stream()), "dfl_gemm_argmax")


RNG_TARGET, RNG_DRAFT = 0, 1   # noise streams of the seeded sampler (csrc/dfl_rng.h)


def _seed64(seed: int) -> int:
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def inv_temperature(temperature: float) -> float:
    """float32(1 / T), computed on the host (the sampling contract)."""
    import numpy as np
    return float(np.float32(1.0 / float(temperature)))


def gemm_sample(wp, x, V: int, K: int, row0: int, nrows: int, ws, out_ids: torch.Tensor, out_off: int = 0, *,
                seed: int, temperature: float, stream: int = RNG_TARGET, pos_dyn=None, pos_word: int = DYN_POS0,
                pos_base: int = 0, pos_add: int = 0, dyn=None, nrows_dyn_word: int = -1,
                logits: Optional[torch.Tensor] = None, margins: Optional[torch.Tensor] = None) -> None:
    """gemm_argmax with the seeded Gumbel-max draw at `temperature` (dfl_gemm_sample): tile row m draws position
    (pos_dyn[pos_word] if pos_dyn is given, else pos_base) + pos_add + m.  wp: packed bf16, or an Fp8Weight
    (the draw over bf16(sum * scale))."""
    if logits is not None:
        assert logits.numel() >= 16 * V
    if margins is not None:
        assert margins.numel() >= out_off + nrows
    check(lib().dfl_gemm_sample(_w(wp, V, K, "wp"), _src(x).ref, V, K, row0, nrows, _p(dyn, I32, "dyn"), nrows_dyn_word,
                                _p(ws), _p(out_ids, I64, "out_ids"), out_off, _p(logits, BF16, "logits"),
                                _p(margins, F32, "margins"), _seed64(seed), inv_temperature(temperature), stream,
                                _p(pos_dyn, I32, "pos_dyn"), pos_word, pos_base, pos_add, _stream()), "dfl_gemm_sample")


def sample_rows(logits: torch.Tensor, *, seed: int, temperature: float, pos0: int = 0, positions=None,
                stream: int = RNG_TARGET, extra: int = 0, out: Optional[torch.Tensor] = None,
                margins: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The seeded draw over materialised bf16 logits [rows, V] (unit inner stride): row r draws position positions[r]
    (int32) or pos0 + r.  Returns int64 ids [rows] (into `out` if given)."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and logits.is_cuda
    if logits.dtype != BF16:
        logits = logits.to(BF16)
    rows, V = logits.shape
    if out is None:
        out = torch.empty(rows, dtype=I64, device=logits.device)
    check(lib().dfl_sample_rows(logits.data_ptr(), logits.stride(0), rows, V, _seed64(seed), inv_temperature(temperature),
                                stream, pos0, _p(positions, I32, "positions"), extra, _p(out, I64, "out"),
                                _p(margins, F32, "margins"), _stream()), "dfl_sample_rows")
    return out


def check_filter(top_k, top_p) -> bool:
    """Validate one request's (top_k, top_p); True if either filter is on (top_k = 0 and top_p = 1.0 are "off")."""
    if int(top_k) != top_k or int(top_k) < 0:
        raise ValueError(f"dflash_amd: top_k must be an integer >= 0 (0 = off), got {top_k!r}")
    if not (0.0 < float(top_p) <= 1.0):
        raise ValueError(f"dflash_amd: top_p must be inside (0, 1] (1.0 = off), got {top_p!r}")
    return int(top_k) > 0 or float(top_p) < 1.0


def sample_rows_nucleus(logits: torch.Tensor, *, temperature: Optional[float] = None, top_k=0, top_p=1.0, seed=0, row0: int = 0,
                        nrows: Optional[int] = None, dyn=None, nrows_dyn_word: int = -1, pos_word: int = -1,
                        pos_base: int = 0, positions=None, pos_add: int = 0, tiles_per_req: int = 1,
                        stream: int = RNG_TARGET, extra: int = 0, out: Optional[torch.Tensor] = None, out_off: int = 0,
                        thresholds: Optional[torch.Tensor] = None, kept: Optional[torch.Tensor] = None,
                        inv_t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The seeded draw under top-k / top-p (dfl_sample_rows_nucleus) over materialised bf16 logits
    [rows <= 16, V] (one tile) or [tiles, 16, V], unit inner stride.
    inv_t: a device fp32 tensor of invT per request slot (`temperature` is then unused, pass None): a slot whose value is
    not > 0 is greedy, its rows of out / thresholds / kept are not written.
    seed / top_k / top_p: a host value, or a device tensor (int64 / int32 / fp32) indexed by request slot
    q = tile // tiles_per_req.  Tile t row m draws position positions[16 t + m] (int32 tensor), or
    (dyn[t][pos_word] if pos_word >= 0 else pos_base) + pos_add + 16 (t % tiles_per_req) + m.  Rows of a tile:
    row0 .. dyn[t][nrows_dyn_word] if nrows_dyn_word >= 0, else row0 .. row0 + nrows.
    Returns int64 ids (`out` if given: [tiles, n] or, for one tile, [n]) at out[t, out_off + m - row0]; `thresholds`
    (fp32) and `kept` (int32), shaped and indexed like out, receive the final threshold and the kept-set size."""
    assert logits.dim() in (2, 3) and logits.stride(-1) == 1 and logits.is_cuda
    if logits.dtype != BF16:
        logits = logits.to(BF16)
    if logits.dim() == 2:
        assert logits.shape[0] <= 16, "one tile holds at most 16 rows"
        tiles, tile_rows, tile_stride = 1, logits.shape[0], 16 * logits.stride(0)
    else:
        assert logits.shape[1] == 16
        tiles, tile_rows, tile_stride = logits.shape[0], 16, logits.stride(0)
    V, ld = logits.shape[-1], logits.stride(-2)
    if nrows is None:
        nrows = tile_rows - row0
    assert 0 <= row0 and row0 + nrows <= tile_rows or nrows_dyn_word >= 0 and tile_rows == 16
    n_out = 16 - row0 if nrows_dyn_word >= 0 else nrows
    if out is None:
        out = torch.empty((tiles, out_off + n_out) if logits.dim() == 3 else (out_off + n_out,), dtype=I64,
                          device=logits.device)
    out_stride = out.stride(0) if out.dim() == 2 else 0
    for o, nm in ((out, "out"), (thresholds, "thresholds"), (kept, "kept")):
        if o is not None:
            assert o.dim() == out.dim() and o.stride(-1) == 1 and (o.dim() == 1 or o.stride(0) == out_stride), nm
            assert o.shape[-1] >= out_off + n_out and (o.dim() == 1 and tiles == 1 or o.shape[0] >= tiles), nm
    if positions is not None:
        assert positions.numel() >= 16 * (tiles - 1) + row0 + n_out
    if dyn is not None:
        assert dyn.numel() >= 8 * tiles
    slots = (tiles + tiles_per_req - 1) // tiles_per_req

    def dev_or_host(v, dtype, name, host):
        if torch.is_tensor(v):
            assert v.numel() >= slots, name
            return _p(v, dtype, name), host(0)
        return None, host(v)

    if not torch.is_tensor(top_k) or not torch.is_tensor(top_p):
        check_filter(0 if torch.is_tensor(top_k) else top_k, 1.0 if torch.is_tensor(top_p) else top_p)
    seeds_p, seed_v = dev_or_host(seed, I64, "seed", _seed64)
    k_p, k_v = dev_or_host(top_k, I32, "top_k", int)
    p_p, p_v = dev_or_host(top_p, F32, "top_p", float)
    if p_p is not None:
        p_v = 1.0
    if (temperature is None) == (inv_t is None):
        raise ValueError("sample_rows_nucleus: give either temperature or inv_t")
    if inv_t is not None:
        assert inv_t.numel() >= slots, "inv_t"
    check(lib().dfl_sample_rows_nucleus(logits.data_ptr(), ld, tile_stride, tiles, V, row0, nrows, _p(dyn, I32, "dyn"),
                                        nrows_dyn_word, pos_word, pos_base, _p(positions, I32, "positions"), pos_add,
                                        tiles_per_req, seeds_p, seed_v, k_p, k_v, p_p, p_v, _p(inv_t, F32, "inv_t"),
                                        0.0 if inv_t is not None else inv_temperature(temperature), stream, extra,
                                        _p(out, I64, "out"), out_stride, out_off, _p(thresholds, F32, "thresholds"),
                                        _p(kept, I32, "kept"), _stream()), "dfl_sample_rows_nucleus")
    return out


MAX_TOP_LOGPROBS = 8


def check_logprobs(logprobs) -> Optional[int]:
    """Validate a `logprobs` keyword: None (off), 0 (the chosen token only) or 1..8 (that many alternatives too)."""
    if logprobs is None:
        return None
    if isinstance(logprobs, bool) or int(logprobs) != logprobs or not 0 <= int(logprobs) <= MAX_TOP_LOGPROBS:
        raise ValueError(f"dflash_amd: logprobs must be None or an integer 0..{MAX_TOP_LOGPROBS}, got {logprobs!r}")
    return int(logprobs)


def logprob_sink(slots: int, length: int, n_top: int, device) -> SimpleNamespace:
    """The buffers dfl_logprob_rows scatters into by position, one row of `length` positions per request slot: lp fp32
    [slots, length], and for n_top > 0 top_ids int64 / top_lp fp32 [slots, length, n_top] (else None).  `slot`: the row
    a single-request verify writes.  Unwritten positions hold NaN / -1."""
    n_top = check_logprobs(n_top)
    lp = torch.full((slots, length), float("nan"), dtype=F32, device=device)
    top_ids = torch.full((slots, length, n_top), -1, dtype=I64, device=device) if n_top else None
    top_lp = torch.full((slots, length, n_top), float("nan"), dtype=F32, device=device) if n_top else None
    return SimpleNamespace(lp=lp, top_ids=top_ids, top_lp=top_lp, n_top=n_top, slot=0)


def logprob_rows(logits: torch.Tensor, ids: torch.Tensor, sink, *, ids_off: int = 0, row0: int = 0,
                 nrows: Optional[int] = None, dyn=None, nrows_dyn_word: int = -1, pos_word: int = -1, pos_base: int = 0,
                 pos_add: int = 0, tiles_per_req: int = 1) -> None:
    """Log-probabilities of the ids a verify commits (dfl_logprob_rows) over materialised bf16
    logits [rows <= 16, V] (one tile) or [tiles, 16, V], unit inner stride: log_softmax of the raw logits, at T = 1 and
    unfiltered.  ids int64: [tiles, n] or, for one tile, [n]; tile t row m takes ids[t, ids_off + m - row0].  Rows of a
    tile as in sample_rows_nucleus.  Tile t (tile j = t % tiles_per_req of slot q = t // tiles_per_req) row m writes at
    position (dyn[t][pos_word] if pos_word >= 0 else pos_base) + pos_add + 16 j + m of the sink's row sink.slot + q:
    sink.lp, and sink.top_ids / sink.top_lp when sink.n_top > 0 (logprob_sink); positions outside a row are dropped."""
    assert logits.dim() in (2, 3) and logits.stride(-1) == 1 and logits.is_cuda and logits.dtype == BF16
    if logits.dim() == 2:
        assert logits.shape[0] <= 16, "one tile holds at most 16 rows"
        tiles, tile_rows, tile_stride = 1, logits.shape[0], 16 * logits.stride(0)
    else:
        assert logits.shape[1] == 16
        tiles, tile_rows, tile_stride = logits.shape[0], 16, logits.stride(0)
    V, ld = logits.shape[-1], logits.stride(-2)
    if nrows is None:
        nrows = tile_rows - row0
    assert 0 <= row0 and row0 + nrows <= tile_rows or nrows_dyn_word >= 0 and tile_rows == 16
    n_ids = 16 - row0 if nrows_dyn_word >= 0 else nrows
    assert ids.dim() in (1, 2) and ids.stride(-1) == 1 and ids.shape[-1] >= ids_off + n_ids, "ids"
    assert ids.dim() == 2 and ids.shape[0] >= tiles or tiles == 1, "ids"
    ids_stride = ids.stride(0) if ids.dim() == 2 else 0
    if dyn is not None:
        assert dyn.numel() >= 8 * tiles
    slots = (tiles + tiles_per_req - 1) // tiles_per_req
    lp, n_top = sink.lp, sink.n_top
    assert lp.dim() == 2 and lp.is_contiguous() and 0 <= sink.slot and sink.slot + slots <= lp.shape[0], "sink.lp"
    length = lp.shape[1]
    tid = tlp = None
    if n_top:
        for o in (sink.top_ids, sink.top_lp):
            assert o is not None and o.shape == (lp.shape[0], length, n_top) and o.is_contiguous(), "sink.top_ids / top_lp"
        tid, tlp = sink.top_ids[sink.slot:], sink.top_lp[sink.slot:]
    if ids.dtype != I64 or not ids.is_cuda:
        raise TypeError("dflash_amd: ids must be an int64 GPU tensor")
    check(lib().dfl_logprob_rows(logits.data_ptr(), ld, tile_stride, tiles, V, row0, nrows, _p(dyn, I32, "dyn"),
                                 nrows_dyn_word, pos_word, pos_base, pos_add, tiles_per_req, ids.data_ptr(), ids_stride,
                                 ids_off, n_top, _p(lp[sink.slot:], F32, "sink.lp"), _p(tid, I64, "sink.top_ids"),
                                 _p(tlp, F32, "sink.top_lp"), length, length, _stream()), "dfl_logprob_rows")


def check_penalties(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
    """Validate one request's (repetition_penalty r > 0, presence_penalty a, frequency_penalty f), all finite; the
    tuple (r, a, f) of floats, or None when all three are neutral (1.0, 0.0, 0.0): the path without penalties."""
    import math
    r, a, f = float(repetition_penalty), float(presence_penalty), float(frequency_penalty)
    if not (math.isfinite(r) and r > 0.0):
        raise ValueError(f"dflash_amd: repetition_penalty must be a finite value > 0 (1.0 = off), got {repetition_penalty!r}")
    if not math.isfinite(a):
        raise ValueError(f"dflash_amd: presence_penalty must be finite (0.0 = off), got {presence_penalty!r}")
    if not math.isfinite(f):
        raise ValueError(f"dflash_amd: frequency_penalty must be finite (0.0 = off), got {frequency_penalty!r}")
    return None if (r == 1.0 and a == 0.0 and f == 0.0) else (r, a, f)


def penalty_state(slots: int, V: int, device) -> torch.Tensor:
    """The penalty table int32 [slots, V], zeroed: per request slot and token, bit 31 = seen in the
    prompt, bits 0..30 = occurrences in the output.  Kept by penalty_count, read by penalty_rows."""
    if V < 8 or V % 8:
        raise ValueError(f"dflash_amd: penalties need a vocabulary that is a multiple of 8, got {V}")
    return torch.zeros(slots, V, dtype=I32, device=device)


def penalty_count(table: torch.Tensor, ids: torch.Tensor, *, lo: int = 0, hi: int = 0, dyn=None, lo_word: int = 0,
                  hi_word: int = 0, as_prompt: bool = False, clear: bool = False) -> None:
    """Add ids[s, lo':hi'] to row s of the penalty table for every slot s (dfl_penalty_count; table int32 [slots, V] or
    [V], ids int64 [slots, n] or [n]).  dyn None: lo' = lo, hi' = hi.  dyn (int32 length records, one per slot): lo' =
    dyn[s][lo_word] + lo, hi' = dyn[s][hi_word] + hi, and a slot whose BS word is 0 is skipped whole.  as_prompt: set the
    prompt flag (bit 31) instead of counting; clear: zero the row first, in the same launch."""
    if table.dim() == 1:
        table = table.unsqueeze(0)
    if ids.dim() == 1:
        ids = ids.unsqueeze(0)
    assert table.dim() == 2 and table.stride(1) == 1 and ids.dim() == 2 and ids.stride(1) == 1
    slots, V = table.shape
    assert ids.shape[0] >= slots or slots == 1, "ids: one row per slot"
    if ids.dtype != I64 or not ids.is_cuda or table.dtype != I32 or not table.is_cuda:
        raise TypeError("dflash_amd: penalty_count takes an int32 GPU table and int64 GPU ids")
    if dyn is not None:
        assert dyn.numel() >= 8 * slots
    check(lib().dfl_penalty_count(table.data_ptr(), table.stride(0), V, slots, ids.data_ptr(), ids.stride(0), ids.shape[1],
                                  _p(dyn, I32, "dyn"), lo_word, hi_word, lo, hi, int(as_prompt), int(clear), _stream()),
          "dfl_penalty_count")


def penalty_rows(logits: torch.Tensor, table: torch.Tensor, *, repetition_penalty=1.0, presence_penalty=0.0,
                 frequency_penalty=0.0, block=None, out: Optional[torch.Tensor] = None, row0: int = 0,
                 nrows: Optional[int] = None, dyn=None, nrows_dyn_word: int = -1, tiles_per_req: int = 1,
                 out_ids: Optional[torch.Tensor] = None, out_off: int = 0) -> torch.Tensor:
    """Penalised logits (dfl_penalty_rows) of materialised bf16 logits [rows <= 16, V] (one tile) or
    [tiles, 16, V], unit inner stride; returns `out` (same shape and strides; None: a new buffer; the logits themselves:
    in place).  table int32 [slots, V] or [V]; block int64 [slots, >= the rows of a request] or 1-D for one slot
    (None: no in-block tokens): row m of tile j of slot q sees block[q, 1 : 16 j + m + 1] on top of table row q.
    The three penalties: a host value, or a device fp32 tensor indexed by slot.  Rows of a tile as in
    sample_rows_nucleus.  out_ids (int64, [tiles, n] or [n]): the penalised rows' argmax at out_ids[t, out_off + m - row0]."""
    assert logits.dim() in (2, 3) and logits.stride(-1) == 1 and logits.is_cuda and logits.dtype == BF16
    if logits.dim() == 2:
        assert logits.shape[0] <= 16, "one tile holds at most 16 rows"
        tiles, tile_rows, tile_stride = 1, logits.shape[0], 16 * logits.stride(0)
    else:
        assert logits.shape[1] == 16
        tiles, tile_rows, tile_stride = logits.shape[0], 16, logits.stride(0)
    V, ld = logits.shape[-1], logits.stride(-2)
    if nrows is None:
        nrows = tile_rows - row0
    assert 0 <= row0 and row0 + nrows <= tile_rows or nrows_dyn_word >= 0 and tile_rows == 16
    n_out = 16 - row0 if nrows_dyn_word >= 0 else nrows
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), dtype=BF16, device=logits.device)
    assert out.shape == logits.shape and out.stride() == logits.stride() and out.dtype == BF16 and out.is_cuda, "out"
    if table.dim() == 1:
        table = table.unsqueeze(0)
    slots = (tiles + tiles_per_req - 1) // tiles_per_req
    assert table.dim() == 2 and table.stride(1) == 1 and table.shape == (table.shape[0], V) and table.shape[0] >= slots
    if table.dtype != I32 or not table.is_cuda:
        raise TypeError("dflash_amd: the penalty table must be an int32 GPU tensor")
    blk_stride = 0
    if block is not None:
        if block.dtype != I64 or not block.is_cuda:
            raise TypeError("dflash_amd: block must be an int64 GPU tensor")
        assert block.stride(-1) == 1 and block.shape[-1] >= 16 * (tiles_per_req - 1) + row0 + n_out, "block"
        assert block.dim() == 2 and block.shape[0] >= slots or block.dim() == 1 and slots == 1, "block"
        blk_stride = block.stride(0) if block.dim() == 2 else 0
    out_stride = 0
    if out_ids is not None:
        assert out_ids.stride(-1) == 1 and out_ids.shape[-1] >= out_off + n_out, "out_ids"
        assert out_ids.dim() == 2 and out_ids.shape[0] >= tiles or out_ids.dim() == 1 and tiles == 1, "out_ids"
        out_stride = out_ids.stride(0) if out_ids.dim() == 2 else 0
    if dyn is not None:
        assert dyn.numel() >= 8 * tiles

    def dev_or_host(v, name, neutral):
        if torch.is_tensor(v):
            assert v.numel() >= slots, name
            return _p(v, F32, name), neutral
        return None, float(v)

    r_p, r_v = dev_or_host(repetition_penalty, "repetition_penalty", 1.0)
    a_p, a_v = dev_or_host(presence_penalty, "presence_penalty", 0.0)
    f_p, f_v = dev_or_host(frequency_penalty, "frequency_penalty", 0.0)
    check(lib().dfl_penalty_rows(logits.data_ptr(), out.data_ptr(), ld, tile_stride, tiles, V, row0, nrows,
                                 _p(dyn, I32, "dyn"), nrows_dyn_word, tiles_per_req, table.data_ptr(), table.stride(0),
                                 None if block is None else block.data_ptr(), blk_stride, r_p, r_v, a_p, a_v, f_p, f_v,
                                 _p(out_ids, I64, "out_ids"), out_stride, out_off, _stream()), "dfl_penalty_rows")
    return out


def check_logit_bias(V: int, logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_tokens=0,
                     stop_token_ids=None):
    """Validate one request's logit_bias ({id: bias}, finite or -inf), allowed_token_ids (non-empty), banned_token_ids
    and min_tokens (int >= 0) for a vocabulary of V.  None when everything is neutral: no / empty
    mapping and lists, a mapping of zeros, min_tokens == 0 or no stop ids — the path without the feature.  Otherwise
    (b, min_tokens): b a host fp32 tensor [V] with -inf where a token is not allowed, banned or biased by -inf, the bias
    (or 0) elsewhere; min_tokens 0 when there is no stop id to suppress."""
    import math
    import operator

    def ids_of(seq, name):
        out = []
        for v in seq:
            try:
                i = operator.index(v)
            except TypeError:
                raise ValueError(f"dflash_amd: {name}: {v!r} is not a token id") from None
            if not 0 <= i < V:
                raise ValueError(f"dflash_amd: {name}: id {i} outside [0, {V})")
            out.append(i)
        return out

    try:
        mt = operator.index(min_tokens)
    except TypeError:
        raise ValueError(f"dflash_amd: min_tokens must be an integer >= 0, got {min_tokens!r}") from None
    if mt < 0:
        raise ValueError(f"dflash_amd: min_tokens must be an integer >= 0, got {min_tokens!r}")
    stops = [int(s) for s in (stop_token_ids if stop_token_ids is not None else ())]
    if not stops:
        mt = 0      # nothing to suppress
    b = torch.zeros(V, dtype=F32)
    for k, v in (logit_bias or {}).items():
        i = ids_of([int(k) if isinstance(k, str) else k], "logit_bias")[0]
        v = float(v)
        if math.isnan(v) or v == math.inf or (v != -math.inf and abs(v) > 3.4028234663852886e38):
            raise ValueError(f"dflash_amd: logit_bias[{i}] = {v!r}: a bias is finite in fp32, or -inf for a ban")
        b[i] = v
    if allowed_token_ids is not None:
        allowed = ids_of(allowed_token_ids, "allowed_token_ids")
        if not allowed:
            raise ValueError("dflash_amd: allowed_token_ids is empty (None: no allow list)")
        keep = torch.zeros(V, dtype=torch.bool)
        keep[torch.tensor(allowed, dtype=I64)] = True
        b[~keep] = -math.inf
    if banned_token_ids is not None:
        banned = ids_of(banned_token_ids, "banned_token_ids")
        if banned:
            b[torch.tensor(banned, dtype=I64)] = -math.inf
    live = b > -math.inf
    if mt > 0:
        for s in stops:
            if 0 <= s < V:
                live[s] = False
    if not bool(live.any()):
        raise ValueError("dflash_amd: logit_bias / allowed_token_ids / banned_token_ids / min_tokens leave no token finite")
    if mt == 0 and not bool((b != 0).any()):
        return None
    return b, mt


def logit_bias_state(slots: int, V: int, device) -> SimpleNamespace:
    """The logit-bias state: .bias fp32 [slots, V], zeroed — one dense table row per request slot —
    and .min_pos int32 [slots], zeroed (0: min_tokens off).  Written by logit_bias_set, read by logit_bias_rows."""
    if V < 8 or V % 8:
        raise ValueError(f"dflash_amd: logit bias needs a vocabulary that is a multiple of 8, got {V}")
    return SimpleNamespace(bias=torch.zeros(slots, V, dtype=F32, device=device),
                           min_pos=torch.zeros(slots, dtype=I32, device=device))


def logit_bias_set(state, slot: int, b, min_pos: int = 0) -> None:
    """Rewrite slot's whole table row (b: a host or device fp32 [V], None: zeros) and its min_pos: nothing of the slot's
    previous request survives.  Admission only, plain copies."""
    if not 0 <= slot < state.bias.shape[0]:
        raise ValueError(f"dflash_amd: logit_bias_set: slot {slot} outside 0..{state.bias.shape[0] - 1}")
    if b is None:
        state.bias[slot].zero_()
    else:
        b = torch.as_tensor(b, dtype=F32)
        if b.shape != (state.bias.shape[1],):
            raise ValueError(f"dflash_amd: logit_bias_set: b has shape {tuple(b.shape)}, the table row ({state.bias.shape[1]},)")
        state.bias[slot].copy_(b)
    state.min_pos[slot:slot + 1].fill_(int(min_pos))


def logit_bias_rows(logits: torch.Tensor, bias: torch.Tensor, *, min_pos=0, stop_ids: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, row0: int = 0, nrows: Optional[int] = None, dyn=None,
                    nrows_dyn_word: int = -1, pos_word: int = -1, pos_base: int = 0, pos_add: int = 0,
                    tiles_per_req: int = 1, out_ids: Optional[torch.Tensor] = None, out_off: int = 0) -> torch.Tensor:
    """Biased logits (dfl_logit_bias_rows) of materialised bf16 logits [rows <= 16, V] (one tile) or
    [tiles, 16, V], unit inner stride; returns `out` (same shape and strides; None: a new buffer; the logits themselves:
    in place).  bias fp32 [slots, V] or [V]: row m of tile j of slot q takes table row q and predicts position
    (dyn[t][pos_word] if pos_word >= 0 else pos_base) + pos_add + 16 j + m; while that is < min_pos (a host int, or a
    device int32 tensor indexed by slot) the stop_ids (device int64, the accept launch's list) are set to -inf.  Rows of a
    tile as in sample_rows_nucleus.  out_ids (int64, [tiles, n] or [n]): the rows' argmax at out_ids[t, out_off + m - row0]."""
    assert logits.dim() in (2, 3) and logits.stride(-1) == 1 and logits.is_cuda and logits.dtype == BF16
    if logits.dim() == 2:
        assert logits.shape[0] <= 16, "one tile holds at most 16 rows"
        tiles, tile_rows, tile_stride = 1, logits.shape[0], 16 * logits.stride(0)
    else:
        assert logits.shape[1] == 16
        tiles, tile_rows, tile_stride = logits.shape[0], 16, logits.stride(0)
    V, ld = logits.shape[-1], logits.stride(-2)
    if nrows is None:
        nrows = tile_rows - row0
    assert 0 <= row0 and row0 + nrows <= tile_rows or nrows_dyn_word >= 0 and tile_rows == 16
    n_out = 16 - row0 if nrows_dyn_word >= 0 else nrows
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), dtype=BF16, device=logits.device)
    assert out.shape == logits.shape and out.stride() == logits.stride() and out.dtype == BF16 and out.is_cuda, "out"
    if bias.dim() == 1:
        bias = bias.unsqueeze(0)
    slots = (tiles + tiles_per_req - 1) // tiles_per_req
    assert bias.dim() == 2 and bias.stride(1) == 1 and bias.shape == (bias.shape[0], V) and bias.shape[0] >= slots
    if bias.dtype != F32 or not bias.is_cuda:
        raise TypeError("dflash_amd: the logit-bias table must be an fp32 GPU tensor")
    mp_p, mp_v = None, 0
    if torch.is_tensor(min_pos):
        assert min_pos.numel() >= slots, "min_pos"
        mp_p = _p(min_pos, I32, "min_pos")
    else:
        mp_v = int(min_pos)
    n_stop = 0 if stop_ids is None else stop_ids.numel()
    out_stride = 0
    if out_ids is not None:
        assert out_ids.stride(-1) == 1 and out_ids.shape[-1] >= out_off + n_out, "out_ids"
        assert out_ids.dim() == 2 and out_ids.shape[0] >= tiles or out_ids.dim() == 1 and tiles == 1, "out_ids"
        out_stride = out_ids.stride(0) if out_ids.dim() == 2 else 0
    if dyn is not None:
        assert dyn.numel() >= 8 * tiles
    check(lib().dfl_logit_bias_rows(logits.data_ptr(), out.data_ptr(), ld, tile_stride, tiles, V, row0, nrows,
                                    _p(dyn, I32, "dyn"), nrows_dyn_word, tiles_per_req, bias.data_ptr(), bias.stride(0),
                                    mp_p, mp_v, _p(stop_ids, I64, "stop_ids") if n_stop else None, n_stop, pos_word,
                                    pos_base, pos_add, _p(out_ids, I64, "out_ids"), out_stride, out_off, _stream()),
          "dfl_logit_bias_rows")
    return out


def check_min_p(min_p) -> Optional[float]:
    """Validate one request's min_p: None or 0 is off and returns None; a float in (0, 1] is
    returned as a float.  A bool, a NaN or anything else raises ValueError."""
    if min_p is None:
        return None
    if isinstance(min_p, (bool, str, bytes)) or torch.is_tensor(min_p):
        raise ValueError(f"dflash_amd: min_p must be None or a number in [0, 1] (0 = off), got {min_p!r}")
    try:
        v = float(min_p)
    except (TypeError, ValueError):
        raise ValueError(f"dflash_amd: min_p must be None or a number in [0, 1] (0 = off), got {min_p!r}") from None
    if not 0.0 <= v <= 1.0:     # a NaN fails both comparisons
        raise ValueError(f"dflash_amd: min_p must be inside [0, 1] (0 = off), got {min_p!r}")
    return v if v > 0.0 else None


def min_p_log(min_p) -> float:
    """float32(ln(min_p)) computed on the host, the L of dfl_min_p_rows; -inf for None / 0 (off)."""
    import math
    import numpy as np
    v = check_min_p(min_p)
    return -math.inf if v is None else float(np.float32(math.log(v)))


def min_p_rows(logits: torch.Tensor, *, min_p=None, log_min_p: Optional[torch.Tensor] = None,
               temperature: Optional[float] = None, inv_t: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None, row0: int = 0, nrows: Optional[int] = None, dyn=None,
               nrows_dyn_word: int = -1, tiles_per_req: int = 1, kept: Optional[torch.Tensor] = None,
               kept_off: int = 0) -> torch.Tensor:
    """min_p-masked logits (dfl_min_p_rows) of materialised bf16 logits [rows <= 16, V] (one tile)
    or [tiles, 16, V], unit inner stride; returns `out` (same shape and strides; None: a new buffer; the logits
    themselves: in place).  Column v of a row stays iff (x_v - max) * invT >= ln(min_p) or x_v is the row's maximum; the
    others become -inf.  Give min_p (a host value, check_min_p) or log_min_p (a device fp32 tensor of float32(ln(min_p))
    per request slot, -inf: off), and temperature (a host value > 0) or inv_t (a device fp32 tensor of invT per slot; a
    slot whose value is not > 0 is greedy: its rows are copied).  Rows of a tile as in sample_rows_nucleus.  kept (int32,
    [tiles, n] or [n]): the number of columns the rule kept at kept[t, kept_off + m - row0]; a copied row reports V."""
    assert logits.dim() in (2, 3) and logits.stride(-1) == 1 and logits.is_cuda and logits.dtype == BF16
    if logits.dim() == 2:
        assert logits.shape[0] <= 16, "one tile holds at most 16 rows"
        tiles, tile_rows, tile_stride = 1, logits.shape[0], 16 * logits.stride(0)
    else:
        assert logits.shape[1] == 16
        tiles, tile_rows, tile_stride = logits.shape[0], 16, logits.stride(0)
    V, ld = logits.shape[-1], logits.stride(-2)
    if nrows is None:
        nrows = tile_rows - row0
    assert 0 <= row0 and row0 + nrows <= tile_rows or nrows_dyn_word >= 0 and tile_rows == 16
    n_out = 16 - row0 if nrows_dyn_word >= 0 else nrows
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), dtype=BF16, device=logits.device)
    assert out.shape == logits.shape and out.stride() == logits.stride() and out.dtype == BF16 and out.is_cuda, "out"
    slots = (tiles + tiles_per_req - 1) // tiles_per_req
    if (min_p is None) == (log_min_p is None):
        raise ValueError("min_p_rows: give either min_p or log_min_p")
    if (temperature is None) == (inv_t is None):
        raise ValueError("min_p_rows: give either temperature or inv_t")
    if log_min_p is not None:
        assert torch.is_tensor(log_min_p) and log_min_p.numel() >= slots, "log_min_p"
    if inv_t is not None:
        assert torch.is_tensor(inv_t) and inv_t.numel() >= slots, "inv_t"
    kept_stride = 0
    if kept is not None:
        assert kept.stride(-1) == 1 and kept.shape[-1] >= kept_off + n_out, "kept"
        assert kept.dim() == 2 and kept.shape[0] >= tiles or kept.dim() == 1 and tiles == 1, "kept"
        kept_stride = kept.stride(0) if kept.dim() == 2 else 0
    if dyn is not None:
        assert dyn.numel() >= 8 * tiles
    check(lib().dfl_min_p_rows(logits.data_ptr(), out.data_ptr(), ld, tile_stride, tiles, V, row0, nrows,
                               _p(dyn, I32, "dyn"), nrows_dyn_word, tiles_per_req, _p(log_min_p, F32, "log_min_p"),
                               0.0 if log_min_p is not None else min_p_log(min_p),
                               _p(inv_t, F32, "inv_t"), 0.0 if inv_t is not None else inv_temperature(temperature),
                               _p(kept, I32, "kept"), kept_stride, kept_off, _stream()), "dfl_min_p_rows")
    return out


I16 = torch.int16


def check_grammar(dfa, V: int, logit_bias_row=None) -> None:
    """Validate a TokenDFA for a vocabulary of V: next an int16 numpy array [S, V], 1 <= S <= 32767,
    V % 8 == 0, successors in [-1, S), start in [0, S), and every state reachable from start has a legal token —
    where logit_bias_row (fp32 [V], the row check_logit_bias returns) is given, one that it does not ban."""
    import numpy as np
    import operator
    if is_byte_grammar(dfa):   # the host-side checks only: reachability is checked on the loaded rows (grammar_load)
        S, Vd = dfa.num_states, dfa.vocab_size
        if not 1 <= S <= 32767:
            raise ValueError(f"dflash_amd: grammar: {S} states, 1..32767 fit the int16 table")
        if Vd != int(V) or Vd < 8 or Vd % 8:
            raise ValueError(f"dflash_amd: grammar: the vocabulary has {Vd} tokens, the model's {V} (a multiple of 8)")
        if not 0 <= dfa.start < S:
            raise ValueError(f"dflash_amd: grammar: start {dfa.start} outside [0, {S})")
        return
    nxt = getattr(dfa, "next", None)
    if not isinstance(nxt, np.ndarray) or nxt.dtype != np.int16 or nxt.ndim != 2:
        raise ValueError("dflash_amd: grammar: TokenDFA.next must be an int16 numpy array [S, V]")
    S, Vd = nxt.shape
    if not 1 <= S <= 32767:
        raise ValueError(f"dflash_amd: grammar: {S} states, 1..32767 fit the int16 table")
    if Vd != int(V) or Vd < 8 or Vd % 8:
        raise ValueError(f"dflash_amd: grammar: the table has {Vd} columns, the vocabulary {V} (a multiple of 8)")
    if int(nxt.min()) < -1 or int(nxt.max()) >= S:
        raise ValueError(f"dflash_amd: grammar: a successor lies outside [-1, {S})")
    try:
        start = operator.index(dfa.start)
    except TypeError:
        raise ValueError(f"dflash_amd: grammar: start {dfa.start!r} is not a state") from None
    if not 0 <= start < S:
        raise ValueError(f"dflash_amd: grammar: start {start} outside [0, {S})")
    open_cols = None
    if logit_bias_row is not None:
        b = torch.as_tensor(logit_bias_row, dtype=F32).cpu().numpy()
        if b.shape != (Vd,):
            raise ValueError(f"dflash_amd: grammar: the bias row has shape {b.shape}, the vocabulary ({Vd},)")
        open_cols = b > -np.inf
    reached = np.zeros(S, dtype=bool)
    reached[start] = True
    frontier = np.array([start])
    while frontier.size:
        rows = nxt[frontier]
        legal = rows >= 0
        dead = ~legal.any(axis=1)
        if dead.any():
            raise ValueError(f"dflash_amd: grammar: state {int(frontier[dead][0])} is reachable from start {start} and has "
                             f"no legal token")
        if open_cols is not None:
            shut = ~(legal & open_cols[None, :]).any(axis=1)
            if shut.any():
                raise ValueError(f"dflash_amd: grammar: every legal token of reachable state {int(frontier[shut][0])} is "
                                 f"banned by logit_bias / allowed_token_ids / banned_token_ids")
        succ = np.unique(rows[legal])
        frontier = succ[~reached[succ]]
        reached[frontier] = True


def grammar_state(slots: int, pool_states: int, V: int, device) -> SimpleNamespace:
    """The grammar state: .table int16 [pool_states, V], the pool, all -1 (no token legal) until
    grammar_load writes a grammar's rows; .base int32 [slots] (-1: the slot has no grammar) and .state int32 [slots]
    (relative to base; -1: violated), written by grammar_set; .used: the pool rows handed out so far (host)."""
    if V < 8 or V % 8:
        raise ValueError(f"dflash_amd: a grammar needs a vocabulary that is a multiple of 8, got {V}")
    if pool_states < 1 or slots < 1:
        raise ValueError(f"dflash_amd: grammar_state: slots={slots} pool_states={pool_states}")
    return SimpleNamespace(table=torch.full((pool_states, V), -1, dtype=I16, device=device),
                           base=torch.full((slots,), -1, dtype=I32, device=device),
                           state=torch.full((slots,), -1, dtype=I32, device=device), used=0)


LIFT_MAX_STATES = 4096   # dfl_grammar_lift / dfl_grammar_reach: the largest automaton lifted and checked on the device


def is_byte_grammar(g) -> bool:
    return hasattr(g, "char_next") and hasattr(g, "vocabulary")


def grammar_load(state, dfa, logit_bias_row=None) -> int:
    """Validate dfa (check_grammar) and put its table into the next free pool rows; returns their base.  A TokenDFA's
    table is copied; a ByteGrammar is lifted on the device (grammar_lift) and its reachability is checked on the rows
    just written (grammar_reach_check: on failure the rows are filled back with -1 and `used` stays) — above
    LIFT_MAX_STATES states it loads as its to_token_dfa().  ValueError when the pool has fewer rows left than the
    grammar has states.  The pool's storage never moves."""
    pool, V = state.table.shape
    check_grammar(dfa, V, logit_bias_row)
    if is_byte_grammar(dfa) and dfa.num_states > LIFT_MAX_STATES:
        dfa = dfa.to_token_dfa()
        check_grammar(dfa, V, logit_bias_row)
    S = dfa.num_states if is_byte_grammar(dfa) else dfa.next.shape[0]
    if state.used + S > pool:
        raise ValueError(f"dflash_amd: the grammar pool is full: {S} states asked, {pool - state.used} of {pool} rows free")
    base = state.used
    if is_byte_grammar(dfa):
        grammar_lift(state, dfa, base)
        try:
            grammar_reach_check(state, base, S, dfa.start, logit_bias_row)
        except ValueError:
            state.table[base:base + S].fill_(-1)
            raise
    else:
        import numpy as np
        state.table[base:base + S].copy_(torch.from_numpy(np.ascontiguousarray(dfa.next)))
    state.used = base + S
    return base


def grammar_lift(state, grammar, base: int) -> None:
    """dfl_grammar_lift: pool rows [base, base + grammar.num_states) of state.table from a
    ByteGrammar's byte automaton and its Vocabulary's device buffers — TokenDFA.from_bytes' table, entry for entry.  Only
    the automaton ([Sc, 256] int16), the accepting flags and, once per vocabulary and device, the byte strings cross the
    bus."""
    import numpy as np
    table = _grammar_pool(state)
    dev = table.device
    data, off, eos = grammar.vocabulary.device_buffers(dev)
    Sc = grammar.num_states
    if off.numel() != table.shape[1] + 1:
        raise ValueError(f"dflash_amd: grammar_lift: the vocabulary has {off.numel() - 1} tokens, the pool {table.shape[1]}")
    acc = np.zeros(Sc, dtype=np.uint8)
    acc[list(grammar.accepting)] = 1
    dfa = torch.from_numpy(grammar.char_next).to(dev)
    acc_t = torch.from_numpy(acc).to(dev)
    n_eos = len(grammar.vocabulary.eos_ids)
    check(lib().dfl_grammar_lift(table.data_ptr(), table.stride(0), table.shape[0], table.shape[1], int(base),
                                 _p(dfa, I16, "dfa"), Sc, _p(data, U8, "token bytes"), data.numel(),
                                 _p(off, I32, "token offsets"), _p(acc_t, U8, "accepting"),
                                 _p(eos, I32, "eos ids") if n_eos else None, n_eos, _stream()), "dfl_grammar_lift")


def grammar_reach(state, base: int, S: int, logit_bias_row=None):
    """dfl_grammar_reach over pool rows [base, base + S): (adj uint8 [S, S], any_legal uint8 [S]) on the device.
    adj[s, t] = 1 iff a legal token that logit_bias_row (fp32 [V]; -inf: banned) does not ban leads from s to t;
    any_legal[s] = 1 iff s has a legal token at all."""
    table = _grammar_pool(state)
    V = table.shape[1]
    bias = None
    if logit_bias_row is not None:
        bias = torch.as_tensor(logit_bias_row, dtype=F32).to(table.device).contiguous()
        if bias.shape != (V,):
            raise ValueError(f"dflash_amd: grammar: the bias row has shape {tuple(bias.shape)}, the vocabulary ({V},)")
    adj = torch.empty((S, S), dtype=U8, device=table.device)
    any_legal = torch.empty((S,), dtype=U8, device=table.device)
    check(lib().dfl_grammar_reach(table.data_ptr(), table.stride(0), table.shape[0], V, int(base), int(S),
                                  _p(bias, F32, "bias row"), adj.data_ptr(), any_legal.data_ptr(), _stream()),
          "dfl_grammar_reach")
    return adj, any_legal


def grammar_reach_check(state, base: int, S: int, start: int, logit_bias_row=None) -> None:
    """check_grammar's reachability check on loaded rows: grammar_reach, its two results copied back, and a breadth-first
    search from start over adj.  The same two ValueErrors: a reachable state without a legal token, a reachable state
    whose legal tokens the bias row bans all.  (The search follows the tokens that can be emitted — legal and not banned
    — where check_grammar follows every legal one.)"""
    adj, any_legal = grammar_reach(state, base, S, logit_bias_row)
    adj, any_legal = adj.cpu().numpy().astype(bool), any_legal.cpu().numpy().astype(bool)
    reached = [False] * S
    reached[start] = True
    frontier = [start]
    while frontier:
        nxt = []
        for s in frontier:
            if not any_legal[s]:
                raise ValueError(f"dflash_amd: grammar: state {s} is reachable from start {start} and has no legal token")
            succ = adj[s].nonzero()[0]
            if not succ.size:
                raise ValueError(f"dflash_amd: grammar: every legal token of reachable state {s} is "
                                 f"banned by logit_bias / allowed_token_ids / banned_token_ids")
            for t in succ.tolist():
                if not reached[t]:
                    reached[t] = True
                    nxt.append(t)
        frontier = sorted(nxt)


def grammar_set(state, slot: int, base, start: int = 0) -> None:
    """Slot's grammar: base (a value grammar_load returned; None or < 0: no grammar, the slot's rows pass unmasked) and
    its state, start.  Admission only, plain fills."""
    if not 0 <= slot < state.base.shape[0]:
        raise ValueError(f"dflash_amd: grammar_set: slot {slot} outside 0..{state.base.shape[0] - 1}")
    if base is None or base < 0:
        base, start = -1, -1
    elif not (base < state.table.shape[0] and 0 <= start < state.table.shape[0] - base):
        raise ValueError(f"dflash_amd: grammar_set: base {base} / start {start} outside the pool of {state.table.shape[0]}")
    state.base[slot:slot + 1].fill_(int(base))
    state.state[slot:slot + 1].fill_(int(start))


def _grammar_pool(state):
    t = state.table
    if t.dtype != I16 or not t.is_cuda or state.base.dtype != I32 or state.state.dtype != I32:
        raise TypeError("dflash_amd: the grammar pool must be an int16 GPU tensor, base / state int32")
    assert t.dim() == 2 and t.stride(1) == 1 and state.base.is_cuda and state.state.is_cuda
    assert state.base.is_contiguous() and state.state.is_contiguous()
    return t


def grammar_rows(logits: torch.Tensor, state, *, block=None, out: Optional[torch.Tensor] = None, row0: int = 0,
                 nrows: Optional[int] = None, dyn=None, nrows_dyn_word: int = -1, tiles_per_req: int = 1,
                 out_ids: Optional[torch.Tensor] = None, out_off: int = 0) -> torch.Tensor:
    """Grammar-masked logits (dfl_grammar_rows) of materialised bf16 logits [rows <= 16, V] (one
    tile) or [tiles, 16, V], unit inner stride; returns `out` (same shape and strides; None: a new buffer; the logits
    themselves: in place).  state: a grammar_state.  block int64 [slots, >= the rows of a request] or 1-D for one slot:
    row m of slot q walks state[q] through block[q, 1 : m + 1] and masks by where it arrives, or is copied unchanged
    when the walk dies; None: no walk, the single-row form for a first token.  Rows of a tile as in penalty_rows.
    out_ids: the rows' argmax at out_ids[t, out_off + m - row0].  tiles_per_req = 2 (17..32-row blocks) is refused."""
    if tiles_per_req != 1:
        raise NotImplementedError("dflash_amd: grammar_rows takes one tile per request (blocks of <= 16 rows)")
    assert logits.dim() in (2, 3) and logits.stride(-1) == 1 and logits.is_cuda and logits.dtype == BF16
    if logits.dim() == 2:
        assert logits.shape[0] <= 16, "one tile holds at most 16 rows"
        tiles, tile_rows, tile_stride = 1, logits.shape[0], 16 * logits.stride(0)
    else:
        assert logits.shape[1] == 16
        tiles, tile_rows, tile_stride = logits.shape[0], 16, logits.stride(0)
    V, ld = logits.shape[-1], logits.stride(-2)
    if nrows is None:
        nrows = tile_rows - row0
    assert 0 <= row0 and row0 + nrows <= tile_rows or nrows_dyn_word >= 0 and tile_rows == 16
    n_out = 16 - row0 if nrows_dyn_word >= 0 else nrows
    if out is None:
        out = torch.empty_strided(logits.shape, logits.stride(), dtype=BF16, device=logits.device)
    assert out.shape == logits.shape and out.stride() == logits.stride() and out.dtype == BF16 and out.is_cuda, "out"
    table = _grammar_pool(state)
    assert table.shape[1] == V and state.base.numel() >= tiles and state.state.numel() >= tiles, "one base / state per slot"
    blk_stride = 0
    if block is not None:
        if block.dtype != I64 or not block.is_cuda:
            raise TypeError("dflash_amd: block must be an int64 GPU tensor")
        assert block.stride(-1) == 1 and block.shape[-1] >= row0 + n_out, "block"
        assert block.dim() == 2 and block.shape[0] >= tiles or block.dim() == 1 and tiles == 1, "block"
        blk_stride = block.stride(0) if block.dim() == 2 else 0
    out_stride = 0
    if out_ids is not None:
        assert out_ids.stride(-1) == 1 and out_ids.shape[-1] >= out_off + n_out, "out_ids"
        assert out_ids.dim() == 2 and out_ids.shape[0] >= tiles or out_ids.dim() == 1 and tiles == 1, "out_ids"
        out_stride = out_ids.stride(0) if out_ids.dim() == 2 else 0
    if dyn is not None:
        assert dyn.numel() >= 8 * tiles
    check(lib().dfl_grammar_rows(logits.data_ptr(), out.data_ptr(), ld, tile_stride, tiles, V, row0, nrows,
                                 _p(dyn, I32, "dyn"), nrows_dyn_word, 1, table.data_ptr(), table.stride(0), table.shape[0],
                                 state.base.data_ptr(), state.state.data_ptr(),
                                 None if block is None else block.data_ptr(), blk_stride, _p(out_ids, I64, "out_ids"),
                                 out_stride, out_off, _stream()), "dfl_grammar_rows")
    return out


def grammar_draft_rows(logits: torch.Tensor, state=None, *, bias: Optional[torch.Tensor] = None, block: torch.Tensor,
                       nrows: Optional[int] = None, dyn=None, nrows_dyn_word: int = -1, tiles_per_req: int = 1) -> None:
    """The draft's block tokens picked under the automaton (dfl_grammar_draft_rows): logits bf16
    [rows <= 16, V] (one slot) or [tiles, 16, V], row m predicting block slot m, as the draft's head launch materialised
    them; block int64 [slots, >= 16] or 1-D for one slot, block[q, 1:n] holding that launch's argmax.  Slot q walks
    state[q] (a grammar_state; None: the ban-only form) row by row: block[q, m] <- the lowest legal column among the
    maxima over the legal, non-NaN columns of row m, legal = a successor >= 0 in the state reached over block[q, 1:m]
    and not banned (bias fp32 [slots, V] or [V], the logit-bias table: -inf is a ban, finite values are ignored; None:
    the grammar-only form).  The walk stops, and the ids from there on stay, at a violated state, a row without such a
    column, or a successor outside the pool.  n = nrows (None: the logits' rows), or dyn[t][nrows_dyn_word].  The
    state is only read.  tiles_per_req = 2 (17..32-row blocks) is refused."""
    args = _grammar_draft_args(logits, state, bias, block, nrows, dyn, nrows_dyn_word, tiles_per_req)
    check(lib().dfl_grammar_draft_rows(*args, _stream()), "dfl_grammar_draft_rows")


def grammar_draft_sample_rows(logits: torch.Tensor, state=None, *, bias: Optional[torch.Tensor] = None, block: torch.Tensor,
                              seeds: torch.Tensor, temperature: Optional[float] = None,
                              inv_ts: Optional[torch.Tensor] = None, pos_dyn_word: int = -1, pos_base: int = 0,
                              nrows: Optional[int] = None, dyn=None, nrows_dyn_word: int = -1,
                              tiles_per_req: int = 1) -> None:
    """grammar_draft_rows under the target's noise (dfl_grammar_draft_sample_rows): block[q, m] <-
    the lowest legal column among the maxima of fmaf(logit, invT, g(seeds[q], RNG_TARGET, base_q + m, v, 0)) over the
    legal columns of row m — what the coupled draft head drew, restricted to what the request can emit.  seeds: int64
    [slots] on the device.  Either `temperature` (one host value) or inv_ts (device fp32 [slots]; a slot whose value is
    not > 0 gets grammar_draft_rows' plain pick).  base_q = dyn[q][pos_dyn_word] (the draft record's DYN_START) when
    pos_dyn_word >= 0, else pos_base."""
    if (temperature is None) == (inv_ts is None):
        raise ValueError("grammar_draft_sample_rows: give either temperature or inv_ts")
    args = _grammar_draft_args(logits, state, bias, block, nrows, dyn, nrows_dyn_word, tiles_per_req)
    tiles = args[3]
    if seeds.dtype != I64 or not seeds.is_cuda or seeds.numel() < tiles:
        raise TypeError("dflash_amd: seeds must be an int64 GPU tensor with one seed per slot")
    if inv_ts is not None and (inv_ts.dtype != F32 or not inv_ts.is_cuda or inv_ts.numel() < tiles):
        raise TypeError("dflash_amd: inv_ts must be an fp32 GPU tensor with one value per slot")
    if pos_dyn_word >= 0:
        assert dyn is not None and dyn.numel() >= 8 * tiles, "pos_dyn_word needs the records"
    check(lib().dfl_grammar_draft_sample_rows(*args, seeds.data_ptr(),
                                              0.0 if inv_ts is not None else inv_temperature(temperature),
                                              _p(inv_ts, F32, "inv_ts"), pos_dyn_word, int(pos_base), _stream()),
          "dfl_grammar_draft_sample_rows")


def _grammar_draft_args(logits, state, bias, block, nrows, dyn, nrows_dyn_word, tiles_per_req) -> tuple:
    """The arguments dfl_grammar_draft_rows and its noise form share, validated."""
    if tiles_per_req != 1:
        raise NotImplementedError("dflash_amd: grammar_draft_rows takes one tile per request (blocks of <= 16 rows)")
    if state is None and bias is None:
        raise ValueError("dflash_amd: grammar_draft_rows needs a grammar state or a bias table to constrain by")
    assert logits.dim() in (2, 3) and logits.stride(-1) == 1 and logits.is_cuda and logits.dtype == BF16
    if logits.dim() == 2:
        assert logits.shape[0] <= 16, "one tile holds at most 16 rows"
        tiles, tile_rows, tile_stride = 1, logits.shape[0], 16 * logits.stride(0)
    else:
        assert logits.shape[1] == 16
        tiles, tile_rows, tile_stride = logits.shape[0], 16, logits.stride(0)
    V, ld = logits.shape[-1], logits.stride(-2)
    if nrows is None:
        nrows = tile_rows
    assert 0 <= nrows <= tile_rows or nrows_dyn_word >= 0 and tile_rows == 16
    n_out = 16 if nrows_dyn_word >= 0 else nrows
    t_p, t_stride, t_rows, b_p, s_p = None, 0, 0, None, None
    if state is not None:
        table = _grammar_pool(state)
        assert table.shape[1] == V and state.base.numel() >= tiles and state.state.numel() >= tiles, "one base / state per slot"
        t_p, t_stride, t_rows, b_p, s_p = table.data_ptr(), table.stride(0), table.shape[0], state.base.data_ptr(), state.state.data_ptr()
    bias_p, bias_stride = None, 0
    if bias is not None:
        if bias.dim() == 1:
            bias = bias.unsqueeze(0)
        assert bias.dim() == 2 and bias.stride(1) == 1 and bias.shape == (bias.shape[0], V) and bias.shape[0] >= tiles
        if bias.dtype != F32 or not bias.is_cuda:
            raise TypeError("dflash_amd: the logit-bias table must be an fp32 GPU tensor")
        bias_p, bias_stride = bias.data_ptr(), bias.stride(0)
    if block.dtype != I64 or not block.is_cuda:
        raise TypeError("dflash_amd: block must be an int64 GPU tensor")
    assert block.stride(-1) == 1 and block.shape[-1] >= n_out, "block"
    assert block.dim() == 2 and block.shape[0] >= tiles or block.dim() == 1 and tiles == 1, "block"
    blk_stride = block.stride(0) if block.dim() == 2 else 0
    assert tiles == 1 or blk_stride >= 16, "block: one row of >= 16 ids per slot"
    if dyn is not None:
        assert dyn.numel() >= 8 * tiles
    return (logits.data_ptr(), ld, tile_stride, tiles, V, nrows, _p(dyn, I32, "dyn"), nrows_dyn_word, t_p, t_stride, t_rows,
            b_p, s_p, bias_p, bias_stride, block.data_ptr(), blk_stride)


def grammar_advance(state, ids: torch.Tensor, *, lo: int = 0, hi: int = 0, dyn=None, lo_word: int = 0,
                    hi_word: int = 0, slots: Optional[int] = None) -> None:
    """Step every slot's state over ids[s, lo':hi'] (dfl_grammar_advance; ids int64 [slots, n] or [n]); the range and the
    idle-slot rule as penalty_count takes them.  An illegal id, or one outside the vocabulary, leaves -1, which stays.
    slots: the first `slots` of the state's slots (None: all)."""
    table = _grammar_pool(state)
    if ids.dim() == 1:
        ids = ids.unsqueeze(0)
    if slots is None:
        slots = state.base.numel()
    assert 0 <= slots <= state.base.numel() == state.state.numel(), "slots"
    assert ids.dim() == 2 and ids.stride(1) == 1 and (ids.shape[0] >= slots or slots == 1), "ids: one row per slot"
    if ids.dtype != I64 or not ids.is_cuda:
        raise TypeError("dflash_amd: grammar_advance takes int64 GPU ids")
    if dyn is not None:
        assert dyn.numel() >= 8 * slots
    check(lib().dfl_grammar_advance(table.data_ptr(), table.stride(0), table.shape[0], table.shape[1],
                                    state.base.data_ptr(), state.state.data_ptr(), slots, ids.data_ptr(), ids.stride(0),
                                    ids.shape[1], _p(dyn, I32, "dyn"), lo_word, hi_word, lo, hi, _stream()),
          "dfl_grammar_advance")


def gemm_resid(wp, x, N: int, K: int, h_io: torch.Tensor, *, add_residual: bool, ss_out=None, tap=None,
               dyn=None) -> None:
    """h_io [16, >=N] bf16 (unit inner stride) updated in place; tap: optional [16, *] view
    receiving the same rows; ss_out: fp32 [N/16 * 16] partial sums of squares."""
    assert h_io.is_cuda and h_io.dtype == BF16 and h_io.stride(1) == 1
    tp, ldt = None, 0
    if tap is not None:
        assert tap.is_cuda and tap.dtype == BF16 and tap.stride(1) == 1
        tp, ldt = tap.data_ptr(), tap.stride(0)
    if ss_out is not None:
        assert ss_out.numel() >= N
    check(lib().dfl_gemm_resid(_w(wp, N, K, "wp"), _src(x).ref, N, K, h_io.data_ptr(), h_io.stride(0),
                               int(add_residual), tp, ldt, _p(ss_out, F32, "ss_out"), _p(dyn, I32, "dyn"), _stream()),
          "dfl_gemm_resid")


def embed_rows(embed, ids, h_out, H: int, ss_out, dyn=None, dyn_word: int = 0) -> None:
    check(lib().dfl_embed_rows(_p(embed, BF16, "embed"), _p(ids, I64, "ids"), _p(h_out, BF16, "h_out"), H,
                               _p(ss_out, F32, "ss_out"), _p(dyn, I32, "dyn"), dyn_word, _stream()), "dfl_embed_rows")


def norm_pack(*, norm_w, frag, H: int, eps: float, part=None, nsplit=0, part_split=0, ldp=0, row_off=0,
              resid_in=None, embed=None, ids=None, h_out=None, h_out2=None, ld2=0, dyn=None, dyn_word=0) -> None:
    # h_out2 may be a column slice of a wider row-major buffer: only its base pointer and ld2 are used
    p2 = None
    if h_out2 is not None:
        assert h_out2.is_cuda and h_out2.dtype == BF16 and h_out2.stride(-1) == 1
        p2 = h_out2.data_ptr()
    check(lib().dfl_norm_pack(_p(part, F32, "part"), nsplit, part_split, ldp, row_off, _p(resid_in, BF16, "resid_in"),
                              _p(embed, BF16, "embed"), _p(ids, I64, "ids"), _p(h_out, BF16, "h_out"), p2, ld2,
                              _p(norm_w, BF16, "norm_w"), eps, _p(frag, BF16, "frag"), H, _p(dyn, I32, "dyn"),
                              dyn_word, _stream()), "dfl_norm_pack")


def qknorm_rope_append(*, qkv, nsplit, split_stride, ld, q_col, k_col, v_col, ctx_row0, blk_row0, n_q, n_kv,
                       q_norm_w, k_norm_w, eps, cos_tab, sin_tab, q_out, kcache, vcache, dyn,
                       ctx_rows_override=-1, row_base=0) -> None:
    assert kcache.shape == vcache.shape and kcache.dim() == 3 and kcache.shape[2] == 128
    check(lib().dfl_qknorm_rope_append(
        _p(qkv, F32, "qkv"), nsplit, split_stride, ld, q_col, k_col, v_col, ctx_row0, blk_row0, n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"),
        _p(sin_tab, BF16, "sin"), cos_tab.shape[0], _p(q_out, BF16, "q_out"), _p(kcache, BF16, "kcache"),
        _p(vcache, BF16, "vcache"), kcache.shape[1], _p(dyn, I32, "dyn"), ctx_rows_override, row_base, _stream()),
        "dfl_qknorm_rope_append")


def attn_ws(n_q: int, max_splits: int, device) -> torch.Tensor:
    return torch.empty(lib().dfl_attn_ws_bytes(n_q, max_splits), dtype=torch.uint8, device=device)


def block_attn(*, q, kcache, vcache, n_q, n_kv, scale, dyn, kv_len_max, ws, max_splits, out_frag,
               causal: bool = False) -> None:
    check(lib().dfl_block_attn(_p(q, BF16, "q"), _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"),
                               kcache.shape[1], n_q, n_kv, scale, int(causal), _p(dyn, I32, "dyn"), kv_len_max,
                               _p(ws), max_splits, _p(out_frag, BF16, "out_frag"), _stream()), "dfl_block_attn")


def attn_fused_ws(n_q: int, n_kv: int, max_splits: int, device) -> torch.Tensor:
    """Zeroed workspace (split partials + arrival tickets) for attn_fused."""
    return torch.zeros(lib().dfl_attn_fused_ws_bytes(n_q, n_kv, max_splits), dtype=torch.uint8, device=device)


def attn_fused(*, qkv, nsplit, split_stride, ld, q_col, k_col, v_col, ctx_row0, blk_row0, n_q, n_kv, q_norm_w,
               k_norm_w, eps, cos_tab, sin_tab, kcache, vcache, scale, dyn, kv_len_max, ws, max_splits, out_frag,
               causal: bool = False) -> None:
    assert kcache.shape == vcache.shape and kcache.dim() == 3 and kcache.shape[2] == 128
    check(lib().dfl_attn_fused(
        _p(qkv, F32, "qkv"), nsplit, split_stride, ld, q_col, k_col, v_col, ctx_row0, blk_row0, n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"),
        _p(sin_tab, BF16, "sin"), cos_tab.shape[0], _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"),
        kcache.shape[1], scale, int(causal), _p(dyn, I32, "dyn"), kv_len_max, _p(ws), max_splits,
        _p(out_frag, BF16, "out_frag"), _stream()), "dfl_attn_fused")


def attn_head_ws(n_q: int, max_splits: int, q_tiles: int, device) -> torch.Tensor:
    """Zeroed workspace (split partials + arrival tickets) for attn_head."""
    return torch.zeros(lib().dfl_attn_head_ws_bytes(n_q, max_splits, q_tiles), dtype=torch.uint8, device=device)


def attn_head(*, xq: torch.Tensor, q_col: int, k_col: int, v_col: int, n_q: int, n_kv: int, q_norm_w, k_norm_w, eps,
              cos_tab, sin_tab, kcache, vcache, scale: float, causal: bool, S: int, tau: int, bs: int, pos0: int,
              ws, max_splits: int, out_frag: torch.Tensor, xc: Optional[torch.Tensor] = None, ck_col: int = 0,
              cv_col: int = 0, dyn: Optional[torch.Tensor] = None, q_tiles: int = 1, out_tile_stride: int = 0) -> None:
    """xq [>= bs, ldq] bf16 rows (unit inner stride) holding q | k | v of the block rows; xc [>= tau, ldc] the
    context rows' k | v (draft).  dyn given: lengths from the device record, S = bound for the split count."""
    assert xq.is_cuda and xq.dtype == BF16 and xq.dim() == 2 and xq.stride(1) == 1 and xq.shape[0] >= min(bs, 16 * q_tiles)
    assert kcache.shape == vcache.shape and kcache.dim() == 3 and kcache.shape[2] == 128
    xcp, ldc = None, 0
    if xc is not None:
        assert xc.is_cuda and xc.dtype == BF16 and xc.dim() == 2 and xc.stride(1) == 1 and xc.shape[0] >= tau
        xcp, ldc = xc.data_ptr(), xc.stride(0)
    check(lib().dfl_attn_head(
        xq.data_ptr(), xq.stride(0), q_col, k_col, v_col, xcp, ldc, ck_col, cv_col, n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"),
        _p(sin_tab, BF16, "sin"), cos_tab.shape[0], _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"),
        kcache.shape[1], scale, int(causal), _p(dyn, I32, "dyn"), S, tau, bs, pos0, q_tiles, _p(ws), max_splits,
        _p(out_frag, BF16, "out_frag"), out_tile_stride, _stream()), "dfl_attn_head")


ATTN_OPROJ_SYNC_WORDS = 1056   # DFL_ATTN_OPROJ_SYNC_WORDS: 32 counter replicas on their own lines + bookkeeping
ATTN_OPROJ_FAIL_WORD = 1025


def attn_head_oproj(*, xq: torch.Tensor, q_col: int, k_col: int, v_col: int, n_q: int, n_kv: int, q_norm_w, k_norm_w, eps,
                    cos_tab, sin_tab, kcache, vcache, scale: float, causal: bool, S: int, tau: int, bs: int, pos0: int,
                    ws, max_splits: int, attn_frag: torch.Tensor, wo, H: int, h_io: torch.Tensor, ss_out, sync,
                    xc: Optional[torch.Tensor] = None, ck_col: int = 0, cv_col: int = 0,
                    dyn: Optional[torch.Tensor] = None) -> None:
    """attn_head (one query tile) + the o_proj / residual GEMM behind it in one launch; sync: int32[ATTN_OPROJ_SYNC_WORDS],
    zeroed once (sync[ATTN_OPROJ_FAIL_WORD] != 0 afterwards: the launch gave up waiting, h_io is invalid)."""
    assert xq.is_cuda and xq.dtype == BF16 and xq.dim() == 2 and xq.stride(1) == 1 and xq.shape[0] >= min(bs, 16)
    assert kcache.shape == vcache.shape and kcache.dim() == 3 and kcache.shape[2] == 128
    assert h_io.is_cuda and h_io.dtype == BF16 and h_io.stride(1) == 1 and h_io.shape[0] >= 16
    assert sync.dtype == I32 and sync.numel() >= ATTN_OPROJ_SYNC_WORDS and attn_frag.numel() >= 16 * n_q * 128
    assert ss_out is None or ss_out.numel() >= H
    xcp, ldc = None, 0
    if xc is not None:
        assert xc.is_cuda and xc.dtype == BF16 and xc.dim() == 2 and xc.stride(1) == 1 and xc.shape[0] >= tau
        xcp, ldc = xc.data_ptr(), xc.stride(0)
    check(lib().dfl_attn_head_oproj(
        xq.data_ptr(), xq.stride(0), q_col, k_col, v_col, xcp, ldc, ck_col, cv_col, n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"),
        _p(sin_tab, BF16, "sin"), cos_tab.shape[0], _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"),
        kcache.shape[1], scale, int(causal), _p(dyn, I32, "dyn"), S, tau, bs, pos0, _p(ws), max_splits,
        _p(attn_frag, BF16, "attn_frag"), _p(wo, BF16, "wo"), H, h_io.data_ptr(), h_io.stride(0), _p(ss_out, F32, "ss_out"),
        _p(sync, I32, "sync"), _stream()), "dfl_attn_head_oproj")


def attn_head_cand(*, xq: torch.Tensor, q_col: int, k_col: int, v_col: int, n_q: int, n_kv: int, q_norm_w, k_norm_w, eps,
                   cos_tab, sin_tab, kcache, vcache, scale: float, S: int, bs: int, ws, max_splits: int,
                   out_frag: torch.Tensor, k_out: torch.Tensor, v_out: torch.Tensor, q_tiles: int = 1) -> None:
    """xq [tiles, 16, ldq] bf16 candidate block rows; out_frag [tiles, 16*n_q*128]; k_out / v_out [C, n_kv, rows, 128]:
    the candidates' new K/V rows (rows 0..bs-1), NOT written to the cache.  q_tiles = 2 (bs 17..32): candidate c owns tiles
    2 c, 2 c + 1 of xq / out_frag."""
    assert xq.is_cuda and xq.dtype == BF16 and xq.dim() == 3 and xq.stride(2) == 1 and xq.shape[1] >= 16
    assert out_frag.dim() == 2 and out_frag.is_contiguous() and out_frag.shape[0] >= xq.shape[0]
    assert k_out.shape == v_out.shape and k_out.dim() == 4 and k_out.shape[3] == 128 and k_out.is_contiguous()
    assert v_out.is_contiguous() and k_out.shape[0] * q_tiles >= xq.shape[0] and k_out.shape[1] == n_kv
    assert kcache.shape == vcache.shape and kcache.dim() == 3 and kcache.shape[2] == 128
    assert q_tiles == 1 or (xq.shape[0] % q_tiles == 0 and k_out.shape[2] >= bs)
    # one tile per candidate: no tile stride (the kernel's arguments are those of the single-tile form)
    check(lib().dfl_attn_head_cand(
        xq.data_ptr(), xq.stride(1), q_col, k_col, v_col, xq.shape[0] // q_tiles, q_tiles * xq.stride(0), n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"),
        _p(sin_tab, BF16, "sin"), cos_tab.shape[0], _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"),
        kcache.shape[1], scale, S, bs, _p(ws), max_splits, _p(out_frag, BF16, "out_frag"), q_tiles * out_frag.stride(0),
        out_frag.stride(0) if q_tiles != 1 else 0, q_tiles, _p(k_out, BF16, "k_out"), _p(v_out, BF16, "v_out"),
        k_out.stride(0), k_out.shape[2], _stream()), "dfl_attn_head_cand")


def attn_head_batch_ws(R: int, n_q: int, max_splits: int, device, q_tiles: int = 1) -> torch.Tensor:
    return torch.zeros(R * lib().dfl_attn_head_ws_bytes(n_q, max_splits, q_tiles), dtype=torch.uint8, device=device)


def attn_head_batch(*, xq: torch.Tensor, q_col: int, k_col: int, v_col: int, R: int, n_q: int, n_kv: int, q_norm_w,
                    k_norm_w, eps, cos_tab, sin_tab, kcache, vcache, layer: int, scale: float, causal: bool, dyn,
                    kv_len_max: int, ws, max_splits: int, out_frag: torch.Tensor, q_tiles: int = 1) -> None:
    """xq [MT, 16, ldq] bf16; kcache/vcache [requests, L, n_kv, rows, 128] (layer `layer` is used); out_frag
    [MT, 16*n_q*128].  q_tiles = 2: request r owns tiles 2 r, 2 r + 1 of xq / out_frag (blocks of 17..32 rows), dyn holds
    one record per REQUEST."""
    assert xq.is_cuda and xq.dtype == BF16 and xq.dim() == 3 and xq.stride(2) == 1
    assert kcache.shape == vcache.shape and kcache.dim() == 5 and kcache.shape[4] == 128 and kcache.is_contiguous()
    assert out_frag.dim() == 2 and out_frag.is_contiguous()
    kc, vc = kcache[0, layer], vcache[0, layer]
    check(lib().dfl_attn_head_batch(
        xq.data_ptr(), xq.stride(1), q_col, k_col, v_col, R, q_tiles * xq.stride(0), n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"),
        _p(sin_tab, BF16, "sin"), cos_tab.shape[0], kc.data_ptr(), vc.data_ptr(), kcache.shape[3], kcache.stride(0), scale,
        int(causal), _p(dyn, I32, "dyn"), kv_len_max, _p(ws), max_splits, _p(out_frag, BF16, "out_frag"),
        q_tiles * out_frag.stride(0), out_frag.stride(0) if q_tiles != 1 else 0, q_tiles, _stream()), "dfl_attn_head_batch")


def attn_head_batch_f32(*, qkv_parts: torch.Tensor, nparts: int, MT: int, ld: int, q_col: int, k_col: int, v_col: int, R: int,
                        n_q: int, n_kv: int, q_norm_w, k_norm_w, eps, cos_tab, sin_tab, kcache, vcache, layer: int, scale: float,
                        causal: bool, dyn, kv_len_max: int, ws, max_splits: int, out_frag: torch.Tensor) -> None:
    """attn_head_batch on the fp32 K-part sums gemm_f32_batch(N = ld) left in qkv_parts ([nparts][MT * 16][ld] floats):
    the parts meet in the attention launch's row loads (no slab / ticket / combine phase in the GEMM)."""
    assert qkv_parts.is_cuda and qkv_parts.dtype == F32 and qkv_parts.is_contiguous() and qkv_parts.numel() >= nparts * MT * 16 * ld
    assert kcache.shape == vcache.shape and kcache.dim() == 5 and kcache.shape[4] == 128 and kcache.is_contiguous()
    assert out_frag.dim() == 2 and out_frag.is_contiguous()
    kc, vc = kcache[0, layer], vcache[0, layer]
    check(lib().dfl_attn_head_batch_f32(
        qkv_parts.data_ptr(), nparts, MT * 16 * ld, ld, q_col, k_col, v_col, R, 16 * ld, n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"), _p(sin_tab, BF16, "sin"),
        cos_tab.shape[0], kc.data_ptr(), vc.data_ptr(), kcache.shape[3], kcache.stride(0), scale, int(causal),
        _p(dyn, I32, "dyn"), kv_len_max, _p(ws), max_splits, _p(out_frag, BF16, "out_frag"), out_frag.stride(0), _stream()),
        "dfl_attn_head_batch_f32")


def topk_rows(logits: torch.Tensor, k: int):
    """logits bf16 [rows, V] (unit inner stride) -> (values fp32 [rows, 8], indices int32 [rows, 8], lse fp32 [rows]);
    columns >= k are unspecified.  Order: value descending, index ascending."""
    assert logits.is_cuda and logits.dtype == BF16 and logits.dim() == 2 and logits.stride(1) == 1
    rows, V = logits.shape
    val = torch.empty(rows, 8, dtype=F32, device=logits.device)
    idx = torch.empty(rows, 8, dtype=I32, device=logits.device)
    lse = torch.empty(rows, dtype=F32, device=logits.device)
    check(lib().dfl_topk_rows(logits.data_ptr(), logits.stride(0), rows, V, k, _p(val), _p(idx), _p(lse), _stream()),
          "dfl_topk_rows")
    return val, idx, lse


def candidate_select(blocks: torch.Tensor, posterior: torch.Tensor, scores: torch.Tensor, bs: int, output_ids, dyn,
                     stop_ids, result: torch.Tensor) -> None:
    """blocks / posterior int64 [C, >= bs]; scores fp32 [C]; result int32 [12]."""
    assert blocks.dim() == 2 and posterior.dim() == 2 and blocks.stride(1) == 1 and posterior.stride(1) == 1
    assert result.numel() >= 12 and scores.numel() >= blocks.shape[0]
    n_stop = 0 if stop_ids is None else stop_ids.numel()
    check(lib().dfl_candidate_select(
        _p(blocks[0], I64, "blocks"), blocks.stride(0), _p(posterior[0], I64, "posterior"), posterior.stride(0),
        _p(scores, F32, "scores"), blocks.shape[0], bs, _p(output_ids, I64, "output_ids"), output_ids.numel(),
        _p(dyn, I32, "dyn"), _p(stop_ids, I64, "stop_ids") if n_stop else None, n_stop, _p(result, I32, "result"),
        _stream()), "dfl_candidate_select")


# ---- sparse-MoE MLP of a target verify (include/dflash_hip.h, moe section) ----------------------------------------
def moe_route(logits: torch.Tensor, E: int, top_k: int, norm_topk: bool, wt: torch.Tensor, active: torch.Tensor,
              lst: torch.Tensor, n_active: torch.Tensor, dyn=None, dyn_word: int = 0) -> None:
    """logits bf16 [16, >= E]; wt bf16 [16, E]; active / lst int32 [E]; n_active int32 [1]."""
    assert logits.dtype == BF16 and logits.dim() == 2 and logits.stride(1) == 1 and logits.shape[0] >= 16
    assert wt.dtype == BF16 and wt.is_contiguous() and wt.numel() >= 16 * E
    check(lib().dfl_moe_route(logits.data_ptr(), logits.stride(0), E, top_k, int(norm_topk), _p(wt), _p(active, I32, "active"),
                              _p(lst, I32, "list"), _p(n_active, I32, "n_active"), _p(dyn, I32, "dyn"), dyn_word,
                              _stream()), "dfl_moe_route")


def moe_router(*, h: Optional[torch.Tensor], norm_w: Optional[torch.Tensor], eps: float, xn: torch.Tensor, wp_router: torch.Tensor,
               K: int, E: int, top_k: int, norm_topk: bool, rlog: torch.Tensor, wt: torch.Tensor, active: torch.Tensor,
               lst: torch.Tensor, n_active: torch.Tensor, ticket: torch.Tensor, dyn=None, dyn_word: int = 0) -> None:
    """RMSNorm (h [16, >= K] rows -> xn frag16; h None: xn is the input) + gate Linear + moe_route in one launch.
    rlog bf16 [16, ld]; ticket int32 [1], zero."""
    assert rlog.dtype == BF16 and rlog.dim() == 2 and rlog.stride(1) == 1 and rlog.shape[0] >= 16
    assert wt.dtype == BF16 and wt.is_contiguous() and wt.numel() >= 16 * E and xn.numel() >= 16 * K
    hp, ldh = None, 0
    if h is not None:
        assert h.is_cuda and h.dtype == BF16 and h.dim() == 2 and h.stride(1) == 1 and h.shape[0] >= 16 and h.shape[1] >= K
        hp, ldh = h.data_ptr(), h.stride(0)
    check(lib().dfl_moe_router(hp, ldh, _p(norm_w, BF16, "norm_w"), eps, _p(xn, BF16, "xn"), _p(wp_router, BF16, "wp_router"), K, E,
                               top_k, int(norm_topk), rlog.data_ptr(), rlog.stride(0), _p(wt), _p(active, I32, "active"),
                               _p(lst, I32, "list"), _p(n_active, I32, "n_active"), _p(dyn, I32, "dyn"), dyn_word,
                               _p(ticket, I32, "ticket"), _stream()), "dfl_moe_router")


def gemm_silu_mul_experts(wp_gu: torch.Tensor, x, E: int, I: int, K: int, act: torch.Tensor, lst: torch.Tensor,
                          n_active: torch.Tensor, dyn=None) -> None:
    """wp_gu bf16 [E, 2*I*K] packed per expert; act bf16 [E, 16*I] (frag16 per expert); lst / n_active: the active
    experts (dfl_moe_route).  Only their outputs are written."""
    assert wp_gu.dim() == 2 and wp_gu.is_contiguous() and act.dim() == 2 and act.is_contiguous()
    check(lib().dfl_gemm_silu_mul_experts(_p(wp_gu, BF16, "wp_gu"), wp_gu.stride(0), _src(x).ref, E, I, K,
                                          _p(act, BF16, "act"), act.stride(0), _p(lst, I32, "list"),
                                          _p(n_active, I32, "n_active"), _p(dyn, I32, "dyn"), _stream()),
          "dfl_gemm_silu_mul_experts")


def moe_gate_up(wp_gu: torch.Tensor, x_frag: torch.Tensor, E: int, I: int, K: int, act: torch.Tensor, lst: torch.Tensor,
                n_active: torch.Tensor, dyn=None, valid_word: int = -1) -> None:
    """gemm_silu_mul_experts for K <= 2048 from frag16 rows: one LDS meeting per (gate, up) tile pair.  wp_gu: packed
    bf16 [E, 2*I*K], an Fp8Experts, or (K = 2048) the Bf16x13Weight of that packed tensor as ONE matrix of E * 2I x K
    (pack_weight_bf16x13: the experts' tiles back to back) — the same bits as the packed tensor gives."""
    assert act.dim() == 2 and act.is_contiguous() and act.shape[1] == 16 * I and x_frag.numel() >= 16 * K
    if isinstance(wp_gu, Bf16x13Weight):
        w = _w(wp_gu, E * 2 * I, K, "wp_gu")
    else:
        w, rows = _we(wp_gu, E, 2 * I, K, "wp_gu")
        assert rows.shape[1] == 2 * I * K
    check(lib().dfl_moe_gate_up(w, _p(x_frag, BF16, "x_frag"), E, I, K, _p(act, BF16, "act"), _p(lst, I32, "list"),
                                _p(n_active, I32, "n_active"), _p(dyn, I32, "dyn"), valid_word, _stream()),
          "dfl_moe_gate_up")


def moe_down(wp_down: torch.Tensor, act: torch.Tensor, wt: torch.Tensor, lst: torch.Tensor, n_active: torch.Tensor, E: int,
             N: int, I: int, nsplit: int, out: torch.Tensor) -> None:
    """wp_down bf16 [E, N*I] packed per expert, or an Fp8Experts; out fp32 [nsplit, 16, N]."""
    assert act.dim() == 2 and act.is_contiguous()
    assert out.dtype == F32 and out.is_contiguous() and out.numel() >= nsplit * 16 * N
    w, rows = _we(wp_down, E, N, I, "wp_down")
    check(lib().dfl_moe_down(w, rows.stride(0), _p(act, BF16, "act"), act.stride(0), _p(wt, BF16, "wt"),
                             _p(lst, I32, "list"), _p(n_active, I32, "n_active"), E, N, I, nsplit, _p(out, F32, "out"),
                             _stream()), "dfl_moe_down")


def argmax(logits: torch.Tensor) -> torch.Tensor:
    """First-max-index argmax over the last axis, int64 (model/utils.py:28-29)."""
    if logits.dtype not in (BF16, F32):
        raise TypeError(f"dflash_amd.argmax: bf16 or fp32 logits, got {logits.dtype}")
    x = logits.contiguous()
    v = x.shape[-1]
    rows = x.numel() // v
    out = torch.empty(x.shape[:-1], dtype=I64, device=x.device)
    check(lib().dfl_argmax(_p(x), 0 if x.dtype == BF16 else 1, rows, v, _p(out), _stream()), "dfl_argmax")
    return out


def accept_commit(block_ids, posterior, bs: int, output_ids, dyn, stop_ids=None, result=None, rearm=None, dyn_t=None) -> None:
    """result: int32[4] on the GPU, or PINNED host memory (the kernel stores the four words with one 16-byte store, a
    CPU thread may poll them).  rearm = (next_block int64 tensor, n, mask_id): the next cycle's block is written by
    the kernel; dyn_t: the next verify's block-form record is kept on the device too (graph replay).  dyn_t without
    rearm is an error (the library refuses it): the record is kept by the re-arming launch only."""
    n_stop = 0 if stop_ids is None else stop_ids.numel()
    rp = None
    if result is not None:
        assert result.numel() >= 4 and result.dtype == I32
        if result.is_cuda:
            rp = _p(result, I32, "result")
        else:
            if not result.is_pinned():
                raise RuntimeError("dflash_amd: a host-side result buffer must be pinned memory")
            rp = result.data_ptr()
    nb, n, mask_id = (None, 0, 0) if rearm is None else rearm
    assert nb is None or nb.numel() >= n
    check(lib().dfl_accept_commit(_p(block_ids, I64, "block_ids"), _p(posterior, I64, "posterior"), bs,
                                  _p(output_ids, I64, "output_ids"), output_ids.numel(), _p(dyn, I32, "dyn"),
                                  _p(stop_ids, I64, "stop_ids") if n_stop else None, n_stop, rp, _p(nb, I64, "next_block"),
                                  int(n), int(mask_id), _p(dyn_t, I32, "dyn_t"), _stream()), "dfl_accept_commit")


# ---- stop sequences (csrc/stop_seq.hip)
STOP_SEQS, STOP_SEQ_LEN = 8, 16   # DFL_STOP_SEQS, DFL_STOP_SEQ_LEN


def check_stop_sequences(seqs, V: int, mask_token_id: Optional[int] = None):
    """Normalise one request's stop sequences to a list of lists of ints (a bare int: a sequence of length 1); None for
    None or an empty list — the path without the feature.  ValueError, before anything touches the GPU: an empty
    sequence, more than 8 sequences, a sequence longer than 16, an id outside [0, V), the mask id inside a sequence."""
    import operator
    if seqs is None:
        return None
    if isinstance(seqs, (str, bytes)) or not hasattr(seqs, "__iter__"):
        raise ValueError(f"dflash_amd: stop_sequences must be a list of token-id sequences, got {seqs!r}")
    out = []
    for k, s in enumerate(seqs):
        if torch.is_tensor(s):
            s = s.tolist()
        if isinstance(s, (str, bytes)):
            raise ValueError(f"dflash_amd: stop_sequences[{k}]: {s!r} is text; token ids are what is matched")
        if not hasattr(s, "__iter__"):
            s = [s]
        ids = []
        for v in s:
            try:
                i = operator.index(v)
            except TypeError:
                raise ValueError(f"dflash_amd: stop_sequences[{k}]: {v!r} is not a token id") from None
            if not 0 <= i < V:
                raise ValueError(f"dflash_amd: stop_sequences[{k}]: id {i} outside [0, {V})")
            if mask_token_id is not None and i == int(mask_token_id):
                raise ValueError(f"dflash_amd: stop_sequences[{k}] holds the mask id {i}, which is never committed")
            ids.append(i)
        if not ids:
            raise ValueError(f"dflash_amd: stop_sequences[{k}] is empty")
        if len(ids) > STOP_SEQ_LEN:
            raise ValueError(f"dflash_amd: stop_sequences[{k}] has {len(ids)} ids, more than {STOP_SEQ_LEN}")
        out.append(ids)
    if len(out) > STOP_SEQS:
        raise ValueError(f"dflash_amd: {len(out)} stop sequences, more than {STOP_SEQS}")
    return out or None


def stop_seq_state(slots: int, device) -> SimpleNamespace:
    """The stop-sequence state, one row per request slot: .seq_ids int32 [slots, 8, 16], .seq_len
    int32 [slots, 8] (0: unused), .first_pos / .min_end int32 [slots], .hit int32 [slots, 2] ({-1, -1}: no match yet).
    Written by stop_seq_set, read (hit: written) by stop_seq_rows."""
    if slots < 1:
        raise ValueError(f"dflash_amd: stop_seq_state: slots={slots} < 1")
    return SimpleNamespace(seq_ids=torch.zeros(slots, STOP_SEQS, STOP_SEQ_LEN, dtype=I32, device=device),
                           seq_len=torch.zeros(slots, STOP_SEQS, dtype=I32, device=device),
                           first_pos=torch.zeros(slots, dtype=I32, device=device),
                           min_end=torch.zeros(slots, dtype=I32, device=device),
                           hit=torch.full((slots, 2), -1, dtype=I32, device=device))


def stop_seq_set(state, slot: int, seqs, first_pos: int = 0, min_end: int = 0) -> None:
    """Rewrite slot's rows whole: its sequences (a list of lists of ints as check_stop_sequences returns it; None: none),
    first_pos (the first position a window may cover: the prompt's length), min_end (no match ends before it; 0: off)
    and hit <- {-1, -1}: nothing of the slot's previous request survives.  Admission only, plain copies."""
    slots = state.seq_len.shape[0]
    if not 0 <= slot < slots:
        raise ValueError(f"dflash_amd: stop_seq_set: slot {slot} outside 0..{slots - 1}")
    seqs = seqs or []
    if len(seqs) > STOP_SEQS or any(not 1 <= len(s) <= STOP_SEQ_LEN for s in seqs):
        raise ValueError("dflash_amd: stop_seq_set: at most 8 sequences of 1..16 ids (check_stop_sequences)")
    ids = torch.zeros(STOP_SEQS, STOP_SEQ_LEN, dtype=I32)
    lens = torch.zeros(STOP_SEQS, dtype=I32)
    for k, s in enumerate(seqs):
        ids[k, :len(s)] = torch.tensor(s, dtype=I32)
        lens[k] = len(s)
    state.seq_ids[slot].copy_(ids)
    state.seq_len[slot].copy_(lens)
    state.first_pos[slot:slot + 1].fill_(int(first_pos))
    state.min_end[slot:slot + 1].fill_(int(min_end))
    state.hit[slot].fill_(-1)


def stop_seq_rows(block: torch.Tensor, posterior: torch.Tensor, output_ids: torch.Tensor, dyn: torch.Tensor, state,
                  bs: Optional[int] = None, slots: Optional[int] = None, output_len: Optional[int] = None) -> None:
    """Match every slot's stop sequences over the tokens the accept launch behind this one is about to commit
    (dfl_stop_seq_rows): block / posterior int64 [slots, >= bs] (or 1-D for one slot), output_ids int64 [slots, n] (or
    1-D), dyn the int32 length records [slots, 8] the accept launch reads (the ragged batch: dyn_d).  bs None: every
    slot's own DFL_DYN_BS word.  slots None: all of the state's.  A match ORs 1 into the slot's stop word and, the first
    time, stores {end position, sequence index} in state.hit."""
    if block.dim() == 1:
        block, posterior = block.unsqueeze(0), posterior.unsqueeze(0)
    if output_ids.dim() == 1:
        output_ids = output_ids.unsqueeze(0)
    if slots is None:
        slots = state.seq_len.shape[0]
    assert 1 <= slots <= state.seq_len.shape[0], "slots"
    assert block.dim() == 2 and posterior.dim() == 2 and output_ids.dim() == 2
    assert block.stride(1) == 1 and posterior.stride(1) == 1 and output_ids.stride(1) == 1
    assert block.shape[0] >= slots and posterior.shape[0] >= slots and output_ids.shape[0] >= slots, "one row per slot"
    assert dyn.numel() >= 8 * slots and dyn.is_contiguous(), "dyn"
    assert state.seq_ids.is_contiguous() and state.seq_len.is_contiguous() and state.hit.is_contiguous()
    out_len = output_ids.shape[1] if output_len is None else int(output_len)
    assert 1 <= out_len <= output_ids.shape[1]
    # (one slot: its row's length stands for the stride, which nothing is addressed by)
    one = slots == 1
    check(lib().dfl_stop_seq_rows(_p(block, I64, "block"), block.shape[1] if one else block.stride(0),
                                  _p(posterior, I64, "posterior"), posterior.shape[1] if one else posterior.stride(0),
                                  _p(output_ids, I64, "output_ids"), output_ids.shape[1] if one else output_ids.stride(0),
                                  out_len, _p(dyn, I32, "dyn"), slots, -1 if bs is None else int(bs),
                                  _p(state.seq_ids, I32, "seq_ids"), _p(state.seq_len, I32, "seq_len"),
                                  _p(state.first_pos, I32, "first_pos"), _p(state.min_end, I32, "min_end"),
                                  _p(state.hit, I32, "hit"), _stream()), "dfl_stop_seq_rows")


# ---- ragged batch of requests (include/dflash_hip.h, second half) ---------------------------
from ._lib import RowsBatch  # noqa: E402


def batch_tiles(R: int) -> int:
    return lib().dfl_batch_tiles(R)


def batch_ksplit(K: int) -> int:
    return lib().dfl_batch_ksplit(K)


class BatchRowSource:
    def __init__(self, struct: RowsBatch, *keep):
        self.struct, self.keep = struct, keep

    @property
    def ref(self):
        return _C.byref(self.struct)


def brows_frag(frag: torch.Tensor) -> BatchRowSource:
    """frag [MT, 16*K] bf16: request r's frag16 buffer is frag[r]."""
    assert frag.dim() == 2 and frag.is_contiguous()
    r0 = Rows(_p(frag, BF16, "frag"), None, 0, None, 0, None, 0.0, -1, 0)
    return BatchRowSource(RowsBatch(r0, frag.stride(0), 0, 0), frag)


def brows_plain(rows: torch.Tensor, valid_word: int = -1) -> BatchRowSource:
    """rows [MT, 16, K] bf16 (unit inner stride)."""
    assert rows.is_cuda and rows.dtype == BF16 and rows.dim() == 3 and rows.stride(2) == 1
    r0 = Rows(None, rows.data_ptr(), rows.stride(1), None, 0, None, 0.0, valid_word, 1)
    return BatchRowSource(RowsBatch(r0, 0, rows.stride(0), 0), rows)


def brows_normed(rows: torch.Tensor, ss: torch.Tensor, nss: int, norm_w: torch.Tensor, eps: float,
                 valid_word: int = -1) -> BatchRowSource:
    """rows [MT, 16, K] + ss [MT, >= nss*16] as a mode-2 source.  The batched GEMMs REJECT it
    (normalised rows come from norm_frag_batch); kept so that the rejection can be tested."""
    assert rows.is_cuda and rows.dtype == BF16 and rows.dim() == 3 and rows.stride(2) == 1
    assert ss.dim() == 2 and ss.shape[1] >= nss * 16 and ss.stride(1) == 1
    r0 = Rows(None, rows.data_ptr(), rows.stride(1), _p(ss[0], F32, "ss"), nss, _p(norm_w, BF16, "norm_w"), eps,
              valid_word, 2)
    return BatchRowSource(RowsBatch(r0, 0, rows.stride(0), ss.stride(0)), rows, ss, norm_w)


def gemm_batch_ws(N: int, K: int, device) -> torch.Tensor:
    return torch.zeros(lib().dfl_gemm_batch_ws_bytes(N, K), dtype=torch.uint8, device=device)


def gemm_f32_batch(wp, x: BatchRowSource, R: int, N: int, K: int, out: torch.Tensor, dyn) -> None:
    assert out.numel() >= batch_ksplit(K) * batch_tiles(R) * 16 * N
    # (an Fp8Weight: every K part comes out scaled, the launch that sums them takes it as it is)
    check(lib().dfl_gemm_f32_batch(_w(wp, N, K, "wp"), x.ref, R, N, K, _p(out, F32, "out"), _p(dyn, I32, "dyn"),
                                   _stream()), "dfl_gemm_f32_batch")


def gemm_silu_mul_batch(wp_gu, x: BatchRowSource, R: int, I: int, K: int, act: torch.Tensor, ws, dyn) -> None:
    assert act.dim() == 2 and act.shape[1] >= 16 * I and act.shape[0] >= batch_tiles(R)
    # (an Fp8Weight runs the ring form only, here and in the two below: a plain-row source is an error, not a fall-back)
    check(lib().dfl_gemm_silu_mul_batch(_w(wp_gu, 2 * I, K, "wp_gu"), x.ref, R, I, K, _p(act, BF16, "act"), act.stride(0),
                                        _p(ws), _p(dyn, I32, "dyn"), _stream()), "dfl_gemm_silu_mul_batch")


def gemm_resid_batch(wp, x: BatchRowSource, R: int, N: int, K: int, h_io: torch.Tensor, *, add_residual: bool,
                     ws, dyn, ss_out=None, tap=None) -> None:
    """h_io [MT, 16, >=N]; tap: optional [MT, 16, *] view; ss_out [MT, >=N]."""
    assert h_io.is_cuda and h_io.dtype == BF16 and h_io.dim() == 3 and h_io.stride(2) == 1
    tp, ldt, tst = None, 0, 0
    if tap is not None:
        assert tap.is_cuda and tap.dtype == BF16 and tap.dim() == 3 and tap.stride(2) == 1
        tp, ldt, tst = tap.data_ptr(), tap.stride(1), tap.stride(0)
    sp, sst = None, 0
    if ss_out is not None:
        assert ss_out.dim() == 2 and ss_out.shape[1] >= N and ss_out.dtype == F32
        sp, sst = ss_out.data_ptr(), ss_out.stride(0)
    check(lib().dfl_gemm_resid_batch(_p(wp, BF16, "wp"), x.ref, R, N, K, h_io.data_ptr(), h_io.stride(1),
                                     h_io.stride(0), int(add_residual), tp, ldt, tst, sp, sst, _p(ws),
                                     _p(dyn, I32, "dyn"), _stream()), "dfl_gemm_resid_batch")


def gemm_argmax_batch(wp, x: BatchRowSource, R: int, V: int, K: int, row0: int, nrows: int, ws,
                      out_ids: torch.Tensor, out_off: int, dyn, nrows_dyn_word: int = -1,
                      logits: Optional[torch.Tensor] = None) -> None:
    """out_ids int64 [MT, n]: ids of request r's rows row0.. at out_ids[r, out_off..]."""
    assert out_ids.dim() == 2 and out_ids.dtype == I64 and out_ids.stride(1) == 1
    lp, lst = None, 0
    if logits is not None:
        assert logits.dim() == 3 and logits.shape[1] == 16 and logits.shape[2] == V and logits.is_contiguous()
        lp, lst = _p(logits, BF16, "logits"), logits.stride(0)
    check(lib().dfl_gemm_argmax_batch(_w(wp, V, K, "wp"), x.ref, R, V, K, row0, nrows, _p(dyn, I32, "dyn"),
                                      nrows_dyn_word, _p(ws), out_ids.data_ptr(), out_ids.stride(0), out_off, lp, lst,
                                      _stream()), "dfl_gemm_argmax_batch")


def seed_i64(seed: int) -> int:
    """A 64-bit seed as the int64 a device seed array holds (same bits)."""
    s = _seed64(seed)
    return s - (1 << 64) if s >= (1 << 63) else s


def gemm_sample_batch(wp, x: BatchRowSource, R: int, V: int, K: int, row0: int, nrows: int, ws,
                      out_ids: torch.Tensor, out_off: int, dyn, *, seeds: torch.Tensor, temperature: Optional[float] = None,
                      stream: int = RNG_TARGET, pos_word: int = DYN_POS0, pos_add: int = 0, tiles_per_req: int = 1,
                      nrows_dyn_word: int = -1, logits: Optional[torch.Tensor] = None,
                      inv_ts: Optional[torch.Tensor] = None) -> None:
    """gemm_argmax_batch with the seeded draw (dfl_gemm_sample_batch): tile t (tile j = t % tiles_per_req of request
    q = t // tiles_per_req) row m draws position dyn[t][pos_word] + pos_add + 16 j + m with seed seeds[q] (int64).
    Either `temperature` (one host value for the launch) or inv_ts: a device fp32 tensor of invT per request slot q, a
    slot whose value is not > 0 taking gemm_argmax_batch's plain argmax."""
    if (temperature is None) == (inv_ts is None):
        raise ValueError("gemm_sample_batch: give either temperature or inv_ts")
    assert out_ids.dim() == 2 and out_ids.dtype == I64 and out_ids.stride(1) == 1
    mt = batch_tiles(R)
    assert dyn is not None and dyn.numel() >= 8 * mt and seeds.numel() >= mt // tiles_per_req
    lp, lst = None, 0
    if logits is not None:
        assert logits.dim() == 3 and logits.shape[1] == 16 and logits.shape[2] == V and logits.is_contiguous()
        lp, lst = _p(logits, BF16, "logits"), logits.stride(0)
    if inv_ts is not None:
        assert inv_ts.numel() >= mt // tiles_per_req, "inv_ts"
    check(lib().dfl_gemm_sample_batch(_w(wp, V, K, "wp"), x.ref, R, V, K, row0, nrows, _p(dyn, I32, "dyn"), nrows_dyn_word,
                                      _p(ws), out_ids.data_ptr(), out_ids.stride(0), out_off, lp, lst,
                                      _p(seeds, I64, "seeds"), _p(inv_ts, F32, "inv_ts"),
                                      0.0 if inv_ts is not None else inv_temperature(temperature), stream, pos_word,
                                      pos_add, tiles_per_req, _stream()), "dfl_gemm_sample_batch")


def embed_rows_batch(embed, ids: torch.Tensor, R: int, h_out: torch.Tensor, H: int, ss_out: torch.Tensor, dyn,
                     dyn_word: int) -> None:
    assert ids.dim() == 2 and ids.dtype == I64 and ids.stride(1) == 1 and h_out.dim() == 3 and ss_out.dim() == 2
    check(lib().dfl_embed_rows_batch(_p(embed, BF16, "embed"), ids.data_ptr(), ids.stride(0), R, h_out.data_ptr(),
                                     h_out.stride(0), H, ss_out.data_ptr(), ss_out.stride(0), _p(dyn, I32, "dyn"),
                                     dyn_word, _stream()), "dfl_embed_rows_batch")


def norm_frag_batch(h: torch.Tensor, R: int, norm_w: torch.Tensor, eps: float, frag: torch.Tensor, dyn,
                    dyn_word: int, part: Optional[torch.Tensor] = None, N: int = 0, K: int = 0,
                    tap: Optional[torch.Tensor] = None, nsplit: Optional[int] = None) -> None:
    """h [MT, 16, H] -> frag [MT, 16*H] = frag16 of the RMS-normalised rows.  part: the fp32
    partial sums gemm_f32_batch(N=H, K) left ([ksplit][MT*16][H]): added to h first (residual
    add, in place); tap: optional [MT, 16, *] view receiving the new rows."""
    assert h.dim() == 3 and h.stride(2) == 1 and frag.dim() == 2 and frag.is_contiguous()
    H = h.shape[2]
    pp, ns, ps, ldp = None, 0, 0, 0
    if part is not None:
        assert N == H and (K > 0 or nsplit)
        ns, ldp = (nsplit if nsplit else batch_ksplit(K)), N   # nsplit: partial sums that are not a K split (MoE expert shares)
        ps = batch_tiles(R) * 16 * N
        assert part.numel() >= ns * ps
        pp = _p(part, F32, "part")
    tp, ldt, tst = None, 0, 0
    if tap is not None:
        assert tap.is_cuda and tap.dtype == BF16 and tap.dim() == 3 and tap.stride(2) == 1
        tp, ldt, tst = tap.data_ptr(), tap.stride(1), tap.stride(0)
    check(lib().dfl_norm_frag_batch(_p(h[0, 0], BF16, "h"), h.stride(0), h.stride(1), R, pp, ns, ps, ldp, tp, ldt, tst,
                                    _p(norm_w, BF16, "norm_w"), eps, _p(frag, BF16, "frag"), frag.stride(0), H,
                                    _p(dyn, I32, "dyn"), dyn_word, _stream()), "dfl_norm_frag_batch")


def kv_append_batch(*, kv, nsplit, split_stride, ld, k_col, v_col, col_layer_stride, n_layers, R, n_kv, k_norm_w,
                    eps, cos_tab, sin_tab, kcache, vcache, dyn, tiles_per_req: int = 1) -> None:
    """kcache/vcache [MT, L, n_kv, rows, 128]; k_norm_w [L, 128] or None.  A 4-D cache [L, n_kv, rows, 128] is ONE
    request's cache shared by all R tiles (request stride 0): the tiles are then consecutive 16-row groups of that
    request's context rows (the large-M context prefill), each with its own S / pos0 in its dyn record."""
    assert kcache.shape == vcache.shape and kcache.shape[-1] == 128 and kcache.is_contiguous() and vcache.is_contiguous()
    if kcache.dim() == 4:
        rows, req_stride, layer_stride = kcache.shape[2], 0, kcache.stride(0)
    else:
        assert kcache.dim() == 5
        rows, req_stride, layer_stride = kcache.shape[3], kcache.stride(0), kcache.stride(1)
    # R counts tiles, dyn holds one record per tile, tiles_per_req tiles share a request's cache
    check(lib().dfl_kv_append_batch(
        _p(kv, F32, "kv"), nsplit, split_stride, ld, k_col, v_col, col_layer_stride, n_layers, R, 16, n_kv,
        _p(k_norm_w, BF16, "k_norm_w"), 128, eps, _p(cos_tab, BF16, "cos"), _p(sin_tab, BF16, "sin"),
        cos_tab.shape[0], _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"), rows,
        req_stride, layer_stride, _p(dyn, I32, "dyn"), tiles_per_req, _stream()), "dfl_kv_append_batch")


def attn_fused_batch_ws(R: int, n_q: int, n_kv: int, max_splits: int, device) -> torch.Tensor:
    return torch.zeros(lib().dfl_attn_fused_batch_ws_bytes(R, n_q, n_kv, max_splits), dtype=torch.uint8,
                       device=device)


def attn_fused_batch(*, qkv, nsplit, split_stride, ld, q_col, k_col, v_col, R, n_q, n_kv, q_norm_w, k_norm_w, eps,
                     cos_tab, sin_tab, kcache, vcache, layer: int, scale, causal: bool, dyn, kv_len_max, ws,
                     max_splits, out_frag) -> None:
    """kcache/vcache [MT, L, n_kv, rows, 128] (layer `layer` is used); out_frag [MT, 16*n_q*128]."""
    assert kcache.shape == vcache.shape and kcache.dim() == 5 and kcache.shape[4] == 128 and kcache.is_contiguous()
    assert out_frag.dim() == 2 and out_frag.is_contiguous()
    kc, vc = kcache[0, layer], vcache[0, layer]
    check(lib().dfl_attn_fused_batch(
        _p(qkv, F32, "qkv"), nsplit, split_stride, ld, q_col, k_col, v_col, 0, 16, R, n_q, n_kv,
        _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps, _p(cos_tab, BF16, "cos"),
        _p(sin_tab, BF16, "sin"), cos_tab.shape[0], kc.data_ptr(), vc.data_ptr(), kcache.shape[3], kcache.stride(0),
        scale, int(causal), _p(dyn, I32, "dyn"), kv_len_max, _p(ws), max_splits, _p(out_frag, BF16, "out_frag"),
        out_frag.stride(0), _stream()), "dfl_attn_fused_batch")


def accept_commit_batch(block: torch.Tensor, posterior: torch.Tensor, R: int, output_ids: torch.Tensor, dyn_d, dyn_t,
                        stop_ids, result: torch.Tensor, rearm_mask_id: Optional[int] = None, tiles_per_req: int = 1,
                        dyn_d_tiles=None, dyn_t_tiles=None, next_block: Optional[torch.Tensor] = None,
                        output_len: Optional[int] = None) -> None:
    """block/posterior int64 [requests, 16 * tiles_per_req]; output_ids int64 [requests, n]; result int32 [requests, 4];
    tiles_per_req = 2: the per-tile records dyn_d_tiles / dyn_t_tiles are kept as well (with one tile per request they are not
    handed over: they may be the per-request records themselves).
    rearm_mask_id: the next block is re-armed, in `block` itself or in next_block (same row stride as block).
    output_len: ids per request the kernel may write (default: the whole row of output_ids)."""
    assert block.dim() == 2 and posterior.dim() == 2 and output_ids.dim() == 2
    n_stop = 0 if stop_ids is None else stop_ids.numel()
    out_len = output_ids.shape[1] if output_len is None else int(output_len)
    assert 0 <= out_len <= output_ids.shape[1]
    nb = None
    if rearm_mask_id is not None:
        nb = block.data_ptr()
        if next_block is not None:
            assert next_block.dim() == 2 and next_block.stride(0) == block.stride(0) and next_block.shape[0] >= R
            nb = _p(next_block, I64, "next_block")
    else:
        assert next_block is None, "next_block needs rearm_mask_id"
    tiled = tiles_per_req != 1
    check(lib().dfl_accept_commit_batch(
        _p(block, I64, "block"), block.stride(0), _p(posterior, I64, "posterior"), posterior.stride(0), R,
        _p(output_ids, I64, "output_ids"), output_ids.stride(0), out_len, _p(dyn_d, I32, "dyn_d"),
        _p(dyn_t, I32, "dyn_t"), _p(stop_ids, I64, "stop_ids") if n_stop else None, n_stop,
        _p(result, I32, "result"), nb, int(rearm_mask_id) if rearm_mask_id is not None else 0, tiles_per_req,
        _p(dyn_d_tiles, I32, "dyn_d_tiles") if tiled else None, _p(dyn_t_tiles, I32, "dyn_t_tiles") if tiled else None,
        _stream()), "dfl_accept_commit_batch")


def admit_slot(r: int, prompt_ids: torch.Tensor, first_token: torch.Tensor, output_ids: torch.Tensor, block: torch.Tensor,
               post: torch.Tensor, result: torch.Tensor, tail_rows: torch.Tensor, taps: torch.Tensor, dyn_d: torch.Tensor,
               dyn_t: torch.Tensor, bs: int, mask_id: int, seeds: Optional[torch.Tensor] = None, seed: int = 0) -> None:
    """Re-arm request slot r of a ragged batch in one launch (dfl_admit_slot): prompt_ids int64 [P], first_token int64 [1]
    (device), output_ids int64 [slots, n], block / post int64 [slots, w], result int32 [slots, 4], tail_rows bf16
    [n_tail <= 16, fc_in] (the prompt's last tapped rows), taps bf16 [tiles, 16, fc_in], dyn_d / dyn_t int32 [slots, 8],
    seeds int64 [slots] or None (the slot's seed is left alone)."""
    n_slots = output_ids.shape[0]
    assert prompt_ids.dim() == 1 and first_token.numel() == 1 and output_ids.dim() == 2 and tail_rows.dim() == 2
    assert block.shape == post.shape and block.shape[0] >= n_slots and result.shape[0] >= n_slots and result.shape[1] == 4
    assert taps.dim() == 3 and taps.shape[0] >= n_slots and taps.shape[1] == 16 and taps.shape[2] == tail_rows.shape[1]
    assert dyn_d.shape[0] >= n_slots and dyn_t.shape[0] >= n_slots and dyn_d.shape[1] == 8 and dyn_t.shape[1] == 8
    assert tail_rows.dtype == BF16 and tail_rows.is_cuda and tail_rows.stride(1) == 1
    assert seeds is None or seeds.numel() >= n_slots
    check(lib().dfl_admit_slot(
        r, n_slots, _p(prompt_ids, I64, "prompt_ids"), prompt_ids.shape[0], _p(first_token, I64, "first_token"),
        _p(output_ids, I64, "output_ids"), output_ids.stride(0), output_ids.shape[1], _p(block, I64, "block"),
        _p(post, I64, "post"), block.shape[1], _p(result, I32, "result"), tail_rows.data_ptr(), tail_rows.stride(0),
        tail_rows.shape[0], _p(taps, BF16, "taps"), taps.shape[2], _p(dyn_d, I32, "dyn_d"), _p(dyn_t, I32, "dyn_t"), bs,
        _p(seeds, I64, "seeds"), int(seed), int(mask_id), _stream()), "dfl_admit_slot")


# ---- target prefill (csrc/prefill.hip)
def prefill_rows_padded(P: int) -> int:
    return lib().dfl_prefill_rows_padded(P)


def prefill_gemm_rows(wp, x_frag, P: int, N: int, K: int, out: torch.Tensor) -> None:
    assert out.dtype == BF16 and out.stride(1) == 1 and out.shape[0] >= prefill_rows_padded(P)
    check(lib().dfl_prefill_gemm_rows(_p(wp, BF16, "wp"), _p(x_frag, BF16, "x_frag"), P, N, K, out.data_ptr(),
                                      out.stride(0), _stream()), "dfl_prefill_gemm_rows")


def prefill_gemm_resid(wp, x_frag, P: int, N: int, K: int, h_io: torch.Tensor, tap=None) -> None:
    assert h_io.dtype == BF16 and h_io.stride(1) == 1 and h_io.shape[0] >= prefill_rows_padded(P)
    tp, ldt = None, 0
    if tap is not None:
        assert tap.is_cuda and tap.dtype == BF16 and tap.stride(1) == 1 and tap.shape[0] >= P
        tp, ldt = tap.data_ptr(), tap.stride(0)
    check(lib().dfl_prefill_gemm_resid(_p(wp, BF16, "wp"), _p(x_frag, BF16, "x_frag"), P, N, K, h_io.data_ptr(),
                                       h_io.stride(0), tp, ldt, _stream()), "dfl_prefill_gemm_resid")


def prefill_gemm_silu(wp_gu, x_frag, P: int, I: int, K: int, act_frag: torch.Tensor) -> None:
    assert act_frag.numel() >= prefill_rows_padded(P) * I
    check(lib().dfl_prefill_gemm_silu(_p(wp_gu, BF16, "wp_gu"), _p(x_frag, BF16, "x_frag"), P, I, K,
                                      _p(act_frag, BF16, "act_frag"), _stream()), "dfl_prefill_gemm_silu")


def prefill_norm_pack(h: torch.Tensor, P: int, H: int, norm_w, eps: float, x_frag: torch.Tensor) -> None:
    assert h.dtype == BF16 and h.stride(1) == 1 and h.shape[0] >= P and x_frag.numel() >= prefill_rows_padded(P) * H
    check(lib().dfl_prefill_norm_pack(h.data_ptr(), h.stride(0), P, H, _p(norm_w, BF16, "norm_w"), eps,
                                      _p(x_frag, BF16, "x_frag"), _stream()), "dfl_prefill_norm_pack")


def prefill_pack_rows(rows: torch.Tensor, P: int, K: int, x_frag: torch.Tensor) -> None:
    """rows [P, K] -> frag16 row tiles (any K % 32 == 0), no norm."""
    assert rows.dtype == BF16 and rows.stride(1) == 1 and rows.shape[0] >= P and x_frag.numel() >= prefill_rows_padded(P) * K
    check(lib().dfl_prefill_pack_rows(rows.data_ptr(), rows.stride(0), P, K, _p(x_frag, BF16, "x_frag"), _stream()),
          "dfl_prefill_pack_rows")


def prefill_qk_rope(qkv: torch.Tensor, P: int, q_col: int, k_col: int, v_col: int, n_q: int, n_kv: int, q_norm_w,
                    k_norm_w, eps: float, cos_tab, sin_tab, pos0: int, kcache, vcache, row0: int) -> None:
    assert qkv.dtype == BF16 and qkv.stride(1) == 1 and kcache.shape == vcache.shape and kcache.shape[2] == 128
    check(lib().dfl_prefill_qk_rope(qkv.data_ptr(), qkv.stride(0), P, q_col, k_col, v_col, n_q, n_kv,
                                    _p(q_norm_w, BF16, "q_norm_w"), _p(k_norm_w, BF16, "k_norm_w"), eps,
                                    _p(cos_tab, BF16, "cos"), _p(sin_tab, BF16, "sin"), cos_tab.shape[0], pos0,
                                    _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"), kcache.shape[1], row0,
                                    _stream()), "dfl_prefill_qk_rope")


def prefill_attn(qkv: torch.Tensor, P: int, q_col: int, kcache, vcache, n_q: int, n_kv: int, scale: float,
                 out_frag: torch.Tensor) -> None:
    """Causal attention of the prompt rows over themselves -> frag16 row tiles of n_q * 128 columns."""
    assert qkv.dtype == BF16 and qkv.stride(1) == 1 and kcache.shape == vcache.shape and kcache.shape[2] == 128
    assert out_frag.numel() >= (P + 15) // 16 * 16 * n_q * 128
    check(lib().dfl_prefill_attn(qkv.data_ptr(), qkv.stride(0), q_col, _p(kcache, BF16, "kcache"), _p(vcache, BF16, "vcache"),
                                 kcache.shape[1], P, n_q, n_kv, scale, _p(out_frag, BF16, "out_frag"), _stream()),
          "dfl_prefill_attn")


# ---- sparse-MoE MLP of the prefill (csrc/prefill.hip: k_pmoe_*, the grouped k_pgemm) ----------------------------
def prefill_moe_scratch(P: int, H: int, I: int, E: int, top_k: int, router_cols: int, device) -> dict:
    """Caller-owned scratch of dfl_prefill_moe_* for P prompt rows (sizes in include/dflash_hip.h)."""
    L = lib()
    mt, mi = int(L.dfl_prefill_moe_max_tiles(P, top_k, E)), int(L.dfl_prefill_moe_max_items(P, top_k, E))
    zi = lambda *s: torch.zeros(*s, dtype=I32, device=device)    # noqa: E731
    zf = lambda *s: torch.zeros(*s, dtype=F32, device=device)    # noqa: E731
    # (128-row work items where an expert serves ~48 rows or more on average, see include/dflash_hip.h)
    return dict(P=P, H=H, I=I, E=E, top_k=top_k, max_tiles=mt, max_items=mi, rows_per_item=128 if P * top_k >= 48 * E else 64,
                rlog=torch.zeros(prefill_rows_padded(P), router_cols, dtype=BF16, device=device),
                pair_e=zi(P, 8), posmap=zi(P, 8), pair_w=zf(P, 8), cnt=zi(E), tile_off=zi(E), src_row=zi(mt * 16),
                items=zi(3 * mi), n_items=zi(2), xg=torch.zeros(mt * 16 * H, dtype=BF16, device=device),
                act_g=torch.zeros(mt * 16 * I, dtype=BF16, device=device), row_w=zf(mt * 16), out32=zf(mt * 16, H),
                zeros=torch.zeros(512, dtype=BF16, device=device))


def prefill_moe_route(rlog: torch.Tensor, P: int, sc: dict, norm_topk: bool = True) -> None:
    """Routing of the P rows from their router logits (bf16 rows) + the plan of the grouped GEMMs, into the scratch."""
    check(lib().dfl_prefill_moe_route(rlog.data_ptr(), rlog.stride(0), P, sc["E"], sc["top_k"], int(bool(norm_topk)),
                                      sc["pair_e"].data_ptr(), sc["pair_w"].data_ptr(), sc["cnt"].data_ptr(),
                                      sc["tile_off"].data_ptr(), sc["items"].data_ptr(), sc["n_items"].data_ptr(),
                                      sc["posmap"].data_ptr(), sc["src_row"].data_ptr(), sc["row_w"].data_ptr(),
                                      sc["rows_per_item"], _stream()),
          "dfl_prefill_moe_route")


def moe_grouped_gate_up(wp_gu, x_frag: torch.Tensor, sc: dict, K: int, *, gather: bool) -> None:
    """The grouped gate/up + SiLU launch over the work list in the scratch `sc` (prefill_moe_route): act_g <- silu(x Wg_e^T)
    * (x Wu_e^T) per item.  wp_gu: packed bf16 [E, 2*I*K], or an Fp8Experts (dfl_moe_grouped_gate_up's e4m3 form: any K,
    unlike moe_gate_up).  gather: x_frag holds the UNGATHERED row tiles and the gather happens in the kernel's addresses
    (src_row); else x_frag is the gathered copy (sc["xg"])."""
    E, I = sc["E"], sc["I"]
    w, rows = _we(wp_gu, E, 2 * I, K, "wp_gu")
    assert rows.shape == (E, 2 * I * K) and x_frag.is_cuda and x_frag.dtype == BF16
    check(lib().dfl_moe_grouped_gate_up(w, rows.stride(0), x_frag.data_ptr(), _p(sc["items"], I32, "items"),
                                        _p(sc["n_items"], I32, "n_items"), sc["max_items"], I, K, _p(sc["act_g"], BF16, "act_g"),
                                        sc["rows_per_item"], _p(sc["src_row"], I32, "src_row") if gather else None,
                                        _p(sc["zeros"], BF16, "zeros") if gather else None, _stream()),
          "dfl_moe_grouped_gate_up")


def moe_grouped_down(wp_down, sc: dict, N: int) -> None:
    """The grouped down projection over the same work list: out32[gathered row] <- row_w * (act_g Wd_e^T), fp32.
    wp_down: packed bf16 [E, N*I], or an Fp8Experts."""
    E, I = sc["E"], sc["I"]
    w, rows = _we(wp_down, E, N, I, "wp_down")
    assert rows.shape == (E, N * I) and sc["out32"].shape[1] == N
    check(lib().dfl_moe_grouped_down(w, rows.stride(0), _p(sc["act_g"], BF16, "act_g"), _p(sc["items"], I32, "items"),
                                     _p(sc["n_items"], I32, "n_items"), sc["max_items"], N, I, _p(sc["row_w"], F32, "row_w"),
                                     _p(sc["out32"], F32, "out32"), sc["rows_per_item"], _stream()),
          "dfl_moe_grouped_down")


def prefill_moe_mlp(router_wp, gu_e, down_e, x_frag, P: int, H: int, I: int, E: int, top_k: int, norm_topk: bool,
                    h_io: torch.Tensor, sc: dict, tap=None) -> None:
    """Qwen3MoeSparseMoeBlock over the P prompt rows of one layer (tf:models/qwen3_moe/modeling_qwen3_moe.py):
    x_frag = the ln2-normalised rows as frag16 tiles; h_io <- h_io + MLP(x) (+ tap copy).  router_wp: the gate Linear's
    weight packed with its rows padded to a multiple of 128; gu_e / down_e: [E, ...] packed expert weights."""
    assert sc["P"] >= P and sc["H"] == H and sc["I"] == I and sc["E"] == E and sc["top_k"] == top_k
    assert gu_e.shape[0] == E and down_e.shape[0] == E and h_io.dtype == BF16 and h_io.stride(1) == 1
    L, st = lib(), _stream()
    rlog = sc["rlog"]
    prefill_gemm_rows(router_wp, x_frag, P, rlog.shape[1], H, rlog)
    prefill_moe_route(rlog, P, sc, norm_topk)
    # The rows are gathered per expert into a copy (xg) that the expert's column blocks then read coalesced.  Gathering
    # inside the gate/up GEMM's LDS-DMA addresses instead (src_row: no gather launch, no copy) was measured at P = 1024
    # on the 30B-A3B widths, same box: 455 -> 479 us per layer — every column block re-reads the rows as scattered 16-byte
    # pieces; it is what the <= 64 decode rows of NativeTarget._moe_mlp_shared use (241 -> 233 us there).
    check(L.dfl_prefill_moe_gather(_p(x_frag, BF16, "x_frag"), P, H, top_k, E, sc["src_row"].data_ptr(), sc["n_items"].data_ptr(),
                                   sc["xg"].data_ptr(), st), "dfl_prefill_moe_gather")
    check(L.dfl_prefill_moe_gemm_silu(_p(gu_e, BF16, "gu_e"), gu_e.stride(0), sc["xg"].data_ptr(), sc["items"].data_ptr(),
                                      sc["n_items"].data_ptr(), sc["max_items"], I, H, sc["act_g"].data_ptr(),
                                      sc["rows_per_item"], None, None, st), "dfl_prefill_moe_gemm_silu")
    check(L.dfl_prefill_moe_gemm_down(_p(down_e, BF16, "down_e"), down_e.stride(0), sc["act_g"].data_ptr(),
                                      sc["items"].data_ptr(), sc["n_items"].data_ptr(), sc["max_items"], H, I,
                                      sc["row_w"].data_ptr(), sc["out32"].data_ptr(), sc["rows_per_item"], st),
          "dfl_prefill_moe_gemm_down")
    tp, ldt = (None, 0) if tap is None else (_p(tap, BF16, "tap") if tap.is_contiguous() else tap.data_ptr(), tap.stride(0))
    check(L.dfl_prefill_moe_combine(sc["out32"].data_ptr(), sc["posmap"].data_ptr(), P, H, top_k, h_io.data_ptr(),
                                    h_io.stride(0), tp, ldt, None, st), "dfl_prefill_moe_combine")
