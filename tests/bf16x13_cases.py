"""Weight matrices for the 13-bit bf16 stream's tests, built from integer arithmetic alone, so the
CPU tests (the packer's own account: nothing refused, every planted patch counted) and the GPU tests (the kernel's
decode) see the SAME bits on either device.  Plain module: no fixtures, no GPU, no library call.

What a matrix of make_case() holds
  * a base per tile: tile t's largest exponent is 123 + SHIFTS[t % 7] (randn * 0.02 has 123 in every tile).  Seven
    shifts, so that tiles 256, 258, 272 and 342 apart — the strides of the tile plans below — and the gate and the up
    tile of a pair never share one; odd shifts move the exponent's low bit, which lives in the L byte.  Magnitudes fall
    off by binades like a Gaussian's small values (half the elements in the top binade, a quarter in the next ...) down
    to 27 binades below the top: all 15 codes occur, nothing leaves the window.
  * ZERO_TILE all zeros (base 0, every code 0).
  * the format's edge values (+-0, denormals, exponent 1, the tile's top binade, its window's lowest binade) in one tile.
  * patches: in every PATCH tile one nonzero element below the window in EACH of the 16 (tile, wave) items.
  * extreme=True (the one-hot probe only: sums over such tiles overflow): a tile holding 0x7f7f (base 112) with the
    lowest binade of its window, and a tile 100 binades down (base 0, mostly denormals).

The tile plans the patch tiles follow (csrc/gemm_skinny.hip: plan_tiles, grid_x_for, tile_of) — plan_argmax / plan_silu
below restate them, and the CPU test checks what is claimed here against them:
  argmax  V  4208: 263 tiles = 256 whole (workgroup b: tile b) + 7 halved (workgroups 0..13: half b & 1 of tile
                   256 + b / 2 as their second item).  Patch tiles 0, 1, 13, 128, 255 (first items), 256, 262 (halved,
                   second: of workgroups 0 and 1, and of 13).
          V  9600: 600 = 512 whole (b, b + 256) + 88 halved (512 + b / 2, third item, b < 176).  Patch tiles 0, 1, 128,
                   174, 255 (first), 256, 257, 384, 430, 511 (second), 512, 576, 599 (halved, third).
          V  8192: 512 whole, no halves.  Patch tiles 0, 1, 128, 255 (first), 256, 257, 384, 511 (second).
          V  2048: 128 tiles, ALL halved, each the only item of its two workgroups.  Patch tiles 0, 64, 127.
  silu    I   512:  32 pairs, one per workgroup (gate tile 2p first, up tile 2p + 1 second).  Pairs 0, 1, 16, 31.
          I  4352: 272 pairs, workgroup b: pairs b, b + 136.  Pairs 0, 1, 68, 135 and 136, 137, 204, 271.
          I  4112: 257 pairs, workgroup b: pairs b, b + 129; workgroup 128 has pair 128 alone.  Pairs 0, 1, 64, 127, 128
                   and 129, 130, 193, 256.
          I  8208: 513 pairs, workgroup b: pairs b, b + 171, b + 342.  Pairs 0, 1, 85, 170; 171, 172, 256, 341; 342, 343,
                   427, 512.
A gate/up case is ONE [2 I, K] matrix in packed tile order (tile 2p = gate rows 16p .., tile 2p + 1 = up rows 16p ..):
split_gateup() gives the two [I, K] matrices, and every row index below counts packed rows."""
from typing import NamedTuple

import torch

BF16 = torch.bfloat16
SHIFTS = [0, 1, -2, 5, -7, 12, -24]   # |s| <= 24: every sum over such tiles stays finite
TOP_E = 123                           # the exponent field of a randn * 0.02 tile's largest magnitude
ZERO_TILE = 5
EDGE_TILE = 6
TOP_TILE, DEEP_TILE = 9, 10           # extreme=True only
# the lane of a patch by wave (variant 0; variant 1 mirrors it: 63 - l): lanes 0 and 63, both 8-column halves
LANES = [0, 63, 8, 23, 36, 47, 15, 48, 5, 58, 27, 33, 20, 44, 9, 54]


class Patch(NamedTuple):
    row: int      # packed row (tile * 16 + lane & 15)
    col: int      # k
    bits: int     # the bf16 itself
    tile: int
    wave: int
    kstep: int    # of the wave's share
    lane: int
    element: int


class Case(NamedTuple):
    w: torch.Tensor        # [N, K] bf16
    patches: list          # of Patch: one per (tile, wave) item of every patch tile
    edges: list            # of (row, col, bits): the planted edge values
    patch_tiles: list
    N: int
    K: int


def grid_x_for(ngroups: int) -> int:
    per_wg = (ngroups + 255) // 256
    return (ngroups + per_wg - 1) // per_wg


def plan_argmax(V: int) -> list:
    """Per workgroup, its items in order: (tile, half) with half -1 for a whole tile."""
    nt = V // 16
    if nt <= 128:
        return [[(b >> 1, b & 1)] for b in range(2 * nt)]
    gx, whole, r = grid_x_for(nt), nt, nt % 256
    if nt > 256 and 0 < r <= 128:
        gx, whole = 256, nt - r
    plan = [[(t, -1) for t in range(b, whole, gx)] for b in range(gx)]
    if whole < nt:
        for b in range(2 * r):
            plan[b].append((whole + (b >> 1), b & 1))
    return plan


def plan_silu(I: int) -> list:
    """Per workgroup, its items in order: the packed tiles gate, up of pair b, then of pair b + gx ..."""
    npairs = I // 16
    gx = grid_x_for(npairs)
    return [[(2 * p + g, -1) for p in range(b, npairs, gx) for g in (0, 1)] for b in range(gx)]


def patch_tiles_for(kind: str, n: int) -> list:
    """The items of the first two workgroups, of the middle one, of the last one, and of the last one that walks the
    longest sequence with a different shift in each pair of consecutive items."""
    plan = plan_argmax(n) if kind == "argmax" else plan_silu(n)
    longest, ns = max(len(p) for p in plan), len(SHIFTS)
    pick = {0, 1, len(plan) // 2, len(plan) - 1,
            max(b for b, p in enumerate(plan) if len(p) == longest and all(x[0] % ns != y[0] % ns for x, y in zip(p, p[1:])))}
    tiles = sorted({t for b in pick for t, _ in plan[b]})
    assert not {ZERO_TILE, EDGE_TILE, TOP_TILE, DEEP_TILE} & set(tiles)
    return tiles


def _from_bits(v: torch.Tensor) -> torch.Tensor:
    return torch.where(v >= 32768, v - 65536, v).to(torch.int16).view(BF16)


def _hash(rows: torch.Tensor, K: int, seed: int) -> torch.Tensor:
    """32 mixed bits per element (int64 tensor), a function of (row, column, seed) alone."""
    cols = torch.arange(K, dtype=torch.int64, device=rows.device)
    h = (rows.view(-1, 1) * K + cols.view(1, -1) + seed * 0x9E3779B1) & 0xffffffff
    h = ((h ^ (h >> 16)) * 0x7feb352d) & 0xffffffff
    h = ((h ^ (h >> 15)) * 0x846ca68b) & 0xffffffff
    return h ^ (h >> 16)


def tile_top_exponent(t: int, extreme: bool = False) -> int:
    if extreme and t == TOP_TILE:
        return 254
    if extreme and t == DEEP_TILE:
        return TOP_E - 100
    return TOP_E + SHIFTS[t % len(SHIFTS)]


def make_case(N: int, K: int, seed: int, patch_tiles, extreme: bool = False, device="cpu") -> Case:
    """The [N, K] matrix described above, on `device`, and the tables of what was planted in it."""
    device = torch.device(device)
    nt, nfr = N // 16, K // 512
    assert N % 16 == 0 and K in (2048, 4096) and nt > max(DEEP_TILE, max(patch_tiles))
    top = torch.tensor([tile_top_exponent(t, extreme) for t in range(nt)], dtype=torch.int64, device=device)
    w = torch.empty(N, K, dtype=BF16, device=device)
    for r0 in range(0, N, 2048):                            # (by row blocks: the int64 temporaries stay small)
        rows = torch.arange(r0, min(r0 + 2048, N), dtype=torch.int64, device=device)
        h = _hash(rows, K, seed)
        # binades below the tile's top: the number of trailing ones of 20 hash bits (0 for half of the elements; the
        # lowest clear bit is a power of two, whose fp32 exponent field is that number), and for one element in 16
        # any of 0..27 alike
        g = (h >> 8) & 0xfffff
        lowest_clear = (~g & (g + 1)).to(torch.float32).view(torch.int32).to(torch.int64)
        drop = (lowest_clear >> 23) - 127
        drop = torch.where((h >> 28) == 0, g % 28, drop)
        e = (top[rows >> 4].view(-1, 1) - drop).clamp_(min=0)
        v = ((h & 1) << 15) | (e << 7) | ((h >> 1) & 0x7f)
        w[r0:r0 + rows.numel()] = _from_bits(v)
    w[16 * ZERO_TILE:16 * ZERO_TILE + 16] = 0

    first = [wv * nfr * 32 for wv in range(16)]             # the first and the last column of every wave's share
    last = [c + nfr * 32 - 1 for c in first]
    wi = w.view(torch.int16)

    def put(row, col, bits):
        wi[row, col] = bits if bits < 32768 else bits - 65536

    def plant_edges(tile, values):
        out = []
        for i, v in enumerate(values):
            row, col = 16 * tile + (5 * i + 3) % 16, (first if i % 2 == 0 else last)[(3 * i) % 16]
            put(row, col, v)
            out.append((row, col, v))
        return out

    t7 = tile_top_exponent(EDGE_TILE) >> 1                  # H & 0x7f of the tile's largest magnitude
    lowest = ((t7 - 14) << 8) | 0x33
    edges = plant_edges(EDGE_TILE, [0x0000, 0x8000, 0x0001, 0x807f, 0x0080, 0x80ff, (t7 << 8) | 0x7f, 0x8000 | (t7 << 8),
                                    lowest, 0x8000 | lowest, 0x8000, 0x007f])
    if extreme:
        edges += plant_edges(TOP_TILE, [0x7f7f, 0xff7f, 113 << 8, 0x8000 | (113 << 8) | 0xff, 0x7f00])
        edges += plant_edges(DEEP_TILE, [0x0001, 0x8001, 0x0080, 0x8f7f, 0x0000, 0x8000])

    patches = []
    for p, t in enumerate(sorted(patch_tiles)):
        hb = (tile_top_exponent(t, extreme) >> 1) - 15
        assert hb >= 1, "a patch needs a window that does not reach the bottom of the range"
        for wv in range(16):
            var = p & 1
            lane = 63 - LANES[wv] if var else LANES[wv]
            kstep, el = (wv + var) % nfr, (3 * wv + var) % 8
            bits = (hb << 8) | ((0x5a + 37 * wv + 11 * p) & 0xff) | (0x8000 if (wv + p) & 1 else 0)
            row, col = 16 * t + (lane & 15), (wv * nfr + kstep) * 32 + (lane >> 4) * 8 + el
            put(row, col, bits)
            patches.append(Patch(row, col, bits, t, wv, kstep, lane, el))
    return Case(w, patches, edges, sorted(patch_tiles), N, K)


ARGMAX_SHAPES = [(4208, 4096), (9600, 4096), (8192, 4096), (2048, 4096), (4208, 2048), (2048, 2048)]
SILU_SHAPES = [(512, 4096), (4352, 4096), (4112, 4096), (8208, 4096), (512, 2048), (4112, 2048)]


def argmax_case(V: int, K: int, extreme: bool = False, device="cpu") -> Case:
    return make_case(V, K, 1000 + V + K, patch_tiles_for("argmax", V), extreme, device)


def silu_case(I: int, K: int, device="cpu") -> Case:
    """The gate element that meets a patched UP element is made positive: silu of a large negative gate (the tiles go
    up to 2^8) underflows, and the product would be 0 whether the patch is applied or not."""
    case = make_case(2 * I, K, 2000 + I + K, patch_tiles_for("silu", I), False, device)
    spots = {(p.row, p.col) for p in case.patches} | {(e[0], e[1]) for e in case.edges}
    wi = case.w.view(torch.int16)
    for p in case.patches:
        if p.tile & 1:
            assert (p.row - 16, p.col) not in spots
            wi[p.row - 16, p.col] &= 0x7fff
    return case


def split_gateup(w: torch.Tensor):
    """[2 I, K] in packed tile order -> gate [I, K], up [I, K]."""
    n, k = w.shape
    v = w.view(n // 32, 2, 16, k)
    return v[:, 0].reshape(n // 2, k).contiguous(), v[:, 1].reshape(n // 2, k).contiguous()


def probe_columns(case: Case) -> list:
    """The columns the one-hot probe reads: every patched one, the first and the last of every wave's share, and every
    planted edge value's — padded to a multiple of 16 (one launch probes 16)."""
    nfr = case.K // 512
    cols = {p.col for p in case.patches} | {e[1] for e in case.edges}
    cols |= {wv * nfr * 32 for wv in range(16)} | {wv * nfr * 32 + nfr * 32 - 1 for wv in range(16)}
    cols = sorted(cols)
    k = 1
    while len(cols) % 16:
        if k not in cols:
            cols.append(k)
        k += 7
    return cols


def apply_tile_shifts(gate: torch.Tensor, up: torch.Tensor, down: torch.Tensor = None) -> None:
    """A model's gate/up [I, K] by the rule above, in place: packed tile t (2p: gate rows 16p .., 2p + 1: up rows 16p ..)
    times 2^SHIFTS[t % 7] — exact in bf16.  down [H, I] (optional): column i divided by the two powers of its gate and
    up rows, so that the MLP's output keeps its order of magnitude (silu(2^a g) * 2^b u is at most 2^(a + b) |g u|)."""
    I = gate.shape[0]
    t = torch.arange(I, device=gate.device) // 16 * 2
    s = torch.tensor(SHIFTS, dtype=torch.float32, device=gate.device)
    sg, su = s[t % len(SHIFTS)], s[(t + 1) % len(SHIFTS)]
    gate.mul_(torch.exp2(sg).view(-1, 1).to(gate.dtype))
    up.mul_(torch.exp2(su).view(-1, 1).to(up.dtype))
    if down is not None:
        down.mul_(torch.exp2(-(sg + su)).view(1, -1).to(down.dtype))


def plant_refusal(w: torch.Tensor, tile: int, wave: int) -> None:
    """Two nonzero elements below tile `tile`'s window in ONE (tile, wave) item of w [N, K]: the packer refuses w."""
    nfr = w.shape[1] // 512
    wi = w[16 * tile:16 * tile + 16].view(torch.int16)
    hb = (int((wi & 0x7fff).max()) >> 8) - 15
    assert hb >= 1
    c0 = wave * nfr * 32
    wi[2, c0 + 6] = (hb << 8) | 0x21
    wi[9, c0 + nfr * 32 - 12] = -32768 + ((hb << 8) | 0x47)
