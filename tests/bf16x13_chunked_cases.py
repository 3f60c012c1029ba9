"""Weight matrices for the K-chunked form of the 13-bit bf16 stream ("down_proj and fc":
dfl_gemm_resid at K a multiple of 2048 above 4096), by the integer arithmetic of tests/bf16x13_cases.py, so the CPU test
(the packer's account) and the GPU test (the kernel's decode) see the same bits.  Plain module: no fixtures, no GPU.

An ITEM here is (tile, chunk, wave): quad 16 * chunk + wave of the tile, 4 k-steps, columns (16 c + w) * 128 .. + 127.
What a matrix of chunked_case() holds
  * a base per tile: tile t's largest exponent is 123 + SHIFTS[t % 7], magnitudes falling off by binades (bf16x13_cases);
  * a zero tile (all codes 0, base 0) where the shape has a tile to spare, and the format's edge values in one tile, each
    in the first or the last column of some (chunk, wave) share;
  * patches: one nonzero element below the window in EVERY wave of EVERY chunk of the patch tiles — the tiles some
    workgroups walk first and second (plan_resid).  k-step, element and lane come from the tables of bf16x13_cases,
    moved on by the chunk so that successive chunks of a wave differ.

The tile plan of a K-chunked dfl_gemm_resid (csrc/gemm_skinny.hip: plan_tiles without half tiles, tile_of): workgroup b
of gx = grid_x_for(N / 16) walks tiles b, b + gx, ...
  N    32:   2 tiles, one per workgroup.  Patch tiles 0, 1; edges in tile 1; no zero tile.
  N    48:   3 tiles, one per workgroup.  Patch tiles 0, 2; zero tile 1; edges in tile 2.
  N  4112: 257 tiles, gx = 129: workgroup b walks b and b + 129, workgroup 128 tile 128 alone.  Patch tiles 0, 1, 64,
           128 (first) and 129, 130, 193 (second); zero tile 5, edges in tile 6."""
import torch

from bf16x13_cases import BF16, LANES, SHIFTS, Case, Patch, _from_bits, _hash, grid_x_for, tile_top_exponent

SHAPES = [(32, 6144), (4112, 6144), (48, 8192)]    # (N, K): 3 chunks; two tiles x 3 chunks per workgroup; 4 chunks


def plan_resid(N: int) -> list:
    """Per workgroup, its tiles in order."""
    nt = N // 16
    gx = grid_x_for(nt)
    return [list(range(b, nt, gx)) for b in range(gx)]


def layout_for(N: int):
    """(patch tiles, zero tile or None, edge tile) of the shapes above."""
    nt = N // 16
    if nt == 2:
        return [0, 1], None, 1
    if nt == 3:
        return [0, 2], 1, 2
    plan = plan_resid(N)
    pick = {0, 1, len(plan) // 2, len(plan) - 1}
    tiles = sorted({t for b in pick for t in plan[b]})
    assert not {5, 6} & set(tiles)
    return tiles, 5, 6


def chunked_case(N: int, K: int, device="cpu") -> Case:
    """The [N, K] matrix described above, on `device`, and the tables of what was planted in it.  Patch.wave holds the
    item's quad 16 * chunk + wave, Patch.kstep the k-step of that quad (0..3)."""
    device = torch.device(device)
    assert N % 16 == 0 and K > 4096 and K % 2048 == 0
    patch_tiles, zero_tile, edge_tile = layout_for(N)
    nt, nq, seed = N // 16, K // 128, 3000 + N + K
    top = torch.tensor([tile_top_exponent(t) for t in range(nt)], dtype=torch.int64, device=device)
    w = torch.empty(N, K, dtype=BF16, device=device)
    for r0 in range(0, N, 1024):
        rows = torch.arange(r0, min(r0 + 1024, N), dtype=torch.int64, device=device)
        h = _hash(rows, K, seed)
        g = (h >> 8) & 0xfffff
        lowest_clear = (~g & (g + 1)).to(torch.float32).view(torch.int32).to(torch.int64)
        drop = (lowest_clear >> 23) - 127
        drop = torch.where((h >> 28) == 0, g % 28, drop)
        e = (top[rows >> 4].view(-1, 1) - drop).clamp_(min=0)
        w[r0:r0 + rows.numel()] = _from_bits(((h & 1) << 15) | (e << 7) | ((h >> 1) & 0x7f))
    if zero_tile is not None:
        w[16 * zero_tile:16 * zero_tile + 16] = 0
    wi = w.view(torch.int16)
    taken = set()

    def put(row, col, bits):
        assert (row, col) not in taken
        taken.add((row, col))
        wi[row, col] = bits if bits < 32768 else bits - 65536

    t7 = tile_top_exponent(edge_tile) >> 1                  # H & 0x7f of the tile's largest magnitude
    lowest = ((t7 - 14) << 8) | 0x33
    edges = []
    for i, v in enumerate([0x0000, 0x8000, 0x0001, 0x807f, 0x0080, 0x80ff, (t7 << 8) | 0x7f, 0x8000 | (t7 << 8), lowest,
                           0x8000 | lowest, 0x8000, 0x007f]):
        q = (7 * i + 2) % nq                                # shares of several chunks
        row, col = 16 * edge_tile + (5 * i + 3) % 16, q * 128 + (0 if i % 2 == 0 else 127)
        put(row, col, v)
        edges.append((row, col, v))

    patches = []
    for p, t in enumerate(patch_tiles):
        hb = (tile_top_exponent(t) >> 1) - 15
        assert hb >= 1
        for q in range(nq):
            c, wv, var = q // 16, q % 16, p & 1
            lane = LANES[(wv + 5 * c) % 16]
            lane = 63 - lane if var else lane
            kstep, el = (wv + var + c) % 4, (3 * wv + var + 5 * c) % 8
            bits = (hb << 8) | ((0x5a + 37 * wv + 11 * p + 3 * c) & 0xff) | (0x8000 if (wv + p + c) & 1 else 0)
            row, col = 16 * t + (lane & 15), q * 128 + kstep * 32 + (lane >> 4) * 8 + el
            put(row, col, bits)
            patches.append(Patch(row, col, bits, t, q, kstep, lane, el))
    return Case(w, patches, edges, patch_tiles, N, K)


def probe_columns(case: Case) -> list:
    """The columns the one-hot probe reads: every patched one, the first and the last of every (chunk, wave) share and
    every planted edge value's — padded to a multiple of 16 (one launch probes 16)."""
    cols = {p.col for p in case.patches} | {e[1] for e in case.edges}
    cols |= {q * 128 for q in range(case.K // 128)} | {q * 128 + 127 for q in range(case.K // 128)}
    cols = sorted(cols)
    k = 1
    while len(cols) % 16:
        if k not in cols:
            cols.append(k)
        k += 7
    return cols


def plant_refusal(w: torch.Tensor, tile: int, chunk: int, wave: int) -> None:
    """Two nonzero elements below tile `tile`'s window in ONE (tile, chunk, wave) item of w [N, K], K > 4096: the packer
    refuses w."""
    wi = w[16 * tile:16 * tile + 16].view(torch.int16)
    hb = (int((wi & 0x7fff).max()) >> 8) - 15
    assert hb >= 1
    c0 = (16 * chunk + wave) * 128
    wi[2, c0 + 6] = (hb << 8) | 0x21
    wi[9, c0 + 128 - 12] = -32768 + ((hb << 8) | 0x47)
