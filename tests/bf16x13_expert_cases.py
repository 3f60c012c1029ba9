"""Expert-tall weight matrices for the tests of the 13-bit expert gate/up stream (dfl_moe_gate_up on DFL_W_BF16X13,
DESIGN.md section 11, "The experts"): tests/bf16x13_cases.py's matrices — a base per tile, a zero tile, the format's edge
values, one planted patch in each of the 16 (tile, wave) items of every patch tile — laid out as an MoE layer's experts,
[E * 2I, 2048] in packed tile order (expert e's gate tile p and up tile p are tiles e * 2 npp + 2p and + 1, npp = I / 16).
Plain module: no fixtures, no GPU, no library call; the CPU and the GPU tests see the same bits.

The item plan it follows (csrc/moe.hip, k_moe_gate_up): item `it` is pair it % npp of expert list[it / npp]; workgroup b
of 256 walks items b, b + 256, b + 512, ..., the first in buffer A, the second in B, the third in A again.
  "few"     E =  4, I =  32,  4 active in order:            8 items, workgroups 0..7 one each; their B request is dead
  "second"  E = 48, I = 112, 40 active in scrambled order: 280 items, workgroups 0..23 have a second item
  "third"   E = 48, I = 176, all 48 in order:              528 items, workgroups 0..15 have a third item
Patch tiles: BOTH tiles of EVERY item of workgroups 0 and 1 and of the last workgroup that walks the longest sequence.

A base per tile: bf16x13_cases gives tile c the shift SHIFTS[c % 7].  With 14 tiles per expert (I = 112) every expert
would repeat the same seven bases, so expert e's tiles are taken from the case matrix ROTATED by 2e tiles within the
expert's range (case_tile below; an even rotation: a gate / up pair stays a pair): the same tile of different experts has
different bases, and a decode that reads expert 0's meta pairs for every expert is wrong nearly everywhere.

The gate element that meets a patched UP element is made positive, as silu_case does; every probed position (a patched
gate or up element under a one-hot row) then has an `act` that is a normal nonzero bf16 (tests/test_bf16x13_experts_cpu.py
asserts it), so that a patch that is not applied shows."""
from typing import NamedTuple

import torch

import bf16x13_cases as X

K = 2048
GRID = 256
SHAPES = {"few": (4, 32, 4), "second": (48, 112, 40), "third": (48, 176, 48)}   # E, I, active experts


class ExpertCase(NamedTuple):
    w: torch.Tensor        # [E * 2I, K] bf16, packed tile order
    patches: list          # of bf16x13_cases.Patch in THIS matrix's rows and tiles
    edges: list            # of (row, col, bits)
    patch_tiles: list
    E: int
    I: int
    lst: list              # the active experts in the order the launch gets them
    plan: list             # per workgroup: its items in order, each (gate tile, up tile)
    special: dict          # name -> tile of this matrix: "zero", "edge" (and "top", "deep" with extreme=True)


def expert_list(E: int, n_active: int) -> list:
    """All experts ascending (what the router writes), or the first n_active of the scramble 7 i + 3 (mod E)."""
    if n_active == E:
        return list(range(E))
    assert E % 7 and n_active < E
    return [(7 * i + 3) % E for i in range(n_active)]


def plan_items(I: int, lst: list) -> list:
    npp = I // 16
    n = len(lst) * npp
    plan = [[] for _ in range(min(GRID, n))]
    for it in range(n):
        t = (lst[it // npp] * npp + it % npp) * 2
        plan[it % GRID].append((t, t + 1))
    return plan


def case_tile(t: int, I: int) -> int:
    """The tile of the bf16x13_cases matrix that tile t of the expert-tall matrix is."""
    per = 2 * (I // 16)
    e, j = divmod(t, per)
    return e * per + (j + 2 * e) % per


def expert_case(name: str, extreme: bool = False, device="cpu") -> ExpertCase:
    E, I, n_active = SHAPES[name]
    nt = E * 2 * (I // 16)
    lst = expert_list(E, n_active)
    plan = plan_items(I, lst)
    longest = max(len(p) for p in plan)
    pick = {0, 1, max(b for b, p in enumerate(plan) if len(p) == longest)}
    ptiles = sorted({t for b in pick for pair in plan[b] for t in pair})
    src = [case_tile(t, I) for t in range(nt)]
    assert sorted(src) == list(range(nt))
    dst = {c: t for t, c in enumerate(src)}
    case = X.make_case(nt * 16, K, 3000 + E * I, [src[t] for t in ptiles], extreme, device)   # (asserts: no special tile patched)
    spots = {(p.row, p.col) for p in case.patches} | {(e[0], e[1]) for e in case.edges}
    wi = case.w.view(torch.int16)
    for p in case.patches:
        if p.tile & 1:
            assert (p.row - 16, p.col) not in spots
            wi[p.row - 16, p.col] &= 0x7fff
    w = case.w.view(nt, 16, K)[torch.tensor(src, device=case.w.device)].reshape(nt * 16, K).contiguous()
    patches = [p._replace(tile=dst[p.tile], row=16 * dst[p.tile] + (p.row & 15)) for p in case.patches]
    edges = [(16 * dst[r >> 4] + (r & 15), c, v) for r, c, v in case.edges]
    special = {"zero": dst[X.ZERO_TILE], "edge": dst[X.EDGE_TILE]}
    if extreme:
        special.update(top=dst[X.TOP_TILE], deep=dst[X.DEEP_TILE])
    assert sorted({p.tile for p in patches}) == ptiles
    return ExpertCase(w, patches, edges, ptiles, E, I, lst, plan, special)


def split_experts(case: ExpertCase) -> list:
    """Per expert: (gate [I, K], up [I, K])."""
    return [X.split_gateup(case.w[e * 2 * case.I:(e + 1) * 2 * case.I]) for e in range(case.E)]


def probe_points(case: ExpertCase) -> list:
    """Per patch: (expert, output column i of that expert, k, gate row, up row) — under a one-hot row e_k,
    act[expert][m, i] = silu(w[gate row, k]) * w[up row, k], and one of the two is the patched element."""
    per = 2 * (case.I // 16)
    out = []
    for p in case.patches:
        e, j = divmod(p.tile, per)
        grow = 16 * (p.tile & ~1) + (p.row & 15)
        out.append((e, (j >> 1) * 16 + (p.row & 15), p.col, grow, grow + 16))
    return out


def probe_columns(case: ExpertCase) -> list:
    """bf16x13_cases.probe_columns: every patched column, the first and the last of every wave's share, the planted edge
    values', padded to a multiple of 16."""
    return X.probe_columns(X.Case(case.w, case.patches, case.edges, case.patch_tiles, case.w.shape[0], K))
