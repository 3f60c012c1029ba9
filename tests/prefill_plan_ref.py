"""Plain fp64 references for the index arithmetic of csrc/prefill.hip that the model-level tests cannot see: the routing
of Qwen3MoeTopKRouter (moe_route.h), the plan k_pmoe_plan builds from the routed pairs, the block form pgemm_launch
picks, and an expert-by-expert evaluation of the routed MLP rows with the kernels' rounding points.  torch on the CPU
(or on whatever device its inputs live on) and numpy only; nothing here imports dflash_amd or needs a GPU.

The plan of a layer, as dfl_prefill_moe_route writes it (P rows, top_k slots per row, E experts, tpi = rows_per_item / 16
gathered tiles per work item):
  cnt[e]        rows routed to expert e
  tile_off[e]   first gathered 16-row tile of expert e: the exclusive prefix of ceil(cnt / 16)
  n_items       [work items, gathered tiles]
  items         per work item (expert, first tile, tiles <= tpi), in expert order; experts without rows have none
  posmap[m][r]  gathered row of pair (m, r); the order inside an expert's rows is arbitrary (atomic ranks)
  src_row[g]    source row of gathered row g, -1 for padding        row_w[g]  its routing weight, 0 for padding
check_plan states what must hold of these whatever the order inside an expert and names the first entry that breaks it."""
from __future__ import annotations

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64

# (P, N, K, block form): the dense k_pgemm cases of tests/test_hip_prefill_forms.py and what each is there to reach
DENSE_CASES = [
    (1024, 8192, 64, 128),    # 512 blocks exactly: the first shape of the 128-row form; one K step, nothing re-staged
    (1000, 8576, 192, 128),   # nbx = 67: a tail of 3 column blocks with nby = 8; KT = 3: both stages reused; ragged rows
    (129, 32768, 128, 128),   # two row blocks, the second with one live row
    (896, 9344, 192, 64),     # 511 blocks, just under the switch; nbx = 73 (tail of 1), 14 row blocks of 64
]


def rbf(x: torch.Tensor) -> torch.Tensor:
    """fp64 values rounded as the kernels round their fp32 registers to bf16, returned as fp64."""
    return x.to(F32).to(BF16).to(F64)


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of the bf16 values at |x| (fp64; the smallest normal binade below it)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.exp2(e - 7)


def pgemm_blocks(P: int, N: int) -> int:
    """Workgroups of 128 x 128 blocks over P rows and N columns."""
    return (N // 128) * ((P + 127) // 128)


def pgemm_form(P: int, N: int) -> int:
    """Rows per block of the dense k_pgemm launch: mirrors pgemm_launch in csrc/prefill.hip (128-row blocks unless that
    leaves fewer than 512 workgroups).  A drifted mirror makes a case miss its form, which the case list asserts."""
    return 128 if pgemm_blocks(P, N) >= 512 else 64


def max_tiles(P: int, top_k: int, E: int) -> int:
    """dfl_prefill_moe_max_tiles: every expert may end in one partial tile."""
    return (P * top_k + 15) // 16 + E


def tie_free_logits(rows: int, E: int, g: torch.Generator) -> torch.Tensor:
    """bf16 router logits in about +-9 with no two equal values in a row (test_hip_moe._tie_free_logits)."""
    pool = torch.unique((torch.randn(20000, generator=g) * 3).to(BF16))
    assert pool.numel() >= E
    return torch.stack([pool[torch.randperm(pool.numel(), generator=g)[:E]] for _ in range(rows)])


def route(logits_bf16: torch.Tensor, top_k: int, norm: bool):
    """fp64 softmax of the bf16 logits [P, E]; top_k by (probability descending, expert index ascending); optional
    renormalisation over the selected; weights rounded to bf16 (moe_route.h, k_pmoe_route).  A row with a NaN logit
    selects experts 0 .. top_k - 1 with NaN weights.  Returns (pair_e int64 [P, top_k], pair_w fp32 [P, top_k])."""
    assert logits_bf16.dtype == BF16 and logits_bf16.dim() == 2 and 1 <= top_k <= logits_bf16.shape[1]
    x = logits_bf16.to(F64)
    bad = torch.isnan(x).any(dim=1)
    x = torch.where(bad[:, None], torch.zeros_like(x), x)
    p = torch.softmax(x, dim=1)
    # a stable ascending sort of -p keeps equal probabilities in index order
    idx = torch.sort(-p, dim=1, stable=True).indices[:, :top_k]
    w = torch.gather(p, 1, idx)
    if norm:
        w = w / w.sum(dim=1, keepdim=True)
    idx = torch.where(bad[:, None], torch.arange(top_k, device=x.device)[None, :].expand_as(idx), idx)
    w = torch.where(bad[:, None], torch.full_like(w, float("nan")), w)
    return idx, w.to(F32).to(BF16).to(F32)


def _first(bad: np.ndarray) -> tuple:
    return tuple(int(v) for v in np.argwhere(bad)[0])


def check_plan(pair_e, pair_w, E: int, tpi: int, cnt, tile_off, n_items, items, posmap, src_row, row_w) -> dict:
    """Raises AssertionError naming the first offending index unless the plan arrays are a plan of the routed pairs
    (pair_e / pair_w [P, top_k]; the other arguments as dfl_prefill_moe_route writes them, see the module docstring)."""
    pair_e = np.asarray(pair_e, dtype=np.int64)
    pair_w = np.asarray(pair_w, dtype=np.float32)
    P, top_k = pair_e.shape
    cnt, tile_off = np.asarray(cnt, dtype=np.int64)[:E], np.asarray(tile_off, dtype=np.int64)[:E]
    n_items, items = [int(v) for v in np.asarray(n_items)[:2]], np.asarray(items, dtype=np.int64)
    posmap, src_row = np.asarray(posmap, dtype=np.int64)[:P, :top_k], np.asarray(src_row, dtype=np.int64)
    row_w = np.asarray(row_w, dtype=np.float32)
    slots = 16 * max_tiles(P, top_k, E)
    assert pair_e.min() >= 0 and pair_e.max() < E, "pair_e outside [0, E)"
    assert src_row.shape[0] >= slots and row_w.shape[0] >= slots, "src_row / row_w shorter than 16 * max_tiles"

    want_cnt = np.bincount(pair_e.ravel(), minlength=E)
    if (cnt != want_cnt).any():
        e, = _first(cnt != want_cnt)
        raise AssertionError(f"cnt[{e}] = {cnt[e]}, {want_cnt[e]} pairs route there")
    tiles = (want_cnt + 15) // 16
    want_off = np.cumsum(tiles) - tiles
    if (tile_off != want_off).any():
        e, = _first(tile_off != want_off)
        raise AssertionError(f"tile_off[{e}] = {tile_off[e]}, the experts before it hold {want_off[e]} tiles")
    want_items = [(e, int(want_off[e]) + b, min(tpi, int(tiles[e]) - b)) for e in range(E) for b in range(0, int(tiles[e]), tpi)]
    want_n = [len(want_items), int(tiles.sum())]
    assert n_items[0] == want_n[0], f"n_items[0] = {n_items[0]}, the plan has {want_n[0]} work items"
    assert n_items[1] == want_n[1], f"n_items[1] = {n_items[1]}, the plan has {want_n[1]} gathered tiles"
    assert items.shape[0] >= 3 * want_n[0], "items shorter than the work list"
    got_items = items[:3 * want_n[0]].reshape(-1, 3)
    want_arr = np.asarray(want_items, dtype=np.int64).reshape(-1, 3)
    if (got_items != want_arr).any():
        w = _first((got_items != want_arr).any(axis=1))[0]
        raise AssertionError(f"items[{w}] = {tuple(int(v) for v in got_items[w])}, expected (expert, first tile, tiles) = {want_items[w]}")

    lo = 16 * want_off[pair_e]
    outside = (posmap < lo) | (posmap >= lo + want_cnt[pair_e])
    if outside.any():
        m, r = _first(outside)
        raise AssertionError(f"posmap[{m}][{r}] = {posmap[m, r]} outside the rows of expert {pair_e[m, r]}: "
                             f"[{lo[m, r]}, {lo[m, r] + want_cnt[pair_e[m, r]]})")
    flat = posmap.ravel()
    order = np.argsort(flat, kind="stable")
    dup = np.nonzero(np.diff(flat[order]) == 0)[0]
    if dup.size:
        a, b = sorted((int(order[dup[0]]), int(order[dup[0] + 1])))
        raise AssertionError(f"posmap[{a // top_k}][{a % top_k}] and posmap[{b // top_k}][{b % top_k}] both name gathered row {flat[a]}")
    rows = np.repeat(np.arange(P, dtype=np.int64), top_k).reshape(P, top_k)
    if (src_row[posmap] != rows).any():
        m, r = _first(src_row[posmap] != rows)
        raise AssertionError(f"src_row[{posmap[m, r]}] = {src_row[posmap[m, r]]}, it is the slot of pair ({m}, {r})")
    got_w = row_w[posmap]
    differ = ~((got_w == pair_w) | (np.isnan(got_w) & np.isnan(pair_w)))
    if differ.any():
        m, r = _first(differ)
        raise AssertionError(f"row_w[{posmap[m, r]}] = {got_w[m, r]}, pair ({m}, {r}) has weight {pair_w[m, r]}")
    free = np.ones(slots, dtype=bool)
    free[flat] = False
    stale = free & ((src_row[:slots] != -1) | ~(row_w[:slots] == 0))
    if stale.any():
        s, = _first(stale)
        raise AssertionError(f"padding slot {s} holds src_row = {src_row[s]}, row_w = {row_w[s]} (expected -1, 0)")
    return dict(cnt=want_cnt, tiles=tiles, tile_off=want_off, n_items=want_n, items=want_items)


FLT_MAX = 3.4028234663852886e38


def expert_act_ref(x, gate_e, up_e, fp32_range: bool = False):
    """One expert's gate/up stage in fp64 with the kernels' rounding points (tf:modeling_qwen3.py:82 — the two Linear
    outputs are bf16, silu is rounded, the product is rounded again): bf16(bf16(silu(bf16(gate_e x))) * bf16(up_e x)).
    x [rows, H], gate_e / up_e [I, H] hold bf16 values in fp64; returns [rows, I] bf16 values in fp64.
    fp32_range: the model evaluates silu in fp32, where exp(-g) overflows for g < -88.72 and g / (1 + inf) is -0 in any
    fp32 evaluation (torch's included), while fp64 still holds |silu| <= 89 e^-89 = 2e-37: those elements are -0 here
    too.  For a comparison in bf16 steps; a bound relative to the sums' magnitude does not see the difference."""
    gb, ub = rbf(x @ gate_e.T), rbf(x @ up_e.T)
    ex = torch.exp(-gb)
    silu = gb / (1.0 + ex)
    if fp32_range:
        silu = torch.where(ex > FLT_MAX, torch.full_like(silu, -0.0), silu)
    return rbf(rbf(silu) * ub)


def moe_rows_ref(x, gate, up, down, pair_e, pair_w):
    """The routed MLP rows of given pairs, expert by expert in fp64 with the roundings of k_pgemm's epilogues:
    out[m, r] = w[m, r] * down_e(bf16(bf16(silu(bf16(gate_e x_m))) * bf16(up_e x_m))), e = pair_e[m, r].
    x [P, H], gate / up [E, I, H], down [E, H, I] hold bf16 values in fp64.  Returns (out, mag) [P, top_k, H] fp64:
    mag[m, r, n] = sum_i |down_e[n, i]| |act_i|, the scale of the error bounds."""
    P, top_k = pair_e.shape
    H = x.shape[1]
    out = torch.zeros(P, top_k, H, dtype=F64, device=x.device)
    mag = torch.zeros_like(out)
    w = pair_w.to(F64).to(x.device)
    for e in range(gate.shape[0]):
        m, r = torch.nonzero(pair_e.to(x.device) == e, as_tuple=True)
        if m.numel() == 0:
            continue
        act = expert_act_ref(x[m], gate[e], up[e])
        out[m, r] = w[m, r][:, None] * (act @ down[e].T)
        mag[m, r] = act.abs() @ down[e].abs().T
    return out, mag
