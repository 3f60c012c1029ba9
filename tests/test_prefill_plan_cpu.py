"""prefill_plan_ref checks something before it judges a kernel: its routing agrees with torch.topk where that is
unambiguous and resolves ties by index, check_plan accepts a plan built the plain way and rejects every single
corruption of one, and every dense case of test_hip_prefill_forms reaches the block form it is there for.  CPU only."""
import numpy as np
import pytest
import torch

import prefill_plan_ref as R

BF16 = torch.bfloat16


@pytest.mark.parametrize("E,top_k,norm", [(16, 4, True), (128, 8, True), (24, 2, False), (200, 8, True), (8, 8, True), (65, 1, False)])
def test_route_agrees_with_topk_on_tie_free_logits(E, top_k, norm):
    g = torch.Generator().manual_seed(E + top_k)
    logits = R.tie_free_logits(40, E, g)
    pe, pw = R.route(logits, top_k, norm)
    prob = torch.softmax(logits.float(), dim=-1)       # Qwen3MoeTopKRouter.forward's arithmetic
    tv, ti = torch.topk(prob, top_k, dim=-1)
    if norm:
        tv = tv / tv.sum(-1, keepdim=True)
    assert torch.equal(pe, ti)
    # fp32 against fp64 in front of the same rounding: at most the neighbouring bf16 value, 2^-7 relative
    assert bool(((pw - tv.to(BF16).float()).abs() <= 2.0 ** -7 * pw).all())
    assert torch.equal(pw, pw.to(BF16).float())
    if norm:
        assert bool(((pw.double().sum(1) - 1).abs() <= top_k * 2.0 ** -9).all())


def test_route_resolves_ties_by_index_and_nan_rows_by_position():
    logits = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0],
                           [0.5, 0.5, 0.5, 0.5, 0.5],
                           [2.0, float("nan"), 1.0, 0.0, 4.0],
                           [4.0, 1.0, 4.0, 0.0, 4.0]], dtype=BF16)
    pe, pw = R.route(logits, 2, True)
    assert pe.tolist() == [[1, 2], [0, 1], [0, 1], [0, 2]]
    assert pw[0].tolist() == [0.5, 0.5] and pw[1].tolist() == [0.5, 0.5] and pw[3].tolist() == [0.5, 0.5]
    assert bool(torch.isnan(pw[2]).all()) and not bool(torch.isnan(pw[[0, 1, 3]]).any())
    pe3, pw3 = R.route(logits, 3, False)
    assert pe3[0].tolist() == [1, 2, 4] and pe3[3].tolist() == [0, 2, 4] and pe3[2].tolist() == [0, 1, 2]
    assert float(pw3[1, 0]) == 0.2001953125       # bf16(1 / 5), not renormalised


def _build(pair_e, pair_w, E, tpi, seed=0):
    """A plan of the routed pairs built the plain way; the order inside an expert is shuffled, as the kernel's may be."""
    P, k = pair_e.shape
    cnt = np.bincount(pair_e.ravel(), minlength=E)
    tiles = (cnt + 15) // 16
    off = np.cumsum(tiles) - tiles
    items = [(e, off[e] + b, min(tpi, tiles[e] - b)) for e in range(E) for b in range(0, tiles[e], tpi)]
    slots = 16 * R.max_tiles(P, k, E)
    posmap, src_row, row_w = np.zeros((P, 8), np.int32), np.full(slots, -1, np.int32), np.zeros(slots, np.float32)
    rng = np.random.default_rng(seed)
    for e in range(E):
        m, r = np.nonzero(pair_e == e)
        posmap[m, r] = 16 * off[e] + rng.permutation(m.size)
    src_row[posmap[:, :k]] = np.arange(P)[:, None]
    row_w[posmap[:, :k]] = pair_w
    return dict(cnt=cnt.astype(np.int32), tile_off=off.astype(np.int32), n_items=np.array([len(items), tiles.sum()], np.int32),
                items=np.concatenate([np.asarray(items, np.int32).ravel(), np.full(9, -7, np.int32)]), posmap=posmap,
                src_row=src_row, row_w=row_w)


def _routed(P=150, E=12, top_k=3, seed=5, skew=True):
    g = torch.Generator().manual_seed(seed)
    logits = R.tie_free_logits(P, E, g)
    if skew:
        logits[:, 4] = 12.0          # one expert with 150 rows: ten tiles, several work items
        logits[:, 7] = -40.0         # and one with none, inside the range
    pe, pw = R.route(logits, top_k, True)
    return pe.numpy(), pw.numpy()


@pytest.mark.parametrize("tpi", [4, 8])
def test_check_plan_accepts_a_plainly_built_plan(tpi):
    pe, pw = _routed()
    plan = _build(pe, pw, 12, tpi)
    st = R.check_plan(pe, pw, 12, tpi, **plan)
    assert st["cnt"][4] == 150 and st["cnt"][7] == 0 and st["n_items"][1] == int(plan["n_items"][1])
    assert [it for it in st["items"] if it[0] == 4] == [(4, int(plan["tile_off"][4]) + b, min(tpi, 10 - b)) for b in range(0, 10, tpi)]
    assert not [it for it in st["items"] if it[0] == 7]
    # a NaN row is a row like any other to the plan: NaN weights compare equal to themselves
    pw2 = pw.copy()
    pw2[17] = np.nan
    R.check_plan(pe, pw2, 12, tpi, **_build(pe, pw2, 12, tpi, seed=1))


def _swap_posmap(p, pe, pw, tpi):
    (m0, r0), (m1, r1) = (0, 0), next((m, r) for m in range(pe.shape[0]) for r in range(pe.shape[1]) if pe[m, r] != pe[0, 0])
    p["posmap"][m0, r0], p["posmap"][m1, r1] = p["posmap"][m1, r1], p["posmap"][m0, r0]
    return "posmap"


def _tile_off_by_one(p, pe, pw, tpi):
    p["tile_off"][9] += 1
    return "tile_off[9]"


def _item_too_long(p, pe, pw, tpi):
    p["items"][3 * 1 + 2] = tpi + 1
    return "items[1]"


def _item_missing(p, pe, pw, tpi):
    n = int(p["n_items"][0])
    p["items"][3 * 2:3 * (n - 1)] = p["items"][3 * 3:3 * n].copy()      # item 2 gone, the rest moved up
    p["items"][3 * (n - 1):3 * n] = -7
    return "items[2]"


def _stale_padding_src(p, pe, pw, tpi):
    s = int(np.nonzero(p["src_row"] < 0)[0][3])
    p["src_row"][s] = 11
    return f"padding slot {s}"


def _weight_moved(p, pe, pw, tpi):
    s = int(p["posmap"][20, 1])
    p["row_w"][s + 1], p["row_w"][s] = p["row_w"][s], 0.0
    return "row_w"


def _tiles_short(p, pe, pw, tpi):
    p["n_items"][1] -= 1
    return "n_items[1]"


CORRUPTIONS = [_swap_posmap, _tile_off_by_one, _item_too_long, _item_missing, _stale_padding_src, _weight_moved, _tiles_short]


@pytest.mark.parametrize("tpi", [4, 8])
@pytest.mark.parametrize("corrupt", CORRUPTIONS, ids=[c.__name__.strip("_") for c in CORRUPTIONS])
def test_check_plan_sees_one_wrong_entry(corrupt, tpi):
    pe, pw = _routed()
    plan = _build(pe, pw, 12, tpi)
    R.check_plan(pe, pw, 12, tpi, **plan)
    named = corrupt(plan, pe, pw, tpi)
    with pytest.raises(AssertionError) as err:
        R.check_plan(pe, pw, 12, tpi, **plan)
    print(f"[parity] {corrupt.__name__.strip('_')}: {err.value}")
    assert named in str(err.value)


def test_dense_cases_reach_their_forms():
    assert [R.pgemm_form(P, N) for P, N, K, form in R.DENSE_CASES] == [form for *_, form in R.DENSE_CASES] == [128, 128, 128, 64]
    assert [R.pgemm_blocks(P, N) for P, N, *_ in R.DENSE_CASES] == [512, 536, 512, 511]
    # the shapes of test_prefill_gemm_epilogues_match_torch all take the 64-row form
    assert {R.pgemm_form(P, N) for P, N in [(200, 256), (128, 384), (1, 128), (300, 1280)]} == {64}
    # column blocks beyond the last full group of 8: the tail branch of the block-index mapping
    assert [(N // 128) % 8 for _, N, *_ in R.DENSE_CASES] == [0, 3, 0, 1]


def test_moe_rows_ref_is_the_per_pair_formula():
    g = torch.Generator().manual_seed(2)
    P, H, I, E, k = 9, 16, 8, 3, 2
    x = torch.randint(-2, 3, (P, H), generator=g).double()
    gate, up = torch.randint(-1, 2, (E, I, H), generator=g).double(), torch.randint(-1, 2, (E, I, H), generator=g).double()
    down = torch.randint(-1, 2, (E, H, I), generator=g).double()
    pe, pw = R.route(R.tie_free_logits(P, E, g), k, True)
    out, mag = R.moe_rows_ref(x, gate, up, down, pe, pw)
    for m in range(P):
        for r in range(k):
            e = int(pe[m, r])
            gb, ub = R.rbf(gate[e] @ x[m]), R.rbf(up[e] @ x[m])
            act = R.rbf(R.rbf(gb * torch.sigmoid(gb)) * ub)
            assert torch.allclose(out[m, r], pw[m, r].double() * (down[e] @ act), rtol=1e-12, atol=0)
            assert torch.allclose(mag[m, r], down[e].abs() @ act.abs(), rtol=1e-12, atol=0)
