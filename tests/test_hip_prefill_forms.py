"""The index arithmetic of csrc/prefill.hip outside its attention kernel, against fp64 (tests/prefill_plan_ref.py):

  A  the dense k_pgemm at the shapes that reach its 128-row form (two LDS stages, PER == 8 wait counts, nby = mtiles / 8)
     with and without the tail branch of the block-index mapping, and the 64-row form just under the switch;
  B  k_pmoe_plan beyond one pass of 8 x 1024 pairs, with more than 64 and with 256 experts, experts without rows inside
     the range, top_k == E, one expert holding 132 tiles, a NaN row, a reused scratch — judged by check_plan;
  C  the grouped GEMMs with more than one column block and re-staged LDS buffers, both operand forms of gate/up, the
     gather, and the combine in both of its forms on integers;
  D  ops.prefill_moe_mlp as NativeTarget calls it, on a scratch made for more rows.

Integer operands make every fp32 sum exact, so a wrong fragment, tile, k-step or block index shows as a wrong integer;
the bounds of the randn runs follow from the rounding points and are stated where they are applied."""
import pytest
import torch

import helpers as H
import prefill_plan_ref as R

pytestmark = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def dev():
    return torch.device("cuda", 0)


def _within(name, got, ref, bound):
    """|got - ref| <= bound per element (fp64 tensors); prints the worst ratio, names the first element beyond it."""
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    print(f"[parity] {name}: worst |err| / bound = {float(ratio.max()):.3g}")
    if bool(bad.any()):
        i = tuple(int(v) for v in torch.nonzero(bad)[0])
        raise AssertionError(f"{name}: element {i}: got {float(got[i])!r}, fp64 {float(ref[i])!r}, bound {float(bound[i]):.3g} "
                             f"({int(bad.sum())} of {bad.numel()} beyond it)")


def _bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ A: dense k_pgemm
@pytest.mark.parametrize("P,N,K,form", R.DENSE_CASES, ids=[f"P{P}-N{N}-K{K}-rows{f}" for P, N, K, f in R.DENSE_CASES])
def test_dense_gemm_block_forms(P, N, K, form):
    """dfl_prefill_gemm_rows / _resid (with tap) / _silu (I = N / 2) at shapes that reach the intended block form, strided
    outputs (ldo = N + 8, ldtap = N + 4) with sentinels.

    Integers (W in [-3, 3], X in [-2, 2], h0 in [-5, 5]): ROWS and RESID bit-equal to fp64 rounded at the kernel's rounding
    points; SILU within 2^-7 |ref| of fp64 silu(gb) * ub on the rounded sums (two bf16 roundings of at most 2^-8 / (1 + 2^-8)
    each; __expf's error is far inside the remaining 2^-16), hence exactly 0 where gb or ub is 0.  One absolute term on
    top, 2^-120 |ub|, for fp32's range: exp(-gb) overflows for gb <= -89 and the activation evaluates to -0 (as torch's fp32
    silu does) where fp64 still holds |silu| <= 89 e^-89 = 2e-37 < 2^-121; the integer sums reach -1152.
    randn: ROWS within 2^-8 |ref| + K 2^-23 sum |w||x| (one bf16 rounding, fp32 accumulation).  RESID rounds twice, the
    sum and then h0 + the rounded sum, so its first term is 2^-7 times the larger of the two values that are rounded
    (relative to |h0 + sum| alone a cancelling h0 would make any kernel fail).  SILU: the ROWS bound on gate and up carried
    through silu (slope within [-0.1, 1.1]), the activation's rounding, the product and its rounding."""
    from dflash_amd import ops
    assert R.pgemm_form(P, N) == form
    d = dev()
    g = torch.Generator(device=d).manual_seed(P + N + K)
    Pp, I = ops.prefill_rows_padded(P), N // 2
    for exact in (True, False):
        if exact:
            W = torch.randint(-3, 4, (N, K), generator=g, device=d).to(BF16)
            X = torch.randint(-2, 3, (P, K), generator=g, device=d).to(BF16)
            h0 = torch.randint(-5, 6, (Pp, N), generator=g, device=d).to(BF16)
        else:
            W = (torch.randn(N, K, generator=g, device=d) * 0.05).to(BF16)
            X = torch.randn(P, K, generator=g, device=d).to(BF16)
            h0 = torch.randn(Pp, N, generator=g, device=d).to(BF16)
        tag = f"{'int' if exact else 'randn'} {P}x{N}x{K}"
        wp = ops.pack_weight(W)
        xf = torch.full((Pp * K,), float("nan"), dtype=BF16, device=d)
        ops.prefill_norm_pack(X, P, K, None, 1e-6, xf)
        ref = X.to(F64) @ W.to(F64).T
        acc_err = K * 2.0 ** -23 * (X.to(F64).abs() @ W.to(F64).abs().T)

        obuf = torch.full((Pp, N + 8), 7.0, dtype=BF16, device=d)
        out = obuf[:, :N]
        ops.prefill_gemm_rows(wp, xf, P, N, K, out)
        assert bool((obuf[:, N:] == 7).all()) and bool((obuf[P:] == 7).all()), f"{tag}: rows wrote outside [P, N]"
        if exact:
            assert torch.equal(_bits(out[:P]), _bits(R.rbf(ref).to(BF16))), f"{tag}: integer GEMM differs"
        else:
            _within(f"rows {tag}", out[:P].to(F64), ref, 2.0 ** -8 * ref.abs() + acc_err)

        hbuf = torch.full((Pp, N + 8), 7.0, dtype=BF16, device=d)
        hbuf[:, :N] = h0
        h = hbuf[:, :N]
        tbuf = torch.full((P, N + 4), 9.0, dtype=BF16, device=d)
        tap = tbuf[:, :N]
        ops.prefill_gemm_resid(wp, xf, P, N, K, h, tap=tap)
        assert bool((hbuf[:, N:] == 7).all()) and bool((tbuf[:, N:] == 9).all()), f"{tag}: resid wrote the sentinel columns"
        assert torch.equal(_bits(h[P:]), _bits(h0[P:])), f"{tag}: resid touched rows >= P"
        assert torch.equal(_bits(tap), _bits(h[:P])), f"{tag}: the tap is not a copy of the new rows"
        total = h0[:P].to(F64) + ref
        if exact:
            assert torch.equal(_bits(h[:P]), _bits(R.rbf(h0[:P].to(F64) + R.rbf(ref)).to(BF16))), f"{tag}: integer residual add differs"
        else:
            _within(f"resid {tag}", h[:P].to(F64), total, 2.0 ** -7 * torch.maximum(ref.abs(), total.abs()) + acc_err)

        gp = ops.pack_weight_gateup(W[:I].contiguous(), W[I:].contiguous())
        act = torch.full((Pp * I,), float("nan"), dtype=BF16, device=d)
        ops.prefill_gemm_silu(gp, xf, P, I, K, act)
        rows = H.unpack_tiles(act, Pp, I)
        assert bool((rows[P:] == 0).all()), f"{tag}: silu fragments of the padded rows are not zero"
        got = rows[:P].to(F64)
        silu = lambda v: v / (1.0 + torch.exp(-v))      # noqa: E731
        if exact:
            gb, ub = R.rbf(ref[:, :I]), R.rbf(ref[:, I:])
            want = silu(gb) * ub
            assert bool((got[(gb == 0) | (ub == 0)] == 0).all()), f"{tag}: silu * up is not 0 where a factor is 0"
            lost = (got == 0) & (want != 0)
            if bool(lost.any()):
                print(f"[parity] silu {tag}: {int(lost.sum())} elements are 0 where fp64 holds up to {float(want[lost].abs().max()):.3g} "
                      f"(largest gate sum among them {float(gb[lost].max())})")
            _within(f"silu {tag}", got, want, 2.0 ** -7 * want.abs() + 2.0 ** -120 * ub.abs())
        else:
            gx, ux = ref[:, :I], ref[:, I:]
            s = silu(gx)
            d_g, d_u = 2.0 ** -8 * gx.abs() + acc_err[:, :I], 2.0 ** -8 * ux.abs() + acc_err[:, I:]
            d_s = 1.1 * d_g + 2.0 ** -8 * (s.abs() + 1.1 * d_g)
            d_p = d_s * (ux.abs() + d_u) + s.abs() * d_u
            _within(f"silu {tag}", got, s * ux, d_p + 2.0 ** -8 * ((s * ux).abs() + d_p))
        del ref, acc_err, total, got, rows


# ------------------------------------------------------------------------------------------------ B: the plan
def _stale(sc):
    """Values no plan holds, in everything the route launch must write."""
    for k in ("src_row", "items", "n_items", "cnt", "tile_off", "posmap", "pair_e"):
        sc[k].fill_(-7 if k != "src_row" else 12345)
    sc["row_w"].fill_(7.0)
    sc["pair_w"].fill_(-7.0)


def _route_and_check(ops, logits, E, top_k, rows_per_item, sc=None, stale=True):
    """ops.prefill_moe_route on given bf16 logits [P, E]; the routed pairs against R.route (experts equal; weights the same
    bf16 value or, fp32 against fp64 in front of the rounding, its neighbour: 2^-7 relative), the plan by R.check_plan."""
    P, d = logits.shape[0], dev()
    if sc is None:
        sc = ops.prefill_moe_scratch(P, 32, 64, E, top_k, (E + 127) // 128 * 128, d)
    assert int(ops.lib().dfl_prefill_moe_max_tiles(P, top_k, E)) == R.max_tiles(P, top_k, E)
    sc["rows_per_item"] = rows_per_item
    if stale:
        _stale(sc)
    sc["rlog"][:P, :E] = logits.to(d)
    ops.prefill_moe_route(sc["rlog"], P, sc, True)
    pe_ref, pw_ref = R.route(logits, top_k, True)
    pe, pw = sc["pair_e"][:P, :top_k].cpu().long(), sc["pair_w"][:P, :top_k].cpu()
    assert torch.equal(pe, pe_ref), "selected experts differ from the fp64 routing"
    nan = torch.isnan(pw_ref)
    assert torch.equal(torch.isnan(pw), nan)
    assert bool(((pw - pw_ref).abs()[~nan] <= 2.0 ** -7 * pw_ref[~nan]).all()), "routing weights beyond one bf16 step"
    assert torch.equal(pw[~nan], pw[~nan].to(BF16).float())
    if stale:
        assert bool((sc["pair_e"][:, top_k:] == -7).all()) and bool((sc["posmap"][:, top_k:] == -7).all())
    st = R.check_plan(pe.numpy(), pw.numpy(), E, rows_per_item // 16, *(sc[k].cpu().numpy() for k in
                      ("cnt", "tile_off", "n_items", "items", "posmap", "src_row", "row_w")))
    return sc, pe_ref, pw_ref, st


PLAN_CASES = [(64, 8, 1025), (65, 1, 300), (128, 8, 2100), (256, 8, 1100), (8, 8, 33)]


@pytest.mark.parametrize("rows_per_item", [64, 128])
@pytest.mark.parametrize("E,top_k,P", PLAN_CASES, ids=[f"E{E}-top{k}-P{P}" for E, k, P in PLAN_CASES])
def test_moe_plan_sizes(E, top_k, P, rows_per_item):
    """A second pass with 8 live pairs, 65 experts (a seventeenth scan lane with one expert), three passes, 256 experts with 50 + 56 of them
    serving no row (empty ranges inside and at the end, all 64 scan lanes), top_k == E."""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(E + top_k + P)
    logits = R.tie_free_logits(P, E, g)
    if E == 256:
        logits[:, 100:150] -= 30.0
        logits[:, 200:] -= 30.0
    *_, st = _route_and_check(ops, logits, E, top_k, rows_per_item)
    assert P * top_k == int(st["cnt"].sum())
    assert (P * top_k > 8192) == ((E, top_k, P) in [(64, 8, 1025), (128, 8, 2100), (256, 8, 1100)])
    if E == 256:
        assert int(st["cnt"][100:150].sum()) == 0 and int(st["cnt"][200:].sum()) == 0 and int((st["cnt"][:100] > 0).all())
        assert int(st["cnt"][150:200].min()) > 0
    if top_k == E:
        assert st["cnt"].tolist() == [P] * E


@pytest.mark.parametrize("rows_per_item", [64, 128])
def test_moe_plan_one_expert_in_every_row(rows_per_item):
    """(128, 8, 2100) with expert 37 first in every row: 132 tiles of one expert, split into 33 or 17 work items."""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(11)
    logits = R.tie_free_logits(2100, 128, g)
    logits[:, 37] = 12.0
    _, pe, _, st = _route_and_check(ops, logits, 128, 8, rows_per_item)
    assert bool((pe[:, 0] == 37).all()) and int(st["tiles"][37]) == 132
    assert len([it for it in st["items"] if it[0] == 37]) == (33 if rows_per_item == 64 else 17)


@pytest.mark.parametrize("rows_per_item", [64, 128])
def test_moe_plan_with_a_nan_row(rows_per_item):
    """One all-NaN row among 40: it takes experts 0 .. top_k - 1 with NaN weights in ITS slots; every other slot is finite."""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(12)
    E, k, P, bad = 16, 4, 40, 23
    logits = R.tie_free_logits(P, E, g)
    logits[bad] = float("nan")
    sc, pe, pw, st = _route_and_check(ops, logits, E, k, rows_per_item)
    assert pe[bad].tolist() == [0, 1, 2, 3] and bool(torch.isnan(pw[bad]).all())
    row_w, src_row = sc["row_w"].cpu(), sc["src_row"].cpu()
    nan_slots = torch.nonzero(torch.isnan(row_w)).flatten()
    assert sorted(nan_slots.tolist()) == sorted(sc["posmap"][bad, :k].tolist()) and bool((src_row[nan_slots] == bad).all())


@pytest.mark.parametrize("rows_per_item", [64, 128])
def test_moe_plan_on_a_reused_scratch(rows_per_item):
    """P = 300, then P = 70 on the same scratch: the second plan stands on its own below 16 * max_tiles(70, ...)."""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(13)
    E, k = 12, 3
    sc, *_ = _route_and_check(ops, R.tie_free_logits(300, E, g), E, k, rows_per_item,
                              sc=ops.prefill_moe_scratch(300, 32, 64, E, k, 128, dev()))
    first_tiles = int(sc["n_items"][1])
    _, _, _, st = _route_and_check(ops, R.tie_free_logits(70, E, g), E, k, rows_per_item, sc=sc, stale=False)
    assert st["n_items"][1] < first_tiles


# ------------------------------------------------------------------------------------------------ C: grouped GEMMs
def _experts(g, E, Hd, Ie):
    gate = torch.randint(-1, 2, (E, Ie, Hd), generator=g).to(BF16).to(dev())
    up = torch.randint(-1, 2, (E, Ie, Hd), generator=g).to(BF16).to(dev())
    down = torch.randint(-1, 2, (E, Hd, Ie), generator=g).to(BF16).to(dev())
    return gate, up, down


def _pack_experts(ops, gate, up, down):
    gu_e = torch.stack([ops.pack_weight_gateup(gate[e].contiguous(), up[e].contiguous()) for e in range(gate.shape[0])])
    down_e = torch.stack([ops.pack_weight(down[e].contiguous()) for e in range(down.shape[0])])
    return gu_e, down_e


def _rows_bound(pw, mag, Ie):
    """Bound of one routed row against moe_rows_ref: w 2^-7 sum |down||act| (the activation's two bf16 roundings, as in A)
    plus the fp32 accumulation of the down sum, Ie 2^-23 of the same scale."""
    return pw.to(F64).to(mag.device)[..., None] * (2.0 ** -7 + Ie * 2.0 ** -23) * mag


@pytest.mark.parametrize("rows_per_item", [64, 128])
@pytest.mark.parametrize("P,skew", [(200, False), (300, True)], ids=["P200-even", "P300-expert0-everywhere"])
def test_grouped_gemms_with_several_column_blocks(P, skew, rows_per_item):
    """Hd 256, Ie 192, 12 experts, top-3 on integers: gate/up with nbx = 3 and KT = 4, down with nbx = 2 and KT = 3, more
    than 8 work items (the second XCD round of the item mapping).  gate/up from the gathered copy and from src_row + zeros
    are bit-equal; every routed slot of out32 against moe_rows_ref within _rows_bound; padding slots exactly 0; slots
    beyond the gathered tiles untouched."""
    from dflash_amd import ops
    Hd, Ie, E, k = 256, 192, 12, 3
    g = torch.Generator().manual_seed(7 + P)
    d = dev()
    x = torch.randint(-2, 3, (P, Hd), generator=g).to(BF16).to(d)
    gate, up, down = _experts(g, E, Hd, Ie)
    logits = R.tie_free_logits(P, E, g)
    if skew:
        logits[:, 0] = 12.0
    Pp = ops.prefill_rows_padded(P)
    xr = torch.zeros(Pp, Hd, dtype=BF16, device=d)
    xr[:P] = x
    xf = torch.full((Pp * Hd,), float("nan"), dtype=BF16, device=d)
    ops.prefill_norm_pack(xr, P, Hd, None, 1e-6, xf)
    gu_e, down_e = _pack_experts(ops, gate, up, down)
    sc, pe, pw, st = _route_and_check(ops, logits, E, k, rows_per_item, sc=ops.prefill_moe_scratch(P, Hd, Ie, E, k, 128, d))
    n_items, n_tiles = st["n_items"]
    assert n_items > 8
    if skew:
        assert int(st["cnt"][0]) == P
    for key in ("xg", "act_g", "out32"):
        sc[key].fill_(float("nan"))
    L, s0 = ops.lib(), 0
    ops.check(L.dfl_prefill_moe_gather(xf.data_ptr(), P, Hd, k, E, sc["src_row"].data_ptr(), sc["n_items"].data_ptr(),
                                       sc["xg"].data_ptr(), s0), "gather")
    srow = sc["src_row"][:n_tiles * 16].long()
    xg = H.unpack_tiles(sc["xg"][:n_tiles * 16 * Hd], n_tiles * 16, Hd)
    assert torch.equal(_bits(xg), _bits(torch.where((srow >= 0)[:, None], x[srow.clamp_min(0)], torch.zeros_like(xg)))), "gathered rows differ"
    ops.check(L.dfl_prefill_moe_gemm_silu(gu_e.data_ptr(), gu_e.stride(0), sc["xg"].data_ptr(), sc["items"].data_ptr(),
                                          sc["n_items"].data_ptr(), sc["max_items"], Ie, Hd, sc["act_g"].data_ptr(), rows_per_item,
                                          None, None, s0), "silu (gathered copy)")
    from_copy = sc["act_g"][:n_tiles * 16 * Ie].clone()
    assert not bool(torch.isnan(from_copy.float()).any()), "a gathered tile's activations were not written"
    sc["act_g"].fill_(float("nan"))
    ops.check(L.dfl_prefill_moe_gemm_silu(gu_e.data_ptr(), gu_e.stride(0), xf.data_ptr(), sc["items"].data_ptr(),
                                          sc["n_items"].data_ptr(), sc["max_items"], Ie, Hd, sc["act_g"].data_ptr(), rows_per_item,
                                          sc["src_row"].data_ptr(), sc["zeros"].data_ptr(), s0), "silu (gather in the addresses)")
    assert torch.equal(_bits(sc["act_g"][:n_tiles * 16 * Ie]), _bits(from_copy)), "the two operand forms of gate/up differ"
    ops.check(L.dfl_prefill_moe_gemm_down(down_e.data_ptr(), down_e.stride(0), sc["act_g"].data_ptr(), sc["items"].data_ptr(),
                                          sc["n_items"].data_ptr(), sc["max_items"], Hd, Ie, sc["row_w"].data_ptr(),
                                          sc["out32"].data_ptr(), rows_per_item, s0), "down")
    ref, mag = R.moe_rows_ref(x.to(F64), gate.to(F64), up.to(F64), down.to(F64), pe.to(d), pw.to(d))
    out32 = sc["out32"]
    got = out32[sc["posmap"][:P, :k].long()].to(F64)
    _within(f"out32 P={P} rows_per_item={rows_per_item}", got, ref, _rows_bound(pw, mag, Ie))
    assert bool((out32[:n_tiles * 16][srow < 0] == 0).all()), "a padding slot of out32 is not 0"
    assert int((srow < 0).sum()) == n_tiles * 16 - P * k
    assert bool(torch.isnan(out32[n_tiles * 16:]).all()), "out32 written beyond the gathered tiles"


@pytest.mark.parametrize("top_k", [1, 3, 8])
def test_combine_is_exact_on_integers(top_k):
    """dfl_prefill_moe_combine on integer out32 (exact fp32 sums; |sum| reaches 480, so the bf16 roundings act): h with a
    strided tap bit-equal to bf16(h0 + bf16(sum)); the sum_out form bit-equal to the fp64 sum with h and tap untouched.
    H = 1280: the column loop of a row's 256 threads runs twice."""
    from dflash_amd import ops
    P, Hc = 37, 1280
    g = torch.Generator().manual_seed(20 + top_k)
    d = dev()
    slots = P * top_k + 40
    out32 = torch.randint(-60, 61, (slots, Hc), generator=g).float().to(d)
    posmap = torch.randint(0, slots, (P, 8), generator=g).to(torch.int32)      # (columns >= top_k: valid slots, never to be read)
    posmap[:, :top_k] = torch.randperm(slots, generator=g)[:P * top_k].view(P, top_k).to(torch.int32)
    posmap = posmap.to(d)
    h0 = torch.randint(-5, 6, (P + 3, Hc), generator=g).to(BF16).to(d)
    hbuf = torch.full((P + 3, Hc + 8), 7.0, dtype=BF16, device=d)
    hbuf[:, :Hc] = h0
    tbuf = torch.full((P, Hc + 4), 9.0, dtype=BF16, device=d)
    h, tap = hbuf[:, :Hc], tbuf[:, :Hc]
    sums = out32.to(F64)[posmap[:, :top_k].long()].sum(dim=1)
    L = ops.lib()
    before_h, before_t = hbuf.clone(), tbuf.clone()
    sum_out = torch.full((P, Hc), float("nan"), dtype=F32, device=d)
    ops.check(L.dfl_prefill_moe_combine(out32.data_ptr(), posmap.data_ptr(), P, Hc, top_k, h.data_ptr(), h.stride(0),
                                        tap.data_ptr(), tap.stride(0), sum_out.data_ptr(), 0), "combine (sum_out)")
    assert torch.equal(sum_out.to(F64), sums), "sum_out differs from the fp64 sum"
    assert torch.equal(_bits(hbuf), _bits(before_h)) and torch.equal(_bits(tbuf), _bits(before_t)), "the sum_out form touched h or the tap"
    sum_only = torch.full((P, Hc), float("nan"), dtype=F32, device=d)       # as NativeTarget._moe_mlp_shared calls it: no h at all
    ops.check(L.dfl_prefill_moe_combine(out32.data_ptr(), posmap.data_ptr(), P, Hc, top_k, None, 0, None, 0,
                                        sum_only.data_ptr(), 0), "combine (sum_out, no h)")
    assert torch.equal(sum_only, sum_out)
    ops.check(L.dfl_prefill_moe_combine(out32.data_ptr(), posmap.data_ptr(), P, Hc, top_k, h.data_ptr(), h.stride(0),
                                        tap.data_ptr(), tap.stride(0), None, 0), "combine")
    want = R.rbf(h0[:P].to(F64) + R.rbf(sums)).to(BF16)
    assert torch.equal(_bits(h[:P]), _bits(want)), "h differs from bf16(h0 + bf16(sum))"
    assert torch.equal(_bits(tap), _bits(want)), "the tap is not a copy of the new rows"
    assert torch.equal(_bits(h[P:]), _bits(h0[P:])) and bool((hbuf[:, Hc:] == 7).all()) and bool((tbuf[:, Hc:] == 9).all())


# ------------------------------------------------------------------------------------------------ D: the wrapper
def test_prefill_moe_mlp_on_a_scratch_made_for_more_rows():
    """ops.prefill_moe_mlp with a scratch made for 300 rows and the wrapper's own rows_per_item, at P = 300 and then P = 70.
    Integer x and experts, a small random bf16 router.  rlog against the fp64 router GEMM with A's ROWS bound; the routing
    reference reads the logits the launch wrote (rlog is the kernel's own rounding of the router GEMM); h_io against
    h0 + bf16(sum of moe_rows_ref) within one bf16 step of the result plus the slots' _rows_bound; the strided tap is a
    copy; rows >= P and the sentinel columns are untouched."""
    from dflash_amd import ops
    Hd, Ie, E, k, RC = 256, 192, 12, 3, 128
    g = torch.Generator().manual_seed(31)
    d = dev()
    gate, up, down = _experts(g, E, Hd, Ie)
    gu_e, down_e = _pack_experts(ops, gate, up, down)
    wr = torch.zeros(RC, Hd, dtype=BF16, device=d)
    wr[:E] = (torch.randn(E, Hd, generator=g) * 0.1).to(BF16).to(d)
    router_wp = ops.pack_weight(wr)
    sc = ops.prefill_moe_scratch(300, Hd, Ie, E, k, RC, d)
    assert sc["rows_per_item"] == 128
    for P in (300, 70):
        Pp = ops.prefill_rows_padded(P)
        x = torch.randint(-2, 3, (P, Hd), generator=g).to(BF16).to(d)
        h0 = torch.randint(-3, 4, (Pp, Hd), generator=g).to(BF16).to(d)
        xr = torch.zeros(Pp, Hd, dtype=BF16, device=d)
        xr[:P] = x
        xf = torch.full((Pp * Hd,), float("nan"), dtype=BF16, device=d)
        ops.prefill_norm_pack(xr, P, Hd, None, 1e-6, xf)
        hbuf = torch.full((Pp, Hd + 8), 7.0, dtype=BF16, device=d)
        hbuf[:, :Hd] = h0
        tbuf = torch.full((P, Hd + 4), 9.0, dtype=BF16, device=d)
        h, tap = hbuf[:, :Hd], tbuf[:, :Hd]
        ops.prefill_moe_mlp(router_wp, gu_e, down_e, xf, P, Hd, Ie, E, k, True, h, sc, tap=tap)
        x64, w64 = x.to(F64), wr[:E].to(F64)
        lref = x64 @ w64.T
        rlog = sc["rlog"][:P, :E].clone()
        _within(f"router logits P={P}", rlog.to(F64), lref, 2.0 ** -8 * lref.abs() + Hd * 2.0 ** -23 * (x64.abs() @ w64.abs().T))
        pe, pw = R.route(rlog.cpu(), k, True)
        got_e, got_w = sc["pair_e"][:P, :k].cpu().long(), sc["pair_w"][:P, :k].cpu()
        assert torch.equal(got_e, pe), f"P={P}: selected experts differ from the fp64 routing of the launch's logits"
        assert bool(((got_w - pw).abs() <= 2.0 ** -7 * pw).all()), f"P={P}: routing weights beyond one bf16 step of the fp64 routing"
        R.check_plan(got_e.numpy(), got_w.numpy(), E, sc["rows_per_item"] // 16, *(sc[key].cpu().numpy() for key in
                     ("cnt", "tile_off", "n_items", "items", "posmap", "src_row", "row_w")))
        ref, mag = R.moe_rows_ref(x64, gate.to(F64), up.to(F64), down.to(F64), pe.to(d), pw.to(d))
        want = R.rbf(h0[:P].to(F64) + R.rbf(ref.sum(dim=1)))
        _within(f"h_io P={P}", h[:P].to(F64), want, R.bf16_ulp(want) + _rows_bound(pw, mag, Ie).sum(dim=1))
        assert torch.equal(_bits(tap), _bits(h[:P])), f"P={P}: the tap is not a copy of the new rows"
        assert torch.equal(_bits(h[P:]), _bits(h0[P:])), f"P={P}: rows >= P touched"
        assert bool((hbuf[:, Hd:] == 7).all()) and bool((tbuf[:, Hd:] == 9).all())
