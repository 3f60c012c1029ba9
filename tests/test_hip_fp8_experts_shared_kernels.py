"""The two grouped expert GEMMs on e4m3 codes — dfl_moe_grouped_gate_up and dfl_moe_grouped_down with an e4m3 descriptor
(csrc/prefill.hip: k_pgemm<PEPI_SILU / PEPI_SCALE32, MW, NST, grouped, W8>), what the shared MoE pass of a verify over 2..4
tiles launches — against the bf16 launch of the same entry point on the dequantised weights (bit for bit) and against
exact arithmetic in fp64 ("The experts").

Why (a) is bit-equality.  A code c is an e4m3 value, exact in bf16, and the scales here are powers of two, so w = c * s is
exact in bf16 as well.  The W8 form stages the codes as they are and converts them in front of the MFMAs; it keeps the
bf16 form's k-steps and their order into every accumulator.  Scaling every A operand of a row by 2^k scales every product
and every fp32 partial sum of that row by 2^k without touching a rounding (no overflow or underflow in range here:
|c| <= 2, 2^-10 <= s <= 2^-6), so the bf16 launch holds S16 = s * S8 exactly, and the W8 epilogue multiplies S8 by s in
front of its first rounding point: rbf(S8 * s) for gate/up, rw * (S8 * s) for down.  Everything behind is the same code on
the same bits.

The work list is dfl_prefill_moe_route's, judged by check_plan (tests/prefill_plan_ref.py).  Experts that serve no row
hold code 0x7F (e4m3 NaN) throughout and NaN scales, outputs are pre-filled with NaN: a stray read or a missing write
shows.  Padding rows come from zeros_1k (gather in the addresses) or are zero in the gathered copy."""
import pytest
import torch

import prefill_plan_ref as R

pytestmark = pytest.mark.gpu
BF16, F32, F64, U8, F8, I32 = torch.bfloat16, torch.float32, torch.float64, torch.uint8, torch.float8_e4m3fn, torch.int32
SCALES = (1.0, 1.5, 0.75, 2.0 ** -3)


def dev():
    return torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _pack_tiles(rows):
    """rows [Pp, K] (Pp % 16 == 0) -> frag16 row tiles [Pp/16][K/32][64][8], flat: the inverse of helpers.unpack_tiles."""
    Pp, K = rows.shape
    return rows.view(Pp // 16, 16, K // 32, 4, 8).permute(0, 2, 3, 1, 4).reshape(-1).contiguous()


def _unpack_tiles(xf, P, K):
    Pp = xf.numel() // K
    return xf.view(Pp // 16, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(Pp, K)[:P]


def _int_codes(shape, lim, g):
    """Random integers in [-lim, lim] as (values fp32, e4m3 codes uint8), on the device."""
    vals = torch.arange(-lim, lim + 1, dtype=F32)
    lut = vals.to(F8).view(U8)
    assert torch.equal(lut.view(F8).float(), vals)                 # small integers are e4m3 values
    idx = torch.randint(0, 2 * lim + 1, shape, generator=g, device=dev())
    return vals.to(dev())[idx], lut.to(dev())[idx]


def _pow2_codes(shape_en, K, g):
    """Random codes with |value| <= 2 and one power-of-two scale 2^-6 .. 2^-10 per row, generated on the device:
    (codes uint8 [E, N, K], scales fp32 [E, N], q * scale as bf16 [E, N, K] — exact)."""
    E, N = shape_en
    q = (torch.randint(0, 0x41, (E, N, K), generator=g, device=dev()) |
         (torch.randint(0, 2, (E, N, K), generator=g, device=dev()) << 7)).to(U8)
    sc = torch.exp2(-torch.randint(6, 11, (E, N), generator=g, device=dev()).float())
    deq = q.view(F8).float() * sc[:, :, None]
    assert torch.equal(deq, deq.to(BF16).float()) and float(q.view(F8).float().abs().max()) == 2.0
    return q, sc, deq.to(BF16)


def _experts8(ops, q, sc, gateup, on):
    """pack_experts_fp8, then the experts without rows poisoned: codes 0x7F throughout, NaN scales."""
    x8 = ops.pack_experts_fp8(q, sc, gateup=gateup)
    x8.wp[~on] = 0x7F
    x8.scale[~on] = float("nan")
    assert x8.scale.data_ptr() % 64 == 0
    return x8


def _pack_bf16(ops, w, gateup, on):
    E, N = w.shape[:2]
    w = torch.where(on[:, None, None], w, torch.full_like(w, float("nan")))      # (the bf16 arm's idle experts: NaN as well)
    if gateup:
        return torch.stack([ops.pack_weight_gateup(w[e, :N // 2].contiguous(), w[e, N // 2:].contiguous()) for e in range(E)])
    return torch.stack([ops.pack_weight(w[e].contiguous()) for e in range(E)])


def _logits(kind):
    """-> (E, top_k, bf16 logits [P, E]).  "skew": P 100 over 6 experts, top-2 — expert 0 in every row (100 rows: two work
    items of 4 + 3 tiles at 64 rows per item, one of 7 tiles at 128), expert 4 in rows 0..4 only (one tile: `ntl` 1 of 4 /
    of 8, the block re-reads it), expert 5 in no row, experts 1..3 share the rest.  "second": P 40 over the same experts
    with expert 2 idle instead — the second plan on a reused scratch.  "a3b": 64 rows (four tiles), top-8 of 128."""
    cg = torch.Generator().manual_seed({"skew": 5, "second": 6, "a3b": 7}[kind])
    if kind == "a3b":
        return 128, 8, R.tie_free_logits(64, 128, cg)
    P = 100 if kind == "skew" else 40
    lg = R.tie_free_logits(P, 6, cg).float()
    lg[:, 0] = 12.0
    lg[:, 5 if kind == "skew" else 2] -= 40.0
    lg[:, 4] -= 40.0
    lg[:5, 4] = 11.0
    return 6, 2, lg.to(BF16)


def _route(ops, kind, Hd, Ie, rows_per_item, g, sc=None):
    """dfl_prefill_moe_route on the logits of `kind` into a scratch for Hd x Ie experts -> (scratch, pair_e, pair_w,
    check_plan's summary, active mask [E])."""
    E, top_k, lg = _logits(kind)
    P = lg.shape[0]
    if sc is None:
        sc = ops.prefill_moe_scratch(100 if kind != "a3b" else 64, Hd, Ie, E, top_k, 128, dev())
    if rows_per_item is not None:
        sc["rows_per_item"] = rows_per_item
    sc["rlog"][:P, :E] = lg.to(dev())
    ops.prefill_moe_route(sc["rlog"], P, sc, True)
    pe, pw = R.route(lg, top_k, True)
    assert torch.equal(sc["pair_e"][:P, :top_k].cpu().long(), pe)
    pw = sc["pair_w"][:P, :top_k].cpu()                      # (the launch's own bf16 weights: what row_w holds)
    st = R.check_plan(pe.numpy(), pw.numpy(), E, sc["rows_per_item"] // 16, *(sc[k].cpu().numpy() for k in
                      ("cnt", "tile_off", "n_items", "items", "posmap", "src_row", "row_w")))
    on = torch.from_numpy(st["cnt"] > 0).to(dev())
    if kind == "skew":
        assert st["cnt"].tolist()[0] == 100 and st["cnt"][4] == 5 and st["cnt"][5] == 0 and int(on.sum()) == 5
        tiles = sorted(it[2] for it in st["items"] if it[0] == 0)
        assert tiles == ([3, 4] if sc["rows_per_item"] == 64 else [7]) and [it[2] for it in st["items"] if it[0] == 4] == [1]
    if kind == "second":
        assert st["cnt"][2] == 0 and st["cnt"][5] > 0
    if kind == "a3b":
        assert int(on.sum()) >= 100 and sc["rows_per_item"] == 64             # the shared pass's own form at this geometry
    return sc, pe, pw, st, on


def _x_tiles(ops, x):
    """x [P, K] bf16 -> the ungathered frag16 row tiles, padded with zero rows to a multiple of 128 rows."""
    P, K = x.shape
    Pp = ops.prefill_rows_padded(P)
    xr = torch.zeros(Pp, K, dtype=BF16, device=dev())
    xr[:P] = x
    return _pack_tiles(xr)


def _gather(ops, xf, sc, P, K, n_tiles):
    L = ops.lib()
    sc["xg"].fill_(float("nan"))
    ops.check(L.dfl_prefill_moe_gather(xf.data_ptr(), P, K, sc["top_k"], sc["E"], sc["src_row"].data_ptr(),
                                       sc["n_items"].data_ptr(), sc["xg"].data_ptr(), 0), "gather")
    assert not bool(torch.isnan(sc["xg"][:n_tiles * 16 * K].float()).any())


def _gate_up(ops, w, xf, sc, K, n_tiles, gather):
    """One launch into a NaN-filled act_g -> the gathered tiles' activation rows [n_tiles * 16, I]; nothing beyond them
    is written."""
    I = sc["I"]
    sc["act_g"].fill_(float("nan"))
    ops.moe_grouped_gate_up(w, xf if gather else sc["xg"], sc, K, gather=gather)
    act = sc["act_g"]
    assert bool(torch.isnan(act[n_tiles * 16 * I:].float()).all()), "act_g written beyond the gathered tiles"
    rows = _unpack_tiles(act[:n_tiles * 16 * I], n_tiles * 16, I).clone()
    assert bool(torch.isfinite(rows.float()).all()), "a gathered tile's activations are NaN or were not written"
    return rows


def _check_gate_up(ops, kind, I, K, rows_per_item, g, sc=None):
    sc, pe, pw, st, on = _route(ops, kind, K, I, rows_per_item, g, sc)
    E, P = sc["E"], pe.shape[0]
    n_tiles = st["n_items"][1]
    srow = sc["src_row"][:n_tiles * 16].long()
    owner = torch.zeros(n_tiles * 16, dtype=torch.long, device=dev())
    for e, t0, nt in st["items"]:
        owner[t0 * 16:(t0 + nt) * 16] = e
    # ---- (a) bit-equality with the bf16 launch of the same entry point on q * scale, both operand forms
    q, s2, deq = _pow2_codes((E, 2 * I), K, g)
    x8, gu_p = _experts8(ops, q, s2, True, on), _pack_bf16(ops, deq, True, on)
    x = torch.randn(P, K, generator=g, device=dev()).to(BF16)
    xf = _x_tiles(ops, x)
    _gather(ops, xf, sc, P, K, n_tiles)
    a8 = _gate_up(ops, x8, xf, sc, K, n_tiles, gather=True)
    assert torch.equal(_bits(a8), _bits(_gate_up(ops, gu_p, xf, sc, K, n_tiles, gather=True))), "W8 differs from bf16 on q * scale"
    assert torch.equal(_bits(a8), _bits(_gate_up(ops, x8, xf, sc, K, n_tiles, gather=False))), "the two operand forms differ"
    assert torch.equal(_bits(a8), _bits(_gate_up(ops, gu_p, xf, sc, K, n_tiles, gather=False)))
    assert bool((a8[srow < 0] == 0).all()), "a padding row's activations are not 0"
    assert float(a8.float().abs().max()) > 0
    del q, s2, deq, x8, gu_p
    # ---- (b) exact sums: integer codes |q| <= 4, integer rows |x| <= 2, scales from SCALES
    qv, qc = _int_codes((E, 2 * I, K), 4, g)
    s4 = torch.tensor(SCALES, device=dev())[torch.randint(0, 4, (E, 2 * I), generator=g, device=dev())]
    x8 = _experts8(ops, qc, s4, True, on)
    x = torch.randint(-2, 3, (P, K), generator=g, device=dev()).float()
    xf = _x_tiles(ops, x.to(BF16))
    _gather(ops, xf, sc, P, K, n_tiles)
    worst = 0.0
    for gather in (True, False):
        got = _gate_up(ops, x8, xf, sc, K, n_tiles, gather=gather).float()
        xg = torch.where((srow >= 0)[:, None], x[srow.clamp_min(0)], torch.zeros((), device=dev()))
        for e in on.nonzero()[:, 0].tolist():
            m = owner == e
            s = (xg[m].double() @ qv[e].double().T) * s4[e].double()             # exact: integers, then a 2-bit scale
            assert torch.equal(s, s.float().double())
            gate, up = s.float().to(BF16).chunk(2, dim=-1)
            ref = (torch.nn.functional.silu(gate.float()).to(BF16).float() * up.float()).to(BF16).float()
            assert float(ref.abs().max()) > 0
            err = float((got[m] - ref).abs().max() / ref.abs().max())
            assert err <= 2e-2, (e, gather, err)                                  # (a NaN fails this too)
            worst = max(worst, err)
        assert bool((got[srow < 0] == 0).all())
    print(f"[parity] grouped gate/up W8 {kind} I {I} K {K} rows_per_item {sc['rows_per_item']}: worst activation error "
          f"{worst:.3e} of the expert's largest value")
    return sc


def _down(ops, w, sc, N, n_tiles):
    sc["out32"].fill_(float("nan"))
    ops.moe_grouped_down(w, sc, N)
    out = sc["out32"]
    assert bool(torch.isnan(out[n_tiles * 16:]).all()), "out32 written beyond the gathered tiles"
    assert bool(torch.isfinite(out[:n_tiles * 16]).all()), "a gathered row of out32 is NaN or was not written"
    return out[:n_tiles * 16].clone()


def _check_down(ops, kind, N, I, rows_per_item, g, sc=None):
    sc, pe, pw, st, on = _route(ops, kind, N, I, rows_per_item, g, sc)
    E, P, top_k = sc["E"], pe.shape[0], sc["top_k"]
    n_tiles = st["n_items"][1]
    srow = sc["src_row"][:n_tiles * 16].long()
    row_w = sc["row_w"][:n_tiles * 16].clone()
    owner = torch.zeros(n_tiles * 16, dtype=torch.long, device=dev())
    for e, t0, nt in st["items"]:
        owner[t0 * 16:(t0 + nt) * 16] = e
    full = sc["act_g"].numel() // I                               # the scratch's rows: the tiles beyond n_tiles hold NaN

    def set_act(rows):
        a = torch.full((full, I), float("nan"), dtype=BF16, device=dev())
        a[:n_tiles * 16] = rows
        sc["act_g"].copy_(_pack_tiles(a))

    # ---- (a)
    q, s2, deq = _pow2_codes((E, N), I, g)
    x8, dn_p = _experts8(ops, q, s2, False, on), _pack_bf16(ops, deq, False, on)
    set_act(torch.randn(n_tiles * 16, I, generator=g, device=dev()).to(BF16))
    o8 = _down(ops, x8, sc, N, n_tiles)
    assert torch.equal(_bits(o8), _bits(_down(ops, dn_p, sc, N, n_tiles))), "W8 differs from bf16 on q * scale"
    assert bool((o8[srow < 0] == 0).all()) and float(o8.abs().max()) > 0         # padding rows: routing weight 0
    del q, s2, deq, x8, dn_p
    # ---- (b) integer activations |a| <= 4 and codes |q| <= 4: a sum is an integer below 16 I <= 2^13, times a scale of
    # at most two bits, times the row's routing weight, a bf16 value of 8 bits: under 24 bits, exact in fp32 — asserted
    qv, qc = _int_codes((E, N, I), 4, g)
    s4 = torch.tensor(SCALES, device=dev())[torch.randint(0, 4, (E, N), generator=g, device=dev())]
    x8 = _experts8(ops, qc, s4, False, on)
    a = torch.randint(-4, 5, (n_tiles * 16, I), generator=g, device=dev()).float()
    set_act(a.to(BF16))
    o8 = _down(ops, x8, sc, N, n_tiles)
    assert torch.equal(row_w, row_w.to(BF16).float())
    ref = torch.zeros(n_tiles * 16, N, dtype=F64, device=dev())
    for e in on.nonzero()[:, 0].tolist():
        m = owner == e
        ref[m] = row_w[m].double()[:, None] * ((a[m].double() @ qv[e].double().T) * s4[e].double()[None, :])
    assert torch.equal(ref, ref.float().double())                 # the bit budget: the reference is an fp32 number
    assert float(ref.abs().max()) > 0
    assert torch.equal(o8, ref.float()), "out32 differs from the fp64 reference"
    # every routed pair finds its row (what dfl_prefill_moe_combine reads)
    assert torch.equal(o8[sc["posmap"][:P, :top_k].long()], ref.float()[sc["posmap"][:P, :top_k].long()])
    return sc


GU_SHAPES = [(64, 64), (192, 192), (64, 320)]        # (I, K): N = 2 I = 128 / 384 / 128 columns; KT = 1 / 3 / 5
DOWN_SHAPES = [(128, 64), (384, 192), (128, 320)]    # (N, I): the same column blocks and K steps for the down projection


@pytest.mark.parametrize("rows_per_item", [64, 128])
@pytest.mark.parametrize("I,K", GU_SHAPES, ids=["N128-K64-prologue-only", "N384-K192-three-stages", "N128-K320-ring-wraps"])
def test_grouped_gate_up_fp8(I, K, rows_per_item):
    """dfl_moe_grouped_gate_up (e4m3) on the "skew" routing (_logits): K = 64 (one K step: the prologue is the whole
    loop), K = 192 (exactly the three stages of the 64-row form), K = 320 (the ring wraps twice; the two-stage 128-row
    form reuses both buffers), one and three column blocks; an item with one tile of its block, an expert over two items
    (64) / one (128), an expert without rows; from src_row + zeros and from the gathered copy.  (a) and (b) of the module
    docstring; (b)'s bar is the 2e-2 of tests/test_hip_fp8_experts_kernels.py (the kernel's __expf)."""
    from dflash_amd import ops
    _check_gate_up(ops, "skew", I, K, rows_per_item, torch.Generator(device=dev()).manual_seed(I + K + rows_per_item))


@pytest.mark.parametrize("rows_per_item", [64, 128])
@pytest.mark.parametrize("N,I", DOWN_SHAPES, ids=["N128-K64-prologue-only", "N384-K192-three-stages", "N128-K320-ring-wraps"])
def test_grouped_down_fp8(N, I, rows_per_item):
    """dfl_moe_grouped_down (e4m3), the same shapes and routing.  (a) bit-equal to the bf16 launch on q * scale; (b) the
    fp32 rows of out32 equal row_w * scale * (act . q) in fp64 bit for bit; padding rows are 0, nothing is written beyond
    the gathered tiles."""
    from dflash_amd import ops
    _check_down(ops, "skew", N, I, rows_per_item, torch.Generator(device=dev()).manual_seed(N + I + rows_per_item))


@pytest.mark.parametrize("rows_per_item", [64, 128])
def test_grouped_fp8_on_a_reused_scratch(rows_per_item):
    """Both launches on P = 100 and then on P = 40 with another idle expert, on the same scratch: the second pass stands on
    its own (stale items, rows and activations of the first are neither read nor kept)."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(77 + rows_per_item)
    sc = _check_gate_up(ops, "skew", 64, 128, rows_per_item, g)
    first = int(sc["n_items"][1])
    sc = _check_gate_up(ops, "second", 64, 128, rows_per_item, g, sc=sc)
    assert int(sc["n_items"][1]) < first
    sc = _check_down(ops, "skew", 128, 64, rows_per_item, g, sc=sc)
    _check_down(ops, "second", 128, 64, rows_per_item, g, sc=sc)


def test_grouped_fp8_at_the_operating_point():
    """E 128, top-8, 64 rows (four tiles), hidden 2048, experts of 768 — a 30B-A3B layer's shared pass, with the
    rows_per_item the scratch picks there (64) and codes generated on the device: both launches, (a) and (b)."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(30)
    sc = _check_gate_up(ops, "a3b", 768, 2048, None, g)
    del sc
    _check_down(ops, "a3b", 2048, 768, None, g)


def test_grouped_ops_refuse_mismatched_experts():
    """ops.moe_grouped_gate_up / moe_grouped_down with an Fp8Experts whose dimensions are not the launch's: an error, no
    launch."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(1)
    _, qc = _int_codes((6, 128, 64), 2, g)
    x8 = ops.pack_experts_fp8(qc, torch.ones(6, 128, device=dev()), gateup=True)
    sc = ops.prefill_moe_scratch(16, 128, 64, 6, 2, 128, dev())
    with pytest.raises(ValueError, match="fp8 experts"):
        ops.moe_grouped_gate_up(x8, torch.zeros(128 * 128, dtype=BF16, device=dev()), sc, 128, gather=True)
    with pytest.raises(ValueError, match="fp8 experts"):
        ops.moe_grouped_down(x8, sc, 256)
