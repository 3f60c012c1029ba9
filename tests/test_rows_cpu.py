"""tests/rows_ref.py without a GPU: the reference against the oracle's leaf ops, every planted fault caught by the very
helper and on the very inputs the GPU tests use (tests/test_hip_rows.py), the two eps faults NOT caught on unit-scale
rows (the blind spot of the older tests, written down), and an fp32 model of the kernels inside the bars."""
import pytest
import torch

import rows_ref as R
from oracle import dflash_oracle as O

BF16 = torch.bfloat16


# ---------------------------------------------------------------- the reference against an independent path
@pytest.mark.parametrize("Hd", [128, 1024, 5120])
def test_row_stage_matches_the_oracle(Hd):
    """h is bit-equal to the torch expression the older tests use.  The fragments are not bit-equal to O.rms_norm by
    construction: the oracle takes mean and rsqrt in fp32, the reference in fp64, so bf16(h * rstd) may flip where it
    lies within an fp32 ulp of a rounding boundary — the same bar as for a kernel applies."""
    c = R._np_case(Hd, "part_resid", "h_out", None, "unit", nsplit=3, row_off=16, seed=Hd)
    inp = R.norm_pack_inputs(c)
    ref = R.norm_pack_ref(c, inp)
    lin = (inp.part_view[0, 16:32] + inp.part_view[1, 16:32] + inp.part_view[2, 16:32]).to(BF16)
    R.assert_bits("h vs torch", ref["h"], inp.resid + lin, log=False)
    R.assert_normed("frag vs O.rms_norm", ref["frag"], O.rms_norm(inp.resid + lin, inp.w, c.eps), log=False)


@pytest.mark.parametrize("norm", [False, True])
def test_head_stage_matches_the_oracle(norm):
    """Unit-scale heads through O.rms_norm + O.rope_cos_sin + O.apply_rotary_std.  Without the norm the oracle rounds in
    the same places (bf16 products, bf16 sum) and the tables hold the same bits: bit-equal.  With it, rstd is fp32
    there and fp64 here: rare last-bit flips, the bars of assert_roped."""
    g = R.gen(11)
    n, n_q, n_kv, pos0 = 17, 4, 2, 1040
    q, k = R.unit((n, n_q, 128), g), R.unit((n, n_kv, 128), g)
    qw, kw = R.head_norm_weight(g), R.head_norm_weight(g)
    pos = pos0 + torch.arange(n)
    cos, sin = R.tables(R.TABLE_ROWS)
    c, s = O.rope_cos_sin(pos[None], O.rope_inv_freq(128, 1e6), BF16)
    assert torch.equal(torch.cat([cos[pos], cos[pos]], -1), c[0]) and torch.equal(torch.cat([sin[pos], sin[pos]], -1), s[0])
    oq, ok = q.transpose(0, 1)[None], k.transpose(0, 1)[None]
    if norm:
        oq, ok = O.rms_norm(oq, qw, 1e-6), O.rms_norm(ok, kw, 1e-6)
    oq, ok = O.apply_rotary_std(oq, ok, c, s)
    cmp = R.assert_roped if norm else R.assert_bits
    cmp("q vs oracle", R.head_stage(q, None, qw if norm else None, 1e-6, pos, cos, sin, R.TABLE_ROWS), oq[0].transpose(0, 1), log=False)
    cmp("k vs oracle", R.head_stage(k, None, kw if norm else None, 1e-6, pos, cos, sin, R.TABLE_ROWS), ok[0].transpose(0, 1), log=False)


def test_kernel_form_of_each_width():
    assert [R.norm_pack_kernel(h) for h in (8, 1024, 4096, 4104, 5120, 8192, 8200, 16384)] == [2, 2, 2, 4, 4, 4, 8, 8]
    forms = {(R.norm_pack_kernel(c.H), c.H) for c in R.norm_pack_cases()}
    assert {(2, 8), (2, 4096), (4, 4104), (4, 5120), (4, 8192), (8, 8200), (8, 16384)} <= forms


def test_every_fault_is_planted_somewhere():
    seen = set()
    for c in R.norm_pack_cases():
        seen |= set(R.norm_pack_faults(c))
    for c in R.append_cases():
        seen |= set(R.append_faults(c))
    assert seen == set(R.FAULTS), set(R.FAULTS) - seen
    assert any(c.pos0 == c.S for c in R.append_cases()) is False            # pos0 != S in every case


# ---------------------------------------------------------------- faults are seen, by the helpers the GPU tests call
def _must_fail(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f"{what}: the faulty reference passed the check")


@pytest.mark.parametrize("c", R.norm_pack_cases(), ids=lambda c: c.id)
def test_norm_pack_faults_are_seen(c):
    inp = R.norm_pack_inputs(c)
    want = R.norm_pack_ref(c, inp)
    pick = (lambda d: {"h": d["h"] if c.out != "none" else None, "frag": d["frag"]})
    R.check_norm_pack(c.id, pick(want), want, log=False)
    for f in R.norm_pack_faults(c):
        bad = R.norm_pack_ref(c, inp, fault=f)
        _must_fail(lambda: R.check_norm_pack(c.id, pick(bad), want, log=False), f"{c.id} {f}")


@pytest.mark.parametrize("c", R.append_cases(), ids=lambda c: c.id)
def test_append_faults_are_seen(c):
    inp = R.append_inputs(c)
    want = R.append_ref(c, inp)
    pick = (lambda d: {"q": d["q"] if c.q_col >= 0 else None, "k": d["k"], "v": d["v"]})
    R.check_append(c.id, pick(want), want, c.norm, log=False)
    assert torch.isfinite(want["k"][~torch.isnan(want["v"])].float()).all()   # (the clamp: no NaN table row is ever used)
    for f in R.append_faults(c):
        bad = R.append_ref(c, inp, fault=f)
        _must_fail(lambda: R.check_append(c.id, pick(bad), want, c.norm, log=False), f"{c.id} {f}")


@pytest.mark.parametrize("c", R.prefill_norm_cases(), ids=lambda c: c.id)
def test_prefill_norm_faults_are_seen(c):
    inp = R.prefill_norm_inputs(c)
    want = R.prefill_norm_ref(c, inp, c.P + 3)
    for f in R.prefill_norm_faults(c):
        bad = R.prefill_norm_ref(c, inp, c.P + 3, fault=f)
        _must_fail(lambda: R.assert_normed(c.id, bad, want, log=False), f"{c.id} {f}")


@pytest.mark.parametrize("c", R.prefill_rope_cases(), ids=lambda c: c.id)
def test_prefill_rope_faults_are_seen(c):
    inp = R.prefill_rope_inputs(c)
    want = R.prefill_rope_ref(c, inp)
    R.check_prefill_rope(c.id, want, want, c, log=False)
    assert torch.isfinite(want["k"][~torch.isnan(want["v"])].float()).all()
    for f in R.prefill_rope_faults(c):
        bad = R.prefill_rope_ref(c, inp, fault=f)
        _must_fail(lambda: R.check_prefill_rope(c.id, bad, want, c, log=False), f"{c.id} {f}")


# ---------------------------------------------------------------- the blind spot, written down
def test_eps_faults_pass_on_unit_scale_rows():
    """On unit-scale rows eps = 1e-6 / 1e-5 moves rstd by 5e-7 / 5e-6 of itself: a kernel without eps, or with 1e-6
    hard-coded, passes the very same bars.  This is what every older test of a norm fed its kernel."""
    g = R.gen(5)
    h, w = R.unit((16, 4096), g), R.norm_weight(4096, g)
    R.assert_normed("unit rows, eps dropped", R.rms(h, w, 1e-6, "eps_dropped"), R.rms(h, w, 1e-6), log=False)
    R.assert_normed("unit rows, eps fixed", R.rms(h, w, 1e-5, "eps_fixed_1e-6"), R.rms(h, w, 1e-5), log=False)
    x, hw = R.unit((64, 8, 128), g), R.head_norm_weight(g)
    pos = 1040 + torch.arange(64)
    cos, sin = R.tables(R.TABLE_ROWS)
    for eps, f in ((1e-6, "eps_dropped"), (1e-5, "eps_fixed_1e-6")):
        R.assert_roped(f"unit heads, {f}", R.head_stage(x, None, hw, eps, pos, cos, sin, R.TABLE_ROWS, f),
                       R.head_stage(x, None, hw, eps, pos, cos, sin, R.TABLE_ROWS), log=False)
    # ... and the same two faults on small rows do not
    for eps, f in ((1e-6, "eps_dropped"), (1e-5, "eps_dropped"), (1e-5, "eps_fixed_1e-6")):
        hs = h * R.small_scale(eps)
        R.assert_small(hs, eps)
        _must_fail(lambda: R.assert_normed("small", R.rms(hs, w, eps, f), R.rms(hs, w, eps), log=False), f"small rows {f}")
        xs = x * R.small_scale(eps)
        R.assert_small(xs, eps)
        _must_fail(lambda: R.assert_roped("small", R.head_stage(xs, None, hw, eps, pos, cos, sin, R.TABLE_ROWS, f),
                                          R.head_stage(xs, None, hw, eps, pos, cos, sin, R.TABLE_ROWS), log=False), f"small heads {f}")


# ---------------------------------------------------------------- the bars have headroom
@pytest.mark.parametrize("Hd", [128, 1024, 5120, 16384])
@pytest.mark.parametrize("family", ["unit", "small6", "small5"])
def test_fp32_model_of_the_kernels_is_inside_the_bars(Hd, family):
    """Another summation order, an fp32 rsqrt moved by -1 / 0 / +1 ulp, fp32 product then bf16: what a correct kernel
    may legitimately compute.  A CPU simulation, not a GPU measurement."""
    g = R.gen(Hd + len(family))
    eps = R.FAMILIES[family][0]
    h = R.bounded((16, Hd), g).to(BF16) * R._amp(family)
    w = R.norm_weight(Hd, g)
    ref = R.rms(h, w, eps)
    zero = dict(share=0.0, steps=0, max_rel=0.0, mean_rel=0.0)
    wn, wr = dict(zero), dict(zero)
    for ulp in (-1, 0, 1):
        rec = R.assert_normed(f"fp32 model H={Hd} {family} ulp {ulp}", R.rms_fp32_model(h, w, eps, ulp), ref, log=False)
        wn = {k: max(wn[k], rec[k]) for k in wn}
    x = R.unit((Hd // 8, 8, 128), g) * R._amp(family)
    hw = R.head_norm_weight(g)
    pos = 39000 + torch.arange(Hd // 8)
    cos, sin = R.tables(R.TABLE_ROWS)
    want = R.rope(R.rms(x, hw, eps), pos, cos, sin, R.TABLE_ROWS)
    for ulp in (-1, 0, 1):
        rec = R.assert_roped(f"fp32 model heads {family} ulp {ulp}", R.rope(R.rms_fp32_model(x, hw, eps, ulp), pos, cos, sin, R.TABLE_ROWS),
                             want, log=False)
        wr = {k: max(wr[k], rec[k]) for k in wr}
    print(f"[model] H={Hd} {family}: normed share {wn['share']:.2e}, {wn['steps']} steps; roped share {wr['share']:.2e}, "
          f"max {wr['max_rel']:.2e} mean {wr['mean_rel']:.2e} of scale")
