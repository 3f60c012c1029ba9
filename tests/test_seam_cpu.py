"""The plain reference of the K-part GEMM / residual-norm seam (tests/seam_ref.py) checked on its own, without a GPU: against
the oracle's RMSNorm, against float64 sums, and — so that the cap the GPU test grants the kernel is known to be earned by
summation order alone — against an fp32 restatement of the kernel's own order.  Also pins which launch forms the shapes
of tests/test_hip_seam.py reach under the mirrored host rules."""
import pytest
import torch

import seam_ref as S
from oracle import dflash_oracle as O

BF16 = torch.bfloat16


def _new_rows(H, seed, nsplit=2, MT=4):
    h, parts, nw = S.norm_case_data(H, MT, nsplit, seed)
    return S.parts_add_ref(h, parts.view(-1, MT, 16, H), nsplit).view(MT * 16, H), nw, h, parts


@pytest.mark.parametrize("H", S.NORM_H)
def test_rms_frag_ref_is_the_oracles_norm(H):
    """Same rounding points as oracle.dflash_oracle.rms_norm; only rstd differs (float64 against torch's fp32 mean)."""
    rows, nw, _, _ = _new_rows(H, 100 + H)
    a, b = S.rms_frag_ref(rows, nw, S.EPS), O.rms_norm(rows, nw, S.EPS)
    d = S.bf16_steps(a, b)
    share = float((d > 0).float().mean())
    print(f"[seam] rms_frag_ref vs oracle rms_norm H={H}: {share:.2e} differ, max {int(d.max())} steps")
    assert b.dtype == BF16 and int(d.max()) <= 2 and share <= S.FLIP_CAP


@pytest.mark.parametrize("H", S.NORM_H)
def test_kernel_summation_order_stays_within_the_cap(H):
    """The kernel's order of adding the squares (8-element chunks per thread, 256 threads, a tree over each row of 16
    lanes, 4 rows, 4 waves) in fp32 against rms_frag_ref on the GPU test's inputs: fewer elements differ than the cap
    allows, none by more than 2 bf16 steps.  (A strictly sequential fp32 sum, far worse than the kernel's order, moves
    2.6e-4 .. 4.9e-4 of the elements at H = 2560 .. 16384.)"""
    rows, nw, _, _ = _new_rows(H, 100 + H)
    ref = S.rms_frag_ref(rows, nw, S.EPS)
    got = S.rms_frag_with_rstd(rows, nw, S.kernel_order_rstd(rows, S.EPS))
    d = S.bf16_steps(got, ref)
    share = float((d > 0).float().mean())
    print(f"[seam] kernel-order fp32 rstd vs float64 rstd H={H}: {share:.2e} differ, max {int(d.max())} steps")
    assert int(d.max()) <= 2 and share < S.FLIP_CAP
    if H == 8:
        assert share == 0


@pytest.mark.parametrize("nsplit", [1, 2, 6, 8])
def test_parts_add_ref_against_a_float64_sum(nsplit):
    """The fp32 sum in part order against the same roundings over a float64 sum.
    Same-sign data (|h|, |parts|: nothing cancels): the fp32 sum is within nsplit * 2^-24 of the float64 one, far inside a
    bf16 step of it, and the result is larger than the sum, so its step is no smaller: at most ONE bf16 step apart, rarely.
    The GPU test's cancelling data: a one-step flip of the rounded sum is a step of the SUM, which may be many steps of a
    result that h has cancelled, and where the parts cancel each other the fp32 error is not small against the sum; what
    holds for any data is |got - want| <= 2^-7 (|bf16 sum| + |want|) + nsplit 2^-23 sum |parts| (a step of x is at most
    2^-7 |x|), and few elements differ at all."""
    MT, H = 4, 2560
    h, parts, _ = S.norm_case_data(H, MT, nsplit, 7 + nsplit)
    p = parts.view(-1, MT, 16, H)

    def both(hh, pp):
        acc64 = pp[:nsplit].double().sum(0)
        return S.parts_add_ref(hh, pp, nsplit), (hh.double() + acc64.to(BF16).double()).to(BF16), acc64

    got, want, _ = both(h.abs(), p.abs())
    d = S.bf16_steps(got, want)
    print(f"[seam] parts_add_ref vs float64 sum, same sign, nsplit={nsplit}: {float((d > 0).float().mean()):.2e} differ, "
          f"max {int(d.max())} steps")
    assert int(d.max()) <= 1
    got, want, acc64 = both(h, p)
    diff = (got.double() - want.double()).abs()
    bound = 2.0 ** -7 * (acc64.to(BF16).double().abs() + want.double().abs()) + nsplit * 2.0 ** -23 * p[:nsplit].double().abs().sum(0)
    share = float((diff > 0).float().mean())
    print(f"[seam] parts_add_ref vs float64 sum, cancelling, nsplit={nsplit}: {share:.2e} differ")
    assert bool((diff <= bound).all()) and share <= 1e-3
    if nsplit >= 2:   # the data separates the two rounding orders: rounding once differs from rounding the sum first
        once = (h.double() + acc64).to(BF16)
        assert float((once != got).float().mean()) > 0.02
        # ... and a dropped last part cannot hide behind cancellation
        assert float((S.parts_add_ref(h, p, nsplit - 1) != got).float().mean()) > 0.5


def test_frag16_round_trip():
    x = torch.arange(16 * 24, dtype=torch.float32).view(16, 24).to(BF16)
    f = S.frag16_pack(x)
    assert torch.equal(S.frag16_unpack(f, 24), x)
    assert float(f[(2 * 16 + 5) * 8 + 3]) == float(x[5, 2 * 8 + 3])     # element (m, k) at ((k/8)*16 + m)*8 + k%8


def test_host_rules_cover_the_launch_forms():
    """The shapes of tests/test_hip_seam.py reach what they are there for (a host-rule change must not silently move them)."""
    cases = S.GEMM_SMALL + S.GEMM_MODEL
    per_wg = [S.tiles_per_wg(N, K) for N, K in cases]
    assert set(range(1, 9)) <= {t for ts in per_wg for t in ts}
    assert S.tiles_per_wg(16 * 1546, 64) == [6, 7] and S.grid_x_for(1546, 1) == 221   # 220 x 7 + 1 x 6
    assert all(S.tiles_per_wg(4096 * n, 32) == [n] for n in range(1, 9))
    assert S.tiles_per_wg(4096, 12288) == [6, 7] and S.tiles_per_wg(5120, 17408) == [11, 12]
    assert {S.batch_ksplit(K) for _, K in cases} >= {1, 2, 3, 5, 6, 9, 16}
    assert S.batch_ksplit(32768) == 16 and S.batch_ksplit(S.GEMM_K_REJECTED) == 17
    assert S.batch_ksplit(2080) == 2 and S.part_ksteps(2080) * 32 == 1280          # parts of 1280 + 800 columns, not 2048 + 32
    assert S.part_ksteps(32) == 8 and S.part_ksteps(4096) * 32 == 2048
    assert [S.batch_ksplit(K) for _, K in S.CHAIN_CASES] == [2, 5, 6]
    # the norm launch: its three instantiations at their boundaries, one chunk in all, one chunk per thread, a partial second
    assert [S.norm_maxc(H) for H in S.NORM_H] == [2, 2, 2, 2, 4, 4, 4, 8, 8]
    assert 8 // 8 == 1 and 2048 // 8 == 256 and 256 < 2560 // 8 < 512 and 16384 // 8 == 8 * 256
    assert [S.batch_tiles(R) for R in (1, 2, 3, 4)] == [2, 2, 4, 4]


def test_norm_cases_cover_the_issue():
    """H, R, part counts both ways, valid-row counts, dyn = NULL, the pure copy and both tap slots are all there."""
    assert {c[0] for c in S.NORM_CASES} == set(S.NORM_H) and {c[1] for c in S.NORM_CASES} == {1, 2, 3, 4}
    for via in ("K", "shares"):
        assert {c[2] for c in S.NORM_CASES if c[3] == via} == {1, 2, 6, 8}
    assert {v for c in S.NORM_CASES if c[4] for v in c[4]} == {16, 9, 1, 0}
    assert any(c[4] is None for c in S.NORM_CASES) and any(c[2] == 0 and c[5] is not None for c in S.NORM_CASES)
    assert {c[5] for c in S.NORM_CASES} == {0, 2, None}


def test_stack_ref_taps_and_repeats():
    """stack_ref on a tiny stack: a repeated tap id gives equal copies, the taps are the layer outputs, and a dense
    layer's contribution follows the documented roundings."""
    g = torch.Generator().manual_seed(3)
    H, QD, I = 16, 24, 32
    r = lambda *s, sc=0.2: (torch.randn(*s, generator=g, dtype=torch.float64) * sc).to(BF16)  # noqa: E731
    L = [dict(ln1=1 + r(H), ln2=1 + r(H), qkv=r(QD + 8, H), o=r(H, QD), gate=r(I, H), up=r(I, H), down=r(H, I)),
         dict(ln1=1 + r(H), ln2=1 + r(H), qkv=r(QD + 8, H), o=r(H, QD), experts=[r(H, H), r(H, H), r(H, H)]),
         dict(ln1=1 + r(H), ln2=1 + r(H), qkv=r(QD + 8, H), o=r(H, QD), gate=r(I, H), up=r(I, H), down=r(H, I))]
    h0 = r(5, H, sc=1.0)
    h, taps, xn = S.stack_ref(h0, L, 1 + r(H), 1e-6, QD, tap_layers=(0, 0, 1))
    assert torch.equal(taps[:, :H], taps[:, H:2 * H]) and not torch.equal(taps[:, :H], taps[:, 2 * H:])
    h1, _, _ = S.stack_ref(h0, L[:1], 1 + r(H), 1e-6, QD)
    assert torch.equal(h1, taps[:, :H])                      # layer 0's output is what the one-layer stack ends with
    assert h.dtype == BF16 and xn.dtype == BF16 and taps.shape == (5, 3 * H)
