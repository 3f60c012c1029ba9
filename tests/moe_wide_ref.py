"""The experts' gate/up launch of a sparse-MoE target wider than 2048 (dfl_gemm_silu_mul_experts, the EPI_SILU_E form of
the skinny-GEMM body in csrc/gemm_skinny.hip): the case table of tests/test_hip_moe_wide.py, the launch form each case
reaches, restated from the host rule and the kernel's index arithmetic, and the fp64 reference.  torch only; nothing here
imports dflash_amd or needs a GPU.

The launch: K / 32 k-steps of a tile are shared out over 16 waves, nfr = ceil(KS / 16) each (wave w owns k-steps
w nfr .. w nfr + nfr - 1, clipped at KS: late waves hold fewer or none).  The (active expert, gate/up pair) items —
n_active x I / 16 of them, in the order of the active-expert list — are dealt to 256 workgroups round-robin: workgroup b
walks pairs b, b + 256, ... ("trips"), double-buffered in LDS, so a third trip reuses both buffers."""
from __future__ import annotations

from typing import NamedTuple

import torch

import prefill_plan_ref as P

F64 = torch.float64
GRID = 256                # dfl_gemm_silu_mul_experts: one workgroup per CU
WAVES, FR = 16, 8         # waves per workgroup, k-steps a wave holds at most (gemm_fr(MT = 1, not chunked))
MAX_K = WAVES * FR * 32   # 4096: one K pass
STEP_BAR, OFF_BAR = 2, 1e-3    # test_gemm_silu_mul_exact's bar for the same finish() epilogue on the same kind of data


class Case(NamedTuple):
    E: int
    I: int
    K: int
    n_active: int
    nv: int           # valid rows (the dyn word); a frag16 source has all 16
    source: str       # "frag" | "rows" | "normed" (test_hip_skinny_gemm._source; normed: one partial sum of squares)

    @property
    def id(self) -> str:
        return f"E{self.E}-I{self.I}-K{self.K}-act{self.n_active}-rows{self.nv}-{self.source}"


CASES = [
    Case(4, 16, 96, 1, 16, "frag"),          # nfr 1; waves 3..15 hold nothing; one pair on one workgroup
    Case(8, 48, 2080, 5, 11, "rows"),        # nfr 5; 13 full waves, three empty; first K the pair kernel refuses
    Case(8, 48, 2080, 5, 16, "frag"),
    Case(8, 64, 3104, 8, 16, "frag"),        # nfr 7; wave 13 holds 6 k-steps, waves 14 and 15 none; n_active == E
    Case(32, 256, 4096, 20, 16, "frag"),     # nfr 8; 320 pairs: workgroups 0..63 walk two pairs, the rest one
    Case(40, 256, 4096, 33, 11, "normed"),   # mode 2, nss 1; 528 pairs: workgroups 0..15 take a third trip
    Case(8, 48, 2080, 0, 16, "frag"),        # n_active = 0: nothing may be written
]


def launch_form(c: Case) -> dict:
    """KS, nfr, the k-steps of waves 0..15 and the pairs ("trips") of workgroups 0..255 — dfl_gemm_silu_mul_experts'
    host rule (nfr = ceil(KS / 16), grid 256) and gemm_body's ks0_of / nf_of / nseq."""
    assert c.K % 32 == 0 and c.I % 16 == 0 and 0 < c.K <= MAX_K and 0 <= c.n_active <= c.E
    KS = c.K // 32
    nfr = -(-KS // WAVES)
    assert 1 <= nfr <= FR
    waves = [max(0, min(nfr, KS - w * nfr)) for w in range(WAVES)]
    assert sum(waves) == KS
    npp = c.I // 16
    npairs = c.n_active * npp
    trips = [0 if b >= npairs else (npairs - 1 - b) // GRID + 1 for b in range(GRID)]
    assert sum(trips) == npairs
    return dict(KS=KS, nfr=nfr, waves=waves, npp=npp, npairs=npairs, trips=trips)


def assert_cases_reach_their_forms() -> None:
    """Every form the case table is there for, computed from the shapes: nfr 1, 5, 7 and 8; empty and partial waves;
    one, two and three trips per workgroup; n_active 0 and E; all three row sources; the first K the pair kernel
    refuses and the last one this launch takes."""
    f = {c: launch_form(c) for c in CASES}
    assert len(set(CASES)) == len(CASES) == 7
    assert {v["nfr"] for v in f.values()} == {1, 5, 7, 8}
    tiny, rows65, frag65, ragged, two, three, none = CASES
    assert f[tiny]["KS"] == 3 and f[tiny]["waves"] == [1, 1, 1] + [0] * 13                 # waves 3..15 hold nothing
    assert f[tiny]["trips"] == [1] + [0] * 255                                            # one pair on one workgroup
    for c in (rows65, frag65, none):
        assert c.K == 2048 + 32 and f[c]["KS"] == 65 and f[c]["waves"] == [5] * 13 + [0] * 3   # 13 full waves, three empty
    assert (rows65.source, rows65.nv, frag65.source, frag65.nv) == ("rows", 11, "frag", 16)
    assert f[rows65]["npairs"] == 15 and f[rows65]["trips"] == [1] * 15 + [0] * 241
    assert f[ragged]["KS"] == 97 and f[ragged]["waves"] == [7] * 13 + [6, 0, 0]           # a partial wave, then empty ones
    assert ragged.n_active == ragged.E and f[ragged]["npairs"] == 32
    assert two.K == three.K == MAX_K and f[two]["waves"] == f[three]["waves"] == [8] * 16
    assert f[two]["npairs"] == 320 and f[two]["trips"] == [2] * 64 + [1] * 192
    assert f[three]["npairs"] == 528 and f[three]["trips"] == [3] * 16 + [2] * 240         # both LDS buffers reused
    assert (three.source, three.nv) == ("normed", 11)
    assert none.n_active == 0 and f[none]["npairs"] == 0 and set(f[none]["trips"]) == {0}
    assert {c.source for c in CASES} == {"frag", "rows", "normed"}
    for c in CASES:
        a = active_experts(c)
        assert len(a) == c.n_active and a == sorted(set(a)) and all(0 <= e < c.E for e in a)
        if 0 < c.n_active < c.E:
            assert a != list(range(c.n_active)), c.id      # not a prefix: a launch that ignored the list would show
        assert 2 * c.E * c.I * c.K * 2 <= 168 * 2 ** 20    # the largest packed weight: 168 MB


def wave_of_kstep(c: Case, ks: int) -> int:
    return ks // launch_form(c)["nfr"]


def active_experts(c: Case) -> list:
    """The case's active experts, ascending as dfl_moe_route lists them: a seeded draw of n_active out of E (never the
    prefix 0 .. n_active - 1 unless that is all of them: the last expert then takes the place of the draw's last)."""
    g = torch.Generator().manual_seed(1000 * c.E + c.n_active)
    a = sorted(torch.randperm(c.E, generator=g)[:c.n_active].tolist())
    if 0 < c.n_active < c.E and a == list(range(c.n_active)):
        a[-1] = c.E - 1
    return a


def gate_up_ref(xs: torch.Tensor, gate: torch.Tensor, up: torch.Tensor, experts) -> dict:
    """{e: [16, I] fp64 holding bf16 values} for the listed experts: exact K-sums (fp64 on integer operands), rounded to
    bf16 where the two Linears round; silu in fp64, rounded; the product, rounded (prefill_plan_ref.expert_act_ref, the
    rounding points of moe_rows_ref).  xs [16, K]: the rows the GEMM must see (rows past the valid count zero); gate / up
    [E, I, K]; any float dtype holding bf16 values."""
    x = xs.to(F64)
    return {int(e): P.expert_act_ref(x, gate[e].to(F64), up[e].to(F64), fp32_range=True) for e in experts}
