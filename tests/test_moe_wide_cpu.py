"""tests/moe_wide_ref.py without a GPU: the launch forms the case table of test_hip_moe_wide.py is there to reach, and the
fp64 reference of the experts' gate/up stage against a plain torch evaluation."""
import torch

import moe_wide_ref as W
import prefill_plan_ref as P
from test_hip_skinny_gemm import _bf16_ulps

BF16, F64 = torch.bfloat16, torch.float64


def test_cases_reach_their_forms():
    """nfr 1, 5, 7 and 8, empty and partial waves, one to three trips per workgroup, n_active 0 and E, every row source."""
    W.assert_cases_reach_their_forms()


def test_launch_form_arithmetic():
    """launch_form against a brute-force statement of the kernel's sharing-out: k-step ks belongs to wave ks // nfr, pair
    p to workgroup p % 256; every K this launch takes (multiples of 32 up to 4096) is covered exactly once."""
    for K in range(32, W.MAX_K + 1, 32):
        c = W.Case(3, 32, K, 2, 16, "frag")
        f = W.launch_form(c)
        owner = [ks // f["nfr"] for ks in range(f["KS"])]
        assert max(owner) < W.WAVES and f["nfr"] <= W.FR
        assert f["waves"] == [owner.count(w) for w in range(W.WAVES)]
        assert all(W.wave_of_kstep(c, ks) == owner[ks] for ks in (0, f["KS"] - 1))
    assert W.launch_form(W.Case(2, 16, 2048, 1, 16, "frag"))["nfr"] == 4       # the pair kernel's last K: 4 k-steps a wave
    assert W.launch_form(W.Case(2, 16, 2080, 1, 16, "frag"))["nfr"] == 5       # ... and the first one beyond it
    for n_active, I in ((0, 48), (1, 16), (5, 48), (20, 256), (33, 256), (64, 1536)):
        f = W.launch_form(W.Case(64, I, 4096, n_active, 16, "frag"))
        pairs = list(range(n_active * (I // 16)))
        assert f["trips"] == [len(pairs[b::W.GRID]) for b in range(W.GRID)]


def test_gate_up_reference_against_plain_torch():
    """gate_up_ref (fp64, the four bf16 rounding points) against torch's own bf16 pipeline — fp32 matmuls of the integer
    operands (exact), torch.nn.functional.silu on the bf16 gate — on two experts of 256 columns, K = 96, integer and
    2^-6-scaled gate weights.  The sums are exact in both, so the two differ only where torch's fp32 silu and the fp64
    one round to different bf16 values: within one bf16 step, on at most 1e-3 of the elements.  Gate sums below -88.72
    (forced in one column) are -0 in both: fp32's exp overflows there."""
    g = torch.Generator().manual_seed(3)
    E, I, K = 2, 256, 96
    x = torch.randint(-2, 3, (16, K), generator=g).float()
    up = torch.randint(-2, 3, (E, I, K), generator=g).float()
    gate = torch.randint(-2, 3, (E, I, K), generator=g).float()
    gate[0, 7] = -2 * torch.sign(x[3]) - (x[3] == 0).float()       # row 3, column 7 of expert 0: a gate sum of about -150
    assert float(x[3] @ gate[0, 7]) < -89
    for scale in (1.0, 2.0 ** -6):
        gs = gate * scale
        ref = W.gate_up_ref(x, gs, up, range(E))
        for e in range(E):
            gb, ub = (x @ gs[e].T).to(BF16), (x @ up[e].T).to(BF16)
            plain = torch.nn.functional.silu(gb) * ub
            assert plain.dtype == BF16
            got = ref[e].to(BF16)
            assert torch.equal(got.to(F64), ref[e])                 # the reference holds bf16 values
            d = _bf16_ulps(got, plain)
            assert int(d.max()) <= 1 and float((d > 0).float().mean()) <= 1e-3, (scale, e, int(d.max()))
        if scale == 1.0:
            assert float(ref[0][3, 7]) == 0.0
    # the shared piece: moe_rows_ref still rounds where expert_act_ref does
    pe = torch.tensor([[0, 1]] * 16)
    pw = torch.full((16, 2), 0.5)
    down = torch.randint(-1, 2, (E, K, I), generator=g).to(F64)
    out, _ = P.moe_rows_ref(x.to(F64), gate.to(F64), up.to(F64), down, pe, pw)
    for e in range(E):
        act = P.expert_act_ref(x.to(F64), gate[e].to(F64), up[e].to(F64))
        assert torch.equal(out[:, e], 0.5 * (act @ down[e].T))

