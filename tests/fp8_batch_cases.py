"""Shapes of the fp8 ragged-batch kernel tests and the host rules that pick each launch form (gemm_batch.hip: ring_plan,
the w16 rule, batch_ksplit / nfr / grid_x_for), restated so that test_fp8_batch_cpu.py can assert — without a GPU — that
the cases test_hip_fp8_batch.py runs reach every form."""


def ring_plan(nunits, upp_max):
    """workgroups, units per workgroup and pass, passes"""
    gx = min(nunits, 256)
    per_wg = -(-nunits // gx)
    npass = -(-per_wg // upp_max)
    return gx, -(-per_wg // npass), npass


def silu_form(R, I):
    per_wg = (I // 16 + 255) // 256
    w16 = per_wg % 4 == 0 or per_wg > 6
    gx, upp, npass = ring_plan(I // 16, 4 if w16 else 3)
    return dict(MT=2 if R <= 2 else 4, NW=16 if w16 else 12, gx=gx, upp=upp, npass=npass, tail=(I // 16) % gx != 0)


def argmax_form(R, V):
    gx, upp, npass = ring_plan(V // 16, 16)
    return dict(MT=2 if R <= 2 else 4, NW=16, gx=gx, upp=upp, npass=npass)


def f32_form(R, N, K, w8=True):
    """K parts, k-steps per wave (W8: rounded up to a pair), workgroups along x, tiles the first / last workgroup walks"""
    KS = K // 32
    ksplit = (KS + 63) // 64
    nfr = -(-KS // (8 * ksplit))
    if w8:
        nfr += nfr & 1
    ntiles = N // 16
    gx_max = max(1, 256 // ksplit)
    per_wg = -(-ntiles // gx_max)
    gx = -(-ntiles // per_wg)
    return dict(MT=2 if R <= 2 else 4, ksplit=ksplit, nfr=nfr, gx=gx, first=(ntiles - 1) // gx + 1, last=(ntiles - 1 - (gx - 1)) // gx + 1)


# (R, I, K), I = 16 x units
SILU_CASES = [(1, 64, 256), (3, 1024, 320), (2, 8192, 256), (4, 12288, 256), (4, 14336, 256), (2, 16384, 256),
              (4, 17408, 256)]
# (R, V, K)
ARGMAX_CASES = [(1, 2048, 256), (4, 4208, 320), (3, 69632, 256), (4, 151936, 512)]
# (R, N, K)
F32_CASES = [(1, 64, 512), (4, 512, 2560), (3, 4112, 1024), (4, 256, 12288), (2, 64, 32768)]


def case_id(c):
    return "R{}-N{}-K{}".format(*c)
