"""FP8 (e4m3) draft weights in the ragged batch, the parts that need no GPU ("The batch forms"):
the three entry points' argument validation on a Weight(wp, scale, W_E4M3) descriptor, and the host form rules behind the
cases of test_hip_fp8_batch.py."""
import ctypes as C

import fp8_batch_cases as FC

NAMES = ("dfl_gemm_f32_batch", "dfl_gemm_silu_mul_batch", "dfl_gemm_argmax_batch")
P = 4096   # stands for a device pointer (64-byte aligned); nothing is launched


def _source(mode):
    from dflash_amd import _lib
    x = _lib.RowsBatch()
    x.r0.mode, x.r0.valid_word = mode, -1
    if mode == 0:
        x.r0.frag, x.frag_stride = P, 16 * 8192
    else:
        x.r0.rows, x.r0.ld, x.rows_stride = P, 8192, 16 * 8192
    return x


def _call(h, name, wp, sc, x, R, N, K):
    from dflash_amd import _lib
    xr = C.byref(x) if x is not None else None
    w = _lib.Weight(wp, sc, _lib.W_E4M3)
    if name == "dfl_gemm_f32_batch":
        return h.dfl_gemm_f32_batch(w, xr, R, N, K, P, None, None)
    if name == "dfl_gemm_silu_mul_batch":
        return h.dfl_gemm_silu_mul_batch(w, xr, R, N, K, P, 16 * N, P, None, None)
    return h.dfl_gemm_argmax_batch(w, xr, R, N, K, 1, 15, None, -1, P, P, 16, 1, None, 0, None)


def test_fp8_batch_entry_points_validate_without_gpu():
    """-22 (DFL_EINVAL) with the entry point's own name in the message, before any launch: K % 64 != 0 (K = 4192 is a
    multiple of 32, which the bf16 siblings take), K = 128, a null scale, a scale that is not 64-byte aligned, R = 5, and
    for the two ring forms a plain-row source — there is no slab form to fall back to."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(name, text, *args):
        assert _call(h, name, *args) == -22, (name, args[3:])
        err = h.dfl_last_error()
        assert (name + ":").encode() in err and text in err, (name, err)

    frag, plain = _source(0), _source(1)
    for name in NAMES:
        refused(name, b"K%64", P, P, frag, 4, 512, 4192)
        refused(name, b"K >= 256", P, P, frag, 4, 512, 128)
        refused(name, b"null", P, None, frag, 4, 512, 512)
        refused(name, b"null", None, P, frag, 4, 512, 512)
        refused(name, b"null", P, P, None, 4, 512, 512)
        refused(name, b"aligned", P, P + 16, frag, 4, 512, 512)
        refused(name, b"R <= 4", P, P, frag, 5, 512, 512)
        refused(name, b"R <= 4", P, P, frag, 0, 512, 512)
        refused(name, b"%16", P, P, frag, 4, 520, 512)
    for name in NAMES[1:]:
        refused(name, b"no slab form", P, P, plain, 4, 512, 512)


def test_fp8_batch_signatures_mirror_their_siblings():
    """One name per launch: the e4m3 form is the same entry point with the format in its weight descriptor."""
    from dflash_amd import _lib
    for name in NAMES:
        assert _lib.SIGNATURES[name][1][0] is C.POINTER(_lib.Weight), name
        assert name + "_fp8" not in _lib.SIGNATURES, name


def test_gpu_cases_reach_every_form():
    """What test_hip_fp8_batch.py's shapes reach under the host rules of gemm_batch.hip."""
    silu = [FC.silu_form(R, I) for R, I, _ in FC.SILU_CASES]
    assert {(f["MT"], f["NW"]) for f in silu} == {(2, 12), (2, 16), (4, 12), (4, 16)}
    assert {f["upp"] for f in silu} == {1, 2, 3, 4}
    assert FC.silu_form(4, 17408)["npass"] == 2 and all(f["npass"] == 1 for f in silu[:-1])
    f = FC.silu_form(4, 14336)
    assert (f["NW"], f["upp"], f["tail"]) == (16, 4, True)                 # 128 workgroups walk 3 units, not 4
    assert FC.silu_form(2, 16384) == dict(MT=2, NW=16, gx=256, upp=4, npass=1, tail=False)
    assert FC.silu_form(1, 64)["gx"] == 4
    for _, _, K in FC.SILU_CASES + FC.ARGMAX_CASES + FC.F32_CASES:
        assert K % 64 == 0 and K >= 256
    assert any((K // 32) % 8 != 0 for _, _, K in FC.SILU_CASES)            # a partial last chunk (K = 320: 8 + 2 k-steps)
    assert any((K // 32) % 8 != 0 for _, _, K in FC.ARGMAX_CASES)
    arg = {V: FC.argmax_form(R, V) for R, V, _ in FC.ARGMAX_CASES}
    assert arg[2048] == dict(MT=2, NW=16, gx=128, upp=1, npass=1)
    assert arg[4208]["upp"] == 2 and 4208 // 16 - 256 == 7                 # 7 workgroups with a second unit
    assert (arg[69632]["npass"], arg[69632]["upp"]) == (2, 9)
    assert (arg[151936]["npass"], arg[151936]["upp"]) == (3, 13)
    f32 = {(N, K): FC.f32_form(R, N, K) for R, N, K in FC.F32_CASES}
    assert f32[64, 512]["ksplit"] == 1 and f32[64, 512]["gx"] == 4
    assert FC.f32_form(4, 512, 2560, w8=False)["nfr"] == 5 and f32[512, 2560]["nfr"] == 6 and f32[512, 2560]["ksplit"] == 2
    assert f32[4112, 1024]["first"] == 2 and f32[4112, 1024]["last"] == 1
    assert f32[256, 12288]["ksplit"] == 6 and f32[64, 32768]["ksplit"] == 16
    # every other case: the bf16 form's share is even already, so both forms give a wave the same k-steps
    assert all(FC.f32_form(R, N, K, w8=False)["nfr"] % 2 == 0 for R, N, K in FC.F32_CASES if K != 2560)
    assert {f["MT"] for f in f32.values()} == {2, 4}
    # the part of the restatement the library answers without a GPU: tiles per launch and K parts
    from dflash_amd import _lib
    h = _lib.lib()
    for R, N, K in FC.F32_CASES + FC.SILU_CASES + FC.ARGMAX_CASES:
        assert h.dfl_batch_tiles(R) == FC.f32_form(R, 16, K)["MT"] and h.dfl_batch_ksplit(K) == FC.f32_form(R, 16, K)["ksplit"]
