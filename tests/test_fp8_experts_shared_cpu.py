"""The two grouped expert GEMMs that take a weight descriptor — dfl_moe_grouped_gate_up and dfl_moe_grouped_down, what
the shared MoE pass over 2..4 tiles launches ("The experts") — the parts that need no GPU: their
declarations, and every refusal the header lists."""
import ctypes as C
import os
import re

import helpers as H

NAMES = ("dfl_moe_grouped_gate_up", "dfl_moe_grouped_down")


def _header_arity(txt, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_grouped_entry_points_are_declared_bound_and_exported():
    from dflash_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dfl_[a-z0-9_]+)\s*\(", txt))
    handle = _lib.lib()
    for n in NAMES:
        assert n in names and n in _lib.SIGNATURES and isinstance(getattr(handle, n), C._CFuncPtr), n
        assert len(_lib.SIGNATURES[n][1]) == _header_arity(txt, n), n
        assert _lib.SIGNATURES[n][1][0] is C.POINTER(_lib.Weight), n       # the format travels in the descriptor
        assert n + "_fp8" not in names and n + "_fp8" not in _lib.SIGNATURES, n
    assert _header_arity(txt, NAMES[0]) == 13 and _header_arity(txt, NAMES[1]) == 12
    # the bare-pointer twins of the prefill keep their signatures
    assert _header_arity(txt, "dfl_prefill_moe_gemm_silu") == 13 and _header_arity(txt, "dfl_prefill_moe_gemm_down") == 12
    assert handle.dfl_version() == 1
    assert re.search(r"#define\s+DFL_ABI_VERSION\s+1\b", txt)


def test_grouped_entry_points_validate_without_gpu():
    """Small integers stand for pointers; every call is refused with DFL_EINVAL (-22) and a message with the entry point's
    own name before anything launches — in both weight formats where the refusal does not depend on the format."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(name, *args, text=None):
        assert getattr(h, name)(*args) == -22, (name, args)
        err = h.dfl_last_error()
        assert (name + ":").encode() in err, (name, err)
        if text:
            assert text in err, (name, err)

    W = _lib.Weight
    e4, b16 = (lambda wp=64, sc=128: W(wp, sc, _lib.W_E4M3)), (lambda wp=64, sc=None: W(wp, sc, _lib.W_BF16))

    # dfl_moe_grouped_gate_up(w, stride, xg, items, n_items, max_items, I, K, act_g, rows_per_item, src_row, zeros_1k, stream)
    def gu(w, stride=None, xg=64, items=64, n=64, mi=4, I=64, K=128, act=64, rpi=64, src=None, zeros=None):
        return (w, 2 * I * K if stride is None else stride, xg, items, n, mi, I, K, act, rpi, src, zeros, None)

    # dfl_moe_grouped_down(w, stride, act_g, items, n_items, max_items, H, I, row_w, out32, rows_per_item, stream)
    def dn(w, stride=None, act=64, items=64, n=64, mi=4, Hd=128, I=64, row_w=64, out=64, rpi=64):
        return (w, Hd * I if stride is None else stride, act, items, n, mi, Hd, I, row_w, out, rpi, None)

    for name, call in ((NAMES[0], gu), (NAMES[1], dn)):
        # the descriptor errors of dfl_common.h
        refused(name, *call(None), text=b"null weight descriptor")
        refused(name, *call(W(64, 128, 2)), text=b"unknown weight format")
        refused(name, *call(W(64, None, -1)), text=b"unknown weight format")
        refused(name, *call(b16(sc=128)), text=b"no scale")
        refused(name, *call(e4(sc=None)), text=b"null scale")
        refused(name, *call(e4(sc=128 + 4)), text=b"64-byte aligned")
        refused(name, *call(e4(sc=128 + 32)), text=b"64-byte aligned")
        for w in (e4(), b16()):
            refused(name, *call(w, K=96) if call is gu else call(w, I=96), text=b"K%64")          # K % 64
            if call is gu:                                                                        # N % 128 (gate/up: N = 2 I)
                refused(name, *call(w, I=96), text=b"I%64")
            else:
                refused(name, *call(w, Hd=192), text=b"N%128")
            refused(name, *call(w, stride=128 * 64 + 16), text=b"stride")                         # longer than N * K
            refused(name, *call(w, stride=128 * 64 - 16), text=b"stride")
            refused(name, *call(w, stride=128 * 64 // 2), text=b"stride")                         # (bf16 bytes / code bytes mixed up)
            for rpi in (0, 16, 32, 96, 256):
                refused(name, *call(w, rpi=rpi), text=b"rows_per_item")
            refused(name, *call(W(None, w.scale, w.format)), text=b"null")
            refused(name, *call(w, items=None), text=b"null")
            refused(name, *call(w, n=None), text=b"null")
    for w in (e4(), b16()):
        refused(NAMES[0], *gu(w, src=64), text=b"src_row and zeros_1k")
        refused(NAMES[0], *gu(w, zeros=64), text=b"src_row and zeros_1k")
        refused(NAMES[0], *gu(w, act=None))
        refused(NAMES[0], *gu(w, xg=None), text=b"null")
        refused(NAMES[1], *dn(w, out=None), text=b"null")
        refused(NAMES[1], *dn(w, row_w=None), text=b"null")
        refused(NAMES[1], *dn(w, act=None), text=b"null")
    # the twins on a bare pointer still speak under their own names
    assert h.dfl_prefill_moe_gemm_silu(64, 2 * 64 * 128, 64, 64, 64, 4, 64, 128, 64, 48, None, None, None) == -22
    assert b"dfl_prefill_moe_gemm_silu:" in h.dfl_last_error()
    assert h.dfl_prefill_moe_gemm_down(64, 128 * 64 + 8, 64, 64, 64, 4, 128, 64, 64, 64, 64, None) == -22
    assert b"dfl_prefill_moe_gemm_down:" in h.dfl_last_error()
