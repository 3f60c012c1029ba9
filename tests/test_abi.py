"""The C-ABI library loads (no GPU needed) and exports exactly what include/*.h declares."""
import ctypes
import os
import re

import helpers as H


def _declared():
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(dfl_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from dflash_amd import _lib
    names = _declared()
    assert len(names) >= 16
    assert sorted(_lib.SIGNATURES) == names, "binding table and header disagree"
    handle = _lib.lib()
    for n in names:
        assert isinstance(getattr(handle, n), ctypes._CFuncPtr)
    assert handle.dfl_version() == 1
    assert handle.dfl_argmax_ws_bytes() > 0 and handle.dfl_attn_ws_bytes(32, 8) > 0


def test_binding_arity_matches_header():
    """Every ctypes signature has as many arguments as the header's prototype (a missing one
    shifts every later argument silently: found the hard way with dfl_accept_commit_batch)."""
    from dflash_amd import _lib
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, (_, args) in _lib.SIGNATURES.items():
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() and p.strip() != "void"]
        assert len(params) == len(args), f"{name}: header has {len(params)} parameters, binding {len(args)}"


def test_batch_entry_points_validate_without_gpu():
    from dflash_amd import _lib
    h = _lib.lib()
    assert h.dfl_batch_tiles(1) == 2 and h.dfl_batch_tiles(2) == 2 and h.dfl_batch_tiles(3) == 4
    assert h.dfl_batch_ksplit(4096) == 2 and h.dfl_batch_ksplit(12288) == 6 and h.dfl_batch_ksplit(512) == 1
    assert h.dfl_gemm_batch_ws_bytes(4096, 4096) > 2 * 256 * 4 * 1024
    assert h.dfl_gemm_f32_batch(None, None, 2, 16, 32, None, None, None) == -22
    assert h.dfl_accept_commit_batch(None, 16, None, 16, 1, None, 1, 1, None, None, None, 0, None, None, 0, 1, None, None,
                                     None) == -22


def test_argument_validation_needs_no_gpu():
    from dflash_amd import _lib
    h = _lib.lib()
    assert h.dfl_pack_weight(None, None, 16, 32, None) == -22
    assert b"null" in h.dfl_last_error()
    assert h.dfl_gemm_f32(1, None, None, 3, 16, 32, 1, 1, None, None) == -22
    assert h.dfl_accept_commit(1, 1, 0, 1, 4, 1, None, 0, None, None, 0, 0, None, None) == -22


def test_no_entry_point_has_a_twin():
    """One entry point per operation: no declared name is another declared name plus _t, _timed or _fp8 — a launch
    takes its weight's format in a dfl_weight.  The two packers are the exception: packing e4m3 codes is a separate
    operation on another element type, and nothing about it is chosen at launch."""
    names = set(_declared())
    packers = {"dfl_pack_weight_fp8", "dfl_pack_weight_gateup_fp8"}
    assert packers <= names
    twins = sorted(n for n in names - packers for suffix in ("_t", "_timed", "_fp8")
                   if n.endswith(suffix) and n[:-len(suffix)] in names)
    assert not twins, twins


def test_folded_entry_points_keep_the_conditional_checks():
    """What only the wider form of a folded entry point required is still required, for that form alone: each call is
    refused with -22 and the entry point's own name in the text.  Small integers stand for pointers: nothing launches."""
    import ctypes as C
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(name, *args):
        assert getattr(h, name)(*args) == -22, name
        assert (name + ":").encode() in h.dfl_last_error(), (name, h.dfl_last_error())

    # dyn_t without the re-arm it belongs to
    refused("dfl_accept_commit", 16, 16, 4, 16, 64, 16, None, 0, None, None, 0, 0, 16, None)
    assert b"dyn_t" in h.dfl_last_error()
    # two tiles per request need both tile records; three tiles do not exist
    batch = (16, 32, 16, 32, 2, 16, 64, 64, 16, 16, None, 0, 16, None, 0)
    refused("dfl_accept_commit_batch", *batch, 2, None, 16, None)
    assert b"tile record" in h.dfl_last_error()
    refused("dfl_accept_commit_batch", *batch, 2, 16, None, None)
    assert b"tile record" in h.dfl_last_error()
    refused("dfl_accept_commit_batch", *batch, 3, 16, 16, None)
    assert b"tiles_per_req=3" in h.dfl_last_error()
    # q_tiles = 3
    refused("dfl_attn_head_batch", 16, 1024, 0, 512, 768, 2, 16384, 4, 2, None, None, 1e-6, 16, 16, 4096, 16, 16, 1024,
            1 << 20, 0.088, 0, 16, 512, 16, 8, 16, 8192, 8192, 3, None)
    assert b"q_tiles" in h.dfl_last_error()
    refused("dfl_attn_head_cand", 16, 1024, 0, 512, 768, 2, 16384, 4, 2, None, None, 1e-6, 16, 16, 4096, 16, 16, 1024,
            0.088, 100, 16, 16, 8, 16, 8192, 8192, 3, 16, 16, 1 << 16, 32, None)
    assert b"q_tiles" in h.dfl_last_error()
    # no per-slot 1/T array: the host value is the temperature, and 0 is none
    x = _lib.RowsBatch()
    x.r0.frag, x.r0.mode, x.frag_stride = 16, 0, 4096 * 16
    refused("dfl_gemm_sample_batch", _lib.Weight(16, None, _lib.W_BF16), C.byref(x), 2, 64, 256, 0, 16, 16, 2, 16, 16, 16, 0, None, 0, 16, None, 0.0, 0, 3,
            1, 1, None)
    assert b"inv_t" in h.dfl_last_error()
    refused("dfl_sample_rows_nucleus", 16, 64, 1024, 1, 64, 0, 16, None, -1, -1, 0, None, 0, 1, None, 1, None, 0, None,
            1.0, None, 0.0, 0, 0, 16, 16, 0, None, None, None)
    assert b"inv_t" in h.dfl_last_error()
    # tiles that share a cache: at least one
    refused("dfl_kv_append_batch", 16, 1, 4096, 256, 0, 128, 256, 1, 2, 16, 2, None, 128, 1e-6, 16, 16, 4096, 16, 16,
            1024, 1 << 20, 1 << 18, 16, 0, None)
    assert b"batch shape" in h.dfl_last_error()
    # the weight descriptor, on a single-request and a batch entry point: a format that is neither of the two, e4m3
    # codes without their scales, a bf16 weight with a scale vector, no descriptor at all
    rows = _lib.Rows()
    rows.frag, rows.mode, rows.valid_word = 16, 0, -1
    for name, rest in (("dfl_gemm_resid", (C.byref(rows), 16, 64, 16, 16, 0, None, 0, None, None, None)),
                       ("dfl_gemm_f32_batch", (C.byref(x), 2, 64, 256, 16, None, None))):
        refused(name, _lib.Weight(4096, 4096, 2), *rest)
        assert b"format 2" in h.dfl_last_error()
        refused(name, _lib.Weight(4096, None, _lib.W_E4M3), *rest)
        assert b"null" in h.dfl_last_error()
        refused(name, _lib.Weight(4096, 4096, _lib.W_BF16), *rest)
        assert b"no scale" in h.dfl_last_error()
        refused(name, None, *rest)
        assert b"descriptor" in h.dfl_last_error()


def test_product_has_no_cpu_path():
    import pytest
    import torch
    from dflash_amd import sample
    with pytest.raises(RuntimeError):
        sample(torch.zeros(1, 2, 8), 0.0)


def test_product_never_imports_the_oracle():
    pkg = os.path.join(H.ROOT, "dflash_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("the oracle", ""), fn


def test_library_reads_no_environment():
    """The shipped library keeps no process state beyond what include/dflash_hip.h names: no source or header of it
    calls getenv, and target.py picks the MoE launch forms by shape, not by a DFL_MOE_* variable."""
    for d in (os.path.join(H.ROOT, "dflash_amd", "csrc"), os.path.join(H.ROOT, "include")):
        files = sorted(os.listdir(d))
        assert files, d
        for fn in files:
            assert "getenv" not in open(os.path.join(d, fn)).read(), fn
    assert "DFL_MOE_" not in open(os.path.join(H.ROOT, "dflash_amd", "target.py")).read()
