"""min_p without a GPU: the properties of the numpy model of the contract, check_min_p, every
refusal of the entry point through the C ABI, and the Python-level refusals that need no launch."""
import inspect
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import min_p_ref as MR

V = 512


def _rows(seed, rows=6):
    rng = np.random.default_rng(seed)
    bits = MR.case_rows(rng, rows, V)
    bits[:, ::17] = 0x0000
    bits[:, 5::31] = 0x8000
    return bits


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("min_p", [1e-4, 0.01, 0.2, 0.5, 0.9, 1.0])
@pytest.mark.parametrize("T", [0.3, 0.7, 1.0, 2.5])
def test_the_argmax_is_invariant_and_the_rule_is_the_probability_rule(min_p, T):
    x = _rows(1)
    for row in x:
        out, kept = MR.process(row, MR.log_min_p(min_p), MR.inv_t(T))
        assert MR.argmax_lowest(out) == MR.argmax_lowest(row)
        on = out != MR.NEG_INF
        assert kept == on.sum() >= 1 and np.array_equal(out[on], row[on])
        # against p_v >= min_p * p_max in float64, away from the boundary
        z = MR.widen(row).astype(np.float64) / T
        ratio = np.exp(z - z.max())
        sure_in, sure_out = ratio > min_p * 1.05, ratio < min_p * 0.95
        assert on[sure_in].all() and not on[sure_out].any()


def test_min_p_one_keeps_exactly_the_maxima():
    x = _rows(2)
    x[0, [7, 300, 511]] = 0x4270                      # a three-way tie at 60.0
    x[1, 9], x[1, 10] = 0x0000, 0x8000                # +0 and -0 are one value
    x[1, np.arange(V) > 10] = 0xC000
    x[1, :9] = 0xC000
    for row in x:
        out, kept = MR.process(row, MR.log_min_p(1.0), MR.inv_t(0.7))
        v = MR.widen(row)
        assert np.array_equal(out != MR.NEG_INF, v == v.max()) and kept == (v == v.max()).sum()
    assert MR.process(x[0], 0.0, 1.0)[1] == 3 and MR.process(x[1], 0.0, 1.0)[1] == 2
    assert MR.process(x[1], 0.0, 1.0)[0][10] == 0x8000            # the bits are copied: -0 stays -0


def test_off_greedy_and_rows_without_a_finite_maximum_are_copied():
    x = _rows(3)[0]
    for L in (-np.inf, 0.5, np.nan, np.float32(1e-30)):
        out, kept = MR.process(x, L, 1.0)
        assert np.array_equal(out, x) and kept == V
    for invT in (0.0, -1.0, np.nan, -0.0):
        out, kept = MR.process(x, -1.0, invT)
        assert np.array_equal(out, x) and kept == V
    for fill in (0xFF80, 0x7FC1):                     # all -inf; all NaN
        r = np.full(V, fill, dtype=np.uint16)
        out, kept = MR.process(r, -1.0, 1.0)
        assert np.array_equal(out, r) and kept == V
    r = x.copy()
    r[5] = 0x7F80                                     # a +inf: the maximum is not finite
    out, kept = MR.process(r, -1.0, 1.0)
    assert np.array_equal(out, r) and kept == V
    assert MR.log_min_p(0) == -np.inf and MR.log_min_p(None) == -np.inf and MR.log_min_p(1) == 0.0


def test_nan_keeps_its_bits_and_minus_inf_stays():
    x = _rows(4)[0]
    x[[3, 40, 41]] = [0x7FC1, 0xFFFF, 0xFF80]
    out, kept = MR.process(x, MR.log_min_p(0.5), MR.inv_t(1.0))
    assert out[3] == 0x7FC1 and out[40] == 0xFFFF and out[41] == 0xFF80
    v = MR.widen(x)
    m = np.nanmax(v)
    assert kept == ((v == m) | ((v - m) >= np.float32(math.log(0.5)))).sum() and kept < V - 3
    assert MR.argmax_lowest(out) == MR.argmax_lowest(x)


def test_the_exact_boundary():
    """invT = 0.5, L = -2: a column at m - 4 gives d = -2 and is kept, one at m - 4.03125 is dropped."""
    x = np.full(8, 0xC2C8, dtype=np.uint16)          # -100
    x[0] = MR.to_bits(np.float32(8.0))
    x[1] = MR.to_bits(np.float32(4.0))
    x[2] = MR.to_bits(np.float32(3.96875))
    assert MR.widen(x[2:3])[0] == np.float32(3.96875)
    out, kept = MR.process(x, -2.0, 0.5)
    assert out[1] == x[1] and out[2] == MR.NEG_INF and kept == 2


# ------------------------------------------------------------------------------------------------------------ check_min_p
def test_check_min_p():
    from dflash_amd import ops
    c = ops.check_min_p
    assert c(None) is None and c(0) is None and c(0.0) is None and c(-0.0) is None
    assert c(0.3) == 0.3 and c(1) == 1.0 and c(1.0) == 1.0 and c(np.float32(0.25)) == 0.25 and c(1e-30) == 1e-30
    for bad in (True, False, float("nan"), -0.1, 1.0001, float("inf"), "0.3", [0.3], object()):
        with pytest.raises(ValueError, match="min_p"):
            c(bad)
    assert ops.min_p_log(None) == -math.inf and ops.min_p_log(0) == -math.inf and ops.min_p_log(1.0) == 0.0
    for v in (0.01, 0.2, 0.5, 0.9):
        assert ops.min_p_log(v) == float(MR.log_min_p(v)) == float(np.float32(math.log(v)))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def _call(h, logits=16, out=32, ld=64, tstride=1024, tiles=1, V=64, row0=0, nrows=16, dyn=None, nword=-1, tpr=1,
          lmp_dev=None, lmp=-1.0, inv_t_dev=None, inv_t=1.0, kept=None, kept_stride=0, kept_off=0):
    return h.dfl_min_p_rows(logits, out, ld, tstride, tiles, V, row0, nrows, dyn, nword, tpr, lmp_dev, lmp, inv_t_dev, inv_t,
                            kept, kept_stride, kept_off, None)


def test_entry_point_refuses_by_name():
    """Small integers stand for pointers: nothing launches."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(word, **kw):
        assert _call(h, **kw) == -22, kw
        err = h.dfl_last_error()
        assert b"dfl_min_p_rows:" in err and word in err, (kw, err)

    assert _call(h, tiles=0) == 0 and _call(h, nrows=0) == 0                      # nothing to do
    assert _call(h, nword=2, dyn=16, row0=16, nrows=0) == 0                       # a record-driven count and no row left: no empty grid
    for name in ("logits", "out"):
        refused(b"null", **{name: None})
    for v in (0, -8, 4, 60, 155656):
        refused(b"V=", V=v, ld=max(v, 64))
    for tpr in (0, 3):
        refused(b"tiles_per_req", tpr=tpr)
    refused(b"ld=32", ld=32)
    refused(b"bad shape", logits=18)                                               # a row off 16 bytes
    refused(b"bad shape", out=40)
    refused(b"tile_stride=512", tiles=2, tstride=512)
    refused(b"rows [4,17)", row0=4, nrows=13)
    refused(b"nrows_dyn_word=2", nword=2)                                          # a record word without dyn
    refused(b"nrows_dyn_word=8", nword=8, dyn=16)
    for bad in (0.5, 1e-30, float("inf"), float("nan")):
        refused(b"log_min_p", lmp=bad)
    for bad in (0.0, -1.0, 2e5, float("nan"), float("inf")):
        refused(b"inv_t", inv_t=bad)
    refused(b"negative", kept_off=-1)
    refused(b"negative", kept_stride=-1)
    # -inf is "off" and allowed; a device array: the host value beside it is unused
    assert _call(h, lmp=float("-inf"), tiles=0) == 0 and _call(h, lmp=0.0, tiles=0) == 0
    assert _call(h, lmp_dev=16, lmp=3.0, tiles=0) == 0 and _call(h, inv_t_dev=16, inv_t=0.0, tiles=0) == 0


def test_header_binding_and_sources_agree():
    from dflash_amd import _lib, build
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    assert "log_min_p" in txt and "dfl_min_p_rows" in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bdfl_min_p_rows\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m
    assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SIGNATURES["dfl_min_p_rows"][1]) == 19
    assert hasattr(_lib.lib(), "dfl_min_p_rows")
    assert "min_p.hip" in build.SOURCES
    src = open(os.path.join(H.ROOT, "dflash_amd", "csrc", "min_p.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomic" not in src.split("#include")[1]


# ------------------------------------------------------------------------------------------------------------ keywords
def test_refusals_that_need_no_launch():
    import torch
    from dflash_amd import DFlashDraftModel
    from dflash_amd.batch import BatchedDecoder, dflash_generate_batch
    from dflash_amd.engine import BatchEngine, dflash_generate_stream
    from dflash_amd.generate import DecodeSession, dflash_generate, dflash_generate_policy, run_decode
    from dflash_amd.target import NativeTarget
    model = SimpleNamespace(device=torch.device("cpu"))
    ids = torch.zeros(1, 8, dtype=torch.long)
    kw = dict(mask_token_id=5, max_new_tokens=8, stop_token_ids=[3])
    hf = SimpleNamespace(config=SimpleNamespace(vocab_size=64))             # a wrapped model: no NativeTarget
    native = object.__new__(NativeTarget)       # (the checks come before the target is touched)
    native.V = 64
    # a target that is no NativeTarget at T > 0: ValueError, through every single-request entry
    for tgt in (hf, object()):
        with pytest.raises(ValueError, match="NativeTarget"):
            DecodeSession(model, tgt, ids, max_block_size=16, temperature=0.7, sampler="device", seed=1, min_p=0.3, **kw)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(model, hf, ids, 5, 8, 16, [3], 0.7, sampler="device", seed=1, min_p=0.3)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate_policy(model=model, target=hf, input_ids=ids, temperature=0.7, fixed_block_size=8,
                               sampler="device", seed=1, min_p=0.3, **kw)
    with pytest.raises(ValueError, match="NativeTarget"):
        run_decode(model, hf, ids, block_size=8, temperature=0.7, clamp_tail=True, sampler="device", seed=1, min_p=0.3, **kw)
    # the torch sampler at T > 0
    with pytest.raises(ValueError, match="sampler='device'"):
        DecodeSession(model, native, ids, max_block_size=16, temperature=0.7, min_p=0.3, **kw)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchedDecoder(None, native, 1, 64, 64, 5, temperature=0.7, min_p=True)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchEngine(None, native, max_rows=64, out_len=64, mask_token_id=5, temperature=0.7, min_p=True)
    with pytest.raises(ValueError, match="sampler='device'"):
        dflash_generate_batch(None, native, [ids], 5, 8, 16, [3], 0.7, min_p=0.3)
    with pytest.raises(ValueError, match="sampler='device'"):
        dflash_generate_stream(None, native, [ids, ids], 5, 8, 16, [3], 0.7, min_p=[0.0, 0.3])
    # bad values, before anything else
    for bad in (True, float("nan"), 1.5, -0.2, "x"):
        with pytest.raises(ValueError, match="min_p"):
            DecodeSession(model, hf, ids, max_block_size=16, temperature=0.0, min_p=bad, **kw)
        with pytest.raises(ValueError, match="min_p"):
            dflash_generate_batch(None, native, [ids], 5, 8, 16, [3], min_p=bad)
    with pytest.raises(ValueError, match="one value per prompt"):
        dflash_generate_batch(None, native, [ids, ids, ids], 5, 8, 16, [3], min_p=[0.1, 0.2])
    with pytest.raises(ValueError, match="one value per prompt"):
        dflash_generate_stream(None, native, [ids], 5, 8, 16, [3], min_p=[0.1, 0.2])
    with pytest.raises(ValueError, match="seed"):
        native.verify(torch.zeros(4, dtype=torch.long), 0, None, temperature=0.7, min_p=0.3)
    with pytest.raises(ValueError, match="row stride of V"):                       # the masked rows' buffer has stride V
        native.verify(torch.zeros(4, dtype=torch.long), 0, None, temperature=0.7, seed=1, min_p=0.3,
                      logits_out=torch.zeros(16, 96, dtype=torch.bfloat16)[:, :64])
    # a request on a decoder / an engine built without the flag
    dec = object.__new__(BatchedDecoder)
    dec.model, dec.target, dec.stop_token_ids, dec.sampler = None, native, [3], "device"
    dec.penalties, dec.filtering, dec.logit_bias, dec.min_p = False, False, False, False
    with pytest.raises(ValueError, match="min_p=True"):
        dec._admit_prefill(0, ids, 0.7, 1, min_p=0.3)
    with pytest.raises(ValueError, match="min_p=True"):
        dec.admit(0, ids, 0.7, seed=1, min_p=0.3)
    dec.TPR, dec.R = 1, 1
    with pytest.raises(ValueError, match="min_p=True"):
        dec.admit_fused(0, ids, 0.0, min_p=1.0)                                    # (at T = 0 too: the slot has no L to write)
    eng = object.__new__(BatchEngine)
    eng.dec = dec
    with pytest.raises(ValueError, match="min_p=True"):
        eng.submit(ids, 8, min_p=0.3)
    with pytest.raises(ValueError, match="min_p"):
        eng.submit(ids, 8, min_p=True)
    eng.min_p, eng.request_temperature, dec.sampler = True, True, "torch"          # validated at submit, not at the admission
    with pytest.raises(ValueError, match="sampler='device'"):
        eng.submit(ids, 8, temperature=0.7, min_p=0.3)
    dec.sampler = "device"
    # T = 0, None and 0 are the call without the keyword: nothing above is asked of them
    for mp in (None, 0, 0.0):
        with pytest.raises(RuntimeError, match="GPU"):
            DecodeSession(model, hf, ids, max_block_size=24, temperature=0.7, min_p=mp, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        DecodeSession(model, hf, ids, max_block_size=24, temperature=0.0, min_p=0.3, **kw)
    # the keyword is where the issue puts it
    for fn in (DecodeSession.__init__, run_decode, dflash_generate, dflash_generate_policy, DFlashDraftModel.spec_generate,
               dflash_generate_batch, dflash_generate_stream, BatchedDecoder.admit, BatchedDecoder.admit_fused,
               BatchEngine.submit, NativeTarget.verify, BatchedDecoder.__init__, BatchEngine.__init__):
        assert "min_p" in inspect.signature(fn).parameters, fn


def test_per_prompt_forms():
    from dflash_amd.batch import _prompt_min_p
    assert _prompt_min_p(None, 3, 0.7, "device") == ([None] * 3, False)
    assert _prompt_min_p(0, 2, 0.7, "torch") == ([None] * 2, False)
    assert _prompt_min_p(0.3, 2, 0.7, "device") == ([0.3, 0.3], True)
    assert _prompt_min_p(0.3, 2, 0.0, "torch") == ([0.3, 0.3], False)              # T = 0: nothing to floor
    assert _prompt_min_p([0, 0.3, 0.5, 1.0], 4, [0.7] * 4, "device") == ([None, 0.3, 0.5, 1.0], True)
    assert _prompt_min_p([None, 0.3], 2, [0.7, 0.0], "torch") == ([None, 0.3], False)
    assert _prompt_min_p((0.0, None), 2, 0.7, "device") == ([None, None], False)
