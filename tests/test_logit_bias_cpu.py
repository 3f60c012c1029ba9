"""Logit bias, allow / ban lists and min_tokens without a GPU: the numpy model of the contract
against transformers' processors, check_logit_bias, every refusal of the entry point through the C ABI, and the
Python-level refusals that need no launch."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import logit_bias_ref as LR

V = 512


def _rows(seed, rows=6):
    """bf16-valued fp32 rows with zeros of both signs planted."""
    rng = np.random.default_rng(seed)
    bits = LR.f32_to_bf16_bits((rng.standard_normal((rows, V)) * 3).astype(np.float32)).reshape(rows, V)
    bits[:, ::17] = 0x0000
    bits[:, 5::31] = 0x8000
    return bits


def _same(a, b):
    """Equal as fp32 values (-0 == +0, -inf == -inf), no NaN on either side."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return not np.isnan(a).any() and not np.isnan(b).any() and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------------------ the model
def test_bias_is_the_hf_sequence_bias_with_single_tokens():
    import torch
    from transformers import SequenceBiasLogitsProcessor
    from dflash_amd import ops
    bits = _rows(1)
    bias = {3: 1.5, 17: -2.25, 34: 0.1, 100: -7.3, 5: 2.0 ** -8, 36: 0.7}      # zero logits (17, 34) and -0 (5, 36) among them
    b, mt = ops.check_logit_bias(V, bias)
    assert mt == 0
    got = SequenceBiasLogitsProcessor(sequence_bias=[[[k], v] for k, v in bias.items()])(
        torch.zeros(6, 3, dtype=torch.long), torch.tensor(LR.bits_to_f32(bits).copy())).numpy()
    assert _same(LR.sum_f32(bits, b.numpy()), got)
    z = LR.process(bits, b.numpy())
    assert np.array_equal(z, np.where(b.numpy() == 0, bits, LR.f32_to_bf16_bits(got).reshape(bits.shape)))


def test_bans_are_the_hf_suppress_tokens():
    import torch
    from transformers import SuppressTokensLogitsProcessor
    from dflash_amd import ops
    bits = _rows(2)
    banned = [0, 17, 5, 200, V - 1]
    b, _ = ops.check_logit_bias(V, None, None, banned)
    got = SuppressTokensLogitsProcessor(banned)(torch.zeros(6, 3, dtype=torch.long),
                                                torch.tensor(LR.bits_to_f32(bits).copy())).numpy()
    assert _same(LR.sum_f32(bits, b.numpy()), got)
    b2, _ = ops.check_logit_bias(V, {k: float("-inf") for k in banned})         # a bias of -inf is a ban
    assert np.array_equal(b2.numpy(), b.numpy())


def test_allow_list_is_the_hf_prefix_constraint_with_a_constant_function():
    import torch
    from transformers import PrefixConstrainedLogitsProcessor
    from dflash_amd import ops
    bits = _rows(3)
    allowed = [1, 17, 5, 18, 300, V - 1]
    b, _ = ops.check_logit_bias(V, None, allowed)
    got = PrefixConstrainedLogitsProcessor(lambda batch, sent: allowed, 1)(
        torch.zeros(6, 3, dtype=torch.long), torch.tensor(LR.bits_to_f32(bits).copy())).numpy()
    assert _same(LR.sum_f32(bits, b.numpy()), got)
    assert np.isfinite(LR.bits_to_f32(LR.process(bits, b.numpy()))).sum() == 6 * len(allowed)


def test_min_tokens_is_the_hf_min_new_tokens_and_switches_off_where_it_does():
    import torch
    from transformers import MinNewTokensLengthLogitsProcessor
    from dflash_amd import ops
    bits = _rows(4, rows=1)[0]
    n_in, min_tokens, stops = 9, 4, [7, 300, 17]
    lb = ops.check_logit_bias(V, None, None, None, min_tokens, stops)
    b, mt = lb
    assert mt == 4 and not b.numpy().any()
    min_pos = n_in + mt
    proc = MinNewTokensLengthLogitsProcessor(n_in, min_tokens, stops)
    x = LR.bits_to_f32(bits)
    on = []
    for p in range(n_in, n_in + 7):       # predicting index p: p ids are in front of it
        got = proc(torch.zeros(1, p, dtype=torch.long), torch.tensor(x.copy()[None])).numpy()[0]
        z = LR.process(bits, b.numpy(), p, min_pos, stops)
        assert _same(LR.bits_to_f32(z), got), p
        on.append(bool(z[7] == 0xFF80))
    assert on == [True] * 4 + [False] * 3          # off from p = min_pos = n_in + min_tokens on
    # stop ids outside the vocabulary are ignored
    assert np.array_equal(LR.process(bits, b.numpy(), 0, 5, [V, -1, 2 ** 40]), bits)


def test_model_special_values_and_argmax():
    sp = np.array(LR.SPECIALS, dtype=np.uint16)
    n = len(sp)
    assert np.array_equal(LR.process(sp, np.zeros(n, np.float32)), sp)
    assert np.array_equal(LR.process(sp, np.full(n, -0.0, np.float32)), sp)
    assert np.array_equal(LR.process(sp, np.full(n, np.nan, np.float32)), sp)              # device values only
    assert np.array_equal(LR.process(sp, np.full(n, np.inf, np.float32)), sp)
    assert (LR.process(sp, np.full(n, -np.inf, np.float32)) == 0xFF80).all()
    z = LR.process(sp, np.full(n, 1.0, np.float32))
    assert z[:5].tolist() == [0x7F80, 0xFF80, 0x7FC0, 0xFFC1, 0x7FFF] and z[5] == z[6] == 0x3F80
    assert np.array_equal(LR.process(np.arange(1 << 16, dtype=np.uint16), np.zeros(1 << 16, np.float32)),
                          np.arange(1 << 16, dtype=np.uint16))
    assert LR.argmax_lowest(np.array([0x7FC0, 0x3F80, 0x3F80, 0xFFC0], dtype=np.uint16)) == 1
    assert LR.argmax_lowest(np.array([0xFF80, 0xFF80], dtype=np.uint16)) == 0              # a fully banned row
    assert LR.argmax_lowest(np.array([0x7FC0, 0x7FC0], dtype=np.uint16)) == 0
    assert LR.position(3, 5, tiles_per_req=2, pos_base=100, pos_add=1) == 100 + 1 + 16 + 5
    assert LR.position(2, 5, tiles_per_req=2, dyn=[[0] * 8, [0] * 8, [0, 0, 0, 40, 0, 0, 0, 0]], pos_word=3, pos_add=1) == 46


# ------------------------------------------------------------------------------------------------------------ the check
def test_check_logit_bias_neutral_forms():
    from dflash_amd import ops
    c = ops.check_logit_bias
    assert c(V) is None and c(V, None, None, None, 0, None) is None and c(V, {}, None, [], 0, [3]) is None
    assert c(V, {3: 0.0, 7: -0.0, 9: 0}) is None                       # a mapping of zeros
    assert c(V, None, None, None, 5, None) is None and c(V, None, None, None, 5, []) is None   # nothing to suppress
    assert c(V, None, None, None, 0, [3, 4]) is None
    assert c(V, None, list(range(V))) is None                          # an allow list of everything
    b, mt = c(V, {3: 0.0}, None, None, 2, [4])
    assert mt == 2 and not b.numpy().any()
    b, mt = c(V, {3: 0.5}, None, None, 5, None)
    assert mt == 0 and b[3] == 0.5                                     # min_tokens without stop ids: off


def test_check_logit_bias_precedence_and_values():
    import torch
    from dflash_amd import ops
    b, mt = ops.check_logit_bias(V, {1: 2.0, 2: -1.0, 3: 4.0, 4: float("-inf"), "6": 1.25}, [1, 2, 3, 4, 5, 6], [3], 1, [2])
    assert b.dtype == torch.float32 and b.shape == (V,) and not b.is_cuda and mt == 1
    bn = b.numpy()
    assert bn[1] == 2.0 and bn[2] == -1.0 and bn[5] == 0.0 and bn[6] == 1.25
    assert bn[3] == -np.inf and bn[4] == -np.inf                       # a ban beats the bias; a -inf bias is a ban
    assert (bn[7:] == -np.inf).all() and bn[0] == -np.inf              # not allowed
    b, _ = ops.check_logit_bias(V, {9: 3.0}, None, [9])
    assert b[9] == -np.inf and (b.numpy()[:9] == 0).all()
    b, _ = ops.check_logit_bias(V, {np.int64(9): np.float32(0.1)}, torch.tensor([9, 10]), np.array([10]))
    assert b[9] == np.float32(0.1) and b[10] == -np.inf


def test_check_logit_bias_refuses():
    from dflash_amd import ops
    c = ops.check_logit_bias
    for kw in (dict(logit_bias={V: 1.0}), dict(logit_bias={-1: 1.0}), dict(allowed_token_ids=[0, V]),
               dict(banned_token_ids=[-3]), dict(allowed_token_ids=[1.5])):
        with pytest.raises(ValueError, match="outside|token id"):
            c(V, **kw)
    for bad in (float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="bias"):
            c(V, {3: bad})
    with pytest.raises(ValueError, match="empty"):
        c(V, None, [])
    with pytest.raises(ValueError, match="no token finite"):
        c(V, None, [3, 4], [3, 4])
    with pytest.raises(ValueError, match="no token finite"):
        c(V, {3: float("-inf")}, [3])
    with pytest.raises(ValueError, match="no token finite"):
        c(V, None, [3, 4], None, 2, [3, 4, 9])                          # the allowed ids are all stop ids under min_tokens
    assert c(V, None, [3, 4], None, 0, [3, 4, 9]) is not None
    for bad in (-1, 1.5, "3", None):
        with pytest.raises(ValueError, match="min_tokens"):
            c(V, None, None, None, bad, [3])
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.logit_bias_state(1, 2047, "cpu")


def test_state_set_rewrites_the_whole_row():
    import torch
    from dflash_amd import ops
    st = ops.logit_bias_state(3, 64, "cpu")
    assert st.bias.shape == (3, 64) and st.bias.dtype == torch.float32 and st.min_pos.dtype == torch.int32
    assert not st.bias.any() and not st.min_pos.any()
    b, mt = ops.check_logit_bias(64, {3: 1.0}, None, [5], 2, [7])
    ops.logit_bias_set(st, 1, b, 10 + mt)
    assert st.bias[1, 3] == 1.0 and st.bias[1, 5] == -np.inf and st.min_pos.tolist() == [0, 12, 0] and not st.bias[[0, 2]].any()
    ops.logit_bias_set(st, 1, None, 0)
    assert not st.bias.any() and not st.min_pos.any()
    with pytest.raises(ValueError, match="slot"):
        ops.logit_bias_set(st, 3, None)
    with pytest.raises(ValueError, match="shape"):
        ops.logit_bias_set(st, 0, torch.zeros(32))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def _call(h, logits=16, out=32, ld=64, tstride=1024, tiles=1, V=64, row0=0, nrows=16, dyn=None, nword=-1, tpr=1, bias=48,
          bias_stride=64, min_pos_dev=None, min_pos=0, stop_ids=None, n_stop=0, pos_word=-1, pos_base=0, pos_add=0,
          out_ids=None, out_stride=0, out_off=0):
    return h.dfl_logit_bias_rows(logits, out, ld, tstride, tiles, V, row0, nrows, dyn, nword, tpr, bias, bias_stride,
                                 min_pos_dev, min_pos, stop_ids, n_stop, pos_word, pos_base, pos_add, out_ids, out_stride,
                                 out_off, None)


def test_entry_point_refuses_by_name():
    """Small integers stand for pointers: nothing launches."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(word, **kw):
        assert _call(h, **kw) == -22, kw
        err = h.dfl_last_error()
        assert b"dfl_logit_bias_rows:" in err and word in err, (kw, err)

    assert _call(h, tiles=0) == 0 and _call(h, nrows=0) == 0                      # nothing to do
    for name in ("logits", "out", "bias"):
        refused(b"null", **{name: None})
    for v in (0, -8, 4, 60, 155656):
        refused(b"V=", V=v, ld=max(v, 64), bias_stride=max(v, 64))
    for tpr in (0, 3):
        refused(b"tiles_per_req", tpr=tpr)
    refused(b"ld=32", ld=32)
    refused(b"bad shape", logits=18)                                               # a row off 16 bytes
    refused(b"tile_stride=512", tiles=2, tstride=512)
    refused(b"bias_stride=32", bias_stride=32)
    refused(b"bias_stride=66", bias_stride=66)
    refused(b"bias_stride", bias=20)                                               # a table row off 16 bytes
    refused(b"rows [4,17)", row0=4, nrows=13)
    refused(b"nrows_dyn_word=2", nword=2)
    refused(b"nrows_dyn_word=8", nword=8, dyn=16)
    refused(b"pos_word=3", pos_word=3)
    refused(b"pos_word=8", pos_word=8, dyn=16)
    refused(b"n_stop=2", n_stop=2)                                                 # stop ids without a pointer
    refused(b"n_stop=65", n_stop=65, stop_ids=16)
    refused(b"n_stop=-1", n_stop=-1)
    refused(b"min_pos=-1", min_pos=-1)
    assert _call(h, min_pos_dev=16, min_pos=-1, tiles=0) == 0                     # a device array: the host value is unused


def test_header_binding_and_sources_agree():
    from dflash_amd import _lib, build
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    assert "min_pos" in txt and "dfl_logit_bias_rows" in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bdfl_logit_bias_rows\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m
    assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SIGNATURES["dfl_logit_bias_rows"][1]) == 24
    assert hasattr(_lib.lib(), "dfl_logit_bias_rows")
    assert "logit_bias.hip" in build.SOURCES
    src = open(os.path.join(H.ROOT, "dflash_amd", "csrc", "logit_bias.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd" not in src


# ------------------------------------------------------------------------------------------------------------ keywords
KEYS = {"logit_bias", "allowed_token_ids", "banned_token_ids", "min_tokens"}


def test_refusals_that_need_no_launch():
    import torch
    from dflash_amd import DFlashDraftModel
    from dflash_amd.batch import BatchedDecoder, dflash_generate_batch, dflash_generate_policy_batch
    from dflash_amd.engine import BatchEngine, dflash_generate_stream
    from dflash_amd.generate import DecodeSession, dflash_generate, dflash_generate_policy, run_decode
    from dflash_amd.target import NativeTarget
    model = SimpleNamespace(device=torch.device("cpu"))
    ids = torch.zeros(1, 8, dtype=torch.long)
    kw = dict(mask_token_id=5, max_new_tokens=8, stop_token_ids=[3])
    hf = SimpleNamespace(config=SimpleNamespace(vocab_size=64))             # a wrapped model: no NativeTarget
    # a target that is no NativeTarget: ValueError, through every single-request entry
    for bias in (dict(logit_bias={3: 1.0}), dict(allowed_token_ids=[1, 2]), dict(banned_token_ids=[4]), dict(min_tokens=2)):
        with pytest.raises(ValueError, match="NativeTarget"):
            DecodeSession(model, hf, ids, max_block_size=16, temperature=0.0, **kw, **bias)
        with pytest.raises(ValueError, match="NativeTarget"):
            DecodeSession(model, object(), ids, max_block_size=16, temperature=0.0, **kw, **bias)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(model, hf, ids, 5, 8, 16, [3], banned_token_ids=[4])
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate_policy(model=model, target=hf, input_ids=ids, temperature=0.0, fixed_block_size=8,
                               logit_bias={3: 1.0}, **kw)
    with pytest.raises(ValueError, match="NativeTarget"):
        run_decode(model, hf, ids, block_size=8, temperature=0.0, clamp_tail=True, min_tokens=3, **kw)
    # bad values, before anything else
    with pytest.raises(ValueError, match="outside"):
        DecodeSession(model, hf, ids, max_block_size=16, temperature=0.0, logit_bias={64: 1.0}, **kw)
    with pytest.raises(ValueError, match="min_tokens"):
        DecodeSession(model, hf, ids, max_block_size=16, temperature=0.0, min_tokens=-1, **kw)
    native = object.__new__(NativeTarget)       # (the checks come before the target is touched: a stand-in with a vocabulary)
    native.V = 64
    with pytest.raises(ValueError, match="empty"):
        dflash_generate_batch(None, native, [ids], 5, 8, 16, [3], allowed_token_ids=[])
    with pytest.raises(ValueError, match="one per prompt"):
        dflash_generate_stream(None, native, [ids], 5, 8, 16, [3], min_tokens=[1, 2])
    with pytest.raises(ValueError, match="one per prompt"):
        dflash_generate_batch(None, native, [ids, ids, ids], 5, 8, 16, [3], logit_bias=[{3: 1.0}, None])
    # T > 0 on the torch sampler; blocks of 17..32 rows
    bias = dict(logit_bias={3: 1.0}, min_tokens=2)
    with pytest.raises(ValueError, match="sampler='device'"):
        DecodeSession(model, native, ids, max_block_size=16, temperature=0.7, **kw, **bias)
    with pytest.raises(NotImplementedError, match="16 rows"):
        DecodeSession(model, native, ids, max_block_size=24, temperature=0.0, **kw, **bias)
    with pytest.raises(NotImplementedError, match="16 rows"):
        dflash_generate_batch(None, native, [ids], 5, 8, 24, [3], **bias)
    with pytest.raises(NotImplementedError, match="16 rows"):
        BatchedDecoder(None, native, 1, 64, 64, 5, tiles_per_request=2, logit_bias=True)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchedDecoder(None, native, 1, 64, 64, 5, temperature=0.7, logit_bias=True)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchEngine(None, native, max_rows=64, out_len=64, mask_token_id=5, temperature=0.7, logit_bias=True)
    # a request on a decoder / an engine built without the flag: ValueError; neutral values are no request for it
    dec = object.__new__(BatchedDecoder)
    dec.target, dec.stop_token_ids, dec.logit_bias = native, [3], False
    with pytest.raises(ValueError, match="logit_bias=True"):
        dec.check_bias(banned_token_ids=[4])
    with pytest.raises(ValueError, match="logit_bias=True"):
        dec.check_bias(min_tokens=1)
    assert dec.check_bias() is None and dec.check_bias(logit_bias={3: 0.0}, banned_token_ids=[], min_tokens=0) is None
    dec.stop_token_ids = None
    assert dec.check_bias(min_tokens=4) is None                                    # no stop ids: nothing to suppress
    # neutral values are the call without the keywords: nothing above is asked of them
    with pytest.raises(RuntimeError, match="GPU"):
        DecodeSession(model, hf, ids, max_block_size=24, temperature=0.7, logit_bias={3: 0.0}, banned_token_ids=[],
                      min_tokens=0, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        DecodeSession(model, object(), ids, max_block_size=24, temperature=0.7, mask_token_id=5, max_new_tokens=8,
                      stop_token_ids=None)
    # the keywords are where the issue puts them, and nowhere else
    for fn in (DecodeSession.__init__, run_decode, dflash_generate, dflash_generate_policy, DFlashDraftModel.spec_generate,
               dflash_generate_batch, dflash_generate_stream, BatchedDecoder.admit, BatchedDecoder.admit_fused,
               BatchEngine.submit):
        assert KEYS <= set(inspect.signature(fn).parameters), fn
    assert not KEYS & set(inspect.signature(dflash_generate_policy_batch).parameters)
    assert "logit_bias" in inspect.signature(BatchedDecoder.__init__).parameters
    assert "logit_bias" in inspect.signature(BatchEngine.__init__).parameters
    assert "logit_bias" in inspect.signature(NativeTarget.verify).parameters


def test_per_prompt_forms():
    from dflash_amd.batch import _prompt_bias
    tgt = SimpleNamespace(V=64)
    kws, on = _prompt_bias(tgt, None, None, None, 0, 3, [3])
    assert not on and all(k == dict(logit_bias=None, allowed_token_ids=None, banned_token_ids=None, min_tokens=0) for k in kws)
    kws, on = _prompt_bias(None, None, None, None, 0, 2, None)                     # the vocabulary is not needed
    assert not on
    kws, on = _prompt_bias(tgt, {3: 1.0}, [1, 2, 3], [4], 2, 2, [3])               # one value for every prompt
    assert on and kws[0] == kws[1] == dict(logit_bias={3: 1.0}, allowed_token_ids=[1, 2, 3], banned_token_ids=[4], min_tokens=2)
    kws, on = _prompt_bias(tgt, [{3: 1.0}, None], [None, [1, 2]], [[4], None], [0, 5], 2, [3])
    assert on and kws[0] == dict(logit_bias={3: 1.0}, allowed_token_ids=None, banned_token_ids=[4], min_tokens=0)
    assert kws[1] == dict(logit_bias=None, allowed_token_ids=[1, 2], banned_token_ids=None, min_tokens=5)
    kws, on = _prompt_bias(tgt, [{3: 0.0}, None], None, [[], None], 4, 2, None)    # all neutral
    assert not on
