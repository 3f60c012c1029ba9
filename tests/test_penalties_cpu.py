"""Repetition / presence / frequency penalties without a GPU: the numpy model of the contract
against transformers' repetition rule and against the written formula, every refusal of the two entry points through the
C ABI, check_penalties, and the Python-level refusals that need no launch."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import penalties_ref as PR


def _bf16_bits(x):
    return PR.f32_to_bf16_bits(np.asarray(x, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------ the model
@pytest.mark.parametrize("r", [1.3, 0.8, 2.0])
def test_repetition_step_is_the_hf_rule(r):
    """Step 1 alone (a = f = 0, before the bf16 rounding) equals RepetitionPenaltyLogitsProcessor exactly in fp32."""
    import torch
    from transformers import RepetitionPenaltyLogitsProcessor
    rng = np.random.default_rng(5)
    V = 512
    x = PR.bits_to_f32(_bf16_bits(rng.standard_normal((6, V)) * 3))
    x[:, ::17] = 0.0
    ids = rng.integers(0, V, (6, 40))
    ids[:, :5] = np.arange(0, 85, 17)          # zero logits among the seen ones
    got = RepetitionPenaltyLogitsProcessor(penalty=r)(torch.tensor(ids), torch.tensor(x.copy())).numpy()
    for i in range(6):
        seen, c = PR.history(ids[i], n_in=40, p=40, V=V)   # prompt only: presence / frequency see nothing
        assert c.sum() == 0 and seen.sum() == len(set(ids[i].tolist()))
        y3 = PR.step3_f64(_bf16_bits(x[i]), seen, c, r, 0.0, 0.0).astype(np.float32)
        assert np.array_equal(y3.view(np.uint32) & 0x7FFFFFFF, got[i].view(np.uint32) & 0x7FFFFFFF)   # (-0 == +0)
        assert (x[i][seen] > 0).any() and (x[i][seen] < 0).any() and (x[i][seen] == 0).any()


def test_presence_and_frequency_follow_the_written_formula():
    V, n_in = 16, 4
    ids = [3, 5, 5, 9, 7, 7, 3, 7, 11, 99, -4]      # prompt 3 5 5 9; output 7 7 3 7 11 and two ids outside [0, V)
    seen, c = PR.history(ids, n_in, len(ids), V)
    assert c.tolist() == [0, 0, 0, 1, 0, 0, 0, 3, 0, 0, 0, 1, 0, 0, 0, 0]
    assert np.nonzero(seen)[0].tolist() == [3, 5, 7, 9, 11]
    x = np.array([2.0, -1.0, 0.5, 2.0, 1.0, -2.0, 3.0, 4.0, 1.0, 1.5, 0.0, -0.0, 1.0, 1.0, 1.0, 1.0], dtype=np.float32)
    r, a, f = 1.5, 0.25, 0.125
    z = PR.bits_to_f32(PR.penalise(_bf16_bits(x), seen, c, r, a, f))
    want = x.copy()
    want[3] = 2.0 / 1.5 - 0.25 - 0.125          # prompt and output
    want[5] = -2.0 * 1.5                        # prompt only: repetition applies, presence and frequency do not
    want[9] = 1.5 / 1.5                         # prompt only
    want[7] = 4.0 / 1.5 - 0.25 - 3 * 0.125      # output only, three times
    want[11] = -0.0 * 1.5 - 0.25 - 0.125        # -0 takes the x * r branch
    assert np.array_equal(z, PR.bits_to_f32(_bf16_bits(want)))
    # a token that occurs only in the prompt: seen, never counted
    assert seen[5] and c[5] == 0 and seen[9] and c[9] == 0
    # the table holds the same history: bit 31 from the prompt, the count from the output
    t = PR.table_of(ids, n_in, len(ids), V).view(np.uint32)
    assert t[3] == 0x80000001 and t[5] == 0x80000000 and t[7] == 3 and t[11] == 1 and t[0] == 0
    s2, c2 = PR.seen_counts(t)
    assert np.array_equal(s2, seen) and np.array_equal(c2, c)
    # in-block tokens count as output on top of the table
    s3, c3 = PR.seen_counts(t, [7, 0, 0, 20])
    assert c3[7] == 4 and c3[0] == 2 and s3[0] and c3.sum() == c.sum() + 3


def test_neutral_values_copy_every_bit_pattern():
    bits = np.arange(1 << 16, dtype=np.uint16)
    for seen, c in ((np.zeros(1 << 16, bool), np.zeros(1 << 16, np.int64)),
                    (np.ones(1 << 16, bool), np.full(1 << 16, 7, np.int64))):
        assert np.array_equal(PR.penalise(bits, seen, c, 1.0, 0.0, 0.0), bits)
    # +-inf and NaN under real penalties: the IEEE operations, a NaN with its bits
    sp = np.array([0x7F80, 0xFF80, 0x7FC1, 0xFFFF, 0x8000, 0x0000], dtype=np.uint16)
    z = PR.penalise(sp, np.ones(6, bool), np.full(6, 2, np.int64), 1.3, 0.2, 0.25)
    assert z[:4].tolist() == [0x7F80, 0xFF80, 0x7FC1, 0xFFFF]
    assert z[4] == z[5] == _bf16_bits(np.float32(-0.2) - np.float32(0.5))       # +-0 * r = +-0, - a, - 2 f
    assert PR.argmax_lowest(np.array([0x7FC0, 0x3F80, 0x3F80, 0xFFC0], dtype=np.uint16)) == 1
    assert PR.argmax_lowest(np.array([0x7FC0, 0x7FC0], dtype=np.uint16)) == 0
    assert PR.argmax_lowest(np.array([0x8000, 0x0000, 0xBF80], dtype=np.uint16)) == 0      # -0 == +0: the lower column


def test_midpoint_screen_is_rare_on_the_test_inputs():
    """The inputs of the GPU tests stay under the cap of near-midpoint elements with the model alone (and r = 1.3 would
    not: one bf16 logit in a hundred lands x * 1.3 on an exact bf16 midpoint)."""
    for V in (48, 2048, 151936):
        rng = np.random.default_rng(V)
        x = PR.case_rows(rng, 1, V)[0]
        seen, c = PR.seen_counts(PR.case_table(rng, V), rng.integers(0, V, 15))
        assert (~seen).sum() > V // 4 and (c > 0).sum() > V // 8 and (seen & (c == 0)).sum() >= 1
        for r, a, f in PR.KERNEL_PARAMS:
            near = PR.near_midpoint(x, seen, c, r, a, f)
            assert near.mean() <= 1e-3, (V, r, near.mean())
            assert not near[~seen].any()
    assert PR.near_midpoint(x, seen, c, 1.3, 0.2, 0.25).mean() > 1e-3
    # the screen itself: a value on a midpoint, one a little off it, a bf16 value
    y = np.array([0x3F80, 0x3F81], dtype=np.uint16)
    one = np.ones(2, bool)
    assert PR.near_midpoint(y, one, np.array([1, 1]), 1.0, 2.0 ** -8, 0.0).tolist() == [False, True]   # 1 - 2^-8 is a bf16 value below 1
    assert PR.near_midpoint(y, one, np.array([1, 1]), 1.0, -2.0 ** -8, 0.0).tolist() == [True, True]
    assert PR.near_midpoint(y, one, np.array([1, 1]), 1.0, -2.0 ** -8 * 1.001, 0.0).tolist() == [False, False]
    assert PR.near_midpoint(y, one, np.array([0, 0]), 1.0, 0.0, 0.0).tolist() == [False, False]


# ------------------------------------------------------------------------------------------------------------ the C ABI
def _rows(h, logits=16, out=32, ld=64, tstride=1024, tiles=1, V=64, row0=0, nrows=16, dyn=None, nword=-1, tpr=1, table=48,
          tab_stride=64, block=None, blk_stride=0, r_dev=None, r=1.3, a_dev=None, a=0.2, f_dev=None, f=0.25, out_ids=None,
          out_stride=0, out_off=0):
    return h.dfl_penalty_rows(logits, out, ld, tstride, tiles, V, row0, nrows, dyn, nword, tpr, table, tab_stride, block,
                              blk_stride, r_dev, r, a_dev, a, f_dev, f, out_ids, out_stride, out_off, None)


def _count(h, table=16, tab_stride=64, V=64, slots=1, ids=32, ids_stride=100, ids_len=100, dyn=None, lo_word=0, hi_word=4,
           lo=0, hi=10, as_prompt=0, clear=0):
    return h.dfl_penalty_count(table, tab_stride, V, slots, ids, ids_stride, ids_len, dyn, lo_word, hi_word, lo, hi,
                               as_prompt, clear, None)


def test_entry_points_refuse_by_name():
    """Small integers stand for pointers: nothing launches."""
    from dflash_amd import _lib
    h = _lib.lib()
    inf, nan = float("inf"), float("nan")

    def refused(fn, name, word, **kw):
        assert fn(h, **kw) == -22, kw
        err = h.dfl_last_error()
        assert name in err and word in err, (kw, err)

    assert _rows(h, tiles=0) == 0 and _rows(h, nrows=0) == 0 and _count(h, slots=0) == 0      # nothing to do
    for name in ("logits", "out", "table"):
        refused(_rows, b"dfl_penalty_rows:", b"null", **{name: None})
    for V in (0, -8, 4, 60, 155656):
        refused(_rows, b"dfl_penalty_rows:", b"V=", V=V, ld=max(V, 64), tab_stride=max(V, 64))
    for bad in (0.0, -1.0, inf, nan):
        refused(_rows, b"dfl_penalty_rows:", b"repetition", r=bad)
    for bad in (inf, -inf, nan):
        refused(_rows, b"dfl_penalty_rows:", b"presence", a=bad)
        refused(_rows, b"dfl_penalty_rows:", b"frequency", f=bad)
    assert _rows(h, r_dev=16, r=nan, a_dev=16, a=inf, f_dev=16, f=nan, tiles=0) == 0     # device arrays: host values unused
    for tpr in (0, 3):
        refused(_rows, b"dfl_penalty_rows:", b"tiles_per_req", tpr=tpr)
    refused(_rows, b"dfl_penalty_rows:", b"ld=32", ld=32)
    refused(_rows, b"dfl_penalty_rows:", b"bad shape", logits=18)                       # a row off 16 bytes
    refused(_rows, b"dfl_penalty_rows:", b"tile_stride=512", tiles=2, tstride=512)
    refused(_rows, b"dfl_penalty_rows:", b"table_stride=32", tab_stride=32)
    refused(_rows, b"dfl_penalty_rows:", b"rows [4,17)", row0=4, nrows=13)
    refused(_rows, b"dfl_penalty_rows:", b"nrows_dyn_word=2", nword=2)
    refused(_rows, b"dfl_penalty_rows:", b"nrows_dyn_word=8", nword=8, dyn=16)
    for name in ("table", "ids"):
        refused(_count, b"dfl_penalty_count:", b"null", **{name: None})
    for V in (0, 12, 155656):
        refused(_count, b"dfl_penalty_count:", b"V=", V=V, tab_stride=max(V, 64))
    refused(_count, b"dfl_penalty_count:", b"table_stride=32", tab_stride=32)
    refused(_count, b"dfl_penalty_count:", b"table_stride", table=20)
    refused(_count, b"dfl_penalty_count:", b"ids_len=-1", ids_len=-1)
    refused(_count, b"dfl_penalty_count:", b"lo_word=8", dyn=16, lo_word=8)
    refused(_count, b"dfl_penalty_count:", b"hi_word=-1", dyn=16, hi_word=-1)


def test_header_binding_and_sources_agree():
    from dflash_amd import _lib, build
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    assert "bit 31" in txt and "fmaf(-f, float(c), y2)" in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, n in (("dfl_penalty_count", 15), ("dfl_penalty_rows", 25)):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
        assert m, name
        assert len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SIGNATURES[name][1]) == n
        assert hasattr(_lib.lib(), name)
    assert "penalties.hip" in build.SOURCES
    assert len([n for n in _lib.SIGNATURES if n.startswith("dfl_penalty")]) == 2


# ------------------------------------------------------------------------------------------------------------ keywords
def test_check_penalties():
    from dflash_amd import ops
    assert ops.check_penalties() is None and ops.check_penalties(1.0, 0.0, 0.0) is None and ops.check_penalties(1, 0, -0.0) is None
    assert ops.check_penalties(1.3, 0.2, 0.25) == (1.3, 0.2, 0.25)
    assert ops.check_penalties(1.0, 0.0, -0.5) == (1.0, 0.0, -0.5) and ops.check_penalties(0.5) == (0.5, 0.0, 0.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="repetition_penalty"):
            ops.check_penalties(bad)
    for bad in (float("inf"), float("nan")):
        with pytest.raises(ValueError, match="presence_penalty"):
            ops.check_penalties(1.0, bad)
        with pytest.raises(ValueError, match="frequency_penalty"):
            ops.check_penalties(1.0, 0.0, bad)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.penalty_state(1, 2047, "cpu")


def test_refusals_that_need_no_launch():
    import torch
    from dflash_amd import DFlashDraftModel
    from dflash_amd.batch import BatchedDecoder, dflash_generate_batch, dflash_generate_policy_batch
    from dflash_amd.engine import dflash_generate_stream
    from dflash_amd.generate import DecodeSession, dflash_generate, dflash_generate_policy, run_decode
    from dflash_amd.target import NativeTarget
    model = SimpleNamespace(device=torch.device("cpu"))
    ids = torch.zeros(1, 8, dtype=torch.long)
    kw = dict(mask_token_id=5, max_new_tokens=8, stop_token_ids=None)
    pen = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.25)
    # a target that is no NativeTarget
    with pytest.raises(ValueError, match="NativeTarget"):
        DecodeSession(model, object(), ids, max_block_size=16, temperature=0.0, **kw, **pen)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(model, object(), ids, 5, 8, 16, None, frequency_penalty=0.1)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate_policy(model=model, target=object(), input_ids=ids, temperature=0.0, fixed_block_size=8,
                               presence_penalty=0.1, **kw)
    # bad values, before anything else
    with pytest.raises(ValueError, match="repetition_penalty"):
        DecodeSession(model, object(), ids, max_block_size=16, temperature=0.0, repetition_penalty=0.0, **kw)
    with pytest.raises(ValueError, match="frequency_penalty"):
        dflash_generate_batch(None, None, [ids], 5, 8, 16, None, frequency_penalty=float("nan"))
    with pytest.raises(ValueError, match="one value per prompt"):
        dflash_generate_stream(None, None, [ids], 5, 8, 16, None, presence_penalty=[0.1, 0.2])
    # T > 0 on the torch sampler; blocks of 17..32 rows (the checks come before the target is touched: a stand-in passes
    # isinstance only)
    native = object.__new__(NativeTarget)
    with pytest.raises(ValueError, match="sampler='device'"):
        DecodeSession(model, native, ids, max_block_size=16, temperature=0.7, **kw, **pen)
    with pytest.raises(NotImplementedError, match="16 rows"):
        DecodeSession(model, native, ids, max_block_size=24, temperature=0.0, **kw, **pen)
    with pytest.raises(NotImplementedError, match="16 rows"):
        dflash_generate_batch(None, None, [ids], 5, 8, 24, None, **pen)
    with pytest.raises(NotImplementedError, match="16 rows"):
        BatchedDecoder(None, native, 1, 64, 64, 5, tiles_per_request=2, penalties=True)
    with pytest.raises(ValueError, match="sampler='device'"):
        BatchedDecoder(None, native, 1, 64, 64, 5, temperature=0.7, penalties=True)
    # neutral values are the call without the keywords: nothing above is asked of them
    with pytest.raises(RuntimeError, match="GPU"):
        DecodeSession(model, object(), ids, max_block_size=24, temperature=0.7, repetition_penalty=1.0, **kw)
    # the keywords are where the issue puts them, and nowhere else
    for fn in (DecodeSession.__init__, run_decode, dflash_generate, dflash_generate_policy, DFlashDraftModel.spec_generate,
               dflash_generate_batch, dflash_generate_stream):
        assert {"repetition_penalty", "presence_penalty", "frequency_penalty"} <= set(inspect.signature(fn).parameters), fn
    assert "repetition_penalty" not in inspect.signature(dflash_generate_policy_batch).parameters
