"""Stop sequences without a GPU: the refusals of ops.check_stop_sequences by their messages, the
trim on hand-made rows against the model of stop_seq_ref.py, the DFL_EINVAL cases of dfl_stop_seq_rows (small integers
stand for pointers: nothing launches) and the "built with stop_sequences=True" refusals of decoder and engine."""
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

import helpers as H
import stop_seq_ref as SR

MASK = 63
V = 64


# ------------------------------------------------------------------------------------------------- check_stop_sequences
def test_check_stop_sequences_normalises():
    from dflash_amd import ops
    assert ops.check_stop_sequences(None, V, MASK) is None
    assert ops.check_stop_sequences([], V, MASK) is None
    assert ops.check_stop_sequences([[1, 2], (3,), 4, torch.tensor([5, 6])], V, MASK) == [[1, 2], [3], [4], [5, 6]]
    assert ops.check_stop_sequences([list(range(16))] * 8, V, MASK) == [list(range(16))] * 8
    assert ops.STOP_SEQS == SR.SEQS == 8 and ops.STOP_SEQ_LEN == SR.SEQ_LEN == 16


@pytest.mark.parametrize("seqs, message", [
    ([[1], []], r"stop_sequences\[1\] is empty"),
    ([[1]] * 9, "9 stop sequences, more than 8"),
    ([list(range(17))], r"stop_sequences\[0\] has 17 ids, more than 16"),
    ([[1, 64]], r"stop_sequences\[0\]: id 64 outside \[0, 64\)"),
    ([[-1]], r"id -1 outside \[0, 64\)"),
    ([[1], [2, MASK]], r"stop_sequences\[1\] holds the mask id 63"),
    ([[1.5]], "is not a token id"),
    (["ab"], "is text"),
    (7, "must be a list"),
])
def test_check_stop_sequences_refuses_by_name(seqs, message):
    from dflash_amd import ops
    with pytest.raises(ValueError, match=message):
        ops.check_stop_sequences(seqs, V, MASK)


# ---------------------------------------------------------------------------------------------------------------- trim
def _trim_both(row, max_length, stop_ids, n_in, hit, seqs, include):
    """(ids kept by generate._kept_cols / _trim, the index it reports) after checking both against the model."""
    from dflash_amd.generate import _kept_cols, _trim
    t = torch.tensor([row], dtype=torch.long)
    sh = None if hit is None else (hit[0], hit[1], len(seqs[hit[1]]), include)
    which = []
    cols = _kept_cols(t, max_length, MASK, stop_ids, n_in, sh, which).tolist()
    want, want_k = SR.trim(row, max_length, MASK, stop_ids, n_in, hit, [len(s) for s in seqs], include)
    assert cols == want and (which[0] if which else None) == want_k
    assert _trim(t, max_length, MASK, stop_ids, n_in, sh)[0].tolist() == [row[c] for c in cols]
    return [row[c] for c in cols], want_k


def test_trim_on_hand_made_rows():
    #      0  1  2 | 3  4  5  6  7  8  9 | mask ...
    row = [9, 9, 9, 1, 2, 3, 4, 5, 6, 7, MASK, MASK]
    seqs = [[8, 8], [4, 5]]
    # no hit, no stop id: everything up to max_length that is not the mask
    assert _trim_both(row, 10, None, 3, None, seqs, True) == (row[:10], None)
    # the sequence [4, 5] ends at position 7: kept with it, cut without it
    assert _trim_both(row, 10, None, 3, [7, 1], seqs, True) == (row[:8], 1)
    assert _trim_both(row, 10, None, 3, [7, 1], seqs, False) == (row[:6], 1)
    # a stop id (2, position 4) earlier than the sequence: the stop id decides, and stays
    assert _trim_both(row, 10, [2], 3, [7, 1], seqs, False) == (row[:5], None)
    # the sequence earlier than a stop id (6, position 8)
    assert _trim_both(row, 10, [6], 3, [7, 1], seqs, True) == (row[:8], 1)
    assert _trim_both(row, 10, [6], 3, [7, 1], seqs, False) == (row[:6], 1)
    # a match at the last kept column (max_length = 8 keeps positions 0..7), and one column further: past the end
    assert _trim_both(row, 8, None, 3, [7, 1], seqs, True) == (row[:8], 1)
    assert _trim_both(row, 8, None, 3, [7, 1], seqs, False) == (row[:6], 1)
    assert _trim_both(row, 7, None, 3, [7, 1], seqs, False) == (row[:7], None)
    # the sequence's last id is itself a stop id: the sequence is reported
    assert _trim_both(row, 10, [5], 3, [7, 1], seqs, False) == (row[:6], 1)
    # a length-1 sequence equal to the first token
    assert _trim_both(row, 10, None, 3, [3, 0], [[1]], True) == (row[:4], 0)
    assert _trim_both(row, 10, None, 3, [3, 0], [[1]], False) == (row[:3], 0)
    # the record of a request that never matched
    assert _trim_both(row, 10, None, 3, [-1, -1], seqs, True)[0] == row[:10]


def test_trim_without_a_hit_is_the_trim_of_before():
    from dflash_amd.generate import _kept_cols, _trim
    row = torch.tensor([[9, 9, 1, 2, 3, MASK, 4, MASK]], dtype=torch.long)
    assert _trim(row, 7, MASK, [3], 2).tolist() == [[9, 9, 1, 2, 3]]
    assert _kept_cols(row, 7, MASK, [3], 2).tolist() == [0, 1, 2, 3, 4]
    assert _trim(row, 7, MASK, None, 2).tolist() == [[9, 9, 1, 2, 3, 4]]


def test_reference_model():
    """The model itself on a hand-made cycle: block / posterior with two accepted tokens and the bonus."""
    out = [7, 7, 1, 2, 0, 0, 0, 0]          # positions 0..3 committed, start = 3 (the previous bonus token, 2)
    block, post = [2, 3, 4, 9], [3, 4, 5, 6]   # block[1] == post[0], block[2] == post[1], block[3] != post[2]: acc = 2
    assert SR.accepted(block, post, 4) == 2 and SR.committed(block, post, 4) == [3, 4, 5]
    m = lambda seqs, fp=2, me=0: SR.match(block, post, out, 3, 4, seqs, fp, me)   # noqa: E731
    assert m([[3, 4]]) == (5, 0) and m([[5]]) == (6, 0) and m([[2, 3]]) == (4, 0) and m([[1, 2, 3]]) == (4, 0)
    assert m([[9]]) is None and m([[4, 9]]) is None            # the rejected draft token
    assert m([[7, 1, 2, 3]]) is None and m([[7, 1, 2, 3]], fp=1) == (4, 0)   # one token inside the prompt
    assert m([[3]], me=5) is None and m([[3]], me=4) == (4, 0)
    assert m([[4, 5], [5]]) == (6, 0) and m([[5], [4, 5]]) == (6, 0) and m([[5], [3]]) == (4, 1)
    dyn = [[0, 0, 4, 0, 3, 0, 0, 0]]
    t = [dict(seqs=[[4]], first_pos=2, min_end=0, hit=[-1, -1])]
    SR.launch([block], [post], [out], dyn, t)
    assert dyn[0][SR.STOP] == 1 and t[0]["hit"] == [5, 0]
    t[0]["seqs"] = [[3]]
    SR.launch([block], [post], [out], dyn, t)
    assert t[0]["hit"] == [5, 0]                                # sticky


# ----------------------------------------------------------------------------------------------------------- the C ABI
def _call(h, **kw):
    a = dict(block=16, blk_stride=16, post=16, post_stride=16, out=16, out_stride=64, out_len=64, dyn=16, slots=1, bs=16,
             seq_ids=16, seq_len=16, first_pos=16, min_end=16, hit=16)
    a.update(kw)
    return h.dfl_stop_seq_rows(a["block"], a["blk_stride"], a["post"], a["post_stride"], a["out"], a["out_stride"],
                               a["out_len"], a["dyn"], a["slots"], a["bs"], a["seq_ids"], a["seq_len"], a["first_pos"],
                               a["min_end"], a["hit"], None)


def test_entry_point_refuses_by_name():
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(word, **kw):
        assert _call(h, **kw) == -22, kw
        err = h.dfl_last_error()
        assert b"dfl_stop_seq_rows:" in err and word in err, (kw, err)

    for name in ("block", "post", "out", "dyn", "seq_ids", "seq_len", "first_pos", "min_end", "hit"):
        refused(b"null", **{name: None})
    for slots in (0, -1):
        refused(b"slots=", slots=slots)
    refused(b"bs=33", bs=33, blk_stride=64, post_stride=64)
    refused(b"blk_stride=8", blk_stride=8)
    refused(b"post_stride=15", post_stride=15)
    refused(b"blk_stride=0", bs=-1, blk_stride=0)                  # the record's size: at least one row
    refused(b"out_stride=32", out_stride=32)
    refused(b"output_len=0", out_len=0)
    assert _call(h, bs=0) == 0                                     # every slot idle: nothing to launch


def test_header_binding_and_sources_agree():
    from dflash_amd import _lib, build
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    assert "#define DFL_STOP_SEQS 8" in txt and "#define DFL_STOP_SEQ_LEN 16" in txt
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bdfl_stop_seq_rows\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m and len([p for p in m.group(1).split(",") if p.strip()]) == len(_lib.SIGNATURES["dfl_stop_seq_rows"][1]) == 16
    assert "stop_seq.hip" in build.SOURCES
    # the accept kernels and their ABI stay as they are: the match is a launch of its own
    acc = open(os.path.join(H.ROOT, "dflash_amd", "csrc", "accept.hip")).read()
    assert "seq_ids" not in acc and "stop_seq" not in acc
    src = open(os.path.join(H.ROOT, "dflash_amd", "csrc", "stop_seq.hip")).read()
    assert "atomic" not in src and "asm" not in src


# ------------------------------------------------------------------------------------------------------------ keywords
def test_refusals_that_need_no_launch():
    from dflash_amd import DFlashDraftModel
    from dflash_amd.batch import BatchedDecoder, _prompt_stop_sequences, dflash_generate_batch, dflash_generate_policy_batch
    from dflash_amd.candidates import dflash_generate_candidate_solutions
    from dflash_amd.engine import BatchEngine, dflash_generate_stream
    from dflash_amd.generate import DecodeSession, dflash_generate, dflash_generate_policy, run_decode
    from dflash_amd.target import NativeTarget
    model = SimpleNamespace(device=torch.device("cpu"))
    ids = torch.zeros(1, 8, dtype=torch.long)
    kw = dict(mask_token_id=MASK, max_new_tokens=8, stop_token_ids=None)
    hf = SimpleNamespace(config=SimpleNamespace(vocab_size=V))
    native = object.__new__(NativeTarget)
    native.V = V
    # bad values, before anything touches the GPU, through every entry; any target will do
    for tgt in (hf, native):
        with pytest.raises(ValueError, match="is empty"):
            DecodeSession(model, tgt, ids, max_block_size=16, temperature=0.0, stop_sequences=[[]], **kw)
        with pytest.raises(ValueError, match="mask id"):
            dflash_generate(model, tgt, ids, MASK, 8, 16, None, stop_sequences=[[1, MASK]])
    with pytest.raises(ValueError, match="more than 16"):
        dflash_generate_policy(model=model, target=hf, input_ids=ids, temperature=0.0, fixed_block_size=8,
                               stop_sequences=[list(range(17))], **kw)
    with pytest.raises(ValueError, match="outside"):
        run_decode(model, hf, ids, block_size=8, temperature=0.0, clamp_tail=True, stop_sequences=[[V]], **kw)
    with pytest.raises(ValueError, match="more than 8"):
        dflash_generate_batch(None, native, [ids], MASK, 8, 16, None, stop_sequences=[[1]] * 9)
    with pytest.raises(ValueError, match="is empty"):
        dflash_generate_stream(None, native, [ids, ids], MASK, 8, 16, None, stop_sequences=[[[1]], [[]]])
    with pytest.raises(ValueError, match="outside"):
        dflash_generate_policy_batch(model=None, target=native, input_ids=[ids], mask_token_id=MASK, max_new_tokens=8,
                                     stop_token_ids=None, temperature=0.0, schedulers=[None], stop_sequences=[[V]])
    # valid sequences pass the checks (the next refusal is the CPU tensor)
    with pytest.raises(RuntimeError, match="GPU"):
        DecodeSession(model, hf, ids, max_block_size=16, temperature=0.0, stop_sequences=[[1, 2], 3], **kw)
    # the multi-candidate loop refuses by name
    with pytest.raises(NotImplementedError, match="stop_sequences"):
        dflash_generate_candidate_solutions(None, None, ids, MASK, 8, 16, None, stop_sequences=[[1]])
    # a request on a decoder / an engine built without the flag
    dec = object.__new__(BatchedDecoder)
    dec.model, dec.target, dec.stop_token_ids, dec.sampler, dec.mask_id = None, native, None, "device", MASK
    dec.penalties, dec.filtering, dec.logit_bias, dec.min_p, dec.sq = False, False, False, False, None
    with pytest.raises(ValueError, match="stop_sequences need a decoder built with stop_sequences=True"):
        dec.admit(0, ids, 0.0, stop_sequences=[[1, 2]])
    dec.TPR, dec.R = 1, 1
    with pytest.raises(ValueError, match="need a decoder built with stop_sequences=True"):
        dec.admit_fused(0, ids, 0.0, stop_sequences=[[1, 2]])
    with pytest.raises(ValueError, match="is empty"):
        dec.admit(0, ids, 0.0, stop_sequences=[[]])
    eng = object.__new__(BatchEngine)
    eng.dec = dec
    with pytest.raises(ValueError, match="built with stop_sequences=True"):
        eng.submit(ids, 8, stop_sequences=[[1, 2]])
    with pytest.raises(ValueError, match="mask id"):
        eng.submit(ids, 8, stop_sequences=[[MASK]])
    # the per-prompt forms
    assert _prompt_stop_sequences(None, 2, None, MASK) == [None, None]
    assert _prompt_stop_sequences([[1, 2], [3]], 2, native, MASK) == [[[1, 2], [3]]] * 2          # one list for every prompt
    assert _prompt_stop_sequences([[[1, 2]], [[3], [4]]], 2, native, MASK) == [[[1, 2]], [[3], [4]]]
    assert _prompt_stop_sequences([None, [[3]]], 2, native, MASK) == [None, [[3]]]
    # the keywords are where the issue puts them
    for fn in (DecodeSession.__init__, run_decode, dflash_generate, dflash_generate_policy, DFlashDraftModel.spec_generate,
               dflash_generate_batch, dflash_generate_policy_batch, dflash_generate_stream, BatchEngine.submit):
        ps = inspect.signature(fn).parameters
        assert ps["stop_sequences"].default is None and ps["include_stop_sequence"].default is True, fn
    for fn in (BatchedDecoder.admit, BatchedDecoder.admit_fused):
        assert inspect.signature(fn).parameters["stop_sequences"].default is None, fn
    for fn in (BatchedDecoder.__init__, BatchEngine.__init__):
        assert inspect.signature(fn).parameters["stop_sequences"].default is False, fn
