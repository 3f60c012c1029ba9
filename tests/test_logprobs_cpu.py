"""Per-token logprobs without a GPU: every refusal of dfl_logprob_rows by name, header and binding
in step, the Python-level errors of the `logprobs` keyword, and the position-scatter argument as a pure simulation."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import helpers as H
import logprobs_ref as LR


def _call(h, logits=1, ld=64, tstride=1024, tiles=1, V=64, row0=0, nrows=16, dyn=None, nword=-1, pword=-1, pbase=0,
          padd=0, tpr=1, ids=1, istride=16, ioff=0, n_top=0, lp=1, top_ids=None, top_lp=None, lstride=100, llen=100):
    return h.dfl_logprob_rows(logits, ld, tstride, tiles, V, row0, nrows, dyn, nword, pword, pbase, padd, tpr, ids, istride,
                              ioff, n_top, lp, top_ids, top_lp, lstride, llen, None)


def test_entry_point_refuses_by_name():
    """Small integers stand for pointers: nothing launches."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(word, **kw):
        assert _call(h, **kw) == -22, kw
        err = h.dfl_last_error()
        assert b"dfl_logprob_rows:" in err and word in err, (kw, err)

    assert _call(h, tiles=0) == 0 and _call(h, nrows=0) == 0 and _call(h, llen=0, lstride=0) == 0   # nothing to do
    for name in ("logits", "ids", "lp"):
        refused(b"null", **{name: None})
    refused(b"V=0", V=0)
    refused(b"V=155656", V=155656, ld=155656)
    assert _call(h, V=155648, ld=155648, tiles=0) == 0
    refused(b"ld=32", ld=32)
    refused(b"tile_stride=512", tiles=2, tstride=512)
    refused(b"rows [4,17)", row0=4, nrows=13)
    refused(b"rows [-1,", row0=-1, nrows=2)
    refused(b"rows [0,-1)", nrows=-1)
    refused(b"n_top=9", n_top=9, top_ids=1, top_lp=1)
    refused(b"n_top=-1", n_top=-1)
    refused(b"top_ids_out", n_top=3)
    refused(b"top_ids_out", n_top=3, top_ids=1)
    refused(b"top_ids_out", n_top=3, top_lp=1)
    refused(b"nrows_dyn_word=2", nword=2)                    # a record word without a record
    refused(b"pos_word=3", pword=3)
    refused(b"nrows_dyn_word=8", nword=8, dyn=1)             # outside the record
    refused(b"pos_word=8", pword=8, dyn=1)
    refused(b"tiles_per_req=3", tpr=3)
    refused(b"tiles_per_req=0", tpr=0)
    refused(b"ids_off=-1", ioff=-1)
    refused(b"ids_stride=-16", istride=-16)
    refused(b"lp_len=-1", llen=-1)
    refused(b"lp_stride=50", lstride=50)


def test_header_and_binding_agree():
    from dflash_amd import _lib, build
    txt = open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bdfl_logprob_rows\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, "dfl_logprob_rows is not declared"
    params = [p for p in m.group(1).split(",") if p.strip()]
    assert len(params) == len(_lib.SIGNATURES["dfl_logprob_rows"][1]) == 23
    assert "logprobs.hip" in build.SOURCES
    assert hasattr(_lib.lib(), "dfl_logprob_rows")


def test_keyword_errors():
    import torch
    from dflash_amd import ops
    from dflash_amd.batch import dflash_generate_batch
    from dflash_amd.generate import DecodeSession, dflash_generate
    assert ops.check_logprobs(None) is None
    assert [ops.check_logprobs(n) for n in range(9)] == list(range(9))
    for bad in (-1, 9, 2.5, True, 100):
        with pytest.raises(ValueError, match="logprobs"):
            ops.check_logprobs(bad)
    model = SimpleNamespace(device=torch.device("cpu"))
    ids = torch.zeros(1, 8, dtype=torch.long)
    kw = dict(mask_token_id=5, max_new_tokens=8, max_block_size=16, stop_token_ids=None, temperature=0.0)
    # a target that is no NativeTarget: refused before anything touches a device
    with pytest.raises(ValueError, match="NativeTarget"):
        DecodeSession(model, object(), ids, logprobs=0, **kw)
    with pytest.raises(ValueError, match="logprobs"):
        DecodeSession(model, object(), ids, logprobs=9, **kw)
    with pytest.raises(ValueError, match="NativeTarget"):
        dflash_generate(model, object(), ids, 5, 8, 16, None, logprobs=3)
    with pytest.raises(ValueError, match="logprobs"):
        dflash_generate_batch(None, None, [ids], 5, 8, 16, None, logprobs=-2)
    # spec_generate keeps the reference's signature
    import inspect
    from dflash_amd import DFlashDraftModel
    assert "logprobs" not in inspect.signature(DFlashDraftModel.spec_generate).parameters


def test_reference_definitions():
    x = LR.bf16_round(np.array([1.0, -np.inf, 3.0, 3.0, -0.0, 0.0, 2.5], dtype=np.float32))
    want = np.log(np.exp(1.0) + 2 * np.exp(3.0) + 2.0 + np.exp(2.5))
    assert abs(LR.lse(x) - want) < 1e-12
    assert np.isnan(LR.logprob(x, -1)) and np.isnan(LR.logprob(x, 7))
    assert LR.logprob(x, 1) == -np.inf
    ids, lps = LR.top(x, 8)
    assert ids.tolist() == [2, 3, 6, 0, 4, 5, 1, -1]           # ties to the lower column; -0 == +0; past V: -1
    assert np.isnan(lps[7]) and lps[6] == -np.inf and abs(lps[0] - (3.0 - want)) < 1e-12
    assert LR.lse(np.full(4, -np.inf)) == -np.inf
    assert LR.position(100, 1, 1, 3) == 120


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_scatter_by_position_keeps_the_committing_cycles_value(seed):
    """A few hundred cycles of random block sizes and acceptance lengths: verify row j of a cycle at `start` writes its
    value at start + j + 1 whether or not the row is accepted; the next cycle starts at start + tau and rewrites
    everything past its own start.  The buffer's first final-length entries then hold, per position, the value of the
    cycle that committed it, and the trim drops whatever the last cycles wrote past the end."""
    rng = np.random.default_rng(seed)
    n_in, max_new = 11, 3000
    max_len = n_in + max_new
    buf = np.full(max_len + 32, np.nan)
    truth = {}
    val = lambda cyc, j: cyc * 100.0 + j   # noqa: E731  (a value that names the cycle and the row)
    buf[n_in] = truth[n_in] = -1.0         # the prefill's token
    start, cyc = n_in, 0
    while start < max_len:
        bs = max(1, min(int(rng.integers(1, 33)), max_len - start))
        tau = int(rng.integers(1, bs + 1))           # accepted draft tokens + the bonus token
        LR.scatter(buf, start, [val(cyc, j) for j in range(bs)])
        for j in range(tau):                         # positions start + 1 .. start + tau are committed by this cycle
            truth[start + j + 1] = val(cyc, j)
        start += tau
        cyc += 1
    assert cyc > 200
    final = min(start + 1, max_len)                  # ids are trimmed to max_length
    got = buf[n_in:final]
    assert not np.isnan(got).any()
    assert got.tolist() == [truth[p] for p in range(n_in, final)]
    assert not np.isnan(buf[final:start + 1]).any() or final == start + 1   # (the tail was written, and is trimmed)
