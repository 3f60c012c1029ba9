"""No-GPU parts of the prompt logprobs: the refusals of dfl_prefill_logprobs through the library,
the Python refusals of the keyword, and the empty result of a one-token prompt."""
import types

import pytest
import torch


def test_prefill_logprobs_validates_without_a_gpu():
    from dflash_amd import _lib
    h = _lib.lib()

    def call(wp=16, xf=16, rows=17, V=4208, K=256, tg=16, nsplit=2, ws=16, out=16):   # never dereferenced: validation only
        return h.dfl_prefill_logprobs(wp, xf, rows, V, K, tg, nsplit, ws, out, None)

    for name in ("wp", "xf", "tg", "ws", "out"):
        assert call(**{name: None}) == -22 and b"dfl_prefill_logprobs: null" in h.dfl_last_error(), name
    for kw in (dict(V=4200), dict(K=96), dict(K=0), dict(rows=0), dict(nsplit=0), dict(nsplit=34), dict(ws=8)):
        assert call(**kw) == -22 and b"dfl_prefill_logprobs" in h.dfl_last_error(), kw
    assert call(nsplit=34) == -22 and b"nsplit=34 outside 1..33" in h.dfl_last_error()     # 4208 columns: 33 blocks


def test_keyword_refusals():
    from dflash_amd import ops
    from dflash_amd.generate import DecodeSession, check_prompt_logprobs
    from dflash_amd.target import NativeTarget
    assert [ops.check_prompt_logprobs(v) for v in (None, False, 0, True)] == [False, False, False, True]
    for n in (1, 2, 5):                                                     # top-N per prompt position: not built
        with pytest.raises(NotImplementedError, match="prompt_logprobs"):
            ops.check_prompt_logprobs(n)
    with pytest.raises(ValueError, match="prompt_logprobs"):
        ops.check_prompt_logprobs("yes")
    wrapped = types.SimpleNamespace()                                       # any target that is no NativeTarget
    assert check_prompt_logprobs(False, wrapped) is False
    with pytest.raises(ValueError, match="prompt_logprobs needs a dflash_amd.NativeTarget"):
        check_prompt_logprobs(True, wrapped)
    with pytest.raises(ValueError, match="prompt_logprobs needs a dflash_amd.NativeTarget"):   # before anything else runs
        DecodeSession(None, wrapped, None, mask_token_id=0, max_new_tokens=1, max_block_size=16, stop_token_ids=None,
                      temperature=0.0, prompt_logprobs=True)
    nt = NativeTarget.__new__(NativeTarget)                                 # prefill="hf" / widths the kernels do not take
    nt.native_prefill = False
    ids, cache = torch.zeros(1, 4, dtype=torch.int64), types.SimpleNamespace(max_rows=8)
    with pytest.raises(ValueError, match="prompt_logprobs needs the native prefill"):
        nt.prefill(ids, cache, prompt_logprobs=True)
    with pytest.raises(NotImplementedError, match="top-N"):
        nt.prefill(ids, cache, prompt_logprobs=3)
    with pytest.raises(ValueError, match="rows >= 1"):                      # ops validates before the device is touched
        ops.prefill_logprobs(None, None, 0, 4208, 256, None)


def test_one_token_prompt_gives_an_empty_result(monkeypatch):
    """P == 1: no row has a successor — an empty fp32 tensor and no launch."""
    from dflash_amd import ops
    from dflash_amd.target import NativeTarget
    nt = NativeTarget.__new__(NativeTarget)
    nt._dev = torch.device("cpu")
    for name in ("prefill_norm_pack", "prefill_logprobs"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("launched for a one-token prompt"))
    out = nt._prompt_logprobs(types.SimpleNamespace(), torch.zeros(1, 1, dtype=torch.int64), None, None)
    assert out.prompt_logprobs.shape == (0,) and out.prompt_logprobs.dtype == torch.float32
