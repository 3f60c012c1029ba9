"""An MXFP4 native target, the parts that need no GPU ("The target")."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch


def test_requantising_the_dequantised_rows_keeps_every_value():
    """dequantize(quantize(dequantize(quantize(w)))) == dequantize(quantize(w)) bit for bit, though scale codes move: a
    block whose largest code lands on 3 (value 1.5 * 2^e, frexp mantissa 0.75) takes scale 2^(e - 2) the second time."""
    from dflash_amd import ops
    w = (torch.randn(16, 256, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
         * torch.logspace(-3, 3, 16, dtype=torch.float64)[:, None]).to(torch.bfloat16)
    w[3, :32] = 0
    w[5, 32:64] = torch.tensor([5.2, -1.4] + [0.3] * 30)        # scale 1: codes up to 6; again 6
    w[5, 64:96] = torch.tensor([-3.2, 1.0] + [0.7] * 30)        # amax 3.2: scale 1, largest code 3 (3.0): the edge
    q1 = ops.quantize_mxfp4_rows(w)
    d1 = ops.dequantize_mxfp4_rows(*q1)
    q2 = ops.quantize_mxfp4_rows(d1)
    assert torch.equal(ops.dequantize_mxfp4_rows(*q2).view(torch.int16), d1.view(torch.int16))
    assert int(q1[1][5, 2]) == 127 and int(q2[1][5, 2]) == 126 and d1[5, 64].item() == -3.0
    assert int(q1[1][5, 1]) == int(q2[1][5, 1]) == 127
    assert 0 < int((q1[1] != q2[1]).sum()) < q1[1].numel()


def _cfg(**over):
    base = dict(hidden_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128, intermediate_size=2048,
                num_hidden_layers=2, vocab_size=4208, attention_bias=False, mlp_bias=False)
    return SimpleNamespace(**{**base, **over})


REFUSALS = [("unknown format", {}, "mxfp6", ValueError, "weight_format"),
            ("sparse MoE", dict(num_experts=64, num_experts_per_tok=4, moe_intermediate_size=512), "mxfp4",
             NotImplementedError, "expert_format"),
            ("hidden % 128", dict(hidden_size=1088), "mxfp4", NotImplementedError, "% 128"),
            ("intermediate % 128", dict(intermediate_size=2112), "mxfp4", NotImplementedError, "% 128")]


@pytest.mark.parametrize("what,over,fmt,exc,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_check_config_refusals_and_the_same_through_the_constructor(what, over, fmt, exc, word):
    """Before any device work: the constructor is handed a config-only stand-in (no weights, no device)."""
    from dflash_amd import NativeTarget
    NativeTarget.check_config(_cfg(), "mxfp4")
    NativeTarget.check_config(_cfg(**over), "bf16")
    with pytest.raises(exc, match=word):
        NativeTarget.check_config(_cfg(**over), fmt)
    with pytest.raises(exc, match=word):
        NativeTarget(SimpleNamespace(config=_cfg(**over)), weight_format=fmt)


@pytest.mark.parametrize("change,word", [(dict(scale=4096 + 32), b"64-byte aligned"), (dict(K=192), b"128"),
                                         (dict(K=8192), b"4096")])
def test_gemm_sample_refuses_a_bad_mxfp4_descriptor_with_nothing_launched(change, word):
    """Small integers stand for pointers: a launch would fault, a refusal returns -22 under the entry point's name."""
    from dflash_amd import _lib
    h = _lib.lib()
    rows = _lib.Rows()
    rows.frag, rows.mode, rows.valid_word = 16, 0, -1
    a = {**dict(scale=4096 + 64, K=128), **change}
    rc = h.dfl_gemm_sample(_lib.Weight(4096, a["scale"], _lib.W_MXFP4), C.byref(rows), 64, a["K"], 0, 16, None, -1, 16, 16, 0,
                           None, None, 1, C.c_float(1.0), 0, None, 0, 0, 0, None)
    err = h.dfl_last_error()
    assert rc == -22 and b"dfl_gemm_sample:" in err and word in err, (rc, err)
