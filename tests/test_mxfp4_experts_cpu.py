"""MXFP4 expert weights without a GPU ("The experts"): configurations, ABI refusals, the packer."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

U8 = torch.uint8


def _cfg(**kw):
    base = dict(num_attention_heads=4, head_dim=128, hidden_size=512, intermediate_size=1024, num_experts=16,
                moe_intermediate_size=256, num_experts_per_tok=4)
    return SimpleNamespace(**{**base, **kw})


def test_check_config_takes_mxfp4_experts_and_refuses_three_ways():
    from dflash_amd import NativeTarget
    from dflash_amd.model import EXPERT_FORMATS
    assert EXPERT_FORMATS == ("bf16", "fp8_e4m3", "mxfp4")
    NativeTarget.check_config(_cfg(), "bf16", "mxfp4")
    for bad in (dict(num_experts=0), dict(hidden_size=576), dict(moe_intermediate_size=192)):
        with pytest.raises(NotImplementedError, match="mxfp4"):
            NativeTarget.check_config(_cfg(**bad), "bf16", "mxfp4")
    with pytest.raises(ValueError, match="weight_format"):       # the dense target has no 4-bit form
        NativeTarget.check_config(_cfg(), "mxfp4", "bf16")
    with pytest.raises(ValueError, match="expert_format"):
        NativeTarget.check_config(_cfg(), "bf16", "mxfp3")
    with pytest.raises(NotImplementedError, match="mxfp4"):      # the constructor checks before it touches the device
        NativeTarget(SimpleNamespace(config=_cfg(num_experts=0)), expert_format="mxfp4")


GU = ("dfl_moe_gate_up", lambda w, I=64, K=2048: (w, 16, 4, I, K, 16, 16, 16, None, -1, None))
DOWN = ("dfl_moe_down", lambda w, stride=2048 * 128 // 2, I=128: (w, stride, 16, 16 * I, 16, 16, 16, 4, 2048, I, 1, 16, None))
REFUSALS = [(GU, dict(scale=None), {}, b"format 3"), (GU, dict(scale=4096 + 32), {}, b"64-byte"), (GU, {}, dict(K=2112), b"128"),
            (GU, {}, dict(K=2176), b"2048"), (DOWN, dict(scale=None), {}, b"format 3"), (DOWN, dict(scale=4096 + 4), {}, b"64-byte"),
            (DOWN, {}, dict(I=192), b"128"), (DOWN, {}, dict(stride=2048 * 128 // 2 - 16), b"stride")]


@pytest.mark.parametrize("entry,wkw,akw,word", REFUSALS)
def test_abi_refuses_bad_mxfp4_expert_launches(entry, wkw, akw, word):
    """-22, the entry point's name and the reason in dfl_last_error, with garbage pointers: nothing is dereferenced or launched."""
    from dflash_amd import _lib
    h = _lib.lib()
    name, args = entry
    w = _lib.Weight(4096, wkw.get("scale", 8192), _lib.W_MXFP4)
    assert getattr(h, name)(*args(C.byref(w), **akw)) == -22
    err = h.dfl_last_error()
    assert (name + ":").encode() in err and word in err, err


@pytest.mark.parametrize("gateup", [True, False])
def test_pack_experts_mxfp4_is_the_dense_packer_per_expert(gateup):
    """Expert e's row of codes / scales is the code / scale region of the dense packer's buffer for that expert alone."""
    from dflash_amd import ops
    E, N, K = 3, 64, 256
    g = torch.Generator().manual_seed(7)
    codes, scales = torch.randint(0, 256, (E, N, K // 2), generator=g).to(U8), torch.randint(100, 140, (E, N, K // 32), generator=g).to(U8)
    x4 = ops.pack_experts_mxfp4(codes, scales, gateup=gateup)
    assert (x4.E, x4.N, x4.K) == (E, N, K) and x4.wp.shape == (E, N * K // 2) and x4.sc.shape == (E, N * K // 32)
    for e in range(E):
        one = (ops.pack_weight_gateup_mxfp4(codes[e, :N // 2], scales[e, :N // 2], codes[e, N // 2:], scales[e, N // 2:]) if gateup
               else ops.pack_weight_mxfp4(codes[e], scales[e]))
        assert torch.equal(x4.wp[e], one.data[:N * K // 2]) and torch.equal(x4.sc[e], one.data[N * K // 2:])
    with pytest.raises(ValueError, match="pack_experts_mxfp4"):
        ops.pack_experts_mxfp4(codes, scales[:, :, :-1], gateup=gateup)
