"""FP8 (e4m3) expert weights of a sparse-MoE native target, the parts that need no GPU ("The
experts"): NativeTarget.check_config with the expert_format keyword, the two expert entry points' declarations and
argument validation, and the quantiser's fixed point on expert-shaped views."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

import helpers as H

BF16 = torch.bfloat16


def _cfg(**over):
    base = dict(hidden_size=1024, num_attention_heads=8, num_key_value_heads=2, head_dim=128, intermediate_size=2048,
                num_hidden_layers=2, vocab_size=4208, attention_bias=False, mlp_bias=False)
    return SimpleNamespace(**{**base, **over})


def _moe(**over):
    return _cfg(**{**dict(num_experts=128, num_experts_per_tok=8, moe_intermediate_size=768), **over})


def test_check_config_with_expert_format():
    """expert_format="fp8_e4m3" is accepted for an MoE config; it refuses, before any device work: an unknown format
    (ValueError), a config without experts and hidden / moe_intermediate widths that are no multiple of 64
    (NotImplementedError).  weight_format="fp8_e4m3" on an MoE config keeps raising as it did."""
    from dflash_amd import NativeTarget
    NativeTarget.check_config(_moe(), "bf16", "bf16")
    NativeTarget.check_config(_moe(), "bf16", "fp8_e4m3")
    NativeTarget.check_config(_moe(), expert_format="fp8_e4m3")
    NativeTarget.check_config(_cfg(), "fp8_e4m3", "bf16")
    for fmt in ("int4", "fp8", "FP8_E4M3", None):
        with pytest.raises(ValueError, match="expert_format"):
            NativeTarget.check_config(_moe(), "bf16", fmt)
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        NativeTarget.check_config(_cfg(), "bf16", "fp8_e4m3")
    for bad in (dict(hidden_size=1056), dict(moe_intermediate_size=800), dict(hidden_size=1056, moe_intermediate_size=96)):
        NativeTarget.check_config(_moe(**bad))
        with pytest.raises(NotImplementedError, match="% 64"):
            NativeTarget.check_config(_moe(**bad), "bf16", "fp8_e4m3")
    # the pinned behaviour, restated: the dense format still refuses an MoE config, whatever the expert format
    for ef in ("bf16", "fp8_e4m3"):
        with pytest.raises(NotImplementedError, match="MoE"):
            NativeTarget.check_config(_moe(), "fp8_e4m3", ef)
    with pytest.raises(NotImplementedError, match="MoE"):
        NativeTarget.check_config(_moe(), "fp8_e4m3")
    # what bf16 refuses, fp8 experts refuse too
    with pytest.raises(NotImplementedError, match="head_dim"):
        NativeTarget.check_config(_moe(head_dim=64), "bf16", "fp8_e4m3")


def test_constructor_refuses_before_any_device_work():
    """A config-only stand-in for the model (no weights, no device): the refusals come out of NativeTarget(...) itself."""
    from dflash_amd import NativeTarget
    with pytest.raises(ValueError, match="expert_format"):
        NativeTarget(SimpleNamespace(config=_moe()), expert_format="e5m2")
    with pytest.raises(NotImplementedError, match="sparse-MoE"):
        NativeTarget(SimpleNamespace(config=_cfg()), expert_format="fp8_e4m3")
    with pytest.raises(NotImplementedError, match="% 64"):
        NativeTarget(SimpleNamespace(config=_moe(moe_intermediate_size=96)), expert_format="fp8_e4m3")
    with pytest.raises(NotImplementedError, match="% 64"):
        NativeTarget(SimpleNamespace(config=_moe(hidden_size=1056)), expert_format="fp8_e4m3")
    with pytest.raises(NotImplementedError, match="MoE"):
        NativeTarget(SimpleNamespace(config=_moe()), weight_format="fp8_e4m3", expert_format="fp8_e4m3")


# ---------------------------------------------------------------------------------------------- the C ABI
def _header_arity(txt, name):
    m = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt)
    assert m, name
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_expert_fp8_entry_points_are_declared_bound_and_exported():
    from dflash_amd import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(H.ROOT, "include", "dflash_hip.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(dfl_[a-z0-9_]+)\s*\(", txt))
    handle = _lib.lib()
    for n in ("dfl_moe_gate_up", "dfl_moe_down"):
        assert n in names and n in _lib.SIGNATURES and isinstance(getattr(handle, n), C._CFuncPtr), n
        assert len(_lib.SIGNATURES[n][1]) == _header_arity(txt, n), n
        # the experts' codes and scales arrive in the weight descriptor: one name per launch
        assert _lib.SIGNATURES[n][1][0] is C.POINTER(_lib.Weight), n
        assert n + "_fp8" not in names and n + "_fp8" not in _lib.SIGNATURES, n
    assert handle.dfl_version() == 1
    assert re.search(r"#define\s+DFL_ABI_VERSION\s+1\b", txt)


def test_expert_fp8_entry_points_validate_without_gpu():
    """Small integers stand for pointers; every call is refused with DFL_EINVAL (-22) and a message with its own name
    before anything launches."""
    from dflash_amd import _lib
    h = _lib.lib()

    def refused(name, *args, text=None):
        assert getattr(h, name)(*args) == -22, (name, args)
        err = h.dfl_last_error()
        assert (name + ":").encode() in err, (name, err)
        if text:
            assert text in err, (name, err)

    def w8(wp, sc):
        return _lib.Weight(wp, sc, _lib.W_E4M3)

    # dfl_moe_gate_up({wp8, wscale, e4m3}, x_frag, E, I, K, act, list, n_active, dyn, valid_word, stream)
    def gu(wp=64, sc=64, x=64, E=8, I=64, K=512, act=64, lst=64, n=64):
        return (w8(wp, sc), x, E, I, K, act, lst, n, None, -1, None)
    refused("dfl_moe_gate_up", *gu(K=96), text=b"multiple of 64")
    refused("dfl_moe_gate_up", *gu(K=1056), text=b"multiple of 64")
    refused("dfl_moe_gate_up", *gu(K=2112), text=b"K <= 2048")
    refused("dfl_moe_gate_up", *gu(K=4096), text=b"K <= 2048")
    refused("dfl_moe_gate_up", *gu(sc=None), text=b"null scale")
    refused("dfl_moe_gate_up", *gu(sc=64 + 4), text=b"64-byte aligned")
    refused("dfl_moe_gate_up", *gu(wp=None), text=b"null")
    refused("dfl_moe_gate_up", *gu(lst=None), text=b"null")
    refused("dfl_moe_gate_up", *gu(I=40))

    # dfl_moe_down({wp8, wscale, e4m3}, stride_bytes, act, act_stride, wt, list, n_active, E, N, I, nsplit, out, stream)
    def dn(wp=64, stride=None, sc=64, act=64, astride=None, E=8, N=64, I=128, nsplit=4, out=64):
        return (w8(wp, sc), N * I if stride is None else stride, act, 16 * I if astride is None else astride, 64, 64, 64, E, N, I,
                nsplit, out, None)
    refused("dfl_moe_down", *dn(I=96), text=b"multiple of 64")
    refused("dfl_moe_down", *dn(I=32), text=b"multiple of 64")
    refused("dfl_moe_down", *dn(sc=None), text=b"null scale")
    refused("dfl_moe_down", *dn(sc=64 + 4), text=b"64-byte aligned")
    refused("dfl_moe_down", *dn(stride=64 * 128 - 16), text=b"strides")     # bytes of codes: shorter than N * I
    refused("dfl_moe_down", *dn(stride=64 * 128 + 8), text=b"strides")      # no whole 16-byte words
    refused("dfl_moe_down", *dn(astride=16 * 128 - 8), text=b"strides")
    refused("dfl_moe_down", *dn(out=None), text=b"null")
    refused("dfl_moe_down", *dn(nsplit=17))
    refused("dfl_moe_down", *dn(N=72))


# ---------------------------------------------------------------------------------------------- the quantiser
@pytest.mark.parametrize("rows,cols", [(4 * 2 * 64, 128), (4 * 128, 64)], ids=["gate_up", "down"])
def test_quantiser_is_a_fixed_point_on_expert_shaped_views(rows, cols):
    """The expert tensors are quantised as flat row views — gate_up_proj [E, 2I, H] as E * 2I rows of H, down_proj
    [E, H, I] as E * H rows of I (E 4, I 64, H 128) — and the model's own tensors are overwritten with q * scale:
    quantising those again (a second target over the same model) must hold the same bf16 values."""
    from dflash_amd import ops
    E = 4
    g = torch.Generator().manual_seed(rows)
    w3 = (torch.randn(E, rows // E, cols, generator=g) * 0.03).to(BF16)
    w3[1, 3] = 0                                                    # an all-zero row: scale 1
    w3[2, 5, 7] = 225.0 * 2.0 ** -10                                # largest code rounds onto 224: the second scale halves
    w3[2, 5, :7] = w3[2, 5, :7].clamp(-0.1, 0.1)
    w3[2, 5, 8:] = w3[2, 5, 8:].clamp(-0.1, 0.1)
    w = w3.view(-1, cols)
    q1, s1 = ops.quantize_fp8_rows(w)
    assert q1.shape == (rows, cols) and s1.shape == (rows,)
    m, _ = torch.frexp(s1)
    assert torch.all(m == 0.5)                                      # powers of two
    d1 = ops.dequantize_fp8_rows(q1, s1)
    q2, s2 = ops.quantize_fp8_rows(d1.view(E, rows // E, cols).view(-1, cols))
    d2 = ops.dequantize_fp8_rows(q2, s2)
    assert torch.equal(d1.view(torch.int16), d2.view(torch.int16))
    q3, s3 = ops.quantize_fp8_rows(d2)
    assert torch.equal(q3, q2) and torch.equal(s3, s2)
