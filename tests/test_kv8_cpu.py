"""e4m3 KV cache, host side: ops.quantize_kv_rows on its edge rows, and the refusals that need no device."""
from types import SimpleNamespace

import pytest
import torch

import helpers as H
from kv8_rows import edge_rows

BF16 = torch.bfloat16


def test_quantize_kv_rows_edges():
    from dflash_amd import ops
    x = edge_rows()
    q, s = ops.quantize_kv_rows(x)
    assert q.dtype == torch.uint8 and q.shape == x.shape and s.shape == (8,) and s.dtype == torch.float32
    assert s[0] == 1.0 and s[1] == 2.0 ** -3 and s[2] == 2.0 and s[3] == 1.0 and s[6] == 2.0 ** -64
    assert torch.equal(torch.log2(s), torch.log2(s).round()) and float(s.min()) >= 2.0 ** -64
    assert abs(float(torch.log2(s[4] / s[7]))) >= 18 and abs(float(torch.log2(s[5] / s[7]))) >= 18
    vals = q.view(torch.float8_e4m3fn).float()
    assert torch.isfinite(vals).all() and float(vals.abs().max()) <= 448.0
    d = ops.dequantize_kv_rows(q, s)
    assert torch.equal(d.double(), vals.double() * s.double()[:, None])            # exact in bf16
    assert float(((d.double() - x.double()).abs() / s.double()[:, None]).max()) <= 16.0   # half an e4m3 step at 448
    q2, s2 = ops.quantize_kv_rows(d)
    assert torch.equal(ops.dequantize_kv_rows(q2, s2), d)                          # a fixed point


def test_kv_format_refusals():
    from dflash_amd import NativeTarget
    from dflash_amd.batch import BatchedDecoder
    from dflash_amd.engine import BatchEngine
    from dflash_amd.synthetic import make_hf_qwen3
    cfg = make_hf_qwen3({**H.TINY_TARGET, "num_layers": 1}, "cpu").config
    NativeTarget.check_config(cfg, kv_format="fp8_e4m3")
    with pytest.raises(ValueError, match="kv_format"):
        NativeTarget.check_config(cfg, kv_format="nope")
    with pytest.raises(NotImplementedError, match="attn_impl='fused'"):
        NativeTarget(SimpleNamespace(config=cfg), attn_impl="fused", kv_format="fp8_e4m3")
    t = SimpleNamespace(kv8=True)
    with pytest.raises(NotImplementedError, match="BatchedDecoder"):
        BatchedDecoder(None, t, 2, 64, 16, 0)
    with pytest.raises(NotImplementedError, match="BatchEngine"):
        BatchEngine(None, t, max_rows=64, out_len=16, mask_token_id=0)
