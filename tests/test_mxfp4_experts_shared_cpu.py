"""dfl_moe_grouped_gate_up / dfl_moe_grouped_down with a DFL_W_MXFP4 descriptor (csrc/moe_w4_shared.hip): every refusal
through the C ABI — DFL_EINVAL, the entry point's own name in dfl_last_error, nothing launched (the pointers are
fakes) — and ops.moe_grouped_* on an Mxfp4Experts of the wrong E x N x K.  No GPU."""
import pytest
import torch

GU = dict(scale=4096, stride=64 * 256, xg=16, items=16, n_items=16, max_items=4, I=64, K=256, act_g=16, rpi=64, src_row=16,
          zeros=16)
DOWN = dict(scale=4096, stride=128 * 128, act_g=16, items=16, n_items=16, max_items=4, H=256, I=128, row_w=16, out32=16, rpi=128)

GU_CASES = [("scale-null", dict(scale=None), b"format 3"), ("scale-misaligned", dict(scale=4096 + 32), b"64-byte"),
            ("K-192", dict(K=192, stride=64 * 192), b"% 128"), ("N-not-16", dict(I=60, stride=60 * 256), b"% 16"),
            ("I-not-32", dict(I=48, stride=48 * 256), b"% 32"), ("stride-bf16", dict(stride=2 * 64 * 256), b"stride"),
            ("rows-per-item-32", dict(rpi=32), b"rows_per_item"), ("src_row-alone", dict(zeros=None), b"zeros_1k"),
            ("zeros-alone", dict(src_row=None), b"zeros_1k"), ("xg-null", dict(xg=None), b"null"),
            ("items-null", dict(items=None), b"null"), ("n_items-null", dict(n_items=None), b"null"),
            ("act_g-null", dict(act_g=None), b"null")]
DOWN_CASES = [("scale-null", dict(scale=None), b"format 3"), ("scale-misaligned", dict(scale=4096 + 16), b"64-byte"),
              ("I-192", dict(I=192, stride=128 * 192), b"% 128"), ("N-not-16", dict(H=248, stride=124 * 128), b"% 16"),
              ("stride-bf16", dict(stride=256 * 128), b"stride"), ("rows-per-item-0", dict(rpi=0), b"rows_per_item"),
              ("act_g-null", dict(act_g=None), b"null"), ("items-null", dict(items=None), b"null"),
              ("row_w-null", dict(row_w=None), b"null"), ("out32-null", dict(out32=None), b"null")]


def _refused(name, args, word):
    from dflash_amd import _lib
    h = _lib.lib()
    assert getattr(h, name)(*args) == -22, name
    err = h.dfl_last_error()
    assert (name + ":").encode() in err and word in err, err


@pytest.mark.parametrize("change,word", [c[1:] for c in GU_CASES], ids=[c[0] for c in GU_CASES])
def test_grouped_gate_up_refuses(change, word):
    from dflash_amd import _lib
    a = {**GU, **change}
    _refused("dfl_moe_grouped_gate_up", (_lib.Weight(4096, a["scale"], _lib.W_MXFP4), a["stride"], a["xg"], a["items"], a["n_items"],
                                         a["max_items"], a["I"], a["K"], a["act_g"], a["rpi"], a["src_row"], a["zeros"], None), word)


@pytest.mark.parametrize("change,word", [c[1:] for c in DOWN_CASES], ids=[c[0] for c in DOWN_CASES])
def test_grouped_down_refuses(change, word):
    from dflash_amd import _lib
    a = {**DOWN, **change}
    _refused("dfl_moe_grouped_down", (_lib.Weight(4096, a["scale"], _lib.W_MXFP4), a["stride"], a["act_g"], a["items"], a["n_items"],
                                      a["max_items"], a["H"], a["I"], a["row_w"], a["out32"], a["rpi"], None), word)


def test_grouped_ops_refuse_mismatched_mxfp4_experts():
    """An Mxfp4Experts whose E x N x K is not the launch's: ValueError in front of any launch (CPU tensors suffice)."""
    from dflash_amd import ops
    x4 = ops.Mxfp4Experts(torch.zeros(6, 128 * 128 // 2, dtype=torch.uint8), torch.zeros(6, 128 * 128 // 32, dtype=torch.uint8),
                          6, 128, 128)
    sc = dict(E=6, I=128)
    with pytest.raises(ValueError, match="mxfp4 experts"):
        ops.moe_grouped_gate_up(x4, torch.zeros(16, dtype=torch.bfloat16), sc, 128, gather=True)     # N = 2 I = 256 asked
    with pytest.raises(ValueError, match="mxfp4 experts"):
        ops.moe_grouped_down(x4, sc, 256)                                                            # N = 256 asked
    with pytest.raises(ValueError, match="mxfp4 experts"):
        ops.moe_grouped_down(x4, dict(E=8, I=128), 128)                                              # E = 8 asked
