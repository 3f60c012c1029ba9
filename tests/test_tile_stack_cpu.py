"""TileStack's protocol between launches (pending sums, pending tap, repeated tap ids) on the CPU: the ops wrappers the
stack calls are replaced by recorders, the buffers are CPU tensors, and the recorded sequence is compared with the one
written out by hand from the layer loops the stack replaced."""
import pytest
import torch

from dflash_amd import tile_stack
from dflash_amd.tile_stack import TileStack

HID, QD, I, NQKV, MT, R = 32, 48, 64, 80, 2, 2
BF16 = torch.bfloat16


class Rec:
    """Recorders under the names of the ops wrappers; every event keeps a snapshot of the tap rows at its launch."""

    def __init__(self, mp, taps=None):
        self.ev, self.taps = [], taps
        mp.setattr(tile_stack.ops, "batch_ksplit", lambda K: 2)
        mp.setattr(tile_stack.ops, "brows_frag", lambda frag: ("src", frag))
        for name in ("norm_frag_batch", "gemm_f32_batch", "gemm_resid_batch", "gemm_silu_mul_batch"):
            mp.setattr(tile_stack.ops, name, lambda *a, _n=name, **kw: self.add(_n, *a, **kw))

    def add(self, name, *a, **kw):
        if kw.get("tap") is not None:   # what the norm launch does to its tap: new rows, different at every launch
            kw["tap"].fill_(float(len(self.ev) + 1))
        self.ev.append((name, a, kw, None if self.taps is None else self.taps.clone()))

    def attend(self, i, lw):
        self.add("attend", i, lw)

    def moe(self, *a):
        self.add("moe", *a)
        return 2

    def names(self):
        return [e[0] for e in self.ev]

    def norms(self):
        return [(j, e) for j, e in enumerate(self.ev) if e[0] == "norm_frag_batch"]


def _stack(part_qkv=False):
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt)  # noqa: E731
    return TileStack(H=HID, q_dim=QD, I=I, nqkv=NQKV, eps=1e-6, MT=MT, gws=torch.zeros(8, dtype=torch.uint8),
                     h=z(MT, 16, HID), attn=z(MT, 16 * QD), act=z(MT, 16 * I), xq=z(MT, 16, NQKV), part_qkv=part_qkv)


def _layers(kinds):
    return [dict(ln1=f"ln1.{i}", ln2=f"ln2.{i}", qkv=f"qkv.{i}", o=f"o.{i}",
                 **(dict(gu_e=f"gu_e.{i}") if k == "moe" else dict(gu=f"gu.{i}", down=f"down.{i}")))
            for i, k in enumerate(kinds)]


def _same_view(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def _norm_args(e):
    """(weight, part, K, nsplit, tap) of a recorded norm launch."""
    _, a, kw, _ = e
    return a[2], kw.get("part"), kw.get("K", 0), kw.get("nsplit"), kw.get("tap")


def test_dense_moe_dense_with_a_repeated_tap(monkeypatch):
    taps = torch.zeros(MT, 16, 3 * HID, dtype=BF16)
    rec = Rec(monkeypatch, taps)
    st = _stack()
    dyn = torch.zeros(MT, 8, dtype=torch.int32)
    L = _layers(["dense", "moe", "dense"])
    st.run(L, R, dyn, rec.attend, qkv="rows", taps=taps, tap_layers=[0, 0, 1], moe=rec.moe)
    st.finish("norm.final")
    dense = ["norm_frag_batch", "gemm_resid_batch", "attend", "gemm_f32_batch", "norm_frag_batch", "gemm_silu_mul_batch",
             "gemm_f32_batch"]
    sparse = dense[:5] + ["moe"]
    assert rec.names() == dense + sparse + dense + ["norm_frag_batch"]
    norms = rec.norms()
    assert [_norm_args(e)[0] for _, e in norms] == ["ln1.0", "ln2.0", "ln1.1", "ln2.1", "ln1.2", "ln2.2", "norm.final"]
    for _, (_, a, kw, _) in norms:   # every norm launch: the stack's rows and tiles, valid rows from the block-size word
        assert a[0] is st.h and a[1] == R and a[4] is st.xn and a[5] is dyn and a[6] == tile_stack.ops.DYN_BS
    slot = lambda j: taps[:, :, j * HID:(j + 1) * HID]  # noqa: E731
    # ln1 of layer 0: nothing waits
    w, part, K, ns, tap = _norm_args(norms[0][1])
    assert part is None and tap is None and not K and ns is None
    # ln1 of layer 1: layer 0's down_proj sums (K parts), layer 0's rows -> slot 0, copied to slot 1 right behind it
    j, e = norms[2]
    w, part, K, ns, tap = _norm_args(e)
    assert part is st.part_h and K == I and ns is None and _same_view(tap, slot(0))
    after = rec.ev[j + 1][3]
    assert torch.equal(after[:, :, HID:2 * HID], after[:, :, :HID]) and float(after[0, 0, 0]) == j + 1
    assert not after[:, :, 2 * HID:].any()
    # ln1 of layer 2: the MoE layer's expert shares, layer 1's rows -> slot 2
    j, e = norms[4]
    w, part, K, ns, tap = _norm_args(e)
    assert part is st.part_h and ns == 2 and _same_view(tap, slot(2))
    assert float(rec.ev[j + 1][3][0, 0, 2 * HID]) == j + 1 and float(rec.ev[j + 1][3][0, 0, 0]) == norms[2][0] + 1
    # finish: the last down_proj's sums, no tap
    w, part, K, ns, tap = _norm_args(norms[6][1])
    assert part is st.part_h and K == I and ns is None and tap is None
    # ln2: always o_proj's sums
    for k in (1, 3, 5):
        w, part, K, ns, tap = _norm_args(norms[k][1])
        assert part is st.part_h and K == QD and ns is None and tap is None
    # attend: once per layer, with the layer's index and weights
    assert [(e[1][0], e[1][1]) for e in rec.ev if e[0] == "attend"] == [(i, L[i]) for i in range(3)]
    # the GEMMs between: operands, widths and destinations
    ev = rec.ev
    assert ev[3][1] == ("o.0", st.src["attn"], R, HID, QD, st.part_h, dyn)
    assert ev[5][1] == ("gu.0", st.src["xn"], R, I, HID, st.act, st.gws, dyn)
    assert ev[6][1] == ("down.0", st.src["act"], R, HID, I, st.part_h, dyn)
    moe = ev[12]
    assert moe[0] == "moe" and moe[1][0] is L[1] and moe[1][1:3] == (R, MT) and moe[1][3] is dyn
    assert moe[1][4] is st.xn and moe[1][5] is st.part_h


def test_tap_of_the_last_layer_is_refused(monkeypatch):
    rec = Rec(monkeypatch)
    st = _stack()
    with pytest.raises(NotImplementedError):
        st.run(_layers(["dense", "moe", "dense"]), R, torch.zeros(MT, 8, dtype=torch.int32), rec.attend, qkv="rows",
               taps=torch.zeros(MT, 16, HID, dtype=BF16), tap_layers=[2], moe=rec.moe)
    assert rec.ev == []


@pytest.mark.parametrize("form", ["rows", "parts"])
def test_qkv_forms(monkeypatch, form):
    rec = Rec(monkeypatch)
    st = _stack(part_qkv=True)
    assert st.part_qkv.dtype == torch.float32 and st.part_qkv.numel() == 2 * MT * 16 * NQKV   # (batch_ksplit = 2 here)
    dyn = torch.zeros(MT, 8, dtype=torch.int32)
    st.run(_layers(["dense"]), R, dyn, rec.attend, qkv=form)
    name, a, kw, _ = rec.ev[1]
    assert rec.names()[:3] == ["norm_frag_batch", "gemm_resid_batch" if form == "rows" else "gemm_f32_batch", "attend"]
    assert a[:5] == ("qkv.0", st.src["xn"], R, NQKV, HID)
    if form == "rows":
        assert a[5] is st.xq and kw == dict(add_residual=False, ws=st.gws, dyn=dyn)
    else:
        assert a[5] is st.part_qkv and a[6] is dyn and kw == {}


def test_buffers_are_adopted_and_sized(monkeypatch):
    Rec(monkeypatch)
    h = torch.zeros(MT, 16, HID, dtype=BF16)
    st = TileStack(H=HID, q_dim=QD, I=I, nqkv=NQKV, eps=1e-6, MT=MT, gws=torch.zeros(8, dtype=torch.uint8), h=h,
                   moe_nsplit=4)
    assert st.h is h and st.part_qkv is None
    assert st.xn.shape == (MT, 16 * HID) and st.attn.shape == (MT, 16 * QD) and st.act.shape == (MT, 16 * I)
    assert st.xq.shape == (MT, 16, NQKV) and st.part_h.numel() == 4 * MT * 16 * HID and st.part_h.dtype == torch.float32
    assert all(st.src[k][1] is b for k, b in (("xn", st.xn), ("attn", st.attn), ("act", st.act)))
