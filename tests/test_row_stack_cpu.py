"""RowStack's layer sequence and the hand-offs between its launches on the CPU: the ops wrappers the stack calls are
replaced by recorders, the buffers are CPU tensors, and the recorded sequence is compared with the one written out by
hand from the two layer loops the stack replaced (DFlashDraftModel.draft_block, NativeTarget.verify).  Also
ops.row_layers, the format choice of this path."""
import pytest
import torch

from dflash_amd import ops, row_stack
from dflash_amd.model import DFlashDraftModel
from dflash_amd.row_stack import RowStack

HID, QD, KVD, I, NQKV, NQ, NKV, SPLITS = 32, 48, 16, 64, 80, 3, 1, 4
BF16 = torch.bfloat16
GEMMS = ("gemm_resid", "gemm_silu_mul", "attn_head", "attn_head_oproj")


class Rec:
    """Recorders under the names of the ops wrappers; every event keeps a snapshot of the tap rows at its launch."""

    def __init__(self, mp, taps=None):
        self.ev, self.taps = [], taps
        mp.setattr(row_stack.ops, "rows_normed", lambda *a: ("normed",) + a)
        mp.setattr(row_stack.ops, "rows_frag", lambda frag: ("frag", frag))
        mp.setattr(row_stack.ops, "attn_head_ws", lambda *a: ("head_ws",) + a)
        for name in GEMMS:
            mp.setattr(row_stack.ops, name, lambda *a, _n=name, **kw: self.add(_n, *a, **kw))

    def add(self, name, *a, **kw):
        if kw.get("tap") is not None:   # what the down_proj launch does to its tap: new rows, different at every launch
            kw["tap"].fill_(float(len(self.ev) + 1))
        self.ev.append((name, a, kw, None if self.taps is None else self.taps.clone()))

    def attend(self, i, lw, x1):
        self.add("attend", i, lw, x1)

    def moe(self, *a):
        self.add("moe", *a)
        return ["xn1.0", "xn1.1"]

    def names(self):
        return [e[0] for e in self.ev]

    def of(self, name):
        return [e for e in self.ev if e[0] == name]


class Event:
    def __init__(self, rec, tag):
        self.rec, self.tag = rec, tag

    def record(self):
        self.rec.add(self.tag)


def _stack(n_layers=3, q_dim=QD):
    return RowStack(H=HID, q_dim=q_dim, kv_dim=KVD, I=I, nqkv=NQKV, n_q=NQ, n_kv=NKV, eps=1e-6, max_splits=SPLITS,
                    device="cpu", ln1=[f"ln1.{i}" for i in range(n_layers)], ln2=[f"ln2.{i}" for i in range(n_layers)],
                    norm="norm.final")


def _layers(kinds):
    return [dict(ln1=f"ln1.{i}", ln2=f"ln2.{i}", qkv=f"qkv.{i}", o=f"o.{i}", q_norm=f"qn.{i}", k_norm=f"kn.{i}",
                 **(dict(gu_e=f"gu_e.{i}") if k == "moe" else dict(gu=f"gu.{i}", down=f"down.{i}")))
            for i, k in enumerate(kinds)]


def _tiles(bs, dyn):
    return [(t, dyn[8 * t:8 * t + 8]) for t in range((bs + 15) // 16)]


def _attn(**over):
    """The target's form: causal, no context rows."""
    kc, vc = [f"k.{i}" for i in range(3)], [f"v.{i}" for i in range(3)]
    return dict(dict(cos_tab="cos", sin_tab="sin", kcache=kc, vcache=vc, causal=True, S=40, tau=0, pos0=40, dyn=None), **over)


def _same_view(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride()


def _attn_kw(st, i, bs, attn):
    """What every attention launch of layer i takes, whichever form it is."""
    return dict(xq=st.xq, q_col=0, k_col=QD, v_col=QD + KVD, n_q=NQ, n_kv=NKV, q_norm_w=f"qn.{i}", k_norm_w=f"kn.{i}",
                eps=1e-6, cos_tab=attn["cos_tab"], sin_tab=attn["sin_tab"], kcache=attn["kcache"][i],
                vcache=attn["vcache"][i], scale=128 ** -0.5, causal=attn["causal"], S=attn["S"], tau=attn["tau"], bs=bs,
                pos0=attn["pos0"], ws=st.head_ws, max_splits=SPLITS, dyn=attn["dyn"])


def _kw_equal(got, want):
    """Keyword arguments: the same keys, tensors by identity of the view, everything else by value."""
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    for k, w in want.items():
        g = got[k]
        assert (_same_view(g, w) if isinstance(w, torch.Tensor) else g == w), k


def test_dense_moe_dense_with_a_repeated_tap(monkeypatch):
    taps = torch.zeros(32, 3 * HID, dtype=BF16)
    rec = Rec(monkeypatch, taps)
    st = _stack()
    dyn = torch.zeros(16, dtype=torch.int32)
    L, tiles, attn = _layers(["dense", "moe", "dense"]), _tiles(12, dyn), _attn()
    out = st.run(L, tiles, attn=attn, bs=12, taps=taps, tap_layers=[0, 0, 1], moe=rec.moe)
    dense = ["gemm_resid", "attn_head", "gemm_resid", "gemm_silu_mul", "gemm_resid"]
    assert rec.names() == dense + dense[:3] + ["moe"] + dense
    s, ev, dt = st.src, rec.ev, tiles[0][1]
    assert out == s["final"][:1]

    def gemm(e, a, **kw):
        assert e[1][:len(a) - 1] == a[:-1] and _same_view(e[1][len(a) - 1], a[-1])   # (the destination comes last)
        _kw_equal(e[2], kw)

    # layer 0 (dense, tapped into slots 0 and 1)
    gemm(ev[0], ("qkv.0", s["ln1"][0][0], NQKV, HID, st.xq), add_residual=False, dyn=dt)
    assert ev[1][1] == ()
    _kw_equal(ev[1][2], dict(_attn_kw(st, 0, 12, attn), out_frag=st.attn, q_tiles=1, out_tile_stride=st.attn.stride(0)))
    gemm(ev[2], ("o.0", s["attn"][0], HID, QD, st.h[:16]), add_residual=True, ss_out=st.ss_h[0], dyn=dt)
    assert ev[3][1][:4] == ("gu.0", s["ln2"][0][0], I, HID) and _same_view(ev[3][1][4], st.act[0]) and ev[3][1][5] is dt
    assert ev[3][2] == {}
    gemm(ev[4], ("down.0", s["act"][0], HID, I, st.h[:16]), add_residual=True, ss_out=st.ss_h[0], tap=taps[:16, :HID],
         dyn=dt)
    # slot 1 receives its copy of slot 0 right behind layer 0's down_proj, before layer 1 launches anything
    after = ev[5][3]
    assert float(after[0, 0]) == 5.0 and torch.equal(after[:, HID:2 * HID], after[:, :HID]) and not after[:, 2 * HID:].any()
    # layer 1 (MoE): o_proj leaves no sums of squares, the callback gets the layer, the tiles, the h tiles, taps, slot 2
    gemm(ev[5], ("qkv.1", s["ln1"][1][0], NQKV, HID, st.xq), add_residual=False, dyn=dt)
    gemm(ev[7], ("o.1", s["attn"][0], HID, QD, st.h[:16]), add_residual=True, ss_out=None, dyn=dt)
    moe = ev[8][1]
    assert moe[0] == 1 and moe[1] is L[1] and moe[2] is tiles and moe[3] is st.h_tiles and moe[4] is taps and moe[5] == [2]
    # layer 2 (dense, not tapped) reads what the MoE layer returned
    gemm(ev[9], ("qkv.2", "xn1.0", NQKV, HID, st.xq), add_residual=False, dyn=dt)
    _kw_equal(ev[10][2], dict(_attn_kw(st, 2, 12, attn), out_frag=st.attn, q_tiles=1, out_tile_stride=st.attn.stride(0)))
    gemm(ev[11], ("o.2", s["attn"][0], HID, QD, st.h[:16]), add_residual=True, ss_out=st.ss_h[0], dyn=dt)
    assert ev[12][1][:4] == ("gu.2", s["ln2"][2][0], I, HID)
    gemm(ev[13], ("down.2", s["act"][0], HID, I, st.h[:16]), add_residual=True, ss_out=st.ss_h[0], tap=None, dyn=dt)

    # the same stack ending on an MoE layer returns the callback's sources
    rec.ev.clear()
    assert st.run(L[:2], tiles, attn=attn, bs=12, moe=rec.moe) == ["xn1.0"]
    assert rec.names() == dense + dense[:3] + ["moe"]


def test_two_tiles(monkeypatch):
    rec = Rec(monkeypatch)
    st = _stack()
    dyn = torch.arange(16, dtype=torch.int32)
    L, tiles, attn = _layers(["dense", "dense"]), _tiles(20, dyn), _attn()
    assert len(tiles) == 2
    out = st.run(L, tiles, attn=attn, bs=20)
    layer = ["gemm_resid"] * 2 + ["attn_head"] + ["gemm_resid"] * 2 + ["gemm_silu_mul"] * 2 + ["gemm_resid"] * 2
    assert rec.names() == layer * 2 and out == st.src["final"]
    s = st.src
    for i in range(2):
        ev = rec.ev[9 * i:9 * i + 9]
        for t in range(2):
            dt, ht = tiles[t][1], st.h[16 * t:16 * t + 16]
            assert ev[t][1][:4] == (f"qkv.{i}", s["ln1"][i][t], NQKV, HID) and _same_view(ev[t][1][4], st.xq[16 * t:])
            assert ev[t][2]["dyn"] is dt
            assert ev[3 + t][1][:4] == (f"o.{i}", s["attn"][t], HID, QD) and _same_view(ev[3 + t][1][4], ht)
            assert _same_view(ev[3 + t][2]["ss_out"], st.ss_h[t]) and ev[3 + t][2]["dyn"] is dt
            assert ev[5 + t][1][:4] == (f"gu.{i}", s["ln2"][i][t], I, HID) and _same_view(ev[5 + t][1][4], st.act[t])
            assert ev[5 + t][1][5] is dt
            assert ev[7 + t][1][:4] == (f"down.{i}", s["act"][t], HID, I) and _same_view(ev[7 + t][1][4], ht)
            assert _same_view(ev[7 + t][2]["ss_out"], st.ss_h[t]) and ev[7 + t][2]["dyn"] is dt and ev[7 + t][2]["tap"] is None
        _kw_equal(ev[2][2], dict(_attn_kw(st, i, 20, attn), out_frag=st.attn, q_tiles=2, out_tile_stride=st.attn.stride(0)))


def test_attend_replaces_qkv_and_attention(monkeypatch):
    rec = Rec(monkeypatch)
    st = _stack()
    L, tiles = _layers(["dense", "dense"]), _tiles(16, torch.zeros(16, dtype=torch.int32))
    st.run(L, tiles, attn=_attn(), bs=16, fuse_oproj=True, attend=rec.attend)   # (fuse_oproj has no say over a callback)
    layer = ["attend", "gemm_resid", "gemm_silu_mul", "gemm_resid"]
    assert rec.names() == layer * 2
    assert [e[1] for e in rec.of("attend")] == [(i, L[i], st.src["ln1"][i]) for i in range(2)]
    assert [e[1][0] for e in rec.of("gemm_resid")] == ["o.0", "down.0", "o.1", "down.1"]


def test_fuse_oproj(monkeypatch):
    rec = Rec(monkeypatch)
    st = _stack()
    dyn = torch.zeros(16, dtype=torch.int32)
    L, attn = _layers(["dense", "dense"]), _attn()
    st.run(L, _tiles(16, dyn), attn=attn, bs=16, fuse_oproj=True)
    assert rec.names() == ["gemm_resid", "attn_head_oproj", "gemm_silu_mul", "gemm_resid"] * 2
    for i, e in enumerate(rec.of("attn_head_oproj")):
        assert e[1] == ()
        _kw_equal(e[2], dict(_attn_kw(st, i, 16, attn), attn_frag=st.attn[0], wo=f"o.{i}", H=HID, h_io=st.h[:16],
                             ss_out=st.ss_h[0], sync=st.sync))
    assert [e[1][0] for e in rec.of("gemm_resid")] == ["qkv.0", "down.0", "qkv.1", "down.1"]   # no o_proj launch
    # two tiles: the two launches
    rec.ev.clear()
    st.run(L, _tiles(20, dyn), attn=attn, bs=20, fuse_oproj=True)
    assert rec.of("attn_head_oproj") == [] and len(rec.of("attn_head")) == 2
    assert [e[1][0] for e in rec.of("gemm_resid")][:5] == ["qkv.0", "qkv.0", "o.0", "o.0", "down.0"]
    # q_dim beyond the fused launch's range: the two launches
    rec.ev.clear()
    wide = _stack(q_dim=4096 + 128)
    wide.run(L, _tiles(16, dyn), attn=attn, bs=16, fuse_oproj=True)
    assert rec.names() == ["gemm_resid", "attn_head", "gemm_resid", "gemm_silu_mul", "gemm_resid"] * 2


def test_draft_attention_arguments(monkeypatch):
    rec = Rec(monkeypatch)
    st = _stack()
    dyn = torch.zeros(16, dtype=torch.int32)
    xc = torch.zeros(16, 3 * 2 * KVD, dtype=BF16)
    attn = _attn(causal=False, S=7, tau=5, pos0=12, dyn=dyn[:8], xc=xc)
    st.run(_layers(["dense"] * 3), _tiles(16, dyn), attn=attn, bs=16)
    for i, e in enumerate(rec.of("attn_head")):
        _kw_equal(e[2], dict(_attn_kw(st, i, 16, attn), xc=xc, ck_col=i * 2 * KVD, cv_col=i * 2 * KVD + KVD,
                             out_frag=st.attn, q_tiles=1, out_tile_stride=st.attn.stride(0)))
        assert e[2]["causal"] is False and (e[2]["S"], e[2]["tau"], e[2]["pos0"]) == (7, 5, 12) and e[2]["dyn"] is attn["dyn"]
    # no context rows (xc None): the launch takes its defaults
    rec.ev.clear()
    st.run(_layers(["dense"]), _tiles(16, dyn), attn=_attn(causal=False, xc=None), bs=16)
    assert not {"xc", "ck_col", "cv_col"} & rec.of("attn_head")[0][2].keys()


def test_gu_events_bracket_one_layers_gate_up(monkeypatch):
    rec = Rec(monkeypatch)
    st = _stack()
    st.run(_layers(["dense"] * 3), _tiles(20, torch.zeros(16, dtype=torch.int32)), attn=_attn(), bs=20,
           gu_events=(1, Event(rec, "e0"), Event(rec, "e1")))
    names = rec.names()
    assert names.count("e0") == 1 and names.count("e1") == 1
    j = names.index("e0")
    assert names[j:j + 4] == ["e0", "gemm_silu_mul", "gemm_silu_mul", "e1"]
    assert [e[1][0] for e in rec.ev[j + 1:j + 3]] == ["gu.1", "gu.1"]


def test_tap_of_the_last_layer_is_refused(monkeypatch):
    rec = Rec(monkeypatch)
    st = _stack()
    with pytest.raises(NotImplementedError):
        st.run(_layers(["dense", "moe", "dense"]), _tiles(16, torch.zeros(16, dtype=torch.int32)), attn=_attn(), bs=16,
               taps=torch.zeros(32, HID, dtype=BF16), tap_layers=[2], moe=rec.moe)
    assert rec.ev == []


def test_buffers_and_source_table(monkeypatch):
    Rec(monkeypatch)
    st = _stack()
    assert st.h.shape == (32, HID) and st.xq.shape == (32, NQKV) and st.h.dtype == st.xq.dtype == BF16
    assert st.attn.shape == (2, 16 * QD) and st.act.shape == (2, 16 * I) and st.attn.dtype == st.act.dtype == BF16
    assert st.ss_emb.shape == (32,) and st.ss_h.shape == (2, HID) and st.ss_emb.dtype == st.ss_h.dtype == torch.float32
    assert st.head_ws == ("head_ws", NQ, SPLITS, 2, "cpu")
    assert st.sync.dtype == torch.int32 and st.sync.numel() == ops.ATTN_OPROJ_SYNC_WORDS and not st.sync.any()
    s = st.src
    assert [len(s[k]) for k in ("ln1", "ln2", "final", "attn", "act")] == [3, 3, 2, 2, 2]

    def normed(src, ss, nss, w):
        tag, rows, ss_, nss_, w_, eps, word = src
        assert tag == "normed" and _same_view(rows, st.h[16 * t:16 * t + 16]) and _same_view(ss_, ss)
        assert (nss_, w_, eps, word) == (nss, w, 1e-6, ops.DYN_BS)

    for t in range(2):
        normed(s["ln1"][0][t], st.ss_emb[16 * t:], 1, "ln1.0")   # layer 0 reads the embedding's sums of squares
        for i in (1, 2):
            normed(s["ln1"][i][t], st.ss_h[t], HID // 16, f"ln1.{i}")
        for i in range(3):
            normed(s["ln2"][i][t], st.ss_h[t], HID // 16, f"ln2.{i}")
        normed(s["final"][t], st.ss_h[t], HID // 16, "norm.final")
        assert s["attn"][t][0] == "frag" and _same_view(s["attn"][t][1], st.attn[t])
        assert s["act"][t][0] == "frag" and _same_view(s["act"][t][1], st.act[t])


def test_raise_if_failed_reads_and_clears_the_fail_word(monkeypatch):
    Rec(monkeypatch)
    st = _stack()
    st.raise_if_failed()
    st.sync[ops.ATTN_OPROJ_FAIL_WORD] = 1
    with pytest.raises(RuntimeError, match="gave up waiting"):
        st.raise_if_failed()
    assert not st.sync.any()


def test_row_layers_forms_and_cache():
    layers = _layers(["dense", "moe", "dense"])
    layers8 = [dict(qkv=f"qkv8.{i}", o=f"o8.{i}", gu=f"gu8.{i}", down=f"down8.{i}") for i in range(3)]
    gu13 = ["gu13.0", None, None]
    cache = {}
    # bf16: gate/up replaced where a 13-bit twin exists, every other dict — the MoE layer's too — passes through
    plain = ops.row_layers(layers, None, gu13, False, cache)
    assert plain[0] == dict(layers[0], gu="gu13.0") and plain[0] is not layers[0] and layers[0]["gu"] == "gu.0"
    assert plain[1] is layers[1] and plain[2] is layers[2]
    # e4m3: exactly the four matrices
    dense = [layers[0], layers[2]]
    codes = ops.row_layers(dense, [layers8[0], layers8[2]], [gu13[0], gu13[2]], True, cache)
    for lw, l8, got in zip(dense, (layers8[0], layers8[2]), codes):
        assert got == dict(lw, **l8) and {k for k in got if got[k] != lw[k]} == {"qkv", "o", "gu", "down"}
    # one list per form, built once
    assert ops.row_layers(layers, None, gu13, False, cache) is plain and ops.row_layers(dense, None, None, True, cache) is codes
    assert sorted(cache) == [False, True]


def test_model_row_layers_follows_streams_fp8_and_a_reload_clears_it():
    m = object.__new__(DFlashDraftModel)   # (no device: only what row_layers reads)
    L = _layers(["dense", "dense"])
    m.w = {"layers": L}
    m.w8 = {"layers": [dict(qkv=f"qkv8.{i}", o=f"o8.{i}", gu=f"gu8.{i}", down=f"down8.{i}") for i in range(2)]}
    m.gu13, m._row_layers = [None, None], {}
    m.fp8_stream, m.attn_impl, m.fuse_oproj, m.wide_hidden = True, "head", False, False
    codes = m.row_layers(16)
    assert codes[1]["down"] == "down8.1" and codes[1]["ln2"] == "ln2.1" and m.row_layers(9) is codes
    plain = m.row_layers(17)   # two tiles: the bf16 kernels on the dequantised copy
    assert plain == L and m.row_layers(16) is codes
    m.fp8_stream = False       # flipped at run time: the form is chosen per call
    assert m.row_layers(16) is plain
    # a reload (load_state_dict) hands in new dicts and an empty cache: the lists are built anew from them
    m.w, m._row_layers = {"layers": _layers(["dense"])}, {}
    assert m.row_layers(17) == m.w["layers"] and len(m.row_layers(17)) == 1 and m.row_layers(17) is not plain
