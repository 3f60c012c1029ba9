"""The 13-bit expert gate/up stream (dfl_moe_gate_up on DFL_W_BF16X13, DESIGN.md section 11, "The experts") without a GPU:
what the entry point refuses and what it no longer refuses, and the packer's own account of the expert-tall matrices the
GPU tests stream (tests/bf16x13_expert_cases.py).  Nothing here launches a kernel: every call is refused before that.
(NativeTarget cannot be built without a GPU — its wiring is checked in tests/test_hip_bf16x13_experts.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_bf16x13_cpu import QUAD, bits, decode, to_packed

BF16 = torch.bfloat16


def _gate_up_args(w, K, E=8, I=64):
    # (w, x_frag, E, I, K, act_frag, list, n_active, dyn, valid_word, stream): small integers as pointers, never read
    return (w, 16, E, I, K, 16, 16, 16, None, -1, None)


def _refused(h, name, text, *args):
    assert getattr(h, name)(*args) == -22, name
    err = h.dfl_last_error()
    assert (name + ":").encode() in err and text in err, (name, err)
    return err


def test_moe_gate_up_refuses_what_the_format_does_not_cover():
    from dflash_amd import _lib
    h, W13 = _lib.lib(), _lib.W_BF16X13
    _refused(h, "dfl_moe_gate_up", b"no scale", *_gate_up_args(_lib.Weight(4096, 4096, W13), 2048))
    for K in (512, 1024, 2112):
        _refused(h, "dfl_moe_gate_up", b"K = 2048", *_gate_up_args(_lib.Weight(4096, None, W13), K))
    _refused(h, "dfl_moe_gate_up", b"null", *_gate_up_args(_lib.Weight(None, None, W13), 2048))
    # the scale comes first, then K, then the pointers: each refusal names what it is about
    _refused(h, "dfl_moe_gate_up", b"no scale", *_gate_up_args(_lib.Weight(None, 4096, W13), 512))
    _refused(h, "dfl_moe_gate_up", b"K = 2048", *_gate_up_args(_lib.Weight(None, None, W13), 512))


def test_moe_gate_up_takes_the_format_at_k_2048():
    """Valid-looking arguments at K = 2048 pass the format's checks: what refuses the call is the expert count (E = 0,
    so that nothing is launched on small integers), in the words it has for every format — not "unknown weight format 2",
    which is the answer of a library without the W13 form."""
    from dflash_amd import _lib
    h, W13 = _lib.lib(), _lib.W_BF16X13
    err = _refused(h, "dfl_moe_gate_up", b"outside range", *_gate_up_args(_lib.Weight(4096, None, W13), 2048, E=0))
    assert b"format" not in err, err
    err = _refused(h, "dfl_moe_gate_up", b"outside range", *_gate_up_args(_lib.Weight(4096, None, W13), 2048, I=40))
    assert b"format" not in err, err
    # the same refusal, word for word, as the bf16 form's
    assert _refused(h, "dfl_moe_gate_up", b"outside range", *_gate_up_args(_lib.Weight(4096, None, _lib.W_BF16), 2048, E=0)) == \
        _refused(h, "dfl_moe_gate_up", b"outside range", *_gate_up_args(_lib.Weight(4096, None, W13), 2048, E=0))


def test_the_other_expert_launches_keep_refusing_the_format():
    from dflash_amd import _lib, ops
    h, W13 = _lib.lib(), _lib.W_BF16X13
    # (w, wp_expert_stride, act, act_expert_stride, wt, list, n_active, E, N, I, nsplit, out, stream)
    _refused(h, "dfl_moe_down", b"unknown weight format 2", _lib.Weight(4096, None, W13), 2048 * 64, 16, 16 * 64, 16, 16, 16,
             8, 2048, 64, 4, 16, None)
    # dfl_gemm_silu_mul_experts takes a bare pointer, no descriptor: there is no format to hand it
    assert _lib.SIGNATURES["dfl_gemm_silu_mul_experts"][1][0] is C.c_void_p
    assert _lib.SIGNATURES["dfl_moe_gate_up"][1][0] is C.POINTER(_lib.Weight) and h.dfl_version() == 1
    twin = ops.Bf16x13Weight(torch.zeros(8, dtype=torch.uint8), 16, 2048)
    with pytest.raises((AttributeError, TypeError, AssertionError)):
        ops.gemm_silu_mul_experts(twin, None, 8, 64, 2048, torch.zeros(8, 16 * 64, dtype=BF16), None, None)


def test_ops_moe_gate_up_checks_the_twins_dimensions_before_any_launch():
    from dflash_amd import ops
    twin = ops.Bf16x13Weight(torch.zeros(8, dtype=torch.uint8), 8 * 2 * 64, 2048)
    act = torch.zeros(4, 16 * 64, dtype=BF16)
    x = torch.zeros(16 * 2048, dtype=BF16)
    with pytest.raises(ValueError, match="bf16x13 weight of 1024 x 2048"):
        ops.moe_gate_up(twin, x, 4, 64, 2048, act, None, None)          # E * 2I = 512 asked for
    assert "experts_gateup" in ops.X13_KINDS and isinstance(ops.X13_KINDS["experts_gateup"], bool)


@pytest.mark.parametrize("name", ["few", "second", "third"])
def test_expert_cases_are_in_format_by_the_packers_account(name):
    """Every expert-tall matrix the GPU tests stream: nothing refused, exactly the planted patches, each patch word naming
    the planted (k-step, lane, element, bits); it decodes back bit for bit; many bases, gate and up tile of a pair with
    different ones, the same tile of different experts with different ones, the items a patched workgroup walks with
    different ones; patches in all 16 waves of both tiles of the first, second and third item; and at every probed
    position the expected `act` is a normal nonzero bf16."""
    import bf16x13_cases as X
    import bf16x13_expert_cases as XE
    from dflash_amd import ops
    extreme = name == "second"
    case = XE.expert_case(name, extreme=extreme)
    E, I, K = case.E, case.I, XE.K
    N, per = E * 2 * I, 2 * (I // 16)
    wp = to_packed(case.w)
    w13, rep = ops.pack_weight_bf16x13(wp, N, K)
    assert w13 is not None and rep["refused"] == 0, rep
    assert rep["patched"] == len(case.patches) == 16 * len(case.patch_tiles), rep
    data = w13.data.numpy()
    assert np.array_equal(decode(data, N, K).reshape(-1), bits(wp)), "the 13-bit form does not reproduce the weight"
    meta = data[N // 16 * (K // 128) * QUAD:].view(np.uint32).reshape(N // 16, 16, 2)
    hb = meta[:, 0, 0].astype(int)
    # bases
    assert len(set(hb.tolist())) >= 5 + 2 * extreme, sorted(set(hb.tolist()))
    assert hb[case.special["zero"]] == 0 and (not extreme or (hb[case.special["top"]] == 112 and hb[case.special["deep"]] == 0))
    assert all(hb[g] != hb[u] for items in case.plan for g, u in items)                 # gate and up of every pair
    same_tile = [(hb[e * per + j], hb[(e + 1) * per + j]) for e in range(E - 1) for j in range(per)]
    assert sum(a != b for a, b in same_tile) >= 0.8 * len(same_tile)                   # the same tile of neighbouring experts
    assert all(len({hb[e * per + j] for e in range(E)}) >= 3 for j in range(per))
    vs_first = [hb[e * per + j] != hb[j] for e in range(1, E) for j in range(per)]     # ... and of expert 0 and any other
    assert sum(vs_first) >= 0.6 * len(vs_first)
    ptiles = set(case.patch_tiles)
    for items in case.plan:
        if items[0][0] in ptiles:      # a patched workgroup: every item of it patched, a base per item
            assert all(t in ptiles for pair in items for t in pair)
            assert all(hb[a[0]] != hb[b[0]] and hb[a[1]] != hb[b[1]] for a, b in zip(items, items[1:])), items
    longest = max(len(items) for items in case.plan)
    assert longest == {"few": 1, "second": 2, "third": 3}[name]
    for pos in range(longest):         # first, second, third item: all 16 waves of the gate and of the up tile
        tiles = {t for items in case.plan if len(items) > pos and items[pos][0] in ptiles for t in items[pos]}
        assert {t & 1 for t in tiles} == {0, 1}
        for par in (0, 1):
            assert {p.wave for p in case.patches if p.tile in tiles and (p.tile & 1) == par} == set(range(16)), (pos, par)
    # the active list: scrambled where the shape says so, and only active experts are patched
    assert sorted(case.lst) == sorted(set(case.lst)) and len(case.lst) == XE.SHAPES[name][2]
    assert (case.lst != sorted(case.lst)) == (name == "second")
    assert {p.tile // per for p in case.patches} <= set(case.lst)
    # the patch words against the table, the planted edge values
    wb = bits(case.w)
    for r, c, v in case.edges:
        assert wb[r, c] == v
    assert {0x0000, 0x8000, 0x0001, 0x807f} <= {v for _, _, v in case.edges}             # +-0, denormals
    assert int((meta[:, :, 1] >> 31).sum()) == len(case.patches)
    for p in case.patches:
        pw = int(meta[p.tile, p.wave, 1])
        assert (pw >> 31, (pw >> 28) & 7, (pw >> 22) & 63, (pw >> 19) & 7, pw & 0xffff) == (1, p.kstep, p.lane, p.element, p.bits)
        assert wb[p.row, p.col] == p.bits and (p.row, p.col) == (16 * p.tile + (p.lane & 15),
                                                                 (p.wave * 4 + p.kstep) * 32 + (p.lane >> 4) * 8 + p.element)
        assert 1 <= (p.bits >> 8) & 0x7f <= hb[p.tile] and p.bits & 0x7fff, "not a nonzero element below the window"
    P = case.patches
    assert {p.kstep for p in P} == set(range(4)) and {p.element for p in P} == set(range(8))
    assert {0, 63} <= {p.lane for p in P} and {(p.lane >> 3) & 1 for p in P} == {0, 1}
    assert {p.bits >> 15 for p in P} == {0, 1}
    assert {p.col for p in P} | {e[1] for e in case.edges} <= set(XE.probe_columns(case))
    # what the one-hot probe expects at every patched position: bf16(bf16(silu(g)) * u), a NORMAL nonzero bf16 (an
    # unapplied patch reads g or u as 0 and gives +-0: visible only because the right answer is not 0)
    pts = XE.probe_points(case)
    g = case.w[[q[3] for q in pts], [q[2] for q in pts]]
    u = case.w[[q[4] for q in pts], [q[2] for q in pts]]
    patched = torch.tensor([[p.row == q[3], p.row == q[4]] for p, q in zip(P, pts)])
    assert (patched.sum(dim=1) == 1).all()
    assert (u[patched[:, 1]].double() != 0).all() and (g[patched[:, 1]].double() > 0).all()   # (a patched up meets a positive gate)
    gd = g.double()
    s = (gd / (1 + torch.exp(-gd))).to(BF16)
    act = (s.double() * u.double()).to(BF16)
    eb = (act.view(torch.int16).to(torch.int32) >> 7) & 0xff
    assert ((eb >= 1) & (eb <= 254)).all(), "an expected act is zero, denormal or not finite"
    assert ((s.view(torch.int16).to(torch.int32) >> 7) & 0xff >= 1).all()
