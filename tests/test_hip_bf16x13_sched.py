"""The unconditional item requests of the 13-bit gate/up launch (k_gemm_w13<EPI_SILU, *>, csrc/gemm_skinny.hip "UNC";
DESIGN.md section 11): the item loop asks for the next item whether there is one or not — past the last item a dummy
whose descriptor holds zero bytes and whose meta load reads pair 0 — so that the compiler counts the loads in flight.  What
that can newly get wrong — a dummy that reads, writes or finishes something, an item decoded under another item's
{base, patch} pair, a sequence whose length is odd or shorter than the two buffers — is read here against the plain
packed bf16 form of the SAME matrix, bit for bit, on matrices with a base per tile and planted patches
(tests/bf16x13_cases.py), at more items per workgroup than the existing shapes walk.

The tile plans (grid_x_for): I = 12304 is 769 pairs over 193 workgroups — workgroups 0..189 walk four pairs (eight
items), 190..192 three (six).  I = 16400 is 1025 pairs over 205 workgroups, five pairs (ten items) each.  I = 512 is 32
pairs, one per workgroup: two items, each buffer used once, the third request a dummy."""
import pytest
import torch

import bf16x13_cases as X
import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
POISON = 0x7fa5       # a NaN no kernel writes
SHAPES = [(12304, 2048), (12304, 4096), (16400, 2048), (16400, 4096), (512, 2048)]
_cases = {}


def dev():
    return torch.device("cuda", 0)


def _same(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == BF16 else a, b.view(torch.int16) if b.dtype == BF16 else b)


def _patch_tiles(I):
    """Every tile of workgroups 0 and 1, of the middle one, of the last one that walks the longest sequence and of the
    last one: both buffers, every loop trip, the last item in front of the dummy."""
    plan = X.plan_silu(I)
    longest = max(len(p) for p in plan)
    pick = {0, 1, len(plan) // 2, max(b for b, p in enumerate(plan) if len(p) == longest), len(plan) - 1}
    tiles = sorted({t for b in pick for t, _ in plan[b]})
    assert not {X.ZERO_TILE, X.EDGE_TILE, X.TOP_TILE, X.DEEP_TILE} & set(tiles)
    return tiles


def _case(I, K):
    """(case, gate, up, packed bf16, 13-bit twin) of a shape: built once, shared by the tests, left unchanged."""
    from dflash_amd import ops
    if (I, K) not in _cases:
        case = X.make_case(2 * I, K, 3000 + I + K, _patch_tiles(I), False, dev())
        spots = {(p.row, p.col) for p in case.patches} | {(e[0], e[1]) for e in case.edges}
        wi = case.w.view(torch.int16)
        for p in case.patches:        # a positive gate over every patched up element (bf16x13_cases.silu_case)
            if p.tile & 1:
                assert (p.row - 16, p.col) not in spots
                wi[p.row - 16, p.col] &= 0x7fff
        gate, up = X.split_gateup(case.w)
        wp = ops.pack_weight_gateup(gate, up)
        w13, rep = ops.pack_weight_bf16x13(wp, 2 * I, K)
        assert w13 is not None and rep["refused"] == 0 and rep["patched"] == len(case.patches), rep
        _cases[(I, K)] = (case, gate, up, wp, w13)
    return _cases[(I, K)]


def _silu(mat, x, I, K, dyn=None, pad=4096):
    """One launch into a poisoned buffer of 16 I + pad elements: (act, the padding behind it)."""
    from dflash_amd import ops
    buf = torch.full((16 * I + pad,), POISON, dtype=torch.int16, device=dev()).view(BF16)
    ops.gemm_silu_mul(mat, x, I, K, buf, dyn=dyn)
    torch.cuda.synchronize()
    return buf[:16 * I], buf[16 * I:]


def test_plans_are_what_the_docstring_says():
    plan = X.plan_silu(12304)
    assert len(plan) == 193 and [len(p) for p in plan] == [8] * 190 + [6] * 3
    plan = X.plan_silu(16400)
    assert len(plan) == 205 and {len(p) for p in plan} == {10}
    assert len(X.plan_silu(512)) == 32


@pytest.mark.parametrize("I,K", SHAPES)
def test_silu_mul_equals_the_bf16_form_at_every_sequence_length(I, K):
    """16, 5 and 1 valid rows (the dyn record), from a normalised source and from a frag16 source: act is the bf16
    launch's, bit for bit, written everywhere, and the buffer behind the launch's columns keeps its poison."""
    from dflash_amd import ops
    case, gate, up, wp, w13 = _case(I, K)
    g = torch.Generator(device=dev()).manual_seed(I + K)
    rows = torch.randn(16, K, generator=g, device=dev()).to(BF16)
    ss = rows.float().pow(2).sum(-1).contiguous()
    nw = (1 + 0.1 * torch.randn(K, generator=g, device=dev())).to(BF16)
    for nvalid in (16, 5, 1):
        dyn = torch.zeros(8, dtype=torch.int32, device=dev())
        dyn[ops.DYN_BS] = nvalid
        frag = torch.empty(16 * K, dtype=BF16, device=dev())
        ops.pack_rows(rows, nvalid, frag)
        srcs = {"frag": ops.rows_frag(frag), "normed": ops.rows_normed(rows, ss, 1, nw, 1e-6, valid_word=ops.DYN_BS)}
        for name, x in srcs.items():
            want, wpad = _silu(wp, x, I, K, dyn)
            got, gpad = _silu(w13, x, I, K, dyn)
            assert (want.view(torch.int16) != POISON).all() and torch.isfinite(want.float()).all()
            assert want.float().abs().max() > 0
            assert _same(got, want), f"{name} source, {nvalid} rows: the 13-bit form differs from the bf16 form"
            assert (gpad.view(torch.int16) == POISON).all() and (wpad.view(torch.int16) == POISON).all()
            rows_of = got.view(I // 8, 16, 8)
            assert (rows_of[:, nvalid:].float() == 0).all()


@pytest.mark.parametrize("I,K", [(12304, 2048), (12304, 4096), (16400, 2048), (512, 2048)])
def test_one_hot_rows_keep_the_patches_of_every_item(I, K):
    """Row m = e_k: act[m, i] = bf16(bf16(silu(g)) * u) of the single weights.  A patch sits in every wave of every tile
    that workgroups 0, 1, the middle one, the last long one and the last one walk — both buffers, every loop trip, the
    item in front of the dummy.  At a patched position act is nonzero, of the right sign and within 2^-6 of fp64 (three
    bf16 roundings of at most 2^-9 each and __expf next to 0): an item decoded under another item's pair — the dummy's,
    say — reads its patched element as 0, or rebuilds the tile around the wrong base."""
    case, gate, up, wp, w13 = _case(I, K)
    cols = X.probe_columns(case)
    seen = 0
    for c0 in range(0, len(cols), 16):
        ck = cols[c0:c0 + 16]
        rows = torch.zeros(16, K, dtype=BF16, device=dev())
        rows[torch.arange(16, device=dev()), torch.tensor(ck, device=dev())] = 1.0
        from dflash_amd import ops
        frag = torch.empty(16 * K, dtype=BF16, device=dev())
        ops.pack_rows(rows, 16, frag)
        x = ops.rows_frag(frag)
        (want, _), (got, gpad) = _silu(wp, x, I, K), _silu(w13, x, I, K)
        assert torch.isfinite(want.float()).all() and want.float().abs().max() > 0
        same = _same(got, want)
        assert (gpad.view(torch.int16) == POISON).all()
        here = [(ck.index(p.col), (p.tile >> 1) * 16 + (p.row & 15)) for p in case.patches if p.col in ck]
        if here:
            act = got.view(I // 8, 16, 8).permute(1, 0, 2).reshape(16, I).double()       # [m, i]
            m, i = (torch.tensor(v, device=dev()) for v in zip(*here))
            k = torch.tensor(ck, device=dev())[m]
            gg, uu = gate[i, k].double(), up[i, k].double()
            ref = gg / (1 + torch.exp(-gg)) * uu
            a = act[m, i]
            assert (ref != 0).all()
            assert (a != 0).all() and (torch.sign(a) == torch.sign(ref)).all(), "a patched element was read as 0"
            assert ((a - ref).abs() <= 2.0 ** -6 * ref.abs()).all(), float(((a - ref).abs() / ref.abs()).max())
            seen += len(here)
        assert same, f"columns {ck}: the 13-bit form differs from the bf16 form"
    assert seen == len(case.patches)


def test_decode_session_at_intermediate_6144():
    """Hidden 2048 / intermediate 6144 (gate/up: 384 pairs, two per workgroup — four items of one quad), every
    gate/up with a base per tile: six cycles, eager and replayed, commit the ids, taus and tapped rows of
    stream_format="bf16"."""
    from dflash_amd import DFlashDraftModel, NativeTarget, ops
    from dflash_amd.config import DFlashConfig
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk, make_hf_qwen3
    I = 6144
    dims = dict(vocab_size=4208, hidden_size=2048, num_layers=4, num_heads=16, num_kv_heads=2, head_dim=128,
                intermediate_size=I, rope_theta=1e6)
    cfg = DFlashConfig(hidden_size=2048, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=2, head_dim=128,
                       intermediate_size=I, vocab_size=4208, num_target_layers=4, block_size=16, rope_theta=1e6,
                       mask_token_id=4207)
    torch.manual_seed(37)
    hf = make_hf_qwen3(dims, dev(), dtype=BF16)
    for layer in hf.model.layers:
        mlp = layer.mlp
        X.apply_tile_shifts(mlp.gate_proj.weight.data, mlp.up_proj.weight.data, mlp.down_proj.weight.data)
    perm = impose_greedy_walk(hf, seed=7)
    prompt = torch.randint(0, 4000, (1, 23), generator=torch.Generator().manual_seed(4)).to(dev())
    n_new = 16 * 8
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = [0, 15, 3, 9, 1, 12, 5, 7]
    sd = H.draft_weights(cfg, seed=8, dtype=BF16)
    for li in range(cfg.num_hidden_layers):
        p = f"layers.{li}.mlp."
        X.apply_tile_shifts(sd[p + "gate_proj.weight"], sd[p + "up_proj.weight"], sd[p + "down_proj.weight"])

    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 4000

    def run(fmt, graph):
        m = DFlashDraftModel(cfg, device=dev(), stream_format=fmt).load_state_dict(sd)
        nt = NativeTarget(hf, stream_format=fmt)
        twins = nt.gu13 + m.gu13
        assert all(isinstance(t, ops.Bf16x13Weight) for t in twins) if fmt == "auto" else not any(twins)
        s = DecodeSession(m, nt, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, max_block_size=16,
                          stop_token_ids=None, temperature=0.0, draft_token_hook=hook)
        s.prefill()
        hidden, taus = [], []
        for i in range(6):
            if graph and i == 2:
                s.capture(16)
            r = s.cycle_graph(16) if graph and i >= 2 else s.cycle(16, ahead_ok=True)
            taus.append(r.tau)
            hidden.append(s.target_hidden.clone())
        torch.cuda.synchronize()
        return s.output_ids[0, :s.start + 1].clone(), taus, hidden

    for graph in (False, True):
        ids_b, taus_b, hid_b = run("bf16", graph)
        ids_a, taus_a, hid_a = run("auto", graph)
        assert ids_b.tolist() == G[:ids_b.numel()].tolist()
        assert torch.equal(ids_a, ids_b) and taus_a == taus_b, f"graph={graph}"
        assert all(_same(a, b) for a, b in zip(hid_a, hid_b)), f"graph={graph}: target_hidden differs"
