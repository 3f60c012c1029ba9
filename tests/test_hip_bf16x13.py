"""The lossless 13-bit bf16 weight stream on the GPU (DFL_W_BF16X13): dfl_gemm_silu_mul and
dfl_gemm_argmax over the 13-bit form against the plain packed bf16 form of the SAME matrix in the same build, bit for
bit — the decode rebuilds the same fragments, so every sum sees the same operands in the same order and no tolerance
applies — and a small decode session whose committed ids and tapped hidden rows do not depend on stream_format."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def dev():
    return torch.device("cuda", 0)


def _bits(v: int) -> torch.Tensor:
    return torch.tensor([v if v < 32768 else v - 65536], dtype=torch.int16).view(BF16)[0]


def _weight(n, k, seed, zero_tile=None):
    """randn * 0.02 [n, k] with the format's edge cases planted in tiles 0 and 1: in the first and the last k-step of a
    wave's share (waves 0 and 15), in lanes 0 (row 0, k group 0) and 63 (row 15, k group 3).  Tile 0: +-0, a denormal,
    exponent 1, the tile's top binade and its window's lowest.  Tile 1: one nonzero element below the window per planted
    item (patched).  zero_tile: that tile all zeros."""
    g = torch.Generator(device=dev()).manual_seed(seed)
    w = (torch.randn(n, k, generator=g, device=dev()) * 0.02).to(BF16)
    nfr = k // 512
    first, last = 0, 15 * nfr * 32 + (nfr - 1) * 32     # first k of wave 0's first k-step, of wave 15's last k-step
    top = int((w[:16].view(torch.int16) & 0x7fff).max()) >> 8      # H & 0x7f of tile 0's largest magnitude
    lowest = ((top - 14) << 8) | 0x33
    plant = [0x0000, 0x8000, 0x0001, 0x807f, 0x0080, 0x80ff, (top << 8) | 0x7f, 0x8000 | (top << 8), lowest, 0x8000 | lowest]
    for i, v in enumerate(plant):
        lane63 = i & 1
        col = (first if i % 4 < 2 else last) + (24 if lane63 else 0) + i // 2
        w[15 if lane63 else 0, col] = _bits(v)
    top1 = int((w[16:32].view(torch.int16) & 0x7fff).max()) >> 8
    below = ((top1 - 15) << 8) | 0x5a
    w[16, first + 2] = _bits(below)                     # tile 1, wave 0, first k-step, lane 0
    w[31, last + 31] = _bits(0x8000 | below)            # tile 1, wave 15, last k-step, lane 63, element 7
    if zero_tile is not None:
        w[16 * zero_tile:16 * zero_tile + 16] = 0
    return w


def _sources(k, seed):
    """A fragment source and a normalised (mode 2) source over the same 16 rows."""
    from dflash_amd import ops
    g = torch.Generator(device=dev()).manual_seed(seed)
    rows = torch.randn(16, k, generator=g, device=dev()).to(BF16)
    frag = torch.empty(16 * k, dtype=BF16, device=dev())
    ops.pack_rows(rows, 16, frag)
    ss = rows.float().pow(2).sum(-1).contiguous()
    nw = (1 + 0.1 * torch.randn(k, generator=g, device=dev())).to(BF16)
    return {"frag": ops.rows_frag(frag), "normed": ops.rows_normed(rows, ss, 1, nw, 1e-6)}, rows


def _same(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == BF16 else a, b.view(torch.int16) if b.dtype == BF16 else b)


@pytest.mark.parametrize("K", [4096, 2048])
@pytest.mark.parametrize("I", [512, 4352])   # 32 pairs: most workgroups idle; 272: workgroups with one and with two pairs
def test_silu_mul_equals_the_bf16_form(I, K):
    from dflash_amd import ops
    gate, up = _weight(I, K, 11, zero_tile=3), _weight(I, K, 12)
    wp = ops.pack_weight_gateup(gate, up)
    w13, rep = ops.pack_weight_bf16x13(wp, 2 * I, K)
    assert w13 is not None and rep["patched"] == 4 and rep["refused"] == 0, rep
    srcs, _ = _sources(K, 13)
    for name, x in srcs.items():
        want = torch.full((16 * I,), float("nan"), dtype=BF16, device=dev())
        got = want.clone()
        ops.gemm_silu_mul(wp, x, I, K, want)
        ops.gemm_silu_mul(w13, x, I, K, got)
        torch.cuda.synchronize()
        assert torch.isfinite(want.float()).all() and want.float().abs().max() > 0
        assert _same(got, want), f"{name} source: the 13-bit form differs from the bf16 form"


@pytest.mark.parametrize("V,K", [(4208, 4096), (9600, 4096), (4208, 2048)])   # 263 tiles: a half-tile tail; 600: 2 - 3 items
def test_argmax_equals_the_bf16_form(V, K):
    from dflash_amd import ops
    w = _weight(V, K, 21, zero_tile=5)
    n1, n2 = 3 * 16 + 5, (V // 16 - 1) * 16 + 9      # a tie across tiles (the second one in the half-tile tail)
    w[n2] = w[n1]
    srcs, rows = _sources(K, 22)
    rows[2] = (w[n1].float() * 50).to(BF16)          # row 2's best logit belongs to n1 AND n2: the first index wins
    frag = torch.empty(16 * K, dtype=BF16, device=dev())
    ops.pack_rows(rows, 16, frag)
    srcs["frag"] = ops.rows_frag(frag)
    srcs["normed"] = ops.rows_normed(rows, rows.float().pow(2).sum(-1).contiguous(), 1, srcs["normed"].keep[2], 1e-6)
    wp = ops.pack_weight(w)
    w13, rep = ops.pack_weight_bf16x13(wp, V, K)
    assert w13 is not None and rep["patched"] == 2 and rep["refused"] == 0, rep
    ws = ops.argmax_ws(dev())
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    dyn[ops.DYN_BS] = 5
    cases = [("16 rows", 0, 16, None, -1), ("15 rows from row 1", 1, 15, None, -1), ("5 rows by the record", 0, 16, dyn, ops.DYN_BS)]
    for sname, x in srcs.items():
        for cname, row0, nrows, d, word in cases:
            out = {}
            for form, mat in (("bf16", wp), ("x13", w13)):
                ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
                logits = torch.full((16, V), float("nan"), dtype=BF16, device=dev())
                margins = torch.full((16,), float("nan"), dtype=torch.float32, device=dev())
                ops.gemm_argmax(mat, x, V, K, row0, nrows, ws, ids, 0, dyn=d, nrows_dyn_word=word, logits=logits,
                                margins=margins)
                torch.cuda.synchronize()
                out[form] = (ids, logits, margins)
            live = 5 if d is not None else nrows
            for a, b, what in zip(out["x13"], out["bf16"], ("ids", "logits", "margins")):
                if what == "logits":
                    a, b = a[row0:row0 + live], b[row0:row0 + live]
                    assert torch.isfinite(b.float()).all()
                else:
                    a, b = a[:live], b[:live]
                assert _same(a, b), f"{sname} source, {cname}: {what} differ from the bf16 form"
            if row0 <= 2 < row0 + live:
                assert int(out["x13"][0][2 - row0]) == n1 and float(out["x13"][2][2 - row0]) == 0.0, (sname, cname)


def test_decode_session_does_not_depend_on_the_stream_format():
    """Six cycles, eager and replayed from the captured graphs: stream_format="auto" (13-bit gate/up in target and draft,
    one shared 13-bit lm_head) commits the ids and taps the hidden rows of stream_format="bf16".  Hidden 2048: the
    narrowest width the 13-bit layout covers (at the hidden 512 of the tiny models "auto" IS plain bf16)."""
    from dflash_amd import DFlashDraftModel, NativeTarget, ops
    from dflash_amd.config import DFlashConfig
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk, make_hf_qwen3
    dims = dict(vocab_size=4208, hidden_size=2048, num_layers=4, num_heads=16, num_kv_heads=2, head_dim=128,
                intermediate_size=2176, rope_theta=1e6)
    cfg = DFlashConfig(hidden_size=2048, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=2, head_dim=128,
                       intermediate_size=2176, vocab_size=4208, num_target_layers=4, block_size=16, rope_theta=1e6,
                       mask_token_id=4207)
    torch.manual_seed(31)
    hf = make_hf_qwen3(dims, dev(), dtype=BF16)
    perm = impose_greedy_walk(hf, seed=6)
    prompt = torch.randint(0, 4000, (1, 23), generator=torch.Generator().manual_seed(4)).to(dev())
    n_new = 16 * 8
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = [0, 15, 3, 9, 1, 12, 5, 7]
    sd = H.draft_weights(cfg, seed=5, dtype=BF16)

    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 4000

    def run(fmt, graph):
        m = DFlashDraftModel(cfg, device=dev(), stream_format=fmt).load_state_dict(sd)
        nt = NativeTarget(hf, stream_format=fmt)
        twins = nt.gu13 + m.gu13
        assert len(twins) == 4 + 2
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
