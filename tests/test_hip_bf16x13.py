"""The lossless 13-bit bf16 weight stream on the GPU (DFL_W_BF16X13): dfl_gemm_silu_mul and
dfl_gemm_argmax over the 13-bit form against the plain packed bf16 form of the SAME matrix in the same build, bit for
bit — the decode rebuilds the same fragments, so every sum sees the same operands in the same order and no tolerance
applies — and a small decode session whose committed ids and tapped hidden rows do not depend on stream_format.
Below that: the same on matrices with a base per tile (tests/bf16x13_cases.py), a one-hot probe that reads single weights
through the kernel's decode — the weight itself is the reference — and sessions over models the packer took only in part."""
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


# ---- a base per tile, patches that count (tests/bf16x13_cases.py; the CPU side: tests/test_bf16x13_cpu.py) ----
# The matrices above give every tile base 46 and patched elements that vanish in a random row's sum.  The ones below have
# seven bases cycling over the tiles (so that the items a workgroup walks, the two tiles of a gate/up pair and a halved
# tail differ), a patch in all 16 waves of the tiles that are some workgroups' first, second and third items, and are
# read two ways: against the bf16 form under random rows, and ALONE under one-hot rows, where a sum is one weight.

def _pack13(wp, N, K, case):
    from dflash_amd import ops
    w13, rep = ops.pack_weight_bf16x13(wp, N, K)
    assert w13 is not None and rep["refused"] == 0 and rep["patched"] == len(case.patches), rep
    meta = w13.data[N // 16 * (K // 128) * ops.X13_QUAD_BYTES:].view(torch.int32).view(N // 16, 16, 2)
    assert torch.unique(meta[:, 0, 0]).numel() >= 5
    return w13


def _argmax(mat, x, V, K, row0=0, nrows=16, dyn=None, word=-1):
    from dflash_amd import ops
    ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
    logits = torch.full((16, V), float("nan"), dtype=BF16, device=dev())
    margins = torch.full((16,), float("nan"), dtype=torch.float32, device=dev())
    ops.gemm_argmax(mat, x, V, K, row0, nrows, ops.argmax_ws(dev()), ids, 0, dyn=dyn, nrows_dyn_word=word, logits=logits,
                    margins=margins)
    torch.cuda.synchronize()
    return ids, logits, margins


def _silu(mat, x, I, K):
    from dflash_amd import ops
    act = torch.full((16 * I,), float("nan"), dtype=BF16, device=dev())
    ops.gemm_silu_mul(mat, x, I, K, act)
    torch.cuda.synchronize()
    return act


def _one_hot(cols, K):
    """The fragment source whose row m is the unit vector e_{cols[m]}."""
    from dflash_amd import ops
    rows = torch.zeros(16, K, dtype=BF16, device=dev())
    rows[torch.arange(16, device=dev()), torch.tensor(cols, device=dev())] = 1.0
    frag = torch.empty(16 * K, dtype=BF16, device=dev())
    ops.pack_rows(rows, 16, frag)
    return ops.rows_frag(frag)


@pytest.mark.parametrize("V,K", [(4208, 4096), (9600, 4096), (8192, 4096), (2048, 4096), (4208, 2048), (2048, 2048)])
def test_argmax_equals_the_bf16_form_with_a_base_per_tile(V, K):
    """263 tiles: whole + a halved tail; 600: whole, whole, half, both buffers; 512: two whole items; 128: every tile
    halved, the first item a half."""
    import bf16x13_cases as X
    from dflash_amd import ops
    case = X.argmax_case(V, K, device=dev())
    wp = ops.pack_weight(case.w)
    w13 = _pack13(wp, V, K, case)
    srcs, _ = _sources(K, 23)
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    dyn[ops.DYN_BS] = 5
    cases = [("16 rows", 0, 16, None, -1), ("15 rows from row 1", 1, 15, None, -1), ("5 rows by the record", 0, 16, dyn, ops.DYN_BS)]
    for sname, x in srcs.items():
        for cname, row0, nrows, d, word in cases:
            want, got = _argmax(wp, x, V, K, row0, nrows, d, word), _argmax(w13, x, V, K, row0, nrows, d, word)
            live = 5 if d is not None else nrows
            for a, b, what in zip(got, want, ("ids", "logits", "margins")):
                if what == "logits":
                    a, b = a[row0:row0 + live], b[row0:row0 + live]
                    assert torch.isfinite(b.float()).all() and b.float().abs().max() > 0
                else:
                    a, b = a[:live], b[:live]
                assert _same(a, b), f"{sname} source, {cname}: {what} differ from the bf16 form"


@pytest.mark.parametrize("I,K", [(512, 4096), (4352, 4096), (4112, 4096), (8208, 4096), (512, 2048), (4112, 2048)])
def test_silu_mul_equals_the_bf16_form_with_a_base_per_tile(I, K):
    """32 pairs: one per workgroup; 272: two; 257: the last workgroup has one pair fewer; 513: three pairs, six items."""
    import bf16x13_cases as X
    from dflash_amd import ops
    case = X.silu_case(I, K, device=dev())
    wp = ops.pack_weight_gateup(*X.split_gateup(case.w))
    w13 = _pack13(wp, 2 * I, K, case)
    srcs, _ = _sources(K, 24)
    for name, x in srcs.items():
        want, got = _silu(wp, x, I, K), _silu(w13, x, I, K)
        assert torch.isfinite(want.float()).all() and want.float().abs().max() > 0
        assert _same(got, want), f"{name} source: the 13-bit form differs from the bf16 form"


@pytest.mark.parametrize("V,K", [(4208, 4096), (9600, 4096), (8192, 4096), (2048, 4096), (4208, 2048), (2048, 2048)])
def test_argmax_logits_of_one_hot_rows_are_the_weights(V, K):
    """Row m of the source is e_k: every sum is ONE product, and logits[m, n] is w[n, k] itself — a reference that owes
    nothing to the bf16 kernel.  (The sum adds the product to +0 and to the other products, all +-0: a weight of -0
    comes out as +0, as IEEE addition has it; every other bit pattern, denormals included, comes out as it is.)  Probed:
    every patched column, the first and the last column of every wave's share, the planted +-0, denormals, top-binade
    and lowest-window values, the base-112 tile and the tile 100 binades down — over ALL V rows, so that a patch written
    to the wrong lane, or into the other workgroup's half of a halved tile, shows as well."""
    import bf16x13_cases as X
    from dflash_amd import ops
    case = X.argmax_case(V, K, extreme=True, device=dev())
    w13 = _pack13(ops.pack_weight(case.w), V, K, case)
    wbits = case.w.view(torch.int16)
    cols = X.probe_columns(case)
    assert {p.col for p in case.patches} | {e[1] for e in case.edges} <= set(cols)
    for c0 in range(0, len(cols), 16):
        ck = cols[c0:c0 + 16]
        ids, logits, _ = _argmax(w13, _one_hot(ck, K), V, K)
        want = wbits[:, ck].t()
        want = torch.where(want == -32768, torch.zeros_like(want), want)
        got = logits.view(torch.int16)
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (f"{bad.shape[0]} logits differ from the weights; the first: column {ck[int(bad[0, 0])]}, "
                                  f"row {int(bad[0, 1])}: {int(got[tuple(bad[0])]) & 0xffff:#06x} for "
                                  f"{int(want[tuple(bad[0])]) & 0xffff:#06x}")
        col = case.w[:, ck].double().t()                    # [16, V]: the argmax is the first largest weight of the column
        first = torch.where(col == col.max(dim=1, keepdim=True).values, torch.arange(V, device=dev()), V).min(dim=1).values
        assert torch.equal(ids, first)


@pytest.mark.parametrize("I,K", [(512, 4096), (4352, 4096), (4112, 4096), (8208, 4096), (512, 2048), (4112, 2048)])
def test_silu_mul_of_one_hot_rows_keeps_every_patch(I, K):
    """The same one-hot rows through gate/up + SiLU: act[m, i] = bf16(bf16(silu(g)) * u) of the single weights g =
    gate[i, k], u = up[i, k].  Bit for bit the bf16 form's; and where g or u is a PATCHED element — one that decodes to 0
    if its patch word is dropped — act is nonzero, has the sign of silu(g) * u and lies within 2^-6 of it (fp64, from the
    weights): three bf16 roundings of at most 2^-9 each and __expf next to 0."""
    import bf16x13_cases as X
    from dflash_amd import ops
    case = X.silu_case(I, K, device=dev())
    gate, up = X.split_gateup(case.w)
    wp = ops.pack_weight_gateup(gate, up)
    w13 = _pack13(wp, 2 * I, K, case)
    cols = X.probe_columns(case)
    seen = 0
    for c0 in range(0, len(cols), 16):
        ck = cols[c0:c0 + 16]
        x = _one_hot(ck, K)
        want, got = _silu(wp, x, I, K), _silu(w13, x, I, K)
        assert torch.isfinite(want.float()).all() and want.float().abs().max() > 0
        same = _same(got, want)
        act = got.view(I // 8, 16, 8).permute(1, 0, 2).reshape(16, I).double()       # [m, i]
        here = [(ck.index(p.col), (p.tile >> 1) * 16 + (p.row & 15)) for p in case.patches if p.col in ck]
        if not here:
            assert same, f"columns {ck}: the 13-bit form differs from the bf16 form"
            continue
        m, i = (torch.tensor(v, device=dev()) for v in zip(*here))
        k = torch.tensor(ck, device=dev())[m]
        g, u = gate[i, k].double(), up[i, k].double()
        ref = g / (1 + torch.exp(-g)) * u
        a = act[m, i]
        assert (ref != 0).all()
        assert (a != 0).all() and (torch.sign(a) == torch.sign(ref)).all(), "a patched element was read as 0"
        assert ((a - ref).abs() <= 2.0 ** -6 * ref.abs()).all(), float(((a - ref).abs() / ref.abs()).max())
        assert same, f"columns {ck}: the 13-bit form differs from the bf16 form"
        seen += len(here)
    assert seen == len(case.patches)


@pytest.mark.parametrize("refused", ["layers", "lm_head"])
def test_decode_session_with_some_matrices_kept_as_bf16(refused):
    """The session test above over a MIXED model: every gate/up has a base per tile (tests/bf16x13_cases.py's rule; the
    down columns undo the powers, so the greedy walk stands), and the packer refuses
      "layers":  target layer 2's and draft layer 1's gate/up (two below-window elements in one (tile, wave) item of the
                 gate) — those layers stream plain bf16 between layers that stream their twins;
      "lm_head": the shared head — the draft's unmask and the target's verify fall back to the packed bf16 head.
    Ids, taus and tapped hidden rows are stream_format="bf16"'s, eager and replayed."""
    import gc

    import bf16x13_cases as X
    from dflash_amd import DFlashDraftModel, NativeTarget, ops
    from dflash_amd.config import DFlashConfig
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk, make_hf_qwen3
    dims = dict(vocab_size=4208, hidden_size=2048, num_layers=4, num_heads=16, num_kv_heads=2, head_dim=128,
                intermediate_size=2176, rope_theta=1e6)
    cfg = DFlashConfig(hidden_size=2048, num_hidden_layers=2, num_attention_heads=16, num_key_value_heads=2, head_dim=128,
                       intermediate_size=2176, vocab_size=4208, num_target_layers=4, block_size=16, rope_theta=1e6,
                       mask_token_id=4207)
    t_bad, d_bad = (2, 1) if refused == "layers" else (None, None)
    torch.manual_seed(33)
    hf = make_hf_qwen3(dims, dev(), dtype=BF16)
    for li, layer in enumerate(hf.model.layers):
        mlp = layer.mlp
        X.apply_tile_shifts(mlp.gate_proj.weight.data, mlp.up_proj.weight.data, mlp.down_proj.weight.data)
        if li == t_bad:
            X.plant_refusal(mlp.gate_proj.weight.data, 4, 3)
    perm = impose_greedy_walk(hf, seed=7)
    if refused == "lm_head":
        X.plant_refusal(hf.lm_head.weight.data, 200, 11)
    prompt = torch.randint(0, 4000, (1, 23), generator=torch.Generator().manual_seed(4)).to(dev())
    n_new = 16 * 8
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = [0, 15, 3, 9, 1, 12, 5, 7]
    sd = H.draft_weights(cfg, seed=8, dtype=BF16)
    for li in range(cfg.num_hidden_layers):
        p = f"layers.{li}.mlp."
        X.apply_tile_shifts(sd[p + "gate_proj.weight"], sd[p + "up_proj.weight"], sd[p + "down_proj.weight"])
        if li == d_bad:
            X.plant_refusal(sd[p + "gate_proj.weight"], 135, 15)

    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 4000

    def run(fmt, graph):
        gc.collect()
        kept0 = ops.bf16x13_report()["kept_bf16"]
        m = DFlashDraftModel(cfg, device=dev(), stream_format=fmt).load_state_dict(sd)
        nt = NativeTarget(hf, stream_format=fmt)
        s = DecodeSession(m, nt, prompt, mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, max_block_size=16,
                          stop_token_ids=None, temperature=0.0, draft_token_hook=hook)
        s.prefill()
        if fmt == "auto":
            want = [li != t_bad for li in range(4)] + [li != d_bad for li in range(2)]
            assert [isinstance(t, ops.Bf16x13Weight) for t in nt.gu13 + m.gu13] == want
            assert [t is None for t in nt.gu13 + m.gu13] == [not v for v in want]
            for t in nt.gu13 + m.gu13:
                if t is not None:     # a base per tile, by the packer's account
                    meta = t.data[t.N // 16 * (t.K // 128) * ops.X13_QUAD_BYTES:].view(torch.int32).view(-1, 16, 2)
                    assert torch.unique(meta[:, 0, 0]).numel() >= 5
            head = ops.bf16x13_twin(nt.lm_wp, nt.V, nt.H, "lm_head")
            assert (head is None) == (refused == "lm_head") and (head is None or isinstance(head, ops.Bf16x13Weight))
            assert ops.bf16x13_report()["kept_bf16"] - kept0 == (2 if refused == "layers" else 1)
        else:
            assert not any(nt.gu13 + m.gu13) and ops.bf16x13_report()["kept_bf16"] == kept0
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
