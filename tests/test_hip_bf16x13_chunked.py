"""The K-chunked form of the 13-bit bf16 weight stream on the GPU (k_gemm_w13c: dfl_gemm_resid over DFL_W_BF16X13 at K a
multiple of 2048 above 4096; DESIGN.md section 11, "down_proj and fc") against the plain packed bf16 form of the SAME
matrix in the same build, bit for bit: the decode rebuilds the same fragments, so every sum sees the same operands in the
same order and no tolerance applies.  The matrices (tests/bf16x13_chunked_cases.py) have a base per tile and a patch in
every (chunk, wave) item of the tiles some workgroups walk first and second; they are read under random rows and ALONE
under one-hot rows, where a sum is one weight and the weight itself is the reference.  Then a decode session whose
down_proj launches (and fc's, where that kind is kept) stream the twins — one layer's down refused by the packer — against stream_format="bf16"."""
import pytest
import torch

import bf16x13_chunked_cases as XC
import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
_cases = {}


def dev():
    return torch.device("cuda", 0)


def _same(a, b):
    return torch.equal(a.view(torch.int16) if a.dtype == BF16 else a, b.view(torch.int16) if b.dtype == BF16 else b)


def _case(N, K):
    """(case, packed bf16, 13-bit twin) of a shape: built once, shared by the tests, left unchanged."""
    from dflash_amd import ops
    if (N, K) not in _cases:
        case = XC.chunked_case(N, K, device=dev())
        wp = ops.pack_weight(case.w)
        w13, rep = ops.pack_weight_bf16x13(wp, N, K)
        assert w13 is not None and rep == {"items": N // 16 * (K // 128), "patched": len(case.patches), "refused": 0}, rep
        _cases[(N, K)] = (case, wp, w13)
    return _cases[(N, K)]


def _resid(mat, x, N, K, h0, add, dyn=None):
    """One dfl_gemm_resid launch on a copy of h0 [16, N + 16] (row stride N + 16): h_io, tap, ss_out."""
    from dflash_amd import ops
    h = h0.clone()
    tap = torch.full((16, N + 32), float("nan"), dtype=BF16, device=dev())
    ss = torch.full((N,), float("nan"), dtype=torch.float32, device=dev())
    ops.gemm_resid(mat, x, N, K, h[:, :N], add_residual=add, ss_out=ss, tap=tap[:, :N], dyn=dyn)
    torch.cuda.synchronize()
    return h, tap, ss


@pytest.mark.parametrize("N,K", XC.SHAPES)
def test_gemm_resid_equals_the_bf16_form(N, K):
    """h_io, tap and ss_out, with and without the residual add, from a frag16 source and from plain rows whose valid
    count (11) comes from the dyn record — fc's form; the columns beyond N and the tap's padding stay untouched."""
    from dflash_amd import ops
    case, wp, w13 = _case(N, K)
    g = torch.Generator(device=dev()).manual_seed(N + K)
    rows = torch.randn(16, K, generator=g, device=dev()).to(BF16)
    frag = torch.empty(16 * K, dtype=BF16, device=dev())
    ops.pack_rows(rows, 16, frag)
    dyn = torch.zeros(16, dtype=torch.int32, device=dev())
    dyn[ops.DYN_TAU] = 11
    h0 = torch.randn(16, N + 16, generator=g, device=dev()).to(BF16)
    sources = {"frag": (ops.rows_frag(frag), None), "plain+dyn": (ops.rows_plain(rows, ops.DYN_TAU), dyn)}
    for sname, (src, d) in sources.items():
        for add in (False, True):
            ref = _resid(wp, src, N, K, h0, add, d)
            got = _resid(w13, src, N, K, h0, add, d)
            for what, a, b in zip(("h_io", "tap", "ss_out"), got, ref):
                assert _same(a, b), f"{sname} source, add_residual={add}: {what} differs from the bf16 form"
            assert _same(got[0][:, N:], h0[:, N:]) and torch.isnan(got[1][:, N:].float()).all()
            assert not torch.isnan(got[2]).any()
            if d is not None and not add:       # rows past the valid count saw zero activations
                assert (got[0][11:, :N].float() == 0).all()
    # the two sources agree with each other where both rows are valid, and the result is not trivially zero
    a = _resid(w13, sources["frag"][0], N, K, h0, False)[0]
    b = _resid(w13, sources["plain+dyn"][0], N, K, h0, False, dyn)[0]
    assert _same(a[:11, :N], b[:11, :N]) and (a[:, :N].float() != 0).any()


@pytest.mark.parametrize("N,K", XC.SHAPES)
def test_one_hot_rows_read_the_weights_themselves(N, K):
    """Row m = e_k without the residual add makes h_io[m, n] = W[n, k]: every patched column, the first and the last
    column of every (chunk, wave) share and every edge value's column, 16 per launch, against the matrix's own bits (a
    denormal is flushed by the MFMA: compared through the bf16 launch, which has the same hardware in its path)."""
    from dflash_amd import ops
    case, wp, w13 = _case(N, K)
    cols = XC.probe_columns(case)
    assert len(cols) % 16 == 0
    wt = case.w
    h0 = torch.zeros(16, N, dtype=BF16, device=dev())
    seen_p, seen_e = 0, 0
    by_col = {}
    for p in case.patches:
        by_col.setdefault(p.col, []).append(p)
    for i in range(0, len(cols), 16):
        cc = cols[i:i + 16]
        x = torch.zeros(16, K, dtype=BF16, device=dev())
        x[torch.arange(16, device=dev()), torch.tensor(cc, device=dev())] = 1.0
        frag = torch.empty(16 * K, dtype=BF16, device=dev())
        ops.pack_rows(x, 16, frag)
        got = _resid(w13, ops.rows_frag(frag), N, K, h0, False)[0]
        ref = _resid(wp, ops.rows_frag(frag), N, K, h0, False)[0]
        assert _same(got, ref), f"columns {cc}: the twin's weights differ from the bf16 form's"
        want = wt[:, torch.tensor(cc, device=dev())].t().contiguous()          # [16, N]
        normal = (want.view(torch.int16) & 0x7f80) != 0                         # (denormals: flushed in the MFMA)
        assert torch.equal(got.view(torch.int16)[normal], want.view(torch.int16)[normal]), f"columns {cc}"
        gi = got.view(torch.int16)
        for m, col in enumerate(cc):
            for p in by_col.get(col, []):
                assert (int(gi[m, p.row]) & 0xffff) == p.bits, f"patch {p} lost"
                seen_p += 1
            for row, ecol, v in case.edges:
                if ecol == col and (v & 0x7f80):
                    assert (int(gi[m, row]) & 0xffff) == v, f"edge value {v:#x} at ({row}, {ecol})"
                    seen_e += 1
    assert seen_p >= len(case.patches) and seen_e == sum(1 for e in case.edges if e[2] & 0x7f80)


def test_decode_session_streams_down_and_fc_twins():
    """Six cycles, eager and replayed, hidden 2048 / intermediate 6144, four target layers and three draft layers
    (fc_in 6144): stream_format="auto" commits the ids, taus and tapped rows of "bf16".  Every down has a base per tile;
    target layer 2's is refused by the packer (two below-window elements in one (tile, chunk, wave) item) and streams
    plain bf16 between layers that stream their twins.  A spy on ops.gemm_resid shows which launches received codes."""
    import gc

    from dflash_amd import DFlashDraftModel, NativeTarget, ops
    from dflash_amd.config import DFlashConfig
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk, make_hf_qwen3
    I = 6144
    dims = dict(vocab_size=4208, hidden_size=2048, num_layers=4, num_heads=16, num_kv_heads=2, head_dim=128,
                intermediate_size=I, rope_theta=1e6)
    cfg = DFlashConfig(hidden_size=2048, num_hidden_layers=3, num_attention_heads=16, num_key_value_heads=2, head_dim=128,
                       intermediate_size=I, vocab_size=4208, num_target_layers=4, block_size=16, rope_theta=1e6,
                       mask_token_id=4207)
    assert cfg.fc_in == 6144
    # even powers of two, at most 16 up: seven different bases (the base follows the exponent's upper seven bits), exact
    # in bf16, and the residual stream stays dominated by the embedding, which the greedy walk needs
    shifts = torch.tensor([0, 2, -2, 4, -4, -6, -8], dtype=torch.float32)

    def shift_rows(w):       # output-row tile t times 2^shifts[t % 7]
        s = shifts.to(w.device)[(torch.arange(w.shape[0], device=w.device) // 16) % 7]
        w.mul_(torch.exp2(s).view(-1, 1).to(w.dtype))

    torch.manual_seed(35)
    hf = make_hf_qwen3(dims, dev(), dtype=BF16)
    perm = impose_greedy_walk(hf, seed=9)
    for li, layer in enumerate(hf.model.layers):       # (behind the walk's own scaling of down_proj, which rounds)
        shift_rows(layer.mlp.down_proj.weight.data)
        if li == 2:
            XC.plant_refusal(layer.mlp.down_proj.weight.data, 7, 1, 5)
    prompt = torch.randint(0, 4000, (1, 23), generator=torch.Generator().manual_seed(4)).to(dev())
    n_new = 16 * 8
    G = greedy_walk(perm, prompt, n_new + 40).to(dev())
    plan = [0, 15, 3, 9, 1, 12, 5, 7]
    sd = H.draft_weights(cfg, seed=8, dtype=BF16)
    for li in range(cfg.num_hidden_layers):
        shift_rows(sd[f"layers.{li}.mlp.down_proj.weight"])

    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % 4000

    def run(fmt, graph, monkey):
        gc.collect()
        kept0 = ops.bf16x13_report()["kept_bf16"]
        m = DFlashDraftModel(cfg, device=dev(), stream_format=fmt).load_state_dict(sd)
        nt = NativeTarget(hf, stream_format=fmt)
        if fmt == "auto":
            assert [isinstance(t, ops.Bf16x13Weight) for t in nt.down13] == [True, True, False, True]
            assert nt.down13[2] is None and all(isinstance(t, ops.Bf16x13Weight) for t in m.down13)
            assert isinstance(m.fc13, ops.Bf16x13Weight) if ops.X13_KINDS["fc"] else m.fc13 is None
            assert ops.bf16x13_report()["kept_bf16"] - kept0 == 1
            for t in [t for t in nt.down13 + m.down13 if t is not None]:     # a base per tile, by the packer's account
                meta = t.data[t.N // 16 * (t.K // 128) * ops.X13_QUAD_BYTES:].view(torch.int32).view(t.N // 16, -1, 2)
                assert meta.shape[1] == 48 and torch.unique(meta[:, 0, 0]).numel() >= 5
        else:
            assert not any(nt.down13 + m.down13) and m.fc13 is None and ops.bf16x13_report()["kept_bf16"] == kept0
        seen = []
        real = ops.gemm_resid

        def spy(wp, x, N, K, *a, **kw):
            seen.append((N, K, isinstance(wp, ops.Bf16x13Weight)))
            return real(wp, x, N, K, *a, **kw)

        monkey.setattr(ops, "gemm_resid", spy)
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
        monkey.setattr(ops, "gemm_resid", real)
        down = [c for n, k, c in seen if (n, k) == (2048, I)]       # (fc among them: fc_in == I)
        other = [c for n, k, c in seen if k <= 4096]
        assert down and not any(other)
        if fmt == "auto":       # per cycle: four target downs (layer 2 plain), three draft downs and fc (by its kind)
            plain = 1 + (0 if ops.X13_KINDS["fc"] else 1)
            assert any(down) and not all(down) and sum(not c for c in down) * 7 <= len(down) * plain, (len(down), sum(down))
        else:
            assert not any(down)
        return s.output_ids[0, :s.start + 1].clone(), taus, hidden

    for graph in (False, True):
        with pytest.MonkeyPatch.context() as monkey:
            ids_b, taus_b, hid_b = run("bf16", graph, monkey)
            ids_a, taus_a, hid_a = run("auto", graph, monkey)
        assert ids_b.tolist() == G[:ids_b.numel()].tolist()
        assert torch.equal(ids_a, ids_b) and taus_a == taus_b, f"graph={graph}"
        assert all(_same(a, b) for a, b in zip(hid_a, hid_b)), f"graph={graph}: target_hidden differs"
