"""The 13-bit expert gate/up stream on the GPU (dfl_moe_gate_up on DFL_W_BF16X13, DESIGN.md section 11, "The experts"):
ops.moe_gate_up over the twin of an MoE layer's expert-tall matrix against the packed bf16 tensor of the SAME weights in
the same build, bit for bit — the decode rebuilds the same fragments, so no tolerance applies — on matrices with a base
per tile and planted patches (tests/bf16x13_expert_cases.py; their CPU account: tests/test_bf16x13_experts_cpu.py), read
under random rows and ALONE under one-hot rows; and a small sparse-MoE target whose decode session and ragged batch do
not depend on stream_format, with a layer the packer refused among them."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16, I32 = torch.bfloat16, torch.int32
K = 2048
POISON = 0x7fa5          # a NaN no kernel produces: what the launch must leave in the experts outside its list
_C = {}


def dev():
    return torch.device("cuda", 0)


def _case(name, extreme=False):
    """name -> (case, packed bf16 [E, 2I*K], its 13-bit twin): built once, shared, never written to."""
    if (name, extreme) not in _C:
        import bf16x13_expert_cases as XE
        from dflash_amd import ops
        case = XE.expert_case(name, extreme=extreme, device=dev())
        wp = torch.stack([ops.pack_weight_gateup(g, u) for g, u in XE.split_experts(case)])
        N = case.E * 2 * case.I
        w13, rep = ops.pack_weight_bf16x13(wp, N, K)
        assert w13 is not None and rep["refused"] == 0 and rep["patched"] == len(case.patches), rep
        meta = w13.data[N // 16 * (K // 128) * ops.X13_QUAD_BYTES:].view(I32).view(N // 16, 16, 2)
        assert torch.unique(meta[:, 0, 0]).numel() >= 5
        _C[name, extreme] = (case, wp, w13)
    return _C[name, extreme]


def _frag(rows):
    from dflash_amd import ops
    frag = torch.empty(16 * K, dtype=BF16, device=dev())
    ops.pack_rows(rows, 16, frag)
    return frag


def _gate_up(mat, frag, case, nv=16):
    """act [E, 16 I] (poisoned first) of one launch over case.lst; nv < 16: that many valid rows through the record."""
    from dflash_amd import ops
    act = torch.full((case.E, 16 * case.I), POISON, dtype=torch.int16, device=dev()).view(BF16)
    lst = torch.zeros(case.E, dtype=I32, device=dev())
    lst[:len(case.lst)] = torch.tensor(case.lst, dtype=I32)
    n = torch.tensor([len(case.lst)], dtype=I32, device=dev())
    dyn, word = None, -1
    if nv < 16:
        dyn, word = torch.zeros(8, dtype=I32, device=dev()), ops.DYN_BS
        dyn[word] = nv
    ops.moe_gate_up(mat, frag, case.E, case.I, K, act, lst, n, dyn=dyn, valid_word=word)
    torch.cuda.synchronize()
    return act.view(torch.int16)


def _rows_of(act, case):
    """[E, 16 I] frag16 per expert -> [E, 16 rows, I]."""
    return act.view(case.E, case.I // 8, 16, 8).permute(0, 2, 1, 3).reshape(case.E, 16, case.I)


@pytest.mark.parametrize("nv", [16, 1, 5])
@pytest.mark.parametrize("name", ["few", "second", "third"])
def test_gate_up_equals_the_bf16_launch(name, nv):
    """8 items: most workgroups leave at once, the B request of the others is a dead item; 280 items over a scrambled
    list: workgroups 0..23 consume B; 528: workgroups 0..15 take a third item back in buffer A and every workgroup's last
    `it + 2G` request is dead.  All of `act` is compared: the experts outside the list keep their poison."""
    case, wp, w13 = _case(name)
    g = torch.Generator(device=dev()).manual_seed(70 + nv)
    frag = _frag(torch.randn(16, K, generator=g, device=dev()).to(BF16))
    want, got = _gate_up(wp, frag, case, nv), _gate_up(w13, frag, case, nv)
    on = torch.zeros(case.E, dtype=torch.bool, device=dev())
    on[torch.tensor(case.lst, device=dev())] = True
    assert (want[~on] == POISON).all() and (want[on] != POISON).all()
    live = _rows_of(want, case)[on][:, :nv].view(BF16).float()
    assert torch.isfinite(live).all() and live.abs().max() > 0
    assert (_rows_of(want, case)[on][:, nv:] == 0).all()             # rows beyond the valid count: silu(0) * 0
    bad = (got != want).nonzero()
    assert bad.numel() == 0, (f"{bad.shape[0]} of {want.numel()} act values differ from the bf16 launch's; the first: expert "
                              f"{int(bad[0, 0])}, element {int(bad[0, 1])}")


@pytest.mark.parametrize("name,extreme", [("second", True), ("third", False)])
def test_gate_up_of_one_hot_rows_keeps_every_patch(name, extreme):
    """Row m of the source is e_k: g and u of act[e][m, i] = bf16(bf16(silu(g)) * u) are the single weights gate_e[i, k]
    and up_e[i, k].  Bit for bit the bf16 launch's over all of `act`; and where g or u is a PATCHED element — one that
    decodes to 0 if its patch word is dropped, or is planted elsewhere if the wrong pair is read — act is nonzero, has the
    sign of silu(g) * u and lies within 2^-6 of it (fp64, from the weights: three bf16 roundings of at most 2^-9 each
    and __expf next to 0).  "second" with the extreme tiles: base 112 and a tile 100 binades down are decoded too."""
    import bf16x13_expert_cases as XE
    case, wp, w13 = _case(name, extreme)
    cols = XE.probe_columns(case)
    pts = XE.probe_points(case)
    assert {q[2] for q in pts} <= set(cols)
    seen = 0
    for c0 in range(0, len(cols), 16):
        ck = cols[c0:c0 + 16]
        rows = torch.zeros(16, K, dtype=BF16, device=dev())
        rows[torch.arange(16, device=dev()), torch.tensor(ck, device=dev())] = 1.0
        frag = _frag(rows)
        want, got = _gate_up(wp, frag, case), _gate_up(w13, frag, case)
        same = torch.equal(got, want)
        here = [(ck.index(k), e, i, gr, ur) for e, i, k, gr, ur in pts if k in ck]
        if here:
            m, e, i, gr, ur = (torch.tensor(v, device=dev()) for v in zip(*here))
            k = torch.tensor(ck, device=dev())[m]
            gw, uw = case.w[gr, k].double(), case.w[ur, k].double()
            ref = gw / (1 + torch.exp(-gw)) * uw
            assert (ref != 0).all()
            for form, act in (("bf16", want), ("13-bit", got)):
                a16 = _rows_of(act, case)[e, m, i]
                a = a16.view(BF16).double()
                assert ((a16 & 0x7f80) != 0).all() and (torch.sign(a) == torch.sign(ref)).all(), \
                    f"{form} form, columns {ck}: a patched element was read as 0"
                assert ((a - ref).abs() <= 2.0 ** -6 * ref.abs()).all(), (form, float(((a - ref).abs() / ref.abs()).max()))
            assert torch.equal(_rows_of(got, case)[e, m, i], _rows_of(want, case)[e, m, i]), f"columns {ck}: patched positions"
            seen += len(here)
        assert same, f"columns {ck}: the 13-bit form differs from the bf16 launch"
    assert seen == len(case.patches)


# ------------------------------------------------------------------------------------------------ the model
def _moe_hf(hidden=2048, layers=3, E=8, top_k=2, Ie=64, mlp_only=(1,), heads=16, kv=2, seed=51, shifts=True):
    """tests/test_hip_moe.py::_moe_hf at hidden 2048: MoE, dense, MoE; every expert's gate/up with a base per tile
    (bf16x13_cases.apply_tile_shifts; the down columns undo the powers)."""
    import bf16x13_cases as X
    tf = pytest.importorskip("transformers")
    cfg = tf.Qwen3MoeConfig(vocab_size=2048, hidden_size=hidden, intermediate_size=2 * hidden, moe_intermediate_size=Ie,
                            num_hidden_layers=layers, num_attention_heads=heads, num_key_value_heads=kv, head_dim=128,
                            num_experts=E, num_experts_per_tok=top_k, decoder_sparse_step=1, norm_topk_prob=True,
                            max_position_embeddings=4096, rms_norm_eps=1e-6, tie_word_embeddings=False,
                            rope_parameters={"rope_type": "default", "rope_theta": 1e6}, mlp_only_layers=list(mlp_only))
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(BF16)
    try:
        with torch.device(dev()):
            m = tf.Qwen3MoeForCausalLM(cfg)
    finally:
        torch.set_default_dtype(prev)
    with torch.no_grad():
        for layer in m.model.layers:
            if hasattr(layer.mlp, "gate"):
                layer.mlp.gate.weight.mul_(8.0)      # (the default init leaves the router nearly flat)
                if shifts:
                    gup, dwn = layer.mlp.experts.gate_up_proj.data, layer.mlp.experts.down_proj.data
                    for e in range(E):
                        X.apply_tile_shifts(gup[e, :Ie], gup[e, Ie:], dwn[e])
    return m.eval()


def _spy(monkeypatch, log):
    """ops.moe_gate_up -> log of "did it get a 13-bit twin"."""
    from dflash_amd import ops
    real = ops.moe_gate_up

    def wrapped(w, *a, **kw):
        log.append(isinstance(w, ops.Bf16x13Weight))
        return real(w, *a, **kw)
    monkeypatch.setattr(ops, "moe_gate_up", wrapped)


def _hook_for(G, plan, vocab=2000):
    def hook(blk, start, call):
        k = min(plan[call % len(plan)], blk.shape[1] - 1)
        blk[0, 1:k + 1] = G[start + 1:start + k + 1]
        if k + 1 < blk.shape[1]:
            blk[0, k + 1] = (G[start + k + 1] + 1) % vocab
    return hook


def test_target_builds_the_twins_where_the_pair_kernel_streams_them(monkeypatch):
    """stream_format="auto" with the kind switched on: a twin per MoE layer at hidden 2048 and bf16 experts — none under
    "bf16", with fp8 experts, at hidden 512 or with the kind off — and expert_weights hands it out only while the pair
    kernel runs; the packed copy stays resident either way."""
    from dflash_amd import NativeTarget, ops
    monkeypatch.setitem(ops.X13_KINDS, "experts_gateup", True)
    hf = _moe_hf(shifts=False)
    nt = NativeTarget(hf)
    for i, lw in enumerate(nt.layers):
        assert ("gu_e13" in lw) == (i != 1) == ("gu_e" in lw)
    lw = nt.layers[0]
    twin = lw["gu_e13"]
    assert isinstance(twin, ops.Bf16x13Weight) and (twin.N, twin.K) == (8 * 2 * 64, 2048)
    assert twin is ops.bf16x13_twin(lw["gu_e"], 8 * 2 * 64, 2048, "experts_gateup")       # one per packed tensor, in the registry
    gw, dw = nt.expert_weights(lw)
    assert gw is twin and dw is lw["down_e"]
    nt.moe_pair_kernel = False
    assert nt.expert_weights(lw)[0] is lw["gu_e"]
    nt.moe_pair_kernel = True
    rep = ops.bf16x13_report()
    assert rep["packed"] >= 3 and isinstance(nt.gu13[1], ops.Bf16x13Weight)               # two expert matrices and the dense layer
    assert not any("gu_e13" in lw for lw in NativeTarget(hf, stream_format="bf16").layers)
    nt8 = NativeTarget(_moe_hf(shifts=False), expert_format="fp8_e4m3")
    assert not any("gu_e13" in lw for lw in nt8.layers) and "gu_e8" in nt8.layers[0]
    small = NativeTarget(_moe_hf(hidden=512, heads=4, shifts=False))
    assert not any("gu_e13" in lw for lw in small.layers)
    monkeypatch.setitem(ops.X13_KINDS, "experts_gateup", False)
    assert not any("gu_e13" in lw for lw in NativeTarget(hf).layers)


@pytest.mark.parametrize("refused", [False, True])
def test_moe_session_and_batch_do_not_depend_on_the_stream_format(refused, monkeypatch):
    """A sparse-MoE target at hidden 2048 (MoE, dense, MoE; 8 experts, top-2, moe_intermediate 64), stream_format="auto"
    against "bf16", eager and by graph replay: a decode session commits the same ids, acceptance lengths and tapped
    hidden rows, and a two-request engine whose expert branch is the per-tile one commits the same ids — with the twins
    streamed in the first arm (the spy) and never in the second.  refused: layer 2's matrix has two below-window elements
    in one (tile, wave) item, so that layer streams plain bf16 behind a layer that streams its twin."""
    import bf16x13_cases as X
    from dflash_amd import DFlashDraftModel, NativeTarget, ops
    from dflash_amd.config import DFlashConfig
    from dflash_amd.engine import BatchEngine
    from dflash_amd.generate import DecodeSession
    from dflash_amd.synthetic import greedy_walk, impose_greedy_walk
    monkeypatch.setitem(ops.X13_KINDS, "experts_gateup", True)
    cfg = DFlashConfig(hidden_size=2048, num_hidden_layers=1, num_attention_heads=16, num_key_value_heads=2, head_dim=128,
                       intermediate_size=2176, vocab_size=2048, num_target_layers=3, block_size=16, rope_theta=1e6,
                       mask_token_id=2047)
    hf = _moe_hf()
    if refused:   # expert 3's gate rows 16..31: packed tile 2 of that expert
        X.plant_refusal(hf.model.layers[2].mlp.experts.gate_up_proj.data[3], 1, 5)
    perm = impose_greedy_walk(hf, seed=9)
    prompts = [torch.randint(0, 2000, (1, P), generator=torch.Generator().manual_seed(4 + P)).to(dev()) for P in (23, 38)]
    n_new = 16 * 8
    Gs = [greedy_walk(perm, p, n_new + 40).to(dev()) for p in prompts]
    plan = [0, 15, 3, 9, 1, 12, 5, 7]
    sd = H.draft_weights(cfg, seed=5, dtype=BF16)
    log = []
    _spy(monkeypatch, log)

    def build(fmt):
        m = DFlashDraftModel(cfg, device=dev(), stream_format=fmt).load_state_dict(sd)
        nt = NativeTarget(hf, stream_format=fmt)
        want = [fmt == "auto", False, fmt == "auto" and not refused]
        assert ["gu_e13" in lw for lw in nt.layers] == want
        return m, nt

    def session(fmt, graph):
        m, nt = build(fmt)
        s = DecodeSession(m, nt, prompts[0], mask_token_id=cfg.mask_token_id, max_new_tokens=n_new, max_block_size=16,
                          stop_token_ids=None, temperature=0.0, draft_token_hook=_hook_for(Gs[0], plan))
        s.prefill()
        del log[:]
        hidden, taus = [], []
        for i in range(6):
            if graph and i == 2:
                s.capture(16)
            r = s.cycle_graph(16) if graph and i >= 2 else s.cycle(16, ahead_ok=True)
            taus.append(r.tau)
            hidden.append(s.target_hidden.clone())
        torch.cuda.synchronize()
        assert log and log.count(True) == (len(log) // 2 * (2 - refused) if fmt == "auto" else 0), (fmt, graph, log)
        return s.output_ids[0, :s.start + 1].clone(), taus, hidden

    def batch(fmt, graph):
        m, nt = build(fmt)
        nt.moe_shared_pass = False            # two tiles: each routes and streams its own experts (the per-tile branch)
        eng = BatchEngine(m, nt, slots=2, max_rows=38 + 60 + 48, out_len=38 + 60 + 16, mask_token_id=cfg.mask_token_id,
                          graph=graph)
        for i, p in enumerate(prompts):
            eng.submit(p, 60, draft_token_hook=_hook_for(Gs[i], plan[i:] + plan[:i]))
        del log[:]
        res = eng.run()
        assert (eng.stats["replayed_cycles"] > 0) == graph
        assert log and log.count(True) == (len(log) // 2 * (2 - refused) if fmt == "auto" else 0), (fmt, graph)
        return [r.output_ids[0].tolist() for r in res], [r.acceptance_lengths for r in res]

    for graph in (False, True):
        ids_b, taus_b, hid_b = session("bf16", graph)
        ids_a, taus_a, hid_a = session("auto", graph)
        assert ids_b.tolist() == Gs[0][:ids_b.numel()].tolist() and max(taus_b) > 8
        assert torch.equal(ids_a, ids_b) and taus_a == taus_b, f"graph={graph}"
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(hid_a, hid_b)), \
            f"graph={graph}: target_hidden differs"
        out_b, acc_b = batch("bf16", graph)
        out_a, acc_a = batch("auto", graph)
        assert out_b == [Gs[i][:prompts[i].shape[1] + 60].tolist() for i in range(2)]
        assert out_a == out_b and acc_a == acc_b, f"graph={graph}"
