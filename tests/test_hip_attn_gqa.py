"""Every attention entry point across GQA group sizes G = n_q / n_kv, key by key against fp64: the census, needle and leak
inputs of attn_keys_ref through the helpers of test_hip_attn_keys, at the case tables of attn_gqa_cases (asserted without
a GPU in test_attn_keys_cpu.py).  The older key-by-key tests run G = 2 and G = 4 (and G = 1, 2, 8 with ONE kv head,
where kvh * G is 0 whatever G is); here every case has n_kv >= 2 and G runs over 1, 3, 5, 6, 7, 8, 16 — what a
40 / 8, 24 / 8, 64 / 8 or 64 / 4 model puts through hpg / hh / split / head of attn_head_body, the pair rule and the
workgroup budget of attn_head_launch, the b % n_kv decode of k_attn_oproj, hq and head / G of dfl_prefill_attn and the
G-wave workgroup of k_block_attn.

A wrong kv head is invisible to the census (its V is the same in every kv head: test_attn_keys_cpu.
test_needle_sees_a_wrong_kv_head_and_the_census_cannot), so every case runs the needle launches too, and every needle
launch probes every query head.  Bars: attn_keys_ref's own (census within one bf16 step, needle bit-equal, leak 2^-6 of
scale; 1e-2 for the prefill kernel, as test_hip_attn_keys).  The row stages that carry head counts run at the same odd
groups against rows_ref at its bars."""
import pytest
import torch

import attn_gqa_cases as C
import attn_keys_ref as R
import helpers as H
import rows_ref as RR
import test_hip_attn_keys as K

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")
dev = K.dev
CAUSAL = pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])


def _hid(h):
    return f"G{h[0] // h[1]}-({h[0]},{h[1]})"


# ---------------------------------------------------------------- dfl_attn_head
@CAUSAL
@pytest.mark.parametrize("case", C.HEAD_CASES, ids=[C.head_id(c) for c in C.HEAD_CASES])
def test_attn_head_gqa(case, causal):
    """dfl_attn_head with the lengths as immediates and from the record: G = 1 .. 16 at 33 and 1041 cached keys; ~5300 keys
    on k_attn_head_pair with three (G = 6) and four (G = 8) workgroups per kv head and split, and on k_attn_head with the
    four splits the budget leaves 40 heads (six tiles per wave); two query tiles at G = 5 and 6."""
    K.test_attn_head_keys(case, causal)


# ---------------------------------------------------------------- the ragged-batch forms
@CAUSAL
@pytest.mark.parametrize("name", list(C.BATCH_CASES), ids=[C.batch_id(n) for n in C.BATCH_CASES])
def test_attn_batch_gqa(name, causal):
    """dfl_attn_head_batch_f32 / dfl_attn_head_batch at G = 3, 5, 6: R = 2 and R = 4 ragged requests, one of them at
    S = 0; R = 4 of G = 6 reaches k_attn_head_pair through n_cand > 2 with three workgroups per kv head; R = 4 requests of
    (40, 8) floor the budget at one split."""
    from dflash_amd import ops
    form, (n_q, n_kv), lens, bss, rows = C.BATCH_CASES[name]
    R_, QS = len(lens), 4
    qd, kd = n_q * 128, n_kv * 128
    ld = qd + 2 * kd
    t = K.Tally(f"attn {C.batch_id(name)} ({n_q},{n_kv}) {'causal' if causal else 'full'}")
    cos, sin = K._tables(2048)
    ws = ops.attn_head_batch_ws(QS, n_q, 32, dev())
    for ps in K._request_sets(lens, bss, causal, n_q, n_kv):
        x, kc, vc, dyn = K._batch_inputs(ps, QS, rows)
        out = torch.full((QS, 16 * qd), NAN, dtype=BF16, device=dev())
        common = dict(q_col=0, k_col=qd, v_col=qd + kd, R=R_, n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6,
                      cos_tab=cos, sin_tab=sin, kcache=kc, vcache=vc, layer=K.LAYER, scale=R.SCALE, causal=causal, dyn=dyn,
                      kv_len_max=rows, ws=ws, max_splits=32, out_frag=out)
        if form == "f32":
            ops.attn_head_batch_f32(qkv_parts=K._parts(x.view(QS * 16, ld), 2).to(dev()), nparts=2, MT=QS, ld=ld, **common)
        else:
            ops.attn_head_batch(xq=x.view(QS, 16, ld).to(dev()), q_tiles=1, **common)
        for r, p in enumerate(ps):
            t.check(p, K._rows_out(out[r:r + 1], p), tag=f"r{r} ")
        K._check_batch_caches(ps, kc, vc, t.name)
    t.report()


# ---------------------------------------------------------------- dfl_attn_head_cand
@pytest.mark.parametrize("heads", C.CAND_HEADS, ids=_hid)
def test_attn_head_cand_gqa(heads):
    """dfl_attn_head_cand: C = 4 candidate blocks on one cached prefix of 300 keys (causal); the candidates' query heads are
    rotated inside each kv group, so a head that reads another group's K / V or another head's q shows."""
    from dflash_amd import ops
    (n_q, n_kv), S, bs, Cn, ms = heads, 300, 16, 4, 16
    qd, kd = n_q * 128, n_kv * 128
    t = K.Tally(f"attn_head_cand ({n_q},{n_kv}) S{S} C{Cn} {R.head_form_id(n_q, n_kv, S, bs, ms, n_cand=Cn)}")
    ws = ops.attn_head_batch_ws(Cn, n_q, ms, dev())
    cos, sin = K._tables(2048)
    for p in K._problem_set(S, 0, bs, True, n_q, n_kv):
        ps = [K._variant(p, c) for c in range(Cn)]
        kc, vc = (x.to(dev()) for x in K._caches(p, S + 8))
        kc0, vc0 = kc.clone(), vc.clone()
        xq = torch.stack([K._block_rows(pc) for pc in ps]).to(dev())
        out = torch.full((Cn, 16 * qd), NAN, dtype=BF16, device=dev())
        k_out = torch.full((Cn, n_kv, 16, 128), NAN, dtype=BF16, device=dev())
        v_out = torch.full_like(k_out, NAN)
        ops.attn_head_cand(xq=xq, q_col=0, k_col=qd, v_col=qd + kd, n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6,
                           cos_tab=cos, sin_tab=sin, kcache=kc, vcache=vc, scale=R.SCALE, S=S, bs=bs, ws=ws, max_splits=ms,
                           out_frag=out, k_out=k_out, v_out=v_out)
        assert K._same_bits(kc, kc0) and K._same_bits(vc, vc0), t.name
        for c, pc in enumerate(ps):
            t.check(pc, K._rows_out(out[c], pc), tag=f"c{c} ")
            assert K._same_bits(k_out[c, :, :bs].cpu(), pc.k[:, S:]) and K._same_bits(v_out[c, :, :bs].cpu(), pc.v[:, S:]), (t.name, c)
    t.report()


# ---------------------------------------------------------------- dfl_attn_head_oproj
@CAUSAL
@pytest.mark.parametrize("heads,S,tau", C.OPROJ_CASES, ids=[f"{_hid(h)}-S{S}-tau{tau}" for h, S, tau in C.OPROJ_CASES])
def test_attn_head_oproj_gqa(heads, S, tau, causal):
    """dfl_attn_head_oproj, H = 512: attn_frag key by key (workgroup b is kv head b % n_kv, y = b / n_kv, with
    n_attn = n_kv * G * (splits + 1)); the fail word and every sync word are 0 afterwards."""
    from dflash_amd import ops
    (n_q, n_kv), Hd, bs, ms = heads, 512, 16, 16
    t = K.Tally(f"attn_head_oproj ({n_q},{n_kv}) S{S} tau{tau} {R.head_form_id(n_q, n_kv, S, bs, ms, oproj=True)} "
                f"{'causal' if causal else 'full'}")
    g = H.gen(S + n_q)
    wop = ops.pack_weight((torch.randn(Hd, n_q * 128, generator=g) * (n_q * 128) ** -0.5).to(BF16).to(dev()))
    h0 = torch.randn(16, Hd, generator=g).to(BF16).to(dev())
    ws = ops.attn_head_ws(n_q, ms, 1, dev())
    sync = torch.zeros(ops.ATTN_OPROJ_SYNC_WORDS, dtype=torch.int32, device=dev())
    cos, sin = K._tables(2048)
    for p in K._problem_set(S, tau, bs, causal, n_q, n_kv):
        kc, vc = (x.to(dev()) for x in K._caches(p, p.n_keys + 8))
        out = torch.full((16 * n_q * 128,), NAN, dtype=BF16, device=dev())
        h, ss = h0.clone(), torch.zeros(Hd, dtype=torch.float32, device=dev())
        ops.attn_head_oproj(**K._head_args(p, cos, sin, K._block_rows(p).to(dev()), K._ctx_rows(p).to(dev())), kcache=kc, vcache=vc,
                            S=S, ws=ws, max_splits=ms, attn_frag=out, wo=wop, H=Hd, h_io=h, ss_out=ss, sync=sync)
        assert int(sync[ops.ATTN_OPROJ_FAIL_WORD]) == 0 and int(sync.abs().sum()) == 0, t.name
        t.check(p, K._rows_out(out, p))
        K._check_caches(p, kc, vc, t.name)
    t.report()


# ---------------------------------------------------------------- dfl_block_attn
def _block_launch(p, n_q, n_kv, dyn, ws, max_splits, causal, out):
    from dflash_amd import ops
    kc, vc = K._caches(p, p.n_keys + 40, upto=p.n_keys)
    q = torch.zeros(n_q, 16, 128, dtype=BF16)
    q[:, :p.bs] = p.q.transpose(0, 1)
    ops.block_attn(q=q.to(dev()), kcache=kc.to(dev()), vcache=vc.to(dev()), n_q=n_q, n_kv=n_kv, scale=R.SCALE, dyn=dyn,
                   kv_len_max=p.n_keys, ws=ws, max_splits=max_splits, out_frag=out, causal=causal)


@CAUSAL
@pytest.mark.parametrize("G,S,max_splits", C.BLOCK_CASES, ids=[f"G{g}-S{S}-ms{ms}" for g, S, ms in C.BLOCK_CASES])
def test_block_attn_gqa(G, S, max_splits, causal):
    """dfl_block_attn with a workgroup of G waves (64, 128, 192, 320, 448, 512 threads) per kv head and split, two kv heads:
    the staging loop's stride, head = kvh * G + wave, and the merge."""
    from dflash_amd import ops
    n_q, n_kv = 2 * G, 2
    tau, bs = (0 if causal else 5), (11 if S == 33 else 16)
    t = K.Tally(f"block_attn ({n_q},{n_kv}) S{S} tau{tau} bs{bs} {'causal' if causal else 'full'} ms{max_splits}")
    ws = ops.attn_ws(n_q, max_splits, dev())
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, S, tau, bs, S)
    for p in K._problem_set(S, tau, bs, causal, n_q, n_kv):
        out = torch.full((16 * n_q * 128,), NAN, dtype=BF16, device=dev())
        _block_launch(p, n_q, n_kv, dyn, ws, max_splits, causal, out)
        t.check(p, K._rows_out(out, p))
    t.report()


def test_block_attn_refuses_group_9():
    """G = 9 (more waves than a workgroup holds): the wrapper's error names the group, nothing is launched — the output
    and the workspace, pre-filled with a sentinel, come back whole."""
    from dflash_amd import ops
    n_q, n_kv = C.BLOCK_REFUSED
    S, bs = 33, 16
    p = R.census_problem(S, 0, bs, False, n_q, n_kv, "lane")
    ws = torch.full_like(ops.attn_ws(n_q, 32, dev()), 0x5A)
    dyn = torch.zeros(8, dtype=torch.int32, device=dev())
    ops.set_dyn(dyn, S, 0, bs, S)
    out = torch.full((16 * n_q * 128,), 7.0, dtype=BF16, device=dev())
    with pytest.raises(RuntimeError, match=r"GQA group must be 1\.\.8 \(n_q=18 n_kv=2\)"):
        _block_launch(p, n_q, n_kv, dyn, ws, 32, False, out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all())


# ---------------------------------------------------------------- dfl_attn_fused / dfl_attn_fused_batch
@CAUSAL
@pytest.mark.parametrize("heads,S,tau", C.FUSED_CASES, ids=[f"{_hid(h)}-S{S}-tau{tau}" for h, S, tau in C.FUSED_CASES])
def test_attn_fused_gqa(heads, S, tau, causal):
    """dfl_attn_fused at the groups it takes, with TWO kv heads (G = 1, 2, 8; G = 4 at (8, 2) is test_hip_attn_keys')."""
    K.test_attn_fused_keys(heads[0], heads[1], S, tau, causal)


def _fused_batch_args(ps, n_q, n_kv, QS, rows, causal, out, ws):
    qd, kd = n_q * 128, n_kv * 128
    ld = qd + 2 * kd
    cos, sin = K._tables(2048)
    x, kc, vc, dyn = K._batch_inputs(ps, QS, rows)
    return kc, vc, dict(qkv=K._parts(x.view(QS * 16, ld), 2).to(dev()), nsplit=2, split_stride=QS * 16 * ld, ld=ld, q_col=0,
                        k_col=qd, v_col=qd + kd, R=len(ps), n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6,
                        cos_tab=cos, sin_tab=sin, kcache=kc, vcache=vc, layer=K.LAYER, scale=R.SCALE, causal=causal, dyn=dyn,
                        kv_len_max=rows, ws=ws, max_splits=32, out_frag=out)


@CAUSAL
@pytest.mark.parametrize("heads", C.FUSED_HEADS, ids=_hid)
def test_attn_fused_batch_gqa(heads, causal):
    """dfl_attn_fused_batch, R = 4 ragged requests (one at S = 0), two kv heads, G = 1, 2, 8."""
    from dflash_amd import ops
    (n_q, n_kv), QS, rows = heads, 4, 700
    t = K.Tally(f"attn_fused_batch ({n_q},{n_kv}) R4 {'causal' if causal else 'full'}")
    ws = ops.attn_fused_batch_ws(QS, n_q, n_kv, 32, dev())
    for ps in K._request_sets(C.LENS4, (16, 16, 5, 12), causal, n_q, n_kv):
        out = torch.full((QS, 16 * n_q * 128), NAN, dtype=BF16, device=dev())
        kc, vc, kw = _fused_batch_args(ps, n_q, n_kv, QS, rows, causal, out, ws)
        ops.attn_fused_batch(**kw)
        for r, p in enumerate(ps):
            t.check(p, K._rows_out(out[r:r + 1], p), tag=f"r{r} ")
        K._check_batch_caches(ps, kc, vc, t.name)
    t.report()


@pytest.mark.parametrize("batch", [False, True], ids=["single", "batch"])
@pytest.mark.parametrize("heads", C.FUSED_REFUSED, ids=_hid)
def test_attn_fused_refuses_other_groups(heads, batch):
    """G = 3, 5, 6, 7, 16: refused, dfl_last_error names the group, and nothing ran — outputs, caches and the workspace
    come back bit for bit."""
    from dflash_amd import ops
    n_q, n_kv = heads
    G, S, bs, QS = n_q // n_kv, 40, 16, 4
    qd, kd = n_q * 128, n_kv * 128
    ld = qd + 2 * kd
    p = R.census_problem(S, 0, bs, False, n_q, n_kv, "lane")
    msg = f"GQA group {G} not in \\{{1,2,4,8\\}}"
    if batch:
        ws = torch.full_like(ops.attn_fused_batch_ws(QS, n_q, n_kv, 32, dev()), 0x5A)
        out = torch.full((QS, 16 * qd), 7.0, dtype=BF16, device=dev())
        kc, vc, kw = _fused_batch_args([p, p], n_q, n_kv, QS, 64, False, out, ws)
        kc0, vc0 = kc.clone(), vc.clone()
        with pytest.raises(RuntimeError, match=msg):
            ops.attn_fused_batch(**kw)
    else:
        ws = torch.full_like(ops.attn_fused_ws(n_q, n_kv, 32, dev()), 0x5A)
        out = torch.full((16 * qd,), 7.0, dtype=BF16, device=dev())
        cos, sin = K._tables(2048)
        dyn = torch.zeros(8, dtype=torch.int32, device=dev())
        ops.set_dyn(dyn, S, 0, bs, S)
        kc, vc = (x.to(dev()) for x in K._caches(p, p.n_keys + 8))
        kc0, vc0 = kc.clone(), vc.clone()
        rows = torch.cat([K._ctx_rows(p, 16), K._block_rows(p, 16)])
        with pytest.raises(RuntimeError, match=msg):
            ops.attn_fused(qkv=K._parts(rows, 2).to(dev()), nsplit=2, split_stride=32 * ld, ld=ld, q_col=0, k_col=qd, v_col=qd + kd,
                           ctx_row0=0, blk_row0=16, n_q=n_q, n_kv=n_kv, q_norm_w=None, k_norm_w=None, eps=1e-6, cos_tab=cos,
                           sin_tab=sin, kcache=kc, vcache=vc, scale=R.SCALE, dyn=dyn, kv_len_max=p.n_keys, ws=ws, max_splits=32,
                           out_frag=out, causal=False)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all())
    assert K._same_bits(kc, kc0) and K._same_bits(vc, vc0)


# ---------------------------------------------------------------- dfl_prefill_attn
@pytest.mark.parametrize("P", C.PREFILL_P)
@pytest.mark.parametrize("heads", C.PREFILL_HEADS, ids=[f"{_hid(h)}-hq{C.prefill_form(h)[0]}x{C.prefill_form(h)[1]}" for h in C.PREFILL_HEADS])
def test_prefill_attn_gqa(heads, P):
    """dfl_prefill_attn with more than one workgroup per kv head: hq = 1 at G = 3, 5, 7 (head = blockIdx.x, kv head
    head / G), three workgroups of hq = 2 at G = 6, two and four of hq = 4 at G = 8 and 16."""
    K.test_prefill_attn_keys(heads[0], heads[1], P)


# ---------------------------------------------------------------- the row stages that carry head counts
def _append_cases():
    cs = []
    for heads in C.ROW_HEADS:
        cs += [RR._ap_case(heads, "ctx_blk", 2, "small5", S=301, pos0=17), RR._ap_case(heads, "blk_only", 1, "small6", tau=0, bs=16, pos0=40000),
               RR._ap_case(heads, "kv_ctx", 3, "unit", tau=9, bs=3)]
    for i, c in enumerate(cs):
        c.seed = 600 + i
    return cs


def _prefill_rope_cases():
    cs = [RR._pq_case(P, heads, fam, True, pos0, 9) for heads in C.ROW_HEADS for P, fam, pos0 in ((3, "small5", 40000), (77, "small6", 5))]
    for i, c in enumerate(cs):
        c.seed = 700 + i
    return cs


@pytest.mark.parametrize("c", _append_cases(), ids=lambda c: c.id)
def test_qknorm_rope_append_gqa(c):
    """dfl_qknorm_rope_append (items = 16 n_q + 64 n_kv) at G = 3, 5, 8 with real RoPE tables and q / k norm weights: every
    head's q rows and every cache row against rows_ref, everything else untouched (test_hip_rows.test_qknorm_rope_append)."""
    import test_hip_rows as TR
    from dflash_amd import ops
    TR.test_qknorm_rope_append(ops, c)


@pytest.mark.parametrize("c", _prefill_rope_cases(), ids=lambda c: c.id)
def test_prefill_qk_rope_gqa(c):
    """dfl_prefill_qk_rope (items = P (n_q + 2 n_kv)) at G = 3, 5, 8 (test_hip_rows.test_prefill_qk_rope)."""
    import test_hip_rows as TR
    from dflash_amd import ops
    TR.test_prefill_qk_rope(ops, c)


@pytest.mark.parametrize("n_kv", sorted({h[1] for h in C.ROW_HEADS} | {8}))
def test_kv_append_batch_gqa(n_kv):
    """dfl_kv_append_batch runs the kernel of dfl_qknorm_rope_append without q rows and never sees n_q: (6, 2), (10, 2) and
    (16, 2) are ONE case to it (the kv-only cases above cover that kernel's head decode per geometry), so it runs once per
    kv head count, (40, 8)'s included: 3 layers, R = 3 tiles with their own S, tau and pos0; K rows against
    rows_ref.head_stage, V rows and every other cache row bit for bit."""
    from dflash_amd import ops
    L, T, rows, eps = 3, 3, 64, 1e-5
    kd = n_kv * 128
    ld = L * 2 * kd
    g = RR.gen(800 + n_kv)
    amp = RR.small_scale(eps)
    parts = RR.unit((2, T * 16, ld), g, torch.float32) * (amp / 2 ** 0.5)
    kw = torch.stack([RR.head_norm_weight(g) for _ in range(L)])
    cos, sin = RR.tables(RR.TABLE_ROWS)
    recs = [(20, 16, 39990), (0, 5, 7), (33, 1, 33 + 4)]          # (S, tau, pos0) per tile
    dyn = torch.full((T, 8), 13, dtype=torch.int32)
    for t_, (S, tau, pos0) in enumerate(recs):
        dyn[t_, 0], dyn[t_, 1], dyn[t_, 3] = S, tau, pos0
    kc = torch.full((T, L, n_kv, rows, 128), NAN, dtype=BF16, device=dev())
    vc = torch.full_like(kc, NAN)
    ops.kv_append_batch(kv=parts.to(dev()), nsplit=2, split_stride=T * 16 * ld, ld=ld, k_col=0, v_col=kd, col_layer_stride=2 * kd,
                        n_layers=L, R=T, n_kv=n_kv, k_norm_w=kw.to(dev()), eps=eps, cos_tab=cos.to(dev()), sin_tab=sin.to(dev()),
                        kcache=kc, vcache=vc, dyn=dyn.to(dev()))
    torch.cuda.synchronize()
    x32 = RR.part_sum(parts)
    xb = x32.to(BF16)
    want_k, want_v = torch.full(kc.shape, NAN, dtype=BF16), torch.full(kc.shape, NAN, dtype=BF16)
    for t_, (S, tau, pos0) in enumerate(recs):
        for ly in range(L):
            c0 = ly * 2 * kd
            xk = xb[t_ * 16:t_ * 16 + tau, c0:c0 + kd].reshape(tau, n_kv, 128)
            RR.assert_small(xk, eps, f"tile {t_} layer {ly}")
            k = RR.head_stage(xk, None, kw[ly], eps, pos0 + torch.arange(tau), cos, sin, RR.TABLE_ROWS)
            want_k[t_, ly, :, S:S + tau] = k.transpose(0, 1)
            want_v[t_, ly, :, S:S + tau] = xb[t_ * 16:t_ * 16 + tau, c0 + kd:c0 + 2 * kd].reshape(tau, n_kv, 128).transpose(0, 1)
    RR.assert_roped(f"kv_append_batch n_kv={n_kv} K", kc, want_k)
    RR.assert_bits(f"kv_append_batch n_kv={n_kv} V and every other row", vc, want_v)
