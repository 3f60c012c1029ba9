"""eps and pos0 at every OTHER site that normalises a row or rotates a head (tests/test_hip_rows.py launches rows.hip and
prefill.hip directly): one small case per entry point, on rows small enough that eps = 1e-5 decides rstd (a mean
square within a factor 4 of eps; the older tests' unit-scale rows move rstd by a few fp32 ulps) and with the RoPE
position 1000 past the cache row (pos0 = S + 1000, another offset per request in the batch forms; the older tests pass
pos0 = S).  Real norm weights, the real theta = 1e6 tables, tests/rows_ref.py as the reference: appended V rows
bit-equal, K rows per assert_roped, the attention output against fp64 softmax attention over the reference's q / K / V
with the bar of test_hip_batch_kernels._attn_case; normalised fragments per assert_normed; the mode-2 row source with
the bar of test_normed_source_accuracy."""
import pytest
import torch

import attn_keys_ref as A
import helpers as H
import rows_ref as R

pytestmark = pytest.mark.gpu
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
NAN = float("nan")
EPS = 1e-5
AMP = R.small_scale(EPS)
S0, TAU, BS, POS_OFF = 40, 5, 12, 1000
SCALE = 128 ** -0.5


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def dev():
    return torch.device("cuda", 0)


def nans(*shape, dtype=BF16):
    return torch.full(shape, NAN, dtype=dtype, device=dev())


def record(S, tau, bs, pos0):
    return torch.tensor([S, tau, bs, pos0, pos0 + tau, 0, 0, 0], dtype=I32)


def _tables():
    cos, sin = R.tables(2048)
    return cos, sin


def _heads(t, col, nh):
    return t[:, col:col + nh * 128].reshape(t.shape[0], nh, 128)


def small_parts(shape_rows, ld, nparts, g):
    """fp32 K parts whose bf16 sum is a small row (every head's mean square within a factor 4 of EPS)."""
    parts = R.unit((nparts, shape_rows, ld), g, F32) * (AMP / nparts ** 0.5)
    x = R.part_sum(parts).to(BF16)
    R.assert_small(x.reshape(shape_rows, ld // 128, 128), EPS)
    return parts, x


def request_ref(xb, xc, n_q, n_kv, qw, kw, S, tau, bs, pos0, K0, V0, causal):
    """xb [>= bs, ld] the block rows and xc [>= tau, ld] the context rows (bf16, q | k | v columns), K0 / V0 the cache
    before the launch -> the new K / V rows [n_kv, tau + bs, 128] and the block's fp64 attention output [bs, n_q, 128]."""
    cos, sin = _tables()
    qd, kd = n_q * 128, n_kv * 128
    new = xb[:bs] if tau == 0 else torch.cat([xc[:tau], xb[:bs]])
    rel = torch.arange(tau + bs)
    k = R.head_stage(_heads(new, qd, n_kv), None, kw, EPS, pos0 + rel, cos, sin, 2048).transpose(0, 1)
    v = _heads(new, qd + kd, n_kv).transpose(0, 1)
    q = R.head_stage(_heads(xb[:bs], 0, n_q), None, qw, EPS, pos0 + tau + torch.arange(bs), cos, sin, 2048)
    out, _ = A.attention_ref(q, torch.cat([K0[:, :S], k], 1), torch.cat([V0[:, :S], v], 1), A.decode_visibility(S, tau, bs, causal),
                             scale=SCALE)
    return dict(k=k.contiguous(), v=v.contiguous(), out=out)


def check_request(name, ref, k_rows, v_rows, out_frag, n_q, bs):
    R.assert_bits(f"{name} V rows", v_rows, ref["v"])
    R.assert_roped(f"{name} K rows", k_rows, ref["k"])
    got = H.unfrag(out_frag, n_q * 128)[:bs].view(bs, n_q, 128)
    assert torch.isfinite(got.float()).all(), name
    H.assert_close(f"{name} attention output", got, ref["out"], max_rel=2 ** -6, mean_rel=H.MEAN_REL)


def check_untouched(name, c, c0, S, n):
    c, c0 = c.cpu(), c0.cpu()
    assert torch.equal(c[..., :S, :], c0[..., :S, :]) and torch.equal(c[..., S + n:, :], c0[..., S + n:, :]), f"{name}: other cache rows changed"


def caches(n_kv, rows, g, lead=()):
    """Cached K at unit scale (post-norm rows are), cached V at the new rows' scale."""
    return R.unit((*lead, n_kv, rows, 128), g), R.unit((*lead, n_kv, rows, 128), g) * AMP


# ---------------------------------------------------------------- one request
SINGLE = ["attn_fused", "attn_head-immediates", "attn_head-record", "attn_head_oproj", "attn_head_cand"]


@pytest.mark.parametrize("form", SINGLE)
def test_single_request_forms(ops, form):
    oproj, cand = form == "attn_head_oproj", form == "attn_head_cand"
    n_q, n_kv = (8, 2) if oproj else (4, 2)
    S, tau, bs = S0, (0 if cand else TAU), BS
    pos0 = S if cand else S + POS_OFF                     # (dfl_attn_head_cand has no pos0: its rows sit at S ..)
    causal = cand
    g = R.gen(SINGLE.index(form))
    ld, qd, kd = (n_q + 2 * n_kv) * 128, n_q * 128, n_kv * 128
    C = 2 if cand else 1
    parts, x = small_parts(32 * C, ld, 2, g)
    qw, kw = R.head_norm_weight(g), R.head_norm_weight(g)
    rows = S + tau + bs + 8
    K0, V0 = caches(n_kv, rows, g)
    cos, sin = (t.to(dev()) for t in _tables())
    kc, vc = K0.to(dev()), V0.to(dev())
    xd = x.to(dev())
    out = nans(C, 16 * qd)
    norm = dict(n_q=n_q, n_kv=n_kv, q_norm_w=qw.to(dev()), k_norm_w=kw.to(dev()), eps=EPS, cos_tab=cos, sin_tab=sin)
    cols = dict(q_col=0, k_col=qd, v_col=qd + kd)
    dyn = record(S, tau, bs, pos0).to(dev())
    if form == "attn_fused":
        ops.attn_fused(qkv=parts.to(dev()), nsplit=2, split_stride=32 * ld, ld=ld, ctx_row0=0, blk_row0=16, **cols, **norm,
                       kcache=kc, vcache=vc, scale=SCALE, dyn=dyn, kv_len_max=S + tau + bs,
                       ws=ops.attn_fused_ws(n_q, n_kv, 32, dev()), max_splits=32, out_frag=out[0], causal=causal)
    elif form.startswith("attn_head-"):
        rec = form.endswith("record")                     # with a record the immediate pos0 must not be used
        ops.attn_head(xq=xd[16:], xc=xd[:16], ck_col=qd, cv_col=qd + kd, **cols, **norm, kcache=kc, vcache=vc, scale=SCALE,
                      causal=causal, S=S, tau=tau, bs=bs, pos0=0 if rec else pos0, dyn=dyn if rec else None,
                      ws=ops.attn_head_ws(n_q, 8, 1, dev()), max_splits=8, out_frag=out[0])
    elif oproj:
        Hd = 512
        wo = (R.unit((Hd, qd), g, F32) * qd ** -0.5).to(BF16).to(dev())
        h_io = R.unit((16, Hd), g).to(dev())
        sync = torch.zeros(ops.ATTN_OPROJ_SYNC_WORDS, dtype=I32, device=dev())
        ops.attn_head_oproj(xq=xd[16:], xc=xd[:16], ck_col=qd, cv_col=qd + kd, **cols, **norm, kcache=kc, vcache=vc, scale=SCALE,
                            causal=causal, S=S, tau=tau, bs=bs, pos0=pos0, ws=ops.attn_head_ws(n_q, 16, 1, dev()), max_splits=16,
                            attn_frag=out[0], wo=ops.pack_weight(wo), H=Hd, h_io=h_io,
                            ss_out=torch.zeros(Hd, dtype=F32, device=dev()), sync=sync)
        torch.cuda.synchronize()
        assert int(sync.abs().sum()) == 0
    else:
        k_out, v_out = nans(C, n_kv, 16, 128), nans(C, n_kv, 16, 128)
        xq = xd.view(C, 32, ld)[:, 16:].contiguous()
        ops.attn_head_cand(xq=xq, **cols, **norm, kcache=kc, vcache=vc, scale=SCALE, S=S, bs=bs,
                           ws=ops.attn_head_batch_ws(C, n_q, 16, dev()), max_splits=16, out_frag=out, k_out=k_out, v_out=v_out)
    torch.cuda.synchronize()
    for c in range(C):
        xb, xc = x.view(C, 32, ld)[c, 16:], x.view(C, 32, ld)[c, :16]
        ref = request_ref(xb, xc, n_q, n_kv, qw, kw, S, tau, bs, pos0, K0, V0, causal)
        if cand:                                          # the staging rows; the shared cache is read-only
            check_request(f"{form} c{c}", ref, k_out[c, :, :bs], v_out[c, :, :bs], out[c], n_q, bs)
        else:
            check_request(form, ref, kc[:, S:S + tau + bs], vc[:, S:S + tau + bs], out[c], n_q, bs)
    n_new = 0 if cand else tau + bs
    check_untouched(form, kc, K0, S, n_new)
    check_untouched(form, vc, V0, S, n_new)


# ---------------------------------------------------------------- the ragged batch
BATCH = ["attn_head_batch", "attn_head_batch_f32", "attn_fused_batch"]
LENS, BSS = (40, 23, 57), (12, 16, 5)


@pytest.mark.parametrize("form", BATCH)
def test_batch_forms(ops, form):
    """Three requests, four slots, the second layer of two; request r rotates at S_r + 1000 + 37 r."""
    n_q, n_kv, Rq, QS, L, layer, rows = 4, 2, 3, 4, 2, 1, 100
    causal = form != "attn_head_batch_f32"
    ld, qd, kd = (n_q + 2 * n_kv) * 128, n_q * 128, n_kv * 128
    g = R.gen(50 + BATCH.index(form))
    nparts = 1 if form == "attn_head_batch" else 2
    parts, x = small_parts(QS * 16, ld, nparts, g)
    qw, kw = R.head_norm_weight(g), R.head_norm_weight(g)
    K0, V0 = caches(n_kv, rows, g, lead=(QS, L))
    kc, vc = K0.to(dev()), V0.to(dev())
    cos, sin = (t.to(dev()) for t in _tables())
    pos0 = [LENS[r] + POS_OFF + 37 * r for r in range(Rq)]
    dyn = torch.zeros(QS, 8, dtype=I32)
    for r in range(Rq):
        dyn[r] = record(LENS[r], 0, BSS[r], pos0[r])
    out = nans(QS, 16 * qd)
    common = dict(q_col=0, k_col=qd, v_col=qd + kd, R=Rq, n_q=n_q, n_kv=n_kv, q_norm_w=qw.to(dev()), k_norm_w=kw.to(dev()), eps=EPS,
                  cos_tab=cos, sin_tab=sin, kcache=kc, vcache=vc, layer=layer, scale=SCALE, causal=causal, dyn=dyn.to(dev()),
                  kv_len_max=max(LENS) + 16, max_splits=32, out_frag=out)
    if form == "attn_head_batch":
        ops.attn_head_batch(xq=x.view(QS, 16, ld).to(dev()), ws=ops.attn_head_batch_ws(QS, n_q, 32, dev()), **common)
    elif form == "attn_head_batch_f32":
        ops.attn_head_batch_f32(qkv_parts=parts.to(dev()), nparts=nparts, MT=QS, ld=ld, ws=ops.attn_head_batch_ws(QS, n_q, 32, dev()),
                                **common)
    else:
        ops.attn_fused_batch(qkv=parts.to(dev()), nsplit=nparts, split_stride=QS * 16 * ld, ld=ld,
                             ws=ops.attn_fused_batch_ws(QS, n_q, n_kv, 32, dev()), **common)
    torch.cuda.synchronize()
    want_k, want_v = K0.clone(), V0.clone()
    for r in range(Rq):
        S, bs = LENS[r], BSS[r]
        ref = request_ref(x.view(QS, 16, ld)[r], None, n_q, n_kv, qw, kw, S, 0, bs, pos0[r], K0[r, layer], V0[r, layer], causal)
        check_request(f"{form} r{r}", ref, kc[r, layer, :, S:S + bs], vc[r, layer, :, S:S + bs], out[r], n_q, bs)
        want_k[r, layer, :, S:S + bs] = kc[r, layer, :, S:S + bs].cpu()
        want_v[r, layer, :, S:S + bs] = ref["v"]
    assert torch.equal(kc.cpu(), want_k) and torch.equal(vc.cpu(), want_v), "rows outside [S, S + bs), the other layer or the spare slot changed"


def test_kv_append_batch(ops):
    """Three tiles, two layers; tile t appends tau_t context rows at cache rows S_t .. rotated at pos0_t + i != S_t + i."""
    n_kv, L, T, rows = 2, 2, 3, 100
    kd = n_kv * 128
    ld = L * 2 * kd
    g = R.gen(70)
    parts, x = small_parts(T * 16, ld, 2, g)
    kw = torch.stack([R.head_norm_weight(g) for _ in range(L)])
    K0, V0 = caches(n_kv, rows, g, lead=(4, L))
    kc, vc = K0.to(dev()), V0.to(dev())
    cos, sin = _tables()
    tiles = [(40, 16, 40 + POS_OFF), (23, 7, 23 + POS_OFF + 37), (57, 1, 57 + POS_OFF + 74)]
    dyn = torch.stack([record(S, tau, 0, p0) for S, tau, p0 in tiles])
    ops.kv_append_batch(kv=parts.to(dev()), nsplit=2, split_stride=T * 16 * ld, ld=ld, k_col=0, v_col=kd, col_layer_stride=2 * kd,
                        n_layers=L, R=T, n_kv=n_kv, k_norm_w=kw.to(dev()), eps=EPS, cos_tab=cos.to(dev()), sin_tab=sin.to(dev()),
                        kcache=kc, vcache=vc, dyn=dyn.to(dev()))
    torch.cuda.synchronize()
    want_k, want_v = K0.clone(), V0.clone()
    for t, (S, tau, p0) in enumerate(tiles):
        for ly in range(L):
            new = x[t * 16:t * 16 + tau, ly * 2 * kd:(ly + 1) * 2 * kd]
            k = R.head_stage(_heads(new, 0, n_kv), None, kw[ly], EPS, p0 + torch.arange(tau), cos, sin, 2048).transpose(0, 1)
            R.assert_roped(f"kv_append_batch tile {t} layer {ly} K rows", kc[t, ly, :, S:S + tau], k.contiguous())
            want_k[t, ly, :, S:S + tau] = kc[t, ly, :, S:S + tau].cpu()
            want_v[t, ly, :, S:S + tau] = _heads(new, kd, n_kv).transpose(0, 1)
    R.assert_bits("kv_append_batch V rows and every other row", vc, want_v)
    assert torch.equal(kc.cpu(), want_k), "a K row outside the appended ones changed"


# ---------------------------------------------------------------- norm only
def small_rows(shape, g):
    h = R.bounded(shape, g).to(BF16) * AMP
    R.assert_small(h, EPS)
    return h


def test_norm_frag_batch(ops):
    Rq, Hd = 3, 1024
    MT = ops.batch_tiles(Rq)
    g = R.gen(80)
    h, w = small_rows((MT, 16, Hd), g), R.norm_weight(Hd, g)
    valid = [16, 9, 2]
    dyn = torch.zeros(MT, 8, dtype=I32)
    for r, nv in enumerate(valid):
        dyn[r, 2] = nv
    xn = nans(MT, 16 * Hd)
    hd = h.to(dev())
    ops.norm_frag_batch(hd, Rq, w.to(dev()), EPS, xn, dyn.to(dev()), ops.DYN_BS)
    torch.cuda.synchronize()
    for r, nv in enumerate(valid):
        want = torch.zeros(16, Hd, dtype=BF16)
        want[:nv] = R.rms(h[r, :nv], w, EPS)
        R.assert_normed(f"norm_frag_batch r{r}", H.unfrag(xn[r], Hd), want)
    assert torch.equal(hd.cpu(), h)


def test_moe_router_norm(ops):
    K, E, top_k, rows = 512, 16, 4, 11
    g = R.gen(81)
    h, w = small_rows((16, K), g), R.norm_weight(K, g)
    rw = (R.unit((E, K), g, F32) * 0.3).to(BF16)
    xn = nans(16 * K)
    ticket = torch.zeros(1, dtype=I32, device=dev())
    dyn = record(0, 0, rows, 0).to(dev())
    ops.moe_router(h=h.to(dev()), norm_w=w.to(dev()), eps=EPS, xn=xn, wp_router=ops.pack_weight(rw.to(dev())), K=K, E=E, top_k=top_k,
                   norm_topk=True, rlog=torch.zeros(16, E, dtype=BF16, device=dev()), wt=torch.zeros(16, E, dtype=BF16, device=dev()),
                   active=torch.zeros(E, dtype=I32, device=dev()), lst=torch.full((E,), -1, dtype=I32, device=dev()),
                   n_active=torch.zeros(1, dtype=I32, device=dev()), ticket=ticket, dyn=dyn, dyn_word=ops.DYN_BS)
    torch.cuda.synchronize()
    assert int(ticket) == 0
    want = torch.zeros(16, K, dtype=BF16)
    want[:rows] = R.rms(h[:rows], w, EPS)
    R.assert_normed("moe_router normalised rows", H.unfrag(xn, K), want)


@pytest.mark.parametrize("entry", ["gemm_f32", "gemm_resid"])
@pytest.mark.parametrize("K,nss", [(512, 1), (4096, 256)], ids=["K512-nss1", "K4096-nss256"])
def test_mode2_row_source(ops, entry, K, nss):
    """The RMSNorm in a skinny GEMM's prologue (dfl_rows mode 2) on small rows: the bar of test_normed_source_accuracy,
    against the reference's normalised rows times the weights in fp64 (rounded once for the bf16 epilogue)."""
    N, nv = 64, 13
    g = R.gen(K + nss)
    h, nw = small_rows((16, K), g), R.norm_weight(K, g)
    w = (R.unit((N, K), g, F32) * 0.03).to(BF16)
    hd = h.to(dev())
    ss = hd.float().pow(2).view(16, nss, K // nss).sum(-1).T.contiguous().view(-1)
    dyn = record(0, nv, nv, 0).to(dev())
    src = ops.rows_normed(hd, ss, nss, nw.to(dev()), EPS, ops.DYN_BS)
    wp = ops.pack_weight(w.to(dev()))
    ref = R.rms(h[:nv], nw, EPS).double() @ w.double().T
    if entry == "gemm_f32":
        out = nans(16, N, dtype=F32)
        ops.gemm_f32(wp, src, None, 1, N, K, 1, out, dyn)
    else:
        out = nans(16, N)
        ops.gemm_resid(wp, src, N, K, out, add_residual=False, dyn=dyn)
        ref = ref.to(BF16).double()
    torch.cuda.synchronize()
    d = (out[:nv].cpu().double() - ref).abs()
    scale = float(ref.abs().max())
    mx, mn = float(d.max()) / scale, float(d.mean()) / scale
    print(f"[parity] mode-2 {entry} K{K} nss{nss}: max {mx:.3e} mean {mn:.3e} of scale {scale:.3g}")
    H._log_parity({"what": f"mode-2 {entry} K{K} nss{nss}", "max_rel": mx, "mean_rel": mn, "scale": scale})
    assert mx <= 2e-2 and mn <= 1e-3
    assert mn <= 2e-5
