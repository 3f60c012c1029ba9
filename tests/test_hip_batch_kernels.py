"""The ragged-batch kernels at the forms the batch runs by default, each against a plain fp32 torch / oracle reference:
the ring GEMMs (dfl_k_gemm_r: gate/up + SiLU*up, lm_head + argmax) from frag16 sources, the attention stage of the draft
and the target verify (dfl_attn_head_batch_f32 / dfl_attn_head_batch), and the context K/V append (dfl_kv_append_batch).

Every kernel picks its instantiation on the host from the shapes, so the shapes below are chosen by the host rules
(ring_plan and the w16 rule in gemm_batch.hip, the pair rule in attn_head.hip), mirrored here to name the form each case
reaches in its test id."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


def dev():
    return torch.device("cuda", 0)


def _cuda_gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _small_ints(shape, g):
    """bf16 integers in [-2, 2] drawn on the device: every product and every fp32 sum of up to 2^22 of them is exact."""
    return torch.randint(-2, 3, shape, generator=g, device=dev(), dtype=torch.int8).to(BF16)


def _bf16_ulps(a, b):
    """Distance in bf16 steps between two bf16 tensors (the bit patterns mapped onto a monotonic integer line)."""
    def line(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


# ---------------------------------------------------------------- ring GEMMs: host rules of gemm_batch.hip
def _ring_plan(nunits, upp_max):
    """ring_plan(): workgroups, units per workgroup and pass, passes."""
    gx = min(nunits, 256)
    per_wg = -(-nunits // gx)
    npass = -(-per_wg // upp_max)
    return gx, -(-per_wg // npass), npass


def _silu_form(R, I):
    per_wg = (I // 16 + 255) // 256
    w16 = per_wg % 4 == 0 or per_wg > 6
    gx, upp, npass = _ring_plan(I // 16, 4 if w16 else 3)
    MT = 2 if R <= 2 else 4
    return dict(MT=MT, NW=16 if w16 else 12, A=3 if MT == 2 else 2, gx=gx, upp=upp, npass=npass)


def _argmax_form(R, V):
    gx, upp, npass = _ring_plan(V // 16, 16)
    return dict(MT=2 if R <= 2 else 4, NW=16, A=2, gx=gx, upp=upp, npass=npass)


def _form_id(f, tpu, kq):
    return f"r<{f['MT']},{tpu},{kq},{f['NW']},{f['A']}>-gx{f['gx']}-upp{f['upp']}-npass{f['npass']}"


# (R, I, K): all four gate/up launch forms (MT 2 / 4 x 12 / 16 waves), upp 1..4, two passes, the bench point, Llama's
# I = 14336 (tail workgroups with 3 of 4 units), hidden 5120 (a group of one), K with a partial last chunk, K = 256
GU_CASES = [(4, 12288, 4096), (2, 12288, 4096), (1, 14336, 4096), (4, 14336, 4096), (3, 2048, 4096), (4, 8192, 4096),
            (4, 17408, 4096), (2, 25600, 4096), (1, 10240, 5120), (4, 4096, 4192), (3, 12288, 256)]
GU_IDS = [f"R{R}-I{I}-K{K}-{_form_id(_silu_form(R, I), 2, 4)}" for R, I, K in GU_CASES]


def test_ring_plans_cover_the_launch_forms():
    """The cases below reach what the issue of each form needs (a guard against a host-rule change silently moving them)."""
    forms = {(f["MT"], f["NW"]) for f in (_silu_form(R, I) for R, I, _ in GU_CASES)}
    assert forms == {(2, 12), (2, 16), (4, 12), (4, 16)}
    assert {_silu_form(R, I)["upp"] for R, I, _ in GU_CASES} == {1, 2, 3, 4}
    assert _silu_form(4, 17408)["npass"] == 2 and _silu_form(4, 17408)["upp"] == 3
    assert _silu_form(2, 25600)["npass"] == 2 and _silu_form(2, 25600)["NW"] == 16
    assert (14336 // 16) % 256 != 0 and _silu_form(4, 14336)["upp"] == 4            # tail workgroups: 3 units
    assert (4192 // 32) % 8 != 0                                                       # a partial last chunk
    assert _argmax_form(4, 151936) == dict(MT=4, NW=16, A=2, gx=256, upp=13, npass=3)
    assert _argmax_form(4, 128256)["npass"] == 2 and _argmax_form(4, 128256)["upp"] == 16
    assert _argmax_form(3, 69632)["npass"] == 2 and -(-(69632 // 16) // 256) == 17   # 9 + 8 units
    assert 4208 // 16 - 256 == 7                                                       # 7 workgroups with a second unit


def _silu_ref(x, gate, up):
    """bf16(bf16(silu(bf16 gate)) * bf16 up), torch's rounding points (tf:modeling_qwen3.py:82)."""
    gb = (x.float() @ gate.float().T).to(BF16).float()
    ub = (x.float() @ up.float().T).to(BF16).float()
    return (torch.nn.functional.silu(gb).to(BF16).float() * ub).to(BF16)


@pytest.mark.parametrize("R,I,K", GU_CASES, ids=GU_IDS)
def test_ring_gemm_silu_mul_batch(R, I, K):
    """dfl_gemm_silu_mul_batch from frag16 tiles (the ring kernel).  Small-integer operands (and gate weights scaled by
    2^-6, so that the bf16 rounding of the gate before SiLU matters): the gate and up sums are exact, so the output is
    within 2 bf16 steps of torch at the same rounding points, and nearly every element equal (the SiLU's exp differs in
    the last fp32 bits, which can move each of the two roundings behind it by one step).  Random bf16 operands: the tolerance of
    test_gemm_silu_mul_batch.  Every request's output tile is written (the padding tile of R = 3 is not checked: the
    ring kernel computes all MT tiles)."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _cuda_gen(R * 7 + I + K)
    dyn = H.dyn_records([(0, 16)] * MT, MT, dev())
    ws = ops.gemm_batch_ws(2 * I, K, dev())
    for kind in ("ints", "frac", "randn"):
        if kind != "randn":   # frac: gate sums n / 64, exact in fp32 but not in bf16, where SiLU is not linear
            gate, up, x = _small_ints((I, K), g), _small_ints((I, K), g), _small_ints((MT, 16, K), g)
            gate = gate * 2 ** -6 if kind == "frac" else gate
        else:
            gate = (torch.randn(I, K, generator=g, device=dev()) * 0.05).to(BF16)
            up = (torch.randn(I, K, generator=g, device=dev()) * 0.05).to(BF16)
            x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
        wp = ops.pack_weight_gateup(gate, up)
        act = torch.full((MT, 16 * I), float("nan"), dtype=BF16, device=dev())
        ops.gemm_silu_mul_batch(wp, ops.brows_frag(H.frag_of(x)), R, I, K, act, ws, dyn)
        for r in range(R):
            got = H.unfrag(act[r], I)
            assert not torch.isnan(got.float()).any(), (kind, r)
            want = _silu_ref(x[r], gate, up)
            if kind != "randn":
                # the kernel's exp differs from torch's by fp32 ulps: that moves a bf16 rounding behind it only for values
                # within a few fp32 ulps of a rounding boundary (~2^-14 of them), so a few elements may be a step off
                d = _bf16_ulps(got, want)
                off = float((d > 0).float().mean())
                print(f"[parity] ring silu {kind} R{R} I{I} K{K} r{r}: max {int(d.max())} bf16 steps, {off:.2e} of the "
                      f"elements off")
                assert int(d.max()) <= 2 and off <= 1e-3, (kind, r, int(d.max()), off)
            else:
                H.assert_close(f"ring silu R{R} I{I} K{K} r{r}", got, want, max_rel=2e-2, mean_rel=2e-3)
        del wp, gate, up


# (R, V, K): the vocabulary in 3 passes of 13 units at R = 1..4, 2 passes of 16, 2 uneven passes (9 + 8), 7 workgroups
# with a second unit, hidden 5120
LM_CASES = [(1, 151936, 4096), (2, 151936, 4096), (3, 151936, 4096), (4, 151936, 4096), (4, 128256, 4096),
            (3, 69632, 4096), (2, 4208, 4096), (1, 151936, 5120)]
LM_IDS = [f"R{R}-V{V}-K{K}-{_form_id(_argmax_form(R, V), 1, 1)}" for R, V, K in LM_CASES]
ROW0 = 1                                           # batch.py: row 0 of a block is the committed token
LM_BS = {1: [16], 2: [16, 1], 3: [16, 5, 1], 4: [16, 9, 1, 13]}   # bs 1: no live rows, its ids stay -1


def _first_argmax(lg):
    """Index of the FIRST maximum of each row (model/utils.py:28-29), not relying on torch's tie order."""
    m = lg.max(dim=-1, keepdim=True).values
    idx = torch.arange(lg.shape[-1], device=lg.device).expand_as(lg)
    return torch.where(lg == m, idx, lg.shape[-1]).min(dim=-1).values


def _forced_ties(V, x0):
    """Pairs of weight columns that get the same row: the largest logit any column can reach for rows 1..4 of request 0
    (2 sign(x) . x), so each of these rows has its maximum at exactly two columns.  The pairs sit inside one tile, in two
    workgroups at the same slot, in one workgroup in pass 0 and pass min(2, npass - 1) (or in its first and last unit
    when there is one pass), and in two waves of one workgroup and pass."""
    gx, upp, npass = _ring_plan(V // 16, 16)
    u = min(1, upp - 1)

    def tile(b, p, uu):
        t = b + (p * upp + uu) * gx
        assert t < V // 16
        return t
    p2 = min(2, npass - 1)
    third = (tile(4, 0, u), tile(4, p2, u)) if npass > 1 else (tile(4, 0, 0), tile(4, 0, upp - 1))
    pairs = {1: (16 * tile(3, 0, u) + 13, 16 * tile(3, 0, u) + 6),
             2: (16 * tile(5, 0, u) + 7, 16 * tile(6, 0, u) + 7),
             3: (16 * third[0] + 9, 16 * third[1] + 9),
             4: (16 * tile(2, 0, 0) + 14, 16 * tile(2, 0, 1) + 14)}
    cols = {}
    for m, (a, b) in pairs.items():
        row = (2 * torch.sign(x0[m].float())).to(BF16)
        cols[a] = cols[b] = row
    assert len(cols) == 8
    return pairs, cols


def _argmax_run(ops, wp, x, R, V, K, ws, dyn, with_logits):
    MT = x.shape[0]
    ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    logits = torch.full((MT, 16, V), 3.0, dtype=BF16, device=dev()) if with_logits else None
    ops.gemm_argmax_batch(wp, ops.brows_frag(H.frag_of(x)), R, V, K, ROW0, 16 - ROW0, ws, ids, ROW0, dyn,
                          nrows_dyn_word=ops.DYN_BS, logits=logits)
    return ids, logits


@pytest.mark.parametrize("R,V,K", LM_CASES, ids=LM_IDS)
def test_ring_gemm_argmax_batch_exact_ties(R, V, K):
    """dfl_gemm_argmax_batch from frag16 tiles (the ring kernel + k_argmax_finish_b) as batch.py calls it: row0 = 1, the
    row counts from the dyn word, ragged counts with a request of no live rows.  Small-integer operands make the fp32
    sums exact, so the bf16 logits are known and the ids must equal the first maximum of the REFERENCE logits — with the
    many bf16 ties near the maximum at this V and forced ties across lanes, workgroups, passes and waves, "first index
    wins" is checked through every merge.  With and without the logits output (the product runs without)."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _cuda_gen(V + K + R)
    x = _small_ints((MT, 16, K), g)
    w = _small_ints((V, K), g)
    pairs, cols = _forced_ties(V, x[0])
    for c, row in cols.items():
        w[c] = row
    bss = LM_BS[R] + [0] * (MT - R)
    dyn = H.dyn_records([(0, b) for b in bss], MT, dev())
    wp = ops.pack_weight(w)
    ws = ops.gemm_batch_ws(V, K, dev())
    ref = (x.view(MT * 16, K).float() @ w.float().T).view(MT, 16, V)      # exact integers
    del w
    ref_bf = ref.to(BF16)
    ids0, _ = _argmax_run(ops, wp, x, R, V, K, ws, dyn, False)
    ids1, logits = _argmax_run(ops, wp, x, R, V, K, ws, dyn, True)
    torch.cuda.synchronize()
    for m, (a, b) in pairs.items():     # the construction: row m of request 0 has its maximum at exactly a and b
        top = ref_bf[0, m].float()
        assert top[a] == top[b] == top.max() and int((top == top.max()).sum()) == 2, m
        assert int(ids0[0, m]) == min(a, b), (m, a, b, int(ids0[0, m]))
    ties = 0
    for r in range(MT):
        n = bss[r] - ROW0
        for ids in (ids0, ids1):
            assert torch.all(ids[r, :ROW0] == -1) and torch.all(ids[r, ROW0 + max(n, 0):] == -1), r
        if n <= 0:
            assert torch.all(logits[r] == 3.0), r          # no live rows: nothing written
            continue
        lg = ref_bf[r, ROW0:ROW0 + n]
        want = _first_argmax(lg.float())
        ties += int(((lg == lg.max(dim=-1, keepdim=True).values).sum(-1) > 1).sum())
        assert torch.equal(ids0[r, ROW0:ROW0 + n], want), (r, ids0[r].tolist(), want.tolist())
        assert torch.equal(ids1[r, ROW0:ROW0 + n], want), r
        assert torch.equal(logits[r, ROW0:ROW0 + n], lg), r
        assert torch.all(logits[r, :ROW0] == 3.0) and torch.all(logits[r, ROW0 + n:] == 3.0), r
    print(f"[parity] ring argmax R{R} V{V} K{K}: {ties} live rows with a tie at the maximum")
    assert ties >= 4                                       # at least the forced ones


@pytest.mark.parametrize("R,V,K", [(4, 151936, 4096), (1, 151936, 5120), (3, 69632, 4096), (2, 4208, 4096)])
def test_ring_gemm_argmax_batch_random(R, V, K):
    """Random bf16 operands: the reference logit at the returned id is within rounding of the reference row maximum (the
    kernel's bf16 logit at its id is >= its bf16 logit at the true argmax; each is within half a bf16 step of the fp32
    sum, so the two true values differ by at most one step: two steps of headroom for the summation order), and the
    logits the kernel writes are within bf16 rounding of fp32."""
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    g = _cuda_gen(V + K + 100 * R)
    x = torch.randn(MT, 16, K, generator=g, device=dev()).to(BF16)
    w = (torch.randn(V, K, generator=g, device=dev()) * 0.05).to(BF16)
    bss = LM_BS[R] + [0] * (MT - R)
    dyn = H.dyn_records([(0, b) for b in bss], MT, dev())
    wp = ops.pack_weight(w)
    ws = ops.gemm_batch_ws(V, K, dev())
    ref = (x.view(MT * 16, K).float() @ w.float().T).view(MT, 16, V)
    del w
    ids0, _ = _argmax_run(ops, wp, x, R, V, K, ws, dyn, False)
    ids1, logits = _argmax_run(ops, wp, x, R, V, K, ws, dyn, True)
    for r in range(R):
        n = bss[r] - ROW0
        assert torch.all(ids0[r, :ROW0] == -1) and torch.all(ids0[r, ROW0 + max(n, 0):] == -1), r
        if n <= 0:
            continue
        rr = ref[r, ROW0:ROW0 + n]
        got = ids0[r, ROW0:ROW0 + n]
        assert torch.equal(got, ids1[r, ROW0:ROW0 + n]), r
        assert int(got.min()) >= 0 and int(got.max()) < V, r
        top = rr.max(dim=-1).values
        step = torch.exp2(torch.floor(torch.log2(top.abs())) - 7)           # one bf16 step at the row maximum
        short = top - rr.gather(1, got[:, None])[:, 0]
        print(f"[parity] ring argmax random R{R} V{V} r{r}: worst shortfall {float((short / step).max()):.2f} bf16 steps")
        assert torch.all(short <= 2 * step), (r, (short / step).tolist())
        # half a bf16 step is at most 2^-8 of the scale (a value just under 2^(e+1) against a scale just over 2^e), plus
        # the fp32 summation-order difference (a few fp32 ulps)
        H.assert_close(f"ring lm_head logits R{R} V{V} K{K} r{r}", logits[r, ROW0:ROW0 + n], rr,
                       max_rel=2 ** -8 * 1.01, mean_rel=2 ** -10)


# ---------------------------------------------------------------- batch attention (attn_head.hip)
MAX_SPLITS = 32                                     # BatchedDecoder's default
HEADS = {"draft": (32, 8, False), "target": (32, 8, True), "moe": (32, 4, True)}   # n_q, n_kv, causal


def _attn_form(n_q, n_kv, R, kv_len_max, q_tiles=1):
    """attn_head_launch's pair rule for a ragged-batch launch: k_attn_head_pair(32) or k_attn_head(32)."""
    G = n_q // n_kv
    nt = (kv_len_max - 16 * q_tiles + 31) // 32
    ns = min((nt + 7) // 8, max(1, (256 if R > 1 else 224) // (n_q * R) - 1))
    return "pair" if q_tiles == 1 and G % 2 == 0 and nt > 8 * ns and (nt > 160 or R > 2) else "head"


# name: lens (S per request), bss, kv_len_max (None: the longest request + the block), cache rows
LENS = {"bench": ((1024, 1000, 1040, 990), (16, 16, 16, 16), None, 1100),
        "r2": ((700, 450), (16, 11), None, 800),
        "r3": ((300, 1200, 40), (7, 16, 16), None, 1280),
        "long": ((6000,), (16,), None, 6100),
        "ragged": ((1030, 0, 17, 600), (16, 16, 5, 12), "cap", 1100)}


def _rope_ref(x, w, pos0, eps=1e-6):
    """x [rows, heads, 128] bf16 (CPU) -> Qwen3RMSNorm over the head, RoPE at positions pos0..: [heads, rows, 128]."""
    from oracle import dflash_oracle as O
    y = O.rms_norm(x[None], w, eps).transpose(1, 2)
    c, s = O.rope_cos_sin(torch.arange(pos0, pos0 + x.shape[0])[None], O.rope_inv_freq(128, 1e6), BF16)
    return O.apply_rotary_dflash(y, y, c, s)[1][0]


def _assert_rope_bar(name, got, ref):
    """test_qknorm_rope_append's bar: RoPE in fp32 against the oracle's bf16 products, a step here and there."""
    d = (got.float() - ref.float()).abs()
    frac = float((d > 0).float().mean())
    print(f"[parity] {name}: max {float(d.max() / ref.float().abs().max()):.3e} of scale, {frac:.2e} of the elements off")
    assert d.max() <= 2 ** -6 * ref.float().abs().max() and frac < 0.02, name


def _attn_case(form, heads, lens_name, nparts, seed, q_tiles=1):
    """One ragged-batch attention launch pair against the reference: two launches on one workspace with different
    lengths (the arrival tickets re-arm)."""
    from dflash_amd import ops
    from dflash_amd.model import _rope_tables
    n_q, n_kv, causal = HEADS[heads]
    lens, bss, kvmode, rows = LENS[lens_name]
    if q_tiles == 2:
        bss = tuple(min(32, 17 + 5 * i) for i in range(len(lens)))
    R, L, layer, QS = len(lens), 2, 1, 4            # QS: request slots of the caches / buffers (4: slot R.. is spare)
    kvmax = rows if kvmode == "cap" else max(s + 16 * q_tiles for s in lens)
    ld = (n_q + 2 * n_kv) * 128
    qd, kd = n_q * 128, n_kv * 128
    g = _cuda_gen(seed)
    qw = (1 + 0.1 * torch.randn(128, generator=g, device=dev())).to(BF16)
    kw = (1 + 0.1 * torch.randn(128, generator=g, device=dev())).to(BF16)
    cos, sin = _rope_tables(128, 1e6, rows + 64, dev())
    ws = (ops.attn_fused_batch_ws(QS, n_q, n_kv, MAX_SPLITS, dev()) if form == "fused"
          else ops.attn_head_batch_ws(QS, n_q, MAX_SPLITS, dev(), q_tiles=q_tiles))
    runs = ((lens, bss), (tuple(max(0, s - 37 * (i + 1)) for i, s in enumerate(lens))[::-1], bss[::-1]))
    for run, (lens, bss) in enumerate(runs):
        kc0 = torch.randn(QS, L, n_kv, rows, 128, generator=g, device=dev()).to(BF16)
        vc0 = torch.randn(QS, L, n_kv, rows, 128, generator=g, device=dev()).to(BF16)
        kc, vc = kc0.clone(), vc0.clone()
        dyn = torch.zeros(QS, 8, dtype=torch.int32)
        for r in range(R):
            dyn[r, ops.DYN_S], dyn[r, ops.DYN_BS], dyn[r, ops.DYN_POS0] = lens[r], bss[r], lens[r]
        dyn = dyn.to(dev())
        parts = torch.randn(nparts, QS * 16 * q_tiles, ld, generator=g, device=dev())
        lin = parts.sum(0).to(BF16).view(QS, 16 * q_tiles, ld)       # the Linear outputs: bf16(part 0 + part 1)
        out = torch.zeros(QS * q_tiles, 16 * qd, dtype=BF16, device=dev())
        common = dict(q_col=0, k_col=qd, v_col=qd + kd, R=R, n_q=n_q, n_kv=n_kv, q_norm_w=qw, k_norm_w=kw, eps=1e-6,
                      cos_tab=cos, sin_tab=sin, kcache=kc, vcache=vc, layer=layer, scale=128 ** -0.5, causal=causal,
                      dyn=dyn, kv_len_max=kvmax, ws=ws, max_splits=MAX_SPLITS, out_frag=out)
        if form == "f32":
            ops.attn_head_batch_f32(qkv_parts=parts, nparts=nparts, MT=QS, ld=ld, **common)
        elif form == "fused":   # per-tile records (one 16-row tile per request here), as batch.py's _attend passes them
            ops.attn_fused_batch(qkv=parts, nsplit=nparts, split_stride=QS * 16 * ld, ld=ld, **common)
        else:
            ops.attn_head_batch(xq=lin.reshape(QS * q_tiles, 16, ld).contiguous(), q_tiles=q_tiles, **common)
        torch.cuda.synchronize()
        kchk, vchk = kc.clone(), vc.clone()
        G = n_q // n_kv
        for r in range(R):
            S, bs = lens[r], bss[r]
            tag = f"{form} {heads} {lens_name} p{nparts} t{q_tiles} launch{run} r{r}"
            rows_r = lin[r, :bs].cpu()
            q = _rope_ref(rows_r[:, :qd].view(bs, n_q, 128), qw.cpu(), S)
            k = _rope_ref(rows_r[:, qd:qd + kd].view(bs, n_kv, 128), kw.cpu(), S)
            v = rows_r[:, qd + kd:].view(bs, n_kv, 128).transpose(0, 1)
            assert torch.equal(vc[r, layer, :, S:S + bs].cpu(), v), tag
            _assert_rope_bar(f"batch attn K rows {tag}", kc[r, layer, :, S:S + bs].cpu(), k)
            kchk[r, layer, :, S:S + bs] = kc0[r, layer, :, S:S + bs]
            vchk[r, layer, :, S:S + bs] = vc0[r, layer, :, S:S + bs]
            # fp32 softmax attention over the cached rows and the new ones
            keys = torch.cat([kc0[r, layer, :, :S], k.to(dev())], dim=1).float().repeat_interleave(G, dim=0)
            vals = torch.cat([vc0[r, layer, :, :S], v.to(dev())], dim=1).float().repeat_interleave(G, dim=0)
            sc = torch.einsum("hqd,hkd->hqk", q.to(dev()).float(), keys) * 128 ** -0.5
            if causal:
                mask = torch.arange(S + bs, device=dev())[None, :] > (S + torch.arange(bs, device=dev()))[:, None]
                sc = sc.masked_fill(mask[None], float("-inf"))
            ref = torch.einsum("hqk,hkd->qhd", torch.softmax(sc, dim=-1), vals)
            got = torch.cat([H.unfrag(out[r * q_tiles + t], qd) for t in range(q_tiles)])[:bs].view(bs, n_q, 128)
            assert torch.isfinite(got.float()).all(), tag
            H.assert_close(f"batch attn out {tag}", got, ref, max_rel=2 ** -6, mean_rel=H.MEAN_REL)
        # rows outside [S, S + bs) of the layer, the other layer and the spare request slots are untouched
        assert torch.equal(kchk, kc0) and torch.equal(vchk, vc0), (form, heads, lens_name, run)


ATTN_F32 = [(h, n, p) for h in HEADS for n in LENS for p in (2,)] + [("draft", "bench", 1), ("target", "ragged", 1)]


@pytest.mark.parametrize("heads,lens_name,nparts", ATTN_F32,
                         ids=[f"{h}-{n}-p{p}-{_attn_form(HEADS[h][0], HEADS[h][1], len(LENS[n][0]), LENS[n][3] if LENS[n][2] else max(LENS[n][0]) + 16)}32"
                              for h, n, p in ATTN_F32])
def test_attn_head_batch_f32_against_reference(heads, lens_name, nparts):
    """dfl_attn_head_batch_f32 (the batch's default attention stage: draft non-causal, target verify causal) on the fp32
    K parts of the q/k/v projection, against q/k/v = bf16(sum of parts), the oracle's RMSNorm and RoPE at each request's
    positions, the append to its cache, and fp32 softmax attention over the cached plus new rows.  V rows bit-exact, K
    rows within the RoPE bar, outputs within test_block_attn's bar, nothing else in the caches touched; a second launch
    with other lengths on the same workspace."""
    _attn_case("f32", heads, lens_name, nparts, seed=100 * list(HEADS).index(heads) + 10 * list(LENS).index(lens_name) + nparts)


ATTN_BF16 = [("draft", "bench", 1), ("target", "ragged", 1), ("moe", "r2", 1), ("target", "r3", 2), ("draft", "r2", 2)]


@pytest.mark.parametrize("heads,lens_name,q_tiles", ATTN_BF16,
                         ids=[f"{h}-{n}-qt{t}-{_attn_form(HEADS[h][0], HEADS[h][1], len(LENS[n][0]), LENS[n][3] if LENS[n][2] else max(LENS[n][0]) + 16 * t, t)}"
                              for h, n, t in ATTN_BF16])
def test_attn_head_batch_against_reference(heads, lens_name, q_tiles):
    """dfl_attn_head_batch on finished bf16 q/k/v rows against the same reference; q_tiles = 2 is the two-tile form
    (blocks of 17..32 rows, q_tiles = 2)."""
    _attn_case("bf16", heads, lens_name, 1, seed=17 * q_tiles + len(lens_name), q_tiles=q_tiles)


ATTN_FUSED = [("draft", "bench", 2), ("target", "ragged", 2), ("moe", "r2", 1), ("target", "r3", 2), ("draft", "long", 1)]


@pytest.mark.parametrize("heads,lens_name,nparts", ATTN_FUSED, ids=[f"{h}-{n}-p{p}" for h, n, p in ATTN_FUSED])
def test_attn_fused_batch_against_reference(heads, lens_name, nparts):
    """dfl_attn_fused_batch (the batch's attention stage when attn_impl != "head") on the fp32 K parts, against the same
    reference and with the same bars as the head forms above; GQA groups 4 and 8, ragged lengths including 0."""
    _attn_case("fused", heads, lens_name, nparts, seed=1000 + 10 * list(LENS).index(lens_name) + nparts)


# ---------------------------------------------------------------- dfl_kv_append_batch / _t (rows.hip)
def _kv_append_check(ops, kc0, vc0, kc, vc, parts, kw, tiles, layers, kd, req_of):
    """tiles: per tile (S, tau); tile t's rows are rows t*16.. of the parts, its cache is request req_of(t)'s."""
    lin = parts.sum(0).to(BF16).cpu()
    kexp, vexp = kc0.clone(), vc0.clone()
    for t, (S, tau) in enumerate(tiles):
        if tau == 0:
            continue
        for ly in range(layers):
            rows = lin[t * 16:t * 16 + tau, ly * 2 * kd:(ly + 1) * 2 * kd]
            n_kv = kd // 128
            k = _rope_ref(rows[:, :kd].reshape(tau, n_kv, 128), kw[ly].cpu(), S)
            v = rows[:, kd:].reshape(tau, n_kv, 128).transpose(0, 1)
            idx = req_of(t)
            kslot = kc[idx][ly] if idx is not None else kc[ly]
            _assert_rope_bar(f"kv_append K tile {t} layer {ly}", kslot[:, S:S + tau].cpu(), k)
            (vexp[idx][ly] if idx is not None else vexp[ly])[:, S:S + tau] = v.to(dev())
            (kexp[idx][ly] if idx is not None else kexp[ly])[:, S:S + tau] = kslot[:, S:S + tau]
    assert torch.equal(vc, vexp)          # V bit-exact, every other row of every layer untouched
    assert torch.equal(kc, kexp)


def _kv_setup(seed, n_tiles, L, n_kv, cache_shape):
    from dflash_amd.model import _rope_tables
    g = _cuda_gen(seed)
    kd = n_kv * 128
    ld = L * 2 * kd
    parts = torch.randn(2, n_tiles * 16, ld, generator=g, device=dev())
    kw = (1 + 0.1 * torch.randn(L, 128, generator=g, device=dev())).to(BF16)
    kc0 = torch.randn(*cache_shape, generator=g, device=dev()).to(BF16)
    vc0 = torch.randn(*cache_shape, generator=g, device=dev()).to(BF16)
    cos, sin = _rope_tables(128, 1e6, cache_shape[-2] + 64, dev())
    return parts, kw, kc0, vc0, cos, sin, kd, ld


def _kv_call(ops, parts, n_tiles, ld, kd, L, n_kv, kw, cos, sin, kc, vc, dyn, tpr=1):
    ops.kv_append_batch(kv=parts, nsplit=2, split_stride=n_tiles * 16 * ld, ld=ld, k_col=0, v_col=kd, col_layer_stride=2 * kd,
                        n_layers=L, R=n_tiles, n_kv=n_kv, k_norm_w=kw, eps=1e-6, cos_tab=cos, sin_tab=sin, kcache=kc,
                        vcache=vc, dyn=dyn, tiles_per_req=tpr)


def _dyn_tiles(tiles):
    d = torch.zeros(len(tiles), 8, dtype=torch.int32)
    for t, (S, tau) in enumerate(tiles):
        d[t, 0], d[t, 1], d[t, 3] = S, tau, S          # S, tau, pos0 = S
    return d.to(dev())


@pytest.mark.parametrize("R", [1, 2, 3, 4])
def test_kv_append_batch_against_oracle(R):
    """dfl_kv_append_batch: the draft's context K/V of 5 layers for R requests in one launch, tau per request in
    {16, 0, 7, 1}, pos0 = S: V bit-exact, K (k_norm + RoPE) within the RoPE bar, every other row untouched."""
    from dflash_amd import ops
    L, n_kv, rows = 5, 8, 400
    parts, kw, kc0, vc0, cos, sin, kd, ld = _kv_setup(R, R, L, n_kv, (4, L, n_kv, rows, 128))
    tiles = [(37, 16), (300, 0), (0, 7), (129, 1)][:R]
    kc, vc = kc0.clone(), vc0.clone()
    _kv_call(ops, parts, R, ld, kd, L, n_kv, kw, cos, sin, kc, vc, _dyn_tiles(tiles))
    _kv_append_check(ops, kc0, vc0, kc, vc, parts, kw, tiles, L, kd, lambda t: t)


def test_kv_append_batch_shared_cache_and_two_tiles_per_request():
    """The 4-D form (ONE request's cache, consecutive 16-row tiles of its context, each with its own S / pos0: the
    large-M context prefill) and tiles_per_req = 2 (two tiles per request cache)."""
    from dflash_amd import ops
    L, n_kv, rows = 5, 8, 300
    # 4-D: 5 tiles of one request, the last one partial
    tiles = [(50 + 16 * t, 16 if t < 4 else 9) for t in range(5)]
    parts, kw, kc0, vc0, cos, sin, kd, ld = _kv_setup(11, 5, L, n_kv, (L, n_kv, rows, 128))
    kc, vc = kc0.clone(), vc0.clone()
    _kv_call(ops, parts, 5, ld, kd, L, n_kv, kw, cos, sin, kc, vc, _dyn_tiles(tiles))
    _kv_append_check(ops, kc0, vc0, kc, vc, parts, kw, tiles, L, kd, lambda t: None)
    # two tiles per request: 3 requests, tile 2 q at S, tile 2 q + 1 at S + 16
    tiles = [(20, 16), (36, 5), (0, 1), (16, 0), (200, 16), (216, 16)]
    parts, kw, kc0, vc0, cos, sin, kd, ld = _kv_setup(12, 6, L, n_kv, (4, L, n_kv, rows, 128))
    kc, vc = kc0.clone(), vc0.clone()
    _kv_call(ops, parts, 6, ld, kd, L, n_kv, kw, cos, sin, kc, vc, _dyn_tiles(tiles), tpr=2)
    _kv_append_check(ops, kc0, vc0, kc, vc, parts, kw, tiles, L, kd, lambda t: t // 2)
