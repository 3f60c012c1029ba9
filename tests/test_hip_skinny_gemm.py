"""The single-request skinny GEMM (k_gemm in gemm_skinny.hip) at the launch forms the one-request path runs, each
against plain fp32 torch or the oracle: dfl_gemm_resid (whole tiles, whole tiles + 8-column halves, all halves,
K-chunked), dfl_gemm_f32 at ksplit 1, dfl_gemm_silu_mul and dfl_gemm_argmax, from frag16, plain-row and normalised
sources (mode 2: the RMSNorm runs in the GEMM prologue from the producer's partial sums of squares).

The host picks the form from the shape: plan_tiles, the chunk rule of dfl_gemm_resid and "a launch that leaves sums of
squares keeps whole tiles".  Those rules are mirrored below; each test id names the form its case reaches, and
test_skinny_plans_cover_the_launch_forms (no GPU) checks that the cases reach every form and tile-count edge.

Exact cases use small-integer operands: every product and fp32 sum is exact, so the outputs must equal torch's bit for
bit at the same bf16 rounding points.  A normalised source is made exact as well: rows of small integers whose mean
square is a power of four and eps = 0 make the normalised rows plain small integers again (see _normed)."""
import pytest
import torch

import helpers as H

BF16 = torch.bfloat16
TAU, BS = 1, 2            # dyn words (dflash_amd.ops.DYN_TAU, DYN_BS)


# ---------------------------------------------------------------- host rules of gemm_skinny.hip / gemm_rows.h
def grid_x_for(ngroups, ksplit=1):
    """grid_x_for(): at most 256 / ksplit workgroups, each walking the same number of groups."""
    gx_max = max(1, 256 // ksplit)
    per_wg = -(-ngroups // gx_max)
    return -(-ngroups // per_wg)


def plan_tiles(ntiles, allow_half):
    """plan_tiles(): (workgroups, tiles walked whole, tiles cut in two 8-column halves)."""
    if allow_half and ntiles <= 128:              # every tile in halves, one per workgroup
        return 2 * ntiles, 0, ntiles
    r = ntiles % 256
    if not allow_half or ntiles <= 256 or r == 0 or r > 128:
        return grid_x_for(ntiles), ntiles, 0
    return 256, ntiles - r, r                     # the last r <= 128 tiles in halves, after the whole ones


def resid_plan(N, K, ss_out):
    """dfl_gemm_resid: K beyond 16 waves x 8 k-steps is walked in chunks of 64 k-steps, and a launch that is chunked or
    leaves sums of squares keeps whole tiles."""
    KS = K // 32
    nch = 1 if KS <= 128 else -(-KS // 64)
    gx, whole, half = plan_tiles(N // 16, nch == 1 and not ss_out)
    return dict(gx=gx, whole=whole, half=half, nch=nch)


def tile_plan(N):
    """dfl_gemm_f32 at ksplit 1 and dfl_gemm_argmax: halves allowed."""
    gx, whole, half = plan_tiles(N // 16, True)
    return dict(gx=gx, whole=whole, half=half, nch=1)


def silu_plan(I):
    """dfl_gemm_silu_mul: gate/up pairs over grid_x_for(I/16) workgroups, never cut."""
    npairs = I // 16
    gx = grid_x_for(npairs)
    return dict(gx=gx, npairs=npairs, per_wg=-(-npairs // gx))


def form_id(p):
    s = f"{p['whole']}w+{p['half']}h" if p["half"] else f"{p['whole']}w-gx{p['gx']}"
    return s + (f"-{p['nch']}ch" if p["nch"] > 1 else "")


# (what, N, K, source, valid word, add_residual, ss_out, tap): the call sites of the one-request path, then the
# tile-count edges of plan_tiles
RESID_CASES = [
    ("qkv", 6144, 4096, "normed", BS, False, False, False),          # r = 128: one whole tile, then a half
    ("moe-qkv", 5120, 2048, "normed", BS, False, False, False),      # 256 whole + 64 in halves
    ("ctx-kv", 10240, 4096, "normed", TAU, False, False, False),     # two whole tiles, then a half
    ("moe-oproj", 2048, 4096, "frag", -1, True, False, False),       # all halves, the prefetched residual
    ("router", 128, 2048, "frag", -1, False, False, False),          # all halves on 16 workgroups
    ("oproj", 4096, 4096, "frag", -1, True, True, False),
    ("qkv-ss", 6144, 4096, "normed", BS, True, True, True),          # ss_out: whole tiles, two per workgroup
    ("t257", 4112, 1024, "rows", TAU, True, False, True),            # 256 whole + 1 in halves
    ("t385", 6160, 1024, "rows", TAU, True, False, False),           # r = 129: whole tiles on 193 workgroups
    ("t129", 2064, 512, "rows", BS, False, False, False),            # whole tiles on 129 workgroups
    ("down", 4096, 12288, "frag", -1, True, True, True),             # 6 chunks
    ("down-llama", 4096, 14336, "frag", -1, True, True, True),       # 7 chunks
    ("fc", 4096, 20480, "rows", TAU, False, True, False),            # 10 chunks from plain rows
    ("fc-4b", 2560, 12800, "rows", TAU, False, True, False),         # 7 chunks, the last one of 16 k-steps
]


def _resid_id(c):
    what, N, K, src, _, add, ss, tap = c
    extra = "".join(s for s, on in (("-add", add), ("-ss", ss), ("-tap", tap)) if on)
    return f"resid-{what}-N{N}-K{K}-{form_id(resid_plan(N, K, ss))}-{src}{extra}"


RESID_IDS = [_resid_id(c) for c in RESID_CASES]
# (N, K, mt, sources): dfl_gemm_f32 at ksplit 1
F32_CASES = [(6144, 4096, 1, ("normed",)), (2048, 4096, 1, ("rows",)), (5120, 2048, 2, ("frag", "normed"))]
F32_IDS = [f"f32-N{N}-K{K}-mt{mt}-{form_id(tile_plan(N))}-{'+'.join(s)}" for N, K, mt, s in F32_CASES]
# (I, K): Qwen3-8B, Llama-3.1-8B (uneven: 224 workgroups of 4 pairs), Qwen3-4B (uneven: 203 workgroups, the last with
# 2 pairs), and a 2048-hidden draft
SILU_CASES = [(12288, 4096), (14336, 4096), (9728, 2560), (6144, 2048)]
SILU_IDS = [f"silu-I{I}-K{K}-{silu_plan(I)['npairs']}p-gx{silu_plan(I)['gx']}" for I, K in SILU_CASES]
ARGMAX_CASES = [151936, 128256]
ARGMAX_IDS = [f"argmax-V{V}-K4096-{form_id(tile_plan(V))}-normed" for V in ARGMAX_CASES]


def test_skinny_plans_cover_the_launch_forms():
    """The cases reach every launch form and the tile-count edges of plan_tiles (a guard against a host-rule change
    silently moving them)."""
    assert plan_tiles(128, True) == (256, 0, 128)             # all halves
    assert plan_tiles(129, True) == (129, 129, 0)             # whole
    assert plan_tiles(256, True) == (256, 256, 0)
    assert plan_tiles(257, True) == (256, 256, 1)
    assert plan_tiles(384, True) == (256, 256, 128)           # r = 128
    assert plan_tiles(385, True) == (193, 385, 0)             # r = 129
    assert plan_tiles(640, True) == (256, 512, 128)
    assert plan_tiles(384, False) == (192, 384, 0) and plan_tiles(128, False) == (128, 128, 0)
    plans = {c[0]: resid_plan(c[1], c[2], c[6]) for c in RESID_CASES}
    assert {c[1] // 16 for c in RESID_CASES} >= {128, 129, 256, 257, 384, 385}
    assert plans["moe-oproj"] == dict(gx=256, whole=0, half=128, nch=1)
    assert plans["qkv"] == dict(gx=256, whole=256, half=128, nch=1)
    assert plans["ctx-kv"] == dict(gx=256, whole=512, half=128, nch=1)
    assert plans["moe-qkv"]["half"] == 64 and plans["router"] == dict(gx=16, whole=0, half=8, nch=1)
    assert plans["qkv-ss"] == dict(gx=192, whole=384, half=0, nch=1)             # ss_out disables halves
    assert plans["t257"]["half"] == 1 and plans["t385"]["gx"] == 193 and plans["t129"]["gx"] == 129
    assert [plans[k]["nch"] for k in ("down", "down-llama", "fc", "fc-4b")] == [6, 7, 10, 7]
    assert all(plans[k]["half"] == 0 for k in ("down", "down-llama", "fc", "fc-4b"))  # chunked: whole tiles
    assert 12800 // 32 % 64 == 16                                                 # a partial last chunk
    srcs = {(c[3], plans[c[0]]["half"] > 0, plans[c[0]]["whole"] > 0, plans[c[0]]["nch"] > 1) for c in RESID_CASES}
    assert {("normed", True, True, False), ("frag", True, False, False), ("frag", False, True, False),
            ("normed", False, True, False), ("rows", True, True, False), ("rows", False, True, False),
            ("frag", False, True, True), ("rows", False, True, True)} <= srcs
    assert any(c[5] for c in RESID_CASES if plans[c[0]]["whole"] == 0)          # the prefetched residual of all halves
    assert tile_plan(6144) == dict(gx=256, whole=256, half=128, nch=1) and tile_plan(2048)["whole"] == 0
    assert tile_plan(5120)["half"] == 64
    assert tile_plan(151936) == dict(gx=256, whole=37 * 256, half=24, nch=1)
    assert tile_plan(128256) == dict(gx=256, whole=31 * 256, half=80, nch=1)
    assert silu_plan(12288) == dict(gx=256, npairs=768, per_wg=3)
    assert silu_plan(14336) == dict(gx=224, npairs=896, per_wg=4)
    assert silu_plan(9728)["gx"] == 203 and 9728 // 16 % 203 != 0
    assert silu_plan(6144) == dict(gx=192, npairs=384, per_wg=2)


# ---------------------------------------------------------------- operands
def dev():
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    from dflash_amd import ops as o
    return o


def _cuda_gen(seed):
    return torch.Generator(device=dev()).manual_seed(seed)


def _small_ints(shape, g, lo=-2, hi=2):
    """bf16 integers in [lo, hi] drawn on the device."""
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev(), dtype=torch.int8).to(BF16)


def _bf16_ulps(a, b):
    """Distance in bf16 steps between two bf16 tensors (the bit patterns mapped onto a monotonic integer line)."""
    def line(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


def _dyn(nv):
    d = torch.zeros(8, dtype=torch.int32)
    d[TAU] = d[BS] = nv
    return d.to(dev())


def _frag(x):
    return H.frag_of(x[None])[0]


def _unit_rows(K, seed):
    """bf16 [16, K] of small integers with a mean square of exactly 1: per row n2 entries +-2, 3 n2 zeros, the rest +-1
    (4 n2 + (K - 4 n2) = K)."""
    g = H.gen(seed)
    rows = []
    for _ in range(16):
        n2 = int(torch.randint(K // 64, K // 8, (1,), generator=g))
        v = torch.ones(K)
        v[:n2], v[n2:4 * n2] = 2.0, 0.0
        sign = torch.randint(0, 2, (K,), generator=g) * 2 - 1
        rows.append(v[torch.randperm(K, generator=g)] * sign)
    return torch.stack(rows).to(BF16).to(dev())


ROW_EXP = torch.tensor([-1, 0, 1, 2] * 4)          # row m is scaled by 2^ROW_EXP[m]: a mean square of 4^ROW_EXP[m]


def _partials(h, nss):
    """[nss * 16] fp32 partial sums of squares, slot j * 16 + m = row m over columns j K/nss .. (j+1) K/nss (the layout
    dfl_gemm_resid leaves in ss_out when nss = K/16)."""
    K = h.shape[1]
    return h.float().pow(2).view(16, nss, K // nss).sum(-1).T.contiguous().view(-1)


def _normed(K, seed, nss=None):
    """An exact normalised source: h = b * 2^e (b of _unit_rows, a mean square of 4^e), norm weights in {+-1, +-2} and
    eps = 0.  rsqrt(4^e) = 2^-e, and each h * rstd is within a few fp32 ulps of b, a bf16 integer, whether rsqrtf is
    exact or not: bf16(h * rstd) = b and the normalised rows are norm_w * b, small integers (checked here against the
    oracle's rms_norm).  Returns h, its partial sums (nss slots, default K/16), norm_w and those normalised rows."""
    from oracle.dflash_oracle import rms_norm
    b = _unit_rows(K, seed)
    h = (b.float() * torch.exp2(ROW_EXP.float()).to(dev())[:, None]).to(BF16)
    g = H.gen(seed + 1)
    nw = (torch.randint(1, 3, (K,), generator=g) * (torch.randint(0, 2, (K,), generator=g) * 2 - 1)).to(BF16).to(dev())
    xn = (nw.float() * b.float()).to(BF16)
    assert torch.equal(rms_norm(h, nw, 0.0), xn)
    return h, _partials(h, nss or K // 16), nw, xn


def _source(ops, kind, K, vw, nv, seed, nss=None):
    """(row source, the rows the GEMM must see as fp32 [16, K]).  Rows >= nv of a plain or normalised source hold
    nonzero data that the kernel must treat as zero.  nss: partial sums of squares of a normalised source (K / 16)."""
    if kind == "frag":
        x = _small_ints((16, K), _cuda_gen(seed))
        return ops.rows_frag(_frag(x)), x.float()
    if kind == "rows":
        x = _small_ints((16, K), _cuda_gen(seed))
        src, xs = ops.rows_plain(x, vw), x.float()
    else:
        h, ss, nw, xs = _normed(K, seed, nss)
        src, xs = ops.rows_normed(h, ss, nss or K // 16, nw, 0.0, vw), xs.float()
    xs = xs.clone()
    xs[nv:] = 0
    return src, xs


def _distinct_resid(ld):
    """bf16 [16, ld]: a distinct value for every (row, column) within 1021 elements of each other, in [2, 512) with
    alternating sign, so that a residual read from a wrong address shows."""
    idx = torch.arange(16 * ld, dtype=torch.int32).view(ld, 16).T
    bits = 0x4000 + idx % 1021 - 0x8000 * ((idx // 1021) % 2)     # the sign bit, as an int16
    return bits.to(torch.int16).contiguous().view(BF16).to(dev())


def _ss_ref(h):
    """ss_out of dfl_gemm_resid for the rows h [16, N]: slot t * 16 + m = sum over tile t of row m squared."""
    return _partials(h, h.shape[1] // 16)


# ---------------------------------------------------------------- dfl_gemm_resid
@pytest.mark.gpu
@pytest.mark.parametrize("case", RESID_CASES, ids=RESID_IDS)
def test_gemm_resid_exact(ops, case):
    """h <- bf16(h + bf16(x W^T)) (or bf16(x W^T) without the residual), the tap and the per-tile sums of squares, at
    every form, bit for bit.  The residual differs in every element and h_io / tap rows are longer than N: a half
    tile or a prefetched residual at a wrong address, or a column written past N, fails exactly.  Valid rows 1 / 7 / 16
    for plain and normalised sources: rows at or past the count are unchanged with a residual, zero without one."""
    what, N, K, kind, vw, add, want_ss, want_tap = case
    w = _small_ints((N, K), _cuda_gen(N + K))
    wp = ops.pack_weight(w)
    ld = N + 48
    for nv in ((16,) if kind == "frag" else (1, 7, 16)):
        src, xs = _source(ops, kind, K, vw, nv, seed=N + K + nv)
        h0 = _distinct_resid(ld)
        h = h0.clone()
        tap = torch.full((16, N + 80), 5.0, dtype=BF16, device=dev()) if want_tap else None
        ss = torch.full((N,), float("nan"), device=dev()) if want_ss else None
        ops.gemm_resid(wp, src, N, K, h, add_residual=add, ss_out=ss, tap=None if tap is None else tap[:, 40:40 + N],
                       dyn=_dyn(nv))
        lin = (xs @ w.float().T).to(BF16)
        want = (h0[:, :N].float() + lin.float()).to(BF16) if add else lin
        assert torch.equal(h[:, :N], want), (what, nv, int((h[:, :N] != want).sum()))
        assert torch.equal(h[:, N:], h0[:, N:]), (what, nv)
        assert torch.equal(h[nv:, :N], h0[nv:, :N] if add else torch.zeros_like(h0[nv:, :N])), (what, nv)
        if tap is not None:
            assert torch.equal(tap[:, 40:40 + N], want), (what, nv)
            assert torch.all(tap[:, :40] == 5.0) and torch.all(tap[:, 40 + N:] == 5.0), (what, nv)
        if ss is not None:
            torch.testing.assert_close(ss, _ss_ref(want), rtol=2e-6, atol=0)


# ---------------------------------------------------------------- dfl_gemm_f32 at ksplit 1
@pytest.mark.gpu
@pytest.mark.parametrize("N,K,mt,kinds", F32_CASES, ids=F32_IDS)
def test_gemm_f32_ksplit1_exact(ops, N, K, mt, kinds):
    """fp32 output of every row tile, bit for bit, in the half-tile plans of a single K pass; the normalised and plain
    sources with 7 valid rows (the rest must come out zero)."""
    w = _small_ints((N, K), _cuda_gen(N + K + mt))
    srcs = [_source(ops, k, K, BS, 7, seed=N + 3 * i) for i, k in enumerate(kinds)]
    out = torch.full((mt * 16, N), float("nan"), device=dev())
    ops.gemm_f32(ops.pack_weight(w), srcs[0][0], srcs[1][0] if mt == 2 else None, mt, N, K, 1, out, _dyn(7))
    for i, (_, xs) in enumerate(srcs):
        assert torch.equal(out[16 * i:16 * i + 16], xs @ w.float().T), (i, kinds[i])


# ---------------------------------------------------------------- dfl_gemm_silu_mul
def _silu_ref(xs, gate, up):
    """bf16(bf16(silu(bf16 gate)) * bf16 up), torch's rounding points (tf:modeling_qwen3.py:82)."""
    gb = (xs @ gate.float().T).to(BF16).float()
    ub = (xs @ up.float().T).to(BF16).float()
    return (torch.nn.functional.silu(gb).to(BF16).float() * ub).to(BF16)


@pytest.mark.gpu
@pytest.mark.parametrize("I,K", SILU_CASES, ids=SILU_IDS)
def test_gemm_silu_mul_exact(ops, I, K):
    """SiLU(gate) * up at the benchmark's gate/up shapes, from the normalised source the layer reads (11 valid rows)
    and from frag16.  The gate and up sums are exact, so the output is within 2 bf16 steps of torch at the same rounding
    points and nearly every element equal (the kernel's exp differs from torch's in the last fp32 bits, which can move
    either rounding behind it by one step: the bound of the ring kernel's test).  Gate weights scaled by 2^-6 put the
    gate sums where SiLU is not linear and their bf16 rounding matters.  Rows past the count are zero."""
    g = _cuda_gen(I + K)
    up = _small_ints((I, K), g)
    gate_i = _small_ints((I, K), g)
    for kind in ("ints", "frac"):
        gate = gate_i * 2 ** -6 if kind == "frac" else gate_i
        wp = ops.pack_weight_gateup(gate, up)
        for sk in ("normed", "frag"):
            nv = 11 if sk == "normed" else 16
            src, xs = _source(ops, sk, K, BS, nv, seed=I + K + len(sk))
            act = torch.full((16 * I,), float("nan"), dtype=BF16, device=dev())
            ops.gemm_silu_mul(wp, src, I, K, act, _dyn(nv))
            got, want = H.unfrag(act, I), _silu_ref(xs, gate, up)
            d = _bf16_ulps(got, want)
            off = float((d > 0).float().mean())
            print(f"[parity] silu {kind} {sk} I{I} K{K}: max {int(d.max())} bf16 steps, {off:.2e} of the elements off")
            assert not torch.isnan(got.float()).any(), (kind, sk)
            assert int(d.max()) <= 2 and off <= 1e-3, (kind, sk, int(d.max()), off)
            assert torch.count_nonzero(got[nv:].float()) == 0, (kind, sk)
        del wp


# ---------------------------------------------------------------- dfl_gemm_argmax
def _first_argmax(lg):
    """Index of the FIRST maximum of each row (model/utils.py:28-29), not relying on torch's tie order."""
    m = lg.max(dim=-1, keepdim=True).values
    idx = torch.arange(lg.shape[-1], device=lg.device).expand_as(lg)
    return torch.where(lg == m, idx, lg.shape[-1]).min(dim=-1).values


def _argmax_ties(V):
    """Rows with their maximum at exactly two columns: the two halves of the last remainder tile (two workgroups), a
    whole tile and a half in one workgroup (the half is its last item), a whole tile and a half in two workgroups,
    workgroup 0's first whole tile and its half, and two whole tiles whose workgroups k_argmax_finish merges in one
    lane (b and b + 64)."""
    _, ntw, r = plan_tiles(V // 16, True)
    k = r // 2
    assert r >= 4 and 255 >= 2 * r
    return {1: (16 * (ntw + r - 1) + 2, 16 * (ntw + r - 1) + 13),        # workgroups 2r - 2 and 2r - 1
            2: (16 * (2 + 256) + 11, 16 * (ntw + 1) + 5),                 # workgroup 2: tile 258, then half 0 of ntw + 1
            3: (16 * (255 + 256 * 5) + 0, 16 * (ntw + k) + 9),            # workgroups 255 and 2k + 1
            4: (16 * 0 + 15, 16 * ntw + 7),                               # workgroup 0: tile 0, then half 0 of ntw
            5: (16 * 5 + 4, 16 * 69 + 4)}                                 # workgroups 5 and 69: one lane of the finish


@pytest.mark.gpu
@pytest.mark.parametrize("V", ARGMAX_CASES, ids=ARGMAX_IDS)
def test_gemm_argmax_normed_exact(ops, V):
    """lm_head + argmax from the normalised source as the verify calls it (row0 0, the row count from the dyn word, the
    ids at out_off), with the logits output and without (the product's fused form).  Exact logits: the ids must be the
    first maximum of torch's logits, through forced ties across the two halves of one tile and between a whole tile and
    a half.  ids outside [out_off, out_off + rows) and logits of dead rows stay untouched; the margins are torch's
    top-2 gaps.  A second launch on the same workspace with other rows (row0 1, host row count) is right as well."""
    K, nv, off = 4096, 11, 16
    w = _small_ints((V, K), _cuda_gen(V))
    h, ss, nw, xn = _normed(K, V)
    ties = _argmax_ties(V)
    for m, (a, b) in ties.items():
        w[a] = w[b] = (2 * torch.sign(xn[m].float())).to(BF16)
    wp = ops.pack_weight(w)
    ws = ops.argmax_ws(dev())
    ref = (xn.float() @ w.float().T).to(BF16)
    for m, (a, b) in ties.items():     # the construction: row m has its maximum at exactly a and b
        top = ref[m].float()
        assert top[a] == top[b] == top.max() and int((top == top.max()).sum()) == 2, m
    src = ops.rows_normed(h, ss, K // 16, nw, 0.0, BS)
    runs = []
    for with_logits in (True, False):
        ids = torch.full((48,), -7, dtype=torch.int64, device=dev())
        mg = torch.full((48,), -7.0, device=dev())
        logits = torch.full((16, V), 3.0, dtype=BF16, device=dev()) if with_logits else None
        ops.gemm_argmax(wp, src, V, K, 0, 16, ws, ids, off, dyn=_dyn(nv), nrows_dyn_word=BS, logits=logits, margins=mg)
        runs.append((ids, mg, logits))
    want = _first_argmax(ref[:nv].float())
    top2 = ref[:nv].float().topk(2, dim=-1).values
    for ids, mg, logits in runs:
        assert torch.equal(ids[off:off + nv], want), (ids[off:off + nv].tolist(), want.tolist())
        assert torch.all(ids[:off] == -7) and torch.all(ids[off + nv:] == -7)
        assert torch.equal(mg[off:off + nv], top2[:, 0] - top2[:, 1])
        assert torch.all(mg[:off] == -7) and torch.all(mg[off + nv:] == -7)
        assert all(float(mg[off + m]) == 0 for m in ties)
        assert all(int(ids[off + m]) == min(ties[m]) for m in ties)
        if logits is not None:
            assert torch.equal(logits[:nv], ref[:nv]) and torch.all(logits[nv:] == 3.0)
    # the same workspace again: other rows, row0 1, the row count from the host
    h2, ss2, nw2, xn2 = _normed(K, V + 5)
    ids = torch.full((16,), -7, dtype=torch.int64, device=dev())
    ops.gemm_argmax(wp, ops.rows_normed(h2, ss2, K // 16, nw2, 0.0), V, K, 1, 15, ws, ids, 0)
    ref2 = (xn2.float() @ w.float().T).to(BF16)
    assert torch.equal(ids[:15], _first_argmax(ref2[1:].float())) and int(ids[15]) == -7


@pytest.mark.gpu
def test_gemm_argmax_events(ops):
    """The optional event pair of dfl_gemm_argmax (what bench.py times the lm_head kernel with): one 16-row tile,
    K = 256, V = 320.  With and without `events=` the ids are the same (and the first maximum of torch's exact logits);
    both events are recorded on the stream, start before end."""
    V, K = 320, 256
    w = _small_ints((V, K), _cuda_gen(3))
    x = _small_ints((16, K), _cuda_gen(4))
    wp, src, ws = ops.pack_weight(w), ops.rows_frag(_frag(x)), ops.argmax_ws(dev())
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    end.record()                      # recorded once so that their handles exist: in the WRONG order, work in between,
    torch.mm(w.float(), w.float().T)  # so that a launch that left them alone would not pass below
    start.record()
    plain = torch.full((16,), -7, dtype=torch.int64, device=dev())
    timed = torch.full((16,), -7, dtype=torch.int64, device=dev())
    ops.gemm_argmax(wp, src, V, K, 0, 16, ws, plain)
    ops.gemm_argmax(wp, src, V, K, 0, 16, ws, timed, events=(start, end))
    torch.cuda.synchronize()
    assert torch.equal(plain, timed)
    assert torch.equal(plain, _first_argmax((x.float() @ w.float().T).to(BF16).float()))
    assert start.query() and end.query() and start.elapsed_time(end) >= 0


# ---------------------------------------------------------------- the normalised source
@pytest.mark.gpu
@pytest.mark.parametrize("nss", [1, 128, 256], ids=lambda n: f"nss{n}")
def test_normed_source_accuracy(ops, nss):
    """Random rows, eps 1e-6, partial sums over K/nss columns each: the GEMM with the RMSNorm in its prologue against
    the oracle's rms_norm + an fp32 matmul, within the bar of test_gemm_row_sources_and_resid_epilogue (1-ulp flips of
    the normalised inputs); rows past the valid count come out zero."""
    from oracle.dflash_oracle import rms_norm
    N, K, nv = 4096, 4096, 13
    g = _cuda_gen(nss)
    h = (torch.randn(16, K, generator=g, device=dev()) * 0.7).to(BF16)
    nw = (1 + 0.1 * torch.randn(K, generator=g, device=dev())).to(BF16)
    w = (torch.randn(N, K, generator=g, device=dev()) * 0.03).to(BF16)
    out = torch.full((16, N), float("nan"), device=dev())
    ops.gemm_f32(ops.pack_weight(w), ops.rows_normed(h, _partials(h, nss), nss, nw, 1e-6, BS), None, 1, N, K, 1, out,
                 _dyn(nv))
    ref = rms_norm(h[:nv], nw, 1e-6).float() @ w.float().T
    d = (out[:nv] - ref).abs()
    scale = float(ref.abs().max())
    print(f"[parity] normed nss{nss}: max {float(d.max()) / scale:.3e} mean {float(d.mean()) / scale:.3e} of scale")
    assert float(d.max()) <= 2e-2 * scale and float(d.mean()) <= 1e-3 * scale
    # the reference rounds at the kernel's points, so flips are rare (measured: mean 5e-8 of scale); a partial sum left
    # out moves rstd by ~1 / (2 nss) and every normalised element with it: ~5e-4 of scale at nss 256
    assert float(d.mean()) <= 2e-5 * scale
    assert torch.count_nonzero(out[nv:]) == 0


def _direct_partials(K, nss, seed):
    """[nss * 16] partial sums given directly (not from the rows): row m's K 4^e split at random over its nss slots, in
    whole multiples of 4^e, so that every sum of them is exact."""
    g = H.gen(seed)
    ss = torch.zeros(nss, 16)
    for m in range(16):
        q = torch.bincount(torch.randint(0, nss, (K,), generator=g), minlength=nss).float()
        ss[:, m] = q * 4.0 ** int(ROW_EXP[m])
    return ss.view(-1).to(dev())


@pytest.mark.gpu
@pytest.mark.parametrize("nss", [1, 128, 256], ids=lambda n: f"nss{n}")
def test_normed_source_partial_slots(ops, nss):
    """Exact form: partial sums given directly, eps 0, a mean square of 4^e per row (see _normed): the output equals
    torch's bit for bit.  Then slot j in {0, 15, 16, nss - 1} of row m in {0, 15} is raised by 3 x the row's total:
    rstd halves, so row m's output must be exactly half (the kernel read that slot for that row), and every other row
    must stay bit-identical to the unperturbed launch (it read no other row's slot)."""
    N, K = 4096, 4096
    h, _, nw, xn = _normed(K, 300 + nss)
    ss = _direct_partials(K, nss, nss)
    w = _small_ints((N, K), _cuda_gen(nss))
    wp = ops.pack_weight(w)

    def run(s):
        out = torch.full((16, N), float("nan"), device=dev())
        ops.gemm_f32(wp, ops.rows_normed(h, s, nss, nw, 0.0), None, 1, N, K, 1, out)
        return out
    base = run(ss)
    assert torch.equal(base, xn.float() @ w.float().T)
    total = ss.view(nss, 16).sum(0)
    for j in sorted({0, 15, 16, nss - 1} & set(range(nss))):
        for m in (0, 15):
            s = ss.clone()
            s[j * 16 + m] += 3 * total[m]
            out = run(s)
            assert torch.equal(out[m], base[m] / 2), (j, m)
            others = [r for r in range(16) if r != m]
            assert torch.equal(out[others], base[others]), (j, m)


@pytest.mark.gpu
def test_normed_source_rejects_more_than_256_partials(ops):
    """The prologue reads at most 256 partial sums per row: a normalised source with more is refused by every entry
    point that takes one, not summed in part."""
    from dflash_amd._lib import DFlashHipError
    N, K = 256, 4096
    h = torch.ones(16, K, dtype=BF16, device=dev())
    nw = torch.ones(K, dtype=BF16, device=dev())
    ss = torch.full((257 * 16,), float(K) / 257, device=dev())
    wp = ops.pack_weight(torch.zeros(N, K, dtype=BF16, device=dev()))
    out = torch.zeros(16, N, device=dev())
    ops.gemm_f32(wp, ops.rows_normed(h, ss, 256, nw, 1e-6), None, 1, N, K, 1, out)     # 256: accepted
    torch.cuda.synchronize()
    bad = ops.rows_normed(h, ss, 257, nw, 1e-6)
    with pytest.raises(DFlashHipError, match="at most 256"):
        ops.gemm_f32(wp, bad, None, 1, N, K, 1, out)
    with pytest.raises(DFlashHipError, match="at most 256"):
        ops.gemm_resid(wp, bad, N, K, torch.zeros(16, N, dtype=BF16, device=dev()), add_residual=False)
    with pytest.raises(DFlashHipError, match="at most 256"):
        ops.gemm_silu_mul(ops.pack_weight_gateup(torch.zeros(N, K, dtype=BF16, device=dev()),
                                                 torch.zeros(N, K, dtype=BF16, device=dev())),
                          bad, N, K, torch.zeros(16 * N, dtype=BF16, device=dev()))
    with pytest.raises(DFlashHipError, match="at most 256"):
        ops.gemm_argmax(wp, bad, N, K, 0, 16, ops.argmax_ws(dev()), torch.zeros(16, dtype=torch.int64, device=dev()))


# ---------------------------------------------------------------- one layer as the verify runs it
@pytest.mark.gpu
def test_layer_chain_qwen3_8b(ops):
    """o_proj (+ residual, ss_out) -> gate/up + SiLU from the ln2-normalised rows (nss 256) -> the 6-chunk down_proj
    (+ residual, ss_out, tap) -> lm_head + argmax from the final-normalised rows (nss 256), at Qwen3-8B widths and in
    the order of the target's verify.  Each stage reads the kernel's own output of the stage before and is compared
    with the oracle's rms_norm + fp32 torch at the bars of the existing tests of each epilogue."""
    from oracle.dflash_oracle import rms_norm
    Hd, I, V, bs, eps = 4096, 12288, 151936, 11, 1e-6
    g = _cuda_gen(8)

    def randn(*shape, s=1.0):
        return (torch.randn(*shape, generator=g, device=dev()) * s).to(BF16)
    wo, wg, wu, wd = randn(Hd, Hd, s=0.02), randn(I, Hd, s=0.02), randn(I, Hd, s=0.02), randn(Hd, I, s=0.02)
    ln2 = (1 + 0.1 * torch.randn(Hd, generator=g, device=dev())).to(BF16)
    fnorm = (1 + 0.1 * torch.randn(Hd, generator=g, device=dev())).to(BF16)
    h0, attn = randn(16, Hd, s=0.5), randn(16, Hd)
    dyn = _dyn(bs)

    def resid_bar(name, got, want):
        dd = (got.float() - want.float()).abs()
        scale = float(want.float().abs().max())
        print(f"[parity] chain {name}: max {float(dd.max()) / scale:.3e} of scale, {float((dd > 0).float().mean()):.2e} "
              f"of the elements off")
        assert float(dd.max()) <= 2 ** -6 * scale and float((dd > 0).float().mean()) < 0.02, name

    # o_proj
    h1 = h0.clone()
    ss1 = torch.full((Hd,), float("nan"), device=dev())
    ops.gemm_resid(ops.pack_weight(wo), ops.rows_frag(_frag(attn)), Hd, Hd, h1, add_residual=True, ss_out=ss1, dyn=dyn)
    resid_bar("o_proj", h1, (h0.float() + (attn.float() @ wo.float().T).to(BF16).float()).to(BF16))
    torch.testing.assert_close(ss1, _ss_ref(h1), rtol=1e-5, atol=0)
    # gate/up + SiLU from the ln2-normalised rows
    act = torch.full((16 * I,), float("nan"), dtype=BF16, device=dev())
    ops.gemm_silu_mul(ops.pack_weight_gateup(wg, wu), ops.rows_normed(h1, ss1, Hd // 16, ln2, eps, BS), I, Hd, act, dyn)
    xn = rms_norm(h1, ln2, eps).float()
    xn[bs:] = 0
    got = H.unfrag(act, I)
    H.assert_close("chain gate/up silu", got[:bs], _silu_ref(xn, wg, wu)[:bs], max_rel=2e-2, mean_rel=2e-3)
    assert torch.count_nonzero(got[bs:].float()) == 0
    # down_proj, K-chunked, with the tap
    h2 = h1.clone()
    ss2 = torch.full((Hd,), float("nan"), device=dev())
    taps = torch.zeros(16, 3 * Hd, dtype=BF16, device=dev())
    ops.gemm_resid(ops.pack_weight(wd), ops.rows_frag(act), Hd, I, h2, add_residual=True, ss_out=ss2,
                   tap=taps[:, Hd:2 * Hd], dyn=dyn)
    resid_bar("down_proj", h2, (h1.float() + (got.float() @ wd.float().T).to(BF16).float()).to(BF16))
    assert torch.equal(taps[:, Hd:2 * Hd], h2) and torch.count_nonzero(taps[:, :Hd]) == 0
    assert torch.count_nonzero(taps[:, 2 * Hd:]) == 0
    torch.testing.assert_close(ss2, _ss_ref(h2), rtol=1e-5, atol=0)
    del wo, wg, wu, wd
    # lm_head + argmax from the final-normalised rows
    wl = randn(V, Hd, s=0.02)
    ids = torch.full((16,), -7, dtype=torch.int64, device=dev())
    logits = torch.full((16, V), float("nan"), dtype=BF16, device=dev())
    ops.gemm_argmax(ops.pack_weight(wl), ops.rows_normed(h2, ss2, Hd // 16, fnorm, eps, BS), V, Hd, 0, bs,
                    ops.argmax_ws(dev()), ids, 0, dyn=dyn, logits=logits)
    ref = rms_norm(h2[:bs], fnorm, eps).float() @ wl.float().T
    assert float((logits[:bs].float() - ref).abs().max()) <= 2 ** -7 * float(ref.abs().max())
    assert torch.isnan(logits[bs:].float()).all() and torch.all(ids[bs:] == -7)
    assert torch.equal(ids[:bs], _first_argmax(logits[:bs].float()))
    H.assert_ids_match_where_safe("chain lm_head", ids[:bs], ref, margin_rel=1e-2)
