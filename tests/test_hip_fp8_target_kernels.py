"""The sampled lm_head with e4m3 weights on the GPU ("The target"): dfl_gemm_sample on e4m3 codes
against torch on exact operands, against dfl_gemm_argmax's logits on the same codes and against the two-step draw over
them; dfl_gemm_sample_batch on e4m3 codes (the ring form, both epilogues) bit for bit against the bf16 form on the
dequantised copy
and against the two-step draw, and what it refuses."""
import ctypes as C

import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu
BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
T = 0.7
# (row0, nrows, pos_add, seed) of test_gemm_sample_matches_the_mirror_and_the_two_step_draw
TRIPLES = ((0, 16, 1, 5), (1, 15, 0, 2 ** 40 + 7), (0, 16, 17, 11))
SCALES = (1.0, 1.5, 0.75, 2.0 ** -3)


def dev():
    return torch.device("cuda", 0)


def _codes(w):
    q = w.float().to(F8)
    assert torch.equal(q.float(), w.float())
    return q.view(torch.uint8).contiguous()


# ---------------------------------------------------------------------------------------------- dfl_gemm_sample on e4m3 codes
def _int_case(V, K, normed):
    """Weights in [-8, 8] (exact in e4m3) and one of SCALES by row (all four inside every tile): with activations that are
    multiples of 1/4 of magnitude <= 4 every K-sum is an integer number of quarters below 2^18 and its product with a
    scale (at most two significant bits) is exact in fp32 — so bf16(sum * scale) is known exactly, and a dropped or
    misindexed scale changes a logit.  Returns (Fp8Weight, row source, exact fp64 logits [16, V])."""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(V + K + normed)
    w = torch.randint(-8, 9, (V, K), generator=g).float()
    scale = torch.tensor(SCALES)[(torch.arange(V) * 7 + torch.arange(V) // 16) % 4]
    assert len(set(scale[:16].tolist())) == 4, "the scales differ inside a tile"
    w8 = ops.pack_weight_fp8(_codes(w).to(dev()), scale.to(dev()))
    x = torch.randint(-4, 5, (16, K), generator=g).to(BF16)
    if not normed:
        src, xe = ops.rows_plain(x.to(dev())), x.double()
    else:
        # the RMSNorm in the GEMM's prologue with operands that keep it exact: the caller-supplied sum of squares
        # 4 K gives rstd = rsqrt(4 + 1e-6) = 0.5 (1 - 1.25e-7), bf16(x * rstd) = x / 2 (an integer or a half: nowhere
        # near a rounding boundary), and the norm weights are powers of two
        nw = torch.tensor([1.0, 2.0, 0.5])[torch.arange(K) % 3].to(BF16)
        ss = torch.full((16,), 4.0 * K)
        src = ops.rows_normed(x.to(dev()), ss.to(dev()), 1, nw.to(dev()), 1e-6)
        xe = x.double() * 0.5 * nw.double()
    exact = (xe @ w.double().T) * scale.double()[None]
    assert float((xe @ w.double().T).abs().max()) * 4 < 2 ** 22
    return w8, src, exact


@pytest.mark.parametrize("normed", [False, True], ids=["plain", "normed"])
@pytest.mark.parametrize("V,K", [(2048, 512), (4208, 1024)])
def test_gemm_sample_fp8_exact_ints(V, K, normed):
    """The materialised logits are torch's bf16(sum * scale) and dfl_gemm_argmax's on the same codes, bit for bit; the ids are
    dfl_sample_rows' over those logits, with positions from a device record and from pos_base; rows outside
    [row0, row0 + nrows) are not written, neither ids nor logits."""
    from dflash_amd import ops
    w8, src, exact = _int_case(V, K, normed)
    want = exact.float().to(BF16)
    assert torch.equal(exact.float().double(), exact), "the scaled sums are exact in fp32"
    ws = ops.argmax_ws(dev())
    rec = torch.tensor([0, 0, 16, 1000, 1000, 0, 0, 0], dtype=torch.int32, device=dev())
    for row0, nrows, pos_add, seed in TRIPLES:
        lg_arg = torch.full((16, V), 3.0, dtype=BF16, device=dev())
        ids_arg = torch.full((16,), -1, dtype=torch.int64, device=dev())
        ops.gemm_argmax(w8, src, V, K, row0, nrows, ws, ids_arg, 0, logits=lg_arg)
        for from_record in (True, False):
            ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
            logits = torch.full((16, V), 3.0, dtype=BF16, device=dev())
            kw = dict(pos_dyn=rec, pos_word=ops.DYN_POS0) if from_record else dict(pos_base=777)
            base = 1000 if from_record else 777
            ops.gemm_sample(w8, src, V, K, row0, nrows, ws, ids, 0, seed=seed, temperature=T, pos_add=pos_add,
                            logits=logits, **kw)
            live = slice(row0, row0 + nrows)
            assert torch.equal(logits[live].cpu().view(torch.int16), want[live].view(torch.int16)), (row0, from_record)
            assert torch.equal(logits.view(torch.int16), lg_arg.view(torch.int16))
            assert torch.all(logits[:row0] == 3.0) and torch.all(logits[row0 + nrows:] == 3.0)
            two = ops.sample_rows(logits[live], seed=seed, temperature=T, pos0=base + pos_add + row0)
            assert torch.equal(ids[:nrows], two), (row0, from_record)
            assert torch.all(ids[nrows:] == -1)
            # the fused form proper (no logits written): the same ids
            ids2 = torch.full((16,), -1, dtype=torch.int64, device=dev())
            ops.gemm_sample(w8, src, V, K, row0, nrows, ws, ids2, 0, seed=seed, temperature=T, pos_add=pos_add, **kw)
            assert torch.equal(ids, ids2)


def test_gemm_sample_fp8_draft_stream_and_margins():
    """The DRAFT noise stream (extra = base) and the perturbed top-2 gap: dfl_sample_rows' over the same logits."""
    from dflash_amd import ops
    V, K = 2048, 512
    w8, src, _ = _int_case(V, K, False)
    ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
    marg = torch.zeros(16, device=dev())
    logits = torch.zeros(16, V, dtype=BF16, device=dev())
    ops.gemm_sample(w8, src, V, K, 0, 16, ops.argmax_ws(dev()), ids, 0, seed=9, temperature=T, stream=ops.RNG_DRAFT,
                    pos_base=300, pos_add=2, logits=logits, margins=marg)
    m2 = torch.zeros(16, device=dev())
    two = ops.sample_rows(logits, seed=9, temperature=T, pos0=302, stream=ops.RNG_DRAFT, extra=300, margins=m2)
    assert torch.equal(ids, two) and torch.equal(marg, m2)


def test_gemm_sample_fp8_full_vocabulary():
    """(V 151936, K 4096), random data quantised by quantize_fp8_rows: every workgroup and merge pass of the real head.
    The fused draw equals the two-step draw over the launch's own logits bit for bit, the logits equal
    dfl_gemm_argmax's on the same codes, and the launch that writes no logits draws the same ids."""
    from dflash_amd import ops
    V, K = 151936, 4096
    gd = torch.Generator(device=dev()).manual_seed(19)
    w = (torch.randn(V, K, generator=gd, device=dev()) * 0.02).to(BF16)
    x = torch.randn(16, K, generator=gd, device=dev()).to(BF16)
    w8 = ops.pack_weight_fp8(*ops.quantize_fp8_rows(w))
    del w
    ws = ops.argmax_ws(dev())
    ss = x.float().pow(2).sum(-1).contiguous()
    nw = (1 + 0.1 * torch.randn(K, generator=gd, device=dev())).to(BF16)
    rec = torch.tensor([0, 0, 13, 4321, 4321, 0, 0, 0], dtype=torch.int32, device=dev())
    for src in (ops.rows_plain(x), ops.rows_normed(x, ss, 1, nw, 1e-6)):
        ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
        logits = torch.zeros(16, V, dtype=BF16, device=dev())
        ops.gemm_sample(w8, src, V, K, 1, 15, ws, ids, 1, seed=2 ** 63 + 3, temperature=T, pos_dyn=rec,
                        pos_word=ops.DYN_POS0, pos_add=1, logits=logits)
        two = ops.sample_rows(logits[1:], seed=2 ** 63 + 3, temperature=T, pos0=4321 + 1 + 1)
        assert torch.equal(ids[1:], two) and int(ids[0]) == -1
        lg = torch.zeros(16, V, dtype=BF16, device=dev())
        ids_arg = torch.full((16,), -1, dtype=torch.int64, device=dev())
        ops.gemm_argmax(w8, src, V, K, 1, 15, ws, ids_arg, 1, logits=lg)
        assert torch.equal(lg.view(torch.int16), logits.view(torch.int16))
        ids2 = torch.full((16,), -1, dtype=torch.int64, device=dev())
        ops.gemm_sample(w8, src, V, K, 1, 15, ws, ids2, 1, seed=2 ** 63 + 3, temperature=T, pos_dyn=rec,
                        pos_word=ops.DYN_POS0, pos_add=1)
        assert torch.equal(ids, ids2)
        assert float((ids[1:] != ids_arg[1:]).float().mean()) > 0.5   # (random logits at T = 0.7: draws, not the argmax)


# ---------------------------------------------------------------------------------------- dfl_gemm_sample_batch on e4m3 codes
V_B = 4208
RING_CASES = [(1, 1), (3, 1), (4, 1), (4, 2)]
SEEDS = [3, 2 ** 63 + 5, 77, 1 << 40]
TS = [0.7, 0.0, 1.3, 0.4]   # per-request temperatures (test_hip_request_temperature.py): request 1 is greedy
_RING = {}


def _ring_case(K):
    """One quantised head, its dequantised bf16 copy and four activation tiles per K, shared and never modified."""
    if K not in _RING:
        from dflash_amd import ops
        g = torch.Generator(device=dev()).manual_seed(50 + K)
        w = (torch.randn(V_B, K, generator=g, device=dev()) * 0.02).to(BF16)
        x = torch.randn(4, 16, K, generator=g, device=dev()).to(BF16)
        q, sc = ops.quantize_fp8_rows(w)
        assert torch.unique(sc).numel() > 1
        _RING[K] = dict(w8=ops.pack_weight_fp8(q, sc), wp=ops.pack_weight(ops.dequantize_fp8_rows(q, sc)), x=x,
                        gws=torch.zeros(ops.lib().dfl_gemm_batch_ws_bytes(V_B, K), dtype=torch.uint8, device=dev()))
    return _RING[K]


def _records(R, tpr):
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    bs = [16, 11, 16, 5][:R] if tpr == 1 else [16, 9, 16, 14][:R]
    rec = torch.zeros(MT, 8, dtype=torch.int32)
    for t in range(R):
        rec[t, ops.DYN_BS], rec[t, ops.DYN_POS0] = bs[t], 500 + 97 * (t // tpr)
    return MT, bs, rec.to(dev())


def _slots(R, tpr, MT, temps):
    from dflash_amd import ops
    n = MT // tpr
    ts = (list(temps)[:R // tpr] + [0.0] * n)[:n]
    seeds = torch.tensor([ops.seed_i64(s) for s in SEEDS[:n]], dtype=torch.int64, device=dev())
    inv = torch.tensor([ops.inv_temperature(t) if t > 0 else 0.0 for t in ts], dtype=torch.float32, device=dev())
    return ts, seeds, inv


def _ring_launch(wp, c, K, R, tpr, rec, seeds, with_logits=True, **temp):
    from dflash_amd import ops
    MT = ops.batch_tiles(R)
    ids = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    logits = torch.full((MT, 16, V_B), 3.0, dtype=BF16, device=dev()) if with_logits else None
    ops.gemm_sample_batch(wp, ops.brows_frag(H.frag_of(c["x"][:MT])), R, V_B, K, 0, 16, c["gws"], ids, 0, rec, seeds=seeds,
                          pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=tpr, nrows_dyn_word=ops.DYN_BS, logits=logits,
                          **temp)
    return ids, logits


@pytest.mark.parametrize("per_request", [False, True], ids=["uniform", "per-request"])
@pytest.mark.parametrize("K", [512, 4096])
@pytest.mark.parametrize("R,tpr", RING_CASES)
def test_ring_sample_fp8_equals_the_bf16_ring_and_the_two_step_draw(R, tpr, K, per_request):
    """dfl_gemm_sample_batch on e4m3 codes against dfl_gemm_sample_batch on the dequantised copy: ids and logits bit for bit.
    Derivable, as for the argmax ring (test_ring_argmax_fp8_equals_the_bf16_ring_on_the_copy): the lm_head forms have
    KQ = 1, so in both a wave owns a column tile and walks ALL k-steps of K in ascending order through the same MFMA
    (the W8 form converts a code to the bf16 value q exactly; chunks past K are zeros in both); its fp32 sum is then
    the bf16 form's sum of q * scale divided by the power-of-two scale — scaling by a power of two commutes with every
    fp32 rounding (random normal data: no subnormals) — and the multiplication by the scale in front of the epilogue
    restores the same bits, which the same epilogue rounds, perturbs and compares.  V = 4208 = 263 tiles: more than one
    pass per workgroup and a last pass with idle waves.  Then the ids against dfl_sample_rows over the launch's own
    logits (a greedy slot: dfl_gemm_argmax_batch's ids on the same codes), rows past a tile's count and tiles past R unwritten, and
    the launch without logits draws the same ids."""
    from dflash_amd import ops
    c = _ring_case(K)
    MT, bs, rec = _records(R, tpr)
    ts, seeds, inv = _slots(R, tpr, MT, TS if per_request else [T] * 4)
    temp = dict(inv_ts=inv) if per_request else dict(temperature=T)
    ids, logits = _ring_launch(c["w8"], c, K, R, tpr, rec, seeds, **temp)
    ids_b, logits_b = _ring_launch(c["wp"], c, K, R, tpr, rec, seeds, **temp)
    assert torch.equal(ids, ids_b)
    assert torch.equal(logits.view(torch.int16), logits_b.view(torch.int16))
    ids_n, _ = _ring_launch(c["w8"], c, K, R, tpr, rec, seeds, with_logits=False, **temp)
    assert torch.equal(ids, ids_n)
    greedy = torch.full((MT, 16), -1, dtype=torch.int64, device=dev())
    ops.gemm_argmax_batch(c["w8"], ops.brows_frag(H.frag_of(c["x"][:MT])), R, V_B, K, 0, 16, c["gws"], greedy, 0, rec,
                          nrows_dyn_word=ops.DYN_BS)
    for t in range(R):
        q, j, n = t // tpr, t % tpr, bs[t]
        pos0 = 500 + 97 * q + 1 + 16 * j
        sd = int(seeds[q]) & 0xFFFFFFFFFFFFFFFF
        if ts[q] > 0:
            two = ops.sample_rows(logits[t, :n], seed=sd, temperature=ts[q], pos0=pos0)
            assert torch.equal(ids[t, :n], two), (t, ts[q])
            assert not torch.equal(ids[t, :n], greedy[t, :n]) or n < 4, t
        else:
            assert per_request and torch.equal(ids[t, :n], greedy[t, :n]), t
        assert torch.all(ids[t, n:] == -1) and torch.all(logits[t, n:] == 3.0), t
    assert torch.all(ids[R:] == -1) and torch.all(logits[R:] == 3.0)
    if per_request:
        assert any(t == 0.0 for t in ts[:max(1, R // tpr)]) or R // tpr < 2


def test_ring_sample_fp8_refusals_launch_nothing():
    """What the ring cannot take is refused with an error (never a quiet fall-back): a source that is not frag16,
    K % 64, K < 256, R outside 1..4, a null or misaligned scale vector.  The ids buffer keeps its fill."""
    from dflash_amd import _lib, ops
    K = 512
    c = _ring_case(K)
    MT, bs, rec = _records(2, 1)
    _, seeds, _ = _slots(2, 1, MT, [T] * 4)
    ids = torch.full((4, 16), -1, dtype=torch.int64, device=dev())
    xf = H.frag_of(c["x"][:2])
    good = ops.brows_frag(xf)
    w8 = c["w8"]

    def call(wp, x, R, Kk):
        ops.gemm_sample_batch(wp, x, R, V_B, Kk, 0, 16, c["gws"], ids, 0, rec, seeds=seeds, temperature=T,
                              pos_word=ops.DYN_POS0, pos_add=1, tiles_per_req=1, nrows_dyn_word=ops.DYN_BS)

    with pytest.raises(_lib.DFlashHipError, match="dfl_gemm_sample_batch:.*ring form"):
        call(w8, ops.brows_plain(c["x"][:2].contiguous()), 2, K)
    for Kk in (288, 192):    # K % 64 != 0; K < 256 (the buffers are never read: refused on the numbers alone)
        fake = ops.Fp8Weight(w8.wp, w8.scale, V_B, Kk)
        with pytest.raises(_lib.DFlashHipError, match="dfl_gemm_sample_batch:.*K"):
            call(fake, good, 2, Kk)
    for R in (0, 5):
        with pytest.raises((_lib.DFlashHipError, AssertionError)):
            call(w8, good, R, K)
    pad = torch.zeros(V_B + 16, dtype=torch.float32, device=dev())
    off = next(i for i in range(1, 16) if pad[i:].data_ptr() % 64)
    pad[off:off + V_B] = w8.scale
    with pytest.raises(_lib.DFlashHipError, match="dfl_gemm_sample_batch:.*64-byte aligned"):
        call(ops.Fp8Weight(w8.wp, pad[off:off + V_B], V_B, K), good, 2, K)
    # a null scale vector, and R out of range, through the C ABI itself
    h = _lib.lib()
    args = lambda scale, R: (_lib.Weight(w8.wp.data_ptr(), scale, _lib.W_E4M3), good.ref, R, V_B, K, 0, 16, rec.data_ptr(), ops.DYN_BS,  # noqa: E731
                             c["gws"].data_ptr(), ids.data_ptr(), 16, 0, None, 0, seeds.data_ptr(), None,
                             C.c_float(1.0 / T), 0, ops.DYN_POS0, 1, 1, None)
    for scale, R in ((None, 2), (w8.scale.data_ptr(), 0), (w8.scale.data_ptr(), 5)):
        assert h.dfl_gemm_sample_batch(*args(scale, R)) == -22
        assert b"dfl_gemm_sample_batch:" in h.dfl_last_error()
    torch.cuda.synchronize()
    assert torch.all(ids == -1)
    call(w8, good, 2, K)     # and the same arguments, valid: it launches
    assert int(ids[0].min()) >= 0
