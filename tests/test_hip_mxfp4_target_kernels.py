"""The sampled lm_head over MXFP4 codes on the GPU (k_gemm_s_w4; DESIGN.md section 17, "The target")."""
import pytest
import torch

pytestmark = pytest.mark.gpu
BF16, U8 = torch.bfloat16, torch.uint8
T = 0.7
TRIPLES = ((0, 16, 1, 5), (1, 15, 0, 2 ** 40 + 7), (0, 7, 17, 11))   # (row0, nrows, pos_add, seed)
# (2048, 512): 16 k-steps, nfr 1 rounds to 4 and waves 4..15 are clipped to nothing; (4208, 1024): 263 tiles = 256 whole +
# 7 cut in halves; (4208, 4096): nfr 8, every wave's share equal to the bf16 form's
SHAPES = [(2048, 512), (4208, 1024), (4208, 4096)]


def dev():
    return torch.device("cuda", 0)


def _int_case(V, K, normed):
    """Random e2m1 codes under block scales {1, 2^-3, 2^2} and all-zero blocks (every kind in every tile and row),
    activations integers of magnitude <= 4 (normed: quarters): products are multiples of 2^-6 and a row's sum of
    magnitudes stays below 2^18, so every fp32 sum is exact in any order.  -> (Mxfp4Weight, row source, fp64 logits)"""
    from dflash_amd import ops
    g = torch.Generator().manual_seed(V + K + normed)
    codes = torch.randint(0, 256, (V, K // 2), generator=g).to(U8)
    kind = (torch.arange(V)[:, None] * 3 + torch.arange(K // 32)[None] + torch.arange(V)[:, None] // 16) % 4
    codes = torch.where(kind.repeat_interleave(16, dim=1) == 3, torch.zeros_like(codes), codes)
    sc = torch.tensor([127, 124, 129, 127])[kind].to(U8)
    w = ops.dequantize_mxfp4_rows(codes, sc).double()
    w4 = ops.pack_weight_mxfp4(codes.to(dev()), sc.to(dev()))
    x = torch.randint(-4, 5, (16, K), generator=g).to(BF16)
    if not normed:
        src, xe = ops.rows_plain(x.to(dev())), x.double()
    else:
        # sum of squares 4 K: rstd = 0.5 (1 - 1.25e-7), bf16(x * rstd) = x / 2; the norm weights are powers of two
        nw = torch.tensor([1.0, 2.0, 0.5])[torch.arange(K) % 3].to(BF16)
        src = ops.rows_normed(x.to(dev()), torch.full((16,), 4.0 * K).to(dev()), 1, nw.to(dev()), 1e-6)
        xe = x.double() * 0.5 * nw.double()
    assert float((xe.abs() @ w.abs().T).max()) < 2 ** 18
    return w4, src, xe @ w.T


@pytest.mark.parametrize("normed", [False, True], ids=["plain", "normed"])
@pytest.mark.parametrize("V,K", SHAPES)
def test_gemm_sample_mxfp4_exact_ints(V, K, normed):
    """Logits: fp64 bf16(x W^T) on the dequantised matrix and dfl_gemm_argmax's on the same blob, bit for bit.  Ids:
    dfl_sample_rows over the launch's own logits, positions from a record and from pos_base.  Other rows: unwritten."""
    from dflash_amd import ops
    w4, src, exact = _int_case(V, K, normed)
    want = exact.float().to(BF16)
    ws = ops.argmax_ws(dev())
    rec = torch.tensor([0, 0, 16, 1000, 1000, 0, 0, 0], dtype=torch.int32, device=dev())
    for row0, nrows, pos_add, seed in TRIPLES:
        lg_arg = torch.full((16, V), 3.0, dtype=BF16, device=dev())
        ops.gemm_argmax(w4, src, V, K, row0, nrows, ws, torch.zeros(16, dtype=torch.int64, device=dev()), 0, logits=lg_arg)
        for from_record in (True, False):
            ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
            logits = torch.full((16, V), 3.0, dtype=BF16, device=dev())
            kw = dict(pos_dyn=rec, pos_word=ops.DYN_POS0) if from_record else dict(pos_base=777)
            base = 1000 if from_record else 777
            ops.gemm_sample(w4, src, V, K, row0, nrows, ws, ids, 0, seed=seed, temperature=T, pos_add=pos_add,
                            logits=logits, **kw)
            live = slice(row0, row0 + nrows)
            assert torch.equal(logits[live].cpu().view(torch.int16), want[live].view(torch.int16)), (row0, from_record)
            assert torch.equal(logits.view(torch.int16), lg_arg.view(torch.int16))
            assert torch.all(logits[:row0] == 3.0) and torch.all(logits[row0 + nrows:] == 3.0)
            two = ops.sample_rows(logits[live], seed=seed, temperature=T, pos0=base + pos_add + row0)
            assert torch.equal(ids[:nrows], two) and torch.all(ids[nrows:] == -1), (row0, from_record)
    ids = torch.full((16,), -1, dtype=torch.int64, device=dev())      # the DRAFT stream: extra = base
    ops.gemm_sample(w4, src, V, K, 0, 16, ws, ids, 0, seed=9, temperature=T, stream=ops.RNG_DRAFT, pos_base=300, pos_add=2,
                    logits=logits)
    assert torch.equal(ids, ops.sample_rows(logits, seed=9, temperature=T, pos0=302, stream=ops.RNG_DRAFT, extra=300))


@pytest.mark.parametrize("normed", [False, True], ids=["plain", "normed"])
def test_gemm_sample_mxfp4_equals_the_bf16_launch_on_the_dequantised_matrix_at_k_4096(normed):
    """randn weights through the quantiser: nfr = 8 in both forms, every wave sums its bf16 counterpart's k-steps in the
    same order — ids and logits EQUAL dfl_gemm_sample's on the packed bf16 copy of the dequantised values."""
    from dflash_amd import ops
    V, K = 4208, 4096
    gd = torch.Generator(device=dev()).manual_seed(23)
    q = ops.quantize_mxfp4_rows((torch.randn(V, K, generator=gd, device=dev()) * 0.02).to(BF16))
    w4, wb = ops.pack_weight_mxfp4(*q), ops.pack_weight(ops.dequantize_mxfp4_rows(*q))
    x = torch.randn(16, K, generator=gd, device=dev()).to(BF16)
    nw = (1 + 0.1 * torch.randn(K, generator=gd, device=dev())).to(BF16)
    src = ops.rows_normed(x, x.float().pow(2).sum(-1).contiguous(), 1, nw, 1e-6) if normed else ops.rows_plain(x)
    out = []
    for w in (w4, wb):
        ids = torch.full((16,), -1, dtype=torch.int64, device=dev())
        logits = torch.zeros(16, V, dtype=BF16, device=dev())
        ops.gemm_sample(w, src, V, K, 0, 13, ops.argmax_ws(dev()), ids, 0, seed=2 ** 63 + 3, temperature=T, pos_base=4321,
                        pos_add=1, logits=logits)
        out.append((ids, logits))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int16), out[1][1].view(torch.int16))
    assert float((out[0][0][:13] != out[1][1][:13].float().argmax(-1)).float().mean()) > 0.5   # draws, not the argmax
