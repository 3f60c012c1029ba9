"""Plain reference of the seam between the ragged-batch K-part GEMM and the residual-norm launch, and of the layer loop
built on it (dflash_amd/tile_stack.py).  torch on whatever device the inputs live on, numpy for the summation-order
model; nothing here imports dflash_amd.ops or needs a GPU.

    dfl_gemm_f32_batch   out[k][r*16+m][n]: fp32 K-part sums, parts batch_tiles(R)*16*N floats apart
    dfl_norm_frag_batch  h <- bf16(h + bf16(part 0 + part 1 + ...)), tap <- h, frag <- norm_w * bf16(h * rstd)

The host rules of csrc/gemm_rows.h / csrc/gemm_batch.hip are mirrored (batch_tiles, batch_ksplit, grid_x_for,
tiles_per_wg) so that a test can name, and a CPU test can pin, the launch form each of its shapes reaches."""
from __future__ import annotations

import numpy as np
import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ---------------------------------------------------------------- host rules (gemm_rows.h, gemm_batch.hip)
def batch_tiles(R: int) -> int:
    return 2 if R <= 2 else 4


def batch_ksplit(K: int) -> int:
    return (K // 32 + 63) // 64


def part_ksteps(K: int) -> int:
    """k-steps of 32 columns one K part covers: 8 waves x nfr (fill_batch)."""
    ks = batch_ksplit(K)
    return 8 * ((K // 32 + 8 * ks - 1) // (8 * ks))


def grid_x_for(ngroups: int, ksplit: int = 1) -> int:
    gx_max = max(256 // ksplit, 1)
    per_wg = (ngroups + gx_max - 1) // gx_max
    return (ngroups + per_wg - 1) // per_wg


def tiles_per_wg(N: int, K: int) -> list:
    """The distinct numbers of 16-column tiles the workgroups of k_gemm_b<MT, EPI_F32> walk (tiles bx, bx + gx, ...)."""
    nt = N // 16
    gx = grid_x_for(nt, batch_ksplit(K))
    return sorted({(nt - 1 - b) // gx + 1 for b in range(gx)})


def gemm_form_id(N: int, K: int) -> str:
    return f"ks{batch_ksplit(K)}-gx{grid_x_for(N // 16, batch_ksplit(K))}-t{'_'.join(map(str, tiles_per_wg(N, K)))}"


def norm_maxc(H: int) -> int:
    """The k_norm_frag_b<MAXC> instantiation dfl_norm_frag_batch picks."""
    return 2 if H <= 4096 else 4 if H <= 8192 else 8


# ---------------------------------------------------------------- frag16: [K/8][16][8], element (m, k) at ((k/8)*16 + m)*8 + k%8
def frag16_pack(x: torch.Tensor) -> torch.Tensor:
    """rows [16, K] -> flat frag16 [16*K]."""
    K = x.shape[1]
    return x.reshape(16, K // 8, 8).permute(1, 0, 2).reshape(-1)


def frag16_unpack(frag: torch.Tensor, K: int) -> torch.Tensor:
    """flat frag16 (the first 16*K elements of frag) -> rows [16, K]."""
    return frag[:16 * K].reshape(K // 8, 16, 8).permute(1, 0, 2).reshape(16, K)


def bf16_steps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Distance in bf16 steps (the bit patterns mapped onto a monotonic integer line)."""
    def line(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (line(a) - line(b)).abs()


# ---------------------------------------------------------------- the two launches
def parts_add_ref(h: torch.Tensor, parts: torch.Tensor, nsplit: int) -> torch.Tensor:
    """bf16(h + bf16(acc)), acc = fp32 zero + parts[0] + parts[1] + ... in that order: the IEEE operations of
    k_norm_frag_b in its order ("fixed part order"), so the result is compared bit for bit.  h [..., H] bf16,
    parts [>= nsplit, ..., H] fp32."""
    assert h.dtype == BF16 and parts.dtype == F32
    acc = torch.zeros_like(parts[0])
    for k in range(nsplit):
        acc = acc + parts[k]
    return (h.float() + acc.to(BF16).float()).to(BF16)


def rms_frag_ref(h_new: torch.Tensor, norm_w: torch.Tensor, eps: float) -> torch.Tensor:
    """bf16(norm_w * bf16(h * rstd)): the rounding points of oracle.dflash_oracle.rms_norm (Qwen3RMSNorm), with rstd from
    a float64 mean of squares, so that its only error is the final rounding to fp32."""
    assert h_new.dtype == BF16 and norm_w.dtype == BF16
    hd = h_new.double()
    rstd = torch.rsqrt(hd.pow(2).mean(-1, keepdim=True) + eps).float()
    return (norm_w.float() * (h_new.float() * rstd).to(BF16).float()).to(BF16)


def kernel_order_rstd(h_new: torch.Tensor, eps: float) -> torch.Tensor:
    """rstd as k_norm_frag_b sums it, in fp32: thread t of 256 adds the squares of its 8-element chunks t, t + 256, ...
    one after the other; a pairwise tree over the 16 lanes of a row, the 4 rows of a wave in order, the 4 waves in
    order; / H + eps; 1 / sqrt.  h_new [rows, H] bf16 -> [rows, 1] fp32."""
    x = h_new.float().cpu().numpy().astype(np.float32)
    rows, H = x.shape
    nch = H // 8
    per = -(-nch // 256)
    sq = np.zeros((rows, per * 256, 8), dtype=np.float32)
    sq[:, :nch] = (x * x).reshape(rows, nch, 8)
    sq = sq.reshape(rows, per, 256, 8)
    ss = np.zeros((rows, 256), dtype=np.float32)
    for i in range(per):
        for j in range(8):
            ss = (ss + sq[:, i, :, j]).astype(np.float32)
    t = ss.reshape(rows, 4, 4, 16)                      # [wave][row of 16 lanes][lane]
    for _ in range(4):
        t = (t[..., 0::2] + t[..., 1::2]).astype(np.float32)
    t = t[..., 0]
    wave = ((t[..., 0] + t[..., 1]).astype(np.float32) + t[..., 2]).astype(np.float32)
    wave = (wave + t[..., 3]).astype(np.float32)       # [rows, 4]
    tot = ((wave[:, 0] + wave[:, 1]).astype(np.float32) + wave[:, 2]).astype(np.float32)
    tot = (tot + wave[:, 3]).astype(np.float32)
    var = (tot / np.float32(H)).astype(np.float32) + np.float32(eps)
    rstd = (np.float32(1) / np.sqrt(var.astype(np.float32))).astype(np.float32)
    return torch.from_numpy(rstd).reshape(rows, 1)


def rms_frag_with_rstd(h_new: torch.Tensor, norm_w: torch.Tensor, rstd: torch.Tensor) -> torch.Tensor:
    return (norm_w.float() * (h_new.float() * rstd.float()).to(BF16).float()).to(BF16)


# ---------------------------------------------------------------- inputs of the norm-launch tests (shared by CPU and GPU tests)
NORM_H = (8, 2048, 2560, 4096, 4104, 5120, 8192, 8200, 16384)
FLIP_CAP = 2e-3     # share of elements a last-bit difference in rstd may move (tests/test_hip_prefill.py uses the same cap)
EPS = 1e-6


def norm_case_data(H: int, MT: int, nsplit: int, seed: int):
    """h [MT, 16, H] bf16 with a per-row scale spread of ~30x; parts [nsplit, MT*16, H] fp32 of mixed sign whose sum
    partly cancels (so that rounding the sum before the add and rounding once differ in many elements);
    norm_w = 1 + 0.1 randn.  Drawn in float64 on the CPU (the same bits on every host)."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.exp(torch.rand(MT, 16, 1, generator=g, dtype=F64) * np.log(30.0)) * 0.2
    h = (torch.randn(MT, 16, H, generator=g, dtype=F64) * scale).to(BF16)
    parts = torch.randn(max(nsplit, 1), MT * 16, H, generator=g, dtype=F64) * 2.0
    if nsplit >= 2:
        parts[nsplit - 1] = -0.9 * parts[:nsplit - 1].sum(0) + 0.3 * torch.randn(MT * 16, H, generator=g, dtype=F64)
    parts = (parts * scale.reshape(1, MT * 16, 1)).to(F32)
    norm_w = (1 + 0.1 * torch.randn(H, generator=g, dtype=F64)).to(BF16)
    return h, parts, norm_w


# ---------------------------------------------------------------- TileStack.run + finish, restated
def _bf(x: torch.Tensor) -> torch.Tensor:
    """One bf16 rounding, kept in float64."""
    return x.to(BF16).double()


def _rms64(h: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    rstd = torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)
    return _bf(w.double() * _bf(h * rstd))


def stack_ref(h0: torch.Tensor, layers: list, final_norm: torch.Tensor, eps: float, q_dim: int, tap_layers=(),
              attend=None):
    """TileStack.run + finish for the rows h0 [n, H] (bf16) of one tile, in float64 with bf16 roundings where the kernels
    round: Linear outputs, bf16(h + bf16(o)) and bf16(h + bf16(down or the sum of the expert shares)),
    bf16(bf16(silu(bf16 g)) * bf16 u), the norm.  layers: dicts of plain [out, in] weights — ln1, qkv, o, ln2 and either
    gate / up / down (dense) or experts = [We_0, We_1, ...] (shares x_norm @ We_s^T).  attend(q) -> attention rows from
    the q columns (default: bf16(tanh(q))).  Returns (h, taps [n, len(tap_layers) * H] — a repeated id gives equal
    copies — and the final normalised rows)."""
    attend = attend or (lambda q: _bf(torch.tanh(q)))
    d = lambda w: w.double()  # noqa: E731
    h = h0.double()
    H = h.shape[1]
    taps = torch.zeros(h.shape[0], len(tap_layers) * H, dtype=F64)
    pend = None
    for i, lw in enumerate(layers):
        if pend is not None:
            h = _bf(h + _bf(pend))
            for j, l in enumerate(tap_layers):
                if l == i - 1:
                    taps[:, j * H:(j + 1) * H] = h
        xn = _rms64(h, lw["ln1"], eps)
        qkv = _bf(xn @ d(lw["qkv"]).T)
        a = attend(qkv[:, :q_dim])
        h = _bf(h + _bf(a @ d(lw["o"]).T))
        xn = _rms64(h, lw["ln2"], eps)
        if "experts" in lw:
            pend = sum(xn @ d(we).T for we in lw["experts"])
        else:
            g, u = _bf(xn @ d(lw["gate"]).T), _bf(xn @ d(lw["up"]).T)
            act = _bf(_bf(torch.nn.functional.silu(g)) * u)
            pend = act @ d(lw["down"]).T
    h = _bf(h + _bf(pend))
    return h.to(BF16), taps.to(BF16), _rms64(h, final_norm, eps).to(BF16)


# ---------------------------------------------------------------- shapes of the K-part GEMM tests (shared by CPU and GPU tests)
# (N, K), each run at R = 1..4.  K = 32: one k-step, so 7 of the 8 waves have none, and N = 4096 n gives every one of the
# 256 workgroups n tiles (the three-buffer rotation leaves its loop at j+1 >= nseq or j+2 >= nseq, or runs it out);
# N = 16 * 1546, K = 64: 220 workgroups with 7 tiles and one with 6; K = 2080: a second part shorter than the first;
# K = 32768: 16 parts, the limit.
GEMM_SMALL = [(4096 * n, 32) for n in range(1, 9)] + [(16 * 1546, 64), (48, 2080), (64, 32768)]
# the model points, run at R = 4: Qwen3-8B o / down, Qwen3-4B o / down, hidden 5120 o / down
GEMM_MODEL = [(4096, 4096), (4096, 12288), (2560, 4096), (2560, 9728), (5120, 5120), (5120, 17408)]
GEMM_K_REJECTED = 32800
# (H, K) of the chained GEMM -> norm tests
CHAIN_CASES = [(512, 2112), (2560, 9728), (4096, 12288)]


# ---------------------------------------------------------------- cases of the norm-launch test
NORM_K_OF = {1: 2048, 2: 4096, 6: 12288, 8: 16384}      # via K: nsplit = dfl_batch_ksplit(K)
# (H, R, nsplit, via, valid rows per request (None: dyn = NULL), tap slot)
NORM_CASES = [
    (8, 1, 1, "K", [9], 0),                        # one chunk in all: 255 threads clamped
    (8, 4, 8, "shares", [16, 9, 1, 0], 2),
    (2048, 2, 2, "K", [16, 1], 0),                 # exactly one chunk per thread
    (2048, 4, 2, "shares", [16, 16, 16, 16], None),
    (2560, 3, 6, "K", [9, 0, 16], 2),              # a partial second chunk
    (2560, 4, 2, "K", None, 0),
    (4096, 4, 8, "shares", [1, 16, 0, 9], 0),      # MAXC = 2 at its limit
    (4096, 1, 6, "K", [16], None),
    (4096, 3, 0, None, [16, 9, 0], 2),             # part = NULL with a tap: a pure copy
    (4104, 2, 1, "shares", [9, 16], 2),            # MAXC = 4, one chunk past 2 x 256
    (5120, 3, 2, "K", [16, 9, 1], 0),
    (8192, 4, 6, "K", [16, 0, 9, 1], 2),           # MAXC = 4 at its limit
    (8200, 1, 6, "shares", [9], 0),                # MAXC = 8, one chunk past 4 x 256
    (8200, 3, 2, "K", [16, 16, 9], 2),
    (16384, 4, 8, "K", [16, 9, 1, 0], 2),          # the limit
    (16384, 2, 1, "K", [0, 16], 0),
]


def norm_case_id(c) -> str:
    valid = "nodyn" if c[4] is None else "v" + "_".join(map(str, c[4]))
    return f"H{c[0]}-maxc{norm_maxc(c[0])}-R{c[1]}-ns{c[2]}{c[3] or ''}-{valid}-tap{c[5]}"
