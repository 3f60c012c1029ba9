// Prompt logprobs: the lm_head over the PREFILL rows with a log-softmax epilogue that never writes a
// logit.  out[m] = z_m[targets[m]] - ln(sum_v exp(z_m[v])), z = the bf16-rounded logits the materialising head launches
// define (fp32 MFMA sums, one rounding), raw distribution at T = 1 — section 12's definition, over P - 1 rows instead of 16.
//
// Operands as k_pgemm (prefill.hip): the packed head [V/16][K/32][64 lanes][8 bf16] is the MFMA A operand, the final-normed
// frag16 row tiles [rows_padded/16][K/32][64][8] the B operand, both staged by LDS-DMA (1 KiB per wave instruction,
// lane-linear) into a two-stage ring and read back with ds_read_b128.  The work split is its own:
//   * a workgroup (4 waves, 2 x 2, each 64 columns x 64 rows) owns ONE 128-row block and ONE strip of 128-column blocks and
//     walks the strip; the K loop runs THROUGH the column-block boundaries — step t = (column block, 64-deep K step) is
//     one linear sequence, so the ring never drains: the first stage of the next column block is in flight while the
//     epilogue of the current one runs on the VALU (and the other workgroup of the CU keeps the matrix pipe busy);
//   * the epilogue keeps, per lane and per row (4 rows: row l & 15 of the wave's 4 row tiles), a running maximum m in the
//     logits' own units (bf16 values: exact), the sum l of exp2((z - m) log2 e) rescaled when m rises, and the logit of
//     the target column if one of the lane's 16 columns is it.  No cross-lane traffic inside the strip;
//   * at the end of the strip the four 16-lane groups meet through v_permlane16/32_swap, the two column waves through
//     768 bytes of LDS, and ONE (m, l, z_t) per (strip, row) goes to ws;
//   * k_plogprob_finish, a second launch (a launch boundary is the cheapest grid-wide dependency here: DESIGN section 7),
//     merges the nsplit partials of a row in a fixed order, one wave per row.
// Every row block of a strip shares blockIdx % 8 — an XCD and its L2 — and they walk the strip's column blocks in step, so
// a column block's weights leave HBM once for all the prompt's row blocks that are resident (grid order, no host loop;
// the grid is padded to whole groups of 8 strips so that this holds for the last strips too).
// Columns past V in the last column block (V % 128 != 0, V % 16 == 0): whole 16-column tiles, masked to -inf by a
// wave-uniform test; their weight requests are clamped to the last real tile.  No load sits under a branch.
#include "dfl_common.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;

constexpr float PL_LOG2E = 1.4426950408889634f;

struct PLogprobArgs {
  const bf16x8 *wp;  // [ntiles][KS][64]
  const bf16x8 *xf;  // [rows_padded / 16][KS][64]
  int KS, ntiles, ncb, nsplit, nrb, rows, V;
  int64_t rows_padded;
  const int64_t *targets;
  f32x4 *ws;  // [nsplit][rows_padded]: (m, l, z_t, 0)
};

__device__ __forceinline__ void plswap16(float &a, float &b) { asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
__device__ __forceinline__ void plswap32(float &a, float &b) { asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b)); }
// max / sum over the four 16-lane groups of the wave, result in every lane (pg_max / pg_sum of prefill.hip)
__device__ __forceinline__ float pl_gmax(float v) {
  float a = v, b = v;
  plswap16(a, b);
  a = b = fmaxf(a, b);
  plswap32(a, b);
  return fmaxf(a, b);
}
__device__ __forceinline__ float pl_gsum(float v) {
  float a = v, b = v;
  plswap16(a, b);
  a = b = a + b;
  plswap32(a, b);
  return a + b;
}
// exp(x - ref) through the hardware's base-2 exponential; x = -inf gives 0, ref is finite
__device__ __forceinline__ float pl_exp(float x, float ref) { return __builtin_amdgcn_exp2f((x - ref) * PL_LOG2E); }
// (m, l) += (pm, pl): the larger maximum, both sums rescaled to it.  Symmetric in its two sides: a butterfly of it leaves
// the same bits in both lanes.
__device__ __forceinline__ void pl_merge(float &m, float &l, float pm, float pl) {
  const float mn = fmaxf(m, pm), ref = mn == -INFINITY ? 0.f : mn;
  l = l * pl_exp(m, ref) + pl * pl_exp(pm, ref);
  m = mn;
}

__global__ __launch_bounds__(256) void k_plogprob(PLogprobArgs a) {
  // [stage][slot: 0..15 = W (n tile, k-step), 16..31 = X (m tile, k-step)][lane]: 64 KiB, two workgroups per CU
  __shared__ bf16x8 lds[2][32][64];
  __shared__ float red[2][64][3];  // the column wave wn = 1 hands its rows' (m, l, z_t) to wn = 0
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63, fm = l & 15, fg = l >> 4;
  const int wn = w & 1, wm = w >> 1;
  // strip / row block of this workgroup: strips in groups of 8, the nrb row blocks of a strip 8 apart in blockIdx, i.e.
  // on one XCD.  The grid is padded to whole groups (k_pgemm packs its last group `tail` apart instead, which takes its
  // row blocks off a common XCD): a workgroup of a strip past the last does nothing.
  const int per = 8 * a.nrb, grp = (int)blockIdx.x / per, rem = (int)blockIdx.x - grp * per;
  const int strip = grp * 8 + (rem & 7), rb = rem >> 3;
  if (strip >= a.nsplit) return;  // workgroup-uniform, in front of every barrier
  const int KT = a.KS >> 1;  // 64-deep steps per column block
  const int c0 = (int)((int64_t)strip * a.ncb / a.nsplit), c1 = (int)((int64_t)(strip + 1) * a.ncb / a.nsplit);
  const int nsteps = (c1 - c0) * KT;  // >= KT: nsplit <= ncb

  // the target column of the lane's four rows; -1: none (a row past `rows`, an id outside [0, V))
  int tgt[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = rb * 128 + (wm * 4 + j) * 16 + fm;
    const int64_t t = a.targets[row < a.rows ? row : a.rows - 1];
    tgt[j] = (row < a.rows && t >= 0 && t < a.V) ? (int)t : -1;
  }

  // step (cb, kt) -> buffer: 16 weight + 16 activation fragments of 1 KiB, dealt round-robin to the 4 waves
  auto stage = [&](int cb, int kt, int buf) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int slot = i * 4 + w;  // wave-uniform
      const int s16 = slot & 15;   // fragment of its operand: (tile s16 >> 1, k-step s16 & 1)
      int tile = cb * 8 + (s16 >> 1);
      tile = tile < a.ntiles ? tile : a.ntiles - 1;  // (the masked tail tiles of the last column block)
      const bf16x8 *src = (slot < 16 ? a.wp + ((size_t)tile * a.KS + kt * 2 + (s16 & 1)) * 64
                                     : a.xf + ((size_t)(rb * 8 + (s16 >> 1)) * a.KS + kt * 2 + (s16 & 1)) * 64) + l;
      __builtin_amdgcn_global_load_lds((glb_void *)src, (lds_void *)&lds[buf][slot][0], 16, 0, 0);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float rm[4], rl[4], rz[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    rm[j] = -INFINITY;
    rl[j] = 0.f;
    rz[j] = -INFINITY;
  }

  int scb = c0, skt = 0;  // the next step to request
  auto request = [&](int buf) {
    stage(scb, skt, buf);
    if (++skt == KT) {
      skt = 0;
      ++scb;
    }
  };
  request(0);
  int buf = 0, kt = 0, cb = c0;
  for (int t = 0; t < nsteps; ++t) {
    // this wave's share of step t has landed (the ring holds one step in flight: the count is 0) ...
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // ... and everyone's; every wave is done reading the buffer of step t - 1.  A bare s_barrier (prefill.hip).
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 1 < nsteps) request(buf ^ 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[4], bq[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = lds[buf][(wn * 4 + i) * 2 + ks][l];
#pragma unroll
      for (int j = 0; j < 4; ++j) bq[j] = lds[buf][16 + (wm * 4 + j) * 2 + ks][l];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bq[j], acc[i][j], 0, 0, 0);
    }
    buf ^= 1;
    if (++kt < KT) continue;
    // ---- the column block is complete: fold its 64 columns x 64 rows into the running (m, l, z_t) ----
    // D layout: lane (fm, fg), acc[i][j][r] = column (cb * 8 + wn * 4 + i) * 16 + 4 fg + r of row tile wm * 4 + j, row fm
    const int nt0 = cb * 8 + wn * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float z[16], bm = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool real = nt0 + i < a.ntiles;  // wave-uniform
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          z[4 * i + r] = real ? rbf(acc[i][j][r]) : -INFINITY;
          bm = fmaxf(bm, z[4 * i + r]);
          acc[i][j][r] = 0.f;
        }
      }
      const float mn = fmaxf(rm[j], bm), ref = mn == -INFINITY ? 0.f : mn;
      float ps = 0.f;  // the block's 16 terms first, then ONE add into the running sum
#pragma unroll
      for (int c = 0; c < 16; ++c) ps += pl_exp(z[c], ref);
      rl[j] = rl[j] * pl_exp(rm[j], ref) + ps;
      rm[j] = mn;
      const int d = tgt[j] - (nt0 * 16 + 4 * fg);  // the target among this lane's columns: d = 16 i + r
      if ((unsigned)d < 64u && (d & 15) < 4) {
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (d == (c >> 2) * 16 + (c & 3)) rz[j] = z[c];
      }
    }
    kt = 0;
    ++cb;
  }

  // ---- the strip is done: the four 16-lane groups, then the two column waves ----
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float M = pl_gmax(rm[j]), ref = M == -INFINITY ? 0.f : M;
    rl[j] = pl_gsum(rl[j] * pl_exp(rm[j], ref));
    rm[j] = M;
    rz[j] = pl_gmax(rz[j]);
    if (wn == 1 && fg == 0) {
      red[wm][j * 16 + fm][0] = rm[j];
      red[wm][j * 16 + fm][1] = rl[j];
      red[wm][j * 16 + fm][2] = rz[j];
    }
  }
  __syncthreads();
  if (wn == 0 && fg == 0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pl_merge(rm[j], rl[j], red[wm][j * 16 + fm][0], red[wm][j * 16 + fm][1]);
      const float zt = fmaxf(rz[j], red[wm][j * 16 + fm][2]);
      const int row = rb * 128 + (wm * 4 + j) * 16 + fm;  // < rows_padded: every padded row has a slot
      a.ws[(int64_t)strip * a.rows_padded + row] = (f32x4){rm[j], rl[j], zt, 0.f};
    }
  }
}

// one wave per row: the lanes take the strips 64 apart, then a butterfly of the symmetric merge (one fixed order: the
// same partials give the same bits on every run)
__global__ __launch_bounds__(256) void k_plogprob_finish(const f32x4 *ws, int nsplit, int64_t rows_padded, int rows, int V,
                                                         const int64_t *targets, float *out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;  // wave-uniform: rows past the count are not written
  float m = -INFINITY, l = 0.f, zt = -INFINITY;
  for (int s = lane; s < nsplit; s += 64) {
    const f32x4 p = ws[(int64_t)s * rows_padded + row];
    pl_merge(m, l, p[0], p[1]);
    zt = fmaxf(zt, p[2]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    pl_merge(m, l, __shfl_xor(m, o, 64), __shfl_xor(l, o, 64));
    zt = fmaxf(zt, __shfl_xor(zt, o, 64));
  }
  if (lane == 0) {
    const int64_t t = targets[row];
    out[row] = (t >= 0 && t < V) ? zt - (m + logf(l)) : __builtin_nanf("");
  }
}

}  // namespace

extern "C" int dfl_prefill_logprobs(const void *wp_head, const void *x_frag, int rows, int V, int K, const int64_t *targets,
                                    int nsplit, float *ws, float *out, void *stream) {
  DFL_REQUIRE(wp_head && x_frag && targets && ws && out, "dfl_prefill_logprobs: null pointer");
  DFL_REQUIRE(rows >= 1 && V > 0 && V % 16 == 0 && K > 0 && K % 64 == 0,
              "dfl_prefill_logprobs: need rows >= 1, V%%16==0, K%%64==0 (rows=%d V=%d K=%d)", rows, V, K);
  const int ncb = (V + 127) / 128;
  DFL_REQUIRE(nsplit >= 1 && nsplit <= ncb, "dfl_prefill_logprobs: nsplit=%d outside 1..%d (the 128-column blocks of V=%d)",
              nsplit, ncb, V);
  const int nrb = (rows + 127) / 128;
  DFL_REQUIRE(((uintptr_t)ws & 15) == 0, "dfl_prefill_logprobs: ws must be 16-byte aligned");
  DFL_REQUIRE(((int64_t)nsplit + 7) / 8 * 8 * nrb <= 0x7fffffff, "dfl_prefill_logprobs: nsplit=%d x %d row blocks exceed the grid", nsplit, nrb);
  PLogprobArgs a{(const bf16x8 *)wp_head, (const bf16x8 *)x_frag, K / 32, V / 16, ncb, nsplit, nrb, rows, V,
                 (int64_t)nrb * 128, targets, (f32x4 *)ws};
  hipLaunchKernelGGL(k_plogprob, dim3((nsplit + 7) / 8 * 8 * nrb), dim3(256), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(k_plogprob_finish, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const f32x4 *)ws, nsplit,
                     (int64_t)nrb * 128, rows, V, targets, out);
  DFL_CHECK_LAUNCH("dfl_prefill_logprobs");
  return DFL_OK;
}
