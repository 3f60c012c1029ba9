// Logit bias, token allow / ban lists and min_tokens on the verify's materialised logits.
//   k_bias_rows: one 1024-thread block per row of bf16 logits [tiles][16][V], the row / tile conventions of nucleus.hip.
//                Row m of tile j of slot q adds the slot's dense fp32 table row b[V] (0: the logit's bits copied, -inf: a
//                ban, else one fp32 add rounded to bf16) and, while the position it predicts lies before the slot's
//                min_pos, sets the stop ids to -inf:
//   1. a suppressed row's stop ids (few) flag their 8-column chunks first
//   2. the dense pass: 16-byte loads of logits and table, the select, a flagged chunk patched in registers, 16-byte
//      stores, running argmax (lowest column on ties)
// No floating-point atomics: the same inputs give the same bits, eager or replayed.
#include "dfl_common.h"

#pragma clang fp contract(off)  // the whole file: the add is an add, rounded once

namespace {

constexpr int LB_NT = 1024;               // threads per row
constexpr int LB_VMAX = 155648;           // the row kernels' common limit (19 * 1024 * 8)
constexpr int LB_FLAG_WORDS = LB_VMAX / 8 / 32;
constexpr int LB_NONE = 0x7fffffff;
constexpr int LB_MAX_STOP = 64;           // stop ids one launch takes
constexpr uint32_t LB_NEG_INF = 0xff80u;  // bf16 -inf

struct BiasArgs {
  const bf16_t *logits;
  bf16_t *out;
  int64_t ld, tile_stride;
  int V, row0, nrows;
  const int32_t *dyn;
  int nrows_word, tiles_per_req;
  const float *bias;
  int64_t bias_stride;
  const int32_t *min_pos_dev;
  int min_pos;
  const int64_t *stop_ids;
  int n_stop, pos_word, pos_base, pos_add;
  int64_t *out_ids;
  int64_t out_stride;
  int out_off;
};

__device__ __forceinline__ float lb_f(uint32_t b) { return __builtin_bit_cast(float, b << 16); }

// The contract's select, the add rounded once in fp32 and once to bf16.  A table value that is NaN or +inf reads as 0;
// a NaN logit keeps its bits under a finite bias.
__device__ __forceinline__ uint32_t lb_value(uint32_t xb, float b) {
  if (b == -INFINITY) return LB_NEG_INF;
  if (b == 0.f || !(b < INFINITY)) return xb;
  const float x = lb_f(xb);
  if (x != x) return xb;
  uint32_t u = __builtin_bit_cast(uint32_t, x + b);
  u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even; an overflow rounds to inf
  return u >> 16;
}

__global__ __launch_bounds__(LB_NT) void k_bias_rows(BiasArgs a) {
  __shared__ uint32_t flags[LB_FLAG_WORDS];
  __shared__ int sstop[LB_MAX_STOP];
  __shared__ float sv[16];
  __shared__ int si[16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.y;
  int rows = a.nrows;
  if (a.dyn && a.nrows_word >= 0) rows = a.dyn[t * DFL_DYN_WORDS + a.nrows_word] - a.row0;
  if ((int)blockIdx.x >= rows) return;  // block-uniform: rows past the tile's valid count are not written
  const int m = a.row0 + blockIdx.x;
  const int q = t / a.tiles_per_req, j = t - q * a.tiles_per_req;
  const int V = a.V, nchunks = V >> 3;
  const int base = (a.dyn && a.pos_word >= 0) ? a.dyn[t * DFL_DYN_WORDS + a.pos_word] : a.pos_base;
  const int64_t pos = (int64_t)base + a.pos_add + 16 * j + m;
  const int min_pos = a.min_pos_dev ? a.min_pos_dev[q] : a.min_pos;
  const int n = (a.n_stop > 0 && pos < (int64_t)min_pos) ? a.n_stop : 0;  // stop ids this row suppresses

  const bf16_t *row = a.logits + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  bf16_t *dst = a.out + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  const float *tab = a.bias + (int64_t)q * a.bias_stride;

  if (n > 0) {  // block-uniform
    for (int w = tid; w < (nchunks + 31) >> 5; w += LB_NT) flags[w] = 0u;
    __syncthreads();
    if (tid < n) {
      const int64_t v = a.stop_ids[tid];
      const bool in = v >= 0 && v < V;  // an id outside the vocabulary is ignored, never indexed
      sstop[tid] = in ? (int)v : -1;
      if (in) atomicOr(&flags[v >> 8], 1u << ((v >> 3) & 31));
    }
    __syncthreads();
  }

  float best = -INFINITY;
  int bi = LB_NONE;
  for (int c = tid; c < nchunks; c += LB_NT) {
    const u32x4 x = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
    const u32x4 w0 = *reinterpret_cast<const u32x4 *>(tab + (int64_t)c * 8);
    const u32x4 w1 = *reinterpret_cast<const u32x4 *>(tab + (int64_t)c * 8 + 4);
    uint32_t zb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t xb = (x[e >> 1] >> (16 * (e & 1))) & 0xffffu;
      const uint32_t w = e < 4 ? w0[e & 3] : w1[e & 3];
      zb[e] = w == 0u ? xb : lb_value(xb, __builtin_bit_cast(float, w));
    }
    if (n > 0 && ((flags[c >> 5] >> (c & 31)) & 1u)) {  // a chunk with a stop id (at most n per row)
      for (int k = 0; k < n; ++k) {
        const int tk = sstop[k];
        if ((tk >> 3) == c) {  // (-1 >> 3 is no chunk)
#pragma unroll
          for (int e = 0; e < 8; ++e) zb[e] = (e == (tk & 7)) ? LB_NEG_INF : zb[e];
        }
      }
    }
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if (e & 1)
        o[e >> 1] |= zb[e] << 16;
      else
        o[e >> 1] = zb[e];
      const float z = lb_f(zb[e]);
      if (z > best || (bi == LB_NONE && z == z)) {  // columns ascend within a thread; a NaN is never the maximum
        best = z;
        bi = c * 8 + e;
      }
    }
    *reinterpret_cast<u32x4 *>(dst + (int64_t)c * 8) = o;
  }
  if (!a.out_ids) return;  // block-uniform
  auto take = [&](float ov, int oi) {
    if (oi != LB_NONE && (bi == LB_NONE || ov > best || (ov == best && oi < bi))) {
      best = ov;
      bi = oi;
    }
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    take(ov, oi);
  }
  if (lane == 0) {
    sv[wave] = best;
    si[wave] = bi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) take(sv[w], si[w]);
    a.out_ids[(int64_t)t * a.out_stride + a.out_off + blockIdx.x] = (int64_t)(bi == LB_NONE ? 0 : bi);
  }
}

}  // namespace

extern "C" int dfl_logit_bias_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V,
                                   int row0, int nrows, const int32_t *dyn, int nrows_dyn_word, int tiles_per_req,
                                   const float *bias, int64_t bias_stride, const int32_t *min_pos_dev, int min_pos,
                                   const int64_t *stop_ids, int n_stop, int pos_word, int pos_base, int pos_add,
                                   int64_t *out_ids, int64_t out_stride, int out_off, void *stream) {
  DFL_REQUIRE(logits && out && bias, "dfl_logit_bias_rows: null pointer");
  DFL_REQUIRE(V >= 1 && V % 8 == 0 && V <= LB_VMAX, "dfl_logit_bias_rows: V=%d is not a multiple of 8 in 8..%d", V, LB_VMAX);
  DFL_REQUIRE(tiles_per_req == 1 || tiles_per_req == 2, "dfl_logit_bias_rows: tiles_per_req=%d", tiles_per_req);
  DFL_REQUIRE(tiles >= 0 && ld >= V && ld % 8 == 0 && (tiles <= 1 || (tile_stride >= 16 * ld && tile_stride % 8 == 0)) &&
                  ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
              "dfl_logit_bias_rows: bad shape tiles=%d ld=%lld tile_stride=%lld (rows on 16 bytes)", tiles, (long long)ld,
              (long long)tile_stride);
  DFL_REQUIRE(bias_stride >= V && bias_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(bias) & 15) == 0,
              "dfl_logit_bias_rows: bias_stride=%lld (>= V, a multiple of 4, rows on 16 bytes)", (long long)bias_stride);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "dfl_logit_bias_rows: rows [%d,%d) outside the tile", row0,
              row0 + nrows);
  DFL_REQUIRE(nrows_dyn_word < DFL_DYN_WORDS && pos_word < DFL_DYN_WORDS && ((nrows_dyn_word < 0 && pos_word < 0) || dyn),
              "dfl_logit_bias_rows: nrows_dyn_word=%d / pos_word=%d need a record inside dyn", nrows_dyn_word, pos_word);
  DFL_REQUIRE(n_stop >= 0 && n_stop <= LB_MAX_STOP && (n_stop == 0 || stop_ids),
              "dfl_logit_bias_rows: n_stop=%d (0..%d, with stop_ids)", n_stop, LB_MAX_STOP);
  DFL_REQUIRE(min_pos_dev || min_pos >= 0, "dfl_logit_bias_rows: min_pos=%d is negative", min_pos);
  DFL_REQUIRE(out_stride >= 0 && out_off >= 0, "dfl_logit_bias_rows: negative stride or offset");
  if (tiles == 0 || (nrows == 0 && nrows_dyn_word < 0)) return DFL_OK;
  BiasArgs p{(const bf16_t *)logits, (bf16_t *)out, ld,          tile_stride, V,        row0,   nrows,    dyn,
             nrows_dyn_word,         tiles_per_req, bias,        bias_stride, min_pos_dev, min_pos, stop_ids, n_stop,
             pos_word,               pos_base,      pos_add,     out_ids,     out_stride, out_off};
  hipLaunchKernelGGL(k_bias_rows, dim3(nrows_dyn_word >= 0 ? 16 - row0 : nrows, tiles), dim3(LB_NT), 0,
                     (hipStream_t)stream, p);
  DFL_CHECK_LAUNCH("dfl_logit_bias_rows");
  return DFL_OK;
}
