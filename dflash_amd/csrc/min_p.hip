// min_p: a probability floor relative to the top token, on the verify's materialised logits.
//   k_min_p_rows: one 1024-thread block per row of bf16 logits [tiles][16][V], the row / tile conventions of nucleus.hip
//                 and logit_bias.hip.  Row m of tile j of slot q keeps column v iff exp(invT (x_v - max)) >= min_p, written
//                 in the log domain with L = ln(min_p) from the host: (x_v - max) * invT >= L.  Everything else is -inf.
//   1. the row, once: 16-byte loads into registers (19 per thread at V = 155648)
//   2. the maximum over the values that are not NaN: per thread, the wave's butterfly, the 16 wave values through LDS
//   3. the select from registers, 16-byte stores, the kept count (integer sums in a fixed order)
// No atomics at all: the same inputs give the same bits, eager or replayed.
#include "dfl_common.h"

#pragma clang fp contract(off)  // the whole file: a subtraction and a multiplication, each rounded once

namespace {

constexpr int MP_NT = 1024;               // threads per row
constexpr int MP_NCH = 19;                // 16-byte chunks per thread: V <= 19 * 1024 * 8
constexpr int MP_VMAX = MP_NCH * MP_NT * 8;
constexpr uint32_t MP_NEG_INF = 0xff80u;  // bf16 -inf

struct MinPArgs {
  const bf16_t *logits;
  bf16_t *out;
  int64_t ld, tile_stride;
  int V, row0, nrows;
  const int32_t *dyn;
  int nrows_word, tiles_per_req;
  const float *log_min_p_dev;
  float log_min_p;
  const float *inv_t_dev;
  float inv_t;
  int32_t *kept_out;
  int64_t kept_stride;
  int kept_off;
};

__device__ __forceinline__ float mp_f(uint32_t b) { return __builtin_bit_cast(float, b << 16); }

__global__ __launch_bounds__(MP_NT) void k_min_p_rows(MinPArgs a) {
  __shared__ float sv[16];
  __shared__ int sc[16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.y;
  int rows = a.nrows;
  if (a.dyn && a.nrows_word >= 0) rows = a.dyn[t * DFL_DYN_WORDS + a.nrows_word] - a.row0;
  if ((int)blockIdx.x >= rows) return;  // block-uniform: rows past the tile's valid count are not written
  const int m = a.row0 + blockIdx.x;
  const int q = t / a.tiles_per_req;
  const float L = a.log_min_p_dev ? a.log_min_p_dev[q] : a.log_min_p;
  const float inv_t = a.inv_t_dev ? a.inv_t_dev[q] : a.inv_t;
  // an off slot (L = -inf, > 0 or NaN) and a greedy slot (invT not > 0) copy their rows: every bit pattern is defined
  const bool on = L <= 0.f && L > -INFINITY && inv_t > 0.f;
  const int V = a.V, nchunks = V >> 3;

  const bf16_t *row = a.logits + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  bf16_t *dst = a.out + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;

  // ---- the row, once ----
  uint32_t r[MP_NCH * 4];
  float xmax = -INFINITY;  // over the values that are not NaN; a row of NaNs keeps -inf and is copied
#pragma unroll
  for (int i = 0; i < MP_NCH; ++i) {
    const int c = i * MP_NT + tid;
    u32x4 x = {0u, 0u, 0u, 0u};
    if (c < nchunks) {
      x = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = mp_f((x[e >> 1] >> (16 * (e & 1))) & 0xffffu);
        if (v > xmax) xmax = v;  // false for a NaN
      }
    }
    r[4 * i + 0] = x[0];
    r[4 * i + 1] = x[1];
    r[4 * i + 2] = x[2];
    r[4 * i + 3] = x[3];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(xmax, o, 64);
    if (ov > xmax) xmax = ov;
  }
  if (lane == 0) sv[wave] = xmax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w)
    if (sv[w] > xmax) xmax = sv[w];
  const bool mask = on && xmax > -INFINITY && xmax < INFINITY;  // block-uniform

  // ---- the select, from registers ----
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < MP_NCH; ++i) {
    const int c = i * MP_NT + tid;
    if (c < nchunks) {
      u32x4 o = {r[4 * i + 0], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]};
      if (mask) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t xb = (o[e >> 1] >> (16 * (e & 1))) & 0xffffu;
          const float x = mp_f(xb);
          const float d = (x - xmax) * inv_t;        // two operations, each rounded once
          const bool keep = x == xmax || d >= L;     // both false for a NaN
          cnt += keep ? 1 : 0;
          if (!keep && x == x) o[e >> 1] = (o[e >> 1] & ~(0xffffu << (16 * (e & 1)))) | (MP_NEG_INF << (16 * (e & 1)));
        }
      }
      *reinterpret_cast<u32x4 *>(dst + (int64_t)c * 8) = o;
    }
  }
  if (!a.kept_out) return;  // block-uniform
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) sc[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < 16; ++w) total += sc[w];
    a.kept_out[(int64_t)t * a.kept_stride + a.kept_off + blockIdx.x] = mask ? total : V;  // a copied row reports V
  }
}

}  // namespace

extern "C" int dfl_min_p_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V, int row0,
                              int nrows, const int32_t *dyn, int nrows_dyn_word, int tiles_per_req,
                              const float *log_min_p_dev, float log_min_p, const float *inv_t_dev, float inv_t,
                              int32_t *kept_out, int64_t kept_stride, int kept_off, void *stream) {
  DFL_REQUIRE(logits && out, "dfl_min_p_rows: null pointer");
  DFL_REQUIRE(V >= 1 && V % 8 == 0 && V <= MP_VMAX, "dfl_min_p_rows: V=%d is not a multiple of 8 in 8..%d", V, MP_VMAX);
  DFL_REQUIRE(tiles_per_req == 1 || tiles_per_req == 2, "dfl_min_p_rows: tiles_per_req=%d", tiles_per_req);
  DFL_REQUIRE(tiles >= 0 && ld >= V && ld % 8 == 0 && (tiles <= 1 || (tile_stride >= 16 * ld && tile_stride % 8 == 0)) &&
                  ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
              "dfl_min_p_rows: bad shape tiles=%d ld=%lld tile_stride=%lld (rows on 16 bytes)", tiles, (long long)ld,
              (long long)tile_stride);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "dfl_min_p_rows: rows [%d,%d) outside the tile", row0,
              row0 + nrows);
  DFL_REQUIRE(nrows_dyn_word < DFL_DYN_WORDS && (nrows_dyn_word < 0 || dyn),
              "dfl_min_p_rows: nrows_dyn_word=%d needs a record inside dyn", nrows_dyn_word);
  // (device values are not validated: an L that is -inf, > 0 or NaN is an off slot, !(invT > 0) a greedy one)
  DFL_REQUIRE(log_min_p_dev || log_min_p <= 0.f, "dfl_min_p_rows: log_min_p=%g is not <= 0 (-inf: off)", (double)log_min_p);
  DFL_REQUIRE(inv_t_dev || (inv_t > 0.f && inv_t <= 1e5f), "dfl_min_p_rows: inv_t=%g outside (0, 1e5]", (double)inv_t);
  DFL_REQUIRE(kept_stride >= 0 && kept_off >= 0, "dfl_min_p_rows: negative stride or offset");
  if (tiles == 0 || (nrows_dyn_word >= 0 ? row0 == 16 : nrows == 0)) return DFL_OK;  // nothing to do: no empty grid
  MinPArgs p{(const bf16_t *)logits, (bf16_t *)out, ld,        tile_stride, V,        row0,        nrows,   dyn, nrows_dyn_word,
             tiles_per_req,          log_min_p_dev, log_min_p, inv_t_dev,   inv_t,    kept_out,    kept_stride, kept_off};
  hipLaunchKernelGGL(k_min_p_rows, dim3(nrows_dyn_word >= 0 ? 16 - row0 : nrows, tiles), dim3(MP_NT), 0,
                     (hipStream_t)stream, p);
  DFL_CHECK_LAUNCH("dfl_min_p_rows");
  return DFL_OK;
}
