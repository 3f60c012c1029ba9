// Repetition / presence / frequency penalties on the verify's materialised logits.
//   k_penalty_count: the per-slot table int32 [V] (bit 31: seen in the prompt, bits 0..30: occurrences in the output) is
//                    kept incrementally — one workgroup per slot adds a range of ids with INTEGER atomics, so a cycle's
//                    cost does not depend on the context length and the result not on the order the adds land in.
//   k_penalty_rows:  one 1024-thread block per row of bf16 logits [tiles][16][V], the row / tile conventions of
//                    nucleus.hip.  Row m of tile j sees the table plus the block's own tokens block[1 .. 16 j + m]:
//   1. up to 31 threads take one in-block token each: the first occurrence of a token in the block counts its later
//      duplicates, reads the raw value and the table word and holds the finished value; its 8-column chunk is flagged
//   2. the dense pass: 16-byte loads of logits and table, the value from the table word alone — a flagged chunk looks
//      its columns up among the held values instead —, 16-byte stores, running argmax (lowest column on ties)
// No floating-point atomics: the same inputs give the same bits, eager or replayed.
#include "dfl_common.h"

namespace {

constexpr int PEN_NT = 1024;               // threads per row / per slot
constexpr int PEN_VMAX = 155648;           // the row kernels' common limit (19 * 1024 * 8)
constexpr int PEN_FLAG_WORDS = PEN_VMAX / 8 / 32;
constexpr int PEN_NONE = 0x7fffffff;

struct PenCountArgs {
  int32_t *table;
  int64_t table_stride;
  int V;
  const int64_t *ids;
  int64_t ids_stride;
  int ids_len;
  const int32_t *dyn;
  int lo_word, hi_word, lo, hi, as_prompt, clear;
};

__global__ __launch_bounds__(PEN_NT) void k_penalty_count(PenCountArgs a) {
  const int s = blockIdx.x, tid = threadIdx.x;
  int lo = a.lo, hi = a.hi;
  if (a.dyn) {
    const int32_t *rec = a.dyn + s * DFL_DYN_WORDS;
    if (rec[DFL_DYN_BS] == 0) return;  // block-uniform: an idle slot is skipped whole, its row is not cleared either
    lo += rec[a.lo_word];
    hi += rec[a.hi_word];
  }
  lo = max(lo, 0);
  hi = min(hi, a.ids_len);
  int32_t *row = a.table + (int64_t)s * a.table_stride;
  if (a.clear) {  // block-uniform
    const int4 z = {0, 0, 0, 0};
    for (int c = tid; 4 * c < a.V; c += PEN_NT) *reinterpret_cast<int4 *>(row + 4 * c) = z;
    __threadfence();  // the zeros are in memory before any atomic of this launch
    __syncthreads();
  }
  const int64_t *ids = a.ids + (int64_t)s * a.ids_stride;
  for (int i = lo + tid; i < hi; i += PEN_NT) {
    const int64_t v = ids[i];
    if (v < 0 || v >= a.V) continue;  // not counted, never indexed
    if (a.as_prompt)
      atomicOr(reinterpret_cast<unsigned int *>(row + v), 0x80000000u);
    else
      atomicAdd(row + v, 1);
  }
}

struct PenArgs {
  const bf16_t *logits;
  bf16_t *out;
  int64_t ld, tile_stride;
  int V, row0, nrows;
  const int32_t *dyn;
  int nrows_word, tiles_per_req;
  const int32_t *table;
  int64_t table_stride;
  const int64_t *block_ids;
  int64_t block_stride;
  const float *r_dev, *a_dev, *f_dev;
  float r, a, f;
  int64_t *out_ids;
  int64_t out_stride;
  int out_off;
};

__device__ __forceinline__ float pen_f(uint32_t b) { return __builtin_bit_cast(float, b << 16); }

// The contract's four steps, each rounded once.  seen: the token occurs in prompt or output; c: occurrences in the output.
// A NaN passes through with its own bits (finite parameters make no NaN out of a number).
__device__ __forceinline__ uint32_t pen_value(uint32_t xb, bool seen, uint32_t c, float r, float a, float f) {
#pragma clang fp contract(off)
  const float x = pen_f(xb);
  if (x != x) return xb;
  float y = x;
  if (seen) y = x > 0.f ? x / r : x * r;
  if (c > 0) y = y - a;
  y = __builtin_fmaf(-f, (float)c, y);
  uint32_t u = __builtin_bit_cast(uint32_t, y);
  u += 0x7fffu + ((u >> 16) & 1u);  // round to nearest even; an overflow rounds to inf
  return u >> 16;
}

__global__ __launch_bounds__(PEN_NT) void k_penalty_rows(PenArgs a) {
  __shared__ uint32_t flags[PEN_FLAG_WORDS];
  __shared__ int sblk[32], stok[32];
  __shared__ uint32_t sz[32];
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
  float r = a.r_dev ? a.r_dev[q] : a.r, pa = a.a_dev ? a.a_dev[q] : a.a, pf = a.f_dev ? a.f_dev[q] : a.f;
  if (!(r > 0.f && r < INFINITY)) r = 1.f;  // device values are not validated: every bit pattern is defined
  if (!(fabsf(pa) < INFINITY)) pa = 0.f;
  if (!(fabsf(pf) < INFINITY)) pf = 0.f;
  // an untouched column is fmaf(-f, 0, x): x itself, except that -0 becomes +0 where -f * 0 is +0
  const bool flip_zero = (__builtin_bit_cast(uint32_t, pf) >> 31) != 0u;

  const bf16_t *row = a.logits + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  bf16_t *dst = a.out + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  const int32_t *tab = a.table + (int64_t)q * a.table_stride;
  const int n = a.block_ids ? 16 * j + m : 0;  // in-block tokens block[1 .. n], n <= 31

  if (n > 0) {  // block-uniform
    for (int w = tid; w < (nchunks + 31) >> 5; w += PEN_NT) flags[w] = 0u;
    if (tid < n) {
      const int64_t v = a.block_ids[(int64_t)q * a.block_stride + 1 + tid];
      sblk[tid] = (v >= 0 && v < V) ? (int)v : -1;
    }
    __syncthreads();
    if (tid < n) {
      const int tok = sblk[tid];
      bool first = tok >= 0;
      uint32_t cnt = 0;
      for (int k = 0; k < n; ++k) {
        const bool same = sblk[k] == tok;
        cnt += same ? 1u : 0u;
        first = first && !(same && k < tid);
      }
      stok[tid] = first ? tok : -1;
      if (first) {
        const uint32_t w = (uint32_t)tab[tok];
        const uint32_t xb = (uint32_t)__builtin_bit_cast(unsigned short, row[tok]);  // read before any store to a row that aliases
        sz[tid] = pen_value(xb, true, (w & 0x7fffffffu) + cnt, r, pa, pf);
        atomicOr(&flags[tok >> 8], 1u << ((tok >> 3) & 31));
      }
    }
    __syncthreads();
  }

  float best = -INFINITY;
  int bi = PEN_NONE;
  for (int c = tid; c < nchunks; c += PEN_NT) {
    const u32x4 x = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
    const u32x4 w0 = *reinterpret_cast<const u32x4 *>(tab + (int64_t)c * 8);
    const u32x4 w1 = *reinterpret_cast<const u32x4 *>(tab + (int64_t)c * 8 + 4);
    const bool flagged = n > 0 && ((flags[c >> 5] >> (c & 31)) & 1u);
    uint32_t zb[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t xb = (x[e >> 1] >> (16 * (e & 1))) & 0xffffu;
      const uint32_t w = e < 4 ? w0[e & 3] : w1[e & 3];
      if (w == 0u)
        zb[e] = (xb == 0x8000u && flip_zero) ? 0u : xb;
      else
        zb[e] = pen_value(xb, true, w & 0x7fffffffu, r, pa, pf);
    }
    if (flagged) {  // a chunk with an in-block token (at most 31 per row): the held values replace the table's
      for (int k = 0; k < n; ++k) {
        const int tk = stok[k];
        if ((tk >> 3) == c) {  // (-1 >> 3 is no chunk)
          const uint32_t v = sz[k];
#pragma unroll
          for (int e = 0; e < 8; ++e) zb[e] = (e == (tk & 7)) ? v : zb[e];
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
      const float z = pen_f(zb[e]);
      if (z > best || (bi == PEN_NONE && z == z)) {  // columns ascend within a thread; a NaN is never the maximum
        best = z;
        bi = c * 8 + e;
      }
    }
    *reinterpret_cast<u32x4 *>(dst + (int64_t)c * 8) = o;
  }
  if (!a.out_ids) return;  // block-uniform
  auto take = [&](float ov, int oi) {
    if (oi != PEN_NONE && (bi == PEN_NONE || ov > best || (ov == best && oi < bi))) {
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
    a.out_ids[(int64_t)t * a.out_stride + a.out_off + blockIdx.x] = (int64_t)(bi == PEN_NONE ? 0 : bi);
  }
}

inline bool finite_f(float x) { return x - x == 0.f; }

}  // namespace

extern "C" int dfl_penalty_count(int32_t *table, int64_t table_stride, int V, int slots, const int64_t *ids,
                                 int64_t ids_stride, int ids_len, const int32_t *dyn, int lo_word, int hi_word, int lo,
                                 int hi, int as_prompt, int clear, void *stream) {
  DFL_REQUIRE(table && ids, "dfl_penalty_count: null pointer");
  DFL_REQUIRE(V >= 1 && V % 8 == 0 && V <= PEN_VMAX, "dfl_penalty_count: V=%d is not a multiple of 8 in 8..%d", V, PEN_VMAX);
  DFL_REQUIRE(slots >= 0 && table_stride >= V && table_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0,
              "dfl_penalty_count: slots=%d table_stride=%lld (>= V, a multiple of 4, rows on 16 bytes)", slots,
              (long long)table_stride);
  DFL_REQUIRE(ids_len >= 0 && ids_stride >= 0 && (slots <= 1 || ids_stride >= ids_len),
              "dfl_penalty_count: ids_len=%d / ids_stride=%lld", ids_len, (long long)ids_stride);
  DFL_REQUIRE(!dyn || (lo_word >= 0 && lo_word < DFL_DYN_WORDS && hi_word >= 0 && hi_word < DFL_DYN_WORDS),
              "dfl_penalty_count: lo_word=%d / hi_word=%d outside the record", lo_word, hi_word);
  if (slots == 0) return DFL_OK;
  PenCountArgs a{table, table_stride, V, ids, ids_stride, ids_len, dyn, lo_word, hi_word, lo, hi, as_prompt, clear};
  hipLaunchKernelGGL(k_penalty_count, dim3(slots), dim3(PEN_NT), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH("dfl_penalty_count");
  return DFL_OK;
}

extern "C" int dfl_penalty_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V, int row0,
                                int nrows, const int32_t *dyn, int nrows_dyn_word, int tiles_per_req, const int32_t *table,
                                int64_t table_stride, const int64_t *block_ids, int64_t block_stride, const float *r_dev,
                                float r, const float *a_dev, float a, const float *f_dev, float f, int64_t *out_ids,
                                int64_t out_stride, int out_off, void *stream) {
  DFL_REQUIRE(logits && out && table, "dfl_penalty_rows: null pointer");
  DFL_REQUIRE(V >= 1 && V % 8 == 0 && V <= PEN_VMAX, "dfl_penalty_rows: V=%d is not a multiple of 8 in 8..%d", V, PEN_VMAX);
  DFL_REQUIRE(r_dev || (finite_f(r) && r > 0.f), "dfl_penalty_rows: repetition penalty %g is not a finite value > 0", (double)r);
  DFL_REQUIRE(a_dev || finite_f(a), "dfl_penalty_rows: presence penalty %g is not finite", (double)a);
  DFL_REQUIRE(f_dev || finite_f(f), "dfl_penalty_rows: frequency penalty %g is not finite", (double)f);
  DFL_REQUIRE(tiles_per_req == 1 || tiles_per_req == 2, "dfl_penalty_rows: tiles_per_req=%d", tiles_per_req);
  DFL_REQUIRE(tiles >= 0 && ld >= V && ld % 8 == 0 && (tiles <= 1 || (tile_stride >= 16 * ld && tile_stride % 8 == 0)) &&
                  ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
              "dfl_penalty_rows: bad shape tiles=%d ld=%lld tile_stride=%lld (rows on 16 bytes)", tiles, (long long)ld,
              (long long)tile_stride);
  DFL_REQUIRE(table_stride >= V && table_stride % 4 == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0,
              "dfl_penalty_rows: table_stride=%lld (>= V, a multiple of 4, rows on 16 bytes)", (long long)table_stride);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "dfl_penalty_rows: rows [%d,%d) outside the tile", row0,
              row0 + nrows);
  DFL_REQUIRE(nrows_dyn_word < DFL_DYN_WORDS && (nrows_dyn_word < 0 || dyn),
              "dfl_penalty_rows: nrows_dyn_word=%d needs a record inside dyn", nrows_dyn_word);
  DFL_REQUIRE(block_stride >= 0 && out_stride >= 0 && out_off >= 0, "dfl_penalty_rows: negative stride or offset");
  if (tiles == 0 || (nrows == 0 && nrows_dyn_word < 0)) return DFL_OK;
  PenArgs p{(const bf16_t *)logits, (bf16_t *)out, ld,    tile_stride, V,     row0,  nrows, dyn, nrows_dyn_word, tiles_per_req,
            table,                  table_stride,  block_ids, block_stride, r_dev, a_dev, f_dev, r,   a,              f,
            out_ids,                out_stride,    out_off};
  hipLaunchKernelGGL(k_penalty_rows, dim3(nrows_dyn_word >= 0 ? 16 - row0 : nrows, tiles), dim3(PEN_NT), 0,
                     (hipStream_t)stream, p);
  DFL_CHECK_LAUNCH("dfl_penalty_rows");
  return DFL_OK;
}
