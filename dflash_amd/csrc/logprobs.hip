// Per-token log-probabilities of committed tokens.  One 1024-thread block per row of materialised
// bf16 logits, the layout and row / tile conventions of nucleus.hip.  The row is read from memory ONCE, as monotone 16-bit
// keys packed two to a register (19 x 16 bytes per thread at V = 151936); every later pass runs from registers:
//   1. the chosen id's value, out of the registers of the thread that holds its column, and the maximum over FINITE
//      values (integer reduction over the keys)
//   2. sum of exp(x - max) in fp32, in ONE fixed order: per thread sequentially in column order, the xor butterfly within
//      the wave, the 16 wave sums through LDS added in wave order by every thread.  No float atomics: the same logits
//      give the same bits on every run, eager or replayed
//   3. n_top rounds of a block argmax by (value descending, column ascending).  A thread keeps the best of its own
//      columns; a round takes the block's best, and only the thread that owned it scans its registers again.
// The numbers are of the RAW distribution: log_softmax of the logits the head produced, at T = 1 and unfiltered,
// whatever temperature and filter chose the token.
#include "dfl_common.h"

namespace {

typedef unsigned long long u64;

constexpr int LP_NT = 1024;                // threads per row
constexpr int LP_NCH = 19;                 // 16-byte chunks per thread: V <= 19 * 1024 * 8
constexpr int LP_VMAX = LP_NCH * LP_NT * 8;
constexpr int LP_TOPMAX = 8;
constexpr uint32_t LP_FIN_LO = 0x0080u, LP_FIN_HI = 0xff7fu;   // keys of the finite values: above -inf, below +inf

struct LpArgs {
  const bf16_t *logits;
  int64_t ld, tile_stride;
  int V, row0, nrows;
  const int32_t *dyn;
  int nrows_word, pos_word, pos_base, pos_add, tiles_per_req;
  const int64_t *ids;
  int64_t ids_stride;
  int ids_off, n_top;
  float *lp_out;
  int64_t *top_ids_out;
  float *top_lp_out;
  int64_t lp_stride;
  int lp_len;
};

// bf16 bits -> key with the order of the VALUES (-0 counts as +0, so equal values have equal keys); NaNs sort above +inf
// (sign clear) or below -inf (sign set): every bit pattern has a place in the order.  Key 0 (the last of the NaNs with
// the sign set) is folded onto key 1, its neighbour among them: 0 is "no column here".
__device__ __forceinline__ uint32_t lp_key(uint32_t b) {
  if (b == 0x8000u) b = 0u;
  return (b & 0x8000u) ? max(~b & 0xffffu, 1u) : (b | 0x8000u);
}
__device__ __forceinline__ float lp_val(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __builtin_bit_cast(float, b << 16);
}
__device__ __forceinline__ uint32_t lp_keys2(uint32_t w) { return lp_key(w & 0xffffu) | (lp_key(w >> 16) << 16); }
// Between two passes over the row's registers: the values pass through an empty asm, so that the compiler starts the next
// pass from the registers alone instead of carrying the previous pass's 152 per-column predicates across (it did: 260
// scalar and 70 vector registers spilled)
#define LP_FENCE(r)                                                      \
  do {                                                                   \
    _Pragma("unroll") for (int n_ = 0; n_ < LP_NCH * 4; ++n_) asm volatile("" : "+v"((r)[n_])); \
  } while (0)

__global__ __launch_bounds__(LP_NT) void k_logprob_rows(LpArgs a) {
  __shared__ uint32_t smax[16];
  __shared__ float ssum[16];
  __shared__ u64 sbest[2][16];
  __shared__ uint32_t sid;   // key of the chosen id's value; 0: no such column

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.y;
  int rows = a.nrows;
  if (a.dyn && a.nrows_word >= 0) rows = a.dyn[t * DFL_DYN_WORDS + a.nrows_word] - a.row0;
  if ((int)blockIdx.x >= rows) return;  // block-uniform: rows past the tile's valid count are not written
  const int m = a.row0 + blockIdx.x;
  const int q = t / a.tiles_per_req, j = t - q * a.tiles_per_req;
  const int base = (a.dyn && a.pos_word >= 0) ? a.dyn[t * DFL_DYN_WORDS + a.pos_word] : a.pos_base;
  const int64_t pos = (int64_t)base + a.pos_add + 16 * j + m;
  if (pos < 0 || pos >= a.lp_len) return;  // block-uniform: a position outside the buffer writes nothing
  const int V = a.V, n_top = a.n_top;
  const int64_t id = a.ids[(int64_t)t * a.ids_stride + a.ids_off + blockIdx.x];
  const bool id_ok = id >= 0 && id < V;

  // ---- the row, once: keys packed two to a register; slots past V hold key 0 and are skipped by index ----
  const bf16_t *row = a.logits + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  const int nchunks = (V + 7) >> 3;
  const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  uint32_t r[LP_NCH * 4];
  // Every load is unconditional, at an index clamped into the row, and what lies past V is masked to key 0 afterwards:
  // no per-chunk branches for the compiler to keep 19 sets of lane masks alive over.
  if (aligned) {  // block-uniform: whole chunks as 16-byte requests, lane-linear; the row's last few columns by one thread
    const int nfull = V >> 3;
#pragma unroll
    for (int i = 0; i < LP_NCH; ++i) {
      const int c = i * LP_NT + tid;
      u32x4 x = {0u, 0u, 0u, 0u};
      if (i * LP_NT < nfull) x = *reinterpret_cast<const u32x4 *>(row + (int64_t)min(c, nfull - 1) * 8);
      const bool in = c < nfull;
      r[4 * i + 0] = in ? lp_keys2(x[0]) : 0u;
      r[4 * i + 1] = in ? lp_keys2(x[1]) : 0u;
      r[4 * i + 2] = in ? lp_keys2(x[2]) : 0u;
      r[4 * i + 3] = in ? lp_keys2(x[3]) : 0u;
    }
    if (V & 7) {  // block-uniform
      uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int e = 0; e < 7; ++e) {
        const int v = nfull * 8 + e;
        const uint32_t b = (uint32_t)__builtin_bit_cast(unsigned short, row[min(v, V - 1)]);
        w[e >> 1] |= (v < V ? lp_key(b) : 0u) << (16 * (e & 1));
      }
      const bool mine = tid == (nfull & (LP_NT - 1));
#pragma unroll
      for (int i = 0; i < LP_NCH; ++i)
        if (i == (nfull >> 10) && mine) {
          r[4 * i + 0] = w[0];
          r[4 * i + 1] = w[1];
          r[4 * i + 2] = w[2];
          r[4 * i + 3] = w[3];
        }
    }
  } else {  // a row that does not start on 16 bytes: column by column
#pragma unroll
    for (int i = 0; i < LP_NCH; ++i) {
      const int v0 = (i * LP_NT + tid) * 8;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (i * LP_NT < nchunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t b = (uint32_t)__builtin_bit_cast(unsigned short, row[min(v0 + e, V - 1)]);
          w[e >> 1] |= (v0 + e < V ? lp_key(b) : 0u) << (16 * (e & 1));
        }
      }
      r[4 * i + 0] = w[0];
      r[4 * i + 1] = w[1];
      r[4 * i + 2] = w[2];
      r[4 * i + 3] = w[3];
    }
  }
  // key of slot (i, e) of this thread; the passes below skip whole chunk rounds past the row (block-uniform)
  auto key = [&](int i, int e) { return (r[4 * i + (e >> 1)] >> (16 * (e & 1))) & 0xffffu; };

  // the chosen id's value, out of the registers of the thread that holds its chunk
  if (tid == 0) sid = 0u;
  __syncthreads();
  if (id_ok) {  // block-uniform
    const int idc = (int)(id >> 3), ide = (int)(id & 7), idi = idc >> 10;
    uint32_t ww = 0u;
#pragma unroll
    for (int i = 0; i < LP_NCH; ++i)
      if (i == idi) ww = (ide & 4) ? ((ide & 2) ? r[4 * i + 3] : r[4 * i + 2]) : ((ide & 2) ? r[4 * i + 1] : r[4 * i + 0]);
    if (tid == (idc & (LP_NT - 1))) sid = (ww >> (16 * (ide & 1))) & 0xffffu;
  }

  // ---- 1. the maximum over finite values (a slot past V holds key 0, which is no finite value's key) ----
  uint32_t kmax = 0u;  // 0: no finite value
#pragma unroll
  for (int i = 0; i < LP_NCH; ++i)
    if (i * LP_NT < nchunks) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t k = key(i, e);
        kmax = max(kmax, k <= LP_FIN_HI ? k : 0u);
      }
    }
  if (kmax < LP_FIN_LO) kmax = 0u;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
  if (lane == 0) smax[wave] = kmax;
  __syncthreads();
#pragma unroll
  for (int w = 0; w < 16; ++w) kmax = max(kmax, smax[w]);
  const float xmax = kmax ? lp_val(kmax) : 0.f;  // no finite value: the sum is 0 and lse = -inf

  // ---- 2. the sum, in one fixed order ----
  LP_FENCE(r);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LP_NCH; ++i)
    if (i * LP_NT < nchunks) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t k = key(i, e);
        const float ex = expf(lp_val(k) - xmax);
        s += (k >= LP_FIN_LO && k <= LP_FIN_HI) ? ex : 0.f;
      }
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) ssum[wave] = s;
  __syncthreads();
  float tot = ssum[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) tot += ssum[w];
  const float lse = xmax + logf(tot);

  const int64_t o = (int64_t)q * a.lp_stride + pos;
  if (tid == 0) {
    const uint32_t kid = sid;  // (written before the barriers above)
    a.lp_out[o] = kid ? lp_val(kid) - lse : __builtin_nanf("");
  }

  // ---- 3. the top n_top columns, one block argmax per round ----
  // best of this thread's columns below `prev`: key << 8 | 255 - (8 i + e), so that the largest is the highest value at
  // the lowest column; 0: none (a slot past V holds key 0)
  auto scan = [&](uint32_t prev) {
    LP_FENCE(r);
    uint32_t nb = 0u;
#pragma unroll
    for (int i = 0; i < LP_NCH; ++i)
      if (i * LP_NT < nchunks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t cand = (key(i, e) << 8) | (uint32_t)(255 - (8 * i + e));
          nb = max(nb, cand < prev ? cand : 0u);
        }
      }
    return nb < 256u ? 0u : nb;
  };
  uint32_t best = n_top > 0 ? scan(0xffffffffu) : 0u;
  for (int n = 0; n < n_top; ++n) {  // block-uniform
    // key << 32 | ~column: the largest is the highest value at the lowest column
    u64 g = 0;
    if (best) {
      const uint32_t li = 255u - (best & 255u);
      const uint32_t col = (((li >> 3) * LP_NT + (uint32_t)tid) << 3) | (li & 7u);
      g = ((u64)(best >> 8) << 32) | (u64)(0xffffffffu - col);
    }
    u64 w = g;
#pragma unroll
    for (int ofs = 32; ofs > 0; ofs >>= 1) {
      const u64 v = (u64)__shfl_xor((long long)w, ofs, 64);
      w = v > w ? v : w;
    }
    if (lane == 0) sbest[n & 1][wave] = w;
    __syncthreads();  // (the other buffer is rewritten only after the next round's barrier: one barrier per round)
    w = sbest[n & 1][0];
#pragma unroll
    for (int x = 1; x < 16; ++x) {
      const u64 v = sbest[n & 1][x];
      w = v > w ? v : w;
    }
    if (tid == 0) {
      const int64_t oo = o * n_top + n;
      if (w) {
        a.top_ids_out[oo] = (int64_t)(0xffffffffu - (uint32_t)w);
        a.top_lp_out[oo] = lp_val((uint32_t)(w >> 32)) - lse;
      } else {  // fewer than n_top columns
        a.top_ids_out[oo] = -1;
        a.top_lp_out[oo] = __builtin_nanf("");
      }
    }
    if (g == w && g != 0 && n + 1 < n_top) {  // the owner: its best column is taken; the best of those after it
      best = scan(best);
    }
  }
}

}  // namespace

extern "C" int dfl_logprob_rows(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int row0, int nrows,
                                const int32_t *dyn, int nrows_dyn_word, int pos_word, int pos_base, int pos_add,
                                int tiles_per_req, const int64_t *ids, int64_t ids_stride, int ids_off, int n_top,
                                float *lp_out, int64_t *top_ids_out, float *top_lp_out, int64_t lp_stride, int lp_len,
                                void *stream) {
  DFL_REQUIRE(logits && ids && lp_out, "dfl_logprob_rows: null pointer");
  DFL_REQUIRE(tiles >= 0 && V > 0 && V <= LP_VMAX && ld >= V && (tiles <= 1 || tile_stride >= 16 * ld),
              "dfl_logprob_rows: bad shape tiles=%d V=%d (at most %d) ld=%lld tile_stride=%lld", tiles, V, LP_VMAX,
              (long long)ld, (long long)tile_stride);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "dfl_logprob_rows: rows [%d,%d) outside the tile", row0,
              row0 + nrows);
  DFL_REQUIRE(nrows_dyn_word < DFL_DYN_WORDS && pos_word < DFL_DYN_WORDS && ((nrows_dyn_word < 0 && pos_word < 0) || dyn),
              "dfl_logprob_rows: nrows_dyn_word=%d / pos_word=%d need a record inside dyn", nrows_dyn_word, pos_word);
  DFL_REQUIRE(tiles_per_req == 1 || tiles_per_req == 2, "dfl_logprob_rows: tiles_per_req=%d", tiles_per_req);
  DFL_REQUIRE(n_top >= 0 && n_top <= LP_TOPMAX, "dfl_logprob_rows: n_top=%d outside 0..%d", n_top, LP_TOPMAX);
  DFL_REQUIRE(n_top == 0 || (top_ids_out && top_lp_out), "dfl_logprob_rows: n_top=%d needs top_ids_out and top_lp_out", n_top);
  DFL_REQUIRE(ids_stride >= 0 && ids_off >= 0, "dfl_logprob_rows: ids_stride=%lld / ids_off=%d is negative",
              (long long)ids_stride, ids_off);
  DFL_REQUIRE(lp_len >= 0 && lp_stride >= lp_len, "dfl_logprob_rows: lp_len=%d / lp_stride=%lld (a slot's row holds lp_len)",
              lp_len, (long long)lp_stride);
  if (tiles == 0 || lp_len == 0 || (nrows == 0 && nrows_dyn_word < 0)) return DFL_OK;
  LpArgs a{(const bf16_t *)logits, ld, tile_stride, V, row0, nrows, dyn, nrows_dyn_word, pos_word, pos_base, pos_add,
           tiles_per_req, ids, ids_stride, ids_off, n_top, lp_out, top_ids_out, top_lp_out, lp_stride, lp_len};
  hipLaunchKernelGGL(k_logprob_rows, dim3(nrows_dyn_word >= 0 ? 16 - row0 : nrows, tiles), dim3(LP_NT), 0,
                     (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH("dfl_logprob_rows");
  return DFL_OK;
}
