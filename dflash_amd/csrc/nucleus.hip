// Top-k / top-p (nucleus) filtering on the seeded draw ("Filtered draw").  One 1024-thread block per
// row of materialised bf16 logits.  The row is read from memory ONCE, as monotone 16-bit keys packed two to a register
// (19 x 16 bytes per thread at V = 151936); every later pass runs from registers:
//   1. row maximum / minimum (integer reduction over the keys)
//   2. top-k threshold: radix selection on the key, 11 bits then 5, integer counts in LDS histograms
//   3. top-p threshold: the same selection over the masses exp(invT (x - max)) of what top-k kept, accumulated as
//      2^-40 fixed-point INTEGER adds, so the sums do not depend on the order the atomics arrive in
//   4. the draw of dfl_rng.h over {key >= threshold}: Philox / log / log only for column groups with a kept column
// With both filters off steps 2 and 3 are skipped and the kernel is the plain draw of k_sample_rows (same ids).
#include "dfl_common.h"
#include "dfl_rng.h"

namespace {

typedef unsigned long long u64;

constexpr int NUC_NT = 1024;                 // threads per row
constexpr int NUC_NCH = 19;                  // 16-byte chunks per thread: V <= 19 * 1024 * 8
constexpr int NUC_VMAX = NUC_NCH * NUC_NT * 8;
constexpr int NUC_L1 = 2048, NUC_L2 = 32;    // bins of the two radix levels (key >> 5, key & 31)
constexpr int NUC_COPIES = 2;                // histogram copies (wave parity), to spread same-address atomics
constexpr float NUC_FIX = 0x1p40f;           // mass 1.0 in fixed point: <= 151936 * 2^40 < 2^58 per sum

struct NucArgs {
  const bf16_t *logits;
  int64_t ld, tile_stride;
  int V, row0, nrows;
  const int32_t *dyn;
  int nrows_word, pos_word, pos_base;
  const int32_t *positions;
  int pos_add, tiles_per_req;
  const int64_t *seeds;
  uint64_t seed;
  const int32_t *top_k_dev;
  int top_k;
  const float *top_p_dev;
  float top_p, inv_t;
  int rng_stream, extra;
  int64_t *out_ids;
  int64_t out_stride;
  int out_off;
  float *thr_out;
  int32_t *kept_out;
  const float *inv_t_dev;  // invT per request slot (NULL: inv_t); a slot whose value is not > 0 is greedy: its rows return
};

struct NucSel {
  int bin;
  u64 above;      // sum of everything above `bin` (the caller's base included)
  double target;  // what the cumulative sum had to reach
};

// bf16 bits -> key with the order of the VALUES (-0 counts as +0, so equal values have equal keys)
__device__ __forceinline__ uint32_t nuc_key(uint32_t b) {
  if (b == 0x8000u) b = 0u;
  return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
__device__ __forceinline__ float nuc_val(uint32_t k) {
  const uint32_t b = (k & 0x8000u) ? (k & 0x7fffu) : (~k & 0xffffu);
  return __builtin_bit_cast(float, b << 16);
}
__device__ __forceinline__ uint32_t nuc_keys2(uint32_t w) { return nuc_key(w & 0xffffu) | (nuc_key(w >> 16) << 16); }

// Selection over hist[copies][nbins], bins counted from the TOP: the first bin at which base + (sum of the bins above
// it and itself) >= target, target = t_abs + t_frac * (sum of all bins).  Integer sums compared as doubles (exact for
// counts; for masses the same integers give the same answer on every run).  Every thread calls it; `sel` is valid
// after it returns.  A target nothing reaches (NaN rows only) selects bin 0.
__device__ void nuc_select(u64 *hist, int nbins, u64 base, double t_abs, double t_frac, NucSel *sel) {
  const int tid = threadIdx.x;
  for (int b = tid; b < nbins; b += NUC_NT) {
    u64 s = hist[b];
#pragma unroll
    for (int c = 1; c < NUC_COPIES; ++c) s += hist[c * nbins + b];
    hist[b] = s;
  }
  __syncthreads();
  if (tid < 64) {
    const int per = (nbins + 63) / 64;
    u64 s = 0;
    for (int k = 0; k < per; ++k) {
      const int d = tid * per + k;
      if (d < nbins) s += hist[nbins - 1 - d];
    }
    u64 inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const u64 v = __shfl_up(inc, o, 64);
      if (tid >= o) inc += v;
    }
    const u64 total = __shfl(inc, 63, 64);
    const double target = t_abs + t_frac * (double)total;
    const u64 mask = __ballot((double)(base + inc) >= target);
    if (mask == 0) {
      if (tid == 0) {
        sel->bin = 0;
        sel->above = base + total - hist[0];
        sel->target = target;
      }
    } else if (tid == __ffsll((long long)mask) - 1) {
      u64 cum = base + inc - s;
      int d = tid * per;
      for (int k = 0; k < per - 1 && d + 1 < nbins; ++k, ++d) {
        const u64 h = hist[nbins - 1 - d];
        if ((double)(cum + h) >= target) break;
        cum += h;
      }
      sel->bin = nbins - 1 - d;
      sel->above = cum;
      sel->target = target;
    }
  }
  __syncthreads();
}

__global__ __launch_bounds__(NUC_NT) void k_sample_rows_nucleus(NucArgs a) {
  __shared__ u64 hist[NUC_COPIES * NUC_L1];
  __shared__ uint32_t smax[16], smin[16];
  __shared__ float sv[16];
  __shared__ int si[16], sc[16];
  __shared__ NucSel sel;
  __shared__ int nlist;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.y;
  int rows = a.nrows;
  if (a.dyn && a.nrows_word >= 0) rows = a.dyn[t * DFL_DYN_WORDS + a.nrows_word] - a.row0;
  if ((int)blockIdx.x >= rows) return;  // block-uniform: rows past the tile's valid count are not written
  const int m = a.row0 + blockIdx.x;
  const int q = t / a.tiles_per_req, j = t - q * a.tiles_per_req;
  const float inv_t = a.inv_t_dev ? a.inv_t_dev[q] : a.inv_t;
  if (!(inv_t > 0.f)) return;  // block-uniform: a greedy slot keeps what the argmax launch in front wrote, diagnostics too
  const int V = a.V;

  uint32_t pos, extra = (uint32_t)a.extra;
  if (a.positions) {
    pos = (uint32_t)a.positions[t * 16 + m];
  } else if (a.dyn && a.pos_word >= 0) {
    const int base = a.dyn[t * DFL_DYN_WORDS + a.pos_word];
    pos = (uint32_t)(base + a.pos_add + 16 * j + m);
    if (a.rng_stream == (int)DFL_RNG_DRAFT) extra = (uint32_t)base;
  } else {
    pos = (uint32_t)(a.pos_base + a.pos_add + 16 * j + m);
  }
  const uint64_t seed = a.seeds ? (uint64_t)a.seeds[q] : a.seed;
  int K = a.top_k_dev ? a.top_k_dev[q] : a.top_k;
  float P = a.top_p_dev ? a.top_p_dev[q] : a.top_p;
  const bool k_on = K > 0 && K < V;
  const bool p_on = P > 0.f && P < 1.f;  // anything else a device array may hold (NaN included) reads as "off"

  const bf16_t *row = a.logits + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  uint32_t T = 0u;  // the threshold key: kept = {key >= T}
  int total = V;    // size of the kept set
  bool listed = false;

  if (k_on || p_on) {
    // ---- the row, once: keys packed two to a register; slots past V hold key 0 and are skipped by index ----
    const int nchunks = (V + 7) >> 3;
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    uint32_t r[NUC_NCH * 4];
    uint32_t kmax = 0u, kmin = 0xffffu;
#pragma unroll
    for (int i = 0; i < NUC_NCH; ++i) {
      const int c = i * NUC_NT + tid;
      uint32_t w[4] = {0u, 0u, 0u, 0u};
      if (c < nchunks) {
        const int nv = V - c * 8;
        if (aligned && nv >= 8) {
          const u32x4 x = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
          w[0] = nuc_keys2(x[0]);
          w[1] = nuc_keys2(x[1]);
          w[2] = nuc_keys2(x[2]);
          w[3] = nuc_keys2(x[3]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e < nv)
              w[e >> 1] |= nuc_key((uint32_t)__builtin_bit_cast(unsigned short, row[(int64_t)c * 8 + e])) << (16 * (e & 1));
        }
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < nv) {
            const uint32_t k = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
            kmax = max(kmax, k);
            kmin = min(kmin, k);
          }
      }
      r[4 * i + 0] = w[0];
      r[4 * i + 1] = w[1];
      r[4 * i + 2] = w[2];
      r[4 * i + 3] = w[3];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, o, 64));
      kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o, 64));
    }
    if (lane == 0) {
      smax[wave] = kmax;
      smin[wave] = kmin;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 16; ++w) {
      kmax = max(kmax, smax[w]);
      kmin = min(kmin, smin[w]);
    }
    const float xmax = nuc_val(kmax);

    // f(key, column) for every valid column this thread holds
    auto each = [&](auto &&f) {
#pragma unroll
      for (int i = 0; i < NUC_NCH; ++i) {
        const int c = i * NUC_NT + tid;
        if (c < nchunks) {
          const int nv = V - c * 8;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (e < nv) f((r[4 * i + (e >> 1)] >> (16 * (e & 1))) & 0xffffu, c * 8 + e);
        }
      }
    };
    auto clear = [&](int n) {
      for (int b = tid; b < n; b += NUC_NT) hist[b] = 0;
      __syncthreads();
    };
    u64 *const h1 = hist + (wave & (NUC_COPIES - 1)) * NUC_L1;
    u64 *const h2 = hist + (wave & (NUC_COPIES - 1)) * NUC_L2;

    T = kmin;
    if (k_on) {
      if (K == 1) {
        T = kmax;
      } else {
        clear(NUC_COPIES * NUC_L1);
        each([&](uint32_t k, int) { atomicAdd(&h1[k >> 5], (u64)1); });
        __syncthreads();
        nuc_select(hist, NUC_L1, 0, (double)K, 0.0, &sel);
        const uint32_t b1 = (uint32_t)sel.bin;
        const u64 above = sel.above;
        clear(NUC_COPIES * NUC_L2);
        each([&](uint32_t k, int) {
          if ((k >> 5) == b1) atomicAdd(&h2[k & 31u], (u64)1);
        });
        __syncthreads();
        nuc_select(hist, NUC_L2, above, (double)K, 0.0, &sel);
        T = (b1 << 5) | (uint32_t)sel.bin;
      }
    }
    if (p_on) {
      const uint32_t Tk = T;
      auto mass = [&](uint32_t k) { return (u64)__float2ull_rn(expf(inv_t * (nuc_val(k) - xmax)) * NUC_FIX); };
      clear(NUC_COPIES * NUC_L1);
      each([&](uint32_t k, int) {
        if (k >= Tk) atomicAdd(&h1[k >> 5], mass(k));
      });
      __syncthreads();
      nuc_select(hist, NUC_L1, 0, 0.0, (double)P, &sel);
      const uint32_t b1 = (uint32_t)sel.bin;
      const u64 above = sel.above;
      const double target = sel.target;
      clear(NUC_COPIES * NUC_L2);
      each([&](uint32_t k, int) {
        if (k >= Tk && (k >> 5) == b1) atomicAdd(&h2[k & 31u], mass(k));
      });
      __syncthreads();
      nuc_select(hist, NUC_L2, above, target, 0.0, &sel);
      T = max(Tk, (b1 << 5) | (uint32_t)sel.bin);
    }
    T = min(T, kmax);  // the argmax is always kept

    // size of the kept set; a small one is compacted into LDS (over the histograms), so that the draw runs over its
    // members alone.  The list's order is whatever the atomics give: the draw breaks ties by column, not by order.
    int cnt = 0;
    each([&](uint32_t k, int) { cnt += k >= T ? 1 : 0; });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if (lane == 0) sc[wave] = cnt;
    if (tid == 0) nlist = 0;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) total += sc[w];
    listed = total <= NUC_COPIES * NUC_L1;
    if (listed) {
      each([&](uint32_t k, int v) {
        if (k >= T) hist[atomicAdd(&nlist, 1)] = ((u64)(uint32_t)v << 16) | k;
      });
      __syncthreads();
    }
  }

  // ---- the draw over {key >= T} ----
  float best = -INFINITY;
  int bi = 0x7fffffff;
  uint32_t kmin = 0xffffu;
  auto take = [&](float x, int v) {
    if (bi == 0x7fffffff || x > best || (x == best && v < bi)) {
      best = x;
      bi = v;
    }
  };
  if (listed) {
    for (int e = tid; e < total; e += NUC_NT) {
      const u64 ent = hist[e];
      const int v = (int)(ent >> 16);
      uint32_t w[4];
      dfl_rng_words(seed, (uint32_t)a.rng_stream, pos, (uint32_t)v, extra, w);
      take(dfl_perturb_w(nuc_val((uint32_t)ent & 0xffffu), inv_t, w[v & 3]), v);
    }
    kmin = T;
  } else {  // the whole row, or most of it: k_sample_rows' loop, one Philox call per 4 columns with a kept one
    const bool al8 = (reinterpret_cast<uintptr_t>(row) & 7) == 0;
    for (int c = tid; 4 * c < V; c += NUC_NT) {
      const int nv = V - 4 * c;
      uint32_t k[4] = {0u, 0u, 0u, 0u};
      if (al8 && nv >= 4) {
        const uint2 x = *reinterpret_cast<const uint2 *>(row + 4 * c);
        k[0] = nuc_key(x.x & 0xffffu);
        k[1] = nuc_key(x.x >> 16);
        k[2] = nuc_key(x.y & 0xffffu);
        k[3] = nuc_key(x.y >> 16);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < nv) k[e] = nuc_key((uint32_t)__builtin_bit_cast(unsigned short, row[4 * c + e]));
      }
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < nv) kmin = min(kmin, k[e]);
        any = any || (e < nv && k[e] >= T);
      }
      if (any) {
        uint32_t w[4];
        dfl_rng_words(seed, (uint32_t)a.rng_stream, pos, (uint32_t)(4 * c), extra, w);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (e < nv && k[e] >= T) take(dfl_perturb_w(nuc_val(k[e]), inv_t, w[e]), 4 * c + e);
      }
    }
    if (k_on || p_on) kmin = T;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, o, 64));
    if (oi != 0x7fffffff) take(ov, oi);
  }
  if (lane == 0) {
    sv[wave] = best;
    si[wave] = bi;
    smin[wave] = kmin;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < 16; ++w) {
      kmin = min(kmin, smin[w]);
      if (si[w] != 0x7fffffff) take(sv[w], si[w]);
    }
    const int64_t o = (int64_t)t * a.out_stride + a.out_off + blockIdx.x;
    a.out_ids[o] = (int64_t)(bi == 0x7fffffff ? 0 : bi);
    if (a.thr_out) a.thr_out[o] = nuc_val(kmin);  // filters off: the row minimum
    if (a.kept_out) a.kept_out[o] = total;
  }
}

}  // namespace

extern "C" int dfl_sample_rows_nucleus(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int row0,
                                       int nrows, const int32_t *dyn, int nrows_dyn_word, int pos_word, int pos_base,
                                       const int32_t *positions, int pos_add, int tiles_per_req, const int64_t *seeds,
                                       uint64_t seed, const int32_t *top_k_dev, int top_k, const float *top_p_dev,
                                       float top_p, const float *inv_t_dev, float inv_t, int rng_stream, int extra,
                                       int64_t *out_ids, int64_t out_stride, int out_off, float *thr_out,
                                       int32_t *kept_out, void *stream) {
  DFL_REQUIRE(logits && out_ids, "dfl_sample_rows_nucleus: null pointer");
  DFL_REQUIRE(tiles >= 0 && V > 0 && V <= NUC_VMAX && ld >= V && (tiles <= 1 || tile_stride >= 16 * ld),
              "dfl_sample_rows_nucleus: bad shape tiles=%d V=%d (at most %d) ld=%lld tile_stride=%lld", tiles, V, NUC_VMAX,
              (long long)ld, (long long)tile_stride);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "dfl_sample_rows_nucleus: rows [%d,%d) outside the tile", row0,
              row0 + nrows);
  DFL_REQUIRE(nrows_dyn_word < DFL_DYN_WORDS && pos_word < DFL_DYN_WORDS && ((nrows_dyn_word < 0 && pos_word < 0) || dyn),
              "dfl_sample_rows_nucleus: nrows_dyn_word=%d / pos_word=%d need a record inside dyn", nrows_dyn_word, pos_word);
  DFL_REQUIRE(tiles_per_req == 1 || tiles_per_req == 2, "dfl_sample_rows_nucleus: tiles_per_req=%d", tiles_per_req);
  DFL_REQUIRE(top_k_dev || top_k >= 0, "dfl_sample_rows_nucleus: top_k=%d is negative", top_k);
  DFL_REQUIRE(top_p_dev || (top_p > 0.f && top_p <= 1.f), "dfl_sample_rows_nucleus: top_p=%g outside (0, 1]", (double)top_p);
  // (device values are not validated: !(invT > 0) is the greedy slot)
  DFL_REQUIRE(inv_t_dev || (inv_t > 0.f && inv_t <= 1e5f), "dfl_sample_rows_nucleus: inv_t=%g outside (0, 1e5]", (double)inv_t);
  DFL_REQUIRE(rng_stream == (int)DFL_RNG_TARGET || rng_stream == (int)DFL_RNG_DRAFT,
              "dfl_sample_rows_nucleus: unknown stream %d", rng_stream);
  if (tiles == 0 || (nrows == 0 && nrows_dyn_word < 0)) return DFL_OK;
  NucArgs a{(const bf16_t *)logits, ld,    tile_stride, V,         row0,  nrows, dyn,       nrows_dyn_word, pos_word,
            pos_base,               positions, pos_add, tiles_per_req, seeds, seed,  top_k_dev, top_k,          top_p_dev,
            top_p,                  inv_t, rng_stream,  extra,     out_ids, out_stride, out_off, thr_out,    kept_out,
            inv_t_dev};
  hipLaunchKernelGGL(k_sample_rows_nucleus, dim3(nrows_dyn_word >= 0 ? 16 - row0 : nrows, tiles), dim3(NUC_NT), 0,
                     (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH("dfl_sample_rows_nucleus");
  return DFL_OK;
}
