// Grammar-aware draft: each block token picked under the automaton ("The draft under the grammar").
//   The draft's head launch leaves bf16 logits [tiles][16][V] (row m predicts block slot m) and the plain argmax ids in
//   block[q][1 .. n-1].  k_grammar_draft_rows: one 1024-thread block per slot walks the rows IN ORDER —
//     s = state[q];  for m = 1 .. n-1:  c = lowest column among the maxima over the legal, non-NaN columns of row m,
//     legal(v) = table[(base + s) * table_stride + v] >= 0  and  bias[q][v] != -inf;   block[q][m] = c;   s = step(s, c)
//   and stops — leaving the ids of the rows behind as the head launch wrote them — at a violated state, a row without a
//   legal non-NaN column, or a successor outside the pool (that id is still written).  The pool, base and state are those
//   of grammar.hip; state[q] is only read: it moves in dfl_grammar_advance alone.  table == NULL: the ban-only form, the
//   rows independent of each other; bias == NULL: the grammar-only form.  A slot without a grammar (base < 0) and without
//   a bias row is left untouched.
//   Per row a dense pass with 16-byte loads of the logits, of the state's table row and of the bias row, several chunks per
//   thread in flight, a running argmax (columns ascend within a thread: the first maximum is the lowest), the wave
//   butterfly, 16 wave results through LDS (two buffers by row parity: one barrier per row), and every thread loads the
//   successor itself (one address for the whole block).  Only the table row depends on the previous pick: the next row's
//   first logits are requested before the reduction.
// No atomics, plain vector stores: the same inputs give the same bits, eager or replayed.
//   The NOISE form (dfl_grammar_draft_sample_rows; DESIGN.md section 20, the coupled draft under a grammar): the same
//   walk, stops and early exits, the comparison key fmaf(z, invT, g(seed[q], TARGET, base_q + m, v, 0)) of dfl_rng.h in
//   place of z — the noise the target's verify row m - 1 will draw position base_q + m with.  One Philox call per four
//   columns, and only for a column group with a legal column.  A slot whose invT is not > 0 compares z: the sibling's pick.
#include "dfl_common.h"
#include "dfl_rng.h"

namespace {

constexpr int GD_NT = 1024;      // threads per slot
constexpr int GD_VMAX = 155648;  // the row kernels' common limit (19 * 1024 * 8)
constexpr int GD_NONE = 0x7fffffff;

struct GrammarDraftArgs {
  const bf16_t *logits;
  int64_t ld, tile_stride;
  int V, nrows;
  const int32_t *dyn;
  int nrows_word;
  const int16_t *table;
  int64_t table_stride;
  int pool_states;
  const int32_t *base, *state;
  const float *bias;
  int64_t bias_stride;
  int64_t *block_ids;
  int64_t block_stride;
};

// what the NOISE form reads on top: per-slot seeds, invT (inv_ts[q], or inv_t where inv_ts is NULL) and the position of
// block slot 0 (dyn[q][pos_word] where pos_word >= 0, else pos_base)
struct GrammarDraftNoiseArgs : GrammarDraftArgs {
  const int64_t *seeds;
  const float *inv_ts;
  float inv_t;
  int pos_word, pos_base;
};
template <bool NOISE>
struct GdArgs {
  using type = GrammarDraftArgs;
};
template <>
struct GdArgs<true> {
  using type = GrammarDraftNoiseArgs;
};

__device__ __forceinline__ float gd_f(uint32_t b) { return __builtin_bit_cast(float, b << 16); }

template <int GD_PF>
__device__ __forceinline__ void gd_load_x(u32x4 (&x)[GD_PF], const bf16_t *row, int tid, int nchunks) {
#pragma unroll
  for (int u = 0; u < GD_PF; ++u) {
    const int c = tid + u * GD_NT;
    x[u] = u32x4{0u, 0u, 0u, 0u};
    if (c < nchunks) x[u] = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
  }
}

// BIAS: the launch has a bias table.  GD_PF: chunks per thread in flight — four (logits and table row: 8 requests), two
// with a bias row (its fp32 columns are two more 16-byte requests per chunk): under 128 VGPRs either way, no scratch.
// NOISE: the key is the perturbed logit (above); two chunks in flight in both forms (the Philox words and the two
// logarithms per column take the registers, and the VALU, not the loads, bounds a noisy row).
template <bool BIAS, int GD_PF, bool NOISE = false>
__global__ __launch_bounds__(GD_NT) void k_grammar_draft_rows(typename GdArgs<NOISE>::type a) {
  __shared__ float sv[2][16];
  __shared__ int si[2][16];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.x;  // one tile per slot
  int n = a.nrows;
  if (a.dyn && a.nrows_word >= 0) n = a.dyn[t * DFL_DYN_WORDS + a.nrows_word];
  n = min(n, 16);
  if (n < 2) return;  // block-uniform: an idle slot, or a block without a draft token
  const int V = a.V, nchunks = V >> 3;

  const int base = a.table ? a.base[t] : -1;
  const bool gram = base >= 0;  // block-uniform
  if (!gram && !BIAS) return;  // nothing to constrain by: the head launch's ids stay
  int st = 0;
  if (gram) {
    st = a.state[t];
    if (st < 0 || st >= a.pool_states - base) return;  // violated: every row of the verify is dead, the ids stay
  }
  const bf16_t *tile = a.logits + (int64_t)t * a.tile_stride;
  const float *brow = BIAS ? a.bias + (int64_t)t * a.bias_stride : nullptr;
  int64_t *blk = a.block_ids + (int64_t)t * a.block_stride;
  // NOISE: block-uniform — the slot's seed, invT and block start; `noisy` false (invT not > 0): the plain pick
  uint64_t seed = 0;
  float inv_t = 0.f;
  uint32_t pos0 = 0;
  bool noisy = false;
  if constexpr (NOISE) {
    inv_t = a.inv_ts ? a.inv_ts[t] : a.inv_t;
    noisy = inv_t > 0.f;
    seed = (uint64_t)a.seeds[t];
    pos0 = (uint32_t)(a.pos_word >= 0 ? a.dyn[t * DFL_DYN_WORDS + a.pos_word] : a.pos_base);
  }

  u32x4 xpre[GD_PF];  // the row's first chunks, requested while the previous row reduces
  gd_load_x(xpre, tile + a.ld, tid, nchunks);

  for (int m = 1; m < n; ++m) {
    const bf16_t *row = tile + (int64_t)m * a.ld;
    const int16_t *tab = gram ? a.table + (int64_t)(base + st) * a.table_stride : nullptr;
    float best = -INFINITY;
    int bi = GD_NONE;
    for (int c0 = tid; c0 < nchunks; c0 += GD_PF * GD_NT) {
      u32x4 x[GD_PF], w[GD_PF];
      f32x4 b[GD_PF][2];
#pragma unroll
      for (int u = 0; u < GD_PF; ++u) {
        const int c = c0 + u * GD_NT;
        const bool in = c < nchunks;
        x[u] = xpre[u];
        if (c0 != tid) {
          x[u] = u32x4{0u, 0u, 0u, 0u};
          if (in) x[u] = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
        }
        w[u] = u32x4{0u, 0u, 0u, 0u};  // no grammar: every column passes
        if (gram && in) w[u] = *reinterpret_cast<const u32x4 *>(tab + (int64_t)c * 8);
        b[u][0] = b[u][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (BIAS && in) {
          b[u][0] = *reinterpret_cast<const f32x4 *>(brow + (int64_t)c * 8);
          b[u][1] = *reinterpret_cast<const f32x4 *>(brow + (int64_t)c * 8 + 4);
        }
      }
#pragma unroll
      for (int u = 0; u < GD_PF; ++u) {
        const int c = c0 + u * GD_NT;
        if (c >= nchunks) break;
        if constexpr (NOISE) {
          if (noisy) {  // block-uniform
#pragma unroll
            for (int h = 0; h < 2; ++h) {  // one Philox call per column group of four, if it has a legal column
              bool legal[4], any = false;
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int e = 4 * h + j;
                const uint32_t wb = (w[u][e >> 1] >> (16 * (e & 1))) & 0xffffu;
                legal[j] = !(wb & 0x8000u) && b[u][h][j] != -INFINITY;
                any |= legal[j];
              }
              if (!any) continue;
              uint32_t wd[4];
              dfl_rng_words(seed, DFL_RNG_TARGET, pos0 + (uint32_t)m, (uint32_t)(c * 8 + 4 * h), 0u, wd);
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int e = 4 * h + j;
                const uint32_t xb = (x[u][e >> 1] >> (16 * (e & 1))) & 0xffffu;
                const float z = dfl_perturb_w(gd_f(xb), inv_t, wd[j]);
                if (legal[j] && (z > best || (bi == GD_NONE && z == z))) {  // a NaN key never wins
                  best = z;
                  bi = c * 8 + e;
                }
              }
            }
            continue;
          }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t xb = (x[u][e >> 1] >> (16 * (e & 1))) & 0xffffu;
          const uint32_t wb = (w[u][e >> 1] >> (16 * (e & 1))) & 0xffffu;
          const bool legal = !(wb & 0x8000u) && b[u][e >> 2][e & 3] != -INFINITY;  // table >= 0 and not banned
          const float z = gd_f(xb);
          if (legal && (z > best || (bi == GD_NONE && z == z))) {  // columns ascend within a thread; a NaN never wins
            best = z;
            bi = c * 8 + e;
          }
        }
      }
    }
    if (m + 1 < n) gd_load_x(xpre, row + a.ld, tid, nchunks);  // block-uniform; independent of the pick below

    auto take = [&](float ov, int oi) {
      if (oi != GD_NONE && (bi == GD_NONE || ov > best || (ov == best && oi < bi))) {
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
    const int p = m & 1;
    if (lane == 0) {
      sv[p][wave] = best;
      si[p][wave] = bi;
    }
    __syncthreads();
    best = sv[p][0];
    bi = si[p][0];
#pragma unroll
    for (int w = 1; w < 16; ++w) take(sv[p][w], si[p][w]);
    if (bi == GD_NONE) return;  // block-uniform: no legal column that is not NaN — this row and the rows behind keep their ids
    if (tid == 0) blk[m] = (int64_t)bi;
    if (gram) {
      const int nx = tab[bi];
      if (nx < 0 || nx >= a.pool_states - base) return;  // the successor leaves the pool: the rows behind keep their ids
      st = nx;
    }
  }
}

}  // namespace

// The checks both entry points share; `who` names the caller in dfl_last_error.
static int gd_check(const char *who, const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int nrows,
                    const int32_t *dyn, int nrows_dyn_word, const int16_t *table, int64_t table_stride, int pool_states,
                    const int32_t *base, const int32_t *state, const float *bias, int64_t bias_stride,
                    const int64_t *block_ids, int64_t block_stride) {
  DFL_REQUIRE(logits && block_ids && (table || bias) && (!table || (base && state)),
              "%s: null pointer (logits, block_ids, a table with base and state, or a bias table)", who);
  DFL_REQUIRE(V >= 1 && V % 8 == 0 && V <= GD_VMAX, "%s: V=%d is not a multiple of 8 in 8..%d", who, V, GD_VMAX);
  DFL_REQUIRE(tiles >= 0 && ld >= V && ld % 8 == 0 && (tiles <= 1 || (tile_stride >= 16 * ld && tile_stride % 8 == 0)) &&
                  (reinterpret_cast<uintptr_t>(logits) & 15) == 0,
              "%s: bad shape tiles=%d ld=%lld tile_stride=%lld (rows on 16 bytes)", who, tiles, (long long)ld,
              (long long)tile_stride);
  DFL_REQUIRE(!table || (pool_states >= 1 && table_stride >= V && table_stride % 8 == 0 &&
                         (reinterpret_cast<uintptr_t>(table) & 15) == 0),
              "%s: pool_states=%d table_stride=%lld (>= 1; >= V, a multiple of 8, rows on 16 bytes)", who, pool_states,
              (long long)table_stride);
  DFL_REQUIRE(!bias || ((tiles <= 1 || bias_stride >= V) && bias_stride >= 0 && bias_stride % 4 == 0 &&
                        (reinterpret_cast<uintptr_t>(bias) & 15) == 0),
              "%s: bias_stride=%lld (>= V, rows on 16 bytes)", who, (long long)bias_stride);
  DFL_REQUIRE(nrows >= 0 && nrows <= 16, "%s: nrows=%d outside the tile", who, nrows);
  DFL_REQUIRE(nrows_dyn_word < DFL_DYN_WORDS && (nrows_dyn_word < 0 || dyn), "%s: nrows_dyn_word=%d needs a record inside dyn",
              who, nrows_dyn_word);
  DFL_REQUIRE(block_stride >= 0 && (tiles <= 1 || block_stride >= 16), "%s: block_stride=%lld (one row of >= 16 ids per slot)",
              who, (long long)block_stride);
  return DFL_OK;
}

extern "C" int dfl_grammar_draft_rows(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int nrows,
                                      const int32_t *dyn, int nrows_dyn_word, const int16_t *table, int64_t table_stride,
                                      int pool_states, const int32_t *base, const int32_t *state, const float *bias,
                                      int64_t bias_stride, int64_t *block_ids, int64_t block_stride, void *stream) {
  if (int rc = gd_check("dfl_grammar_draft_rows", logits, ld, tile_stride, tiles, V, nrows, dyn, nrows_dyn_word, table,
                        table_stride, pool_states, base, state, bias, bias_stride, block_ids, block_stride))
    return rc;
  if (tiles == 0 || (nrows < 2 && nrows_dyn_word < 0)) return DFL_OK;
  GrammarDraftArgs p{(const bf16_t *)logits, ld,   tile_stride, V,           nrows,     dyn,         nrows_dyn_word, table,
                     table_stride,           pool_states, base, state,       bias,      bias_stride, block_ids,      block_stride};
  if (bias)
    hipLaunchKernelGGL((k_grammar_draft_rows<true, 2>), dim3(tiles), dim3(GD_NT), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL((k_grammar_draft_rows<false, 4>), dim3(tiles), dim3(GD_NT), 0, (hipStream_t)stream, p);
  DFL_CHECK_LAUNCH("dfl_grammar_draft_rows");
  return DFL_OK;
}

extern "C" int dfl_grammar_draft_sample_rows(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V,
                                             int nrows, const int32_t *dyn, int nrows_dyn_word, const int16_t *table,
                                             int64_t table_stride, int pool_states, const int32_t *base,
                                             const int32_t *state, const float *bias, int64_t bias_stride,
                                             int64_t *block_ids, int64_t block_stride, const int64_t *seeds, float inv_t,
                                             const float *inv_ts, int pos_dyn_word, int pos_base, void *stream) {
  const char *who = "dfl_grammar_draft_sample_rows";
  if (int rc = gd_check(who, logits, ld, tile_stride, tiles, V, nrows, dyn, nrows_dyn_word, table, table_stride,
                        pool_states, base, state, bias, bias_stride, block_ids, block_stride))
    return rc;
  DFL_REQUIRE(seeds, "%s: null pointer (seeds: one int64 per slot)", who);
  DFL_REQUIRE(pos_dyn_word < DFL_DYN_WORDS && (pos_dyn_word < 0 || dyn), "%s: pos_dyn_word=%d needs a record inside dyn", who,
              pos_dyn_word);
  DFL_REQUIRE(pos_dyn_word >= 0 || pos_base >= 0, "%s: pos_base=%d is negative", who, pos_base);
  if (tiles == 0 || (nrows < 2 && nrows_dyn_word < 0)) return DFL_OK;
  GrammarDraftNoiseArgs p{};
  static_cast<GrammarDraftArgs &>(p) =
      GrammarDraftArgs{(const bf16_t *)logits, ld,   tile_stride, V,     nrows, dyn,         nrows_dyn_word, table,
                       table_stride,           pool_states, base, state, bias,  bias_stride, block_ids,      block_stride};
  p.seeds = seeds;
  p.inv_ts = inv_ts;
  p.inv_t = inv_t;
  p.pos_word = pos_dyn_word;
  p.pos_base = pos_base;
  if (bias)
    hipLaunchKernelGGL((k_grammar_draft_rows<true, 2, true>), dim3(tiles), dim3(GD_NT), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL((k_grammar_draft_rows<false, 2, true>), dim3(tiles), dim3(GD_NT), 0, (hipStream_t)stream, p);
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}
