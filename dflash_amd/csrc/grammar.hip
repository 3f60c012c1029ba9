// Grammar-constrained decoding: a token automaton on the verify's materialised logits.
//   The pool is one int16 table [pool_states][table_stride >= V] holding several grammars at different base rows;
//   table[(base + s) * table_stride + v] >= 0 is the state after token v in state s, < 0 means v is illegal there.  Per
//   slot: base[slot] (int32, the grammar's first pool row, < 0: no grammar) and state[slot] (int32, relative to base,
//   -1: violated, sticky).  Every row offset is formed in 64 bits.
//   k_grammar_rows:    one 1024-thread block per row of bf16 logits [tiles][16][V], the row / tile conventions of
//                      penalties.hip.  Row m of tile j of slot q
//   1. requests its first logits chunk and the block's ids (one thread each, into LDS), then walks state[q] through
//      block[1 .. 16 j + m] — at most 31 dependent 2-byte loads, the same in every thread of the block, in flight beside
//      the logits
//   2. the dense pass: 16-byte loads of logits and of the state's table row, out = table < 0 ? -inf : logit, 16-byte
//      stores, running argmax (lowest column on ties).  A dead row (an illegal step, no grammar, a violated slot, an id
//      outside the vocabulary) reads no table: it is copied, and its argmax is the raw row's
//   k_grammar_advance: one wave per slot, lane 0 walks a range of committed ids from state[slot] and stores the result.
// No floating-point atomics: the same inputs give the same bits, eager or replayed.
#include "dfl_common.h"

namespace {

constexpr int GR_NT = 1024;               // threads per row
constexpr int GR_VMAX = 155648;           // the row kernels' common limit (19 * 1024 * 8)
constexpr int GR_NONE = 0x7fffffff;
constexpr uint32_t GR_NEG_INF = 0xff80u;  // bf16 -inf

struct GrammarArgs {
  const bf16_t *logits;
  bf16_t *out;
  int64_t ld, tile_stride;
  int V, row0, nrows;
  const int32_t *dyn;
  int nrows_word, tiles_per_req;
  const int16_t *table;
  int64_t table_stride;
  int pool_states;
  const int32_t *base, *state;
  const int64_t *block_ids;
  int64_t block_stride;
  int64_t *out_ids;
  int64_t out_stride;
  int out_off;
};

__device__ __forceinline__ float gr_f(uint32_t b) { return __builtin_bit_cast(float, b << 16); }

// One step of the automaton from pool row `row` (absolute, inside the pool) over id v: the successor relative to the
// grammar's base, or -1 where v is outside the vocabulary, illegal, or leads outside the pool (never indexed).
__device__ __forceinline__ int gr_step(const int16_t *table, int64_t table_stride, int pool_states, int V, int base,
                                       int st, int64_t v) {
  if (v < 0 || v >= V) return -1;
  const int nx = table[(int64_t)(base + st) * table_stride + v];
  return (nx < 0 || nx >= pool_states - base) ? -1 : nx;
}

__global__ __launch_bounds__(GR_NT) void k_grammar_rows(GrammarArgs a) {
  __shared__ float sv[16];
  __shared__ int si[16], sblk[32];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.y;
  int rows = a.nrows;
  if (a.dyn && a.nrows_word >= 0) rows = a.dyn[t * DFL_DYN_WORDS + a.nrows_word] - a.row0;
  if ((int)blockIdx.x >= rows) return;  // block-uniform: rows past the tile's valid count are not written
  const int m = a.row0 + blockIdx.x;
  const int q = t / a.tiles_per_req, j = t - q * a.tiles_per_req;
  const int V = a.V, nchunks = V >> 3;

  const bf16_t *row = a.logits + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;
  bf16_t *dst = a.out + (int64_t)t * a.tile_stride + (int64_t)m * a.ld;

  // the first chunk's logits are requested before the walk: its serial loads run beside them
  u32x4 x = {0u, 0u, 0u, 0u};
  if (tid < nchunks) x = *reinterpret_cast<const u32x4 *>(row + (int64_t)tid * 8);

  // the block's ids do not depend on the state: n threads fetch one each, so that only the table loads are serial
  const int n = a.block_ids ? 16 * j + m : 0;  // in-block tokens block[1 .. n], n <= 31
  if (n > 0) {                                 // block-uniform
    if (tid < n) {
      const int64_t v = a.block_ids[(int64_t)q * a.block_stride + 1 + tid];
      sblk[tid] = (v >= 0 && v < V) ? (int)v : -1;
    }
    __syncthreads();
  }
  // the walk: block-uniform, every thread repeats it (one address per step for the whole block)
  const int base = a.base[q];
  int st = a.state[q];
  if (base < 0 || st < 0 || st >= a.pool_states - base) st = -1;
  for (int i = 0; i < n && st >= 0; ++i) st = gr_step(a.table, a.table_stride, a.pool_states, V, base, st, sblk[i]);
  const bool live = st >= 0;  // block-uniform
  const int16_t *tab = a.table + (live ? (int64_t)(base + st) * a.table_stride : (int64_t)0);

  float best = -INFINITY;
  int bi = GR_NONE;
  for (int c = tid; c < nchunks; c += GR_NT) {
    if (c != tid) x = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
    u32x4 w = {0u, 0u, 0u, 0u};  // a dead row reads no table: every column passes
    if (live) w = *reinterpret_cast<const u32x4 *>(tab + (int64_t)c * 8);
    u32x4 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t xb = (x[e >> 1] >> (16 * (e & 1))) & 0xffffu;
      const uint32_t wb = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
      const uint32_t zb = (wb & 0x8000u) ? GR_NEG_INF : xb;  // table < 0
      if (e & 1)
        o[e >> 1] |= zb << 16;
      else
        o[e >> 1] = zb;
      const float z = gr_f(zb);
      if (z > best || (bi == GR_NONE && z == z)) {  // columns ascend within a thread; a NaN is never the maximum
        best = z;
        bi = c * 8 + e;
      }
    }
    *reinterpret_cast<u32x4 *>(dst + (int64_t)c * 8) = o;
  }
  if (!a.out_ids) return;  // block-uniform
  auto take = [&](float ov, int oi) {
    if (oi != GR_NONE && (bi == GR_NONE || ov > best || (ov == best && oi < bi))) {
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
    a.out_ids[(int64_t)t * a.out_stride + a.out_off + blockIdx.x] = (int64_t)(bi == GR_NONE ? 0 : bi);
  }
}

struct GrammarAdvanceArgs {
  const int16_t *table;
  int64_t table_stride;
  int pool_states, V;
  const int32_t *base;
  int32_t *state;
  const int64_t *ids;
  int64_t ids_stride;
  int ids_len;
  const int32_t *dyn;
  int lo_word, hi_word, lo, hi;
};

__global__ __launch_bounds__(64) void k_grammar_advance(GrammarAdvanceArgs a) {
  const int s = blockIdx.x;
  if (threadIdx.x != 0) return;  // one lane walks: the steps depend on each other
  int lo = a.lo, hi = a.hi;
  if (a.dyn) {
    const int32_t *rec = a.dyn + s * DFL_DYN_WORDS;
    if (rec[DFL_DYN_BS] == 0) return;  // an idle slot is left alone
    lo += rec[a.lo_word];
    hi += rec[a.hi_word];
  }
  lo = max(lo, 0);
  hi = min(hi, a.ids_len);
  const int base = a.base[s];
  int st = a.state[s];
  if (base < 0 || st < 0 || lo >= hi) return;  // no grammar, violated (sticky), or nothing committed
  if (st >= a.pool_states - base) st = -1;
  const int64_t *ids = a.ids + (int64_t)s * a.ids_stride;
  for (int i = lo; i < hi && st >= 0; ++i) st = gr_step(a.table, a.table_stride, a.pool_states, a.V, base, st, ids[i]);
  a.state[s] = st;
}

bool gr_pool_ok(const void *table, int64_t table_stride, int pool_states, int V) {
  return pool_states >= 1 && table_stride >= V && table_stride % 8 == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0;
}

}  // namespace

extern "C" int dfl_grammar_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V, int row0,
                                int nrows, const int32_t *dyn, int nrows_dyn_word, int tiles_per_req, const int16_t *table,
                                int64_t table_stride, int pool_states, const int32_t *base, const int32_t *state,
                                const int64_t *block_ids, int64_t block_stride, int64_t *out_ids, int64_t out_stride,
                                int out_off, void *stream) {
  DFL_REQUIRE(logits && out && table && base && state, "dfl_grammar_rows: null pointer");
  DFL_REQUIRE(V >= 1 && V % 8 == 0 && V <= GR_VMAX, "dfl_grammar_rows: V=%d is not a multiple of 8 in 8..%d", V, GR_VMAX);
  DFL_REQUIRE(tiles_per_req == 1 || tiles_per_req == 2, "dfl_grammar_rows: tiles_per_req=%d", tiles_per_req);
  DFL_REQUIRE(tiles >= 0 && ld >= V && ld % 8 == 0 && (tiles <= 1 || (tile_stride >= 16 * ld && tile_stride % 8 == 0)) &&
                  ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
              "dfl_grammar_rows: bad shape tiles=%d ld=%lld tile_stride=%lld (rows on 16 bytes)", tiles, (long long)ld,
              (long long)tile_stride);
  DFL_REQUIRE(gr_pool_ok(table, table_stride, pool_states, V),
              "dfl_grammar_rows: pool_states=%d table_stride=%lld (>= 1; >= V, a multiple of 8, rows on 16 bytes)",
              pool_states, (long long)table_stride);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "dfl_grammar_rows: rows [%d,%d) outside the tile", row0,
              row0 + nrows);
  DFL_REQUIRE(nrows_dyn_word < DFL_DYN_WORDS && (nrows_dyn_word < 0 || dyn),
              "dfl_grammar_rows: nrows_dyn_word=%d needs a record inside dyn", nrows_dyn_word);
  DFL_REQUIRE(block_stride >= 0 && out_stride >= 0 && out_off >= 0, "dfl_grammar_rows: negative stride or offset");
  if (tiles == 0 || (nrows == 0 && nrows_dyn_word < 0)) return DFL_OK;
  GrammarArgs p{(const bf16_t *)logits, (bf16_t *)out, ld,          tile_stride, V,     row0,      nrows,        dyn,
                nrows_dyn_word,         tiles_per_req, table,       table_stride, pool_states, base, state,  block_ids,
                block_stride,           out_ids,       out_stride,  out_off};
  hipLaunchKernelGGL(k_grammar_rows, dim3(nrows_dyn_word >= 0 ? 16 - row0 : nrows, tiles), dim3(GR_NT), 0,
                     (hipStream_t)stream, p);
  DFL_CHECK_LAUNCH("dfl_grammar_rows");
  return DFL_OK;
}

extern "C" int dfl_grammar_advance(const int16_t *table, int64_t table_stride, int pool_states, int V, const int32_t *base,
                                   int32_t *state, int slots, const int64_t *ids, int64_t ids_stride, int ids_len,
                                   const int32_t *dyn, int lo_word, int hi_word, int lo, int hi, void *stream) {
  DFL_REQUIRE(table && base && state && ids, "dfl_grammar_advance: null pointer");
  DFL_REQUIRE(V >= 1 && V % 8 == 0 && V <= GR_VMAX, "dfl_grammar_advance: V=%d is not a multiple of 8 in 8..%d", V, GR_VMAX);
  DFL_REQUIRE(gr_pool_ok(table, table_stride, pool_states, V),
              "dfl_grammar_advance: pool_states=%d table_stride=%lld (>= 1; >= V, a multiple of 8, rows on 16 bytes)",
              pool_states, (long long)table_stride);
  DFL_REQUIRE(slots >= 0 && ids_len >= 0 && ids_stride >= 0 && (slots <= 1 || ids_stride >= ids_len),
              "dfl_grammar_advance: slots=%d ids_len=%d / ids_stride=%lld", slots, ids_len, (long long)ids_stride);
  DFL_REQUIRE(!dyn || (lo_word >= 0 && lo_word < DFL_DYN_WORDS && hi_word >= 0 && hi_word < DFL_DYN_WORDS),
              "dfl_grammar_advance: lo_word=%d / hi_word=%d outside the record", lo_word, hi_word);
  if (slots == 0) return DFL_OK;
  GrammarAdvanceArgs a{table, table_stride, pool_states, V, base, state, ids, ids_stride, ids_len, dyn, lo_word, hi_word, lo, hi};
  hipLaunchKernelGGL(k_grammar_advance, dim3(slots), dim3(64), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH("dfl_grammar_advance");
  return DFL_OK;
}
