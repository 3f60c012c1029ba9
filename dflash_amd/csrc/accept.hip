// Integer side of the hot path: greedy argmax over materialised logits (the
// target's posterior at T=0, model/utils.py:28-29) and the acceptance scan with
// commit, bonus token, stop test and rollback bookkeeping (model/dflash.py:258-268).
#include "dfl_common.h"
#include "dfl_rng.h"

namespace {

// Seeded draw over materialised bf16 logits, one 1024-thread block per row: argmax_v fmaf(bf16 logit, invT, g) with the
// noise of dfl_rng.h at position pos[r] (or pos0 + r), first index on ties — the same value the EPI_SAMPLE epilogue
// of the lm_head GEMM compares, so both give the same ids.  margin_out (optional): perturbed top-1 minus top-2.
__global__ __launch_bounds__(1024) void k_sample_rows(const bf16_t *__restrict__ logits, int64_t ld, int V, uint64_t seed,
                                                     float inv_t, int rng_stream, int pos0, const int32_t *pos, int extra,
                                                     int64_t *out_ids, float *margin_out) {
  __shared__ float sv[16], s2[16];
  __shared__ int si[16];
  const int r = blockIdx.x;
  const bf16_t *row = logits + (int64_t)r * ld;
  const uint32_t p = (uint32_t)(pos ? pos[r] : pos0 + r);
  float best = -INFINITY, second = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = threadIdx.x; 4 * c < V; c += 1024) {  // one Philox call per 4 columns; columns ascend within a thread
    uint32_t w[4];
    dfl_rng_words(seed, (uint32_t)rng_stream, p, (uint32_t)(4 * c), (uint32_t)extra, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int v = 4 * c + j;
      if (v < V) {
        const float x = dfl_perturb_w(bf2f(row[v]), inv_t, w[j]);
        if (x > best || bi == 0x7fffffff) {
          second = best;
          best = x;
          bi = v;
        } else {
          second = fmaxf(second, x);
        }
      }
    }
  }
  auto merge = [&](float ov, int oi, float os) {
    const bool have = bi != 0x7fffffff, ohave = oi != 0x7fffffff;
    second = fmaxf(second, os);
    if (have && ohave) second = fmaxf(second, fminf(best, ov));
    if (ohave && (!have || ov > best || (ov == best && oi < bi))) {
      best = ov;
      bi = oi;
    }
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64), os = __shfl_xor(second, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    merge(ov, oi, os);
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = best;
    s2[threadIdx.x >> 6] = second;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w) merge(sv[w], si[w], s2[w]);
    out_ids[r] = (int64_t)bi;
    if (margin_out) margin_out[r] = best - second;
  }
}

// One 256-thread block per row.  torch.argmax returns the FIRST maximal index, so
// the reduction is on (value desc, index asc).  Values are compared as fp32 (exact
// for bf16 inputs).
template <typename T, int VEC>
__global__ __launch_bounds__(256) void k_argmax(const T *__restrict__ logits, int64_t V, int64_t *__restrict__ ids) {
  __shared__ float sv[4];
  __shared__ int64_t si[4];
  const T *row = logits + (int64_t)blockIdx.x * V;
  float best = -INFINITY;
  int64_t bi = INT64_MAX;
  auto take = [&](float v, int64_t i) {
    if (v > best || (v == best && i < bi) || (bi == INT64_MAX)) {
      best = v;
      bi = i;
    }
  };
  const int64_t nvec = ((reinterpret_cast<uintptr_t>(row) % (VEC * sizeof(T))) == 0) ? V / VEC : 0;
  typedef T vec_t __attribute__((ext_vector_type(VEC)));
  for (int64_t c = threadIdx.x; c < nvec; c += 256) {
    const vec_t v = *reinterpret_cast<const vec_t *>(row + c * VEC);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const float f = (float)v[j];
      if (f > best || bi == INT64_MAX) {  // indices ascend within a thread
        best = f;
        bi = c * VEC + j;
      }
    }
  }
  for (int64_t i = nvec * VEC + threadIdx.x; i < V; i += 256) take((float)row[i], i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int64_t oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) {
      best = ov;
      bi = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = best;
    si[threadIdx.x >> 6] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (sv[w] > best || (sv[w] == best && si[w] < bi)) {
        best = sv[w];
        bi = si[w];
      }
    ids[blockIdx.x] = bi;
  }
}

// Single wavefront.  Lane i compares draft token i+1 with the target's token for
// the same position; the accepted length is the number of trailing-zero-free ones
// of the ballot (first mismatch by ffs), no host round trip.
// next_block (optional): the NEXT cycle's block, re-armed here so that the host need not copy it out of output_ids
// (model/dflash.py:235: block = output_ids[:, start:start+bs] = the bonus token followed by mask ids) — rearm_n slots.
__global__ __launch_bounds__(64) void k_accept_commit(const int64_t *block_ids, const int64_t *posterior, int bs,
                                                      int64_t *output_ids, int64_t output_len, int32_t *dyn,
                                                      const int64_t *stop_ids, int n_stop, int32_t *result,
                                                      int64_t *next_block, int rearm_n, int64_t mask_id, int32_t *dyn_t) {
  const int i = threadIdx.x;
  const int start = dyn[DFL_DYN_START];
  const bool cmp = i < bs - 1;
  const bool eq = cmp && (block_ids[i + 1] == posterior[i]);
  const unsigned long long mism = __ballot(cmp && !eq);
  int acc = mism ? (int)__builtin_ctzll(mism) : bs - 1;  // leading matches, 0..bs-1
  // commit block[0..acc] at start.., then the target's own token (model/dflash.py:259-260)
  int64_t tok = -1;
  if (i <= acc)
    tok = block_ids[i];
  else if (i == acc + 1)
    tok = posterior[acc];
  if (i <= acc + 1 && start + i < output_len) output_ids[start + i] = tok;
  bool hit = false;
  if (i <= acc + 1)
    for (int s = 0; s < n_stop; ++s) hit |= (tok == stop_ids[s]);
  const bool any_stop = __ballot(hit) != 0ull;
  if (next_block && i < rearm_n) {  // every compared id was read before the ballot above: in-place re-arm is safe
    const int64_t bonus = posterior[acc];
    next_block[i] = i == 0 ? bonus : mask_id;
  }
  if (i == 0) {
    const int new_start = start + acc + 1;
    dyn[DFL_DYN_S] = start;         // draft cache keeps rows [0, start): crop(start), :246
    dyn[DFL_DYN_TAU] = acc + 1;     // next cycle's context rows, :263
    dyn[DFL_DYN_POS0] = start;
    dyn[DFL_DYN_START] = new_start; // :261
    dyn[DFL_DYN_STOP] |= any_stop ? 1 : 0;
    dyn[DFL_DYN_CYCLE] += 1;
    if (dyn_t) {  // the block-form record of the NEXT verify (its block size word stays): rows kept = positions = new start
      dyn_t[DFL_DYN_S] = new_start;
      dyn_t[DFL_DYN_TAU] = 0;
      dyn_t[DFL_DYN_POS0] = new_start;
      dyn_t[DFL_DYN_START] = new_start;
    }
    if (result) {
      // Hand-over a CPU thread may be polling (pinned host memory): the payload words first, then — behind a
      // system-scope release, so that no store can overtake them — the cycle counter as the LAST word.  The host
      // polls word 3 and reads words 0..2 only after it has changed (generate.py); no reliance on a 16-byte store
      // arriving whole.
      result[0] = acc;
      result[1] = new_start;
      result[2] = dyn[DFL_DYN_STOP];
      __hip_atomic_store(&result[3], dyn[DFL_DYN_CYCLE], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// Ragged batch: one wavefront per request (grid.x = request).  Besides the draft-form
// lengths dyn_d (S = rows kept in the draft cache, tau = context rows of the next cycle) it
// maintains the block-form lengths dyn_t = {S = new start, tau = 0, pos0 = new start} which
// the target verify AND the draft's block stage read, so that a steady-state cycle needs no
// host-side length update at all.
__global__ __launch_bounds__(64) void k_accept_commit_b(const int64_t *block_ids, int64_t blk_stride,
                                                        const int64_t *posterior, int64_t post_stride,
                                                        int64_t *output_ids, int64_t out_stride, int64_t output_len,
                                                        int32_t *dyn_d, int32_t *dyn_t, const int64_t *stop_ids,
                                                        int n_stop, int32_t *result, int64_t *next_block,
                                                        int64_t mask_id, int rearm_n, int tiles_per_req, int32_t *dyn_dt,
                                                        int32_t *dyn_tt) {
  const int r = blockIdx.x, i = threadIdx.x;
  if (next_block) next_block += r * blk_stride;
  block_ids += r * blk_stride;
  posterior += r * post_stride;
  output_ids += r * out_stride;
  dyn_d += r * DFL_DYN_WORDS;
  dyn_t += r * DFL_DYN_WORDS;
  const int start = dyn_d[DFL_DYN_START];
  const int bs = dyn_d[DFL_DYN_BS];
  const bool cmp = i < bs - 1;
  const bool eq = cmp && (block_ids[i + 1] == posterior[i]);
  const unsigned long long mism = __ballot(cmp && !eq);
  const int acc = mism ? (int)__builtin_ctzll(mism) : bs - 1;
  int64_t tok = -1;
  if (i <= acc)
    tok = block_ids[i];
  else if (i == acc + 1 && bs > 0)  // (an idle request has acc = -1: nothing of its rows is read)
    tok = posterior[acc];
  if (bs > 0 && i <= acc + 1 && start + i < output_len) output_ids[start + i] = tok;
  bool hit = false;
  if (bs > 0 && i <= acc + 1)
    for (int s = 0; s < n_stop; ++s) hit |= (tok == stop_ids[s]);
  const bool any_stop = __ballot(hit) != 0ull;
  // the next cycle's block = output_ids[new start .. +bs) = [bonus token, mask, mask, ...]
  // (model/dflash.py:235); all reads of block_ids above precede these writes in the wave
  const int64_t bonus = __shfl(tok, acc + 1, 64);  // posterior[acc]; every lane takes part
  if (next_block && bs > 0 && i < rearm_n) next_block[i] = i == 0 ? bonus : mask_id;
  if (i == 0 && bs > 0) {
    const int new_start = start + acc + 1;
    const int stop = dyn_d[DFL_DYN_STOP] | (any_stop ? 1 : 0);
    const int cyc = dyn_d[DFL_DYN_CYCLE] + 1;
    dyn_d[DFL_DYN_S] = start;
    dyn_d[DFL_DYN_TAU] = acc + 1;
    dyn_d[DFL_DYN_POS0] = start;
    dyn_d[DFL_DYN_START] = new_start;
    dyn_d[DFL_DYN_STOP] = stop;
    dyn_d[DFL_DYN_CYCLE] = cyc;
    dyn_t[DFL_DYN_S] = new_start;
    dyn_t[DFL_DYN_TAU] = 0;
    dyn_t[DFL_DYN_BS] = bs;
    dyn_t[DFL_DYN_POS0] = new_start;
    dyn_t[DFL_DYN_START] = new_start;
    dyn_t[DFL_DYN_STOP] = stop;
    dyn_t[DFL_DYN_CYCLE] = cyc;
    // blocks of 17..32 rows: the request's tiles have length records of their own for the per-tile launches (GEMMs,
    // norms, context K/V append): tile j holds context rows 16 j .. of the tau accepted ones and block rows 16 j ..
    for (int j = 0; dyn_dt && j < tiles_per_req; ++j) {
      int32_t *dd = dyn_dt + (r * tiles_per_req + j) * DFL_DYN_WORDS, *dt = dyn_tt + (r * tiles_per_req + j) * DFL_DYN_WORDS;
      const int tj = acc + 1 - 16 * j, bj = bs - 16 * j;
      dd[DFL_DYN_S] = start + 16 * j;
      dd[DFL_DYN_TAU] = tj < 0 ? 0 : (tj > 16 ? 16 : tj);
      dd[DFL_DYN_POS0] = start + 16 * j;
      dd[DFL_DYN_START] = new_start;
      dt[DFL_DYN_S] = new_start;
      dt[DFL_DYN_TAU] = 0;
      dt[DFL_DYN_BS] = bj < 0 ? 0 : (bj > 16 ? 16 : bj);
      dt[DFL_DYN_POS0] = new_start;
      dt[DFL_DYN_START] = new_start;
    }
    if (result) {
      result[r * 4 + 0] = acc;
      result[r * 4 + 1] = new_start;
      result[r * 4 + 2] = stop;
      result[r * 4 + 3] = cyc;
    }
  }
}

}  // namespace

extern "C" int dfl_argmax(const void *logits, int dtype, int rows, int64_t V, int64_t *ids, void *stream) {
  DFL_REQUIRE(logits && ids, "dfl_argmax: null pointer");
  DFL_REQUIRE(rows >= 0 && V > 0, "dfl_argmax: bad shape rows=%d V=%lld", rows, (long long)V);
  DFL_REQUIRE(dtype == 0 || dtype == 1, "dfl_argmax: dtype must be 0 (bf16) or 1 (fp32)");
  if (rows == 0) return DFL_OK;
  if (dtype == 0)
    hipLaunchKernelGGL((k_argmax<bf16_t, 8>), dim3(rows), dim3(256), 0, (hipStream_t)stream, (const bf16_t *)logits, V, ids);
  else
    hipLaunchKernelGGL((k_argmax<float, 4>), dim3(rows), dim3(256), 0, (hipStream_t)stream, (const float *)logits, V, ids);
  DFL_CHECK_LAUNCH("dfl_argmax");
  return DFL_OK;
}

extern "C" int dfl_sample_rows(const void *logits, int64_t ld, int rows, int V, uint64_t seed, float inv_t, int rng_stream,
                               int pos0, const int32_t *pos, int extra, int64_t *out_ids, float *margin_out, void *stream) {
  DFL_REQUIRE(logits && out_ids, "dfl_sample_rows: null pointer");
  DFL_REQUIRE(rows >= 0 && V > 0 && ld >= V, "dfl_sample_rows: bad shape rows=%d V=%d ld=%lld", rows, V, (long long)ld);
  DFL_REQUIRE(inv_t > 0.f && inv_t <= 1e5f, "dfl_sample_rows: inv_t=%g outside (0, 1e5]", (double)inv_t);
  DFL_REQUIRE(rng_stream == (int)DFL_RNG_TARGET || rng_stream == (int)DFL_RNG_DRAFT, "dfl_sample_rows: unknown stream %d",
              rng_stream);
  if (rows == 0) return DFL_OK;
  hipLaunchKernelGGL(k_sample_rows, dim3(rows), dim3(1024), 0, (hipStream_t)stream, (const bf16_t *)logits, ld, V, seed, inv_t,
                     rng_stream, pos0, pos, extra, out_ids, margin_out);
  DFL_CHECK_LAUNCH("dfl_sample_rows");
  return DFL_OK;
}

// next_block == NULL: no re-arm (rearm_n / mask_id unused); dyn_t (optional) needs next_block.
extern "C" int dfl_accept_commit(const int64_t *block_ids, const int64_t *posterior, int bs, int64_t *output_ids,
                                 int64_t output_len, int32_t *dyn, const int64_t *stop_ids, int n_stop,
                                 int32_t *result, int64_t *next_block, int rearm_n, int64_t mask_id, int32_t *dyn_t,
                                 void *stream) {
  DFL_REQUIRE(block_ids && posterior && output_ids && dyn, "dfl_accept_commit: null pointer");
  DFL_REQUIRE(next_block || !dyn_t, "dfl_accept_commit: dyn_t is kept only together with the re-arm (next_block is null)");
  // lane acc + 1 <= bs writes the bonus token: bs = 64 would need a 65th lane
  DFL_REQUIRE(bs >= 1 && bs <= 63, "dfl_accept_commit: bs=%d outside 1..63", bs);
  DFL_REQUIRE(!next_block || (rearm_n >= 1 && rearm_n <= 64), "dfl_accept_commit: rearm_n=%d outside 1..64", rearm_n);
  DFL_REQUIRE(n_stop == 0 || stop_ids, "dfl_accept_commit: n_stop>0 without stop_ids");
  if (!next_block) rearm_n = 0, mask_id = 0;
  hipLaunchKernelGGL(k_accept_commit, dim3(1), dim3(64), 0, (hipStream_t)stream, block_ids, posterior, bs, output_ids,
                     output_len, dyn, stop_ids, n_stop, result, next_block, rearm_n, mask_id, dyn_t);
  DFL_CHECK_LAUNCH("dfl_accept_commit");
  return DFL_OK;
}

// Tile records given (required for tiles_per_req == 2): the per-tile form, whose block holds 16 * tiles_per_req slots.
extern "C" int dfl_accept_commit_batch(const int64_t *block_ids, int64_t blk_stride, const int64_t *posterior,
                                       int64_t post_stride, int R, int64_t *output_ids, int64_t out_stride,
                                       int64_t output_len, int32_t *dyn_d, int32_t *dyn_t, const int64_t *stop_ids,
                                       int n_stop, int32_t *result, int64_t *next_block, int64_t mask_id, int tiles_per_req,
                                       int32_t *dyn_d_tiles, int32_t *dyn_t_tiles, void *stream) {
  DFL_REQUIRE(block_ids && posterior && output_ids && dyn_d && dyn_t, "dfl_accept_commit_batch: null pointer");
  DFL_REQUIRE(R >= 1 && R <= 1024 && (tiles_per_req == 1 || tiles_per_req == 2),
              "dfl_accept_commit_batch: R=%d tiles_per_req=%d outside range", R, tiles_per_req);
  if (tiles_per_req == 2 || dyn_d_tiles || dyn_t_tiles) {
    DFL_REQUIRE(dyn_d_tiles && dyn_t_tiles, "dfl_accept_commit_batch: null tile record");
    DFL_REQUIRE(blk_stride >= 16 * tiles_per_req, "dfl_accept_commit_batch: blk_stride=%lld below the %d block slots",
                (long long)blk_stride, 16 * tiles_per_req);
  }
  DFL_REQUIRE(n_stop == 0 || stop_ids, "dfl_accept_commit_batch: n_stop>0 without stop_ids");
  hipLaunchKernelGGL(k_accept_commit_b, dim3(R), dim3(64), 0, (hipStream_t)stream, block_ids, blk_stride, posterior,
                     post_stride, output_ids, out_stride, output_len, dyn_d, dyn_t, stop_ids, n_stop, result, next_block,
                     mask_id, 16 * tiles_per_req, tiles_per_req, dyn_d_tiles, dyn_t_tiles);
  DFL_CHECK_LAUNCH("dfl_accept_commit_batch");
  return DFL_OK;
}

// ---- slot admission (ragged batch): one launch re-arms slot r for a newly prefilled request ----------------------
namespace {

// Every record a decode cycle reads for slot r, written from device-resident inputs: the id row (prompt, first token,
// mask), the block, the context tile (the prompt's last n_tail tapped rows, 16 bytes per lane, the rest zero), both
// length records and the seed.  The first token is read from device memory: it never visits the host.
__global__ __launch_bounds__(256) void k_admit_slot(int r, const int64_t *__restrict__ prompt_ids, int P,
                                                    const int64_t *__restrict__ first_token, int64_t *output_ids,
                                                    int64_t out_len, int64_t *block, int64_t *post, int blk_w, int32_t *result,
                                                    const bf16_t *__restrict__ tail_rows, int64_t ld_tail, int n_tail,
                                                    bf16_t *taps_tile, int fc_in, int32_t *dyn_d, int32_t *dyn_t, int bs,
                                                    int64_t *seeds, int64_t seed, int64_t mask_id) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  const int vec_per_row = fc_in / 8;
  const int64_t nvec = (int64_t)16 * vec_per_row;
  for (int64_t v = tid; v < nvec; v += nthr) {
    const int row = (int)(v / vec_per_row), col = (int)(v % vec_per_row);
    u32x4 x = {0u, 0u, 0u, 0u};
    if (row < n_tail) x = *reinterpret_cast<const u32x4 *>(tail_rows + (int64_t)row * ld_tail + 8 * col);
    *reinterpret_cast<u32x4 *>(taps_tile + (int64_t)row * fc_in + 8 * col) = x;
  }
  const int64_t first = *first_token;
  for (int64_t i = tid; i < out_len; i += nthr) output_ids[i] = i < P ? prompt_ids[i] : (i == P ? first : mask_id);
  if (blockIdx.x != 0) return;
  const int i = threadIdx.x;
  if (i < blk_w) {
    block[i] = i == 0 ? first : mask_id;
    post[i] = 0;
  }
  if (i < 4) result[i] = 0;
  if (i < DFL_DYN_WORDS) {
    const int S = P - n_tail;
    int d = 0, t = 0;
    switch (i) {
      case DFL_DYN_S: d = S, t = P; break;
      case DFL_DYN_TAU: d = n_tail; break;
      case DFL_DYN_BS: d = bs, t = bs; break;
      case DFL_DYN_POS0: d = S, t = P; break;
      case DFL_DYN_START: d = P, t = P; break;
      default: break;   // DFL_DYN_STOP, DFL_DYN_CYCLE and the spare word: cleared
    }
    dyn_d[i] = d;
    dyn_t[i] = t;
  }
  if (i == 0 && seeds) seeds[r] = seed;
}

}  // namespace

extern "C" int dfl_admit_slot(int r, int n_slots, const int64_t *prompt_ids, int P, const int64_t *first_token,
                              int64_t *output_ids, int64_t out_stride, int64_t out_len, int64_t *block, int64_t *post,
                              int blk_w, int32_t *result, const void *tail_rows, int64_t ld_tail, int n_tail, void *taps,
                              int fc_in, int32_t *dyn_d, int32_t *dyn_t, int bs, int64_t *seeds, int64_t seed,
                              int64_t mask_id, void *stream) {
  DFL_REQUIRE(n_slots >= 1 && r >= 0 && r < n_slots, "dfl_admit_slot: slot r=%d outside 0..%d", r, n_slots - 1);
  DFL_REQUIRE(P >= 1 && (int64_t)P + 1 <= out_len && out_stride >= out_len,
              "dfl_admit_slot: prompt of %d ids + first token does not fit out_len=%lld", P, (long long)out_len);
  DFL_REQUIRE(n_tail >= 0 && n_tail <= 16 && n_tail <= P, "dfl_admit_slot: n_tail=%d outside 0..min(16, P)", n_tail);
  DFL_REQUIRE(blk_w >= 1 && blk_w <= 64 && bs >= 0 && bs <= blk_w, "dfl_admit_slot: blk_w=%d bs=%d outside range", blk_w, bs);
  DFL_REQUIRE(fc_in >= 8 && fc_in % 8 == 0 && ld_tail % 8 == 0 && (n_tail == 0 || ld_tail >= fc_in) &&
                  (uintptr_t)tail_rows % 16 == 0 && (uintptr_t)taps % 16 == 0,
              "dfl_admit_slot: tapped rows need fc_in %% 8 == 0 and 16-byte aligned rows (fc_in=%d ld=%lld)", fc_in,
              (long long)ld_tail);
  DFL_REQUIRE(prompt_ids && first_token && output_ids && block && post && result && taps && dyn_d && dyn_t,
              "dfl_admit_slot: null pointer");
  DFL_REQUIRE(n_tail == 0 || tail_rows, "dfl_admit_slot: null pointer (tail_rows with n_tail > 0)");
  const int64_t work = (int64_t)16 * (fc_in / 8) > out_len ? (int64_t)16 * (fc_in / 8) : out_len;
  const int grid = (int)((work + 255) / 256 < 128 ? (work + 255) / 256 : 128);
  hipLaunchKernelGGL(k_admit_slot, dim3(grid), dim3(256), 0, (hipStream_t)stream, r, prompt_ids, P, first_token,
                     output_ids + (int64_t)r * out_stride, out_len, block + (int64_t)r * blk_w, post + (int64_t)r * blk_w, blk_w,
                     result + 4 * r, (const bf16_t *)tail_rows, ld_tail, n_tail, (bf16_t *)taps + (int64_t)r * 16 * fc_in, fc_in,
                     dyn_d + r * DFL_DYN_WORDS, dyn_t + r * DFL_DYN_WORDS, bs, seeds, seed, mask_id);
  DFL_CHECK_LAUNCH("dfl_admit_slot");
  return DFL_OK;
}
