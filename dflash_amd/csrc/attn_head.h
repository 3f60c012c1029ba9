// The single-request attention stage as a device function (attn_head.hip: bf16 cache; attn_head_kv8.hip: e4m3 cache):
// argument block, wave butterflies, the norm + RoPE row items, LDS layout and attn_head_body itself.
#pragma once
#include "gemm_rows.h"
#include <stdlib.h>
#include <type_traits>

namespace {

typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

struct HeadAttnArgs {
  const bf16_t *xq;  // block rows [bs][ldq]: q | k | v column blocks
  int64_t ldq;
  int q_col, k_col, v_col;
  const bf16_t *xc;  // context rows [tau][ldc] (k, v only); may be null when tau == 0
  int64_t ldc;
  int ck_col, cv_col;
  const bf16_t *q_w, *k_w;
  float eps;
  const bf16_t *cos_tab, *sin_tab;
  int max_pos;
  bf16_t *kc, *vc;
  int cache_rows;
  int n_q, n_kv, G;
  float scale_log2;
  int causal;
  const int32_t *dyn;
  int S, tau, bs, pos0;  // used when dyn == nullptr
  bf16x8 *out_frag;
  int64_t out_tile_stride;  // bf16x8 units between the frag16 buffers of the two query tiles
  float *o_part;   // [ns][n_q][QT*16][128]
  float *ml_part;  // [ns][n_q][QT*16][2]
  int *tickets;    // [n_q]
  int ns_old;      // splits over the cached (old) keys; split ns_old owns the new rows
  // candidate blocks (grid.z = candidate, SURVEY.md §8f-4: several drafts of one block verified against ONE cached
  // prefix): candidate c reads its block rows at xq + c * xq_cand_stride, writes its frag16 output at
  // out_frag + c * out_cand_stride, its partials / tickets at + c * ws_cand_stride floats, and its NEW K/V rows
  // not into the cache but into kv_out rows [0, bs): [c][n_kv][out_rows][128] — the caller copies the winner's.
  // The same dimension carries the REQUESTS of a ragged batch (dfl_attn_head_batch): then every request also has its
  // own length record (dyn + c * dyn_cand_stride ints) and its own cache (+ c * cache_cand_stride elements).
  int64_t xq_cand_stride, out_cand_stride, ws_cand_stride, cache_cand_stride;
  int dyn_cand_stride;
  // XF32 instantiations (round 4: dfl_attn_head_batch_f32): the block rows arrive as the fp32 K-PART SUMS of the qkv GEMM
  // (dfl_gemm_f32_batch: [part][tile rows][ldq]) instead of finished bf16 rows; a row value is bf16(part 0 + part 1) —
  // the Linear's bf16 output, summed in the order the GEMM's own combine used.  The K parts of q/k/v then meet HERE (these
  // loads are a few KB per workgroup) and the qkv launch carries no slabs, ticket or combine phase (18.3 -> 14.7 us at 4
  // tiles).  ldq / the column offsets / xq_cand_stride count floats of one part.
  const float *xq32;
  int64_t part_stride32;  // floats between the parts
  int nparts32;           // 1 or 2
  bf16_t *k_out, *v_out;   // null: the new rows go to the cache at rows S + rel
  int64_t kv_out_cand_stride;
  int out_rows;
};

// 64-lane butterflies on VALU: v_permlane16_swap / v_permlane32_swap (gfx950) instead of
// ds_bpermute round trips (~100 cycles each on a lone wave).  swap16 exchanges the odd 16-lane rows of
// its first operand with the even rows of the second; swap32 the upper half of the first with the lower
// half of the second: started from two copies of x, the two results are x's rows {0,0,2,2} and
// {1,1,3,3} (resp. halves {lo,lo} and {hi,hi}), whose max / sum is the xor-16 (xor-32) butterfly.
// Inline asm, not __builtin_amdgcn_permlane{16,32}_swap: hipcc (ROCm 7.2) treats the builtin's two
// results as equal when its operands are (it reasons per lane) and folds max(r0, r1) to r0.  The
// s_nop covers the VALU-write -> permlane-swap-read hazard the compiler pads the same way.
__device__ __forceinline__ void swap16(float &a, float &b) {
  asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ void swap32(float &a, float &b) {
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
__device__ __forceinline__ float wave_g_max(float v) {  // max over the four 16-lane rows, in every lane
  float a = v, b = v;
  swap16(a, b);
  a = b = fmaxf(a, b);
  swap32(a, b);
  return fmaxf(a, b);
}
__device__ __forceinline__ float wave_g_sum(float v) {
  float a = v, b = v;
  swap16(a, b);
  a = b = a + b;
  swap32(a, b);
  return a + b;
}

// NP items per 16-lane group, an item = 128 values of one (row, head): lane c = l & 15 owns
// d = 8c .. 8c+7.  Loads first (all in flight), then Linear-output values -> per-head RMSNorm
// (Qwen3RMSNorm over head_dim, model/dflash.py:72,79; skipped when nw == nullptr) -> RoPE
// (rotate_half pairs lane c with lane c^8: DPP row_ror:8), each product and sum rounded to bf16
// where torch rounds (model/dflash.py:22-28).  src[p] == nullptr marks an absent item.
template <int NP>
struct RopeLoads {
  bf16x8 xv[NP], cs[NP], sn[NP], wv;
  f32x4 pa[NP][2], pb[NP][2];  // XF32: the item's 8 values of K part 0 / part 1 (untouched, i.e. optimised away, otherwise)
};

// issue: the loads only (row values, cos/sin rows, norm weight).  A wave's vector loads return in issue
// order, so these few KB are requested BEFORE the K/V tile burst and arrive within one round trip.
template <int NP>
__device__ __forceinline__ void rope_issue(const bf16_t *const (&src)[NP], const int (&pos)[NP], const bf16_t *nw,
                                           const bf16_t *cos_tab, const bf16_t *sin_tab, int max_pos, const bf16_t *safe,
                                           int l, RopeLoads<NP> &ld) {
  const int d0 = (l & 15) * 8;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    ld.xv[p] = *reinterpret_cast<const bf16x8 *>((src[p] ? src[p] : safe) + d0);
    int pp = pos[p] < max_pos ? pos[p] : max_pos - 1;
    pp = pp < 0 ? 0 : pp;
    ld.cs[p] = *reinterpret_cast<const bf16x8 *>(cos_tab + (int64_t)pp * 64 + (d0 & 63));
    ld.sn[p] = *reinterpret_cast<const bf16x8 *>(sin_tab + (int64_t)pp * 64 + (d0 & 63));
  }
  // unconditional (a load under a branch makes hipcc wait vmcnt(0) at the join): no norm -> 16 B nobody uses
  ld.wv = *reinterpret_cast<const bf16x8 *>((nw ? nw : safe) + d0);
}

// XF32: the same requests for items given as fp32 K-part sums (src[p]: part 0; part 1 at + part_stride; nparts 1: part 1
// is a second read of part 0 that the finish ignores — no load under a branch).  rope_sum32 turns them into the bf16
// Linear outputs rope_finish expects.
template <int NP>
__device__ __forceinline__ void rope_issue32(const float *const (&src)[NP], const int (&pos)[NP], const bf16_t *nw,
                                             const bf16_t *cos_tab, const bf16_t *sin_tab, int max_pos, const float *safe32,
                                             const bf16_t *safe, int64_t part_stride, int nparts, int l, RopeLoads<NP> &ld) {
  const int d0 = (l & 15) * 8;
  const int64_t ps = nparts > 1 ? part_stride : 0;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const float *b = (src[p] ? src[p] : safe32) + d0;
    ld.pa[p][0] = *reinterpret_cast<const f32x4 *>(b);
    ld.pa[p][1] = *reinterpret_cast<const f32x4 *>(b + 4);
    ld.pb[p][0] = *reinterpret_cast<const f32x4 *>(b + ps);
    ld.pb[p][1] = *reinterpret_cast<const f32x4 *>(b + ps + 4);
    int pp = pos[p] < max_pos ? pos[p] : max_pos - 1;
    pp = pp < 0 ? 0 : pp;
    ld.cs[p] = *reinterpret_cast<const bf16x8 *>(cos_tab + (int64_t)pp * 64 + (d0 & 63));
    ld.sn[p] = *reinterpret_cast<const bf16x8 *>(sin_tab + (int64_t)pp * 64 + (d0 & 63));
  }
  ld.wv = *reinterpret_cast<const bf16x8 *>((nw ? nw : safe) + d0);
}
template <int NP>
__device__ __forceinline__ void rope_sum32(RopeLoads<NP> &ld, int nparts) {
#pragma unroll
  for (int p = 0; p < NP; ++p)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s0 = ld.pa[p][j >> 2][j & 3], s1 = ld.pb[p][j >> 2][j & 3];
      ld.xv[p][j] = f2bf(nparts > 1 ? s0 + s1 : s0);  // fixed part order, one rounding: the Linear's bf16 output
    }
}

template <int NP>
__device__ __forceinline__ void rope_finish(const RopeLoads<NP> &ld, const bool (&rope)[NP], bool has_norm, float eps, int l,
                                            bf16x8 (&out)[NP]) {
  const int c = l & 15;
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    float x[8], n[8];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] = bf2f(ld.xv[p][j]);
      ss += x[j] * x[j];
    }
    if (has_norm) {
      ss += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, ss), 0xB1, 0xF, 0xF, true));
      ss += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, ss), 0x4E, 0xF, 0xF, true));
      ss += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, ss), 0x141, 0xF, 0xF, true));
      ss += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, ss), 0x140, 0xF, 0xF, true));
      const float rstd = rsqrtf(ss * (1.f / 128.f) + eps);
#pragma unroll
      for (int j = 0; j < 8; ++j) n[j] = rbf(bf2f(ld.wv[j]) * rbf(x[j] * rstd));
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) n[j] = x[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pn =
          __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, n[j]), 0x128, 0xF, 0xF, true));
      const float cj = bf2f(ld.cs[p][j]), sj = bf2f(ld.sn[p][j]);
      const float r = rbf(rbf(n[j] * cj) + rbf((c < 8 ? -pn : pn) * sj));
      out[p][j] = f2bf(rope[p] ? r : x[j]);
    }
  }
}

template <int NP>
__device__ __forceinline__ void rope_items(const bf16_t *const (&src)[NP], const int (&pos)[NP], const bool (&rope)[NP],
                                           const bf16_t *nw, float eps, const bf16_t *cos_tab, const bf16_t *sin_tab,
                                           int max_pos, const bf16_t *safe, int l, bf16x8 (&out)[NP]) {
  RopeLoads<NP> ld;
  rope_issue<NP>(src, pos, nw, cos_tab, sin_tab, max_pos, safe, l, ld);
  rope_finish<NP>(ld, rope, nw != nullptr, eps, l, out);
}

__device__ __forceinline__ int k_swz(int row, int ch) { return row * 256 + ((ch ^ (row & 15)) << 4); }
__device__ __forceinline__ int v_swz(int row, int ch) {
  return row * 256 + ((((ch >> 1) ^ (row & 7)) << 5) | ((ch & 1) << 4));
}

// ---- KV8: the cache as OCP e4m3 codes, one power-of-two fp32 scale per (row, kv head) (dflash_hip.h, "e4m3 KV cache") ----
// The argument block of the e4m3 form: kc / vc point at the CODES (uint8 [n_kv][cache_rows][128], one byte per element —
// the base's typed pointers are only carried), the scales sit beside them.
struct HeadAttnArgs8 : HeadAttnArgs {
  float *k_scale, *v_scale;  // [n_kv][cache_rows]
};

__device__ __forceinline__ float row_max16(float v) {  // max over the 16 lanes of a DPP row, in each of them
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)));
  v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)));
  return v;
}

// One row of 128 bf16 values held by a 16-lane group (lane c: elements 8c .. 8c+7) -> its scale, the lane's 8 codes and
// their dequantised values.  The rule of ops.quantize_kv_rows on integers: amax = m * 2^e with m in [1, 2), 448 = 1.75 * 2^8,
// so ceil(log2(amax / 448)) = e - 8, one more where m > 1.75; not below 2^-64; 1 for an all-zero row.  x / scale is exact
// (a power of two), the conversion rounds to nearest even and never sees more than 448; code * scale is an exact bf16.
typedef __attribute__((ext_vector_type(2))) short s16x2;
typedef __attribute__((ext_vector_type(2))) uint32_t kv8_codes;
typedef __attribute__((ext_vector_type(2))) int i32x2;
typedef __attribute__((address_space(3))) i32x2 lds_i32x2;
#ifndef DFL_KV8_V_CODES
#define DFL_KV8_V_CODES 1  // 1: the V tile holds codes, read with ds_read_b64_tr_b8; 0: the measured loser, kept for A/B builds
#endif
__device__ __forceinline__ void kv8_quant_row(const bf16x8 x, float &scale, kv8_codes &codes, bf16x8 &deq) {
  float am = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) am = fmaxf(am, fabsf(bf2f(x[j])));
  const uint32_t ab = __builtin_bit_cast(uint32_t, row_max16(am));
  int se = (int)(ab >> 23) - 8 + ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
  se = se < 127 - 64 ? 127 - 64 : se;
  se = ab == 0 ? 127 : se;
  scale = __builtin_bit_cast(float, (uint32_t)se << 23);
  const float inv = __builtin_bit_cast(float, (uint32_t)(254 - se) << 23);
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    s16x2 w = {0, 0};
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, bf2f(x[4 * d]) * inv, bf2f(x[4 * d + 1]) * inv, 1.0f, false);
    w = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(w, bf2f(x[4 * d + 2]) * inv, bf2f(x[4 * d + 3]) * inv, 1.0f, true);
    codes[d] = __builtin_bit_cast(uint32_t, w);
    const bf16x2 lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(codes[d], scale, false);
    const bf16x2 hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(codes[d], scale, true);
    deq[4 * d] = lo[0], deq[4 * d + 1] = lo[1], deq[4 * d + 2] = hi[0], deq[4 * d + 3] = hi[1];
  }
}

#ifdef DFL_ATTN_STAMPS  // diagnostic build only (scripts/dbg_attn_head_stamps.py): 100 MHz wall stamps of lane 0 of
// workgroup (kv head 0, query head 0) of the first old-key split [0] and of the new-row split [1]
__device__ unsigned long long g_hstamps[2][8];
#define HSTAMP(i)                                                                                  \
  do {                                                                                             \
    if (tid == 0 && kvh == 0 && hh == 0 && (split == 0 || is_new))                                 \
      g_hstamps[is_new ? 1 : 0][i] = __builtin_amdgcn_s_memrealtime();                             \
  } while (0)
// ... and of the first and the last o_proj workgroup of k_attn_oproj [0], [1] (scripts/dbg_attn_oproj_stamps.py)
__device__ unsigned long long g_ostamps[2][8];
// [split]: latest ticket-time of any attention workgroup of that key split; [15]: latest head-done signal
__device__ unsigned long long g_amax[16];
#define OSTAMP(i)                                                                                  \
  do {                                                                                             \
    if (tid == 0 && (t == 0 || t == p.ntiles - 1)) g_ostamps[t ? 1 : 0][i] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#else
#define HSTAMP(i)
#define OSTAMP(i)
#endif

template <int QT, int NW>
struct HeadLds {
  static_assert(NW * 4 >= QT * 16 && NW * 8192 >= 32768, "q rows: 4 per wave; new K / V: two 32-row tiles each");
  static constexpr int kVPriv = NW * 8192;           // wave-private V tiles (old splits) | new K, new V (new split)
  static constexpr int kQ = kVPriv;                  // q rows, swizzled like K: QT * 4 KB
  static constexpr int kLoop = kVPriv + QT * 4096;
  // after the loop: NW waves x QT x [16][kRow] fp32, rows padded 128 -> 132 floats: the 16 query rows of a wave's
  // ds_write_b128 (and of the merge's ds_read_b128) then fall on different banks (unpadded: 8-way conflicts,
  // 2.3 us of the stage)
  static constexpr int kRow = 132;
  static constexpr int kMergeO = 0;
  static constexpr int kMergeML = NW * QT * 16 * kRow * 4;  // NW waves x QT x [16][2] fp32
  static constexpr int kMerge = kMergeML + NW * QT * 128;
  static constexpr int kRaw = kLoop > kMerge ? kLoop : kMerge;
  // 8 waves: > 80 KB, one workgroup per CU, the geometry the sc1 hand-off is measured for
  static constexpr int kBytes = NW < 8 ? kRaw : (kRaw > 84 * 1024 ? kRaw : 84 * 1024);
};

// The stage as a device function of an NW-wave workgroup: k_attn_head runs it alone on 8 waves; k_attn_oproj runs it on 4,
// beside the o_proj workgroups that wait for it (SIGNAL: the workgroup that writes a head's final output stores it
// write-through and then counts the head on *done_ctr).  (kvh, by, cand) = blockIdx.x / .y / .z of k_attn_head:
// cand = candidate of a multi-candidate verify / request of a ragged batch (0 otherwise).
// HP (with QT = 2): the two 16-row "tiles" are not two query tiles of one head but the same <= 16 rows of TWO query heads
// of the kv group (head, head + 1): every K/V tile a wave fetches serves both.  Long prefixes (the host switches at
// ~5k keys): the G heads of a kv group otherwise pull the same K/V through their XCD's L2 G times (S = 8192: 134 MB of
// L2 reads per launch for 33.5 MB of cache, PMC: HBM fetch 34 MB), and with half the workgroups per split there are
// twice the splits.
// Args = HeadAttnArgs8 (KV8, attn_head_kv8.hip): the cache holds e4m3 codes and per-row scales; every key the stage sees
// is exactly code * scale (an exact bf16), so the result is the bf16 stage's on the dequantised cache:
//   * a key row is 128 B: a lane takes 16 consecutive d of its key per load (two loads per row, where bf16 needs four)
//     and feeds the word's two 8-byte halves to two MFMA k-steps (w8_frag: v_cvt_scalef32_pk_bf16_fp8 at scale 1).  The
//     contraction order over d is free: k-step s = 2h + e covers d = 64h + 16g + 8e .. +8 of lane group g, and the Q
//     B-fragments are read from LDS in the same order (qchunk);
//   * the scales meet the SCALARS: the fp32 score of key j is multiplied by k_scale[j] in front of scale_log2, p_j by
//     v_scale[j] in front of its bf16 rounding — both exact for powers of two.  A lane's 8 keys of a tile (u*16 + 4g + r)
//     are two 16-byte scale loads per tensor, unconditional and clamped like the tile loads; what they read past S is
//     SELECTED away, never multiplied (it may be anything, being written by this launch's new-row split);
//   * the wave-private V tile holds the 4 KB of codes as loaded (4 loads and 4 ds_write_b128 per lane and tile instead
//     of 8 and 8); ONE ds_read_b64_tr_b8 per 16 columns brings a lane the codes of its 8 keys, converted in registers in
//     front of the MFMA.  -DDFL_KV8_V_CODES=0 builds the other candidate — codes converted on the way into a bf16 tile,
//     read with ds_read_b64_tr_b16 as the bf16 stage does — which measured 2 - 5 % slower;
//   * the new-row split quantises each row after norm + RoPE (kv8_quant_row), attends over the DEQUANTISED rows in its
//     LDS tiles, and its hh == 0 workgroup writes codes and scales to the cache.
// No context rows, candidates, head pairs or fp32 partials in this form (the host function admits none).
template <int QT, int NW, bool SIGNAL, bool HP = false, bool XF32 = false, class Args = HeadAttnArgs>
__device__ __forceinline__ void attn_head_body(const Args &a, char *lds, int *s_last_p, const int kvh, const int by,
                                               const int cand, int *done_ctr) {
  constexpr bool KV8 = std::is_same<Args, HeadAttnArgs8>::value;
  constexpr bool VCODES = KV8 && DFL_KV8_V_CODES != 0;
  static_assert(!HP || QT == 2, "head pairs use the two-tile register layout");
  static_assert(!KV8 || (!HP && !XF32 && !SIGNAL), "the e4m3 cache: the plain one- and two-tile kernels only");
  using L = HeadLds<QT, NW>;
  int &s_last = *s_last_p;

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
  const int hpg = HP ? a.G >> 1 : a.G;  // workgroups per kv head and split
  const int hh = by % hpg, split = by / hpg;
  const int head = kvh * a.G + (HP ? 2 * hh : hh);
  const int ns = a.ns_old + 1;
  const bool is_new = split == a.ns_old;
  int S = a.S, tau = a.tau, bs = a.bs, pos0 = a.pos0;
  if (a.dyn) {
    const int32_t *dp = a.dyn + cand * a.dyn_cand_stride;
    S = dp[DFL_DYN_S];
    tau = dp[DFL_DYN_TAU];
    bs = dp[DFL_DYN_BS];
    pos0 = dp[DFL_DYN_POS0];
  }
  if constexpr (KV8) tau = 0;  // (no context rows in this form, whatever the record says)
  const int n_new = tau + bs;  // <= 64
  const int qi = l & 15, g = l >> 4;
  HSTAMP(0);
  // per-candidate / per-request views as plain locals: the argument block stays untouched
  const bf16_t *const xq = XF32 ? a.cos_tab : a.xq + cand * a.xq_cand_stride;  // (XF32: only the dummy loads' safe address)
  const float *const xq32 = XF32 ? a.xq32 + cand * a.xq_cand_stride : nullptr;
  bf16x8 *const out_frag = a.out_frag + cand * a.out_cand_stride;
  float *const o_part = a.o_part + cand * a.ws_cand_stride;
  float *const ml_part = a.ml_part + cand * a.ws_cand_stride;
  int *const tickets = a.tickets + cand * a.ws_cand_stride;
  bf16_t *const kc = a.kc + cand * a.cache_cand_stride, *const vc = a.vc + cand * a.cache_cand_stride;
  bf16_t *const k_new = a.k_out ? a.k_out + cand * a.kv_out_cand_stride : kc;
  bf16_t *const v_new = a.k_out ? a.v_out + cand * a.kv_out_cand_stride : vc;
  const int new_rows_cap = a.k_out ? a.out_rows : a.cache_rows;
  const int new_row0 = a.k_out ? 0 : S;
  const bf16_t *kbase = kc + (int64_t)kvh * a.cache_rows * 128;
  const bf16_t *vbase = vc + (int64_t)kvh * a.cache_rows * 128;


  // ---- old-key tiles of this split; wave w walks t0 + w, t0 + w + NW, ...
  int t0 = 0, t1 = 0;
  if (!is_new && a.ns_old > 0) {
    const int nt = (S + 31) >> 5;
    const int tps = (nt + a.ns_old - 1) / a.ns_old;
    t0 = split * tps;
    t1 = t0 + tps;
    t0 = t0 > nt ? nt : t0;
    t1 = t1 > nt ? nt : t1;
  }
  const int old_last = S > 0 ? S - 1 : 0;
  // KV8: the raw 16-byte code words stay in flight as they are — half the registers — beside the tile's scales
  // (sc[0..1]: k_scale of the lane's keys u*16 + 4g + r, sc[2..3]: v_scale of the same keys)
  constexpr int KF = KV8 ? 2 : 4, VF = KV8 ? 4 : 8, SF = KV8 ? 4 : 1;
  bf16x8 kA[2][KF], vA[VF], kB[2][KF], vB[VF];
  f32x4 sA[SF], sB[SF];
  // Q chunk (8 d) that k-step s of lane group g contracts: bf16 d = 32s + 8g; KV8 d = 64 (s >> 1) + 16g + 8 (s & 1)
  auto qchunk = [&](int s) { return KV8 ? 8 * (s >> 1) + 2 * g + (s & 1) : s * 4 + g; };
  // all loads of a tile are unconditional with clamped rows (they batch; rows >= S are masked
  // below and never touch memory another workgroup writes in this launch)
  // (lim = old_last: a real tile; lim = 0: a DUMMY fetch — every lane reads row 0, one or two cache lines per
  // instruction, already in L1/L2 — issued where the loops below have nothing left to prefetch, see there)
  // (KV8: the four scales of keys r4 .. r4 + 3, r4 clamped to the group of four that holds row lim — cache_rows % 4 == 0)
  auto fetch_sc = [&](f32x4(&sc)[SF], int half, int t, int lim) {
    if constexpr (KV8) {
      const float *sb = (half ? a.v_scale : a.k_scale) + (int64_t)kvh * a.cache_rows;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        int r4 = t * 32 + u * 16 + 4 * g;
        r4 = r4 < (lim & ~3) ? r4 : (lim & ~3);
        sc[2 * half + u] = *reinterpret_cast<const f32x4 *>(sb + r4);
      }
    }
  };
  auto fetch_k = [&](bf16x8(&kf)[2][KF], f32x4(&sc)[SF], int t, int lim) {
    fetch_sc(sc, 0, t, lim);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      int row = t * 32 + u * 16 + qi;
      row = row < lim ? row : lim;
#pragma unroll
      for (int s = 0; s < KF; ++s) {
        if constexpr (KV8)
          kf[u][s] = *reinterpret_cast<const bf16x8 *>(reinterpret_cast<const char *>(a.kc) +
                                                       ((int64_t)kvh * a.cache_rows + row) * 128 + s * 64 + g * 16);
        else
          kf[u][s] = *reinterpret_cast<const bf16x8 *>(kbase + (int64_t)row * 128 + s * 32 + g * 8);
      }
    }
  };
  auto fetch_v = [&](bf16x8(&vr)[VF], f32x4(&sc)[SF], int t, int lim) {
    fetch_sc(sc, 1, t, lim);
#pragma unroll
    for (int i = 0; i < VF; ++i) {
      const int c = l + 64 * i;
      if constexpr (KV8) {  // 8 words of 16 codes per row
        int row = t * 32 + (c >> 3);
        row = row < lim ? row : lim;
        vr[i] = *reinterpret_cast<const bf16x8 *>(reinterpret_cast<const char *>(a.vc) +
                                                  ((int64_t)kvh * a.cache_rows + row) * 128 + (c & 7) * 16);
      } else {
        int row = t * 32 + (c >> 4);
        row = row < lim ? row : lim;
        vr[i] = *reinterpret_cast<const bf16x8 *>(vbase + (int64_t)row * 128 + (c & 15) * 8);
      }
    }
  };
  auto fetch = [&](bf16x8(&kf)[2][KF], bf16x8(&vr)[VF], f32x4(&sc)[SF], int t, int lim) {
    fetch_k(kf, sc, t, lim);
    fetch_v(vr, sc, t, lim);
  };
  // ---- q rows of this head: QT*16 items, 4 per wave (waves 0 .. 4*QT-1), written swizzled like a K tile.
  // Their loads go out first, the first K/V tile's behind them (vmcnt is in order), the arithmetic after both.
  char *q_lds = lds + L::kQ;
  const int jq = 4 * w + g;  // this 16-lane group's q item (QT = 1: waves 0..3 hold rows, the others a dummy)
  const int jrow = HP ? jq & 15 : jq;            // its block row ...
  const int jhead = HP ? head + (jq >> 4) : head;  // ... and query head
  RopeLoads<1> qld;
  {
    const int pos[1] = {pos0 + tau + jrow};
    if constexpr (XF32) {
      const float *src[1] = {jrow < bs ? xq32 + (int64_t)jrow * a.ldq + a.q_col + jhead * 128 : nullptr};
      rope_issue32<1>(src, pos, a.q_w, a.cos_tab, a.sin_tab, a.max_pos, xq32, xq, a.part_stride32, a.nparts32, l, qld);
    } else {
      const bf16_t *src[1] = {jrow < bs ? xq + (int64_t)jrow * a.ldq + a.q_col + jhead * 128 : nullptr};
      rope_issue<1>(src, pos, a.q_w, a.cos_tab, a.sin_tab, a.max_pos, xq, l, qld);
    }
  }
  // (compiler fences: without them hipcc hoists the K/V burst above the q loads and sinks the norm-weight load
  // into a branch of the arithmetic, and the q rows wait for the whole burst after all)
  asm volatile("" ::: "memory");
  auto finish_q = [&]() {
    if (jq < QT * 16) {
      const bool rp[1] = {true};
      bf16x8 ov[1];
      if constexpr (XF32) rope_sum32<1>(qld, a.nparts32);
      rope_finish<1>(qld, rp, a.q_w != nullptr, a.eps, l, ov);
      const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      *reinterpret_cast<bf16x8 *>(q_lds + (jq >> 4) * 4096 + k_swz(jq & 15, qi)) = jrow < bs ? ov[0] : z;
    }
  };
  int tcur = t0 + w;
  char *new_k = lds, *new_v = lds + 16384;  // up to two 32-row tiles each
  if (!is_new) {
    // the first tile's loads are issued by EVERY wave of an old split, with or without a tile (clamped rows of
    // valid cache memory): under a per-wave branch the compiler loses count of what is in flight and makes the q
    // arithmetic wait for the whole K/V burst instead of for its own four loads
    fetch(kA, vA, sA, tcur < t1 ? tcur : 0, old_last);
    asm volatile("" ::: "memory");
    finish_q();
  } else {
    // ---- new split: this cycle's K / V rows of the kv head -> LDS tiles (and the cache, hh == 0).  Its loads go
    // out right behind the q loads (no K/V tile burst in this workgroup), then q, then the rows.
    auto sweep = [&](auto np_tag) {
      constexpr int NP = decltype(np_tag)::value;
      const bf16_t *src[NP];
      const float *src32[NP];
      int pos[NP], rel[NP];
      bool rp[NP], isv[NP];
      bf16x8 ov[NP];
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int it = (p * NW + w) * 4 + g;  // 4 NW items per pass
        isv[p] = it >= n_new;
        rel[p] = isv[p] ? it - n_new : it;
        const bool ok = it < 2 * n_new;
        // (arithmetic, not a select between two argument FIELDS: hipcc turns such a select into a select of their
        // addresses plus a per-lane global load with vmcnt(0) — four dependent round trips in this prologue)
        const int vsel = isv[p] ? 1 : 0;
        if constexpr (XF32) {  // (no context rows in this form: the host admits tau == 0 only)
          src32[p] = ok ? xq32 + (int64_t)rel[p] * a.ldq + a.k_col + vsel * (a.v_col - a.k_col) + kvh * 128 : nullptr;
          src[p] = ok ? xq : nullptr;   // presence flag for the stores below
        } else {
          const bf16_t *row = rel[p] < tau ? a.xc + (int64_t)rel[p] * a.ldc + a.ck_col + vsel * (a.cv_col - a.ck_col)
                                           : xq + (int64_t)(rel[p] - tau) * a.ldq + a.k_col + vsel * (a.v_col - a.k_col);
          src[p] = ok ? row + kvh * 128 : nullptr;
          src32[p] = nullptr;
        }
        pos[p] = pos0 + rel[p];
        rp[p] = !isv[p];
      }
      RopeLoads<NP> kld;
      if constexpr (XF32)
        rope_issue32<NP>(src32, pos, a.k_w, a.cos_tab, a.sin_tab, a.max_pos, xq32, xq, a.part_stride32, a.nparts32, l, kld);
      else
        rope_issue<NP>(src, pos, a.k_w, a.cos_tab, a.sin_tab, a.max_pos, xq, l, kld);
      asm volatile("" ::: "memory");
      finish_q();
      if constexpr (XF32) rope_sum32<NP>(kld, a.nparts32);
      rope_finish<NP>(kld, rp, a.k_w != nullptr, a.eps, l, ov);
      float qs[NP];
      kv8_codes qc[NP];
      if constexpr (KV8) {  // every item, present or not: the row maximum is a cross-lane step
#pragma unroll
        for (int p = 0; p < NP; ++p) kv8_quant_row(ov[p], qs[p], qc[p], ov[p]);
      }
#pragma unroll
      for (int p = 0; p < NP; ++p)
        if (src[p]) {
          const int jt = rel[p] >> 5, r = rel[p] & 31;
          *reinterpret_cast<bf16x8 *>((isv[p] ? new_v + jt * 8192 + v_swz(r, qi) : new_k + jt * 8192 + k_swz(r, qi))) = ov[p];
          const int crow = new_row0 + rel[p];
          if constexpr (KV8) {
            if (hh == 0 && crow < a.cache_rows) {
              const int64_t at = (int64_t)kvh * a.cache_rows + crow;
              *reinterpret_cast<kv8_codes *>(reinterpret_cast<char *>(isv[p] ? a.vc : a.kc) + at * 128 + qi * 8) = qc[p];
              if (qi == 0) (isv[p] ? a.v_scale : a.k_scale)[at] = qs[p];
            }
          } else if (hh == 0 && crow < new_rows_cap)
            *reinterpret_cast<bf16x8 *>((isv[p] ? v_new : k_new) + ((int64_t)kvh * new_rows_cap + crow) * 128 + qi * 8) = ov[p];
        }
    };
    if (2 * n_new <= NW * 4)
      sweep(std::integral_constant<int, 1>{});
    else if (2 * n_new <= NW * 8)
      sweep(std::integral_constant<int, 2>{});
    else  // (the host function of a 4-wave launch admits tau + bs <= 32)
      sweep(std::integral_constant<int, 4>{});
  }
  HSTAMP(1);
  __syncthreads();

  // Q^T B-fragments: lane (q = l&15, g) holds Q[q][32 s + 8 g .. +8]
  bf16x8 qf[QT][4];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt)
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[qt][s] = *reinterpret_cast<const bf16x8 *>(q_lds + qt * 4096 + k_swz(qi, qchunk(s)));

  f32x4 o[QT][8];
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m_run[qt] = -INFINITY;
    l_run[qt] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) o[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  // one 32-key tile: K fragments in registers, V tile (swizzled rows) at vt in LDS.
  // key0 = index of the tile's first key in its own numbering (old: cache row; new: rel);
  // nvalid = keys of that numbering that exist; vrows = rows of the V tile holding real data.
  // kfrag(u, s): the K A-fragment of k-step s (registers as loaded, converted codes, or the new rows' LDS tile);
  // sc (KV8): the tile's scales, see above — the new rows sit in LDS dequantised, their scales here are 1
  auto compute = [&](auto kfrag, const f32x4(&sc8)[SF], const char *vt, int key0, int nvalid, int vrows, bool new_rows) {
    const int qq = qi >> 2, p4 = l & 3;
    int r0 = 4 * g + qq, r1 = 16 + 4 * g + qq;
    // (VCODES: lane i of a 16-lane group addresses 8 bytes of row i >> 1 of the group's 8 keys u*16 + 4g + r)
    const int rc = 4 * g + ((qi >> 1) & 3) + 16 * (qi >> 3);
    r0 = r0 < vrows ? r0 : vrows - 1;  // rows past the data hold stale LDS bytes: P is 0 there, but 0 x NaN is not
    r1 = r1 < vrows ? r1 : vrows - 1;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      f32x4 sc[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        sc[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s) sc[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kfrag(u, s), qf[qt][s], sc[u], 0, 0, 0);
      }
      // lane (q, g): sc[u][r] is key key0 + u*16 + 4g + r
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = key0 + u * 16 + 4 * g + r;
          // causal (target verify): query row j sees new row rel <= tau + j; cached rows always
          const bool vis = key < nvalid && (!new_rows || !a.causal || key <= tau + (HP ? 0 : qt * 16) + qi);
          float ks = 1.f;  // (KV8: exact, then the bf16 stage's rounding)
          if constexpr (KV8) ks = sc8[u][r];
          const float v = vis ? (KV8 ? sc[u][r] * ks : sc[u][r]) * a.scale_log2 : -INFINITY;
          sc[u][r] = v;
          mx = fmaxf(mx, v);
        }
      mx = wave_g_max(mx);
      const float m_new = fmaxf(m_run[qt], mx);
      const float m_ref = m_new == -INFINITY ? 0.f : m_new;
      const float alpha = __builtin_amdgcn_exp2f(m_run[qt] - m_ref);
      m_run[qt] = m_new;
      float psum = 0.f;
      bf16x8 pb;
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = __builtin_amdgcn_exp2f(sc[u][r] - m_ref);
          psum += p;
          if constexpr (KV8)  // (a key past nvalid: p is 0, its scale may be anything)
            pb[u * 4 + r] = f2bf(key0 + u * 16 + 4 * g + r < nvalid ? p * sc8[2 + u][r] : 0.f);
          else
            pb[u * 4 + r] = f2bf(p);
        }
      l_run[qt] = l_run[qt] * alpha + psum;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) o[qt][dt] *= alpha;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) {
        if constexpr (VCODES) {
          if (!new_rows) {  // the tile holds codes: ONE transposed read brings the lane's 8 keys of column 16 dt + qi
            const u32x2 q = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr8_b64_v2i32(
                (lds_i32x2 *)(vt + rc * 128 + (((dt ^ (rc & 7)) << 4) | ((qi & 1) << 3)))));
            const bf16x2 a0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[0], 1.0f, false);
            const bf16x2 a1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[0], 1.0f, true);
            const bf16x2 a2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[1], 1.0f, false);
            const bf16x2 a3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(q[1], 1.0f, true);
            const bf16x8 vq = {a0[0], a0[1], a1[0], a1[1], a2[0], a2[1], a3[0], a3[1]};
            o[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vq, pb, o[qt][dt], 0, 0, 0);
            continue;
          }
        }
        const bf16x4 v0 =
            __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(vt + r0 * 256 + (((dt ^ (r0 & 7)) << 5) | (p4 << 3))));
        const bf16x4 v1 =
            __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4 *)(vt + r1 * 256 + (((dt ^ (r1 & 7)) << 5) | (p4 << 3))));
        const bf16x8 va = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        o[qt][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(va, pb, o[qt][dt], 0, 0, 0);
      }
    }
  };

  if (is_new) {
    const int ntile = (n_new + 31) >> 5;  // 1 or 2
    if (w < ntile) {
      bf16x8 kf[2][4];
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int s = 0; s < 4; ++s)
          kf[u][s] = *reinterpret_cast<const bf16x8 *>(new_k + w * 8192 + k_swz(u * 16 + qi, qchunk(s)));
      int vrows = n_new - w * 32;
      vrows = vrows > 32 ? 32 : vrows;
      f32x4 ones[SF];
#pragma unroll
      for (int i = 0; i < SF; ++i) ones[i] = (f32x4){1.f, 1.f, 1.f, 1.f};
      compute([&](int u, int s) { return kf[u][s]; }, ones, new_v + w * 8192, w * 32, n_new, vrows, true);
    }
  } else {
    char *my_v = lds + w * 8192;
    auto put_v = [&](const bf16x8(&vr)[VF]) {
#pragma unroll
      for (int i = 0; i < VF; ++i) {
        const int c = l + 64 * i;
        if constexpr (VCODES) {  // the word as it is: 4 KB of codes per tile, 16-byte chunks swizzled by the row
          *reinterpret_cast<bf16x8 *>(my_v + (c >> 3) * 128 + (((c & 7) ^ ((c >> 3) & 7)) << 4)) = vr[i];
        } else if constexpr (KV8) {  // 16 codes -> chunks 2 (c & 7) and 2 (c & 7) + 1 of the row: 32 contiguous bytes of the tile
          *reinterpret_cast<bf16x8 *>(my_v + v_swz(c >> 3, 2 * (c & 7))) = w8_frag(vr[i], 0);
          *reinterpret_cast<bf16x8 *>(my_v + v_swz(c >> 3, 2 * (c & 7) + 1)) = w8_frag(vr[i], 1);
        } else {
          *reinterpret_cast<bf16x8 *>(my_v + v_swz(c >> 4, c & 15)) = vr[i];
        }
      }
    };
    // a tile's K registers as MFMA A-fragments
    auto frag_of = [&](const bf16x8(&kf)[2][KF]) {
      return [&kf](int u, int s) {
        if constexpr (KV8)
          return w8_frag(kf[u][s >> 1], s & 1);
        else
          return kf[u][s];
      };
    };
    // the wave's own LDS tile: its ds_write -> ds_read order is program order (lgkmcnt), no barrier
    // A wave with ONE tile (S ~ 1k: every wave) just computes it.  A wave with several walks them with the next tile
    // in flight, and there every fetch is UNCONDITIONAL: behind a conditional fetch hipcc cannot count the loads in
    // flight and waits vmcnt(0) before the next ds_write / MFMA, i.e. for the tile it has just requested — one full
    // memory round trip per tile (2.9 us per tile at S = 8192, where a wave walks six).  Where nothing is left to
    // prefetch the fetch degenerates to a dummy (lim = 0).
    if (tcur + NW >= t1) {
      if (tcur < t1) {
        put_v(vA);
        compute(frag_of(kA), sA, my_v, tcur * 32, S, 32, false);
      }
    } else if (QT == 1) {
      for (; tcur < t1; tcur += 2 * NW) {
        fetch(kB, vB, sB, tcur + NW, tcur + NW < t1 ? old_last : 0);
        put_v(vA);
        compute(frag_of(kA), sA, my_v, tcur * 32, S, 32, false);
        fetch(kA, vA, sA, tcur + 2 * NW, tcur + 2 * NW < t1 ? old_last : 0);
        if (tcur + NW < t1) {
          put_v(vB);
          compute(frag_of(kB), sB, my_v, (tcur + NW) * 32, S, 32, false);
        }
      }
    } else {
      // two query tiles / a head pair: 64 accumulator + 32 q registers more, no room for a second K/V tile in flight
      // (a head pair with K double-buffered and its q fragments re-read from LDS sat at 254 VGPRs and ran SLOWER:
      // 4.98 against 4.68 ms per cycle at S = 8192).  (First form of the two-tile kernel: hipcc spilled
      // each V fragment right behind its load: eight serial round trips per tile.)  K of the next tile is requested
      // once the current one's QK^T is done with it, V once it sits in LDS
      for (; tcur < t1; tcur += NW) {
        const int lim = tcur + NW < t1 ? old_last : 0;
        // (KV8: compute reads this tile's v scales after the next tile's are requested: a copy keeps them)
        f32x4 sC[SF];
#pragma unroll
        for (int i = 0; i < SF; ++i) sC[i] = sA[i];
        put_v(vA);
        fetch_v(vA, sA, tcur + NW, lim);
        compute(frag_of(kA), sC, my_v, tcur * 32, S, 32, false);
        fetch_k(kA, sA, tcur + NW, lim);
      }
    }
  }

  // ---- the NW waves meet in LDS
  HSTAMP(2);
  __syncthreads();
  HSTAMP(3);
  {
    float *mo = reinterpret_cast<float *>(lds + L::kMergeO);
    float *mml = reinterpret_cast<float *>(lds + L::kMergeML);
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const float lt = wave_g_sum(l_run[qt]);
      float *op = mo + ((w * QT + qt) * 16 + qi) * L::kRow;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) *reinterpret_cast<f32x4 *>(op + dt * 16 + 4 * g) = o[qt][dt];
      if (g == 0) {
        mml[((w * QT + qt) * 16 + qi) * 2] = m_run[qt];
        mml[((w * QT + qt) * 16 + qi) * 2 + 1] = lt;
      }
    }
  }
  __syncthreads();
  const bool has_item = tid < QT * 256;  // QT = 1 on 8 waves: the upper 4 have no item (they still join the barriers)
  const int qt = tid >> 8, q = (tid >> 4) & 15, dg = tid & 15;
  float M = -INFINITY, Lsum = 0.f, acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (has_item) {
    const float *mo = reinterpret_cast<const float *>(lds + L::kMergeO);
    const float *mml = reinterpret_cast<const float *>(lds + L::kMergeML);
    float ms[NW], ls[NW];
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
      ms[ww] = mml[((ww * QT + qt) * 16 + q) * 2];
      ls[ww] = mml[((ww * QT + qt) * 16 + q) * 2 + 1];
      M = fmaxf(M, ms[ww]);
    }
    const float mref = M == -INFINITY ? 0.f : M;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {  // fixed wave order: reproducible sums
      const float wgt = __builtin_amdgcn_exp2f(ms[ww] - mref);  // exp2(-inf) = 0: a wave without tiles
      const float *op = mo + ((ww * QT + qt) * 16 + q) * L::kRow + dg * 8;
      const f32x4 a0 = *reinterpret_cast<const f32x4 *>(op), a1 = *reinterpret_cast<const f32x4 *>(op + 4);
      Lsum += wgt * ls[ww];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        acc[j] += wgt * a0[j];
        acc[4 + j] += wgt * a1[j];
      }
    }
  }
  auto emit = [&](float Lt, const float(&v)[8]) {  // frag16 chunk (n>>3 = head*16 + dg, row q) of query tile qt
    const float inv = Lt > 0.f ? 1.f / Lt : 0.f;
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = f2bf(v[j] * inv);
    if (SIGNAL && q >= bs) r = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};  // the GEMM behind it takes rows >= bs as zero
    bf16x8 *dst = HP ? &out_frag[((head + qt) * 16 + dg) * 16 + q] : &out_frag[qt * a.out_tile_stride + (head * 16 + dg) * 16 + q];
    if (SIGNAL) {  // read by other workgroups of THIS launch: write-through
      const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(dst, 0, 16, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, r), rd, 0, 0, 16);
    } else {
      *dst = r;
    }
  };
  // SIGNAL: every storing wave drains, the workgroup meets, one lane counts the head as done (hand-off row 1 of the
  // table in MI355X_MICROARCH.md: sc1 stores, drain, barrier, agent-scope add; consumers poll, barrier, sc1 loads)
  auto signal = [&]() {
    if (SIGNAL) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      // one wave instruction, 32 lanes: +1 on each of the 32 replicas of the counter (a line of its own each), so that a
      // replica has 8 pollers, not 256
      if (tid < 32) __hip_atomic_fetch_add(done_ctr + tid * 32, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef DFL_ATTN_STAMPS
      if (tid == 0) atomicMax(&g_amax[15], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
    }
  };
  HSTAMP(4);
  if (ns == 1) {
    if (has_item) emit(Lsum, acc);
    signal();
    return;
  }

  // ---- publish the workgroup's partial write-through, drain, ticket; the head's last arriver merges
  const size_t item_row = HP ? (size_t)(head + qt) * 16 + q : (size_t)head * (QT * 16) + qt * 16 + q;
  const size_t rows_per_split = (size_t)a.n_q * (HP ? 16 : QT * 16);
  const __amdgpu_buffer_rsrc_t ro =
      __builtin_amdgcn_make_buffer_rsrc(o_part, 0, (int)(rows_per_split * ns * 128 * sizeof(float)), 0x00020000);
  const __amdgpu_buffer_rsrc_t rm =
      __builtin_amdgcn_make_buffer_rsrc(ml_part, 0, (int)(rows_per_split * ns * 2 * sizeof(float)), 0x00020000);
  if (has_item) {
    const int off = (int)((((size_t)split * rows_per_split + item_row) * 128 + dg * 8) * sizeof(float));
    const f32x4 s0 = {acc[0], acc[1], acc[2], acc[3]}, s1 = {acc[4], acc[5], acc[6], acc[7]};
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, s0), ro, off, 0, 16);  // sc1
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, s1), ro, off + 16, 0, 16);
    if (dg == 0) {
      const int offm = (int)((((size_t)split * rows_per_split + item_row) * 2) * sizeof(float));
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, M), rm, offm, 0, 16);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, Lsum), rm, offm + 4, 0, 16);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  HSTAMP(5);
  if (tid == 0) {
    const int ticket = __hip_atomic_fetch_add(&tickets[head], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = ticket == ns - 1;
    if (last) __hip_atomic_store(&tickets[head], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
    s_last = last;
  }
  __syncthreads();
  HSTAMP(6);
#ifdef DFL_ATTN_STAMPS
  if (tid == 0) atomicMax(&g_amax[split < 15 ? split : 14], (unsigned long long)__builtin_amdgcn_s_memrealtime());
#endif
  if (!s_last) return;

  // every load of the handed-off bytes is an sc1 load (L2-served): no acquire needed
  if (has_item) {
    float Mg = -INFINITY, Lg = 0.f, ag[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) ag[j] = 0.f;
    constexpr int U = 8;  // at 1k keys ns = 5 or 6: one round trip
    for (int s = 0; s < ns; s += U) {
      float ms[U], ls[U];
      f32x4 a0[U], a1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int sc = s + u < ns ? s + u : ns - 1;
        const int off = (int)((((size_t)sc * rows_per_split + item_row) * 128 + dg * 8) * sizeof(float));
        const int offm = (int)((((size_t)sc * rows_per_split + item_row) * 2) * sizeof(float));
        ms[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, offm, 0, 16));
        ls[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rm, offm + 4, 0, 16));
        a0[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ro, off, 0, 16));
        a1[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ro, off + 16, 0, 16));
      }
      float mnew = Mg;
#pragma unroll
      for (int u = 0; u < U; ++u) mnew = fmaxf(mnew, s + u < ns ? ms[u] : -INFINITY);
      const float mref = mnew == -INFINITY ? 0.f : mnew;
      const float scale = __builtin_amdgcn_exp2f(Mg - mref);
      Mg = mnew;
      Lg *= scale;
#pragma unroll
      for (int j = 0; j < 8; ++j) ag[j] *= scale;
#pragma unroll
      for (int u = 0; u < U; ++u) {  // fixed split order
        const float wgt = s + u < ns ? __builtin_amdgcn_exp2f(ms[u] - mref) : 0.f;
        Lg += wgt * ls[u];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          ag[j] += wgt * a0[u][j];
          ag[4 + j] += wgt * a1[u][j];
        }
      }
    }
    emit(Lg, ag);
  }
  signal();
#ifdef DFL_ATTN_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  HSTAMP(7);
}

// ---- host side: the old-key splits of a launch (attn_head.hip, attn_head_kv8.hip) ----
// The measured choice.  The head and o_proj pairs are swept at compile time by scripts/dbg_attn_head_stamps.py /
// dbg_attn_oproj_stamps.py (-DDFL_ATTN_HEAD_TILES=... etc.).
#ifndef DFL_ATTN_HEAD_TILES
#define DFL_ATTN_HEAD_TILES 8  // 32-key tiles per split: a workgroup's 8 waves take one each per round
#endif
#ifndef DFL_ATTN_HEAD_WGS
#define DFL_ATTN_HEAD_WGS 224  // workgroups per launch beyond which the splits grow instead
#endif
// nt tiles at `tiles` per split, at most wgs / heads_x_blocks - 1 of them (the new rows are a split of their own)
inline int head_old_splits(int nt, int tiles, int wgs, int heads_x_blocks) {
  const int ns = (nt + tiles - 1) / tiles;
  int budget = wgs / heads_x_blocks - 1;
  budget = budget < 1 ? 1 : budget;
  return ns > budget ? budget : ns;
}

}  // namespace
