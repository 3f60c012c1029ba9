// The target's KV cache as OCP e4m3 codes: uint8 [kv head][rows][128] for K and for V, one
// power-of-two fp32 scale per (row, kv head) beside each — 264 bytes per row and head instead of 512.
//   dfl_attn_head_kv8   the single-request attention stage (attn_head.h: attn_head_body on HeadAttnArgs8) over such a cache:
//                       causal or not, no context rows, blocks of <= 16 rows (one query tile) or 17..32 (two); grid, key
//                       splits, ticket and merge as dfl_attn_head, same workspace.  Every key it sees is code * scale.
//   dfl_kv_quant_rows   the prefill's way into the cache: one layer's bf16 K and V rows -> codes + scales, and the
//                       dequantised values back in place, so that the prefill's attention sees what the verify will.
#include "attn_head.h"


namespace {

template <int QT>
__global__ __launch_bounds__(512) void k_attn_head_kv8(HeadAttnArgs8 a) {
  __shared__ __attribute__((aligned(16))) char lds[HeadLds<QT, 8>::kBytes];
  __shared__ int s_last;
  attn_head_body<QT, 8, false, false, false, HeadAttnArgs8>(a, lds, &s_last, blockIdx.x, blockIdx.y, 0, nullptr);
}

// One 16-lane group per item (tensor, kv head, row): lane c holds elements 8c .. 8c+7.  256 threads = 16 items.
__global__ __launch_bounds__(256) void k_kv_quant_rows(bf16_t *k_rows, bf16_t *v_rows, int src_rows, int P, int n_kv,
                                                       uint8_t *kc, uint8_t *vc, float *k_scale, float *v_scale, int cache_rows,
                                                       int row0) {
  const int item = blockIdx.x * 16 + (threadIdx.x >> 4), c = threadIdx.x & 15;
  const int n = 2 * n_kv * P;
  const int it = item < n ? item : n - 1;  // (a group past the end repeats the last item: the row maximum is cross-lane)
  const int isv = it / (n_kv * P), kvh = (it / P) % n_kv, r = it % P;
  bf16_t *src = (isv ? v_rows : k_rows) + ((int64_t)kvh * src_rows + r) * 128 + c * 8;
  float scale;
  kv8_codes codes;
  bf16x8 deq;
  kv8_quant_row(*reinterpret_cast<const bf16x8 *>(src), scale, codes, deq);
  if (item >= n) return;
  const int64_t at = (int64_t)kvh * cache_rows + row0 + r;
  *reinterpret_cast<kv8_codes *>((isv ? vc : kc) + at * 128 + c * 8) = codes;
  if (c == 0) (isv ? v_scale : k_scale)[at] = scale;
  *reinterpret_cast<bf16x8 *>(src) = deq;
}

}  // namespace

extern "C" int dfl_attn_head_kv8(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, int n_q, int n_kv,
                                 const void *q_norm_w, const void *k_norm_w, float eps, const void *cos_tab,
                                 const void *sin_tab, int max_pos, void *kcodes, void *vcodes, float *k_scale, float *v_scale,
                                 int cache_rows, float scale, int causal, const int32_t *dyn, int S, int bs, int pos0,
                                 int q_tiles, void *ws, int max_splits, void *out_frag, int64_t out_tile_stride, void *stream) {
  DFL_REQUIRE(xq && cos_tab && sin_tab && kcodes && vcodes && k_scale && v_scale && out_frag && ws,
              "dfl_attn_head_kv8: null pointer");
  DFL_REQUIRE((q_norm_w == nullptr) == (k_norm_w == nullptr), "dfl_attn_head_kv8: give both norm weights or neither");
  DFL_REQUIRE(n_q > 0 && n_kv > 0 && n_q % n_kv == 0, "dfl_attn_head_kv8: bad head counts (n_q=%d n_kv=%d)", n_q, n_kv);
  DFL_REQUIRE(q_tiles == 1 || q_tiles == 2, "dfl_attn_head_kv8: q_tiles must be 1 or 2");
  DFL_REQUIRE(ldq > 0 && ldq % 8 == 0 && q_col >= 0 && k_col >= 0 && v_col >= 0 && q_col % 8 == 0 && k_col % 8 == 0 &&
                  v_col % 8 == 0 && max_pos > 0,
              "dfl_attn_head_kv8: bad block-row layout");
  DFL_REQUIRE(S >= 0 && bs >= 1 && bs <= 16 * q_tiles, "dfl_attn_head_kv8: lengths S=%d bs=%d outside the kernel's range (q_tiles=%d)",
              S, bs, q_tiles);
  // (the scale loads are 16-byte loads of four consecutive rows: every kv head's scale row must start on one)
  DFL_REQUIRE(cache_rows % 4 == 0 && ((uintptr_t)k_scale & 15) == 0 && ((uintptr_t)v_scale & 15) == 0 &&
                  ((uintptr_t)kcodes & 15) == 0 && ((uintptr_t)vcodes & 15) == 0,
              "dfl_attn_head_kv8: cache_rows = %d must be a multiple of 4, codes and scales 16-byte aligned", cache_rows);
  DFL_REQUIRE(S + bs <= cache_rows, "dfl_attn_head_kv8: S + bs = %d exceeds cache_rows = %d", S + bs, cache_rows);
  DFL_REQUIRE(max_splits >= 2 || (S == 0 && !dyn), "dfl_attn_head_kv8: cached keys need a split of their own (max_splits >= 2)");
  DFL_REQUIRE(max_splits >= 1 && out_tile_stride >= 0 && out_tile_stride % 8 == 0,
              "dfl_attn_head_kv8: bad max_splits / out_tile_stride");
  // the old-key splits of dfl_attn_head's plain kernels (no head pairs in this form)
  const int nt = (S + 31) / 32;
  int ns_old = head_old_splits(nt, DFL_ATTN_HEAD_TILES, DFL_ATTN_HEAD_WGS, n_q);
  ns_old = ns_old > max_splits - 1 ? max_splits - 1 : ns_old;
  if (nt == 0 && !dyn) ns_old = 0;
  HeadAttnArgs8 a{};
  a.xq = (const bf16_t *)xq;
  a.ldq = ldq;
  a.q_col = q_col, a.k_col = k_col, a.v_col = v_col;
  a.q_w = (const bf16_t *)q_norm_w, a.k_w = (const bf16_t *)k_norm_w;
  a.eps = eps;
  a.cos_tab = (const bf16_t *)cos_tab, a.sin_tab = (const bf16_t *)sin_tab;
  a.max_pos = max_pos;
  a.kc = (bf16_t *)kcodes, a.vc = (bf16_t *)vcodes;
  a.k_scale = k_scale, a.v_scale = v_scale;
  a.cache_rows = cache_rows;
  a.n_q = n_q, a.n_kv = n_kv, a.G = n_q / n_kv;
  a.scale_log2 = scale * 1.4426950408889634f;
  a.causal = causal ? 1 : 0;
  a.dyn = dyn;
  a.S = S, a.tau = 0, a.bs = bs, a.pos0 = pos0;
  a.out_frag = (bf16x8 *)out_frag;
  a.out_tile_stride = out_tile_stride / 8;
  const int64_t rows = (int64_t)max_splits * n_q * q_tiles * 16;
  a.o_part = (float *)ws;
  a.ml_part = (float *)ws + rows * 128;
  a.tickets = (int *)((float *)ws + rows * 130);
  a.ns_old = ns_old;
  const dim3 grid(n_kv, a.G * (ns_old + 1), 1);
  if (q_tiles == 1)
    hipLaunchKernelGGL(k_attn_head_kv8<1>, grid, dim3(512), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_attn_head_kv8<2>, grid, dim3(512), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH("dfl_attn_head_kv8");
  return DFL_OK;
}

extern "C" int dfl_kv_quant_rows(void *k_rows, void *v_rows, int src_rows, int P, int n_kv, void *kcodes, void *vcodes,
                                 float *k_scale, float *v_scale, int cache_rows, int row0, void *stream) {
  DFL_REQUIRE(k_rows && v_rows && kcodes && vcodes && k_scale && v_scale, "dfl_kv_quant_rows: null pointer");
  DFL_REQUIRE(n_kv > 0 && P >= 0 && P <= src_rows && row0 >= 0 && row0 + P <= cache_rows,
              "dfl_kv_quant_rows: rows [%d, %d) of %d source rows do not fit cache_rows = %d", row0, row0 + P, src_rows, cache_rows);
  DFL_REQUIRE((((uintptr_t)k_rows | (uintptr_t)v_rows) & 15) == 0 && (((uintptr_t)kcodes | (uintptr_t)vcodes) & 7) == 0,
              "dfl_kv_quant_rows: rows must be 16-byte aligned, codes 8-byte aligned");
  if (P == 0) return DFL_OK;
  const int n = 2 * n_kv * P;
  hipLaunchKernelGGL(k_kv_quant_rows, dim3((n + 15) / 16), dim3(256), 0, (hipStream_t)stream, (bf16_t *)k_rows, (bf16_t *)v_rows,
                     src_rows, P, n_kv, (uint8_t *)kcodes, (uint8_t *)vcodes, k_scale, v_scale, cache_rows, row0);
  DFL_CHECK_LAUNCH("dfl_kv_quant_rows");
  return DFL_OK;
}
