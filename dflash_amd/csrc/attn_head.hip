// Block attention, second form (round 2): the attention stage of one block in ONE launch, reading
// the q/k/v projections as FINISHED bf16 Linear outputs (dfl_gemm_resid with add_residual = 0)
// instead of fp32 K-split partials.  Replaces model/dflash.py:71-99 (q/k-norm, local RoPE of :22-28,
// cache append, attention over cached prefix + context + block rows) and, with causal = 1, the same
// stage of the target's verify forward (:249-255).
//
// Why a second form (profiles/r1_*: k_attn_fused = 19.6 us per launch for 4.3 MB of K/V): the first
// form's critical path was  q prologue 4.4 -> new K/V rows 2.4 -> 4 LDS-staged tiles of one wave per
// SIMD 5.8 -> release fence + ticket 2.3 -> 9-way merge of 32 KB partials by ONE workgroup 5.4 us.
// This form removes each of those:
//   * grid (kv head, G query heads x splits): a workgroup owns ONE query head, its 8 waves own
//     disjoint 32-key tiles — no LDS staging shared between waves, no barrier in the tile loop:
//     K fragments go HBM/L2 -> VGPR directly in MFMA A-operand order (a lane's 16 B = 8 consecutive
//     d of one key; 16 keys x 64 B per load instruction, whole 256-B rows over the four k-steps),
//     V rows go through a wave-private 8 KB LDS tile for the transposed read (ds_read_b64_tr_b16);
//   * the G workgroups of a kv head have equal blockIdx.x = kv head: with 8 kv heads they share an
//     XCD under round-robin placement, so the K/V rows they all read come from HBM once and from that
//     XCD's L2 afterwards (speed only, never correctness);
//   * the 8 waves' (m, l, O) meet in LDS (64 KB), so a workgroup publishes ONE 8 KB partial per
//     query tile; at 1k keys that is 6 partials per head instead of 9 x 32 KB per kv head, merged by
//     the last arriver of the HEAD (32 mergers side by side instead of 8);
//   * partials are published with write-through (sc1) stores + drain + relaxed ticket and read back
//     with sc1 loads: no release fence (L2 write-back) and no acquire (L1 invalidate) on the path
//     (MI355X_MICROARCH.md, hand-off table row 1);
//   * this cycle's new rows (context + block: <= 64) are a split of their own: its workgroups turn
//     the rows into K/V (norm, RoPE) in LDS, attend over them from there, and the hh = 0 workgroup
//     also appends them to the cache; no workgroup reads a cache row written in this launch;
//   * lengths may come as immediates (host-driven loop) instead of a dependent scalar load.
// MFMA: S^T = K Q^T and O^T += V^T P^T on v_mfma_f32_16x16x32_bf16 as in attn_block.hip (same
// fragment layouts, same base-2 online softmax in fp32, P rounded to bf16 for the PV product).
#include "attn_head.h"

namespace {

template <int QT>
__global__ __launch_bounds__(512) void k_attn_head(HeadAttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[HeadLds<QT, 8>::kBytes];
  __shared__ int s_last;
  attn_head_body<QT, 8, false>(a, lds, &s_last, blockIdx.x, blockIdx.y, blockIdx.z, nullptr);
}

__global__ __launch_bounds__(512) void k_attn_head_pair(HeadAttnArgs a) {  // two query heads per workgroup
  __shared__ __attribute__((aligned(16))) char lds[HeadLds<2, 8>::kBytes];
  __shared__ int s_last;
  attn_head_body<2, 8, false, true>(a, lds, &s_last, blockIdx.x, blockIdx.y, blockIdx.z, nullptr);
}

// the same two kernels on fp32 K-part sums of the qkv GEMM (HeadAttnArgs::xq32)
__global__ __launch_bounds__(512) void k_attn_head32(HeadAttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[HeadLds<1, 8>::kBytes];
  __shared__ int s_last;
  attn_head_body<1, 8, false, false, true>(a, lds, &s_last, blockIdx.x, blockIdx.y, blockIdx.z, nullptr);
}
__global__ __launch_bounds__(512) void k_attn_head_pair32(HeadAttnArgs a) {
  __shared__ __attribute__((aligned(16))) char lds[HeadLds<2, 8>::kBytes];
  __shared__ int s_last;
  attn_head_body<2, 8, false, true, true>(a, lds, &s_last, blockIdx.x, blockIdx.y, blockIdx.z, nullptr);
}

// ---------------------------------------------------------------------------------------------------------------
// Attention stage + o_proj in ONE launch (round 2; VERDICT r1 item 4: a stage pair kept inside a launch where the
// hand-off buys more than the boundary it replaces).  The attention stage leaves HBM idle for ~10 us per layer, and
// o_proj's weights (Qwen3-8B: 33.5 MB = 131 KB per CU) fit the chip's register files.  So the launch carries, behind
// the attention workgroups, one workgroup per 16-column output tile of o_proj that requests its whole weight slice
// (32 k-steps per wave = 128 VGPRs) the moment it starts — the weights stream from HBM WHILE the attention runs —
// then waits for the heads' final outputs, loads them (sc1), and is 32 MFMAs per wave, a 4-wave LDS reduction and the
// residual epilogue away from done.
// MEASURED (profiles/r2_attn_oproj_stamps.txt): 23.2 us per launch against 10.5 + 9.8 us for the two
// launches it replaces, so the callers keep two launches (fuse_oproj = False) and this stays an opt-in, tested variant.
// The weights do land early (7 us) and every workgroup is resident, but each cross-XCD hand-off costs ~2 us at either
// end (write-through drain, then loads served from beyond L2): ticket 11.5 -> heads merged 16.5 -> seen 17.2 ->
// 128 KB of activations per o_proj workgroup loaded 21.5 -> done 22.5, and the weight stream slows the attention
// itself by 3 us.  The boundary it removes is priced at 1.8 us.
//   * every workgroup has 4 waves with the 256-VGPR budget (__launch_bounds__(256, 2)): a CU holds two, whichever
//     kind; with <= 256 attention workgroups + H/16 = 256 o_proj workgroups the whole grid is resident at once;
//   * no attention workgroup ever waits; an o_proj workgroup waits only for attention workgroups, which have LOWER
//     linear ids (dispatched first), so progress never depends on co-residency; the wait is BOUNDED all the same
//     (2 ms, then *fail = 1 and the workgroup leaves: wrong numbers and a raised error, never a hang);
//   * hand-off: the workgroup that merges a head stores its frag16 output write-through, drains, meets, and adds 1 to
//     each of 32 replicas of `done`; one lane per o_proj workgroup polls ITS replica (relaxed agent-scope load +
//     s_sleep), the workgroup barrier spreads the news, an agent-scope acquire fence precedes the activation loads;
//   * the last o_proj workgroup past its wait re-arms both counters: the launch is capturable and re-launchable as is.
struct AttnOArgs {
  HeadAttnArgs at;
  int n_attn;         // attention workgroups = n_kv * G * (ns_old + 1); workgroup b < n_attn: kv head b % n_kv, y = b / n_kv
  const bf16x8 *wo;   // packed o_proj weight [ntiles][KS][64]
  int KS, ntiles;     // q_dim / 32 (<= 128), H / 16
  bf16_t *h_io;       // residual stream [16][ldh]: h <- bf16(h + bf16(attn . Wo^T))
  int64_t ldh;
  float *ss_out;      // [ntiles][16] partial sums of squares of the new rows (next GEMM's RMSNorm)
  int *done;          // 32 replicas of the heads-done counter, 32 ints (one 128-B line) apart
  int *o_done, *fail;
  int done_target;    // = n_q: heads whose output must be complete
};

__global__ __launch_bounds__(256, 2) void k_attn_oproj(AttnOArgs p) {
  __shared__ __attribute__((aligned(16))) char lds[HeadLds<1, 4>::kBytes];
  __shared__ int s_last;
  const int b = blockIdx.x;
  if (b < p.n_attn) {
    attn_head_body<1, 4, true>(p.at, lds, &s_last, b % p.at.n_kv, b / p.at.n_kv, 0, p.done);
    return;
  }
  const int t = b - p.n_attn;  // output column tile
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
  OSTAMP(0);
  // ---- the whole weight slice of the tile, now: wave w holds k-steps [32 w, 32 w + 32)
  bf16x8 wv[4][8];
  {
    const bf16x8 *base = p.wo + ((size_t)t * p.KS + 32 * w) * 64;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      int nf = p.KS - 32 * w - 8 * c;
      nf = nf < 0 ? 0 : (nf > 8 ? 8 : nf);
      load_ksteps<8>(wv[c], base + c * 8 * 64, nf, l);
    }
  }
#ifdef DFL_ATTN_STAMPS
  OSTAMP(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  OSTAMP(2);  // weights landed
#endif
  // ---- wait (bounded) until every head's output is complete
  if (tid == 0) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    const int *mine = p.done + (t & 31) * 32;  // 8 pollers per replica
    while (__hip_atomic_load(mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < p.done_target) {
      __builtin_amdgcn_s_sleep(8);
      if (__builtin_amdgcn_s_memrealtime() - t0 > 200000ull) {  // 2 ms of the 100 MHz clock
        *p.fail = 1;
        break;
      }
    }
  }
  OSTAMP(3);  // heads done (lane 0's poll)
  __syncthreads();
  // ---- the activation fragments (frag16 of the 16 rows: k-step ks = 1 KiB at out_frag + 64 ks), sc1 loads: 128 KB per
  // workgroup, 4.3 us; an agent-scope acquire fence (L2 invalidate) + plain loads instead took 11 us
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  {
    const __amdgpu_buffer_rsrc_t rx =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8 *>(p.at.out_frag), 0, p.KS * 1024, 0x00020000);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      bf16x8 xv[8];
#pragma unroll
      for (int f = 0; f < 8; ++f)  // (k-steps past KS: out of the descriptor's range, read as zeros)
        xv[f] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rx, ((32 * w + 8 * c + f) * 64 + l) * 16, 0, 16));
#pragma unroll
      for (int f = 0; f < 8; ++f) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wv[c][f], xv[f], acc, 0, 0, 0);
    }
  }
  float *red = reinterpret_cast<float *>(lds);  // [4 waves][256]
  *reinterpret_cast<f32x4 *>(&red[w * 256 + l * 4]) = acc;
  OSTAMP(4);  // activations loaded, MFMAs done (wave 0)
  __syncthreads();
  OSTAMP(5);
  {  // thread (row m, column nl) of the tile; D layout of the MFMA as in gemm_skinny.hip
    const int m = tid >> 4, nl = tid & 15;
    const int idx = 4 * (m + 16 * (nl >> 2)) + (nl & 3);
    float s = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) s += red[ww * 256 + idx];
    const int n = t * 16 + nl;
    const float v = rbf(s);  // the Linear's bf16 output (model/dflash.py:101)
    bf16_t *hp = p.h_io + (int64_t)m * p.ldh + n;
    const float hn = rbf(bf2f(*hp) + v);  // residual add (:140)
    *hp = f2bf(hn);
    const float qs = row_sum16(hn * hn);
    if (nl == 0 && p.ss_out) p.ss_out[t * 16 + m] = qs;
  }
#ifdef DFL_ATTN_STAMPS
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  OSTAMP(6);
  // ---- the last o_proj workgroup past its wait re-arms the counters for the next launch
  if (tid == 0) {
    const int k = __hip_atomic_fetch_add(p.o_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == p.ntiles - 1) {
      for (int r = 0; r < 32; ++r) __hip_atomic_store(p.done + r * 32, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p.o_done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

}  // namespace

#ifdef DFL_ATTN_STAMPS
extern "C" int dfl_debug_read_head_stamps(unsigned long long *host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_hstamps), sizeof(unsigned long long) * 16);
}
extern "C" int dfl_debug_read_attn_max(unsigned long long *host_out) {  // reads and clears
  const int rc = (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_amax), sizeof(unsigned long long) * 16);
  unsigned long long z[16] = {};
  return rc ? rc : (int)hipMemcpyToSymbol(HIP_SYMBOL(g_amax), z, sizeof(z));
}
extern "C" int dfl_debug_read_oproj_stamps(unsigned long long *host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_ostamps), sizeof(unsigned long long) * 16);
}
#endif

extern "C" int64_t dfl_attn_head_ws_bytes(int n_q, int max_splits, int q_tiles) {
  const int64_t b = (int64_t)max_splits * n_q * q_tiles * 16 * (128 + 2) * sizeof(float) + (int64_t)n_q * sizeof(int) + 64;
  return (b + 15) / 16 * 16;   // per-candidate blocks of a multi-candidate launch stay 16-byte aligned
}

// Old-key split constants of the o_proj form (the plain form's: attn_head.h)
#ifndef DFL_ATTN_OPROJ_TILES
#define DFL_ATTN_OPROJ_TILES 4
#endif
#ifndef DFL_ATTN_OPROJ_WGS
#define DFL_ATTN_OPROJ_WGS 256  // with the o_proj tail: 4-wave workgroups, two per CU; 256 attention + H/16 o_proj workgroups fill the 512 slots
#endif

namespace {
// several blocks per launch — requests of a ragged batch, candidates: ONE round of workgroups, 256; with 448 the
// second half-round of a 4-request launch was a tail: 6.10 -> 5.99 ms per 4-request cycle
constexpr int HEAD_WGS_MULTI = 256;
static_assert(DFL_ATTN_HEAD_TILES >= 1 && DFL_ATTN_OPROJ_TILES >= 1, "tiles per split");

// o_proj behind the attention stage in the same launch (dfl_attn_head_oproj)
struct OprojTail {
  const void *wo;
  int q_dim, H;
  void *h_io;
  int64_t ldh;
  float *ss_out;
  int32_t *sync;
};

// What an entry point asks of attn_head_launch.  The defaults are a single block on the cache with one query tile:
// an entry point names only the fields its form uses.
struct HeadLaunch {
  const void *xq = nullptr;  // block rows (nparts32 > 0: fp32 K-part sums, HeadAttnArgs::xq32, strides in floats)
  int64_t ldq = 0;
  int q_col = 0, k_col = 0, v_col = 0;
  const void *xc = nullptr;  // context rows (the draft's single-request form only)
  int64_t ldc = 0;
  int ck_col = 0, cv_col = 0;
  int n_q = 0, n_kv = 0;
  const void *q_norm_w = nullptr, *k_norm_w = nullptr;
  float eps = 0.f;
  const void *cos_tab = nullptr, *sin_tab = nullptr;
  int max_pos = 0;
  void *kcache = nullptr, *vcache = nullptr;
  int cache_rows = 0;
  float scale = 0.f;
  int causal = 0;
  const int32_t *dyn = nullptr;  // null: the immediates below are the lengths; else S bounds dyn[S]
  int S = 0, tau = 0, bs = 0, pos0 = 0;
  int q_tiles = 1;
  void *ws = nullptr;
  int max_splits = 0;
  void *out_frag = nullptr;
  int64_t out_tile_stride = 0;
  // several blocks per launch (grid.z): candidates on one cache, or the requests of a ragged batch
  int n_cand = 1;
  int64_t xq_cand_stride = 0, out_cand_stride = 0;
  void *k_out = nullptr, *v_out = nullptr;  // K/V staging area of the candidates
  int64_t kv_out_cand_stride = 0;
  int out_rows = 0;
  int dyn_cand_stride = 0;
  int64_t cache_cand_stride = 0;
  const OprojTail *tail = nullptr;
  int nparts32 = 0;
  int64_t part_stride32 = 0;
  void *stream = nullptr;
};

int attn_head_launch(const HeadLaunch &L) {
  DFL_REQUIRE(L.xq && L.cos_tab && L.sin_tab && L.kcache && L.vcache && L.out_frag && L.ws, "dfl_attn_head: null pointer");
  DFL_REQUIRE(L.nparts32 >= 0 && L.nparts32 <= 2 &&
                  (L.nparts32 == 0 || (!L.tail && L.q_tiles == 1 && L.tau == 0 && !L.xc && L.part_stride32 % 4 == 0)),
              "dfl_attn_head: the fp32-partials form takes 1 or 2 K parts, one query tile, no context rows");
  DFL_REQUIRE((L.q_norm_w == nullptr) == (L.k_norm_w == nullptr), "dfl_attn_head: give both norm weights or neither");
  DFL_REQUIRE(L.n_q > 0 && L.n_kv > 0 && L.n_q % L.n_kv == 0, "dfl_attn_head: bad head counts (n_q=%d n_kv=%d)", L.n_q, L.n_kv);
  DFL_REQUIRE(L.q_tiles == 1 || L.q_tiles == 2, "dfl_attn_head: q_tiles must be 1 or 2");
  DFL_REQUIRE(L.ldq > 0 && L.ldq % 8 == 0 && L.q_col >= 0 && L.k_col >= 0 && L.v_col >= 0 && L.q_col % 8 == 0 &&
                  L.k_col % 8 == 0 && L.v_col % 8 == 0 && L.max_pos > 0,
              "dfl_attn_head: bad block-row layout");
  DFL_REQUIRE(L.S >= 0 && L.tau >= 0 && L.tau <= 32 && L.bs >= 1 && L.bs <= 16 * L.q_tiles && L.tau + L.bs <= 64,
              "dfl_attn_head: lengths S=%d tau=%d bs=%d outside the kernel's range (q_tiles=%d)", L.S, L.tau, L.bs, L.q_tiles);
  DFL_REQUIRE(L.tau == 0 || (L.xc && L.ldc > 0 && L.ldc % 8 == 0 && L.ck_col >= 0 && L.cv_col >= 0 && L.ck_col % 8 == 0 &&
                             L.cv_col % 8 == 0),
              "dfl_attn_head: context rows without a context source");
  DFL_REQUIRE(L.S + (L.k_out ? 0 : L.tau + L.bs) <= L.cache_rows, "dfl_attn_head: S + tau + bs = %d exceeds cache_rows = %d",
              L.S + L.tau + L.bs, L.cache_rows);
  DFL_REQUIRE(L.max_splits >= 1 && L.out_tile_stride >= 0 && L.out_tile_stride % 8 == 0,
              "dfl_attn_head: bad max_splits / out_tile_stride");
  DFL_REQUIRE(L.n_cand >= 1 && L.n_cand <= 64, "dfl_attn_head: n_cand outside 1..64");
  DFL_REQUIRE(L.n_cand == 1 || (L.xq_cand_stride % 8 == 0 && L.out_cand_stride % 8 == 0 && L.cache_cand_stride % 8 == 0 &&
                              ((L.k_out && L.v_out) || L.cache_cand_stride >= (int64_t)L.n_kv * L.cache_rows * 128)),
              "dfl_attn_head: several blocks per launch need 8-element strides and either a K/V staging area "
              "(candidates on one cache) or a cache per request");
  DFL_REQUIRE(!L.k_out == !L.v_out &&
                  (!L.k_out || (L.out_rows >= L.tau + L.bs && L.kv_out_cand_stride >= (int64_t)L.n_kv * L.out_rows * 128)),
              "dfl_attn_head: bad K/V staging area");
  // Old-key splits: a workgroup's 8 waves take one 32-key tile each per round, so up to 8 tiles
  // per split cost one round; beyond ~224 workgroups per launch the splits grow instead
  // (S here is the bound the caller sized the launch for when the lengths come from dyn).
  const int G = L.n_q / L.n_kv;
  const int nt = (L.S + 31) / 32;
  const int tiles = L.tail ? DFL_ATTN_OPROJ_TILES : DFL_ATTN_HEAD_TILES;
  const int wgs = L.n_cand > 1 ? HEAD_WGS_MULTI : DFL_ATTN_HEAD_WGS;
  int ns_old = head_old_splits(nt, tiles, L.tail ? DFL_ATTN_OPROJ_WGS : wgs, L.n_q * L.n_cand);
  // Head pairs (k_attn_head_pair): when the splits the budget allows would leave a wave more than one tile, two heads
  // per workgroup halve the K/V pulled through L2 and double the splits.
  // Measured on the 8B shapes (cycle, ms): S = 2048 4.28 -> 4.40 (worse), 4096 4.48 -> 4.49, 8192 4.78 -> 4.68: on from ~5k keys.
  // Several blocks per launch (requests of a ragged batch, candidates): the one round of workgroups leaves a single
  // old-key split per head from two requests on, i.e. ~4 tiles per wave at S = 1k — pairs on whenever the budget
  // leaves a wave more than one tile (round 3, same box: 4 requests 6.03 -> 5.81 ms per cycle, 3 requests 5.97 -> 5.69;
  // 2 requests 5.22 -> 5.29: from three blocks on).
  const bool pair = !L.tail && L.q_tiles == 1 && G % 2 == 0 && L.bs <= 16 && nt > tiles * ns_old && (nt > 160 || L.n_cand > 2);
  if (pair) {
    ns_old = head_old_splits(nt, tiles, wgs, (L.n_q / 2) * L.n_cand);
  }
  ns_old = ns_old > L.max_splits - 1 ? L.max_splits - 1 : ns_old;
  if (nt == 0 && !L.dyn) ns_old = 0;
  HeadAttnArgs a{};
  a.xq = (const bf16_t *)L.xq;
  a.ldq = L.ldq;
  a.q_col = L.q_col;
  a.k_col = L.k_col;
  a.v_col = L.v_col;
  a.xc = (const bf16_t *)L.xc;
  a.ldc = L.ldc;
  a.ck_col = L.ck_col;
  a.cv_col = L.cv_col;
  a.q_w = (const bf16_t *)L.q_norm_w;
  a.k_w = (const bf16_t *)L.k_norm_w;
  a.eps = L.eps;
  a.cos_tab = (const bf16_t *)L.cos_tab;
  a.sin_tab = (const bf16_t *)L.sin_tab;
  a.max_pos = L.max_pos;
  a.kc = (bf16_t *)L.kcache;
  a.vc = (bf16_t *)L.vcache;
  a.cache_rows = L.cache_rows;
  a.n_q = L.n_q;
  a.n_kv = L.n_kv;
  a.G = G;
  a.scale_log2 = L.scale * 1.4426950408889634f;
  a.causal = L.causal ? 1 : 0;
  a.dyn = L.dyn;
  a.S = L.S;
  a.tau = L.tau;
  a.bs = L.bs;
  a.pos0 = L.pos0;
  a.out_frag = (bf16x8 *)L.out_frag;
  a.out_tile_stride = L.out_tile_stride / 8;
  const int64_t rows = (int64_t)L.max_splits * L.n_q * L.q_tiles * 16;
  a.o_part = (float *)L.ws;
  a.ml_part = (float *)L.ws + rows * 128;
  a.tickets = (int *)((float *)L.ws + rows * 130);
  a.ns_old = ns_old;
  a.xq_cand_stride = L.xq_cand_stride;
  a.out_cand_stride = L.out_cand_stride / 8;
  a.ws_cand_stride = dfl_attn_head_ws_bytes(L.n_q, L.max_splits, L.q_tiles) / 4;
  a.k_out = (bf16_t *)L.k_out;
  a.v_out = (bf16_t *)L.v_out;
  a.kv_out_cand_stride = L.kv_out_cand_stride;
  a.out_rows = L.out_rows;
  a.dyn_cand_stride = L.dyn_cand_stride;
  a.cache_cand_stride = L.cache_cand_stride;
  const dim3 grid(L.n_kv, (pair ? G / 2 : G) * (ns_old + 1), L.n_cand);
  hipStream_t st = (hipStream_t)L.stream;
  if (L.nparts32 > 0) {
    a.xq = nullptr;
    a.xq32 = (const float *)L.xq;
    a.nparts32 = L.nparts32;
    a.part_stride32 = L.part_stride32;
    if (pair)
      hipLaunchKernelGGL(k_attn_head_pair32, grid, dim3(512), 0, st, a);
    else
      hipLaunchKernelGGL(k_attn_head32, grid, dim3(512), 0, st, a);
    DFL_CHECK_LAUNCH("dfl_attn_head_batch_f32");
    return DFL_OK;
  }
  if (pair) {
    hipLaunchKernelGGL(k_attn_head_pair, grid, dim3(512), 0, st, a);
    DFL_CHECK_LAUNCH("dfl_attn_head");
    return DFL_OK;
  }
  if (L.tail) {
    AttnOArgs p{};
    p.at = a;
    p.n_attn = L.n_kv * G * (ns_old + 1);
    p.wo = (const bf16x8 *)L.tail->wo;
    p.KS = L.tail->q_dim / 32;
    p.ntiles = L.tail->H / 16;
    p.h_io = (bf16_t *)L.tail->h_io;
    p.ldh = L.tail->ldh;
    p.ss_out = L.tail->ss_out;
    p.done = L.tail->sync;
    p.o_done = L.tail->sync + 1024;
    p.fail = L.tail->sync + 1025;
    p.done_target = L.n_q;
    hipLaunchKernelGGL(k_attn_oproj, dim3(p.n_attn + p.ntiles), dim3(256), 0, st, p);
    DFL_CHECK_LAUNCH("dfl_attn_head_oproj");
    return DFL_OK;
  }
  if (L.q_tiles == 1)
    hipLaunchKernelGGL(k_attn_head<1>, grid, dim3(512), 0, st, a);
  else
    hipLaunchKernelGGL(k_attn_head<2>, grid, dim3(512), 0, st, a);
  DFL_CHECK_LAUNCH("dfl_attn_head");
  return DFL_OK;
}
}  // namespace

extern "C" int dfl_attn_head(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, const void *xc, int64_t ldc,
                             int ck_col, int cv_col, int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w,
                             float eps, const void *cos_tab, const void *sin_tab, int max_pos, void *kcache,
                             void *vcache, int cache_rows, float scale, int causal, const int32_t *dyn, int S, int tau,
                             int bs, int pos0, int q_tiles, void *ws, int max_splits, void *out_frag,
                             int64_t out_tile_stride, void *stream) {
  HeadLaunch L;
  L.xq = xq, L.xc = xc, L.ldc = ldc, L.ck_col = ck_col, L.cv_col = cv_col;
  L.ldq = ldq, L.q_col = q_col, L.k_col = k_col, L.v_col = v_col;
  L.n_q = n_q, L.n_kv = n_kv, L.q_norm_w = q_norm_w, L.k_norm_w = k_norm_w, L.eps = eps;
  L.cos_tab = cos_tab, L.sin_tab = sin_tab, L.max_pos = max_pos;
  L.kcache = kcache, L.vcache = vcache, L.cache_rows = cache_rows, L.scale = scale, L.causal = causal;
  L.dyn = dyn, L.S = S, L.tau = tau, L.bs = bs, L.pos0 = pos0, L.q_tiles = q_tiles;
  L.ws = ws, L.max_splits = max_splits, L.out_frag = out_frag, L.out_tile_stride = out_tile_stride, L.stream = stream;
  return attn_head_launch(L);
}

extern "C" int dfl_attn_head_oproj(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, const void *xc, int64_t ldc,
                                   int ck_col, int cv_col, int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w,
                                   float eps, const void *cos_tab, const void *sin_tab, int max_pos, void *kcache,
                                   void *vcache, int cache_rows, float scale, int causal, const int32_t *dyn, int S, int tau,
                                   int bs, int pos0, void *ws, int max_splits, void *attn_frag, const void *wo_packed, int H,
                                   void *h_io, int64_t ldh, float *ss_out, int32_t *sync, void *stream) {
  DFL_REQUIRE(wo_packed && h_io && sync, "dfl_attn_head_oproj: null pointer");
  DFL_REQUIRE(H > 0 && H % 16 == 0 && ldh >= H && n_q * 128 <= 4096 && bs <= 16 && tau + bs <= 32,
              "dfl_attn_head_oproj: H=%d q_dim=%d tau=%d bs=%d outside the kernel's range (q_dim <= 4096, tau + bs <= 32)", H,
              n_q * 128, tau, bs);
  const OprojTail tail{wo_packed, n_q * 128, H, h_io, ldh, ss_out, sync};
  HeadLaunch L;
  L.xq = xq, L.xc = xc, L.ldc = ldc, L.ck_col = ck_col, L.cv_col = cv_col;
  L.ldq = ldq, L.q_col = q_col, L.k_col = k_col, L.v_col = v_col;
  L.n_q = n_q, L.n_kv = n_kv, L.q_norm_w = q_norm_w, L.k_norm_w = k_norm_w, L.eps = eps;
  L.cos_tab = cos_tab, L.sin_tab = sin_tab, L.max_pos = max_pos;
  L.kcache = kcache, L.vcache = vcache, L.cache_rows = cache_rows, L.scale = scale, L.causal = causal;
  L.dyn = dyn, L.S = S, L.tau = tau, L.bs = bs, L.pos0 = pos0;
  L.ws = ws, L.max_splits = max_splits, L.out_frag = attn_frag, L.tail = &tail, L.stream = stream;
  return attn_head_launch(L);
}

// Candidate c = q_tiles consecutive 16-row tiles of xq / out_frag (blocks of 17..32 rows: two); staging rows 0..bs-1.
// Causal, no context rows, the lengths are the immediates S and bs.
extern "C" int dfl_attn_head_cand(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, int n_cand,
                                  int64_t xq_cand_stride, int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w,
                                  float eps, const void *cos_tab, const void *sin_tab, int max_pos, const void *kcache,
                                  const void *vcache, int cache_rows, float scale, int S, int bs, void *ws, int max_splits,
                                  void *out_frag, int64_t out_cand_stride, int64_t out_tile_stride, int q_tiles, void *k_out,
                                  void *v_out, int64_t kv_out_cand_stride, int out_rows, void *stream) {
  DFL_REQUIRE(n_cand >= 1 && k_out && v_out, "dfl_attn_head_cand: needs the K/V staging area");
  DFL_REQUIRE(q_tiles == 1 || q_tiles == 2, "dfl_attn_head_cand: q_tiles must be 1 or 2");
  HeadLaunch L;
  L.xq = xq;
  L.ldq = ldq, L.q_col = q_col, L.k_col = k_col, L.v_col = v_col;
  L.n_q = n_q, L.n_kv = n_kv, L.q_norm_w = q_norm_w, L.k_norm_w = k_norm_w, L.eps = eps;
  L.cos_tab = cos_tab, L.sin_tab = sin_tab, L.max_pos = max_pos;
  L.kcache = const_cast<void *>(kcache), L.vcache = const_cast<void *>(vcache), L.cache_rows = cache_rows;
  L.scale = scale, L.causal = 1, L.S = S, L.bs = bs, L.pos0 = S, L.q_tiles = q_tiles;
  L.ws = ws, L.max_splits = max_splits, L.out_frag = out_frag, L.out_tile_stride = out_tile_stride;
  L.n_cand = n_cand, L.xq_cand_stride = xq_cand_stride, L.out_cand_stride = out_cand_stride;
  L.k_out = k_out, L.v_out = v_out, L.kv_out_cand_stride = kv_out_cand_stride, L.out_rows = out_rows, L.stream = stream;
  return attn_head_launch(L);
}

// Request r = q_tiles consecutive 16-row tiles of xq / out_frag (strides per request; blocks of 17..32 rows: two), one
// cache, one length record whose bs counts both tiles.
extern "C" int dfl_attn_head_batch(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, int R, int64_t xq_req_stride,
                                   int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w, float eps,
                                   const void *cos_tab, const void *sin_tab, int max_pos, void *kcache, void *vcache,
                                   int cache_rows, int64_t cache_req_stride, float scale, int causal, const int32_t *dyn,
                                   int kv_len_max, void *ws, int max_splits, void *out_frag, int64_t out_req_stride,
                                   int64_t out_tile_stride, int q_tiles, void *stream) {
  DFL_REQUIRE(dyn, "dfl_attn_head_batch: the requests' lengths come from dyn (R records)");
  DFL_REQUIRE(q_tiles == 1 || q_tiles == 2, "dfl_attn_head_batch: q_tiles must be 1 or 2");
  DFL_REQUIRE(kv_len_max >= 16 * q_tiles && kv_len_max <= cache_rows,
              "dfl_attn_head_batch: kv_len_max=%d outside %d..cache_rows", kv_len_max, 16 * q_tiles);
  // lengths from the device records (block form: tau = 0, bs <= 16 * q_tiles); kv_len_max - 16 * q_tiles bounds every S
  HeadLaunch L;
  L.xq = xq;
  L.ldq = ldq, L.q_col = q_col, L.k_col = k_col, L.v_col = v_col;
  L.n_q = n_q, L.n_kv = n_kv, L.q_norm_w = q_norm_w, L.k_norm_w = k_norm_w, L.eps = eps;
  L.cos_tab = cos_tab, L.sin_tab = sin_tab, L.max_pos = max_pos;
  L.kcache = kcache, L.vcache = vcache, L.cache_rows = cache_rows, L.scale = scale, L.causal = causal;
  L.dyn = dyn, L.S = kv_len_max - 16 * q_tiles, L.bs = 16 * q_tiles, L.q_tiles = q_tiles;
  L.ws = ws, L.max_splits = max_splits, L.out_frag = out_frag, L.out_tile_stride = out_tile_stride;
  L.n_cand = R, L.xq_cand_stride = xq_req_stride, L.out_cand_stride = out_req_stride;
  L.dyn_cand_stride = DFL_DYN_WORDS, L.cache_cand_stride = cache_req_stride, L.stream = stream;
  return attn_head_launch(L);
}

// dfl_attn_head_batch on the fp32 K-PART SUMS of the qkv projection (dfl_gemm_f32_batch's output: [part][R tiles x 16
// rows][ldq] floats) instead of finished bf16 rows: request r's rows of part k at xq_parts + k * part_stride +
// r * xq_req_stride (floats); a value is bf16(part 0 + part 1).  The K parts of the projection meet in this launch's row
// loads, so the GEMM in front of it needs no slab / ticket / combine phase of its own.
extern "C" int dfl_attn_head_batch_f32(const float *xq_parts, int nparts, int64_t part_stride, int64_t ldq, int q_col, int k_col,
                                       int v_col, int R, int64_t xq_req_stride, int n_q, int n_kv, const void *q_norm_w,
                                       const void *k_norm_w, float eps, const void *cos_tab, const void *sin_tab, int max_pos,
                                       void *kcache, void *vcache, int cache_rows, int64_t cache_req_stride, float scale,
                                       int causal, const int32_t *dyn, int kv_len_max, void *ws, int max_splits,
                                       void *out_frag, int64_t out_req_stride, void *stream) {
  DFL_REQUIRE(dyn, "dfl_attn_head_batch_f32: the requests' lengths come from dyn (R records)");
  DFL_REQUIRE(nparts == 1 || nparts == 2, "dfl_attn_head_batch_f32: 1 or 2 K parts (got %d)", nparts);
  DFL_REQUIRE(kv_len_max >= 16 && kv_len_max <= cache_rows, "dfl_attn_head_batch_f32: kv_len_max=%d outside 16..cache_rows",
              kv_len_max);
  HeadLaunch L;
  L.xq = xq_parts, L.nparts32 = nparts, L.part_stride32 = part_stride;
  L.ldq = ldq, L.q_col = q_col, L.k_col = k_col, L.v_col = v_col;
  L.n_q = n_q, L.n_kv = n_kv, L.q_norm_w = q_norm_w, L.k_norm_w = k_norm_w, L.eps = eps;
  L.cos_tab = cos_tab, L.sin_tab = sin_tab, L.max_pos = max_pos;
  L.kcache = kcache, L.vcache = vcache, L.cache_rows = cache_rows, L.scale = scale, L.causal = causal;
  L.dyn = dyn, L.S = kv_len_max - 16, L.bs = 16;
  L.ws = ws, L.max_splits = max_splits, L.out_frag = out_frag;
  L.n_cand = R, L.xq_cand_stride = xq_req_stride, L.out_cand_stride = out_req_stride;
  L.dyn_cand_stride = DFL_DYN_WORDS, L.cache_cand_stride = cache_req_stride, L.stream = stream;
  return attn_head_launch(L);
}
