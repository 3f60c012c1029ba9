// The shared MoE pass on OCP MXFP4 codes: dfl_moe_grouped_gate_up / dfl_moe_grouped_down with DFL_W_MXFP4 (prefill.hip
// dispatches here; layout in include/dflash_hip.h, the 4-bit pieces in gemm_rows.h, DESIGN.md section 17, "The shared
// pass").  A source of its own, built like moe_w4.hip without gfx950's packed fp32 instructions (build.py).
//
// Not a third k_pgemm flag: that kernel is the prefill's block form (128 x 64 blocks, the weights staged through LDS), and
// at 4 bits an item's weights are a quarter of the bf16 bytes, so its per-item ramp and staging would weigh four times as
// much.  This is the decode-shaped grouped kernel:
//   * a work item is dfl_prefill_moe_route's (expert, first gathered tile, tiles); a workgroup takes (item, group of NW
//     column units), a WAVE owns one unit — two adjacent column tiles of the expert: a (gate, up) pair, or two tiles of the
//     down projection — and walks K itself.  The accumulators are the finished sums of (column tile, row tile): no K split,
//     no cross-wave sum, k-steps 0 .. K/32 - 1 in order into every accumulator, which is the bf16 grouped launch's order;
//     e2m1 * 2^n is exact in bf16, so the launch gives the bits of the bf16 launch on the dequantised weights;
//   * weights: HBM -> VGPR -> MFMA.  A chunk is 128 k: ONE non-temporal 16-byte word per lane and tile plus one scale dword,
//     the scale in front of its word (load_words_w4), A = 3 chunks in flight per wave; w4_frag converts in front of the
//     MFMAs of each k-step (the block scale rides in the conversion).  No LDS stage for the weights;
//   * activations: the item's <= 4 row tiles of a chunk (4 k-steps x 4 tiles x 1 KiB fragments, frag16 = MFMA B order)
//     enter LDS once per workgroup by LDS-DMA in its buffer form, A chunks ahead in a ring of A + 1 slots of 16 KiB; every
//     wave issues 16 / NW pieces per chunk.  The gather happens in the addresses: lane (g, r) of a piece of gathered row
//     tile t reads 16 bytes of source row src_row[16 t + r]; a padding row, a row tile beyond the item's count and a chunk
//     past K get an offset outside the descriptor — zeros in LDS, no traffic (so zeros_1k is asked for, as the bf16 form
//     does, but not read).  src_row == NULL: the gathered copy, lane-linear;
//   * one s_barrier per chunk; every request of the loop is unconditional with a constant count per iteration, so the
//     wave's in-order vmcnt is waited on by an immediate: at the top of iteration c its pieces of chunk c are older than
//     exactly A * 4 weight requests and (A - 1) * 16 / NW pieces.  The ring is read by inline asm (gemm_ring.h: behind an
//     LDS read the compiler can see, it waits for every LDS-DMA in flight);
//   * row tiles beyond the item's count are neither read from LDS, nor computed, nor written.  An item of 5..8 tiles
//     (rows_per_item 128) is served in two passes of <= 4 row tiles over the same weights: right, not fast.
#include "gemm_rows.h"

#include <type_traits>

namespace {

typedef __attribute__((address_space(3))) void s_lds_void;

enum { W4S_SILU = 0, W4S_SCALE32 = 1 };
// waves per workgroup: two 8-wave workgroups share a CU.  Same box, 30B-A3B, 2 / 4 tiles: gate/up 46.6 / 48.6 us, down
// 29.5 / 30.7 us; with 16 waves (one workgroup and one ring per CU) 60.0 / 61.0 and 31.4 / 33.2 us
// (profiles/mxfp4_experts_shared_ab.txt) — 16 stays out
constexpr int W4S_NW = 8;
constexpr int W4S_A = 3;                 // chunks of look-ahead (weights in flight per wave: A x 2 KiB)
constexpr int W4S_NS = W4S_A + 1;        // ring slots
constexpr int W4S_SLOT = 16 * 1024;      // [4 k-steps][4 row tiles][1 KiB]
constexpr unsigned W4S_OOB = 0x80000000u;  // the activation descriptor's extent: an offset from here on reads zeros

struct MoeW4SArgs {
  const bf16x8 *wp;      // codes [E][ntiles][KS/4][64 lanes][16 B]
  int64_t expert16;      // 16-byte units of codes per expert
  const char *wscale;    // e8m0 [E][ntiles][KS/4][16 columns][4 B]
  const bf16x8 *xf;      // frag16 row tiles [.][KS][64]: ungathered (src_row) or gathered
  const int32_t *items, *n_items, *src_row;
  int KS, ntiles, nunits;  // K / 32 (% 4 == 0), column tiles per expert, units of two adjacent tiles per expert
  bf16x8 *act;           // SILU: frag16 tiles of I columns [gathered tile][KSo][64]
  int KSo;
  const float *row_w;    // SCALE32: [gathered row]
  float *out32;          //          [gathered row][ld32]
  int64_t ld32;
};

// p[i], i wave-uniform, by ONE scalar load through the constant address space (the plan was written by an earlier launch)
__device__ __forceinline__ int plan_at(const int32_t *p, int i) {
  typedef const __attribute__((address_space(4))) int32_t *cptr;
  return *(cptr)(uintptr_t)(p + __builtin_amdgcn_readfirstlane(i));
}

// the fragments of row tiles 0 .. NT - 1 of one k-step out of a ring slot (1 KiB apart), hidden from the compiler
template <int NT>
__device__ __forceinline__ void ring_read(bf16x8 (&b)[NT], unsigned addr) {
  if constexpr (NT == 4)
    asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\t"
                 "ds_read_b128 %3, %4 offset:3072\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3]) : "v"(addr) : "memory");
  else if constexpr (NT == 3)
    asm volatile("ds_read_b128 %0, %3\n\tds_read_b128 %1, %3 offset:1024\n\tds_read_b128 %2, %3 offset:2048\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]) : "v"(addr) : "memory");
  else if constexpr (NT == 2)
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(b[0]), "=&v"(b[1]) : "v"(addr) : "memory");
  else
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(b[0]) : "v"(addr) : "memory");
}

// (four waves per SIMD, i.e. 128 VGPRs: two 8-wave workgroups and their two 64 KiB rings share a CU)
template <int EPI>
__global__ __launch_bounds__(W4S_NW * 64) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_moe_w4_shared(MoeW4SArgs a) {
  constexpr int NW = W4S_NW, A = W4S_A, NS = W4S_NS, SP = 16 / NW;
  constexpr int VMC = A * 4 + (A - 1) * SP;  // requests of a wave younger than its pieces of the chunk it is about to read
  static_assert(NW % 4 == 0 && 16 % NW == 0, "a wave's pieces of a chunk belong to ONE row tile (w & 3)");
  __shared__ __attribute__((aligned(1024))) unsigned char ring[NS * W4S_SLOT];
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
  const int fm = l & 15, fg = l >> 4;  // D layout (A = W columns, B = rows): row fm of the row tile, columns 4 fg .. + 3
  // (item, column group): the column groups of an item share blockIdx % 8, i.e. an XCD and its L2 (k_pgemm's grouped map)
  const int ncg = (a.nunits + NW - 1) / NW;
  const int seq = blockIdx.x >> 3, item = (seq / ncg) * 8 + (blockIdx.x & 7), cg = seq % ncg;
  if (item >= plan_at(a.n_items, 0)) return;  // (uniform: the grid is sized for the worst case)
  const int e = plan_at(a.items, 3 * item), tile0 = plan_at(a.items, 3 * item + 1), nt_all = plan_at(a.items, 3 * item + 2);
  const int words = a.KS >> 2;                  // chunks: 1 KiB wave words (and 64-byte scale lines) per column tile
  const int nit = (words + A - 1) / A * A;      // iterations, rounded up to the unroll (past K: clipped, zeros, no traffic)
  const int u = cg * NW + w, t0 = 2 * u;        // the wave's unit and its first column tile
  const int ntw = __builtin_amdgcn_readfirstlane(u < a.nunits ? min(2, a.ntiles - t0) : 0);  // its column tiles (0: no unit)
  const bf16x8 *wbase = a.wp + e * a.expert16 + (int64_t)(ntw ? t0 : 0) * words * 64;
  const char *sbase = a.wscale + ((int64_t)e * a.ntiles + (ntw ? t0 : 0)) * words * 64;
  const unsigned ring_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)ring;
  const __amdgpu_buffer_rsrc_t xr =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8 *>(a.xf), 0, (int)W4S_OOB, 0x00020000);
  const int tw = w & 3;  // the row tile of this wave's pieces: piece i = w + s * NW is (k-step i >> 2, row tile i & 3)

  auto wload = [&](bf16x8(&wv)[2], uint32_t(&sv)[2], int c) {
    load_words_w4<2>(wv, sv, wbase + c * 64, sbase + c * 64, c < words ? ntw : 0, words, l);
  };

  for (int p0 = 0; p0 < nt_all; p0 += 4) {  // (one pass unless rows_per_item is 128 and the item has 5..8 tiles)
    const int ntl = __builtin_amdgcn_readfirstlane(min(4, nt_all - p0)), tl0 = tile0 + p0;
    // byte offset of this lane's 16 bytes of a piece at k-step 0
    unsigned xoff = W4S_OOB;
    if (tw < ntl) {
      if (a.src_row) {
        const int m = a.src_row[(tl0 + tw) * 16 + fm];
        if (m >= 0) xoff = (((unsigned)(m >> 4) * a.KS) * 64 + fg * 16 + (m & 15)) * 16;
      } else {
        xoff = ((unsigned)(tl0 + tw) * a.KS * 64 + l) * 16;
      }
    }
    int slot_w = 0, slot_r = 0;  // ring slots of the next stage() / the next chunk to compute
    auto stage = [&](int c) {
      const unsigned slot = ring_base + (unsigned)slot_w * W4S_SLOT;
      slot_w = slot_w + 1 == NS ? 0 : slot_w + 1;
      const unsigned vo = c < words ? xoff + (unsigned)c * 4096 : W4S_OOB;
#pragma unroll
      for (int s = 0; s < SP; ++s) {
        const int f = (w >> 2) + s * (NW / 4);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (s_lds_void *)(uintptr_t)(slot + (unsigned)(f * 4 + tw) * 1024), 16,
                                                 vo + f * 1024, 0, 0, 0);
      }
    };

    bf16x8 wreg[A][2];
    uint32_t sreg[A][2];
#pragma unroll
    for (int c = 0; c < A; ++c) {  // pieces, then weights, per chunk: the order VMC counts
      stage(c);
      __builtin_amdgcn_sched_barrier(0);
      wload(wreg[c], sreg[c], c);
      __builtin_amdgcn_sched_barrier(0);
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int tp = 0; tp < 2; ++tp)
#pragma unroll
      for (int t = 0; t < 4; ++t) acc[tp][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // one k-step for NT live row tiles: the NT fragments out of the ring against the two tiles' converted weights
    auto kstep = [&](auto ntc, const bf16x8(&wf)[2], unsigned rd) {
      constexpr int NT = decltype(ntc)::value;
      bf16x8 b[NT];
      ring_read<NT>(b, rd);
#pragma unroll
      for (int tp = 0; tp < 2; ++tp)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[tp][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[tp], b[t], acc[tp][t], 0, 0, 0);
    };
    // one chunk: per k-step the two tiles' weights converted once, in front of that k-step's MFMAs (the branch on the item's
    // tile count is wave-uniform and holds no request)
    auto chunk = [&](const bf16x8(&wv)[2], const uint32_t(&sv)[2], unsigned rd) {
#pragma unroll
      for (int f = 0; f < 4; ++f) {
        const bf16x8 wf[2] = {w4_frag(wv[0], sv[0], f), w4_frag(wv[1], sv[1], f)};
        if (ntl == 1) kstep(std::integral_constant<int, 1>{}, wf, rd + f * 4096);
        else if (ntl == 2) kstep(std::integral_constant<int, 2>{}, wf, rd + f * 4096);
        else if (ntl == 3) kstep(std::integral_constant<int, 3>{}, wf, rd + f * 4096);
        else kstep(std::integral_constant<int, 4>{}, wf, rd + f * 4096);
      }
    };

    for (int c0 = 0; c0 < nit; c0 += A) {
#pragma unroll
      for (int ca = 0; ca < A; ++ca) {
        const int c = c0 + ca;
        // this wave's pieces of chunk c have landed ...
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");
        // ... and everyone's; every wave has finished reading the chunk before, whose slot the next request takes
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        stage(c + A);
        __builtin_amdgcn_sched_barrier(0);
        const unsigned rd = ring_base + (unsigned)slot_r * W4S_SLOT + l * 16;
        slot_r = slot_r + 1 == NS ? 0 : slot_r + 1;
        if (c < words && ntw) chunk(wreg[ca], sreg[ca], rd);  // (uniform; no request inside)
        // the registers just consumed take the same words of the chunk A ahead
        __builtin_amdgcn_sched_barrier(0);
        wload(wreg[ca], sreg[ca], c + A);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // the padding pieces past the last chunk still target the ring: nothing of this wave is in flight when it leaves
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    // ---- epilogues: pgemm_epilogue's (prefill.hip), no scale multiply
    if (ntw) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t >= ntl) continue;
        const int mt = tl0 + t;
        if (EPI == W4S_SILU) {  // tf:modeling_qwen3.py:82, rounded where torch rounds
          const int n0 = u * 16 + 4 * fg;
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float gb = rbf(acc[0][t][r]), ub = rbf(acc[1][t][r]);
            const float act = rbf(gb / (1.f + __expf(-gb)));
            o[r] = f2bf(act * ub);
          }
          bf16_t *dst =
              reinterpret_cast<bf16_t *>(a.act + ((size_t)mt * a.KSo + (n0 >> 5)) * 64 + ((n0 >> 3) & 3) * 16 + fm) + (n0 & 7);
          *reinterpret_cast<bf16x4 *>(dst) = o;
        } else {  // an expert's down projection: scaled by the row's routing weight, kept fp32
          const int m = mt * 16 + fm;
          const float rw = a.row_w[m];
#pragma unroll
          for (int tp = 0; tp < 2; ++tp) {
            if (tp >= ntw) continue;
            f32x4 o;
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = rw * acc[tp][t][r];
            *reinterpret_cast<f32x4 *>(a.out32 + (int64_t)m * a.ld32 + (t0 + tp) * 16 + 4 * fg) = o;
          }
        }
      }
    }
    if (p0 + 4 < nt_all) {  // every wave has left the ring before the next pass's prologue writes it
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
    }
  }
}

// what both launches ask of the descriptor and the plan, in the order include/dflash_hip.h lists
bool w4s_fill(MoeW4SArgs &a, const char *who, const dfl_weight *w, int64_t w_expert_stride, const void *x, const int32_t *items,
              const int32_t *n_items, int max_items, int N, int K, const char *kname, int rows_per_item) {
  if (!w4_scales_ok(who, w)) return false;
  if (N <= 0 || K <= 0 || K % 128 || N % 16) {
    dfl_set_error("%s: DFL_W_MXFP4 needs %s %% 128 == 0 (a chunk is one 4-k-step word per column tile) and N %% 16 == 0 "
                  "(N=%d %s=%d)", who, kname, N, kname, K);
    return false;
  }
  if (w_expert_stride != (int64_t)N * K / 2) {
    dfl_set_error("%s: DFL_W_MXFP4 expert stride must be N*K/2 bytes of codes (N=%d %s=%d, stride %lld)", who, N, kname, K,
                  (long long)w_expert_stride);
    return false;
  }
  if (rows_per_item != 64 && rows_per_item != 128) {
    dfl_set_error("%s: rows_per_item must be 64 or 128", who);
    return false;
  }
  if (!w->wp || !x || !items || !n_items || max_items < 1) {
    dfl_set_error("%s: null pointer (or max_items < 1)", who);
    return false;
  }
  a.wp = (const bf16x8 *)w->wp;
  a.expert16 = w_expert_stride / 16;
  a.wscale = (const char *)w->scale;
  a.xf = (const bf16x8 *)x;
  a.items = items;
  a.n_items = n_items;
  a.KS = K / 32;
  a.ntiles = N / 16;
  a.nunits = (a.ntiles + 1) / 2;
  return true;
}

template <int EPI>
void w4s_launch(const MoeW4SArgs &a, int max_items, hipStream_t st) {
  constexpr int NW = W4S_NW;
  const int ncg = (a.nunits + NW - 1) / NW;
  hipLaunchKernelGGL((k_moe_w4_shared<EPI>), dim3((max_items + 7) / 8 * 8 * ncg), dim3(NW * 64), 0, st, a);
}

}  // namespace

int dfl_moe_grouped_gate_up_w4(const char *who, const dfl_weight *w, int64_t w_expert_stride, const void *xg, const int32_t *items,
                               const int32_t *n_items, int max_items, int I, int K, void *act_g, int rows_per_item,
                               const int32_t *src_row, const void *zeros_1k, void *stream) {
  MoeW4SArgs a{};
  if (!w4s_fill(a, who, w, w_expert_stride, xg, items, n_items, max_items, 2 * I, K, "K", rows_per_item)) return DFL_EINVAL;
  DFL_REQUIRE(I % 32 == 0, "%s: DFL_W_MXFP4 needs I %% 32 == 0 (act_g's frag16 tiles are 32 columns deep; I=%d)", who, I);
  DFL_REQUIRE(!src_row == !zeros_1k, "%s: src_row and zeros_1k come together", who);
  DFL_REQUIRE(act_g, "%s: null pointer", who);
  a.src_row = src_row;
  a.act = (bf16x8 *)act_g;
  a.KSo = I / 32;
  w4s_launch<W4S_SILU>(a, max_items, (hipStream_t)stream);
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}

int dfl_moe_grouped_down_w4(const char *who, const dfl_weight *w, int64_t w_expert_stride, const void *act_g, const int32_t *items,
                            const int32_t *n_items, int max_items, int H, int I, const float *row_w, float *out32,
                            int rows_per_item, void *stream) {
  MoeW4SArgs a{};
  if (!w4s_fill(a, who, w, w_expert_stride, act_g, items, n_items, max_items, H, I, "I", rows_per_item)) return DFL_EINVAL;
  DFL_REQUIRE(row_w && out32, "%s: null pointer", who);
  a.row_w = row_w;
  a.out32 = out32;
  a.ld32 = H;
  w4s_launch<W4S_SCALE32>(a, max_items, (hipStream_t)stream);
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}
