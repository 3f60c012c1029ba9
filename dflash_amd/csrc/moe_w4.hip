// The sparse-MoE expert launches on OCP MXFP4 codes: dfl_moe_gate_up / dfl_moe_down with DFL_W_MXFP4 (moe.hip dispatches
// here; layout in include/dflash_hip.h, the 4-bit pieces in gemm_rows.h).  A source of its own,
// built without gfx950's packed fp32 instructions (build.py): the kernels' fp32 arithmetic is scalar-per-lane v_fma / v_mul.
#include "gemm_rows.h"

namespace {

// ---- W4: the experts as OCP MXFP4 (DFL_W_MXFP4 through dfl_moe_gate_up / dfl_moe_down; gemm_rows.h, dflash_hip.h) ----
// Kernels and argument structs of their own: the bf16, W8 and W13 instantiations (moe.hip) do not change by an instruction.
// Per expert the codes lie in the dense format's tile layout, [tiles][K/128][64 lanes][16 B], experts back to back; the
// e8m0 scales are an array of their own, [E][tiles][K/128][16 columns] dwords (byte d = k-step 4 j + d) — per tile the
// dense format's scale region, so load_ksteps_w4 reads both as it does for k_gemm_w4.
#ifndef DFL_MOE_W4_GU_PAIRS
#define DFL_MOE_W4_GU_PAIRS 1   // (gate, up) pairs per LDS meeting: 1 or 2.  Same box, 46 / 80 active experts of 30B-A3B: one
                                // pair 17.6 / 25.9 us, two pairs 18.8 / 26.3 us (profiles/mxfp4_experts_ab.txt) — two stays out
#endif
#ifndef DFL_MOE_W4_DOWN_CT
#define DFL_MOE_W4_DOWN_CT 2    // widest column-tile count per workgroup of the down launch: 2 or 4.  Under the target's 4 shares
                                // 2 tiles 13.5 / 20.0 us, 4 tiles (128 workgroups) 17.2 / 25.7 us; 4 tiles under 8 shares 12.0 /
                                // 16.8 us, but the share count is the whole target's (same file)
#endif

// list[i] of the active experts, i wave-uniform: ONE scalar load through the constant address space (the router wrote the
// list in an earlier launch).  As a vector load — what hipcc makes of a plain a.list[i] — the dependent request sits in
// the wave's vmcnt queue behind the weights in flight, and the address arithmetic of the next item waits for all of them.
__device__ __forceinline__ int list_at(const int32_t *list, int i) {
  typedef const __attribute__((address_space(4))) int32_t *cptr;
  return *(cptr)(uintptr_t)(list + __builtin_amdgcn_readfirstlane(i));
}

struct MoeGuArgs4 {
  const bf16x8 *wp;      // codes [E][2*npp tiles][KS/4][64 lanes][16 B], experts back to back
  const char *wscale;    // e8m0 [E][2*npp][KS/4][16 columns][4 B]
  const bf16x8 *xfrag;   // frag16 of the 16 normalised rows [KS][64]
  const int32_t *list, *n_active, *dyn;
  int valid_word;
  int KS, npp;           // K / 32 (<= 64, % 4 == 0), I / 16
  bf16_t *act;           // [E][16 * I] frag16 per expert
};

// Gate/up on 4-bit codes, K % 128 == 0, K <= 2048.  Wave w's four k-steps of a tile are exactly 16-byte word w of that
// tile, so a tile costs a wave ONE 16-byte non-temporal load and one scale dword (bf16: four loads, W8: two), the scale
// requested in front of the word it scales; w4_frag builds each k-step's fragment, block scale applied, right in front of
// its MFMA.  Same k-steps per wave in the same order, same 16-way sum, same rounding points and epilogue as the bf16
// form, and e2m1 * 2^n is exact in bf16: the bits of the bf16 launch on the dequantised weights.
// An item is 32 KB per workgroup at K = 2048 where the bf16 form's is 128 KB, so its barrier and LDS sum weigh four times
// as much.  PP = 2: one meeting serves the two adjacent pairs (p, p + 1) of an expert — four raw words in flight per
// wave (the bf16 form holds eight registers' worth), one barrier for both pairs, 512 finishing threads.  Each pair's
// per-wave sums and the order of its 16-way sum are those of PP = 1, so no bit moves.  An odd npp leaves the expert's
// last item with one pair: the second pair's descriptors are clipped to zero and its finishing threads store nothing.
// A dead item (past the workgroup's last) clips every descriptor.
template <int PP>
__global__ __launch_bounds__(1024) void k_moe_gate_up_w4(MoeGuArgs4 a) {
  __shared__ float red[2][16][2 * PP][256];
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
  const int nfw = __builtin_amdgcn_readfirstlane(4 * w < a.KS ? 4 : 0);   // (K % 128 == 0: a whole word or none)
  const int ipe = (a.npp + PP - 1) / PP;                                  // items per expert
  const int nitems = a.n_active[0] * ipe;
  const int words = a.KS >> 2;                                            // 1 KiB wave words (and 64-byte scale lines) per tile
  const int64_t tile = (int64_t)words * 64, expert = 2 * a.npp * tile;    // 16-byte units
  bf16x8 wA[2 * PP], wB[2 * PP], xr[4];
  uint32_t sA[2 * PP], sB[2 * PP];   // the tiles' scale dwords of this lane's column
  // (every request unconditional, a dummy past the end: see k_moe_down)
  auto issue = [&](bf16x8(&wv)[2 * PP], uint32_t(&sv)[2 * PP], int it) {
    const bool live = it < nitems;
    it = live ? it : nitems - 1;
    const int e = list_at(a.list, it / ipe), t0 = 2 * PP * (it % ipe);   // the item's first tile of the expert: gate tile of pair PP * q
    const bf16x8 *base = a.wp + e * expert + t0 * tile + w * 64;
    const char *sbase = a.wscale + (((int64_t)e * 2 * a.npp + t0) * words + w) * 64;
    const int nt = __builtin_amdgcn_readfirstlane(live && nfw ? min(2 * PP, 2 * a.npp - t0) : 0);   // (odd npp: the tail item has one pair)
    load_words_w4<2 * PP>(wv, sv, base, sbase, nt, words, l);
  };
  int it = blockIdx.x;
  if (it >= nitems) return;
  load_ksteps<4, 0>(xr, a.xfrag + 4 * w * 64, nfw, l);   // activations first: a wave's loads return in issue order
  issue(wA, sA, it);
  const int nv = (a.dyn && a.valid_word >= 0) ? a.dyn[a.valid_word] : 16;
  if ((l & 15) >= nv) {
#pragma unroll
    for (int f = 0; f < 4; ++f) xr[f] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  }
  int pos = 0;
  auto consume = [&](const bf16x8(&wv)[2 * PP], const uint32_t(&sv)[2 * PP], int itc) {
    const int buf = pos & 1;
    ++pos;
#pragma unroll
    for (int t = 0; t < 2 * PP; ++t) {   // gate tile, up tile (, gate tile, up tile)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int f = 0; f < 4; ++f)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w4_frag(wv[t], sv[t], f), xr[f], acc, 0, 0, 0);
      *reinterpret_cast<f32x4 *>(&red[buf][w][t][l * 4]) = acc;
    }
    __syncthreads();
    if (tid < 256 * PP) {  // thread (pair tid >> 8 of the item, row m, column nl): D layout as in k_moe_gate_up
      const int pp = tid >> 8, m = (tid >> 4) & 15, nl = tid & 15;
      const int idx = 4 * (m + 16 * (nl >> 2)) + (nl & 3);
      float sg = 0.f, su = 0.f;
#pragma unroll
      for (int ww = 0; ww < 16; ++ww) {
        sg += red[buf][ww][2 * pp][idx];
        su += red[buf][ww][2 * pp + 1][idx];
      }
      const float gb = rbf(sg), ub = rbf(su);   // the Linears' bf16 outputs
      const float act = rbf(gb / (1.f + __expf(-gb)));
      const int e = list_at(a.list, itc / ipe), p = PP * (itc % ipe) + pp, n = p * 16 + nl;
      if (PP == 1 || p < a.npp)
        a.act[(int64_t)e * (16 * 16 * a.npp) + ((size_t)(n >> 3) * 16 + m) * 8 + (n & 7)] = f2bf(act * ub);
    }
  };
  const int G = gridDim.x;
  for (; it < nitems; it += 2 * G) {
    issue(wB, sB, it + G);
    __builtin_amdgcn_sched_barrier(0);
    consume(wA, sA, it);
    __builtin_amdgcn_sched_barrier(0);
    issue(wA, sA, it + 2 * G);
    __builtin_amdgcn_sched_barrier(0);
    if (it + G < nitems) consume(wB, sB, it + G);
    __builtin_amdgcn_sched_barrier(0);
  }
}

struct MoeDownArgs4 {
  const bf16x8 *wd;     // codes [E][ntiles][KSe/4][64 lanes][16 B]
  int64_t wd_stride;    // 16-byte units per expert
  const char *wscale;   // e8m0 [E][ntiles][KSe/4][16 columns][4 B]
  const bf16x8 *act;    // [E] frag16 [KSe][64]
  int64_t act_stride;   // bf16x8 units per expert
  const bf16_t *wt;     // [16][E]
  const int32_t *list, *n_active;
  int E, KSe, ntiles;
  float *out;           // [nsplit][16][ldo]
  int ldo;
};

// Down on 4-bit codes, I % 128 == 0.  An item is k_moe_down's (expert, chunk of 4 k-steps): per column tile ONE 16-byte
// word and one scale dword (column l & 15, group ks0 / 4), requested with the item behind the routing weight and the
// activations; the block scale rides in the conversion, so `total += acc * wr` stands exactly as in the bf16 form and
// the launch gives the bf16 launch's bits on the dequantised weights.  At 4 bits the item's activation fragments (4 KB,
// re-read from L2) outweigh a tile's weights (1 KB): CT = 4 shares them between four column tiles.  A tile's sums do not
// depend on CT.
template <int CT>
__global__ __launch_bounds__(1024) void k_moe_down_w4(MoeDownArgs4 a) {
  constexpr int NW = 16;
  __shared__ float red[NW][CT][256];
  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), l = tid & 63;
  const int t0 = blockIdx.x * CT, split = blockIdx.y, nsplit = gridDim.y;
  const int n = *a.n_active;
  const int per = (n + nsplit - 1) / nsplit;
  const int p0 = split * per, p1 = min(n, p0 + per);
  const int cpe = a.KSe >> 2;   // chunks (= words per tile) per expert
  const int nitems = (p1 > p0 ? p1 - p0 : 0) * cpe;
  f32x4 total[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) total[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  bf16x8 wA[CT], xA[4], wB[CT], xB[4];
  uint32_t sA[CT], sB[CT];
  bf16_t rA = 0, rB = 0;
  // (every request unconditional, a dummy past the end: see k_moe_down)
  auto issue = [&](bf16x8(&wv)[CT], uint32_t(&sv)[CT], bf16x8(&xv)[4], bf16_t &wr, int it) {
    const bool live = it < nitems;
    it = live ? it : nitems - 1;
    const int e = list_at(a.list, p0 + it / cpe), ch = it % cpe;
    const int nf = __builtin_amdgcn_readfirstlane(live ? 4 : 0);
    // the routing weight of this lane's row; first: loads return in order.  Through a descriptor that a dead item clips
    // to zero: its consume() then adds 0 * 0 and needs no guard (see the loop)
    const __amdgpu_buffer_rsrc_t rt =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t *>(a.wt), 0, live ? 16 * a.E * (int)sizeof(bf16_t) : 0, 0x00020000);
    wr = __builtin_bit_cast(bf16_t, __builtin_amdgcn_raw_buffer_load_b16(rt, (l & 15) * a.E * (int)sizeof(bf16_t),
                                                                         e * (int)sizeof(bf16_t), 0));
    load_ksteps<4, 0>(xv, a.act + e * a.act_stride + (size_t)ch * 256, nf, l);  // re-read by every column group: L2
    const int64_t word = (int64_t)t0 * cpe + ch;   // word ch of the workgroup's first tile; the others cpe words further each
    load_words_w4<CT>(wv, sv, a.wd + e * a.wd_stride + word * 64, a.wscale + ((int64_t)e * a.ntiles * cpe + word) * 64,
                      nf ? CT : 0, cpe, l);
  };
  auto consume = [&](const bf16x8(&wv)[CT], const uint32_t(&sv)[CT], const bf16x8(&xv)[4], bf16_t wraw) {
    const float wr = bf2f(wraw);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int f = 0; f < 4; ++f)
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w4_frag(wv[c], sv[c], f), xv[f], acc, 0, 0, 0);
      total[c] += acc * wr;
    }
  };
  int it = w;
  if (it < nitems) {
    issue(wA, sA, xA, rA, it);
    for (; it < nitems; it += 2 * NW) {
      issue(wB, sB, xB, rB, it + NW);
      __builtin_amdgcn_sched_barrier(0);
      consume(wA, sA, xA, rA);
      __builtin_amdgcn_sched_barrier(0);
      issue(wA, sA, xA, rA, it + 2 * NW);
      __builtin_amdgcn_sched_barrier(0);
      // (unconditional: behind `if (it + NW < nitems)` hipcc sinks the CT = 4 form's requests for B into the branch, below
      // A's waits and MFMAs; a dead B is zero codes, zero activations and a zero routing weight)
      consume(wB, sB, xB, rB);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) *reinterpret_cast<f32x4 *>(&red[w][c][l * 4]) = total[c];
  __syncthreads();
  for (int o = tid; o < 256 * CT; o += NW * 64) {
    const int c = o >> 8, m = (o >> 4) & 15, nl = o & 15;
    const int idx = 4 * (m + 16 * (nl >> 2)) + (nl & 3);
    float s = 0.f;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) s += red[ww][c][idx];
    a.out[((size_t)split * 16 + m) * a.ldo + (t0 + c) * 16 + nl] = s;
  }
}

}  // namespace

int dfl_moe_gate_up_w4(const char *who, const dfl_weight *w, const void *x_frag, int E, int I, int K, void *act_frag,
                       const int32_t *list, const int32_t *n_active, const int32_t *dyn, int valid_word, void *stream) {
  if (!w4_scales_ok(who, w)) return DFL_EINVAL;
  DFL_REQUIRE(w->wp && x_frag && act_frag && list && n_active, "%s: null pointer", who);
  DFL_REQUIRE(E >= 1 && E <= 1024 && I > 0 && I % 16 == 0, "%s: E=%d I=%d outside range", who, E, I);
  DFL_REQUIRE(K > 0 && K % 128 == 0 && K <= 2048,
              "%s: DFL_W_MXFP4 needs K %% 128 == 0 (a wave's share of a tile is one 4-k-step word) and K <= 2048 (K=%d)", who, K);
  MoeGuArgs4 a{};
  a.wp = (const bf16x8 *)w->wp;
  a.wscale = (const char *)w->scale;
  a.xfrag = (const bf16x8 *)x_frag;
  a.list = list;
  a.n_active = n_active;
  a.dyn = dyn;
  a.valid_word = valid_word;
  a.KS = K / 32;
  a.npp = I / 16;
  a.act = (bf16_t *)act_frag;
  hipLaunchKernelGGL((k_moe_gate_up_w4<DFL_MOE_W4_GU_PAIRS>), dim3(256), dim3(1024), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}

// wp_expert_stride: bytes of codes between experts
int dfl_moe_down_w4(const char *who, const dfl_weight *w, int64_t wp_expert_stride, const void *act_frag, int64_t act_expert_stride,
                const void *wt, const int32_t *list, const int32_t *n_active, int E, int N, int I, int nsplit, float *out,
                void *stream) {
  if (!w4_scales_ok(who, w)) return DFL_EINVAL;
  DFL_REQUIRE(w->wp && act_frag && wt && list && n_active && out, "%s: null pointer", who);
  DFL_REQUIRE(E >= 1 && N > 0 && I > 0 && N % 16 == 0 && nsplit >= 1 && nsplit <= 16, "%s: bad shape", who);
  DFL_REQUIRE(I % 128 == 0, "%s: DFL_W_MXFP4 needs I %% 128 == 0 (an item is one 4-k-step word per column tile; I=%d)", who, I);
  DFL_REQUIRE(wp_expert_stride >= (int64_t)N * I / 2 && wp_expert_stride % 16 == 0 && act_expert_stride >= (int64_t)16 * I &&
                  act_expert_stride % 8 == 0,
              "%s: expert strides too short", who);
  MoeDownArgs4 a{};
  a.wd = (const bf16x8 *)w->wp;
  a.wd_stride = wp_expert_stride / 16;
  a.wscale = (const char *)w->scale;
  a.act = (const bf16x8 *)act_frag;
  a.act_stride = act_expert_stride / 8;
  a.wt = (const bf16_t *)wt;
  a.list = list;
  a.n_active = n_active;
  a.E = E;
  a.KSe = I / 32;
  a.ntiles = N / 16;
  a.out = out;
  a.ldo = N;
  // the widest form whose column-tile count divides the launch's (DFL_MOE_W4_DOWN_CT at most)
#if DFL_MOE_W4_DOWN_CT == 4
  if (N % 64 == 0)
    hipLaunchKernelGGL((k_moe_down_w4<4>), dim3(N / 64, nsplit), dim3(1024), 0, (hipStream_t)stream, a);
  else
#endif
  if (N % 32 == 0)
    hipLaunchKernelGGL((k_moe_down_w4<2>), dim3(N / 32, nsplit), dim3(1024), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((k_moe_down_w4<1>), dim3(N / 16, nsplit), dim3(1024), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}
