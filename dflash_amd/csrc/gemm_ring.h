// Ragged-batch GEMM, second form (round 4): waves OWN column tiles and walk K themselves; the activations of the
// R <= 4 request tiles stream through an LDS ring that every wave of the workgroup reads.
//
// Why: the first form (gemm_batch.hip: k_gemm_b) keeps the activations in registers, which at
// four request tiles allows a 2048-wide K part per workgroup — so K is cut over grid.y and the fused epilogues (SiLU*up,
// argmax) get their finished sums through fp32 slabs in HBM, an arrival ticket and a combine phase in the last workgroup
// to arrive (measured, round 3: lm_head 1.13 x its bytes and 0.65 of the HBM peak, gate/up 1.155 x and 0.60, and every
// launch starts with 256 KB of activation loads per workgroup in front of its first MFMA).  Here:
//   * a wave owns TPU column tiles (one tile, or a gate/up pair) and 1/KQ of every K chunk; its accumulators are the
//     FINISHED sums of (tile, request) over its k-steps, so there is no K cut over workgroups, no slab, no ticket, no
//     combine — at most one KQ-way sum through LDS at the very end (gate/up: KQ = 4);
//   * weights go HBM -> VGPR -> MFMA as before (packed fragments, nt buffer loads clipped at the tile's K), A chunks of
//     the wave's own k-steps in flight;
//   * the activations of a chunk (CK k-steps x MT requests x 1 KiB fragments, already in MFMA B-operand order: the
//     frag16 layout) enter LDS ONCE per workgroup by LDS-DMA (global_load_lds_dwordx4, lane-linear image, conflict-free
//     ds_read_b128), A chunks ahead of their use in a ring of A + 1 slots; every wave issues its share of the pieces.
//     What must be buffered is set by the weights in flight: F bytes of weights over U tiles cover F / U k-steps of K,
//     whose activations (MT KiB per k-step) have to be in LDS — gate/up at 4 tiles: 96..144 KB of weights in flight per
//     CU over 6 tiles = 16..24 k-steps = 64..96 KB of ring (why the small-N projections stay on the
//     register-resident form);
//   * one s_barrier per chunk; every load of the loop is unconditional with a constant count per iteration, so that
//     the in-order vmcnt of a wave can be waited on by immediates: at the top of iteration c the wave's DMA pieces of
//     chunk c are older than exactly A * KPC * TPU weight loads + (A - 1) * SP pieces.
// The compiler must not see the LDS reads of the ring: behind an LDS read that "may alias" LDS-DMA requests in flight
// hipcc waits vmcnt for the youngest of them (SIInsertWaitcnts), i.e. for the chunk just requested.  They are inline
// asm with their own lgkmcnt wait.
#pragma once
#include "gemm_rows.h"
#include "dfl_rng.h"

// (External linkage for the argument struct and the kernel template: hipFuncSetAttribute — more than 64 KB of dynamic
// LDS — needs the kernel's address, and the host-side handle of a kernel with internal linkage is not emitted.)
struct GemmRArgs {
  const bf16x8 *wp;  // packed weights [ntiles][KS][64]
  const bf16x8 *xf;  // frag16 activations of request 0 [KS][64]; request r at + r * frag_stride8
  int64_t frag_stride8;
  int KS, ntiles;
  int nunits;  // tiles (TPU = 1) or gate/up pairs (TPU = 2)
  int upp;     // units per workgroup and pass (<= NW / KQ)
  int npass;   // passes over K per workgroup (lm_head: its 37-38 tiles in 3 passes of 13)
  const int32_t *dyn;  // [MT][DFL_DYN_WORDS]
  // EPI_SILU
  bf16_t *act;  // frag16 [I/8][16][8] per request
  int64_t act_stride;
  // EPI_ARGMAX
  int row0, nrows, nrows_word;
  float *best_val;  // [gridDim.x][MT][16]
  int *best_idx;
  bf16_t *logits;  // optional [16][N] per request
  int64_t logits_stride;
  int N;
  // EPI_SAMPLE (with the EPI_ARGMAX fields): tile mt is tile j = mt % tiles_per_req of request q = mt / tiles_per_req; its
  // row m draws position base + pos_add + 16 j + m with base = dyn[mt][pos_word] and the seed seeds[q] (dfl_rng.h);
  // the DRAFT stream takes extra = base (the block start), the TARGET stream extra = 0
  const int64_t *seeds;
  float inv_t;
  int rng_stream, pos_word, pos_add, tiles_per_req;
  // EPI_SAMPLE_T (with the EPI_SAMPLE fields but inv_t): request slot q draws at invT = inv_ts[q]; a slot whose value is
  // not > 0 (0, negative, NaN) takes the plain argmax of EPI_ARGMAX: no Philox call, no noise
  const float *inv_ts;
  // W8 (wp: e4m3 codes [ntiles][KS / 2][64 lanes][16 B]): fp32 scale per column in packed tile order, 64-byte aligned
  const float *wscale;
};

namespace {
typedef __attribute__((address_space(3))) void r_lds_void;
typedef __attribute__((address_space(1))) void r_glb_void;

constexpr int R_CK = 8;  // k-steps per ring slot
}  // namespace

// MT request tiles, TPU tiles per unit, KQ waves per unit (each takes R_CK / KQ k-steps of every chunk), NW waves per
// workgroup, A chunks of look-ahead (weights in flight per wave: A * R_CK / KQ * TPU KiB; ring: A + 1 slots)
// W8: the weights are e4m3 codes, one 16-byte word per lane carrying the k-steps 2j and 2j + 1
// (gemm_rows.h).  A wave's share of a chunk — KPC k-steps from kc * 8 + q * KPC, a whole number of aligned pairs — is
// KPC / 2 loads, kept as raw words and converted in front of each of the two MFMAs a word feeds; the finished fp32 sums
// are multiplied by the columns' scales in front of the epilogue's first rounding.  Half the loads per chunk: VMC below.
template <int MT, int TPU, int KQ, int NW, int A, int EPI, bool W8 = false>
__global__ __launch_bounds__(NW * 64) void dfl_k_gemm_r(GemmRArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)  // the host pass needs the kernel's handle only; with this body it drops the instantiation (no diagnostic)
  constexpr int CK = R_CK, KPC = CK / KQ, NS = A + 1;
  constexpr int NPIECE = CK * MT;                 // 1 KiB pieces per chunk
  constexpr int SP = (NPIECE + NW - 1) / NW;      // pieces per wave and chunk (surplus: a duplicate of the last piece)
  constexpr int WPC = W8 ? KPC / 2 : KPC;         // weight loads per chunk and tile (W8: one word per k-step pair)
  constexpr int VMC = A * WPC * TPU + (A - 1) * SP;  // VMEM ops of a wave younger than its pieces of the chunk it is about to read
  static_assert(!W8 || KPC % 2 == 0, "W8: a wave's share of a chunk is whole k-step pairs");
  static_assert(!W8 || KQ == 1 || MT <= KQ, "W8: a wave finishes at most one (unit, request) item: upp * MT <= NW");
  constexpr bool ARG = EPI == EPI_ARGMAX || EPI == EPI_SAMPLE || EPI == EPI_SAMPLE_T;  // a running (perturbed) argmax per row
  static_assert(EPI == EPI_SILU || ARG, "the ring form has the SiLU epilogue and the three argmax ones");
  static_assert(CK % KQ == 0 && VMC < 64, "chunk split / vmcnt immediate");
  static_assert(NS * NPIECE * 1024 <= 160 * 1024, "ring exceeds LDS");
  static_assert(NW * TPU * MT * 1024 <= 160 * 1024 || KQ == 1, "the final KQ-way sum reuses the ring's LDS (ring_lds_bytes)");
  extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];  // [NS][NPIECE][1024]

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63;
  const int fm = l & 15, fg = l >> 4;  // D layout: row m, columns 4 fg .. 4 fg + 3
  const int u = w / KQ, q = w - u * KQ;
  const int nch = (a.KS + CK - 1) / CK;  // every workgroup walks the whole K, chunk c at k-steps [c * CK, c * CK + CK)
  const int nit = (nch + A - 1) / A * A;  // chunk iterations, rounded up to the unroll (clipped weights: zeros)
  const unsigned ring_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)ring;

  int arg_rows[MT];
  float best[MT];
  int bestn[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    best[mt] = -INFINITY;
    bestn[mt] = 0x7fffffff;
    arg_rows[mt] = 0;
    if (ARG && EPI != EPI_SAMPLE_T) {  // (EPI_SAMPLE_T reads the count in its epilogue: four fewer SGPRs across the K walk)
      arg_rows[mt] = a.nrows;
      if (a.dyn && a.nrows_word >= 0) arg_rows[mt] = a.dyn[mt * DFL_DYN_WORDS + a.nrows_word] - a.row0;
    }
  }

  // this wave's pieces of a chunk: piece i = (k-step f = i / MT, request mt = i % MT) -> LDS slot offset i * 1024.
  // NW % MT == 0: all pieces of a wave belong to ONE request, i.e. one buffer descriptor (clipped at K: a k-step past
  // it reads as zeros and costs no traffic).  The buffer form of the LDS-DMA, not global_load_lds: behind a FLAT-encoded
  // instruction that may touch LDS hipcc flushes vmcnt to ZERO at the next register dependency ("pending flat"),
  // i.e. it would wait for the chunks just requested before the first MFMA of every iteration.
  static_assert(NW % MT == 0, "a wave's pieces share a request");
  const int pmt = w % MT;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16x8 *>(a.xf + pmt * a.frag_stride8), 0, a.KS * 1024, 0x00020000);
  int pks[SP], poff[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    int i = w + s * NW;
    i = i < NPIECE ? i : i - NW;  // surplus: the wave's previous piece again (same bytes to the same place)
    pks[s] = i / MT;
    poff[s] = i * 1024;
  }
  // A pass runs nit >= nch iterations (the unroll's multiple): iterations >= nch are padding (k-steps past K: zeros).
  // (Every workgroup starts at chunk 0.  A start rotated by workgroup, (b * m) % chunks, was measured at 4 tiles: gate/up
  // 37.3 us unrotated against 39.8 / 38.9 / 39.5 at m = 1 / 3 / 5, lm_head 221 - 222 us either way
  // (profiles/r4_ring_microbench.txt) — HBM channel camping is not what limits the walk, and workgroups in step share
  // each activation chunk's L2 lines.)
  auto kchunk = [&](int c) { return c < nch ? c : nch; };
  int slot_w = 0, slot_r = 0;  // ring slots of the next stage() / the next chunk to compute (cycle 0 .. NS - 1)
  auto stage = [&](int kc) {   // data chunk kc -> the next ring slot
    const unsigned slot = ring_base + (unsigned)slot_w * (NPIECE * 1024);
    slot_w = slot_w + 1 == NS ? 0 : slot_w + 1;
#pragma unroll
    for (int s = 0; s < SP; ++s)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (r_lds_void *)(uintptr_t)(slot + poff[s]), 16, l * 16, (kc * CK + pks[s]) * 1024, 0, 0);
  };
  // the wave's unit of pass p: weights base of its TPU tiles and their K extent in bytes (0: no unit — zeros, no traffic)
  constexpr bool CONT = KQ == 1;  // passes run as ONE pipeline: the last A iterations of a pass request the next pass's first chunks
  auto unit_of = [&](int p, const bf16x8 *(&base)[TPU], int &bytes, int &g) {
    g = (int)blockIdx.x + (p * a.upp + u) * (int)gridDim.x;
    const bool have = p < a.npass && u < a.upp && g < a.nunits;
#pragma unroll
    for (int tp = 0; tp < TPU; ++tp) base[tp] = a.wp + (size_t)(have ? TPU * g + tp : 0) * a.KS * (W8 ? 32 : 64);
    bytes = have ? a.KS * (W8 ? 512 : 1024) : 0;
  };
  // W8: the scales of the tiles whose sums this wave FINISHES in pass p — its own unit's (KQ = 1), or those of the item
  // (unit slot w / MT, request w % MT) it takes after the KQ-way sum — 16 per tile by one scalar load (gemm_rows.h:
  // no VMEM operation, the counts above stand), requested right behind the pass's first weights (in front of them the
  // scalar wait for a descriptor word would wait for the scales too)
  auto scales_of = [&](int p, f32x16(&sc)[TPU]) {
    const int uu = KQ == 1 ? u : w / MT;
    const int g = (int)blockIdx.x + (p * a.upp + uu) * (int)gridDim.x;
    const bool have = p < a.npass && (KQ == 1 ? u < a.upp : w < a.upp * MT) && g < a.nunits;
#pragma unroll
    for (int tp = 0; tp < TPU; ++tp) sc[tp] = tile_scales(a.wscale, have ? TPU * g + tp : 0);
  };
  f32x16 scur[TPU], snxt[TPU];
  bf16x8 wreg[A][WPC][TPU];
  // weights of data chunk kc for this wave: k-steps kc * CK + q * KPC + j of the unit's tiles (W8: the pair j)
  auto wload1 = [&](bf16x8(&dst)[TPU], const bf16x8 *const(&base)[TPU], int bytes, int kc, int j) {
    const int soff = W8 ? ((kc * CK + q * KPC) / 2 + j) * 1024 : (kc * CK + q * KPC + j) * 1024;
#pragma unroll
    for (int tp = 0; tp < TPU; ++tp) {
      const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8 *>(base[tp]), 0, bytes, 0x00020000);
      dst[tp] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(wr, l * 16, soff, 2));
    }
  };
  auto wload = [&](bf16x8(&dst)[WPC][TPU], const bf16x8 *const(&base)[TPU], int bytes, int kc) {
#pragma unroll
    for (int j = 0; j < WPC; ++j) wload1(dst[j], base, bytes, kc, j);
  };

  const bf16x8 *wcur[TPU], *wnxt[TPU];
  int bcur, bnxt, gcur, gnxt;
  unit_of(0, wcur, bcur, gcur);
  // ---- prologue: the first A chunks, pieces then weights per chunk (the order the immediates below assume)
#pragma unroll
  for (int c = 0; c < A; ++c) {
    stage(kchunk(c));
    __builtin_amdgcn_sched_barrier(0);
    wload(wreg[c], wcur, bcur, kchunk(c));
    __builtin_amdgcn_sched_barrier(0);
  }
  if constexpr (W8) scales_of(0, scur);

  for (int p = 0; p < a.npass; ++p) {
    unit_of(CONT ? p + 1 : a.npass, wnxt, bnxt, gnxt);  // (not CONT: nothing is requested across a pass boundary)
    if constexpr (W8 && CONT) scales_of(p + 1, snxt);   // with the next pass's weights, not behind this K walk
    f32x4 acc[TPU][MT];
#pragma unroll
    for (int tp = 0; tp < TPU; ++tp)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[tp][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < nit; c0 += A) {
#pragma unroll
      for (int ca = 0; ca < A; ++ca) {
        const int c = c0 + ca;
        // this wave's pieces of the chunk it is about to read have landed ...
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");
        // ... and everyone's; every wave has finished reading the chunk before, whose slot the next request takes
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // A chunks ahead: this pass's chunk c + A, or (one pipeline over the passes) the next pass's chunk c + A - nit
        const int cn = c + A;
        const bool nx = cn >= nit;
        const int kcn = nx ? (CONT && p + 1 < a.npass ? kchunk(cn - nit) : nch) : kchunk(cn);
        stage(kcn);
        __builtin_amdgcn_sched_barrier(0);
        // (uniform selects, not a branch: loads under a branch cost the counted waits)
        const bf16x8 *wsel[TPU];
#pragma unroll
        for (int tp = 0; tp < TPU; ++tp) wsel[tp] = nx ? wnxt[tp] : wcur[tp];
        const int bsel = nx ? bnxt : bcur;
        const unsigned rd = ring_base + (unsigned)slot_r * (NPIECE * 1024) + (unsigned)(q * KPC * MT) * 1024 + l * 16;
        slot_r = slot_r + 1 == NS ? 0 : slot_r + 1;
#pragma unroll
        for (int j = 0; j < KPC; ++j) {
          bf16x8 b[MT];
          if constexpr (MT == 4) {
            asm volatile(
                "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\t"
                "ds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                : "v"(rd + j * MT * 1024)
                : "memory");
          } else if constexpr (MT == 2) {
            asm volatile(
                "ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(b[0]), "=&v"(b[1])
                : "v"(rd + j * MT * 1024)
                : "memory");
          } else {
            asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(b[0]) : "v"(rd + j * MT * 1024) : "memory");
          }
          if constexpr (W8) {
#pragma unroll
            for (int tp = 0; tp < TPU; ++tp) {
              const bf16x8 wf = w8_frag(wreg[ca][j >> 1][tp], j & 1);
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                acc[tp][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, b[mt], acc[tp][mt], 0, 0, 0);
            }
            if (j & 1) {  // both k-steps of the word are consumed: it takes the same pair of the chunk A ahead
              __builtin_amdgcn_sched_barrier(0);
              wload1(wreg[ca][j >> 1], wsel, bsel, kcn, j >> 1);
              __builtin_amdgcn_sched_barrier(0);
            }
          } else {
#pragma unroll
            for (int tp = 0; tp < TPU; ++tp)
#pragma unroll
              for (int mt = 0; mt < MT; ++mt)
                acc[tp][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wreg[ca][j][tp], b[mt], acc[tp][mt], 0, 0, 0);
            // the registers just consumed take the same k-step of the chunk A ahead at once (past K: clipped, zeros, no
            // traffic): the wave keeps A chunks of weights in flight all the time, not A - 1 while it computes
            __builtin_amdgcn_sched_barrier(0);
            wload1(wreg[ca][j], wsel, bsel, kcn, j);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    }

    // ---- finished sums of (unit, request): KQ-way sum through LDS, then the fused epilogue in the MFMA D layout
    auto epilogue = [&](int t_last, int mt, const f32x4 &s, const f32x4 &g4) {
      // s: sums of tile t_last (row fm, columns 4 fg .. + 3); SILU: g4 = the gate tile's sums, s = the up tile's
      const int n0 = (EPI == EPI_SILU ? (t_last >> 1) : t_last) * 16 + 4 * fg;
      if (EPI == EPI_SILU) {  // tf:modeling_qwen3.py:82, rounded where torch rounds
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gb = rbf(g4[r]), ub = rbf(s[r]);
          const float act = rbf(gb / (1.f + __expf(-gb)));
          o[r] = f2bf(act * ub);
        }
        *reinterpret_cast<bf16x4 *>(a.act + mt * a.act_stride + ((size_t)(n0 >> 3) * 16 + fm) * 8 + (n0 & 7)) = o;
      } else {  // EPI_ARGMAX, EPI_SAMPLE, EPI_SAMPLE_T
        int nlive = arg_rows[mt];
        if (EPI == EPI_SAMPLE_T) {
          nlive = a.nrows;
          if (a.dyn && a.nrows_word >= 0) nlive = a.dyn[mt * DFL_DYN_WORDS + a.nrows_word] - a.row0;
        }
        const bool live = (fm >= a.row0) && (fm < a.row0 + nlive);
        if (a.logits && live) {
          bf16x4 o = {f2bf(s[0]), f2bf(s[1]), f2bf(s[2]), f2bf(s[3])};
          *reinterpret_cast<bf16x4 *>(a.logits + mt * a.logits_stride + (size_t)fm * a.N + n0) = o;
        }
        uint32_t wd[4] = {0u, 0u, 0u, 0u};
        if (EPI == EPI_SAMPLE) {  // the thread's 4 columns are one column group: ONE Philox call covers them
          const int q = mt / a.tiles_per_req, j = mt - q * a.tiles_per_req;
          const int base = a.dyn[mt * DFL_DYN_WORDS + a.pos_word];
          dfl_rng_words((uint64_t)a.seeds[q], (uint32_t)a.rng_stream, (uint32_t)(base + a.pos_add + 16 * j + fm),
                        (uint32_t)n0, a.rng_stream == (int)DFL_RNG_DRAFT ? (uint32_t)base : 0u, wd);
        }
        // EPI_SAMPLE_T: the same draw at the tile's own invT (wave-uniform: one scalar load per tile and pass, as the
        // seed's) under a uniform branch; a greedy tile skips it whole and compares what EPI_ARGMAX compares
        float pv[4] = {0.f, 0.f, 0.f, 0.f};
        if (EPI == EPI_SAMPLE_T) {
#pragma unroll
          for (int r = 0; r < 4; ++r) pv[r] = rbf(s[r]);
          const int q = mt >> (a.tiles_per_req - 1), j = mt & (a.tiles_per_req - 1);  // (tiles_per_req is 1 or 2)
          const float inv_t = a.inv_ts[q];
          if (inv_t > 0.f) {
            const int base = a.dyn[mt * DFL_DYN_WORDS + a.pos_word];
            dfl_rng_words((uint64_t)a.seeds[q], (uint32_t)a.rng_stream, (uint32_t)(base + a.pos_add + 16 * j + fm),
                          (uint32_t)n0, a.rng_stream == (int)DFL_RNG_DRAFT ? (uint32_t)base : 0u, wd);
#pragma unroll
            for (int r = 0; r < 4; ++r) pv[r] = dfl_perturb_w(pv[r], inv_t, wd[r]);
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // lm_head output is bf16 before argmax (model/dflash.py:238,247); first maximum kept
          float vb = EPI == EPI_SAMPLE_T ? pv[r] : rbf(s[r]);
          if (EPI == EPI_SAMPLE) vb = dfl_perturb_w(vb, a.inv_t, wd[r]);  // Gumbel-max (dfl_rng.h)
          if (live && (vb > best[mt] || (vb == best[mt] && n0 + r < bestn[mt]) || bestn[mt] == 0x7fffffff)) {
            best[mt] = vb;
            bestn[mt] = n0 + r;
          }
        }
      }
    };

    if constexpr (KQ == 1) {
      if (bcur) {  // (the wave has a unit in this pass)
        if constexpr (W8) {  // sum * scale, in front of every rounding of the epilogue
          const f32x4 sl = lane_scales(scur[TPU - 1], fg), s0 = lane_scales(scur[0], fg);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) epilogue(TPU * gcur + TPU - 1, mt, acc[TPU - 1][mt] * sl, acc[0][mt] * s0);
        } else {
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) epilogue(TPU * gcur + TPU - 1, mt, acc[TPU - 1][mt], acc[0][mt]);
        }
      }
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (padding pieces past the last chunk still target the ring)
      __builtin_amdgcn_s_barrier();                     // every wave has left the ring
      asm volatile("" ::: "memory");
      float *red = reinterpret_cast<float *>(ring);     // [NW][TPU][MT][256]
#pragma unroll
      for (int tp = 0; tp < TPU; ++tp)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4 *>(&red[((w * TPU + tp) * MT + mt) * 256 + l * 4]) = acc[tp][mt];
      __syncthreads();
      for (int it = w; it < a.upp * MT; it += NW) {  // item = (unit slot, request)
        const int uu = it / MT, mt = it - uu * MT;
        const int gg = (int)blockIdx.x + (p * a.upp + uu) * (int)gridDim.x;
        if (gg >= a.nunits) continue;
        f32x4 s[TPU];
#pragma unroll
        for (int tp = 0; tp < TPU; ++tp) {
          s[tp] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int qq = 0; qq < KQ; ++qq)  // fixed order: deterministic sums
            s[tp] += *reinterpret_cast<const f32x4 *>(&red[(((uu * KQ + qq) * TPU + tp) * MT + mt) * 256 + l * 4]);
          if constexpr (W8) s[tp] *= lane_scales(scur[tp], fg);  // behind the KQ-way sum (it == w: scales_of's item)
        }
        epilogue(TPU * gg + TPU - 1, mt, s[TPU - 1], s[0]);
      }
      __syncthreads();
    }
    // ---- the next pass
#pragma unroll
    for (int tp = 0; tp < TPU; ++tp) wcur[tp] = wnxt[tp];
    bcur = bnxt;
    gcur = gnxt;
    if constexpr (W8 && CONT) {
#pragma unroll
      for (int tp = 0; tp < TPU; ++tp) scur[tp] = snxt[tp];
    }
    if (!CONT && p + 1 < a.npass) {  // the ring was reused for the sums: a prologue of its own
      unit_of(p + 1, wcur, bcur, gcur);
      slot_r = slot_w;
#pragma unroll
      for (int c = 0; c < A; ++c) {
        stage(kchunk(c));
        __builtin_amdgcn_sched_barrier(0);
        wload(wreg[c], wcur, bcur, kchunk(c));
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (W8) scales_of(p + 1, scur);
    }
  }

  if (ARG) {
    // the waves' candidates per (request, row) meet in LDS: ONE entry per workgroup goes out (the finish kernel scans
    // gridDim.x entries per row, not gridDim.x * NW: 30 us -> 5 us at 256 x 16)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (padding pieces past the last chunk still target the ring)
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    float *cv = reinterpret_cast<float *>(ring);             // [NW][MT][16]
    int *ci = reinterpret_cast<int *>(ring) + NW * MT * 16;  // [NW][MT][16]
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float bv = best[mt];
      int bn = bestn[mt];
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {  // lanes of a row (same fm) differ in fg
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bn, o, 64);
        if (ov > bv || (ov == bv && oi < bn)) {
          bv = ov;
          bn = oi;
        }
      }
      if (fg == 0) {
        cv[(w * MT + mt) * 16 + fm] = bv;
        ci[(w * MT + mt) * 16 + fm] = bn;
      }
    }
    __syncthreads();
    if (tid < MT * 16) {
      float bv = -INFINITY;
      int bn = 0x7fffffff;
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) {
        const float ov = cv[ww * MT * 16 + tid];
        const int oi = ci[ww * MT * 16 + tid];
        if (oi != 0x7fffffff && (bn == 0x7fffffff || ov > bv || (ov == bv && oi < bn))) {
          bv = ov;
          bn = oi;
        }
      }
      a.best_val[(size_t)blockIdx.x * MT * 16 + tid] = bv;  // [gridDim.x][MT][16]
      a.best_idx[(size_t)blockIdx.x * MT * 16 + tid] = bn;
    }
  }
#endif
}

namespace {

template <int MT, int TPU, int KQ, int NW, int A>
constexpr int ring_lds_bytes() {
  const int ring = (A + 1) * R_CK * MT * 1024, red = KQ > 1 ? NW * TPU * MT * 1024 : 0;
  return ring > red ? ring : red;
}

// The ring form takes fragment sources (mode 0) whose K fits whole k-steps; the caller falls back to k_gemm_b otherwise.
inline bool ring_ok(const dfl_rows_batch *x, int K) { return x && x->r0.mode == 0 && x->r0.frag && K % 32 == 0 && K >= 256; }

}  // namespace
