// The ragged-batch GEMMs on OCP MXFP4 codes: dfl_gemm_f32_batch / dfl_gemm_silu_mul_batch / dfl_gemm_argmax_batch with
// DFL_W_MXFP4 (gemm_batch.hip dispatches here; layout in include/dflash_hip.h, the 4-bit pieces in gemm_rows.h, DESIGN.md
// section 17, "The batch forms").  A source of its own — kernels and argument structs — built like moe_w4.hip without
// gfx950's packed fp32 instructions (build.py), so that no instantiation of gemm_ring.h / gemm_batch.hip changes.
//
// The invariant that decides every work split below: BIT EQUALITY with the bf16 sibling on the dequantised weights.
// e2m1 * 2^n is exact in bf16, so both forms feed identical fragments to identical MFMAs; what is left is the fp32 order.
// Every accumulator chain here receives the k-steps its bf16 counterpart receives, ascending, and every cross-wave sum
// runs in the bf16 form's order.
//
// A 16-byte word of a lane holds FOUR k-steps of a column tile, so none of the bf16 wave maps carries over:
//   * ring, lm_head + argmax (dfl_k_gemm_r at KQ = 1): a wave owns a column tile and walks all of K — one chain per (tile,
//     request) as there; a chunk of 8 k-steps is two words and two scale dwords in place of eight loads;
//   * ring, gate/up + SiLU (dfl_k_gemm_r at KQ = 4, KPC = 2): the bf16 form gives (pair, request) the value
//     (((0 + P0) + P1) + P2) + P3, P_q one chain over k-steps 8c + 2q, 8c + 2q + 1 — half a word.  Here a unit (a gate/up
//     pair) is FOUR waves (tile tp, half h): the wave loads word 2c + h of its ONE tile and keeps two chains per request,
//     dwords 0, 1 -> P_{2h}, dwords 2, 3 -> P_{2h+1}.  (Two waves per unit, each with both tiles, would leave 6 waves on a
//     CU at the 8B shape — 3 units per workgroup — i.e. two SIMDs with twice the MFMAs of the others, and at 4 bits the
//     MFMA time of 4 request tiles is no longer small against the stream.)  The h = 0 wave sums (0 + P0) + P1 in its
//     registers; that and the raw P2, P3 meet in LDS, 3 partials per (tile, request) in place of 4, and the wave that
//     finishes the item adds + P2, + P3: the bf16 order.  Units per workgroup, NW (12 / 16) and passes are the bf16 plan's;
//   * register-resident K parts (k_gemm_b, EPI_F32): the bf16 form's K parts, grid and wave shares; a wave's nfr k-steps
//     arrive as nfr / 4 words.  Taken only where nfr = ceil(K / 32 / (8 ksplit)) is 4 or 8: shares are then whole aligned
//     words and every chain is the bf16 form's.  Other K are refused — rounding nfr up would move k-steps between waves.
// Weights go HBM -> VGPR -> MFMA as raw words; w4_frag (v_cvt_scalef32_pk_bf16_fp4, the block scale in the conversion, no
// epilogue multiply) runs right in front of the MFMAs of its k-step.  Activations move as in the bf16 siblings: the LDS
// ring filled by the buffer form of LDS-DMA and read by inline asm, or k_gemm_b's register-resident fragments.
//
// vmcnt of the ring form.  A wave's requests per chunk are SP pieces (LDS-DMA) and HW (scale dword, word) pairs, issued as
//   pieces(k), [scale, word] x HW of chunk k, pieces(k + 1), ...
// in the prologue (chunks 0 .. A - 1) and, in iteration c, pieces(c + A) then — behind the k-steps of each word — that word's
// successor A chunks ahead, scale first.  Every request is unconditional (a unit-less wave, a chunk past K and the padding
// iterations read through clipped descriptors: code 0 under scale code 0 = +0, no traffic), so at the top of iteration c the
// wave's pieces of chunk c are older than exactly  VMC = A * 2 * HW + (A - 1) * SP  requests: the weights of chunks
// c .. c + A - 1 (scale dwords count) and the pieces of chunks c + 1 .. c + A - 1.  No scale is requested behind the K walk:
// the next pass's first words (lm_head: the passes are one pipeline) bring theirs.
#include "gemm_rows.h"

// (External linkage for the argument struct and the kernel template: hipFuncSetAttribute needs the kernel's address.)
struct GemmR4Args {
  const bf16x8 *wp;    // codes [ntiles][KS / 4][64 lanes][16 B]
  const char *wscale;  // e8m0 [ntiles][KS / 4][16 columns][4 B], 64-byte aligned
  const bf16x8 *xf;    // frag16 activations of request 0 [KS][64]; request r at + r * frag_stride8
  int64_t frag_stride8;
  int KS, ntiles;      // K / 32 (% 4 == 0), column tiles
  int nunits, upp, npass;  // units (tiles, or gate/up pairs), units per workgroup and pass, passes
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
};

namespace {
typedef __attribute__((address_space(3))) void r4_lds_void;
constexpr int R4_CK = 8;  // k-steps per ring slot: two words of a tile
}  // namespace

// MT request tiles, NW waves per workgroup, A chunks of look-ahead (ring: A + 1 slots of 8 MT KiB)
template <int MT, int NW, int A, int EPI>
__global__ __launch_bounds__(NW * 64) void dfl_k_gemm_r4(GemmR4Args a) {
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass needs the kernel's handle only)
  static_assert(EPI == EPI_SILU || EPI == EPI_ARGMAX, "the 4-bit ring form has the SiLU and the argmax epilogue");
  constexpr bool SILU = EPI == EPI_SILU;
  constexpr int CK = R4_CK, NS = A + 1;
  constexpr int NPIECE = CK * MT;             // 1 KiB pieces per chunk
  constexpr int SP = (NPIECE + NW - 1) / NW;  // pieces per wave and chunk (surplus: a duplicate of the wave's last piece)
  constexpr int HW = SILU ? 1 : 2;            // words of a chunk per wave (SILU: the half h of its tile's two)
  constexpr int NC = SILU ? 2 : 1;            // accumulator chains per request
  constexpr int WPU = SILU ? 4 : 1;           // waves per unit
  constexpr int VMC = A * 2 * HW + (A - 1) * SP;  // derived in the head comment; scale dwords count
  constexpr bool CONT = !SILU;                // passes run as ONE pipeline (SILU reuses the ring for its sums)
  static_assert(VMC < 64, "vmcnt immediate");
  static_assert(NS * NPIECE * 1024 <= 160 * 1024, "ring exceeds LDS");
  static_assert(!SILU || NW * MT * 1536 <= 160 * 1024, "SILU: 3 partials x 2 tiles x MT KiB per unit of 4 waves");
  static_assert(!SILU || (NW / 4) * MT <= NW, "SILU: a wave finishes at most one (unit, request) item");
  static_assert(NW % MT == 0 && NW % WPU == 0, "a wave's pieces share a request; whole units");
  extern __shared__ __attribute__((aligned(1024))) unsigned char ring[];  // [NS][NPIECE][1024]

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63;
  const int fm = l & 15, fg = l >> 4;  // D layout: row m, columns 4 fg .. 4 fg + 3
  const int u = w / WPU, tp = SILU ? (w >> 1) & 1 : 0, h = SILU ? w & 1 : 0;
  const int words = a.KS >> 2;
  const int nch = (a.KS + CK - 1) / CK;  // every workgroup walks the whole K
  const int nit = (nch + A - 1) / A * A;
  const unsigned ring_base = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)ring;

  int arg_rows[MT];
  float best[MT];
  int bestn[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    best[mt] = -INFINITY;
    bestn[mt] = 0x7fffffff;
    arg_rows[mt] = 0;
    if (!SILU) {
      arg_rows[mt] = a.nrows;
      if (a.dyn && a.nrows_word >= 0) arg_rows[mt] = a.dyn[mt * DFL_DYN_WORDS + a.nrows_word] - a.row0;
    }
  }

  // this wave's pieces of a chunk (gemm_ring.h): piece i = (k-step i / MT, request i % MT) -> slot offset i * 1024
  const int pmt = w % MT;
  const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16x8 *>(a.xf + pmt * a.frag_stride8), 0, a.KS * 1024, 0x00020000);
  int pks[SP], poff[SP];
#pragma unroll
  for (int s = 0; s < SP; ++s) {
    int i = w + s * NW;
    i = i < NPIECE ? i : i - NW;
    pks[s] = i / MT;
    poff[s] = i * 1024;
  }
  auto kchunk = [&](int c) { return c < nch ? c : nch; };
  int slot_w = 0, slot_r = 0;
  auto stage = [&](int kc) {
    const unsigned slot = ring_base + (unsigned)slot_w * (NPIECE * 1024);
    slot_w = slot_w + 1 == NS ? 0 : slot_w + 1;
#pragma unroll
    for (int s = 0; s < SP; ++s)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(xr, (r4_lds_void *)(uintptr_t)(slot + poff[s]), 16, l * 16, (kc * CK + pks[s]) * 1024, 0, 0);
  };
  // the wave's tile of pass p, in words from the start of the codes (the scale lines run alongside); nw = 0: no unit
  auto unit_of = [&](int p, int &t64, int &nw, int &g) {
    g = (int)blockIdx.x + (p * a.upp + u) * (int)gridDim.x;
    const bool have = p < a.npass && u < a.upp && g < a.nunits;
    t64 = have ? (SILU ? 2 * g + tp : g) * words : 0;
    nw = have ? words : 0;
  };
  bf16x8 wreg[A][HW];
  uint32_t sreg[A][HW];
  // word j of data chunk kc for this wave — word 2 kc + h + j of its tile — and, in front of it, its scale dword
  auto wload1 = [&](bf16x8 &wd, uint32_t &sc, int t64, int nw, int kc, int j) {
    const int wi = 2 * kc + h + j;
    bf16x8 wv[1];
    uint32_t sv[1];
    load_words_w4<1>(wv, sv, a.wp + (size_t)(t64 + wi) * 64, a.wscale + (size_t)(t64 + wi) * 64, wi < nw ? 1 : 0, 1, l);
    wd = wv[0];
    sc = sv[0];
  };

  int tcur, tnxt, ncur, nnxt, gcur, gnxt;
  unit_of(0, tcur, ncur, gcur);
  auto prologue = [&]() {  // the first A chunks, pieces then weights per chunk: the order VMC counts
#pragma unroll
    for (int c = 0; c < A; ++c) {
      stage(kchunk(c));
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int j = 0; j < HW; ++j) wload1(wreg[c][j], sreg[c][j], tcur, ncur, kchunk(c), j);
      __builtin_amdgcn_sched_barrier(0);
    }
  };
  prologue();

  for (int p = 0; p < a.npass; ++p) {
    unit_of(CONT ? p + 1 : a.npass, tnxt, nnxt, gnxt);  // (not CONT: nothing is requested across a pass boundary)
    f32x4 acc[NC][MT];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[ch][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < nit; c0 += A) {
#pragma unroll
      for (int ca = 0; ca < A; ++ca) {
        const int c = c0 + ca;
        // this wave's pieces of the chunk it is about to read have landed ...
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VMC) : "memory");
        // ... and everyone's; every wave has finished reading the chunk before, whose slot the next request takes
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        const int cn = c + A;
        const bool nx = cn >= nit;
        const int kcn = nx ? (CONT && p + 1 < a.npass ? kchunk(cn - nit) : nch) : kchunk(cn);
        stage(kcn);
        __builtin_amdgcn_sched_barrier(0);
        const int tsel = nx ? tnxt : tcur, nsel = nx ? nnxt : ncur;  // (uniform selects, not a branch)
        const unsigned rd = ring_base + (unsigned)slot_r * (NPIECE * 1024) + (unsigned)(h * 4 * MT) * 1024 + l * 16;
        slot_r = slot_r + 1 == NS ? 0 : slot_r + 1;
#pragma unroll
        for (int j = 0; j < HW; ++j) {
#pragma unroll
          for (int d = 0; d < 4; ++d) {
            bf16x8 b[MT];
            const unsigned ra = rd + (unsigned)((j * 4 + d) * MT) * 1024;
            if constexpr (MT == 4) {
              asm volatile(
                  "ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\t"
                  "ds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072\n\t"
                  "s_waitcnt lgkmcnt(0)"
                  : "=&v"(b[0]), "=&v"(b[1]), "=&v"(b[2]), "=&v"(b[3])
                  : "v"(ra)
                  : "memory");
            } else {
              static_assert(MT == 2, "2 or 4 request tiles");
              asm volatile(
                  "ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\t"
                  "s_waitcnt lgkmcnt(0)"
                  : "=&v"(b[0]), "=&v"(b[1])
                  : "v"(ra)
                  : "memory");
            }
            const bf16x8 wf = w4_frag(wreg[ca][j], sreg[ca][j], d);
            const int ch = SILU ? d >> 1 : 0;  // (compile-time under the unroll)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
              acc[ch][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, b[mt], acc[ch][mt], 0, 0, 0);
          }
          // the word just consumed takes the same word of the chunk A ahead at once, its scale in front of it
          __builtin_amdgcn_sched_barrier(0);
          wload1(wreg[ca][j], sreg[ca][j], tsel, nsel, kcn, j);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    }

    // ---- the fused epilogues of the bf16 ring (gemm_ring.h), on the finished sums in the MFMA D layout
    auto epilogue = [&](int t_last, int mt, const f32x4 &s, const f32x4 &g4) {
      const int n0 = (SILU ? (t_last >> 1) : t_last) * 16 + 4 * fg;
      if (SILU) {  // tf:modeling_qwen3.py:82, rounded where torch rounds
        bf16x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gb = rbf(g4[r]), ub = rbf(s[r]);
          const float act = rbf(gb / (1.f + __expf(-gb)));
          o[r] = f2bf(act * ub);
        }
        *reinterpret_cast<bf16x4 *>(a.act + mt * a.act_stride + ((size_t)(n0 >> 3) * 16 + fm) * 8 + (n0 & 7)) = o;
      } else {
        const bool live = (fm >= a.row0) && (fm < a.row0 + arg_rows[mt]);
        if (a.logits && live) {
          bf16x4 o = {f2bf(s[0]), f2bf(s[1]), f2bf(s[2]), f2bf(s[3])};
          *reinterpret_cast<bf16x4 *>(a.logits + mt * a.logits_stride + (size_t)fm * a.N + n0) = o;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // lm_head output is bf16 before argmax; first maximum kept
          const float vb = rbf(s[r]);
          if (live && (vb > best[mt] || (vb == best[mt] && n0 + r < bestn[mt]) || bestn[mt] == 0x7fffffff)) {
            best[mt] = vb;
            bestn[mt] = n0 + r;
          }
        }
      }
    };

    if constexpr (!SILU) {
      if (ncur) {  // (the wave has a tile in this pass)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) epilogue(gcur, mt, acc[0][mt], acc[0][mt]);
      }
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (padding pieces past the last chunk still target the ring)
      __builtin_amdgcn_s_barrier();                     // every wave has left the ring
      asm volatile("" ::: "memory");
      float *red = reinterpret_cast<float *>(ring);     // [NW / 4 units][2 tiles][3][MT][256]
      float *mine = red + (size_t)((u * 2 + tp) * 3) * MT * 256 + l * 4;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        if (h == 0) {  // (0 + P0) + P1 in registers: the first two terms of the bf16 form's sum (0.f first: -0 matters)
          f32x4 s = {0.f, 0.f, 0.f, 0.f};
          s += acc[0][mt];
          s += acc[1][mt];
          *reinterpret_cast<f32x4 *>(mine + mt * 256) = s;
        } else {       // P2 and P3 as they are
          *reinterpret_cast<f32x4 *>(mine + (MT + mt) * 256) = acc[0][mt];
          *reinterpret_cast<f32x4 *>(mine + (2 * MT + mt) * 256) = acc[1][mt];
        }
      }
      __syncthreads();
      for (int it = w; it < a.upp * MT; it += NW) {  // item = (unit slot, request)
        const int uu = it / MT, mt = it - uu * MT;
        const int gg = (int)blockIdx.x + (p * a.upp + uu) * (int)gridDim.x;
        if (gg >= a.nunits) continue;
        f32x4 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const float *src = red + (size_t)((uu * 2 + t) * 3) * MT * 256 + mt * 256 + l * 4;
          s[t] = *reinterpret_cast<const f32x4 *>(src);               // (0 + P0) + P1
          s[t] += *reinterpret_cast<const f32x4 *>(src + MT * 256);      // + P2
          s[t] += *reinterpret_cast<const f32x4 *>(src + 2 * MT * 256);  // + P3
        }
        epilogue(2 * gg + 1, mt, s[1], s[0]);
      }
      __syncthreads();
    }
    // ---- the next pass
    tcur = tnxt;
    ncur = nnxt;
    gcur = gnxt;
    if (!CONT && p + 1 < a.npass) {  // the ring was reused for the sums: a prologue of its own
      unit_of(p + 1, tcur, ncur, gcur);
      slot_r = slot_w;
      prologue();
    }
  }

  if (!SILU) {
    // the waves' candidates per (request, row) meet in LDS: ONE entry per workgroup goes out (gemm_ring.h)
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

// ---- the register-resident K-part form: k_gemm_b<MT, EPI_F32> (gemm_batch.hip) on 4-bit words ----
struct GemmB4Args {
  const bf16x8 *wp;    // codes [ntiles][KS / 4][64 lanes][16 B]
  const char *wscale;  // e8m0 [ntiles][KS / 4][16 columns][4 B]
  RowSrc src;          // request 0; request r at the strides below
  int64_t frag_stride, rows_stride;
  const int32_t *dyn;  // [R][DFL_DYN_WORDS]
  int KS, ntiles, nfr;  // nfr: 4 or 8 k-steps per wave
  float *out;          // [ksplit][MT*16][ldo]
  int ldo;
};

// The bf16 kernel's shape: 8 waves x 8 k-steps of every request's tile in registers, K parts over grid.y, three rotating
// weight items.  An item is nfr / 4 words and their scale dwords (load_ksteps_w4: the scales in front, both clipped at the
// wave's share), i.e. 10 registers in place of 32: the MT = 4 kernel is far from the 256-VGPR edge its sibling lives at.
// A wave's chain: its k-steps ks0 .. ks0 + nfr - 1 ascending, then zeros — the bf16 form's; the 8 partial tiles meet in
// LDS and are summed from 0.f in wave order — the bf16 form's.
template <int MT>
__global__ __launch_bounds__(512) void k_gemm_b4(GemmB4Args a) {
  constexpr int FR = 8, NW = 8;
  __shared__ float red[2][NW][MT][256];

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63;
  const int ky = blockIdx.y;
  const int fm = l & 15, fg = l >> 4;

  RowSrc src[MT];
  int nv[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    src[mt] = a.src;
    if (a.src.frag) src[mt].frag = a.src.frag + (mt * a.frag_stride) / 8;
    if (a.src.rows) src[mt].rows = a.src.rows + mt * a.rows_stride;
    nv[mt] = (a.src.valid_word >= 0 && a.dyn) ? a.dyn[mt * DFL_DYN_WORDS + a.src.valid_word] : 16;
  }

  const int ks0 = (ky * NW + w) * a.nfr;  // % 4 == 0: the share starts at a word
  int nf0 = a.KS - ks0;
  nf0 = nf0 < 0 ? 0 : (nf0 > a.nfr ? a.nfr : nf0);  // % 4 == 0 as KS and nfr are

  const int stride = gridDim.x;
  const int nseq = (int)blockIdx.x < a.ntiles ? (a.ntiles - 1 - (int)blockIdx.x) / stride + 1 : 0;
  auto tile_of = [&](int j) -> int { return (int)blockIdx.x + j * stride; };
  // (live = false: a dummy request — empty descriptors, zeros, no traffic — see the main loop)
  auto load_item = [&](bf16x8(&wr)[2], uint32_t(&sc)[2], int t, bool live = true) {
    const size_t word0 = ((size_t)t * a.KS + ks0) >> 2;
    load_ksteps_w4<FR>(wr, sc, a.wp + word0 * 64, a.wscale + word0 * 64, live ? nf0 : 0, l);
  };

  bf16x8 xr[MT][FR];
  bf16x8 wA[2], wB[2], wC[2];
  uint32_t sA[2], sB[2], sC[2];
  if (nseq > 0) load_item(wA, sA, tile_of(0));
  if (nseq > 1) load_item(wB, sB, tile_of(1));
  {
    int ks[FR];
    bool take[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) {
      take[f] = f < nf0;
      ks[f] = take[f] ? ks0 + f : 0;
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) build_x<FR, false>(src[mt], ks, take, l, nv[mt], 1.f, xr[mt]);
  }

  f32x4 acc[MT];
  auto process = [&](const bf16x8(&wr)[2], const uint32_t(&sc)[2], int t, int pos) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int f = 0; f < FR; ++f) {  // k-steps past the wave's share: zero weights and zero activations
      const bf16x8 wf = w4_frag(wr[f >> 2], sc[f >> 2], f & 3);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xr[mt][f], acc[mt], 0, 0, 0);
    }
    const int buf = pos & 1;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4 *>(&red[buf][w][mt][l * 4]) = acc[mt];
    __syncthreads();
    if (w < MT) {  // wave mt finishes request mt's tile
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ww = 0; ww < NW; ++ww) s += *reinterpret_cast<const f32x4 *>(&red[buf][ww][w][l * 4]);
      *reinterpret_cast<f32x4 *>(a.out + ((size_t)(ky * MT + w) * 16 + fm) * a.ldo + t * 16 + 4 * fg) = s;
    }
  };

  // three rotating items, every request unconditional and pinned in front of the MFMAs (k_gemm_b: behind a branch hipcc
  // cannot count the loads in flight and waits for the item just requested)
  for (int j = 0; j < nseq; j += 3) {
    load_item(wC, sC, tile_of(j + 2 < nseq ? j + 2 : j), j + 2 < nseq);
    __builtin_amdgcn_sched_barrier(0);
    process(wA, sA, tile_of(j), j);
    if (j + 1 >= nseq) break;
    __builtin_amdgcn_sched_barrier(0);
    load_item(wA, sA, tile_of(j + 3 < nseq ? j + 3 : j), j + 3 < nseq);
    __builtin_amdgcn_sched_barrier(0);
    process(wB, sB, tile_of(j + 1), j + 1);
    if (j + 2 >= nseq) break;
    __builtin_amdgcn_sched_barrier(0);
    load_item(wB, sB, tile_of(j + 4 < nseq ? j + 4 : j), j + 4 < nseq);
    __builtin_amdgcn_sched_barrier(0);
    process(wC, sC, tile_of(j + 2), j + 2);
  }
}

// ---- host side ----
// Look-ahead A (chunks of 8 k-steps).  What bounds the bytes in flight here is the ring, not the registers: a chunk of a
// tile is 1 KiB of codes against 8 MT KiB of activations in LDS, so A is what 160 KiB of ring holds (MT = 4: 5 slots of
// 32 KiB) or what divides the 8B widths' 16 chunks without padding iterations (MT = 2: 9 slots of 16 KiB).
constexpr int W4_A2 = 8, W4_A4 = 4;

template <int MT, int NW, int A, int EPI>
constexpr int r4_lds_bytes() {
  const int ring = (A + 1) * R4_CK * MT * 1024, red = EPI == EPI_SILU ? NW * MT * 1536 : 0;
  return ring > red ? ring : red;
}

template <int MT, int NW, int A, int EPI>
bool launch_r4(const char *who, const GemmR4Args &a, int gx, hipStream_t st) {
  constexpr int lds = r4_lds_bytes<MT, NW, A, EPI>();
  void (*kern)(GemmR4Args) = dfl_k_gemm_r4<MT, NW, A, EPI>;
  static const hipError_t attr =
      hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (attr != hipSuccess) {
    (void)hipGetLastError();
    dfl_set_error("%s: %d bytes of dynamic LDS refused: %s", who, lds, hipGetErrorString(attr));
    return false;
  }
  hipLaunchKernelGGL(kern, dim3(gx), dim3(NW * 64), lds, st, a);
  return true;
}

// gemm_batch.hip's ring_plan
void r4_plan(GemmR4Args &a, int nunits, int upp_max, int &gx) {
  gx = nunits < 256 ? nunits : 256;
  const int per_wg = (nunits + gx - 1) / gx;
  a.nunits = nunits;
  a.npass = (per_wg + upp_max - 1) / upp_max;
  a.upp = (per_wg + a.npass - 1) / a.npass;
}

// What every batch form asks of a DFL_W_MXFP4 descriptor, the scale region first (include/dflash_hip.h)
bool w4_batch_ok(const char *who, const dfl_weight *w, const dfl_rows_batch *x, int R, int N, int K) {
  if (!w->scale) {
    dfl_set_error("%s: format 3 (DFL_W_MXFP4) in the batch forms takes its e8m0 scale region through `scale`: it is NULL", who);
    return false;
  }
  if (((uintptr_t)w->scale & 63) != 0) {
    dfl_set_error("%s: the DFL_W_MXFP4 scale region must be 64-byte aligned", who);
    return false;
  }
  if (!w->wp || !x) {
    dfl_set_error("%s: null pointer (weight or row source)", who);
    return false;
  }
  if (R < 1 || R > 4 || N <= 0 || N % 16 || K <= 0 || K % 128) {
    dfl_set_error("%s: DFL_W_MXFP4 needs 1 <= R <= 4, N %% 16 == 0, K %% 128 == 0 (R=%d N=%d K=%d)", who, R, N, K);
    return false;
  }
  return true;
}

// ... and the ring ones: no slab form on 4-bit codes
bool w4_ring_ok(const char *who, const dfl_rows_batch *x, int K) {
  if (x->r0.mode != 0 || !x->r0.frag || x->frag_stride % 8 || K < 256) {
    dfl_set_error("%s: DFL_W_MXFP4 needs the ring form: frag16 row sources (mode 0) with frag_stride %% 8 == 0 and K >= 256 "
                  "(K=%d); there is no slab form", who, K);
    return false;
  }
  return true;
}

void fill_r4(GemmR4Args &a, const dfl_weight *w, const dfl_rows_batch *x, int N, int K, const int32_t *dyn) {
  a.wp = (const bf16x8 *)w->wp;
  a.wscale = (const char *)w->scale;
  a.xf = (const bf16x8 *)x->r0.frag;
  a.frag_stride8 = x->frag_stride / 8;
  a.KS = K / 32;
  a.ntiles = N / 16;
  a.dyn = dyn;
}

}  // namespace

int dfl_gemm_f32_batch_w4(const char *who, const dfl_weight *w, const dfl_rows_batch *x, int R, int N, int K, float *out,
                          const int32_t *dyn, void *stream) {
  GemmB4Args a{};
  if (!w4_batch_ok(who, w, x, R, N, K)) return DFL_EINVAL;
  DFL_REQUIRE(out, "%s: null pointer", who);
  const int KS = K / 32, ksplit = (KS + 63) / 64;  // gemm_batch.hip's batch_ksplit and nfr
  DFL_REQUIRE(ksplit <= 16, "%s: K=%d beyond 16 K parts of 2048", who, K);
  const int nfr = (KS + 8 * ksplit - 1) / (8 * ksplit);
  DFL_REQUIRE(nfr % 4 == 0, "%s: DFL_W_MXFP4 needs whole 4-k-step words per wave: the bf16 launch's %d k-steps per wave at K=%d "
              "are not a multiple of 4 (taken: K = 1024 and multiples of 2048)", who, nfr, K);
  if (!fill_src(a.src, &x->r0, K, who)) return DFL_EINVAL;
  DFL_REQUIRE(x->r0.mode != 2, "%s: the batched GEMMs take normalised rows from dfl_norm_frag_batch (mode 0), not mode 2", who);
  DFL_REQUIRE(!(x->r0.valid_word >= 0 && !dyn) && x->frag_stride % 8 == 0,
              "%s: row validity needs dyn; frag_stride must be a multiple of 8", who);
  a.wp = (const bf16x8 *)w->wp;
  a.wscale = (const char *)w->scale;
  a.frag_stride = x->frag_stride;
  a.rows_stride = x->rows_stride;
  a.dyn = dyn;
  a.KS = KS;
  a.ntiles = N / 16;
  a.nfr = nfr;
  a.out = out;
  a.ldo = N;
  const dim3 grid(grid_x_for(a.ntiles, ksplit), ksplit);
  if (R <= 2)
    hipLaunchKernelGGL((k_gemm_b4<2>), grid, dim3(512), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((k_gemm_b4<4>), grid, dim3(512), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}

int dfl_gemm_silu_mul_batch_w4(const char *who, const dfl_weight *w, const dfl_rows_batch *x, int R, int I, int K, void *act_frag,
                               int64_t act_stride, const int32_t *dyn, void *stream) {
  if (!w4_batch_ok(who, w, x, R, I, K) || !w4_ring_ok(who, x, K)) return DFL_EINVAL;
  DFL_REQUIRE(act_frag, "%s: null pointer", who);
  DFL_REQUIRE(act_stride >= 16 * (int64_t)I, "%s: act_stride < 16*I", who);
  GemmR4Args r{};
  fill_r4(r, w, x, 2 * I, K, dyn);
  r.act = (bf16_t *)act_frag;
  r.act_stride = act_stride;
  // the bf16 plan: 3 units (12 waves) or 4 (16 waves) per workgroup and pass, four waves per unit
  const int per_wg = (I / 16 + 255) / 256;
  const bool w16 = per_wg % 4 == 0 || per_wg > 6;
  int gx = 0;
  r4_plan(r, I / 16, w16 ? 4 : 3, gx);
  const hipStream_t st = (hipStream_t)stream;
  const bool ok = R <= 2 ? (w16 ? launch_r4<2, 16, W4_A2, EPI_SILU>(who, r, gx, st) : launch_r4<2, 12, W4_A2, EPI_SILU>(who, r, gx, st))
                         : (w16 ? launch_r4<4, 16, W4_A4, EPI_SILU>(who, r, gx, st) : launch_r4<4, 12, W4_A4, EPI_SILU>(who, r, gx, st));
  if (!ok) return DFL_ELAUNCH;
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}

// The ring launch only: the caller (gemm_batch.hip) runs its k_argmax_finish_b over *ncand entries per row and request.
int dfl_gemm_argmax_batch_w4(const char *who, const dfl_weight *w, const dfl_rows_batch *x, int R, int V, int K, int row0, int nrows,
                             const int32_t *dyn, int nrows_dyn_word, float *best_val, int *best_idx, void *logits,
                             int64_t logits_stride, int *ncand, void *stream) {
  if (!w4_batch_ok(who, w, x, R, V, K) || !w4_ring_ok(who, x, K)) return DFL_EINVAL;
  DFL_REQUIRE(best_val && best_idx, "%s: null pointer", who);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "%s: rows [%d,%d) outside the tile", who, row0, row0 + nrows);
  GemmR4Args r{};
  fill_r4(r, w, x, V, K, dyn);
  r.row0 = row0;
  r.nrows = nrows;
  r.nrows_word = nrows_dyn_word;
  r.best_val = best_val;
  r.best_idx = best_idx;
  r.logits = (bf16_t *)logits;
  r.logits_stride = logits_stride;
  r.N = V;
  int gx = 0;
  r4_plan(r, V / 16, 16, gx);  // a wave owns a column tile over the whole K, passes of <= 16 tiles per workgroup
  const hipStream_t st = (hipStream_t)stream;
  const bool ok = R <= 2 ? launch_r4<2, 16, W4_A2, EPI_ARGMAX>(who, r, gx, st) : launch_r4<4, 16, W4_A4, EPI_ARGMAX>(who, r, gx, st);
  if (!ok) return DFL_ELAUNCH;
  *ncand = gx;
  return DFL_OK;
}
