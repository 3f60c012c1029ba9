// Skinny (M <= 32 rows) weight-streaming GEMM for gfx950.
//
// Shape of the problem: every nn.Linear of the draft step and of the
// target's verify sees at most 16 block rows (+ <=16 context rows), so each weight byte
// is used for <= 32 rows and the kernel is bound by HBM.  Design:
//   * weights are pre-packed (dfl_pack_weight) so a wave's 16-B-per-lane load is one
//     contiguous 1 KiB run AND one MFMA 16x16x32 A fragment: HBM -> VGPR -> matrix core,
//     no LDS, no shuffles (guide: "GEMV / M<=16: load straight to VGPRs, deep unroll,
//     late vmcnt");
//   * a 1024-thread workgroup = 16 waves splits K 16 ways and walks the workgroup's
//     column tiles, prefetching the next item's weights while the current one is in the
//     MFMA; per tile the 16 partial 16x16 tiles meet in LDS (double-buffered, one
//     barrier per tile) and 256 threads finish it;
//   * the activation operand comes from a row source (dfl_rows): ready-made frag16
//     fragments, plain bf16 rows, or the residual stream + per-tile sums of squares, in
//     which case the wave applies the RMSNorm itself while building its fragments —
//     the norm between two GEMMs is then not a launch of its own;
//   * epilogues: fp32 partials (K split over grid.y) / SiLU(gate)*up -> frag16 /
//     running bf16 argmax (lm_head) / residual add -> h, taps, sums of squares;
//   * K beyond 16 waves x 8 steps: either grid.y partials, or (CHUNKED) the workgroup
//     loops over K chunks itself so that the epilogue sees finished sums.
//   * W8 (k_gemm_w8, the draft's optional fp8 weights): the same kernel over e4m3 codes, one byte per weight, two
//     k-steps per 16-byte word, converted to bf16 in registers; one fp32 scale per output row on the fp32 sum.
//   * W4 (k_gemm_w4, the draft's optional MXFP4 weights): the same kernel over e2m1 codes, four k-steps per 16-byte word,
//     each dword converted to a bf16 fragment with its block's e8m0 scale applied in the conversion; no epilogue multiply.
// MFMA utilisation is a few percent by construction; the roofline is HBM: every launch
// costs ~3.6 us + bytes / 6.5 TB/s (scripts/bench_gemm.py).
#include "gemm_rows.h"
#include "dfl_rng.h"

namespace {

struct GemmArgs {
  // (the kernels take the fields that their first requests need a second time, as flat leading arguments: GemmHead below)
  const bf16x8 *wp;  // packed weights [ntiles][KS][64]
  int KS;      // K / 32
  int ntiles;  // N / 16
  int nfr;     // k-steps per wave per chunk (<= FR)
  int nch;     // K chunks walked inside the workgroup (1 unless CHUNKED)
  // tiles [0, ntiles) are walked whole (workgroup b: b, b+G, ...); tiles [ntiles, ntiles + nhalf/2) are cut in two
  // 8-column halves, one per workgroup b < nhalf (tile ntiles + b/2, half b&1), as that workgroup's LAST item:
  // 384 tiles (qkv of an 8B model) are 1.5 tiles for each of 256 workgroups instead of 2 for each of 192
  int nhalf;
  int gx;  // gridDim.x, as an argument: the built-in comes from the hidden arguments at the far end of the block
  const int32_t *dyn;
  RowSrc src[2];
  // EPI_F32
  float *out;  // [ksplit][MT*16][ldo]
  int ldo;
  // EPI_SILU
  bf16_t *act;  // frag16 [I/8][16][8]
  // EPI_SILU over the ACTIVE experts of a sparse-MoE layer (dfl_gemm_silu_mul_experts): the experts' packed gate/up
  // weights and frag16 outputs lie back to back, so (expert e, pair p) is pair e * npp + p of one tall matrix; the
  // workgroups share out the pairs of the n_active[0] experts listed in elist
  const int32_t *elist, *n_active;
  int npp;
  // EPI_ARGMAX
  int row0, nrows;
  int nrows_word;
  float *best_val;  // [gridDim.x][16]
  int *best_idx;
  float *best2_val;  // [gridDim.x][16] runner-up value (top-2 logit margin), optional
  bf16_t *logits;  // optional [16][N]
  int N;
  // EPI_RESID
  bf16_t *h_io;  // [16][ldh]: h <- bf16(h + bf16(acc)) (add_resid) or bf16(acc)
  int64_t ldh;
  int add_resid;
  bf16_t *tap;  // optional second copy of the new rows, row stride ldtap
  int64_t ldtap;
  float *ss_out;  // [ntiles][16] sum over the tile's 16 columns of h_new^2
  // W8 kernels (k_gemm_w8): wp holds e4m3 codes (gemm_rows.h, W8); wscale[16 t + nl] multiplies the fp32 K-sum of
  // packed tile t, column nl, before the epilogue's first rounding.  Last, so that no other field moves.
  // W13 kernels (k_gemm_w13): wp holds the 13-bit quads and wscale points at the {base, patch} pairs behind them.
  const float *wscale;
};

// EPI_SAMPLE (which reads the EPI_ARGMAX fields of GemmArgs as well): row m draws position base + pos_add + m, base =
// pos_dyn[pos_word] or pos_base; the DRAFT stream takes extra = base (the block start), the TARGET stream extra = 0.
// A kernel argument of its own (k_gemm_s): GemmArgs, and with it the code of every other instantiation, is unchanged.
struct SampleArgs {
  uint64_t seed;
  float inv_t;
  int rng_stream;
  const int32_t *pos_dyn;
  int pos_word, pos_base, pos_add;
};

// ---- the head of the launch arguments ---------------------------------------------------------------------------------
// gfx950 delivers the first 14 dwords of the kernel-argument block in SGPRs at wave start (kernarg preload, build.py:
// -amdgpu-kernarg-preload-count), but only leading scalar and pointer parameters, never a struct passed by value.  So the
// kernels take, in FRONT of GemmArgs, a flat copy of everything that the instructions up to item 0's weight request
// read (judged from the ISA: the row requests of src[0] come first, and they are in the same order-of-issue chain), and
// overwrite the struct's fields with it: gemm_body then finds those values in registers and the first vector address
// waits for no cold fetch of the argument block.  14 dwords are five pointers and four words, so the small fields share
// one 64-bit word (HeadBits); gemm_head() builds the head from the finished GemmArgs and refuses a launch whose values
// do not fit, so the two cannot drift.  src[1] (MT = 2) stays in the struct.
struct HeadBits {
  uint64_t KS : 17, nfr : 4, mode : 2, valid_word1 : 6 /* valid_word + 1 */, nrows_word1 : 6 /* nrows_word + 1 */, gx : 9,
      nhalf : 9, nch_nss : 11 /* CHUNKED: nch; otherwise nss of a normalised src[0] */;
};
static_assert(sizeof(HeadBits) == 8, "HeadBits is one 64-bit kernel argument");
struct GemmHead {
  const bf16x8 *wp;
  const void *x;  // src[0]: frag (mode 0) or rows (mode 1/2)
  const float *ss;
  const bf16_t *nw;
  const int32_t *dyn;
  uint64_t bits;
  int ld, ntiles;
};
#define GEMM_HEAD_DWORDS 14  // tests/test_launch_args.py: the preload length the compiler must report for these kernels
static_assert(sizeof(GemmHead) == 4 * GEMM_HEAD_DWORDS, "the head is what the hardware preloads: at most 14 dwords, no padding");
#define GEMM_HEAD_PARAMS \
  const bf16x8 *wp, const void *x, const float *ss, const bf16_t *nw, const int32_t *dyn, uint64_t bits, int ld, int ntiles
#define GEMM_HEAD_NAMES wp, x, ss, nw, dyn, bits, ld, ntiles
#define GEMM_HEAD_OF(h) (h).wp, (h).x, (h).ss, (h).nw, (h).dyn, (h).bits, (h).ld, (h).ntiles

template <bool CHUNKED, bool NORM>
__device__ __forceinline__ GemmArgs with_head(GemmArgs a, GEMM_HEAD_PARAMS) {
  const HeadBits b = __builtin_bit_cast(HeadBits, bits);
  a.wp = wp;
  a.dyn = dyn;
  a.ntiles = ntiles;
  a.KS = (int)b.KS;
  a.nfr = (int)b.nfr;
  a.nhalf = (int)b.nhalf;
  a.gx = (int)b.gx;
  a.nch = CHUNKED ? (int)b.nch_nss : 1;
  a.nrows_word = (int)b.nrows_word1 - 1;
  RowSrc &s = a.src[0];
  s.frag = reinterpret_cast<const bf16x8 *>(x);
  s.rows = reinterpret_cast<const bf16_t *>(x);
  s.ld = ld;
  s.ss = ss;
  s.nw = nw;
  s.mode = (int)b.mode;
  s.valid_word = (int)b.valid_word1 - 1;
  if (NORM) s.nss = (int)b.nch_nss;
  return a;
}

// host: the head of a finished GemmArgs (gx included)
template <bool CHUNKED>
bool gemm_head(GemmHead &h, const GemmArgs &a) {
  const RowSrc &s = a.src[0];
  HeadBits b{};
  b.KS = a.KS;
  b.nfr = a.nfr;
  b.mode = s.mode;
  b.valid_word1 = s.valid_word < 0 ? 0 : s.valid_word + 1;
  b.nrows_word1 = a.nrows_word < 0 ? 0 : a.nrows_word + 1;
  b.gx = a.gx;
  b.nhalf = a.nhalf;
  const int nch_nss = CHUNKED ? a.nch : (s.mode == 2 ? s.nss : 0);
  b.nch_nss = nch_nss;
  const int64_t ld = s.mode == 0 ? 0 : s.ld;  // (a fragment source has no row stride)
  const bool fits = (int)b.KS == a.KS && (int)b.nfr == a.nfr && (int)b.mode == s.mode && (int)b.gx == a.gx &&
                    (int)b.nhalf == a.nhalf && (int)b.nch_nss == nch_nss && (CHUNKED || a.nch == 1) && ld == (int)ld &&
                    (int)b.valid_word1 == (s.valid_word < 0 ? 0 : s.valid_word + 1) &&
                    (int)b.nrows_word1 == (a.nrows_word < 0 ? 0 : a.nrows_word + 1);
  if (!fits) {
    dfl_set_error("skinny GEMM: launch arguments outside the preloaded head's fields (K=%d, grid %d, ld=%lld)", a.KS * 32, a.gx,
                  (long long)s.ld);
    return false;
  }
  h.wp = a.wp;
  h.x = s.mode == 0 ? (const void *)s.frag : (const void *)s.rows;
  h.ss = s.ss;
  h.nw = s.nw;
  h.dyn = a.dyn;
  h.bits = __builtin_bit_cast(uint64_t, b);
  h.ld = (int)ld;
  h.ntiles = a.ntiles;
  return true;
}

#ifdef DFL_GEMM_STAMPS  // diagnostic build only (scripts/dbg_gemm_stamps.py): 100 MHz wall stamps of workgroup 0,
// and the start / first-item / end stamps of EVERY workgroup (is the tail a few late workgroups or all of them?)
__device__ unsigned long long g_gstamps[8];
__device__ unsigned long long g_wgstamps[256][4];
#define GSTAMP(i)                                                                         \
  do {                                                                                    \
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) g_gstamps[i] = __builtin_amdgcn_s_memrealtime(); \
    if (threadIdx.x == 0 && blockIdx.y == 0 && blockIdx.x < 256 && ((i) == 0 || (i) == 4 || (i) == 5))            \
      g_wgstamps[blockIdx.x][(i) == 0 ? 0 : (i) - 3] = __builtin_amdgcn_s_memrealtime();                           \
  } while (0)
#else
#define GSTAMP(i)
#endif

constexpr int gemm_fr(int MT, bool CHUNKED) { return CHUNKED ? 4 : (MT == 1 ? 8 : 4); }

// One launch.  Order of the prologue (round 3; measured with scripts/dbg_gemm_stamps.py, scripts/ab_prof.sh and against
// the pure-stream floor of scripts/probes/l2_prefetch_probe.hip — a stream of the same bytes in the same four launches
// per layer takes 62 us where the round-2 kernels took 80):
//   0. the lengths (dyn words): dependent SCALAR loads.  Requested behind the first weight burst they came back 5 - 9 us
//      later — most of what round 2 called the "rstd prologue".  Asked for before any vector load they cost nothing.
//   1. the activation side: the wave's row fragments (8 KB, from L2), for a normalised source one chunk of the RMSNorm
//      weight (staged ONCE per workgroup in LDS instead of 32 VGPRs per lane) and the producer's partial sums of
//      squares.  A wave's vector loads return in issue order and, at a launch's start, everything requested behind the
//      first weight burst queues behind ~32-64 MB in the memory system: asked for first, the rows are back after
//      ~1.5 us and the sum of squares -> rstd -> normalise chain (1-2 us of VALU on 16 waves) runs UNDER the weight
//      latency.  (Weights first: the rows came back 8 us later and the chain ran with HBM idle — gate/up 34.8 -> 36.6 us,
//      qkv 14.3 -> 16.4 us in the cycle.)  Launches without a normalised source put a workgroup barrier here, so that
//      every wave's row requests are in the CU's in-order memory pipe before any wave's weight request.
//   2. then item 0's weights and (residual launches without a norm) the residual value of the first tile;
//   3. only then the waits: rstd across the 16 waves, normalise, and the item loop (item i+1 requested at its top).
// Every load of the prologue is unconditional (clamped addresses, zero-length descriptors): a load under a branch
// costs a vmcnt(0) at the join, i.e. the whole burst.
// NORM: the launch has a normalised source (mode 2); the other instantiation carries none of that code or its LDS.
// Variants built, measured on the same box and dropped (DESIGN.md section 5 has the numbers; the code is in the history,
// commits dc953f3 and 5c920f1): item 1's weights requested in the prologue as well; the workgroup summing the squares
// of its own rows (v_dot2c) instead of loading the producer's partials; waiting for the rows before the first weight
// request; an 8-wave, three-buffer form of the K-chunked kernel.
// W8: the weights are e4m3 codes, two k-steps per 16-byte word (gemm_rows.h): half as many loads per item, each word
// converted into two fragments in front of its MFMAs; the finishing thread's scale is requested WITH the item's weights.
// Everything else (masks, the half-tile lane rule, the LDS meeting, the tile plan) is the bf16 form's.
// W13: the weights are the lossless 13-bit form of bf16 (gemm_rows.h): an item is two quads of four k-steps, six 16-byte and
// two 4-byte words per lane instead of eight 16-byte ones, decoded into the SAME fragments in front of the MFMAs; the
// tile's base and the item's patch word come by a scalar load issued with the item's request.  MT = 1.
// W13 && CHUNKED (k_gemm_w13c; K a multiple of 2048 above 4096, so every chunk is whole): in chunk c wave w owns k-steps
// (16 c + w) * 4 .. + 3 — quad 16 c + w of the tile.  An item is that ONE quad (the request of k_moe_gate_up: SG, NB, L0,
// L1; 13 VGPRs in flight against 16), its meta pair is pair (t * nch + c) * 16 + w, and the chunk's activation fragments
// go behind the quad as in the bf16 form.
// UNC (the W13 gate/up + SiLU launch only): the item loop requests the next item UNCONDITIONALLY — past the last item a
// dummy whose descriptor holds zero bytes and whose meta load reads pair 0 — so that hipcc counts the loads in flight
// exactly.  Behind the loop's `if (i + 1 < nitems)` it counts from the merged state, as if the request had not been made:
// the first decode of an item then waits at vmcnt(3) / (1) / (0), i.e. for five of the eight words of the item the wave
// has JUST asked for and, before its last k-steps, for all of it.  The bf16 form has the same waits and loses little (its
// process step is 8 MFMAs); the 13-bit form puts 8 x 19 VALU of decode per item into that window.  Unconditional, the
// waits are vmcnt(15) .. (8): an item's decode starts as its own words land, with the whole next item still in flight.
// Same requests in the same order, same fragments, same MFMAs, same finish(): the conditional loop's bits.
// W4 (k_gemm_w4; DFL_W_MXFP4): the weights are e2m1 codes, FOUR k-steps per 16-byte word, with one e8m0 scale per k-step and
// column (gemm_rows.h): a quarter as many loads per item, the item's scale dwords requested WITH its words (item 0's in the
// prologue, never behind the K loop), each dword converted into its fragment — block scale included — in front of its
// MFMA; no epilogue multiply.  A wave's share is whole words (nfr % 4 == 0).  Everything else is the bf16 form's.
template <int MT, bool CHUNKED, int EPI, bool NORM, bool W8 = false, bool W13 = false, bool UNC = false, bool W4 = false>
__device__ __forceinline__ void gemm_body(const GemmArgs &a, const SampleArgs &sa) {
  GSTAMP(0);
  static_assert(!W13 || (MT == 1 && !W8), "W13: the single-tile bf16 kernels only");
  static_assert(!W4 || (MT == 1 && !W8 && !W13), "W4: the single-tile kernels only, one format per kernel");
  static_assert(!UNC || (W13 && !CHUNKED && EPI == EPI_SILU), "unconditional item requests: the W13 gate/up launch only");
  static_assert(!W13 || !CHUNKED || (EPI == EPI_RESID && !NORM), "W13, K-chunked: the residual launch only");
  constexpr int FR = gemm_fr(MT, CHUNKED);
  constexpr int NW = W13 ? (CHUNKED ? 3 : 6) : (W8 ? FR / 2 : (W4 ? FR / 4 : FR));  // 16-byte weight words per item and lane
  // red[buf][wave][mt][256]: lane l owns floats 4l..4l+3 (its MFMA D regs)
  __shared__ float red[2][16][MT][256];
  __shared__ float ssred[NORM ? MT : 1][16][16];
  __shared__ bf16x8 nwl[NORM ? MT : 1][NORM ? 512 : 1];  // mode 2: the norm weight of K <= 4096, chunk c = elements 8c .. 8c+7

  const int tid = threadIdx.x;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l = tid & 63;

  auto ks0_of = [&](int c) { return ((blockIdx.y * a.nch + c) * 16 + w) * a.nfr; };
  auto nf_of = [&](int c) {
    int nf = a.KS - ks0_of(c);
    return nf < 0 ? 0 : (nf > a.nfr ? a.nfr : nf);
  };

  // ---- tile sequence of this workgroup.  F32/ARGMAX/RESID: tiles bx, bx+G, ...
  // SILU: the packed weight interleaves (gate tile p, up tile p) and the sequence walks
  // pairs p = bx, bx+G, ... as gate,up,gate,up: the finishing thread meets a pair's two
  // sums in consecutive positions.
  const int stride = a.gx;
  constexpr bool SILU = EPI == EPI_SILU || EPI == EPI_SILU_E;
  constexpr bool moe = EPI == EPI_SILU_E;  // the tile sequence comes from the active-expert list (dependent scalar loads)
  const int nwhole = (!SILU && (int)blockIdx.x < a.ntiles) ? (a.ntiles - 1 - (int)blockIdx.x) / stride + 1 : 0;  // whole tiles of this workgroup
  const bool has_half = !SILU && (int)blockIdx.x < a.nhalf;
  const int myhalf = (int)blockIdx.x & 1;
  auto half_of = [&](int j) -> int { return (!SILU && j >= nwhole) ? myhalf : -1; };  // -1: a whole tile
  auto tile_of = [&](int j) -> int {
    if (!SILU) return j < nwhole ? (int)blockIdx.x + j * stride : a.ntiles + ((int)blockIdx.x >> 1);
    int p = (int)blockIdx.x + (j >> 1) * stride;
    if (moe) p = a.elist[p / a.npp] * a.npp + p % a.npp;  // scalar loads: p is uniform over the workgroup
    return 2 * p + (j & 1);
  };

  bf16x8 wA[NW], wB[NW];
  float scA = 1.f, scB = 1.f;  // W8: the scale of this thread's column (tid & 15) of the item in wA / wB
  W13Extra exA{}, exB{};       // W13: the item's sign words and its {base, patch} pair; W4: sg = the item's scale dwords
  bf16x8 xA[MT][FR], xB[MT][FR];
  bf16x8 xr[MT][FR];  // activations of the (single) chunk stay in registers for the launch

  const int nf0 = nf_of(0);
  const int ngroups = SILU ? a.ntiles >> 1 : a.ntiles;
  int nseq;
  if (SILU) {
    const int npairs = moe ? a.n_active[0] * a.npp : a.ntiles >> 1;
    nseq = (int)blockIdx.x < npairs ? 2 * ((npairs - 1 - (int)blockIdx.x) / stride + 1) : 0;
  } else {
    nseq = nwhole + (has_half ? 1 : 0);
  }
  const int nitems = nseq * a.nch;

  int nv[MT];
  auto read_nv = [&]() {  // row validity (rows >= dyn[valid_word] count as zero): scalar loads, on their own counter
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const RowSrc &s0 = a.src[mt];
      nv[mt] = (s0.valid_word >= 0 && a.dyn) ? a.dyn[s0.valid_word] : 16;
    }
  };

  // finishing thread f < MT*256: row m = (f&255)>>4, column nl = f&15 of the tile
  float best = -INFINITY;  // running argmax
  int bestn = 0x7fffffff;
  float second = -INFINITY;  // runner-up VALUE as torch.topk(2) defines it: a tie with the best counts
  float gate_sum = 0.f;    // SILU: the pair's gate sum, kept across one position
  int arg_rows = 0;
  int pos_row0 = 0, rng_extra = 0;  // EPI_SAMPLE: position drawn by tile row 0, counter word `extra`

  // chunked kernels: item (tile t, chunk c) = the wave's weights of that chunk AND its activation fragments.  Only the
  // REQUESTS are made here; the mask (rows beyond the valid count, k-steps beyond K) is applied in process(), right in
  // front of the MFMAs.  Round 2 masked right behind the requests: a wait for the activation loads — which return after
  // the weights requested in front of them — so every wave waited for the item it had JUST asked for and no two items
  // of a wave were ever in flight (down_proj at 4.9 TB/s, its workgroups ending 3.4 us apart).
  auto load_item_x = [&](bf16x8(&xb)[MT][FR], int c) {
    const int ks0 = ks0_of(c);
    int ks[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) ks[f] = ks0 + f < a.KS ? ks0 + f : a.KS - 1;
    bf16x8 wv[MT][FR];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int f = 0; f < FR; ++f) wv[mt][f] = xb[mt][f] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) issue_x<FR, false>(a.src[mt], ks, l, nv[mt], xb[mt], wv[mt]);  // no mode 2 here
  };
  // W8: the wave's k-steps ks0 .. ks0 + nf of tile t (nf = 0: nothing is fetched) and, WITH that request, the scale of
  // this thread's column — not behind the K loop: a dependent load at the tail of a one-tile launch is ~1 us
  auto load_w8 = [&](bf16x8(&wr)[NW], float &sc, int t, int ks0, int nf, int half) {
    if constexpr (W8) {
      load_ksteps_w8<FR>(wr, a.wp + ((size_t)t * (a.KS >> 1) + (ks0 >> 1)) * 64, nf, l, half);
      sc = a.wscale[(size_t)t * 16 + (tid & 15)];
    }
  };
  // W13: (K is 2048 or 4096, so ks0 and nf are whole quads) the meta pair WITH the request, as the W8 scale
  // chunked: the one quad of (tile t, chunk c), whole tiles only, and the pair of (t * nch + c, wave)
  auto load_w13 = [&](bf16x8(&wr)[NW], W13Extra &ex, int t, int ks0, int nf, int half, int c = 0) {
    if constexpr (W13 && CHUNKED) {
      const char *base = reinterpret_cast<const char *>(a.wp);
      load_quads_w13(wr, ex.sg[0], base + ((size_t)t * (a.KS >> 2) + (ks0 >> 2)) * W13_QUAD_BYTES, nf >> 2, l);
      ex.meta = w13_meta(reinterpret_cast<const u32x2 *>(a.wscale), nf > 0 ? t * a.nch + c : 0, w);
    } else if constexpr (W13) {
      const char *base = reinterpret_cast<const char *>(a.wp);
      load_quads_w13(wr, ex.sg, base + ((size_t)t * (a.KS >> 2) + (ks0 >> 2)) * W13_QUAD_BYTES, nf >> 2, l, half);
      ex.meta = w13_meta(reinterpret_cast<const u32x2 *>(a.wscale), nf > 0 ? t : 0, w);  // (nothing fetched: any valid pair)
    }
  };
  // W4: the wave's words ks0 / 4 .. of tile t and, WITH that request, their scale dwords (a.wscale = the scale region)
  auto load_w4 = [&](bf16x8(&wr)[NW], W13Extra &ex, int t, int ks0, int nf, int half) {
    if constexpr (W4) {
      const size_t word = (size_t)t * (a.KS >> 2) + (ks0 >> 2);
      load_ksteps_w4<FR>(wr, ex.sg, a.wp + word * 64, reinterpret_cast<const char *>(a.wscale) + word * 64, nf, l, half);
    }
  };
  auto load_item = [&](bf16x8(&wr)[NW], float &sc, W13Extra &ex, bf16x8(&xb)[MT][FR], int t, int c, int half) {
    if constexpr (W4)
      load_w4(wr, ex, t, ks0_of(c), nf_of(c), half);
    else if constexpr (W13)
      load_w13(wr, ex, t, ks0_of(c), nf_of(c), half, c);
    else if constexpr (W8)
      load_w8(wr, sc, t, ks0_of(c), nf_of(c), half);
    else
      load_ksteps<FR>(wr, a.wp + ((size_t)t * a.KS + ks0_of(c)) * 64, nf_of(c), l, half);
    if (CHUNKED) load_item_x(xb, c);  // the weights first (HBM), the activation fragments (L2) behind them
  };

  f32x4 acc[MT];
  // EPI_RESID without a normalised source (o_proj, down_proj: one tile per workgroup): this thread's residual value
  // of the FIRST tile, requested in the prologue
  constexpr bool PREF = EPI == EPI_RESID && !NORM;
  bf16_t resid0 = (bf16_t)0.f;

  auto finish = [&](int t, int pos, float wsc) {
    const int buf = pos & 1;
    const int hf = half_of(pos);  // a half tile: the other 8 columns belong to the neighbouring workgroup
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<f32x4 *>(&red[buf][w][mt][l * 4]) = acc[mt];
    __syncthreads();
    // D layout of mfma 16x16x32 (A = W rows n, B = x^T cols m): lane L reg r holds
    // n_local = 4*(L>>4) + r, m = L & 15, i.e. float 4L + r of the wave's slot.
    if (tid < MT * 256) {
      const int mt = tid >> 8, ff = tid & 255;
      const int m = ff >> 4, nl = ff & 15;
      const int idx = 4 * (m + 16 * (nl >> 2)) + (nl & 3);
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < 16; ++ww) s += red[buf][ww][mt][idx];
      if (W8) s *= wsc;  // the row's scale on the fp32 K-sum, in front of every rounding point below
      const bool colok = hf < 0 || (nl >> 3) == hf;
      if (EPI == EPI_F32) {
        if (colok) a.out[((size_t)(blockIdx.y * MT + mt) * 16 + m) * a.ldo + t * 16 + nl] = s;
      } else if (SILU) {
        if (buf == 0) {
          gate_sum = s;
        } else {
          // tf:modeling_qwen3.py:82: gate/up Linear outputs are bf16, silu is evaluated in
          // fp32 and rounded, the product is rounded again.
          const float gb = rbf(gate_sum), ub = rbf(s);
          const float act = rbf(gb / (1.f + __expf(-gb)));
          const int n = (t >> 1) * 16 + nl;
          a.act[((size_t)(n >> 3) * 16 + m) * 8 + (n & 7)] = f2bf(act * ub);
        }
      } else if (EPI == EPI_ARGMAX || EPI == EPI_SAMPLE) {
        const int n = t * 16 + nl;
        float vb = rbf(s);  // lm_head output is bf16 before argmax (model/dflash.py:238,247)
        const bool live = (m >= a.row0) && (m < a.row0 + arg_rows) && colok;
        if (a.logits && live) a.logits[(size_t)m * a.N + n] = f2bf(s);
        if (EPI == EPI_SAMPLE) {  // Gumbel-max: the same running argmax over bf16(logit) * invT + g(seed, p, n)
          uint32_t wd[4];
          dfl_rng_words(sa.seed, (uint32_t)sa.rng_stream, (uint32_t)(pos_row0 + m), (uint32_t)n, (uint32_t)rng_extra, wd);
          const int k = nl & 3;
          vb = dfl_perturb_w(vb, sa.inv_t, k == 0 ? wd[0] : (k == 1 ? wd[1] : (k == 2 ? wd[2] : wd[3])));
        }
        // n grows along the sequence for a fixed thread: strict '>' keeps the first maximum
        if (live && (vb > best || bestn == 0x7fffffff)) {
          second = best;
          best = vb;
          bestn = n;
        } else if (live) {
          second = fmaxf(second, vb);
        }
      } else {  // EPI_RESID: model/dflash.py:140,144 residual adds (bf16 + bf16 -> bf16)
        const int n = t * 16 + nl;
        const float v = rbf(s);  // the Linear's bf16 output
        bf16_t *hp = a.h_io + (int64_t)m * a.ldh + n;
        // the first tile's old value came with the prologue's loads (a dependent ~1 us load at the tail of the
        // one-tile launches o_proj / down_proj otherwise); later tiles of a workgroup read theirs here
        float hn = v;
        if (a.add_resid) hn = rbf(bf2f((PREF && pos == 0) ? resid0 : *hp) + v);
        if (colok) {
          *hp = f2bf(hn);
          if (a.tap) a.tap[(int64_t)m * a.ldtap + n] = f2bf(hn);
        }
        const float q = row_sum16(hn * hn);  // the 16 threads of row m are one DPP row
        if (nl == 0 && a.ss_out) a.ss_out[t * 16 + m] = q;
      }
    }
  };

  auto process = [&](bf16x8(&wr)[NW], float wsc, const W13Extra &ex, bf16x8(&xb)[MT][FR], int t, int c, int pos) {
    if (!CHUNKED || c == 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const int ks0c = ks0_of(c);
#pragma unroll
    for (int f = 0; f < FR; ++f)  // k-steps past the wave's share carry zero weights AND zero activations
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        bf16x8 xv = xr[mt][f];
        if (CHUNKED) {
          const bool keep = ks0c + f < a.KS && (a.src[mt].mode == 0 || (l & 15) < nv[mt]);
          xv = keep ? xb[mt][f] : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
        }
        bf16x8 wf;
        if constexpr (W13 && CHUNKED)
          wf = w13_frag(wr, ex.sg[0], ex.meta, f, l);
        else if constexpr (W13)
          wf = w13_frag(wr, ex, f, l);
        else if constexpr (W4)
          wf = w4_frag(wr[f >> 2], ex.sg[f >> 2], f & 3);
        else
          wf = weight_frag<W8>(wr, f);
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, xv, acc[mt], 0, 0, 0);
      }
    if (!CHUNKED || c == a.nch - 1) finish(t, pos, wsc);
  };

  // item 0 of this workgroup (F32 / ARGMAX / RESID): whole tile blockIdx.x, or — a launch cut entirely in halves
  // (plan_tiles: at most 128 tiles) — half blockIdx.x & 1 of tile blockIdx.x >> 1
  const int first_tile = (SILU || nwhole > 0) ? (int)blockIdx.x : a.ntiles + ((int)blockIdx.x >> 1);
  const int first_half = (SILU || nwhole > 0) ? -1 : myhalf;
  const bool first_live = SILU ? (int)blockIdx.x < ngroups : (nwhole > 0 || has_half);
  // the residual value of this thread's element of the FIRST tile (every thread asks: ff = tid & 255 — no branch)
  auto ask_resid0 = [&]() {
    if (PREF) {
      const int ff = tid & 255;
      resid0 = a.h_io[(int64_t)(ff >> 4) * a.ldh + first_tile * 16 + (ff & 15)];
    }
  };

  // ---- (0) the lengths: dependent SCALAR loads (argument block -> dyn -> word), on their own counter and out of order
  // with the vector loads — but through the same L2: requested behind the first weight burst they came back 5 - 9 us
  // later (the "rstd prologue" of round 2 was mostly this wait).  Asked for before any vector load they cost nothing.
  read_nv();
  // (only the REQUEST here: row0 / nrows are not in the head of the launch arguments, and arithmetic on the word would
  // be a wait in front of the first vector request; arg_rows is settled below, behind item 0's weight request)
  int arg_word = 0;
  const bool arg_dyn = (EPI == EPI_ARGMAX || EPI == EPI_SAMPLE) && a.dyn && a.nrows_word >= 0;
  if (arg_dyn) arg_word = a.dyn[a.nrows_word];
  if (EPI == EPI_SAMPLE) {
    const int base = sa.pos_dyn ? sa.pos_dyn[sa.pos_word] : sa.pos_base;
    pos_row0 = base + sa.pos_add;
    rng_extra = sa.rng_stream == (int)DFL_RNG_DRAFT ? base : 0;
  }
  __builtin_amdgcn_sched_barrier(0);
  float rstd[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) rstd[mt] = 1.f;
  if (!CHUNKED) {
    // ---- (1) the activation side, all unconditional: norm weight chunk (mode 2; any other mode reads 16 B of its own
    // operand and ignores them), partial sums of squares, the wave's activation fragments, the residual value
    bf16x8 nwv[MT];
    float ssv[MT][4];
    bool any_norm = false;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const RowSrc &s = a.src[mt];
#pragma unroll
      for (int u = 0; u < 4; ++u) ssv[mt][u] = 0.f;
      nwv[mt] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
      if (NORM) {
        const int c = min(tid & 511, a.KS * 4 - 1);
        const char *nb = s.mode == 2 ? reinterpret_cast<const char *>(s.nw)
                                     : (s.mode == 0 ? reinterpret_cast<const char *>(s.frag) : reinterpret_cast<const char *>(s.rows));
        nwv[mt] = *reinterpret_cast<const bf16x8 *>(nb + c * 16);
      }
      if (NORM && s.mode == 2) {  // uniform (a kernel argument); the loads inside are clamped, not guarded
        // the nss <= 256 partial sums of squares of a row are summed by the 16 waves together:
        // wave w takes partials w, w+16, ... (four loads in flight per lane)
        const int m = l & 15, part = l >> 4;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = w + 16 * (part + 4 * u);
          ssv[mt][u] = s.ss[(i < s.nss ? i : s.nss - 1) * 16 + m];
        }
        any_norm = true;
      }
    }
    int ks[FR];
    bool take[FR];
#pragma unroll
    for (int f = 0; f < FR; ++f) {
      take[f] = f < nf0;
      ks[f] = take[f] ? ks0_of(0) + f : 0;
    }
    bf16x8 raw[MT][FR], wv0[MT][FR];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int f = 0; f < FR; ++f) wv0[mt][f] = raw[mt][f] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) issue_x<FR, false>(a.src[mt], ks, l, 16, raw[mt], wv0[mt]);
    __builtin_amdgcn_sched_barrier(0);  // the ORDER of issue is the point: hipcc moved the weight requests in front
    if (!NORM) {  // every wave's row requests enter the CU's in-order memory pipe before any weight request
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    // ---- (2) item 0's weights.  No guards on the k-step count anywhere: a runtime guard makes hipcc branch around
    // every fragment load and wait vmcnt(0) after each (49 full waits instead of 16 in the SILU kernel, 34 -> 41 us).
    // load_ksteps clips at the wave's share through the buffer descriptor instead (zero weights, no traffic), and
    // activations past the share are zero as well.  (The expert list of an MoE launch is a dependent scalar load: that
    // launch asks for its first weights once it knows the tile.)
    if constexpr (W4)
      load_w4(wA, exA, SILU ? 2 * (int)blockIdx.x : first_tile, ks0_of(0), first_live ? nf0 : 0, first_half);
    else if constexpr (W13)
      load_w13(wA, exA, SILU ? 2 * (int)blockIdx.x : first_tile, ks0_of(0), first_live ? nf0 : 0, first_half);
    else if constexpr (W8)
      load_w8(wA, scA, SILU ? 2 * (int)blockIdx.x : first_tile, ks0_of(0), first_live ? nf0 : 0, first_half);
    else if (!moe)
      load_ksteps<FR>(wA, a.wp + ((size_t)(SILU ? 2 * blockIdx.x : first_tile) * a.KS + ks0_of(0)) * 64,
                      first_live ? nf0 : 0, l, first_half);
    else if (nitems > 0)
      load_ksteps<FR>(wA, a.wp + ((size_t)tile_of(0) * a.KS + ks0_of(0)) * 64, nf0, l);
    GSTAMP(6);
    __builtin_amdgcn_sched_barrier(0);
    ask_resid0();
    GSTAMP(1);
    // ---- (3) rstd, normalise
    if (NORM && any_norm) {  // uniform over the workgroup: the modes are kernel arguments
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const RowSrc &s = a.src[mt];
        if (NORM) nwl[mt][tid & 511] = nwv[mt];  // both halves of the workgroup store the same 512 chunks
        if (NORM && s.mode == 2) {
          const int m = l & 15, part = l >> 4;
          float v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) v[u] = (w + 16 * (part + 4 * u)) < s.nss ? ssv[mt][u] : 0.f;
          float t = (v[0] + v[1]) + (v[2] + v[3]);  // nss <= 256 (fill_src): the prologue's loads cover every partial
          t += __shfl_xor(t, 16, 64);
          t += __shfl_xor(t, 32, 64);
          if (part == 0) ssred[mt][w][m] = t;
        }
      }
      __syncthreads();
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        if (a.src[mt].mode == 2) {
          float t = 0.f;
#pragma unroll
          for (int ww = 0; ww < 16; ++ww) t += ssred[mt][ww][l & 15];
          rstd[mt] = rsqrtf(t / (float)(a.KS * 32) + a.src[mt].eps);
        }
    }
    GSTAMP(2);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (NORM)
        finish_xl<FR>(a.src[mt], ks, take, l, nv[mt], rstd[mt], raw[mt], nwl[mt], xr[mt]);
      else
        finish_x<FR, false>(a.src[mt], take, l, nv[mt], 1.f, raw[mt], wv0[mt], xr[mt]);
    }
  } else {
    // chunked kernels build their activation fragments per item: item 0's behind the weights already requested
    if constexpr (W4)
      load_w4(wA, exA, first_tile, ks0_of(0), first_live ? nf0 : 0, first_half);
    else if constexpr (W8)
      load_w8(wA, scA, first_tile, ks0_of(0), first_live ? nf0 : 0, first_half);
    else if constexpr (W13)
      load_w13(wA, exA, first_tile, ks0_of(0), first_live ? nf0 : 0, first_half, 0);
    else if (nitems > 0 || !moe)
      load_ksteps<FR>(wA, a.wp + ((size_t)first_tile * a.KS + ks0_of(0)) * 64, first_live ? nf0 : 0, l, first_half);
    GSTAMP(6);
    load_item_x(xA, 0);
    ask_resid0();
    GSTAMP(1);
    GSTAMP(2);
  }

  if (EPI == EPI_ARGMAX || EPI == EPI_SAMPLE) arg_rows = arg_dyn ? arg_word - a.row0 : a.nrows;
  GSTAMP(3);
  if (nitems > 0) {
    int j = 0, c = 0;  // current item
    for (int i = 0;; i += 2) {
      int jn = j, cn = c + 1;  // item i+1
      if (cn == a.nch) {
        cn = 0;
        ++jn;
      }
      // (requesting unconditionally — a zero-length dummy past the last item, so that hipcc can count the loads in
      // flight — was tried twice in this 16-wave kernel, rounds 2 and 3: 20.4 -> 20.8 us on down_proj; not kept)
      // (... and in the 13-bit gate/up launch, where the decode sits in the wait: kept, UNC above)
      if constexpr (UNC) {
        const bool live = i + 1 < nitems;
        load_w13(wB, exB, live ? tile_of(jn) : 0, ks0_of(0), live ? nf0 : 0, -1);
        __builtin_amdgcn_sched_barrier(0);
      } else if (i + 1 < nitems) {
        load_item(wB, scB, exB, xB, tile_of(jn), cn, half_of(jn));
      }
      process(wA, scA, exA, xA, tile_of(j), c, j);
      if (i == 0) GSTAMP(4);
      if (i + 1 >= nitems) break;
      int j2 = jn, c2 = cn + 1;  // item i+2
      if (c2 == a.nch) {
        c2 = 0;
        ++j2;
      }
      if constexpr (UNC) {
        const bool live = i + 2 < nitems;
        __builtin_amdgcn_sched_barrier(0);
        load_w13(wA, exA, live ? tile_of(j2) : 0, ks0_of(0), live ? nf0 : 0, -1);
        __builtin_amdgcn_sched_barrier(0);
      } else if (i + 2 < nitems) {
        load_item(wA, scA, exA, xA, tile_of(j2), c2, half_of(j2));
      }
      process(wB, scB, exB, xB, tile_of(jn), cn, jn);
      if (i + 2 >= nitems) break;
      j = j2;
      c = c2;
    }
  }

  GSTAMP(5);
  if (EPI == EPI_ARGMAX || EPI == EPI_SAMPLE) {
    // the 16 threads of row m are consecutive lanes: shuffle down to lane nl == 0
    if (tid < 256) {
#pragma unroll
      for (int o = 1; o <= 8; o <<= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bestn, o, 64);
        const float os = __shfl_xor(second, o, 64);
        second = fmaxf(fmaxf(second, os), fminf(best, ov));  // runner-up of the union
        if (ov > best || (ov == best && oi < bestn)) {
          best = ov;
          bestn = oi;
        }
      }
      if ((tid & 15) == 0) {
        a.best_val[blockIdx.x * 16 + (tid >> 4)] = best;
        a.best_idx[blockIdx.x * 16 + (tid >> 4)] = bestn;
        if (a.best2_val) a.best2_val[blockIdx.x * 16 + (tid >> 4)] = second;
      }
    }
  }
}

template <int MT, bool CHUNKED, int EPI, bool NORM>
__global__ __launch_bounds__(1024) void k_gemm(GEMM_HEAD_PARAMS, GemmArgs rest) {
  gemm_body<MT, CHUNKED, EPI, NORM>(with_head<CHUNKED, NORM>(rest, GEMM_HEAD_NAMES), SampleArgs{});
}

// the W8 form (e4m3 weights, gemm_body): a name of its own, so that the bf16 kernels keep theirs
template <bool CHUNKED, int EPI, bool NORM>
__global__ __launch_bounds__(1024) void k_gemm_w8(GEMM_HEAD_PARAMS, GemmArgs rest) {
  gemm_body<1, CHUNKED, EPI, NORM, true>(with_head<CHUNKED, NORM>(rest, GEMM_HEAD_NAMES), SampleArgs{});
}

// the W13 form (lossless 13-bit bf16, gemm_body): gate/up + SiLU and lm_head + argmax, the two launches it pays for
template <int EPI, bool NORM>
__global__ __launch_bounds__(1024) void k_gemm_w13(GEMM_HEAD_PARAMS, GemmArgs rest) {
  gemm_body<1, false, EPI, NORM, false, true, EPI == EPI_SILU>(with_head<false, NORM>(rest, GEMM_HEAD_NAMES), SampleArgs{});
}

// ... and its K-chunked form (down_proj, fc: K a multiple of 2048 above 4096), one quad per item
template <int EPI>
__global__ __launch_bounds__(1024) void k_gemm_w13c(GEMM_HEAD_PARAMS, GemmArgs rest) {
  gemm_body<1, true, EPI, false, false, true>(with_head<true, false>(rest, GEMM_HEAD_NAMES), SampleArgs{});
}

// the W4 form (MXFP4 codes with their block scales, gemm_body): the draft's gate/up, lm_head and residual launches
template <bool CHUNKED, int EPI, bool NORM>
__global__ __launch_bounds__(1024) void k_gemm_w4(GEMM_HEAD_PARAMS, GemmArgs rest) {
  gemm_body<1, CHUNKED, EPI, NORM, false, false, false, true>(with_head<CHUNKED, NORM>(rest, GEMM_HEAD_NAMES), SampleArgs{});
}

template <bool NORM>
__global__ __launch_bounds__(1024) void k_gemm_s(GEMM_HEAD_PARAMS, GemmArgs rest, SampleArgs sa) {
  gemm_body<1, false, EPI_SAMPLE, NORM>(with_head<false, NORM>(rest, GEMM_HEAD_NAMES), sa);
}

// ... and its W8 form (dfl_gemm_sample on e4m3 codes): the scale on the fp32 sum, the perturbation on bf16(sum * scale)
template <bool NORM>
__global__ __launch_bounds__(1024) void k_gemm_s_w8(GEMM_HEAD_PARAMS, GemmArgs rest, SampleArgs sa) {
  gemm_body<1, false, EPI_SAMPLE, NORM, true>(with_head<false, NORM>(rest, GEMM_HEAD_NAMES), sa);
}

// the instantiation for this launch's row sources (a normalised source needs the NORM kernels)
template <int MT, bool CHUNKED, int EPI, bool W8 = false>
bool launch_gemm(GemmArgs &a, dim3 grid, hipStream_t stream) {
  bool norm = false;
  for (int mt = 0; mt < MT; ++mt) norm |= a.src[mt].mode == 2;
  a.gx = (int)grid.x;
  GemmHead h;
  if (!gemm_head<CHUNKED>(h, a)) return false;
  if constexpr (W8) {
    static_assert(MT == 1, "the W8 kernels take one 16-row tile");
    if (!a.wscale || a.KS % 2 || a.nfr % 2) {  // whole k-step pairs: per tile and per wave
      dfl_set_error("skinny GEMM (fp8): needs a scale vector, K %% 64 == 0 and an even share per wave (K=%d, nfr=%d)",
                    a.KS * 32, a.nfr);
      return false;
    }
    if constexpr (!CHUNKED) {
      if (norm) {
        hipLaunchKernelGGL((k_gemm_w8<false, EPI, true>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
        return true;
      }
    }
    hipLaunchKernelGGL((k_gemm_w8<CHUNKED, EPI, false>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
    return true;
  }
  if constexpr (!CHUNKED) {  // (the chunked form takes no normalised source: its callers reject one)
    if (norm) {
      hipLaunchKernelGGL((k_gemm<MT, false, EPI, true>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
      return true;
    }
  }
  hipLaunchKernelGGL((k_gemm<MT, CHUNKED, EPI, false>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
  return true;
}

// Bytes of a DFL_W_BF16X13 weight of N x K (dflash_hip.h): the quads of all tiles, then the {base, patch} pairs
static int64_t w13_quads_bytes(int N, int K) { return (int64_t)(N / 16) * (K / 128) * W13_QUAD_BYTES; }

// The W13 launch of dfl_gemm_silu_mul / dfl_gemm_argmax.  The layout covers whole quads per wave: K = 2048 (nfr = 4) or
// 4096 (nfr = 8); a.wp is the weight's first byte, N its packed rows.
template <int EPI>
bool launch_gemm_w13(const char *who, GemmArgs &a, const dfl_weight *w, int N, dim3 grid, hipStream_t stream) {
  if (w->scale) {
    dfl_set_error("%s: a DFL_W_BF16X13 weight takes no scale vector (the bases and patch words follow the codes)", who);
    return false;
  }
  if (a.KS % 64 || a.nfr % 4 || a.nfr * 16 != a.KS) {
    dfl_set_error("%s: DFL_W_BF16X13 covers K = 2048 and K = 4096 only (whole quads of four k-steps per wave; K=%d, %d k-steps "
                  "per wave)", who, a.KS * 32, a.nfr);
    return false;
  }
  a.wscale = reinterpret_cast<const float *>(reinterpret_cast<const char *>(w->wp) + w13_quads_bytes(N, a.KS * 32));
  a.gx = (int)grid.x;
  GemmHead h;
  if (!gemm_head<false>(h, a)) return false;
  if (a.src[0].mode == 2)
    hipLaunchKernelGGL((k_gemm_w13<EPI, true>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
  else
    hipLaunchKernelGGL((k_gemm_w13<EPI, false>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
  return true;
}

// The W4 launch of dfl_gemm_resid / dfl_gemm_silu_mul / dfl_gemm_argmax (DFL_W_MXFP4, dflash_hip.h).  a.wp is the weight's
// first byte and N its packed rows: the scale region starts N * K / 2 bytes in.  K % 128 == 0, and every wave's share is
// whole 4-k-step words (the callers round nfr up, as the W8 form rounds to even).
template <bool CHUNKED, int EPI>
bool launch_gemm_w4(const char *who, GemmArgs &a, const dfl_weight *w, int N, dim3 grid, hipStream_t stream) {
  if (w->scale) {
    dfl_set_error("%s: a DFL_W_MXFP4 weight takes no scale vector (the block scales follow the codes)", who);
    return false;
  }
  if (a.KS % 4 || a.nfr % 4 || a.nfr > 8) {
    dfl_set_error("%s: DFL_W_MXFP4 needs K %% 128 == 0 and whole 4-k-step words per wave (K=%d, %d k-steps per wave)", who,
                  a.KS * 32, a.nfr);
    return false;
  }
  a.wscale = reinterpret_cast<const float *>(reinterpret_cast<const char *>(w->wp) + (int64_t)N * a.KS * 16);
  a.gx = (int)grid.x;
  GemmHead h;
  if (!gemm_head<CHUNKED>(h, a)) return false;
  if constexpr (!CHUNKED) {
    if (a.src[0].mode == 2) {
      hipLaunchKernelGGL((k_gemm_w4<false, EPI, true>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
      return true;
    }
  }
  hipLaunchKernelGGL((k_gemm_w4<CHUNKED, EPI, false>), grid, dim3(1024), 0, stream, GEMM_HEAD_OF(h), a);
  return true;
}

// Cross-workgroup finish of the fused argmax: one wave per row.  margin_out (optional):
// top-1 minus top-2 logit of the row — the reference's only confidence statistic
// (benchmark_candidate_solutions.py:296-302: topk(2) values, a tie gives 0).
__global__ __launch_bounds__(64) void k_argmax_finish(const float *best_val, const int *best_idx, const float *best2_val,
                                                      int nblk, int row0, int nrows, const int32_t *dyn, int nrows_word,
                                                      int64_t *out_ids, int out_off, float *margin_out) {
  int rows = nrows;
  if (dyn && nrows_word >= 0) rows = dyn[nrows_word] - row0;
  const int m = row0 + blockIdx.x;
  if ((int)blockIdx.x >= rows) return;
  float bv = -INFINITY, sv = -INFINITY;
  int bi = 0x7fffffff;
  for (int b = threadIdx.x; b < nblk; b += 64) {
    const float ov = best_val[b * 16 + m];
    const int oi = best_idx[b * 16 + m];
    const float os = best2_val ? best2_val[b * 16 + m] : -INFINITY;
    if (oi != 0x7fffffff) sv = fmaxf(fmaxf(sv, os), bi == 0x7fffffff ? -INFINITY : fminf(bv, ov));
    if (ov > bv || (ov == bv && oi < bi) || bi == 0x7fffffff) {
      bv = ov;
      bi = oi;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const float os = __shfl_xor(sv, o, 64);
    const bool have = bi != 0x7fffffff, ohave = oi != 0x7fffffff;
    sv = fmaxf(sv, os);
    if (have && ohave) sv = fmaxf(sv, fminf(bv, ov));
    if (ohave && (!have || ov > bv || (ov == bv && oi < bi))) {
      bv = ov;
      bi = oi;
    }
  }
  if (threadIdx.x == 0) {
    out_ids[out_off + blockIdx.x] = (int64_t)bi;
    if (margin_out) margin_out[out_off + blockIdx.x] = bv - sv;
  }
}

// ---- one-time packing ---------------------------------------------------------
// out chunk index c = ((t*KS + ks)*64 + l): 16 B from W[t*16 + (l&15)][ks*32 + (l>>4)*8 ...]
__global__ void k_pack_weight(const bf16x8 *__restrict__ w, bf16x8 *__restrict__ wp, int ntiles, int KS,
                              int tile_mul, int tile_add) {
  const size_t total = (size_t)ntiles * KS * 64;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < total; c += (size_t)gridDim.x * blockDim.x) {
    const int l = c & 63;
    const size_t tk = c >> 6;
    const int ks = tk % KS;
    const size_t t = tk / KS;
    const size_t row = t * 16 + (l & 15);
    const size_t src = row * (size_t)(KS * 4) + (size_t)ks * 4 + (l >> 4);  // in 16-B units
    const size_t dt = t * tile_mul + tile_add;
    wp[(dt * KS + ks) * 64 + l] = w[src];
  }
}

// The W8 layout (gemm_rows.h): a byte permutation of row-major e4m3 codes q [N][K].  Out word c = ((t*KP + j)*64 + l),
// KP = K / 64: bytes 0-7 from q[t*16 + (l&15)][64j + 8(l>>4) ..], bytes 8-15 from 32 columns further on.
__global__ void k_pack_weight_fp8(const uint2 *__restrict__ q, uint4 *__restrict__ wp, int ntiles, int KP, int tile_mul,
                                  int tile_add) {
  const size_t total = (size_t)ntiles * KP * 64;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < total; c += (size_t)gridDim.x * blockDim.x) {
    const int l = c & 63;
    const size_t tj = c >> 6;
    const int j = tj % KP;
    const size_t t = tj / KP;
    const size_t row = t * 16 + (l & 15);
    const size_t src = row * (size_t)(KP * 8) + (size_t)j * 8 + (l >> 4);  // in 8-byte units
    const uint2 lo = q[src], hi = q[src + 4];
    const size_t dt = t * tile_mul + tile_add;
    wp[(dt * KP + j) * 64 + l] = make_uint4(lo.x, lo.y, hi.x, hi.y);
  }
}

// h[m] = embed[ids[m]] (bf16 rows) and the rows' sums of squares (one partial per row)
__global__ __launch_bounds__(256) void k_embed_rows(const bf16_t *embed, const int64_t *ids, bf16_t *h, int H,
                                                    float *ss_out, const int32_t *dyn, int dyn_word) {
  __shared__ float wsum[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int nv = dyn ? dyn[dyn_word] : 16;
  float ss = 0.f;
  if (m < nv) {
    const bf16_t *src = embed + ids[m] * (int64_t)H;
    for (int c = tid; c < (H >> 3); c += 256) {
      const bf16x8 v = *reinterpret_cast<const bf16x8 *>(src + c * 8);
      *reinterpret_cast<bf16x8 *>(h + (int64_t)m * H + c * 8) = v;
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += bf2f(v[j]) * bf2f(v[j]);
    }
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) wsum[tid >> 6] = ss;
  __syncthreads();
  if (tid == 0) ss_out[m] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

}  // namespace

#ifdef DFL_GEMM_STAMPS
extern "C" int dfl_debug_read_gemm_stamps(unsigned long long *host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_gstamps), sizeof(unsigned long long) * 8);
}
extern "C" int dfl_debug_read_wg_stamps(unsigned long long *host_out) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_wgstamps), sizeof(unsigned long long) * 256 * 4);
}
#endif

// Grid and tile split of a launch over `ntiles` column tiles (single K pass).  When the tiles do not divide over the
// 256 CUs and the remainder is at most half a round (r <= 128), the last r tiles are cut in 8-column halves, one for
// each of 2r workgroups: every CU streams within half a tile of the same byte count.  (qkv of an 8B model: 384 tiles =
// 1.5 per workgroup on 256 CUs instead of 2 on 192 of them; lm_head: 9496 = 37 x 256 + 24.)
static void plan_tiles(GemmArgs &a, int ntiles, bool allow_half, int &gx) {
  gx = grid_x_for(ntiles);
  a.ntiles = ntiles;
  a.nhalf = 0;
  const int r = ntiles % 256;
  // (round 4) at most 128 tiles: ALL of them in halves, one per workgroup — twice the CUs stream half the bytes each
  // (o_proj / down_proj of a hidden-2048 model: 128 workgroups of one 16-column tile were half the chip).
  if (allow_half && ntiles <= 128) {
    gx = 2 * ntiles;
    a.ntiles = 0;
    a.nhalf = 2 * ntiles;
    return;
  }
  if (!allow_half || ntiles <= 256 || r == 0 || r > 128) return;
  gx = 256;
  a.ntiles = ntiles - r;
  a.nhalf = 2 * r;
}

extern "C" int dfl_pack_weight(const void *w, void *wp, int N, int K, void *stream) {
  DFL_REQUIRE(w && wp, "dfl_pack_weight: null pointer");
  DFL_REQUIRE(N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0, "dfl_pack_weight: need N%%16==0, K%%32==0 (N=%d K=%d)", N, K);
  hipLaunchKernelGGL(k_pack_weight, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const bf16x8 *)w, (bf16x8 *)wp,
                     N / 16, K / 32, 1, 0);
  DFL_CHECK_LAUNCH("dfl_pack_weight");
  return DFL_OK;
}

extern "C" int dfl_pack_weight_gateup(const void *gate, const void *up, void *wp, int I, int K, void *stream) {
  DFL_REQUIRE(gate && up && wp, "dfl_pack_weight_gateup: null pointer");
  DFL_REQUIRE(I > 0 && K > 0 && I % 16 == 0 && K % 32 == 0, "dfl_pack_weight_gateup: need I%%16==0, K%%32==0");
  hipLaunchKernelGGL(k_pack_weight, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const bf16x8 *)gate,
                     (bf16x8 *)wp, I / 16, K / 32, 2, 0);
  hipLaunchKernelGGL(k_pack_weight, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const bf16x8 *)up, (bf16x8 *)wp,
                     I / 16, K / 32, 2, 1);
  DFL_CHECK_LAUNCH("dfl_pack_weight_gateup");
  return DFL_OK;
}

extern "C" int dfl_pack_weight_fp8(const void *q, void *wp8, int N, int K, void *stream) {
  DFL_REQUIRE(q && wp8, "dfl_pack_weight_fp8: null pointer");
  DFL_REQUIRE(N > 0 && K > 0 && N % 16 == 0 && K % 64 == 0, "dfl_pack_weight_fp8: need N%%16==0, K%%64==0 (N=%d K=%d)", N, K);
  hipLaunchKernelGGL(k_pack_weight_fp8, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const uint2 *)q, (uint4 *)wp8,
                     N / 16, K / 64, 1, 0);
  DFL_CHECK_LAUNCH("dfl_pack_weight_fp8");
  return DFL_OK;
}

extern "C" int dfl_pack_weight_gateup_fp8(const void *gate_q, const void *up_q, void *wp8, int I, int K, void *stream) {
  DFL_REQUIRE(gate_q && up_q && wp8, "dfl_pack_weight_gateup_fp8: null pointer");
  DFL_REQUIRE(I > 0 && K > 0 && I % 16 == 0 && K % 64 == 0, "dfl_pack_weight_gateup_fp8: need I%%16==0, K%%64==0 (I=%d K=%d)", I,
              K);
  hipLaunchKernelGGL(k_pack_weight_fp8, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const uint2 *)gate_q, (uint4 *)wp8,
                     I / 16, K / 64, 2, 0);
  hipLaunchKernelGGL(k_pack_weight_fp8, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const uint2 *)up_q, (uint4 *)wp8,
                     I / 16, K / 64, 2, 1);
  DFL_CHECK_LAUNCH("dfl_pack_weight_gateup_fp8");
  return DFL_OK;
}

extern "C" int dfl_embed_rows(const void *embed, const int64_t *ids, void *h_out, int H, float *ss_out,
                              const int32_t *dyn, int dyn_word, void *stream) {
  DFL_REQUIRE(embed && ids && h_out && ss_out, "dfl_embed_rows: null pointer");
  DFL_REQUIRE(H > 0 && H % 8 == 0, "dfl_embed_rows: H%%8 != 0");
  hipLaunchKernelGGL(k_embed_rows, dim3(16), dim3(256), 0, (hipStream_t)stream, (const bf16_t *)embed, ids,
                     (bf16_t *)h_out, H, ss_out, dyn, dyn_word);
  DFL_CHECK_LAUNCH("dfl_embed_rows");
  return DFL_OK;
}

extern "C" int dfl_gemm_f32(const void *wp, const dfl_rows *x0, const dfl_rows *x1, int mt, int N, int K, int ksplit,
                            float *out, const int32_t *dyn, void *stream) {
  DFL_REQUIRE(wp && out, "dfl_gemm_f32: null pointer");
  DFL_REQUIRE(mt == 1 || mt == 2, "dfl_gemm_f32: mt must be 1 or 2");
  DFL_REQUIRE(N > 0 && K > 0 && N % 16 == 0 && K % 32 == 0, "dfl_gemm_f32: need N%%16==0, K%%32==0 (N=%d K=%d)", N, K);
  const int KS = K / 32;
  const int fr_max = mt == 1 ? 8 : 4;
  DFL_REQUIRE(ksplit >= pick_ksplit_min(KS, fr_max) && ksplit <= 64, "dfl_gemm_f32: ksplit=%d too small for K=%d (need >= %d)",
              ksplit, K, pick_ksplit_min(KS, fr_max));
  GemmArgs a{};
  if (!fill_src(a.src[0], x0, K, "dfl_gemm_f32")) return DFL_EINVAL;
  if (mt == 2 && !fill_src(a.src[1], x1, K, "dfl_gemm_f32")) return DFL_EINVAL;
  a.wp = (const bf16x8 *)wp;
  a.dyn = dyn;
  a.KS = KS;
  a.ntiles = N / 16;
  a.nfr = (KS + 16 * ksplit - 1) / (16 * ksplit);
  a.nch = 1;
  a.out = out;
  a.ldo = N;
  int gx1 = 0;
  if (ksplit == 1) plan_tiles(a, N / 16, true, gx1);
  dim3 grid(ksplit == 1 ? gx1 : grid_x_for(a.ntiles, ksplit), ksplit);
  const bool ok = mt == 1 ? launch_gemm<1, false, EPI_F32>(a, grid, (hipStream_t)stream)
                          : launch_gemm<2, false, EPI_F32>(a, grid, (hipStream_t)stream);
  if (!ok) return DFL_EINVAL;
  DFL_CHECK_LAUNCH("dfl_gemm_f32");
  return DFL_OK;
}

// The entry points that take a dfl_weight: one body for both formats.  W8 = the weights are e4m3 codes in the W8 layout
// with one fp32 scale per packed row (w->scale), K % 64 == 0, and every wave's share (nfr) is rounded up to whole k-step
// pairs.
namespace {
template <bool W8, bool W13 = false, bool W4 = false>
int gemm_silu_mul_impl(const char *who, const dfl_weight *w, const dfl_rows *x, int I, int K, void *act_frag,
                       const int32_t *dyn, void *stream) {
  DFL_REQUIRE(w->wp && act_frag && (!W8 || w->scale), "%s: null pointer", who);
  DFL_REQUIRE(I > 0 && K > 0 && I % 16 == 0 && K % (W4 ? 128 : W8 ? 64 : 32) == 0, "%s: need I%%16==0, K%%%d==0", who,
              W4 ? 128 : W8 ? 64 : 32);
  const int KS = K / 32;
  DFL_REQUIRE(KS <= 16 * 8, "%s: K=%d needs a K split, which the fused activation cannot take", who, K);
  GemmArgs a{};
  if (!fill_src(a.src[0], x, K, who)) return DFL_EINVAL;
  a.wp = (const bf16x8 *)w->wp;
  a.wscale = w->scale;
  a.dyn = dyn;
  a.KS = KS;
  a.ntiles = 2 * (I / 16);
  a.nfr = (KS + 15) / 16;
  if (W8) a.nfr += a.nfr & 1;
  if (W4) a.nfr = (a.nfr + 3) & ~3;
  a.nch = 1;
  a.act = (bf16_t *)act_frag;
  if constexpr (W4) {
    if (!launch_gemm_w4<false, EPI_SILU>(who, a, w, 2 * I, dim3(grid_x_for(I / 16), 1), (hipStream_t)stream)) return DFL_EINVAL;
  } else if constexpr (W13) {
    if (!launch_gemm_w13<EPI_SILU>(who, a, w, 2 * I, dim3(grid_x_for(I / 16), 1), (hipStream_t)stream)) return DFL_EINVAL;
  } else if (!launch_gemm<1, false, EPI_SILU, W8>(a, dim3(grid_x_for(I / 16), 1), (hipStream_t)stream)) {
    return DFL_EINVAL;
  }
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}
}  // namespace

extern "C" int dfl_gemm_silu_mul(const dfl_weight *w_gateup, const dfl_rows *x, int I, int K, void *act_frag,
                                 const int32_t *dyn, void *stream) {
  const char *who = "dfl_gemm_silu_mul";
  if (w_gateup && w_gateup->format == DFL_W_BF16X13)  // (weight_ok knows the two formats every entry point takes)
    return gemm_silu_mul_impl<false, true>(who, w_gateup, x, I, K, act_frag, dyn, stream);
  if (w_gateup && w_gateup->format == DFL_W_MXFP4)
    return gemm_silu_mul_impl<false, false, true>(who, w_gateup, x, I, K, act_frag, dyn, stream);
  if (!weight_ok(who, w_gateup)) return DFL_EINVAL;
  return w_gateup->format == DFL_W_BF16 ? gemm_silu_mul_impl<false>(who, w_gateup, x, I, K, act_frag, dyn, stream)
                                        : gemm_silu_mul_impl<true>(who, w_gateup, x, I, K, act_frag, dyn, stream);
}

// One launch for the gate/up projection of EVERY active expert of a sparse-MoE layer (Qwen3-MoE:
// tf:models/qwen3_moe/modeling_qwen3_moe.py, Qwen3MoeExperts.forward: act_fn(gate) * up per expert).  The 16 block rows
// are one MFMA tile whatever subset of them an expert serves, so an expert costs its weight bytes once.  One workgroup
// per CU; each builds its activation fragments ONCE and walks its share of the (active expert, gate/up pair) items,
// the next item's weights prefetched under the current one — round 2, first form: grid.z = expert, 8 workgroups per
// expert, every one with its own prologue and no overlap between successive workgroups of a CU: 4.7 TB/s at 82
// active experts (109.6 us per layer of a 30B-A3B-shaped target).
extern "C" int dfl_gemm_silu_mul_experts(const void *wp_gateup, int64_t wp_expert_stride, const dfl_rows *x, int E, int I, int K,
                                         void *act_frag, int64_t act_expert_stride, const int32_t *list,
                                         const int32_t *n_active, const int32_t *dyn, void *stream) {
  DFL_REQUIRE(wp_gateup && act_frag && list && n_active, "dfl_gemm_silu_mul_experts: null pointer");
  DFL_REQUIRE(E >= 1 && E <= 1024 && I > 0 && K > 0 && I % 16 == 0 && K % 32 == 0, "dfl_gemm_silu_mul_experts: bad shape");
  DFL_REQUIRE(wp_expert_stride == (int64_t)2 * I * K && act_expert_stride == (int64_t)16 * I,
              "dfl_gemm_silu_mul_experts: the experts' weights and outputs must lie back to back (strides %lld, %lld)",
              (long long)wp_expert_stride, (long long)act_expert_stride);
  const int KS = K / 32;
  DFL_REQUIRE(KS <= 16 * 8, "dfl_gemm_silu_mul_experts: K=%d exceeds 4096", K);
  GemmArgs a{};
  if (!fill_src(a.src[0], x, K, "dfl_gemm_silu_mul_experts")) return DFL_EINVAL;
  a.wp = (const bf16x8 *)wp_gateup;
  a.dyn = dyn;
  a.KS = KS;
  a.ntiles = 2 * (I / 16) * E;
  a.nfr = (KS + 15) / 16;
  a.nch = 1;
  a.act = (bf16_t *)act_frag;
  a.elist = list;
  a.n_active = n_active;
  a.npp = I / 16;
  if (!launch_gemm<1, false, EPI_SILU_E>(a, dim3(256, 1), (hipStream_t)stream)) return DFL_EINVAL;
  DFL_CHECK_LAUNCH("dfl_gemm_silu_mul_experts");
  return DFL_OK;
}

extern "C" int64_t dfl_argmax_ws_bytes(void) { return 256 * 16 * (int64_t)(2 * sizeof(float) + sizeof(int)); }

namespace {
// who: dfl_gemm_argmax, or dfl_gemm_sample with its draw in smp; w has passed weight_ok
int gemm_argmax_impl(const char *who, const dfl_weight *w, const dfl_rows *x, int V, int K, int row0, int nrows,
                     const int32_t *dyn, int nrows_dyn_word, void *ws, int64_t *out_ids, int out_off, void *logits,
                     float *margin_out, hipEvent_t ev0, hipEvent_t ev1, void *stream, const SampleArgs *smp = nullptr) {
  const bool w8 = w->format == DFL_W_E4M3, w13 = w->format == DFL_W_BF16X13, w4 = w->format == DFL_W_MXFP4;
  DFL_REQUIRE(w->wp && ws && out_ids && (!w8 || w->scale), "%s: null pointer", who);
  DFL_REQUIRE(V > 0 && K > 0 && V % 16 == 0 && K % (w4 ? 128 : w8 ? 64 : 32) == 0, "%s: need V%%16==0, K%%%d==0 (V=%d K=%d)", who,
              w4 ? 128 : w8 ? 64 : 32, V, K);
  DFL_REQUIRE(row0 >= 0 && nrows >= 0 && row0 + nrows <= 16, "%s: rows [%d,%d) outside the 16-row tile", who, row0,
              row0 + nrows);
  const int KS = K / 32;
  DFL_REQUIRE(KS <= 16 * 8, "%s: K=%d exceeds 4096 (argmax needs finished sums)", who, K);
  GemmArgs a{};
  if (!fill_src(a.src[0], x, K, who)) return DFL_EINVAL;
  a.wp = (const bf16x8 *)w->wp;
  a.dyn = dyn;
  a.KS = KS;
  a.ntiles = V / 16;
  a.nfr = (KS + 15) / 16;
  if (w8) a.nfr += a.nfr & 1;
  if (w4) a.nfr = (a.nfr + 3) & ~3;
  a.wscale = w->scale;
  a.nch = 1;
  a.row0 = row0;
  a.nrows = nrows;
  a.nrows_word = nrows_dyn_word;
  a.best_val = (float *)ws;
  a.best_idx = (int *)((char *)ws + 256 * 16 * sizeof(float));
  a.best2_val = margin_out ? (float *)((char *)ws + 256 * 16 * (sizeof(float) + sizeof(int))) : nullptr;
  a.logits = (bf16_t *)logits;
  a.N = V;
  int gx = 0;
  plan_tiles(a, V / 16, true, gx);
  if (ev0) (void)hipEventRecord(ev0, (hipStream_t)stream);
  if (smp) {
    a.gx = gx;
    GemmHead h;
    if (!gemm_head<false>(h, a)) return DFL_EINVAL;
    if (w8) {  // (K % 64 and the scale vector are checked above; nfr is even: whole k-step pairs per wave)
      if (a.src[0].mode == 2)
        hipLaunchKernelGGL(k_gemm_s_w8<true>, dim3(gx, 1), dim3(1024), 0, (hipStream_t)stream, GEMM_HEAD_OF(h), a, *smp);
      else
        hipLaunchKernelGGL(k_gemm_s_w8<false>, dim3(gx, 1), dim3(1024), 0, (hipStream_t)stream, GEMM_HEAD_OF(h), a, *smp);
    } else if (a.src[0].mode == 2)
      hipLaunchKernelGGL(k_gemm_s<true>, dim3(gx, 1), dim3(1024), 0, (hipStream_t)stream, GEMM_HEAD_OF(h), a, *smp);
    else
      hipLaunchKernelGGL(k_gemm_s<false>, dim3(gx, 1), dim3(1024), 0, (hipStream_t)stream, GEMM_HEAD_OF(h), a, *smp);
  } else if (w13) {
    if (!launch_gemm_w13<EPI_ARGMAX>(who, a, w, V, dim3(gx, 1), (hipStream_t)stream)) return DFL_EINVAL;
  } else if (w4) {
    if (!launch_gemm_w4<false, EPI_ARGMAX>(who, a, w, V, dim3(gx, 1), (hipStream_t)stream)) return DFL_EINVAL;
  } else if (w8) {
    if (!launch_gemm<1, false, EPI_ARGMAX, true>(a, dim3(gx, 1), (hipStream_t)stream)) return DFL_EINVAL;
  } else {
    if (!launch_gemm<1, false, EPI_ARGMAX>(a, dim3(gx, 1), (hipStream_t)stream)) return DFL_EINVAL;
  }
  if (ev1) (void)hipEventRecord(ev1, (hipStream_t)stream);
  hipLaunchKernelGGL(k_argmax_finish, dim3(16), dim3(64), 0, (hipStream_t)stream, a.best_val, a.best_idx, a.best2_val, gx,
                     row0, nrows, dyn, nrows_dyn_word, out_ids, out_off, margin_out);
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}
}  // namespace

extern "C" int dfl_gemm_argmax(const dfl_weight *w, const dfl_rows *x, int V, int K, int row0, int nrows,
                               const int32_t *dyn, int nrows_dyn_word, void *ws, int64_t *out_ids, int out_off,
                               void *logits, float *margin_out, void *ev_start, void *ev_end, void *stream) {
  const char *who = "dfl_gemm_argmax";
  if (!(w && (w->format == DFL_W_BF16X13 || w->format == DFL_W_MXFP4)) && !weight_ok(who, w)) return DFL_EINVAL;
  return gemm_argmax_impl(who, w, x, V, K, row0, nrows, dyn, nrows_dyn_word, ws, out_ids, out_off, logits, margin_out,
                          (hipEvent_t)ev_start, (hipEvent_t)ev_end, stream);
}

extern "C" int dfl_gemm_sample(const dfl_weight *w, const dfl_rows *x, int V, int K, int row0, int nrows,
                               const int32_t *dyn, int nrows_dyn_word, void *ws, int64_t *out_ids, int out_off,
                               void *logits, float *margin_out, uint64_t seed, float inv_t, int rng_stream,
                               const int32_t *pos_dyn, int pos_word, int pos_base, int pos_add, void *stream) {
  const char *who = "dfl_gemm_sample";
  if (!weight_ok(who, w)) return DFL_EINVAL;
  DFL_REQUIRE(w->wp && (w->format == DFL_W_BF16 || w->scale) && ws && out_ids, "%s: null pointer", who);
  DFL_REQUIRE(inv_t > 0.f && inv_t <= 1e5f, "%s: inv_t=%g outside (0, 1e5]", who, (double)inv_t);
  DFL_REQUIRE(rng_stream == (int)DFL_RNG_TARGET || rng_stream == (int)DFL_RNG_DRAFT, "%s: unknown stream %d", who,
              rng_stream);
  DFL_REQUIRE(!pos_dyn || (pos_word >= 0 && pos_word < DFL_DYN_WORDS), "%s: pos_word=%d outside the record", who, pos_word);
  const SampleArgs smp{seed, inv_t, rng_stream, pos_dyn, pos_word, pos_base, pos_add};
  return gemm_argmax_impl(who, w, x, V, K, row0, nrows, dyn, nrows_dyn_word, ws, out_ids, out_off, logits, margin_out,
                          nullptr, nullptr, stream, &smp);
}


namespace {
template <bool W8, bool W13 = false, bool W4 = false>
int gemm_resid_impl(const char *who, const dfl_weight *w, const dfl_rows *x, int N, int K, void *h_io, int64_t ldh,
                    int add_residual, void *tap, int64_t ldtap, float *ss_out, const int32_t *dyn, void *stream) {
  DFL_REQUIRE(w->wp && h_io && (!W8 || w->scale), "%s: null pointer", who);
  DFL_REQUIRE(N > 0 && K > 0 && N % 16 == 0 && K % (W4 ? 128 : W8 ? 64 : 32) == 0, "%s: need N%%16==0, K%%%d==0 (N=%d K=%d)", who,
              W4 ? 128 : W8 ? 64 : 32, N, K);
  DFL_REQUIRE(ldh >= N && (!tap || ldtap >= N), "%s: row strides shorter than N", who);
  const int KS = K / 32;
  GemmArgs a{};
  if (!fill_src(a.src[0], x, K, who)) return DFL_EINVAL;
  a.wp = (const bf16x8 *)w->wp;
  a.wscale = w->scale;
  a.dyn = dyn;
  a.KS = KS;
  a.ntiles = N / 16;
  a.h_io = (bf16_t *)h_io;
  a.ldh = ldh;
  a.add_resid = add_residual ? 1 : 0;
  a.tap = (bf16_t *)tap;
  a.ldtap = ldtap;
  a.ss_out = ss_out;
  int gx = 0;
  // (a half tile has no slot of its own in ss_out: launches that leave sums of squares keep whole tiles)
  plan_tiles(a, N / 16, KS <= 16 * 8 && !ss_out, gx);
  const dim3 grid(gx, 1);
  if (KS <= 16 * 8) {  // the whole K fits the 16 waves x 8 steps of one pass
    a.nfr = (KS + 15) / 16;
    if (W8) a.nfr += a.nfr & 1;
    if (W4) a.nfr = (a.nfr + 3) & ~3;
    a.nch = 1;
    if constexpr (W4) {
      if (!launch_gemm_w4<false, EPI_RESID>(who, a, w, N, grid, (hipStream_t)stream)) return DFL_EINVAL;
    } else if (!launch_gemm<1, false, EPI_RESID, W8>(a, grid, (hipStream_t)stream)) {
      return DFL_EINVAL;
    }
  } else {  // walk K in chunks of 16 waves x 4 steps inside the workgroup
    DFL_REQUIRE(a.src[0].mode != 2, "%s: a normalised source needs K <= 4096", who);
    a.nfr = 4;
    a.nch = (KS + 63) / 64;  // 64 k-steps per chunk: 16 waves x 4
    if constexpr (W4) {
      if (!launch_gemm_w4<true, EPI_RESID>(who, a, w, N, grid, (hipStream_t)stream)) return DFL_EINVAL;
    } else if constexpr (W13) {  // (dfl_gemm_resid: K is a whole number of chunks, no scale; whole tiles only — KS > 128 above)
      a.wscale = reinterpret_cast<const float *>(reinterpret_cast<const char *>(w->wp) + w13_quads_bytes(N, K));
      a.gx = (int)grid.x;
      GemmHead h;
      if (!gemm_head<true>(h, a)) return DFL_EINVAL;
      hipLaunchKernelGGL((k_gemm_w13c<EPI_RESID>), grid, dim3(1024), 0, (hipStream_t)stream, GEMM_HEAD_OF(h), a);
    } else if (!launch_gemm<1, true, EPI_RESID, W8>(a, grid, (hipStream_t)stream)) {
      return DFL_EINVAL;
    }
  }
  DFL_CHECK_LAUNCH(who);
  return DFL_OK;
}
}  // namespace

extern "C" int dfl_gemm_resid(const dfl_weight *w, const dfl_rows *x, int N, int K, void *h_io, int64_t ldh,
                              int add_residual, void *tap, int64_t ldtap, float *ss_out, const int32_t *dyn,
                              void *stream) {
  const char *who = "dfl_gemm_resid";
  // the 13-bit form where its K-chunked layout covers the launch; any other K falls through to weight_ok's refusal
  if (w && w->format == DFL_W_BF16X13 && K > 4096 && K % 2048 == 0) {
    DFL_REQUIRE(!w->scale, "%s: a DFL_W_BF16X13 weight takes no scale vector (the bases and patch words follow the codes)", who);
    return gemm_resid_impl<false, true>(who, w, x, N, K, h_io, ldh, add_residual, tap, ldtap, ss_out, dyn, stream);
  }
  if (w && w->format == DFL_W_MXFP4)
    return gemm_resid_impl<false, false, true>(who, w, x, N, K, h_io, ldh, add_residual, tap, ldtap, ss_out, dyn, stream);
  if (!weight_ok(who, w)) return DFL_EINVAL;
  return w->format == DFL_W_BF16
             ? gemm_resid_impl<false>(who, w, x, N, K, h_io, ldh, add_residual, tap, ldtap, ss_out, dyn, stream)
             : gemm_resid_impl<true>(who, w, x, N, K, h_io, ldh, add_residual, tap, ldtap, ss_out, dyn, stream);
}
