// Pieces shared by the skinny GEMM kernels (gemm_skinny.hip: one request;
// gemm_batch.hip: a ragged batch of requests over one weight stream).
#pragma once
#include "dfl_common.h"

namespace {

enum { EPI_F32 = 0, EPI_SILU = 1, EPI_ARGMAX = 2, EPI_RESID = 3, EPI_SILU_E = 4 /* SILU over a list of active experts */,
       EPI_SAMPLE = 5 /* EPI_ARGMAX over bf16(logit) * invT + Gumbel noise (dfl_rng.h) */,
       EPI_SAMPLE_T = 6 /* EPI_SAMPLE with invT per request slot from a device array; !(invT > 0): that slot's plain argmax */ };

struct RowSrc {
  const bf16x8 *frag;  // mode 0: frag16 [KS][64]
  const bf16_t *rows;  // mode 1/2: row-major [16][K], row stride ld
  int64_t ld;
  const float *ss;     // mode 2: [nss][16] partial sums of squares per row
  int nss;
  const bf16_t *nw;    // mode 2: RMSNorm weight [K]
  float eps;
  int valid_word;      // dyn word with the number of valid rows, < 0: all 16
  int mode;
};

__device__ __forceinline__ bf16x8 ld_stream(const bf16x8 *p) { return __builtin_nontemporal_load(p); }

// Up to NF consecutive k-steps (1 KiB each, wave-wide) of a packed column tile, starting at
// `first` (= tile base + ks0 * 64), as buffer loads: the descriptor (first, nf KiB) sits in
// SGPRs, the lane offset is one constant VGPR, k-step offsets go to the immediate / scalar
// offset fields — no 64-bit VGPR address per fragment.  A k-step >= nf (past the wave's share
// or past K) is outside the descriptor's range: it returns ZERO and costs no memory traffic,
// so neither the loads nor the MFMAs that consume them need a guard (guards around loads make
// hipcc wait vmcnt(0) per fragment; zero weights add zero).
// `half` (0 / 1; -1 = the whole tile): only the lanes of columns 8*half .. 8*half+7 of the 16-column tile load (lane l
// holds column l & 15); the others get an offset past the descriptor, i.e. zeros and no traffic — branch-free.
template <int NF, int AUX = 2 /* nt: streamed once; 0 for fragments many workgroups re-read from L2 */>
__device__ __forceinline__ void load_ksteps(bf16x8 (&wr)[NF], const bf16x8 *first, int nf, int l, int half = -1) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16x8 *>(first), 0, (nf < 0 ? 0 : nf) * 1024, 0x00020000);
  const int voff = (half < 0 || ((l >> 3) & 1) == half) ? l * 16 : 0x40000000;
#pragma unroll
  for (int f = 0; f < NF; ++f)
    wr[f] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff + (f & 3) * 1024, (f >> 2) * 4096, AUX));
}

// ---- W8: weights stored as OCP e4m3 codes (one byte each), converted to bf16 in registers (exact) ----
// Packed layout [N/16][K/64][64 lanes][16 B]: lane l (column l & 15, kq = l >> 4) holds the 8 codes of k-step 2j
// (k = 64j + 8kq ..) in bytes 0-7 and those of k-step 2j+1 (k = 64j + 32 + 8kq ..) in bytes 8-15, so one 16-byte load
// per lane is still one contiguous 1 KiB wave request and carries TWO MFMA A-fragments.
// The W8 form of load_ksteps: the wave's NF k-steps (NF even) as NF/2 loads; `nf` (k-steps of the wave's share, even)
// clips the descriptor at nf * 512 bytes.  The raw 16-byte words stay in flight as they are (half the registers of the
// bf16 form); w8_frag turns one into the fragment of k-step f right in front of its MFMA.
template <int NF, int AUX = 2>
__device__ __forceinline__ void load_ksteps_w8(bf16x8 (&wr)[NF / 2], const bf16x8 *first, int nf, int l, int half = -1) {
  static_assert(NF % 2 == 0, "W8: a wave's share is a whole number of k-step pairs");
  load_ksteps<NF / 2, AUX>(wr, first, nf >> 1, l, half);
}

// the 8 e4m3 codes in half `hi` (0: bytes 0-7, 1: bytes 8-15) of one 16-byte word -> bf16x8
__device__ __forceinline__ bf16x8 w8_frag(bf16x8 raw, int hi) {
  const u32x4 q = __builtin_bit_cast(u32x4, raw);
  const uint32_t d0 = hi ? q[2] : q[0], d1 = hi ? q[3] : q[1];
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, 1.0f, true);
  return (bf16x8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

// fragment of k-step f of an item's weight registers: bf16 words as loaded, or converted from e4m3
template <bool W8, int NW>
__device__ __forceinline__ bf16x8 weight_frag(const bf16x8 (&wr)[NW], int f) {
  if constexpr (W8)
    return w8_frag(wr[f >> 1], f & 1);
  else
    return wr[f];
}

// ---- W4: weights stored as OCP MXFP4 — e2m1 codes, one e8m0 scale per 32 consecutive k of a row (DFL_W_MXFP4) ----
// Codes [N/16][K/128][64 lanes][16 B]: lane l (column l & 15, kq = l >> 4) holds in dword d of its 16-byte word the 8 codes
// of k-step 4 j + d (k = 128 j + 32 d + 8 kq ..), low nibble first — so one 16-byte load per lane is still one contiguous
// 1 KiB wave request and carries FOUR MFMA A-fragments, and one k-step fragment of one column is exactly one MX block.
// Scales behind the codes: e8m0 bytes [N/16][K/128][16 columns][4 B], one dword per (column, 128-k group), byte d the scale
// of k-step 4 j + d.
// The W4 form of load_ksteps: the wave's NF k-steps (NF % 4 == 0) as NF/4 weight loads and NF/4 scale dwords, both through
// descriptors that clip at the wave's share `nf` (k-steps, % 4 == 0): a clipped read is code 0 under scale code 0, i.e. +0.
// The scale dwords are requested IN FRONT of the words they scale (a wave's loads return in order: the first conversion
// then waits for one small request and one word).  The raw words stay in flight as they are — a quarter of the bf16
// form's registers; w4_frag turns dword f & 3 into the fragment of k-step f right in front of its MFMA.
template <int NF, int AUX = 2>
__device__ __forceinline__ void load_ksteps_w4(bf16x8 (&wr)[NF / 4], uint32_t (&sc)[2], const bf16x8 *first,
                                               const char *first_scale, int nf, int l, int half = -1) {
  static_assert(NF % 4 == 0 && NF <= 8, "W4: a wave's share is a whole number of 4-k-step words (at most two)");
  const int nw = nf < 0 ? 0 : nf >> 2;
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(first_scale), 0, nw * 64, 0x00020000);
  const bool mine = half < 0 || ((l >> 3) & 1) == half;
  const int voff4 = mine ? (l & 15) * 4 : 0x40000000;
#pragma unroll
  for (int q = 0; q < NF / 4; ++q) sc[q] = __builtin_amdgcn_raw_buffer_load_b32(rs, voff4 + q * 64, 0, AUX);
  load_ksteps<NF / 4, AUX>(wr, first, nw, l, half);
}

// the 8 e2m1 codes in dword d (0..3) of one 16-byte word, times 2^(scale byte d - 127) -> bf16x8 (exact: the block scale
// rides in the conversion, so the launch has no epilogue multiply)
__device__ __forceinline__ bf16x8 w4_frag(bf16x8 raw, uint32_t scales, int d) {
  const uint32_t q = __builtin_bit_cast(u32x4, raw)[d];
  const float s = __builtin_bit_cast(float, ((scales >> (8 * d)) & 0xffu) << 23);
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 2);
  const bf16x2 e = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(q, s, 3);
  return (bf16x8){a[0], a[1], b[0], b[1], c[0], c[1], e[0], e[1]};
}

// ---- W13: bf16 weights stored losslessly in 13 bits (DFL_W_BF16X13, dflash_hip.h) ----
// A bf16 is L = bits[7:0] (e0, m6..m0) and H = bits[15:8] (s, e7..e1).  Per packed 16-column tile, hb = max(0, max(H & 0x7f)
// - 15); a weight keeps L, its sign and a 4-bit code c: c = 0 <=> (H & 0x7f) == 0, c = 1..15 <=> (H & 0x7f) == hb + c.
// Unit of the layout: a QUAD of four k-steps of one tile, 3328 bytes = four lane-linear planes
//   L0 [64 lanes][16 B]  L bytes of k-step 0 (bytes 0-7: elements 0..7) and k-step 1 (bytes 8-15)
//   L1 [64 lanes][16 B]  the same of k-steps 2 and 3
//   NB [64 lanes][16 B]  dword f = the codes of k-step f: byte b = c[b] | c[b + 4] << 4
//   SG [64 lanes][ 4 B]  bit 8 b + r = the sign of element 4 (r & 1) + b of k-step r >> 1
// with lane l = (column l & 15, kq = l >> 4) as in the bf16 form, so the half-tile lane rule carries over.  A tile is
// K / 128 quads back to back; a wave's share is nfr / 4 of them (nfr = 4 or 8: K = 2048 or 4096), so the descriptor
// clips at whole quads, and a clipped read (all bits zero) decodes to +0 as the bf16 form's does.
// Behind the quads of all tiles: meta [ntiles][16 waves] of {hb, patch} dword pairs, read by a scalar load.  patch:
// bit 31 valid, 30:28 k-step of the wave's share, 27:22 lane, 21:19 element, 15:0 the bf16 itself — the one nonzero
// weight of that (tile, wave) item that lies below the window (its stored code is 0).
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
#define W13_QUAD_BYTES 3328
struct W13Extra {
  uint32_t sg[2];  // the SG words of the item's two quads
  u32x2 meta;      // {hb, patch} of the item's (tile, wave)
};

// the wave's nq (0..2) quads starting at `first`, six 16-byte and two 4-byte requests, all through one descriptor
template <int AUX = 2>
__device__ __forceinline__ void load_quads_w13(bf16x8 (&wr)[6], uint32_t (&sg)[2], const char *first, int nq, int l,
                                               int half = -1) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(first), 0, (nq < 0 ? 0 : nq) * W13_QUAD_BYTES, 0x00020000);
  const bool mine = half < 0 || ((l >> 3) & 1) == half;
  const int voff = mine ? l * 16 : 0x40000000, voff4 = mine ? l * 4 : 0x40000000;
  // Order of issue: a wave's loads return in order, and k-step f needs its SG word, its NB word and one L word.  The two
  // small SG requests go first and NB in front of L0 / L1, so that the first decode waits for four requests, not eight.
#pragma unroll
  for (int q = 0; q < 2; ++q) sg[q] = __builtin_amdgcn_raw_buffer_load_b32(r, voff4 + 3072, q * W13_QUAD_BYTES, AUX);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
#pragma unroll
    for (int p = 2; p < 5; ++p)  // NB, L0, L1
      wr[3 * q + p % 3] =
          __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, voff + (p % 3) * 1024, q * W13_QUAD_BYTES, AUX));
  }
}

// ONE quad (nq = 0 or 1) at `first` through a descriptor of its own, for the kernels whose item is one quad per tile
// (k_moe_gate_up at K = 2048: a gate and an up quad): the 4-byte SG request, then NB, L0, L1 as above — a tile's first
// decode waits for three requests, and nothing of a second quad is ever asked for.  wr: {L0, L1, NB}.
template <int AUX = 2>
__device__ __forceinline__ void load_quads_w13(bf16x8 (&wr)[3], uint32_t &sg, const char *first, int nq, int l) {
  const __amdgpu_buffer_rsrc_t r =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(first), 0, (nq < 0 ? 0 : nq) * W13_QUAD_BYTES, 0x00020000);
  sg = __builtin_amdgcn_raw_buffer_load_b32(r, l * 4 + 3072, 0, AUX);
#pragma unroll
  for (int p = 2; p < 5; ++p)  // NB, L0, L1
    wr[p % 3] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(r, l * 16 + (p % 3) * 1024, 0, AUX));
}

// {hb, patch} of (tile t, wave w): wave-uniform address, constant address space -> one scalar load, no VMEM operation
__device__ __forceinline__ u32x2 w13_meta(const u32x2 *meta, int t, int w) {
  typedef const __attribute__((address_space(4))) u32x2 *cptr;
  return *(cptr)(uintptr_t)(meta + (size_t)__builtin_amdgcn_readfirstlane(t) * 16 + w);
}

// four H bytes from four codes (one per byte) and the SG word: (c ? hb + c : 0) | sign << 7
__device__ __forceinline__ uint32_t w13_high(uint32_t c, uint32_t sgw, int r, u16x2 hb2) {
  const uint32_t nz = ((c + 0x0f0f0f0fu) >> 4) & 0x01010101u;  // 1 in every byte whose code is not 0
  const u16x2 e = __builtin_bit_cast(u16x2, nz) * hb2 + __builtin_bit_cast(u16x2, c);  // bytes stay below 128: no carry
  return __builtin_bit_cast(uint32_t, e) | ((sgw << (7 - r)) & 0x80808080u);
}

// the fragment of k-step f (0..7) of the wave's share, decoded right in front of its MFMA: k-step f & 3 of the quad whose
// L0 or L1 word (the one that holds it) is lq, whose NB word is nq and whose SG word is sgw; meta = the item's {hb, patch}
__device__ __forceinline__ bf16x8 w13_frag(bf16x8 lq, bf16x8 nq, uint32_t sgw, u32x2 meta, int f, int l) {
  const int ff = f & 3;
  const u32x4 lw = __builtin_bit_cast(u32x4, lq);
  const uint32_t la = (ff & 1) ? lw[2] : lw[0], lb = (ff & 1) ? lw[3] : lw[1];
  const uint32_t n = __builtin_bit_cast(u32x4, nq)[ff];
  const uint32_t hb = __builtin_amdgcn_readfirstlane(meta[0]) & 0x7f, pw = __builtin_amdgcn_readfirstlane(meta[1]);
  const u16x2 hb2 = {(unsigned short)hb, (unsigned short)hb};
  const uint32_t ha = w13_high(n & 0x0f0f0f0fu, sgw, 2 * ff, hb2);
  const uint32_t hh = w13_high((n >> 4) & 0x0f0f0f0fu, sgw, 2 * ff + 1, hb2);
  u32x4 o;
  o[0] = __builtin_amdgcn_perm(ha, la, 0x05010400u);  // L0 H0 L1 H1
  o[1] = __builtin_amdgcn_perm(ha, la, 0x07030602u);  // L2 H2 L3 H3
  o[2] = __builtin_amdgcn_perm(hh, lb, 0x05010400u);
  o[3] = __builtin_amdgcn_perm(hh, lb, 0x07030602u);
  if ((pw >> 28) == (8u | (uint32_t)f)) {  // wave-uniform: the item's one exception sits in this k-step
    const int pl = (pw >> 22) & 63, el = (pw >> 19) & 7;
    const uint32_t raw = pw & 0xffffu;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const uint32_t nd = (el & 1) ? (o[d] & 0xffffu) | (raw << 16) : (o[d] & 0xffff0000u) | raw;
      o[d] = (l == pl && (el >> 1) == d) ? nd : o[d];
    }
  }
  return __builtin_bit_cast(bf16x8, o);
}
// ... of a two-quad item (f = 0..7)
__device__ __forceinline__ bf16x8 w13_frag(const bf16x8 (&wr)[6], const W13Extra &ex, int f, int l) {
  const int q = f >> 2;
  return w13_frag(wr[3 * q + ((f & 3) >> 1)], wr[3 * q + 2], ex.sg[q], ex.meta, f, l);
}
// ... of a one-quad item (f = 0..3)
__device__ __forceinline__ bf16x8 w13_frag(const bf16x8 (&wr)[3], uint32_t sgw, u32x2 meta, int f, int l) {
  return w13_frag(wr[f >> 1], wr[2], sgw, meta, f, l);
}

// The 16 fp32 scales of packed tile t (wscale + 16 t, 64-byte aligned) by ONE scalar load: the address is wave-uniform
// and the pointer is read through the constant address space, so no VMEM operation is issued — the ragged-batch ring
// kernel counts its vector loads by vmcnt immediates, and the register-resident one would wait for its weight items in
// flight behind a vector load.  lane_scales picks the four of the lane's columns 4 fg .. 4 fg + 3 (MFMA D layout).
typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x16 tile_scales(const float *wscale, int t) {
  typedef const __attribute__((address_space(4))) f32x16 *cptr;
  return *(cptr)(uintptr_t)(wscale + (size_t)__builtin_amdgcn_readfirstlane(t) * 16);
}
__device__ __forceinline__ f32x4 lane_scales(const f32x16 &s, int fg) {
  f32x4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = fg == 0 ? s[r] : fg == 1 ? s[4 + r] : fg == 2 ? s[8 + r] : s[12 + r];
  return o;
}

// sum over the 16 lanes of a DPP row, result in each of them
__device__ __forceinline__ float row_sum16(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  return v;
}

// B-operand fragments of k-steps ks[0..NF) for lane l (m = l&15, kq = l>>4):
// x[m][ks*32 + kq*8 .. +8], in two steps so that the caller can put its weight loads BETWEEN
// them: a wave's vector loads return in issue order (vmcnt), so activation loads issued after
// a weight burst are held back until the burst has landed — and the rstd / normalise chain
// behind them with it (scripts/dbg_gemm_stamps.py: the prologue then ran AFTER the first
// burst with HBM idle, 4-5 us per launch).  issue_x: the loads (raw rows or fragments, norm
// weights); finish_x: mask / normalise.  `take[f]` false -> zero fragment (k-step past the
// wave's share or past K; ks[f] is then any valid step).  The source mode is switched
// OUTSIDE the fragment loops so that the loads of one call are issued together; branching
// per fragment serialised them with a vmcnt(0) each (+6.5 us per launch, measured).
template <int NF, bool NORM = true>
__device__ __forceinline__ void issue_x(const RowSrc &s, const int (&ks)[NF], int l, int nv, bf16x8 (&raw)[NF],
                                        bf16x8 (&wv)[NF]) {
  // one branch-free load sequence for all modes (a mode branch around the loads made hipcc keep
  // the fragment arrays in scratch memory): per-lane base + k-step stride, both by select
  // All 16 rows are loaded, valid or not (the caller's buffer covers 16 rows, dflash_hip.h):
  // no address depends on `nv`, so nothing here waits for the scalar load of the lengths.
  (void)nv;
  const int m = l & 15, kq = l >> 4;
  const bool fr = s.mode == 0;
  const char *base = fr ? reinterpret_cast<const char *>(s.frag) + l * 16
                        : reinterpret_cast<const char *>(s.rows) + ((int64_t)m * s.ld + kq * 8) * 2;
  const int kstep = fr ? 1024 : 64;  // bytes per k-step: a 64-lane fragment / 32 bf16 of a row
  // norm weights: only mode 2 has them; the others read (and ignore) 16 B of their own operand
  const char *nwb = s.mode == 2 ? reinterpret_cast<const char *>(s.nw) + kq * 16 : base;
  const int nstep = s.mode == 2 ? 64 : kstep;
#pragma unroll
  for (int f = 0; f < NF; ++f) raw[f] = *reinterpret_cast<const bf16x8 *>(base + (int64_t)ks[f] * kstep);
  if (NORM) {  // compile-time: kernels that never see mode 2 skip these loads
#pragma unroll
    for (int f = 0; f < NF; ++f) wv[f] = *reinterpret_cast<const bf16x8 *>(nwb + (int64_t)ks[f] * nstep);
  }
}

template <int NF, bool NORM = true>
__device__ __forceinline__ void finish_x(const RowSrc &s, const bool (&take)[NF], int l, int nv, float rstd,
                                         const bf16x8 (&raw)[NF], const bf16x8 (&wv)[NF], bf16x8 (&x)[NF]) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (s.mode == 0) {
#pragma unroll
    for (int f = 0; f < NF; ++f) x[f] = take[f] ? raw[f] : z;
    return;
  }
  const int m = l & 15;
  const bool norm = NORM && s.mode == 2;  // Qwen3RMSNorm: weight * bf16(x * rstd), tf:modeling_qwen3.py:59-64
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const bf16x8 r = raw[f];  // whole-vector copies: element access through the array
    bf16x8 o = r;             // reference kept the arrays in scratch memory
    if (norm) {
      const bf16x8 wq = wv[f];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(wq[j]) * rbf(bf2f(r[j]) * rstd));
    }
    x[f] = (take[f] && m < nv) ? o : z;
  }
}

// finish_x with the RMSNorm weight read from LDS (nwl[c] = elements 8c .. 8c+7, staged once per workgroup by the
// caller, K <= 4096): no second 32-VGPR fragment array is alive while the activation loads are in flight.
template <int NF>
__device__ __forceinline__ void finish_xl(const RowSrc &s, const int (&ks)[NF], const bool (&take)[NF], int l, int nv,
                                          float rstd, const bf16x8 (&raw)[NF], const bf16x8 *nwl, bf16x8 (&x)[NF]) {
  const bf16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  if (s.mode == 0) {
#pragma unroll
    for (int f = 0; f < NF; ++f) x[f] = take[f] ? raw[f] : z;
    return;
  }
  const int m = l & 15, kq = l >> 4;
  const bool norm = s.mode == 2;  // Qwen3RMSNorm: weight * bf16(x * rstd), tf:modeling_qwen3.py:59-64
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const bf16x8 r = raw[f];
    bf16x8 o = r;
    if (norm) {
      const bf16x8 wq = nwl[(ks[f] * 4 + kq) & 511];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(wq[j]) * rbf(bf2f(r[j]) * rstd));
    }
    x[f] = (take[f] && m < nv) ? o : z;
  }
}

template <int NF, bool NORM = true>
__device__ __forceinline__ void build_x(const RowSrc &s, const int (&ks)[NF], const bool (&take)[NF], int l, int nv,
                                        float rstd, bf16x8 (&x)[NF]) {
  bf16x8 raw[NF], wv[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) wv[f] = raw[f] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
  issue_x<NF, NORM>(s, ks, l, nv, raw, wv);
  finish_x<NF, NORM>(s, take, l, nv, rstd, raw, wv, x);
}

// ---- host side ----
inline int pick_ksplit_min(int KS, int fr_max) { return (KS + 16 * fr_max - 1) / (16 * fr_max); }

// Workgroups along x for `ngroups` tile groups when the K axis is cut `ksplit` ways: at
// most 256 workgroups in all (one 16-wave workgroup per CU), every workgroup walking the
// same number of groups so that no CU streams twice as long as its neighbour.
inline int grid_x_for(int ngroups, int ksplit = 1) {
  int gx_max = 256 / ksplit;
  if (gx_max < 1) gx_max = 1;
  const int per_wg = (ngroups + gx_max - 1) / gx_max;
  return (ngroups + per_wg - 1) / per_wg;
}

inline bool fill_src(RowSrc &d, const dfl_rows *s, int K, const char *who) {
  if (!s) {
    dfl_set_error("%s: null row source", who);
    return false;
  }
  d.frag = (const bf16x8 *)s->frag;
  d.rows = (const bf16_t *)s->rows;
  d.ld = s->ld;
  d.ss = s->ss;
  d.nss = s->nss;
  d.nw = (const bf16_t *)s->norm_w;
  d.eps = s->eps;
  d.valid_word = s->valid_word;
  d.mode = s->mode;

  const bool ok = (s->mode == 0 && s->frag) || (s->mode == 1 && s->rows && s->ld >= K && s->ld % 8 == 0) ||
                  (s->mode == 2 && s->rows && s->ss && s->nss >= 1 && s->norm_w && s->ld >= K && s->ld % 8 == 0);
  if (!ok) dfl_set_error("%s: bad row source (mode %d)", who, s->mode);
  if (ok && s->mode == 2 && K > 4096) {  // the norm weight is staged in 8 KB of LDS; the in-kernel rstd covers one K pass
    dfl_set_error("%s: a normalised row source needs K <= 4096 (K=%d)", who, K);
    return false;
  }
  // one partial per 16-column tile of K <= 4096: the prologue's 16 waves x 4 lane groups x 4 loads read 256 slots
  if (ok && s->mode == 2 && s->nss > 256) {
    dfl_set_error("%s: a normalised row source takes at most 256 partial sums of squares (nss=%d)", who, s->nss);
    return false;
  }
  return ok;
}


}  // namespace
