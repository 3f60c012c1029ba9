/*
 * dflash_hip.h — C ABI of libdflash_hip.so: the MI355X (gfx950) kernels behind the
 * DFlash block-diffusion speculative-decoding hot path.
 *
 * Drop-in boundary: the reference has no FFI — its hot path is
 * Python calling torch/transformers ops.  Each entry point below replaces the
 * torch op sequence at the cited reference lines (paths relative to the reference
 * repo; `tf:` = transformers 5.15.0).  The Python mirror of the reference's
 * operator API (dflash_amd.DFlashDraftModel.forward / spec_generate, dflash_generate,
 * dflash_generate_policy) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer into caller-owned memory (torch storage)
 *    unless named host_*; the library allocates nothing, reads no environment
 *    variable and keeps no state except the thread-local last-error string and,
 *    per ring-GEMM kernel instantiation, the result of the one call that raises
 *    its dynamic-LDS limit (made at its first launch, never changed after);
 *  - `stream` is a hipStream_t passed as void* (NULL = default stream); calls only
 *    enqueue work, never synchronise, and are capturable into a hipGraph;
 *  - return 0 on success, a negative DFL_E* code on a rejected argument or a
 *    failed launch; dfl_last_error() gives the text;
 *  - bf16 storage everywhere, fp32 accumulation; ids are int64 (torch.long).
 *
 * Device layouts (MI355X-first)
 *  - "packed weight": a row-major [N][K] bf16 nn.Linear weight re-laid as
 *    [N/16][K/32][64 lanes][8] so that one wave-wide 16-B load is one MFMA
 *    16x16x32 A-operand fragment and a column tile streams as one contiguous run;
 *  - "frag16 activations": up to 16 rows x K bf16 stored as [K/8][16][8], i.e. the
 *    matching MFMA B-operand fragments, written directly by the producing kernel;
 *  - "dyn": int32[8] per request on the device: {S, tau, bs, pos0, ...} — draft
 *    cache length before this cycle, context rows, block rows, absolute position
 *    of the first context row.  Kernels read lengths from it so that one captured
 *    graph serves every cycle.
 *
 * One entry point per operation: dfl_gemm_argmax, dfl_sample_rows_nucleus, dfl_attn_head_cand, dfl_attn_head_batch,
 * dfl_accept_commit, dfl_gemm_sample_batch, dfl_kv_append_batch and dfl_accept_commit_batch each took over the arguments
 * of their former `_t` / `_timed` / `_rearm` twins (optional ones are nullable or have a neutral value, said at each),
 * and the ten launches that have an e4m3 form take the matrix as a dfl_weight in place of a former `_fp8` twin.
 */
#ifndef DFLASH_HIP_H
#define DFLASH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFL_ABI_VERSION 1

#define DFL_OK 0
#define DFL_EINVAL (-22)   /* bad shape / alignment / null pointer */
#define DFL_ELAUNCH (-5)   /* hipLaunch failed (text in dfl_last_error) */

#define DFL_DYN_WORDS 8
#define DFL_DYN_S 0        /* rows already in the draft KV cache               */
#define DFL_DYN_TAU 1      /* context rows appended this cycle (prev acc+1)     */
#define DFL_DYN_BS 2       /* block (noise) rows this cycle                     */
#define DFL_DYN_POS0 3     /* absolute position id of the first context row     */
#define DFL_DYN_START 4    /* `start` of the decode loop (= pos0 + tau)         */
#define DFL_DYN_STOP 5     /* 1 once a stop token was committed                 */
#define DFL_DYN_CYCLE 6    /* cycles run                                        */

/* Where one 16-row activation tile of a GEMM comes from.
 *  mode 0  frag   : frag16 fragments [K/8][16][8] written by a producer kernel;
 *  mode 1  rows   : plain bf16 rows [16][K] with row stride ld (e.g. the target taps); all 16
 *                   rows must be READABLE memory (they are loaded before the valid count is known
 *                   and masked afterwards), whatever dyn[valid_word] says;
 *  mode 2  normed : rows = the residual stream h (a buffer of 16 readable rows), and the GEMM applies the RMSNorm while
 *                   it builds its fragments: x = norm_w * bf16(h * rsqrt(sum_i ss[i][m] / K
 *                   + eps)) (Qwen3RMSNorm, tf:models/qwen3/modeling_qwen3.py:59-64), where
 *                   ss[nss][16] are partial sums of squares of each row left by the
 *                   producer (dfl_embed_rows: nss = 1; dfl_gemm_resid: nss = N/16), 1 <= nss <= 256;
 *                   K <= 4096.
 * Rows >= dyn[valid_word] (valid_word >= 0) are treated as zero. */
typedef struct dfl_rows {
  const void *frag;
  const void *rows;
  int64_t ld;
  const float *ss;
  int32_t nss;
  const void *norm_w;
  float eps;
  int32_t valid_word;
  int32_t mode;
} dfl_rows;

/* What the matrix of a launch is (dfl_rows says where the activations come from).  An entry point takes one exactly when
 * it has an e4m3 form; the others take the packed bf16 weight as `const void *wp`.
 * ---- FP8 (OCP e4m3fn) weight streaming, weight-only (W8A16) ----
 * The weight is stored as one e4m3 code per element plus one fp32 scale per output row; the kernels convert the codes
 * to bf16 in registers (exact), run the same bf16 MFMA on the same bf16 activations, and multiply the fp32 K-sum by
 * the row's scale before the epilogue's first rounding: Linear output = bf16(sum_k x[m][k] * q[n][k] * scale[n]).
 * Packed layout [N/16][K/64][64 lanes][16 B]: lane l (column 16 t + (l & 15), kq = l >> 4) holds the 8 codes of
 * k = 64 j + 8 kq .. in bytes 0-7 and those of k = 64 j + 32 + 8 kq .. in bytes 8-15.  K % 64 == 0.
 * scale: fp32 [N] in PACKED tile order: scale[16 t + nl] belongs to column nl of packed tile t — row order for
 * dfl_pack_weight_fp8, (gate tile p, up tile p) interleaved for dfl_pack_weight_gateup_fp8.  Any fp32 multiplier is
 * taken; a code of 0x7f / 0xff is NaN.  Everything else of a launch is the same contract in both formats, argument for
 * argument; what the e4m3 form narrows is said at each entry point.
 * DFL_EINVAL: a null descriptor, a format other than the two, DFL_W_BF16 with a scale, DFL_W_E4M3 without one.
 * ---- DFL_W_BF16X13: the packed bf16 weight in 13 bits per element, losslessly ----
 * Taken by dfl_gemm_silu_mul and dfl_gemm_argmax at K = 2048 or K = 4096, by dfl_moe_gate_up at K = 2048 and by
 * dfl_gemm_resid at K a multiple of 2048 ABOVE 4096 (the K-chunked form below) ONLY; every other entry point, and
 * dfl_gemm_resid at any other K, refuses it as an unknown format. Same results as DFL_W_BF16 on the same matrix, bit for bit: the kernels rebuild the bf16 fragments in
 * registers from 13/16 of the bytes.  A bf16 is L = bits[7:0] and H = bits[15:8].  Per packed 16-column tile the base is
 * hb = max(0, max(H & 0x7f) - 15); an element keeps L, its sign and a 4-bit code c: c = 0 <=> (H & 0x7f) == 0 (+-0,
 * denormals, exponent 1: L is kept), c = 1..15 <=> (H & 0x7f) == hb + c.  All-zero bits decode to +0.
 * wp points at ONE buffer (scale must be NULL): the quads of all packed tiles, then the meta pairs.
 *   quad = four k-steps of one tile, 3328 bytes: L0 [64 lanes][16 B] (L of k-step 0, elements 0..7, then of k-step 1),
 *     L1 (k-steps 2, 3), NB [64][16 B] (dword f = codes of k-step f: byte b = c[b] | c[b + 4] << 4), SG [64][4 B] (bit
 *     8 b + r = sign of element 4 (r & 1) + b of k-step r >> 1); lane l = column l & 15, k group l >> 4 as in the packed
 *     bf16 layout.  Tile t holds K / 128 quads at byte (t * K / 128) * 3328; tiles in dfl_pack_weight[_gateup] order.
 *   meta = uint32 [N / 16][16 waves][2] at byte (N / 16) * (K / 128) * 3328: {hb, patch}.  Wave w of the kernel owns k-steps
 *     w * K / 512 .. of a tile.  patch: bit 31 valid, 30:28 k-step within the wave's share, 27:22 lane, 21:19 element,
 *     15:0 the bf16 itself: the ONE nonzero element of that (tile, wave) item below the window (stored with c = 0).  A
 *     matrix with two such elements in one item has no BF16X13 form and stays DFL_W_BF16.
 *   K > 4096 (K % 2048 == 0; dfl_gemm_resid): the quads as above; the kernel walks K in nch = K / 2048 chunks and in
 *     chunk c wave w owns k-steps (16 c + w) * 4 .. + 3 — quad 16 c + w of the tile — so an ITEM is (tile, chunk, wave),
 *     one quad.  meta = uint32 [N / 16][nch][16][2]: the pair of (t, c, w) at index (t * nch + c) * 16 + w (nch = 1 gives
 *     the formula above), the base repeated per (chunk, wave), the patch word's k-step field 0..3.
 * The packer is dflash_amd.ops.pack_weight_bf16x13 (tensor ops over the packed bf16 weight, once at load).
 * ---- DFL_W_MXFP4: OCP Microscaling MXFP4, weight-only (W4A16) ----
 * Taken by dfl_gemm_resid (any K % 128 == 0, the K-chunked form included), dfl_gemm_silu_mul and dfl_gemm_argmax ONLY;
 * every other entry point refuses it as an unknown format.  An element is an e2m1 code (bit 3 sign, bits 2:0 the magnitudes
 * 0, .5, 1, 1.5, 2, 3, 4, 6) and every 32 consecutive k of a row share one e8m0 scale code s: the weight is e2m1 * 2^(s - 127).
 * The kernels convert code pairs to bf16 with the block scale applied in the conversion (exact), run the same bf16 MFMA
 * on the same bf16 activations and have no epilogue multiply: Linear output = bf16(sum_k x[m][k] * w[n][k]), every rounding
 * point where the bf16 form has it.  One MFMA k-step of one column is 32 consecutive k: a k-step fragment is one MX block.
 * wp points at ONE buffer of N * K / 2 + N * K / 32 bytes (scale must be NULL): the codes, then the scales.
 *   codes  [N/16][K/128][64 lanes][16 B]: lane l is column 16 t + (l & 15), kq = l >> 4; dword d (0..3) of the lane's 16-byte
 *     word holds k-step 4 j + d: its 8 codes are those of k = 128 j + 32 d + 8 kq .. + 7, two per byte in k order, the LOW
 *     nibble first.
 *   scales e8m0 bytes [N/16][K/128][16 columns][4 B] at byte offset N * K / 2: one dword per (column, 128-k group), byte d
 *     the scale of k-step 4 j + d (k = 128 j + 32 d ..).  The kernel forms the fp32 multiplier as code << 23.
 *   Tiles t in dfl_pack_weight order, or (dfl_gemm_silu_mul, N = 2 I) in dfl_pack_weight_gateup order — gate tile p, up tile
 *     p interleaved — codes and scales alike.
 * Scale codes 7..247 (exponents -120..120); anything else is undefined, as other unvalidated device data.
 * K % 128 == 0; a wave's share is a whole number of 4-k-step words (the launcher rounds it up, as the e4m3 form rounds to
 * even).  DFL_EINVAL, by the entry point's name: K % 128 != 0, a non-NULL scale.
 * Quantiser and packers: dflash_amd.ops.quantize_mxfp4_rows / pack_weight_mxfp4 / pack_weight_gateup_mxfp4 (tensor ops). */
enum { DFL_W_BF16 = 0, DFL_W_E4M3 = 1, DFL_W_BF16X13 = 2, DFL_W_MXFP4 = 3 };
typedef struct dfl_weight {
  const void *wp;      /* packed weight: dfl_pack_weight[_gateup] (bf16) or dfl_pack_weight[_gateup]_fp8 (codes) */
  const float *scale;  /* DFL_W_E4M3: fp32 scale per packed row, in packed tile order; DFL_W_BF16: must be NULL */
  int32_t format;
} dfl_weight;

int dfl_version(void);
const char *dfl_last_error(void);

/* ---- one-time layout conversion (weight load; not on the per-cycle path) ---- */

/* nn.Linear weight [N][K] bf16 row-major -> packed weight.  N%16==0, K%32==0. */
int dfl_pack_weight(const void *w, void *wp, int N, int K, void *stream);
/* gate_proj and up_proj [I][K] each -> one packed weight of 2I rows with tiles
 * interleaved (gate tile t, up tile t) so SiLU(gate)*up fuses into the GEMM
 * epilogue (tf:models/qwen3/modeling_qwen3.py:81-83). */
int dfl_pack_weight_gateup(const void *gate, const void *up, void *wp, int I, int K, void *stream);
/* The same two for e4m3 codes (dfl_weight): q [N][K] uint8 row-major -> wp8 (N * K bytes); gate_q / up_q [I][K] -> one
 * packed weight of 2I rows, tiles interleaved as dfl_pack_weight_gateup.  N%16==0 / I%16==0, K%64==0. */
int dfl_pack_weight_fp8(const void *q, void *wp8, int N, int K, void *stream);
int dfl_pack_weight_gateup_fp8(const void *gate_q, const void *up_q, void *wp8, int I, int K, void *stream);

/* ---- per-cycle kernels ---- */

/* dyn <- {S, tau, bs, pos0, start=pos0+tau, stop=0, cycle=0, 0}: all DFL_DYN_WORDS words, the spare one cleared. */
int dfl_set_dyn(int32_t *dyn, int S, int tau, int bs, int pos0, void *stream);
/* Blocks of 17..32 rows (results.md:11-16 sweeps 20 and 24; benchmark_dynamic_schedule.py:44-51 takes any
 * candidate >= 2) run as TWO 16-row tiles: every GEMM / embed launch is issued once per tile on rows 16 t ..
 * with the tile's own record.  dyn holds 2 x DFL_DYN_WORDS ints; record t gets
 * {S, clamp(tau - 16 t, 0, 16), clamp(bs - 16 t, 0, 16), pos0, start = pos0 + tau (unclamped), 0, 0, 0}. */
int dfl_set_dyn2(int32_t *dyn, int S, int tau, int bs, int pos0, void *stream);

/* rows x K bf16 (row stride ldx elements) -> frag16; rows beyond n_valid zeroed.
 * n_valid = dyn[dyn_word] if dyn != NULL else rows.  Used for the target taps
 * (model/utils.py:16-25 output) feeding fc. */
int dfl_pack_rows(const void *x, int64_t ldx, int rows, int K, void *xf, const int32_t *dyn, int dyn_word,
                  void *stream);

/* Skinny GEMM, weights streamed once: out[c][mt*16+m][n] = sum_{k in chunk c} x_mt[m][k] * W[n][k]
 * (fp32 partials, summed and rounded to bf16 by the consumer exactly where the
 * reference's nn.Linear output is rounded).  Replaces F.linear at model/dflash.py:70,
 * 73-76 (q/k/v of context and block rows).  mt in {1,2} row tiles (x1 ignored for
 * mt==1), N%16==0, K%32==0, out has ksplit*mt*16*N floats;
 * ksplit >= ceil(K/32 / (16*8/mt)). */
int dfl_gemm_f32(const void *wp, const dfl_rows *x0, const dfl_rows *x1, int mt, int N, int K, int ksplit, float *out,
                 const int32_t *dyn, void *stream);

/* act = bf16(silu(bf16(x Wg^T))) * bf16(x Wu^T) written as frag16 [I/8][16][8]
 * (tf:...modeling_qwen3.py:82 inner expression).  w_gateup from dfl_pack_weight_gateup[_fp8].
 * K/32 <= 128 (no K split: the activation needs the finished sums).  e4m3: gate and up sums are scaled separately,
 * each before its bf16 rounding.  DFL_W_BF16X13 (of the dfl_pack_weight_gateup layout, N = 2 I): K = 2048 or 4096, scale
 * NULL; anything else is refused by name.  Same bits as DFL_W_BF16.  DFL_W_MXFP4 (gate/up tile order, N = 2 I): K % 128
 * == 0, scale NULL; gate and up blocks carry their own scales. */
int dfl_gemm_silu_mul(const dfl_weight *w_gateup, const dfl_rows *x, int I, int K, void *act_frag, const int32_t *dyn,
                      void *stream);

/* lm_head GEMM fused with the greedy unmask: ids[r] = argmax_n bf16(x[r] . W[n])
 * for r in [row0, row0+nrows), first index on ties (model/dflash.py:238-247 +
 * model/utils.py:28-29).  The 15 x V logits are never materialised unless
 * `logits` != NULL (bf16 [16][V], rows outside the range untouched).
 * ws: workspace of dfl_argmax_ws_bytes() bytes.  out_ids int64, written at
 * out_ids[r - row0 + out_off]. nrows_dyn_word >= 0: rows = dyn[word] - row0.
 * margin_out (optional, fp32, same indexing as out_ids): top-1 minus top-2 bf16 logit of the
 * row, the reference's confidence statistic (benchmark_candidate_solutions.py:296-302,
 * torch.topk(2) values: an exact tie gives 0) — the per-position confidence comes with the
 * unmask at no extra pass over the logits.
 * ev_start / ev_end (each optional): hipEvent_t recorded on `stream` right before and right after the GEMM launch (the
 * argmax finish launch comes behind ev_end): bench.py times the lm_head kernel itself with them (roofline.achieved).
 * e4m3: ids, logits and margins over bf16(sum * scale).  DFL_W_BF16X13: K = 2048 or 4096, scale NULL; same bits as
 * DFL_W_BF16 (dfl_gemm_sample does not take it).  DFL_W_MXFP4: K % 128 == 0, scale NULL; ids, logits and margins over
 * bf16(sum) of the dequantised weights (dfl_gemm_sample refuses it). */
int64_t dfl_argmax_ws_bytes(void);
int dfl_gemm_argmax(const dfl_weight *w, const dfl_rows *x, int V, int K, int row0, int nrows, const int32_t *dyn,
                    int nrows_dyn_word, void *ws, int64_t *out_ids, int out_off, void *logits, float *margin_out,
                    void *ev_start, void *ev_end, void *stream);

/* Seeded sampling at temperature T fused into the same lm_head GEMM (Gumbel-max):
 *   ids[r] = argmax_n fmaf(bf16(x[r] . W[n]), inv_t, g(seed, rng_stream, p_r, n, extra)), first index on ties,
 * inv_t = float32(1 / T), g the Gumbel noise of dfl_rng.h (Philox4x32-10, key = seed, counter = (n >> 2, p, extra,
 * stream)).  Tile row m draws position p = base + pos_add + m with base = pos_dyn[pos_word] (a device length record, so
 * a captured graph draws fresh positions on every replay) or, pos_dyn NULL, base = pos_base.  rng_stream 0 (TARGET):
 * extra = 0; 1 (DRAFT): extra = base.  Everything else as dfl_gemm_argmax; margin_out is the perturbed top-2 gap.
 * e4m3: the draw perturbs bf16(sum * scale[n]), the logit dfl_gemm_argmax materialises for the same weight. */
int dfl_gemm_sample(const dfl_weight *w, const dfl_rows *x, int V, int K, int row0, int nrows, const int32_t *dyn,
                    int nrows_dyn_word, void *ws, int64_t *out_ids, int out_off, void *logits, float *margin_out,
                    uint64_t seed, float inv_t, int rng_stream, const int32_t *pos_dyn, int pos_word, int pos_base,
                    int pos_add, void *stream);

/* GEMM with the residual epilogue (o_proj / down_proj / fc, model/dflash.py:101,140,144,177):
 *   v = bf16(x W^T);  h_io[m][n] <- add_residual ? bf16(h_io[m][n] + v) : v;
 *   tap[m][n] <- the same value (optional: a tapped target layer, model/utils.py:16-25);
 *   ss_out[n/16][m] <- sum over the tile's 16 columns of h_new^2 (optional; feeds the
 *   mode-2 row source of the next GEMM, so the RMSNorm is no launch of its own).
 * Any K: beyond 4096 the workgroup walks K in chunks itself (x must then be mode 0/1).
 * DFL_W_BF16X13: K > 4096 and K % 2048 == 0 only (the K-chunked form), scale NULL; same bits as DFL_W_BF16.
 * DFL_W_MXFP4: any K % 128 == 0 (both forms, half tiles included), scale NULL. */
int dfl_gemm_resid(const dfl_weight *w, const dfl_rows *x, int N, int K, void *h_io, int64_t ldh, int add_residual,
                   void *tap, int64_t ldtap, float *ss_out, const int32_t *dyn, void *stream);

/* h_out[m] = embed[ids[m]] for m < dyn[dyn_word] (model/dflash.py:237) and ss_out[m] =
 * sum of squares of that row (one partial per row: nss = 1 for the next GEMM). */
int dfl_embed_rows(const void *embed, const int64_t *ids, void *h_out, int H, float *ss_out, const int32_t *dyn,
                   int dyn_word, void *stream);

/* Row-wise residual/norm stage that also converts to frag16:
 *   v   = part ? bf16(sum_c part[c][row_off+m][:]) : (none)
 *   h   = embed ? embed[ids[m]] : resid_in ? resid_in[m] : 0       (bf16)
 *   h   = part ? (resid_in||embed ? bf16(h + v) : v) : h            (model/dflash.py:140,144)
 *   h_out[m] = h                                   (if h_out; h_out2[m*ld2 ..] gets the same row:
 *                                                   a tapped target layer, model/utils.py:16-25)
 *   frag[m]  = norm_w * bf16(h * rsqrt(mean(h^2)+eps))  (Qwen3RMSNorm, tf:...:59-64)
 * rows m >= n_valid (dyn[dyn_word], or 16) get zero fragments.  H%8==0, H<=16384.
 * part row stride ldp floats, split stride part_split floats. */
int dfl_norm_pack(const float *part, int nsplit, int64_t part_split, int ldp, int row_off, const void *resid_in,
                  const void *embed, const int64_t *ids, void *h_out, void *h_out2, int64_t ld2, const void *norm_w,
                  float eps, void *frag, int H, const int32_t *dyn, int dyn_word, void *stream);

/* q_norm/k_norm + RoPE + KV append (model/dflash.py:71-85 with the local
 * apply_rotary_pos_emb of :22-28).  qkv: fp32 partials from dfl_gemm_f32,
 * element (split c, buffer row r, column j) at qkv[c*split_stride + r*ld + j];
 * q/k/v column blocks start at q_col/k_col/v_col (q_col < 0: no q wanted);
 * context rows sit at buffer rows ctx_row0.., block rows at blk_row0.. (< 0: none).
 * Writes
 *   q_out  bf16 [n_q][16][128]       (block rows only: q uses the last bs positions)
 *   kcache/vcache bf16 [n_kv][cache_rows][128] at rows S + rel, rel = row_base + i
 *   for context row i, tau + j for block row j; RoPE position = pos0 + rel.
 * cos/sin: bf16 [max_pos][64] tables (tf:...:125-137, computed by the host in fp32
 * then cast, as the reference does).  head_dim must be 128.  q_norm_w == k_norm_w ==
 * NULL skips the per-head norms (Llama-style attention).
 * ctx_rows_override >= 0: that many context rows instead of dyn tau and no block
 * rows — the draft-cache prefill of the prompt's context in 16-row groups, with
 * row_base = index of the group's first row (the record's tau and bs are then ignored).
 * Edges: a position >= max_pos rotates with table row max_pos - 1 (clamped, no read past the
 * tables); a K/V row whose cache row S + rel is >= cache_rows is silently not stored (q_out
 * is still written; dfl_kv_append_batch runs the same kernel).  The position clamp holds at
 * every norm + RoPE site below that takes max_pos (dfl_attn_fused, dfl_attn_head and its
 * forms, the _batch forms). */
int dfl_qknorm_rope_append(const float *qkv, int nsplit, int64_t split_stride, int ld, int q_col, int k_col,
                           int v_col, int ctx_row0, int blk_row0, int n_q, int n_kv, const void *q_norm_w,
                           const void *k_norm_w, float eps, const void *cos_tab, const void *sin_tab, int max_pos,
                           void *q_out, void *kcache, void *vcache, int cache_rows, const int32_t *dyn,
                           int ctx_rows_override, int row_base, void *stream);

/* GQA attention of the block's 16 query rows over the cached prefix + this cycle's
 * rows: softmax(q k^T * scale) v over kv_len = S + tau + bs keys.  causal = 0: no mask
 * (the draft, is_causal=False, model/dflash.py:86-99).  causal = 1: query row j sees
 * cache rows <= S + tau + j (the target's verify forward over the same block).  MFMA QK^T / PV, K/V tiles
 * staged in LDS, split over the key axis with a log-sum-exp merge.
 * ws: dfl_attn_ws_bytes(n_q, max_splits) bytes.  out: frag16 [n_q*128/8][16][8].
 * GQA group n_q / n_kv: 1..8 (one wave per query head of the group); anything else is DFL_EINVAL, nothing launched. */
int64_t dfl_attn_ws_bytes(int n_q, int max_splits);
int dfl_block_attn(const void *q, const void *kcache, const void *vcache, int cache_rows, int n_q, int n_kv,
                   float scale, int causal, const int32_t *dyn, int kv_len_max, void *ws, int max_splits,
                   void *out_frag, void *stream);

/* The whole attention stage of a block in ONE launch: q/k-norm + RoPE + KV append
 * (model/dflash.py:71-85) + attention (:86-99, causal = 0; target verify, causal = 1)
 * + the merge of the key splits, result as frag16 for o_proj.  Same arithmetic as
 * dfl_qknorm_rope_append + dfl_block_attn (V rows bit-identical, K up to rare 1-ulp flips); the key axis is
 * split over workgroups and merged by the last one to arrive.  tau + bs <= 32 new rows.
 * ws: dfl_attn_fused_ws_bytes(n_q, n_kv, max_splits) bytes, ZEROED once by the caller
 * (it holds the arrival tickets, which every launch leaves at zero again).
 * GQA group n_q / n_kv: 1, 2, 4 or 8 (dfl_attn_fused_batch likewise); anything else is DFL_EINVAL, nothing launched.
 * dfl_attn_head and its forms and dfl_prefill_attn take any n_q % n_kv == 0. */
int64_t dfl_attn_fused_ws_bytes(int n_q, int n_kv, int max_splits);
int dfl_attn_fused(const float *qkv, int nsplit, int64_t split_stride, int ld, int q_col, int k_col, int v_col,
                   int ctx_row0, int blk_row0, int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w,
                   float eps, const void *cos_tab, const void *sin_tab, int max_pos, void *kcache, void *vcache,
                   int cache_rows, float scale, int causal, const int32_t *dyn, int kv_len_max, void *ws,
                   int max_splits, void *out_frag, void *stream);

/* The attention stage, second form: same arithmetic as dfl_attn_fused (model/dflash.py:71-99; causal = 1: the
 * target verify's stage, :249-255), but q/k/v arrive as FINISHED bf16 Linear outputs — dfl_gemm_resid(add_residual
 * = 0) of the block rows into xq [bs][ldq] (q | k | v column blocks at q_col / k_col / v_col) and, for the draft,
 * of the context rows into xc [tau][ldc] (k, v at ck_col / cv_col; xc may be NULL when tau == 0) — and the grid is
 * (kv head, query heads of the group x key splits): one query head per workgroup (two, sharing every K/V tile, from
 * ~5k cached keys), 8 waves over disjoint 32-key
 * tiles with no barrier in the loop, wave results merged in LDS, one 8 KB partial per workgroup published
 * write-through and merged by the head's last arriver (csrc/attn_head.hip).  New rows (tau + bs <= 64, tau <= 32)
 * are appended to the cache at rows S.. by the launch itself.  bs <= 16 * q_tiles, q_tiles in {1, 2}: the second
 * query tile's frag16 output lies out_tile_stride bf16 elements after the first.
 * Lengths: dyn == NULL -> the immediates S, tau, bs, pos0; else they are read from dyn and S is the caller's
 * upper bound on dyn[S] (it sizes the key splits, as kv_len_max does for dfl_attn_fused).
 * ws: dfl_attn_head_ws_bytes(n_q, max_splits, q_tiles) bytes, ZEROED once (arrival tickets, left zero).  Only the tickets
 * need the zeros: the split partials in front of them may hold anything.  The figure, like dfl_attn_fused_ws_bytes and
 * dfl_attn_fused_batch_ws_bytes, ends in 64 bytes of slack behind the last ticket: an upper bound, not a tight size. */
int64_t dfl_attn_head_ws_bytes(int n_q, int max_splits, int q_tiles);
int dfl_attn_head(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, const void *xc, int64_t ldc,
                  int ck_col, int cv_col, int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w, float eps,
                  const void *cos_tab, const void *sin_tab, int max_pos, void *kcache, void *vcache, int cache_rows,
                  float scale, int causal, const int32_t *dyn, int S, int tau, int bs, int pos0, int q_tiles,
                  void *ws, int max_splits, void *out_frag, int64_t out_tile_stride, void *stream);

/* dfl_attn_head (q_tiles = 1) AND the o_proj + residual GEMM that follows it (model/dflash.py:101,140; for the
 * target tf:modeling_qwen3.py o_proj) in ONE launch: besides the attention workgroups the grid carries one workgroup
 * per 16-column tile of o_proj, which pulls its weight slice into registers while the attention runs (the stage
 * leaves HBM idle), waits for the heads' outputs (bounded: 2 ms), and finishes the GEMM with dfl_gemm_resid's
 * epilogue: h_io [16][ldh] <- bf16(h_io + bf16(attn . Wo^T)), ss_out [H/16][16] partial sums of squares.
 * Range: q_dim = n_q * 128 <= 4096, bs <= 16, tau + bs <= 32, H % 16 == 0.  attn_frag: frag16 of the attention output
 * (16 * q_dim bf16; rows >= bs are written as zeros).  sync: DFL_ATTN_OPROJ_SYNC_WORDS int32, ZEROED once; sync[1025] != 0 after a launch means an
 * o_proj workgroup gave up waiting and h_io is invalid (the Python layer raises; it cannot happen on an idle GPU). */
#define DFL_ATTN_OPROJ_SYNC_WORDS 1056
int dfl_attn_head_oproj(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, const void *xc, int64_t ldc,
                        int ck_col, int cv_col, int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w, float eps,
                        const void *cos_tab, const void *sin_tab, int max_pos, void *kcache, void *vcache,
                        int cache_rows, float scale, int causal, const int32_t *dyn, int S, int tau, int bs, int pos0,
                        void *ws, int max_splits, void *attn_frag, const void *wo_packed, int H, void *h_io,
                        int64_t ldh, float *ss_out, int32_t *sync, void *stream);

/* ---- multi-candidate verify (benchmark_candidate_solutions.py) ----
 * Several drafts of ONE block are verified against ONE cached prefix and the best is kept (:570-618).
 *
 * dfl_attn_head_cand: dfl_attn_head (causal, no context rows) for n_cand candidate blocks in one launch
 * (grid.z = candidate): candidate c's block rows at xq + c * xq_cand_stride elements, its frag16 output at out_frag +
 * c * out_cand_stride elements; every candidate attends the same cached rows [0, S) plus ITS OWN bs new rows, which go
 * not to the cache but to the staging area k_out / v_out [c][n_kv][out_rows][128] (rows 0..bs-1) — the reference clones
 * and batch-repeats the whole DynamicCache instead (:76-81, :572-575) and selects the winner's copy (:604-608); here the
 * caller copies the winner's bs rows into the cache.  q_tiles = 2 (candidate blocks of 17..32 rows): candidate c = two
 * consecutive 16-row tiles of xq and of out_frag, out_tile_stride elements apart (q_tiles = 1: pass 0).
 * ws: n_cand * dfl_attn_head_ws_bytes(n_q, max_splits, q_tiles) bytes, zeroed. */
int dfl_attn_head_cand(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, int n_cand, int64_t xq_cand_stride,
                       int n_q, int n_kv, const void *q_norm_w, const void *k_norm_w, float eps, const void *cos_tab,
                       const void *sin_tab, int max_pos, const void *kcache, const void *vcache, int cache_rows,
                       float scale, int S, int bs, void *ws, int max_splits, void *out_frag, int64_t out_cand_stride,
                       int64_t out_tile_stride, int q_tiles, void *k_out, void *v_out, int64_t kv_out_cand_stride,
                       int out_rows, void *stream);

/* dfl_attn_head for the R requests of a ragged batch in one launch (grid.z = request; replaces dfl_attn_fused_batch):
 * request r's block rows at xq + r * xq_req_stride, its lengths at dyn + r * DFL_DYN_WORDS (block form: the context rows
 * are cached already, dyn tau == 0), its cache at + r * cache_req_stride, its frag16 output at + r * out_req_stride.
 * kv_len_max bounds S + 16 * q_tiles over the requests (it sizes the key splits).  q_tiles = 2 (blocks of 17..32 rows;
 * benchmark.py's block-size sweep, results.md:11-16, with several requests per GPU): request r is TWO consecutive 16-row
 * tiles of xq and of out_frag (out_tile_stride elements apart; q_tiles = 1: pass 0), one cache and one length record whose
 * bs counts both tiles.  ws: R * dfl_attn_head_ws_bytes(n_q, max_splits, q_tiles) bytes, zeroed once. */
int dfl_attn_head_batch(const void *xq, int64_t ldq, int q_col, int k_col, int v_col, int R, int64_t xq_req_stride, int n_q,
                        int n_kv, const void *q_norm_w, const void *k_norm_w, float eps, const void *cos_tab,
                        const void *sin_tab, int max_pos, void *kcache, void *vcache, int cache_rows,
                        int64_t cache_req_stride, float scale, int causal, const int32_t *dyn, int kv_len_max, void *ws,
                        int max_splits, void *out_frag, int64_t out_req_stride, int64_t out_tile_stride, int q_tiles,
                        void *stream);
/* dfl_attn_head_batch on the fp32 K-PART SUMS of the q/k/v projection (dfl_gemm_f32_batch's output) instead of finished
 * bf16 rows (model/dflash.py:70-76: a q/k/v value is the Linear's bf16 output = bf16(part 0 + part 1)): request r's rows of
 * part k at xq_parts + k * part_stride + r * xq_req_stride floats, row stride ldq floats; nparts = dfl_batch_ksplit(hidden)
 * must be 1 or 2.  The K parts of the projection meet in this launch's row loads, so the GEMM in front of it needs no slab /
 * ticket / combine phase (qkv at 4 request tiles: 18.3 -> 14.7 us).  Blocks of <= 16 rows. */
int dfl_attn_head_batch_f32(const float *xq_parts, int nparts, int64_t part_stride, int64_t ldq, int q_col, int k_col,
                            int v_col, int R, int64_t xq_req_stride, int n_q, int n_kv, const void *q_norm_w,
                            const void *k_norm_w, float eps, const void *cos_tab, const void *sin_tab, int max_pos,
                            void *kcache, void *vcache, int cache_rows, int64_t cache_req_stride, float scale, int causal,
                            const int32_t *dyn, int kv_len_max, void *ws, int max_splits, void *out_frag,
                            int64_t out_req_stride, void *stream);

/* Per row of bf16 logits [rows][ld] (rows <= 64): the k <= 8 largest values with their indices, ordered (value
 * descending, index ascending) — out_val fp32 [rows][8], out_idx int32 [rows][8] — and the row's log-sum-exp (fp32).
 * What the candidate builders take from the 15 x V draft logits: torch.topk at :216, :296, the top-2 probability
 * margin softmax(x)[top1] - softmax(x)[top2] = exp(v1 - lse) - exp(v2 - lse) at :98-101, :305-307, and
 * log_softmax(x)[token] = x[token] - lse at :119-131.  torch.topk's order among EQUAL values is an implementation
 * detail; this one is fixed (and equals torch.argmax's for k = 1). */
int dfl_topk_rows(const void *logits, int64_t ld, int rows, int V, int k, float *out_val, int32_t *out_idx, float *out_lse,
                  void *stream);

/* Acceptance length of every candidate block against its posterior, the choice of :592-601 — maximise tau, then the
 * draft score, then prefer the lower candidate index, evaluated as the reference does: argmax over the fp32 value
 * tau * 1e6 + draft_score - idx * 1e-3 — and the winner's commit (:612-613) with the stop test and length bookkeeping
 * of dfl_accept_commit.  blocks / posterior int64 [n_cand][stride], scores fp32 [n_cand], n_cand <= 8.
 * result int32 [12]: {acc, new_start, stop, winner, acc of candidate 0..7 (-1 beyond n_cand)}. */
int dfl_candidate_select(const int64_t *blocks, int64_t blk_stride, const int64_t *posterior, int64_t post_stride,
                         const float *scores, int n_cand, int bs, int64_t *output_ids, int64_t output_len, int32_t *dyn,
                         const int64_t *stop_ids, int n_stop, int32_t *result, void *stream);

/* ---- sparse-MoE MLP of a target's verify forward (BASELINE configs[4]; tf:models/qwen3_moe/modeling_qwen3_moe.py) ----
 * The reference calls the HF target (model/dflash.py:249-255); for an MoE target these three replace its
 * Qwen3MoeSparseMoeBlock on the <= 16 block rows:
 *  dfl_moe_route: router logits bf16 [16][ld] (the gate Linear's output: dfl_gemm_resid, no residual) -> softmax in fp32 ->
 *    top_k (<= 8; ties: lower expert first) -> divided by their sum (norm_topk) -> bf16 -> wt bf16 [16][E] (0 = not routed);
 *    active int32 [E]; list = the active experts in ascending order, *n_active their number.  Rows >= dyn[dyn_word] route
 *    nowhere.  E <= 256.
 *  dfl_gemm_silu_mul_experts: dfl_gemm_silu_mul for every ACTIVE expert (list[0 .. *n_active)) in one launch: the
 *    workgroups share out the (expert, gate/up column pair) items; expert e's packed gate/up weight at wp + e *
 *    wp_expert_stride elements, its frag16 output at act_frag + e * act_expert_stride — back to back: the strides must
 *    be exactly 2*I*K and 16*I.
 *  dfl_moe_down: out[c][m][n] = sum over the c-th share of the active experts of wt[m][e] * (act_e[m] . Wd_e[n]) as fp32
 *    (nsplit shares; dfl_norm_pack adds them to the residual stream and rounds once, where the reference rounds every
 *    expert's output and accumulates in bf16: fewer roundings, inside the bf16 tolerance). */
int dfl_moe_route(const void *logits, int ld, int E, int top_k, int norm_topk, void *wt, int32_t *active, int32_t *list,
                  int32_t *n_active, const int32_t *dyn, int dyn_word, void *stream);
/* The block's post-attention RMSNorm (Qwen3MoeRMSNorm), the gate Linear and dfl_moe_route in ONE launch (round 4; they are
 * latency, not bytes: 15 % of a 48-layer verify as three launches).  h != NULL: rows [16][ldh] bf16 are normalised with
 * norm_w / eps and written to xn_frag (frag16 [K/8][16][8], the expert GEMMs' source; rows >= dyn[dyn_word]: zeros);
 * h == NULL: xn_frag already holds the normalised rows.  wp_router: the gate weight [E padded to 16][K] packed
 * (dfl_pack_weight); rlog bf16 [16][ld] receives the logits (ld >= padded E, ld % 8 == 0); wt / active / list / n_active
 * as dfl_moe_route writes them (same arithmetic).  ticket: one int32, zero before the first launch, left zero by every
 * launch.  K <= 4096, E even. */
int dfl_moe_router(const void *h, int64_t ldh, const void *norm_w, float eps, void *xn_frag, const void *wp_router, int K,
                   int E, int top_k, int norm_topk, void *rlog, int ld, void *wt, int32_t *active, int32_t *list,
                   int32_t *n_active, const int32_t *dyn, int dyn_word, int32_t *ticket, void *stream);
int dfl_gemm_silu_mul_experts(const void *wp_gateup, int64_t wp_expert_stride, const dfl_rows *x, int E, int I, int K,
                              void *act_frag, int64_t act_expert_stride, const int32_t *list, const int32_t *n_active,
                              const int32_t *dyn, void *stream);
/* dfl_gemm_silu_mul_experts for K <= 2048 and frag16 rows (x_frag: [K/32][64] fragments): an item is the (gate, up)
 * tile PAIR of an active expert, the 16 waves of a workgroup meet once per pair (at K = 2048 a tile is 64 KB and the
 * per-tile meeting of the general kernel weighs twice what it does at K = 4096).  Same results, same layouts; rows
 * >= dyn[valid_word] count as zero (valid_word < 0 or dyn NULL: all 16).
 * e4m3 (both launches; one fp32 scale per output row, read only): the same items, the same k-steps per wave in the same
 * order, the fp32 sums multiplied by the row's scale in front of the first rounding point — with power-of-two scales
 * bit-equal to the bf16 launch on q * scale.  The scales must be 64-byte aligned.
 *  dfl_moe_gate_up: the experts' codes back to back, each 2*I*K bytes in dfl_pack_weight_gateup_fp8's layout; scale fp32
 *    [E][2*I] in that layout's tile order (gate tile p's 16 scales, then up tile p's).  K % 64 == 0.
 *  dfl_moe_down: expert e's codes (dfl_pack_weight_fp8 of its [N][I] weight) at wp + e * wp_expert_stride BYTES (>= N*I,
 *    % 16 == 0); scale fp32 [E][N].  I % 64 == 0.
 * DFL_W_BF16X13 (dfl_moe_gate_up only; dfl_moe_down refuses it: its K = I is not the layout's): K = 2048, scale NULL.  wp
 * is the 13-bit form of the experts' packed gate/up weights taken as ONE matrix of N = E * 2*I rows (dflash_amd.ops.
 * pack_weight_bf16x13 of the [E][2*I*K] tensor as it stands): the quads of all E * 2*I / 16 tiles, expert after expert
 * in dfl_pack_weight_gateup order, then the {base, patch} pairs of all tiles.  Wave w's four k-steps of a tile are quad
 * w of that tile, so an item streams one quad of the gate tile and one of the up tile and rebuilds the bf16 form's
 * fragments in registers: the same bits as the DFL_W_BF16 launch on the same weights, from 13/16 of the bytes. */
int dfl_moe_gate_up(const dfl_weight *w_gateup, const void *x_frag, int E, int I, int K, void *act_frag, const int32_t *list,
                    const int32_t *n_active, const int32_t *dyn, int valid_word, void *stream);
int dfl_moe_down(const dfl_weight *w_down, int64_t wp_expert_stride, const void *act_frag, int64_t act_expert_stride,
                 const void *wt, const int32_t *list, const int32_t *n_active, int E, int N, int I, int nsplit, float *out,
                 void *stream);

/* First-max-index argmax over the last axis (model/utils.py:28-29).
 * dtype: 0 = bf16, 1 = fp32.  ids int64 [rows]. */
int dfl_argmax(const void *logits, int dtype, int rows, int64_t V, int64_t *ids, void *stream);

/* The draw of dfl_gemm_sample over materialised bf16 logits [rows][ld] (the first V columns): row r draws position
 * pos[r] (pos int32, may be NULL: pos0 + r) with the given `extra` counter word.  Same value compared as the fused
 * epilogue, so the same ids.  out_ids int64 [rows]; margin_out (optional) fp32 [rows]: perturbed top-1 minus top-2. */
int dfl_sample_rows(const void *logits, int64_t ld, int rows, int V, uint64_t seed, float inv_t, int rng_stream, int pos0,
                    const int32_t *pos, int extra, int64_t *out_ids, float *margin_out, void *stream);

/* The seeded draw restricted by top-k and top-p ("Filtered draw") over materialised bf16 logits laid
 * out as tiles [tiles][16][V] (row stride ld, tile stride tile_stride, in elements; V <= 155648).  Per row:
 *   t_k = the top_k-th largest value (the row minimum if top_k == 0 or >= V);
 *   t_p = the largest t with sum_{x >= t, x >= t_k} w >= top_p * sum_{x >= t_k} w, w = exp(inv_t (x - max));  top_p >= 1: t_k;
 *   id  = argmax over {v : x_v >= max(t_k, t_p)} of fmaf(x_v, inv_t, noise of dfl_rng.h), lowest v on ties.
 * Ties at a threshold are kept whole; with both filters off the ids are those of dfl_sample_rows.
 * Rows: tile t takes rows row0 .. row0 + n, n = dyn[t][nrows_dyn_word] - row0 if nrows_dyn_word >= 0, else nrows (the
 * convention of dfl_gemm_sample_batch); other rows are not written.  Tile t is tile j = t % tiles_per_req of request slot
 * q = t / tiles_per_req.  Row m of it draws position
 *   positions[16 t + m]                                         if positions != NULL (int32), else
 *   (pos_word >= 0 ? dyn[t][pos_word] : pos_base) + pos_add + 16 j + m.
 * The DRAFT stream with a record position takes that record word as its `extra` counter word; otherwise `extra`.
 * seeds / top_k_dev / top_p_dev: device arrays (int64 / int32 / fp32) indexed by q, or NULL for the host value beside
 * them; a device top_k < 0 or top_p outside (0, 1) reads as "off".  Everything a replayed launch needs is read by
 * address.  out_ids[t * out_stride + out_off + (m - row0)]; thr_out (fp32: the final threshold) and kept_out (int32: the
 * size of the kept set) are optional and indexed like out_ids.
 * invT: inv_t_dev is a device fp32 array indexed by q (NULL: the host inv_t, as with top_k_dev / top_k; a non-NULL array
 * makes the host value unused and unchecked).  The slot's invT feeds both the masses exp(invT (x - max)) and the draw.  A
 * slot whose value is not > 0 (0, negative, NaN) is GREEDY: its rows return at once and write nothing — out_ids, thr_out
 * and kept_out keep what they held, the way rows past a tile's valid count do.  In the filtering verify the
 * dfl_gemm_argmax_batch launch in front has already written that slot's argmax ids (lowest index on ties) where this
 * launch would write.  Device values are not validated: every bit pattern is defined. */
int dfl_sample_rows_nucleus(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int row0, int nrows,
                            const int32_t *dyn, int nrows_dyn_word, int pos_word, int pos_base, const int32_t *positions,
                            int pos_add, int tiles_per_req, const int64_t *seeds, uint64_t seed, const int32_t *top_k_dev,
                            int top_k, const float *top_p_dev, float top_p, const float *inv_t_dev, float inv_t,
                            int rng_stream, int extra, int64_t *out_ids, int64_t out_stride, int out_off, float *thr_out,
                            int32_t *kept_out, void *stream);

/* Log-probabilities of the tokens a verify commits, and optionally of the top alternatives at each position (DESIGN.md
 * section 12), over materialised bf16 logits laid out as tiles [tiles][16][V] — layout, rows and tiles exactly as
 * dfl_sample_rows_nucleus takes them (ld, tile_stride in elements, V <= 155648; row0 / nrows or dyn[t][nrows_dyn_word];
 * tile t = tile j = t % tiles_per_req of request slot q = t / tiles_per_req; rows past a tile's valid count write nothing).
 * The numbers are of the RAW distribution: log_softmax of the logits as the head produced them, at T = 1 and unfiltered,
 * whatever temperature, top-k or top-p chose the token.  Per row, in fp32:
 *   lse = max + log(sum exp(x - max)), max over the FINITE values; -inf, +inf and NaN entries contribute 0 (a row without
 *         a finite value has lse = -inf).  The sum has one fixed order (per thread in column order, the wave's butterfly,
 *         the 16 wave sums in wave order): the same logits give the same bits on every run.
 *   lp  = x[id] - lse, id = ids[t * ids_stride + ids_off + (m - row0)] (int64: the out_ids indexing of the sampling
 *         launches).  An id outside [0, V) writes NaN and reads nothing out of the row.
 *   top : the n_top (0..8) columns first in the order (value descending, column ascending), as column ids (int64) and
 *         x - lse.  -0 and +0 are one value; a NaN sorts above +inf (sign clear) or below -inf (sign set), so every bit
 *         pattern has a place.  V < n_top: the entries past V are id -1 and NaN.  n_top = 0: the outputs may be NULL.
 * Outputs are scattered by POSITION: row m of tile t writes at
 *   pos = (pos_word >= 0 ? dyn[t][pos_word] : pos_base) + pos_add + 16 j + m     (the position rule of the filtered draw)
 * into lp_out[q * lp_stride + pos] and top_ids_out / top_lp_out[(q * lp_stride + pos) * n_top + i]; pos < 0 or
 * pos >= lp_len writes nothing.  Verify row j of a cycle starting at `start` predicts position start + j + 1, and the
 * token committed there is always posterior[j]; a later cycle rewrites every position past its own start, so each
 * committed position keeps the value of the cycle that committed it.  Launch it behind the last launch that writes the
 * posterior and BEFORE the accept launch, which advances the records the positions are read from. */
int dfl_logprob_rows(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int row0, int nrows,
                     const int32_t *dyn, int nrows_dyn_word, int pos_word, int pos_base, int pos_add, int tiles_per_req,
                     const int64_t *ids, int64_t ids_stride, int ids_off, int n_top, float *lp_out, int64_t *top_ids_out,
                     float *top_lp_out, int64_t lp_stride, int lp_len, void *stream);

/* Repetition / presence / frequency penalties.  The state is one table row per request slot,
 * int32 [slots][table_stride >= V]: bit 31 = the token occurs in the PROMPT, bits 0..30 = its occurrences in the OUTPUT.
 * V is a multiple of 8, at most 155648; table rows start on 16 bytes (table_stride a multiple of 4).
 *
 * dfl_penalty_count adds a range of ids to the rows of slots 0 .. slots-1, one workgroup per slot: slot s takes
 * ids[s * ids_stride + i] (int64) for i in [lo', hi'), clamped into [0, ids_len), where
 *   dyn == NULL: lo' = lo, hi' = hi;
 *   dyn != NULL: lo' = dyn[s][lo_word] + lo, hi' = dyn[s][hi_word] + hi, and a slot whose DFL_DYN_BS word is 0 is IDLE:
 *                it is skipped whole (not cleared either), the rule of dfl_accept_commit_batch — a parked slot is not
 *                counted twice.  Behind an accept launch, lo_word = DFL_DYN_S, hi_word = DFL_DYN_START, lo = hi = 1 is
 *                exactly what that launch committed: output_ids(S, START].
 * as_prompt != 0: bit 31 is set (integer atomic or); else the count goes up by 1 per occurrence (integer atomic add).
 * clear != 0: the slot's row is zeroed first, inside the same launch, before its adds.  Ids outside [0, V) are not
 * counted and never indexed.  Integer adds only: the result does not depend on the order they land in. */
int dfl_penalty_count(int32_t *table, int64_t table_stride, int V, int slots, const int64_t *ids, int64_t ids_stride,
                      int ids_len, const int32_t *dyn, int lo_word, int hi_word, int lo, int hi, int as_prompt, int clear,
                      void *stream);

/* Penalised logits of a verify's rows: reads materialised bf16 logits laid out as tiles [tiles][16][V] — rows, tiles, dyn /
 * nrows_dyn_word / tiles_per_req exactly as dfl_sample_rows_nucleus takes them (ld and tile_stride in elements, multiples
 * of 8, rows on 16 bytes) — and writes `out`, same layout; out may be the logits themselves.  Rows past a tile's valid
 * count return at once and write nothing.  Row m of tile t (tile j = t % tiles_per_req of slot q = t / tiles_per_req) is
 * penalised by table row q plus the block's own tokens block_ids[q * block_stride + 1 .. 16 j + m] (int64; NULL: none):
 *   seen(v) = the table word of v is not 0, or v is among those tokens
 *   c(v)    = bits 0..30 of the table word + the occurrences of v among those tokens
 * and, x being the bf16 logit widened to fp32, in fp32 IEEE operations each rounded once:
 *   y1 = seen ? (x > 0 ? x / r : x * r) : x        (a true, correctly rounded division; -0 takes x * r)
 *   y2 = y1 - (c > 0 ? a : 0)
 *   y3 = fmaf(-f, float(c), y2)
 *   z  = y3 rounded to bf16, nearest even
 * +-inf go through the same operations; a NaN keeps its bits.  With r = 1, a = 0, f = 0 every z is x bit for bit.  Block
 * ids outside [0, V) are ignored.  r / a / f: device fp32 arrays indexed by q, or NULL for the host value beside them
 * (the way top_k_dev / top_k work).  Host values are validated (r finite and > 0, a and f finite); device values are
 * not: a device r that is not > 0 or not finite reads as 1, a non-finite a or f reads as 0, so every bit pattern is defined.
 * out_ids (optional, int64): out_ids[t * out_stride + out_off + (m - row0)] = the penalised row's argmax, the lowest
 * column among those equal to the maximum over the values that are not NaN (-0 == +0); 0 for a row of NaNs.  On rows
 * without NaN these are the ids of dfl_argmax; greedy rows need no further launch, a sampled row's id is overwritten
 * by the draw behind it.  No floating-point atomics: the same inputs give the same bits, eager or replayed. */
int dfl_penalty_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V, int row0, int nrows,
                     const int32_t *dyn, int nrows_dyn_word, int tiles_per_req, const int32_t *table, int64_t table_stride,
                     const int64_t *block_ids, int64_t block_stride, const float *r_dev, float r, const float *a_dev,
                     float a, const float *f_dev, float f, int64_t *out_ids, int64_t out_stride, int out_off,
                     void *stream);

/* Logit bias, token allow / ban lists and min_tokens.  The state is one dense table row per
 * request slot, fp32 [slots][bias_stride >= V] (rows on 16 bytes, bias_stride a multiple of 4), and one int32 min_pos per
 * slot.  logits / out / ld / tile_stride / tiles / V / row0 / nrows / dyn / nrows_dyn_word / tiles_per_req / out_ids /
 * out_stride / out_off exactly as dfl_penalty_rows takes them; out may be the logits themselves; rows past a tile's valid
 * count return at once and write nothing.  Row m of tile t (tile j = t % tiles_per_req of slot q = t / tiles_per_req)
 * predicts position
 *   p = (pos_word >= 0 ? dyn[t][pos_word] : pos_base) + pos_add + 16 j + m        (the rule of dfl_logprob_rows)
 * and, x being the bf16 logit widened to fp32 and b = bias[q * bias_stride + v]:
 *   z = (b == 0)    ? x           the bits of x copied: -0 stays -0, a NaN keeps its bits
 *     : (b == -inf) ? -inf        whatever x is
 *     :               x + b in fp32, rounded to bf16 nearest even (a NaN x keeps its bits)
 *   if p < min_pos[q]:  z[s] = -inf for every s among stop_ids[0 .. n_stop) that lies in [0, V)
 * min_pos: min_pos_dev[q] (device int32 by slot), or the host value when min_pos_dev is NULL; 0 is off.  A stop id outside
 * [0, V) is ignored and never indexed; n_stop <= 64.  Table values are not validated: a NaN or +inf reads as 0, so every
 * bit pattern is defined.  out_ids (optional): the processed row's argmax by the rule of dfl_penalty_rows; a fully
 * banned row gives 0.  No floating-point atomics: the same inputs give the same bits, eager or replayed. */
int dfl_logit_bias_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V, int row0,
                        int nrows, const int32_t *dyn, int nrows_dyn_word, int tiles_per_req, const float *bias,
                        int64_t bias_stride, const int32_t *min_pos_dev, int min_pos, const int64_t *stop_ids, int n_stop,
                        int pos_word, int pos_base, int pos_add, int64_t *out_ids, int64_t out_stride, int out_off,
                        void *stream);

/* min_p: a probability floor relative to the top token.  logits / out / ld / tile_stride / tiles /
 * V / row0 / nrows / dyn / nrows_dyn_word / tiles_per_req exactly as dfl_penalty_rows takes them; out may be the logits
 * themselves; rows past a tile's valid count return at once and write nothing.  Row m of tile t belongs to slot
 * q = t / tiles_per_req.  L = log_min_p_dev[q] and invT = inv_t_dev[q] (device fp32 by slot), or the host values beside
 * them when the array is NULL; L = float32(ln(min_p)) from the host, -inf for min_p = 0.  x being the row's bf16 logits
 * widened to fp32, in fp32 IEEE operations each rounded once, never contracted:
 *   m   = max over the entries of x that are not NaN                  (-0 == +0)
 *   d_v = (x_v - m) * invT
 *   z_v = (x_v == m or d_v >= L) ? x_v : -inf                         (the bits of x copied; a NaN x_v keeps its bits too)
 * which is exp(invT (x_v - m)) >= min_p, p_v >= min_p * p_max on the tempered distribution.  The maximum is always kept:
 * the row's argmax (lowest column on ties) does not move.  A row is copied whole, bit for bit, when its slot is off
 * (L is -inf, > 0 or NaN), when its slot is greedy (invT not > 0) or when m is not finite (+inf, or no entry that is not
 * NaN or -inf).  Host values are validated (log_min_p <= 0, -inf allowed; inv_t in (0, 1e5]); device values are not: every
 * bit pattern is defined above.  kept_out (optional, int32): kept_out[t * kept_stride + kept_off + (m - row0)] = the
 * number of columns with x_v == m or d_v >= L (a NaN is not counted); a row that is copied whole reports V.  No atomics:
 * the same inputs give the same bits, eager or replayed. */
int dfl_min_p_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V, int row0, int nrows,
                   const int32_t *dyn, int nrows_dyn_word, int tiles_per_req, const float *log_min_p_dev, float log_min_p,
                   const float *inv_t_dev, float inv_t, int32_t *kept_out, int64_t kept_stride, int kept_off,
                   void *stream);

/* Grammar-constrained decoding: a token automaton.  The state is a POOL, int16
 * [pool_states][table_stride >= V] (rows on 16 bytes, table_stride a multiple of 8), holding several grammars at different
 * base rows: table[(base + s) * table_stride + v] >= 0 is the state, relative to base, after token v in state s; < 0: v is
 * illegal in s.  Per slot two int32 values: base[slot], the grammar's first pool row (< 0: the slot has no grammar), and
 * state[slot], relative to base (-1: violated, sticky).  Every row offset (base + s) * table_stride is formed in 64 bits.
 * A state or successor with base + s >= pool_states reads as violated and is never indexed.
 *
 * dfl_grammar_rows: logits / out / ld / tile_stride / tiles / V / row0 / nrows / dyn / nrows_dyn_word / tiles_per_req /
 * block_ids / block_stride / out_ids / out_stride / out_off exactly as dfl_penalty_rows takes them; out may be the logits
 * themselves; rows past a tile's valid count return at once and write nothing.  Row m of tile t (tile j = t %
 * tiles_per_req of slot q = t / tiles_per_req) starts from s = state[q] and walks the block's own tokens
 * block_ids[q * block_stride + 1 .. 16 j + m] (int64; NULL: no walk — the single-row form for a first token):
 *   s <- table[(base[q] + s) * table_stride + id], and the row is DEAD once base[q] < 0, s < 0, or an id is outside [0, V)
 *   live: z[v] = table[(base[q] + s) * table_stride + v] < 0 ? -inf : x[v]      (the bits of x copied; a NaN keeps its bits)
 *   dead: z = x
 * A dead row is never committed by the accept rule: row m is compared, or used as the bonus, only when block[1 .. m] were
 * all accepted, each of them picked from a live row.  out_ids (optional): the row's argmax by the rule of
 * dfl_penalty_rows; a row that is all -inf gives 0.  No floating-point atomics: the same inputs give the same bits, eager
 * or replayed. */
int dfl_grammar_rows(const void *logits, void *out, int64_t ld, int64_t tile_stride, int tiles, int V, int row0, int nrows,
                     const int32_t *dyn, int nrows_dyn_word, int tiles_per_req, const int16_t *table, int64_t table_stride,
                     int pool_states, const int32_t *base, const int32_t *state, const int64_t *block_ids,
                     int64_t block_stride, int64_t *out_ids, int64_t out_stride, int out_off, void *stream);

/* dfl_grammar_advance walks what was committed: one wave per slot 0 .. slots-1, one lane stepping state[s] over
 * ids[s * ids_stride + i] (int64) for i in [lo', hi') — ids / ids_stride / ids_len / dyn / lo_word / hi_word / lo / hi
 * exactly as dfl_penalty_count takes them (behind an accept launch: DFL_DYN_S, DFL_DYN_START, 1, 1 is output_ids(S,
 * START]).  An illegal step or an id outside [0, V) stores -1.  A slot whose DFL_DYN_BS word is 0, whose base is < 0, whose
 * state is < 0 or whose range is empty is left alone.  Plain vector stores. */
int dfl_grammar_advance(const int16_t *table, int64_t table_stride, int pool_states, int V, const int32_t *base,
                        int32_t *state, int slots, const int64_t *ids, int64_t ids_stride, int ids_len, const int32_t *dyn,
                        int lo_word, int hi_word, int lo, int hi, void *stream);

/* dfl_grammar_draft_rows: the draft's block tokens picked under the automaton ("The draft under
 * the grammar").  logits / ld / tile_stride / tiles / V / dyn / nrows_dyn_word and the pool as dfl_grammar_rows takes
 * them, ONE tile per slot (tile t is slot t); nrows (0..16) is the block size n, or dyn[t][nrows_dyn_word] when
 * nrows_dyn_word >= 0.  Row m of the bf16 logits predicts block slot m; block_ids[t * block_stride + 1 .. n-1] (int64)
 * hold the head launch's plain argmax on entry.  One 1024-thread workgroup per slot walks the rows in order:
 *   s = state[t]                         (base[t] < 0 or table == NULL: no grammar, every column grammar-legal)
 *   for m = 1 .. n-1:
 *     legal(v) = (no grammar or table[(base[t] + s) * table_stride + v] >= 0) and (bias == NULL or bias[t][v] != -inf)
 *     grammar and s < 0 (or base + s >= pool_states): stop
 *     c = the lowest legal column among those whose logit is maximal over the legal, non-NaN columns; none: stop
 *     block_ids[t * block_stride + m] = c
 *     grammar: s = table[(base[t] + s) * table_stride + c], a successor outside the pool: stop
 * "stop" leaves the ids from there on as they were.  -0 == +0; a legal -inf wins only when every legal column is -inf or
 * NaN.  bias (fp32 [tiles][bias_stride >= V], rows on 16 bytes; NULL: the grammar-only form): the logit-bias table, of
 * which only the bans (-inf) are read.  table == NULL (with bias): the ban-only form, rows independent of each other.  A
 * slot with neither a grammar nor a bias table, an idle slot (n < 2) and row 0 are left untouched.  state is only read.
 * Every pool offset is formed in 64 bits.  No atomics, plain vector stores: the same inputs give the same bits, eager or
 * replayed. */
int dfl_grammar_draft_rows(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int nrows,
                           const int32_t *dyn, int nrows_dyn_word, const int16_t *table, int64_t table_stride,
                           int pool_states, const int32_t *base, const int32_t *state, const float *bias,
                           int64_t bias_stride, int64_t *block_ids, int64_t block_stride, void *stream);

/* dfl_grammar_draft_sample_rows: the noise form of dfl_grammar_draft_rows ("The coupled draft under
 * a grammar").  Every argument up to block_stride, the walk, the stops and what is left untouched are the sibling's; the
 * quantity compared over the legal columns of row m of slot t is
 *   key(v) = fmaf(bf16 logit[v], invT_t, g(seeds[t], DFL_RNG_TARGET, p = base_t + m, v, extra = 0))      (dfl_rng.h)
 * — the noise the target's verify row m - 1 draws position base_t + m with — and c is the lowest legal column among
 * those whose key is maximal over the legal columns with a non-NaN key.  base_t = dyn[t][pos_dyn_word] when
 * pos_dyn_word >= 0 (the draft record's DFL_DYN_START), else pos_base.  seeds: int64 [tiles].  invT_t = inv_ts[t] (fp32
 * [tiles]) when inv_ts is given, else inv_t; a slot whose invT is not > 0 (0, negative, NaN) compares the logits
 * themselves: the sibling's pick, bit for bit.  Philox is called once per four columns, only where one of them is legal. */
int dfl_grammar_draft_sample_rows(const void *logits, int64_t ld, int64_t tile_stride, int tiles, int V, int nrows,
                                  const int32_t *dyn, int nrows_dyn_word, const int16_t *table, int64_t table_stride,
                                  int pool_states, const int32_t *base, const int32_t *state, const float *bias,
                                  int64_t bias_stride, int64_t *block_ids, int64_t block_stride, const int64_t *seeds,
                                  float inv_t, const float *inv_ts, int pos_dyn_word, int pos_base, void *stream);

/* dfl_grammar_lift: a byte automaton lifted to the pool's token rows on the device.  dfa: int16
 * [Sc][256] on the device (16-byte aligned), dfa[s * 256 + b] the state after byte b in state s, < 0 (or >= Sc): dead.
 * tok_bytes (uint8, n_bytes of them) holds the vocabulary's byte strings back to back, token v being
 * tok_bytes[tok_off[v] .. tok_off[v + 1]) (tok_off int32 [V + 1]; a token whose range is empty, reversed or outside the
 * buffer is illegal everywhere).  accepting: uint8 [Sc], nonzero = accepting.  eos_ids: int32 [n_eos] (NULL with
 * n_eos = 0).  Writes rows [base, base + Sc) of the pool, columns [0, V):
 *   table[(base + s) * table_stride + v] = the state where walking token v's bytes from s ends (relative to base), -1 if
 *                                          the walk dies or the token is empty
 *   v an eos id:                           s where accepting[s], -1 elsewhere (whatever its bytes give)
 * Columns >= V and every other row are not touched.  Refused (DFL_EINVAL, nothing launched): a null pointer, V % 8, Sc
 * outside 1..4096, base < 0 or base + Sc > pool_states, table_stride < V or not a multiple of 8, rows off 16 bytes.
 * Plain 16-byte vector stores, no atomics; every pool offset is formed in 64 bits. */
int dfl_grammar_lift(int16_t *table, int64_t table_stride, int pool_states, int V, int base, const int16_t *dfa, int Sc,
                     const uint8_t *tok_bytes, int64_t n_bytes, const int32_t *tok_off, const uint8_t *accepting,
                     const int32_t *eos_ids, int n_eos, void *stream);

/* dfl_grammar_reach: which states a loaded grammar's states lead to.  Reads pool rows [base, base + S), 1 <= S <= 4096,
 * columns [0, V); bias (optional, fp32 [V]): a column holding -inf is banned.  Writes, whole,
 *   adj uint8 [S][S]:    adj[s * S + t] = 1 iff some token v with table[(base + s) * table_stride + v] = t that is not
 *                        banned exists, else 0
 *   any_legal uint8 [S]: 1 iff row s has a legal token at all (banned or not)
 * The same refusals as dfl_grammar_lift.  Byte stores of a value that does not depend on the order of the threads. */
int dfl_grammar_reach(const int16_t *table, int64_t table_stride, int pool_states, int V, int base, int S,
                      const float *bias, uint8_t *adj, uint8_t *any_legal, void *stream);

/* Acceptance scan + commit + bonus token + stop test + length bookkeeping in one
 * wavefront (model/dflash.py:258-268):
 *   acc = #leading i with block[i+1] == posterior[i]           (0..bs-1)
 *   output_ids[start .. start+acc] = block[0..acc]; output_ids[start+acc+1] = posterior[acc]
 *   dyn: S <- start, tau <- acc+1, pos0 <- start, start <- start+acc+1, cycle++, stop |= any stop id
 *        among the acc+2 tokens just written
 * result (int32[4], may be pinned host memory mapped to the device): {acc, new_start, stop, cycle}; words 0..2 are
 * stored first, the cycle counter (>= 1) last behind a system-scope release: a polling host waits for word 3 to change
 * and reads the others afterwards.
 * next_block != NULL: the next cycle's block is RE-ARMED on the device as well (model/dflash.py:235: block =
 * output_ids[:, start:start+bs] = the token just committed at the new start followed by mask ids): next_block[0] <-
 * posterior[acc], next_block[1 .. rearm_n-1] <- mask_id, 1 <= rearm_n <= 64 (next_block may be block_ids itself).  NULL:
 * no re-arm, rearm_n / mask_id unused.
 * dyn_t != NULL (needs next_block): the block-form length record of the NEXT target verify is maintained too (S = POS0 =
 * START = new start, TAU = 0; its BS word is left alone): with it a steady-state cycle needs no host-side length at all —
 * verify and accept can be replayed from a hipGraph (DecodeSession.capture). */
int dfl_accept_commit(const int64_t *block_ids, const int64_t *posterior, int bs, int64_t *output_ids,
                      int64_t output_len, int32_t *dyn, const int64_t *stop_ids, int n_stop, int32_t *result,
                      int64_t *next_block, int rearm_n, int64_t mask_id, int32_t *dyn_t, void *stream);

/* ======================================================================================
 * Target PREFILL on the kernels (model/dflash.py:218-225: target(input_ids, ..., output_hidden_states=True) over the
 * P prompt rows).  Same operands as the decode path: weights as packed by dfl_pack_weight /
 * dfl_pack_weight_gateup, activations as frag16 row tiles — tile t (rows 16t .. 16t+15) of K columns at
 * x_frag + t * 16 * K elements, dfl_prefill_rows_padded(P) / 16 tiles (rows are padded to a multiple of 128; the
 * padding holds zero fragments).  LDS-tiled MFMA GEMM (128 x 128 block tiles, LDS-DMA staging).  N % 128 == 0,
 * K % 64 == 0.  Row buffers must hold dfl_prefill_rows_padded(P) rows; rows >= P are never stored.
 * ====================================================================================== */
int64_t dfl_prefill_rows_padded(int P);

/* out[m][n] = bf16(x[m] . W[n])  (bf16 rows, row stride ldo): the q/k/v projection of the prompt rows. */
int dfl_prefill_gemm_rows(const void *wp, const void *x_frag, int P, int N, int K, void *out, int64_t ldo, void *stream);

/* h_io[m][n] = bf16(h_io[m][n] + bf16(x[m] . W[n])) (o_proj / down_proj + residual add); tap (optional) gets a copy
 * of the new rows (row stride ldtap): a tapped target layer, model/utils.py:16-25. */
int dfl_prefill_gemm_resid(const void *wp, const void *x_frag, int P, int N, int K, void *h_io, int64_t ldh, void *tap,
                           int64_t ldtap, void *stream);

/* act = bf16(silu(gate) * up) over the interleaved gate/up weight (tf:modeling_qwen3.py:82), written as frag16 row
 * tiles of I columns (the down projection's input).  I % 64 == 0. */
int dfl_prefill_gemm_silu(const void *wp_gateup, const void *x_frag, int P, int I, int K, void *act_frag, void *stream);

/* Rows h [P][H] (bf16, row stride ldh) -> Qwen3RMSNorm (tf:modeling_qwen3.py:59-64; norm_w NULL: none) -> frag16 row
 * tiles of H columns; all dfl_prefill_rows_padded(P) / 16 tiles are written (zero fragments beyond row P).
 * H % 32 == 0 and H <= 8192 (a wave keeps its row in registers): a wider H returns DFL_EINVAL and launches nothing. */
int dfl_prefill_norm_pack(const void *h, int64_t ldh, int P, int H, const void *norm_w, float eps, void *x_frag,
                          void *stream);
/* rows [P][K] (row stride ld) -> frag16 row tiles of K columns, any K % 32 == 0 (the draft's fc operand: K = 5 H tapped
 * states per prompt row, model/dflash.py:166-171); no norm. */
int dfl_prefill_pack_rows(const void *rows, int64_t ld, int P, int K, void *x_frag, void *stream);

/* Per-head q/k RMSNorm (weights may be NULL: Llama) + RoPE at positions pos0 + row over the P rows of a bf16 q/k/v row
 * buffer (row stride ld): q is rewritten in place, k (normed, rotated) and v go to cache rows row0 + row of
 * kcache / vcache [n_kv][cache_rows][128].  cos/sin: bf16 [max_pos][64]; a position >= max_pos rotates with table row
 * max_pos - 1 (clamped).  row0 + P <= cache_rows is required (DFL_EINVAL otherwise): no row is ever dropped here. */
int dfl_prefill_qk_rope(void *qkv_rows, int64_t ld, int P, int q_col, int k_col, int v_col, int n_q, int n_kv,
                        const void *q_norm_w, const void *k_norm_w, float eps, const void *cos_tab, const void *sin_tab,
                        int max_pos, int pos0, void *kcache, void *vcache, int cache_rows, int row0, void *stream);

/* Causal attention of the P prompt rows over themselves (GQA, head_dim 128): q = the rows dfl_prefill_qk_rope left in
 * the q/k/v row buffer (row stride ldq, q columns from q_col), K/V = cache rows [0, P) it wrote.  softmax(q k^T * scale)
 * v in fp32 with P rounded to bf16 for the PV product (as dfl_attn_head).  out_frag: frag16 row tiles of n_q * 128
 * columns (o_proj's operand); the tiles of rows >= P within the last written tile are zero. */
int dfl_prefill_attn(const void *q_rows, int64_t ldq, int q_col, const void *kcache, const void *vcache, int cache_rows,
                     int P, int n_q, int n_kv, float scale, void *out_frag, void *stream);

/* Sparse-MoE MLP of the prefill: Qwen3MoeSparseMoeBlock over the P prompt rows of one layer of an MoE target
 * (tf:models/qwen3_moe/modeling_qwen3_moe.py: Qwen3MoeTopKRouter.forward + Qwen3MoeExperts.forward; the reference
 * reaches it through the HF forward of model/dflash.py:218-225, a Python loop over the experts).  The layer's
 * (row, slot) pairs are sorted by expert on the device and each expert's rows gathered into 16-row frag16 tiles, so
 * every expert's packed weights are read once by MFMA row blocks of its own rows.  Call order per layer:
 *   router logits = dfl_prefill_gemm_rows(router weight padded to a multiple of 128 rows) on the ln2-normalised tiles
 *   dfl_prefill_moe_route   fp32 softmax / top-k (probability desc, index asc) / renormalise per row -> pair_e / pair_w
 *                           [P][8]; then (one workgroup) per-expert counts cnt and tile offsets, the work list items =
 *                           (expert, first gathered tile, tiles <= 4) with n_items[0] = items, [1] = tiles, posmap
 *                           [P][8] = gathered row of each pair, src_row / row_w [gathered row] = its source row (-1:
 *                           padding) and routing weight (bf16 value, as float).  WHICH gathered row of its expert's tiles
 *                           a (row, slot) pair gets is decided by the order integer atomics land in: posmap, src_row,
 *                           row_w and the row order of xg / act_g / out32 may differ from launch to launch on the same
 *                           inputs; pair_e / pair_w / cnt / tile_off / n_items and what dfl_prefill_moe_combine leaves
 *                           in h (each row's slots added in slot order) do not
 *   dfl_prefill_moe_gather  the source rows' normalised fragments into the gathered tiles xg (zero for padding rows)
 *   dfl_prefill_moe_gemm_silu   act_g = silu(xg Wg_e^T) * (xg Wu_e^T) per expert (gate/up interleaved as dfl_pack_weight_gateup);
 *                               with src_row (and 1 KiB of zeros for padding rows) `xg` is the UNGATHERED x_frag and the
 *                               gather happens in the kernel's LDS-DMA addresses: no dfl_prefill_moe_gather call, no xg
 *   dfl_prefill_moe_gemm_down   out32[gathered row][H] = row_w * (act_g Wd_e^T), fp32
 *   dfl_prefill_moe_combine     h[m] = bf16(h[m] + bf16(sum over the row's k slots of out32)) (+ tap copy): the sum over
 *                               experts is rounded once (HF: per-expert bf16 adds), as in dfl_moe_down's consumer.
 *                               sum_out != NULL: the fp32 sums [P][H] are stored there instead and h is left alone (the
 *                               ragged-batch decode path adds them in its next dfl_norm_frag_batch).
 * Scratch is caller-owned: cnt / tile_off int32 [E], items int32 [3 * max_items], src_row int32 / row_w float
 * [max_tiles * 16], xg bf16 [max_tiles * 16 * H], act_g bf16 [max_tiles * 16 * I], out32 float [max_tiles * 16 * H].
 * rows_per_item: 64 or 128 rows of one expert per work item (4 or 8 gathered tiles), the same in the three calls of a
 * layer that take it; 128 reads an expert's weights once where it serves up to 128 rows.  E <= 256, top_k <= 8, H % 128 == 0, I % 64 == 0, expert strides = elements per expert. */
int64_t dfl_prefill_moe_max_tiles(int P, int top_k, int E);
int64_t dfl_prefill_moe_max_items(int P, int top_k, int E);
int dfl_prefill_moe_route(const void *logits, int64_t ld, int P, int E, int top_k, int norm_topk, int32_t *pair_e,
                          float *pair_w, int32_t *cnt, int32_t *tile_off, int32_t *items, int32_t *n_items, int32_t *posmap,
                          int32_t *src_row, float *row_w, int rows_per_item, void *stream);
int dfl_prefill_moe_gather(const void *x_frag, int P, int H, int top_k, int E, const int32_t *src_row, const int32_t *n_items,
                           void *xg, void *stream);
int dfl_prefill_moe_gemm_silu(const void *wp_gateup_e, int64_t w_expert_stride, const void *xg, const int32_t *items,
                              const int32_t *n_items, int max_items, int I, int K, void *act_g, int rows_per_item,
                              const int32_t *src_row, const void *zeros_1k, void *stream);
int dfl_prefill_moe_gemm_down(const void *wp_down_e, int64_t w_expert_stride, const void *act_g, const int32_t *items,
                              const int32_t *n_items, int max_items, int H, int I, const float *row_w, float *out32,
                              int rows_per_item, void *stream);
int dfl_prefill_moe_combine(const float *out32, const int32_t *posmap, int P, int H, int top_k, void *h_io, int64_t ldh,
                            void *tap, int64_t ldtap, float *sum_out, void *stream);
/* The two grouped expert GEMMs with the experts' weights as a dfl_weight: what the shared MoE pass of a verify over 2..4
 * tiles launches ("The experts"); every other argument is dfl_prefill_moe_gemm_silu's / _down's.
 * DFL_W_BF16: exactly the launch of dfl_prefill_moe_gemm_silu / _down (those two are this implementation on a bare bf16
 * pointer).  DFL_W_E4M3: expert e's codes at wp + e * w_expert_stride BYTES in dfl_pack_weight_gateup_fp8's (gate/up,
 * N = 2*I rows) or dfl_pack_weight_fp8's (down, N = H rows) layout, scale fp32 [E][N] in that layout's tile order (N floats
 * per expert, 64-byte aligned).  The codes are staged to LDS as they are and converted in front of each MFMA: the same
 * k-steps in the same order into every accumulator, the fp32 sums multiplied by the row's scale in front of the first
 * rounding point (gate/up: before the bf16 rounding of the two Linears' outputs; down: row_w * (sum * scale)) — with
 * power-of-two scales bit-equal to the bf16 launch on q * scale.
 * w_expert_stride: elements of the weight's format between experts; it must be N * K.  N % 128 == 0, K % 64 == 0,
 * rows_per_item 64 or 128, src_row and zeros_1k together or neither; DFL_EINVAL, nothing launched, on any of these, on
 * the descriptor errors of dfl_weight and on scales that are not 64-byte aligned. */
int dfl_moe_grouped_gate_up(const dfl_weight *w_gateup_e, int64_t w_expert_stride, const void *xg, const int32_t *items,
                            const int32_t *n_items, int max_items, int I, int K, void *act_g, int rows_per_item,
                            const int32_t *src_row, const void *zeros_1k, void *stream);
int dfl_moe_grouped_down(const dfl_weight *w_down_e, int64_t w_expert_stride, const void *act_g, const int32_t *items,
                         const int32_t *n_items, int max_items, int H, int I, const float *row_w, float *out32,
                         int rows_per_item, void *stream);

/* ======================================================================================
 * Ragged batch of requests on one GPU (BASELINE.json configs[2]; SURVEY.md §8e: "within a
 * GPU the requests are a ragged batch for the kernels: shared weight stream, per-request
 * S and tau").  The reference has no batched form of the path — "batch" there is a Python
 * loop over prompts (benchmark_batched.py:212-243, benchmark.py:445) — so these entry
 * points replace R consecutive passes of model/dflash.py:235-268 by one pass in which the
 * R requests share every weight byte.  Request r (0 <= r < R <= 4 per launch):
 *   - 16-row tile at `base + r * stride` of every activation buffer,
 *   - lengths at dyn + r * DFL_DYN_WORDS,
 *   - KV cache at cache + r * cache_req_stride.
 * The GEMMs are compiled for 2 or 4 tiles: buffers (and dyn) must hold dfl_batch_tiles(R)
 * requests; the unused ones need valid (readable) memory and dyn words of zero.
 * ====================================================================================== */
typedef struct dfl_rows_batch {
  dfl_rows r0;          /* request 0: mode 0 (frag16) or 1 (plain rows); mode 2 is rejected — take
                         * normalised rows from dfl_norm_frag_batch */
  int64_t frag_stride;  /* bf16 elements between the requests' frag16 buffers (mode 0), %8 == 0 */
  int64_t rows_stride;  /* bf16 elements between the requests' row buffers (mode 1, 2) */
  int64_t ss_stride;    /* floats between the requests' sum-of-squares partials (mode 2) */
} dfl_rows_batch;

int dfl_batch_tiles(int R);  /* 2 for R <= 2, else 4 */
/* K parts the batched GEMMs cut K into (grid.y): ceil(K / 2048), at most 16 (K <= 32768).  A part is NOT 2048 columns
 * unless K is a multiple of it: the K / 32 k-steps are dealt evenly, part c covers the 8 * ceil(K / 32 / (8 * ksplit))
 * k-steps from c times that many on (K = 2080: 1280 + 800 columns), the last part what is left. */
int dfl_batch_ksplit(int K);
/* workspace of the fused-epilogue batched GEMMs: arrival tickets (ZEROED once by the caller,
 * left zero by every launch), argmax candidates, fp32 partial tiles of the K parts */
int64_t dfl_gemm_batch_ws_bytes(int N, int K);

/* e4m3 weights in the batched GEMMs that take a dfl_weight ("The batch forms"): scales 64-byte
 * aligned, K % 64 == 0, K >= 256.  The sums are multiplied by the columns' scales in front of the bf16 form's first
 * rounding: gate and up separately, logits and argmax over bf16(sum * scale), and EVERY K part of dfl_gemm_f32_batch's
 * output (the launch that sums the parts is untouched).  dfl_gemm_silu_mul_batch, dfl_gemm_argmax_batch and
 * dfl_gemm_sample_batch run e4m3 in the ring form only: -22 for a source that is not frag16 (mode 0), never a quiet
 * fall-back to the slab form or to the bf16 kernels. */
/* dfl_gemm_f32 for R requests: out[c][r*16+m][n], c < dfl_batch_ksplit(K) partial sums
 * (out holds ksplit * dfl_batch_tiles(R) * 16 * N floats). */
int dfl_gemm_f32_batch(const dfl_weight *w, const dfl_rows_batch *x, int R, int N, int K, float *out, const int32_t *dyn,
                       void *stream);
/* dfl_gemm_silu_mul for R requests; request r's frag16 output at act_frag + r * act_stride. */
int dfl_gemm_silu_mul_batch(const dfl_weight *w_gateup, const dfl_rows_batch *x, int R, int I, int K, void *act_frag,
                            int64_t act_stride, void *ws, const int32_t *dyn, void *stream);
/* dfl_gemm_resid for R requests (h_io, tap, ss_out advance by their strides per request). */
int dfl_gemm_resid_batch(const void *wp, const dfl_rows_batch *x, int R, int N, int K, void *h_io, int64_t ldh,
                         int64_t h_stride, int add_residual, void *tap, int64_t ldtap, int64_t tap_stride,
                         float *ss_out, int64_t ss_stride, void *ws, const int32_t *dyn, void *stream);
/* dfl_gemm_argmax for R requests: out_ids[r * out_stride + out_off + (row - row0)]. */
int dfl_gemm_argmax_batch(const dfl_weight *w, const dfl_rows_batch *x, int R, int V, int K, int row0, int nrows,
                          const int32_t *dyn, int nrows_dyn_word, void *ws, int64_t *out_ids, int64_t out_stride,
                          int out_off, void *logits, int64_t logits_stride, void *stream);
/* dfl_gemm_sample for R <= 4 request tiles on one pass over the weights (ring form, EPI_SAMPLE epilogue): tile t is tile
 * j = t % tiles_per_req of request q = t / tiles_per_req; its row m draws position dyn[t][pos_word] + pos_add + 16 j + m
 * with seed seeds[q] (int64, one per request slot: a captured batch graph and a re-admitted slot keep working).  dyn
 * holds batch_tiles(R) records, seeds batch_tiles(R) / tiles_per_req entries.  No slab form: -22 where the ring form
 * does not apply.
 * inv_ts == NULL: every slot draws at the host inv_t (in (0, 1e5]).  inv_ts != NULL (EPI_SAMPLE_T epilogue; inv_t unused):
 * a device fp32 array of batch_tiles(R) / tiles_per_req entries, indexed by q like seeds, read by address on every launch
 * (a replayed graph sees what an admission wrote).  Per slot:
 *   inv_ts[q] > 0     sampled: argmax_v fmaf(bf16(logit_v), inv_ts[q], noise of dfl_rng.h) — the draw at that slot's own
 *                     invT (the host writes float32(1 / T));
 *   otherwise         (0, negative, NaN) greedy: argmax_v bf16(logit_v), lowest v on ties, no Philox call and no noise —
 *                     bit for bit the ids of dfl_gemm_argmax_batch on the same inputs.
 * Device values are not validated. */
int dfl_gemm_sample_batch(const dfl_weight *w, const dfl_rows_batch *x, int R, int V, int K, int row0, int nrows,
                          const int32_t *dyn, int nrows_dyn_word, void *ws, int64_t *out_ids, int64_t out_stride,
                          int out_off, void *logits, int64_t logits_stride, const int64_t *seeds, const float *inv_ts,
                          float inv_t, int rng_stream, int pos_word, int pos_add, int tiles_per_req, void *stream);
/* dfl_embed_rows for R requests: ids[r * ids_stride + m]. */
int dfl_embed_rows_batch(const void *embed, const int64_t *ids, int64_t ids_stride, int R, void *h_out,
                         int64_t h_stride, int H, float *ss_out, int64_t ss_stride, const int32_t *dyn, int dyn_word,
                         void *stream);

/* Residual add + RMSNorm of R requests' rows straight into frag16 (model/dflash.py:140,144 +
 * Qwen3RMSNorm, tf:models/qwen3/modeling_qwen3.py:59-64):
 *   h[r][m]   <- part ? bf16(h[r][m] + bf16(sum_{k<nsplit} part[k*part_split + (r*16+m)*ldp ..])) : h[r][m]
 *   tap[r][m] <- that row (optional: a tapped target layer, model/utils.py:16-25)
 *   frag[r]   <- norm_w * bf16(h * rstd);  rows >= dyn[r][dyn_word] (all 16 rows count when dyn is NULL): frag zeroed,
 *                h AND tap untouched (a tap row keeps what it held), their part rows loaded but ignored (readable memory, any contents).
 * The sum starts from an fp32 zero and takes the parts in the order k = 0, 1, ...; part k of request r's row m starts at
 * part + k * part_split + (r * 16 + m) * ldp — for dfl_gemm_f32_batch's output part_split = dfl_batch_tiles(R) * 16 * N
 * and ldp = N, whatever number of tile slots the caller's other buffers have.  Only the requests r < R are touched.
 * H % 8 == 0, H <= 16384; ldh >= H, ldh % 8 == 0; ldp >= H, ldp % 4 == 0, nsplit >= 1 (with part); ldtap >= H,
 * ldtap % 8 == 0 (with tap); frag_stride >= 16 * H, % 8 == 0; 1 <= R <= 4: DFL_EINVAL otherwise, nothing launched.
 * `part` = the fp32 K-part sums of the o_proj / down_proj GEMM just before it
 * (dfl_gemm_f32_batch): the parts meet at this launch boundary — the kernel reads every h row
 * anyway — instead of inside the GEMM.  The batched GEMMs read their normalised operand from
 * here (the in-GEMM norm of the single-request path is replicated in every workgroup, which
 * at 4 tiles costs more than this launch). */
int dfl_norm_frag_batch(void *h, int64_t h_stride, int64_t ldh, int R, const float *part, int nsplit,
                        int64_t part_split, int ldp, void *tap, int64_t ldtap, int64_t tap_stride, const void *norm_w,
                        float eps, void *frag, int64_t frag_stride, int H, const int32_t *dyn, int dyn_word,
                        void *stream);

/* Context K/V of ALL draft layers for R requests in one launch (model/dflash.py:73-85, the
 * context half): kv = fp32 partials of the context rows times the concatenated k/v weights
 * of the n_layers layers (layer i's k columns at k_col + i * col_layer_stride, v alike);
 * k_norm + RoPE (position pos0 + row) -> caches at rows S + row, row < dyn tau.  The block
 * stage that follows then sees them as cached rows (lengths in block form, see
 * dfl_accept_commit_batch).  R counts 16-row TILES with one length record each, tiles_per_req (>= 1) consecutive tiles
 * sharing one request's cache: 1 for blocks of <= 16 rows; 2 for the context rows of requests that run 17..32-row blocks
 * (up to 32 accepted rows per cycle). */
int dfl_kv_append_batch(const float *kv, int nsplit, int64_t split_stride, int ld, int k_col, int v_col,
                        int col_layer_stride, int n_layers, int R, int req_rows, int n_kv, const void *k_norm_w,
                        int64_t kw_layer_stride, float eps, const void *cos_tab, const void *sin_tab, int max_pos,
                        void *kcache, void *vcache, int cache_rows, int64_t cache_req_stride,
                        int64_t cache_layer_stride, const int32_t *dyn, int tiles_per_req, void *stream);

/* dfl_attn_fused for R requests (grid.z = request): request r's block rows at partial-buffer
 * rows blk_row0 + r * req_rows, cache at + r * cache_req_stride, frag16 output at
 * + r * out_req_stride; no context rows in this form (dyn tau == 0).
 * ws: dfl_attn_fused_batch_ws_bytes bytes, zeroed once. */
int64_t dfl_attn_fused_batch_ws_bytes(int R, int n_q, int n_kv, int max_splits);
int dfl_attn_fused_batch(const float *qkv, int nsplit, int64_t split_stride, int ld, int q_col, int k_col, int v_col,
                         int blk_row0, int req_rows, int R, int n_q, int n_kv, const void *q_norm_w,
                         const void *k_norm_w, float eps, const void *cos_tab, const void *sin_tab, int max_pos,
                         void *kcache, void *vcache, int cache_rows, int64_t cache_req_stride, float scale, int causal,
                         const int32_t *dyn, int kv_len_max, void *ws, int max_splits, void *out_frag,
                         int64_t out_req_stride, void *stream);

/* dfl_accept_commit for R requests, one wavefront each (model/dflash.py:258-268 per request).
 * bs is read from dyn_d.  Updates dyn_d (draft form: S <- start, tau <- acc+1, pos0 <- start,
 * start <- start+acc+1) and dyn_t (block form: S = pos0 = start = new start, tau = 0, bs / stop / cycle
 * copied from dyn_d), the latter read by the target verify and by the draft's block stage of the next cycle;
 * the spare word of both is left alone.
 * result int32 [R][4] = {acc, new_start, stop, cycle}.  A request with dyn_d bs == 0 is idle: none of its rows
 * is read and no word of its slot (ids, records, result, block) is written.
 * next_block (optional, may alias block_ids; same stride): re-armed for the next cycle as
 * [bonus token, mask_id x (16 * tiles_per_req - 1)] = output_ids[new start .. ) (model/dflash.py:235).
 * Requests of tiles_per_req (1 or 2) 16-row tiles — 2: blocks of up to 32 rows.  With dyn_d_tiles / dyn_t_tiles (both or
 * neither; required for tiles_per_req = 2; blk_stride >= 16 * tiles_per_req) one record per TILE is kept for the per-tile
 * launches besides the per-request records (dyn_d_tiles: S / pos0 = start + 16 j, tau = the tile's share of the acc + 1
 * context rows, start = new start; dyn_t_tiles: block form with bs = the tile's share of the block rows); every other
 * word of a tile record (dyn_d_tiles bs, stop, cycle, spare) is left as it was.  tiles_per_req = 1 with the per-request
 * records passed as the tile records too leaves what NULL tile records leave. */
int dfl_accept_commit_batch(const int64_t *block_ids, int64_t blk_stride, const int64_t *posterior,
                            int64_t post_stride, int R, int64_t *output_ids, int64_t out_stride, int64_t output_len,
                            int32_t *dyn_d, int32_t *dyn_t, const int64_t *stop_ids, int n_stop, int32_t *result,
                            int64_t *next_block, int64_t mask_id, int tiles_per_req, int32_t *dyn_d_tiles,
                            int32_t *dyn_t_tiles, void *stream);

/* Slot admission of the ragged batch: ONE launch re-arms request slot r (0 <= r < n_slots) for a request whose prompt
 * has just been prefilled, from device-resident inputs only (nothing is read back, nothing copied from the host):
 *   output_ids[r][0..P) <- prompt_ids, [P] <- *first_token (a device int64), (P, out_len) <- mask_id
 *   block[r] <- [*first_token, mask_id x (blk_w - 1)];  post[r], result[r] <- 0   (block / post: [n_slots][blk_w])
 *   taps tile r (16 rows of fc_in bf16 at taps + r * 16 * fc_in) <- tail_rows[0..n_tail) (row stride ld_tail), rows
 *     n_tail..15 zero: the prompt's last n_tail = min(16, P) tapped rows, the first cycle's context tile
 *   dyn_d[r] <- {P - n_tail, n_tail, bs, P - n_tail, P, 0, 0, 0};  dyn_t[r] <- {P, 0, bs, P, P, 0, 0, 0}
 *   seeds[r] <- seed  (seeds may be NULL: the slot's seed is left alone)
 * Rows of the slot's KV caches past these lengths keep whatever the slot's previous request left: no launch reads them
 * before the cycle that rewrites them.  fc_in % 8 == 0, rows 16-byte aligned.  DFL_EINVAL: null pointer, r outside
 * 0..n_slots-1, P < 1 or P + 1 > out_len, n_tail outside 0..min(16, P), bs outside 0..blk_w. */
int dfl_admit_slot(int r, int n_slots, const int64_t *prompt_ids, int P, const int64_t *first_token, int64_t *output_ids,
                   int64_t out_stride, int64_t out_len, int64_t *block, int64_t *post, int blk_w, int32_t *result,
                   const void *tail_rows, int64_t ld_tail, int n_tail, void *taps, int fc_in, int32_t *dyn_d,
                   int32_t *dyn_t, int bs, int64_t *seeds, int64_t seed, int64_t mask_id, void *stream);

/* Stop sequences: per-slot, multi-token stops matched in front of the accept launch, over
 * exactly the tokens that launch is about to commit.  One wavefront per slot s = 0 .. slots-1; rows of slot s at
 * block_ids + s * blk_stride, posterior + s * post_stride, output_ids + s * out_stride (int64), its record at
 * dyn + s * DFL_DYN_WORDS (for the ragged batch: the draft-form record dyn_d, whose stop word the accept launch copies
 * and publishes), its tables at
 *   seq_ids   int32 [slots][DFL_STOP_SEQS][DFL_STOP_SEQ_LEN]      seq_len  int32 [slots][DFL_STOP_SEQS], 0 = unused
 *   first_pos int32 [slots]   min_end  int32 [slots]               hit      int32 [slots][2], {-1, -1} = none yet
 * bs >= 0: the block size of every slot; bs < 0: the record's DFL_DYN_BS word (cut to min(32, blk_stride, post_stride):
 * nothing past a row is read).  With start = dyn[DFL_DYN_START] and acc = the leading i < bs - 1 with
 * block_ids[i + 1] == posterior[i] (the accept launch's ballot), the newly committed ids are those of positions
 * start + 1 .. start + acc + 1 = block_ids[1 .. acc] then posterior[acc]; position start and everything before it is
 * read from output_ids (never below index 0, never at or past output_len).  For every end position e in that range and
 * every sequence k with length L_k > 0 (a stored length is taken into 0..16), the window [e - L_k + 1, e] MATCHES when it
 * equals seq_ids[s][k][0 .. L_k), e - L_k + 1 >= max(first_pos[s], 0) and e >= min_end[s].  Of all matches the smallest e
 * wins, at equal e the smallest k; then dyn[DFL_DYN_STOP] |= 1 and, only while hit[s] is still {-1, -1}, hit[s] <- {e, k}.
 * A slot with block size 0 or with every L_k == 0 is left untouched, and so is everything of a slot without a match.
 * Nothing but the stop word and hit is written, with plain vector stores; the logits are never read.
 * DFL_EINVAL, nothing launched: a null pointer, slots < 1, bs > 32, blk_stride or post_stride below max(bs, 1),
 * output_len < 1, out_stride < output_len.  bs == 0 launches nothing and returns DFL_OK. */
#define DFL_STOP_SEQS 8
#define DFL_STOP_SEQ_LEN 16
#define DFL_STOP_SEQ_MAX_BS 32
int dfl_stop_seq_rows(const int64_t *block_ids, int64_t blk_stride, const int64_t *posterior, int64_t post_stride,
                      const int64_t *output_ids, int64_t out_stride, int64_t output_len, int32_t *dyn, int slots, int bs,
                      const int32_t *seq_ids, const int32_t *seq_len, const int32_t *first_pos, const int32_t *min_end,
                      int32_t *hit, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DFLASH_HIP_H */
