// Stop sequences: multi-token, per-slot stops matched on the device, in front of the accept launch.
// The launch recomputes the accept launch's ballot, so it sees exactly the tokens that launch is about to commit — never a
// rejected draft token — and ORs DFL_DYN_STOP, which the accept launch then carries into the block-form record and
// publishes in its result words.  It never reads the logits.
#include "dfl_common.h"

namespace {

constexpr int SQ_N = DFL_STOP_SEQS, SQ_L = DFL_STOP_SEQ_LEN, SQ_BS = DFL_STOP_SEQ_MAX_BS;
constexpr int SQ_WIN = SQ_L - 1 + SQ_BS + 1;   // ids a launch can look at: 15 behind start, start itself, <= 32 new ones

// One wavefront per slot.  Lane i takes the accept ballot's comparison i; lanes 0..47 then stage the ids at positions
// start - 15 .. start + acc + 1 (output_ids up to start, block[1..acc], posterior[acc]); lane j <= acc owns end position
// e = start + 1 + j and walks the slot's sequences in index order; the lowest lane with a match wins.
__global__ __launch_bounds__(64) void k_stop_seq_rows(const int64_t *block_ids, int64_t blk_stride, const int64_t *posterior,
                                                      int64_t post_stride, const int64_t *output_ids, int64_t out_stride,
                                                      int64_t output_len, int32_t *dyn, int bs_host,
                                                      const int32_t *__restrict__ seq_ids, const int32_t *__restrict__ seq_len,
                                                      const int32_t *__restrict__ first_pos, const int32_t *__restrict__ min_end,
                                                      int32_t *hit) {
  __shared__ int64_t s_tok[SQ_WIN];
  __shared__ int32_t s_seq[SQ_N * SQ_L];
  __shared__ int32_t s_len[SQ_N];
  const int r = blockIdx.x, i = threadIdx.x;
  block_ids += r * blk_stride;
  posterior += r * post_stride;
  output_ids += r * out_stride;
  dyn += r * DFL_DYN_WORDS;
  seq_ids += r * (SQ_N * SQ_L);
  seq_len += r * SQ_N;
  hit += r * 2;
  int bs = bs_host >= 0 ? bs_host : dyn[DFL_DYN_BS];
  // a record's block size beyond the rows the strides give (or beyond 32) is cut to them: nothing past a row is read
  const int cap = (int)(blk_stride < post_stride ? blk_stride : post_stride);
  bs = bs > SQ_BS ? SQ_BS : bs;
  bs = bs > cap ? cap : bs;
  if (bs <= 0) return;   // idle slot (wave-uniform)
  if (i < SQ_N) {
    const int l = seq_len[i];
    s_len[i] = l < 0 ? 0 : (l > SQ_L ? SQ_L : l);
  }
  s_seq[i] = seq_ids[i];
  s_seq[i + 64] = seq_ids[i + 64];
  __syncthreads();
  int any_len = 0;
#pragma unroll
  for (int k = 0; k < SQ_N; ++k) any_len |= s_len[k];
  if (any_len == 0) return;   // no sequences (wave-uniform)

  const int start = dyn[DFL_DYN_START];
  const bool cmp = i < bs - 1;
  const bool eq = cmp && (block_ids[i + 1] == posterior[i]);
  const unsigned long long mism = __ballot(cmp && !eq);
  const int acc = mism ? (int)__builtin_ctzll(mism) : bs - 1;   // leading matches, 0..bs-1: the accept launch's value
  if (i < SQ_WIN) {
    const int64_t p = (int64_t)start - (SQ_L - 1) + i;   // position of window slot i
    const int d = i - (SQ_L - 1);                        // p - start
    int64_t t = -1;                                      // no token id is negative: never equal to a sequence id
    if (d <= 0) {
      if (p >= 0 && p < output_len) t = output_ids[p];
    } else if (d <= acc) {
      t = block_ids[d];
    } else if (d == acc + 1) {
      t = posterior[acc];
    }
    s_tok[i] = t;
  }
  __syncthreads();
  int kbest = -1;
  if (i <= acc) {
    const int64_t e = (int64_t)start + 1 + i;
    const int fp = first_pos[r] < 0 ? 0 : first_pos[r];
    if (e >= (int64_t)min_end[r]) {
      for (int k = 0; k < SQ_N && kbest < 0; ++k) {
        const int L = s_len[k];
        if (L == 0 || e - L + 1 < (int64_t)fp) continue;
        bool m = true;
        // window slot of position e is (SQ_L - 1) + 1 + i
        for (int c = 0; c < L; ++c) m &= (s_tok[SQ_L + i - (L - 1) + c] == (int64_t)s_seq[k * SQ_L + c]);
        if (m) kbest = k;
      }
    }
  }
  const unsigned long long found = __ballot(kbest >= 0);
  if (found == 0ull) return;
  const int win = (int)__builtin_ctzll(found);   // the smallest end position
  if (i == win) {
    dyn[DFL_DYN_STOP] |= 1;
    if (hit[0] == -1 && hit[1] == -1) {
      hit[0] = start + 1 + i;
      hit[1] = kbest;
    }
  }
}

}  // namespace

extern "C" int dfl_stop_seq_rows(const int64_t *block_ids, int64_t blk_stride, const int64_t *posterior, int64_t post_stride,
                                 const int64_t *output_ids, int64_t out_stride, int64_t output_len, int32_t *dyn, int slots,
                                 int bs, const int32_t *seq_ids, const int32_t *seq_len, const int32_t *first_pos,
                                 const int32_t *min_end, int32_t *hit, void *stream) {
  DFL_REQUIRE(block_ids && posterior && output_ids && dyn && seq_ids && seq_len && first_pos && min_end && hit,
              "dfl_stop_seq_rows: null pointer");
  DFL_REQUIRE(slots >= 1 && slots <= 65535, "dfl_stop_seq_rows: slots=%d outside 1..65535", slots);
  DFL_REQUIRE(bs <= DFL_STOP_SEQ_MAX_BS, "dfl_stop_seq_rows: bs=%d outside 0..%d (negative: the record's DFL_DYN_BS)", bs,
              DFL_STOP_SEQ_MAX_BS);
  const int64_t need = bs > 0 ? bs : 1;
  DFL_REQUIRE(blk_stride >= need && post_stride >= need,
              "dfl_stop_seq_rows: blk_stride=%lld / post_stride=%lld below the %lld block rows", (long long)blk_stride,
              (long long)post_stride, (long long)need);
  DFL_REQUIRE(output_len >= 1 && out_stride >= output_len, "dfl_stop_seq_rows: out_stride=%lld below output_len=%lld (>= 1)",
              (long long)out_stride, (long long)output_len);
  if (bs == 0) return DFL_OK;   // every slot idle
  hipLaunchKernelGGL(k_stop_seq_rows, dim3(slots), dim3(64), 0, (hipStream_t)stream, block_ids, blk_stride, posterior,
                     post_stride, output_ids, out_stride, output_len, dyn, bs, seq_ids, seq_len, first_pos, min_end, hit);
  DFL_CHECK_LAUNCH("dfl_stop_seq_rows");
  return DFL_OK;
}
