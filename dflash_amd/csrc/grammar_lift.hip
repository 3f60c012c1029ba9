// Structured outputs: a byte automaton lifted to the token table on the device.
//   k_grammar_lift:  pool rows [base, base + Sc) of the int16 table from a byte DFA int16 [Sc][256] (-1: dead) and the
//                    vocabulary's byte strings (uint8, back to back, int32 offsets [V + 1]) — TokenDFA.from_bytes entry
//                    for entry.  grid (V / 8 / 512, Sc / 16): a thread owns 8 consecutive tokens, whose first 8 bytes it
//                    holds in registers (the rest is read from the buffer), and walks them from each of its workgroup's
//                    16 states: byte position outer, token inner, so that 8 independent table reads are in flight per
//                    step.  A state's 8 successors go out as one 16-byte store.  The byte DFA is copied to LDS when it
//                    has at most 128 states (64 KiB) and read through L2 above.
//   k_grammar_reach: one 1024-thread workgroup per pool row s of a loaded grammar: the successors of its legal, not
//                    banned tokens are marked in an LDS byte map (plain stores of 1: the order does not matter), which
//                    then goes out as row s of adj, whole; any_legal[s] beside it.
// Plain vector stores, no atomics: the same inputs give the same bits.  Every pool offset is formed in 64 bits.
#include "dfl_common.h"

namespace {

constexpr int LF_NT = 512;           // threads of a lift workgroup: 4096 tokens
constexpr int LF_SLICE = 16;         // states of a lift workgroup
constexpr int LF_LDS_STATES = 128;   // the byte DFA fits LDS up to here (128 * 256 * 2 = 64 KiB)
constexpr int LF_REG = 8;            // bytes of a token held in registers
constexpr int LF_MAX_STATES = 4096;
constexpr int RC_NT = 1024;

struct LiftArgs {
  int16_t *table;
  int64_t table_stride;
  int V, base, Sc;
  const int16_t *dfa;
  const uint8_t *bytes;
  int64_t n_bytes;
  const int32_t *off;
  const uint8_t *accepting;
  const int32_t *eos;
  int n_eos;
};

template <bool LDS>
__global__ __launch_bounds__(LF_NT) void k_grammar_lift(LiftArgs a) {
  __shared__ __attribute__((aligned(16))) int16_t sd[LDS ? LF_LDS_STATES * 256 : 8];
  const int tid = threadIdx.x;
  const int Sc = a.Sc;
  if (LDS) {  // the whole automaton: a walk reaches any state
    const u32x4 *src = reinterpret_cast<const u32x4 *>(a.dfa);
    u32x4 *dst = reinterpret_cast<u32x4 *>(sd);
    for (int i = tid; i < Sc * 32; i += LF_NT) dst[i] = src[i];
    __syncthreads();
  }
  const int c = blockIdx.x * LF_NT + tid;  // tokens 8 c .. 8 c + 7
  if (c >= (a.V >> 3)) return;
  const int16_t *dfa = LDS ? sd : a.dfa;

  int start[8], len[8], maxlen = 0;
  uint32_t w0[8], w1[8];
  int prev = a.off[c * 8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int next = a.off[c * 8 + e + 1];
    int n = next - prev;
    if (prev < 0 || n < 0 || (int64_t)prev + n > a.n_bytes) n = 0;  // offsets that leave the buffer: the token is illegal
    start[e] = prev;
    len[e] = n;
    maxlen = max(maxlen, n);
    w0[e] = 0u;
    w1[e] = 0u;
    for (int i = 0; i < LF_REG && i < n; ++i) {
      const uint32_t b = a.bytes[(int64_t)prev + i];
      if (i < 4)
        w0[e] |= b << (8 * i);
      else
        w1[e] |= b << (8 * (i - 4));
    }
    prev = next;
  }
  uint32_t eos_mask = 0u;
  for (int k = 0; k < a.n_eos; ++k) {
    const int id = a.eos[k];
    if (id >= 0 && (id >> 3) == c) eos_mask |= 1u << (id & 7);
  }

  const int s0 = blockIdx.y * LF_SLICE, s1 = min(s0 + LF_SLICE, Sc);
  const int head = min(maxlen, LF_REG);
  for (int s = s0; s < s1; ++s) {
    int cur[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cur[e] = len[e] > 0 ? s : -1;  // an empty byte string is illegal everywhere
    for (int i = 0; i < head; ++i) {
      const int sh = 8 * (i & 3);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint32_t b = ((i < 4 ? w0[e] : w1[e]) >> sh) & 0xffu;
        const bool on = i < len[e] && cur[e] >= 0;  // a walk stops at its first dead step
        const int nx = dfa[(on ? cur[e] : 0) * 256 + (int)b];
        if (on) cur[e] = (nx < 0 || nx >= Sc) ? -1 : nx;
      }
    }
    if (maxlen > LF_REG) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const uint8_t *p = a.bytes + (int64_t)start[e];
        for (int i = LF_REG; i < len[e] && cur[e] >= 0; ++i) {
          const int nx = dfa[cur[e] * 256 + (int)p[i]];
          cur[e] = (nx < 0 || nx >= Sc) ? -1 : nx;
        }
      }
    }
    if (eos_mask) {  // an eos id: the state itself where it accepts, illegal elsewhere, whatever its bytes give
      const int at = a.accepting[s] ? s : -1;
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if ((eos_mask >> e) & 1u) cur[e] = at;
    }
    u32x4 o;
#pragma unroll
    for (int h = 0; h < 4; ++h)
      o[h] = ((uint32_t)cur[2 * h] & 0xffffu) | (((uint32_t)cur[2 * h + 1] & 0xffffu) << 16);
    *reinterpret_cast<u32x4 *>(a.table + (int64_t)(a.base + s) * a.table_stride + (int64_t)c * 8) = o;
  }
}

struct ReachArgs {
  const int16_t *table;
  int64_t table_stride;
  int V, base, S;
  const float *bias;
  uint8_t *adj, *any_legal;
};

__global__ __launch_bounds__(RC_NT) void k_grammar_reach(ReachArgs a) {
  __shared__ uint8_t seen[LF_MAX_STATES];
  __shared__ int legal;
  const int tid = threadIdx.x, s = blockIdx.x, S = a.S;
  for (int t = tid; t < S; t += RC_NT) seen[t] = 0;
  if (tid == 0) legal = 0;
  __syncthreads();
  const int16_t *row = a.table + (int64_t)(a.base + s) * a.table_stride;
  bool mine = false;
  for (int c = tid; c < (a.V >> 3); c += RC_NT) {
    const u32x4 w = *reinterpret_cast<const u32x4 *>(row + (int64_t)c * 8);
    if ((w[0] & w[1] & w[2] & w[3] & 0x80008000u) == 0x80008000u) continue;  // no legal token among the 8
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int t = (int)(int16_t)((w[e >> 1] >> (16 * (e & 1))) & 0xffffu);
      if (t < 0) continue;
      mine = true;
      if (a.bias && a.bias[c * 8 + e] == -INFINITY) continue;  // banned
      if (t < S) seen[t] = 1;
    }
  }
  if (mine) legal = 1;
  __syncthreads();
  for (int t = tid; t < S; t += RC_NT) a.adj[(int64_t)s * S + t] = seen[t];
  if (tid == 0) a.any_legal[s] = legal ? 1 : 0;
}

bool lf_pool_ok(const void *table, int64_t table_stride, int pool_states, int V) {
  return pool_states >= 1 && table_stride >= V && table_stride % 8 == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0;
}

}  // namespace

extern "C" int dfl_grammar_lift(int16_t *table, int64_t table_stride, int pool_states, int V, int base,
                                const int16_t *dfa, int Sc, const uint8_t *tok_bytes, int64_t n_bytes,
                                const int32_t *tok_off, const uint8_t *accepting, const int32_t *eos_ids, int n_eos,
                                void *stream) {
  DFL_REQUIRE(table && dfa && tok_bytes && tok_off && accepting && (eos_ids || n_eos == 0),
              "dfl_grammar_lift: null pointer");
  DFL_REQUIRE(V >= 8 && V % 8 == 0, "dfl_grammar_lift: V=%d is not a positive multiple of 8", V);
  DFL_REQUIRE(Sc >= 1 && Sc <= LF_MAX_STATES, "dfl_grammar_lift: Sc=%d outside 1..%d", Sc, LF_MAX_STATES);
  DFL_REQUIRE(lf_pool_ok(table, table_stride, pool_states, V),
              "dfl_grammar_lift: pool_states=%d table_stride=%lld (>= 1; >= V, a multiple of 8, rows on 16 bytes)",
              pool_states, (long long)table_stride);
  DFL_REQUIRE(base >= 0 && (int64_t)base + Sc <= pool_states, "dfl_grammar_lift: rows [%d,%lld) outside the pool of %d",
              base, (long long)base + Sc, pool_states);
  DFL_REQUIRE(n_bytes >= 0 && n_bytes < ((int64_t)1 << 31) && n_eos >= 0 &&
                  (reinterpret_cast<uintptr_t>(dfa) & 15) == 0,
              "dfl_grammar_lift: n_bytes=%lld n_eos=%d (the byte DFA on 16 bytes)", (long long)n_bytes, n_eos);
  LiftArgs a{table, table_stride, V, base, Sc, dfa, tok_bytes, n_bytes, tok_off, accepting, eos_ids, n_eos};
  const dim3 grid(((V >> 3) + LF_NT - 1) / LF_NT, (Sc + LF_SLICE - 1) / LF_SLICE);
  if (Sc <= LF_LDS_STATES)
    hipLaunchKernelGGL(k_grammar_lift<true>, grid, dim3(LF_NT), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_grammar_lift<false>, grid, dim3(LF_NT), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH("dfl_grammar_lift");
  return DFL_OK;
}

extern "C" int dfl_grammar_reach(const int16_t *table, int64_t table_stride, int pool_states, int V, int base, int S,
                                 const float *bias, uint8_t *adj, uint8_t *any_legal, void *stream) {
  DFL_REQUIRE(table && adj && any_legal, "dfl_grammar_reach: null pointer");
  DFL_REQUIRE(V >= 8 && V % 8 == 0, "dfl_grammar_reach: V=%d is not a positive multiple of 8", V);
  DFL_REQUIRE(S >= 1 && S <= LF_MAX_STATES, "dfl_grammar_reach: S=%d outside 1..%d", S, LF_MAX_STATES);
  DFL_REQUIRE(lf_pool_ok(table, table_stride, pool_states, V),
              "dfl_grammar_reach: pool_states=%d table_stride=%lld (>= 1; >= V, a multiple of 8, rows on 16 bytes)",
              pool_states, (long long)table_stride);
  DFL_REQUIRE(base >= 0 && (int64_t)base + S <= pool_states, "dfl_grammar_reach: rows [%d,%lld) outside the pool of %d",
              base, (long long)base + S, pool_states);
  ReachArgs a{table, table_stride, V, base, S, bias, adj, any_legal};
  hipLaunchKernelGGL(k_grammar_reach, dim3(S), dim3(RC_NT), 0, (hipStream_t)stream, a);
  DFL_CHECK_LAUNCH("dfl_grammar_reach");
  return DFL_OK;
}
