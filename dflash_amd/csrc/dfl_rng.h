// Counter-based noise for seeded on-device sampling.  Stateless: every value is a pure function
// of (seed, stream, position, vocab id, extra), so a draw does not depend on the launch form, on the other rows of the
// launch or on how often a captured graph has been replayed.
//
// Bit for bit (tests/sampling_ref.py mirrors it in numpy):
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (v >> 2, p, extra, stream)                      all uint32
//   w       = Philox4x32-10(counter, key)[v & 3]              (Random123's constants and key schedule)
//   u       = ((w >> 9) + 0.5) * 2^-23                        exact in fp32, strictly inside (0, 1)
//   g       = -logf(-logf(u))                                 standard Gumbel
//   value   = fmaf(bf16(logit_v), invT, g)                    one rounding; the draw is its argmax (lowest v on ties)
// The four columns 4c .. 4c+3 share one Philox call.
#pragma once
#include <stdint.h>

#define DFL_RNG_TARGET 0u  // the target's posterior: p = output position the row predicts, extra = 0
#define DFL_RNG_DRAFT 1u   // the draft's block slots (policy loop at T > 0): p = slot position, extra = block start

__device__ __forceinline__ void dfl_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k0 += 0x9E3779B9u;
      k1 += 0xBB67AE85u;
    }
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = lo1;
    c[2] = n2;
    c[3] = lo0;
  }
}

// the four words of column group v >> 2
__device__ __forceinline__ void dfl_rng_words(uint64_t seed, uint32_t stream, uint32_t p, uint32_t v, uint32_t extra,
                                              uint32_t w[4]) {
  w[0] = v >> 2;
  w[1] = p;
  w[2] = extra;
  w[3] = stream;
  dfl_philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__device__ __forceinline__ float dfl_gumbel(uint32_t w) {
  const float u = __fmaf_rn((float)(w >> 9), 0x1p-23f, 0x1p-24f);
  return -logf(-logf(u));
}

// fmaf(bf16 value, invT, Gumbel noise of word w): the quantity the sampled argmax compares
__device__ __forceinline__ float dfl_perturb_w(float vb, float inv_t, uint32_t w) {
  return __fmaf_rn(vb, inv_t, dfl_gumbel(w));
}
