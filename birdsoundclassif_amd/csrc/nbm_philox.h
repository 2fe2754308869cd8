// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the dropout keep rule built on it.
// A dropout mask is a pure function of (seed, call, site, element index): nothing is stored, the backward pass evaluates it again.
//   counter (c0, c1, c2, c3) = (q & 0xffffffff, q >> 32, site_id, call), q = element index >> 2; element i takes output word i & 3
//   key (k0, k1)             = low and high half of the 64-bit seed
//   keep iff word >= threshold, threshold = round(p * 2^32)
// ops.dropout_keep_reference (NumPy) is the specification; this header agrees with it bit for bit.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NBM_PHILOX_FN __host__ __device__ inline
#else
#define NBM_PHILOX_FN inline
#endif

NBM_PHILOX_FN void nbm_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                     uint32_t out[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the four mask words of quad q (elements 4q .. 4q + 3) of one dropout site
NBM_PHILOX_FN void nbm_dropout_words(uint64_t seed, uint32_t call, uint32_t site_id, uint64_t q, uint32_t out[4]) {
  nbm_philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), site_id, call, (uint32_t)seed, (uint32_t)(seed >> 32), out);
}

// the mask word of a single element
NBM_PHILOX_FN uint32_t nbm_dropout_word(uint64_t seed, uint32_t call, uint32_t site_id, uint64_t element) {
  uint32_t w[4];
  nbm_dropout_words(seed, call, site_id, element >> 2, w);
  const uint32_t e = (uint32_t)element & 3u;
  return e == 0 ? w[0] : e == 1 ? w[1] : e == 2 ? w[2] : w[3];
}
