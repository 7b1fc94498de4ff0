// The dropout mask of libtssep_hip.so: ONE definition, compiled for the host (tssep_dropout_keep_host, the tests'
// reference) and for the device (dropout.hip) from this text, so the two agree bit for bit.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123), multipliers
// 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds.
//   key     = the 64-bit seed {lo, hi}
//   counter = {group lo, group hi, draw lo, draw hi}
//   group   = logical element index / 4; element index = r * P + c for row r = (n, t) of the producing layer and column c
//             of its P outputs -- NOT the address: the padded leading dimension and the speaker-combined layout
//             [B, T, K * P] do not enter
//   draw    = the per-device count of dropout sites run so far (device memory; tssep_dropout_draw)
// Element e takes output word e % 4: 32 random bits per element.
//   keep(e) <=> word >= floor(p * 2^32), compared in 64 bits: p = 0 keeps everything, p = 1 nothing.
// (32 bits per element was kept after the measurement recorded in DESIGN.md 4.7 / profiles/dropout_tail.json.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TSSEP_HD __host__ __device__ __forceinline__
#else
#define TSSEP_HD static inline
#endif

struct tssep_philox_out {
  uint32_t w[4];
};

TSSEP_HD tssep_philox_out tssep_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                              uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  tssep_philox_out o;
  o.w[0] = c0; o.w[1] = c1; o.w[2] = c2; o.w[3] = c3;
  return o;
}

// the four words of one group of four consecutive logical elements
TSSEP_HD tssep_philox_out tssep_dropout_words(int64_t seed, int64_t draw, int64_t group) {
  return tssep_philox4x32_10((uint32_t)(uint64_t)group, (uint32_t)((uint64_t)group >> 32), (uint32_t)(uint64_t)draw,
                             (uint32_t)((uint64_t)draw >> 32), (uint32_t)(uint64_t)seed, (uint32_t)((uint64_t)seed >> 32));
}

// floor(p * 2^32) for p in [0, 1] (exact in double: p * 2^32 only shifts the exponent)
static inline uint64_t tssep_dropout_threshold(double p) { return (uint64_t)(p * 4294967296.0); }
// 1 / (1 - p) in fp32, the factor both directions multiply with (p = 1: nothing is kept, the factor is never used)
static inline float tssep_dropout_scale(double p) { return p < 1.0 ? (float)(1.0 / (1.0 - p)) : 0.0f; }

TSSEP_HD bool tssep_dropout_keep(uint32_t word, uint64_t threshold) { return (uint64_t)word >= threshold; }
