// Spectral features without a maximum: AbsSTFT, Log1pAbsSTFT and MVNLog1pAbsSTFT (tssep/train/feature_extractor.py:112-168
// and the padertorch classes it star-imports), and the running-mean form of the last for a live stream (this project's
// own).  Forward only: no parameter precedes the features.
//
//   kind 0   |X|                                         one pass, one element per thread
//   kind 1   L = log1p(|X|)                              one pass, one element per thread
//   kind 2   L - mean over the T frames of L             two passes, one thread per (b, f) walking the frames
//   causal   S = a S + L, n = a n + 1, out = L - S / n   one pass, one thread per (b, f) walking the frames
//
// Every kernel takes |X| and L from the two routines below, so kind 1 IS the L of kind 2 and of the causal call.  The sums
// are float64 chains in frame order, one per (b, f): no atomics, the same bits on every run and under any split of the
// frames into causal calls.  `out` has row pitch ld_out and 4-byte alignment only (the caller may point it into a wider
// buffer): scalar stores, columns [0, F) of each row and nothing else.
#include <math.h>
#include "common.h"

namespace {

constexpr int SPEC_MAXF = 1025;      // as tssep_feat_fwd's documented range
constexpr int PT_PER = 4;            // elements per thread of the one-pass kernel
constexpr int UN = 8;                // frames whose loads are in flight ahead of the chain

// explicit roundings (no contraction): re^2, im^2, their sum, the square root -- the arithmetic tests/specfeat_reference.py
// derives its bound from
__device__ __forceinline__ float spec_abs(float2 x) {
  return sqrtf(__fadd_rn(__fmul_rn(x.x, x.x), __fmul_rn(x.y, x.y)));
}
__device__ __forceinline__ float spec_log1p(float2 x) { return log1pf(spec_abs(x)); }

// kinds 0 and 1: a block takes 256 * PT_PER consecutive elements of the flat [B T F] index; row and bin of the block's
// first element once (64-bit), of each element from there (32-bit: the offset is below 1025 + 1024)
template <int KIND>
__global__ __launch_bounds__(256) void specfeat_point_kernel(const float2* __restrict__ X, int64_t total, int F,
                                                             float* __restrict__ out, int64_t ld_out) {
  const int64_t base = (int64_t)blockIdx.x * (256 * PT_PER);
  const int64_t row0 = base / F;
  const unsigned f0 = (unsigned)(base - row0 * F);
  float2 xv[PT_PER];
#pragma unroll
  for (int k = 0; k < PT_PER; ++k) {
    const int64_t i = base + threadIdx.x + 256 * k;
    xv[k] = i < total ? X[i] : make_float2(0.f, 0.f);
  }
#pragma unroll
  for (int k = 0; k < PT_PER; ++k) {
    const unsigned local = threadIdx.x + 256 * k;
    if (base + local < total) {
      const unsigned g = f0 + local, dr = g / (unsigned)F, f = g - dr * (unsigned)F;
      out[(row0 + dr) * ld_out + f] = KIND == 0 ? spec_abs(xv[k]) : spec_log1p(xv[k]);
    }
  }
}

// one thread per (b, f), f fastest: a wave reads a frame's row coalesced, and the frame loop keeps UN loads in flight (the
// chain depends on the loads, the loads do not depend on the chain).
//   SUM    : S += L over the T frames, mean[b F + f] = S / T                                        (pass 1 of kind 2)
//   CENTER : out = (float)((double)L - mean[b F + f])                                               (pass 2 of kind 2)
//   CAUSAL : S = a S + L, n = a n + 1, out = (float)((double)L - S / n); state [B, F + 1] = {S[b, :], n[b]}
// a S with a = 1 is S itself, so SUM's chain is CAUSAL's at forgetting 1 and kind 2's last frame has the causal call's bits.
enum { SUM = 0, CENTER = 1, CAUSAL = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void specfeat_chain_kernel(const float2* __restrict__ X, int64_t B, int64_t T, int F,
                                                             double alpha, const double* __restrict__ state_in,
                                                             double* __restrict__ state_out, double* __restrict__ mean,
                                                             float* __restrict__ out, int64_t ld_out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * F) return;
  const int64_t b = i / F;
  const int f = (int)(i - b * F);
  const float2* x = X + b * T * F + f;
  float* o = MODE == SUM ? nullptr : out + b * T * ld_out + f;
  double S = 0.0, n = 0.0;
  if (MODE == CAUSAL && state_in) {
    S = state_in[b * (F + 1) + f];
    n = state_in[b * (F + 1) + F];
  }
  const double m = MODE == CENTER ? mean[i] : 0.0;
  auto step = [&](float2 xv, int64_t t) {
    const double L = (double)spec_log1p(xv);
    if (MODE == SUM) {
      S = __dadd_rn(S, L);
    } else if (MODE == CENTER) {
      o[t * ld_out] = (float)__dsub_rn(L, m);
    } else {
      S = __dadd_rn(__dmul_rn(alpha, S), L);
      n = __dadd_rn(__dmul_rn(alpha, n), 1.0);
      o[t * ld_out] = (float)__dsub_rn(L, __ddiv_rn(S, n));
    }
  };
  int64_t t = 0;
  for (; t + UN <= T; t += UN) {
    float2 xv[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) xv[u] = x[(t + u) * F];
#pragma unroll
    for (int u = 0; u < UN; ++u) step(xv[u], t + u);
  }
  for (; t < T; ++t) step(x[t * F], t);
  if (MODE == SUM) mean[i] = __ddiv_rn(S, (double)T);
  if (MODE == CAUSAL && state_out) {
    state_out[b * (F + 1) + f] = S;
    if (f == 0) state_out[b * (F + 1) + F] = n;
  }
}

inline bool spec_shape_ok(int64_t B, int64_t T, int F) {
  // (grids: B F / 256 and B T F / 1024 blocks, both within 2^31 - 1)
  return B > 0 && T > 0 && F > 0 && F <= SPEC_MAXF && B <= (int64_t)0x7fffffff * 256 / SPEC_MAXF &&
         T <= ((int64_t)0x7fffffff * 1024) / (B * F);
}

}  // namespace

extern "C" int64_t tssep_specfeat_workspace_bytes(int64_t B, int64_t T, int F, int kind) {
  if (!spec_shape_ok(B, T, F) || kind != 2) return 0;
  return B * (int64_t)F * 8;
}

extern "C" int tssep_specfeat_fwd(const float* X, int64_t B, int64_t T, int F, int kind, float* out, int64_t ld_out,
                                  void* ws, void* stream) {
  if (!X || !out) return TSSEP_E_NULL;
  if (!spec_shape_ok(B, T, F) || ld_out < F) return TSSEP_E_SHAPE;
  if (kind < 0 || kind > 2) return TSSEP_E_UNSUPPORTED;
  if (kind == 2 && !ws) return TSSEP_E_NULL;
  if ((((uintptr_t)X) & 7u) || (((uintptr_t)out) & 3u) || (kind == 2 && (((uintptr_t)ws) & 7u))) return TSSEP_E_ALIGN;
  const float2* X2 = (const float2*)X;
  if (kind < 2) {
    const int64_t total = B * T * F;
    const unsigned blocks = (unsigned)((total + 256 * PT_PER - 1) / (256 * PT_PER));
    if (kind == 0)
      hipLaunchKernelGGL(specfeat_point_kernel<0>, dim3(blocks), dim3(256), 0, S_, X2, total, F, out, ld_out);
    else
      hipLaunchKernelGGL(specfeat_point_kernel<1>, dim3(blocks), dim3(256), 0, S_, X2, total, F, out, ld_out);
    return tssep_launch_status();
  }
  const unsigned blocks = (unsigned)((B * F + 255) / 256);
  hipLaunchKernelGGL(specfeat_chain_kernel<SUM>, dim3(blocks), dim3(256), 0, S_, X2, B, T, F, 1.0, (const double*)nullptr,
                     (double*)nullptr, (double*)ws, (float*)nullptr, ld_out);
  hipLaunchKernelGGL(specfeat_chain_kernel<CENTER>, dim3(blocks), dim3(256), 0, S_, X2, B, T, F, 1.0, (const double*)nullptr,
                     (double*)nullptr, (double*)ws, out, ld_out);
  return tssep_launch_status();
}

extern "C" int tssep_specfeat_causal_fwd(const float* X, int64_t B, int64_t Tc, int F, double forgetting,
                                         const double* state_in, double* state_out, float* out, int64_t ld_out,
                                         void* stream) {
  if (!X || !out) return TSSEP_E_NULL;
  if (!spec_shape_ok(B, Tc, F) || ld_out < F) return TSSEP_E_SHAPE;
  if (!(forgetting > 0.0 && forgetting <= 1.0)) return TSSEP_E_SHAPE;
  if (state_in && state_out) {      // the new state may not overlap the old one: other threads still read it
    const uintptr_t a = (uintptr_t)state_in, c = (uintptr_t)state_out, bytes = (uintptr_t)(B * (int64_t)(F + 1) * 8);
    if (a < c + bytes && c < a + bytes) return TSSEP_E_SHAPE;
  }
  if ((((uintptr_t)X) & 7u) || (((uintptr_t)out) & 3u) || (((uintptr_t)state_in) & 7u) || (((uintptr_t)state_out) & 7u))
    return TSSEP_E_ALIGN;
  hipLaunchKernelGGL(specfeat_chain_kernel<CAUSAL>, dim3((unsigned)((B * F + 255) / 256)), dim3(256), 0, S_, (const float2*)X,
                     B, Tc, F, forgetting, state_in, state_out, (double*)nullptr, out, ld_out);
  return tssep_launch_status();
}
