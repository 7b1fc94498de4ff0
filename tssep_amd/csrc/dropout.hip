// Dropout in front of a Tanh (tssep/train/rnnp.py:98-100, tssep/train/net.py:623-625) as one streaming pass each way:
//   forward   y  = keep ? tanh(z / (1 - p)) : 0            (in place on the projection GEMM's plain store)
//   backward  dz = keep ? dy (1 - y^2) / (1 - p) : 0       (the mask is regenerated, never stored)
// The mask is the counter-based one of dropout_philox.h; seed and draw count come from DEVICE memory (`used`, written by
// tssep_dropout_draw in front of the forward), so a captured hipGraph draws a fresh mask at every replay and the backward
// of a forward finds exactly that forward's mask.  Layouts and launch shapes follow tanh_bwd_*_kernel (elementwise.hip).
#include "gemm_common.h"
#include "dropout_philox.h"

namespace {

using gemm_detail::gemm_tanh;

// state = {seed, draw}: hand this site its own copy and count the draw
__global__ void dropout_draw_kernel(int64_t* __restrict__ state, int64_t* __restrict__ used) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t seed = state[0], draw = state[1];
    used[0] = seed;
    used[1] = draw;
    state[1] = draw + 1;
  }
}

// logical row (b,k,t) -> row of the speaker-combined tensor [B, T, K * P], in units of P
__device__ __forceinline__ int64_t combined_row(int64_t row, int K, int T, int& k) {
  const int64_t bk = row / T;
  const int t = (int)(row - bk * T);
  const int64_t b = bk / K;
  k = (int)(bk - b * K);
  return (b * T + t) * K;
}

// ---- forward ------------------------------------------------------------------------------------------------------
// mode 0: rows of P at leading dimension ld == P (item e IS the address); 1: padded rows; 2: speaker-combined
// (z and y may be the same buffer: no __restrict__ on them; every item reads its 16 bytes before it writes them)
__global__ void dropout_tanh_fwd_v4_kernel(const f32x4* z, f32x4* y, int64_t rows, int P4,
                                           int64_t ld4, int K, int T, int mode, uint64_t thr, float scale,
                                           const int64_t* __restrict__ used) {
  const int64_t seed = used[0], draw = used[1];
  const int64_t total = rows * P4;
  GRID_STRIDE(e, total) {
    int64_t a = e;
    if (mode) {
      const int64_t row = e / P4;
      const int q = (int)(e - row * P4);
      if (mode == 2) {
        int k;
        const int64_t r0 = combined_row(row, K, T, k);
        a = (r0 + k) * P4 + q;
      } else {
        a = row * ld4 + q;
      }
    }
    const f32x4 v = z[a];
    const tssep_philox_out w = tssep_dropout_words(seed, draw, e);      // P % 4 == 0: group e = elements 4e .. 4e + 3
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = tssep_dropout_keep(w.w[i], thr) ? gemm_tanh(v[i] * scale) : 0.0f;
    y[a] = o;
  }
}
__global__ void dropout_tanh_fwd_kernel(const float* z, float* y, int64_t rows, int64_t P,
                                        int64_t ld, int K, int T, int combined, uint64_t thr, float scale,
                                        const int64_t* __restrict__ used) {
  const int64_t seed = used[0], draw = used[1];
  const int64_t total = rows * P;
  GRID_STRIDE(e, total) {
    const int64_t row = e / P, c = e - row * P;
    int64_t a;
    if (combined) {
      int k;
      const int64_t r0 = combined_row(row, K, T, k);
      a = (r0 + k) * P + c;
    } else {
      a = row * ld + c;
    }
    const tssep_philox_out w = tssep_dropout_words(seed, draw, e >> 2);
    y[a] = tssep_dropout_keep(w.w[e & 3], thr) ? gemm_tanh(z[a] * scale) : 0.0f;
  }
}

// ---- backward: dz rows are always (b,k,t) x P, dense; combined != 0: dy and y live in [B,T,K*P] --------------------
__global__ void dropout_tanh_bwd_v4_kernel(const f32x4* __restrict__ dy, const f32x4* __restrict__ y,
                                           f32x4* __restrict__ dz, int64_t rows, int P4, int K, int T, int combined,
                                           uint64_t thr, float scale, const int64_t* __restrict__ used) {
  const int64_t seed = used[0], draw = used[1];
  const int64_t total = rows * P4;
  GRID_STRIDE(e, total) {
    int64_t src = e;
    if (combined) {
      const int64_t row = e / P4;
      const int q = (int)(e - row * P4);
      int k;
      const int64_t r0 = combined_row(row, K, T, k);
      src = (r0 + k) * P4 + q;
    }
    const f32x4 v = y[src], d = __builtin_nontemporal_load(dy + src);
    const tssep_philox_out w = tssep_dropout_words(seed, draw, e);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = tssep_dropout_keep(w.w[i], thr) ? d[i] * (1.0f - v[i] * v[i]) * scale : 0.0f;
    dz[e] = o;
  }
}
__global__ void dropout_tanh_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                        float* __restrict__ dz, int64_t rows, int64_t P, int K, int T, int combined,
                                        uint64_t thr, float scale, const int64_t* __restrict__ used) {
  const int64_t seed = used[0], draw = used[1];
  const int64_t total = rows * P;
  GRID_STRIDE(e, total) {
    int64_t src = e;
    if (combined) {
      const int64_t row = e / P, c = e - row * P;
      int k;
      const int64_t r0 = combined_row(row, K, T, k);
      src = (r0 + k) * P + c;
    }
    const tssep_philox_out w = tssep_dropout_words(seed, draw, e >> 2);
    const float v = y[src];
    dz[e] = tssep_dropout_keep(w.w[e & 3], thr) ? dy[src] * (1.0f - v * v) * scale : 0.0f;
  }
}

inline bool bad_p(double p) { return !(p >= 0.0 && p <= 1.0); }

}  // namespace

extern "C" int tssep_philox4x32_10_host(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  if (!ctr || !key || !out) return TSSEP_E_NULL;
  const tssep_philox_out o = tssep_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = o.w[i];
  return TSSEP_OK;
}
extern "C" int tssep_dropout_keep_host(int64_t seed, int64_t draw, int64_t first, int64_t n, double p, uint8_t* keep) {
  if (!keep) return TSSEP_E_NULL;
  if (first < 0 || n < 0 || bad_p(p)) return TSSEP_E_SHAPE;
  const uint64_t thr = tssep_dropout_threshold(p);
  int64_t group = -1;
  tssep_philox_out w = {};
  for (int64_t i = 0; i < n; ++i) {
    const int64_t e = first + i;
    if ((e >> 2) != group) {
      group = e >> 2;
      w = tssep_dropout_words(seed, draw, group);
    }
    keep[i] = tssep_dropout_keep(w.w[e & 3], thr) ? 1 : 0;
  }
  return TSSEP_OK;
}
extern "C" int tssep_dropout_draw(int64_t* state, int64_t* used, void* stream) {
  if (!state || !used) return TSSEP_E_NULL;
  hipLaunchKernelGGL(dropout_draw_kernel, dim3(1), dim3(64), 0, S_, state, used);
  return tssep_launch_status();
}
extern "C" int tssep_dropout_tanh_fwd(const float* z, float* y, int64_t rows, int64_t P, int64_t ld, int64_t K,
                                      int64_t T, int combined, double p, const int64_t* used, void* stream) {
  if (!z || !y || !used) return TSSEP_E_NULL;
  if (rows <= 0 || P <= 0 || K <= 0 || T <= 0 || bad_p(p)) return TSSEP_E_SHAPE;
  if (combined ? rows % (K * T) != 0 : ld < P) return TSSEP_E_SHAPE;
  const uint64_t thr = tssep_dropout_threshold(p);
  const float scale = tssep_dropout_scale(p);
  if (P % 4 == 0 && (combined || ld % 4 == 0) && aligned16(z) && aligned16(y)) {
    const int mode = combined ? 2 : (ld == P ? 0 : 1);
    hipLaunchKernelGGL(dropout_tanh_fwd_v4_kernel, dim3(grid_for(rows * P / 4)), dim3(256), 0, S_, (const f32x4*)z,
                       (f32x4*)y, rows, (int)(P / 4), ld / 4, (int)K, (int)T, mode, thr, scale, used);
  } else {
    hipLaunchKernelGGL(dropout_tanh_fwd_kernel, dim3(grid_for(rows * P)), dim3(256), 0, S_, z, y, rows, P, ld, (int)K,
                       (int)T, combined, thr, scale, used);
  }
  return tssep_launch_status();
}
extern "C" int tssep_dropout_tanh_bwd(const float* dy, const float* y, float* dz, int64_t rows, int64_t P, int64_t K,
                                      int64_t T, int combined_in, double p, const int64_t* used, void* stream) {
  if (!dy || !y || !dz || !used) return TSSEP_E_NULL;
  if (rows <= 0 || P <= 0 || K <= 0 || T <= 0 || rows % (K * T) || bad_p(p)) return TSSEP_E_SHAPE;
  const uint64_t thr = tssep_dropout_threshold(p);
  const float scale = tssep_dropout_scale(p);
  if (P % 4 == 0 && aligned16(dy) && aligned16(y) && aligned16(dz))
    hipLaunchKernelGGL(dropout_tanh_bwd_v4_kernel, dim3(grid_for(rows * P / 4)), dim3(256), 0, S_, (const f32x4*)dy,
                       (const f32x4*)y, (f32x4*)dz, rows, (int)(P / 4), (int)K, (int)T, combined_in, thr, scale, used);
  else
    hipLaunchKernelGGL(dropout_tanh_bwd_kernel, dim3(grid_for(rows * P)), dim3(256), 0, S_, dy, y, dz, rows, P, (int)K,
                       (int)T, combined_in, thr, scale, used);
  return tssep_launch_status();
}
