// FreqMSE (tssep/train/loss.py:250-269 on STFTDomain, :102-115): the STFT-domain squared error
//   cost[b,i,j] = sum_t (1/F) sum_f |E[b,i,t,f] - S[b,j,t,f]|^2
// as chunk partials of the K x K costs (finished by tssep_pit_assign, elementwise.hip) and its backward.
// Two pairs of entry points: the fused pair forms E = sigmoid(logit) * Observation on the fly (net.py:983 +
// enhancer.py:98-100) and never writes mask or estimate; the generic pair reads an estimate that exists (complex64,
// or complex128 from the differentiable beamformer).
//
// Access pattern: the frame rows of maskhead.hip's gated kernels -- lane l of a wave owns the bins l, l + 64, ... of a
// row, 4-byte loads on the fp32 rows (F = 513: rows are 4-byte aligned only), 8-byte loads on the complex64 rows.
// Forward: one workgroup per (utterance, chunk of SPEC_CT frames); the chunk's (t, f) positions are contiguous in every
// [T, F] plane and are dealt to the 256 lanes (position n0 + tid, + 256, ...), K x K accumulators per lane.
// Reduction: lane chain -> wave tree -> the four waves, a fixed order without atomics (pair_cost_partial_kernel's).
// Float32 roundings on the longest path of a term into part: 1 (m Y_c) + 1 (- t_c) + 2 (the two fused squares) per
// addend, then ceil(SPEC_CT F / 256) lane adds (two fused adds per position) + 6 (wave tree) + 2 (the four waves).
#include "common.h"

namespace {

constexpr int SPEC_CT = 4;          // frames per chunk
constexpr int SPEC_MAX_K = 8;       // tssep_pit_assign's limit

__device__ __forceinline__ float sq_acc(float dr, float di, float acc) { return fmaf(di, di, fmaf(dr, dr, acc)); }

// EST: 0 = fused (the estimate bin is fl(m Y_re), fl(m Y_im) from the logit), 1 = complex64 estimate, 2 = complex128
// estimate (kept in double until the difference)
template <int K, bool DIAG, int EST>
__global__ __launch_bounds__(256) void specmse_partial_kernel(const void* __restrict__ src,
                                                              const float2* __restrict__ obs,
                                                              const float2* __restrict__ tgt, int64_t T, int64_t F,
                                                              unsigned nchunks, float* __restrict__ part) {
#pragma clang fp contract(off)
  constexpr int NA = DIAG ? K : K * K;
  __shared__ float red[4][NA];
  const int64_t b = blockIdx.x / nchunks;
  const int64_t c = (int64_t)blockIdx.x - b * nchunks;
  const int64_t TF = T * F;
  const int64_t t1 = (c + 1) * SPEC_CT < T ? (c + 1) * SPEC_CT : T;
  const int64_t n1 = t1 * F;
  const float2* __restrict__ Y = obs + b * TF;
  const float2* __restrict__ S = tgt + b * K * TF;
  float acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.f;
  for (int64_t n = c * SPEC_CT * F + threadIdx.x; n < n1; n += 256) {
    float2 tv[K];
#pragma unroll
    for (int j = 0; j < K; ++j) tv[j] = S[j * TF + n];
    float2 y = make_float2(0.f, 0.f);
    if (EST == 0) y = Y[n];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const int64_t e = (b * K + i) * TF + n;
      if (EST == 2) {               // differenced in double, the difference rounded to float32 once
        const double2 ev = static_cast<const double2*>(src)[e];
        if (DIAG) {
          acc[i] = sq_acc((float)(ev.x - (double)tv[i].x), (float)(ev.y - (double)tv[i].y), acc[i]);
        } else {
#pragma unroll
          for (int j = 0; j < K; ++j)
            acc[i * K + j] = sq_acc((float)(ev.x - (double)tv[j].x), (float)(ev.y - (double)tv[j].y), acc[i * K + j]);
        }
      } else {
        float2 ev;
        if (EST == 0) {
          const float m = sigmoidf_mask(static_cast<const float*>(src)[e]);
          ev = make_float2(m * y.x, m * y.y);
        } else {
          ev = static_cast<const float2*>(src)[e];
        }
        if (DIAG) {
          acc[i] = sq_acc(ev.x - tv[i].x, ev.y - tv[i].y, acc[i]);
        } else {
#pragma unroll
          for (int j = 0; j < K; ++j) acc[i * K + j] = sq_acc(ev.x - tv[j].x, ev.y - tv[j].y, acc[i * K + j]);
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const float s = wave_sum(acc[a]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][a] = s;
  }
  __syncthreads();
  if (threadIdx.x < K * K) {
    const int i = threadIdx.x / K, j = threadIdx.x - i * K;
    const int a = DIAG ? i : (int)threadIdx.x;
    const float s = (red[0][a] + red[1][a]) + (red[2][a] + red[3][a]);
    part[(int64_t)blockIdx.x * (K * K) + threadIdx.x] = (!DIAG || i == j) ? s : 0.f;
  }
}

// the target row of estimate row (b, k): perm[b, k] (NULL: k); a corrupt entry must not turn into a read outside tgt
__device__ __forceinline__ int64_t matched_row(const int32_t* __restrict__ perm, int64_t b, int64_t K, int64_t k) {
  int64_t j = perm ? (int64_t)perm[b * K + k] : k;
  if (j < 0 || j >= K) j = k;
  return j;
}

// d(logit) = gout[b] (2/F) Re(conj(d) Y) m (1 - m), d = m Y - S[b, perm(k)]: one wave per (b, k, t) frame as
// maskhead_gated_bwd_kernel.  bt_major: the row is stored at (b, t) x (iperm[b, k], f) -- the same values elsewhere.
__global__ __launch_bounds__(256) void mask_specmse_bwd_kernel(
    const float* __restrict__ logit, const float2* __restrict__ obs, const float2* __restrict__ tgt,
    const int32_t* __restrict__ perm, const float* __restrict__ gout, const int32_t* __restrict__ iperm, int bt_major,
    float* __restrict__ dlogit, int64_t frames, int64_t K, int64_t T, int64_t F) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  for (int64_t fr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); fr < frames; fr += nwaves) {
    const int64_t bk = fr / T, t = fr - bk * T;
    const int64_t b = bk / K, k = bk - b * K;
    const int64_t j = matched_row(perm, b, K, k);
    const float* __restrict__ Lr = logit + fr * F;
    const float2* __restrict__ Or = obs + (b * T + t) * F;
    const float2* __restrict__ Sr = tgt + ((b * K + j) * T + t) * F;
    float* Dr = dlogit + fr * F;
    if (bt_major) {
      int64_t kpos = iperm ? (int64_t)iperm[b * K + k] : k;
      if (kpos < 0 || kpos >= K) kpos = k;       // (nor into a store outside dlogit)
      Dr = dlogit + ((b * T + t) * K + kpos) * F;
    }
    const float coef = (2.0f * gout[b]) / (float)F;
    for (int64_t f = lane; f < F; f += 64) {
      const float m = sigmoidf_mask(Lr[f]);
      const float2 y = Or[f], s = Sr[f];
      const float dr = m * y.x - s.x, di = m * y.y - s.y;
      const float dm = dr * y.x + di * y.y;
      const float mm = m * (1.0f - m);
      Dr[f] = (coef * dm) * mm;
    }
  }
}

// d(loss)/d(E) = gout[b] (2/F) (E - S[b, perm(k)]) in the estimate's dtype (torch's complex-gradient convention)
template <typename C2, typename R>
__global__ __launch_bounds__(256) void specmse_bwd_kernel(const C2* __restrict__ est, const float2* __restrict__ tgt,
                                                          const int32_t* __restrict__ perm,
                                                          const float* __restrict__ gout, C2* __restrict__ dest,
                                                          int64_t total, int64_t K, int64_t TF, int64_t F) {
#pragma clang fp contract(off)
  GRID_STRIDE(e, total) {
    const int64_t bk = e / TF, n = e - bk * TF;
    const int64_t b = bk / K, k = bk - b * K;
    const int64_t j = matched_row(perm, b, K, k);
    const R coef = ((R)2 * (R)gout[b]) / (R)F;
    const C2 ev = est[e];
    const float2 s = tgt[(b * K + j) * TF + n];
    C2 o;
    o.x = coef * (ev.x - (R)s.x);
    o.y = coef * (ev.y - (R)s.y);
    dest[e] = o;
  }
}

inline unsigned frame_grid(int64_t frames) {
  const int64_t blocks = (frames + 3) / 4, cap = 256 * 8;
  return (unsigned)(blocks < cap ? (blocks > 0 ? blocks : 1) : cap);
}

inline bool spec_shape_ok(int64_t B, int64_t K, int64_t T, int64_t F) {
  if (B <= 0 || K <= 0 || K > SPEC_MAX_K || T <= 0 || F <= 0) return false;
  const int64_t nchunks = (T + SPEC_CT - 1) / SPEC_CT;
  return B <= 0x7fffffffLL / nchunks;
}

template <bool DIAG, int EST>
void specmse_launch(int K, unsigned grid, void* stream, const void* src, const float2* obs, const float2* tgt,
                    int64_t T, int64_t F, unsigned nchunks, float* part) {
  switch (K) {
#define SP_CASE(k)                                                                                               \
  case k:                                                                                                        \
    hipLaunchKernelGGL((specmse_partial_kernel<k, DIAG, EST>), dim3(grid), dim3(256), 0, S_, src, obs, tgt, T, F, \
                       nchunks, part);                                                                           \
    break;
    SP_CASE(1) SP_CASE(2) SP_CASE(3) SP_CASE(4) SP_CASE(5) SP_CASE(6) SP_CASE(7) SP_CASE(8)
#undef SP_CASE
  }
}

template <int EST>
int specmse_fwd(const void* src, const float* obs, const float* tgt, int64_t B, int64_t K, int64_t T, int64_t F,
                int diag_only, float* part, void* stream) {
  if (!spec_shape_ok(B, K, T, F)) return TSSEP_E_SHAPE;
  const int64_t nchunks = tssep_specmse_chunks(T);
  const unsigned grid = (unsigned)(B * nchunks);
  if (diag_only)
    specmse_launch<true, EST>((int)K, grid, stream, src, (const float2*)obs, (const float2*)tgt, T, F,
                              (unsigned)nchunks, part);
  else
    specmse_launch<false, EST>((int)K, grid, stream, src, (const float2*)obs, (const float2*)tgt, T, F,
                               (unsigned)nchunks, part);
  return tssep_launch_status();
}

}  // namespace

extern "C" int64_t tssep_specmse_chunks(int64_t T) { return T > 0 ? (T + SPEC_CT - 1) / SPEC_CT : 0; }
extern "C" int64_t tssep_specmse_workspace_bytes(int64_t B, int64_t K, int64_t T, int64_t F) {
  if (!spec_shape_ok(B, K, T, F)) return 0;
  const int64_t bytes = B * tssep_specmse_chunks(T) * K * K * (int64_t)sizeof(float);
  return (bytes + 15) / 16 * 16;
}

extern "C" int tssep_mask_specmse_fwd(const float* logit, const float* obs, const float* tgt, int64_t B, int64_t K,
                                      int64_t T, int64_t F, int diag_only, float* part, void* stream) {
  if (!logit || !obs || !tgt || !part) return TSSEP_E_NULL;
  if ((((uintptr_t)logit) & 3u) || (((uintptr_t)obs) & 7u) || (((uintptr_t)tgt) & 7u)) return TSSEP_E_ALIGN;
  return specmse_fwd<0>(logit, obs, tgt, B, K, T, F, diag_only, part, stream);
}

extern "C" int tssep_mask_specmse_bwd(const float* logit, const float* obs, const float* tgt, const int32_t* perm,
                                      const float* gout, int64_t B, int64_t K, int64_t T, int64_t F,
                                      const int32_t* iperm, int bt_major, float* dlogit, void* stream) {
  if (!logit || !obs || !tgt || !gout || !dlogit) return TSSEP_E_NULL;      // perm, iperm may be NULL (identity)
  if (!spec_shape_ok(B, K, T, F)) return TSSEP_E_SHAPE;
  if ((((uintptr_t)logit) & 3u) || (((uintptr_t)obs) & 7u) || (((uintptr_t)tgt) & 7u)) return TSSEP_E_ALIGN;
  hipLaunchKernelGGL(mask_specmse_bwd_kernel, dim3(frame_grid(B * K * T)), dim3(256), 0, S_, logit,
                     (const float2*)obs, (const float2*)tgt, perm, gout, iperm, bt_major, dlogit, B * K * T, K, T, F);
  return tssep_launch_status();
}

extern "C" int tssep_specmse_fwd(const void* est, int est_f64, const float* tgt, int64_t B, int64_t K, int64_t T,
                                 int64_t F, int diag_only, float* part, void* stream) {
  if (!est || !tgt || !part) return TSSEP_E_NULL;
  if ((((uintptr_t)est) & (est_f64 ? 15u : 7u)) || (((uintptr_t)tgt) & 7u)) return TSSEP_E_ALIGN;
  if (est_f64) return specmse_fwd<2>(est, nullptr, tgt, B, K, T, F, diag_only, part, stream);
  return specmse_fwd<1>(est, nullptr, tgt, B, K, T, F, diag_only, part, stream);
}

extern "C" int tssep_specmse_bwd(const void* est, int est_f64, const float* tgt, const int32_t* perm,
                                 const float* gout, int64_t B, int64_t K, int64_t T, int64_t F, void* dest,
                                 void* stream) {
  if (!est || !tgt || !gout || !dest) return TSSEP_E_NULL;                  // perm may be NULL (identity)
  if (!spec_shape_ok(B, K, T, F)) return TSSEP_E_SHAPE;
  if (((((uintptr_t)est) | ((uintptr_t)dest)) & (est_f64 ? 15u : 7u)) || (((uintptr_t)tgt) & 7u)) return TSSEP_E_ALIGN;
  const int64_t TF = T * F, total = B * K * TF;
  if (est_f64)
    hipLaunchKernelGGL((specmse_bwd_kernel<double2, double>), dim3(grid_for(total)), dim3(256), 0, S_,
                       (const double2*)est, (const float2*)tgt, perm, gout, (double2*)dest, total, K, TF, F);
  else
    hipLaunchKernelGGL((specmse_bwd_kernel<float2, float>), dim3(grid_for(total)), dim3(256), 0, S_,
                       (const float2*)est, (const float2*)tgt, perm, gout, (float2*)dest, total, K, TF, F);
  return tssep_launch_status();
}
