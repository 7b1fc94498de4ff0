// SDR / SI-SDR (this project's own semantics, the reference has no such loss).  Per utterance b,
// estimate row i against target row j, sums over the N samples:
//   a_i = sum e_i^2,  b_j = sum t_j^2,  c_ij = sum e_i t_j
//   scale-invariant: alpha = c / (b + eps), s = alpha c, n = a - s;   plain: s = b, n = a - 2 c + b   (n < 0 -> 0)
//   D = n + tau s + eps,  value = 10 log10((s + eps) / D) dB,  cost = -value / K
// Three kernels: the statistics as chunk partials (one pass over est and tgt), the dB map on the K x K statistics, and
// the backward dest = gout (P e + Q t) with two coefficients per (b, i).  tssep_pit_assign (elementwise.hip) finds the
// assignment on `cost` in between.
//
// Statistics: the shape of pair_cost_partial_kernel -- one workgroup of 256 lanes per (utterance, chunk of SDR_CHUNK
// samples), flat grid, 16-byte loads when every row starts on a 16-byte boundary, scalar loads otherwise, int64
// offsets, a fixed order without atomics.  The noise energy n is a difference of these sums, so float32 is kept only
// where it is cheap: the per-lane chain acc = fma(e, t, acc) of at most SDR_CHUNK / 256 = 32 terms.
// FLOAT32 ROUNDINGS ON THE LONGEST PATH INTO A PARTIAL: SDR_CHUNK / 256 = 32 (one per fused multiply-add; the products
// themselves are exact inside the fma).  Everything behind the lane chain -- the wave tree (6 adds), the four waves
// (2), the stored partials, the chunk loop of sdr_cost_kernel (nchunks - 1) -- is float64.
#include "common.h"

namespace {

constexpr int SDR_CHUNK = 8192;     // samples per workgroup of the statistics pass
constexpr int SDR_SEG = 8192;       // samples of one row per workgroup of the backward
constexpr int SDR_MAX_K = 8;        // tssep_pit_assign's limit

__host__ __device__ constexpr int sdr_nstat(int K) { return K * K + 2 * K; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// part [B][nchunks][K*K + 2K]: c_ij at i*K + j, a_i at K*K + i, b_j at K*K + K + j.  DIAG: only c_ii is accumulated
// (a pit=False loss), the other c entries are written as 0.
template <int K, bool DIAG>
__global__ __launch_bounds__(256) void sdr_stats_partial_kernel(const float* __restrict__ est,
                                                                const float* __restrict__ tgt, int64_t N,
                                                                unsigned nchunks, int vec, double* __restrict__ part) {
  constexpr int NC = DIAG ? K : K * K, NA = NC + 2 * K, NS = sdr_nstat(K);
  __shared__ double red[4][NA];
  const int64_t b = blockIdx.x / nchunks;
  const int64_t n0 = (int64_t)(blockIdx.x - (unsigned)b * nchunks) * SDR_CHUNK;
  const float* __restrict__ e0 = est + b * K * N;
  const float* __restrict__ t0 = tgt + b * K * N;
  float acc[NA];                  // [0, NC): c   [NC, NC + K): a   [NC + K, NA): b
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.f;
  if (vec) {                      // N % 4 == 0 and 16-byte aligned bases: every row starts on a 16-byte boundary
    for (int it = 0; it < SDR_CHUNK / 1024; ++it) {
      const int64_t n = n0 + (int64_t)(it * 256 + (int)threadIdx.x) * 4;
      if (n < N) {
        f32x4 tv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) tv[j] = *reinterpret_cast<const f32x4*>(t0 + j * N + n);
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) acc[NC + K + j] = fmaf(tv[j][q], tv[j][q], acc[NC + K + j]);
#pragma unroll
        for (int i = 0; i < K; ++i) {
          const f32x4 ev = *reinterpret_cast<const f32x4*>(e0 + i * N + n);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            acc[NC + i] = fmaf(ev[q], ev[q], acc[NC + i]);
            if (DIAG) {
              acc[i] = fmaf(ev[q], tv[i][q], acc[i]);
            } else {
#pragma unroll
              for (int j = 0; j < K; ++j) acc[i * K + j] = fmaf(ev[q], tv[j][q], acc[i * K + j]);
            }
          }
        }
      }
    }
  } else {
    for (int it = 0; it < SDR_CHUNK / 256; ++it) {
      const int64_t n = n0 + it * 256 + (int)threadIdx.x;
      if (n < N) {
        float tv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) {
          tv[j] = t0[j * N + n];
          acc[NC + K + j] = fmaf(tv[j], tv[j], acc[NC + K + j]);
        }
#pragma unroll
        for (int i = 0; i < K; ++i) {
          const float ev = e0[i * N + n];
          acc[NC + i] = fmaf(ev, ev, acc[NC + i]);
          if (DIAG) {
            acc[i] = fmaf(ev, tv[i], acc[i]);
          } else {
#pragma unroll
            for (int j = 0; j < K; ++j) acc[i * K + j] = fmaf(ev, tv[j], acc[i * K + j]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const double s = wave_sum_f64((double)acc[a]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][a] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < NS) {
    const int x = threadIdx.x;
    int a = x - K * K + NC;                                     // a_i, b_j
    bool live = true;
    if (x < K * K) {
      const int i = x / K, j = x - i * K;
      a = DIAG ? i : x;
      live = !DIAG || i == j;
    }
    const double s = (red[0][a] + red[1][a]) + (red[2][a] + red[3][a]);
    part[(int64_t)blockIdx.x * NS + x] = live ? s : 0.0;
  }
}

// One workgroup (128 lanes) per utterance: stat[b] = the chunk partials summed in chunk order (float64), then lane
// i*K + j maps (c_ij, a_i, b_j) to value (dB) and cost = -value / K, both formed in float64 and rounded once.
// diag_only: value and cost are 0 off the diagonal (c_ij was not computed there).  `x < 0 ? 0 : x` and not fmax: a NaN
// statistic must reach the value.
template <int K>
__global__ __launch_bounds__(128) void sdr_cost_kernel(const double* __restrict__ part, int nchunks,
                                                       int scale_invariant, double tau, double eps, int diag_only,
                                                       double* __restrict__ stat, float* __restrict__ value,
                                                       float* __restrict__ cost) {
  constexpr int NS = sdr_nstat(K), KK = K * K;
  __shared__ double st[NS];
  const int64_t b = blockIdx.x;
  const int x = threadIdx.x;
  if (x < NS) {
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += part[(b * nchunks + c) * NS + x];
    st[x] = s;
    stat[b * NS + x] = s;
  }
  __syncthreads();
  if (x < KK) {
    const int i = x / K, j = x - i * K;
    double v = 0.0;
    if (!diag_only || i == j) {
      const double c = st[x], a = st[KK + i], bb = st[KK + K + j];
      double s, n;
      if (scale_invariant) {
        s = (c / (bb + eps)) * c;
        n = a - s;
      } else {
        s = bb;
        n = a - 2.0 * c + bb;
      }
      n = n < 0.0 ? 0.0 : n;
      const double D = n + tau * s + eps;
      v = 10.0 * log10((s + eps) / D);
    }
    value[b * KK + x] = (float)v;
    cost[b * KK + x] = (float)(-v / (double)K);
  }
}

// dest[b,i,:] = Pg e_i + Qg t_perm(i):  g = gout[b] 20 / (K ln 10),
//   scale-invariant: P = g / D, Q = -g alpha (1 / (s + eps) + (1 - tau) / D)
//   plain:           P = g / D, Q = -P; both 0 where n was clamped
// One workgroup per (row (b, i), segment of SDR_SEG samples): the coefficients are workgroup-uniform, formed from stat
// in float64 and rounded once (with gout folded in).  Per element: fl(Qg t), then one fused multiply-add.
__global__ __launch_bounds__(256) void sdr_bwd_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                                      const int32_t* __restrict__ perm,
                                                      const double* __restrict__ stat, const float* __restrict__ gout,
                                                      int K, int64_t N, unsigned nseg, int scale_invariant, double tau,
                                                      double eps, int vec, float* __restrict__ dest) {
  const int64_t row = blockIdx.x / nseg;
  const int64_t n0 = (int64_t)(blockIdx.x - (unsigned)row * nseg) * SDR_SEG;
  const int64_t b = row / K;
  const int i = (int)(row - b * K);
  int j = perm ? (int)perm[row] : i;
  if (j < 0 || j >= K) j = i;                   // (a corrupt perm must not turn into a read outside tgt)
  const double* __restrict__ st = stat + b * sdr_nstat(K);
  const double c = st[i * K + j], a = st[K * K + i], bb = st[K * K + K + j];
  const double g = (double)gout[b] * (20.0 / ((double)K * 2.30258509299404568402));
  double P, Q;
  if (scale_invariant) {
    const double alpha = c / (bb + eps), s = alpha * c;
    double n = a - s;
    n = n < 0.0 ? 0.0 : n;
    const double D = n + tau * s + eps;
    P = g / D;
    Q = -g * alpha * (1.0 / (s + eps) + (1.0 - tau) / D);
  } else {
    const double n = a - 2.0 * c + bb;
    const double D = (n < 0.0 ? 0.0 : n) + tau * bb + eps;
    P = n < 0.0 ? 0.0 : g / D;
    Q = -P;
  }
  const float Pf = (float)P, Qf = (float)Q;
  const float* __restrict__ e0 = est + row * N;
  const float* __restrict__ t0 = tgt + (b * K + j) * N;
  float* __restrict__ d0 = dest + row * N;
  if (vec) {
    for (int it = 0; it < SDR_SEG / 1024; ++it) {
      const int64_t n = n0 + (int64_t)(it * 256 + (int)threadIdx.x) * 4;
      if (n < N) {
        const f32x4 ev = *reinterpret_cast<const f32x4*>(e0 + n);
        const f32x4 tv = *reinterpret_cast<const f32x4*>(t0 + n);
        f32x4 o;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = fmaf(Pf, ev[q], Qf * tv[q]);
        *reinterpret_cast<f32x4*>(d0 + n) = o;
      }
    }
  } else {
    for (int it = 0; it < SDR_SEG / 256; ++it) {
      const int64_t n = n0 + it * 256 + (int)threadIdx.x;
      if (n < N) d0[n] = fmaf(Pf, e0[n], Qf * t0[n]);
    }
  }
}

inline bool sdr_shape_ok(int64_t B, int64_t K, int64_t N) {
  if (B <= 0 || K <= 0 || K > SDR_MAX_K || N <= 0) return false;
  const int64_t nchunks = (N + SDR_CHUNK - 1) / SDR_CHUNK, nseg = (N + SDR_SEG - 1) / SDR_SEG;
  return B <= 0x7fffffffLL / nchunks && B * K <= 0x7fffffffLL / nseg;      // the flat grids of both passes
}

template <bool DIAG>
void sdr_stats_launch(int K, unsigned grid, void* stream, const float* est, const float* tgt, int64_t N,
                      unsigned nchunks, int vec, double* part) {
  switch (K) {
#define SDR_CASE(k)                                                                                             \
  case k:                                                                                                       \
    hipLaunchKernelGGL((sdr_stats_partial_kernel<k, DIAG>), dim3(grid), dim3(256), 0, S_, est, tgt, N, nchunks, \
                       vec, part);                                                                              \
    break;
    SDR_CASE(1) SDR_CASE(2) SDR_CASE(3) SDR_CASE(4) SDR_CASE(5) SDR_CASE(6) SDR_CASE(7) SDR_CASE(8)
#undef SDR_CASE
  }
}

}  // namespace

extern "C" int64_t tssep_sdr_chunks(int64_t N) { return N > 0 ? (N + SDR_CHUNK - 1) / SDR_CHUNK : 0; }
extern "C" int64_t tssep_sdr_workspace_bytes(int64_t B, int64_t K, int64_t N) {
  if (!sdr_shape_ok(B, K, N)) return 0;
  return B * tssep_sdr_chunks(N) * sdr_nstat((int)K) * (int64_t)sizeof(double);
}

extern "C" int tssep_sdr_stats_fwd(const float* est, const float* tgt, int64_t B, int64_t K, int64_t N, int diag_only,
                                   double* part, void* stream) {
  if (!est || !tgt || !part) return TSSEP_E_NULL;
  if (!sdr_shape_ok(B, K, N)) return TSSEP_E_SHAPE;
  if (((((uintptr_t)est) | ((uintptr_t)tgt)) & 3u) || (((uintptr_t)part) & 7u)) return TSSEP_E_ALIGN;
  const int64_t nchunks = tssep_sdr_chunks(N);
  const unsigned grid = (unsigned)(B * nchunks);
  const int vec = (N % 4 == 0) && aligned16(est) && aligned16(tgt);
  if (diag_only) sdr_stats_launch<true>((int)K, grid, stream, est, tgt, N, (unsigned)nchunks, vec, part);
  else sdr_stats_launch<false>((int)K, grid, stream, est, tgt, N, (unsigned)nchunks, vec, part);
  return tssep_launch_status();
}

extern "C" int tssep_sdr_cost(const double* part, int64_t B, int64_t K, int64_t nchunks, int scale_invariant,
                              double tau, double eps, int diag_only, double* stat, float* value, float* cost,
                              void* stream) {
  if (!part || !stat || !value || !cost) return TSSEP_E_NULL;
  if (B <= 0 || B > 0x7fffffffLL || K <= 0 || K > SDR_MAX_K || nchunks <= 0 || nchunks > 0x7fffffffLL)
    return TSSEP_E_SHAPE;
  if (!(eps > 0.0) || !(tau >= 0.0)) return TSSEP_E_UNSUPPORTED;
  if ((((uintptr_t)part) | ((uintptr_t)stat)) & 7u) return TSSEP_E_ALIGN;
  switch (K) {
#define SDR_CASE(k)                                                                                            \
  case k:                                                                                                      \
    hipLaunchKernelGGL(sdr_cost_kernel<k>, dim3((unsigned)B), dim3(128), 0, S_, part, (int)nchunks,            \
                       scale_invariant, tau, eps, diag_only, stat, value, cost);                               \
    break;
    SDR_CASE(1) SDR_CASE(2) SDR_CASE(3) SDR_CASE(4) SDR_CASE(5) SDR_CASE(6) SDR_CASE(7) SDR_CASE(8)
#undef SDR_CASE
  }
  return tssep_launch_status();
}

extern "C" int tssep_sdr_bwd(const float* est, const float* tgt, const int32_t* perm, const double* stat,
                             const float* gout, int64_t B, int64_t K, int64_t N, int scale_invariant, double tau,
                             double eps, float* dest, void* stream) {
  if (!est || !tgt || !stat || !gout || !dest) return TSSEP_E_NULL;          // perm may be NULL (identity)
  if (!sdr_shape_ok(B, K, N)) return TSSEP_E_SHAPE;
  if (!(eps > 0.0) || !(tau >= 0.0)) return TSSEP_E_UNSUPPORTED;
  if (((((uintptr_t)est) | ((uintptr_t)tgt) | ((uintptr_t)dest)) & 3u) || (((uintptr_t)stat) & 7u)) return TSSEP_E_ALIGN;
  const int64_t nseg = (N + SDR_SEG - 1) / SDR_SEG;
  const int vec = (N % 4 == 0) && aligned16(est) && aligned16(tgt) && aligned16(dest);
  hipLaunchKernelGGL(sdr_bwd_kernel, dim3((unsigned)(B * K * nseg)), dim3(256), 0, S_, est, tgt, perm, stat, gout,
                     (int)K, N, (unsigned)nseg, scale_invariant, tau, eps, vec, dest);
  return tssep_launch_status();
}
