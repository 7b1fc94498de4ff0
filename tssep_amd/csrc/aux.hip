// Learned speaker embeddings (tssep/train/net.py:19-158, 250-330, 809-896): the gradient of the speaker conditioning
// with respect to the embedding, instance normalisation, ReLU and the length-aware mean over packed enrolment rows.
// Every kernel streams its operands once (bandwidth-bound), sums in a fixed order (no floating-point
// atomics: two runs are bit-identical) and takes everything it needs from its arguments and device memory.
#include <math.h>
#include <type_traits>
#include "common.h"

namespace {

constexpr int AUX_TCH = 64;      // frames per time chunk of the d_aux partials

// ---- d(conditioning) / d(embedding) ---------------------------------------------------------------------------
// Stage 1.  One workgroup per (b, speaker s, time chunk, tile of 64 lanes): for every trial tr the rows
// (b, tr, (s - tr) mod K, t) of its chunk are T consecutive rows of dxs.  Wave w takes the frames t0 + w, t0 + w + 4, ...
// (four loads in flight per lane), adds them in ascending (trial, frame) order into ONE accumulator per column, and wave
// 0 adds the four waves' sums in ascending wave order.  VEC: a lane owns 4 consecutive columns (16-byte loads), the
// column window [col0, col0 + ncol) starts on a multiple of 4 and may carry pad columns nobody reads afterwards.
template <bool VEC, bool MUL>
__global__ __launch_bounds__(256) void cond_aux_bwd_partial_kernel(
    const float* __restrict__ dxs, int64_t ld_dxs, const float* __restrict__ pre, int64_t ld_pre,
    float* __restrict__ part, int64_t BS, int64_t K, int64_t T, int trials, int col0, int ncol, int ldp, int ntile) {
  constexpr int V = VEC ? 4 : 1;
  __shared__ float red[4][64 * V];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t bs = blockIdx.x / ntile;
  const int tile = (int)(blockIdx.x - bs * ntile);
  const int64_t chunk = blockIdx.y;
  const int j = (tile * 64 + lane) * V;
  const bool active = j < ncol;
  const int64_t b = bs / K;
  const int s = (int)(bs - b * K);
  const int64_t t0 = chunk * AUX_TCH, t1 = (t0 + AUX_TCH < T) ? t0 + AUX_TCH : T;
  float acc[V];
#pragma unroll
  for (int i = 0; i < V; ++i) acc[i] = 0.f;
  const float* p = MUL ? pre + b * T * ld_pre + col0 + j : nullptr;
  for (int tr = 0; tr < trials; ++tr) {
    int k = s - tr;
    if (k < 0) k += (int)K;
    const float* d = dxs + (((b * trials + tr) * K + k) * T) * ld_dxs + col0 + j;
    for (int64_t t = t0 + w; t < t1; t += 16) {
      float dv[4][V], pv[4][V];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t tt = t + 4 * u;
        const bool on = active && tt < t1;
        if (VEC) {
          f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
          if (on) {
            a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d + tt * ld_dxs));
            if (MUL) c = *reinterpret_cast<const f32x4*>(p + tt * ld_pre);
          }
#pragma unroll
          for (int i = 0; i < V; ++i) { dv[u][i] = a[i]; pv[u][i] = c[i]; }
        } else {
          dv[u][0] = on ? __builtin_nontemporal_load(d + tt * ld_dxs) : 0.f;
          pv[u][0] = (on && MUL) ? p[tt * ld_pre] : 0.f;
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] += MUL ? dv[u][i] * pv[u][i] : dv[u][i];
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) red[w][lane * V + i] = acc[i];
  __syncthreads();
  if (w == 0 && active) {
    float* o = part + (chunk * BS + bs) * ldp + j;
#pragma unroll
    for (int i = 0; i < V; ++i)
      o[i] = ((red[0][lane * V + i] + red[1][lane * V + i]) + red[2][lane * V + i]) + red[3][lane * V + i];
  }
}
// Stage 2: the chunks in ascending order.
__global__ void cond_aux_bwd_reduce_kernel(const float* __restrict__ part, int64_t BS, int nchunk, int ldp, int off,
                                           int C, float* __restrict__ d_aux, int64_t ld_out) {
  const int64_t total = BS * C;
  GRID_STRIDE(e, total) {
    const int64_t bs = e / C;
    const int c = (int)(e - bs * C);
    float s = part[bs * ldp + off + c];
    for (int ch = 1; ch < nchunk; ++ch) s += part[((int64_t)ch * BS + bs) * ldp + off + c];
    d_aux[bs * ld_out + c] = s;
  }
}

// ---- d(conditioning) / d(frame-wise embedding) ------------------------------------------------------------------
// aux rows are (b, s, ta); bucket ta holds the frames [ta stride, min((ta + 1) stride, T)): `stride` of them, fewer in the
// last bucket, all T when stride >= T.  One WAVE per (b, s, ta, chunk of AUX_TFR frames of the bucket, tile of 64 lanes):
// it adds the frames of its chunk in ascending (trial, frame) order into one accumulator per column (four loads in
// flight per lane), so nothing is shared between waves.  A bucket of at most AUX_TFR frames is one chunk and goes
// straight to d_aux; longer buckets go to the workspace [chunk][(b, s, ta)][ncol] and cond_aux_bwd_reduce_kernel adds
// the chunks in ascending order.  A chunk behind the end of the last bucket stores zeros.
constexpr int AUX_TFR = 16;
template <bool VEC, bool MUL>
__global__ __launch_bounds__(256) void cond_aux_t_bwd_partial_kernel(
    const float* __restrict__ dxs, int64_t ld_dxs, const float* __restrict__ pre, int64_t ld_pre,
    float* __restrict__ out, int64_t ld_out, int64_t BSA, int64_t K, int64_t T, int trials, int64_t Ta, int64_t stride,
    int64_t nchunk, int64_t units, int col0, int ncol, int ntile, int off, int C) {
  constexpr int V = VEC ? 4 : 1;
  const int lane = threadIdx.x & 63;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (int64_t)gridDim.x * 4) {
    const int64_t q = u / ntile;
    const int tile = (int)(u - q * ntile);
    const int64_t bsa = q / nchunk, chunk = q - bsa * nchunk;
    const int64_t bs = bsa / Ta, ta = bsa - bs * Ta;
    const int64_t b = bs / K;
    const int s = (int)(bs - b * K);
    const int j = (tile * 64 + lane) * V;
    const bool active = j < ncol;
    const int64_t first = ta * stride;                                   // < T
    const int64_t end = stride >= T - first ? T : first + stride;        // (no first + stride past T: no overflow)
    const int64_t t0 = first + chunk * AUX_TFR, t1 = (t0 + AUX_TFR < end) ? t0 + AUX_TFR : end;
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    const float* p = MUL ? pre + b * T * ld_pre + col0 + j : nullptr;
    for (int tr = 0; tr < trials; ++tr) {
      int k = s - tr;
      if (k < 0) k += (int)K;
      const float* d = dxs + (((b * trials + tr) * K + k) * T) * ld_dxs + col0 + j;
      for (int64_t t = t0; t < t1; t += 4) {
        float dv[4][V], pv[4][V];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int64_t tt = t + g;
          const bool on = active && tt < t1;
          if (VEC) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, c = {0.f, 0.f, 0.f, 0.f};
            if (on) {
              a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(d + tt * ld_dxs));
              if (MUL) c = *reinterpret_cast<const f32x4*>(p + tt * ld_pre);
            }
#pragma unroll
            for (int i = 0; i < V; ++i) { dv[g][i] = a[i]; pv[g][i] = c[i]; }
          } else {
            dv[g][0] = on ? __builtin_nontemporal_load(d + tt * ld_dxs) : 0.f;
            pv[g][0] = (on && MUL) ? p[tt * ld_pre] : 0.f;
          }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
          for (int i = 0; i < V; ++i) acc[i] += MUL ? dv[g][i] * pv[g][i] : dv[g][i];
      }
    }
    if (active) {
      float* o = out + (chunk * BSA + bsa) * ld_out;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const int c = j + i - off;
        if (c >= 0 && c < C) o[c] = acc[i];
      }
    }
  }
}

// ---- instance normalisation -----------------------------------------------------------------------------------
// scale of a centred sum of squares over cnt values: InstanceNorm (mode 0): std with cnt - unbiased in the denominator
// (net.py:281-285); InstanceNorm_v2 (mode 1): ||x - mean|| / sqrt(cnt) (net.py:322-330).  No epsilon, as the reference.
__device__ __forceinline__ float instnorm_scale(float ss, int64_t cnt, int mode, int unbiased) {
  return mode == 0 ? sqrtf(ss / (float)(cnt - unbiased)) : sqrtf(ss) / sqrtf((float)cnt);
}
__device__ __forceinline__ float instnorm_dof(int64_t cnt, int mode, int unbiased) {
  return (float)(mode == 0 ? cnt - unbiased : cnt);
}
// The statistics (mean, centred sum of squares, the backward's two sums) are ACCUMULATED in double and rounded to fp32
// once: the data, the stored statistics and every output stay fp32, and the mean's error is one rounding of the mean
// instead of a chain of fp32 additions over values of any magnitude (an element near zero in a row whose mean is near
// zero has an error budget of a few 2^-24 |mean| / std only).  The kernels stay bandwidth-bound.
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// statistics along the last axis: one wave per row; the row is read three times (HBM once, then the caches)
__global__ __launch_bounds__(256) void instnorm_row_fwd_kernel(const float* __restrict__ x, int64_t ld_x,
                                                               float* __restrict__ y, int64_t ld_y,
                                                               float* __restrict__ mean, float* __restrict__ rscale,
                                                               int64_t rows, int C, int mode, int unbiased) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const float* xr = x + row * ld_x;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += (double)xr[c];
    const float m = (float)(wave_sum_f64(s) / (double)C);
    double ss = 0.0;
    for (int c = lane; c < C; c += 64) {
      const float d = xr[c] - m;
      ss += (double)d * (double)d;
    }
    const float sc = instnorm_scale((float)wave_sum_f64(ss), C, mode, unbiased);
    float* yr = y + row * ld_y;
    for (int c = lane; c < C; c += 64) yr[c] = (xr[c] - m) / sc;
    if (lane == 0) {
      mean[row] = m;
      rscale[row] = 1.0f / sc;
    }
  }
}
// dx = r (dy - mean(dy) - yhat sum(dy yhat) / dof), yhat = (x - mean) r
__global__ __launch_bounds__(256) void instnorm_row_bwd_kernel(const float* __restrict__ dy, int64_t ld_dy,
                                                               const float* __restrict__ x, int64_t ld_x,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ rscale, float* __restrict__ dx,
                                                               int64_t ld_dx, int64_t rows, int C, int mode,
                                                               int unbiased) {
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const float* xr = x + row * ld_x;
    const float* gr = dy + row * ld_dy;
    const float m = mean[row], r = rscale[row];
    double sa = 0.0, sb = 0.0;
    for (int c = lane; c < C; c += 64) {
      const float g = gr[c];
      sa += (double)g;
      sb += (double)g * (double)((xr[c] - m) * r);
    }
    const float a = (float)(wave_sum_f64(sa) / (double)C);
    const float b = (float)(wave_sum_f64(sb) / (double)instnorm_dof(C, mode, unbiased));
    float* o = dx + row * ld_dx;
    for (int c = lane; c < C; c += 64) o[c] = r * ((gr[c] - a) - ((xr[c] - m) * r) * b);
  }
}
// Column sums over the n frames of one sequence for a tile of 64 columns: wave w, accumulator u take the frames
// t = w + 4 u (mod 16); the four accumulators, then the four waves, are added in ascending order.  Every thread of the
// workgroup returns the same value for its column.
template <class A, class Fn>
__device__ __forceinline__ A time_sum(A (*red)[64], int64_t n, int lane, int w, bool active, Fn term) {
  A acc[4] = {0, 0, 0, 0};
  for (int64_t t = w; t < n; t += 16) {
    A v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = (active && t + 4 * u < n) ? (A)term(t + 4 * u) : (A)0;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] += v[u];
  }
  __syncthreads();      // (the previous sum's readers are done with red)
  red[w][lane] = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  __syncthreads();
  return ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
}
// statistics along the time axis of x [R, n, C]: one workgroup per (sequence r, tile of 64 columns)
__global__ __launch_bounds__(256) void instnorm_time_fwd_kernel(const float* __restrict__ x, int64_t ld_x,
                                                                float* __restrict__ y, int64_t ld_y,
                                                                float* __restrict__ mean, float* __restrict__ rscale,
                                                                int64_t n, int C, int ntile, int mode, int unbiased) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = blockIdx.x / ntile;
  const int c = (int)(blockIdx.x - r * ntile) * 64 + lane;
  const bool active = c < C;
  const float* xc = x + r * n * ld_x + c;
  const float m = (float)(time_sum(red, n, lane, w, active, [&](int64_t t) { return (double)xc[t * ld_x]; }) / (double)n);
  const double ss = time_sum(red, n, lane, w, active, [&](int64_t t) {
    const float d = xc[t * ld_x] - m;
    return (double)d * (double)d;
  });
  const float sc = instnorm_scale((float)ss, n, mode, unbiased);
  if (!active) return;
  float* yc = y + r * n * ld_y + c;
  for (int64_t t = w; t < n; t += 4) yc[t * ld_y] = (xc[t * ld_x] - m) / sc;
  if (w == 0) {
    mean[r * C + c] = m;
    rscale[r * C + c] = 1.0f / sc;
  }
}
__global__ __launch_bounds__(256) void instnorm_time_bwd_kernel(const float* __restrict__ dy, int64_t ld_dy,
                                                                const float* __restrict__ x, int64_t ld_x,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ rscale, float* __restrict__ dx,
                                                                int64_t ld_dx, int64_t n, int C, int ntile, int mode,
                                                                int unbiased) {
  __shared__ double red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t r = blockIdx.x / ntile;
  const int c = (int)(blockIdx.x - r * ntile) * 64 + lane;
  const bool active = c < C;
  const float* xc = x + r * n * ld_x + c;
  const float* gc = dy + r * n * ld_dy + c;
  const float m = active ? mean[r * C + c] : 0.f, rs = active ? rscale[r * C + c] : 0.f;
  const float a = (float)(time_sum(red, n, lane, w, active, [&](int64_t t) { return (double)gc[t * ld_dy]; }) / (double)n);
  const float b = (float)(time_sum(red, n, lane, w, active, [&](int64_t t) {
    return (double)gc[t * ld_dy] * (double)((xc[t * ld_x] - m) * rs);
  }) / (double)instnorm_dof(n, mode, unbiased));
  if (!active) return;
  float* o = dx + r * n * ld_dx + c;
  for (int64_t t = w; t < n; t += 4) o[t * ld_dx] = rs * ((gc[t * ld_dy] - a) - ((xc[t * ld_x] - m) * rs) * b);
}

// ---- ReLU (net.py:121-123) ------------------------------------------------------------------------------------
// torch.nn.ReLU keeps NaN (fmaxf would return the 0: a NaN in an enrolment activation has to reach the loss, not be trained
// on as a zero), and its gradient is zero where the activation is <= 0, so it passes at a NaN.  Finite inputs: max(v, 0)
// and y > 0, bit for bit.
__device__ __forceinline__ float relu_keep_nan(float v) { return (v > 0.f || v != v) ? v : 0.f; }
__device__ __forceinline__ bool relu_passes(float y) { return !(y <= 0.f); }
__global__ void relu_fwd_kernel(float* __restrict__ y, int64_t ld, int64_t rows, int C) {
  const int64_t total = rows * C;
  GRID_STRIDE(e, total) {
    const int64_t row = e / C;
    float* p = y + row * ld + (e - row * C);
    *p = relu_keep_nan(*p);
  }
}
__global__ void relu_fwd_v4_kernel(f32x4* __restrict__ y, int64_t ldq, int64_t rows, int nq) {
  const int64_t total = rows * nq;
  GRID_STRIDE(e, total) {
    const int64_t row = e / nq;
    f32x4* p = y + row * ldq + (e - row * nq);
    const f32x4 v = *p;
    const f32x4 o = {relu_keep_nan(v[0]), relu_keep_nan(v[1]), relu_keep_nan(v[2]), relu_keep_nan(v[3])};
    *p = o;
  }
}
__global__ void relu_bwd_kernel(const float* __restrict__ dy, int64_t ld_dy, const float* __restrict__ y, int64_t ld_y,
                                float* __restrict__ dx, int64_t ld_dx, int64_t rows, int C) {
  const int64_t total = rows * C;
  GRID_STRIDE(e, total) {
    const int64_t row = e / C, c = e - row * C;
    dx[row * ld_dx + c] = relu_passes(y[row * ld_y + c]) ? dy[row * ld_dy + c] : 0.f;
  }
}
__global__ void relu_bwd_v4_kernel(const f32x4* __restrict__ dy, int64_t ld_dy, const f32x4* __restrict__ y,
                                   int64_t ld_y, f32x4* __restrict__ dx, int64_t ld_dx, int64_t rows, int nq) {
  const int64_t total = rows * nq;
  GRID_STRIDE(e, total) {
    const int64_t row = e / nq, q = e - row * nq;
    const f32x4 g = dy[row * ld_dy + q], v = y[row * ld_y + q];
    const f32x4 o = {relu_passes(v[0]) ? g[0] : 0.f, relu_passes(v[1]) ? g[1] : 0.f, relu_passes(v[2]) ? g[2] : 0.f,
                     relu_passes(v[3]) ? g[3] : 0.f};
    dx[row * ld_dx + q] = o;
  }
}

// ---- length-aware mean over packed rows (padded_sequence_reduction, net.py:147-149, 989-) ------------------------
// one workgroup per (segment s, tile of 64 columns): rows row0[s] .. row0[s+1] - 1, summed like time_sum; the fused ReLU
// and its mask are relu_keep_nan / relu_passes above
__global__ __launch_bounds__(256) void segment_mean_fwd_kernel(const float* __restrict__ h, int64_t ld_h,
                                                               const int64_t* __restrict__ row0,
                                                               float* __restrict__ out, int64_t ld_out, int C,
                                                               int ntile, int relu) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t s = blockIdx.x / ntile;
  const int c = (int)(blockIdx.x - s * ntile) * 64 + lane;
  const bool active = c < C;
  const int64_t r0 = row0[s], n = row0[s + 1] - r0;
  const float* hc = h + r0 * ld_h + c;
  const float sum = time_sum(red, n, lane, w, active, [&](int64_t t) {
    const float v = hc[t * ld_h];
    return relu ? relu_keep_nan(v) : v;
  });
  if (active && w == 0) out[s * ld_out + c] = sum / (float)n;
}
__global__ __launch_bounds__(256) void segment_mean_bwd_kernel(const float* __restrict__ dout, int64_t ld_dout,
                                                               const float* __restrict__ h, int64_t ld_h,
                                                               const int64_t* __restrict__ row0,
                                                               float* __restrict__ dh, int64_t ld_dh, int C, int ntile,
                                                               int relu) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t s = blockIdx.x / ntile;
  const int c = (int)(blockIdx.x - s * ntile) * 64 + lane;
  if (c >= C) return;
  const int64_t r0 = row0[s], n = row0[s + 1] - r0;
  const float g = dout[s * ld_dout + c] / (float)n;
  for (int64_t t = w; t < n; t += 4) {
    const int64_t row = r0 + t;
    dh[row * ld_dh + c] = (!relu || relu_passes(h[row * ld_h + c])) ? g : 0.f;
  }
}

inline int64_t aux_chunks(int64_t T) { return (T + AUX_TCH - 1) / AUX_TCH; }
// column window of dxs the d_aux kernels read with 16-byte loads: [col0, col0 + ncol), both multiples of 4
inline void aux_window(int F, int E, int* col0, int* ncol) {
  const int c0 = E ? F : 0, c1 = E ? F + E : F;
  *col0 = c0 & ~3;
  *ncol = ((c1 + 3) & ~3) - *col0;
}

// launch(V, M) with the integral constants of (vec, mul): the <VEC, MUL> instantiation of a d_aux partial kernel
template <class Fn>
inline void aux_dispatch(bool vec, bool mul, Fn launch) {
  if (vec && mul) launch(std::true_type{}, std::true_type{});
  else if (vec) launch(std::true_type{}, std::false_type{});
  else if (mul) launch(std::false_type{}, std::true_type{});
  else launch(std::false_type{}, std::false_type{});
}

}  // namespace

extern "C" int64_t tssep_cond_aux_bwd_workspace_bytes(int64_t B, int64_t K, int64_t T, int F, int E) {
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || E < 0) return 0;
  int col0, ncol;
  aux_window(F, E, &col0, &ncol);
  return aux_chunks(T) * B * K * (int64_t)ncol * (int64_t)sizeof(float);
}

static int cond_aux_bwd(const float* dxs, int64_t ld_dxs, const float* pre, int64_t ld_pre, float* d_aux,
                        int64_t ld_daux, void* ws, int64_t B, int64_t K, int64_t T, int F, int E, int trials,
                        void* stream) {
  const bool mul = pre != nullptr;
  if (!dxs || !d_aux || !ws) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || E < 0 || trials <= 0 || trials > K) return TSSEP_E_SHAPE;
  const int C = mul ? F : E, W = mul ? F : F + E;
  if (ld_dxs < W || ld_daux < C || (mul && ld_pre < F)) return TSSEP_E_SHAPE;
  const int64_t BS = B * K, nchunk = aux_chunks(T);
  if (nchunk > 65535 || BS * 64 > 0x7fffffffLL) return TSSEP_E_SHAPE;
  int col0, ncol;
  aux_window(F, mul ? 0 : E, &col0, &ncol);
  const int ldp = ncol;
  float* part = (float*)ws;
  const bool vec = (ld_dxs & 3) == 0 && ld_dxs >= col0 + ncol && aligned16(dxs) &&
                   (!mul || ((ld_pre & 3) == 0 && ld_pre >= ncol && aligned16(pre)));
  if (!vec) { col0 = mul ? 0 : F; ncol = C; }
  const int off = (mul ? 0 : F) - col0;      // where column c of d_aux sits in a row of the partials
  const int ntile = ((vec ? ncol / 4 : ncol) + 63) / 64;
  const dim3 grid((unsigned)(BS * ntile), (unsigned)nchunk);
  aux_dispatch(vec, mul, [&](auto V, auto M) {
    hipLaunchKernelGGL((cond_aux_bwd_partial_kernel<decltype(V)::value, decltype(M)::value>), grid, dim3(256), 0, S_,
                       dxs, ld_dxs, pre, ld_pre, part, BS, K, T, trials, col0, ncol, ldp, ntile);
  });
  hipLaunchKernelGGL(cond_aux_bwd_reduce_kernel, dim3(grid_for(BS * C)), dim3(256), 0, S_, part, BS, (int)nchunk, ldp,
                     off, C, d_aux, ld_daux);
  return tssep_launch_status();
}

extern "C" int tssep_cond_mul_aux_bwd(const float* dxs, int64_t ld_dxs, const float* pre, int64_t ld_pre, float* d_aux,
                                      int64_t ld_daux, void* ws, int64_t B, int64_t K, int64_t T, int F, int trials,
                                      void* stream) {
  if (!pre) return TSSEP_E_NULL;
  return cond_aux_bwd(dxs, ld_dxs, pre, ld_pre, d_aux, ld_daux, ws, B, K, T, F, 0, trials, stream);
}
extern "C" int tssep_cond_cat_aux_bwd(const float* dxs, int64_t ld_dxs, float* d_aux, int64_t ld_daux, void* ws,
                                      int64_t B, int64_t K, int64_t T, int F, int E, int trials, void* stream) {
  if (E <= 0) return TSSEP_E_SHAPE;
  return cond_aux_bwd(dxs, ld_dxs, nullptr, 0, d_aux, ld_daux, ws, B, K, T, F, E, trials, stream);
}

// chunks of AUX_TFR frames in the longest bucket
static inline int64_t aux_t_chunks(int64_t T, int64_t stride) {
  return ((stride < T ? stride : T) + AUX_TFR - 1) / AUX_TFR;
}
extern "C" int64_t tssep_cond_aux_t_bwd_workspace_bytes(int64_t B, int64_t K, int64_t T, int F, int E, int64_t Ta,
                                                        int64_t stride) {
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || E < 0 || !cond_t_shape_ok(T, Ta, stride)) return -1;
  const int64_t nchunk = aux_t_chunks(T, stride);
  if (nchunk == 1) return 0;
  int col0, ncol;
  aux_window(F, E, &col0, &ncol);
  return nchunk * B * K * Ta * (int64_t)ncol * (int64_t)sizeof(float);
}

static int cond_aux_t_bwd(const float* dxs, int64_t ld_dxs, const float* pre, int64_t ld_pre, float* d_aux,
                          int64_t ld_daux, void* ws, int64_t B, int64_t K, int64_t T, int F, int E, int trials,
                          int64_t Ta, int64_t stride, void* stream) {
  const bool mul = pre != nullptr;
  if (!dxs || !d_aux) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || E < 0 || trials <= 0 || trials > K || !cond_t_shape_ok(T, Ta, stride))
    return TSSEP_E_SHAPE;
  const int C = mul ? F : E, W = mul ? F : F + E;
  if (ld_dxs < W || ld_daux < C || (mul && ld_pre < F)) return TSSEP_E_SHAPE;
  const int64_t BSA = B * K * Ta, nchunk = aux_t_chunks(T, stride);
  const bool direct = nchunk == 1;
  if (!direct && !ws) return TSSEP_E_NULL;
  int col0, ncol;
  aux_window(F, mul ? 0 : E, &col0, &ncol);
  const bool vec = (ld_dxs & 3) == 0 && ld_dxs >= col0 + ncol && aligned16(dxs) &&
                   (!mul || ((ld_pre & 3) == 0 && ld_pre >= ncol && aligned16(pre)));
  if (!vec) { col0 = mul ? 0 : F; ncol = C; }
  // where column c of d_aux sits in the window: the partials keep the whole window (ldp columns), the reduce picks
  const int off = (mul ? 0 : F) - col0, ldp = vec ? ncol : C;
  const int ntile = ((vec ? ncol / 4 : ncol) + 63) / 64;
  const int64_t units = BSA * nchunk * ntile;
  float* out = direct ? d_aux : (float*)ws;
  const int64_t ld_out = direct ? ld_daux : ldp;
  const int o = direct ? off : 0, c = direct ? C : ncol;
  const dim3 grid(grid_for(units * 64));
  aux_dispatch(vec, mul, [&](auto V, auto M) {
    hipLaunchKernelGGL((cond_aux_t_bwd_partial_kernel<decltype(V)::value, decltype(M)::value>), grid, dim3(256), 0, S_,
                       dxs, ld_dxs, pre, ld_pre, out, ld_out, BSA, K, T, trials, Ta, stride, nchunk, units, col0, ncol,
                       ntile, o, c);
  });
  if (!direct)
    hipLaunchKernelGGL(cond_aux_bwd_reduce_kernel, dim3(grid_for(BSA * C)), dim3(256), 0, S_, (const float*)ws, BSA,
                       (int)nchunk, ldp, off, C, d_aux, ld_daux);
  return tssep_launch_status();
}

extern "C" int tssep_cond_mul_aux_t_bwd(const float* dxs, int64_t ld_dxs, const float* pre, int64_t ld_pre, float* d_aux,
                                        int64_t ld_daux, void* ws, int64_t B, int64_t K, int64_t T, int F, int trials,
                                        int64_t Ta, int64_t stride, void* stream) {
  if (!pre) return TSSEP_E_NULL;
  return cond_aux_t_bwd(dxs, ld_dxs, pre, ld_pre, d_aux, ld_daux, ws, B, K, T, F, 0, trials, Ta, stride, stream);
}
extern "C" int tssep_cond_cat_aux_t_bwd(const float* dxs, int64_t ld_dxs, float* d_aux, int64_t ld_daux, void* ws,
                                        int64_t B, int64_t K, int64_t T, int F, int E, int trials, int64_t Ta,
                                        int64_t stride, void* stream) {
  if (E <= 0) return TSSEP_E_SHAPE;
  return cond_aux_t_bwd(dxs, ld_dxs, nullptr, 0, d_aux, ld_daux, ws, B, K, T, F, E, trials, Ta, stride, stream);
}

static int instnorm_check(int64_t R, int64_t n, int C, int axis, int mode, int unbiased) {
  if (R <= 0 || n <= 0 || C <= 0) return TSSEP_E_SHAPE;
  if ((axis != 0 && axis != 1) || (mode != 0 && mode != 1) || (unbiased != 0 && unbiased != 1))
    return TSSEP_E_UNSUPPORTED;
  if (axis == 1 && R * ((C + 63) / 64) > 0x7fffffffLL) return TSSEP_E_SHAPE;
  return TSSEP_OK;
}
extern "C" int tssep_instnorm_fwd(const float* x, int64_t ld_x, float* y, int64_t ld_y, float* mean, float* rscale,
                                  int64_t R, int64_t n, int C, int axis, int mode, int unbiased, void* stream) {
  if (!x || !y || !mean || !rscale) return TSSEP_E_NULL;
  const int rc = instnorm_check(R, n, C, axis, mode, unbiased);
  if (rc) return rc;
  if (ld_x < C || ld_y < C) return TSSEP_E_SHAPE;
  if (axis == 0) {
    hipLaunchKernelGGL(instnorm_row_fwd_kernel, dim3(grid_for(R * n, 4)), dim3(256), 0, S_, x, ld_x, y, ld_y, mean,
                       rscale, R * n, C, mode, unbiased);
  } else {
    const int ntile = (C + 63) / 64;
    hipLaunchKernelGGL(instnorm_time_fwd_kernel, dim3((unsigned)(R * ntile)), dim3(256), 0, S_, x, ld_x, y, ld_y,
                       mean, rscale, n, C, ntile, mode, unbiased);
  }
  return tssep_launch_status();
}
extern "C" int tssep_instnorm_bwd(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, const float* mean,
                                  const float* rscale, float* dx, int64_t ld_dx, int64_t R, int64_t n, int C, int axis,
                                  int mode, int unbiased, void* stream) {
  if (!dy || !x || !mean || !rscale || !dx) return TSSEP_E_NULL;
  const int rc = instnorm_check(R, n, C, axis, mode, unbiased);
  if (rc) return rc;
  if (ld_x < C || ld_dy < C || ld_dx < C) return TSSEP_E_SHAPE;
  if (axis == 0) {
    hipLaunchKernelGGL(instnorm_row_bwd_kernel, dim3(grid_for(R * n, 4)), dim3(256), 0, S_, dy, ld_dy, x, ld_x, mean,
                       rscale, dx, ld_dx, R * n, C, mode, unbiased);
  } else {
    const int ntile = (C + 63) / 64;
    hipLaunchKernelGGL(instnorm_time_bwd_kernel, dim3((unsigned)(R * ntile)), dim3(256), 0, S_, dy, ld_dy, x, ld_x,
                       mean, rscale, dx, ld_dx, n, C, ntile, mode, unbiased);
  }
  return tssep_launch_status();
}

extern "C" int tssep_relu_fwd(float* y, int64_t ld, int64_t rows, int C, void* stream) {
  if (!y) return TSSEP_E_NULL;
  if (rows <= 0 || C <= 0 || ld < C) return TSSEP_E_SHAPE;
  const int cp = (C + 3) & ~3;
  if ((ld & 3) == 0 && ld >= cp && aligned16(y))
    hipLaunchKernelGGL(relu_fwd_v4_kernel, dim3(grid_for(rows * (cp / 4))), dim3(256), 0, S_, (f32x4*)y, ld / 4, rows,
                       cp / 4);
  else
    hipLaunchKernelGGL(relu_fwd_kernel, dim3(grid_for(rows * C)), dim3(256), 0, S_, y, ld, rows, C);
  return tssep_launch_status();
}
extern "C" int tssep_relu_bwd(const float* dy, int64_t ld_dy, const float* y, int64_t ld_y, float* dx, int64_t ld_dx,
                              int64_t rows, int C, void* stream) {
  if (!dy || !y || !dx) return TSSEP_E_NULL;
  if (rows <= 0 || C <= 0 || ld_dy < C || ld_y < C || ld_dx < C) return TSSEP_E_SHAPE;
  const int cp = (C + 3) & ~3;
  if (((ld_dy | ld_y | ld_dx) & 3) == 0 && ld_dy >= cp && ld_y >= cp && ld_dx >= cp && aligned16(dy) &&
      aligned16(y) && aligned16(dx))
    hipLaunchKernelGGL(relu_bwd_v4_kernel, dim3(grid_for(rows * (cp / 4))), dim3(256), 0, S_, (const f32x4*)dy,
                       ld_dy / 4, (const f32x4*)y, ld_y / 4, (f32x4*)dx, ld_dx / 4, rows, cp / 4);
  else
    hipLaunchKernelGGL(relu_bwd_kernel, dim3(grid_for(rows * C)), dim3(256), 0, S_, dy, ld_dy, y, ld_y, dx, ld_dx,
                       rows, C);
  return tssep_launch_status();
}

extern "C" int tssep_segment_mean_fwd(const float* h, int64_t ld_h, const int64_t* row0, float* out, int64_t ld_out,
                                      int64_t S, int C, int relu, void* stream) {
  if (!h || !row0 || !out) return TSSEP_E_NULL;
  const int ntile = (C + 63) / 64;
  if (S <= 0 || C <= 0 || ld_h < C || ld_out < C || S * ntile > 0x7fffffffLL) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(segment_mean_fwd_kernel, dim3((unsigned)(S * ntile)), dim3(256), 0, S_, h, ld_h, row0, out,
                     ld_out, C, ntile, relu != 0);
  return tssep_launch_status();
}
extern "C" int tssep_segment_mean_bwd(const float* dout, int64_t ld_dout, const float* h, int64_t ld_h,
                                      const int64_t* row0, float* dh, int64_t ld_dh, int64_t S, int C, int relu,
                                      void* stream) {
  if (!dout || !row0 || !dh || (relu && !h)) return TSSEP_E_NULL;
  const int ntile = (C + 63) / 64;
  if (S <= 0 || C <= 0 || ld_dout < C || ld_dh < C || (relu && ld_h < C) || S * ntile > 0x7fffffffLL)
    return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(segment_mean_bwd_kernel, dim3((unsigned)(S * ntile)), dim3(256), 0, S_, dout, ld_dout, h, ld_h,
                     row0, dh, ld_dh, C, ntile, relu != 0);
  return tssep_launch_status();
}
