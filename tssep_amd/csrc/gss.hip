// Guided source separation: a complex angular central Gaussian mixture model per (block, frequency bin) with the
// speaker activities as hard priors on the class affiliations; the posteriors are the masks of a mask-based MVDR.
// The definition is this project's own, DESIGN 4.24 (the header states it in full).
//
//   gss_prep_kernel        yh[f,t,:] = y[:,t,f] / |y[:,t,f]|, zeros for a frame that is not ok (norm 0 or not finite):
//                          the one strided pass; every later pass reads a bin's frames as one contiguous run.
//   gss_stats_kernel       grid (bin, block, chunk of GSS_CHUNK frames).  Per tile of 64 frames phase A computes, one
//                          thread per (frame, class), q, log p, gamma and w = gamma / q from the model of the iteration
//                          before (iteration 0: the start values); phase B has one thread per (class, entry of the lower
//                          triangle) -- and one per class for n_c -- that walks the tile's frames in order and adds to
//                          its own accumulator.  The chunk's partial sums go to the workspace.
//   gss_update_kernel      grid (bin, block): the chunk partials summed in chunk order by the entry's owner, the scale,
//                          the trace normalisation and the load, Cholesky, log det, L^-1, log pi: the model.
//   gss_posterior_kernel   phase A once more with the last model; gamma of the block's out range to the output.
//
// Every sum over frames has one owner and one order (frames ascending inside a chunk, chunks ascending): no atomics, no
// wave reductions, the same bits on every call.  With load > 0 and the frames that are not ok skipped, B_c is Hermitian
// positive definite up to rounding: the factorisation has no failing path and nothing is read back by the host.
#include <float.h>
#include "common.h"

namespace {

constexpr int GSS_MAXD = 8, GSS_MAXK = 8, GSS_MAXC = GSS_MAXK + 1;
constexpr int GSS_TILE = 64;              // frames per tile (phase A and phase B meet in LDS)
constexpr int GSS_CHUNK = 256;            // frames per workgroup of the statistics pass: four tiles
constexpr int GSS_THREADS = 256;
constexpr int GSS_MAXENT = GSS_MAXC * (GSS_MAXD * (GSS_MAXD + 1) / 2 + 1);       // 333 accumulators: two per thread
static_assert(GSS_MAXENT <= 2 * GSS_THREADS, "two entries per thread");

struct GssLay {
  int64_t o_yh, o_model, o_part, total;   // bytes
  int64_t nch;                            // chunks per block
  int C, ntri, nent, msz;                 // classes, lower-triangle entries, entries per class (ntri + 1), model doubles
};

__host__ __device__ inline int gss_msz(int D) { return 2 * D * D + 2; }     // L^-1 [D,D] complex | ld | log pi

static bool gss_lay(int P, int D, int K, int64_t T, int F, int64_t max_fit, GssLay& l) {
  if (D < 1 || D > GSS_MAXD || K < 1 || K > GSS_MAXK) return false;
  if (P < 1 || P > 65535 || T < 1 || F < 1 || max_fit < 1 || T > ((int64_t)1 << 30)) return false;
  if (max_fit > T) max_fit = T;
  l.C = K + 1;
  l.ntri = D * (D + 1) / 2;
  l.nent = l.ntri + 1;
  l.msz = gss_msz(D);
  l.nch = (max_fit + GSS_CHUNK - 1) / GSS_CHUNK;
  if (l.nch > 65535) return false;
  const int64_t yh = 16 * (int64_t)D * T * F;
  const int64_t model = 8 * (int64_t)P * F * l.C * l.msz;
  const int64_t part = 16 * (int64_t)P * F * l.nch * l.C * l.nent;
  l.o_yh = 0;
  l.o_model = yh;
  l.o_part = l.o_model + ((model + 15) & ~(int64_t)15);
  l.total = l.o_part + part;
  return l.total < ((int64_t)1 << 40);
}

struct GssBlock { int64_t sf, ef, so, eo; };

// a row of the block table, clamped: 0 <= sf <= so <= eo <= ef <= T and ef - sf <= max_fit
__device__ __forceinline__ GssBlock gss_block(const int32_t* __restrict__ blocks, int p, int64_t T, int64_t max_fit) {
  GssBlock b;
  const int64_t sf = blocks[4 * p], ef = blocks[4 * p + 1], so = blocks[4 * p + 2], eo = blocks[4 * p + 3];
  b.sf = sf < 0 ? 0 : (sf > T ? T : sf);
  b.ef = ef < b.sf ? b.sf : (ef > T ? T : ef);
  if (b.ef - b.sf > max_fit) b.ef = b.sf + max_fit;
  b.so = so < b.sf ? b.sf : (so > b.ef ? b.ef : so);
  b.eo = eo < b.so ? b.so : (eo > b.ef ? b.ef : eo);
  return b;
}

// ------------------------------------------------------------------------------------------------ normalisation
__global__ __launch_bounds__(256) void gss_prep_kernel(const double* __restrict__ obs, double* __restrict__ yh, int D,
                                                       int64_t T, int F) {
  const int64_t n = T * F;
  GRID_STRIDE(i, n) {
    const int64_t t = i / F, f = i - t * F;
    double re[GSS_MAXD], im[GSS_MAXD];
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < GSS_MAXD; ++d) {
      if (d < D) {
        const double* p = obs + 2 * (((int64_t)d * T + t) * F + f);
        re[d] = p[0];
        im[d] = p[1];
        s += re[d] * re[d] + im[d] * im[d];
      }
    }
    const double nrm = sqrt(s);
    const bool ok = nrm > 0.0 && nrm <= DBL_MAX;      // a NaN compares false
    double* o = yh + 2 * ((f * T + t) * D);
#pragma unroll
    for (int d = 0; d < GSS_MAXD; ++d) {
      if (d < D) {
        o[2 * d] = ok ? re[d] / nrm : 0.0;
        o[2 * d + 1] = ok ? im[d] / nrm : 0.0;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ phase A
struct GssTile {
  double model[GSS_MAXC * (2 * GSS_MAXD * GSS_MAXD + 2)];      // 9.4 KB
  double y[GSS_TILE * 2 * GSS_MAXD];                          // 8 KB: yh of the tile, frame-major
  double g[GSS_TILE * GSS_MAXC];                              // log p, then gamma
  double w[GSS_TILE * GSS_MAXC];                              // q, then gamma / q
  double e[GSS_TILE * GSS_MAXC];                              // exp(log p - max)
  unsigned act[GSS_TILE];                                     // bit c: a_tc; bit 31: ok_t
};

// the tile's frames [t0, t0 + nt) of bin f into LDS: yh, the activity bits and ok
__device__ __forceinline__ void gss_load_tile(GssTile& s, const double* __restrict__ yh,
                                              const uint8_t* __restrict__ activity, int64_t f, int64_t t0, int nt,
                                              int D, int K, int64_t T) {
  const double* src = yh + 2 * ((f * T + t0) * D);
  for (int i = threadIdx.x; i < nt * 2 * D; i += GSS_THREADS) s.y[i] = src[i];
  __syncthreads();
  if (threadIdx.x < GSS_TILE) {
    const int t = threadIdx.x;
    unsigned bits = 0;
    if (t < nt) {
      for (int k = 0; k < K; ++k) bits |= (activity[(int64_t)k * T + t0 + t] != 0 ? 1u : 0u) << k;
      bits |= 1u << K;
      double n2 = 0.0;
      for (int d = 0; d < 2 * D; ++d) n2 += s.y[t * 2 * D + d] * s.y[t * 2 * D + d];
      if (n2 > 0.5) bits |= 1u << 31;                          // yh has norm 1, or is all zeros (not ok)
    }
    s.act[t] = bits;
  }
  __syncthreads();
}

// gamma -> s.g and w = gamma / q -> s.w for the tile; START: the start values (gamma = a / sum a, q = 1)
template <bool START>
__device__ __forceinline__ void gss_posterior_tile(GssTile& s, int nt, int D, int C) {
  const int msz = gss_msz(D);
  if (START) {
    for (int i = threadIdx.x; i < nt * C; i += GSS_THREADS) {
      const int t = i / C, c = i - t * C;
      const unsigned bits = s.act[t];
      const bool on = (bits >> 31) && ((bits >> c) & 1u);
      const double v = on ? 1.0 / (double)__popc(bits & 0x1ffu) : 0.0;
      s.g[i] = v;
      s.w[i] = v;
    }
    __syncthreads();
    return;
  }
  for (int i = threadIdx.x; i < nt * C; i += GSS_THREADS) {
    const int t = i / C, c = i - t * C;
    const unsigned bits = s.act[t];
    const double* m = s.model + c * msz;
    const double ld = m[2 * D * D], lpi = m[2 * D * D + 1];
    double q = 1.0, lp = -INFINITY;
    if ((bits >> 31) && ((bits >> c) & 1u) && lpi > -INFINITY) {
      const double* y = s.y + t * 2 * D;
      q = 0.0;
      for (int r = 0; r < D; ++r) {
        double vr = 0.0, vi = 0.0;
        for (int j = 0; j <= r; ++j) {
          const double lr = m[2 * (r * D + j)], li = m[2 * (r * D + j) + 1];
          vr += lr * y[2 * j] - li * y[2 * j + 1];
          vi += lr * y[2 * j + 1] + li * y[2 * j];
        }
        q += vr * vr + vi * vi;
      }
      q = q > DBL_MIN ? q : DBL_MIN;
      lp = lpi - ld - (double)D * log(q);
    }
    s.g[i] = lp;
    s.w[i] = q;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nt * C; i += GSS_THREADS) {
    const int t = i / C;
    double mx = -INFINITY;
    for (int c = 0; c < C; ++c) mx = fmax(mx, s.g[t * C + c]);
    const double lp = s.g[i];
    s.e[i] = (mx > -INFINITY && lp > -INFINITY) ? exp(lp - mx) : 0.0;    // every active class empty: gamma = 0
  }
  __syncthreads();
  for (int i = threadIdx.x; i < nt * C; i += GSS_THREADS) {
    const int t = i / C;
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += s.e[t * C + c];
    const double gam = sum > 0.0 ? s.e[i] / sum : 0.0;
    s.g[i] = gam;
    s.w[i] = gam / s.w[i];
  }
  __syncthreads();
}

__device__ __forceinline__ void gss_load_model(GssTile& s, const double* __restrict__ model, int64_t prob, int D,
                                               int C) {
  const int n = C * gss_msz(D);
  const double* src = model + prob * n;
  for (int i = threadIdx.x; i < n; i += GSS_THREADS) s.model[i] = src[i];
  // (the barrier of gss_load_tile follows before anybody reads)
}

// entry e of a class: (i, j) of the lower triangle row by row, or i = -1: the class's n_c
__device__ __forceinline__ void gss_entry(int e, int ntri, int& i, int& j) {
  if (e >= ntri) { i = -1; j = 0; return; }
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

// ------------------------------------------------------------------------------------------------ statistics
template <bool START>
__global__ __launch_bounds__(GSS_THREADS) void gss_stats_kernel(const double* __restrict__ yh,
                                                                const uint8_t* __restrict__ activity,
                                                                const int32_t* __restrict__ blocks,
                                                                const double* __restrict__ model,
                                                                double* __restrict__ part, int D, int K, int64_t T,
                                                                int F, int64_t max_fit, int64_t nch) {
  __shared__ GssTile s;
  const int64_t f = blockIdx.x;
  const int p = blockIdx.y;
  const int64_t ch = blockIdx.z;
  const GssBlock b = gss_block(blocks, p, T, max_fit);
  const int64_t c0 = b.sf + ch * GSS_CHUNK;
  if (c0 >= b.ef) return;                                     // (the whole workgroup: nobody waits at a barrier)
  const int64_t c1 = c0 + GSS_CHUNK < b.ef ? c0 + GSS_CHUNK : b.ef;
  const int C = K + 1, ntri = D * (D + 1) / 2, nent = ntri + 1;
  const int64_t prob = (int64_t)p * F + f;
  if (!START) gss_load_model(s, model, prob, D, C);

  int ec[2], ei[2], ej[2];
  double ar[2] = {0.0, 0.0}, ai[2] = {0.0, 0.0};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + u * GSS_THREADS;
    ec[u] = e < C * nent ? e / nent : -1;
    gss_entry(e < C * nent ? e - ec[u] * nent : 0, ntri, ei[u], ej[u]);
  }

  for (int64_t t0 = c0; t0 < c1; t0 += GSS_TILE) {
    const int nt = (int)(c1 - t0 < GSS_TILE ? c1 - t0 : GSS_TILE);
    gss_load_tile(s, yh, activity, f, t0, nt, D, K, T);
    gss_posterior_tile<START>(s, nt, D, C);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int c = ec[u];
      if (c < 0) continue;
      if (ei[u] < 0) {
        for (int t = 0; t < nt; ++t) ar[u] += s.g[t * C + c];
      } else {
        const int i = ei[u], j = ej[u];
        for (int t = 0; t < nt; ++t) {
          const double w = s.w[t * C + c];
          const double* y = s.y + t * 2 * D;
          const double yir = y[2 * i], yii = y[2 * i + 1], yjr = y[2 * j], yji = y[2 * j + 1];
          ar[u] += w * (yir * yjr + yii * yji);               // yh_i conj(yh_j)
          ai[u] += w * (yii * yjr - yir * yji);
        }
      }
    }
    __syncthreads();                                          // the tile is read out: the next one may be loaded
  }
  double* dst = part + 2 * ((prob * nch + ch) * (int64_t)(C * nent));
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int e = threadIdx.x + u * GSS_THREADS;
    if (ec[u] >= 0) {
      dst[2 * e] = ar[u];
      dst[2 * e + 1] = ai[u];
    }
  }
}

// ------------------------------------------------------------------------------------------------ model update
__global__ __launch_bounds__(GSS_THREADS) void gss_update_kernel(const int32_t* __restrict__ blocks,
                                                                 const double* __restrict__ part,
                                                                 double* __restrict__ model, int D, int K, int64_t T,
                                                                 int F, int64_t max_fit, int64_t nch, double load,
                                                                 int uniform_weights) {
  __shared__ double sB[GSS_MAXC * 2 * GSS_MAXD * GSS_MAXD];   // B_c, then L_c (lower triangle)
  __shared__ double sM[GSS_MAXC * (2 * GSS_MAXD * GSS_MAXD + 2)];     // the model record: L_c^-1, ld, log pi
  __shared__ double sn[GSS_MAXC];
  const int64_t f = blockIdx.x;
  const int p = blockIdx.y;
  const GssBlock b = gss_block(blocks, p, T, max_fit);
  const int64_t used = (b.ef - b.sf + GSS_CHUNK - 1) / GSS_CHUNK;       // the chunks the statistics pass wrote
  const int C = K + 1, ntri = D * (D + 1) / 2, nent = ntri + 1, msz = gss_msz(D);
  const int64_t prob = (int64_t)p * F + f;
  const double* src = part + 2 * (prob * nch * (int64_t)(C * nent));
  for (int e = threadIdx.x; e < C * nent; e += GSS_THREADS) {
    double ar = 0.0, ai = 0.0;
    for (int64_t ch = 0; ch < used; ++ch) {
      ar += src[2 * (ch * (C * nent) + e)];
      ai += src[2 * (ch * (C * nent) + e) + 1];
    }
    const int c = e / nent;
    int i, j;
    gss_entry(e - c * nent, ntri, i, j);
    if (i < 0) {
      sn[c] = ar;
    } else {
      sB[2 * ((c * D + i) * D + j)] = ar;
      sB[2 * ((c * D + i) * D + j) + 1] = i == j ? 0.0 : ai;
    }
  }
  for (int i = threadIdx.x; i < C * msz; i += GSS_THREADS) sM[i] = 0.0;
  __syncthreads();
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    double* B = sB + 2 * c * D * D;
    double* M = sM + c * msz;
    const double n = sn[c];
    double ntot = 0.0;
    for (int k = 0; k < C; ++k) ntot += sn[k];
    if (!(n > 0.0)) {
      M[2 * D * D] = 0.0;
      M[2 * D * D + 1] = -INFINITY;
    } else {
      const double sc = (double)D / n;
      double tr = 0.0;
      for (int i = 0; i < D; ++i) {
        for (int j = 0; j <= i; ++j) {
          B[2 * (i * D + j)] *= sc;
          B[2 * (i * D + j) + 1] *= sc;
        }
        tr += B[2 * (i * D + i)];
      }
      for (int i = 0; i < D; ++i) {
        for (int j = 0; j <= i; ++j) {                        // (B D) / tr as written: exactly 1 for D = 1
          B[2 * (i * D + j)] = B[2 * (i * D + j)] * (double)D / tr;
          B[2 * (i * D + j) + 1] = B[2 * (i * D + j) + 1] * (double)D / tr;
        }
        B[2 * (i * D + i)] += load;
      }
      // Cholesky, in place on the lower triangle: B = L L^H
      double ld = 0.0;
      for (int j = 0; j < D; ++j) {
        double d = B[2 * (j * D + j)];
        for (int k = 0; k < j; ++k) {
          const double lr = B[2 * (j * D + k)], li = B[2 * (j * D + k) + 1];
          d -= lr * lr + li * li;
        }
        const double ljj = sqrt(d);
        B[2 * (j * D + j)] = ljj;
        ld += log(ljj);
        for (int i = j + 1; i < D; ++i) {
          double xr = B[2 * (i * D + j)], xi = B[2 * (i * D + j) + 1];
          for (int k = 0; k < j; ++k) {
            const double ar = B[2 * (i * D + k)], ai = B[2 * (i * D + k) + 1];
            const double br = B[2 * (j * D + k)], bi = B[2 * (j * D + k) + 1];
            xr -= ar * br + ai * bi;                          // L_ik conj(L_jk)
            xi -= ai * br - ar * bi;
          }
          B[2 * (i * D + j)] = xr / ljj;
          B[2 * (i * D + j) + 1] = xi / ljj;
        }
      }
      // X = L^-1, column by column: X_jj = 1 / L_jj, X_ij = -(sum_{k=j}^{i-1} L_ik X_kj) / L_ii
      for (int j = 0; j < D; ++j) {
        M[2 * (j * D + j)] = 1.0 / B[2 * (j * D + j)];
        for (int i = j + 1; i < D; ++i) {
          double xr = 0.0, xi = 0.0;
          for (int k = j; k < i; ++k) {
            const double ar = B[2 * (i * D + k)], ai = B[2 * (i * D + k) + 1];
            const double br = M[2 * (k * D + j)], bi = M[2 * (k * D + j) + 1];
            xr += ar * br - ai * bi;
            xi += ar * bi + ai * br;
          }
          const double lii = B[2 * (i * D + i)];
          M[2 * (i * D + j)] = -xr / lii;
          M[2 * (i * D + j) + 1] = -xi / lii;
        }
      }
      M[2 * D * D] = 2.0 * ld;
      M[2 * D * D + 1] = uniform_weights ? 0.0 : log(n / ntot);
    }
  }
  __syncthreads();
  double* dst = model + prob * (int64_t)(C * msz);
  for (int i = threadIdx.x; i < C * msz; i += GSS_THREADS) dst[i] = sM[i];
}

// ------------------------------------------------------------------------------------------------ output
template <typename OUT>
__global__ __launch_bounds__(GSS_THREADS) void gss_posterior_kernel(const double* __restrict__ yh,
                                                                    const uint8_t* __restrict__ activity,
                                                                    const int32_t* __restrict__ blocks,
                                                                    const double* __restrict__ model,
                                                                    OUT* __restrict__ out, int D, int K, int64_t T,
                                                                    int F, int64_t max_fit) {
  __shared__ GssTile s;
  const int64_t f = blockIdx.x;
  const int p = blockIdx.y;
  const int64_t ch = blockIdx.z;
  const GssBlock b = gss_block(blocks, p, T, max_fit);
  const int64_t c0 = b.so + ch * GSS_CHUNK;
  if (c0 >= b.eo) return;
  const int64_t c1 = c0 + GSS_CHUNK < b.eo ? c0 + GSS_CHUNK : b.eo;
  const int C = K + 1;
  gss_load_model(s, model, (int64_t)p * F + f, D, C);
  for (int64_t t0 = c0; t0 < c1; t0 += GSS_TILE) {
    const int nt = (int)(c1 - t0 < GSS_TILE ? c1 - t0 : GSS_TILE);
    gss_load_tile(s, yh, activity, f, t0, nt, D, K, T);
    gss_posterior_tile<false>(s, nt, D, C);
    for (int i = threadIdx.x; i < nt * C; i += GSS_THREADS) {
      const int c = i / nt, t = i - c * nt;
      out[((int64_t)c * T + t0 + t) * F + f] = (OUT)s.g[t * C + c];
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ table -> activity
// one workgroup per row (strided over the rows beyond the grid): every frame of the row gets a 1.  Rows may overlap:
// all writers store the same byte.
__global__ __launch_bounds__(256) void seg_activity_kernel(const int32_t* __restrict__ table, int64_t S, int K,
                                                           int64_t T, uint8_t* __restrict__ act) {
  for (int64_t r = blockIdx.x; r < S; r += gridDim.x) {
    const int64_t k = table[3 * r], s0 = table[3 * r + 1], e0 = table[3 * r + 2];
    if (k < 0 || k >= K || s0 < 0 || e0 > T || s0 >= e0) continue;
    for (int64_t t = s0 + threadIdx.x; t < e0; t += blockDim.x) act[k * T + t] = 1;
  }
}

}  // namespace

extern "C" int64_t tssep_gss_workspace_bytes(int P, int D, int K, int64_t T, int F, int64_t max_fit) {
  GssLay l;
  return gss_lay(P, D, K, T, F, max_fit, l) ? l.total : 0;
}

extern "C" int tssep_gss_fit(const double* obs, const uint8_t* activity, const int32_t* blocks, void* out, int out_f64,
                             void* workspace, int P, int D, int K, int64_t T, int F, int64_t max_fit, int iterations,
                             double load, int uniform_weights, void* stream) {
  if (!obs || !activity || !blocks || !out || !workspace) return TSSEP_E_NULL;
  if (D < 1 || D > GSS_MAXD || K < 1 || K > GSS_MAXK) return TSSEP_E_UNSUPPORTED;
  if (!(load > 0.0) || !(load <= DBL_MAX) || iterations < 1) return TSSEP_E_SHAPE;
  GssLay l;
  if (!gss_lay(P, D, K, T, F, max_fit, l)) return TSSEP_E_SHAPE;
  if (!aligned16(obs) || !aligned16(workspace) || (((uintptr_t)out) & 7u) || (((uintptr_t)blocks) & 3u))
    return TSSEP_E_ALIGN;
  if (max_fit > T) max_fit = T;
  char* ws = static_cast<char*>(workspace);
  double* yh = reinterpret_cast<double*>(ws + l.o_yh);
  double* model = reinterpret_cast<double*>(ws + l.o_model);
  double* part = reinterpret_cast<double*>(ws + l.o_part);
  const dim3 blk(GSS_THREADS), gs((unsigned)F, (unsigned)P, (unsigned)l.nch), gu((unsigned)F, (unsigned)P);
  hipLaunchKernelGGL(gss_prep_kernel, dim3(grid_for(T * (int64_t)F, 256, 1 << 16)), dim3(256), 0, S_, obs, yh, D, T, F);
  for (int it = 0; it < iterations; ++it) {
    if (it == 0)
      hipLaunchKernelGGL(gss_stats_kernel<true>, gs, blk, 0, S_, yh, activity, blocks, model, part, D, K, T, F, max_fit,
                         l.nch);
    else
      hipLaunchKernelGGL(gss_stats_kernel<false>, gs, blk, 0, S_, yh, activity, blocks, model, part, D, K, T, F,
                         max_fit, l.nch);
    hipLaunchKernelGGL(gss_update_kernel, gu, blk, 0, S_, blocks, part, model, D, K, T, F, max_fit, l.nch, load,
                       uniform_weights);
  }
  if (out_f64)
    hipLaunchKernelGGL(gss_posterior_kernel<double>, gs, blk, 0, S_, yh, activity, blocks, model, (double*)out, D, K,
                       T, F, max_fit);
  else
    hipLaunchKernelGGL(gss_posterior_kernel<float>, gs, blk, 0, S_, yh, activity, blocks, model, (float*)out, D, K, T,
                       F, max_fit);
  return tssep_launch_status();
}

extern "C" int tssep_segments_to_activity(const int32_t* table, int64_t S, int K, int64_t T, uint8_t* activity,
                                          void* stream) {
  if (!activity || (S > 0 && !table)) return TSSEP_E_NULL;
  if (S < 0 || K < 1 || T < 1 || T > ((int64_t)1 << 30) || K > 65535) return TSSEP_E_SHAPE;
  if (S > 0 && (((uintptr_t)table) & 3u)) return TSSEP_E_ALIGN;
  if (hipMemsetAsync(activity, 0, (size_t)K * (size_t)T, S_) != hipSuccess) return TSSEP_E_LAUNCH;
  if (S > 0)
    hipLaunchKernelGGL(seg_activity_kernel, dim3(grid_for(S, 1, 4096)), dim3(256), 0, S_, table, S, K, T, activity);
  return tssep_launch_status();
}
