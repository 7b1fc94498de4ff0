// WPE dereverberation in complex128 -- WPE / ChannelWiseWPE of the reference (tssep/train/enhancer.py:292-367), which
// runs nara_wpe's wpe_v8 on the host.  Per frequency bin, Y [D, T], K = taps * D:
//   Yt[tau*D + d, t] = Y[d, t - delay - tau]          (zero in front of the segment's first frame)
//   X = Y;  `iterations` times:
//     p[t]   = mean_d |X[d,t]|^2,   eps = 1e-10 max_t p[t],   li[t] = 1 / max(p[t], eps)
//     R = sum_t li[t] Yt[:,t] Yt[:,t]^H     P = sum_t li[t] Yt[:,t] Y[:,t]^H      (t over the statistics range)
//     R G = P                                X = Y - G^H Yt
// All stages run over a segment table (rows (s, e), packed output rows row0[i] .. row0[i+1]), so one set of launches
// serves the whole observation (one row (0, T)) and the segment-wise use; every row is computed as if its slice were
// the whole array: chunks and blocks are laid out from the row's own first frame, so the summation order of a row
// depends on nothing but its length.
//   wpe_prep_kernel        prefix sums of the rows' chunk counts (correlation chunks of TCHUNK frames, blocks of FBLK)
//   wpe_power_kernel       lane = bin: p into the li buffer, per (row, bin) maximum by an atomic max on the bit pattern
//   wpe_lambda_kernel      li = 1 / max(p, 1e-10 pmax), in place
//   wpe_corr_kernel        one workgroup per (chunk, bin): thread = one 4 x 4 complex tile of the lower tile triangle
//                          of R or of P, operands from an LDS window of Y frames, fp64 vector FMAs
//   wpe_reduce_kernel      chunk partials -> full R (both triangles, real diagonal) and P, chunks in ascending order
//   wpe_solve_kernel       one workgroup per (row, bin): Cholesky R = L L^H in LDS with P eliminated alongside, then
//                          L^H G = W;  a pivot that is not positive and finite counts in info[row]
//   wpe_filter_kernel<D>   lane = bin, 4 frames per lane in registers: X = Y - G^H Yt into the packed output
// No access leaves the buffers whatever the table holds: rows are clamped to [0, T], packed indices are checked
// against N.
#include <atomic>

#include "common.h"

namespace {

constexpr int WMAXD = 8;
constexpr int WMAXK = 80;
constexpr int WMAXDELAY = 256;
constexpr int TCHUNK = 256;      // frames per correlation chunk (tests restate it: WPE_TCHUNK)
constexpr int TSUB = 32;         // frames per LDS window step
constexpr int FBLK = 64;         // frames per power / filter workgroup (4 waves x 16)
constexpr int TB = 4;            // frames per lane in the filter

struct Lay {
  int K, M, PB, tilesR, ntiles;
  int64_t gmax, fmax;
  int64_t o_cstart, o_fstart, o_pmax, o_lam, o_part, o_R, o_P, o_G, total;
};
__host__ int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }
__host__ bool wpe_shape_ok(int S, int64_t N, int D, int64_t T, int F, int taps, int delay) {
  return S > 0 && S <= (1 << 20) && N > 0 && T > 0 && F > 0 && D >= 1 && D <= WMAXD && taps >= 1 &&
         (int64_t)taps * D <= WMAXK && delay >= 0 && delay <= WMAXDELAY && T < ((int64_t)1 << 30) &&
         N < ((int64_t)1 << 30) && (N / FBLK + S) * ((F + 63) / 64) < ((int64_t)1 << 30) &&
         (N / TCHUNK + S) * (int64_t)F < ((int64_t)1 << 30) && (int64_t)S * F < ((int64_t)1 << 30) &&
         (int64_t)S * F * ((int64_t)taps * D * (taps * D + D)) < ((int64_t)1 << 38);
}
__host__ Lay make_lay(int S, int64_t N, int D, int F, int taps) {
  Lay l;
  l.K = taps * D;
  l.M = (l.K + 3) / 4;
  l.PB = (D + 3) / 4;
  l.tilesR = l.M * (l.M + 1) / 2;
  l.ntiles = l.tilesR + l.M * l.PB;
  l.gmax = N / TCHUNK + S;
  l.fmax = N / FBLK + S;
  int64_t o = 0;
  l.o_cstart = o; o += up16((int64_t)(S + 1) * 4);
  l.o_fstart = o; o += up16((int64_t)(S + 1) * 4);
  l.o_pmax = o;   o += up16((int64_t)S * F * 8);
  l.o_lam = o;    o += up16(N * F * 8);
  l.o_part = o;   o += l.gmax * F * l.ntiles * 256;
  l.o_R = o;      o += (int64_t)S * F * l.K * l.K * 16;
  l.o_P = o;      o += (int64_t)S * F * l.K * D * 16;
  l.o_G = o;      o += (int64_t)S * l.K * D * F * 16;
  l.total = o;
  return l;
}

struct Row { int s, e; };
__device__ __forceinline__ Row load_row(const int32_t* __restrict__ tab, int i, int64_t T) {
  Row g{tab[2 * i], tab[2 * i + 1]};
  if (g.s < 0) g.s = 0;
  if (g.e > (int)T) g.e = (int)T;
  if (g.e < g.s) g.e = g.s;
  return g;
}
// the row whose blocks hold block `g` of the prefix `start` [S + 1]; -1 past the end
__device__ __forceinline__ int locate(const int32_t* __restrict__ start, int S, int g) {
  if (g >= start[S]) return -1;
  int lo = 0, hi = S;                     // start[lo] <= g < start[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void wpe_prep_kernel(const int32_t* __restrict__ tab, int32_t* __restrict__ cstart,
                                int32_t* __restrict__ fstart, int S, int64_t T, int64_t gmax, int64_t fmax) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t c = 0, b = 0;
  for (int i = 0; i < S; ++i) {
    cstart[i] = (int32_t)c;
    fstart[i] = (int32_t)b;
    const Row g = load_row(tab, i, T);
    const int len = g.e - g.s;
    c += (len + TCHUNK - 1) / TCHUNK;
    b += (len + FBLK - 1) / FBLK;
    if (c > gmax) c = gmax;               // a table longer than the packed buffer: the tail gets no blocks
    if (b > fmax) b = fmax;
  }
  cstart[S] = (int32_t)c;
  fstart[S] = (int32_t)b;
}

// ---------------------------------------------------------------------------------- power ----
__device__ __forceinline__ unsigned long long power_key(double p) {
  // non-negative doubles order like their bit patterns; NaN takes the largest key and comes back as NaN
  return p != p ? 0x7ff8000000000000ull : (unsigned long long)__double_as_longlong(p);
}

__global__ __launch_bounds__(256) void wpe_power_kernel(
    const double2* __restrict__ obs, const double2* __restrict__ xs, const int32_t* __restrict__ tab,
    const int64_t* __restrict__ row0, const int32_t* __restrict__ fstart, double* __restrict__ lam,
    unsigned long long* __restrict__ pmax, int S, int64_t N, int D, int64_t T, int F, int nf) {
  const int ft = blockIdx.x % nf;
  const int g = blockIdx.x / nf;
  const int sg = locate(fstart, S, g);
  if (sg < 0) return;
  const Row r = load_row(tab, sg, T);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = ft * 64 + lane;
  if (f >= F) return;
  const int t0 = r.s + (g - fstart[sg]) * FBLK + wave * (FBLK / 4);
  const int t1 = t0 + FBLK / 4 < r.e ? t0 + FBLK / 4 : r.e;
  const int64_t n0 = row0[sg];
  double best = 0.0;
  bool nan = false;
  for (int t = t0; t < t1; ++t) {
    const int64_t n = n0 + (t - r.s);
    if (n < 0 || n >= N) continue;
    double p = 0.0;
    for (int d = 0; d < D; ++d) {
      const double2 x = xs ? xs[((int64_t)d * N + n) * F + f] : obs[((int64_t)d * T + t) * F + f];
      p += x.x * x.x + x.y * x.y;
    }
    p /= (double)D;
    lam[n * F + f] = p;
    if (p != p) nan = true;
    best = p > best ? p : best;
  }
  if (t1 > t0) atomicMax(pmax + (int64_t)sg * F + f, power_key(nan ? __longlong_as_double(0x7ff8000000000000ll) : best));
}

__global__ __launch_bounds__(256) void wpe_lambda_kernel(
    const int32_t* __restrict__ tab, const int64_t* __restrict__ row0, const int32_t* __restrict__ fstart,
    double* __restrict__ lam, const unsigned long long* __restrict__ pmax, int S, int64_t N, int64_t T, int F,
    int nf) {
  const int ft = blockIdx.x % nf;
  const int g = blockIdx.x / nf;
  const int sg = locate(fstart, S, g);
  if (sg < 0) return;
  const Row r = load_row(tab, sg, T);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = ft * 64 + lane;
  if (f >= F) return;
  const int t0 = r.s + (g - fstart[sg]) * FBLK + wave * (FBLK / 4);
  const int t1 = t0 + FBLK / 4 < r.e ? t0 + FBLK / 4 : r.e;
  const int64_t n0 = row0[sg];
  const double eps = 1e-10 * __longlong_as_double((long long)pmax[(int64_t)sg * F + f]);
  for (int t = t0; t < t1; ++t) {
    const int64_t n = n0 + (t - r.s);
    if (n < 0 || n >= N) continue;
    const double p = lam[n * F + f];
    lam[n * F + f] = 1.0 / (p > eps ? p : eps);       // np.maximum: a NaN on either side gives NaN
  }
}

// --------------------------------------------------------------------------- correlations ----
struct TileId { int isP, bi, bj; };
__device__ __forceinline__ TileId tile_of(int q, int tilesR, int PB) {
  TileId t;
  if (q < tilesR) {
    int bi = 0;
    while ((bi + 1) * (bi + 2) / 2 <= q) ++bi;
    t.isP = 0; t.bi = bi; t.bj = q - bi * (bi + 1) / 2;
  } else {
    t.isP = 1; t.bi = (q - tilesR) / PB; t.bj = (q - tilesR) % PB;
  }
  return t;
}

__global__ __launch_bounds__(256) void wpe_corr_kernel(
    const double2* __restrict__ obs, const double* __restrict__ lam, const int32_t* __restrict__ tab,
    const int64_t* __restrict__ row0, const int32_t* __restrict__ cstart, double2* __restrict__ part, int S,
    int64_t N, int D, int64_t T, int F, int taps, int delay, int valid, int ntiles, int tilesR, int PB,
    int64_t per_xcd, int64_t nblocks) {
  extern __shared__ double2 win[];                       // [W frames][D], then TSUB weights
  // consecutive (chunk, bin) on ONE XCD: block ids go round-robin over the 8 XCDs, and the eight bins of a 128-byte
  // line of Y should meet in one L2
  const int64_t L = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if ((int64_t)(blockIdx.x >> 3) >= per_xcd || L >= nblocks) return;
  const int g = (int)(L / F), f = (int)(L % F);
  const int sg = locate(cstart, S, g);
  if (sg < 0) return;
  const Row r = load_row(tab, sg, T);
  const int K = taps * D;
  const int hist = delay + taps - 1;
  const int W = TSUB + hist;
  double* lamw = reinterpret_cast<double*>(win + (size_t)W * D);
  const int tid = threadIdx.x;
  const int t0 = r.s + (g - cstart[sg]) * TCHUNK;
  const int t1 = t0 + TCHUNK < r.e ? t0 + TCHUNK : r.e;
  const int vstart = valid ? r.s + hist : r.s;
  const int64_t n0 = row0[sg];

  const bool active = tid < ntiles;
  const TileId tl = tile_of(active ? tid : 0, tilesR, PB);
  int roff[4], coff[4];
  bool rok[4], cok[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = 4 * tl.bi + q;
    rok[q] = i < K;
    roff[q] = rok[q] ? (taps - 1 - i / D) * D + i % D : 0;
    const int j = 4 * tl.bj + q;
    if (tl.isP) {
      cok[q] = j < D;
      coff[q] = cok[q] ? hist * D + j : 0;
    } else {
      cok[q] = j < K;
      coff[q] = cok[q] ? (taps - 1 - j / D) * D + j % D : 0;
    }
  }
  double2 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = double2{0.0, 0.0};

  for (int ts = t0; ts < t1; ts += TSUB) {
    __syncthreads();
    const int wb = ts - hist;
    for (int idx = tid; idx < W * D; idx += 256) {
      const int fr = idx / D, d = idx - fr * D;
      const int u = wb + fr;
      // frames in front of the row's first one are zero (the reference slices before it calls WPE); never loaded
      win[idx] = (u >= r.s && u < t1) ? obs[((int64_t)d * T + u) * F + f] : double2{0.0, 0.0};
    }
    if (tid < TSUB) {
      const int t = ts + tid;
      const int64_t n = n0 + (t - r.s);
      lamw[tid] = (t < t1 && n >= 0 && n < N) ? lam[n * F + f] : 0.0;
    }
    __syncthreads();
    if (!active) continue;
    const int lo = vstart > ts ? vstart - ts : 0;
    const int hi = t1 - ts < TSUB ? t1 - ts : TSUB;
    for (int q = lo; q < hi; ++q) {
      const double w = lamw[q];
      const double2* fr = win + q * D;
      double2 a[4], b[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const double2 v = fr[roff[x]];
        a[x] = double2{rok[x] ? w * v.x : 0.0, rok[x] ? w * v.y : 0.0};
        const double2 u = fr[coff[x]];
        b[x] = double2{cok[x] ? u.x : 0.0, cok[x] ? u.y : 0.0};
      }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
          acc[x][y].x += a[x].x * b[y].x + a[x].y * b[y].y;      // (w a) conj(b)
          acc[x][y].y += a[x].y * b[y].x - a[x].x * b[y].y;
        }
    }
  }
  if (!active) return;
  double2* out = part + (((int64_t)g * F + f) * ntiles + tid) * 16;
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) out[x * 4 + y] = acc[x][y];
}

// chunk partials -> R [S][F][K][K] (full, Hermitian by construction, real diagonal) and P [S][F][K][D]
__global__ __launch_bounds__(256) void wpe_reduce_kernel(
    const double2* __restrict__ part, const int32_t* __restrict__ cstart, double2* __restrict__ R,
    double2* __restrict__ P, int S, int D, int F, int K, int ntiles, int tilesR, int PB, int64_t gmax) {
  const int E = K * K + K * D;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)S * F * E) return;
  const int el = (int)(i % E);
  const int64_t sf = i / E;
  const int f = (int)(sf % F), sg = (int)(sf / F);
  int tile, pos;
  bool conj = false, diag = false;
  if (el < K * K) {
    int a = el / K, b = el % K;
    diag = a == b;
    if (a < b) { const int t = a; a = b; b = t; conj = true; }
    tile = (a / 4) * (a / 4 + 1) / 2 + b / 4;
    pos = (a % 4) * 4 + b % 4;
  } else {
    const int a = (el - K * K) / D, b = (el - K * K) % D;
    tile = tilesR + (a / 4) * PB + b / 4;
    pos = (a % 4) * 4 + b % 4;
  }
  double2 s = {0.0, 0.0};
  const int c0 = cstart[sg], c1 = cstart[sg + 1];
  for (int c = c0; c < c1 && c < gmax; ++c) {
    const double2 v = part[(((int64_t)c * F + f) * ntiles + tile) * 16 + pos];
    s.x += v.x;
    s.y += v.y;
  }
  if (conj) s.y = -s.y;
  if (diag) s.y = 0.0;
  if (el < K * K) R[sf * K * K + el] = s;
  else P[sf * K * D + (el - K * K)] = s;
}

// ---------------------------------------------------------------------------------- solve ----
__global__ __launch_bounds__(256) void wpe_solve_kernel(const double2* __restrict__ R,
                                                        const double2* __restrict__ P,
                                                        double2* __restrict__ G, int* __restrict__ info, int D,
                                                        int F, int K) {
  extern __shared__ double2 sm[];
  double2* A = sm;               // [K][K], lower triangle -> L (the diagonal keeps the pivots d, L_kk = sqrt d)
  double2* B = sm + K * K;       // [K][D]: P -> W = L^-1 P -> G
  const int tid = threadIdx.x;
  const int64_t sf = blockIdx.x;
  const int f = (int)(sf % F), sg = (int)(sf / F);
  for (int i = tid; i < K * K; i += 256) A[i] = R[sf * K * K + i];
  for (int i = tid; i < K * D; i += 256) B[i] = P[sf * K * D + i];
  bool bad = false;
  for (int k = 0; k < K; ++k) {
    __syncthreads();
    const double d = A[k * K + k].x;
    if (!(d > 0.0) || !(d < __longlong_as_double(0x7ff0000000000000ll))) bad = true;
    const double s = sqrt(d);
    for (int i = k + 1 + tid; i < K; i += 256) {
      const double2 v = A[i * K + k];
      A[i * K + k] = double2{v.x / s, v.y / s};
    }
    if (tid < D) {
      const double2 v = B[k * D + tid];
      B[k * D + tid] = double2{v.x / s, v.y / s};
    }
    __syncthreads();
    const int m = K - k - 1;
    for (int idx = tid; idx < m * m; idx += 256) {
      const int ii = idx / m, jj = idx - ii * m;
      if (jj > ii) continue;
      const int i = k + 1 + ii, j = k + 1 + jj;
      const double2 a = A[i * K + k], b = A[j * K + k];
      double2 v = A[i * K + j];
      v.x -= a.x * b.x + a.y * b.y;                      // a conj(b)
      v.y -= a.y * b.x - a.x * b.y;
      A[i * K + j] = v;
    }
    for (int idx = tid; idx < m * D; idx += 256) {
      const int i = k + 1 + idx / D, c = idx % D;
      const double2 a = A[i * K + k], w = B[k * D + c];
      double2 v = B[i * D + c];
      v.x -= a.x * w.x - a.y * w.y;
      v.y -= a.x * w.y + a.y * w.x;
      B[i * D + c] = v;
    }
  }
  for (int k = K - 1; k >= 0; --k) {
    __syncthreads();
    const double s = sqrt(A[k * K + k].x);
    if (tid < D) {
      const double2 v = B[k * D + tid];
      B[k * D + tid] = double2{v.x / s, v.y / s};
    }
    __syncthreads();
    for (int idx = tid; idx < k * D; idx += 256) {
      const int j = idx / D, c = idx % D;
      const double2 a = A[k * K + j], g = B[k * D + c];   // conj(L[k][j]) G[k][c]
      double2 v = B[j * D + c];
      v.x -= a.x * g.x + a.y * g.y;
      v.y -= a.x * g.y - a.y * g.x;
      B[j * D + c] = v;
    }
  }
  __syncthreads();
  for (int i = tid; i < K * D; i += 256) G[((int64_t)sg * K * D + i) * F + f] = B[i];
  if (bad && tid == 0) atomicAdd(info + sg, 1);
}

// --------------------------------------------------------------------------------- filter ----
template <int D>
__global__ __launch_bounds__(256) void wpe_filter_kernel(
    const double2* __restrict__ obs, const double2* __restrict__ G, const int32_t* __restrict__ tab,
    const int64_t* __restrict__ row0, const int32_t* __restrict__ fstart, double2* __restrict__ out, int S,
    int64_t N, int64_t T, int F, int nf, int taps, int delay) {
  const int ft = blockIdx.x % nf;
  const int g = blockIdx.x / nf;
  const int sg = locate(fstart, S, g);
  if (sg < 0) return;
  const Row r = load_row(tab, sg, T);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = ft * 64 + lane;
  if (f >= F) return;
  const int K = taps * D;
  const int64_t n0 = row0[sg];
  const int tw = r.s + (g - fstart[sg]) * FBLK + wave * (FBLK / 4);
  const double2* Gs = G + (int64_t)sg * K * D * F + f;
  for (int tg = tw; tg < tw + FBLK / 4 && tg < r.e; tg += TB) {
    double2 acc[TB][D];
#pragma unroll
    for (int b = 0; b < TB; ++b)
#pragma unroll
      for (int d = 0; d < D; ++d)
        acc[b][d] = tg + b < r.e ? obs[((int64_t)d * T + tg + b) * F + f] : double2{0.0, 0.0};
#pragma unroll 1
    for (int tau = 0; tau < taps; ++tau) {
#pragma unroll 1
      for (int din = 0; din < D; ++din) {
        double2 y[TB];
#pragma unroll
        for (int b = 0; b < TB; ++b) {
          const int u = tg + b - delay - tau;
          y[b] = (u >= r.s && tg + b < r.e) ? obs[((int64_t)din * T + u) * F + f] : double2{0.0, 0.0};
        }
        const double2* gi = Gs + (int64_t)(tau * D + din) * D * F;
#pragma unroll
        for (int d = 0; d < D; ++d) {
          const double2 gv = gi[(int64_t)d * F];
#pragma unroll
          for (int b = 0; b < TB; ++b) {
            acc[b][d].x -= gv.x * y[b].x + gv.y * y[b].y;      // conj(g) y
            acc[b][d].y -= gv.x * y[b].y - gv.y * y[b].x;
          }
        }
      }
    }
#pragma unroll
    for (int b = 0; b < TB; ++b) {
      const int64_t n = n0 + (tg + b - r.s);
      if (tg + b >= r.e || n < 0 || n >= N) continue;
#pragma unroll
      for (int d = 0; d < D; ++d) out[((int64_t)d * N + n) * F + f] = acc[b][d];
    }
  }
}

// ------------------------------------------------------------------------------ launchers ----
int run_prep(const int32_t* tab, char* ws, const Lay& l, int S, int64_t T, hipStream_t s) {
  hipLaunchKernelGGL(wpe_prep_kernel, dim3(1), dim3(64), 0, s, tab, reinterpret_cast<int32_t*>(ws + l.o_cstart),
                     reinterpret_cast<int32_t*>(ws + l.o_fstart), S, T, l.gmax, l.fmax);
  return tssep_launch_status();
}

int run_power(const double* obs, const double* xs, const int32_t* tab, const int64_t* row0, double* lam, char* ws,
              const Lay& l, int S, int64_t N, int D, int64_t T, int F, hipStream_t s) {
  unsigned long long* pmax = reinterpret_cast<unsigned long long*>(ws + l.o_pmax);
  const int32_t* fstart = reinterpret_cast<const int32_t*>(ws + l.o_fstart);
  if (hipMemsetAsync(pmax, 0, (size_t)S * F * 8, s) != hipSuccess) return TSSEP_E_LAUNCH;
  const int nf = (F + 63) / 64;
  const dim3 grid((unsigned)(l.fmax * nf));
  hipLaunchKernelGGL(wpe_power_kernel, grid, dim3(256), 0, s, reinterpret_cast<const double2*>(obs),
                     reinterpret_cast<const double2*>(xs), tab, row0, fstart, lam, pmax, S, N, D, T, F, nf);
  int st = tssep_launch_status();
  if (st != TSSEP_OK) return st;
  hipLaunchKernelGGL(wpe_lambda_kernel, grid, dim3(256), 0, s, tab, row0, fstart, lam, pmax, S, N, T, F, nf);
  return tssep_launch_status();
}

int run_corr(const double* obs, const double* lam, const int32_t* tab, const int64_t* row0, double* R, double* P,
             char* ws, const Lay& l, int S, int64_t N, int D, int64_t T, int F, int taps, int delay, int valid,
             hipStream_t s) {
  const int32_t* cstart = reinterpret_cast<const int32_t*>(ws + l.o_cstart);
  double2* part = reinterpret_cast<double2*>(ws + l.o_part);
  const int64_t nblocks = l.gmax * F;
  const int64_t per_xcd = (nblocks + 7) / 8;
  const size_t lds = (size_t)(TSUB + delay + taps - 1) * D * 16 + TSUB * 8;
  hipLaunchKernelGGL(wpe_corr_kernel, dim3((unsigned)(per_xcd * 8)), dim3(256), lds, s,
                     reinterpret_cast<const double2*>(obs), lam, tab, row0, cstart, part, S, N, D, T, F, taps, delay,
                     valid, l.ntiles, l.tilesR, l.PB, per_xcd, nblocks);
  int st = tssep_launch_status();
  if (st != TSSEP_OK) return st;
  const int64_t n = (int64_t)S * F * (l.K * l.K + l.K * D);
  hipLaunchKernelGGL(wpe_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, cstart,
                     reinterpret_cast<double2*>(R), reinterpret_cast<double2*>(P), S, D, F, l.K, l.ntiles, l.tilesR,
                     l.PB, l.gmax);
  return tssep_launch_status();
}

int run_solve(const double* R, const double* P, double* G, int* info, int S, int D, int F, int K, hipStream_t s) {
  // per device: a second GPU of the process needs the attribute on its own copy of the kernel
  static std::atomic<bool> attr_set[64];
  int devid = 0;
  if (hipGetDevice(&devid) != hipSuccess) return TSSEP_E_LAUNCH;
  if (devid < 0 || devid >= 64 || !attr_set[devid].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(wpe_solve_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (WMAXK * WMAXK + WMAXK * WMAXD) * 16) != hipSuccess)
      return TSSEP_E_LAUNCH;
    if (devid >= 0 && devid < 64) attr_set[devid].store(true, std::memory_order_release);
  }
  const size_t lds = (size_t)(K * K + K * D) * 16;
  hipLaunchKernelGGL(wpe_solve_kernel, dim3((unsigned)((int64_t)S * F)), dim3(256), lds, s,
                     reinterpret_cast<const double2*>(R), reinterpret_cast<const double2*>(P),
                     reinterpret_cast<double2*>(G), info, D, F, K);
  return tssep_launch_status();
}

template <int D>
int launch_filter(const double* obs, const double* G, const int32_t* tab, const int64_t* row0, const int32_t* fstart,
                  double* out, int64_t fmax, int S, int64_t N, int64_t T, int F, int taps, int delay, hipStream_t s) {
  const int nf = (F + 63) / 64;
  hipLaunchKernelGGL(wpe_filter_kernel<D>, dim3((unsigned)(fmax * nf)), dim3(256), 0, s,
                     reinterpret_cast<const double2*>(obs), reinterpret_cast<const double2*>(G), tab, row0, fstart,
                     reinterpret_cast<double2*>(out), S, N, T, F, nf, taps, delay);
  return tssep_launch_status();
}

int run_filter(const double* obs, const double* G, const int32_t* tab, const int64_t* row0, double* out, char* ws,
               const Lay& l, int S, int64_t N, int D, int64_t T, int F, int taps, int delay, hipStream_t s) {
  const int32_t* fstart = reinterpret_cast<const int32_t*>(ws + l.o_fstart);
#define CALL(DD) launch_filter<DD>(obs, G, tab, row0, fstart, out, l.fmax, S, N, T, F, taps, delay, s)
  switch (D) {
    case 1: return CALL(1);
    case 2: return CALL(2);
    case 3: return CALL(3);
    case 4: return CALL(4);
    case 5: return CALL(5);
    case 6: return CALL(6);
    case 7: return CALL(7);
    case 8: return CALL(8);
    default: return TSSEP_E_UNSUPPORTED;
  }
#undef CALL
}

int check_args(int S, int64_t N, int D, int64_t T, int F, int taps, int delay) {
  if (D > WMAXD || (taps >= 1 && D >= 1 && (int64_t)taps * D > WMAXK) || delay > WMAXDELAY) return TSSEP_E_UNSUPPORTED;
  return wpe_shape_ok(S, N, D, T, F, taps, delay) ? TSSEP_OK : TSSEP_E_SHAPE;
}

}  // namespace

extern "C" int64_t tssep_wpe_workspace_bytes(int S, int64_t N, int D, int64_t T, int F, int taps, int delay) {
  if (!wpe_shape_ok(S, N, D, T, F, taps, delay)) return 0;
  return make_lay(S, N, D, F, taps).total;
}

extern "C" int tssep_wpe_power(const double* obs, const double* x_seg, const int32_t* segments,
                               const int64_t* row0, double* lam, void* workspace, int S, int64_t N, int D,
                               int64_t T, int F, void* stream) {
  if (!obs || !segments || !row0 || !lam || !workspace) return TSSEP_E_NULL;
  int st = check_args(S, N, D, T, F, 1, 0);
  if (st != TSSEP_OK) return st;
  if (!aligned16(obs) || !aligned16(workspace) || (x_seg && !aligned16(x_seg))) return TSSEP_E_ALIGN;
  // the prefix arrays and the maxima sit at offsets that do not depend on taps
  const Lay l = make_lay(S, N, D, F, 1);
  char* ws = static_cast<char*>(workspace);
  st = run_prep(segments, ws, l, S, T, (hipStream_t)stream);
  if (st != TSSEP_OK) return st;
  return run_power(obs, x_seg, segments, row0, lam, ws, l, S, N, D, T, F, (hipStream_t)stream);
}

extern "C" int tssep_wpe_correlations(const double* obs, const double* lam, const int32_t* segments,
                                      const int64_t* row0, double* R, double* P, void* workspace, int S,
                                      int64_t N, int D, int64_t T, int F, int taps, int delay, int valid_mode,
                                      void* stream) {
  if (!obs || !lam || !segments || !row0 || !R || !P || !workspace) return TSSEP_E_NULL;
  int st = check_args(S, N, D, T, F, taps, delay);
  if (st != TSSEP_OK) return st;
  if (!aligned16(obs) || !aligned16(workspace) || !aligned16(R) || !aligned16(P)) return TSSEP_E_ALIGN;
  const Lay l = make_lay(S, N, D, F, taps);
  char* ws = static_cast<char*>(workspace);
  st = run_prep(segments, ws, l, S, T, (hipStream_t)stream);
  if (st != TSSEP_OK) return st;
  return run_corr(obs, lam, segments, row0, R, P, ws, l, S, N, D, T, F, taps, delay, valid_mode != 0,
                  (hipStream_t)stream);
}

extern "C" int tssep_wpe_solve(const double* R, const double* P, double* G, int* info, int S, int D, int F,
                               int taps, void* stream) {
  if (!R || !P || !G || !info) return TSSEP_E_NULL;
  int st = check_args(S, 1, D, 1, F, taps, 0);
  if (st != TSSEP_OK) return st;
  if (!aligned16(R) || !aligned16(P) || !aligned16(G)) return TSSEP_E_ALIGN;
  if (hipMemsetAsync(info, 0, sizeof(int) * (size_t)S, (hipStream_t)stream) != hipSuccess) return TSSEP_E_LAUNCH;
  return run_solve(R, P, G, info, S, D, F, taps * D, (hipStream_t)stream);
}

extern "C" int tssep_wpe_filter(const double* obs, const double* G, const int32_t* segments, const int64_t* row0,
                                double* obs_seg, void* workspace, int S, int64_t N, int D, int64_t T, int F,
                                int taps, int delay, void* stream) {
  if (!obs || !G || !segments || !row0 || !obs_seg || !workspace) return TSSEP_E_NULL;
  int st = check_args(S, N, D, T, F, taps, delay);
  if (st != TSSEP_OK) return st;
  if (!aligned16(obs) || !aligned16(G) || !aligned16(obs_seg) || !aligned16(workspace)) return TSSEP_E_ALIGN;
  const Lay l = make_lay(S, N, D, F, taps);
  char* ws = static_cast<char*>(workspace);
  st = run_prep(segments, ws, l, S, T, (hipStream_t)stream);
  if (st != TSSEP_OK) return st;
  return run_filter(obs, G, segments, row0, obs_seg, ws, l, S, N, D, T, F, taps, delay, (hipStream_t)stream);
}

extern "C" int tssep_wpe_fwd(const double* obs, const int32_t* segments, const int64_t* row0, double* obs_seg,
                             void* workspace, int* info, int S, int64_t N, int D, int64_t T, int F, int taps,
                             int delay, int iterations, int valid_mode, void* stream) {
  if (!obs || !segments || !row0 || !obs_seg || !workspace || !info) return TSSEP_E_NULL;
  int st = check_args(S, N, D, T, F, taps, delay);
  if (st != TSSEP_OK) return st;
  if (iterations < 1) return TSSEP_E_SHAPE;
  if (!aligned16(obs) || !aligned16(obs_seg) || !aligned16(workspace)) return TSSEP_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const Lay l = make_lay(S, N, D, F, taps);
  char* ws = static_cast<char*>(workspace);
  double* lam = reinterpret_cast<double*>(ws + l.o_lam);
  double* R = reinterpret_cast<double*>(ws + l.o_R);
  double* P = reinterpret_cast<double*>(ws + l.o_P);
  double* G = reinterpret_cast<double*>(ws + l.o_G);
  // one count over all iterations: a failed factorisation of an early iteration stays visible
  if (hipMemsetAsync(info, 0, sizeof(int) * (size_t)S, s) != hipSuccess) return TSSEP_E_LAUNCH;
  st = run_prep(segments, ws, l, S, T, s);
  for (int it = 0; it < iterations && st == TSSEP_OK; ++it) {
    st = run_power(obs, it ? obs_seg : nullptr, segments, row0, lam, ws, l, S, N, D, T, F, s);
    if (st == TSSEP_OK)
      st = run_corr(obs, lam, segments, row0, R, P, ws, l, S, N, D, T, F, taps, delay, valid_mode != 0, s);
    if (st == TSSEP_OK) st = run_solve(R, P, G, info, S, D, F, l.K, s);
    if (st == TSSEP_OK) st = run_filter(obs, G, segments, row0, obs_seg, ws, l, S, N, D, T, F, taps, delay, s);
  }
  return st;
}
