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
//
// The online (recursive least squares) form, DESIGN 4.19, is one more kernel at the end of the file:
//   wpe_online_kernel      one workgroup per (batch element, bin): Q (both triangles, rows padded to an odd count), G and
//                          the ring of the last frames in LDS across the frames of a call, one rank-one update per frame
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

// --------------------------------------------------------------------------- online (RLS) ----
// Per (b, f), frame by frame (Yt as above, zeros in front of the stream; a = forgetting, c = power_context):
//   p = sum_{s=t-c..t} sum_d |y_s[d]|^2 / (D (c + 1))     pmax = max(pmax, p) over the finite p
//   pmax == 0: x = y, nothing moves.   lam = max(p, 1e-10 pmax)
//   x = y - G^H Yt (the output)        u = Q Yt      den = a lam + Re(Yt^H u)      not (0 < den < inf): info += 1, nothing moves
//   k = u / den       Q = (Q - k u^H) / a   (lower triangle computed, mirrored, real diagonal)       G += k x^H
// LDS: Q [K][K | 1] with both triangles (an odd row stride: the rows of a matrix-vector product fall on different banks),
// G transposed [D][K], the ring [R + 1][D] (R = max(delay + taps - 1, c) carried frames and the current one), Yt, u, k [K],
// x [D].  The matrix-vector products split a row over S lanes of a wave (S from K + D alone), joined by xor shuffles; den is
// summed per wave by the same butterfly, so every thread holds the same bits and every branch is uniform.  Four barriers
// per frame.  The state in memory holds the lower triangle only, and zeros for Q while pmax == 0 (a stream that has seen
// nothing but silence carries the state of a fresh one: all zeros).
constexpr int OMAXPC = 256;
constexpr int ONTRI = (WMAXK * (WMAXK + 1) / 2 + 255) / 256;      // triangle entries per thread
constexpr size_t OMAXLDS =
    (size_t)(WMAXK * (WMAXK | 1) + WMAXK * WMAXD + (WMAXDELAY + WMAXK) * WMAXD + 3 * WMAXK + WMAXD) * 16;

struct OLay { int K, LD, R, S, ntri; size_t lds; };
__host__ OLay online_lay(int D, int taps, int delay, int pc) {
  OLay l;
  l.K = taps * D;
  l.LD = l.K | 1;
  const int hist = delay + taps - 1;
  l.R = hist > pc ? hist : pc;
  l.S = 1;
  while (l.S < 8 && 2 * l.S * (l.K + D) <= 256) l.S *= 2;
  l.ntri = l.K * (l.K + 1) / 2;
  l.lds = (size_t)(l.K * l.LD + D * l.K + (l.R + 1) * D + 3 * l.K + D) * 16;
  return l;
}
__host__ int online_args(int64_t B, int D, int64_t T, int F, int taps, int delay, int pc) {
  if (B <= 0 || D < 1 || T <= 0 || F <= 0 || taps < 1 || delay < 0 || pc < 0) return TSSEP_E_SHAPE;
  if (D > WMAXD || (int64_t)taps * D > WMAXK || delay > WMAXDELAY || pc > OMAXPC) return TSSEP_E_UNSUPPORTED;
  if (B * F >= ((int64_t)1 << 30) || T >= ((int64_t)1 << 30) || B * D * T * F >= ((int64_t)1 << 40)) return TSSEP_E_SHAPE;
  return TSSEP_OK;
}

__device__ __forceinline__ int tri_row(int idx) {
  int i = (int)((sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
  while (i * (i + 1) / 2 > idx) --i;
  while ((i + 1) * (i + 2) / 2 <= idx) ++i;
  return i;
}
__device__ __forceinline__ double2 load_obs(const void* __restrict__ obs, int obs_f64, int64_t at) {
  if (obs_f64) return static_cast<const double2*>(obs)[at];
  const float2 v = static_cast<const float2*>(obs)[at];
  return double2{(double)v.x, (double)v.y};
}

__global__ __launch_bounds__(256) void wpe_online_kernel(
    const void* __restrict__ obs, int obs_f64, const double2* __restrict__ Qin, const double2* __restrict__ Gin,
    const double2* __restrict__ ringin, const double* __restrict__ pmaxin, double2* __restrict__ Qout,
    double2* __restrict__ Gout, double2* __restrict__ ringout, double* __restrict__ pmaxout, int* __restrict__ info,
    double2* __restrict__ out, int D, int64_t T, int F, int taps, int delay, int pc, int R, int S, double a, double ia,
    double load) {
  extern __shared__ double2 osm[];
  const int K = taps * D, LD = K | 1, ntri = K * (K + 1) / 2;
  double2* Q = osm;                    // [K][LD]
  double2* Gt = Q + K * LD;            // [D][K]
  double2* ring = Gt + D * K;          // [R + 1][D]
  double2* yt = ring + (R + 1) * D;    // [K]
  double2* u = yt + K;                 // [K]
  double2* kk = u + K;                 // [K]
  double2* xs = kk + K;                // [D]
  const int tid = threadIdx.x;
  const int64_t bf = blockIdx.x;
  const int64_t b = bf / F;
  const int f = (int)(bf % F);
  const double INF = __longlong_as_double(0x7ff0000000000000ll);

  double pmax = pmaxin ? pmaxin[bf] : 0.0;
  const bool fresh = !Qin || pmax == 0.0;
  int ij[ONTRI];
#pragma unroll
  for (int q = 0; q < ONTRI; ++q) {
    const int idx = tid + 256 * q;
    ij[q] = -1;
    if (idx < ntri) {
      const int i = tri_row(idx), j = idx - i * (i + 1) / 2;
      ij[q] = (i << 8) | j;
      double2 v = fresh ? double2{i == j ? 1.0 / load : 0.0, 0.0} : Qin[bf * ntri + idx];
      if (i == j) v.y = 0.0;
      Q[i * LD + j] = v;
      if (i != j) Q[j * LD + i] = double2{v.x, -v.y};
    }
  }
  for (int idx = tid; idx < K * D; idx += 256) {
    const int i = idx / D, d = idx - i * D;
    Gt[d * K + i] = fresh ? double2{0.0, 0.0} : Gin[bf * K * D + idx];
  }
  for (int idx = tid; idx < R * D; idx += 256) ring[idx] = ringin ? ringin[bf * R * D + idx] : double2{0.0, 0.0};

  const int my_tau = tid < K ? tid / D : 0;
  const int my_d = tid < K ? tid - my_tau * D : 0;
  const int my_lag = delay + my_tau;
  const int r = tid / S, s = tid - r * S;
  const int lane = tid & 63;
  const int64_t at0 = ((b * D + (tid < D ? tid : 0)) * T) * F + f;      // frame 0 of this thread's channel
  int cur = R;                                                          // the slot of the current frame
  int bad = 0;
  double2 ynext = double2{0.0, 0.0};
  if (tid < D) ring[cur * D + tid] = load_obs(obs, obs_f64, at0);
  __syncthreads();

  for (int64_t n = 0; n < T; ++n) {
    if (tid < D && n + 1 < T) ynext = load_obs(obs, obs_f64, at0 + (n + 1) * F);
    if (tid < K) {
      int slot = cur - my_lag;
      if (slot < 0) slot += R + 1;
      yt[tid] = ring[slot * D + my_d];
    }
    double p = 0.0;
    for (int c = pc; c >= 0; --c) {
      int slot = cur - c;
      if (slot < 0) slot += R + 1;
      for (int d = 0; d < D; ++d) {
        const double2 v = ring[slot * D + d];
        p += v.x * v.x + v.y * v.y;
      }
    }
    p /= (double)(D * (pc + 1));
    if (p > pmax && p < INF) pmax = p;
    const bool silent = pmax == 0.0;
    const double flo = 1e-10 * pmax;
    const double lam = p < flo ? flo : p;                               // a NaN stays one
    __syncthreads();

    double2 acc = {0.0, 0.0};
    if (r < K) {
      const double2* row = Q + r * LD;
      for (int j = s; j < K; j += S) {
        const double2 q = row[j], y = yt[j];
        acc.x += q.x * y.x - q.y * y.y;
        acc.y += q.x * y.y + q.y * y.x;
      }
    } else if (r < K + D) {
      const double2* col = Gt + (r - K) * K;
      for (int i = s; i < K; i += S) {
        const double2 g = col[i], y = yt[i];
        acc.x += g.x * y.x + g.y * y.y;                                 // conj(g) y
        acc.y += g.x * y.y - g.y * y.x;
      }
    }
    for (int m = 1; m < S; m <<= 1) {
      acc.x += __shfl_xor(acc.x, m);
      acc.y += __shfl_xor(acc.y, m);
    }
    if (s == 0) {
      if (r < K) {
        u[r] = acc;
      } else if (r < K + D) {
        const int d = r - K;
        const double2 y = ring[cur * D + d];
        const double2 x = silent ? y : double2{y.x - acc.x, y.y - acc.y};
        xs[d] = x;
        out[((b * D + d) * T + n) * F + f] = x;
      }
    }
    __syncthreads();

    double part = 0.0;
    for (int i = lane; i < K; i += 64) part += yt[i].x * u[i].x + yt[i].y * u[i].y;
    for (int m = 32; m >= 1; m >>= 1) part += __shfl_xor(part, m);
    const double den = a * lam + part;
    const bool ok = !silent && den > 0.0 && den < INF;
    if (!silent && !ok && tid == 0) ++bad;
    if (ok && tid < K) kk[tid] = double2{u[tid].x / den, u[tid].y / den};
    __syncthreads();

    if (ok) {
#pragma unroll
      for (int q = 0; q < ONTRI; ++q) {
        if (ij[q] < 0) continue;
        const int i = ij[q] >> 8, j = ij[q] & 255;
        const double2 k = kk[i], w = u[j];
        double2 v = Q[i * LD + j];
        v.x = (v.x - (k.x * w.x + k.y * w.y)) * ia;                     // k conj(w)
        v.y = i == j ? 0.0 : (v.y - (k.y * w.x - k.x * w.y)) * ia;
        Q[i * LD + j] = v;
        if (i != j) Q[j * LD + i] = double2{v.x, -v.y};
      }
      for (int idx = tid; idx < K * D; idx += 256) {
        const int d = idx / K, i = idx - d * K;
        const double2 k = kk[i], x = xs[d];
        double2 g = Gt[idx];
        g.x += k.x * x.x + k.y * x.y;                                   // k conj(x)
        g.y += k.y * x.x - k.x * x.y;
        Gt[idx] = g;
      }
    }
    cur = cur == R ? 0 : cur + 1;
    if (tid < D && n + 1 < T) ring[cur * D + tid] = ynext;
    __syncthreads();
  }

  // `cur` is the slot frame T would take: the last R frames sit in the R slots behind it
  const bool zero = pmax == 0.0;
#pragma unroll
  for (int q = 0; q < ONTRI; ++q) {
    if (ij[q] < 0) continue;
    const int i = ij[q] >> 8, j = ij[q] & 255;
    Qout[bf * ntri + tid + 256 * q] = zero ? double2{0.0, 0.0} : Q[i * LD + j];
  }
  for (int idx = tid; idx < K * D; idx += 256) {
    const int i = idx / D, d = idx - i * D;
    Gout[bf * K * D + idx] = Gt[d * K + i];
  }
  for (int idx = tid; idx < R * D; idx += 256) {
    const int fr = idx / D, d = idx - fr * D;
    int slot = cur - R + fr;
    if (slot < 0) slot += R + 1;
    ringout[bf * R * D + idx] = ring[slot * D + d];
  }
  if (tid == 0) {
    pmaxout[bf] = pmax;
    if (bad) atomicAdd(info + b, bad);
  }
}

int run_online(const void* obs, int obs_f64, const double* q_in, const double* g_in, const double* ring_in,
               const double* pmax_in, const int* info_in, double* q_out, double* g_out, double* ring_out,
               double* pmax_out, int* info_out, double* out, int64_t B, int D, int64_t T, int F, int taps, int delay,
               int pc, double forgetting, double load, hipStream_t s) {
  static std::atomic<bool> attr_set[64];
  int devid = 0;
  if (hipGetDevice(&devid) != hipSuccess) return TSSEP_E_LAUNCH;
  if (devid < 0 || devid >= 64 || !attr_set[devid].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(wpe_online_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)OMAXLDS) != hipSuccess)
      return TSSEP_E_LAUNCH;
    if (devid >= 0 && devid < 64) attr_set[devid].store(true, std::memory_order_release);
  }
  const OLay l = online_lay(D, taps, delay, pc);
  if (l.lds > OMAXLDS) return TSSEP_E_UNSUPPORTED;
  // the count of a stream goes on: the kernel adds to what the call before left
  if (info_in) {
    if (info_in != info_out &&
        hipMemcpyAsync(info_out, info_in, sizeof(int) * (size_t)B, hipMemcpyDeviceToDevice, s) != hipSuccess)
      return TSSEP_E_LAUNCH;
  } else if (hipMemsetAsync(info_out, 0, sizeof(int) * (size_t)B, s) != hipSuccess) {
    return TSSEP_E_LAUNCH;
  }
  hipLaunchKernelGGL(wpe_online_kernel, dim3((unsigned)(B * F)), dim3(256), l.lds, s, obs, obs_f64,
                     reinterpret_cast<const double2*>(q_in), reinterpret_cast<const double2*>(g_in),
                     reinterpret_cast<const double2*>(ring_in), pmax_in, reinterpret_cast<double2*>(q_out),
                     reinterpret_cast<double2*>(g_out), reinterpret_cast<double2*>(ring_out), pmax_out, info_out,
                     reinterpret_cast<double2*>(out), D, T, F, taps, delay, pc, l.R, l.S, forgetting, 1.0 / forgetting,
                     load);
  return tssep_launch_status();
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

extern "C" int64_t tssep_wpe_online_state_bytes(int64_t B, int D, int F, int taps, int delay, int power_context) {
  if (online_args(B, D, 1, F, taps, delay, power_context) != TSSEP_OK) return 0;
  const OLay l = online_lay(D, taps, delay, power_context);
  return B * F * (16 * (int64_t)(l.ntri + l.K * D + l.R * D) + 8) + 4 * B;
}

extern "C" int tssep_wpe_online_fwd(const void* obs, int obs_f64, const double* q_in, const double* g_in,
                                    const double* ring_in, const double* pmax_in, const int* info_in, double* q_out,
                                    double* g_out, double* ring_out, double* pmax_out, int* info_out, double* out,
                                    int64_t B, int D, int64_t T, int F, int taps, int delay, int power_context,
                                    double forgetting, double load, void* stream) {
  int st = online_args(B, D, T, F, taps, delay, power_context);
  if (st != TSSEP_OK) return st;
  if (!(forgetting > 0.0 && forgetting <= 1.0) || !(load > 0.0 && load < __builtin_inf())) return TSSEP_E_SHAPE;
  const bool ring = online_lay(D, taps, delay, power_context).R > 0;
  if (!obs || !q_out || !g_out || !pmax_out || !info_out || !out || (ring && !ring_out)) return TSSEP_E_NULL;
  const int given = (q_in != nullptr) + (g_in != nullptr) + (pmax_in != nullptr) + (info_in != nullptr) +
                    (!ring || ring_in != nullptr);
  if (q_in ? given != 5 : given != (ring ? 0 : 1)) return TSSEP_E_NULL;       // a whole state or none
  if (!aligned16(out) || !aligned16(q_out) || !aligned16(g_out) || !aligned16(ring_out) || !aligned16(q_in) ||
      !aligned16(g_in) || !aligned16(ring_in) || (((uintptr_t)obs) & (obs_f64 ? 15u : 7u)) ||
      (((uintptr_t)pmax_in) & 7u) || (((uintptr_t)pmax_out) & 7u))
    return TSSEP_E_ALIGN;
  return run_online(obs, obs_f64, q_in, g_in, ring_in, pmax_in, info_in, q_out, g_out, ring_out, pmax_out, info_out, out,
                    B, D, T, F, taps, delay, power_context, forgetting, load, (hipStream_t)stream);
}
