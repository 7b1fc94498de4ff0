// Mask-based MVDR beamformer (Souden) in complex128 -- the eval-time enhancer of the reference,
// TorchBF.__call__ (tssep/train/enhancer.py:215-265):
//   psd[m,k,f]  = sum_t w_m[k,t,f] Y[:,t,f] Y[:,t,f]^H        (torch.einsum, :226-250)
//   phi         = solve(psd[interference], psd[target])        (torch.linalg.solve, :253)
//   bf[k,f,:]   = phi[:, ref] / max(Re trace(phi), eps)        (:254-258)
//   enh[k,t,f]  = sum_d conj(bf[k,f,d]) Y[d,t,f]   (* max(mask, masking_eps))   (:259-264)
//
// All of it is HBM-bound double-precision vector work (no matrix cores: D <= 8 channels), laid out
// with lane = frequency bin so that every load and store of a wave is 512 B - 1 KB contiguous:
//   1. mvdr_psd_kernel<D>     one wave per (64 bins, time chunk, speaker): 2 D*D doubles of
//                             Hermitian accumulators (target, interference) per lane; 4 speakers
//                             per workgroup share the Y frames through LDS; the chunk partials go
//                             to the workspace (fixed summation order -> run-to-run identical).
//                             The workgroups that share one Y tile are mapped to ONE XCD so the
//                             tile is fetched from HBM once and served from that XCD's L2 after.
//   2. mvdr_reduce_kernel     adds the chunk partials (into chunk 0), one lane per element;
//      mvdr_solve_kernel<D>   one lane per (speaker, bin): LU with partial pivoting (LAPACK zgesv's
//                             pivot rule, |re|+|im|), trace, scaling -- in registers for D <= 6,
//      mvdr_weights_kernel    with the D x D systems in LDS ([element][lane]) for D = 7, 8.
//   3. mvdr_apply_kernel<D>   one wave per (64 bins, time chunk, up to 4 speakers): Y read once
//                             for the speakers of a group.
// The segment-wise pipeline of ClassicBF_np (one beamformer per activity interval of a speaker, the
// distortion mask taken from the other speakers' masks) and the backward of the dense pipeline
// follow in this file, and last the frame-recursive (online) MVDR, one kernel; the segments share the solve kernels.
// The statistics pass and the first
// time pass of the backward run on one frame pipeline (decode_time_tile / frame_pipeline).
#include "common.h"

#include <type_traits>

namespace {

constexpr int MAXD = 8;
constexpr int KG = 4;                    // speakers per apply workgroup

struct Plan {
  int nf;          // 64-bin tiles
  int chunks;      // time chunks of the PSD pass
  int64_t tchunk;  // frames per chunk
};
// Time chunks of the statistics pass: 512 workgroups are resident at once (2 per CU); pick the chunk
// count that minimises (rounds of resident workgroups) x (frames per chunk) -- one workgroup more
// than a round costs a whole extra round -- with a small charge per chunk for the partials' traffic.
__host__ Plan make_plan(int64_t B, int K, int64_t T, int F) {
  Plan p;
  p.nf = (F + 63) / 64;
  const int64_t per_chunk = B * p.nf * ((K + 3) / 4);        // workgroups of 4 speakers
  int64_t cmax = (T + 15) / 16;
  if (cmax > 256) cmax = 256;
  int64_t best_c = 1;
  double best = 1e300;
  for (int64_t c = 1; c <= cmax; ++c) {
    const int64_t frames = (T + c - 1) / c;
    const int64_t rounds = (per_chunk * c + 511) / 512;
    const double cost = (double)rounds * (double)(frames + 8) + 0.5 * (double)c;
    if (cost < best) { best = cost; best_c = c; }
  }
  p.tchunk = (T + best_c - 1) / best_c;
  p.chunks = (int)((T + p.tchunk - 1) / p.tchunk);
  return p;
}

__device__ __forceinline__ double load_mask(const void* masks, int f64, int64_t i) {
  return f64 ? static_cast<const double*>(masks)[i] : (double)static_cast<const float*>(masks)[i];
}

// The float / double pair of a launch whose kernel is templated on the mask's dtype: `launch` is a
// generic lambda that gets the mask pointer typed (MT = mask_t<decltype(pointer)>)
template <typename P> using mask_t = std::remove_cv_t<std::remove_pointer_t<P>>;
template <typename Launch> int launch_mt(int mask_f64, const void* masks, Launch launch) {
  if (mask_f64) launch(static_cast<const double*>(masks));
  else launch(static_cast<const float*>(masks));
  return tssep_launch_status();
}

// XCD-aware block -> (tile, member): consecutive block ids go round-robin over the 8 XCDs, so the
// `members` workgroups that read the same tile get ids  8*(tile/8*members + member) + tile%8
__device__ __forceinline__ bool xcd_tile(int64_t bid, int members, int64_t tiles, int64_t& tile,
                                         int& member) {
  const int xcd = (int)(bid & 7);
  const int64_t within = bid >> 3;
  tile = (within / members) * 8 + xcd;
  member = (int)(within % members);
  return tile < tiles;
}
__host__ int64_t xcd_grid(int64_t tiles, int members) { return ((tiles + 7) / 8) * 8 * members; }

// ------------------------------------------------------------------ the time passes ----
// One workgroup = 4 waves = 4 speakers of one (64 bins, time chunk) tile.  Every wave fetches one
// frame of Y per step and shares it with the other three through LDS (double buffered, one barrier
// per step), so Y crosses the L2 once per 4 speakers instead of once per (speaker, mask): a first
// version with one wave per (speaker, mask) reading Y straight from L2 was L2-bandwidth bound
// (16 x 92 MB per 30-s utterance, 1.7 TB/s of algorithmic traffic).  mvdr_psd_kernel and
// mvdr_bwd_gw_kernel run on this pipeline; mvdr_bwd_mask_kernel keeps its own copy of it (on the shared one its
// D = 8 float instantiation wrote the NaNs of singular bins with the other sign bit).
constexpr int PW = 4;      // waves (= speakers) per workgroup
__host__ int64_t time_grid(const Plan& p, int64_t B, int K) {
  return xcd_grid(B * p.chunks * p.nf, (K + PW - 1) / PW);
}

// What a workgroup of a time pass works on: frames [t0, t1) of chunk c, wave = speaker k (kvalid:
// k < K), lane = bin fraw (f: clamped into [0, F) for the reads)
struct TimeTile {
  int64_t b, t0, t1;
  int c, lane, wave, k, fraw, f, steps;
  bool kvalid;
};
__device__ __forceinline__ bool decode_time_tile(const Plan& plan, int64_t B, int K, int64_t T,
                                                 int F, TimeTile& tt) {
  const int groups = (K + PW - 1) / PW;
  int64_t tile;
  int grp;
  if (!xcd_tile(blockIdx.x, groups, B * plan.chunks * plan.nf, tile, grp)) return false;
  const int ft = (int)(tile % plan.nf);
  tt.c = (int)((tile / plan.nf) % plan.chunks);
  tt.b = tile / ((int64_t)plan.nf * plan.chunks);
  tt.lane = threadIdx.x & 63;
  tt.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar: uniform branches
  tt.k = grp * PW + tt.wave;
  tt.kvalid = tt.k < K;
  tt.fraw = ft * 64 + tt.lane;
  tt.f = tt.fraw < F ? tt.fraw : F - 1;
  tt.t0 = tt.c * plan.tchunk;
  tt.t1 = tt.t0 + plan.tchunk < T ? tt.t0 + plan.tchunk : T;
  tt.steps = (int)((tt.t1 - tt.t0 + PW - 1) / PW);
  return true;
}

// The double-buffered loop over the steps of a chunk.  The frames arrive by asynchronous
// global -> LDS copies (1 KB per wave instruction, lane-linear: exactly [channel][lane] of double2),
// no staging registers; y0: the observation of the batch element at bin f.  fetch(s, regs) loads
// what else step s needs into the caller's Regs, compute(s, regs) consumes ybuf[s & 1].
// Written as a function of the __restrict__ y0 and the array reference, the compiler no longer takes the copies of
// step s + 1 in flight for aliases of the LDS reads of step s: the s_waitcnt vmcnt(0) after each barrier and the
// waits between the reads are gone (46 -> 14 s_waitcnt in mvdr_psd_kernel<6, float>), the full wait in front of
// each barrier stays.  That is right, the two touch different halves of ybuf, and it is where the 8 % of the
// statistics pass at 8 x cfg5 came from; it hangs on alias information that a later edit can lose again.
template <int D, typename Regs, typename Fetch, typename Compute>
__device__ __forceinline__ void frame_pipeline(const TimeTile& tt, double2 (&ybuf)[2][PW][D][64],
                                               const double2* __restrict__ y0, int64_t T, int F,
                                               Fetch fetch, Compute compute) {
  // wave w brings frame t0 + PW s + w of step s; frames past the chunk are zero-filled
  auto fetch_y = [&](int s_) {
    const int64_t t = tt.t0 + (int64_t)s_ * PW + tt.wave;
    if (t < tt.t1) {
#pragma unroll
      for (int d = 0; d < D; ++d)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(y0 + (d * T + t) * F),
            (__attribute__((address_space(3))) void*)&ybuf[s_ & 1][tt.wave][d][0], 16, 0, 0);
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) ybuf[s_ & 1][tt.wave][d][tt.lane] = double2{0.0, 0.0};
    }
  };
  // one barrier per step: it drains the copies of step s (every wave waits for its own before
  // arriving) and separates compute(s-1) from the copies of step s+1 into the same buffer
  Regs ra, rb;
  fetch_y(0);
  fetch(0, ra);
  for (int s = 0; s < tt.steps; s += 2) {
    __syncthreads();
    if (s + 1 < tt.steps) { fetch_y(s + 1); fetch(s + 1, rb); }
    if (tt.kvalid) compute(s, ra);
    if (s + 1 >= tt.steps) break;
    __syncthreads();
    if (s + 2 < tt.steps) { fetch_y(s + 2); fetch(s + 2, ra); }
    if (tt.kvalid) compute(s + 1, rb);
  }
}

// ------------------------------------------------------------------ packed Hermitian ----
// [D diagonals, then re / im per pair i < j] x F
// one packed Hermitian accumulator -> out (already at its matrix and bin)
template <int D>
__device__ __forceinline__ void store_packed_herm(double* __restrict__ out, int F, const double (&diag)[D],
                                                  const double2 (&off)[D * (D - 1) / 2 + 1]) {
#pragma unroll
  for (int i = 0; i < D; ++i) out[(int64_t)i * F] = diag[i];
#pragma unroll
  for (int p = 0; p < D * (D - 1) / 2; ++p) {
    out[(int64_t)(D + 2 * p) * F] = off[p].x;
    out[(int64_t)(D + 2 * p + 1) * F] = off[p].y;
  }
}

template <typename MT> struct MaskRegs { MT w0[PW], w1[PW]; };

// Target AND interference statistics of a speaker per wave
template <int D, typename MT>
__global__ __launch_bounds__(64 * PW, D <= 6 ? 2 : 1) void mvdr_psd_kernel(
    const double2* __restrict__ obs, const MT* __restrict__ masks, double* __restrict__ part,
    int64_t B, int K, int M, int64_t T, int F, Plan plan) {
  __shared__ double2 ybuf[2][PW][D][64];
  TimeTile tt;
  if (!decode_time_tile(plan, B, K, T, F, tt)) return;
  // target: mask 0.  interference: mask 1 if given, else 1 - mask 0 (enhancer.py:236-250)
  const MT* mk0 = masks + ((tt.b * K + (tt.kvalid ? tt.k : 0)) * M) * T * F + tt.f;
  const MT* mk1 = mk0 + (M == 2 ? T * (int64_t)F : 0);
  const double2* y0 = obs + tt.b * D * T * F + tt.f;

  double diag[2][D];
  double2 off[2][D * (D - 1) / 2 + 1];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int i = 0; i < D; ++i) diag[m][i] = 0.0;
#pragma unroll
    for (int i = 0; i < D * (D - 1) / 2; ++i) off[m][i] = double2{0.0, 0.0};
  }
  auto fetch_m = [&](int s_, MaskRegs<MT>& r) {
    // unconditional loads (a branch per load would serialise them); frames past the chunk read
    // the last frame's mask and meet zero-filled Y
#pragma unroll
    for (int fr = 0; fr < PW; ++fr) {
      int64_t t = tt.t0 + (int64_t)s_ * PW + fr;
      t = t < tt.t1 ? t : tt.t1 - 1;
      r.w0[fr] = mk0[t * F];
      r.w1[fr] = mk1[t * F];
    }
  };
  auto compute = [&](int s_, const MaskRegs<MT>& r) {
#pragma unroll
    for (int fr = 0; fr < PW; ++fr) {
      double2 y[D];
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = ybuf[s_ & 1][fr][d][tt.lane];
      const double w0 = (double)r.w0[fr];
      const double w1 = M == 2 ? (double)r.w1[fr] : 1.0 - w0;
      // y_i conj(y_j) once, weighted into both accumulators
      int p = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double pd = y[i].x * y[i].x + y[i].y * y[i].y;
        diag[0][i] += w0 * pd;
        diag[1][i] += w1 * pd;
#pragma unroll
        for (int j = i + 1; j < D; ++j, ++p) {
          const double pr = y[i].x * y[j].x + y[i].y * y[j].y;
          const double pi = y[i].y * y[j].x - y[i].x * y[j].y;
          off[0][p].x += w0 * pr;
          off[0][p].y += w0 * pi;
          off[1][p].x += w1 * pr;
          off[1][p].y += w1 * pi;
        }
      }
    }
  };
  frame_pipeline<D, MaskRegs<MT>>(tt, ybuf, y0, T, F, fetch_m, compute);
  if (!tt.kvalid || tt.fraw >= F) return;
#pragma unroll
  for (int m = 0; m < 2; ++m)
    store_packed_herm<D>(
        part + ((((tt.b * plan.chunks + tt.c) * K + tt.k) * 2 + m) * (int64_t)(D * D)) * F + tt.f, F, diag[m], off[m]);
}

__device__ __forceinline__ double2 cmul(double2 a, double2 b) {
  return double2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x};
}
// component-wise select (a ?: on the struct type selects between ADDRESSES and pins both arrays
// in scratch memory)
__device__ __forceinline__ double2 sel(bool c, double2 a, double2 b) {
  return double2{c ? a.x : b.x, c ? a.y : b.y};
}
// 1 / a without forming |a|^2 (no spurious overflow / underflow)
__device__ __forceinline__ double2 crecip(double2 a) {
  if (fabs(a.x) >= fabs(a.y)) {
    const double r = a.y / a.x, den = a.x + a.y * r;
    return double2{1.0 / den, -r / den};
  }
  const double r = a.x / a.y, den = a.x * r + a.y;
  return double2{r / den, -1.0 / den};
}

// chunk partials -> chunk 0, in a fixed order (one lane per (b, k, m, element, bin))
__global__ __launch_bounds__(256) void mvdr_reduce_kernel(double* __restrict__ part, int64_t rows,
                                                          int F, int chunks, int64_t per_b) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;      // over B * per_b
  if (i >= rows * F) return;
  const int64_t b = i / per_b, r = i - b * per_b;
  double* p = part + b * chunks * per_b + r;
  double s = p[0];
  for (int c = 1; c < chunks; ++c) s += p[c * per_b];
  p[0] = s;
}

// Register-resident solve for D <= 6 (2 D^2 complex doubles per lane; every index is static after
// unrolling, row exchanges are selects).  Same arithmetic as mvdr_weights_kernel below.
template <int D>
__global__ __launch_bounds__(64) void mvdr_solve_kernel(
    const double* __restrict__ part, double2* __restrict__ wconj, int* __restrict__ info,
    int64_t B, int K, int F, int chunks, int ref, double eps, int info_per_k) {
  const int nf = (F + 63) / 64;
  const int ft = blockIdx.x % nf;
  const int k = (blockIdx.x / nf) % K;
  const int64_t b = blockIdx.x / ((int64_t)nf * K);
  const int f = ft * 64 + threadIdx.x;
  if (f >= F) return;
  constexpr int DD = D * D;
  double2 A[D][D], X[D][D];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const double* q = part + (((b * chunks) * K + k) * 2 + m) * (int64_t)DD * F + f;
    int p = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double v = q[(int64_t)i * F];
      if (m) A[i][i] = double2{v, 0.0}; else X[i][i] = double2{v, 0.0};
    }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i + 1; j < D; ++j, ++p) {
        const double re = q[(int64_t)(D + 2 * p) * F], im = q[(int64_t)(D + 2 * p + 1) * F];
        if (m) { A[i][j] = double2{re, im}; A[j][i] = double2{re, -im}; }
        else   { X[i][j] = double2{re, im}; X[j][i] = double2{re, -im}; }
      }
  }
  bool singular = false;
#pragma unroll
  for (int p = 0; p < D; ++p) {
    int piv = p;
    double best = fabs(A[p][p].x) + fabs(A[p][p].y);
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const double v = fabs(A[i][p].x) + fabs(A[i][p].y);
      if (v > best) { best = v; piv = i; }
    }
    if (best == 0.0) singular = true;
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const bool sw = piv == i;
#pragma unroll
      for (int j = p; j < D; ++j) {
        const double2 t = A[p][j], u = A[i][j];
        A[p][j] = sel(sw, u, t);
        A[i][j] = sel(sw, t, u);
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 t = X[p][j], u = X[i][j];
        X[p][j] = sel(sw, u, t);
        X[i][j] = sel(sw, t, u);
      }
    }
    const double2 r = crecip(A[p][p]);
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const double2 l = cmul(A[i][p], r);
#pragma unroll
      for (int j = p + 1; j < D; ++j) {
        const double2 a = A[p][j];
        A[i][j] = double2{A[i][j].x - (l.x * a.x - l.y * a.y), A[i][j].y - (l.x * a.y + l.y * a.x)};
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 a = X[p][j];
        X[i][j] = double2{X[i][j].x - (l.x * a.x - l.y * a.y), X[i][j].y - (l.x * a.y + l.y * a.x)};
      }
    }
  }
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    const double2 r = crecip(A[i][i]);
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double2 s = X[i][j];
#pragma unroll
      for (int q = i + 1; q < D; ++q) {
        const double2 a = A[i][q], x = X[q][j];
        s.x -= a.x * x.x - a.y * x.y;
        s.y -= a.x * x.y + a.y * x.x;
      }
      X[i][j] = cmul(s, r);
    }
  }
  if (singular) atomicAdd(info + k * info_per_k, 1);
  double lam = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) lam += X[i][i].x;
  if (lam < eps) lam = eps;
  const double scl = 1.0 / lam;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    double2 v = X[d][0];
#pragma unroll
    for (int c = 1; c < D; ++c) v = sel(ref == c, X[d][c], v);
    wconj[((b * K + k) * D + d) * (int64_t)F + f] = double2{v.x * scl, -(v.y * scl)};
  }
}

// General (D <= 8) solve with the systems in LDS; chunk partials already reduced (chunk 0).
__global__ __launch_bounds__(64) void mvdr_weights_kernel(
    const double* __restrict__ part, double2* __restrict__ wconj, int* __restrict__ info,
    int64_t B, int K, int D, int F, int chunks, int ref, double eps, int info_per_k) {
  extern __shared__ double2 sm[];
  const int lane = threadIdx.x;
  const int nf = (F + 63) / 64;
  const int ft = blockIdx.x % nf;
  const int k = (blockIdx.x / nf) % K;
  const int64_t b = blockIdx.x / ((int64_t)nf * K);
  const int f = ft * 64 + lane;
  if (f >= F) return;
  const int DD = D * D;
  double2* A = sm + lane;                    // interference psd, element e at A[e * 64]
  double2* Bm = sm + DD * 64 + lane;         // target psd -> phi
#define A_(i, j) A[((i) * D + (j)) * 64]
#define B_(i, j) Bm[((i) * D + (j)) * 64]
  for (int m = 0; m < 2; ++m) {
    int p = 0;
    for (int i = 0; i < D; ++i) {
      const double s = part[((((b * chunks) * K + k) * 2 + m) * (int64_t)DD + i) * F + f];
      if (m) A_(i, i) = double2{s, 0.0}; else B_(i, i) = double2{s, 0.0};
    }
    for (int i = 0; i < D; ++i)
      for (int j = i + 1; j < D; ++j, ++p) {
        const double* q = part + ((((b * chunks) * K + k) * 2 + m) * (int64_t)DD + D + 2 * p) * F + f;
        const double re = q[0], im = q[F];
        if (m) { A_(i, j) = double2{re, im}; A_(j, i) = double2{re, -im}; }
        else   { B_(i, j) = double2{re, im}; B_(j, i) = double2{re, -im}; }
      }
  }
  // ---- LU with partial pivoting on [A | B]  (zgetrf's pivot: first max of |re| + |im|)
  bool singular = false;
  for (int p = 0; p < D; ++p) {
    int piv = p;
    double best = fabs(A_(p, p).x) + fabs(A_(p, p).y);
    for (int i = p + 1; i < D; ++i) {
      const double v = fabs(A_(i, p).x) + fabs(A_(i, p).y);
      if (v > best) { best = v; piv = i; }
    }
    if (best == 0.0) singular = true;
    if (piv != p)
      for (int j = 0; j < D; ++j) {
        const double2 ta = A_(p, j); A_(p, j) = A_(piv, j); A_(piv, j) = ta;
        const double2 tb = B_(p, j); B_(p, j) = B_(piv, j); B_(piv, j) = tb;
      }
    const double2 r = crecip(A_(p, p));
    for (int i = p + 1; i < D; ++i) {
      const double2 l = cmul(A_(i, p), r);
      for (int j = p + 1; j < D; ++j) {
        const double2 a = A_(p, j), x = A_(i, j);
        A_(i, j) = double2{x.x - (l.x * a.x - l.y * a.y), x.y - (l.x * a.y + l.y * a.x)};
      }
      for (int j = 0; j < D; ++j) {
        const double2 a = B_(p, j), x = B_(i, j);
        B_(i, j) = double2{x.x - (l.x * a.x - l.y * a.y), x.y - (l.x * a.y + l.y * a.x)};
      }
    }
  }
  // ---- back substitution: phi overwrites B
  for (int i = D - 1; i >= 0; --i) {
    const double2 r = crecip(A_(i, i));
    for (int j = 0; j < D; ++j) {
      double2 s = B_(i, j);
      for (int q = i + 1; q < D; ++q) {
        const double2 a = A_(i, q), x = B_(q, j);
        s.x -= a.x * x.x - a.y * x.y;
        s.y -= a.x * x.y + a.y * x.x;
      }
      B_(i, j) = cmul(s, r);
    }
  }
  if (singular) atomicAdd(info + k * info_per_k, 1);
  double lam = 0.0;
  for (int i = 0; i < D; ++i) lam += B_(i, i).x;
  if (lam < eps) lam = eps;                       // clamp(min=eps); NaN stays NaN
  const double scl = 1.0 / lam;                   // complex / (real + 0i) the way torch divides
  for (int d = 0; d < D; ++d) {
    const double2 v = B_(d, ref);
    wconj[((b * K + k) * D + d) * (int64_t)F + f] = double2{v.x * scl, -(v.y * scl)};
  }
#undef A_
#undef B_
}

template <int D>
__global__ __launch_bounds__(64) void mvdr_apply_kernel(
    const double2* __restrict__ obs, const double2* __restrict__ wconj,
    const void* __restrict__ masks, int mask_f64, double2* __restrict__ enh, int64_t B, int K,
    int M, int64_t T, int F, int nf, int achunks, int64_t tchunk, int masking,
    double masking_eps) {
  const int groups = (K + KG - 1) / KG;
  int64_t tile;
  int grp;
  if (!xcd_tile(blockIdx.x, groups, B * achunks * nf, tile, grp)) return;
  const int ft = (int)(tile % nf);
  const int c = (int)((tile / nf) % achunks);
  const int64_t b = tile / ((int64_t)nf * achunks);
  const int f = ft * 64 + threadIdx.x;
  if (f >= F) return;
  const int k0 = grp * KG;
  const int nk = K - k0 < KG ? K - k0 : KG;
  double2 w[KG][D];
#pragma unroll
  for (int kk = 0; kk < KG; ++kk)
#pragma unroll
    for (int d = 0; d < D; ++d)
      w[kk][d] = kk < nk ? wconj[((b * K + k0 + kk) * D + d) * (int64_t)F + f] : double2{0.0, 0.0};
  const int64_t t0 = c * tchunk;
  const int64_t t1 = t0 + tchunk < T ? t0 + tchunk : T;
  const double2* y0 = obs + b * D * T * F + f;
#pragma unroll 2
  for (int64_t t = t0; t < t1; ++t) {
    double2 y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = y0[(d * T + t) * F];
#pragma unroll
    for (int kk = 0; kk < KG; ++kk) {
      if (kk >= nk) break;
      double2 e = {0.0, 0.0};
#pragma unroll
      for (int d = 0; d < D; ++d) {
        e.x += w[kk][d].x * y[d].x - w[kk][d].y * y[d].y;
        e.y += w[kk][d].x * y[d].y + w[kk][d].y * y[d].x;
      }
      if (masking) {
        double mk = load_mask(masks, mask_f64, (((b * K + k0 + kk) * M) * T + t) * F + f);
        if (mk < masking_eps) mk = masking_eps;
        e.x *= mk;
        e.y *= mk;
      }
      enh[((b * K + k0 + kk) * T + t) * F + f] = e;
    }
  }
}

template <int D>
int launch_psd(const double* obs, const void* masks, int mask_f64, double* part, int64_t B, int K,
               int M, int64_t T, int F, const Plan& p, hipStream_t s) {
  return launch_mt(mask_f64, masks, [&](auto* mk) {
    hipLaunchKernelGGL((mvdr_psd_kernel<D, mask_t<decltype(mk)>>), dim3((unsigned)time_grid(p, B, K)),
                       dim3(64 * PW), 0, s, reinterpret_cast<const double2*>(obs), mk, part, B, K, M, T, F, p);
  });
}

// Time chunks of an apply pass: about 4096 waves in all, 16 frames per chunk at the least
struct ApplyChunks { int64_t tchunk; int achunks; };
__host__ ApplyChunks apply_chunks(int64_t waves, int64_t T) {
  int64_t c = (4096 + waves - 1) / waves;
  const int64_t cmax = (T + 15) / 16;
  if (c > cmax) c = cmax;
  if (c < 1) c = 1;
  const int64_t tchunk = (T + c - 1) / c;
  return ApplyChunks{tchunk, (int)((T + tchunk - 1) / tchunk)};
}

template <int D>
int launch_apply(const double* obs, const double* wconj, const void* masks, int mask_f64,
                 double* enh, int64_t B, int K, int M, int64_t T, int F, int masking,
                 double masking_eps, hipStream_t s) {
  const int nf = (F + 63) / 64;
  const int groups = (K + KG - 1) / KG;
  const ApplyChunks a = apply_chunks(B * nf * groups, T);
  const int64_t grid = xcd_grid(B * a.achunks * nf, groups);
  hipLaunchKernelGGL(mvdr_apply_kernel<D>, dim3((unsigned)grid), dim3(64), 0, s,
                     reinterpret_cast<const double2*>(obs), reinterpret_cast<const double2*>(wconj),
                     masks, mask_f64, reinterpret_cast<double2*>(enh), B, K, M, T, F, nf, a.achunks,
                     a.tchunk, masking, masking_eps);
  return tssep_launch_status();
}

#define DISPATCH_D(D, CALL)                    \
  switch (D) {                                 \
    case 1: return CALL(1);                    \
    case 2: return CALL(2);                    \
    case 3: return CALL(3);                    \
    case 4: return CALL(4);                    \
    case 5: return CALL(5);                    \
    case 6: return CALL(6);                    \
    case 7: return CALL(7);                    \
    case 8: return CALL(8);                    \
    default: return TSSEP_E_UNSUPPORTED;       \
  }

bool shape_ok(int64_t B, int K, int M, int D, int64_t T, int F) {
  return B > 0 && K > 0 && T > 0 && F > 0 && D > 0 && (M == 1 || M == 2) &&
         B * K * 2 * ((F + 63) / 64) * ((T + 15) / 16 + 8) < (int64_t)1 << 28;
}

}  // namespace

extern "C" int64_t tssep_mvdr_partial_bytes(int64_t B, int K, int D, int64_t T, int F) {
  if (B <= 0 || K <= 0 || D <= 0 || D > MAXD || T <= 0 || F <= 0) return 0;
  const Plan p = make_plan(B, K, T, F);
  return B * p.chunks * K * 2 * (int64_t)(D * D) * F * (int64_t)sizeof(double);
}

extern "C" int tssep_mvdr_psd(const double* obs, const void* masks, int mask_f64, double* partials,
                              int64_t B, int K, int M, int D, int64_t T, int F, void* stream) {
  if (!obs || !masks || !partials) return TSSEP_E_NULL;
  if (!shape_ok(B, K, M, D, T, F)) return TSSEP_E_SHAPE;
  if (D > MAXD) return TSSEP_E_UNSUPPORTED;
  if (!aligned16(obs)) return TSSEP_E_ALIGN;
  const Plan p = make_plan(B, K, T, F);
#define CALL(DD) launch_psd<DD>(obs, masks, mask_f64, partials, B, K, M, T, F, p, (hipStream_t)stream)
  DISPATCH_D(D, CALL)
#undef CALL
}

template <int D>
int launch_solve(const double* part, double* wconj, int* info, int64_t B, int K, int F, int nf,
                 int chunks, int ref, double eps, hipStream_t s, int info_per_k = 0) {
  hipLaunchKernelGGL(mvdr_solve_kernel<D>, dim3((unsigned)(B * K * nf)), dim3(64), 0, s, part,
                     reinterpret_cast<double2*>(wconj), info, B, K, F, chunks, ref, eps, info_per_k);
  return tssep_launch_status();
}

// The per-bin solve of K systems per batch element out of (reduced) chunk 0 of `part`: in registers
// for D <= 6, in LDS for D = 7, 8.  info_per_k = 0: one counter of singular systems; 1: one per k.
static int solve_systems(const double* part, double* wconj, int* info, int64_t B, int K, int D, int F,
                  int nf, int chunks, int ref, double eps, int info_per_k, hipStream_t s) {
  switch (D) {
    case 1: return launch_solve<1>(part, wconj, info, B, K, F, nf, chunks, ref, eps, s, info_per_k);
    case 2: return launch_solve<2>(part, wconj, info, B, K, F, nf, chunks, ref, eps, s, info_per_k);
    case 3: return launch_solve<3>(part, wconj, info, B, K, F, nf, chunks, ref, eps, s, info_per_k);
    case 4: return launch_solve<4>(part, wconj, info, B, K, F, nf, chunks, ref, eps, s, info_per_k);
    case 5: return launch_solve<5>(part, wconj, info, B, K, F, nf, chunks, ref, eps, s, info_per_k);
    case 6: return launch_solve<6>(part, wconj, info, B, K, F, nf, chunks, ref, eps, s, info_per_k);
    default: break;
  }
  const size_t lds = (size_t)2 * D * D * 64 * sizeof(double2);
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(mvdr_weights_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            2 * MAXD * MAXD * 64 * (int)sizeof(double2)) != hipSuccess)
      return TSSEP_E_LAUNCH;
    attr_set = true;
  }
  hipLaunchKernelGGL(mvdr_weights_kernel, dim3((unsigned)(B * K * nf)), dim3(64), lds, s, part,
                     reinterpret_cast<double2*>(wconj), info, B, K, D, F, chunks, ref, eps,
                     info_per_k);
  return tssep_launch_status();
}

extern "C" int tssep_mvdr_weights(double* partials, double* wconj, int* info, int64_t B, int K,
                                  int D, int64_t T, int F, int reference_channel, double eps,
                                  void* stream) {
  if (!partials || !wconj || !info) return TSSEP_E_NULL;
  if (!shape_ok(B, K, 1, D, T, F) || reference_channel < 0 || reference_channel >= D)
    return TSSEP_E_SHAPE;
  if (D > MAXD) return TSSEP_E_UNSUPPORTED;
  if (!aligned16(wconj)) return TSSEP_E_ALIGN;
  const Plan p = make_plan(B, K, T, F);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(info, 0, sizeof(int), s) != hipSuccess) return TSSEP_E_LAUNCH;
  if (p.chunks > 1) {
    const int64_t rows = B * K * 2 * D * D;
    hipLaunchKernelGGL(mvdr_reduce_kernel, dim3((unsigned)((rows * F + 255) / 256)), dim3(256), 0, s,
                       partials, rows, F, p.chunks, (int64_t)K * 2 * D * D * F);
  }
  return solve_systems(partials, wconj, info, B, K, D, F, p.nf, p.chunks, reference_channel, eps, 0, s);
}

extern "C" int tssep_mvdr_apply(const double* obs, const double* wconj, const void* masks,
                                int mask_f64, double* enh, int64_t B, int K, int M, int D, int64_t T,
                                int F, int masking, double masking_eps, void* stream) {
  if (!obs || !wconj || !enh || (masking && !masks)) return TSSEP_E_NULL;
  if (!shape_ok(B, K, M, D, T, F)) return TSSEP_E_SHAPE;
  if (D > MAXD) return TSSEP_E_UNSUPPORTED;
  if (!aligned16(obs) || !aligned16(wconj) || !aligned16(enh)) return TSSEP_E_ALIGN;
#define CALL(DD) \
  launch_apply<DD>(obs, wconj, masks, mask_f64, enh, B, K, M, T, F, masking, masking_eps, (hipStream_t)stream)
  DISPATCH_D(D, CALL)
#undef CALL
}

extern "C" int64_t tssep_mvdr_workspace_bytes(int64_t B, int K, int D, int64_t T, int F) {
  const int64_t pb = tssep_mvdr_partial_bytes(B, K, D, T, F);
  if (pb == 0) return 0;
  return pb + B * K * D * (int64_t)F * 16 + 16;
}

extern "C" int tssep_mvdr_souden_fwd(const double* obs, const void* masks, int mask_f64, double* enh,
                                     void* workspace, int* info, int64_t B, int K, int M, int D,
                                     int64_t T, int F, int reference_channel, double eps, int masking,
                                     double masking_eps, void* stream) {
  if (!workspace) return TSSEP_E_NULL;
  if (!aligned16(workspace)) return TSSEP_E_ALIGN;
  const int64_t pb = tssep_mvdr_partial_bytes(B, K, D, T, F);
  if (pb == 0) return D > MAXD ? TSSEP_E_UNSUPPORTED : TSSEP_E_SHAPE;
  double* part = static_cast<double*>(workspace);
  double* wconj = reinterpret_cast<double*>(static_cast<char*>(workspace) + ((pb + 15) / 16) * 16);
  int st = tssep_mvdr_psd(obs, masks, mask_f64, part, B, K, M, D, T, F, stream);
  if (st != TSSEP_OK) return st;
  st = tssep_mvdr_weights(part, wconj, info, B, K, D, T, F, reference_channel, eps, stream);
  if (st != TSSEP_OK) return st;
  return tssep_mvdr_apply(obs, wconj, masks, mask_f64, enh, B, K, M, D, T, F, masking, masking_eps,
                          stream);
}

// ------------------------------------------------------------------ segment-wise MVDR ----
// ClassicBF_np.__call__ with segment_bf=True (tssep/train/enhancer.py:451-590): for every row
// (k, s, e) of a device segment table one Souden MVDR from the statistics of frames [s, e) only,
//   target weight      m_k ** mask_power
//   distortion weight  n_k ** mask_power,  n_k = max(sum_{j != k} m_j, eps)   (SumCrossTalker)
//                                          n_k = max(1 - m_k, 0)              (OneMinus)
//   psd = sum_t w Y Y^H / (e - s)   [real part only with psd_real: _get_psd, :281-288]
// applied to [s, e); every other (k, t) of the output is written as zero.  The distortion mask is
// formed in the mask's own dtype inside the statistics pass and never stored.  A constant number
// of launches whatever the table holds:
//   seg_map_kernel        (k, t) -> covering segment or -1, one thread per (k, t)
//   seg_psd_kernel<D,MT>  one wave per (64 bins, segment, one of C slices of the segment): both
//                         Hermitian accumulators per lane, slice partials to the workspace
//   seg_finalize_kernel   slice partials -> slice 0 in a fixed order, / (e - s), psd_real
//   mvdr_solve_kernel<D> / mvdr_weights_kernel   with "speakers" = segments, one info slot each
//   seg_info_kernel       the info slot of an ignored row back to zero
//   seg_apply_kernel<D>   one wave per (64 bins, time chunk, speaker); weights reloaded when the
//                         covering segment changes
// A row with k outside [0, K) or an empty [s, e) after clamping to [0, T] takes part in nothing
// but its own (zero) statistics: no access leaves the buffers whatever the table holds.
namespace {

struct Seg { int k, s, e; };
__device__ __forceinline__ Seg load_seg(const int32_t* __restrict__ tab, int i, int K, int64_t T) {
  Seg g{tab[3 * i], tab[3 * i + 1], tab[3 * i + 2]};
  if (g.s < 0) g.s = 0;
  if (g.e > (int)T) g.e = (int)T;
  if (g.k < 0 || g.k >= K || g.e < g.s) { g.k = 0; g.e = g.s = 0; }
  return g;
}

__host__ int seg_chunks(int S, int F) {
  const int64_t waves = (int64_t)S * ((F + 63) / 64);
  int64_t c = (4096 + waves - 1) / waves;
  return (int)(c < 1 ? 1 : c > 16 ? 16 : c);
}

__global__ __launch_bounds__(256) void seg_map_kernel(const int32_t* __restrict__ tab,
                                                      int32_t* __restrict__ map, int K, int S,
                                                      int64_t T) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= K * T) return;
  const int k = (int)(i / T), t = (int)(i - k * T);
  int hit = -1;
  for (int j = 0; j < S; ++j) {
    const int kk = tab[3 * j], s = tab[3 * j + 1], e = tab[3 * j + 2];
    if (kk == k && s <= t && t < e) hit = j;
  }
  map[i] = hit;
}

// The solve sees the zero statistics of an ignored row as a singular system; an ignored row reports nothing.
__global__ __launch_bounds__(256) void seg_info_kernel(const int32_t* __restrict__ tab,
                                                       int* __restrict__ info, int K, int S, int64_t T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= S) return;
  const Seg g = load_seg(tab, i, K, T);
  if (g.e <= g.s) info[i] = 0;
}

template <typename MT> __device__ __forceinline__ MT mask_pow(MT x, int ipow, double p) {
  if (ipow == 1) return x;
  if (ipow == 2) return x * x;
  return (MT)pow((double)x, p);
}
template <> __device__ __forceinline__ float mask_pow<float>(float x, int ipow, double p) {
  if (ipow == 1) return x;
  if (ipow == 2) return x * x;
  return powf(x, (float)p);
}

// PACKED: obs is the packed per-row observation [D, N, F] of the WPE stage (frame t of row sg at row0[sg] + t - s)
template <int D, typename MT, bool PACKED>
__global__ __launch_bounds__(64, D <= 6 ? 2 : 1) void seg_psd_kernel(
    const double2* __restrict__ obs, const MT* __restrict__ masks, const int32_t* __restrict__ tab,
    double* __restrict__ part, int K, int S, int64_t T, int F, int nf, int C, int mode,
    double dist_eps, int ipow, double mask_power, const int64_t* __restrict__ row0, int64_t N) {
  const int ft = blockIdx.x % nf;
  const int c = (blockIdx.x / nf) % C;
  const int sg = blockIdx.x / (nf * C);
  const Seg g = load_seg(tab, sg, K, T);
  const int lane = threadIdx.x;
  const int fraw = ft * 64 + lane;
  const int f = fraw < F ? fraw : F - 1;
  const int per = (g.e - g.s + C - 1) / C;
  const int t0 = g.s + c * per;
  const int t1 = t0 + per < g.e ? t0 + per : g.e;
  const MT deps = (MT)dist_eps;
  const int64_t TO = PACKED ? N : T;                       // frames of the observation buffer
  const int64_t shift = PACKED ? row0[sg] - g.s : 0;       // frame t -> row t + shift of it

  double diag[2][D];
  double2 off[2][D * (D - 1) / 2 + 1];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
#pragma unroll
    for (int i = 0; i < D; ++i) diag[m][i] = 0.0;
#pragma unroll
    for (int i = 0; i < D * (D - 1) / 2; ++i) off[m][i] = double2{0.0, 0.0};
  }
#pragma unroll 1
  for (int t = t0; t < t1; ++t) {
    double2 y[D];
    const int64_t to = PACKED ? (t + shift < 0 ? 0 : t + shift >= N ? N - 1 : t + shift) : t;
#pragma unroll
    for (int d = 0; d < D; ++d) y[d] = obs[((int64_t)d * TO + to) * F + f];
    const MT* mrow = masks + (int64_t)t * F + f;
    const MT tgt = mrow[(int64_t)g.k * T * F];
    MT dist;
    if (mode == 0) {
      // np.sum(np.delete(masks, k, axis=1), axis=1): ascending j without k, in the mask's dtype
      dist = (MT)0;
      for (int j = 0; j < K; ++j)
        if (j != g.k) dist += mrow[(int64_t)j * T * F];
      dist = dist > deps ? dist : deps;
    } else {
      dist = (MT)1 - tgt;
      dist = dist > (MT)0 ? dist : (MT)0;
    }
    const double w0 = (double)mask_pow<MT>(tgt, ipow, mask_power);
    const double w1 = (double)mask_pow<MT>(dist, ipow, mask_power);
    int p = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double pd = y[i].x * y[i].x + y[i].y * y[i].y;
      diag[0][i] += w0 * pd;
      diag[1][i] += w1 * pd;
#pragma unroll
      for (int j = i + 1; j < D; ++j, ++p) {
        const double pr = y[i].x * y[j].x + y[i].y * y[j].y;
        const double pi = y[i].y * y[j].x - y[i].x * y[j].y;
        off[0][p].x += w0 * pr;
        off[0][p].y += w0 * pi;
        off[1][p].x += w1 * pr;
        off[1][p].y += w1 * pi;
      }
    }
  }
  if (fraw >= F) return;
#pragma unroll
  for (int m = 0; m < 2; ++m)
    store_packed_herm<D>(part + ((((int64_t)c * S + sg) * 2 + m) * (int64_t)(D * D)) * F + f, F, diag[m], off[m]);
}

// slice partials -> slice 0, scaled by 1 / (e - s) the way numpy divides complex by real; with
// psd_real the imaginary slots become zero: (psd + swapaxes(psd, -2, -1)) / 2 of a Hermitian
// matrix is its real part (enhancer.py:288)
__global__ __launch_bounds__(256) void seg_finalize_kernel(double* __restrict__ part,
                                                           const int32_t* __restrict__ tab, int K,
                                                           int S, int D, int64_t T, int F, int C,
                                                           int psd_real) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_seg = (int64_t)2 * D * D * F;
  if (i >= S * per_seg) return;
  const int sg = (int)(i / per_seg);
  const int el = (int)((i - sg * per_seg) / F) % (D * D);
  const Seg g = load_seg(tab, sg, K, T);
  double s = part[i];
  for (int c = 1; c < C; ++c) s += part[c * S * per_seg + i];
  const int len = g.e - g.s;
  s = len > 0 ? s * (1.0 / (double)len) : 0.0;
  if (psd_real && el >= D && ((el - D) & 1)) s = 0.0;
  part[i] = s;
}

template <int D, typename MT, bool PACKED>
__global__ __launch_bounds__(64) void seg_apply_kernel(
    const double2* __restrict__ obs, const double2* __restrict__ wconj,
    const int32_t* __restrict__ map, const MT* __restrict__ masks, double2* __restrict__ enh, int K,
    int64_t T, int F, int nf, int achunks, int tchunk, int masking, double masking_eps,
    const int32_t* __restrict__ tab, const int64_t* __restrict__ row0, int64_t N) {
  // speaker fastest: the waves that read the same Y tile are neighbours in launch order
  const int k = blockIdx.x % K;
  const int ft = (blockIdx.x / K) % nf;
  const int c = blockIdx.x / (K * nf);
  const int f = ft * 64 + threadIdx.x;
  if (f >= F) return;
  const int t0 = c * tchunk;
  const int t1 = (int64_t)t0 + tchunk < T ? t0 + tchunk : (int)T;
  const MT meps = (MT)masking_eps;
  double2 w[D];
  int cur = -1;
  const int64_t TO = PACKED ? N : T;
  int64_t shift = 0;
  for (int t = t0; t < t1; ++t) {
    const int sg = __builtin_amdgcn_readfirstlane(map[(int64_t)k * T + t]);
    double2 e = {0.0, 0.0};
    if (sg >= 0) {
      if (sg != cur) {
#pragma unroll
        for (int d = 0; d < D; ++d) w[d] = wconj[((int64_t)sg * D + d) * F + f];
        cur = sg;
        if (PACKED) shift = row0[sg] - load_seg(tab, sg, K, T).s;
      }
      const int64_t to = PACKED ? (t + shift < 0 ? 0 : t + shift >= N ? N - 1 : t + shift) : t;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const double2 y = obs[((int64_t)d * TO + to) * F + f];
        e.x += w[d].x * y.x - w[d].y * y.y;
        e.y += w[d].x * y.y + w[d].y * y.x;
      }
      if (masking) {
        MT mk = masks[((int64_t)k * T + t) * F + f];
        mk = mk > meps ? mk : meps;
        e.x *= (double)mk;
        e.y *= (double)mk;
      }
    }
    enh[((int64_t)k * T + t) * F + f] = e;
  }
}

bool seg_shape_ok(int K, int S, int D, int64_t T, int F) {
  return K > 0 && S > 0 && D > 0 && T > 0 && F > 0 && T < ((int64_t)1 << 30) &&
         (int64_t)K * T < ((int64_t)1 << 31) && (int64_t)S * ((F + 63) / 64) * 16 < ((int64_t)1 << 30) &&
         (int64_t)S * 2 * D * D * F < ((int64_t)1 << 36);
}
int64_t seg_part_bytes(int S, int D, int F) {
  return (int64_t)seg_chunks(S, F) * S * 2 * D * D * F * (int64_t)sizeof(double);
}

template <int D, bool PACKED = false>
int launch_seg_psd(const double* obs, const void* masks, int mask_f64, const int32_t* tab,
                   double* part, int K, int S, int64_t T, int F, int mode, double dist_eps,
                   double mask_power, hipStream_t s, const int64_t* row0 = nullptr, int64_t N = 0) {
  const int nf = (F + 63) / 64, C = seg_chunks(S, F);
  const int ipow = mask_power == 1.0 ? 1 : mask_power == 2.0 ? 2 : 0;
  const dim3 grid((unsigned)((int64_t)S * C * nf));
  return launch_mt(mask_f64, masks, [&](auto* mk) {
    hipLaunchKernelGGL((seg_psd_kernel<D, mask_t<decltype(mk)>, PACKED>), grid, dim3(64), 0, s,
                       reinterpret_cast<const double2*>(obs), mk, tab, part, K, S, T, F, nf, C, mode,
                       dist_eps, ipow, mask_power, row0, N);
  });
}

template <int D, bool PACKED = false>
int launch_seg_apply(const double* obs, const double* wconj, const int32_t* map, const void* masks,
                     int mask_f64, double* enh, int K, int64_t T, int F, int masking,
                     double masking_eps, hipStream_t s, const int32_t* tab = nullptr,
                     const int64_t* row0 = nullptr, int64_t N = 0) {
  const int nf = (F + 63) / 64;
  const ApplyChunks a = apply_chunks((int64_t)nf * K, T);
  const dim3 grid((unsigned)((int64_t)a.achunks * nf * K));
  return launch_mt(mask_f64, masks, [&](auto* mk) {
    hipLaunchKernelGGL((seg_apply_kernel<D, mask_t<decltype(mk)>, PACKED>), grid, dim3(64), 0, s,
                       reinterpret_cast<const double2*>(obs), reinterpret_cast<const double2*>(wconj),
                       map, mk, reinterpret_cast<double2*>(enh), K, T, F, nf, a.achunks, (int)a.tchunk,
                       masking, masking_eps, tab, row0, N);
  });
}

}  // namespace

extern "C" int64_t tssep_mvdr_segments_workspace_bytes(int K, int S, int D, int64_t T, int F) {
  if (D > MAXD || !seg_shape_ok(K, S, D, T, F)) return 0;
  const int64_t pb = (seg_part_bytes(S, D, F) + 15) / 16 * 16;
  return pb + (int64_t)S * D * F * 16 + ((int64_t)K * T * 4 + 15) / 16 * 16;
}

namespace {

// row0 == nullptr: obs is [D, T, F]; else the packed [D, N, F] with row i at rows row0[i] .. row0[i + 1]
int seg_psd_stage(const double* obs, const void* masks, int mask_f64, const int32_t* segments, void* workspace,
                  int K, int S, int D, int64_t T, int F, int mode, double distortion_eps, double mask_power,
                  int psd_real, const int64_t* row0, int64_t N, void* stream) {
  if (!obs || !masks || !segments || !workspace) return TSSEP_E_NULL;
  if (!seg_shape_ok(K, S, D, T, F) || (mode != 0 && mode != 1) || !(mask_power > 0.0))
    return TSSEP_E_SHAPE;
  if (D > MAXD || (mode == 1 && K != 1)) return TSSEP_E_UNSUPPORTED;
  if (!aligned16(obs) || !aligned16(workspace)) return TSSEP_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
#define CALL(DD)                                                                                                \
  (row0 ? launch_seg_psd<DD, true>(obs, masks, mask_f64, segments, part, K, S, T, F, mode, distortion_eps,     \
                                   mask_power, s, row0, N)                                                     \
        : launch_seg_psd<DD>(obs, masks, mask_f64, segments, part, K, S, T, F, mode, distortion_eps, mask_power, s))
  const int st = [&]() -> int { DISPATCH_D(D, CALL) }();
#undef CALL
  if (st != TSSEP_OK) return st;
  const int64_t n = (int64_t)S * 2 * D * D * F;
  hipLaunchKernelGGL(seg_finalize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part,
                     segments, K, S, D, T, F, seg_chunks(S, F), psd_real);
  return tssep_launch_status();
}

int seg_fwd(const double* obs, const void* masks, int mask_f64, const int32_t* segments, double* enh,
            void* workspace, int* info, int K, int S, int D, int64_t T, int F, int mode, double distortion_eps,
            double mask_power, int psd_real, double eps, int masking, double masking_eps, const int64_t* row0,
            int64_t N, void* stream) {
  if (!enh || !info) return TSSEP_E_NULL;
  if (!aligned16(enh)) return TSSEP_E_ALIGN;
  int st = seg_psd_stage(obs, masks, mask_f64, segments, workspace, K, S, D, T, F, mode, distortion_eps,
                         mask_power, psd_real, row0, N, stream);
  if (st != TSSEP_OK) return st;
  hipStream_t s = (hipStream_t)stream;
  const int64_t pb = (seg_part_bytes(S, D, F) + 15) / 16 * 16;
  double* part = static_cast<double*>(workspace);
  double* wconj = reinterpret_cast<double*>(static_cast<char*>(workspace) + pb);
  int32_t* map = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + pb + (int64_t)S * D * F * 16);
  if (hipMemsetAsync(info, 0, sizeof(int) * (size_t)S, s) != hipSuccess) return TSSEP_E_LAUNCH;
  hipLaunchKernelGGL(seg_map_kernel, dim3((unsigned)(((int64_t)K * T + 255) / 256)), dim3(256), 0, s,
                     segments, map, K, S, T);
  st = tssep_launch_status();
  if (st != TSSEP_OK) return st;
  // reference channel 0 (bf_kwargs, enhancer.py:497-506); the segments stand where the speakers do
  st = solve_systems(part, wconj, info, 1, S, D, F, (F + 63) / 64, 1, 0, eps, 1, s);
  if (st != TSSEP_OK) return st;
  hipLaunchKernelGGL(seg_info_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, segments, info, K,
                     S, T);
  st = tssep_launch_status();
  if (st != TSSEP_OK) return st;
#define CALL(DD)                                                                                                  \
  (row0 ? launch_seg_apply<DD, true>(obs, wconj, map, masks, mask_f64, enh, K, T, F, masking, masking_eps, s,    \
                                     segments, row0, N)                                                          \
        : launch_seg_apply<DD>(obs, wconj, map, masks, mask_f64, enh, K, T, F, masking, masking_eps, s))
  DISPATCH_D(D, CALL)
#undef CALL
}

}  // namespace

extern "C" int tssep_mvdr_segments_psd(const double* obs, const void* masks, int mask_f64,
                                       const int32_t* segments, void* workspace, int K, int S, int D,
                                       int64_t T, int F, int mode, double distortion_eps,
                                       double mask_power, int psd_real, void* stream) {
  return seg_psd_stage(obs, masks, mask_f64, segments, workspace, K, S, D, T, F, mode, distortion_eps, mask_power,
                       psd_real, nullptr, 0, stream);
}

extern "C" int tssep_mvdr_segments_fwd(const double* obs, const void* masks, int mask_f64,
                                       const int32_t* segments, double* enh, void* workspace,
                                       int* info, int K, int S, int D, int64_t T, int F, int mode,
                                       double distortion_eps, double mask_power, int psd_real,
                                       double eps, int masking, double masking_eps, void* stream) {
  return seg_fwd(obs, masks, mask_f64, segments, enh, workspace, info, K, S, D, T, F, mode, distortion_eps,
                 mask_power, psd_real, eps, masking, masking_eps, nullptr, 0, stream);
}

extern "C" int tssep_mvdr_segments_fwd_obs(const double* obs_seg, const int64_t* row0, int64_t N,
                                           const void* masks, int mask_f64, const int32_t* segments,
                                           double* enh, void* workspace, int* info, int K, int S, int D,
                                           int64_t T, int F, int mode, double distortion_eps,
                                           double mask_power, int psd_real, double eps, int masking,
                                           double masking_eps, void* stream) {
  if (!row0) return TSSEP_E_NULL;
  if (N <= 0 || N >= ((int64_t)1 << 30)) return TSSEP_E_SHAPE;
  return seg_fwd(obs_seg, masks, mask_f64, segments, enh, workspace, info, K, S, D, T, F, mode, distortion_eps,
                 mask_power, psd_real, eps, masking, masking_eps, row0, N, stream);
}

// ------------------------------------------------------------------ backward of the Souden MVDR ----
// d(loss)/d(masks) of tssep_mvdr_souden_fwd for a given G = d(loss)/d(enh) (torch's convention for complex
// tensors); the observation gets no gradient.  Per (b, k, f), with P = Phi_n^-1 Phi_s, lam = Re tr P,
// c = max(lam, eps), e(t) = w^H y_t, g(t) = max(m_s(t), masking_eps) with masking, else 1:
//   gw  = sum_t conj(G(t) g(t)) y_t                                       mvdr_bwd_gw_kernel<D>, time pass 1
//   gP  = (gw / c) e_ref^T + gc I,  gc = -Re(gw^H P[:, ref]) / c^2 where lam >= eps, else 0
//   Z   = Phi_n^-H gP,  Hs = herm(Z),  Hn = herm(-Z P^H)                  mvdr_bwd_solve_kernel<D>
//   dm_s(t) = Re(y_t^H Hs y_t) [+ Re(conj(e(t)) G(t)) where m_s(t) >= masking_eps]
//   dm_n(t) = Re(y_t^H Hn y_t)         (M = 1: one matrix Hs - Hn)        mvdr_bwd_mask_kernel<D>, time pass 2
// Both time passes keep the forward's layout: lane = bin, one wave per (64 bins, time chunk, speaker), four
// speakers per workgroup sharing the Y frames through LDS, the chunks of make_plan.  The chunk partials of gw
// are added in chunk order by mvdr_reduce_kernel; pass 2 writes every element of dmask exactly once (the masking
// term is formed there, from the forward's wconj): no atomics, run-to-run identical.
// Saved between forward and backward: nothing but the forward's workspace -- the reduced statistics (chunk 0 of
// the partials) and wconj.  P and lam are NOT saved: the solve repeats the forward's elimination, the same
// operations in the same order.  That gives the forward's P to rounding, NOT bit for bit: which product of an
// a*b +- c*d the compiler contracts into an FMA is decided per kernel, not by the expression (at D = 2 the sum of two products in
// the back substitution's cmul(s, r) is fma(c, d, a * b) in mvdr_solve_kernel and fma(a, b, c * d) in
// mvdr_bwd_solve_kernel: profiles/mvdr_solve_contraction.txt; a body shared by both kernels still came out with
// one choice each).  A pivot or the clamp can therefore be decided the
// other way where two candidates, or lam and eps, lie within a rounding of each other.
namespace {

template <typename MT> struct GradRegs { double2 g[PW]; MT m[PW]; };

template <int D, typename MT>
__global__ __launch_bounds__(64 * PW, 2) void mvdr_bwd_gw_kernel(
    const double2* __restrict__ obs, const double2* __restrict__ genh, const MT* __restrict__ masks,
    double* __restrict__ part, int64_t B, int K, int M, int64_t T, int F, Plan plan, int masking,
    double masking_eps) {
  __shared__ double2 ybuf[2][PW][D][64];
  TimeTile tt;
  if (!decode_time_tile(plan, B, K, T, F, tt)) return;
  const int64_t bk = tt.b * K + (tt.kvalid ? tt.k : 0);
  const MT* mk0 = masks + (bk * M) * T * F + tt.f;           // only read with masking
  const double2* g0 = genh + bk * T * F + tt.f;
  const double2* y0 = obs + tt.b * D * T * F + tt.f;

  double2 acc[D];
#pragma unroll
  for (int d = 0; d < D; ++d) acc[d] = double2{0.0, 0.0};
  auto fetch_g = [&](int s_, GradRegs<MT>& r) {
    // frames past the chunk read the last frame's G and meet zero-filled Y
#pragma unroll
    for (int fr = 0; fr < PW; ++fr) {
      int64_t t = tt.t0 + (int64_t)s_ * PW + fr;
      t = t < tt.t1 ? t : tt.t1 - 1;
      r.g[fr] = g0[t * F];
      r.m[fr] = masking ? mk0[t * F] : (MT)1;
    }
  };
  auto compute = [&](int s_, const GradRegs<MT>& r) {
#pragma unroll
    for (int fr = 0; fr < PW; ++fr) {
      double2 g = r.g[fr];
      if (masking) {                                          // Ge = G max(m_s, masking_eps)
        double mk = (double)r.m[fr];
        if (mk < masking_eps) mk = masking_eps;
        g.x *= mk;
        g.y *= mk;
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {                           // conj(Ge) y_d
        const double2 y = ybuf[s_ & 1][fr][d][tt.lane];
        acc[d].x += g.x * y.x + g.y * y.y;
        acc[d].y += g.x * y.y - g.y * y.x;
      }
    }
  };
  frame_pipeline<D, GradRegs<MT>>(tt, ybuf, y0, T, F, fetch_g, compute);
  if (!tt.kvalid || tt.fraw >= F) return;
  double* out = part + (((tt.b * plan.chunks + tt.c) * K + tt.k) * (int64_t)(2 * D)) * F + tt.f;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    out[(int64_t)(2 * d) * F] = acc[d].x;
    out[(int64_t)(2 * d + 1) * F] = acc[d].y;
  }
}

// The three D x D complex matrices of one system: registers (every index static after unrolling) or LDS
// ([matrix][element][lane]).  Two matrices as in the forward pair would not do: P is needed next to the
// factors of Phi_n and Z.
constexpr bool bwd_in_registers(int D) { return D <= 6; }
constexpr int bwd_lanes(int D) {        // bins per workgroup: what 3 D^2 complex doubles per lane leave room for in 160 KB
  return bwd_in_registers(D) || 3 * D * D * 64 * 16 <= 160 * 1024 ? 64 : 32;
}
template <int D, bool REG, int LB> struct Sys3 {
  double2 r[REG ? 3 : 1][REG ? D : 1][REG ? D : 1];
  double2* s;
  __device__ __forceinline__ double2 get(int m, int i, int j) const {
    if constexpr (REG) return r[m][i][j]; else return s[((m * D + i) * D + j) * LB];
  }
  __device__ __forceinline__ void set(int m, int i, int j, double2 v) {
    if constexpr (REG) r[m][i][j] = v; else s[((m * D + i) * D + j) * LB] = v;
  }
};

// One lane per (b, k, bin).  part: the forward's partials with the chunk sums in chunk 0; gw: the reduced
// chunk 0 of pass 1; herm [B, K, M, D*D, F] packed Hermitian (M = 2: Hs, Hn; M = 1: Hs - Hn).
// Phi_n is read from its packed form and so is exactly Hermitian: Phi_n^H Z = gP is solved with the factors of
// Phi_n itself, the row exchanges and multipliers of the elimination recorded and replayed on gP.
// A singular system (the forward raises for those) divides by zero in its own lane only: Inf / NaN stay in the bin.
template <int D>
__global__ __launch_bounds__(64) void mvdr_bwd_solve_kernel(
    const double* __restrict__ part, const double* __restrict__ gw, double* __restrict__ herm,
    int64_t B, int K, int M, int F, int chunks, int ref, double eps) {
  constexpr bool REG = bwd_in_registers(D);
  constexpr int LB = bwd_lanes(D);
  constexpr int DD = D * D;
  extern __shared__ double2 sm[];
  const int lane = threadIdx.x;
  const int nfl = (F + LB - 1) / LB;
  const int ft = blockIdx.x % nfl;
  const int k = (blockIdx.x / nfl) % K;
  const int64_t b = blockIdx.x / ((int64_t)nfl * K);
  const int f = ft * LB + lane;
  if (lane >= LB || f >= F) return;
  Sys3<D, REG, LB> S;
  S.s = sm + lane;
  enum { A = 0, X = 1, Z = 2 };
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const double* q = part + (((b * chunks) * K + k) * 2 + m) * (int64_t)DD * F + f;
    const int dst = m ? A : X;
    int p = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) S.set(dst, i, i, double2{q[(int64_t)i * F], 0.0});
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = i + 1; j < D; ++j, ++p) {
        const double re = q[(int64_t)(D + 2 * p) * F], im = q[(int64_t)(D + 2 * p + 1) * F];
        S.set(dst, i, j, double2{re, im});
        S.set(dst, j, i, double2{re, -im});
      }
  }
  // ---- the forward's elimination of [A | X] (mvdr_solve_kernel), keeping the exchanges and the multipliers
  int pv[D];
#pragma unroll
  for (int p = 0; p < D; ++p) {
    int piv = p;
    double best = fabs(S.get(A, p, p).x) + fabs(S.get(A, p, p).y);
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const double2 a = S.get(A, i, p);
      const double v = fabs(a.x) + fabs(a.y);
      if (v > best) { best = v; piv = i; }
    }
    pv[p] = piv;
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const bool sw = piv == i;
#pragma unroll
      for (int j = p; j < D; ++j) {
        const double2 t = S.get(A, p, j), u = S.get(A, i, j);
        S.set(A, p, j, sel(sw, u, t));
        S.set(A, i, j, sel(sw, t, u));
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 t = S.get(X, p, j), u = S.get(X, i, j);
        S.set(X, p, j, sel(sw, u, t));
        S.set(X, i, j, sel(sw, t, u));
      }
    }
    const double2 r = crecip(S.get(A, p, p));
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const double2 l = cmul(S.get(A, i, p), r);
      S.set(A, i, p, l);                                      // kept for the replay on gP
#pragma unroll
      for (int j = p + 1; j < D; ++j) {
        const double2 a = S.get(A, p, j), x = S.get(A, i, j);
        S.set(A, i, j, double2{x.x - (l.x * a.x - l.y * a.y), x.y - (l.x * a.y + l.y * a.x)});
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 a = S.get(X, p, j), x = S.get(X, i, j);
        S.set(X, i, j, double2{x.x - (l.x * a.x - l.y * a.y), x.y - (l.x * a.y + l.y * a.x)});
      }
    }
  }
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    const double2 r = crecip(S.get(A, i, i));
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double2 s = S.get(X, i, j);
#pragma unroll
      for (int q = i + 1; q < D; ++q) {
        const double2 a = S.get(A, i, q), x = S.get(X, q, j);
        s.x -= a.x * x.x - a.y * x.y;
        s.y -= a.x * x.y + a.y * x.x;
      }
      S.set(X, i, j, cmul(s, r));                             // X holds P from here on
    }
  }
  double lam = 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i) lam += S.get(X, i, i).x;
  const bool open = lam >= eps;                               // the clamp passes the gradient at equality
  if (lam < eps) lam = eps;
  const double scl = 1.0 / lam;
  // ---- gP = (gw / c) e_ref^T + gc I
  const double* gq = gw + (((b * chunks) * K + k) * (int64_t)(2 * D)) * F + f;
  double2 u[D];
  double dot = 0.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double2 g = double2{gq[(int64_t)(2 * d) * F], gq[(int64_t)(2 * d + 1) * F]};
    double2 p = S.get(X, d, 0);
#pragma unroll
    for (int cc = 1; cc < D; ++cc) p = sel(ref == cc, S.get(X, d, cc), p);
    dot += g.x * p.x + g.y * p.y;                             // Re(conj(gw_d) P[d, ref])
    u[d] = double2{g.x * scl, g.y * scl};
  }
  const double gc = open ? -(dot * scl * scl) : 0.0;
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double2 v = sel(ref == j, u[i], double2{0.0, 0.0});
      if (i == j) v.x += gc;
      S.set(Z, i, j, v);
    }
  // ---- Z = A^-1 gP: the recorded exchanges and multipliers, then the back substitution
#pragma unroll
  for (int p = 0; p < D; ++p) {
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const bool sw = pv[p] == i;
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 t = S.get(Z, p, j), v = S.get(Z, i, j);
        S.set(Z, p, j, sel(sw, v, t));
        S.set(Z, i, j, sel(sw, t, v));
      }
    }
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const double2 l = S.get(A, i, p);
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 a = S.get(Z, p, j), x = S.get(Z, i, j);
        S.set(Z, i, j, double2{x.x - (l.x * a.x - l.y * a.y), x.y - (l.x * a.y + l.y * a.x)});
      }
    }
  }
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    const double2 r = crecip(S.get(A, i, i));
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double2 s = S.get(Z, i, j);
#pragma unroll
      for (int q = i + 1; q < D; ++q) {
        const double2 a = S.get(A, i, q), x = S.get(Z, q, j);
        s.x -= a.x * x.x - a.y * x.y;
        s.y -= a.x * x.y + a.y * x.x;
      }
      S.set(Z, i, j, cmul(s, r));
    }
  }
  // ---- Hs = herm(Z), Hn = herm(-Z P^H), an element at a time: W[i][j] = sum_q Z[i][q] conj(P[j][q])
  double* hs = herm + ((b * K + k) * M) * (int64_t)DD * F + f;
  double* hn = hs + (int64_t)DD * F;                          // M = 2 only
  auto zph = [&](int i, int j) {
    double2 w = {0.0, 0.0};
#pragma unroll
    for (int q = 0; q < D; ++q) {
      const double2 z = S.get(Z, i, q), p = S.get(X, j, q);
      w.x += z.x * p.x + z.y * p.y;
      w.y += z.y * p.x - z.x * p.y;
    }
    return w;
  };
  int p = 0;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const double s = S.get(Z, i, i).x, n = -zph(i, i).x;
    if (M == 2) { hs[(int64_t)i * F] = s; hn[(int64_t)i * F] = n; }
    else hs[(int64_t)i * F] = s - n;
  }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = i + 1; j < D; ++j, ++p) {
      const double2 a = S.get(Z, i, j), c = S.get(Z, j, i), wa = zph(i, j), wc = zph(j, i);
      const double2 s = {0.5 * (a.x + c.x), 0.5 * (a.y - c.y)};
      const double2 n = {-0.5 * (wa.x + wc.x), -0.5 * (wa.y - wc.y)};
      if (M == 2) {
        hs[(int64_t)(D + 2 * p) * F] = s.x;
        hs[(int64_t)(D + 2 * p + 1) * F] = s.y;
        hn[(int64_t)(D + 2 * p) * F] = n.x;
        hn[(int64_t)(D + 2 * p + 1) * F] = n.y;
      } else {
        hs[(int64_t)(D + 2 * p) * F] = s.x - n.x;
        hs[(int64_t)(D + 2 * p + 1) * F] = s.y - n.y;
      }
    }
}

// Time pass 2: q_H(t) = Re(y^H H y) = sum_i H_ii |y_i|^2 + 2 sum_{i<j} (Re H_ij Re(y_i conj y_j) + Im H_ij Im(y_i conj y_j))
// -- the products of the statistics pass, contracted with one (M = 1) or two (M = 2) Hermitian matrices per lane.
// 2 D^2 doubles of matrices, D weights and the D frame values per lane: 256 registers (two workgroups per CU) hold
// that up to D = 5; D = 6 spilled 290 bytes per lane there, so from D = 6 on a workgroup has the CU to itself.
template <int D, typename MT>
__global__ __launch_bounds__(64 * PW, D <= 5 ? 2 : 1) void mvdr_bwd_mask_kernel(
    const double2* __restrict__ obs, const double2* __restrict__ genh, const double2* __restrict__ wconj,
    const double* __restrict__ herm, const MT* __restrict__ masks, MT* __restrict__ dmask, int64_t B, int K,
    int M, int64_t T, int F, Plan plan, int masking, double masking_eps) {
  __shared__ double2 ybuf[2][PW][D][64];
  constexpr int NP = D * (D - 1) / 2;
  const int groups = (K + PW - 1) / PW;
  int64_t tile;
  int grp;
  if (!xcd_tile(blockIdx.x, groups, B * plan.chunks * plan.nf, tile, grp)) return;
  const int ft = (int)(tile % plan.nf);
  const int c = (int)((tile / plan.nf) % plan.chunks);
  const int64_t b = tile / ((int64_t)plan.nf * plan.chunks);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k = grp * PW + wave;
  const bool kvalid = k < K;
  const int fraw = ft * 64 + lane;
  const int f = fraw < F ? fraw : F - 1;
  const int64_t t0 = c * plan.tchunk;
  const int64_t t1 = t0 + plan.tchunk < T ? t0 + plan.tchunk : T;
  const int steps = (int)((t1 - t0 + PW - 1) / PW);
  const int64_t bk = b * K + (kvalid ? k : 0);
  const MT* mk0 = masks + (bk * M) * T * F + f;              // only read with masking
  const double2* g0 = genh + bk * T * F + f;                 // only read with masking
  const double2* y0 = obs + b * D * T * F + f;
  MT* dm0 = dmask + (bk * M) * T * F + f;

  double hd[2][D];
  double2 ho[2][NP + 1];
  double2 w[D];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const double* q = herm + ((bk * M) + (m < M ? m : 0)) * (int64_t)(D * D) * F + f;
#pragma unroll
    for (int i = 0; i < D; ++i) hd[m][i] = q[(int64_t)i * F];
#pragma unroll
    for (int p = 0; p < NP; ++p) ho[m][p] = double2{q[(int64_t)(D + 2 * p) * F], q[(int64_t)(D + 2 * p + 1) * F]};
  }
#pragma unroll
  for (int d = 0; d < D; ++d) w[d] = masking ? wconj[(bk * D + d) * (int64_t)F + f] : double2{0.0, 0.0};

  auto fetch_y = [&](int s_) {
    const int64_t t = t0 + (int64_t)s_ * PW + wave;
    if (t < t1) {
#pragma unroll
      for (int d = 0; d < D; ++d)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(y0 + (d * T + t) * F),
            (__attribute__((address_space(3))) void*)&ybuf[s_ & 1][wave][d][0], 16, 0, 0);
    } else {
#pragma unroll
      for (int d = 0; d < D; ++d) ybuf[s_ & 1][wave][d][lane] = double2{0.0, 0.0};
    }
  };
  auto fetch_g = [&](int s_, GradRegs<MT>& r) {
    if (!masking) return;
#pragma unroll
    for (int fr = 0; fr < PW; ++fr) {
      int64_t tt = t0 + (int64_t)s_ * PW + fr;
      tt = tt < t1 ? tt : t1 - 1;
      r.g[fr] = g0[tt * F];
      r.m[fr] = mk0[tt * F];
    }
  };
  auto compute = [&](int s_, const GradRegs<MT>& r) {
#pragma unroll
    for (int fr = 0; fr < PW; ++fr) {
      const int64_t t = t0 + (int64_t)s_ * PW + fr;
      if (t >= t1) break;
      double2 y[D];
#pragma unroll
      for (int d = 0; d < D; ++d) y[d] = ybuf[s_ & 1][fr][d][lane];
      double qd[2] = {0.0, 0.0}, qo[2] = {0.0, 0.0};
      int p = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double pd = y[i].x * y[i].x + y[i].y * y[i].y;
        qd[0] += hd[0][i] * pd;
        qd[1] += hd[1][i] * pd;
#pragma unroll
        for (int j = i + 1; j < D; ++j, ++p) {
          const double pr = y[i].x * y[j].x + y[i].y * y[j].y;
          const double pi = y[i].y * y[j].x - y[i].x * y[j].y;
          qo[0] += ho[0][p].x * pr + ho[0][p].y * pi;
          qo[1] += ho[1][p].x * pr + ho[1][p].y * pi;
        }
      }
      double q0 = qd[0] + 2.0 * qo[0];
      const double q1 = qd[1] + 2.0 * qo[1];
      if (masking && (double)r.m[fr] >= masking_eps) {        // d max(m, eps) / dm = 1 at equality too (torch.clamp)
        double2 e = {0.0, 0.0};
#pragma unroll
        for (int d = 0; d < D; ++d) {
          e.x += w[d].x * y[d].x - w[d].y * y[d].y;
          e.y += w[d].x * y[d].y + w[d].y * y[d].x;
        }
        q0 += e.x * r.g[fr].x + e.y * r.g[fr].y;              // Re(conj(e) G)
      }
      if (fraw < F) {
        dm0[t * F] = (MT)q0;
        if (M == 2) dm0[(T + t) * F] = (MT)q1;
      }
    }
  };
  GradRegs<MT> ra, rb;
  fetch_y(0);
  fetch_g(0, ra);
  for (int s = 0; s < steps; s += 2) {
    __syncthreads();
    if (s + 1 < steps) { fetch_y(s + 1); fetch_g(s + 1, rb); }
    if (kvalid) compute(s, ra);
    if (s + 1 >= steps) break;
    __syncthreads();
    if (s + 2 < steps) { fetch_y(s + 2); fetch_g(s + 2, ra); }
    if (kvalid) compute(s + 1, rb);
  }
}

int64_t bwd_gw_bytes(int64_t B, int K, int D, const Plan& p, int F) {
  return ((B * p.chunks * K * 2 * D * (int64_t)F * (int64_t)sizeof(double)) + 15) / 16 * 16;
}

template <int D>
int launch_bwd_gw(const double* obs, const double* genh, const void* masks, int mask_f64, double* part, int64_t B,
                  int K, int M, int64_t T, int F, const Plan& p, int masking, double masking_eps, hipStream_t s) {
  return launch_mt(mask_f64, masks, [&](auto* mk) {
    hipLaunchKernelGGL((mvdr_bwd_gw_kernel<D, mask_t<decltype(mk)>>), dim3((unsigned)time_grid(p, B, K)),
                       dim3(64 * PW), 0, s, reinterpret_cast<const double2*>(obs),
                       reinterpret_cast<const double2*>(genh), mk, part, B, K, M, T, F, p, masking, masking_eps);
  });
}

template <int D>
int launch_bwd_solve(const double* part, const double* gw, double* herm, int64_t B, int K, int M, int F, int chunks,
                     int ref, double eps, hipStream_t s) {
  constexpr int LB = bwd_lanes(D);
  constexpr size_t lds = bwd_in_registers(D) ? 0 : (size_t)3 * D * D * LB * sizeof(double2);
  if (lds > 0) {
    static bool attr_set = false;
    if (!attr_set) {
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(mvdr_bwd_solve_kernel<D>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return TSSEP_E_LAUNCH;
      attr_set = true;
    }
  }
  const int nfl = (F + LB - 1) / LB;
  hipLaunchKernelGGL(mvdr_bwd_solve_kernel<D>, dim3((unsigned)(B * K * nfl)), dim3(64), lds, s, part, gw, herm, B, K,
                     M, F, chunks, ref, eps);
  return tssep_launch_status();
}

template <int D>
int launch_bwd_mask(const double* obs, const double* genh, const double* wconj, const double* herm, const void* masks,
                    int mask_f64, void* dmask, int64_t B, int K, int M, int64_t T, int F, const Plan& p, int masking,
                    double masking_eps, hipStream_t s) {
  return launch_mt(mask_f64, masks, [&](auto* mk) {
    using MT = mask_t<decltype(mk)>;
    hipLaunchKernelGGL((mvdr_bwd_mask_kernel<D, MT>), dim3((unsigned)time_grid(p, B, K)), dim3(64 * PW), 0, s,
                       reinterpret_cast<const double2*>(obs), reinterpret_cast<const double2*>(genh),
                       reinterpret_cast<const double2*>(wconj), herm, mk, static_cast<MT*>(dmask), B, K, M, T, F, p,
                       masking, masking_eps);
  });
}

}  // namespace

extern "C" int64_t tssep_mvdr_bwd_workspace_bytes(int64_t B, int K, int M, int D, int64_t T, int F) {
  if (D > MAXD || !shape_ok(B, K, M, D, T, F)) return 0;
  const Plan p = make_plan(B, K, T, F);
  return bwd_gw_bytes(B, K, D, p, F) + B * K * M * (int64_t)(D * D) * F * (int64_t)sizeof(double);
}

extern "C" int tssep_mvdr_bwd_gw(const double* obs, const double* genh, const void* masks, int mask_f64,
                                 double* gw_partials, int64_t B, int K, int M, int D, int64_t T, int F, int masking,
                                 double masking_eps, void* stream) {
  if (!obs || !genh || !gw_partials || (masking && !masks)) return TSSEP_E_NULL;
  if (!shape_ok(B, K, M, D, T, F)) return TSSEP_E_SHAPE;
  if (D > MAXD) return TSSEP_E_UNSUPPORTED;
  if (!aligned16(obs) || !aligned16(genh)) return TSSEP_E_ALIGN;
  const Plan p = make_plan(B, K, T, F);
#define CALL(DD) \
  launch_bwd_gw<DD>(obs, genh, masks, mask_f64, gw_partials, B, K, M, T, F, p, masking, masking_eps, (hipStream_t)stream)
  DISPATCH_D(D, CALL)
#undef CALL
}

extern "C" int tssep_mvdr_bwd_solve(const double* fwd_partials, double* gw_partials, double* herm, int64_t B, int K,
                                    int M, int D, int64_t T, int F, int reference_channel, double eps, void* stream) {
  if (!fwd_partials || !gw_partials || !herm) return TSSEP_E_NULL;
  if (!shape_ok(B, K, M, D, T, F) || reference_channel < 0 || reference_channel >= D) return TSSEP_E_SHAPE;
  if (D > MAXD) return TSSEP_E_UNSUPPORTED;
  const Plan p = make_plan(B, K, T, F);
  hipStream_t s = (hipStream_t)stream;
  if (p.chunks > 1) {
    // the forward's reducer: rows of F doubles, per_b doubles per (batch element, chunk)
    const int64_t rows = B * K * 2 * D;
    hipLaunchKernelGGL(mvdr_reduce_kernel, dim3((unsigned)((rows * F + 255) / 256)), dim3(256), 0, s, gw_partials,
                       rows, F, p.chunks, (int64_t)K * 2 * D * F);
    const int st = tssep_launch_status();
    if (st != TSSEP_OK) return st;
  }
#define CALL(DD) \
  launch_bwd_solve<DD>(fwd_partials, gw_partials, herm, B, K, M, F, p.chunks, reference_channel, eps, s)
  DISPATCH_D(D, CALL)
#undef CALL
}

extern "C" int tssep_mvdr_bwd_mask(const double* obs, const double* genh, const double* wconj, const double* herm,
                                   const void* masks, int mask_f64, void* dmask, int64_t B, int K, int M, int D,
                                   int64_t T, int F, int masking, double masking_eps, void* stream) {
  if (!obs || !herm || !dmask || (masking && (!masks || !genh || !wconj))) return TSSEP_E_NULL;
  if (!shape_ok(B, K, M, D, T, F)) return TSSEP_E_SHAPE;
  if (D > MAXD) return TSSEP_E_UNSUPPORTED;
  if (!aligned16(obs) || (masking && (!aligned16(genh) || !aligned16(wconj)))) return TSSEP_E_ALIGN;
  const Plan p = make_plan(B, K, T, F);
#define CALL(DD)                                                                                              \
  launch_bwd_mask<DD>(obs, genh, wconj, herm, masks, mask_f64, dmask, B, K, M, T, F, p, masking, masking_eps, \
                      (hipStream_t)stream)
  DISPATCH_D(D, CALL)
#undef CALL
}

extern "C" int tssep_mvdr_souden_bwd(const double* obs, const void* masks, int mask_f64, const double* genh,
                                     const void* fwd_workspace, void* bwd_workspace, void* dmask, int64_t B, int K,
                                     int M, int D, int64_t T, int F, int reference_channel, double eps, int masking,
                                     double masking_eps, void* stream) {
  if (!fwd_workspace || !bwd_workspace) return TSSEP_E_NULL;
  if (!aligned16(fwd_workspace) || !aligned16(bwd_workspace)) return TSSEP_E_ALIGN;
  const int64_t pb = tssep_mvdr_partial_bytes(B, K, D, T, F);
  if (pb == 0 || !shape_ok(B, K, M, D, T, F)) return D > MAXD ? TSSEP_E_UNSUPPORTED : TSSEP_E_SHAPE;
  const double* part = static_cast<const double*>(fwd_workspace);
  const double* wconj = reinterpret_cast<const double*>(static_cast<const char*>(fwd_workspace) + ((pb + 15) / 16) * 16);
  double* gwp = static_cast<double*>(bwd_workspace);
  double* herm = reinterpret_cast<double*>(static_cast<char*>(bwd_workspace) + bwd_gw_bytes(B, K, D, make_plan(B, K, T, F), F));
  int st = tssep_mvdr_bwd_gw(obs, genh, masks, mask_f64, gwp, B, K, M, D, T, F, masking, masking_eps, stream);
  if (st != TSSEP_OK) return st;
  st = tssep_mvdr_bwd_solve(part, gwp, herm, B, K, M, D, T, F, reference_channel, eps, stream);
  if (st != TSSEP_OK) return st;
  return tssep_mvdr_bwd_mask(obs, genh, wconj, herm, masks, mask_f64, dmask, B, K, M, D, T, F, masking, masking_eps,
                             stream);
}

// ------------------------------------------------------------------ online (frame-recursive) MVDR ----
// This project's own (the reference has no online mode).  Per (b, speaker k, bin f), frame by frame:
//   Phi_s = alpha Phi_s + m y y^H        Phi_n = alpha Phi_n + (1 - m) y y^H        l = delta Re tr(Phi_s + Phi_n) / D
//   phi   = solve(Phi_n + l I, Phi_s)    w = phi[:, ref] / max(Re tr phi, eps)      enh = w^H y  (* max(m, masking_eps))
// The filter of frame t is made of the statistics up to and including t.  With alpha = 1, delta = 0 the filter of the
// last frame is the one tssep_mvdr_souden_fwd applies to the whole utterance.  While the trace is exactly zero (digital
// silence since the stream began) the output is zero and nothing is solved.  A frame whose loaded Phi_n is singular
// (delta = 0 in front of frame D - 1) leaves Inf / NaN in its own output element only: the statistics never read phi.
// One launch does all T frames of a call: one wave per (b, k, 64 bins), lane = bin, the two packed Hermitian
// accumulators in registers across the frame loop -- read from state_in (NULL: zeros) at entry, written to state_out at
// exit -- and one step per frame in a fixed order, so the result is the same however the frames are split over calls.
// The K waves of a (b, 64 bins) tile read the same Y frames: xcd_tile places them on one XCD, whose L2 serves the
// tile after the first of them fetched it (a per-step workgroup barrier for an LDS hand-over would sit in a sequential
// chain of a few microseconds per frame to save 16 D bytes per lane, and D = 7, 8 need the LDS of a CU for one wave).
namespace {

// [A | X] -> X = A^-1 X on matrices 0 (A) and 1 (X) of a Sys3: the elimination of mvdr_solve_kernel / mvdr_bwd_solve_kernel
// (first maximum of |re| + |im| down the column, exchanges as selects, crecip of the pivot, rows top to bottom), in
// registers or on the LDS [element][lane] layout, whatever S is.  A zero pivot divides by zero in its own lane.
template <int D, typename S> __device__ __forceinline__ void lu_solve(S& s) {
  enum { A = 0, X = 1 };
#pragma unroll
  for (int p = 0; p < D; ++p) {
    int piv = p;
    double best = fabs(s.get(A, p, p).x) + fabs(s.get(A, p, p).y);
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const double2 a = s.get(A, i, p);
      const double v = fabs(a.x) + fabs(a.y);
      if (v > best) { best = v; piv = i; }
    }
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const bool sw = piv == i;
#pragma unroll
      for (int j = p; j < D; ++j) {
        const double2 t = s.get(A, p, j), u = s.get(A, i, j);
        s.set(A, p, j, sel(sw, u, t));
        s.set(A, i, j, sel(sw, t, u));
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 t = s.get(X, p, j), u = s.get(X, i, j);
        s.set(X, p, j, sel(sw, u, t));
        s.set(X, i, j, sel(sw, t, u));
      }
    }
    const double2 r = crecip(s.get(A, p, p));
#pragma unroll
    for (int i = p + 1; i < D; ++i) {
      const double2 l = cmul(s.get(A, i, p), r);
#pragma unroll
      for (int j = p + 1; j < D; ++j) {
        const double2 a = s.get(A, p, j), x = s.get(A, i, j);
        s.set(A, i, j, double2{x.x - (l.x * a.x - l.y * a.y), x.y - (l.x * a.y + l.y * a.x)});
      }
#pragma unroll
      for (int j = 0; j < D; ++j) {
        const double2 a = s.get(X, p, j), x = s.get(X, i, j);
        s.set(X, i, j, double2{x.x - (l.x * a.x - l.y * a.y), x.y - (l.x * a.y + l.y * a.x)});
      }
    }
  }
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
    const double2 r = crecip(s.get(A, i, i));
#pragma unroll
    for (int j = 0; j < D; ++j) {
      double2 acc = s.get(X, i, j);
#pragma unroll
      for (int q = i + 1; q < D; ++q) {
        const double2 a = s.get(A, i, q), x = s.get(X, q, j);
        acc.x -= a.x * x.x - a.y * x.y;
        acc.y -= a.x * x.y + a.y * x.x;
      }
      s.set(X, i, j, cmul(acc, r));
    }
  }
}

constexpr size_t online_lds(int D) { return bwd_in_registers(D) ? 0 : (size_t)2 * D * D * 64 * sizeof(double2); }

// obs [B,D,T,F] complex128 (obs_f64) or complex64; masks [B,K,T,F]; state [B,K,2,D*D,F] packed Hermitian (0: Phi_s,
// 1: Phi_n); enh [B,K,T,F] complex128.  state_in may be state_out: a lane reads its elements before it writes them.
template <int D, typename MT>
__global__ __launch_bounds__(64) void mvdr_online_kernel(
    const void* __restrict__ obs, int obs_f64, const MT* __restrict__ masks, const double* state_in, double* state_out,
    double2* __restrict__ enh, int64_t B, int K, int64_t T, int F, int ref, double alpha, double delta, double eps,
    int masking, double masking_eps) {
  constexpr bool REG = bwd_in_registers(D);
  constexpr int DD = D * D, NP = D * (D - 1) / 2;
  extern __shared__ double2 sm[];
  const int nf = (F + 63) / 64;
  int64_t tile;
  int k;
  if (!xcd_tile(blockIdx.x, K, B * nf, tile, k)) return;
  const int64_t b = tile / nf;
  const int f = (int)(tile % nf) * 64 + (int)threadIdx.x;
  if (f >= F) return;                                      // (one wave, no barrier, LDS columns are per lane)
  const int64_t bk = b * K + k;

  double diag[2][D];
  double2 off[2][NP + 1];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const double* q = state_in ? state_in + (bk * 2 + m) * (int64_t)DD * F + f : nullptr;
#pragma unroll
    for (int i = 0; i < D; ++i) diag[m][i] = q ? q[(int64_t)i * F] : 0.0;
#pragma unroll
    for (int p = 0; p < NP; ++p)
      off[m][p] = q ? double2{q[(int64_t)(D + 2 * p) * F], q[(int64_t)(D + 2 * p + 1) * F]} : double2{0.0, 0.0};
  }
  const MT* mk = masks + bk * T * F + f;
  double2* out = enh + bk * T * F + f;
  const int64_t y0 = b * D * T * F + f;
  Sys3<D, REG, 64> S;
  S.s = sm + threadIdx.x;
  enum { A = 0, X = 1 };

#pragma unroll 1
  for (int64_t t = 0; t < T; ++t) {
    double2 y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int64_t i = y0 + (d * T + t) * F;
      if (obs_f64) {
        y[d] = static_cast<const double2*>(obs)[i];
      } else {
        const float2 v = static_cast<const float2*>(obs)[i];
        y[d] = double2{(double)v.x, (double)v.y};
      }
    }
    const double w0 = (double)mk[t * F];
    const double w1 = 1.0 - w0;
    // the statistics pass's products y_i conj(y_j), behind the forgetting factor
    double tr = 0.0;
    int p = 0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const double pd = y[i].x * y[i].x + y[i].y * y[i].y;
      diag[0][i] = alpha * diag[0][i] + w0 * pd;
      diag[1][i] = alpha * diag[1][i] + w1 * pd;
      tr += diag[0][i] + diag[1][i];
#pragma unroll
      for (int j = i + 1; j < D; ++j, ++p) {
        const double pr = y[i].x * y[j].x + y[i].y * y[j].y;
        const double pi = y[i].y * y[j].x - y[i].x * y[j].y;
        off[0][p].x = alpha * off[0][p].x + w0 * pr;
        off[0][p].y = alpha * off[0][p].y + w0 * pi;
        off[1][p].x = alpha * off[1][p].x + w1 * pr;
        off[1][p].y = alpha * off[1][p].y + w1 * pi;
      }
    }
    double2 e = {0.0, 0.0};
    if (tr != 0.0) {                                       // (a NaN trace goes through the solve and stays NaN)
      const double load = delta * tr / (double)D;
      p = 0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        S.set(A, i, i, double2{diag[1][i] + load, 0.0});
        S.set(X, i, i, double2{diag[0][i], 0.0});
#pragma unroll
        for (int j = i + 1; j < D; ++j, ++p) {
          S.set(A, i, j, off[1][p]);
          S.set(A, j, i, double2{off[1][p].x, -off[1][p].y});
          S.set(X, i, j, off[0][p]);
          S.set(X, j, i, double2{off[0][p].x, -off[0][p].y});
        }
      }
      lu_solve<D>(S);
      double lam = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) lam += S.get(X, i, i).x;
      if (lam < eps) lam = eps;
      const double scl = 1.0 / lam;
#pragma unroll
      for (int d = 0; d < D; ++d) {
        double2 v = S.get(X, d, 0);
#pragma unroll
        for (int c = 1; c < D; ++c) v = sel(ref == c, S.get(X, d, c), v);
        const double2 w = {v.x * scl, -(v.y * scl)};       // conj(w_d), as mvdr_apply_kernel takes it
        e.x += w.x * y[d].x - w.y * y[d].y;
        e.y += w.x * y[d].y + w.y * y[d].x;
      }
      if (masking) {
        double g = w0;
        if (g < masking_eps) g = masking_eps;
        e.x *= g;
        e.y *= g;
      }
    }
    out[t * F] = e;
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
    store_packed_herm<D>(state_out + (bk * 2 + m) * (int64_t)DD * F + f, F, diag[m], off[m]);
}

template <int D>
int launch_online(const void* obs, int obs_f64, const void* masks, int mask_f64, const double* state_in,
                  double* state_out, double* enh, int64_t B, int K, int64_t T, int F, int ref, double alpha,
                  double delta, double eps, int masking, double masking_eps, hipStream_t s) {
  const int64_t grid = xcd_grid(B * ((F + 63) / 64), K);
  int attr = TSSEP_OK;
  const int st = launch_mt(mask_f64, masks, [&](auto* mk) {
    auto kernel = mvdr_online_kernel<D, mask_t<decltype(mk)>>;
    if (online_lds(D) > 64 * 1024) {                       // D = 7, 8: more than the default 64 KB of dynamic LDS
      static bool attr_set = false;                        // (one per instantiation of this lambda)
      if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)online_lds(D)) != hipSuccess) {
          attr = TSSEP_E_LAUNCH;
          return;
        }
        attr_set = true;
      }
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64), online_lds(D), s, obs, obs_f64, mk, state_in,
                       state_out, reinterpret_cast<double2*>(enh), B, K, T, F, ref, alpha, delta, eps, masking,
                       masking_eps);
  });
  return attr != TSSEP_OK ? attr : st;
}

}  // namespace

extern "C" int64_t tssep_mvdr_online_state_bytes(int64_t B, int K, int D, int F) {
  if (B <= 0 || K <= 0 || D <= 0 || D > MAXD || F <= 0) return 0;
  return B * K * 2 * (int64_t)(D * D) * F * (int64_t)sizeof(double);
}

extern "C" int tssep_mvdr_online_fwd(const void* obs, int obs_f64, const void* masks, int mask_f64,
                                     const double* state_in, double* state_out, double* enh, int64_t B, int K,
                                     int D, int64_t T, int F, int reference_channel, double forgetting,
                                     double diag_load, double eps, int masking, double masking_eps, void* stream) {
  if (!obs || !masks || !state_out || !enh) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || D <= 0 || T <= 0 || F <= 0 || reference_channel < 0 || reference_channel >= D ||
      !(forgetting > 0.0 && forgetting <= 1.0) || !(diag_load >= 0.0))
    return TSSEP_E_SHAPE;
  if (D > MAXD) return TSSEP_E_UNSUPPORTED;
  if (xcd_grid(B * ((F + 63) / 64), K) >= ((int64_t)1 << 31) || B * (K > D ? K : D) * T * F >= ((int64_t)1 << 40))
    return TSSEP_E_SHAPE;
  if (!aligned16(enh) || (((uintptr_t)obs) & (obs_f64 ? 15u : 7u)) || (((uintptr_t)state_out) & 7u) ||
      (((uintptr_t)state_in) & 7u))
    return TSSEP_E_ALIGN;
#define CALL(DD)                                                                                                 \
  launch_online<DD>(obs, obs_f64, masks, mask_f64, state_in, state_out, enh, B, K, T, F, reference_channel,      \
                    forgetting, diag_load, eps, masking, masking_eps, (hipStream_t)stream)
  DISPATCH_D(D, CALL)
#undef CALL
}
