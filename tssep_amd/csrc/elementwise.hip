// Streaming (HBM-bound) helper kernels of the TS-SEP hot path: speaker conditioning,
// tanh backward, layout changes (the logit map and its fused two-mask form with the sigmoid), column sums, split
// reductions and the two losses.
// Reference call sites are cited per entry point in include/tssep_hip.h.
#include <math.h>
#include "common.h"

namespace {

// ---- speaker conditioning -----------------------------------------------------------------
// rows of xs are (b, trial, k, t); trial tr puts speaker (k + tr) % K at position k (net.py:913-924); pre rows are (b,t)
__device__ __forceinline__ void cond_row(int64_t row, int64_t K, int64_t T, int trials, int64_t& b,
                                         int64_t& t, int64_t& spk) {
  t = row % T;
  const int64_t q = row / T, k = q % K, bt = q / K;
  const int64_t tr = bt % trials;
  b = bt / trials;
  spk = k + tr;
  if (spk >= K) spk -= K;
}
// aux rows are (b, spk) for utterance-level embeddings (!TIME) and (b, spk, ta), ta = t / stride, for frame-wise ones
// (TIME; net.py:866-894 at stride 1).  That row index is ALL the two levels differ in: every kernel below is one body
// for both, so a time-constant frame-wise aux gives the utterance level's bits.  !TIME ignores Ta and stride and
// carries no division for them.
template <bool TIME>
__device__ __forceinline__ int64_t cond_ta(int64_t t, int64_t stride) { return TIME ? t / stride : 0; }
template <bool TIME>
__device__ __forceinline__ int64_t cond_aux_row(int64_t b, int64_t K, int64_t spk, int64_t Ta, int64_t ta) {
  return TIME ? (b * K + spk) * Ta + ta : b * K + spk;
}
// one wave per output row: the row decomposition (3 divisions, and t / stride) once per row instead of per element
template <bool TIME>
__global__ __launch_bounds__(256) void cond_mul_fwd_kernel(
    const float* __restrict__ pre, int64_t ld_pre, const float* __restrict__ aux, int64_t ld_aux,
    float* __restrict__ xs, int64_t ld_xs, int64_t B, int64_t K, int64_t T, int F, int trials, int64_t Ta,
    int64_t stride) {
  const int lane = threadIdx.x & 63;
  const int64_t rows = B * trials * K * T;
  const bool vec = F <= 1024 && ((ld_pre | ld_aux | ld_xs) & 3) == 0 && ld_pre >= ((F + 3) & ~3) &&
                   ld_aux >= ((F + 3) & ~3) && ld_xs >= ((F + 3) & ~3) &&
                   ((((uintptr_t)pre) | ((uintptr_t)aux) | ((uintptr_t)xs)) & 15) == 0;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    int64_t b, t, spk;
    cond_row(row, K, T, trials, b, t, spk);
    const float* p = pre + (b * T + t) * ld_pre;
    const float* a = aux + cond_aux_row<TIME>(b, K, spk, Ta, cond_ta<TIME>(t, stride)) * ld_aux;
    float* o = xs + row * ld_xs;
    if (vec) {
      // 16-byte accesses, all loads of the row first (F <= 1024: at most 4 quads per lane); the pad
      // columns of a row (ld rounded to 4) are written too: they are zero in both inputs
      const int nq = (F + 3) >> 2;
      f32x4 pv[4], av[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = lane + 64 * r;
        if (q < nq) {
          pv[r] = *reinterpret_cast<const f32x4*>(p + 4 * q);
          av[r] = *reinterpret_cast<const f32x4*>(a + 4 * q);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q = lane + 64 * r;
        if (q < nq) __builtin_nontemporal_store(pv[r] * av[r], reinterpret_cast<f32x4*>(o + 4 * q));
      }
    } else {
      for (int f = lane; f < F; f += 64) o[f] = p[f] * a[f];
    }
  }
}
// 16-byte variant: a thread owns 4 consecutive features of one (b, t) row and sums over (trial, speaker);
// the K * trials loads are independent of each other (no per-element index arithmetic, 4x fewer requests)
template <bool TIME>
__global__ void cond_mul_bwd_v4_kernel(const float* __restrict__ dxs, int64_t ld_dxs,
                                       const float* __restrict__ aux, int64_t ld_aux,
                                       float* __restrict__ dpre, int64_t ld_dpre, int64_t B, int64_t K,
                                       int64_t T, int F, int trials, int64_t Ta, int64_t stride) {
  const int nq = (F + 3) >> 2;
  const int64_t total = B * T * nq;
  GRID_STRIDE(e, total) {
    const int64_t row = e / nq;
    const int q = (int)(e - row * nq);
    const int64_t t = row % T, b = row / T;
    const int64_t ta = cond_ta<TIME>(t, stride);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int tr = 0; tr < trials; ++tr) {
#pragma unroll 4
      for (int64_t k = 0; k < K; ++k) {
        int64_t spk = k + tr;
        if (spk >= K) spk -= K;
        const f32x4 d = *reinterpret_cast<const f32x4*>(dxs + (((b * trials + tr) * K + k) * T + t) * ld_dxs + 4 * q);
        const f32x4 a = *reinterpret_cast<const f32x4*>(aux + cond_aux_row<TIME>(b, K, spk, Ta, ta) * ld_aux + 4 * q);
        s[0] += d[0] * a[0]; s[1] += d[1] * a[1]; s[2] += d[2] * a[2]; s[3] += d[3] * a[3];
      }
    }
    *reinterpret_cast<f32x4*>(dpre + row * ld_dpre + 4 * q) = s;
  }
}
template <bool TIME>
__global__ void cond_mul_bwd_kernel(const float* __restrict__ dxs, int64_t ld_dxs,
                                    const float* __restrict__ aux, int64_t ld_aux,
                                    float* __restrict__ dpre, int64_t ld_dpre, int64_t B, int64_t K,
                                    int64_t T, int F, int trials, int64_t Ta, int64_t stride) {
  const int64_t total = B * T * F;
  GRID_STRIDE(e, total) {
    const int64_t row = e / F;
    const int f = (int)(e - row * F);
    const int64_t t = row % T, b = row / T;
    const int64_t ta = cond_ta<TIME>(t, stride);
    float s = 0.f;
    for (int tr = 0; tr < trials; ++tr)
      for (int64_t k = 0; k < K; ++k) {
        int64_t spk = k + tr;
        if (spk >= K) spk -= K;
        s += dxs[(((b * trials + tr) * K + k) * T + t) * ld_dxs + f] *
             aux[cond_aux_row<TIME>(b, K, spk, Ta, ta) * ld_aux + f];
      }
    dpre[row * ld_dpre + f] = s;
  }
}
template <bool TIME>
__global__ void cond_cat_fwd_kernel(const float* __restrict__ pre, int64_t ld_pre,
                                    const float* __restrict__ aux, int64_t ld_aux,
                                    float* __restrict__ xs, int64_t ld_xs, int64_t B, int64_t K,
                                    int64_t T, int F, int E, int trials, int64_t Ta, int64_t stride) {
  const int W = F + E;
  const int64_t total = B * trials * K * T * W;
  GRID_STRIDE(e, total) {
    const int64_t row = e / W;
    const int c = (int)(e - row * W);
    int64_t b, t, spk;
    cond_row(row, K, T, trials, b, t, spk);
    xs[row * ld_xs + c] =
        c < F ? pre[(b * T + t) * ld_pre + c]
              : aux[cond_aux_row<TIME>(b, K, spk, Ta, cond_ta<TIME>(t, stride)) * ld_aux + (c - F)];
  }
}
// (d(pre) of cat does not read the embedding: one kernel for both levels)
__global__ void cond_cat_bwd_kernel(const float* __restrict__ dxs, int64_t ld_dxs,
                                    float* __restrict__ dpre, int64_t ld_dpre, int64_t B,
                                    int64_t K, int64_t T, int F, int trials) {
  const int64_t total = B * T * F;
  GRID_STRIDE(e, total) {
    const int64_t row = e / F;
    const int f = (int)(e - row * F);
    const int64_t t = row % T, b = row / T;
    float s = 0.f;
    for (int64_t q = 0; q < (int64_t)trials * K; ++q) s += dxs[((b * trials * K + q) * T + t) * ld_dxs + f];
    dpre[row * ld_dpre + f] = s;
  }
}

// ---- tanh backward (+ optional layout change) ---------------------------------------------
// dz rows are always (b,k,t) x P.  combined != 0: dy and y live in [B,T,K*P].
__global__ void tanh_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y,
                                float* __restrict__ dz, int64_t rows, int64_t P, int64_t K,
                                int64_t T, int combined) {
  const int64_t total = rows * P;
  GRID_STRIDE(e, total) {
    int64_t src = e;
    if (combined) {
      const int64_t row = e / P, p = e - row * P;
      const int64_t t = row % T, bk = row / T, k = bk % K, b = bk / K;
      src = ((b * T + t) * K + k) * P + p;
    }
    const float v = y[src];
    dz[e] = dy[src] * (1.0f - v * v);
  }
}
// P % 4 == 0 and 16-byte aligned buffers: one float4 per thread and iteration
__global__ void tanh_bwd_v4_kernel(const f32x4* __restrict__ dy, const f32x4* __restrict__ y,
                                   f32x4* __restrict__ dz, int64_t rows, int P4, int K, int T,
                                   int combined) {
  const int64_t total = rows * P4;
  GRID_STRIDE(e, total) {
    int64_t src = e;
    if (combined) {
      const int64_t row = e / P4;
      const int p = (int)(e - row * P4);
      const int64_t bk = row / T;
      const int t = (int)(row - bk * T);
      const int64_t b = bk / K;
      const int k = (int)(bk - b * K);
      src = ((b * T + t) * K + k) * P4 + p;
    }
    const f32x4 v = y[src], d = __builtin_nontemporal_load(dy + src);
    f32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = d[i] * (1.0f - v[i] * v[i]);
    dz[e] = o;
  }
}

// ---- column sums (bias gradients), deterministic two-pass ---------------------------------
constexpr int CS_SLABS = 128;
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ A,
                                                             int64_t M, int64_t N, int64_t lda,
                                                             float* __restrict__ ws) {
  __shared__ float red[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int64_t n = (int64_t)blockIdx.x * 64 + tx;
  const int64_t per = (M + CS_SLABS - 1) / CS_SLABS;
  const int64_t m0 = (int64_t)blockIdx.y * per;
  const int64_t m1 = m0 + per < M ? m0 + per : M;
  float s = 0.f;
  if (n < N) {
    // 4 independent loads in flight per thread (one per loop trip left the slab latency-bound)
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int64_t m = m0 + ty;
    for (; m + 12 < m1; m += 16) {
      const float a0 = A[m * lda + n], a1 = A[(m + 4) * lda + n];
      const float a2 = A[(m + 8) * lda + n], a3 = A[(m + 12) * lda + n];
      s0 += a0; s1 += a1; s2 += a2; s3 += a3;
    }
    for (; m < m1; m += 4) s0 += A[m * lda + n];
    s = (s0 + s1) + (s2 + s3);
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && n < N)
    ws[(int64_t)blockIdx.y * N + n] = (red[0][tx] + red[1][tx]) + (red[2][tx] + red[3][tx]);
}
// dst[i] (+)= sum_s src[s*stride + i]
__global__ void reduce_splits_kernel(const float* __restrict__ src, int nsplit, int64_t stride,
                                     int64_t count, float* __restrict__ dst, int accumulate) {
  GRID_STRIDE(i, count) {
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += src[k * stride + i];
    dst[i] = accumulate ? dst[i] + s : s;
  }
}

// split-K partials [nsplit][M][ldp] of a weight-gradient GEMM whose B operand carried a virtual ones column:
// columns [0, N) -> dW [M, ld_w] (dense), column N -> the bias gradient db [M] (the column sums of dY).
__global__ void reduce_splits_bias_kernel(const float* __restrict__ src, int nsplit, int64_t stride,
                                          int64_t M, int64_t N, int64_t ldp, float* __restrict__ dw,
                                          int64_t ld_w, float* __restrict__ db, int accumulate) {
  const int64_t total = M * (N + 1);
  GRID_STRIDE(i, total) {
    const int64_t m = i / (N + 1), n = i - m * (N + 1);
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += src[k * stride + m * ldp + n];
    float* d = n < N ? dw + m * ld_w + n : db + m;
    *d = accumulate ? *d + s : s;
  }
}

// ---- LogMAE -------------------------------------------------------------------------------
constexpr int LM_CHUNK = 4096;
__global__ __launch_bounds__(256) void absdiff_partial_kernel(const float* __restrict__ est,
                                                              const float* __restrict__ tgt,
                                                              int64_t N, float* __restrict__ part,
                                                              int nchunks) {
  __shared__ float red[4];
  const int64_t row = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * LM_CHUNK;
  float s = 0.f;
  for (int i = threadIdx.x; i < LM_CHUNK; i += 256) {
    const int64_t n = n0 + i;
    if (n < N) s += fabsf(est[row * N + n] - tgt[row * N + n]);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[row * nchunks + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
// loss[b] = log10( sum_k (sum_c part[b*K+k][c]) / N ),  sums[b] = the argument of the log
__global__ void logmae_finalize_kernel(const float* __restrict__ part, int64_t B, int64_t K,
                                       int nchunks, int64_t N, float* __restrict__ loss,
                                       float* __restrict__ sums) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float tot = 0.f;
  for (int64_t k = 0; k < K; ++k) {
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += part[(b * K + k) * nchunks + c];
    tot += s / (float)N;
  }
  sums[b] = tot;
  loss[b] = log10f(tot);
}
__global__ void logmae_bwd_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                  const float* __restrict__ sums, const float* __restrict__ gout,
                                  int64_t KN, int64_t N, int64_t total, float* __restrict__ dest) {
  const float ln10 = 2.30258509299404568402f;
  GRID_STRIDE(e, total) {
    const int64_t b = e / KN;
    // sums == NULL: plain MAE (tssep/train/loss.py:214-216), d/d est = gout sign(est - tgt) / N
    const float coef = sums ? gout[b] / ((float)N * ln10 * sums[b]) : gout[b] / (float)N;
    const float d = est[e] - tgt[e];
    dest[e] = d > 0.f ? coef : (d < 0.f ? -coef : 0.f);
  }
}

// ---- pairwise costs and the permutation-invariant assignment (pit=True; MSE) ----------------
// C[b,i,j] = (1/N) sum_n |est[b,i,n] - tgt[b,j,n]|^P.  One workgroup per (utterance, chunk of PC_CHUNK samples): the K
// est rows and the K tgt rows of the chunk are read ONCE (2 B K N floats in all, what one tssep_logmae_fwd reads) into
// K x K accumulators per lane; wave -> workgroup in a fixed order as absdiff_partial_kernel, no atomics.
// part [B][nchunks][K][K]; flat grid (b and the chunk share blockIdx.x: no 65535 cap on B).
// DIAG: only the K matched pairs i == j (a pit=False loss); the other entries of `part` are written as 0.
// Float32 roundings on the longest path into part: P == 1: 1 (e - t), P == 2: 2 (the square of the rounded difference;
// the product is fused into the add), + PC_CHUNK / 256 adds of the lane chain + 6 (wave tree) + 2 (the four waves).
constexpr int PC_CHUNK = 8192;
constexpr int PIT_MAX_K = 8;
template <int P>
__device__ __forceinline__ float pc_term(float e, float t, float acc) {
  const float d = e - t;
  return P == 1 ? acc + fabsf(d) : fmaf(d, d, acc);
}
template <int K, int P, bool DIAG>
__global__ __launch_bounds__(256) void pair_cost_partial_kernel(const float* __restrict__ est,
                                                                const float* __restrict__ tgt, int64_t N,
                                                                unsigned nchunks, int vec,
                                                                float* __restrict__ part) {
  constexpr int NA = DIAG ? K : K * K;
  __shared__ float red[4][NA];
  const int64_t b = blockIdx.x / nchunks;
  const int64_t n0 = (int64_t)(blockIdx.x - (unsigned)b * nchunks) * PC_CHUNK;
  const float* __restrict__ e0 = est + b * K * N;
  const float* __restrict__ t0 = tgt + b * K * N;
  float acc[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) acc[a] = 0.f;
  if (vec) {                     // N % 4 == 0 and 16-byte aligned bases: every row starts on a 16-byte boundary
    for (int it = 0; it < PC_CHUNK / 1024; ++it) {
      const int64_t n = n0 + (int64_t)(it * 256 + (int)threadIdx.x) * 4;
      if (n < N) {
        f32x4 tv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) tv[j] = *reinterpret_cast<const f32x4*>(t0 + j * N + n);
#pragma unroll
        for (int i = 0; i < K; ++i) {
          const f32x4 ev = *reinterpret_cast<const f32x4*>(e0 + i * N + n);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (DIAG) {
              acc[i] = pc_term<P>(ev[q], tv[i][q], acc[i]);
            } else {
#pragma unroll
              for (int j = 0; j < K; ++j) acc[i * K + j] = pc_term<P>(ev[q], tv[j][q], acc[i * K + j]);
            }
          }
        }
      }
    }
  } else {
    for (int it = 0; it < PC_CHUNK / 256; ++it) {
      const int64_t n = n0 + it * 256 + (int)threadIdx.x;
      if (n < N) {
        float tv[K];
#pragma unroll
        for (int j = 0; j < K; ++j) tv[j] = t0[j * N + n];
#pragma unroll
        for (int i = 0; i < K; ++i) {
          const float ev = e0[i * N + n];
          if (DIAG) {
            acc[i] = pc_term<P>(ev, tv[i], acc[i]);
          } else {
#pragma unroll
            for (int j = 0; j < K; ++j) acc[i * K + j] = pc_term<P>(ev, tv[j], acc[i * K + j]);
          }
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

// `a` before `b` in the order the assignment minimises: a NaN sum first (as torch.min, it reaches the loss), then the
// smaller float32 sum, then -- among equal sums -- the smaller index in itertools.permutations(range(K)) order
__device__ __forceinline__ bool pit_before(float sa, int ia, float sb, int ib) {
  const bool na = sa != sa, nb = sb != sb;
  if (na || nb) return na && (!nb || ia < ib);
  return sa < sb || (sa == sb && ia < ib);
}
// Lexicographic enumeration of the permutations of range(K) (the order of itertools.permutations), split as
// index = prefix * TAIL! + sub: the first K - TAIL entries are decoded from `prefix` in the factorial number system (the
// radices are compile-time constants: no integer division is executed), the last TAIL = min(K, 3) entries run through
// the TAIL! orders of the TAIL elements left over, ascending -- one decode and one prefix sum serve TAIL! permutations.
template <int K>
struct PitPlan {
  static constexpr int TAIL = K < 3 ? K : 3;
  static constexpr int NSUB = TAIL == 3 ? 6 : TAIL;        // TAIL!
  static constexpr int L = K - TAIL;
  static constexpr int fact(int n) { return n <= 1 ? 1 : n * fact(n - 1); }
  static constexpr int NPREFIX = fact(K) / NSUB;
};
// -> the prefix entries (4 bits each, entry i at bits 4 i); avail: the elements left over, ascending, 4 bits each
template <int K>
__device__ __forceinline__ unsigned pit_prefix(int pidx, uint64_t& avail) {
  using P = PitPlan<K>;
  avail = 0x76543210ull;
  unsigned perm = 0;
#pragma unroll
  for (int i = 0; i < P::L; ++i) {
    const int f = P::fact(K - 1 - i) / P::NSUB;             // permutations of the prefix behind entry i
    const int d = pidx / f;
    pidx -= d * f;
    perm |= (unsigned)((avail >> (4 * d)) & 15u) << (4 * i);
    avail = (avail & ((1ull << (4 * d)) - 1ull)) | ((avail >> (4 * d + 4)) << (4 * d));
  }
  return perm;
}
// the sub-th order of TAIL elements: which of the (ascending) left-over elements goes to tail position a
__device__ __forceinline__ int pit_sub(int tail, int sub, int a) {
  // TAIL == 3: 012 021 102 120 201 210, two bits per position; TAIL == 2: 01 10; TAIL == 1: 0
  const unsigned t3[6] = {0x24u, 0x18u, 0x21u, 0x09u, 0x12u, 0x06u};
  if (tail == 3) return (int)((t3[sub] >> (2 * a)) & 3u);
  return tail == 2 ? (a ^ sub) : 0;
}
// One workgroup per utterance: cost[b] = (sum over the chunks in chunk order) / N, then the assignment.  pit != 0:
// the prefixes are dealt to the 256 lanes (lane l takes l, l + 256, ...: ascending indices within a lane), each
// sum_i C[i, perm(i)] in float32 in ascending i out of LDS, and the best (pit_before) is reduced wave -> workgroup.
// pit == 0: the identity.
template <int K>
__global__ __launch_bounds__(256) void pit_assign_kernel(const float* __restrict__ part, int nchunks, int64_t N,
                                                         int pit, int logarithm, float* __restrict__ cost,
                                                         int32_t* __restrict__ perm, float* __restrict__ sums,
                                                         float* __restrict__ loss) {
  using P = PitPlan<K>;
  constexpr int KK = K * K, NONE = 0x7fffffff;
  __shared__ float C[KK];
  __shared__ float best_s[4];
  __shared__ int best_i[4];
  const int64_t b = blockIdx.x;
  if ((int)threadIdx.x < KK) {
    float s = 0.f;
    for (int c = 0; c < nchunks; ++c) s += part[(b * nchunks + c) * KK + threadIdx.x];
    s = s / (float)N;
    C[threadIdx.x] = s;
    if (cost) cost[b * KK + threadIdx.x] = s;
  }
  __syncthreads();
  float bs = 0.f;
  int bi = NONE;                                // (a lane without a permutation never wins: every real index is smaller)
  if (pit) {
    for (int pidx = threadIdx.x; pidx < P::NPREFIX; pidx += 256) {
      uint64_t avail;
      const unsigned pm = pit_prefix<K>(pidx, avail);
      float sp = 0.f;                           // (0 + x is exact: the sum starts at C[0, perm(0)])
#pragma unroll
      for (int i = 0; i < P::L; ++i) sp += C[i * K + ((pm >> (4 * i)) & 15u)];
      float c[P::TAIL][P::TAIL];                // c[a][e] = C[L + a, e-th element left over]
#pragma unroll
      for (int a = 0; a < P::TAIL; ++a)
#pragma unroll
        for (int e = 0; e < P::TAIL; ++e) c[a][e] = C[(P::L + a) * K + (int)((avail >> (4 * e)) & 15u)];
#pragma unroll
      for (int sub = 0; sub < P::NSUB; ++sub) {
        float s = sp;
#pragma unroll
        for (int a = 0; a < P::TAIL; ++a) s += c[a][pit_sub(P::TAIL, sub, a)];
        const int idx = pidx * P::NSUB + sub;
        if (bi == NONE || pit_before(s, idx, bs, bi)) { bs = s; bi = idx; }
      }
    }
  } else if (threadIdx.x == 0) {
    for (int i = 0; i < K; ++i) bs += C[i * K + i];
    bi = 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (oi != NONE && (bi == NONE || pit_before(os, oi, bs, bi))) { bs = os; bi = oi; }
  }
  if ((threadIdx.x & 63) == 0) { best_s[threadIdx.x >> 6] = bs; best_i[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (best_i[w] != NONE && pit_before(best_s[w], best_i[w], bs, bi)) { bs = best_s[w]; bi = best_i[w]; }
    unsigned pm = 0x76543210u;
    if (pit) {
      uint64_t avail;
      const int pidx = bi / P::NSUB, sub = bi - pidx * P::NSUB;
      pm = pit_prefix<K>(pidx, avail);
      for (int a = 0; a < P::TAIL; ++a)
        pm |= (unsigned)((avail >> (4 * pit_sub(P::TAIL, sub, a))) & 15u) << (4 * (P::L + a));
    }
    for (int i = 0; i < K; ++i) perm[b * K + i] = (int32_t)((pm >> (4 * i)) & 15u);
    sums[b] = bs;
    loss[b] = logarithm ? log10f(bs) : bs;
  }
}
// logmae_bwd_kernel with the target row taken through perm (NULL: the identity) and the P == 2 branch:
// P == 1: coef sign(e - t), P == 2: coef 2 (e - t); coef = gout[b] / N, over ln10 sums[b] when sums != NULL.
template <int P>
__global__ void pair_loss_bwd_kernel(const float* __restrict__ est, const float* __restrict__ tgt,
                                     const int32_t* __restrict__ perm, const float* __restrict__ sums,
                                     const float* __restrict__ gout, int64_t K, int64_t N, int64_t total,
                                     float* __restrict__ dest) {
  const float ln10 = 2.30258509299404568402f;
  const int64_t KN = K * N;
  GRID_STRIDE(e, total) {
    const int64_t b = e / KN, r = e - b * KN;
    const int64_t i = r / N, n = r - i * N;
    int64_t j = perm ? (int64_t)perm[b * K + i] : i;
    if (j < 0 || j >= K) j = i;                 // (a corrupt perm must not turn into a read outside tgt)
    const float g = P == 2 ? 2.0f * gout[b] : gout[b];
    const float coef = sums ? g / ((float)N * ln10 * sums[b]) : g / (float)N;
    const float d = est[e] - tgt[(b * K + j) * N + n];
    dest[e] = P == 2 ? coef * d : (d > 0.f ? coef : (d < 0.f ? -coef : 0.f));
  }
}

// ---- VAD BCE ------------------------------------------------------------------------------
// one wave per (b,k,t) row: x = mean_f logit ; l = max(x,0) - x*y + log1p(exp(-|x|))
__global__ __launch_bounds__(256) void vadbce_rows_kernel(const float* __restrict__ logit,
                                                          const float* __restrict__ vad,
                                                          int64_t rows, int F,
                                                          float* __restrict__ xmean,
                                                          float* __restrict__ lrow) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float s = 0.f;
  for (int f = lane; f < F; f += 64) s += logit[row * F + f];
  s = wave_sum(s);
  if (lane == 0) {
    const float x = s / (float)F, y = vad[row];
    xmean[row] = x;
    lrow[row] = fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
  }
}
__global__ void vadbce_finalize_kernel(const float* __restrict__ lrow, int64_t B, int64_t KT,
                                       float* __restrict__ loss) {
  __shared__ float red[4];
  const int64_t b = blockIdx.x;
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < KT; i += 256) s += lrow[b * KT + i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[b] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)KT;
}
__global__ void vadbce_bwd_kernel(const float* __restrict__ xmean, const float* __restrict__ vad,
                                  const float* __restrict__ gout, int64_t KT, int F,
                                  int64_t total, float* __restrict__ dlogit) {
  GRID_STRIDE(e, total) {
    const int64_t row = e / F;
    const int64_t b = row / KT;
    const float x = xmean[row];
    dlogit[e] = gout[b] * (sigmoidf_acc(x) - vad[row]) / ((float)KT * (float)F);
  }
}

// ---- VAD BCE on the gate column of an explicit_vad logit (SignalAndVADSigmoidBCE, loss.py:348-395) ----------------
// x = logit[row * ld] (column 0 of a row of ld = F + 1 floats); the same per-row loss and fixed-order mean over (k, t) as
// vadbce; bwd writes whole rows: gout[b] (sigmoid(x) - y) / (K T) at column 0, zeros behind it
__global__ void gatebce_rows_kernel(const float* __restrict__ logit, int64_t ld, const float* __restrict__ vad,
                                    int64_t rows, float* __restrict__ lrow) {
  GRID_STRIDE(row, rows) {
    const float x = logit[row * ld], y = vad[row];
    lrow[row] = fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
  }
}
__global__ void gatebce_bwd_kernel(const float* __restrict__ logit, int64_t ld, const float* __restrict__ vad,
                                   const float* __restrict__ gout, int64_t KT, int64_t total,
                                   float* __restrict__ dlogit) {
  GRID_STRIDE(e, total) {
    const int64_t row = e / ld;
    float v = 0.f;
    if (e == row * ld) v = gout[row / KT] * (sigmoidf_acc(logit[e]) - vad[row]) / (float)KT;
    dlogit[e] = v;
  }
}

// ---- the VAD losses' targets on the device (loss.py:312-327, utils.py:11-77) -----------------------------------------
// frame magnitudes of a spectrum in memory: one wave per frame, a[frame] = sum_f |X[frame, f]| -- per lane over
// f = lane, lane + 64, ..., then across the wave (a fixed order)
template <bool COMPLEX>
__global__ __launch_bounds__(256) void framemag_kernel(const float* __restrict__ X, int64_t frames, int64_t F,
                                                       float* __restrict__ a) {
  const int lane = threadIdx.x & 63;
  for (int64_t fr = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); fr < frames; fr += (int64_t)gridDim.x * 4) {
    float s = 0.f;
    if (COMPLEX) {
      const float2* xr = reinterpret_cast<const float2*>(X) + fr * F;
      for (int64_t f = lane; f < F; f += 64) {
        const float2 v = xr[f];
        s += sqrtf(v.x * v.x + v.y * v.y);
      }
    } else {
      const float* xr = X + fr * F;
      for (int64_t f = lane; f < F; f += 64) s += fabsf(xr[f]);
    }
    s = wave_sum(s);
    if (lane == 0) a[fr] = s;
  }
}

// the maximum of torch.amax: a NaN wins and stays
__device__ __forceinline__ float nanmax(float m, float v) { return (v > m || v != v) ? v : m; }

// one workgroup per row of a [rows, T]: the row's maximum, then the decisions a / m > thr (IEEE division, strict
// comparison -- torch's `target / torch.amax(target, -1, keepdim=True) > thr` on float32; NOT a > thr m, which decides
// ties differently).  The second walk over the row reads what the first left in the cache.
__global__ __launch_bounds__(256) void vad_from_mag_kernel(const float* __restrict__ a, int64_t rows, int64_t T, float thr,
                                                           float* __restrict__ vad) {
  __shared__ float red[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float* ar = a + row * T;
    float m = -INFINITY;
    for (int64_t t = tid; t < T; t += 256) m = nanmax(m, ar[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = nanmax(nanmax(red[0], red[1]), nanmax(red[2], red[3]));
    for (int64_t t = tid; t < T; t += 256) vad[row * T + t] = (ar[t] / m > thr) ? 1.f : 0.f;
    __syncthreads();          // red is rewritten by the next row
  }
}

// sample activity -> frame activity: the sample at the end of the hop that frame t is centred on (the last sample that
// paderbox's sample_index_to_stft_frame_index maps to t) decides the frame
__global__ void vad_frames_kernel(const uint8_t* __restrict__ v, int64_t N, int64_t T, int64_t shift, int64_t off,
                                  int64_t total, float* __restrict__ out) {
  GRID_STRIDE(e, total) {
    const int64_t row = e / T, t = e - row * T;
    const int64_t i = (t + 1) * shift + off;
    out[e] = (i >= 0 && i < N && v[row * N + i] != 0) ? 1.f : 0.f;
  }
}

// ---- logit layout map: raw GEMM output -> [B, K, T, F] (+ trial mean, + 't' broadcast) ------
// Covers the tail of MaskEstimator_v2.forward: the final einops rearrange / reduce-repeat
// (net.py:631-659), the mean over permutation trials (net.py:928-951) and the speaker
// un-permutation (net.py:957-967).
//   raw index, speakers in columns (ts_vad):  ((b*trials + tr)*T + t) * (K*Fr) + k*Fr + fr
//   raw index, speakers in rows (ts_vad off): ((b*K + k)*T + t) * Fr + fr           (trials == 1)
//   Fr = F ('tf') or 1 ('t', value repeated over frequency)
// Trial tr holds speaker (k + tr) % K at position k; speaker s lands at output index perm[b,s].
struct MapArgs {
  int64_t B, K, T; int F, Fr, trials, spk_rows;
  const int32_t* perm; const int32_t* iperm;
};
__device__ __forceinline__ int64_t raw_index(const MapArgs& a, int64_t b, int tr, int64_t t, int k,
                                             int fr) {
  if (a.spk_rows) return ((b * a.K + k) * a.T + t) * a.Fr + fr;
  return ((b * a.trials + tr) * a.T + t) * (a.K * a.Fr) + (int64_t)k * a.Fr + fr;
}
// The trial mean.  A power of two of trials: the fp32 sum in trial order, then * fl(1 / trials), an exact scaling --
// trials - 1 roundings, (trials - 1) U mean |raw|.  Any other count: fl(1 / trials) and the product with it would be two
// more roundings and leave that bound (seen at trials = 3: up to 1.27 x), so the sum and the division are carried in
// double and rounded once, U |mean|.  Shared by logit_map_fwd_kernel and mask_map_fwd_kernel: the same bits in both.
__device__ __forceinline__ bool odd_trials(int trials) { return (trials & (trials - 1)) != 0; }
__device__ __forceinline__ float mean_of(double sum, int trials) { return (float)(sum / (double)trials); }
__global__ void logit_map_fwd_kernel(const float* __restrict__ raw, MapArgs a,
                                     float* __restrict__ out) {
  const int64_t total = a.B * a.K * a.T * a.F;
  const float inv = 1.0f / (float)a.trials;
  const bool exact_mean = odd_trials(a.trials);
  GRID_STRIDE(e, total) {
    const int64_t row = e / a.F;
    const int f = (int)(e - row * a.F);
    const int64_t t = row % a.T, bj = row / a.T, j = bj % a.K, b = bj / a.K;
    const int s = a.iperm ? a.iperm[b * a.K + j] : (int)j;
    const int fr = a.Fr == 1 ? 0 : f;
    if (exact_mean) {
      double acc = 0.0;
      for (int tr = 0; tr < a.trials; ++tr) {
        int k = s - tr;
        if (k < 0) k += (int)a.K;
        acc += (double)raw[raw_index(a, b, tr, t, k, fr)];
      }
      out[e] = mean_of(acc, a.trials);
      continue;
    }
    float acc = 0.f;
    for (int tr = 0; tr < a.trials; ++tr) {
      int k = s - tr;
      if (k < 0) k += (int)a.K;
      acc += raw[raw_index(a, b, tr, t, k, fr)];
    }
    out[e] = a.trials == 1 ? acc : acc * inv;
  }
}
// draw (raw layout) <- dout [B,K,T,F]: one wave per run of F contiguous raw elements (one
// (b, trial, t, k)); the index decomposition once per run instead of five divisions per element
__global__ __launch_bounds__(256) void logit_map_bwd_tf_kernel(const float* __restrict__ dout, MapArgs a,
                                                               float* __restrict__ draw) {
  const int lane = threadIdx.x & 63;
  const int64_t runs = a.B * a.trials * a.T * a.K;
  const float inv = 1.0f / (float)a.trials;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < runs; u += (int64_t)gridDim.x * 4) {
    int64_t b, t; int tr, k;
    if (a.spk_rows) {
      t = u % a.T; const int64_t bk = u / a.T; k = (int)(bk % a.K); b = bk / a.K; tr = 0;
    } else {
      k = (int)(u % a.K); const int64_t row = u / a.K;
      t = row % a.T; const int64_t bt = row / a.T; tr = (int)(bt % a.trials); b = bt / a.trials;
    }
    int s = k + tr;
    if (s >= a.K) s -= (int)a.K;
    const int j = a.perm ? a.perm[b * a.K + s] : s;
    const float* src = dout + ((b * a.K + j) * a.T + t) * a.F;
    float* dst = draw + u * a.F;
    for (int f = lane; f < a.F; f += 64) dst[f] = a.trials == 1 ? src[f] : src[f] * inv;
  }
}
__global__ __launch_bounds__(256) void logit_map_bwd_t_kernel(const float* __restrict__ dout,
                                                              MapArgs a, float* __restrict__ draw) {
  const int lane = threadIdx.x & 63;
  const int64_t total = a.B * a.trials * a.T * a.K;     // raw elements (Fr == 1)
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= total) return;
  int64_t b, t; int tr, k;
  if (a.spk_rows) {
    t = e % a.T; const int64_t bk = e / a.T; k = (int)(bk % a.K); b = bk / a.K; tr = 0;
  } else {
    const int64_t row = e / a.K; k = (int)(e - row * a.K);
    t = row % a.T; const int64_t bt = row / a.T; tr = (int)(bt % a.trials); b = bt / a.trials;
  }
  int s = k + tr;
  if (s >= a.K) s -= (int)a.K;
  const int j = a.perm ? a.perm[b * a.K + s] : s;
  const float* p = dout + ((b * a.K + j) * a.T + t) * a.F;
  float acc = 0.f;
  for (int f = lane; f < a.F; f += 64) acc += p[f];
  acc = wave_sum(acc);
  if (lane == 0) draw[e] = acc / (float)a.trials;
}

// ---- fused two-mask tail: raw GEMM output -> logit and mask [B, K, M, T, F], and back -------------------------
// The logit map above with M masks per speaker (nmask of MaskEstimator_v2, net.py:629-659: '(spk mask freq)' columns)
// and the final sigmoid (net.py:983) in the same pass, so the tail's largest tensors are walked once each way.
//   raw index, speakers in columns (ts_vad):  ((b*trials + tr)*T + t) * (K*M*Fr) + (k*M + m)*Fr + fr
//   raw index, speakers in rows (ts_vad off): ((b*K + k)*T + t) * (M*Fr) + m*Fr + fr          (trials == 1)
//   out index:                                (((b*K + j)*M + m)*T + t)*F + f
// Both raw layouts are runs of Fr floats numbered (b, tr, t, k, m) / (b, k, t, m); the output is runs of F floats numbered
// (b, j, m, t).  One wave per run, the index decomposition once per run; trial and permutation conventions as above.
__device__ __forceinline__ int64_t mask_run_base(const MapArgs& a, int M, int64_t b, int64_t t, int m, int s) {
  // spk_rows: the raw run of speaker s; else the raw run of (trial 0, position 0), trial tr / position k at
  // + tr * T*K*M + k * M
  if (a.spk_rows) return ((b * a.K + s) * a.T + t) * M + m;
  return (b * a.trials * a.T + t) * (a.K * M) + m;
}
__global__ __launch_bounds__(256) void mask_map_fwd_kernel(const float* __restrict__ raw, MapArgs a, int M,
                                                           float* __restrict__ logit, float* __restrict__ mask) {
  const int lane = threadIdx.x & 63;
  const int64_t runs = a.B * a.K * M * a.T;
  const int64_t step = a.T * a.K * M;                    // raw runs per trial
  const float inv = 1.0f / (float)a.trials;
  const bool exact_mean = odd_trials(a.trials);
  for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < runs; v += (int64_t)gridDim.x * 4) {
    const int64_t t = v % a.T, q = v / a.T;
    const int m = (int)(q % M);
    const int64_t bj = q / M, j = bj % a.K, b = bj / a.K;
    const int s = a.iperm ? a.iperm[b * a.K + j] : (int)j;
    const int64_t base = mask_run_base(a, M, b, t, m, s);
    float* lo = logit + v * a.F;
    float* mo = mask + v * a.F;
    for (int f = lane; f < a.F; f += 64) {
      const int fr = a.Fr == 1 ? 0 : f;
      float x;
      if (exact_mean) {                                  // (never with spk_rows: trials == 1 there)
        double acc = 0.0;
        for (int tr = 0; tr < a.trials; ++tr) {
          int k = s - tr;
          if (k < 0) k += (int)a.K;
          acc += (double)raw[(base + tr * step + (int64_t)k * M) * a.Fr + fr];
        }
        x = mean_of(acc, a.trials);
      } else {
        float acc = 0.f;
        if (a.spk_rows) {
          acc += raw[base * a.Fr + fr];
        } else {
          for (int tr = 0; tr < a.trials; ++tr) {
            int k = s - tr;
            if (k < 0) k += (int)a.K;
            acc += raw[(base + tr * step + (int64_t)k * M) * a.Fr + fr];
          }
        }
        x = a.trials == 1 ? acc : acc * inv;
      }
      lo[f] = x;
      mo[f] = sigmoidf_mask(x);
    }
  }
}
// raw run u -> (b, tr, t, k, m), then the output run of speaker (k + tr) % K, mask m
__device__ __forceinline__ int64_t mask_run_source(const MapArgs& a, int M, int64_t u) {
  const int m = (int)(u % M);
  const int64_t r = u / M;
  int64_t b, t; int tr, k;
  if (a.spk_rows) {
    t = r % a.T; const int64_t bk = r / a.T; k = (int)(bk % a.K); b = bk / a.K; tr = 0;
  } else {
    k = (int)(r % a.K); const int64_t row = r / a.K;
    t = row % a.T; const int64_t bt = row / a.T; tr = (int)(bt % a.trials); b = bt / a.trials;
  }
  int s = k + tr;
  if (s >= a.K) s -= (int)a.K;
  const int j = a.perm ? a.perm[b * a.K + s] : s;
  return (((b * a.K + j) * M + m) * a.T + t) * a.F;
}
// d(raw) of one element: fl(fl(dmask * s) * fl(1 - s)) [+ dlogit], every operation rounded on its own
__device__ __forceinline__ float mask_map_term(const float* __restrict__ dmask, const float* __restrict__ mask,
                                               const float* __restrict__ dlogit, int64_t i) {
#pragma clang fp contract(off)
  const float sg = mask[i];
  float g = dmask[i] * sg;
  g = g * (1.0f - sg);
  if (dlogit) g = g + dlogit[i];
  return g;
}
__global__ __launch_bounds__(256) void mask_map_bwd_tf_kernel(const float* __restrict__ dmask,
                                                              const float* __restrict__ mask,
                                                              const float* __restrict__ dlogit, MapArgs a, int M,
                                                              float* __restrict__ draw) {
  const int lane = threadIdx.x & 63;
  const int64_t runs = a.B * a.trials * a.T * a.K * M;
  const float inv = 1.0f / (float)a.trials;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < runs; u += (int64_t)gridDim.x * 4) {
    const int64_t src = mask_run_source(a, M, u);
    float* dst = draw + u * a.F;
    for (int f = lane; f < a.F; f += 64) {
      const float g = mask_map_term(dmask, mask, dlogit, src + f);
      dst[f] = a.trials == 1 ? g : g * inv;
    }
  }
}
// 't': one raw element per run, the sum over f in logit_map_bwd_t_kernel's order (a lane its bins l, l + 64, ..., then
// the shuffle tree)
__global__ __launch_bounds__(256) void mask_map_bwd_t_kernel(const float* __restrict__ dmask,
                                                             const float* __restrict__ mask,
                                                             const float* __restrict__ dlogit, MapArgs a, int M,
                                                             float* __restrict__ draw) {
  const int lane = threadIdx.x & 63;
  const int64_t runs = a.B * a.trials * a.T * a.K * M;     // raw elements (Fr == 1)
  const float inv = 1.0f / (float)a.trials;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < runs; u += (int64_t)gridDim.x * 4) {
    const int64_t src = mask_run_source(a, M, u);
    float acc = 0.f;
    for (int f = lane; f < a.F; f += 64) acc += mask_map_term(dmask, mask, dlogit, src + f);
    acc = wave_sum(acc);
    if (lane == 0) draw[u] = a.trials == 1 ? acc : acc * inv;
  }
}

}  // namespace

// The conditioning entry points: one launcher per role for both levels; the utterance level passes Ta = 0, stride = 1,
// which cond_t_shape_ok is not asked about and the <false> kernels ignore.
template <bool TIME>
static int cond_mul_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux, float* xs, int64_t ld_xs,
                        int64_t B, int64_t K, int64_t T, int F, int trials, int64_t Ta, int64_t stride, void* stream) {
  if (!pre || !aux || !xs) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || trials <= 0 || trials > K || (TIME && !cond_t_shape_ok(T, Ta, stride)))
    return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(cond_mul_fwd_kernel<TIME>, dim3(grid_for(B * trials * K * T * 64)), dim3(256), 0, S_,
                     pre, ld_pre, aux, ld_aux, xs, ld_xs, B, K, T, F, trials, Ta, stride);
  return tssep_launch_status();
}
template <bool TIME>
static int cond_mul_bwd(const float* dxs, int64_t ld_dxs, const float* aux, int64_t ld_aux, float* dpre,
                        int64_t ld_dpre, int64_t B, int64_t K, int64_t T, int F, int trials, int64_t Ta, int64_t stride,
                        void* stream) {
  if (!dxs || !aux || !dpre) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || trials <= 0 || trials > K || (TIME && !cond_t_shape_ok(T, Ta, stride)))
    return TSSEP_E_SHAPE;
  const int64_t fp = (F + 3) & ~3;
  // 16-byte path: every row holds whole quads at 16-byte addresses (the pad columns of a row are summed too: products
  // of the inputs' pad columns, zero in the step)
  const bool vec = ((ld_dxs | ld_aux | ld_dpre) & 3) == 0 && ld_dxs >= fp && ld_aux >= fp && ld_dpre >= fp &&
                   ((((uintptr_t)dxs) | ((uintptr_t)aux) | ((uintptr_t)dpre)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(cond_mul_bwd_v4_kernel<TIME>, dim3(grid_for(B * T * (fp / 4))), dim3(256), 0, S_, dxs, ld_dxs,
                       aux, ld_aux, dpre, ld_dpre, B, K, T, F, trials, Ta, stride);
  else
    hipLaunchKernelGGL(cond_mul_bwd_kernel<TIME>, dim3(grid_for(B * T * F)), dim3(256), 0, S_, dxs, ld_dxs,
                       aux, ld_aux, dpre, ld_dpre, B, K, T, F, trials, Ta, stride);
  return tssep_launch_status();
}
template <bool TIME>
static int cond_cat_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux, float* xs, int64_t ld_xs,
                        int64_t B, int64_t K, int64_t T, int F, int E, int trials, int64_t Ta, int64_t stride,
                        void* stream) {
  if (!pre || !aux || !xs) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || E <= 0 || trials <= 0 || trials > K ||
      (TIME && !cond_t_shape_ok(T, Ta, stride)))
    return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(cond_cat_fwd_kernel<TIME>, dim3(grid_for(B * trials * K * T * (F + E))), dim3(256),
                     0, S_, pre, ld_pre, aux, ld_aux, xs, ld_xs, B, K, T, F, E, trials, Ta, stride);
  return tssep_launch_status();
}

extern "C" int tssep_cond_mul_fwd(const float* pre, int64_t ld_pre, const float* aux,
                                  int64_t ld_aux, float* xs, int64_t ld_xs, int64_t B, int64_t K,
                                  int64_t T, int F, int trials, void* stream) {
  return cond_mul_fwd<false>(pre, ld_pre, aux, ld_aux, xs, ld_xs, B, K, T, F, trials, 0, 1, stream);
}
extern "C" int tssep_cond_mul_t_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux, float* xs,
                                    int64_t ld_xs, int64_t B, int64_t K, int64_t T, int F, int trials, int64_t Ta,
                                    int64_t stride, void* stream) {
  return cond_mul_fwd<true>(pre, ld_pre, aux, ld_aux, xs, ld_xs, B, K, T, F, trials, Ta, stride, stream);
}
extern "C" int tssep_cond_mul_bwd(const float* dxs, int64_t ld_dxs, const float* aux,
                                  int64_t ld_aux, float* dpre, int64_t ld_dpre, int64_t B,
                                  int64_t K, int64_t T, int F, int trials, void* stream) {
  return cond_mul_bwd<false>(dxs, ld_dxs, aux, ld_aux, dpre, ld_dpre, B, K, T, F, trials, 0, 1, stream);
}
extern "C" int tssep_cond_mul_t_bwd(const float* dxs, int64_t ld_dxs, const float* aux, int64_t ld_aux, float* dpre,
                                    int64_t ld_dpre, int64_t B, int64_t K, int64_t T, int F, int trials, int64_t Ta,
                                    int64_t stride, void* stream) {
  return cond_mul_bwd<true>(dxs, ld_dxs, aux, ld_aux, dpre, ld_dpre, B, K, T, F, trials, Ta, stride, stream);
}
extern "C" int tssep_cond_cat_fwd(const float* pre, int64_t ld_pre, const float* aux,
                                  int64_t ld_aux, float* xs, int64_t ld_xs, int64_t B, int64_t K,
                                  int64_t T, int F, int E, int trials, void* stream) {
  return cond_cat_fwd<false>(pre, ld_pre, aux, ld_aux, xs, ld_xs, B, K, T, F, E, trials, 0, 1, stream);
}
extern "C" int tssep_cond_cat_t_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux, float* xs,
                                    int64_t ld_xs, int64_t B, int64_t K, int64_t T, int F, int E, int trials,
                                    int64_t Ta, int64_t stride, void* stream) {
  return cond_cat_fwd<true>(pre, ld_pre, aux, ld_aux, xs, ld_xs, B, K, T, F, E, trials, Ta, stride, stream);
}
extern "C" int tssep_cond_cat_bwd(const float* dxs, int64_t ld_dxs, float* dpre, int64_t ld_dpre,
                                  int64_t B, int64_t K, int64_t T, int F, int trials, void* stream) {
  if (!dxs || !dpre) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || trials <= 0 || trials > K) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(cond_cat_bwd_kernel, dim3(grid_for(B * T * F)), dim3(256), 0, S_, dxs, ld_dxs,
                     dpre, ld_dpre, B, K, T, F, trials);
  return tssep_launch_status();
}
extern "C" int tssep_tanh_bwd(const float* dy, const float* y, float* dz, int64_t rows, int64_t P,
                              int64_t K, int64_t T, int combined_in, void* stream) {
  if (!dy || !y || !dz) return TSSEP_E_NULL;
  if (rows <= 0 || P <= 0 || K <= 0 || T <= 0 || rows % (K * T)) return TSSEP_E_SHAPE;
  if (P % 4 == 0 && aligned16(dy) && aligned16(y) && aligned16(dz))
    hipLaunchKernelGGL(tanh_bwd_v4_kernel, dim3(grid_for(rows * P / 4)), dim3(256), 0, S_,
                       (const f32x4*)dy, (const f32x4*)y, (f32x4*)dz, rows, (int)(P / 4), (int)K, (int)T,
                       combined_in);
  else
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(grid_for(rows * P)), dim3(256), 0, S_, dy, y, dz, rows,
                       P, K, T, combined_in);
  return tssep_launch_status();
}
extern "C" int64_t tssep_colsum_workspace_bytes(int64_t M, int64_t N) {
  (void)M;
  return (int64_t)CS_SLABS * N * (int64_t)sizeof(float);
}
extern "C" int tssep_colsum_f32(const float* A, int64_t M, int64_t N, int64_t lda, float* out,
                                int accumulate, void* ws, void* stream) {
  if (!A || !out || !ws) return TSSEP_E_NULL;
  if (M <= 0 || N <= 0) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)((N + 63) / 64), CS_SLABS), dim3(256), 0,
                     S_, A, M, N, lda, (float*)ws);
  hipLaunchKernelGGL(reduce_splits_kernel, dim3(grid_for(N)), dim3(256), 0, S_, (const float*)ws,
                     CS_SLABS, N, N, out, accumulate);
  return tssep_launch_status();
}
extern "C" int tssep_reduce_splits(const float* src, int nsplit, int64_t stride, int64_t count,
                                   float* dst, int accumulate, void* stream) {
  if (!src || !dst) return TSSEP_E_NULL;
  if (nsplit <= 0 || count <= 0) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(reduce_splits_kernel, dim3(grid_for(count)), dim3(256), 0, S_, src, nsplit,
                     stride, count, dst, accumulate);
  return tssep_launch_status();
}

extern "C" int tssep_reduce_splits_bias(const float* src, int nsplit, int64_t stride, int64_t M, int64_t N,
                                        int64_t ldp, float* dw, int64_t ld_w, float* db, int accumulate,
                                        void* stream) {
  if (!src || !dw || !db) return TSSEP_E_NULL;
  if (nsplit <= 0 || M <= 0 || N <= 0 || ldp < N + 1 || ld_w < N) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(reduce_splits_bias_kernel, dim3(grid_for(M * (N + 1))), dim3(256), 0, S_, src, nsplit,
                     stride, M, N, ldp, dw, ld_w, db, accumulate);
  return tssep_launch_status();
}

extern "C" int64_t tssep_logmae_chunks(int64_t N) { return (N + LM_CHUNK - 1) / LM_CHUNK; }
extern "C" int64_t tssep_logmae_workspace_bytes(int64_t B, int64_t K, int64_t N) {
  return B * K * tssep_logmae_chunks(N) * (int64_t)sizeof(float);
}
extern "C" int tssep_logmae_finalize(const float* partial, int64_t B, int64_t K, int64_t nchunks,
                                     int64_t N, float* loss, float* sums, void* stream) {
  if (!partial || !loss || !sums) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || nchunks <= 0 || N <= 0) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(logmae_finalize_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, S_,
                     partial, B, K, (int)nchunks, N, loss, sums);
  return tssep_launch_status();
}
extern "C" int tssep_logmae_fwd(const float* est, const float* tgt, int64_t B, int64_t K,
                                int64_t N, float* loss, float* sums, void* ws, void* stream) {
  if (!est || !tgt || !loss || !sums || !ws) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || N <= 0 || B * K > 65535) return TSSEP_E_SHAPE;
  const int nchunks = (int)tssep_logmae_chunks(N);
  hipLaunchKernelGGL(absdiff_partial_kernel, dim3((unsigned)nchunks, (unsigned)(B * K)), dim3(256),
                     0, S_, est, tgt, N, (float*)ws, nchunks);
  return tssep_logmae_finalize((const float*)ws, B, K, nchunks, N, loss, sums, stream);
}
extern "C" int tssep_logmae_bwd(const float* est, const float* tgt, const float* sums,
                                const float* gout, int64_t B, int64_t K, int64_t N, float* dest,
                                void* stream) {
  if (!est || !tgt || !gout || !dest) return TSSEP_E_NULL;      // sums may be NULL (MAE)
  if (B <= 0 || K <= 0 || N <= 0) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(logmae_bwd_kernel, dim3(grid_for(B * K * N)), dim3(256), 0, S_, est, tgt, sums,
                     gout, K * N, N, B * K * N, dest);
  return tssep_launch_status();
}
extern "C" int64_t tssep_pair_cost_chunks(int64_t N) { return (N + PC_CHUNK - 1) / PC_CHUNK; }
extern "C" int64_t tssep_pair_cost_workspace_bytes(int64_t B, int64_t K, int64_t N) {
  return B * tssep_pair_cost_chunks(N) * K * K * (int64_t)sizeof(float);
}
template <int P, bool DIAG>
static void pair_cost_launch(int K, unsigned grid, void* stream, const float* est, const float* tgt, int64_t N,
                             unsigned nchunks, int vec, float* part) {
  switch (K) {
#define PC_CASE(k)                                                                                            \
  case k:                                                                                                     \
    hipLaunchKernelGGL((pair_cost_partial_kernel<k, P, DIAG>), dim3(grid), dim3(256), 0, S_, est, tgt, N,     \
                       nchunks, vec, part);                                                                   \
    break;
    PC_CASE(1) PC_CASE(2) PC_CASE(3) PC_CASE(4) PC_CASE(5) PC_CASE(6) PC_CASE(7) PC_CASE(8)
#undef PC_CASE
  }
}
extern "C" int tssep_pair_cost_fwd(const float* est, const float* tgt, int64_t B, int64_t K, int64_t N, int p,
                                   int diag_only, float* part, void* stream) {
  if (!est || !tgt || !part) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || K > PIT_MAX_K || N <= 0 || (p != 1 && p != 2)) return TSSEP_E_SHAPE;
  const int64_t nchunks = tssep_pair_cost_chunks(N);
  if (B * nchunks > 0x7fffffffLL) return TSSEP_E_SHAPE;
  const unsigned grid = (unsigned)(B * nchunks);
  const int vec = (N & 3) == 0 && aligned16(est) && aligned16(tgt);
  if (p == 1) {
    if (diag_only) pair_cost_launch<1, true>((int)K, grid, stream, est, tgt, N, (unsigned)nchunks, vec, part);
    else pair_cost_launch<1, false>((int)K, grid, stream, est, tgt, N, (unsigned)nchunks, vec, part);
  } else {
    if (diag_only) pair_cost_launch<2, true>((int)K, grid, stream, est, tgt, N, (unsigned)nchunks, vec, part);
    else pair_cost_launch<2, false>((int)K, grid, stream, est, tgt, N, (unsigned)nchunks, vec, part);
  }
  return tssep_launch_status();
}
extern "C" int tssep_pit_assign(const float* part, int64_t B, int64_t K, int64_t nchunks, int64_t N, int pit,
                                int logarithm, float* cost, int32_t* perm, float* sums, float* loss, void* stream) {
  if (!part || !perm || !sums || !loss) return TSSEP_E_NULL;      // cost may be NULL (not wanted)
  if (B <= 0 || B > 0x7fffffffLL || K <= 0 || K > PIT_MAX_K || nchunks <= 0 || nchunks > 0x7fffffffLL || N <= 0)
    return TSSEP_E_SHAPE;
  switch (K) {
#define PA_CASE(k)                                                                                            \
  case k:                                                                                                     \
    hipLaunchKernelGGL(pit_assign_kernel<k>, dim3((unsigned)B), dim3(256), 0, S_, part, (int)nchunks, N, pit,  \
                       logarithm, cost, perm, sums, loss);                                                    \
    break;
    PA_CASE(1) PA_CASE(2) PA_CASE(3) PA_CASE(4) PA_CASE(5) PA_CASE(6) PA_CASE(7) PA_CASE(8)
#undef PA_CASE
  }
  return tssep_launch_status();
}
extern "C" int tssep_pair_loss_bwd(const float* est, const float* tgt, const int32_t* perm, const float* sums,
                                   const float* gout, int64_t B, int64_t K, int64_t N, int p, float* dest,
                                   void* stream) {
  if (!est || !tgt || !gout || !dest) return TSSEP_E_NULL;        // perm may be NULL (identity), sums may be NULL (no log)
  if (B <= 0 || K <= 0 || K > PIT_MAX_K || N <= 0 || (p != 1 && p != 2)) return TSSEP_E_SHAPE;
  if (p == 1)
    hipLaunchKernelGGL(pair_loss_bwd_kernel<1>, dim3(grid_for(B * K * N)), dim3(256), 0, S_, est, tgt, perm, sums,
                       gout, K, N, B * K * N, dest);
  else
    hipLaunchKernelGGL(pair_loss_bwd_kernel<2>, dim3(grid_for(B * K * N)), dim3(256), 0, S_, est, tgt, perm, sums,
                       gout, K, N, B * K * N, dest);
  return tssep_launch_status();
}
extern "C" int64_t tssep_vadbce_workspace_bytes(int64_t B, int64_t K, int64_t T) {
  return B * K * T * (int64_t)sizeof(float);
}
extern "C" int tssep_vadbce_fwd(const float* logit, const float* vad, int64_t B, int64_t K,
                                int64_t T, int F, float* loss, float* xmean, void* ws,
                                void* stream) {
  if (!logit || !vad || !loss || !xmean || !ws) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0) return TSSEP_E_SHAPE;
  const int64_t rows = B * K * T;
  hipLaunchKernelGGL(vadbce_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, S_, logit,
                     vad, rows, F, xmean, (float*)ws);
  hipLaunchKernelGGL(vadbce_finalize_kernel, dim3((unsigned)B), dim3(256), 0, S_, (const float*)ws,
                     B, K * T, loss);
  return tssep_launch_status();
}
extern "C" int tssep_vadbce_bwd(const float* xmean, const float* vad, const float* gout, int64_t B,
                                int64_t K, int64_t T, int F, float* dlogit, void* stream) {
  if (!xmean || !vad || !gout || !dlogit) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(vadbce_bwd_kernel, dim3(grid_for(B * K * T * F)), dim3(256), 0, S_, xmean, vad,
                     gout, K * T, F, B * K * T * F, dlogit);
  return tssep_launch_status();
}
extern "C" int tssep_gatebce_fwd(const float* logit, int64_t ld, const float* vad, int64_t B, int64_t K, int64_t T,
                                 float* loss, void* ws, void* stream) {
  if (!logit || !vad || !loss || !ws) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || ld <= 0) return TSSEP_E_SHAPE;
  const int64_t rows = B * K * T;
  hipLaunchKernelGGL(gatebce_rows_kernel, dim3(grid_for(rows)), dim3(256), 0, S_, logit, ld, vad, rows, (float*)ws);
  hipLaunchKernelGGL(vadbce_finalize_kernel, dim3((unsigned)B), dim3(256), 0, S_, (const float*)ws, B, K * T, loss);
  return tssep_launch_status();
}
extern "C" int tssep_gatebce_bwd(const float* logit, int64_t ld, const float* vad, const float* gout, int64_t B,
                                 int64_t K, int64_t T, float* dlogit, void* stream) {
  if (!logit || !vad || !gout || !dlogit) return TSSEP_E_NULL;
  if (B <= 0 || K <= 0 || T <= 0 || ld <= 0) return TSSEP_E_SHAPE;
  hipLaunchKernelGGL(gatebce_bwd_kernel, dim3(grid_for(B * K * T * ld)), dim3(256), 0, S_, logit, ld, vad, gout,
                     K * T, B * K * T * ld, dlogit);
  return tssep_launch_status();
}
extern "C" int tssep_framemag_fwd(const float* X, int is_complex, int64_t rows, int64_t T, int64_t F, float* a,
                                  void* stream) {
  if (!X || !a) return TSSEP_E_NULL;
  if (rows <= 0 || T <= 0 || F <= 0) return TSSEP_E_SHAPE;
  if ((((uintptr_t)X) & (is_complex ? 7u : 3u)) || (((uintptr_t)a) & 3u)) return TSSEP_E_ALIGN;
  const int64_t frames = rows * T;
  const unsigned grid = grid_for(frames, 4, 16384);              // one wave per frame, grid-stride beyond the cap
  if (is_complex)
    hipLaunchKernelGGL(framemag_kernel<true>, dim3(grid), dim3(256), 0, S_, X, frames, F, a);
  else
    hipLaunchKernelGGL(framemag_kernel<false>, dim3(grid), dim3(256), 0, S_, X, frames, F, a);
  return tssep_launch_status();
}
extern "C" int tssep_vad_from_mag(const float* a, int64_t rows, int64_t T, double threshold, float* vad, void* stream) {
  if (!a || !vad) return TSSEP_E_NULL;
  if (rows <= 0 || T <= 0) return TSSEP_E_SHAPE;
  if ((((uintptr_t)a) | ((uintptr_t)vad)) & 3u) return TSSEP_E_ALIGN;
  hipLaunchKernelGGL(vad_from_mag_kernel, dim3(grid_for(rows, 1, 65536)), dim3(256), 0, S_, a, rows, T, (float)threshold,
                     vad);
  return tssep_launch_status();
}
extern "C" int tssep_vad_frames(const uint8_t* vad_samples, int64_t rows, int64_t N, int window_length, int shift,
                                int fading, float* Vad, int64_t T, void* stream) {
  if (!vad_samples || !Vad) return TSSEP_E_NULL;
  if (rows <= 0 || N <= 0 || T <= 0 || window_length <= 0 || shift <= 0) return TSSEP_E_SHAPE;
  if (fading < 0 || fading > 2) return TSSEP_E_UNSUPPORTED;
  if (((uintptr_t)Vad) & 3u) return TSSEP_E_ALIGN;
  const int64_t pad = (int64_t)window_length - shift;
  const int64_t lead = fading == 0 ? 0 : (fading == 1 ? pad : (pad >= 0 ? pad / 2 : -((1 - pad) / 2)));   // (Python's //)
  hipLaunchKernelGGL(vad_frames_kernel, dim3(grid_for(rows * T)), dim3(256), 0, S_, vad_samples, N, T, (int64_t)shift,
                     (int64_t)(window_length / 2) - lead - 1, rows * T, Vad);
  return tssep_launch_status();
}
static int map_args(MapArgs& a, const int32_t* perm, const int32_t* iperm, int64_t B, int trials,
                    int64_t K, int64_t T, int F, int Fr, int spk_rows) {
  if (B <= 0 || K <= 0 || T <= 0 || F <= 0 || trials <= 0 || (Fr != F && Fr != 1))
    return TSSEP_E_SHAPE;
  if (spk_rows && trials != 1) return TSSEP_E_UNSUPPORTED;
  if ((perm == nullptr) != (iperm == nullptr)) return TSSEP_E_NULL;
  a.B = B; a.K = K; a.T = T; a.F = F; a.Fr = Fr; a.trials = trials; a.spk_rows = spk_rows;
  a.perm = perm; a.iperm = iperm;
  return TSSEP_OK;
}
extern "C" int tssep_logit_map_fwd(const float* raw, const int32_t* perm, const int32_t* iperm,
                                   int64_t B, int trials, int64_t K, int64_t T, int F, int Fr,
                                   int spk_rows, float* out, void* stream) {
  if (!raw || !out) return TSSEP_E_NULL;
  MapArgs a;
  if (int e = map_args(a, perm, iperm, B, trials, K, T, F, Fr, spk_rows)) return e;
  hipLaunchKernelGGL(logit_map_fwd_kernel, dim3(grid_for(B * K * T * F)), dim3(256), 0, S_, raw, a,
                     out);
  return tssep_launch_status();
}
extern "C" int tssep_logit_map_bwd(const float* dout, const int32_t* perm, const int32_t* iperm,
                                   int64_t B, int trials, int64_t K, int64_t T, int F, int Fr,
                                   int spk_rows, float* draw, void* stream) {
  if (!dout || !draw) return TSSEP_E_NULL;
  MapArgs a;
  if (int e = map_args(a, perm, iperm, B, trials, K, T, F, Fr, spk_rows)) return e;
  if (Fr == 1 && F != 1) {
    const int64_t total = B * trials * T * K;
    hipLaunchKernelGGL(logit_map_bwd_t_kernel, dim3((unsigned)((total + 3) / 4)), dim3(256), 0, S_,
                       dout, a, draw);
  } else {
    hipLaunchKernelGGL(logit_map_bwd_tf_kernel, dim3(grid_for(B * trials * T * K * 64)), dim3(256),
                       0, S_, dout, a, draw);
  }
  return tssep_launch_status();
}

extern "C" int tssep_mask_map_fwd(const float* raw, const int32_t* perm, const int32_t* iperm, int64_t B,
                                  int trials, int64_t K, int M, int64_t T, int F, int Fr, int spk_rows,
                                  float* logit, float* mask, void* stream) {
  if (!raw || !logit || !mask) return TSSEP_E_NULL;
  if (M <= 0) return TSSEP_E_SHAPE;
  MapArgs a;
  if (int e = map_args(a, perm, iperm, B, trials, K, T, F, Fr, spk_rows)) return e;
  hipLaunchKernelGGL(mask_map_fwd_kernel, dim3(grid_for(B * K * M * T * 64)), dim3(256), 0, S_, raw, a, M,
                     logit, mask);
  return tssep_launch_status();
}
extern "C" int tssep_mask_map_bwd(const float* dmask, const float* mask, const float* dlogit,
                                  const int32_t* perm, const int32_t* iperm, int64_t B, int trials, int64_t K,
                                  int M, int64_t T, int F, int Fr, int spk_rows, float* draw, void* stream) {
  if (!dmask || !mask || !draw) return TSSEP_E_NULL;            // dlogit may be NULL (nobody else used logit)
  if (M <= 0) return TSSEP_E_SHAPE;
  MapArgs a;
  if (int e = map_args(a, perm, iperm, B, trials, K, T, F, Fr, spk_rows)) return e;
  const unsigned grid = grid_for(B * trials * T * K * M * 64);
  if (Fr == 1 && F != 1)
    hipLaunchKernelGGL(mask_map_bwd_t_kernel, dim3(grid), dim3(256), 0, S_, dmask, mask, dlogit, a, M, draw);
  else
    hipLaunchKernelGGL(mask_map_bwd_tf_kernel, dim3(grid), dim3(256), 0, S_, dmask, mask, dlogit, a, M, draw);
  return tssep_launch_status();
}
