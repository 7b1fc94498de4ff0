// GRU recurrence (forward and backward-through-time) for gfx950, one or two directions of time.
//
// Replaces the T-sequential part of torch.nn.GRU as the reference uses it (tssep/train/rnnp.py:40,87 typ = 'gru' /
// 'bgru': one layer, batch_first).  The input projection x W_ih^T + b is a plain GEMM done beforehand, as for the LSTM.
//
// Design: lstm.hip's streaming decomposition, unchanged -- 8 sequences x 1 direction per 256-thread workgroup, no
// inter-workgroup exchange, W_hh streamed from L2 through a three-stage register ring that keeps running across time
// steps, the previous step's h in LDS, v_mfma_f32_4x4x1 with block = hidden unit, row = slot, column = sequence, so that
// after the k loop every lane owns the four values of ONE (unit, sequence) cell and the cell update is lane-local.
// Exact fp32 (fmaf chain, OCML tanhf, sigmoidf_acc).
//
// A GRU cell needs four values: the pre-activations of r and z, the input half of n, and q = W_hn h + b_hn, which stays
// apart because r multiplies it.  Four SLOTS per unit (r, z, n, q) therefore keep every shape of the LSTM path,
// G = 4 D H gate columns:
//                        slot 0          slot 1          slot 2      slot 3
//   wih_p row            W_ir[u]         W_iz[u]         W_in[u]     0
//   bias_p               b_ir + b_hr     b_iz + b_hz     b_in        b_hn
//   W_hh row             W_hr[u]         W_hz[u]         0           W_hn[u]
// The input GEMM writes (a_r, a_z, a_n, b_hn) + the recurrent product adds (W_hr h, W_hz h, 0, W_hn h).
// The price of the zero slot: the input GEMM, the gate tensor and the W_hh stream are each 4/3 of a three-row layout.
//
// Packed layouts (tssep_gru_pack), the LSTM's with slot for gate:
//   gate columns: [dir][unit][slot]            (4H per direction)
//   whh_f : [dir][wave 4][kq KQ3][i NB][lane 64][4],  u = (wave*NB + i)*16 + lane/4, slot = lane%4, k = 4kq + e
//   whh_b : [dir][slot 4][kq KQ3][ubb NBB][lane 64][4] = W_hh[row(slot)*H + 4kq + e][ubb*64 + lane]     (BPTT)
// with NB = ceil(ceil(H/16)/4), NBB = ceil(H/64), KQ3 = ceil(ceil(H/4)/3)*3; zero padded.
#include "common.h"

namespace {

__host__ __device__ inline int gru_nb(int H) { return ((H + 15) / 16 + 3) / 4; }
__host__ __device__ inline int gru_nbb(int H) { return (H + 63) / 64; }
__host__ __device__ inline int gru_kq3(int H) { return (((H + 3) / 4 + 2) / 3) * 3; }

// torch's gate-major row block (r, z, n) a slot of the hidden-side matrix reads; -1: the zero slot
__host__ __device__ inline int gru_hh_row(int slot) { return slot == 2 ? -1 : slot == 3 ? 2 : slot; }

// ------------------------------------------------------------------------- pack
__global__ void gru_pack_kernel(const float* w_ih_f, const float* w_hh_f, const float* b_ih_f,
                                const float* b_hh_f, const float* w_ih_r, const float* w_hh_r,
                                const float* b_ih_r, const float* b_hh_r, int H, int I, int64_t ld_i,
                                float* wih_p, float* bias_p, float* whh_f, float* whh_b, int ND) {
  // ND directions (1: the *_r pointers are null and never read -- every d below is 0)
  const int NB = gru_nb(H), NBB = gru_nbb(H), KQ3 = gru_kq3(H);
  const int n_bias = ND * 4 * H;
  const int64_t n_wih = (int64_t)n_bias * ld_i;
  const int64_t n_f = (int64_t)ND * 4 * KQ3 * NB * 256;
  const int64_t n_b = (int64_t)ND * 4 * KQ3 * NBB * 256;
  const int64_t total = n_wih + n_bias + n_f + n_b;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    if (e < n_wih) {
      const int64_t row = e / ld_i, k = e - row * ld_i;
      const int d = (int)(row / (4 * H)), us = (int)(row % (4 * H));
      const int u = us >> 2, s = us & 3;
      const float* w = d ? w_ih_r : w_ih_f;
      wih_p[e] = (k < I && s < 3) ? w[(int64_t)(s * H + u) * I + k] : 0.f;
    } else if (e < n_wih + n_bias) {
      const int row = (int)(e - n_wih);
      const int d = row / (4 * H), us = row % (4 * H);
      const int u = us >> 2, s = us & 3;
      const float* bi = d ? b_ih_r : b_ih_f;
      const float* bh = d ? b_hh_r : b_hh_f;
      bias_p[row] = s < 2 ? bi[s * H + u] + bh[s * H + u] : s == 2 ? bi[2 * H + u] : bh[2 * H + u];
    } else if (e < n_wih + n_bias + n_f) {
      int64_t r = e - n_wih - n_bias;
      const int el = (int)(r & 3); r >>= 2;
      const int lane = (int)(r & 63); r >>= 6;
      const int i = (int)(r % NB); r /= NB;
      const int kq = (int)(r % KQ3); r /= KQ3;
      const int wave = (int)(r & 3);
      const int d = (int)(r >> 2);
      const int u = (wave * NB + i) * 16 + (lane >> 2), g = gru_hh_row(lane & 3), k = 4 * kq + el;
      const float* w = d ? w_hh_r : w_hh_f;
      whh_f[e - n_wih - n_bias] = (g >= 0 && u < H && k < H) ? w[(int64_t)(g * H + u) * H + k] : 0.f;
    } else {
      int64_t r = e - n_wih - n_bias - n_f;
      const int el = (int)(r & 3); r >>= 2;
      const int lane = (int)(r & 63); r >>= 6;
      const int ubb = (int)(r % NBB); r /= NBB;
      const int kq = (int)(r % KQ3); r /= KQ3;
      const int g = gru_hh_row((int)(r & 3));
      const int d = (int)(r >> 2);
      const int unit = ubb * 64 + lane, kk = 4 * kq + el;
      const float* w = d ? w_hh_r : w_hh_f;
      whh_b[e - n_wih - n_bias - n_f] =
          (g >= 0 && unit < H && kk < H) ? w[(int64_t)(g * H + kk) * H + unit] : 0.f;
    }
  }
}

// dst_d[(g*H + u)*ncols + k] = sum_s src[s*split_stride + (d*4H + 4u + slot(g))*ld + k], g = 0..2 (r, z, n);
// slot(g) = g on the input side, (0, 1, 3) on the hidden side
__global__ void gru_unpack_kernel(const float* __restrict__ src, int64_t ld, int nsplit,
                                  int64_t split_stride, int H, int ncols, int hh, float* dst_f,
                                  float* dst_r, int accumulate, int ND) {
  const int64_t per = (int64_t)3 * H * ncols, total = ND * per;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int d = e >= per;
    const int64_t r = e - d * per;
    const int64_t row = r / ncols;
    const int k = (int)(r - row * ncols);
    const int g = (int)(row / H), u = (int)(row % H);
    const int slot = (hh && g == 2) ? 3 : g;
    const float* p = src + ((int64_t)d * 4 * H + 4 * u + slot) * ld + k;
    float s = 0.f;
    for (int i = 0; i < nsplit; ++i) s += p[i * split_stride];
    float* o = (d ? dst_r : dst_f) + r;
    *o = accumulate ? *o + s : s;
  }
}

// --------------------------------------------------------------------- forward
#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_4x4x1f32((a), (b), (c), 0, 0, 0)

// ND = 2: both directions of time, blockIdx.y = direction, zero initial state.  ND = 1: ONE direction, forward in time
// (gates [N,T,H,4], hout columns 0..H-1), with an optional initial state h0 [N,H] and an optional final state hT [N,H];
// everything about the state is compiled out of the ND = 2 instantiation.
template <int NB, int ND>
__global__ __launch_bounds__(256, 1) void gru_fwd_kernel(
    float* __restrict__ gates, float* __restrict__ hout, int64_t ldo, int64_t dstride,
    const float* __restrict__ whh_f, int64_t N, int64_t T, int H, int KQ3,
    const float* __restrict__ h0, float* __restrict__ hT) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int KROW = 4 * KQ3 + 12;
  float* hs = smem;  // [2][8][KROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = ND == 2 ? blockIdx.y : 0;
  const int64_t seq0 = (int64_t)blockIdx.x * 8;
  const int ub = lane >> 2, j = lane & 3;
  for (int i = tid; i < 2 * 8 * KROW; i += 256) hs[i] = 0.f;
  if constexpr (ND == 1) {
    if (h0) {      // (uniform) the previous chunk's last h, behind the zero fill; the barrier below publishes it
      __syncthreads();
      for (int i = tid; i < 8 * H; i += 256) {
        const int s = i / H, k = i - s * H;
        if (seq0 + s < N) hs[s * KROW + k] = h0[(seq0 + s) * H + k];
      }
    }
  }

  const f32x4* W = reinterpret_cast<const f32x4*>(whh_f) +
                   ((int64_t)(dir * 4 + wave) * KQ3) * NB * 64 + lane;
  int64_t nrow[2];
  bool nvalid[2];
#pragma unroll
  for (int sg = 0; sg < 2; ++sg) {
    const int64_t n = seq0 + sg * 4 + j;
    nvalid[sg] = n < N;
    nrow[sg] = nvalid[sg] ? n : 0;
  }
  int u[NB];
  bool uvalid[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    u[i] = (wave * NB + i) * 16 + ub;
    uvalid[i] = u[i] < H;
  }
  float hp[NB][2];      // h of the previous step, per cell (what c is to the LSTM kernel)
#pragma unroll
  for (int i = 0; i < NB; ++i) { hp[i][0] = 0.f; hp[i][1] = 0.f; }
  if constexpr (ND == 1) {
    if (h0) {
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int sg = 0; sg < 2; ++sg)
          if (nvalid[sg] && uvalid[i]) hp[i][sg] = h0[nrow[sg] * H + u[i]];
    }
  }

  f32x4 w0[NB], w1[NB], w2[NB];
#define LOADW(dst, kq_)                                              \
  {                                                                  \
    const f32x4* p_ = W + (int64_t)(kq_) * NB * 64;                  \
    _Pragma("unroll") for (int i = 0; i < NB; ++i) dst[i] = p_[i * 64]; \
  }
#define LOADH(ha_, hb_, kq_)                                            \
  {                                                                     \
    ha_ = *reinterpret_cast<const f32x4*>(hrow0 + 4 * (kq_));           \
    hb_ = *reinterpret_cast<const f32x4*>(hrow1 + 4 * (kq_));           \
  }
#define MM(src, ha_, hb_)                                               \
  {                                                                     \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                     \
      _Pragma("unroll") for (int i = 0; i < NB; ++i) {                  \
        acc[i][0] = MFMA4(src[i][e], ha_[e], acc[i][0]);                \
        acc[i][1] = MFMA4(src[i][e], hb_[e], acc[i][1]);                \
      }                                                                 \
    }                                                                   \
  }
#define SB __builtin_amdgcn_sched_barrier(0)
  LOADW(w0, 0);
  LOADW(w1, 1);
  __syncthreads();

  int cur = 0;
  for (int64_t step = 0; step < T; ++step) {
    const int64_t t = dir ? T - 1 - step : step;
    f32x4 gx[NB][2];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        // streamed once: non-temporal so these lines do not push W_hh out of the XCD's L2
        if (nvalid[sg] && uvalid[i])
          v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(
              gates + (((nrow[sg] * T + t) * ND + dir) * (int64_t)H + u[i]) * 4));
        gx[i][sg] = v;
      }
    f32x4 acc[NB][2];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* hrow0 = hs + (cur * 8 + j) * KROW;
    const float* hrow1 = hs + (cur * 8 + 4 + j) * KROW;
    f32x4 ha0, hb0, ha1, hb1, ha2, hb2;
    LOADH(ha0, hb0, 0);
    LOADH(ha1, hb1, 1);
    for (int kq = 0; kq < KQ3; kq += 3) {
      // 3-stage ring (W from L2, h from LDS), order pinned: the scheduler otherwise sinks the
      // loads to the loop tail and exposes their latency
      LOADW(w2, kq + 2); LOADH(ha2, hb2, kq + 2); SB;
      MM(w0, ha0, hb0); SB;
      LOADW(w0, (kq + 3 < KQ3 ? kq + 3 : 0)); LOADH(ha0, hb0, kq + 3); SB;
      MM(w1, ha1, hb1); SB;
      LOADW(w1, (kq + 4 < KQ3 ? kq + 4 : 1)); LOADH(ha1, hb1, kq + 4); SB;
      MM(w2, ha2, hb2); SB;
    }
    float* hnext = hs + ((cur ^ 1) * 8) * KROW;
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        const f32x4 a = acc[i][sg] + gx[i][sg];
        const float rg = sigmoidf_acc(a[0]), zg = sigmoidf_acc(a[1]);
        const float q = a[3];
        const float ng = tanhf(fmaf(rg, q, a[2]));
        // (the two contractions are written out: every instantiation rounds alike)
        const float h = fmaf(zg, hp[i][sg], (1.f - zg) * ng);
        hp[i][sg] = h;
        if (uvalid[i]) {
          hnext[(sg * 4 + j) * KROW + u[i]] = h;
          if (nvalid[sg]) {
            const int64_t cellidx = ((nrow[sg] * T + t) * ND + dir) * (int64_t)H + u[i];
            __builtin_nontemporal_store(f32x4{rg, zg, ng, q},
                                        reinterpret_cast<f32x4*>(gates + cellidx * 4));
            __builtin_nontemporal_store(h, hout + (nrow[sg] * T + t) * ldo + dir * dstride + u[i]);
            if constexpr (ND == 1) {
              if (step == T - 1 && hT) hT[nrow[sg] * H + u[i]] = h;      // the state a next chunk starts from
            }
          }
        }
      }
    __syncthreads();
    cur ^= 1;
  }
#undef LOADW
}

// -------------------------------------------------------------------- backward
// gates (r, z, n, q) -> (da_r, da_z, da_n, da_q) in place.  dh = dhout[t] + dh z of the later step (lane-local) +
// W_hr^T da_r + W_hz^T da_z + W_hn^T da_q of the later step (wave = slot, partial sums through LDS; the slot-2 wave
// multiplies the zero block).  h_prev = hout at the neighbouring frame of this direction's time order, 0 at its first.
template <int NB, int NBB, int ND>
__global__ __launch_bounds__(256, 1) void gru_bwd_kernel(
    float* __restrict__ gates, const float* __restrict__ hout, const float* __restrict__ dhout,
    int64_t ldo, int64_t dstride, const float* __restrict__ whh_b, int64_t N, int64_t T, int H, int KQ3,
    const float* __restrict__ h0, const float* __restrict__ dhT, float* __restrict__ dh0) {
  // h0 / dhT / dh0: [N, H], ND == 1 only, each may be null (zeros / not wanted)
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int KROW = 4 * KQ3 + 12;
  const int PROW = NBB * 64 + 4;
  float* dgs = smem;                     // [4 slots][8 seqs][KROW]
  float* part = smem + 4 * 8 * KROW;     // [4 waves][8 seqs][PROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int dir = ND == 2 ? blockIdx.y : 0;
  const int64_t seq0 = (int64_t)blockIdx.x * 8;
  const int ub = lane >> 2, j = lane & 3;
  for (int i = tid; i < 4 * 8 * KROW + 4 * 8 * PROW; i += 256) smem[i] = 0.f;

  const f32x4* W = reinterpret_cast<const f32x4*>(whh_b) +
                   ((int64_t)(dir * 4 + wave) * KQ3) * NBB * 64 + lane;
  int64_t nrow[2];
  bool nvalid[2];
#pragma unroll
  for (int sg = 0; sg < 2; ++sg) {
    const int64_t n = seq0 + sg * 4 + j;
    nvalid[sg] = n < N;
    nrow[sg] = nvalid[sg] ? n : 0;
  }
  int u[NB];
  bool uvalid[NB];
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    u[i] = (wave * NB + i) * 16 + ub;
    uvalid[i] = u[i] < H;
  }
  float dhc[NB][2];      // dh z of the later step
#pragma unroll
  for (int i = 0; i < NB; ++i) { dhc[i][0] = 0.f; dhc[i][1] = 0.f; }
  if constexpr (ND == 1) {
    if (dhT) {      // the gradient arriving for the final h: one more addend of the last frame's dh, in the carry's place
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int sg = 0; sg < 2; ++sg)
          if (uvalid[i] && nvalid[sg]) dhc[i][sg] = dhT[nrow[sg] * H + u[i]];
    }
  }

  f32x4 w0[NBB], w1[NBB], w2[NBB];
#define LOADW(dst, kq_)                                                  \
  {                                                                      \
    const f32x4* p_ = W + (int64_t)(kq_) * NBB * 64;                     \
    _Pragma("unroll") for (int i = 0; i < NBB; ++i) dst[i] = p_[i * 64]; \
  }
#undef MM
#define MM(src, ha_, hb_)                                               \
  {                                                                     \
    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                     \
      _Pragma("unroll") for (int i = 0; i < NBB; ++i) {                 \
        acc[i][0] = MFMA4(src[i][e], ha_[e], acc[i][0]);                \
        acc[i][1] = MFMA4(src[i][e], hb_[e], acc[i][1]);                \
      }                                                                 \
    }                                                                   \
  }
  LOADW(w0, 0);
  LOADW(w1, 1);
  __syncthreads();

  for (int64_t step = 0; step < T; ++step) {
    const int64_t t = dir ? step : T - 1 - step;
    const bool has_prev = step + 1 < T;          // an h before this step exists (zero initial state otherwise)
    const int64_t tp = dir ? t + 1 : t - 1;      // its time index
    // ---- cell backward (lane-local) ----
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        f32x4 dg4 = {0.f, 0.f, 0.f, 0.f};
        if (uvalid[i]) {
          const int s = sg * 4 + j;
          float dh = part[(0 * 8 + s) * PROW + u[i]] + part[(1 * 8 + s) * PROW + u[i]] +
                     part[(2 * 8 + s) * PROW + u[i]] + part[(3 * 8 + s) * PROW + u[i]];
          if (nvalid[sg]) {
            const int64_t cellidx = ((nrow[sg] * T + t) * ND + dir) * (int64_t)H + u[i];
            const f32x4 g4 =
                __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(gates + cellidx * 4));
            float hprev = has_prev ? __builtin_nontemporal_load(
                                         hout + (nrow[sg] * T + tp) * ldo + dir * dstride + u[i])
                                   : 0.f;
            dh += __builtin_nontemporal_load(dhout + (nrow[sg] * T + t) * ldo + dir * dstride + u[i]);
            dh += dhc[i][sg];
            if constexpr (ND == 1) {
              if (!has_prev && h0) hprev = h0[nrow[sg] * H + u[i]];      // the state the forward started from
            }
            const float rg = g4[0], zg = g4[1], ng = g4[2], q = g4[3];
            const float dn = dh * (1.f - zg);
            const float dz = dh * (hprev - ng);
            const float dan = dn * fmaf(-ng, ng, 1.f);
            dhc[i][sg] = dh * zg;
            dg4[0] = dan * q * rg * (1.f - rg);
            dg4[1] = dz * zg * (1.f - zg);
            dg4[2] = dan;
            dg4[3] = dan * rg;
            __builtin_nontemporal_store(dg4, reinterpret_cast<f32x4*>(gates + cellidx * 4));
          }
#pragma unroll
          for (int g = 0; g < 4; ++g) dgs[(g * 8 + s) * KROW + u[i]] = dg4[g];
        }
      }
    __syncthreads();
    // ---- dh_prev[unit, seq] = sum_{slot,kk} W_hh[row(slot)*H+kk][unit] * dgates[seq][slot][kk]; wave = slot
    f32x4 acc[NBB][2];
#pragma unroll
    for (int i = 0; i < NBB; ++i) {
      acc[i][0] = f32x4{0.f, 0.f, 0.f, 0.f};
      acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* hrow0 = dgs + (wave * 8 + j) * KROW;
    const float* hrow1 = dgs + (wave * 8 + 4 + j) * KROW;
    f32x4 ha0, hb0, ha1, hb1, ha2, hb2;
    LOADH(ha0, hb0, 0);
    LOADH(ha1, hb1, 1);
    for (int kq = 0; kq < KQ3; kq += 3) {
      // 3-stage ring (W from L2, dgates from LDS), order pinned as in the forward
      LOADW(w2, kq + 2); LOADH(ha2, hb2, kq + 2); SB;
      MM(w0, ha0, hb0); SB;
      LOADW(w0, (kq + 3 < KQ3 ? kq + 3 : 0)); LOADH(ha0, hb0, kq + 3); SB;
      MM(w1, ha1, hb1); SB;
      LOADW(w1, (kq + 4 < KQ3 ? kq + 4 : 1)); LOADH(ha1, hb1, kq + 4); SB;
      MM(w2, ha2, hb2); SB;
    }
#pragma unroll
    for (int i = 0; i < NBB; ++i)
#pragma unroll
      for (int sg = 0; sg < 2; ++sg)
        *reinterpret_cast<f32x4*>(part + (wave * 8 + sg * 4 + j) * PROW + i * 64 + 4 * ub) =
            acc[i][sg];
    __syncthreads();
  }
  if constexpr (ND == 1) {
    if (dh0) {      // the gradient of the initial state: the partial sums and the lane-local carry of one more step
#pragma unroll
      for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int sg = 0; sg < 2; ++sg)
          if (uvalid[i] && nvalid[sg]) {
            const int s = sg * 4 + j;
            const float p = part[(0 * 8 + s) * PROW + u[i]] + part[(1 * 8 + s) * PROW + u[i]] +
                            part[(2 * 8 + s) * PROW + u[i]] + part[(3 * 8 + s) * PROW + u[i]];
            dh0[nrow[sg] * H + u[i]] = p + dhc[i][sg];
          }
    }
  }
#undef LOADW
#undef LOADH
#undef MM
#undef SB
}

// ------------------------------------------------------------------- launchers
int pack_sizes(int ND, int H, int I, int64_t ld_i, tssep_lstm_sizes* out) {
  if (!out) return TSSEP_E_NULL;
  if ((ND != 1 && ND != 2) || H <= 0 || I <= 0 || ld_i < I || (ld_i & 3)) return TSSEP_E_SHAPE;
  if (gru_nb(H) > 8) return TSSEP_E_UNSUPPORTED;      // H <= 512
  out->wih_p = (int64_t)ND * 4 * H * ld_i;
  out->bias_p = (int64_t)ND * 4 * H;
  out->whh_f = (int64_t)ND * 4 * gru_kq3(H) * gru_nb(H) * 256;
  out->whh_b = (int64_t)ND * 4 * gru_kq3(H) * gru_nbb(H) * 256;
  return TSSEP_OK;
}

template <int ND>
int launch_fwd(float* gates, float* hout, int64_t ldo, int64_t dstride, const float* whh_f,
               const float* h0, float* hT, int64_t N, int64_t T, int H, void* stream) {
  if (!aligned16(gates) || !aligned16(whh_f)) return TSSEP_E_ALIGN;
  const int NB = gru_nb(H), KQ3 = gru_kq3(H);
  if (NB > 8) return TSSEP_E_UNSUPPORTED;
  dim3 grid((unsigned)((N + 7) / 8), ND);
  const size_t lds = (size_t)2 * 8 * (4 * KQ3 + 12) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
#define L(NB_)                                                                                  \
  hipLaunchKernelGGL((gru_fwd_kernel<NB_, ND>), grid, dim3(256), lds, s, gates, hout, ldo,      \
                     dstride, whh_f, N, T, H, KQ3, h0, hT)
  switch (NB) {
    case 1: L(1); break;
    case 2: L(2); break;
    case 3: L(3); break;
    case 4: L(4); break;
    case 5: L(5); break;
    case 6: L(6); break;
    case 7: L(7); break;
    default: L(8); break;
  }
#undef L
  return tssep_launch_status();
}

template <int ND>
int launch_bwd(float* gates, const float* hout, const float* dhout, int64_t ldo, int64_t dstride,
               const float* whh_b, const float* h0, const float* dhT, float* dh0, int64_t N, int64_t T,
               int H, void* stream) {
  if (!aligned16(gates) || !aligned16(whh_b)) return TSSEP_E_ALIGN;
  const int NB = gru_nb(H), NBB = gru_nbb(H), KQ3 = gru_kq3(H);
  if (NB > 8) return TSSEP_E_UNSUPPORTED;
  dim3 grid((unsigned)((N + 7) / 8), ND);
  const size_t lds = (size_t)(4 * 8 * (4 * KQ3 + 12) + 4 * 8 * (NBB * 64 + 4)) * sizeof(float);
  hipStream_t s = (hipStream_t)stream;
#define L(NB_)                                                                                 \
  hipLaunchKernelGGL((gru_bwd_kernel<NB_, NB_, ND>), grid, dim3(256), lds, s, gates, hout,     \
                     dhout, ldo, dstride, whh_b, N, T, H, KQ3, h0, dhT, dh0)
  // NB = ceil(ceil(H/16)/4) and NBB = ceil(H/64) are the same number
  switch (NB == NBB ? NB : 0) {
    case 1: L(1); break;
    case 2: L(2); break;
    case 3: L(3); break;
    case 4: L(4); break;
    case 5: L(5); break;
    case 6: L(6); break;
    case 7: L(7); break;
    case 8: L(8); break;
    default: return TSSEP_E_UNSUPPORTED;
  }
#undef L
  return tssep_launch_status();
}

}  // namespace

extern "C" int tssep_gru_pack_sizes(int nd, int H, int I, int64_t ld_i, tssep_lstm_sizes* out) {
  return pack_sizes(nd, H, I, ld_i, out);
}

extern "C" int tssep_gru_pack(int nd, const float* w_ih_f, const float* w_hh_f, const float* b_ih_f,
                              const float* b_hh_f, const float* w_ih_r, const float* w_hh_r,
                              const float* b_ih_r, const float* b_hh_r, int H, int I, int64_t ld_i,
                              float* wih_p, float* bias_p, float* whh_f, float* whh_b, void* stream) {
  if (!w_ih_f || !w_hh_f || !b_ih_f || !b_hh_f || !wih_p || !bias_p || !whh_f || !whh_b)
    return TSSEP_E_NULL;
  if (nd == 2 && (!w_ih_r || !w_hh_r || !b_ih_r || !b_hh_r)) return TSSEP_E_NULL;
  tssep_lstm_sizes sz;
  if (int e = pack_sizes(nd, H, I, ld_i, &sz)) return e;
  if (!aligned16(wih_p) || !aligned16(whh_f) || !aligned16(whh_b)) return TSSEP_E_ALIGN;
  const int64_t total = sz.wih_p + sz.bias_p + sz.whh_f + sz.whh_b;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(gru_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     w_ih_f, w_hh_f, b_ih_f, b_hh_f, w_ih_r, w_hh_r, b_ih_r, b_hh_r, H, I, ld_i,
                     wih_p, bias_p, whh_f, whh_b, nd);
  return tssep_launch_status();
}

extern "C" int tssep_gru_unpack(int nd, const float* src, int64_t ld, int nsplit, int64_t split_stride,
                                int H, int ncols, int which, float* dst_f, float* dst_r,
                                int accumulate, void* stream) {
  if (!src || !dst_f || (nd == 2 && !dst_r)) return TSSEP_E_NULL;
  if ((nd != 1 && nd != 2) || H <= 0 || ncols <= 0 || nsplit <= 0 ||
      (which != TSSEP_GRU_IH && which != TSSEP_GRU_HH))
    return TSSEP_E_SHAPE;
  const int64_t total = (int64_t)nd * 3 * H * ncols;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(gru_unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     src, ld, nsplit, split_stride, H, ncols, which == TSSEP_GRU_HH, dst_f, dst_r,
                     accumulate, nd);
  return tssep_launch_status();
}

extern "C" int tssep_gru_fwd(float* gates, float* hout, int64_t ldo, int64_t dstride,
                             const float* whh_f, int64_t N, int64_t T, int H, void* stream) {
  if (!gates || !hout || !whh_f) return TSSEP_E_NULL;
  if (N <= 0 || T <= 0 || H <= 0 || dstride < H || ldo < dstride + H) return TSSEP_E_SHAPE;
  return launch_fwd<2>(gates, hout, ldo, dstride, whh_f, nullptr, nullptr, N, T, H, stream);
}

extern "C" int tssep_gru_bwd(float* gates, const float* hout, const float* dhout, int64_t ldo,
                             int64_t dstride, const float* whh_b, int64_t N, int64_t T, int H,
                             void* stream) {
  if (!gates || !hout || !dhout || !whh_b) return TSSEP_E_NULL;
  if (N <= 0 || T <= 0 || H <= 0 || dstride < H || ldo < dstride + H) return TSSEP_E_SHAPE;
  return launch_bwd<2>(gates, hout, dhout, ldo, dstride, whh_b, nullptr, nullptr, nullptr, N, T, H, stream);
}

// ---- one direction of time (typ = 'gru'): the same kernels with ND = 1 ----
extern "C" int tssep_gru1_fwd(float* gates, float* hout, int64_t ldo, const float* whh_f,
                              const float* h0, float* hT, int64_t N, int64_t T, int H, void* stream) {
  if (!gates || !hout || !whh_f) return TSSEP_E_NULL;
  if (N <= 0 || T <= 0 || H <= 0 || ldo < H) return TSSEP_E_SHAPE;
  return launch_fwd<1>(gates, hout, ldo, 0, whh_f, h0, hT, N, T, H, stream);
}

extern "C" int tssep_gru1_bwd_state(float* gates, const float* hout, const float* dhout, int64_t ldo,
                                    const float* whh_b, const float* h0, const float* dhT, float* dh0,
                                    int64_t N, int64_t T, int H, void* stream) {
  if (!gates || !hout || !dhout || !whh_b) return TSSEP_E_NULL;      // every state argument may be null
  if (N <= 0 || T <= 0 || H <= 0 || ldo < H) return TSSEP_E_SHAPE;
  return launch_bwd<1>(gates, hout, dhout, ldo, 0, whh_b, h0, dhT, dh0, N, T, H, stream);
}

extern "C" int tssep_gru1_bwd(float* gates, const float* hout, const float* dhout, int64_t ldo,
                              const float* whh_b, int64_t N, int64_t T, int H, void* stream) {
  return tssep_gru1_bwd_state(gates, hout, dhout, ldo, whh_b, nullptr, nullptr, nullptr, N, T, H, stream);
}
