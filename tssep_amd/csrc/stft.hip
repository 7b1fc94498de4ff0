// STFT / inverse STFT / adjoint of the inverse STFT with paderbox semantics, size 1024.
//
// Replaces fe.stft (tssep/train/model.py:503-504) and fe.istft (tssep/train/model.py:661-664;
// third-party padertorch/paderbox code, restated in oracle/stft.py) and the autograd backward
// of the latter.
//
// FFT plan: a 1024-point real FFT is a 512-point complex FFT of z[n] = x[2n] + i x[2n+1]
// plus a butterfly pass.  The 512-point transform is a Stockham autosort radix-8 x 3
// (Govindaraju et al. formulation): ONE WAVE per frame, 8 complex points per lane in
// registers, three in-register 8-point DFTs, the two transposes in between through a
// per-wave LDS line.  The line index is padded (i + i/8) so the stride-8 scatter of the
// first stage is bank-conflict free for ds_write_b64.
//
// All three kernels are HBM/L2 streaming kernels in the roofline sense
// (5 128 B per frame for the STFT, K x 5 128 B per frame for the inverse).
#include <math.h>
#include "common.h"

namespace {

// Buffer resources for the frame streams: one 4-SGPR descriptor per row (base + byte range) and ONE 32-bit lane
// offset; the r-th access of a lane is an immediate offset.  Out-of-range elements (the fading zeros in front of a
// row, the padding behind it) read as 0 by the range check -- no per-load masks, no per-load 64-bit addresses.
typedef __amdgpu_buffer_rsrc_t srd_t;
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ srd_t make_srd(const void* p, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)(bytes > 0x7fffffff ? 0x7fffffff : bytes), 0x00020000);
}
__device__ __forceinline__ float2 bload2(srd_t r, unsigned voff) {
  const u32x2_t v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, 0, 0);
  return make_float2(__uint_as_float(v[0]), __uint_as_float(v[1]));
}

__device__ __forceinline__ float bload1(srd_t r, unsigned voff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, 0, 0));
}
__device__ __forceinline__ void bstore1(srd_t r, unsigned voff, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)voff, 0, 0);
}

constexpr int NH = 512;          // complex FFT length
constexpr int LINE = NH + NH / 8;  // padded LDS line (float2)
#define PADI(i) ((i) + ((i) >> 3))
#define WAVE_SYNC()                                          \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
  } while (0)

__device__ __forceinline__ float2 cmul(float2 a, float2 b) {
  return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }  // a * (-i)

// in-register 8-point DFT (forward, exp(-2 pi i nk/8)), natural order in and out
__device__ __forceinline__ void fft8(float2 (&v)[8]) {
  const float h = 0.70710678118654752440f;
  float2 a0 = cadd(v[0], v[4]), a4 = csub(v[0], v[4]);
  float2 a1 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]);
  float2 a2 = cadd(v[2], v[6]), a6 = csub(v[2], v[6]);
  float2 a3 = cadd(v[3], v[7]), a7 = csub(v[3], v[7]);
  a5 = make_float2(h * (a5.x + a5.y), h * (a5.y - a5.x));   // * exp(-i pi/4)
  a6 = mul_mi(a6);                                          // * (-i)
  a7 = make_float2(h * (a7.y - a7.x), -h * (a7.x + a7.y));  // * exp(-3 i pi/4)
  float2 b0 = cadd(a0, a2), b2 = csub(a0, a2), b1 = cadd(a1, a3), b3 = mul_mi(csub(a1, a3));
  float2 b4 = cadd(a4, a6), b6 = csub(a4, a6), b5 = cadd(a5, a7), b7 = mul_mi(csub(a5, a7));
  v[0] = cadd(b0, b1); v[4] = csub(b0, b1);
  v[2] = cadd(b2, b3); v[6] = csub(b2, b3);
  v[1] = cadd(b4, b5); v[5] = csub(b4, b5);
  v[3] = cadd(b6, b7); v[7] = csub(b6, b7);
}

// tw2[lane + 64 r] = exp(-2 pi i (lane + 64 r) / 1024) = tw2[lane] * exp(-2 pi i r / 16): one per-lane value
// loaded once per kernel and eight compile-time constants, instead of eight table loads from global memory
// in every frame's dependent chain
__device__ __forceinline__ float2 tw16(int r) {
  constexpr float c[8] = {1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f,
                          0.0f, -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f};
  constexpr float sn[8] = {0.0f, -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f,
                           -1.0f, -0.92387953251128674f, -0.70710678118654752f, -0.38268343236508977f};
  return make_float2(c[r], sn[r]);
}

// w[r] = tw2_lane * exp(-2 pi i r / 16), r < 8: three complex products (r = 1, 2, 3); r + 4 is a further factor -i
__device__ __forceinline__ void lane_twiddles(float2 tw2_lane, float2 (&w)[8]) {
  w[0] = tw2_lane;
#pragma unroll
  for (int r = 1; r < 4; ++r) w[r] = cmul(tw2_lane, tw16(r));
#pragma unroll
  for (int r = 0; r < 4; ++r) w[r + 4] = mul_mi(w[r]);
}

// 512-point forward FFT by one wave.  In: v[r] = z[lane + 64 r].  Out: buf[PADI(k)] = Z[k].
// twl[k] = exp(-2 pi i k / 512) (LDS copy).  The line is private to the wave: LDS operations of one
// wave execute in order, so the hand-offs between lanes need only a wave-level fence (the compiler
// must not reorder them) -- block-wide barriers here coupled the 4 independent waves of a block
// five times per frame.
__device__ __forceinline__ void fft512_wave(float2 (&v)[8], float2* buf, const float2* twl, int lane) {
  fft8(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[PADI(8 * lane + r)] = v[r];
  WAVE_SYNC();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[PADI(lane + 64 * r)];
  WAVE_SYNC();
  {
    const int k = lane & 7;
#pragma unroll
    for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], twl[k * r * 8]);
    fft8(v);
    const int d = (lane >> 3) * 64 + k;
#pragma unroll
    for (int r = 0; r < 8; ++r) buf[PADI(d + 8 * r)] = v[r];
  }
  WAVE_SYNC();
#pragma unroll
  for (int r = 0; r < 8; ++r) v[r] = buf[PADI(lane + 64 * r)];
  WAVE_SYNC();
#pragma unroll
  for (int r = 1; r < 8; ++r) v[r] = cmul(v[r], twl[lane * r]);
  fft8(v);
#pragma unroll
  for (int r = 0; r < 8; ++r) buf[PADI(lane + 64 * r)] = v[r];
  WAVE_SYNC();
}

// frames -> rfft.  Used as the STFT (window = analysis window, scales 1) and as the adjoint of
// the inverse STFT (window = synthesis window, interior bins x 2/1024, DC/Nyquist x 1/1024).
// tw: [512] exp(-2 pi i k/512) followed by [513] exp(-2 pi i k/1024).
//
// MASKED = true fuses the mask head's backward into the adjoint (tssep/train/net.py:983 sigmoid +
// tssep/train/enhancer.py:98-100 Masking, backward): a frame's d(estimate) bin never leaves the wave;
// the epilogue reads the logit (4 B) and the observation bin (8 B, shared by the K speakers of an
// utterance: L2) and writes d(logit) = Re(conj(Obs) dEst) m (1 - m), m = sigmoid(logit) -- the chain
// adjoint -> mask head moves 8 K F + 8 F bytes per frame instead of 24 K F + 8 F.
//
// GATED (MASKED only; MaskEstimator_v2(explicit_vad=True), net.py:969-979): logit rows hold F + 1 = 514 floats, the frame's
// VAD logit v at column 0 and the mask logits l_f at 1..F; the mask is sigmoid(l_f) sigmoid(v).  Each d(l_f) is formed
// like the ungated one with the gate as one more factor, and d(v) = g (1 - g) sum_f dm_f sigmoid(l_f) by an in-wave
// reduction over the frame's bins (fixed order: deterministic) -- stored by lane 0 at column 0, where the Linear's
// backward reads it.  vad != NULL folds the VADSigmoidBCE gradient of the gate column into that store:
// + gbce[b] (sigmoid(v) - vad[row, t]) inv_kt (loss.py:302-310, 348-395).
#ifndef TSSEP_RFFT_OCC
#define TSSEP_RFFT_OCC 3
#endif
//
// MAG (plain only; the VAD losses' STFT-magnitude target, loss.py:312-327): no spectrum is written; the epilogue sums
// |X[k]| = sqrtf(re^2 + im^2) of the bins it formed -- per lane over k = lane, lane + 64, ..., the Nyquist bin by lane 0,
// then across the wave: a fixed order -- and lane 0 stores the frame's magnitude at dlogit[row * T + t].
//
// STREAM (plain only; tssep_stft_stream_fwd): x is the NEW samples of a live signal, [rows, T * 256], and `tail` the 768
// samples in front of them ([rows, 768]; NULL: zeros, the leading fade).  Frame t reads the virtual concatenation
// [tail | x] at 256 t: sample pair lane + 64 r lies in the tail while 2 t + r < 6 -- for all lanes of the wave at once, so
// each of the eight loads picks one of two descriptors by a scalar condition.  Everything behind the loads is the code of
// the whole-signal transform: the frames carry its bits.
//
// STREAM == 2 (tssep_istft_stream_bwd / tssep_mask_istft_stream_bwd; plain, masked and gated): the adjoint of the streaming
// inverse STFT.  x is dy [rows, N], the gradient of the hops the call completed, `tail` the gradient d_ola_out [rows, 768]
// of the carry behind the call (NULL: zeros) and pad_left = 256 skip.  Call-frame t reads the virtual concatenation
// g = [skip zero hops | dy (zeros from N on, up to hop T) | d_ola_out] at 256 t, where the hops from T on are d_ola_out
// whatever skip is (skip > T: the zeros end at hop T).  The half hop r of the frame lies in hop t + r / 2 of g, for all
// lanes of the wave at once, so each of the eight loads picks its descriptor -- an empty one for the zero hops -- by a
// scalar condition.  An odd N or a dy that is not 8-byte aligned (a sample pair may straddle the end
// of the row) reads every pair as two 4-byte loads through the same descriptors: the range check stays the only mask.
template <bool MASKED, bool GATED = false, bool MAG = false, int STREAM = 0>
__global__ __launch_bounds__(256, TSSEP_RFFT_OCC) void rfft_frames_kernel(
    const float* __restrict__ x, int64_t rows, int64_t N, int64_t T, int shift, int pad_left,
    const float* __restrict__ window, const float2* __restrict__ tw, float2* __restrict__ X,
    float s_in, float s_edge, int iters, const float* __restrict__ logit,
    const float2* __restrict__ obs, float* __restrict__ dlogit, int64_t Kspk,
    const float* __restrict__ tgt, const float* __restrict__ sums, const float* __restrict__ gout,
    const int32_t* __restrict__ iperm, int bt_major, const float* __restrict__ vad = nullptr,
    const float* __restrict__ gbce = nullptr, float inv_kt = 0.f, const float* __restrict__ tail = nullptr) {
  static_assert(MASKED || !GATED, "the gate belongs to the mask head");
  static_assert(!MASKED || !MAG, "the frame magnitudes are the plain STFT's");
  static_assert(STREAM != 1 || (!MASKED && !MAG), "the streaming STFT is the plain transform");
  static_assert(STREAM != 2 || !MAG, "the stream adjoint forms spectra or logit gradients");
  constexpr int LDL = NH + 1 + (GATED ? 1 : 0);   // logit / d(logit) row length
  constexpr int C0 = GATED ? 1 : 0;               // column of bin 0
  // MASKED with tgt != NULL: x is the time-domain ESTIMATE and the frame's samples are the loss gradient
  // d LogMAE / d est = gout[b] sign(est - tgt) / (N ln10 sums[b])  (sums == NULL: MAE, gout[b] sign / N;
  // tssep/train/loss.py:214-216, 244-247) formed while they are loaded -- tssep_logmae_bwd and its [B,K,N]
  // gradient leave the step.  bt_major: d(logit) is stored where the final Linear's backward reads it, rows
  // (b,t) x (speaker position iperm[b,k], f) -- the inverse of the store remap of the forward
  // (net.py:637-641, 957-967) -- instead of [B,K,T,F] + tssep_logit_map_bwd.
  __shared__ float2 twl[NH];
  __shared__ float2 wl[NH];               // the window as sample pairs: read per frame from LDS -- as global loads the
  __shared__ float2 line[4][LINE];        // compiler kept eight 64-bit per-lane addresses alive across the frame loop
  const int tid = threadIdx.x, lane = tid & 63;
  // (wave-uniform; through readfirstlane so that the per-frame buffer resources below are built in SGPRs -- from a
  // VGPR the compiler wraps EVERY buffer access in a waterfall loop: ~10 extra instructions and a serialisation each)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int i = tid; i < NH; i += 256) { twl[i] = tw[i]; wl[i] = reinterpret_cast<const float2*>(window)[i]; }
  __syncthreads();
  const float2 tw2_lane = tw[NH + lane];
  const int64_t total = rows * T;
  for (int it = 0; it < iters; ++it) {
    const int64_t fidx = ((int64_t)blockIdx.x * iters + it) * 4 + wave;
    const bool valid = fidx < total;
    const int64_t row = valid ? fidx / T : 0;
    const int64_t t = valid ? fidx - row * T : 0;
    const int64_t base = t * shift - pad_left;
    const float* xr = x + row * N;
    // Sample loads, branch-free per lane: the eight loads of a frame go out back to back and are waited for
    // once.  (With per-lane branches around them the compiler waited for each load before issuing the
    // next: eight serialised round trips per frame.)  Wave-uniform fast path: N even, x 8-byte aligned and
    // the frame start even -> every sample pair is one aligned float2 that lies inside the row or outside
    // it as a whole; otherwise two clamped 4-byte loads per pair.
    const bool lossgrad = MASKED && tgt != nullptr;          // kernel-uniform
    const float* tr_ = lossgrad ? tgt + row * N : xr;
    float coef = 0.f;
    if (lossgrad) {
      const int64_t b = row / Kspk;
      coef = sums ? gout[b] / ((float)N * 2.30258509299404568402f * sums[b]) : gout[b] / (float)N;
    }
    auto lg = [&](float e, float t_) { const float d = e - t_; return d > 0.f ? coef : (d < 0.f ? -coef : 0.f); };
    const bool fast = ((N & 1) == 0) && ((base & 1) == 0) && ((((uintptr_t)x) & 7u) == 0) &&
                      (!lossgrad || (((uintptr_t)tgt) & 7u) == 0);
    float2 v[8];
    if (!valid) {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = make_float2(0.f, 0.f);
    } else if constexpr (STREAM == 2) {
      // (base and range of the part are picked as scalars and the descriptor built from them, and the two load widths
      // have a loop each: with a three-way pick of whole descriptors and the width inside one loop the compiler turned
      // every load into a chain of scalar branches, 7 % of the launch at 253 frames)
      const float* cp = tail ? tail + row * 768 : xr;
      const int64_t cbytes = tail ? 768 * 4 : 0;
      const int skip_h = pad_left >> 8, Ti = (int)T;             // (T <= 2^20: the launcher's guard)
      const bool pairs = ((N & 1) == 0) && ((((uintptr_t)x) & 7u) == 0);     // (kernel-uniform)
      auto part = [&](int r, unsigned& vo) __attribute__((always_inline)) {
        const int h = (int)t + (r >> 1);                         // the hop of g this half hop lies in (wave-uniform)
        // (the carry first: with skip > T a hop T <= h < skip is a pending hop the call's frames added to -- the forward
        // skips only hops it would have STORED)
        const bool carry = h >= Ti, zero = !carry && h < skip_h;
        const int h0 = carry ? h - Ti : (zero ? 0 : h - skip_h);
        vo = (unsigned)(((h0 * 256 + (r & 1) * 128) + 2 * lane) * 4);
        return make_srd(carry ? cp : xr, carry ? cbytes : (zero ? (int64_t)0 : N * 4));
      };
      float2 xv[8];
      if (pairs) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          unsigned vo;
          const srd_t s = part(r, vo);
          xv[r] = bload2(s, vo);
        }
      } else {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          unsigned vo;
          const srd_t s = part(r, vo);
          xv[r] = make_float2(bload1(s, vo), bload1(s, vo + 4u));
        }
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float2 wv = wl[lane + 64 * r];
        v[r] = make_float2(xv[r].x * wv.x, xv[r].y * wv.y);
      }
    } else if constexpr (STREAM == 1) {
      const srd_t sx = make_srd(xr, N * 4), st = make_srd(tail ? tail + row * 768 : xr, tail ? 768 * 4 : 0);
      const unsigned vo = (unsigned)((t * 256 + 2 * lane) * 4);
      float2 xv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const bool in_tail = 2 * t + r < 6;                    // (wave-uniform)
        xv[r] = bload2(in_tail ? st : sx, vo + 512u * r - (in_tail ? 0u : 768u * 4u));
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float2 wv = wl[lane + 64 * r];
        v[r] = make_float2(xv[r].x * wv.x, xv[r].y * wv.y);
      }
    } else if (fast) {
      // (base + 2 lane + 128 r) may be negative or beyond the row: as an unsigned byte offset it then lies outside
      // the descriptor's range and the pair reads as (0, 0)
      const unsigned vo = (unsigned)((base + 2 * lane) * 4);
      const srd_t sx = make_srd(xr, N * 4);
      float2 xv[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) xv[r] = bload2(sx, vo + 512u * r);
      if (lossgrad) {
        const srd_t st_ = make_srd(tr_, N * 4);
        float2 tv[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) tv[r] = bload2(st_, vo + 512u * r);
#pragma unroll
        for (int r = 0; r < 8; ++r) xv[r] = make_float2(lg(xv[r].x, tv[r].x), lg(xv[r].y, tv[r].y));
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const float2 wv = wl[lane + 64 * r];
        v[r] = make_float2(xv[r].x * wv.x, xv[r].y * wv.y);
      }
    } else {
      float xa[8], xb[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int64_t i0 = base + 2 * (lane + 64 * r), i1 = i0 + 1;
        const int64_t c0 = i0 < 0 ? 0 : (i0 >= N ? N - 1 : i0), c1 = i1 < 0 ? 0 : (i1 >= N ? N - 1 : i1);
        xa[r] = xr[c0];
        xb[r] = xr[c1];
        if (lossgrad) { xa[r] = lg(xa[r], tr_[c0]); xb[r] = lg(xb[r], tr_[c1]); }
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int64_t i0 = base + 2 * (lane + 64 * r), i1 = i0 + 1;
        const float2 wv = wl[lane + 64 * r];
        v[r] = make_float2((i0 >= 0 && i0 < N) ? xa[r] * wv.x : 0.f, (i1 >= 0 && i1 < N) ? xb[r] * wv.y : 0.f);
      }
    }
    float2* buf = line[wave];
    // MASKED: row = (utterance b, speaker); the observation frame is the utterance's.  The epilogue's logit and
    // observation bins do not depend on the transform: requested BEFORE it (24 registers), their latency hides
    // behind the FFT instead of ending every frame with a round trip to memory
    const float* Lr = MASKED ? logit + fidx * LDL : nullptr;
    const float2* Or = MASKED ? obs + ((row / Kspk) * T + t) * (NH + 1) : nullptr;
    float lg8[8];
    float2 ob8[8];
    float lgate = 0.f;                        // GATED: the frame's VAD logit (every lane the same address)
    float vadv = 0.f, gbv = 0.f;              // GATED with the BCE fold: Vad[row, t], gbce[b] -- requested here too, so that
                                              // the d(v) store at the frame's end does not wait for a round trip
    if (GATED && valid && vad) {
      vadv = vad[row * T + t];
      gbv = gbce[row / Kspk];
    }
    if (MASKED && valid) {
      __builtin_amdgcn_sched_barrier(0);      // (not above the sample loads: the kernel is at its register ceiling there)
      const srd_t sl = make_srd(Lr, LDL * 4), so = make_srd(Or, (NH + 1) * 8);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        ob8[r] = bload2(so, (unsigned)(lane * 8 + 512 * r));
        lg8[r] = bload1(sl, (unsigned)(C0 * 4 + lane * 4 + 256 * r));
      }
      if (GATED) lgate = bload1(sl, 0u);
    }
    fft512_wave(v, buf, twl, lane);
    if (valid) {
      float2* Xo = (MASKED || MAG) ? nullptr : X + fidx * (NH + 1);
      float* Dr = MASKED ? dlogit + fidx * LDL : nullptr;
      if (MASKED && bt_major) {
        const int64_t b = row / Kspk, j = row - b * Kspk;
        const int64_t kpos = iperm ? (int64_t)iperm[b * Kspk + j] : j;
        Dr = dlogit + ((b * T + t) * Kspk + kpos) * LDL;
      }
      const float gm = GATED ? sigmoidf_mask(lgate) : 1.f;
      float gpart = 0.f;                      // GATED: this lane's sum_f dm_f sigmoid(l_f); MAG: this lane's sum_f |X_f|
      auto emit = [&](int k, float2 o, float lgk, float2 ob) {
        if (GATED) {
          const float s = sigmoidf_mask(lgk);
          const float dm = ob.x * o.x + ob.y * o.y;
          Dr[C0 + k] = dm * gm * s * (1.0f - s);
          gpart += dm * s;
        } else if (MASKED) {
          const float m = sigmoidf_mask(lgk);
          Dr[k] = (ob.x * o.x + ob.y * o.y) * m * (1.0f - m);
        } else if (MAG) {
          gpart += sqrtf(o.x * o.x + o.y * o.y);
        } else {
          Xo[k] = o;
        }
      };
      float2 wr[8];
      lane_twiddles(tw2_lane, wr);
      const float hs_in = 0.5f * s_in;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int k = lane + 64 * r;
        const float2 zk = buf[PADI(k)];
        const int km = (NH - k) & (NH - 1);
        float2 zm = buf[PADI(km)];
        zm.y = -zm.y;
        const float2 u = cmul(wr[r], csub(zk, zm));
        float2 o = make_float2(zk.x + zm.x + u.y, zk.y + zm.y - u.x);
        if (k == 0) {
          o.x *= 0.5f * s_edge; o.y = 0.f;
        } else {
          o.x *= hs_in; o.y *= hs_in;
        }
        emit(k, o, MASKED ? lg8[r] : 0.f, MASKED ? ob8[r] : make_float2(0.f, 0.f));
      }
      if (lane == 0) {
        const float2 z0 = buf[0];
        emit(NH, make_float2((z0.x - z0.y) * s_edge, 0.f), MASKED ? Lr[C0 + NH] : 0.f, MASKED ? Or[NH] : make_float2(0.f, 0.f));
      }
      if (GATED) {
        const float tot = wave_sum(gpart);
        if (lane == 0) {
          float dv = tot * gm * (1.0f - gm);
          if (vad) dv += gbv * (sigmoidf_acc(lgate) - vadv) * inv_kt;
          Dr[0] = dv;
        }
      }
      if (MAG) {
        const float tot = wave_sum(gpart);
        if (lane == 0) dlogit[fidx] = tot;
      }
    }
    WAVE_SYNC();          // the line is rewritten by this wave's next frame
  }
}

// inverse STFT: a workgroup walks `hcb` consecutive output hops of one row.  Its 4 waves inverse-transform
// 4 consecutive frames per iteration into a RING of 7 windowed frames in LDS (4 being written + the 3
// older ones the pending hops still need); after each iteration the hops whose 4 contributing frames are
// complete are emitted: every output sample sums its <= 4 frame contributions in a fixed order
// (deterministic overlap-add).  Only the first 3 frames of a chunk are transformed twice (by the
// neighbouring chunk as well): 66 transforms per 63 hops.  Round 1 parked HC + 3 = 12 frames per 9 hops
// (a third of all transforms redundant, 48 KB of LDS, two workgroups per CU); the ring needs 28 KB and
// three workgroups fit.
constexpr int RING = 7;
constexpr int HCB_MAX = 64;              // hops per workgroup (upper bound; the launcher balances the chunks)

//
// MASKED = true fuses the mask head in front (net.py:983 + enhancer.py:98-100): a frame's spectrum is
// formed in the wave's LDS line as sigmoid(logit) * Obs (logit 4 B per bin; the 8-B observation bin is
// shared by the K speakers of an utterance: L2) -- neither the mask nor the masked STFT is written;
// the chain mask head -> inverse STFT moves (4 K F + 8 F) + 4 K 256 bytes per frame instead of
// 16 K F + 8 F + 8 K F + 4 K 256.  (Measured, batch 768: 2.07 ms against 1.44 + 1.98 ms; the kernel is bound
// by the per-wave FFT chain, not by bytes: the hardware exp / rcp sigmoid instead of the accurate one changed
// nothing, three resident workgroups instead of two gained 20 %.)
//
// GATED (MASKED only, explicit_vad): logit rows of F + 1 floats, the VAD logit v at column 0; the spectrum is
// sigmoid(l_f) sigmoid(v) Obs -- one more 4-B load per frame, requested with the frame's bins.
#ifndef TSSEP_ISTFT_OCC
#define TSSEP_ISTFT_OCC 3            // waves per SIMD the register allocation aims at (A/B: build with -D...=2)
#endif
//
// STREAM (tssep_istft_stream_fwd / tssep_mask_istft_stream_fwd): the T frames are the NEXT frames of a live stream and
// y [rows, N] the hops they complete.  Hop j = 0 .. T - 1 of the call sums ring frames j .. j + 3 as above, where ring
// frame l stands for frame l - 3 of the call: ring frames 0, 1, 2 are not transformed -- their last quarter holds the
// carry ola_in [rows, 3, 256], the oldest-first partial sums of the three hops the stream's earlier frames left pending
// (NULL: zeros), and the quarters a later hop reads hold 0 -- so a hop adds the carry first and then the call's frames in
// order: the sum of the whole-utterance kernel, bit for bit (x + 0 = x; only a -0 may become +0).  The first `skip` hops
// (3 at the start of a stream) lie before the utterance's first sample and are not stored.  The workgroup of the last
// chunk leaves the partial sums of the three hops still pending in ola_out.
template <bool MASKED, bool GATED = false, bool STREAM = false>
__global__ __launch_bounds__(256, TSSEP_ISTFT_OCC) void istft_kernel(
    const float2* __restrict__ X, int64_t T, int shift_, int64_t N,
    const float* __restrict__ wsyn, const float2* __restrict__ tw, float* __restrict__ y,
    const float* __restrict__ tgt, float* __restrict__ abs_partial, int nchunks, int hcb,
    const float* __restrict__ logit, const float2* __restrict__ obs, int64_t Kspk,
    const float* __restrict__ ola_in = nullptr, float* __restrict__ ola_out = nullptr, int skip = 0) {
  __shared__ float2 twl[NH];
  __shared__ float2 line[4][LINE];
  __shared__ __attribute__((aligned(16))) float fr[RING][1024];       // (51 KB with the rest: three workgroups per CU --
                                                                      // no room for the window table the rfft kernel keeps)
  __shared__ float red[4];
  static_assert(MASKED || !GATED, "the gate belongs to the mask head");
  constexpr int LDL = NH + 1 + (GATED ? 1 : 0);   // logit row length
  constexpr int C0 = GATED ? 1 : 0;               // column of bin 0
  const int tid = threadIdx.x, lane = tid & 63;
  // (wave-uniform; through readfirstlane so that the per-frame buffer resources below are built in SGPRs -- from a
  // VGPR the compiler wraps EVERY buffer access in a waterfall loop: ~10 extra instructions and a serialisation each)
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t row = blockIdx.y;
  const int c = blockIdx.x;
  for (int i = tid; i < NH; i += 256) twl[i] = tw[i];
  __syncthreads();
  const float2 tw2_lane = tw[NH + lane];
  const int64_t t_lo = (int64_t)c * hcb;   // hop h of this chunk sums frames t_lo + h .. t_lo + h + 3
  const int64_t n0 = t_lo * 256;
  const int64_t total_hops = STREAM ? T : (N + 255) / 256;
  const int hops = (int)(total_hops - t_lo < hcb ? total_hops - t_lo : hcb);
  const int iters = (hops + 3 + 3) / 4;    // frames 0 .. hops + 2
  const float hinv = 0.5f / 512.0f;
  float* yr = y + row * N;
  const float* tr = tgt ? tgt + row * N : nullptr;
  constexpr int TOFF = STREAM ? 3 : 0;     // ring frame l of the chunk is frame t_lo + l - TOFF
  // the chunk's samples [n0, min(N, n0 + 256 hops)) of this row; STREAM: y begins `skip` hops into the call, so the chunk's
  // samples lie at [n0 - 256 skip, ...) of the row and the first `yadj` of them in front of it (chunk 0 only: a further
  // chunk begins at least 33 hops in)
  int64_t chunk_bytes = ((N - n0 < (int64_t)hops * 256 ? N - n0 : (int64_t)hops * 256)) * 4;
  int64_t ylo = n0;
  int yadj = 0;
  if constexpr (STREAM) {
    const int64_t ybeg = n0 - 256 * (int64_t)skip;
    const int64_t yhi = ybeg + (int64_t)hops * 256 < N ? ybeg + (int64_t)hops * 256 : N;
    ylo = ybeg > 0 ? ybeg : 0;
    yadj = (int)(ylo - ybeg);
    chunk_bytes = (yhi > ylo ? yhi - ylo : 0) * 4;
  }
  const srd_t sy = make_srd(yr + ylo, chunk_bytes), str_ = make_srd(tr ? tr + n0 : yr + n0, chunk_bytes);
  float asum = 0.f;
  float2* buf = line[wave];
  // MASKED: the logits and observation bins of a frame are requested one iteration ahead (27 registers), right after
  // the previous frame's have been consumed: their latency hides behind that frame's transform and the hop emission
  // instead of opening every iteration (out-of-range frames get an empty resource: the loads return 0)
  float lg8[8], lgn = 0.f, lgg = 0.f;
  float2 ob8[8], obn = make_float2(0.f, 0.f);
  const int64_t urow = MASKED ? row / Kspk : 0;        // the utterance of this (utterance, speaker) row
  auto request = [&](int it_) __attribute__((always_inline)) {
    const int lf_ = it_ * 4 + wave;
    const int64_t t_ = t_lo + lf_ - TOFF;
    const bool ok = it_ < iters && (!STREAM || t_ >= 0) && t_ < T && lf_ < hops + 3;
    const int64_t tt = ok ? t_ : 0;
    const srd_t sl = make_srd(logit + (row * T + tt) * LDL, ok ? LDL * 4 : 0);
    const srd_t so = make_srd(obs + (urow * T + tt) * (NH + 1), ok ? (NH + 1) * 8 : 0);
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      lg8[r] = bload1(sl, (unsigned)(C0 * 4 + lane * 4 + 256 * r));
      ob8[r] = bload2(so, (unsigned)(lane * 8 + 512 * r));
    }
    lgn = bload1(sl, (unsigned)((C0 + NH) * 4));   // bin 512 (every lane the same address; lane 0 uses it)
    obn = bload2(so, (unsigned)(NH * 8));
    if (GATED) lgg = bload1(sl, 0u);               // the VAD logit (column 0)
  };
  if (MASKED) request(0);
  for (int it = 0; it < iters; ++it) {
    const int lf = it * 4 + wave;
    const int64_t t = t_lo + lf - TOFF;
    const bool valid = (!STREAM || t >= 0) && t < T && lf < hops + 3;
    float* slot = fr[lf % RING];
    float2 xnyq = make_float2(0.f, 0.f);              // MASKED: X[512], needed by lane 0 only
    if (MASKED) {
      if (valid) {
        const float g = GATED ? sigmoidf_mask(lgg) : 1.f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const int k = lane + 64 * r;
          const float m = GATED ? sigmoidf_mask(lg8[r]) * g : sigmoidf_mask(lg8[r]);
          buf[PADI(k)] = make_float2(ob8[r].x * m, ob8[r].y * m);
        }
        const float m = GATED ? sigmoidf_mask(lgn) * g : sigmoidf_mask(lgn);
        xnyq = make_float2(obn.x * m, obn.y * m);
        WAVE_SYNC();
      }
      __builtin_amdgcn_sched_barrier(0);
      request(it + 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (valid) {
      float2 v[8];
      const float2* Xr = MASKED ? nullptr : X + (row * T + t) * (NH + 1);
      float2 wr[8];
      lane_twiddles(tw2_lane, wr);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int k = lane + 64 * r;
        float2 xk = MASKED ? buf[PADI(k)] : Xr[k];
        float2 xm = MASKED ? (k == 0 ? xnyq : buf[PADI(NH - k)]) : Xr[NH - k];
        xm.y = -xm.y;
        if (k == 0) { xk.y = 0.f; xm.y = 0.f; }
        // (the 1/512 of the inverse transform rides on the 1/2 of the even / odd split: a power of two, exact)
        const float2 e = make_float2(hinv * (xk.x + xm.x), hinv * (xk.y + xm.y));
        const float2 w = make_float2(wr[r].x, -wr[r].y);
        const float2 o = cmul(make_float2(hinv * (xk.x - xm.x), hinv * (xk.y - xm.y)), w);
        // Zi = E + i O ; feed conj(Zi) to the forward FFT
        v[r] = make_float2(e.x - o.y, -(e.y + o.x));
      }
      if (MASKED) WAVE_SYNC();        // every lane has read the spectrum before the FFT reuses the line
      fft512_wave(v, buf, twl, lane);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const int n = lane + 64 * r;
        const float2 z = buf[PADI(n)];
        const float2 w = *reinterpret_cast<const float2*>(wsyn + 2 * n);
        *reinterpret_cast<float2*>(&slot[2 * n]) = make_float2(z.x * w.x, -z.y * w.y);
      }
      WAVE_SYNC();          // the wave's line is reused by its next frame; ring slots are disjoint
    } else {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        float2 z = make_float2(0.f, 0.f);
        if constexpr (STREAM) {       // ring frame lf < 3 of the call: the carry of pending hop lf in the last quarter
          if (t < 0 && r >= 6 && ola_in)
            z = *reinterpret_cast<const float2*>(ola_in + (row * 3 + lf) * 256 + 2 * (lane + 64 * (r - 6)));
        }
        *reinterpret_cast<float2*>(&slot[2 * (lane + 64 * r)]) = z;
      }
    }
    __syncthreads();        // frames <= 4 it + 3 are in the ring
    // emit the hops completed by this iteration: h in [4 it - 3, 4 it] (4 x 256 samples, 4 per thread).
    // The target samples are requested for all four hops first: interleaved with the stores of y the
    // compiler kept each load behind the previous store and waited for it (four serialised round trips
    // per iteration, a third of a workgroup's time).
    {
      // y and the target through buffer resources whose range ends with this chunk's samples: hops in front of
      // the chunk (h < 0 wraps to a huge offset) or behind it load 0 / are not stored -- no per-lane branches
      float tv[4], sv[4];
      bool em[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int h = 4 * it - 3 + q;
        em[q] = h >= 0 && h < hops && n0 + (int64_t)h * 256 + tid < N;
        tv[q] = tr ? bload1(str_, (unsigned)(((4 * it - 3 + q) * 256 + tid) * 4)) : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int h = 4 * it - 3 + q + RING * 2;           // (non-negative index into the ring; RING * 2 > 3)
        float s = fr[h % RING][tid + 768];
        s += fr[(h + 1) % RING][tid + 512];
        s += fr[(h + 2) % RING][tid + 256];
        s += fr[(h + 3) % RING][tid];
        sv[q] = s;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        bstore1(sy, (unsigned)(((4 * it - 3 + q) * 256 + tid - yadj) * 4), sv[q]);
        if (tr && em[q]) asum += fabsf(sv[q] - tv[q]);
      }
    }
    __syncthreads();        // the next iteration overwrites the slots of frames <= 4 it
  }
  if (abs_partial) {
    asum = wave_sum(asum);
    if (lane == 0) red[wave] = asum;
    __syncthreads();
    if (tid == 0) abs_partial[row * nchunks + c] = (red[0] + red[1]) + (red[2] + red[3]);
  }
  if constexpr (STREAM) {
    // the last chunk holds the call's last frame at ring index hops + 2 (the ring keeps the six frames in front of the
    // last iteration's newest): the partial sums of the three pending hops, oldest frame first as in the emission above
    if (c == nchunks - 1) {
      const float *f0 = fr[hops % RING], *f1 = fr[(hops + 1) % RING], *f2 = fr[(hops + 2) % RING];
      float* o = ola_out + row * 768;
      float s0 = f0[tid + 768];
      s0 += f1[tid + 512];
      s0 += f2[tid + 256];
      float s1 = f1[tid + 768];
      s1 += f2[tid + 512];
      o[tid] = s0;
      o[256 + tid] = s1;
      o[512 + tid] = f2[tid + 768];
    }
  }
}

// the gradient of the carry in front of a call: hop j = 0, 1, 2 of g = [skip zero hops | dy | d_ola_out] (a copy)
__global__ __launch_bounds__(256) void stream_carry_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ d_ola_out,
                                                               float* __restrict__ d_ola_in, int64_t rows, int64_t Tc, int skip,
                                                               int64_t N) {
  const int64_t row = blockIdx.x / 3;                               // (768 = 3 x 256: a block is one hop of one row)
  const int j = (int)(blockIdx.x - row * 3);
  if (row >= rows) return;
  float v = 0.f;
  if (j >= Tc) {
    if (d_ola_out) v = d_ola_out[row * 768 + (j - Tc) * 256 + threadIdx.x];
  } else if (j >= skip) {
    const int64_t n = (int64_t)(j - skip) * 256 + threadIdx.x;
    if (n < N) v = dy[row * N + n];
  }
  d_ola_in[row * 768 + j * 256 + threadIdx.x] = v;
}

// the sample tail a push leaves: the last 768 samples of [tail_in | x_new] (tail_in NULL: zeros)
__global__ __launch_bounds__(256) void stream_tail_kernel(const float* __restrict__ x_new, const float* __restrict__ tail_in,
                                                          float* __restrict__ tail_out, int64_t rows, int64_t n_new) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;      // (768 = 3 x 256: a block lies inside one row)
  const int64_t row = idx / 768;
  if (row >= rows) return;
  const int64_t v = n_new + (idx - row * 768);                      // position in [tail_in | x_new]
  tail_out[idx] = v < 768 ? (tail_in ? tail_in[row * 768 + v] : 0.f) : x_new[row * n_new + v - 768];
}

}  // namespace

extern "C" int64_t tssep_stft_frames(int64_t N, int size, int shift, int window_length, int pad,
                                     int fading) {
  if (window_length <= 0) window_length = size;
  int64_t n = N;
  if (fading) n += 2 * (int64_t)(window_length - shift);
  if (pad) {
    int64_t num = n - window_length;
    int64_t q = num <= 0 ? 0 : (num + shift - 1) / shift;
    return q + 1;
  }
  return (n - window_length) / shift + 1;
}

// the general plan (stft_generic.hip): every other size / shift the reference's `fe` slot may name
int tssep_generic_plan_supported(int size, int shift);
int tssep_generic_twiddles(int size, float* host_out);
int tssep_generic_rfft(const float* x, int64_t rows, int64_t N, int size, int shift, int pad_left, const float* window,
                       const float* tw, float* X, int64_t T, float s_in, float s_edge, void* stream);
int tssep_generic_framemag(const float* x, int64_t rows, int64_t N, int size, int shift, int pad_left, const float* window,
                           const float* tw, float* a, int64_t T, void* stream);
int tssep_generic_istft(const float* X, int64_t rows, int64_t T, int size, int shift, int pad_left, const float* wsyn,
                        const float* tw, float* y, int64_t N, void* stream);

extern "C" int tssep_fft_twiddles(int size, float* host_out) {
  if (!host_out) return TSSEP_E_NULL;
  if (size != 1024) return tssep_generic_twiddles(size, host_out);      // (the same table layout for every plan)
  const int nh = size / 2;
  for (int k = 0; k < nh; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)nh;
    host_out[2 * k] = (float)cos(a);
    host_out[2 * k + 1] = (float)sin(a);
  }
  for (int k = 0; k <= nh; ++k) {
    const double a = -2.0 * M_PI * (double)k / (double)size;
    host_out[2 * (nh + k)] = (float)cos(a);
    host_out[2 * (nh + k) + 1] = (float)sin(a);
  }
  return TSSEP_OK;
}

static int check_plan(int size, int shift) {
  if (size != 1024 || shift != 256) return TSSEP_E_UNSUPPORTED;
  return TSSEP_OK;
}
static bool generic_plan(int size, int shift) { return check_plan(size, shift) != TSSEP_OK && tssep_generic_plan_supported(size, shift); }
extern "C" int tssep_stft_plan(int size, int shift) {
  return check_plan(size, shift) == TSSEP_OK ? 1 : (tssep_generic_plan_supported(size, shift) ? 2 : 0);
}

static bool misaligned(const void* p, uintptr_t bytes) { return (((uintptr_t)p) & (bytes - 1)) != 0; }

// ---- the two launchers: what varies between the entry points, the checks they share, the grid, the launch ----------
// One launch of rfft_frames_kernel.  A member an entry point does not name stays zero / NULL.  (The entry point names the
// instantiation, not the launcher: the compiler emits the device functions in the order the host code names them.)
using rfft_kernel_t = decltype(&rfft_frames_kernel<false>);
struct RfftLaunch {
  rfft_kernel_t kernel;                        // the instantiation, named by the entry point
  bool masked;                                 // its MASKED flag: which of the members below it reads
  float* amag;                                 // its MAG flag (non-NULL): the frame magnitudes [rows, T] instead of X
  const float* x;                              // [rows, N]: the signal, dy, or with tgt != NULL the time-domain estimate
  int64_t rows, N, T;
  int size, shift, fading;
  const float *window, *tw;
  float s_in, s_edge;
  float* X;                                    // !masked: the spectra [rows, T, 513] (complex)
  const float *logit, *obs;                    // masked: rows = B K logit rows, the B observation spectra
  float* dlogit;
  int64_t K;
  const float *tgt, *sums, *gout;              // the loss fold (tgt == NULL: x is dy itself; sums == NULL: MAE)
  const int32_t* iperm;                        // the layout fold
  int bt_major;
  const float *vad, *gbce;                     // gated: the BCE fold on the gate column (vad == NULL: none)
  const float* tail;                           // the STREAM instantiations: the samples in front of x / the carry's gradient
                                               // behind dy (NULL: zeros)
  int stream_bwd;                              // STREAM == 2: x = dy may be NULL with N == 0; skip hops of zeros in front
  int skip;
};

// (the checks that do not depend on the plan: the general plan of stft_generic.hip takes the same arguments)
static int rfft_check(const RfftLaunch& a) {
  if ((!a.x && !(a.stream_bwd && a.N == 0)) || !a.window || !a.tw) return TSSEP_E_NULL;
  if (a.masked ? (!a.logit || !a.obs || !a.dlogit || (a.tgt && !a.gout) || (a.vad && !a.gbce)) : (!a.X && !a.amag))
    return TSSEP_E_NULL;
  if (a.rows <= 0 || (a.masked && a.K <= 0) || (a.stream_bwd ? a.N < 0 : a.N <= 0) || a.T <= 0) return TSSEP_E_SHAPE;
  if (misaligned(a.tw, 8) || misaligned(a.window, 8)) return TSSEP_E_ALIGN;
  if (a.masked ? (misaligned(a.logit, 4) || misaligned(a.dlogit, 4) || misaligned(a.obs, 8))
               : (a.amag ? misaligned(a.amag, 4) : misaligned(a.X, 8)))
    return TSSEP_E_ALIGN;
  return TSSEP_OK;
}

static int rfft_launch(const RfftLaunch& a, void* stream) {
  if (int e = rfft_check(a)) return e;
  if (int e = check_plan(a.size, a.shift)) return e;
  const int iters = 4;                         // frames per wave: 4 waves x 4 frames per workgroup
  const int64_t blocks = (a.rows * a.T + 4 * iters - 1) / (4 * iters);
  if (blocks > 0x7fffffff) return TSSEP_E_SHAPE;
  // (pad_left: the fade in front of the signal; the stream adjoint's skipped hops)
  const int pad_left = a.stream_bwd ? a.skip * a.shift : (a.fading ? a.size - a.shift : 0);
  hipLaunchKernelGGL(a.kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a.x, a.rows, a.N, a.T, a.shift,
                     pad_left, a.window, (const float2*)a.tw, (float2*)a.X, a.s_in, a.s_edge, iters,
                     a.logit, (const float2*)a.obs, a.amag ? a.amag : a.dlogit, a.masked ? a.K : (int64_t)1, a.tgt, a.sums, a.gout, a.iperm,
                     a.bt_major, a.vad, a.gbce, a.masked ? 1.0f / ((float)a.K * (float)a.T) : 0.f, a.tail);
  return tssep_launch_status();
}

// chunks per row: balanced, at most HCB_MAX hops each
extern "C" int64_t tssep_istft_chunks(int64_t N) {
  const int64_t hops = (N + 255) / 256;
  return (hops + HCB_MAX - 1) / HCB_MAX;
}

// One launch of istft_kernel: X (plain) or logit + obs (masked) -> y, with the |y - tgt| partial sums on the side.
using istft_kernel_t = decltype(&istft_kernel<false>);
struct IstftLaunch {
  istft_kernel_t kernel;                       // the instantiation, named by the entry point
  bool masked;                                 // its MASKED flag
  const float* X;                              // !masked: the spectra [rows, T, 513] (complex)
  const float *logit, *obs;                    // masked: rows = B K logit rows, the B observation spectra
  int64_t rows, K, T, N;
  int size, shift, fading;
  const float *wsyn, *tw;
  float* y;
  const float* tgt;                            // both or neither
  float* abs_partial;
};

static int istft_launch(const IstftLaunch& a, void* stream) {
  if ((a.masked ? (!a.logit || !a.obs) : !a.X) || !a.wsyn || !a.tw || !a.y) return TSSEP_E_NULL;
  if (a.rows <= 0 || (a.masked && a.K <= 0) || a.N <= 0 || a.T <= 0) return TSSEP_E_SHAPE;
  if ((a.tgt == nullptr) != (a.abs_partial == nullptr)) return TSSEP_E_NULL;
  if (int e = check_plan(a.size, a.shift)) return e;
  if (!a.fading) return TSSEP_E_UNSUPPORTED;
  if (misaligned(a.tw, 8) || misaligned(a.wsyn, 8)) return TSSEP_E_ALIGN;
  if (a.masked ? (misaligned(a.logit, 4) || misaligned(a.obs, 8)) : misaligned(a.X, 8)) return TSSEP_E_ALIGN;
  if (a.rows > 65535) return TSSEP_E_SHAPE;    // (the row is blockIdx.y)
  const int nchunks = (int)tssep_istft_chunks(a.N);
  const int hcb = (int)(((a.N + 255) / 256 + nchunks - 1) / nchunks);          // hops per chunk
  hipLaunchKernelGGL(a.kernel, dim3((unsigned)nchunks, (unsigned)a.rows), dim3(256), 0, (hipStream_t)stream,
                     (const float2*)a.X, a.T, a.shift, a.N, a.wsyn, (const float2*)a.tw, a.y, a.tgt, a.abs_partial, nchunks,
                     hcb, a.logit, (const float2*)a.obs, a.masked ? a.K : (int64_t)1, (const float*)nullptr, (float*)nullptr, 0);
  return tssep_launch_status();
}

// ---- the entry points ----------------------------------------------------------------------------------------------
extern "C" int tssep_stft_fwd(const float* x, int64_t rows, int64_t N, int size, int shift,
                              int fading, const float* window, const float* tw, float* X,
                              int64_t T, void* stream) {
  const RfftLaunch a = {.kernel = rfft_frames_kernel<false>, .x = x, .rows = rows, .N = N, .T = T, .size = size,
                        .shift = shift, .fading = fading, .window = window, .tw = tw, .s_in = 1.0f, .s_edge = 1.0f, .X = X};
  if (generic_plan(size, shift)) {
    if (int e = rfft_check(a)) return e;
    return tssep_generic_rfft(x, rows, N, size, shift, fading ? size - shift : 0, window, tw, X, T, 1.0f, 1.0f, stream);
  }
  return rfft_launch(a, stream);
}

extern "C" int tssep_istft_bwd(const float* dy, int64_t rows, int64_t N, int size, int shift,
                               int fading, const float* wsyn, const float* tw, float* dX,
                               int64_t T, void* stream) {
  const RfftLaunch a = {.kernel = rfft_frames_kernel<false>, .x = dy, .rows = rows, .N = N, .T = T, .size = size,
                        .shift = shift, .fading = fading, .window = wsyn, .tw = tw, .s_in = 2.0f / (float)size,
                        .s_edge = 1.0f / (float)size, .X = dX};
  if (generic_plan(size, shift)) {
    if (int e = rfft_check(a)) return e;
    return tssep_generic_rfft(dy, rows, N, size, shift, fading ? size - shift : 0, wsyn, tw, dX, T, a.s_in, a.s_edge, stream);
  }
  return rfft_launch(a, stream);
}

// the adjoint with the mask head's backward behind it (and, _bwd_loss / _gated_bwd, the loss in front and the final
// Linear's layout behind): B K rows, the synthesis window, the adjoint's scales
static RfftLaunch mask_bwd(rfft_kernel_t kernel, const float* x, const float* logit, const float* obs, int64_t B, int64_t K,
                           int64_t N, int size, int shift, int fading, const float* wsyn, const float* tw, float* dlogit,
                           int64_t T) {
  return {.kernel = kernel, .masked = true, .x = x, .rows = B * K, .N = N, .T = T, .size = size, .shift = shift,
          .fading = fading, .window = wsyn, .tw = tw, .s_in = 2.0f / (float)size, .s_edge = 1.0f / (float)size,
          .logit = logit, .obs = obs, .dlogit = dlogit, .K = K};
}

extern "C" int tssep_mask_istft_bwd(const float* dy, const float* logit, const float* obs, int64_t B,
                                    int64_t K, int64_t N, int size, int shift, int fading,
                                    const float* wsyn, const float* tw, float* dlogit, int64_t T,
                                    void* stream) {
  return rfft_launch(mask_bwd(rfft_frames_kernel<true>, dy, logit, obs, B, K, N, size, shift, fading, wsyn, tw, dlogit, T),
                     stream);
}

extern "C" int tssep_mask_istft_bwd_loss(const float* est, const float* tgt, const float* sums, const float* gout,
                                         const float* logit, const float* obs, int64_t B, int64_t K, int64_t N,
                                         int size, int shift, int fading, const float* wsyn, const float* tw,
                                         const int32_t* iperm, int bt_major, float* dlogit, int64_t T,
                                         void* stream) {
  // tgt == NULL: `est` is dy itself (only the output layout is folded); sums == NULL: MAE
  RfftLaunch a = mask_bwd(rfft_frames_kernel<true>, est, logit, obs, B, K, N, size, shift, fading, wsyn, tw, dlogit, T);
  a.tgt = tgt, a.sums = sums, a.gout = gout, a.iperm = iperm, a.bt_major = bt_major;
  return rfft_launch(a, stream);
}

extern "C" int tssep_istft_fwd(const float* X, int64_t rows, int64_t T, int size, int shift,
                               int fading, const float* wsyn, const float* tw, float* y, int64_t N,
                               const float* tgt, float* abs_partial, void* stream) {
  if (generic_plan(size, shift)) {
    if (!X || !wsyn || !tw || !y) return TSSEP_E_NULL;
    if (rows <= 0 || N <= 0 || T <= 0) return TSSEP_E_SHAPE;
    // (the general plan has no fused |estimate - target| sums: a time-domain loss reads the estimate itself)
    if (tgt || abs_partial) return TSSEP_E_UNSUPPORTED;
    if (misaligned(X, 8) || misaligned(tw, 8)) return TSSEP_E_ALIGN;
    return tssep_generic_istft(X, rows, T, size, shift, fading ? size - shift : 0, wsyn, tw, y, N, stream);
  }
  return istft_launch({.kernel = istft_kernel<false>, .X = X, .rows = rows, .T = T, .N = N, .size = size, .shift = shift,
                       .fading = fading, .wsyn = wsyn, .tw = tw, .y = y, .tgt = tgt, .abs_partial = abs_partial}, stream);
}

// sigmoid -> Masking -> inverse STFT over B K logit rows
static int mask_istft_fwd(istft_kernel_t kernel, const float* logit, const float* obs, int64_t B, int64_t K, int64_t T,
                          int size, int shift, int fading, const float* wsyn, const float* tw, float* y, int64_t N,
                          const float* tgt, float* abs_partial, void* stream) {
  return istft_launch({.kernel = kernel, .masked = true, .logit = logit, .obs = obs, .rows = B * K, .K = K, .T = T, .N = N,
                       .size = size, .shift = shift, .fading = fading, .wsyn = wsyn, .tw = tw, .y = y, .tgt = tgt,
                       .abs_partial = abs_partial}, stream);
}

extern "C" int tssep_mask_istft_fwd(const float* logit, const float* obs, int64_t B, int64_t K,
                                    int64_t T, int size, int shift, int fading, const float* wsyn,
                                    const float* tw, float* y, int64_t N, const float* tgt,
                                    float* abs_partial, void* stream) {
  return mask_istft_fwd(istft_kernel<true>, logit, obs, B, K, T, size, shift, fading, wsyn, tw, y, N, tgt, abs_partial,
                        stream);
}

// ---- explicit_vad: the gated fused tail (logit rows of F + 1 = 514 floats, the VAD logit at column 0) --------------
extern "C" int tssep_mask_istft_gated_fwd(const float* logit, const float* obs, int64_t B, int64_t K, int64_t T, int size,
                                          int shift, int fading, const float* wsyn, const float* tw, float* y, int64_t N,
                                          const float* tgt, float* abs_partial, void* stream) {
  return mask_istft_fwd(istft_kernel<true, true>, logit, obs, B, K, T, size, shift, fading, wsyn, tw, y, N, tgt, abs_partial,
                        stream);
}

extern "C" int tssep_mask_istft_gated_bwd(const float* est, const float* tgt, const float* sums, const float* gout,
                                          const float* vad, const float* gout_vad, const float* logit, const float* obs,
                                          int64_t B, int64_t K, int64_t N, int size, int shift, int fading,
                                          const float* wsyn, const float* tw, const int32_t* iperm, int bt_major,
                                          float* dlogit, int64_t T, void* stream) {
  // tgt == NULL: `est` is dy itself; sums == NULL: MAE; vad == NULL: no BCE term on the gate column
  RfftLaunch a = mask_bwd(rfft_frames_kernel<true, true>, est, logit, obs, B, K, N, size, shift, fading, wsyn, tw, dlogit,
                          T);
  a.tgt = tgt, a.sums = sums, a.gout = gout, a.iperm = iperm, a.bt_major = bt_major, a.vad = vad, a.gbce = gout_vad;
  return rfft_launch(a, stream);
}

// ---- the VAD losses' magnitude target (named last: the kernels above keep their place in the code object) --------
// the STFT's frame magnitudes a[r,t] = sum_f |X[r,t,f]| without the spectrum (the VAD losses' magnitude target)
extern "C" int tssep_stft_framemag_fwd(const float* x, int64_t rows, int64_t N, int size, int shift, int fading,
                                       const float* window, const float* tw, float* a, int64_t T, void* stream) {
  const RfftLaunch l = {.kernel = rfft_frames_kernel<false, false, true>, .amag = a, .x = x, .rows = rows, .N = N, .T = T,
                        .size = size, .shift = shift, .fading = fading, .window = window, .tw = tw, .s_in = 1.0f,
                        .s_edge = 1.0f};
  if (generic_plan(size, shift)) {
    if (int e = rfft_check(l)) return e;
    return tssep_generic_framemag(x, rows, N, size, shift, fading ? size - shift : 0, window, tw, a, T, stream);
  }
  return rfft_launch(l, stream);
}

// ---- the online forms (plan 1 only): a live signal in pushes of whole hops, the state carried by the caller ---------
static bool overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t p = (uintptr_t)a, q = (uintptr_t)b;
  return p < q + (uintptr_t)bytes && q < p + (uintptr_t)bytes;
}

extern "C" int tssep_stft_stream_fwd(const float* x_new, int64_t rows, int64_t n_new, const float* tail_in, float* tail_out,
                                     int size, int shift, const float* window, const float* tw, float* X, int64_t Tc,
                                     void* stream) {
  if (!x_new || !tail_out || !window || !tw || !X) return TSSEP_E_NULL;
  if (int e = check_plan(size, shift)) return e;
  if (rows <= 0 || Tc < 1 || n_new != Tc * shift) return TSSEP_E_SHAPE;
  const int64_t tail_bytes = rows * (size - shift) * 4;
  if (tail_in && overlap(tail_in, tail_out, tail_bytes)) return TSSEP_E_SHAPE;
  if (misaligned(x_new, 8) || misaligned(tail_out, 8) || misaligned(tail_in, 8) || misaligned(tw, 8) || misaligned(window, 8) ||
      misaligned(X, 8))
    return TSSEP_E_ALIGN;
  if (rows * 3 > 0x7fffffff) return TSSEP_E_SHAPE;
  // (the whole-signal launcher: no fade in front, the rows are the new samples)
  const RfftLaunch a = {.kernel = rfft_frames_kernel<false, false, false, 1>, .x = x_new, .rows = rows, .N = n_new, .T = Tc,
                        .size = size, .shift = shift, .fading = 0, .window = window, .tw = tw, .s_in = 1.0f, .s_edge = 1.0f,
                        .X = X, .tail = tail_in};
  if (int e = rfft_launch(a, stream)) return e;
  hipLaunchKernelGGL(stream_tail_kernel, dim3((unsigned)(rows * 3)), dim3(256), 0, (hipStream_t)stream, x_new, tail_in,
                     tail_out, rows, n_new);
  return tssep_launch_status();
}

// One launch of the STREAM instantiations of istft_kernel.  y holds the Tc - skip hops the call completes (none: y may be NULL and N is 0);
// `last` lets the final hop end early, at the utterance's last sample.
static int istft_stream_launch(int variant, const float* X, const float* logit, const float* obs, int64_t rows, int64_t K,
                               int64_t Tc, int size, int shift, const float* wsyn, const float* tw, const float* ola_in,
                               float* ola_out, int skip, int last, float* y, int64_t N, void* stream) {
  const bool masked = variant != 0;
  if ((masked ? (!logit || !obs) : !X) || !wsyn || !tw || !ola_out) return TSSEP_E_NULL;
  if (int e = check_plan(size, shift)) return e;
  if (rows <= 0 || (masked && (K <= 0 || rows % K)) || Tc < 1 || skip < 0 || skip > 3 || rows > 65535) return TSSEP_E_SHAPE;
  const int64_t hops = Tc > skip ? Tc - skip : 0;
  if (N < 0 || N > hops * shift || (last ? N <= (hops - 1) * shift && hops > 0 : N != hops * shift)) return TSSEP_E_SHAPE;
  if (N > 0 && !y) return TSSEP_E_NULL;
  if (ola_in && overlap(ola_in, ola_out, rows * (size - shift) * 4)) return TSSEP_E_SHAPE;
  if (misaligned(tw, 8) || misaligned(wsyn, 8) || misaligned(ola_in, 8) || misaligned(ola_out, 4) || misaligned(y, 4))
    return TSSEP_E_ALIGN;
  if (masked ? (misaligned(logit, 4) || misaligned(obs, 8)) : misaligned(X, 8)) return TSSEP_E_ALIGN;
  const int nchunks = (int)((Tc + HCB_MAX - 1) / HCB_MAX);
  const int hcb = (int)((Tc + nchunks - 1) / nchunks);
  const istft_kernel_t kernel = variant == 0 ? istft_kernel<false, false, true>
                                              : (variant == 1 ? istft_kernel<true, false, true> : istft_kernel<true, true, true>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)nchunks, (unsigned)rows), dim3(256), 0, (hipStream_t)stream, (const float2*)X, Tc,
                     shift, N, wsyn, (const float2*)tw, y, (const float*)nullptr, (float*)nullptr, nchunks, hcb, logit,
                     (const float2*)obs, masked ? K : (int64_t)1, ola_in, ola_out, skip);
  return tssep_launch_status();
}

extern "C" int tssep_istft_stream_fwd(const float* X, int64_t rows, int64_t Tc, int size, int shift, const float* wsyn,
                                      const float* tw, const float* ola_in, float* ola_out, int skip, int last, float* y,
                                      int64_t N, void* stream) {
  return istft_stream_launch(0, X, nullptr, nullptr, rows, 1, Tc, size, shift, wsyn, tw, ola_in, ola_out, skip, last, y, N,
                             stream);
}

extern "C" int tssep_mask_istft_stream_fwd(const float* logit, int gated, const float* obs, int64_t B, int64_t K, int64_t Tc,
                                           int size, int shift, const float* wsyn, const float* tw, const float* ola_in,
                                           float* ola_out, int skip, int last, float* y, int64_t N, void* stream) {
  if (B <= 0 || K <= 0) return (!logit || !obs || !wsyn || !tw || !ola_out) ? TSSEP_E_NULL : TSSEP_E_SHAPE;
  return istft_stream_launch(gated ? 2 : 1, nullptr, logit, obs, B * K, K, Tc, size, shift, wsyn, tw, ola_in, ola_out, skip,
                             last, y, N, stream);
}

// ---- the adjoints of the two streaming tails: one launch of a STREAM == 2 instantiation of rfft_frames_kernel, and the
// copy that hands the carry's gradient on.  (Named last: the kernels above keep their place in the code object.)
static int istft_stream_bwd_launch(int variant, const float* dy, const float* d_ola_out, const float* logit, const float* obs,
                                   int64_t rows, int64_t K, int64_t Tc, int size, int shift, const float* wsyn, const float* tw,
                                   int skip, int last, int64_t N, float* dX, float* dlogit, float* d_ola_in, void* stream) {
  const bool masked = variant != 0;
  if ((masked ? (!logit || !obs || !dlogit) : !dX) || !wsyn || !tw) return TSSEP_E_NULL;
  if (int e = check_plan(size, shift)) return e;
  // (Tc: the frame offsets of a row are 32-bit byte offsets)
  if (rows <= 0 || (masked && (K <= 0 || rows % K)) || Tc < 1 || Tc > (1 << 20) || skip < 0 || skip > 3 || rows * 3 > 0x7fffffff)
    return TSSEP_E_SHAPE;
  const int64_t hops = Tc > skip ? Tc - skip : 0;
  if (N < 0 || N > hops * shift || (last ? N <= (hops - 1) * shift && hops > 0 : N != hops * shift)) return TSSEP_E_SHAPE;
  if (N > 0 && !dy) return TSSEP_E_NULL;
  if (d_ola_in && d_ola_out && overlap(d_ola_in, d_ola_out, rows * (size - shift) * 4)) return TSSEP_E_SHAPE;
  if (misaligned(dy, 4) || misaligned(d_ola_out, 8) || misaligned(d_ola_in, 4)) return TSSEP_E_ALIGN;
  const rfft_kernel_t kernel = variant == 0 ? rfft_frames_kernel<false, false, false, 2>
                                             : (variant == 1 ? rfft_frames_kernel<true, false, false, 2>
                                                             : rfft_frames_kernel<true, true, false, 2>);
  const RfftLaunch a = {.kernel = kernel, .masked = masked, .x = dy, .rows = rows, .N = N, .T = Tc, .size = size, .shift = shift,
                        .fading = 1, .window = wsyn, .tw = tw, .s_in = 2.0f / (float)size, .s_edge = 1.0f / (float)size,
                        .X = dX, .logit = logit, .obs = obs, .dlogit = dlogit, .K = K, .tail = d_ola_out, .stream_bwd = 1,
                        .skip = skip};
  if (int e = rfft_launch(a, stream)) return e;
  if (!d_ola_in) return TSSEP_OK;
  hipLaunchKernelGGL(stream_carry_bwd_kernel, dim3((unsigned)(rows * 3)), dim3(256), 0, (hipStream_t)stream, dy, d_ola_out,
                     d_ola_in, rows, Tc, skip, N);
  return tssep_launch_status();
}

extern "C" int tssep_istft_stream_bwd(const float* dy, const float* d_ola_out, int64_t rows, int64_t Tc, int size, int shift,
                                      const float* wsyn, const float* tw, int skip, int last, int64_t N, float* dX,
                                      float* d_ola_in, void* stream) {
  return istft_stream_bwd_launch(0, dy, d_ola_out, nullptr, nullptr, rows, 1, Tc, size, shift, wsyn, tw, skip, last, N, dX,
                                 nullptr, d_ola_in, stream);
}

extern "C" int tssep_mask_istft_stream_bwd(const float* dy, const float* d_ola_out, const float* logit, int gated,
                                           const float* obs, int64_t B, int64_t K, int64_t Tc, int size, int shift,
                                           const float* wsyn, const float* tw, int skip, int last, int64_t N, float* dlogit,
                                           float* d_ola_in, void* stream) {
  if (B <= 0 || K <= 0) return (!logit || !obs || !wsyn || !tw || !dlogit) ? TSSEP_E_NULL : TSSEP_E_SHAPE;
  return istft_stream_bwd_launch(gated ? 2 : 1, dy, d_ola_out, logit, obs, B * K, K, Tc, size, shift, wsyn, tw, skip, last, N,
                                 nullptr, dlogit, d_ola_in, stream);
}
