// Discretisation of estimated masks: masks -> per-speaker activity -> decision, closing, runs -> the segment table
// of the segment-wise beamformer (tssep_mvdr_segments_fwd), born on the device.  DESIGN 4.13.
//
//   tssep_mask_activity      a[k,t] = fl32(sum_f masks[k,0,t,f]) / fl32(F): the one pass over many bytes, a pure read
//                            stream.  One wave per (k, t) row: a scalar head up to the first 16-byte boundary, 16-byte
//                            loads, a scalar tail; every lane sums its own elements in ascending order, then one xor
//                            butterfly over the wave.  The order is a function of (F, address of the row mod 16) only.
//                            (Adding 0.0 for an element past the end changes nothing: the masks' sums are >= +0.)
//   tssep_activity_segments  b = a > threshold; closing = dilation then erosion with clipped windows; maximal runs;
//                            runs shorter than min_frames dropped; rows (k, s, e) in order.
//
// The closing is done on runs, not on frames, so no window is ever swept and a window larger than the row costs
// nothing: with hd = dilation / 2 and he = erosion / 2 (both clamped to T, a clipped window cannot see further)
//   - dilation turns the raw run [s, e) into [max(0, s - hd), min(T, e + hd)); two neighbours with a gap g = s' - e
//     become one run iff g <= 2 hd;
//   - erosion turns the merged, dilated run [sd, ed) into [sd == 0 ? 0 : sd + he, ed == T ? T : ed - he): frames outside
//     the row count as active, so a run that reaches the first or the last frame keeps that side; an empty result is
//     dropped (an erosion window is contiguous, it lies in one dilated run or it fails).
// Three order-preserving compactions, each "count per block -> one exclusive scan of the block counts -> scatter by
// rank": (1) the rising and the falling edges of b, 256 frames to a block, one frame of halo each side; the i-th
// rising and the i-th falling edge of a row belong to the same run, and every row has as many of the one as of the
// other, so both are scattered by their GLOBAL rank and meet in the same slot; (2) of the raw runs those starts whose
// gap to the previous end of the same row exceeds 2 hd and those ends whose gap to the next start does: again
// i-th with i-th; (3) of the merged runs those that survive the erosion with at least min_frames frames.
// Nine launches (the last scan also writes the count) whatever T, the content or the number of runs; no atomics: every
// slot has one writer, the table is the same on every call.  A row of T frames holds at most ceil(T / 2) runs at every stage, so nothing overflows the
// K * ceil(T / 2) rows of tssep_segments_capacity(); every scatter is bounded by that capacity all the same.
#include "common.h"

namespace {

constexpr int SEG_BLOCK = 256;            // frames (stage 1) or runs (stages 2, 3) per block
constexpr int64_t SEG_MAX = (int64_t)1 << 30;

__host__ __device__ inline int64_t seg_capacity(int64_t K, int64_t T) {
  if (K < 1 || T < 1 || T > SEG_MAX) return 0;
  const int64_t per = (T + 1) / 2;
  if (K > SEG_MAX / per) return 0;
  return K * per;
}

// ---------------------------------------------------------------------------------------------- activity
constexpr int ACT_GRID_CAP = 2048;        // blocks of four waves; the waves stride over the rows beyond 8192

// Every load of a row is issued before the first add: the indices past the row's end are clamped to a valid element and
// the value is dropped by a select, so no load sits behind a branch (a row of F = 513 is two 16-byte loads and at most
// two scalar ones per lane, one memory latency in all).
__global__ __launch_bounds__(256) void mask_activity_kernel(const float* __restrict__ masks, int64_t rows, int64_t T,
                                                            int64_t M, int F, float* __restrict__ act) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const bool small = rows <= INT32_MAX;
  const float fF = (float)F;
  for (int64_t r = wave; r < rows; r += nwaves) {
    // mask index 0 of speaker k = r / T, frame r - k T: row r + k (M - 1) T of the [K M T, F] matrix
    const int64_t k = M == 1 ? 0 : (small ? (int64_t)((uint32_t)r / (uint32_t)T) : r / T);
    const float* __restrict__ p = masks + (r + k * (M - 1) * T) * (int64_t)F;
    int head = (int)(((16u - ((unsigned)(uintptr_t)p & 15u)) & 15u) >> 2);   // floats in front of the 16-byte boundary
    if (head > F) head = F;
    const int nvec = (F - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const float hv = p[lane < head ? lane : 0];
    const float tv = p[lane < F - tail0 ? tail0 + lane : 0];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (nvec > 0) {
      const f32x4* __restrict__ pv = reinterpret_cast<const f32x4*>(p + head);
      for (int base = 0; base < nvec; base += 256) {
        f32x4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = base + 64 * j + lane;
          v[j] = pv[i < nvec ? i : nvec - 1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = base + 64 * j + lane < nvec;
          acc.x += in ? v[j].x : 0.f;
          acc.y += in ? v[j].y : 0.f;
          acc.z += in ? v[j].z : 0.f;
          acc.w += in ? v[j].w : 0.f;
        }
      }
    }
    float s = (acc.x + acc.y) + (acc.z + acc.w);
    s += lane < head ? hv : 0.f;
    s += lane < F - tail0 ? tv : 0.f;
    s = wave_sum(s);
    if (lane == 0) act[r] = s / fF;       // one IEEE division (hipcc's default: correctly rounded)
  }
}

// ---------------------------------------------------------------------------------------------- compaction
// ranks of two flags among the 256 threads of a block, and the block's totals
__device__ __forceinline__ void block_rank2(bool fa, bool fb, int& ra, int& rb, int& ta, int& tb) {
  __shared__ int wa[4], wb[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long ma = __ballot(fa), mb = __ballot(fb);
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  ra = __popcll(ma & below);
  rb = __popcll(mb & below);
  if (lane == 0) { wa[w] = __popcll(ma); wb[w] = __popcll(mb); }
  __syncthreads();
  ta = tb = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < w) { ra += wa[i]; rb += wb[i]; }
    ta += wa[i];
    tb += wb[i];
  }
}

// counts [n] pairs -> exclusive prefix in place, the totals to total[0..1].  One block, tile by tile with a carry.
__global__ __launch_bounds__(1024) void seg_scan_kernel(int2* __restrict__ counts, int64_t n, int* __restrict__ total,
                                                        int32_t* __restrict__ count_out) {
  __shared__ int2 wsum[16];
  __shared__ int2 carry;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = make_int2(0, 0);
  __syncthreads();
  for (int64_t base = 0; base < n; base += 1024) {
    const int64_t i = base + threadIdx.x;
    const int2 v = i < n ? counts[i] : make_int2(0, 0);
    int2 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int ux = __shfl_up(inc.x, o, 64), uy = __shfl_up(inc.y, o, 64);
      if (lane >= o) { inc.x += ux; inc.y += uy; }
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int2 off = carry;
    for (int j = 0; j < w; ++j) { off.x += wsum[j].x; off.y += wsum[j].y; }
    if (i < n) counts[i] = make_int2(off.x + inc.x - v.x, off.y + inc.y - v.y);
    __syncthreads();
    if (threadIdx.x == 1023) carry = make_int2(off.x + inc.x, off.y + inc.y);
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    total[0] = carry.x;
    total[1] = carry.y;
    if (count_out) count_out[0] = carry.x;
  }
}

// stage 1: block = (row, chunk of 256 frames).  Rising edge at t: b[t] and not b[t-1]; falling edge owned by the last
// frame of the run: b[t] and not b[t+1], the run ends at t + 1.  Frames outside the row are inactive.
template <bool SCATTER>
__global__ __launch_bounds__(SEG_BLOCK) void seg_edges_kernel(const float* __restrict__ act, int64_t T, int chunks,
                                                              float threshold, int2* __restrict__ counts, int cap,
                                                              int* __restrict__ rs, int* __restrict__ re,
                                                              int* __restrict__ rrow) {
  const int64_t row = blockIdx.x / chunks;
  const int64_t t = (int64_t)(blockIdx.x % chunks) * SEG_BLOCK + threadIdx.x;
  const float* __restrict__ a = act + row * T;
  const bool in = t < T;
  const int64_t tc = in ? t : T - 1;                          // clamped: the three loads sit behind no branch
  const float a0 = a[tc], am = a[tc > 0 ? tc - 1 : 0], ap = a[tc + 1 < T ? tc + 1 : T - 1];
  const bool b = in && a0 > threshold;                       // strict; a NaN compares false
  const bool bp = in && t > 0 && am > threshold;
  const bool bn = in && t + 1 < T && ap > threshold;
  const bool rise = b && !bp, fall = b && !bn;
  int ra, rb, ta, tb;
  block_rank2(rise, fall, ra, rb, ta, tb);
  if (!SCATTER) {
    if (threadIdx.x == 0) counts[blockIdx.x] = make_int2(ta, tb);
  } else {
    const int2 off = counts[blockIdx.x];
    if (rise && off.x + ra < cap) { rs[off.x + ra] = (int)t; rrow[off.x + ra] = (int)row; }
    if (fall && off.y + rb < cap) re[off.y + rb] = (int)t + 1;
  }
}

// stage 2: one thread per raw run g < n1[0].  A start is kept when its gap to the previous end of the row exceeds
// 2 hd (or there is none), an end when the gap to the next start does.
template <bool SCATTER>
__global__ __launch_bounds__(SEG_BLOCK) void seg_merge_kernel(const int* __restrict__ rs, const int* __restrict__ re,
                                                              const int* __restrict__ rrow, const int* __restrict__ n1,
                                                              int hd, int2* __restrict__ counts, int cap,
                                                              int* __restrict__ ms, int* __restrict__ me,
                                                              int* __restrict__ mrow) {
  int n = n1[0];
  if (n > cap) n = cap;
  const int g = blockIdx.x * SEG_BLOCK + threadIdx.x;
  bool ks = false, ke = false;
  int s = 0, e = 0, r = 0;
  if (g < n) {
    s = rs[g], e = re[g], r = rrow[g];
    ks = g == 0 || rrow[g - 1] != r || (int64_t)s - re[g - 1] > 2 * (int64_t)hd;
    ke = g == n - 1 || rrow[g + 1] != r || (int64_t)rs[g + 1] - e > 2 * (int64_t)hd;
  }
  int ra, rb, ta, tb;
  block_rank2(ks, ke, ra, rb, ta, tb);
  if (!SCATTER) {
    if (threadIdx.x == 0) counts[blockIdx.x] = make_int2(ta, tb);
  } else {
    const int2 off = counts[blockIdx.x];
    if (ks && off.x + ra < cap) { ms[off.x + ra] = s; mrow[off.x + ra] = r; }
    if (ke && off.y + rb < cap) me[off.y + rb] = e;
  }
}

// stage 3: one thread per merged run j < n2[0]: dilate, erode, drop what is shorter than min_frames, write the row.
template <bool SCATTER>
__global__ __launch_bounds__(SEG_BLOCK) void seg_emit_kernel(const int* __restrict__ ms, const int* __restrict__ me,
                                                             const int* __restrict__ mrow, const int* __restrict__ n2,
                                                             int T, int hd, int he, int min_frames,
                                                             int2* __restrict__ counts, int cap,
                                                             int32_t* __restrict__ table) {
  int n = n2[0];
  if (n > cap) n = cap;
  const int j = blockIdx.x * SEG_BLOCK + threadIdx.x;
  bool keep = false;
  int64_t s = 0, e = 0;
  if (j < n) {
    s = ms[j] - hd <= 0 ? 0 : (int64_t)ms[j] - hd + he;      // hd, he <= T <= 2^30
    e = me[j] >= T - hd ? T : (int64_t)me[j] + hd - he;
    keep = e - s >= min_frames;
  }
  int ra, rb, ta, tb;
  block_rank2(keep, keep, ra, rb, ta, tb);
  if (!SCATTER) {
    if (threadIdx.x == 0) counts[blockIdx.x] = make_int2(ta, tb);
  } else {
    const int at = counts[blockIdx.x].x + ra;
    if (keep && at < cap) {
      table[3 * (int64_t)at] = mrow[j];
      table[3 * (int64_t)at + 1] = (int32_t)s;          // kept: 0 <= s < e <= T
      table[3 * (int64_t)at + 2] = (int32_t)e;
    }
  }
}

}  // namespace

extern "C" int64_t tssep_segments_capacity(int64_t K, int64_t T) { return seg_capacity(K, T); }

extern "C" int tssep_mask_activity(const float* masks, int64_t K, int M, int64_t T, int F, float* activity,
                                   void* stream) {
  if (!masks || !activity) return TSSEP_E_NULL;
  if (K < 1 || M < 1 || T < 1 || F < 1 || K > INT32_MAX || T > INT32_MAX) return TSSEP_E_SHAPE;
  if ((((uintptr_t)masks) | ((uintptr_t)activity)) & 3u) return TSSEP_E_ALIGN;
  const int64_t rows = K * T;
  hipLaunchKernelGGL(mask_activity_kernel, dim3(grid_for(rows, 4, ACT_GRID_CAP)), dim3(256), 0, S_, masks, rows, T,
                     (int64_t)M, F, activity);
  return tssep_launch_status();
}

extern "C" int tssep_activity_segments(const float* activity, int64_t K, int64_t T, float threshold, int64_t dilation,
                                       int64_t erosion, int64_t min_frames, int32_t* table, int32_t* count,
                                       void* workspace, void* stream) {
  if (!activity || !table || !count || !workspace) return TSSEP_E_NULL;
  const int64_t cap64 = seg_capacity(K, T);
  if (cap64 <= 0 || dilation < 1 || erosion < 1 || !(dilation & 1) || !(erosion & 1) || min_frames < 1)
    return TSSEP_E_SHAPE;
  if ((((uintptr_t)activity) | ((uintptr_t)table) | ((uintptr_t)count)) & 3u || (((uintptr_t)workspace) & 7u))
    return TSSEP_E_ALIGN;
  const int cap = (int)cap64;
  const int hd = (int)(dilation / 2 < T ? dilation / 2 : T), he = (int)(erosion / 2 < T ? erosion / 2 : T);
  const int mf = (int)(min_frames <= T ? min_frames : T + 1);
  const int chunks = (int)((T + SEG_BLOCK - 1) / SEG_BLOCK);
  const int64_t nb1 = K * chunks, nb2 = (cap64 + SEG_BLOCK - 1) / SEG_BLOCK;
  // workspace, in ints: totals [8] | counts of the stages 2 nb1, 2 nb2, 2 nb2 | rs, re, rrow, ms, me, mrow [cap] each
  // (<= 9 cap + 12: nb1 <= cap, 4 nb2 <= cap + 4)
  int* w = (int*)workspace;
  int* total = w;
  int2* c1 = (int2*)(w + 8);
  int2* c2 = c1 + nb1;
  int2* c3 = c2 + nb2;
  int* rs = (int*)(c3 + nb2);
  int *re = rs + cap, *rrow = re + cap, *ms = rrow + cap, *me = ms + cap, *mrow = me + cap;
  const dim3 g1((unsigned)nb1), g2((unsigned)nb2), blk(SEG_BLOCK);
  hipLaunchKernelGGL(seg_edges_kernel<false>, g1, blk, 0, S_, activity, T, chunks, threshold, c1, cap, rs, re, rrow);
  hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(1024), 0, S_, c1, nb1, total, (int32_t*)nullptr);
  hipLaunchKernelGGL(seg_edges_kernel<true>, g1, blk, 0, S_, activity, T, chunks, threshold, c1, cap, rs, re, rrow);
  hipLaunchKernelGGL(seg_merge_kernel<false>, g2, blk, 0, S_, rs, re, rrow, total, hd, c2, cap, ms, me, mrow);
  hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(1024), 0, S_, c2, nb2, total + 2, (int32_t*)nullptr);
  hipLaunchKernelGGL(seg_merge_kernel<true>, g2, blk, 0, S_, rs, re, rrow, total, hd, c2, cap, ms, me, mrow);
  hipLaunchKernelGGL(seg_emit_kernel<false>, g2, blk, 0, S_, ms, me, mrow, total + 2, (int)T, hd, he, mf, c3, cap, table);
  hipLaunchKernelGGL(seg_scan_kernel, dim3(1), dim3(1024), 0, S_, c3, nb2, total + 4, count);
  hipLaunchKernelGGL(seg_emit_kernel<true>, g2, blk, 0, S_, ms, me, mrow, total + 2, (int)T, hd, he, mf, c3, cap, table);
  return tssep_launch_status();
}
