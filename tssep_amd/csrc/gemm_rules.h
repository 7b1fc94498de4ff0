// Rules of the split-bf16 GEMM dispatcher (host only; the candidate table that hangs them on kernels is in
// gemm_bf16x3.hip): per candidate, WHEN it is wanted in automatic mode (`wants_*`) and, for the weight-gradient kernels,
// the split count to launch it with (`splits_*`) -- pure functions of the request, a kernel's two rules next to each
// other on the same tile-geometry helpers.  What a kernel REQUIRES is checked by its launcher, not here.
// The rules are stated in quantities of the request (padding waste of a tile shape, K stages per tile, bytes of
// the C stream) -- profiles/r4_gemm_shape_sweep.jsonl holds, per shape of a sweep over units / projs / speakers,
// the time of every candidate next to the one the rules pick.
#pragma once
#include <algorithm>
#include "gemm_common.h"

namespace gemm_detail {

inline int64_t cdiv(int64_t x, int64_t y) { return (x + y - 1) / y; }
inline int64_t rup(int64_t x, int64_t y) { return cdiv(x, y) * y; }

// N = 256 q + 1 (q >= 1): q column tiles + a VALU column (big, big_p, tall4_xcol; the streaming kernel leaves these shapes)
inline bool n_256q_plus_1(int64_t N) { return N > 256 && N % 256 == 1; }
// N = 128 q + 1 | 2 (q >= 1): the last columns ride on the VALU of the q-th column tile of the 512 x 128 weight-gradient
// kernel (one real column at most; the ones column of b_ones_col is the last column).  `tn_xc`: GemmSwitches::tn_xc, or 1
inline bool n_128q_plus_12(int64_t N, int ones, int tn_xc) { return tn_xc && N > 128 && N % 128 >= 1 && N % 128 <= 2 && N % 128 - ones <= 1; }
inline int64_t tn_big_col_tiles(int64_t N, int ones, int tn_xc) { return n_128q_plus_12(N, ones, tn_xc) ? N / 128 : cdiv(N, 128); }

// What the rules read of a request, and the derived quantities several of them share
struct GemmRequest {
  const tssep_gemm_args* g; const StoreMap& sm; int splitk;
  bool two, shift;             // two: weight gradients only, the dY_lo * X_hi product dropped
  GemmSwitches sw;
  GemmRequest(const tssep_gemm_args* g_, const StoreMap& sm_, int splitk_)
      : g(g_), sm(sm_), splitk(splitk_), two(g_->precision == 2), shift(g_->kperiod > 0), sw(gemm_switches()) {}

  // ---- row x row family
  int64_t n256() const { return rup(g->N, 256); }
  bool xcol_shape() const { return n_256q_plus_1(g->N) && (g->K & 3) == 0; }      // N = 256 q + 1: q tiles + a VALU column
  int64_t ct256() const { return xcol_shape() ? (g->N - 1) / 256 : n256() / 256; }   // column tiles of the 256-wide kernels
  bool short_k() const { return g->K < 448; }      // a tile's life is mostly its C store below this
  // Occupancy (round 4, the 8-utterance shard of the 8-GPU configuration: M = 2024 / 8096 rows): a kernel whose tiles do
  // not fill three quarters of the CUs once leaves the chip idle -- 128 x 128 tiles on two workgroups per CU then run up
  // to 2.7 x faster (profiles/r4_gemm_shape_sweep_b8.jsonl: 168 against 70 TFLOP/s at 8096 x 320 x 2400).  The
  // persistent streaming kernel balances its own tile list: half the CUs suffice there.
  int64_t mt256() const { return cdiv(g->M, 256); }
  bool fills(int64_t col_tiles, int64_t need) const { return mt256() * col_tiles >= need; }
  // ... and a one-workgroup-per-CU kernel whose last resident round is mostly empty loses it whole: 380 tiles = 1.48
  // rounds of 256 run at 74 % (the 8-speaker pre-net, 97 152 x 256 x 512: 261 against 312 TFLOP/s on the persistent kernel)
  bool rounds_ok(int64_t col_tiles) const { const int64_t t = mt256() * col_tiles; return t * 5 >= rup(t, 256) * 4; }
  // (the persistent big tile against the persistent 256 x 128 tile, whose list is twice as fine: 90 %)
  bool rounds_ok9(int64_t col_tiles) const { const int64_t t = mt256() * col_tiles; return t * 10 >= rup(t, 256) * 9; }
  // the folded Tanh backward with the un-combining remap reads its aux operand in the unhidden epilogue -- below K = 1536
  // the eight-wave tiles win (280 against 230 at 194 304 x 1280 x 1024; at K = 2400, the default size, `big` leads 338 to 300)
  bool aux_remap_short() const { return g->act == 2 && sm.remap && g->K < 1536; }

  // ---- weight-gradient family
  int ones() const { return g->b_ones_col ? 1 : 0; }
  int64_t nreal() const { return g->N - ones(); }
  int64_t ks() const { return g->b_kshift < 0 ? -g->b_kshift : g->b_kshift; }
  int64_t ktiles() const { return cdiv(g->K, 16); }
  // Occupancy of a weight gradient: its tiles times the splits its K allows (>= 8 K tiles of 16 rows per split, <= 64
  // splits) must fill three quarters of the CUs, else the next smaller tile is tried (the 8-utterance shard: K = 2024
  // rows -> 15 splits; the 256 x 160 tile of dW_hh then has 150 workgroups at most: 54 against 89 TFLOP/s on 128 x 128)
  int64_t max_splits() const { return std::min<int64_t>(64, std::max<int64_t>(1, ktiles() / 8)); }
  bool tn_fills(int64_t tiles) const { return tiles * max_splits() >= 192; }
};

// =============================================== row x row: A[M, K] B[N, K]^T ===============================================
// 192 x 320 persistent tile (gemm_bf16x3_bigp320.hip, round 4) where 320-wide column tiles compute at least 10 % fewer
// columns than 256-wide ones (N = 320: the Tanh projections and d(input) of birnn1; N = 600: 640 against 768 columns)
inline bool wants_big_p320(const GemmRequest& q) {
  const int64_t n320 = rup(q.g->N, 320), t320 = cdiv(q.g->M, 192) * (n320 / 320);
  return q.sw.big_p320 && n320 * 11 <= q.n256() * 10 && n320 * 10 <= q.g->N * 11 && !q.g->accumulate && q.sm.remap <= 1 &&
         t320 >= 192 && t320 * 10 >= rup(t320, 256) * 9;
}
// persistent big tile (gemm_bf16x3_bigp.hip, round 4): the same tile without the per-tile drain / dispatch / prologue and
// with a four times cheaper transposition -- plain / bias / Tanh stores, also remapped (the logit layer), any K.  profiles/r4_ab_gemm_big_p.jsonl: 5.57
// against 6.46 ms (big) at 777 216 x 2400 x 513, 3.53 against 4.15 (stream) at K = 320; the shorter fixed part of a tile
// also pays for more column padding than the tiled kernel's 10 %: N = 600 (768 columns computed) 1.05 against 1.12 ms on
// the streaming kernel
// (N = 256 q + 1 with M a multiple of 256: q tiles + the VALU column, as in the tiled kernel)
inline bool wants_big_p(const GemmRequest& q) {
  const tssep_gemm_args* g = q.g;
  const bool pads_to_256_loosely = g->N >= 256 && q.n256() * 100 <= g->N * 130;
  return q.sw.big_p && (pads_to_256_loosely || (q.xcol_shape() && g->M % 256 == 0 && !q.sm.remap)) && q.sm.remap <= 1 &&
         !g->accumulate && q.fills(q.ct256(), 192) && q.rounds_ok9(q.ct256());
}
// big-tile kernel (gemm_bf16x3_big.hip) where the 256-wide tile applies.  (K < 448: a tile's life is mostly its
// C store there -- the streaming kernel, which hides it, measured 4.14 against 4.56 ms at K = 320, N = 2400; from
// K = 513 up this kernel wins: 6.55 / 6.63, 3.10 / 3.42 at K = 1280, 2.75 / 3.29 at K = 2400, N = 1280; sw.big 2 =
// regardless of K)
// Round 4 (profiles/r4_gemm_shape_sweep.jsonl, units x projs x speakers): N = 256 / 512 (projs = 256) belong here too
// (302 against 244 TFLOP/s at 777 216 x 256 x 1024 with the Tanh store); not the short-K folded Tanh backward with the
// un-combining remap (aux_remap_short)
inline bool wants_big(const GemmRequest& q) {
  const bool pads_to_256_any = q.g->N >= 256 && q.n256() * 10 <= q.g->N * 11;      // < 10 % column padding, also one or two column tiles (projs = 256)
  return q.sw.big && (!q.short_k() || q.sw.big == 2) && (pads_to_256_any || q.xcol_shape()) && !q.aux_remap_short() &&
         q.fills(q.ct256(), 192) && q.rounds_ok(q.ct256());
}
// persistent streaming kernel (gemm_bf16x3_stream.hip): plain row-major stores; the N = 256 q + 1 shapes keep
// the wide tile with its VALU column
inline bool wants_stream(const GemmRequest& q) { return q.sw.stream && !q.sm.remap && !n_256q_plus_1(q.g->N) && q.fills(cdiv(q.g->N, 128), 128); }
// 256 x 160 tile where 160-wide column tiles waste >= 10 % fewer columns than 128-wide ones (N = 320: the Tanh
// projections and d(input) of birnn1, which the two kernels above do not take)
// (a looser rule -- 4 % fewer columns at short K, for the logit layer's N = 2052 -- looked 19 % better in the first,
// incumbent-first sweep and measured equal to slower in the interleaved one: not adopted)
inline bool wants_nt_w160(const GemmRequest& q) { const int64_t n160 = rup(q.g->N, 160); return q.sw.nt_w160 && n160 * 11 <= rup(q.g->N, BN) * 10 && q.fills(n160 / 160, 192); }
// wide (256 x 256) eight-wave tile where rounding N up to 256 wastes < 10 % of the columns
// (not below K = 448: 145 against 207 TFLOP/s on the four-wave tile for the 8-speaker logit layer, 97 152 x 4104 x 256;
// from K = 448 up the big-tile kernel above has taken the request unless it cannot address it)
inline bool wants_tall4(const GemmRequest& q) {
  const bool pads_to_256 = q.g->N >= 1024 && q.n256() * 10 <= q.g->N * 11;      // < 10 % column padding
  return q.sw.wide && pads_to_256 && !q.short_k() && !q.aux_remap_short() && q.fills(q.n256() / 256, 192);
}
// ... with the VALU column (the launcher requires xcol_shape)
inline bool wants_tall4_xcol(const GemmRequest& q) { return q.sw.xcol != 0 && q.fills((q.g->N - 1) / 256, 192); }
inline bool wants_tall2(const GemmRequest& q) { return q.fills(cdiv(q.g->N, BN), 192); }

// ============================= weight gradients: dW[M, N] = dY[K, M]^T X[K, N], split over K =============================
// What every kernel of the family requires: both operands k-major, plain store, 16-byte rows (see gemm_bf16x3_tn_kernel)
inline bool tn_takes(const GemmRequest& q) {
  const tssep_gemm_args* g = q.g;
  return g->a_kmajor && g->b_kmajor && !q.sm.remap && !g->bias && g->act == 0 && (g->lda & 3) == 0 && (g->ldb & 3) == 0 &&
         aligned16(g->A) && aligned16(g->B) && rup(g->M, 4) <= g->lda && q.nreal() >= 1 && rup(q.nreal(), 4) <= g->ldb &&
         g->M >= 4 && (!q.shift || (q.ks() <= 32 && q.ks() < g->K));
}
// Split counts: tools/sweep_splitk.py, profiles/r2_splitk_sweep.jsonl, r3_wgrad_*_sweep.jsonl -- a model
// that prices whole rounds of 512 resident workgroups predicts up to 20 % from other factors; measured, the large-K
// shapes get SLOWER with more splits (the tiles of a K slab share it through one L2 only while they run together),
// and these rules are within 0..5 % of the best S on every shape of the step.
// (the workgroups of S / 8 K slabs per XCD, in whole rounds of its 32 CUs)
inline double xcd_round_waste(int64_t tiles, int S) { const int64_t wg = tiles * (S / 8); return (double)rup(wg, 32) / (double)wg; }
// the smallest multiple of 8 (<= smax, >= kt_min K tiles per split) within `slack` of the best fill of whole rounds of 32
inline int smallest_s_near_best_fill(const GemmRequest& q, int64_t tiles, int smax, int kt_min, double slack) {
  double waste = 1e30;
  for (int S = 8; S <= smax && (int64_t)S * kt_min <= q.ktiles(); S += 8) waste = std::min(waste, xcd_round_waste(tiles, S));
  for (int S = 8; S <= smax && (int64_t)S * kt_min <= q.ktiles(); S += 8)
    if (xcd_round_waste(tiles, S) <= waste * slack) return S;
  return 8;
}
// The general rule (128 x 128 tiles: tn, tn_tall, and every kernel below K of its own rule)
inline int splits_general(const GemmRequest& q) {
  const int64_t ktiles = q.ktiles(), tiles = cdiv(q.g->M, 128) * cdiv(q.g->N, 128);
  // the two largest dW_ih GEMMs of the step (K = 777 216 rows, 95 / 57 tiles): the sweep's best S is the smallest one --
  // 8.37 vs 8.65 ms and 5.16 vs 5.24 ms standalone, -0.5 ms per step in an alternating A/B x3
  if (q.g->K >= 400000 && tiles >= 48) return 8;
  const int64_t smax = ktiles / 8;          // every split keeps >= 8 K tiles
  if (tiles <= 16 && ktiles >= 64 * 8) {
    // few tiles (a projection weight gradient off the 320-row tile): one resident round of 512 workgroups -- 32 splits
    // 1.38 ms, the 56 of the general rule 1.51 (tools/sweep_wgrad_small.py); never more splits than K tiles allow
    const int64_t v = std::min(512 / tiles / 8 * 8, smax / 8 * 8);
    return (int)std::max<int64_t>(v, 8);
  }
  int64_t sp = std::max<int64_t>(1, std::min(cdiv(768, tiles), smax));
  // multiples of the XCD count: split z runs on XCD z % 8 (gemm_common.h)
  if (sp > 1) sp = std::min(rup(sp, 8), std::max<int64_t>(smax / 8 * 8, 8));
  return (int)std::min<int64_t>(sp, 64);
}

// gemm_bf16x3_tn_w160.hip, its three forms (tn_w160_wide, gemm_common.h) in the order they are tried:
// 256 x 320 workgroups (round 5) for the dW_ih GEMMs whose input width is a multiple of
// 320 (+ the ones column): birnn1 (N = 321) 3.14 against 3.79 ms on the 192 x 320 tile, birnn2 (N = 1281) 3.00 against
// 3.61 ms on the 512 x 128 tile (tools/exp_wgrad_w320.py) -- 31 % / 28 % fewer staged bytes per MFMA; M pads to 256
// by at most 8 % (the logit layer's M = 2052 stays on the 192-row tile)
// (256 x 256 workgroups, round 5: dW_ih of birnn0, N = 513 + 1 -- two column tiles + two VALU columns, 20 % fewer staged
// bytes per MFMA than the 512 x 128 tile)
inline int64_t tn_w160_wide_tiles(const GemmRequest& q, int wide) {      // (extra columns ride on the VALU)
  return (rup(q.g->M, 256) / 256) * cdiv(tn_w160_wide_cols(q.g, wide), wide == 4 ? 256 : 320);
}
// (swapped operands, round 5: the projection weight gradients -- 320 x 600 + 1 -- 0.92 against 1.34 ms on the 320 x 128 tile)
// (from K = 81 920 rows: the three tiles of the swapped problem need ~80 splits of >= 64 K tiles each to fill the chip)
inline bool wants_tn_w160_swapped(const GemmRequest& q) { return q.sw.tn_w160 && tn_w160_wide(q.g) == 7 && !q.two && q.g->K >= 80 * 64 * 16; }
// (M pads to 256-row tiles by at most 13 %: the logit layer's 2052 -> 2304, 0.69 against 0.83 ms on the 192 x 320 tile)
inline bool wants_tn_w160_wide(const GemmRequest& q) {
  const tssep_gemm_args* g = q.g;
  const int wide = tn_w160_wide(g);
  const bool takes = wide == 4 || (wide == 5 && rup(tn_w160_wide_cols(g, wide), 320) <= rup(g->N, 128));
  return q.sw.tn_w160 && !q.shift && takes && g->M >= 1024 && (rup(g->M, 256) - g->M) * 100 <= 13 * g->M &&
         q.tn_fills(tn_w160_wide_tiles(q, wide));
}
// 256 x 160 tile where 160-wide column tiles waste >= 10 % fewer columns than 128-wide ones (dW_hh: N = units = 300)
inline bool wants_tn_w160(const GemmRequest& q) {
  const int64_t n160 = rup(q.g->N, 160);
  return q.sw.tn_w160 && n160 * 11 <= rup(q.g->N, BN) * 10 && q.tn_fills(cdiv(q.g->M, 256) * (n160 / 160));
}
inline int splits_tn_w160(const GemmRequest& q) {
  const tssep_gemm_args* g = q.g;
  if (q.ktiles() < 64 * 8) return splits_general(q);
  const int wide = tn_w160_wide(g);
  // swapped operands: the tiles of the transposed problem (three for 320 x 600 + 1), up to 96 splits as on the 320 x 128
  // tile before (0.92 ms at S = 80, 1.06 at 64, 1.16 at 48; 777 216 rows)
  if (wide == 7) return smallest_s_near_best_fill(q, cdiv(g->N, 256) * cdiv(g->M, 320), 96, 64, 1.07);
  // 256 x 320 tiles, ONE workgroup per CU, the tiles of a K slab on one XCD (32 CUs): the multiple of 8 that fills whole
  // rounds of 32 best, the smallest one among equals, >= 64 K tiles per split (tools/exp_wgrad_w320.py: dW_ih of birnn1,
  // 10 tiles: 3.14 ms at S = 24, 3.25 at 48, 3.75 at 16; birnn2, 40 tiles: 3.00 at 32, 3.09 at 24, 3.43 at 48; dW_hh,
  // 5 tiles: 48; tools/exp_wgrad_w320.py --sweep)
  // (the smallest S within 7 % of the best fill: dW_ih of birnn0, 20 tiles, 5.54 ms at S = 24 (60 per XCD), 5.69-5.79 at 64
  // (160 = five full rounds) -- and a third of the partial sums to reduce)
  if (wide) return smallest_s_near_best_fill(q, tn_w160_wide_tiles(q, wide), 64, 64, 1.07);
  // 256 x 160 tile, two workgroups per CU, one round of at most 512 (tools/sweep_wgrad_splits.py: dW_hh 2.00 ms at
  // S = 48, 2.30 at 40, 3.13 at 56)
  const int64_t tiles = (rup(g->M, 256) / 256) * (rup(g->N, 160) / 160);
  return (int)std::max<int64_t>(8, std::min(512 / tiles / 8 * 8, q.ktiles() / 64 / 8 * 8));
}

// 192 x 320 tile (gemm_bf16x3_tn_p320.hip, round 4) where it computes at least 10 % less than the 512 x 128 tile:
// N = 320 (+ the ones column) -- dW_ih of birnn1: 2496 x 320 against 2560 x 384, the logit layer's weight gradient
// (M = 2052): 2112 x 320 against 2560 x 384
inline int64_t tn_p320_tiles(const GemmRequest& q) { return cdiv(q.g->M, 192) * cdiv(q.nreal(), 320); }
inline bool wants_tn_p320(const GemmRequest& q) {
  const int64_t a320 = tn_p320_tiles(q) * 192 * 320;
  const int64_t a512 = rup(q.g->M, 512) * tn_big_col_tiles(q.g->N, q.ones(), 1) * 128;
  return q.sw.tn_p320 && !q.shift && !q.two && q.g->M >= 768 && a320 * 100 <= a512 * 90 && q.tn_fills(tn_p320_tiles(q));
}
inline int splits_tn_p320(const GemmRequest& q) {
  if (q.g->K < 16 * 64) return splits_general(q);
  // 192 x 320 tiles, ONE workgroup per CU, the tiles of a K slab on one XCD (32 CUs): the multiple of 8 that fills whole
  // rounds of 32 best (13 tiles: 56 splits = 91 workgroups per XCD in 3 rounds)
  int best = 8; double waste = 1e30;
  for (int S = 8; S <= 64 && (int64_t)S * 8 <= q.ktiles(); S += 8) {
    const double w = xcd_round_waste(tn_p320_tiles(q), S);
    if (w < waste - 1e-9) { waste = w; best = S; }
  }
  return best;
}

// big-tile weight-gradient kernel: unshifted, M padded to 512 by at most a quarter (the dW_ih GEMMs: M = 8 units; round 4:
// the logit layer's M = speakers x 513 = 2052 / 4104 too -- 297 against 232 and 278 against 211 TFLOP/s on the tiles
// the 10 % rule of round 3 left them, profiles/r4_gemm_shape_sweep.jsonl)
inline bool wants_tn_big(const GemmRequest& q) {
  const int64_t m512 = rup(q.g->M, 512);
  return q.sw.tn_big && !q.shift && q.g->M >= 1024 && m512 * 4 <= q.g->M * 5 && q.tn_fills((m512 / 512) * cdiv(q.g->N, 128));
}
inline int splits_tn_big(const GemmRequest& q) {
  if (q.g->K < 16 * 64) return splits_general(q);
  // 512 x 128 tiles, ONE workgroup per CU, the tiles of a K slab on one XCD (32 CUs) -> as many slabs per XCD as fill
  // its CUs best; multiples of 8 only (N = 128 q + 1 | 2: the last columns ride on the VALU of the q-th column tile)
  return smallest_s_near_best_fill(q, cdiv(q.g->M, 512) * tn_big_col_tiles(q.g->N, q.ones(), q.sw.tn_xc), 32, 0, 1.0);
}

// 320 x 128 tile where 320-row tiles waste >= 10 % fewer rows than 128-row ones (the projection weight
// gradients: M = projs = 320, N = 2 units + 1: 1.18 vs 1.38 ms at each kernel's best split count), four column
// tiles or more (one column tile: 0.13 vs 0.08 ms, profiles/r3_wgrad_h160_sweep.jsonl)
inline int64_t tn_h160_tiles(const GemmRequest& q) { return (rup(q.g->M, 320) / 320) * cdiv(q.g->N, 128); }
inline bool wants_tn_h160(const GemmRequest& q) {
  return q.sw.tn_h160 && !q.shift && rup(q.g->M, 320) * 11 <= rup(q.g->M, BM) * 10 && q.g->N > 3 * BN && q.tn_fills(tn_h160_tiles(q));
}
inline int splits_tn_h160(const GemmRequest& q) {
  if (q.ktiles() < 64 * 8) return splits_general(q);
  // 320 x 128 tile, two workgroups per CU, one round of at most 512, at most 96 splits
  return (int)std::max<int64_t>(8, std::min<int64_t>({512 / tn_h160_tiles(q) / 8 * 8, 96, q.ktiles() / 16 / 8 * 8}));
}

// 256 x 128 tile (the launcher requires M >= 1024 padding to 256-row tiles by at most 8 %, |shift| <= 16).
// rule 4: the time-shifted dW_hh GEMMs (-2.3 ms per step, alternating A/B) and, round 3, the unshifted ones
// with at most 3 or at least 9 column tiles (dW_ih of birnn1: N = 321, birnn2: N = 1281 -- 4.89 vs 5.27 ms and
// 4.28 vs 4.55 ms with the split counts tssep_gemm_wgrad_splits gives them, profiles/r3_wgrad_tile_sweep.jsonl);
// the 5-column-tile shapes (N = 514 / 554) stay on the 128 x 128 tile: there the larger tile measured equal or
// slower at every split count.  (1: all eligible, 2: shifted only, 3: unshifted only, 0: off)
inline bool wants_tn_tall(const GemmRequest& q) {
  const int64_t tmode = q.sw.tn_tall, ntl = cdiv(q.g->N, BN);
  const bool want = tmode == 1 || (tmode == 2 && q.shift) || (tmode == 3 && !q.shift) ||
                    (tmode == 4 && (q.shift || ntl <= 3 || ntl >= 9));
  return want && q.tn_fills(cdiv(q.g->M, 256) * ntl);
}
inline bool wants_always(const GemmRequest&) { return true; }      // tn, pipe: what is left of their family

// A row of the candidate table (gemm_bf16x3.hip): the kernel, its name (tssep_gemm_kernel_name), the family whose
// preconditions guard the row, the rule, the launcher, and the split rule of a weight-gradient kernel (null: the general one)
enum GemmFamily { GEMM_ANY, GEMM_NT, GEMM_TN };
struct GemmCandidate {
  int32_t kid; const char* name; GemmFamily family;
  bool (*wants)(const GemmRequest&);
  int (*launch)(const GemmRequest&, const GemmCall&);
  int (*splits)(const GemmRequest&);
};

}  // namespace gemm_detail

// the first row of kernel `kid` in the table, or null
const gemm_detail::GemmCandidate* tssep_gemm_bf16x3_candidate(int32_t kid);
