/*
 * tssep_hip.h -- C ABI of libtssep_hip.so: the MI355X (gfx950) kernels behind the
 * TS-VAD / TS-SEP forward/backward hot path.
 *
 * The reference (merlresearch/tssep) has no FFI: every operation below replaces a
 * PyTorch ATen call made from the reference's Python hot path.  Each entry point
 * cites the reference call site (file:line under /root/reference) it replaces.
 *
 * Conventions
 *   - plain device pointers + explicit sizes/leading dimensions; no torch types
 *   - the CALLER owns every buffer (inputs, outputs, workspace); nothing is
 *     allocated, nothing global is mutated, no host synchronisation inside, and the
 *     library reads no environment variable: what runs is a function of the arguments
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*)
 *   - return value: 0 = ok, <0 = TSSEP_E_* (invalid shape / alignment / unsupported);
 *     never throws across the boundary
 *   - all floating point is IEEE fp32 (complex = interleaved re,im fp32)
 *   - re-entrant across streams/devices; no internal locking
 */
#ifndef TSSEP_HIP_H
#define TSSEP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSSEP_OK 0
#define TSSEP_E_SHAPE (-1)       /* a size is out of the supported range        */
#define TSSEP_E_ALIGN (-2)       /* a pointer / leading dimension is misaligned */
#define TSSEP_E_UNSUPPORTED (-3) /* valid request the kernels do not cover      */
#define TSSEP_E_LAUNCH (-4)      /* hipLaunch reported an error                 */
#define TSSEP_E_NULL (-5)        /* required pointer is NULL                    */

/* Library identification: returns ABI version (bumped on any signature change). */
int tssep_abi_version(void);
/* Name of the code object target the library was built for ("gfx950"). */
const char* tssep_arch(void);

/* ------------------------------------------------------------------ probes ---
 * Hardware self-checks used by tests: dump the lane<->element maps of the MFMA
 * instructions the kernels rely on.  out: device float[...] (see probe.hip). */
int tssep_probe_mfma(float* out_4x4, float* out_32x32, void* stream);
/* out[b] = XCD (HW_REG_XCC_ID) that ran workgroup b of an nblocks x 512-thread launch. */
int tssep_probe_xcc(int* out, int nblocks, void* stream);
/* Shader clock under load: out[2b] = s_memtime ticks, out[2b+1] = 100 MHz reference ticks spent by
 * block b in `iters` x 8 bf16 MFMAs per wave (heavy != 0) or as many s_sleep (heavy == 0). */
int tssep_probe_clock(int64_t* out, int nblocks, int iters, int heavy, void* stream);
/* Store-flavour probe: every one of `nblocks` workgroups rewrites its own bytes_per_wg (multiple of 4096) of buf
 * `reps` times with 16-byte stores of one flavour (0 plain, 1 sc0, 2 sc1, 3 sc0 sc1, 4 nt), streams `pressure`
 * bytes (0: none) of stream_src [2 x stream_bytes: the upper half receives 2/3 x pressure bytes of non-temporal
 * stores per rewrite] through the L2 between two rewrites, and -- read_flavour != 0 -- reads
 * the region of the workgroup 8 blocks on (same XCD) with 16-byte loads (1 sc1, 2 nt, 3 sc0 sc1, 4 sc0) after every
 * rewrite.  Under rocprofv3 --pmc WRITE_SIZE it tells whether rewritten lines reach the memory side once or every
 * time, and whether a peer's read forces them out (the exchange granules of the W-stationary recurrences: DESIGN 4.2). */
int tssep_probe_rewrite(float* buf, int nblocks, int bytes_per_wg, int reps, int flavour, int read_flavour,
                        const float* stream_src, int64_t stream_bytes, int pressure, float* sink, void* stream);

/* ------------------------------------------------------------------- STFT ----
 * paderbox-semantics STFT (fading + end padding + periodic window + rfft, no
 * scaling).  Replaces fe.stft at tssep/train/model.py:503-504.
 *   x      [rows, N]            real input (rows = B*C)
 *   window [size]               analysis window
 *   tw     [size/2 + size/4..]  twiddle table built by tssep_fft_twiddles
 *   X      [rows, T, size/2+1]  complex64 out, T = tssep_stft_frames(N,...)
 * FFT plans (tssep_stft_plan): 1 = size 1024 / shift 256, the plan of the reference's configs
 * (tssep/exp/init_cfg_common.yaml:33-43; specialised kernels, the only plan of the fused tssep_mask_istft_* entry points);
 * 2 = the general plan behind tssep_stft_fwd / tssep_istft_fwd / tssep_istft_bwd: size even, size / 2 = 2^a 3^b 5^c <= 2048,
 * 1 <= shift <= min(size, 512) -- 512 / 128, TorchMFCC's own default 400 / 200
 * (tssep/train/feature_extractor_torchaudio.py:24-25), ...; 0 = not built -> TSSEP_E_UNSUPPORTED. */
int tssep_stft_plan(int size, int shift);
int64_t tssep_stft_frames(int64_t N, int size, int shift, int window_length,
                          int pad, int fading);
int tssep_fft_twiddles(int size, float* host_out /* HOST buffer, 2*(size/2 + size/2+1) floats */);
int tssep_stft_fwd(const float* x, int64_t rows, int64_t N, int size, int shift,
                   int fading, const float* window, const float* tw,
                   float* X, int64_t T, void* stream);

/* Inverse STFT (irfft, biorthogonal synthesis window, overlap-add, un-fade,
 * truncate).  Replaces fe.istft at tssep/train/model.py:661-664.
 *   X [rows, T, F] complex64, wsyn [size], y [rows, N]
 * Optional fused LogMAE partial sums (tssep/train/loss.py:244-247): with tgt [rows,N] and
 * abs_partial [rows, tssep_istft_chunks(N)] non-NULL, abs_partial[row,c] = sum over the
 * chunk's samples of |y - tgt| (summed in a fixed order -> deterministic). */
int64_t tssep_istft_chunks(int64_t N);
int tssep_istft_fwd(const float* X, int64_t rows, int64_t T, int size, int shift,
                    int fading, const float* wsyn, const float* tw,
                    float* y, int64_t N, const float* tgt, float* abs_partial, void* stream);
/* Adjoint of tssep_istft_fwd: dy [rows,N] -> dX [rows,T,F] complex64
 * (torch convention: dRe + i dIm). */
int tssep_istft_bwd(const float* dy, int64_t rows, int64_t N, int size, int shift,
                    int fading, const float* wsyn, const float* tw,
                    float* dX, int64_t T, void* stream);

/* Mask head fused with the inverse STFT and with its adjoint: the chain
 *   mask = sigmoid(logit)                      tssep/train/net.py:983
 *   stft_estimate = Observation * mask         tssep/train/enhancer.py:98-100
 *   time_estimate = fe.istft(stft_estimate)    tssep/train/model.py:661-664
 * without writing mask or stft_estimate (results identical to tssep_maskhead_fwd followed by
 * tssep_istft_fwd; the unfused entry points remain for callers that want the intermediates).
 *   logit [B, K, T, F] fp32, obs [B, T, F] complex64 (reference channel), y [B*K, N]
 *   tgt / abs_partial: as tssep_istft_fwd (rows = B*K).
 * Backward: dy [B*K, N] -> dlogit [B, K, T, F] = Re(conj(obs) dEst) m (1 - m), dEst = adjoint(dy)
 * (identical to tssep_istft_bwd followed by tssep_maskhead_bwd with dmask = NULL). */
int tssep_mask_istft_fwd(const float* logit, const float* obs, int64_t B, int64_t K, int64_t T,
                         int size, int shift, int fading, const float* wsyn, const float* tw,
                         float* y, int64_t N, const float* tgt, float* abs_partial, void* stream);
int tssep_mask_istft_bwd(const float* dy, const float* logit, const float* obs, int64_t B,
                         int64_t K, int64_t N, int size, int shift, int fading,
                         const float* wsyn, const float* tw, float* dlogit, int64_t T, void* stream);
/* The same backward with the time-domain loss in front and the final Linear behind it folded in:
 *   input : est, tgt [B*K, N] and the loss's own backward arguments instead of dy -- the frame samples are
 *           d LogMAE / d est = gout[b] sign(est - tgt) / (N ln10 sums[b])  (tssep/train/loss.py:244-247;
 *           sums == NULL: MAE, gout[b] sign(est - tgt) / N, loss.py:214-216), i.e. what tssep_logmae_bwd
 *           would have written to a [B, K, N] buffer first (tgt == NULL: `est` IS dy, as above);
 *   output: bt_major = 0: dlogit [B, K, T, F] as above; bt_major = 1: rows (b, t) x (speaker position
 *           iperm[b*K + k] (NULL: k), f) -- the layout the final Linear's backward GEMMs read, i.e. what
 *           tssep_logit_map_bwd (trials = 1, 'tf' resolution) would have produced from dlogit
 *           (tssep/train/net.py:637-641, 957-967 backwards). */
int tssep_mask_istft_bwd_loss(const float* est, const float* tgt, const float* sums, const float* gout,
                              const float* logit, const float* obs, int64_t B, int64_t K, int64_t N,
                              int size, int shift, int fading, const float* wsyn, const float* tw,
                              const int32_t* iperm, int bt_major, float* dlogit, int64_t T, void* stream);
/* The gated tail of MaskEstimator_v2(explicit_vad=True) (tssep/train/net.py:630, 969-979): logit rows of F + 1 = 514
 * floats, the VAD logit v at column 0 and the mask logits l_f at 1..513 -- the rows the head GEMM writes.
 *   forward : as tssep_mask_istft_fwd with the mask sigmoid(l_f) * sigmoid(v).
 *   backward: as tssep_mask_istft_bwd_loss (est = dy when tgt == NULL; iperm / bt_major alike) with
 *             d(l_f) = dm_f g s_f (1 - s_f) and d(v) = g (1 - g) sum_f dm_f s_f  (dm_f = Re(conj(obs) dEst_f), s_f =
 *             sigmoid(l_f), g = sigmoid(v); an in-wave reduction, deterministic) stored at column 0.  vad [B*K, T] and
 *             gout_vad [B] non-NULL add the SignalAndVADSigmoidBCE term (tssep/train/loss.py:348-395) of the gate:
 *             + gout_vad[b] (sigmoid(v) - vad) / (K T).  dlogit rows are F + 1 floats. */
int tssep_mask_istft_gated_fwd(const float* logit, const float* obs, int64_t B, int64_t K, int64_t T, int size,
                               int shift, int fading, const float* wsyn, const float* tw, float* y, int64_t N,
                               const float* tgt, float* abs_partial, void* stream);
int tssep_mask_istft_gated_bwd(const float* est, const float* tgt, const float* sums, const float* gout,
                               const float* vad, const float* gout_vad, const float* logit, const float* obs,
                               int64_t B, int64_t K, int64_t N, int size, int shift, int fading,
                               const float* wsyn, const float* tw, const int32_t* iperm, int bt_major,
                               float* dlogit, int64_t T, void* stream);

/* --------------------------------------------------------------- features ----
 * ConcaternatedSTFTFeatures(TorchMFCC, Log1pMaxNormAbsSTFT).stft_to_feature
 * (tssep/train/feature_extractor.py:352-360, feature_extractor_torchaudio.py:93-106,
 * feature_extractor.py:233-248).
 *   X     [B, T, F] complex64 (reference channel already selected)
 *   fb    [F, n_mels], dct [n_mels, n_mfcc]    (fp32, row major)
 *   out   [B, T, ld_out] : cols [0,n_mfcc) = MFCC, [n_mfcc, n_mfcc+F) = log1p feature
 *   ws    workspace, tssep_feat_workspace_bytes(B,T,n_mels,F,stat_axis) bytes
 * n_mfcc == 0 skips the MFCC block (plain Log1pMaxNormAbsSTFT).
 * stat_axis: the maximum the log1p feature is normalised by, Log1pMaxNormAbsSTFT's `statistics_axis`
 * (feature_extractor.py:239-242): 0 = 'tf' one per utterance (every shipped config), 1 = 't' one per
 * (utterance, frequency) over the frames, 2 = 'f' one per frame over the frequencies.
 * The dB floor (top_db) is taken over the WHOLE batch, as torchaudio's
 * AmplitudeToDB does for the 3-D input the reference passes.  top_db < 0 selects TorchMFCC's `log_mels`
 * (feature_extractor_torchaudio.py:98-100): log(mel + 1e-6) instead of dB, no floor.  The filterbank may be any
 * matrix whose columns are non-zero on ONE contiguous band (HTK or Slaney scale, with or without area normalisation). */
int64_t tssep_feat_workspace_bytes(int64_t B, int64_t T, int n_mels, int F, int stat_axis);
int tssep_feat_fwd(const float* X, int64_t B, int64_t T, int F,
                   const float* fb, const float* dct, int n_mels, int n_mfcc,
                   float top_db, int stat_axis, float* out, int64_t ld_out, void* ws, void* stream);

/* Spectral features without a maximum (csrc/specfeat.hip): AbsSTFT, Log1pAbsSTFT and MVNLog1pAbsSTFT
 * (tssep/train/feature_extractor.py:112-168 and the padertorch classes it star-imports).
 *   X     [B, T, F] complex64, 1 <= F <= 1025, 8-byte aligned
 *   out   float32, row pitch ld_out >= F, 4-byte aligned: columns [0, F) of each of the B T rows are written and nothing
 *         else (the caller may point it at column n_mfcc of a wider [B, T, ld] buffer)
 *   kind  0 = |X|;  1 = L = log1p(|X|);  2 = L - mean over the T frames of L, one mean per (b, f)
 *         (np.mean(feature, axis=-2, keepdims=True), feature_extractor.py:161); any other: TSSEP_E_UNSUPPORTED
 *   ws    tssep_specfeat_workspace_bytes(B, T, F, kind) bytes, 8-byte aligned: B F float64 means for kind 2; 0 bytes for
 *         kinds 0 and 1, whose ws may be NULL
 * |X| = sqrt(re re + im im) with every operation rounded to float32, L = log1pf of it: one routine for every kind and for
 * the causal call.  The mean is S / T with S the float64 sum of the frames' L in frame order.  Kinds 0 and 1 are one
 * launch, kind 2 two.  No atomics, the same bits on every run; no host sync, no allocation, capturable.  F > 1025, a
 * non-positive size, ld_out < F or a grid past 2^31 - 1 blocks (B F / 256, B T F / 1024): TSSEP_E_SHAPE.
 *
 * tssep_specfeat_causal_fwd: the running-mean form of kind 2 over a chunk of Tc >= 1 frames per utterance (this
 * project's own).  state [B, F + 1] float64, 8-byte aligned: columns 0..F-1 the sums S[b, f], column F the weight n[b];
 * state_in NULL = zeros (a fresh stream), state_out NULL = not written, a state_out overlapping state_in: TSSEP_E_SHAPE.
 * Per frame in frame order, a = forgetting in (0, 1] (else TSSEP_E_SHAPE), each operation rounded to float64:
 *     S = a S + (double)L;   n = a n + 1;   out = (float)((double)L - S / n)
 * One strict chain per (b, f): any split of an utterance into calls gives the bits of one call, the first frame of a
 * fresh stream is exactly 0, and with a = 1 the last frame equals kind 2's of the same frames.  One launch. */
int64_t tssep_specfeat_workspace_bytes(int64_t B, int64_t T, int F, int kind);
int tssep_specfeat_fwd(const float* X, int64_t B, int64_t T, int F, int kind,
                       float* out, int64_t ld_out, void* ws, void* stream);
int tssep_specfeat_causal_fwd(const float* X, int64_t B, int64_t Tc, int F, double forgetting,
                              const double* state_in, double* state_out,
                              float* out, int64_t ld_out, void* stream);

/* ------------------------------------------------------------------- GEMM ----
 * Exact-fp32 MFMA GEMM (v_mfma_f32_32x32x2_f32): C = epilogue(A x B).
 * Replaces nn.Linear / the LSTM input GEMM (tssep/train/rnnp.py:88-96,146-161,
 * tssep/train/net.py:663-666) and their autograd backward GEMMs.
 *   op A: a_kmajor=0 -> A(m,k)=A[m*lda+k]   ; a_kmajor=1 -> A(m,k)=A[k*lda+m]
 *   op B: b_kmajor=0 -> B(k,n)=B[n*ldb+k]   ; b_kmajor=1 -> B(k,n)=B[k*ldb+n]
 *   (kmajor=0 is the "row x row" form y = x W^T; kmajor=1 reads the transposed
 *    operand in place, used by dgrad / wgrad)
 * see struct for the fused prologue / epilogue options. */
typedef struct tssep_gemm_args {
  const float* A; const float* B; float* C;
  int64_t M, N, K;
  int64_t lda, ldb, ldc;          /* lda, ldb multiples of 4; A, B 16-byte aligned */
  int32_t a_kmajor, b_kmajor;     /* (1,0) is not built */
  /* time shift on the reduction index of a k-major B (wgrad of W_hh pairs dgates_t with
   * h_{t-1}): B row k is read at k+b_kshift and taken as 0 when (k % kperiod)+b_kshift
   * falls outside [0,kperiod).  kperiod = 0 disables. */
  int64_t b_kshift, kperiod;
  /* epilogue */
  const float* bias;              /* [N] added to every row; NULL = off */
  int32_t act;                    /* 0 none, 1 tanh (Tanh between post-net layers, net.py:623-625; computed as
                                   * 1 - 2 / (1 + e^2x) on the hardware exp / rcp: absolute error <= 3e-7),
                                   * 2 multiply by 1 - aux^2: the BACKWARD of that Tanh folded into the store of
                                   * the d(input) GEMM of the layer that consumed its output (aux = that input) */
  int32_t accumulate;             /* C += result */
  /* output remap (c_remap != 0): row m = (b*c_K + k)*c_T + t and column n = q*c_cm + r are
   * stored at C[b*c_sb + k*c_sk + t*c_st + q'*c_co + r], q' = c_perm ? c_perm[b*c_perm_ld+q] : q.
   * Covers 'spk time feature -> 1 time (spk feature)' (net.py:608-611) and
   * '1 time (spk mask freq) -> spk mask time freq' + the speaker un-permutation
   * (net.py:637-641, 957-967) inside the producing GEMM's store.
   * c_remap = 2: the same map through the plain 4-byte-per-lane store only (the reference the 16-byte variants
   * are tested against; same values). */
  int32_t c_remap;
  int64_t c_T, c_K, c_sb, c_sk, c_st, c_cm, c_co;
  const int32_t* c_perm; int64_t c_perm_ld;
  /* split-K: gridDim.z = splitk partial products are written to C + z*c_split_stride
   * (no bias/act/remap); the caller reduces them.  <=1 = single pass. */
  int32_t splitk; int64_t c_split_stride;
  /* arithmetic: 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32);
   * 1 = split-bf16 "bf16x3": every fp32 operand is split on the fly into bf16 hi + bf16 lo and
   *     the product is hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation
   *     (per-product relative error <= ~2^-16, i.e. fp32-class for the 1e-3 parity bar);
   * 2 = weight gradients only (a_kmajor = b_kmajor = 1): as 1 with the A_lo * B_hi product dropped -- dY enters as
   *     plain bf16, X keeps hi + lo (opt-in side line of bench.py, never the default);
   * 3 = plain bf16 (opt-in side line, never the default): both operands rounded to bf16, ONE product per k-step, fp32
   *     accumulation -- in the kernels that have the variant (the persistent row x row kernels TSSEP_GEMM_BIG_P /
   *     _BIG_P320); every other kernel computes a precision-3 request as precision 1 (at least as accurate). */
  int32_t precision;
  /* k-major B only, precision 1 only: column N-1 of B is VIRTUAL and reads as 1.0 for every valid
   * k, so column N-1 of C holds the column sums of A -- the bias gradient comes out of the
   * weight-gradient GEMM that streams d(gates) anyway (B then has N-1 real columns). */
  int32_t b_ones_col;
  /* act == 2 only: aux[m*ldaux + n], indexed like the UNREMAPPED C (row m, column n) */
  const float* aux; int64_t ldaux;
} tssep_gemm_args;
int tssep_gemm_f32(const tssep_gemm_args* args, void* stream);

/* The kernels behind tssep_gemm_f32.  The library picks one per request from the request alone (shape, layout,
 * epilogue): no environment variable, no global state.  A caller that wants to know, or to decide itself
 * (autotuning sweeps, A/B timing), uses the three calls below; every kernel of the split-bf16 family gives
 * bit-identical results for the same request (same k order per output element, same epilogue arithmetic). */
#define TSSEP_GEMM_AUTO 0        /* let the library choose                                                    */
#define TSSEP_GEMM_F32 1         /* precision 0: exact-fp32 MFMA, 128 x 128 tiles                              */
#define TSSEP_GEMM_PIPE 2        /* 128 x 128 x 32, every layout / epilogue                                    */
#define TSSEP_GEMM_TALL2 3       /* row x row, 256 x 128, four waves                                           */
#define TSSEP_GEMM_TALL4 4       /* row x row, 256 x 256, eight waves                                          */
#define TSSEP_GEMM_TALL4_XCOL 5  /* ... N = 256 q + 1: the last column on the VALU                             */
#define TSSEP_GEMM_BIG 6         /* row x row, 256 x 256, four waves of 128 x 128 (one per SIMD)               */
#define TSSEP_GEMM_STREAM 7      /* row x row, persistent, plain stores hidden behind the next tile            */
#define TSSEP_GEMM_NT_W160 8     /* row x row, 256 x 160                                                       */
#define TSSEP_GEMM_TN 9          /* weight gradient (both operands k-major), 128 x 128                         */
#define TSSEP_GEMM_TN_TALL 10    /* weight gradient, 256 x 128                                                 */
#define TSSEP_GEMM_TN_BIG 11     /* weight gradient, 512 x 128, four waves of 128 x 128                        */
#define TSSEP_GEMM_TN_W160 12    /* weight gradient, 256 x 160; eight waves on 256 x 320 / 256 x 256 (also swapped)  */
#define TSSEP_GEMM_TN_H160 13    /* weight gradient, 320 x 128                                                 */
#define TSSEP_GEMM_BIG_P 14      /* row x row, 256 x 256 persistent: plain / bias / Tanh store hidden behind tiles */
#define TSSEP_GEMM_BIG_P320 15   /* row x row, 192 x 320 persistent (N = 320 q): plain / bias / Tanh / its backward  */
#define TSSEP_GEMM_TN_P320 16    /* weight gradient, 192 x 320 (N = 320 q, + the ones column)                  */
#define TSSEP_GEMM_KERNEL_LAST 16
/* As tssep_gemm_f32, on the kernel named (TSSEP_GEMM_AUTO = tssep_gemm_f32); TSSEP_E_UNSUPPORTED when that
 * kernel does not cover the request. */
int tssep_gemm_f32_on(const tssep_gemm_args* args, int32_t kernel, void* stream);
/* *kernel = the kernel tssep_gemm_f32_on(args, force, .) would launch; nothing is launched, C may be NULL. */
int tssep_gemm_plan(const tssep_gemm_args* args, int32_t force, int32_t* kernel);
const char* tssep_gemm_kernel_name(int32_t kernel);
/* Recommended splitk (>= 1; < 0 = TSSEP_E_*) for the weight gradient dW[M,N] = dY[K,M]^T X[K,N] described by
 * `args` (a_kmajor = b_kmajor = 1; splitk, c_split_stride and C are ignored): follows the kernel the library
 * picks for it. */
int tssep_gemm_wgrad_splits(const tssep_gemm_args* args);
/* The split count the split rule OF kernel `kernel_id` (TSSEP_GEMM_*) gives this request: tssep_gemm_wgrad_splits returns
 * an S for which tssep_gemm_plan(.., splitk = S) names a kernel k with tssep_gemm_wgrad_split_rule(g, k) == S (a fixed
 * point), or 8 when there is none (ABI 4). */
int tssep_gemm_wgrad_split_rule(const tssep_gemm_args* g, int32_t kernel_id);

/* column sums: out[n] (+)= sum_m A[m*lda+n]  (bias gradients) */
int tssep_colsum_f32(const float* A, int64_t M, int64_t N, int64_t lda, float* out,
                     int accumulate, void* ws, void* stream);
int64_t tssep_colsum_workspace_bytes(int64_t M, int64_t N);

/* ------------------------------------------------------------------ BLSTM ----
 * One bidirectional LSTM layer, zero initial state (torch.nn.LSTM as used at
 * tssep/train/rnnp.py:88-95,146-153).  The input projection x W_ih^T + b is done by
 * tssep_gemm_f32 into `gates`; these kernels run the T-sequential recurrence.
 *
 * Packed layouts (built by tssep_lstm_pack from torch-layout parameters):
 *   gate columns are ordered [dir][unit][gate(i,f,g,o)]  (4H per direction)
 *   wih_p  [2*4H, ld_i]   rows permuted to that order, K zero-padded to ld_i
 *   bias_p [2*4H]         b_ih + b_hh, permuted
 *   whh_f / whh_b         streaming layouts for the forward / backward recurrence
 * sizes in floats: tssep_lstm_pack_sizes(). */
typedef struct tssep_lstm_sizes {
  int64_t wih_p, bias_p, whh_f, whh_b;   /* floats */
} tssep_lstm_sizes;
int tssep_lstm_pack_sizes(int H, int I, int64_t ld_i, tssep_lstm_sizes* out);
/* torch-layout parameters of both directions (suffix _f = forward, _r = "_reverse"):
 * w_ih [4H,I], w_hh [4H,H], b_ih [4H], b_hh [4H]  (gate-major rows i,f,g,o). */
int tssep_lstm_pack(const float* w_ih_f, const float* w_hh_f, const float* b_ih_f,
                    const float* b_hh_f, const float* w_ih_r, const float* w_hh_r,
                    const float* b_ih_r, const float* b_hh_r, int H, int I, int64_t ld_i,
                    float* wih_p, float* bias_p, float* whh_f, float* whh_b, void* stream);
/* gates [N,T,2,H,4]: in = pre-activations from the input GEMM; out = activated gates
 * (kept for backward).  cell [N,T,2,H]; hout [N,T,ldo] (cols d*dstride+u).  Columns of hout / dhout
 * outside d*dstride .. d*dstride+H-1 (dstride > H, ldo > dstride + H) are never written and never read by
 * any recurrence kernel, streaming or W-stationary: a caller whose next GEMM reads them zeroes them once
 * (tests/test_gpu_recurrence_kernels.py holds every kernel to this).  H <= 512 (round 4; the
 * W-stationary families below cover H <= 320 / 304, which is where the reference's configs live). */
int tssep_blstm_fwd(float* gates, float* cell, float* hout, int64_t ldo, int64_t dstride,
                    const float* whh_f, int64_t N, int64_t T, int H, void* stream);
/* dhout [N,T,ldo] -> gates is overwritten with d(pre-activation) in the same layout. */
int tssep_blstm_bwd(float* gates, const float* cell, const float* dhout, int64_t ldo,
                    int64_t dstride, const float* whh_b, int64_t N, int64_t T, int H, void* stream);
/* gradient unpack + split-K reduction: a matrix with packed (dir,unit,gate) rows back to
 * torch's gate-major rows:
 *   dst_d[(g*H + u)*ncols + k] (+)= sum_{s<nsplit} src[s*split_stride + (d*4H + 4u + g)*ld + k] */
int tssep_lstm_unpack(const float* src, int64_t ld, int nsplit, int64_t split_stride,
                      int H, int ncols, float* dst_f, float* dst_r, int accumulate, void* stream);

/* ONE direction of time (torch.nn.LSTM(bidirectional=False), tssep/train/rnnp.py:80-96 typ='lstm'): the streaming
 * kernels above instantiated for one direction -- 8 sequences per workgroup, no exchange between workgroups, no spin,
 * no error flag, no concurrency contract (capturable, safe beside anything).  Layouts are the [dir = 0] half of the
 * two-direction ones: gate columns [unit][gate], wih_p [4H, ld_i], bias_p [4H]; gates [N,T,H,4], cell [N,T,H],
 * hout / dhout [N,T,ldo] with columns 0..H-1 (H..ldo-1 are never written and never read).  H <= 512.
 * h0 / c0 [N,H]: the state the recurrence starts from -- both or neither (one alone: TSSEP_E_NULL); null = zeros.
 * hT / cT [N,H], each nullable: the state after the last frame, the bits of hout[:, T-1, :H] / cell[:, T-1].
 * tssep_lstm1_bwd assumes a ZERO initial state and no gradient for the final one; tssep_lstm1_bwd_state is the same
 * kernel with the carried state's gradient (truncated or full BPTT over chunks).  Every state argument is [N,H] and
 * nullable; all null = tssep_lstm1_bwd, bit for bit:
 *   c0        the state the forward started from (the forget gate's gradient at frame 0 reads it); null = zeros
 *   dhT, dcT  the gradient arriving for (hT, cT); null = zeros.  dhT stands where the four partial sums of
 *             W_hh^T d(gates) stand at the top of a step, (dhT + 0 + 0 + 0) + dhout[T-1], and dcT where the carried
 *             dc stands, so a backward run as chunks, last chunk first, each taking the next one's (dh0, dc0) as its
 *             (dhT, dcT) and cell[:, first frame - 1] as its c0, writes the bits of the one launch over all frames
 *   dh0, dc0  the gradient of (h0, c0), written when not null: the four partial sums of the last product in the
 *             order a step adds them, and the carried dc * f
 * The term sum_n d(gates)[n, 0]^T h0[n] of dW_hh is the caller's (the frame-shifted product pairs frame 0 with 0). */
int tssep_lstm1_pack_sizes(int H, int I, int64_t ld_i, tssep_lstm_sizes* out);
int tssep_lstm1_pack(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                     int H, int I, int64_t ld_i, float* wih_p, float* bias_p, float* whh_f,
                     float* whh_b, void* stream);
int tssep_lstm1_fwd(float* gates, float* cell, float* hout, int64_t ldo, const float* whh_f,
                    const float* h0, const float* c0, float* hT, float* cT,
                    int64_t N, int64_t T, int H, void* stream);
int tssep_lstm1_bwd(float* gates, const float* cell, const float* dhout, int64_t ldo,
                    const float* whh_b, int64_t N, int64_t T, int H, void* stream);
int tssep_lstm1_bwd_state(float* gates, const float* cell, const float* dhout, int64_t ldo, const float* whh_b,
                          const float* c0, const float* dhT, const float* dcT, float* dh0, float* dc0,
                          int64_t N, int64_t T, int H, void* stream);
/* dst[(g*H + u)*ncols + k] (+)= sum_{s<nsplit} src[s*split_stride + (4u + g)*ld + k] */
int tssep_lstm1_unpack(const float* src, int64_t ld, int nsplit, int64_t split_stride,
                       int H, int ncols, float* dst, int accumulate, void* stream);

/* -------------------------------------------------------------------- GRU ----
 * One GRU layer over one or two directions of time (torch.nn.GRU as built at tssep/train/rnnp.py:40,87 for
 * typ = 'gru' / 'bgru'; one layer, batch_first): the streaming decomposition of tssep_blstm_* / tssep_lstm1_* -- 8
 * sequences x 1 direction per workgroup, no exchange between workgroups, no spin, no error flag, no concurrency
 * contract (capturable, safe beside anything), exact fp32.  H <= 512.  torch's math, parameter rows gate-major (r, z, n):
 *   r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)       z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
 *   n = tanh(W_in x + b_in + r * (W_hn h + b_hn))     h' = (1 - z) * n + z * h
 *
 * Every unit owns FOUR slots (r, z, n, q), q = W_hn h + b_hn (apart, because r multiplies it), so every shape of the
 * LSTM path holds: gate columns [dir][unit][slot], 4H per direction.  Packed by tssep_gru_pack (sizes in floats:
 * tssep_gru_pack_sizes, the LSTM's struct -- they are the LSTM's sizes):
 *                         slot 0          slot 1          slot 2      slot 3
 *   wih_p  [nd*4H, ld_i]  W_ir[u]         W_iz[u]         W_in[u]     0          (K zero-padded to ld_i)
 *   bias_p [nd*4H]        b_ir + b_hr     b_iz + b_hz     b_in        b_hn
 *   whh_f / whh_b         W_hr[u]         W_hz[u]         0           W_hn[u]    (streaming layouts, forward / BPTT)
 * nd = 1 | 2 directions; nd = 1: the *_r pointers are not read (null is fine) and every [dir] axis has one entry.
 * w_ih [3H,I], w_hh [3H,H], b_ih [3H], b_hh [3H]. */
int tssep_gru_pack_sizes(int nd, int H, int I, int64_t ld_i, tssep_lstm_sizes* out);
int tssep_gru_pack(int nd, const float* w_ih_f, const float* w_hh_f, const float* b_ih_f,
                   const float* b_hh_f, const float* w_ih_r, const float* w_hh_r,
                   const float* b_ih_r, const float* b_hh_r, int H, int I, int64_t ld_i,
                   float* wih_p, float* bias_p, float* whh_f, float* whh_b, void* stream);
/* Two directions.  gates [N,T,2,H,4]: in = the input GEMM's (a_r, a_z, a_n, b_hn); out = (r, z, n, q), kept for the
 * backward.  hout [N,T,ldo] (cols d*dstride+u; the columns outside are never written and never read, as for
 * tssep_blstm_fwd).  There is no cell tensor: the state is h. */
int tssep_gru_fwd(float* gates, float* hout, int64_t ldo, int64_t dstride, const float* whh_f,
                  int64_t N, int64_t T, int H, void* stream);
/* dhout [N,T,ldo] -> gates is overwritten with (da_r, da_z, da_n, da_q) in the same layout; reads the forward's hout
 * (h_prev: the neighbouring frame in the direction's time order, 0 at its first frame). */
int tssep_gru_bwd(float* gates, const float* hout, const float* dhout, int64_t ldo, int64_t dstride,
                  const float* whh_b, int64_t N, int64_t T, int H, void* stream);
/* ONE direction, forward in time: gates [N,T,H,4], hout / dhout [N,T,ldo] with columns 0..H-1.
 * h0 [N,H], nullable: the state the recurrence starts from; null = zeros.  hT [N,H], nullable: the state after the
 * last frame, the bits of hout[:, T-1, :H].  tssep_gru1_bwd assumes a ZERO initial state and no gradient for the final
 * one; tssep_gru1_bwd_state is the same kernel with both, every state argument [N,H] and nullable (all null =
 * tssep_gru1_bwd, bit for bit): h0 is h_prev of frame 0, in dz = dh (h_prev - n); dhT is one more addend of dh at
 * frame T-1, in the carry's place: (0 + dhout) + dhT; dh0 = (p0 + p1 + p2 + p3) + dh z of frame 0.  A chunked backward is NOT
 * the whole launch's bits: the whole launch adds dhout between the partial sums and the carry, and one tensor dh0 cannot
 * hand both over apart (one rounding of dh per boundary).  The h0 term of dW_hh is the caller's, as for the LSTM. */
int tssep_gru1_fwd(float* gates, float* hout, int64_t ldo, const float* whh_f, const float* h0,
                   float* hT, int64_t N, int64_t T, int H, void* stream);
int tssep_gru1_bwd(float* gates, const float* hout, const float* dhout, int64_t ldo,
                   const float* whh_b, int64_t N, int64_t T, int H, void* stream);
int tssep_gru1_bwd_state(float* gates, const float* hout, const float* dhout, int64_t ldo, const float* whh_b,
                         const float* h0, const float* dhT, float* dh0,
                         int64_t N, int64_t T, int H, void* stream);
/* gradient unpack + split-K reduction: a matrix with packed (dir,unit,slot) rows back to torch's [3H, ncols] rows:
 *   dst_d[(g*H + u)*ncols + k] (+)= sum_{s<nsplit} src[s*split_stride + (d*4H + 4u + slot(g))*ld + k],  g = 0..2
 * which = TSSEP_GRU_IH: slot(g) = (0, 1, 2) -- dW_ih, db_ih; TSSEP_GRU_HH: slot(g) = (0, 1, 3) -- dW_hh, db_hh (the one
 * place where b_ih and b_hh stop sharing a gradient).  The unused slot's row of src is never read.  nd = 1: dst_r is
 * not written (null is fine). */
#define TSSEP_GRU_IH 0
#define TSSEP_GRU_HH 1
int tssep_gru_unpack(int nd, const float* src, int64_t ld, int nsplit, int64_t split_stride,
                     int H, int ncols, int which, float* dst_f, float* dst_r, int accumulate,
                     void* stream);

/* Cluster (W-stationary) recurrence -- latency-optimised alternative to tssep_blstm_fwd/bwd for
 * batches that do not fill the chip (same math, same tensor layouts; see lstm_cluster.hip).
 * A cluster of ceil(H/32) co-resident workgroups keeps W_hh in registers and exchanges h / dh
 * through 8-byte {tag,value} granules in `xbuf` (tssep_lstm_cluster_xbuf_bytes; zeroed inside
 * the call by a memset node on `stream`).  `max_wgs` = number of CUs (sizes the grid so that
 * neighbouring clusters hide each other's exchange latency; cluster membership is taken by
 * arrival ticket, so correctness does not depend on residency or dispatch order).
 * `ms` = sequences per cluster / 4: 2, 4, or 0 = automatic.  H <= 304, T < 65535.
 *
 * `err` (both W-stationary families, cluster and on-chip): device int[4], zeroed ONCE by the caller
 * and then owned by the library: err[0] is set non-zero when a bounded spin timed out (the workgroup
 * gives up and the outputs of that launch are garbage: the caller MUST read err[0] before it trusts
 * or checkpoints anything computed from them); err[1] is the launch epoch the granule tags carry,
 * advanced on the device in front of every launch (so captured hipGraphs replay with fresh epochs).
 *
 * CONCURRENCY CONTRACT: at most ONE W-stationary launch (tssep_blstm_cluster_* / tssep_blstm_onchip_*)
 * may be in flight per device at any time, across all streams and processes that share `err`: the
 * clusters are formed from the workgroups of one launch by arrival ticket and spin on their peers,
 * and two such grids competing for CUs can starve each other into the timeout.  Launch them on one
 * stream (other kernels may run concurrently on other streams). */
int tssep_lstm_cluster_supported(int H);
int64_t tssep_lstm_cluster_pack_floats(int H, int which /* 0: whh_cf, 1: whh_cb */);
int tssep_lstm_pack_cluster(const float* w_hh_f, const float* w_hh_r, int H,
                            float* whh_cf, float* whh_cb, void* stream);
int64_t tssep_lstm_cluster_xbuf_bytes(int64_t N, int H, int backward, int max_wgs, int ms);
int tssep_blstm_cluster_fwd(float* gates, float* cell, float* hout, int64_t ldo, int64_t dstride,
                            const float* whh_cf, void* xbuf, int* err,
                            int64_t N, int64_t T, int H, int max_wgs, int ms, void* stream);
int tssep_blstm_cluster_bwd(float* gates, const float* cell, const float* dhout, int64_t ldo,
                            int64_t dstride, const float* whh_cb, void* xbuf, int* err,
                            int64_t N, int64_t T, int H, int max_wgs, int ms, void* stream);

/* On-chip-weights recurrence on the bf16 matrix cores (lstm_onchip.hip): a cluster of
 * ceil(H/64) workgroups keeps W_hh on chip as split bf16 (hi+lo) and evaluates the recurrent
 * product as hi*hi + hi*lo + lo*hi with fp32 accumulation (fp32-class accuracy), 32 sequences per
 * cluster and step; h / partial dh travel as fp32 in 8-byte {tag, value} granules (the tag carries
 * a per-launch epoch and the step: the data is the flag).  Clusters are formed from workgroups of
 * ONE XCD (HW_REG_XCC_ID), so the exchange stays in that XCD's L2.  Same tensor layouts as
 * tssep_blstm_fwd/bwd.  `layout` bits: 1 = experimental time-major-in-groups-of-32 row order,
 * 8 = force cross-XCD clusters (write-through exchange), 32 = forward only: keep the activation
 * stream temporal (default: non-temporal from 160 sequences up, so that it does not evict the
 * exchange granules from the L2).  xbuf: caller-owned 16-byte-aligned scratch of
 * tssep_lstm_onchip_xbuf_bytes() bytes (zeroed by the call); err: device int[4] and the concurrency
 * contract as stated for the cluster kernels above.  max_wgs: number of CUs the launch may occupy.
 * H <= 304. */
int tssep_lstm_onchip_supported(int H);
/* Longest sequence (frames) one launch takes for `seqs_per_item` sequences per work item (32: the kernels
 * declared here; 16: the interleaved tssep_blstm_onchip16_* below): 32-bit lane offsets into the gate tensor,
 * ((1 << 31) - 8192) / ((seqs - 1) 2H 16) -- 14 913 / 7 215 frames at H = 300.  Longer: TSSEP_E_SHAPE (the
 * streaming kernels tssep_blstm_fwd/bwd have no limit, like tssep/train/rnnp.py:111-173). */
int64_t tssep_lstm_onchip_max_steps(int H, int seqs_per_item);
int64_t tssep_lstm_onchip_pack_floats(int H, int which /* 0: forward, 1: backward */);
int tssep_lstm_pack_onchip(const float* w_hh_f, const float* w_hh_r, int H, float* wf, float* wb,
                           void* stream);
int64_t tssep_lstm_onchip_xbuf_bytes(int64_t N, int H, int backward);
int tssep_blstm_onchip_fwd(float* gates, float* cell, float* hout, int64_t ldo, int64_t dstride,
                           const float* wf, void* xbuf, int* err, int64_t N, int64_t T, int H,
                           int max_wgs, int layout, void* stream);
int tssep_blstm_onchip_bwd(float* gates, const float* cell, const float* dhout, int64_t ldo,
                           int64_t dstride, const float* wb, void* xbuf, int* err, int64_t N,
                           int64_t T, int H, int max_wgs, int layout, void* stream);

/* Interleaved forward of the same recurrence (round 3): `groups` (2 or 1; 4 on request) independent groups of 16 sequences per
 * cluster share the stationary W_hh in rotation, so that a group's exchange of h overlaps the other groups' MFMAs and
 * cell updates (the kernel above walks one group of 32 sequences through a serial chain).  Same tensors, same
 * semantics, same err / concurrency contract; own weight pack (16 x 16 x 32 MFMA fragments) and own exchange
 * buffer layout.  tssep_blstm_onchip16_groups(): the group count the launcher uses for N sequences on max_wgs CUs
 * (0: shape not supported -- H % 4, H > 320 -- call tssep_blstm_onchip_fwd instead); groups = 0 in the launch = that
 * choice.  ldo, dstride multiples of 4; gates / cell / hout 16-byte aligned; XCD-local clusters only. */
int64_t tssep_lstm_onchip16_pack_floats(int H);
int tssep_lstm_pack_onchip16(const float* w_hh_f, const float* w_hh_r, int H, float* wf, void* stream);
int64_t tssep_lstm_onchip16_xbuf_bytes(int64_t N, int H);
int tssep_blstm_onchip16_groups(int64_t N, int H, int max_wgs);
int tssep_blstm_onchip16_fwd(float* gates, float* cell, float* hout, int64_t ldo, int64_t dstride,
                             const float* wf, void* xbuf, int* err, int64_t N, int64_t T, int H,
                             int max_wgs, int layout, int groups, void* stream);
/* Interleaved backward: the same rotation for the reduce-scatter of dh (exchange waves / io waves as in the forward, a
 * ring of four LDS slots {gate activations, c_(t-1), dh} filled by asynchronous copies two phases ahead).  Own weight
 * pack (W_hh^T as 16 x 16 x 32 MFMA fragments) and exchange layout; H = 257 .. 320 (five workgroups per cluster),
 * H % 4 == 0; groups as for the forward (0 = the launcher's choice). */
int64_t tssep_lstm_onchip16_bwd_pack_floats(int H);
int tssep_lstm_pack_onchip16_bwd(const float* w_hh_f, const float* w_hh_r, int H, float* wb, void* stream);
int64_t tssep_lstm_onchip16_bwd_xbuf_bytes(int64_t N, int H);
int tssep_blstm_onchip16_bwd(float* gates, const float* cell, const float* dhout, int64_t ldo, int64_t dstride,
                             const float* wb, void* xbuf, int* err, int64_t N, int64_t T, int H, int max_wgs,
                             int layout, int groups, void* stream);

/* ---------------------------------------------------------- elementwise ------*/
/* d(pre-tanh) = dy * (1 - y^2) for the Tanh between post-net layers (tssep/train/net.py:623-625).
 * dz rows are (b,k,t) x P; combined_in != 0: dy and y live in the speaker-combined layout
 * [B,T,K*P] of 'spk time feature -> 1 time (spk feature)' (net.py:608-611). */
int tssep_tanh_bwd(const float* dy, const float* y, float* dz, int64_t rows, int64_t P,
                   int64_t K, int64_t T, int combined_in, void* stream);
/* Dropout in front of a Tanh: Linear -> Dropout(p) -> Tanh inside RNNP_packed (tssep/train/rnnp.py:98-100) and
 * birnn -> Dropout(p) -> Tanh between post-net modules (tssep/train/net.py:623-625), training mode.
 *   keep(e) <=> word(e) >= floor(p * 2^32)   (64-bit compare: p = 0 keeps all, p = 1 none)
 *   word(e) = output word e % 4 of Philox4x32-10(counter = {e / 4 as lo, hi; draw as lo, hi}, key = seed as lo, hi)
 *   e = r * P + c: LOGICAL element (row r = (n,t) of the producing layer, column c), whatever layout it is stored in
 * (one definition for host and device: tssep_amd/csrc/dropout_philox.h).  p outside [0, 1]: TSSEP_E_SHAPE.
 * The two *_host functions run on the host and touch no GPU (tests, tools): the raw generator, and keep[i] (0 / 1) of the
 * elements first .. first + n - 1 of the mask {seed, draw}. */
int tssep_philox4x32_10_host(const uint32_t* ctr /* [4] */, const uint32_t* key /* [2] */, uint32_t* out /* [4] */);
int tssep_dropout_keep_host(int64_t seed, int64_t draw, int64_t first, int64_t n, double p, uint8_t* keep);
/* state, used: DEVICE int64[2] = {seed, draw}.  One thread: used <- state, then state.draw += 1.  Runs in front of every
 * dropout forward; the forward and its backward read `used`, so a replayed hipGraph draws a fresh mask each time. */
int tssep_dropout_draw(int64_t* state, int64_t* used, void* stream);
/* y = keep ? tanh(z / (1 - p)) : 0 with the Tanh of the GEMMs' fused store (act = 1) on z * fp32(1 / (1 - p)); y may
 * be z.  rows x P logical elements; combined == 0: row r at z + r * ld (ld >= P); combined != 0: z and y are the
 * speaker-combined [B,T,K*P] of rows (b,k,t), addressed as in tssep_tanh_bwd (ld is ignored). */
int tssep_dropout_tanh_fwd(const float* z, float* y, int64_t rows, int64_t P, int64_t ld, int64_t K, int64_t T,
                           int combined, double p, const int64_t* used, void* stream);
/* dz = keep ? dy * (1 - y^2) / (1 - p) : 0; layouts exactly as tssep_tanh_bwd (dz dense rows (b,k,t) x P). */
int tssep_dropout_tanh_bwd(const float* dy, const float* y, float* dz, int64_t rows, int64_t P, int64_t K, int64_t T,
                           int combined_in, double p, const int64_t* used, void* stream);
/* Speaker conditioning (tssep/train/net.py:862-896) fused with the permutation-trial fold
 * (net.py:913-924): xs rows are (b, trial, k, t); trial tr holds speaker (k+tr)%K at position k.
 *   mul: xs[row, f] = pre[(b,t), f] * aux[(b,spk), f]
 *   cat: xs[row, :] = [pre[(b,t), :F] | aux[(b,spk), :E]]
 * bwd: dpre[(b,t), f] = sum over (trial,k) rows (aux has no gradient: aux_net is None). */
int tssep_cond_mul_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux,
                       float* xs, int64_t ld_xs, int64_t B, int64_t K, int64_t T, int F,
                       int trials, void* stream);
int tssep_cond_mul_bwd(const float* dxs, int64_t ld_dxs, const float* aux, int64_t ld_aux,
                       float* dpre, int64_t ld_dpre, int64_t B, int64_t K, int64_t T, int F,
                       int trials, void* stream);
int tssep_cond_cat_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux,
                       float* xs, int64_t ld_xs, int64_t B, int64_t K, int64_t T, int F, int E,
                       int trials, void* stream);
int tssep_cond_cat_bwd(const float* dxs, int64_t ld_dxs, float* dpre, int64_t ld_dpre,
                       int64_t B, int64_t K, int64_t T, int F, int trials, void* stream);
/* The same conditioning on FRAME-WISE embeddings (net.py:866-867, aux_time = "time"): aux rows are (b, spk, ta) with
 * leading dimension ld_aux, frame t reads row ta = t / stride, and Ta == ceil(T / stride) (anything else, or
 * stride < 1: TSSEP_E_SHAPE before any launch).  stride = 1 is the reference's branch; stride >= T is one row per
 * speaker.  Each entry point shares its kernel (one template, the aux row index its only branch) and its launcher with
 * the entry point above of the same role: row decomposition, (trial, k) order and the choice between 16-byte and 4-byte
 * accesses are the same code, and a time-constant aux gives their bits.  d(pre) of cat does not read aux:
 * tssep_cond_cat_bwd.
 * Algorithmic HBM bytes (R = B*trials*K*T rows of xs; the aux rows are re-read `stride` times from the caches):
 *   mul fwd  4 * (R*F + B*T*F + B*K*Ta*F)          (pre re-read trials*K times from the caches)
 *   mul bwd  4 * (R*F + B*K*Ta*F + B*T*F)
 *   cat fwd  4 * (R*(F+E) + B*T*F + B*K*Ta*E) */
int tssep_cond_mul_t_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux, float* xs,
                         int64_t ld_xs, int64_t B, int64_t K, int64_t T, int F, int trials, int64_t Ta,
                         int64_t stride, void* stream);
int tssep_cond_mul_t_bwd(const float* dxs, int64_t ld_dxs, const float* aux, int64_t ld_aux, float* dpre,
                         int64_t ld_dpre, int64_t B, int64_t K, int64_t T, int F, int trials, int64_t Ta,
                         int64_t stride, void* stream);
int tssep_cond_cat_t_fwd(const float* pre, int64_t ld_pre, const float* aux, int64_t ld_aux, float* xs,
                         int64_t ld_xs, int64_t B, int64_t K, int64_t T, int F, int E, int trials, int64_t Ta,
                         int64_t stride, void* stream);

/* ------------------------------------------------- learned embeddings (aux.hip) ----
 * Gradient of the conditioning with respect to the embedding (aux_net / a trainable embedding, net.py:816-838):
 *   mul: d_aux[(b,s), f] = sum_tr sum_t dxs[(b,tr,(s-tr) mod K,t), f] * pre[(b,t), f]
 *   cat: d_aux[(b,s), e] = sum_tr sum_t dxs[(b,tr,(s-tr) mod K,t), F+e]
 * d_aux rows (b,s) with leading dimension ld_daux.  Two launches: partial sums per chunk of 64 frames (wave w of a
 * workgroup adds the frames t0+w, t0+w+4, ... of trial 0, 1, ... in that order, the four waves are added in ascending
 * order), then the chunks in ascending order: no atomics, bit-identical from run to run.  16-byte loads when
 * ld_dxs (and ld_pre) are multiples of 4 covering the 4-aligned column window and the pointers are 16-byte aligned.
 * ws: caller-owned, tssep_cond_aux_bwd_workspace_bytes(B, K, T, F, E) bytes (E = 0: mul; host-only, 0 = bad shape).
 * Algorithmic HBM bytes: 4 * B*trials*K*T * C (dxs columns read, C = F or E) [+ 4 * B*T*F of pre, re-read K*trials
 * times from the caches] + 4 * B*K*C. */
int64_t tssep_cond_aux_bwd_workspace_bytes(int64_t B, int64_t K, int64_t T, int F, int E);
int tssep_cond_mul_aux_bwd(const float* dxs, int64_t ld_dxs, const float* pre, int64_t ld_pre, float* d_aux,
                           int64_t ld_daux, void* ws, int64_t B, int64_t K, int64_t T, int F, int trials,
                           void* stream);
int tssep_cond_cat_aux_bwd(const float* dxs, int64_t ld_dxs, float* d_aux, int64_t ld_daux, void* ws,
                           int64_t B, int64_t K, int64_t T, int F, int E, int trials, void* stream);
/* The same gradient for FRAME-WISE embeddings (rows (b, s, ta), see tssep_cond_mul_t_fwd): bucket ta holds the frames
 * ta*stride .. min((ta+1)*stride, T) - 1 (the last bucket may be shorter; stride >= T: one bucket of all T frames)
 *   mul: d_aux[(b,s,ta), f] = sum_tr sum_{t in bucket ta} dxs[(b,tr,(s-tr) mod K,t), f] * pre[(b,t), f]
 *   cat: d_aux[(b,s,ta), e] = sum_tr sum_{t in bucket ta} dxs[(b,tr,(s-tr) mod K,t), F+e]
 * One wave per (b, s, ta, chunk of 16 frames of the bucket) adds its frames in ascending (trial, frame) order into one
 * accumulator per column; buckets of at most 16 frames are stored straight to d_aux (one launch), longer ones go
 * through the workspace and a second launch adds the chunks in ascending order.  No atomics: bit-identical from run to
 * run.  16-byte loads under the conditions of tssep_cond_*_aux_bwd.
 * ws: caller-owned, tssep_cond_aux_t_bwd_workspace_bytes(B, K, T, F, E, Ta, stride) bytes (E = 0: mul; host-only;
 * -1 = bad shape; 0 = no workspace is needed and ws may be NULL).
 * Algorithmic HBM bytes: 4 * B*trials*K*T * C (dxs columns read, C = F or E) [+ 4 * B*T*F of pre, re-read K*trials
 * times from the caches] + 4 * B*K*Ta*C. */
int64_t tssep_cond_aux_t_bwd_workspace_bytes(int64_t B, int64_t K, int64_t T, int F, int E, int64_t Ta,
                                             int64_t stride);
int tssep_cond_mul_aux_t_bwd(const float* dxs, int64_t ld_dxs, const float* pre, int64_t ld_pre, float* d_aux,
                             int64_t ld_daux, void* ws, int64_t B, int64_t K, int64_t T, int F, int trials,
                             int64_t Ta, int64_t stride, void* stream);
int tssep_cond_cat_aux_t_bwd(const float* dxs, int64_t ld_dxs, float* d_aux, int64_t ld_daux, void* ws,
                             int64_t B, int64_t K, int64_t T, int F, int E, int trials, int64_t Ta,
                             int64_t stride, void* stream);
/* InstanceNorm (mode 0, net.py:250-285: (x - mean) / std, unbiased 0 / 1) and InstanceNorm_v2 (mode 1, net.py:288-330:
 * (x - mean) / (||x - mean|| / sqrt(count))) over x [R, n, C] (rows (r,t), leading dimension ld_x).  axis 0: statistics
 * along the last axis, mean / rscale [R*n]; axis 1: along the time axis, mean / rscale [R*C].  The variance is summed
 * from centred values (the sums are accumulated in double, everything stored is fp32); no epsilon (a constant row
 * gives inf / nan as in the reference).  rscale = 1 / scale.
 * bwd: dx = rscale * (dy - mean(dy) - yhat * sum(dy * yhat) / dof), yhat = (x - mean) * rscale.
 * Algorithmic HBM bytes: fwd 8 * R*n*C, bwd 12 * R*n*C (re-reads are served by the caches). */
int tssep_instnorm_fwd(const float* x, int64_t ld_x, float* y, int64_t ld_y, float* mean, float* rscale,
                       int64_t R, int64_t n, int C, int axis, int mode, int unbiased, void* stream);
int tssep_instnorm_bwd(const float* dy, int64_t ld_dy, const float* x, int64_t ld_x, const float* mean,
                       const float* rscale, float* dx, int64_t ld_dx, int64_t R, int64_t n, int C, int axis,
                       int mode, int unbiased, void* stream);
/* ReLU of the AuxNet MLP (net.py:121-123): y = max(y, 0) in place; dx = y > 0 ? dy : 0 from the OUTPUT's sign.
 * Bytes: fwd 8 * rows*C, bwd 12 * rows*C. */
int tssep_relu_fwd(float* y, int64_t ld, int64_t rows, int C, void* stream);
int tssep_relu_bwd(const float* dy, int64_t ld_dy, const float* y, int64_t ld_y, float* dx, int64_t ld_dx,
                   int64_t rows, int C, void* stream);
/* Length-aware mean over packed rows (pad_sequence + padded_sequence_reduction 'mean', net.py:142-149):
 * out[s, :] = mean of the rows row0[s] .. row0[s+1]-1 of h [N, C]; row0: DEVICE int64 [S+1], ascending, no empty
 * segment.  relu != 0: the mean of max(h, 0) (fwd) and the mask h > 0 on the broadcast (bwd; h is the forward's input).
 * bwd: dh[row, :] = dout[s, :] / len_s.  One launch for any S.  Bytes: fwd 4 * (N + S) * C, bwd 4 * (S + N [+ N]) * C. */
int tssep_segment_mean_fwd(const float* h, int64_t ld_h, const int64_t* row0, float* out, int64_t ld_out,
                           int64_t S, int C, int relu, void* stream);
int tssep_segment_mean_bwd(const float* dout, int64_t ld_dout, const float* h, int64_t ld_h, const int64_t* row0,
                           float* dh, int64_t ld_dh, int64_t S, int C, int relu, void* stream);

/* -------------------------------------------------------------- mask head ----
 * mask = sigmoid(logit); est = Obs * mask   (tssep/train/net.py:981-986 +
 * tssep/train/enhancer.py:98-100).   logit/mask [B,K,T,F] fp32, obs [B,T,F] c64,
 * est [B,K,T,F] c64.  Algorithmic HBM bytes per (b,t): 16*K*F + 8*F. */
int tssep_maskhead_fwd(const float* logit, const float* obs, float* mask, float* est,
                       int64_t B, int64_t K, int64_t T, int F, void* stream);
/* dlogit = (Re(conj(obs) * dest) + dmask) * m * (1 - m); dmask may be NULL. */
int tssep_maskhead_bwd(const float* dest, const float* dmask, const float* mask,
                       const float* obs, float* dlogit,
                       int64_t B, int64_t K, int64_t T, int F, void* stream);
/* Gated mask head (explicit_vad, tssep/train/net.py:969-979): logit [B,K,T,F+1] with the VAD logit at column 0 ->
 * vmask [B,K,T] = g = sigmoid(v), mask [B,K,T,F] = sigmoid(l_f) g, est = Obs * mask (est may be NULL).
 * bwd: dm_f = Re(conj(obs) dest_f) + dmask_f, dlogit [B,K,T,F+1]: d(l_f) = dm_f g s_f (1 - s_f),
 * d(v) = (sum_f dm_f s_f + dvmask) g (1 - g); dest, dmask and dvmask may each be NULL. */
int tssep_maskhead_gated_fwd(const float* logit, const float* obs, float* mask, float* est, float* vmask,
                             int64_t B, int64_t K, int64_t T, int F, void* stream);
int tssep_maskhead_gated_bwd(const float* dest, const float* dmask, const float* dvmask, const float* logit,
                             const float* obs, float* dlogit, int64_t B, int64_t K, int64_t T, int F, void* stream);

/* Masking on a given mask (standalone enhancer call, tssep/train/enhancer.py:98-100):
 * est = Obs * mask, and its backward dmask = Re(conj(Obs) * dest). */
int tssep_mask_mul_fwd(const float* mask, const float* obs, float* est,
                       int64_t B, int64_t K, int64_t T, int F, void* stream);
int tssep_mask_mul_bwd(const float* dest, const float* obs, float* dmask,
                       int64_t B, int64_t K, int64_t T, int F, void* stream);

/* ------------------------------------------------------------------ losses ---
 * LogMAE (tssep/train/loss.py:244-247): loss[b] = log10(sum_k mean_n |est-tgt|).
 * Deterministic two-stage reduction; `sums[b]` (the argument of the log) is kept for bwd.
 * tssep_logmae_finalize consumes the partial sums tssep_istft_fwd can emit
 * (partial [B*K, nchunks]).  bwd: dest = gout[b] * sign(est-tgt) / (N ln10 sums[b]).
 * MAE (tssep/train/loss.py:194-216) is the same reduction without the logarithm: its value is
 * sums[b], and tssep_logmae_bwd with sums == NULL gives its gradient gout[b] * sign(est-tgt) / N. */
int64_t tssep_logmae_chunks(int64_t N);
int64_t tssep_logmae_workspace_bytes(int64_t B, int64_t K, int64_t N);
int tssep_logmae_fwd(const float* est, const float* tgt, int64_t B, int64_t K, int64_t N,
                     float* loss, float* sums, void* ws, void* stream);
int tssep_logmae_finalize(const float* partial, int64_t B, int64_t K, int64_t nchunks, int64_t N,
                          float* loss, float* sums, void* stream);
int tssep_logmae_bwd(const float* est, const float* tgt, const float* sums, const float* gout,
                     int64_t B, int64_t K, int64_t N, float* dest, void* stream);
/* Pairwise costs and the permutation-invariant assignment (pit=True of tssep/train/loss.py:194-247 through
 * pt.ops.losses.pit_loss; MSE, loss.py:183-190).  est, tgt [B,K,N], K <= 8 (TSSEP_E_SHAPE beyond).
 * tssep_pair_cost_fwd: ONE pass over est and tgt (2 B K N floats read, whatever K is) leaves the chunk partials
 *   part [B][nchunks][K][K] of sum_n |est[b,i,n] - tgt[b,j,n]|^p, p = 1 or 2, nchunks = tssep_pair_cost_chunks(N);
 *   fixed-order reduction, no atomics.  diag_only != 0: only i == j is computed (pit=False), the rest is written as 0.
 * tssep_pit_assign: cost[b,i,j] = (sum_c part[b,c,i,j]) / N (cost may be NULL), then per utterance
 *   pit != 0: perm[b] = argmin over the K! permutations of sum_i cost[b,i,perm(i)] (float32, ascending i; among equal
 *   sums the first in itertools.permutations(range(K)) order; a NaN sum wins, so it reaches the loss);
 *   pit == 0: the identity.  perm [B,K] int32 (perm[b,i] = the target row matched to estimate row i),
 *   sums[b] = the minimum, loss[b] = logarithm ? log10(sums[b]) : sums[b].  A caller-supplied cost matrix [B,K,K] is
 *   passed as part with nchunks = 1, N = 1.
 * tssep_pair_loss_bwd: dest[b,i,n] = c sign(e - t) (p = 1) or c 2 (e - t) (p = 2), t = tgt[b,perm[b,i],n] read in place
 *   (perm == NULL: identity), c = gout[b] / N, divided by ln10 sums[b] when sums != NULL (LogMAE). */
int64_t tssep_pair_cost_chunks(int64_t N);
int64_t tssep_pair_cost_workspace_bytes(int64_t B, int64_t K, int64_t N);
int tssep_pair_cost_fwd(const float* est, const float* tgt, int64_t B, int64_t K, int64_t N, int p, int diag_only,
                        float* part, void* stream);
int tssep_pit_assign(const float* part, int64_t B, int64_t K, int64_t nchunks, int64_t N, int pit, int logarithm,
                     float* cost, int32_t* perm, float* sums, float* loss, void* stream);
int tssep_pair_loss_bwd(const float* est, const float* tgt, const int32_t* perm, const float* sums, const float* gout,
                        int64_t B, int64_t K, int64_t N, int p, float* dest, void* stream);
/* FreqMSE (tssep/train/loss.py:250-269 on STFTDomain, :102-115): the squared error of two spectra,
 *   cost[b,i,j] = sum_t (1/F) sum_f |E[b,i,t,f] - S[b,j,t,f]|^2,   E, S [B,K,T,F], K <= 8, any F >= 1
 * (TSSEP_E_SHAPE for K > 8 or an empty dimension; int64 element offsets throughout).  tgt is complex64.
 * Forward: chunk partials part [B][nchunks][K][K] of sum_{t in chunk} sum_f |E_i - S_j|^2, the layout of
 *   tssep_pair_cost_fwd with the chunks over T, nchunks = tssep_specmse_chunks(T); fixed-order two-stage reduction, no
 *   atomics: two runs agree bit for bit.  diag_only != 0: only i == j is computed (pit=False), the rest is written as 0.
 *   Finished by tssep_pit_assign(part, B, K, nchunks, N = F, pit, logarithm = 0, ...): its / N is the mean over F.
 *   tssep_specmse_workspace_bytes: the bytes of part rounded up to 16; 0 for a shape the kernels refuse.
 * tssep_mask_specmse_*: E = sigmoid(logit) * obs formed on the fly (net.py:983, enhancer.py:98-100; logit [B,K,T,F]
 *   fp32, obs [B,T,F] complex64), neither mask nor estimate is written.  Backward, with t = S[b, perm[b,k]] (perm ==
 *   NULL: identity), m = sigmoid(l), d = m Y - t:
 *     dlogit = gout[b] (2/F) Re(conj(d) Y) m (1 - m);
 *   bt_major / iperm as tssep_mask_istft_bwd_loss: bt_major = 1 stores rows (b, t) x (iperm[b*K + k] (NULL: k), f), the
 *   same values bit for bit as bt_major = 0's [B,K,T,F].
 * tssep_specmse_*: an estimate in memory, complex64 (est_f64 == 0) or complex128 (est_f64 != 0).  A complex128
 *   estimate is differenced with the target in double; the forward rounds that difference to float32 before it is
 *   squared and summed (the partials are float32 either way), the backward stays in double throughout.
 *   Backward: dest = gout[b] (2/F) (E - t) in the estimate's dtype (torch's complex-gradient convention). */
int64_t tssep_specmse_chunks(int64_t T);
int64_t tssep_specmse_workspace_bytes(int64_t B, int64_t K, int64_t T, int64_t F);
int tssep_mask_specmse_fwd(const float* logit, const float* obs, const float* tgt, int64_t B, int64_t K, int64_t T,
                           int64_t F, int diag_only, float* part, void* stream);
int tssep_mask_specmse_bwd(const float* logit, const float* obs, const float* tgt, const int32_t* perm,
                           const float* gout, int64_t B, int64_t K, int64_t T, int64_t F, const int32_t* iperm,
                           int bt_major, float* dlogit, void* stream);
int tssep_specmse_fwd(const void* est, int est_f64, const float* tgt, int64_t B, int64_t K, int64_t T, int64_t F,
                      int diag_only, float* part, void* stream);
int tssep_specmse_bwd(const void* est, int est_f64, const float* tgt, const int32_t* perm, const float* gout,
                      int64_t B, int64_t K, int64_t T, int64_t F, void* dest, void* stream);
/* SDR / SI-SDR (this project's own loss; the reference has none).  est, tgt [B,K,N], K <= 8 (TSSEP_E_SHAPE beyond).
 * With a_i = sum_n e_i^2, b_j = sum_n t_j^2, c_ij = sum_n e_i t_j:
 *   scale_invariant != 0: alpha = c / (b + eps), s = alpha c, n = a - s;   else: s = b, n = a - 2 c + b;   n < 0 -> 0
 *   D = n + tau s + eps,  value[b,i,j] = 10 log10((s + eps) / D) dB,  cost = -value / K;  tau = 10^(-sdr_max / 10) or 0.
 * tssep_sdr_stats_fwd: ONE pass over est and tgt leaves the float64 chunk partials part [B][nchunks][K*K + 2K]
 *   (c_ij at i*K + j, a_i at K*K + i, b_j at K*K + K + j), nchunks = tssep_sdr_chunks(N).  Float32 only in the per-lane
 *   chain of at most 32 fused multiply-adds, float64 behind it; fixed order, no atomics: two runs agree bit for bit.
 *   diag_only != 0: only c_ii is computed (pit=False), the other c entries are written as 0.
 *   tssep_sdr_workspace_bytes: the bytes of part; 0 for a shape the kernels refuse.
 * tssep_sdr_cost: stat [B][K*K + 2K] float64 = the partials summed in chunk order (kept for the backward), value and
 *   cost [B,K,K] float32, formed in float64 and rounded once; diag_only != 0: both 0 off the diagonal.  The assignment
 *   and the loss follow from tssep_pit_assign(cost, B, K, nchunks = 1, N = 1, pit, logarithm = 0, ...).
 *   eps > 0 and tau >= 0, otherwise TSSEP_E_UNSUPPORTED.
 * tssep_sdr_bwd: dest[b,i,:] = P e_i + Q t, t = tgt[b, perm[b,i]] read in place (perm == NULL: identity), with
 *   g = gout[b] 20 / (K ln 10):  scale-invariant P = g / D, Q = -g alpha (1 / (s + eps) + (1 - tau) / D);
 *   plain P = g / D = -Q, both 0 where n was clamped.  P, Q are formed from stat in float64 and rounded once. */
int64_t tssep_sdr_chunks(int64_t N);
int64_t tssep_sdr_workspace_bytes(int64_t B, int64_t K, int64_t N);
int tssep_sdr_stats_fwd(const float* est, const float* tgt, int64_t B, int64_t K, int64_t N, int diag_only,
                        double* part, void* stream);
int tssep_sdr_cost(const double* part, int64_t B, int64_t K, int64_t nchunks, int scale_invariant, double tau,
                   double eps, int diag_only, double* stat, float* value, float* cost, void* stream);
int tssep_sdr_bwd(const float* est, const float* tgt, const int32_t* perm, const double* stat, const float* gout,
                  int64_t B, int64_t K, int64_t N, int scale_invariant, double tau, double eps, float* dest,
                  void* stream);
/* VADSigmoidBCE with target 'Vad' (tssep/train/loss.py:329-345,302-310):
 * x = mean_f logit[b,k,t,:]; loss[b] = mean_{k,t} BCEWithLogits(x, vad).
 * xmean [B,K,T] is kept for bwd; ws: tssep_vadbce_workspace_bytes.
 * bwd writes dlogit[b,k,t,f] = gout[b]*(sigmoid(x)-y)/(K*T*F). */
int64_t tssep_vadbce_workspace_bytes(int64_t B, int64_t K, int64_t T);
int tssep_vadbce_fwd(const float* logit, const float* vad, int64_t B, int64_t K, int64_t T, int F,
                     float* loss, float* xmean, void* ws, void* stream);
int tssep_vadbce_bwd(const float* xmean, const float* vad, const float* gout,
                     int64_t B, int64_t K, int64_t T, int F, float* dlogit, void* stream);
/* The VAD BCE of SignalAndVADSigmoidBCE (tssep/train/loss.py:348-395) on the gate column of an explicit_vad logit:
 * x = logit[row * ld] (rows (b,k,t), ld = F + 1), loss[b] = mean_{k,t} BCEWithLogits(x, vad) (ws: B*K*T floats;
 * the fixed-order reduction of tssep_vadbce_fwd).  bwd writes whole rows of dlogit [B*K*T, ld]:
 * gout[b] (sigmoid(x) - vad) / (K T) at column 0, zeros elsewhere. */
int tssep_gatebce_fwd(const float* logit, int64_t ld, const float* vad, int64_t B, int64_t K, int64_t T,
                      float* loss, void* ws, void* stream);
int tssep_gatebce_bwd(const float* logit, int64_t ld, const float* vad, const float* gout, int64_t B, int64_t K,
                      int64_t T, float* dlogit, void* stream);
/* The targets of the VAD losses, built on the device (tssep/train/loss.py:134-146, 312-327, 381-393; tssep/util/utils.py:11-77).
 * Frame magnitudes a [rows, T] float32, a[r,t] = sum_{f=0..F-1} |X[r,t,f]|, summed per lane (f = lane, lane + 64, ...;
 * the last bin of the fused form by lane 0), then across the wave: a fixed order, the same bits on every run.
 *   tssep_stft_framemag_fwd: the arguments of tssep_stft_fwd (both FFT plans) without the spectrum: X[r,t,f] is formed by
 *     the arithmetic of tssep_stft_fwd and never written, |X| = sqrtf(re^2 + im^2), F = size / 2 + 1.
 *   tssep_framemag_fwd: from a spectrum in memory, X [rows, T, F] complex64 (is_complex != 0) or float32 (|X| = fabsf),
 *     any F >= 1, one wave per frame.
 * tssep_vad_from_mag: vad[r,t] = (a[r,t] / max_t a[r,t] > (float)threshold) ? 1 : 0 with the IEEE float32 division and the
 *   strict comparison of `target / torch.amax(target, -1, keepdim=True) > threshold` (loss.py:319-321): the same decisions
 *   bit for bit given the same a.  A row whose maximum is 0 (an absent speaker: 0 / 0 = NaN compares false) gives zeros; a
 *   NaN in a row makes the row's maximum NaN as torch.amax does.  One workgroup walks a row twice (the maximum, then the
 *   decisions): any T >= 1, no workspace, no atomics.
 * tssep_vad_frames: the frame activity of a sample activity (utils.py:11-77 is this gather): vad_samples [rows, N] uint8,
 *   non-zero = active; Vad[r,t] = active(vad_samples[r, i]) as 1.f / 0.f, i = (t + 1) shift + window_length / 2 - lead - 1,
 *   lead = 0 / window_length - shift / (window_length - shift) / 2 for fading = 0 (none) / 1 (full) / 2 (half); 0 where i
 *   lies outside [0, N).  T: the caller's frame count (tssep_stft_frames with pad = 1). */
int tssep_stft_framemag_fwd(const float* x, int64_t rows, int64_t N, int size, int shift, int fading,
                            const float* window, const float* tw, float* a, int64_t T, void* stream);
int tssep_framemag_fwd(const float* X, int is_complex, int64_t rows, int64_t T, int64_t F, float* a, void* stream);
int tssep_vad_from_mag(const float* a, int64_t rows, int64_t T, double threshold, float* vad, void* stream);
int tssep_vad_frames(const uint8_t* vad_samples, int64_t rows, int64_t N, int window_length, int shift, int fading,
                     float* Vad, int64_t T, void* stream);

/* -------------------------------------------------------- logit layout map ---
 * Tail of MaskEstimator_v2.forward: final einops rearrange / reduce-repeat
 * (tssep/train/net.py:631-659), mean over permutation trials (net.py:928-951) and the speaker
 * un-permutation (net.py:957-967):  raw GEMM output -> out [B,K,T,F].
 *   spk_rows = 0: raw[((b*trials+tr)*T + t) * (K*Fr) + k*Fr + fr]   (ts_vad combination layer)
 *   spk_rows = 1: raw[((b*K + k)*T + t) * Fr + fr]                   (ts_vad off, trials == 1)
 *   Fr = F ('tf') or 1 ('t': the value is repeated over frequency).
 * perm[b,s] = output index of speaker s, iperm its inverse (both NULL = identity).
 * Trial mean: trials a power of two: the fp32 sum in trial order, * (1/trials); any other count: sum and division in
 * double, rounded once -- |error| <= (trials - 1) * 2^-24 * mean|raw| either way. */
int tssep_logit_map_fwd(const float* raw, const int32_t* perm, const int32_t* iperm, int64_t B,
                        int trials, int64_t K, int64_t T, int F, int Fr, int spk_rows,
                        float* out, void* stream);
int tssep_logit_map_bwd(const float* dout, const int32_t* perm, const int32_t* iperm, int64_t B,
                        int trials, int64_t K, int64_t T, int F, int Fr, int spk_rows,
                        float* draw, void* stream);

/* Fused two-mask tail (nmask = M masks per speaker, tssep/train/net.py:629-659 with '(spk mask freq)' columns, the
 * trial mean :928-951, the un-permutation :957-967 and the sigmoid :983): one pass each way between the final
 * Linear's GEMM and the enhancer.  Any M >= 1.
 *   spk_rows = 0: raw[((b*trials+tr)*T + t) * (K*M*Fr) + (k*M + m)*Fr + fr]
 *   spk_rows = 1: raw[((b*K + k)*T + t) * (M*Fr) + m*Fr + fr]                 (trials == 1)
 *   logit, mask [B,K,M,T,F] fp32: index (((b*K + j)*M + m)*T + t)*F + f;  Fr = F ('tf') or 1 ('t').
 * fwd: logit with tssep_logit_map_fwd's arithmetic (the same device function: bit-identical at M = 1),
 *      mask = the mask head's sigmoid of it.  Bytes: 4 * (trials * B*K*M*T*Fr + 2 * B*K*M*T*F).
 * bwd: draw (raw layout) = (dmask * s * (1 - s) [+ dlogit]) [* 1/trials], every operation rounded on its own; 't': the
 *      sum over f in tssep_logit_map_bwd's lane order.  dlogit may be NULL.  Bytes: 4 * ((2 | 3) * B*K*M*T*F +
 *      trials * B*K*M*T*Fr).  Argument checks as tssep_logit_map_*, and TSSEP_E_SHAPE for M <= 0. */
int tssep_mask_map_fwd(const float* raw, const int32_t* perm, const int32_t* iperm, int64_t B,
                       int trials, int64_t K, int M, int64_t T, int F, int Fr, int spk_rows,
                       float* logit, float* mask, void* stream);
int tssep_mask_map_bwd(const float* dmask, const float* mask, const float* dlogit,
                       const int32_t* perm, const int32_t* iperm, int64_t B, int trials, int64_t K,
                       int M, int64_t T, int F, int Fr, int spk_rows, float* draw, void* stream);

/* ------------------------------------------------- mask-based MVDR beamformer ----
 * Eval-time enhancer TorchBF('mvdr_souden') of the reference, tssep/train/enhancer.py:140-265, in
 * complex128 as there (the reference asserts Observation.dtype == complex128, :224):
 *   psd_m[k,f]  = sum_t w_m[k,t,f] Y[:,t,f] Y[:,t,f]^H     w_0 = mask 0 (target),
 *                                                          w_1 = mask 1, or 1 - mask 0 when M == 1
 *   phi         = psd_1^-1 psd_0     (LU, partial pivoting = torch.linalg.solve / zgesv)
 *   bf[k,f,:]   = phi[:, reference_channel] / max(Re trace(phi), eps)
 *   enh[k,t,f]  = sum_d conj(bf[k,f,d]) Y[d,t,f]     (* max(mask 0, masking_eps) if masking)
 * obs  [B,D,T,F] complex128 (interleaved re,im doubles), D <= 8
 * masks [B,K,M,T,F] fp32 (mask_f64 = 0) or fp64 (mask_f64 = 1), M in {1,2}
 * enh  [B,K,T,F] complex128.      eps: pass DBL_MIN for the reference's eps=None.
 * info[0] (device int) receives the number of (b,k,f) systems with an exactly zero pivot
 * (torch.linalg.solve raises for those; the host mirror does the same).
 * Algorithmic HBM bytes: 2 * 16*D*T*F (Y for the statistics, Y again for the filtering)
 *   + K*M*T*F*sizeof(mask) + 16*K*T*F, per batch element.
 * The three stages are exported for tests and profiling; _souden_fwd runs them back to back on
 * `stream` out of one caller-owned workspace of tssep_mvdr_workspace_bytes().  No host sync. */
int64_t tssep_mvdr_partial_bytes(int64_t B, int K, int D, int64_t T, int F);
int64_t tssep_mvdr_workspace_bytes(int64_t B, int K, int D, int64_t T, int F);
int tssep_mvdr_psd(const double* obs, const void* masks, int mask_f64, double* partials,
                   int64_t B, int K, int M, int D, int64_t T, int F, void* stream);
/* wconj [B,K,D,F] complex128 = conj(bf), bin-contiguous.  Consumes `partials` (the chunk sums are
 * formed in place).  masking_eps is compared in double: a caller that holds fp32 masks passes the
 * fp32-rounded value to reproduce torch.clamp(mask_fp32, min=masking_eps) bit for bit. */
int tssep_mvdr_weights(double* partials, double* wconj, int* info, int64_t B, int K, int D,
                       int64_t T, int F, int reference_channel, double eps, void* stream);
int tssep_mvdr_apply(const double* obs, const double* wconj, const void* masks, int mask_f64,
                     double* enh, int64_t B, int K, int M, int D, int64_t T, int F, int masking,
                     double masking_eps, void* stream);
int tssep_mvdr_souden_fwd(const double* obs, const void* masks, int mask_f64, double* enh,
                          void* workspace, int* info, int64_t B, int K, int M, int D, int64_t T,
                          int F, int reference_channel, double eps, int masking,
                          double masking_eps, void* stream);

/* Backward of tssep_mvdr_souden_fwd: dmask [B,K,M,T,F] (the masks' dtype) = d(loss)/d(masks) for
 * genh [B,K,T,F] complex128 = d(loss)/d(enh) in torch's convention for complex tensors; the observation gets no
 * gradient.  With P = phi, lam = Re trace(P), c = max(lam, eps), g = max(mask 0, masking_eps) (masking) or 1:
 *   gw   = sum_t conj(genh g) Y[:,t]                  gP = (gw / c) e_ref^T + gc I,
 *   gc   = -Re(gw^H P[:, ref]) / c^2 where lam >= eps, else 0 (the clamp passes the gradient at equality)
 *   Z    = psd_1^-H gP       Hs = herm(Z)       Hn = herm(-Z P^H)
 *   dmask[:,:,0] = Re(y^H Hs y) (+ Re(conj(enh / g) genh) where mask 0 >= masking_eps, with masking)
 *   dmask[:,:,1] = Re(y^H Hn y)           (M == 1: dmask[:,:,0] uses Hs - Hn instead of Hs)
 * fwd_workspace: the workspace tssep_mvdr_souden_fwd left behind for the same arguments (the reduced statistics in
 * chunk 0 of its partials, then wconj); phi is recomputed from it with the forward's own elimination.
 * bwd_workspace (16-byte aligned, tssep_mvdr_bwd_workspace_bytes(); host-only, 0 for an unsupported shape):
 *   gw_partials doubles [B][chunks][K][2*D][F] (rows Re gw_d, Im gw_d; the chunks of the forward's statistics pass;
 *   _bwd_solve adds them into chunk 0), rounded up to 16 bytes, then
 *   herm        doubles [B][K][M][D*D][F], packed Hermitian like the statistics: rows 0..D-1 the diagonal, then for
 *   every pair i < j in row-major order the rows Re H[i,j], Im H[i,j];  M == 2: Hs, Hn;  M == 1: Hs - Hn.
 * masks, genh and wconj may be NULL without masking.  No atomics: every result is identical from run to run; every
 * element of dmask is written exactly once.  No host sync. */
int64_t tssep_mvdr_bwd_workspace_bytes(int64_t B, int K, int M, int D, int64_t T, int F);
int tssep_mvdr_bwd_gw(const double* obs, const double* genh, const void* masks, int mask_f64,
                      double* gw_partials, int64_t B, int K, int M, int D, int64_t T, int F, int masking,
                      double masking_eps, void* stream);
int tssep_mvdr_bwd_solve(const double* fwd_partials, double* gw_partials, double* herm, int64_t B, int K,
                         int M, int D, int64_t T, int F, int reference_channel, double eps, void* stream);
int tssep_mvdr_bwd_mask(const double* obs, const double* genh, const double* wconj, const double* herm,
                        const void* masks, int mask_f64, void* dmask, int64_t B, int K, int M, int D,
                        int64_t T, int F, int masking, double masking_eps, void* stream);
int tssep_mvdr_souden_bwd(const double* obs, const void* masks, int mask_f64, const double* genh,
                          const void* fwd_workspace, void* bwd_workspace, void* dmask, int64_t B, int K,
                          int M, int D, int64_t T, int F, int reference_channel, double eps, int masking,
                          double masking_eps, void* stream);

/* Online (frame-recursive) MVDR -- this project's own, the reference has no online mode.  Per batch
 * element b, speaker k and bin f, for the T frames of the call in order, one mask per speaker:
 *   Phi_s = forgetting Phi_s + m y y^H          Phi_n = forgetting Phi_n + (1 - m) y y^H
 *   phi   = solve(Phi_n + diag_load Re tr(Phi_s + Phi_n) / D I, Phi_s)       (the elimination of tssep_mvdr_weights)
 *   enh   = (phi[:, reference_channel] / max(Re tr phi, eps))^H y            (* max(m, masking_eps) if masking)
 * The filter of a frame uses the statistics up to and including that frame.  While the trace is exactly zero the
 * output is zero; a singular loaded Phi_n (diag_load = 0 in front of frame D - 1) leaves Inf / NaN in that frame's
 * output element only.  forgetting in (0, 1], diag_load >= 0 (else TSSEP_E_SHAPE).
 * obs   [B,D,T,F] complex128 (obs_f64 = 1, 16-byte aligned) or complex64 (obs_f64 = 0, 8-byte aligned), D <= 8
 * masks [B,K,T,F] fp32 (mask_f64 = 0) or fp64;      enh [B,K,T,F] complex128
 * state doubles [B][K][2: Phi_s, Phi_n][D*D][F], packed Hermitian like the statistics (rows 0..D-1 the diagonal, then
 *   for every pair i < j in row-major order the rows Re, Im): tssep_mvdr_online_state_bytes() bytes (host-only, 0 for
 *   an unsupported shape).  state_in NULL: a fresh stream (zeros); state_in == state_out is allowed.
 * One launch, one step per frame in a fixed order: output and state do not depend on how a stream's frames are split
 * over calls.  Algorithmic HBM bytes: T*F*(8|16)*D (Y; once per speaker out of L2) + K*T*F*(sizeof(mask) + 16)
 * + 2 * 16*K*D*D*F (the state in and out), per batch element.  No workspace, no atomics, no host sync. */
int64_t tssep_mvdr_online_state_bytes(int64_t B, int K, int D, int F);
int tssep_mvdr_online_fwd(const void* obs, int obs_f64, const void* masks, int mask_f64,
                          const double* state_in, double* state_out, double* enh, int64_t B, int K, int D,
                          int64_t T, int F, int reference_channel, double forgetting, double diag_load,
                          double eps, int masking, double masking_eps, void* stream);

/* Segment-wise MVDR: ClassicBF_np('mvdr_souden') of the reference with segment_bf=True,
 * tssep/train/enhancer.py:451-590, one beamformer per row (k, s, e) of a segment table:
 *   n_k         = max(sum_{j != k} m_j, distortion_eps)   mode 0, SumCrossTalker (ascending j,
 *                                                          in the mask's dtype)
 *               = max(1 - m_k, 0)                          mode 1, OneMinus (K == 1 only)
 *   psd_0|1     = sum_{t in [s,e)} (m_k | n_k)**mask_power Y[:,t,f] Y[:,t,f]^H / (e - s)
 *                 psd_real != 0: only the real part is kept -- what _get_psd's
 *                 (psd + swapaxes(psd, -2, -1)) / 2 (:288) does; 0: the Hermitian matrix
 *   bf          = phi[:, 0] / max(Re trace(phi), eps),  phi = psd_1^-1 psd_0   (as above)
 *   enh[k,t,f]  = sum_d conj(bf_d) Y[d,t,f]  (* max(m_k, masking_eps) if masking),  t in [s,e)
 *               = 0 at every (k, t) that no row of the table covers (written by the kernel).
 * obs [D,T,F] complex128, D <= 8;  masks [K,1,T,F] fp32 | fp64;  enh [K,T,F] complex128
 * segments [S,3] int32 on the device; the intervals of one speaker are disjoint (the host mirror
 *   checks it); a row with k outside [0,K) or an empty interval is ignored.
 * distortion_eps and masking_eps are compared in the mask's dtype (rounded to fp32 for fp32 masks).
 * info [S] device ints: the number of bins of segment i whose system had an exactly zero pivot.
 * A constant number of launches whatever S is, no host sync; workspace (16-byte aligned):
 * tssep_mvdr_segments_workspace_bytes(), host-only, 0 for an unsupported shape (D > 8 ...).
 * _segments_psd runs the statistics stage alone and leaves both PSDs at the start of the
 * workspace as doubles [S][2: target, distortion][D*D][F]: element rows 0..D-1 the diagonal, then
 * for every pair i < j in row-major order the rows Re psd[i,j], Im psd[i,j]. */
int64_t tssep_mvdr_segments_workspace_bytes(int K, int S, int D, int64_t T, int F);
int tssep_mvdr_segments_psd(const double* obs, const void* masks, int mask_f64,
                            const int32_t* segments, void* workspace, int K, int S, int D,
                            int64_t T, int F, int mode, double distortion_eps, double mask_power,
                            int psd_real, void* stream);
int tssep_mvdr_segments_fwd(const double* obs, const void* masks, int mask_f64,
                            const int32_t* segments, double* enh, void* workspace, int* info, int K,
                            int S, int D, int64_t T, int F, int mode, double distortion_eps,
                            double mask_power, int psd_real, double eps, int masking,
                            double masking_eps, void* stream);

/* The same on a packed per-row observation, as tssep_wpe_fwd leaves it: obs_seg [D,N,F] complex128, frame t of
 * row i at packed row row0[i] + t - s_i (row0: int64 [S+1] on the device, the prefix of the row lengths).  Masks,
 * table, output, workspace and info as above; the statistics and the filtering of a row read its own packed
 * frames, so every row may carry a differently dereverberated observation. */
int tssep_mvdr_segments_fwd_obs(const double* obs_seg, const int64_t* row0, int64_t N, const void* masks,
                                int mask_f64, const int32_t* segments, double* enh, void* workspace,
                                int* info, int K, int S, int D, int64_t T, int F, int mode,
                                double distortion_eps, double mask_power, int psd_real, double eps,
                                int masking, double masking_eps, void* stream);

/* ------------------------------------------- masks -> segment table (discretisation) ----
 * The step between an estimated mask and the segment-wise beamformer above (the "threshold, then closing by dilation
 * and erosion" of the TS-VAD / TS-SEP papers); the semantics are this project's own, DESIGN 4.13:
 *   a[k,t]  = fl32(sum_f masks[k,0,t,f]) / fl32(F)       tssep_mask_activity: masks [K,M,T,F] fp32, mask index 0 read by
 *             stride (M = 2: index 1 is never touched), activity [K,T] fp32.  The sum is fp32 in an order that depends
 *             on F and on the row's address modulo 16 only (two calls give the same bits), the division one correctly
 *             rounded fp32 division.  One pass, K*T*F*4 bytes read, no atomics.
 *   b[k,t]  = a[k,t] > threshold                         strict, in fp32; a NaN is inactive
 *   closing = binary dilation with the odd window `dilation`, then binary erosion with the odd window `erosion`, both
 *             clipped to [0,T): frames outside the row count as inactive for the dilation and as active for the erosion
 *             (a run that reaches the first or the last frame is not eroded from that side).  Window 1 = identity; a
 *             window larger than 2 T is legal.
 *   runs    = the maximal runs [s,e) of ones per row; those with e - s < min_frames are dropped
 *   table   int32 rows (k, s, e), sorted by k then s, 0 <= s < e <= T, count[0] rows of them: the form
 *           tssep_mvdr_segments_fwd takes.  table holds tssep_segments_capacity(K, T) = K * ceil(T / 2) rows (a row of
 *           T frames cannot hold more runs: no overflow case); rows past count[0] are not written.
 * tssep_segments_capacity is host-only (no launch): 0 for a shape the kernels refuse (K < 1, T < 1, T > 2^30 or
 * K * ceil(T / 2) > 2^30).
 * workspace: 4 * (9 * capacity + 16) bytes, 8-byte aligned.  A fixed number of launches (nine) whatever T, the content
 * or the number of runs; the order of the table comes from prefix sums, never from atomics: the same table on every
 * call.  No host sync.  TSSEP_E_SHAPE before any launch for K, T, F or M < 1, an even or non-positive window,
 * min_frames < 1. */
int64_t tssep_segments_capacity(int64_t K, int64_t T);
int tssep_mask_activity(const float* masks, int64_t K, int M, int64_t T, int F, float* activity, void* stream);
int tssep_activity_segments(const float* activity, int64_t K, int64_t T, float threshold, int64_t dilation,
                            int64_t erosion, int64_t min_frames, int32_t* table, int32_t* count, void* workspace,
                            void* stream);

/* ------------------------------------------------------- WPE dereverberation ----
 * WPE / ChannelWiseWPE of the reference (tssep/train/enhancer.py:292-367; nara_wpe's wpe_v8 on the host
 * there), complex128.  Per frequency bin, K = taps * D:
 *   Yt[tau*D + d, t] = Y[d, t - delay - tau], zero where that frame lies in front of the row's first frame
 *   X = Y;  `iterations` times:
 *     p[t] = mean_d |X[d,t]|^2    eps = 1e-10 max_t p[t] (per row and bin)    li[t] = 1 / max(p[t], eps)
 *     R = sum_t li[t] Yt[:,t] Yt[:,t]^H    P = sum_t li[t] Yt[:,t] Y[:,t]^H
 *         t over the row's frames (valid_mode = 0, 'full') or those with t - s >= delay + taps - 1 (1, 'valid')
 *     R G = P    (Cholesky; R is Hermitian positive definite for a row of at least K + delay frames of
 *                 generic data)                      X = Y - G^H Yt  at all frames of the row
 * obs      [D,T,F] complex128 (interleaved re,im doubles), bin-contiguous
 * segments [S,2] int32 on the device, rows (s, e) clamped to [0,T]; rows may overlap or repeat
 * row0     [S+1] int64 on the device, the prefix of the row lengths e - s; N = row0[S]
 * obs_seg  [D,N,F] complex128: row i occupies packed rows row0[i] .. row0[i+1].  A row is computed as if its
 *          slice were the whole array (the taps never reach in front of s), in a summation order that depends on
 *          its length only: the packed output of a row is bit-identical whatever else the table holds.
 * lam      [N,F] doubles, the li above;   R [S,F,K,K] complex128, stored FULL (both triangles, exactly real
 *          diagonal);   P [S,F,K,D];   G [S,K,D,F] (bin-contiguous)
 * info     [S] device ints: the number of bins of row i whose factorisation met a pivot that is not positive or
 *          not finite.  tssep_wpe_solve writes the slot; tssep_wpe_fwd writes the count over all iterations.
 * Limits: D 1..8, taps >= 1, taps * D <= 80, 0 <= delay <= 256, iterations >= 1.
 * A fixed number of launches per iteration whatever S is, no host sync, everything on `stream` out of one
 * caller-owned workspace (16-byte aligned) of tssep_wpe_workspace_bytes(): host-only, 0 for an unsupported
 * shape.  The stages are exported for tests and profiling; each may be called alone with the same workspace.
 * _power: x_seg NULL reads X = Y from obs through the table, else the packed [D,N,F] estimate. */
int64_t tssep_wpe_workspace_bytes(int S, int64_t N, int D, int64_t T, int F, int taps, int delay);
int tssep_wpe_power(const double* obs, const double* x_seg, const int32_t* segments, const int64_t* row0,
                    double* lam, void* workspace, int S, int64_t N, int D, int64_t T, int F, void* stream);
int tssep_wpe_correlations(const double* obs, const double* lam, const int32_t* segments,
                           const int64_t* row0, double* R, double* P, void* workspace, int S, int64_t N,
                           int D, int64_t T, int F, int taps, int delay, int valid_mode, void* stream);
int tssep_wpe_solve(const double* R, const double* P, double* G, int* info, int S, int D, int F, int taps,
                    void* stream);
int tssep_wpe_filter(const double* obs, const double* G, const int32_t* segments, const int64_t* row0,
                     double* obs_seg, void* workspace, int S, int64_t N, int D, int64_t T, int F, int taps,
                     int delay, void* stream);
int tssep_wpe_fwd(const double* obs, const int32_t* segments, const int64_t* row0, double* obs_seg,
                  void* workspace, int* info, int S, int64_t N, int D, int64_t T, int F, int taps, int delay,
                  int iterations, int valid_mode, void* stream);

/* Online WPE -- the recursive least squares form, this project's own (the reference has no online mode).
 * Per batch element b and bin f, for the T frames of the call in order, K = taps * D, Yt as above with zeros in front of
 * the stream's first frame, a = forgetting, c = power_context:
 *   p    = sum_{s=t-c..t} sum_d |y_s[d]|^2 / (D (c + 1))         pmax = max(pmax, p) over the finite p
 *   pmax == 0: x = y, nothing is updated.                        lam = max(p, 1e-10 pmax)
 *   x    = y - G^H Yt   (the output: G of the frames before t)   u = Q Yt     den = a lam + Re(Yt^H u)
 *   not (0 < den < inf): info[b] += 1, nothing is updated.       k = u / den
 *   Q    = (Q - k u^H) / a    (one triangle computed and mirrored, real diagonal; Q_0 = I / load)      G = G + k x^H
 * obs  [B,D,T,F] complex128 (obs_f64 = 1, 16-byte aligned) or complex64 (0, 8-byte aligned);  out [B,D,T,F] complex128
 * The state, five buffers, each with a successor (x_in == x_out is allowed; all *_in NULL: a fresh stream):
 *   q    [B,F,K(K+1)/2] complex128, the lower triangle row by row ((i, j), j <= i, at i(i+1)/2 + j); zeros while pmax == 0
 *   g    [B,F,K,D] complex128       ring [B,F,R,D] complex128, the last R = max(delay + taps - 1, c) frames, oldest first
 *        (R = 0: no buffer, NULL is fine)       pmax [B,F] doubles       info [B] ints, counted on over the stream
 * A state of zeros is a fresh stream, and a stream that has seen only silence leaves zeros.
 * Limits: D 1..8, taps >= 1, taps * D <= 80, 0 <= delay <= 256, 0 <= power_context <= 256 (TSSEP_E_UNSUPPORTED beyond);
 * forgetting in (0, 1], load > 0 (else TSSEP_E_SHAPE).  One kernel launch, one workgroup per (b, f) with Q, G and the
 * ring in LDS (up to 157 KiB) across the frames of the call; every sum runs in an order fixed by (D, taps, delay, c):
 * output and state do not depend on how a stream's frames are split over calls.  No workspace, no host sync; the only
 * atomic is the integer count into info.  tssep_wpe_online_state_bytes: the bytes of the five buffers together,
 * host-only, 0 for an unsupported shape. */
int64_t tssep_wpe_online_state_bytes(int64_t B, int D, int F, int taps, int delay, int power_context);
int tssep_wpe_online_fwd(const void* obs, int obs_f64, const double* q_in, const double* g_in, const double* ring_in,
                         const double* pmax_in, const int* info_in, double* q_out, double* g_out, double* ring_out,
                         double* pmax_out, int* info_out, double* out, int64_t B, int D, int64_t T, int F, int taps,
                         int delay, int power_context, double forgetting, double load, void* stream);

/* -------------------------------------------------------------- optimizer -----
 * One optimizer step on flat fp32 buffers: global-norm gradient clipping
 * (torch.nn.utils.clip_grad_norm_, max_norm <= 0 disables) + Adam (torch.optim.Adam update rule,
 * amsgrad off) -- the reference's trainer settings (tssep/train/experiment.py:147-150).  No host
 * synchronisation; norm_out[0] (optional) receives the pre-clip gradient norm.
 * step = 1-based update count; ws: tssep_adam_workspace_bytes(). */
int64_t tssep_adam_workspace_bytes(void);
int tssep_adam_step(float* param, float* exp_avg, float* exp_avg_sq, const float* grad, int64_t n,
                    int64_t step, float max_norm, float lr, float beta1, float beta2, float eps,
                    float weight_decay, float* norm_out, void* ws, void* stream);
/* The same step behind a device-side guard: err = the error flag of the W-stationary recurrences (err[0] != 0: a launch
 * of this step gave up on a peer, the gradient is garbage) -> the update is skipped on the device, parameters and
 * moments stay those of the last good step; the host raises at its next check of the flag.  err == NULL: no guard. */
int tssep_adam_step_guarded(float* param, float* exp_avg, float* exp_avg_sq, const float* grad, int64_t n,
                            int64_t step, float max_norm, float lr, float beta1, float beta2, float eps,
                            float weight_decay, float* norm_out, void* ws, const int* err, void* stream);

/* split-K / slab reduction: dst[i] (+)= sum_{s<nsplit} src[s*stride + i] */
int tssep_reduce_splits(const float* src, int nsplit, int64_t stride, int64_t count, float* dst,
                        int accumulate, void* stream);
/* the same for the partials [nsplit][M][ldp] of a weight-gradient GEMM with b_ones_col (tssep_gemm_f32):
 * columns [0,N) -> dw [M, ld_w], column N (the column sums of dY = the bias gradient of an nn.Linear,
 * tssep/train/rnnp.py:96,161, net.py:663-666) -> db [M] */
int tssep_reduce_splits_bias(const float* src, int nsplit, int64_t stride, int64_t M, int64_t N,
                             int64_t ldp, float* dw, int64_t ld_w, float* db, int accumulate,
                             void* stream);

/* ------------------------------------------------------------------ online ---
 * A live signal in pushes: causal feature statistics and state-carrying STFT / inverse STFT (this project's own; the
 * reference has no online path).  The caller owns every state buffer; a state's successor is ANOTHER buffer (the caller
 * ping-pongs two): one that overlaps its predecessor is TSSEP_E_SHAPE.  A fixed number of launches whatever the chunk
 * length, no allocation, no host sync.  The stream kernels are built for FFT plan 1 (size 1024, shift 256, full fading, a
 * full-size window); any other plan: TSSEP_E_UNSUPPORTED.
 *
 * tssep_feat_causal_fwd: tssep_feat_fwd with the statistics over the frames t' <= t of the utterance (the current frame
 *   included) instead of the whole utterance / batch:
 *     norm[b,t]  = max_{t' <= t, f} |X[b,t',f]|,            log1p(|X| (e - 1) / norm[b,t]);  norm == 0 (silence so far): 0
 *     floor[b,t] = max_{t' <= t, m} dB[b,t',m] - top_db,    PER UTTERANCE, never over the batch (top_db < 0: log_mels, no floor)
 *   X is a chunk of T frames per utterance; state_in / state_out [B, 2] = {running max |X|, running max dB} in front of /
 *   behind the chunk (state_in NULL: {0, -inf}, a fresh stream; state_out NULL: not written).  max is exact: any split of
 *   an utterance into calls gives the bits of one call.  The frame's own arithmetic is tssep_feat_fwd's: frame t equals
 *   tssep_feat_fwd(stat_axis 0) of X[:, :t+1] at t.  Four launches (init, pass 1, scan, pass 2).
 *   ws: tssep_feat_causal_workspace_bytes(B, T, n_mels, F) bytes, 16-byte aligned.
 * tssep_stft_stream_fwd: the Tc frames a push of n_new = Tc * shift samples completes, read from [tail_in | x_new]
 *   (tail_in [rows, size - shift]: the samples in front of the push; NULL: zeros = the leading fade of a fresh stream),
 *   X [rows, Tc, size/2+1] with the bits tssep_stft_fwd gives those frames; tail_out = the last size - shift samples of
 *   [tail_in | x_new].  The trailing fade is a push of zeros by the caller.  Two launches.
 *   n_new != Tc * shift or Tc < 1: TSSEP_E_SHAPE.  x_new, tail_*, X 8-byte aligned.
 * tssep_istft_stream_fwd (X [rows, Tc, F] complex64) / tssep_mask_istft_stream_fwd (logit [B*K, Tc, F] or, gated != 0,
 *   [B*K, Tc, F + 1] with the VAD logit at column 0; obs [B, Tc, F] complex64): the hops the stream's next Tc frames
 *   complete.  A hop sums four frames oldest first; ola_in / ola_out [rows, 3, shift] hold the oldest-first partial sums
 *   of the three hops pending in front of / behind the call (ola_in NULL: zeros), added FIRST, so the concatenated
 *   output equals tssep_istft_fwd / tssep_mask_istft_fwd / tssep_mask_istft_gated_fwd of all frames bit for bit (a -0
 *   may come out as +0).  skip in 0..3: the call's first `skip` hops lie before the utterance's first sample and are not
 *   stored -- max(0, 3 - frames of the earlier calls): 3 for the first call.  y [rows, N], N = max(Tc - skip, 0) * shift;
 *   last != 0: the final hop may end early, (hops - 1) * shift < N <= hops * shift (the utterance's length); anything else
 *   TSSEP_E_SHAPE.  y may be NULL when N == 0.  One launch, Tc beyond one workgroup's 64 hops included. */
int64_t tssep_feat_causal_workspace_bytes(int64_t B, int64_t T, int n_mels, int F);
int tssep_feat_causal_fwd(const float* X, int64_t B, int64_t T, int F, const float* fb, const float* dct,
                          int n_mels, int n_mfcc, float top_db, const float* state_in, float* state_out,
                          float* out, int64_t ld_out, void* ws, void* stream);
int tssep_stft_stream_fwd(const float* x_new, int64_t rows, int64_t n_new, const float* tail_in, float* tail_out,
                          int size, int shift, const float* window, const float* tw, float* X, int64_t Tc,
                          void* stream);
int tssep_istft_stream_fwd(const float* X, int64_t rows, int64_t Tc, int size, int shift, const float* wsyn,
                           const float* tw, const float* ola_in, float* ola_out, int skip, int last, float* y,
                           int64_t N, void* stream);
int tssep_mask_istft_stream_fwd(const float* logit, int gated, const float* obs, int64_t B, int64_t K, int64_t Tc,
                                int size, int shift, const float* wsyn, const float* tw, const float* ola_in,
                                float* ola_out, int skip, int last, float* y, int64_t N, void* stream);

/* ---- training on a stream: the adjoints of the two streaming tails ----
 * tssep_istft_stream_bwd / tssep_mask_istft_stream_bwd: the backward of one call of tssep_istft_stream_fwd /
 *   tssep_mask_istft_stream_fwd with the same Tc, skip, last and N.  dy [rows, N]: the gradient of the samples the call
 *   completed (may be NULL when N == 0); d_ola_out [rows, 3, shift]: the gradient of the carry behind the call (NULL:
 *   zeros -- nobody differentiates it: the stream is truncated here).  With the gradient signal g of Tc + 3 hops,
 *     Tc <= h: d_ola_out[h - Tc] (FIRST: it holds whatever skip is -- with skip > Tc the hops Tc .. skip - 1 are pending
 *     hops the call's frames added to);   h < min(skip, Tc): 0;   skip <= h < Tc: dy[(h - skip) shift ...], 0 from N on,
 *   call-frame i gets the adjoint of the inverse STFT of g[i shift .. i shift + size): dX [rows, Tc, F] complex64 with the
 *   per-frame arithmetic of tssep_istft_bwd, or dlogit (the shape of logit) with that of tssep_mask_istft_bwd /
 *   tssep_mask_istft_gated_bwd (tgt = vad = NULL, bt_major = 0); d_ola_in [rows, 3, shift] = hops 0, 1, 2 of g, the
 *   gradient of the carry in front (NULL: not wanted).  Run the calls of a stream last first and hand each d_ola_in on as
 *   the earlier call's d_ola_out: the concatenated dX / dlogit equal tssep_istft_bwd / tssep_mask_istft_bwd /
 *   tssep_mask_istft_gated_bwd of all frames on the concatenated dy bit for bit (a -0 may come out as +0).
 *   Guards as the forward's: any plan but 1024 / 256: TSSEP_E_UNSUPPORTED; skip / last / N that no forward call takes,
 *   Tc < 1 or Tc > 2^20, d_ola_in overlapping d_ola_out: TSSEP_E_SHAPE.  dy, d_ola_in 4-byte, d_ola_out 8-byte aligned.
 *   One launch, and one small copy launch when d_ola_in is wanted; no atomics. */
int tssep_istft_stream_bwd(const float* dy, const float* d_ola_out, int64_t rows, int64_t Tc, int size, int shift,
                           const float* wsyn, const float* tw, int skip, int last, int64_t N, float* dX,
                           float* d_ola_in, void* stream);
int tssep_mask_istft_stream_bwd(const float* dy, const float* d_ola_out, const float* logit, int gated,
                                const float* obs, int64_t B, int64_t K, int64_t Tc, int size, int shift,
                                const float* wsyn, const float* tw, int skip, int last, int64_t N, float* dlogit,
                                float* d_ola_in, void* stream);

/* ---- guided source separation: a cACGMM with the activities as hard priors ----
 * This project's own definition (the reference has no GSS).  obs [D,T,F] complex128, activity uint8 [K,T] with
 * entries 0 / 1, 1 <= D <= 8, 1 <= K <= 8; classes c = 0..K, class K is noise and active in every frame.  blocks
 * int32 [P,4] on the device, rows (s_fit, e_fit, s_out, e_out) with s_fit <= s_out < e_out <= e_fit; every (block, bin)
 * is one problem fitted on [s_fit, e_fit) whose posteriors are written for [s_out, e_out).  Per problem:
 *   nrm_t = sqrt(sum_d |y_t[d]|^2), ok_t = nrm_t finite and > 0, yh_t = y_t / nrm_t; a frame that is not ok takes part
 *   in no sum and gets gamma = 0.  Start: gamma_tc = a_tc / sum_c' a_c't, q_tc = 1.  `iterations` times:
 *     n_c = sum_t gamma_tc (n_c == 0: the class is empty in this problem, log p = -inf)
 *     B_c = (D / n_c) sum_t (gamma_tc / q_tc) yh_t yh_t^H;  B_c = B_c D / Re tr B_c + load I
 *     L_c = chol(B_c), ld_c = 2 sum_i log L_c[i,i], q_tc = max(|L_c^-1 yh_t|^2, DBL_MIN)
 *     log p_tc = log pi_c - ld_c - D log q_tc where a_tc = 1, else -inf;  pi_c = n_c / sum n (uniform_weights: 1)
 *     gamma_tc = softmax_c(log p_tc)
 * out [K+1,T,F] float32 (out_f64 = 0: the rounding of the float64 value) or float64.  The block table is built and
 * checked by the host caller (the out ranges tile [0,T)); the kernels clamp every row to [0,T] and the fit range to
 * max_fit frames (the host's maximum of e_fit - s_fit), so no access leaves the buffers whatever the table holds.
 * All arithmetic float64; every sum over frames has one owner thread and an order fixed by the shape: no atomics,
 * two calls give the same bits.  2 * iterations + 2 launches whatever P, T and the content; no host sync.
 * workspace: tssep_gss_workspace_bytes() bytes (host only; 0 for an unsupported shape), 16-byte aligned.
 * TSSEP_E_UNSUPPORTED for D or K outside 1..8, TSSEP_E_SHAPE for load <= 0 (or not finite), iterations < 1, P, T, F
 * or max_fit < 1, P > 65535 -- before any launch.
 *
 * tssep_segments_to_activity: the segment table int32 [S,3] of rows (k, s, e) -> activity uint8 [K,T], 1 inside the
 * rows.  A row with k outside [0,K), s < 0, e > T or s >= e is ignored (as tssep_mvdr_segments_fwd ignores it).
 * S = 0 is legal (all zeros; table may be NULL then).  Two launches, no host sync. */
int64_t tssep_gss_workspace_bytes(int P, int D, int K, int64_t T, int F, int64_t max_fit);
int tssep_gss_fit(const double* obs, const uint8_t* activity, const int32_t* blocks, void* out, int out_f64,
                  void* workspace, int P, int D, int K, int64_t T, int F, int64_t max_fit, int iterations,
                  double load, int uniform_weights, void* stream);
int tssep_segments_to_activity(const int32_t* table, int64_t S, int K, int64_t T, uint8_t* activity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TSSEP_HIP_H */
