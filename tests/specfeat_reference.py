"""Float64 definitions of the spectral features of csrc/specfeat.hip and the per-element bounds their float32 kernels are
held to (tests/test_specfeat_reference.py without a device, tests/test_gpu_specfeat_kernels.py and
tests/test_gpu_specfeat.py on one).  numpy throughout; X is complex64 [..., T, F], up-cast to complex128 first.

Definitions
    abs_feature         |X|
    log1p_abs_feature   L = log1p(|X|)                               (padertorch's Log1pAbsSTFT; the reference's doctest)
    mvn_feature         L - mean over the T frames of L              (np.mean(feature, axis=-2, keepdims=True))
    mvn_causal_feature  per frame, in frame order, a = forgetting:   S = a S + L;  n = a n + 1;  out = L - S / n

Bounds, in units of U = 2^-24 (the unit roundoff of float32; one ulp is at most 2 U relative)

  |X|.  The kernel computes sqrt(fl(fl(re re) + fl(im im))), every operation rounded to nearest.  The two squares are
  within U of re^2 and im^2 relatively, both are non-negative, so their exact sum is within U of p = re^2 + im^2; the
  rounded sum is within 2 U + U^2.  The square root halves a relative error (sqrt(1 + 2 U) <= 1 + U), and sqrtf is
  correctly rounded: one more U.  First order: 2 U |X|.  The first-order figure leaves no room for the U^2 terms and for
  a square that falls below the normal range (where fl() loses relative accuracy, for components far below the other),
  so C0 = 3:
                                    | |X|_kernel - |X| |  <=  C0 U |X| + TINY

  L.  log1p is increasing and concave with log1p'(a) = 1 / (1 + a), so an argument a (1 + e) moves the value by at most
  e a / (1 + a) <= e log1p(a)        (a / (1 + a) <= log1p(a) for a >= 0).
  The propagated input error is therefore C0 U L.  OCML's log1pf is documented to 2 ulp (the OpenCL full-profile limit it
  honours), at most 4 U relative to the value it returns.  C1 = C0 + 4 = 7:
                                    | L_kernel - L |  <=  C1 U L + TINY

  MVN (whole utterance or running).  The mean is a weighted mean of the frames' L with non-negative weights summing to
  one, so its error is at most the same mean of the frames' errors, C1 U mean(L), plus the float64 chain: one rounding
  per frame for S, one per frame for n, the division -- (frames + 4) 2^-53 relative, kept as its own term although it is
  five orders below U at the lengths tested.  The difference is formed in float64 and rounded once to float32, U |out|:
                 | out_kernel - out |  <=  (C1 U + (frames + 4) 2^-53) (L + mean) + U |out| + TINY
  `mean` is the reference's own mean at that frame (S / n for the running form), `frames` the frames the state has seen.
  A float32 running sum does not meet this: at 2 10^5 frames of L ~ 1 its spacing is 2^-6, five orders above C1 U.

  TINY = 2^-126, the smallest normal float32, is the absolute floor throughout.

The constants follow from the derivation above, not from what the kernels give; what the kernels do give is printed by the
GPU tests (`worst`) and recorded in DESIGN.md 4.23.  Checked without a device: the float32 numpy restatement
(`restatement32`) stands at 0.62 of the |X| bound, 0.50 of L's, 0.36 of the MVN's and 0.38 of the running MVN's over the
shapes below and magnitudes 1e-6 ... 1e3."""
import numpy as np

U = 2.0 ** -24
EPS64 = 2.0 ** -53
TINY = 2.0 ** -126
C0 = 3.0
LOG1P_ULPS = 2.0
C1 = C0 + 2.0 * LOG1P_ULPS

# the shapes of tests/test_gpu_specfeat_kernels.py: T = 70 takes the unrolled frame loop (8 frames a trip) and its
# remainder, T = 1 and 2 the remainder alone; F = 1 and 5 put several utterances into one wave, 513 is the shipped
# size, 1025 the largest
BS, TS, FS = (1, 3), (1, 2, 70), (1, 5, 513, 1025)


def make_input(B, T, F, seed=0):
    """complex64 [B, T, F]: magnitudes over nine decades (1e-6 ... 1e3), every phase; utterance 1 of a batch is digital
    silence, and so is one frame of utterance 0 when it has more than two."""
    rng = np.random.RandomState(1000 * seed + 97 * B + 13 * T + F)
    mag = 10.0 ** rng.uniform(-6.0, 3.0, size=(B, T, F))
    X = (mag * np.exp(2j * np.pi * rng.uniform(size=(B, T, F)))).astype(np.complex64)
    if B > 1:
        X[1] = 0
    if T > 2:
        X[0, T // 2] = 0
    return X


def _c128(X):
    X = np.asarray(X)
    return X.astype(np.complex128)


def abs_feature(X):
    return np.abs(_c128(X))


def log1p_abs_feature(X):
    return np.log1p(np.abs(_c128(X)))


def mvn_feature(X):
    L = log1p_abs_feature(X)
    return L - np.mean(L, axis=-2, keepdims=True)


def mvn_causal_feature(X, S=None, n=None, forgetting=1.0, with_mean=False):
    """-> (out [..., T, F], S [..., F], n [...]) (with_mean: also the running mean S / n of every frame).  S, n None: a
    fresh stream."""
    L = log1p_abs_feature(X)
    lead, (T, F) = L.shape[:-2], L.shape[-2:]
    S = np.zeros(lead + (F,)) if S is None else np.array(S, dtype=np.float64)
    n = np.zeros(lead) if n is None else np.array(n, dtype=np.float64)
    out, means = np.empty_like(L), np.empty_like(L)
    for t in range(T):
        S = forgetting * S + L[..., t, :]
        n = forgetting * n + 1.0
        means[..., t, :] = S / n[..., None]
        out[..., t, :] = L[..., t, :] - means[..., t, :]
    return (out, S, n, means) if with_mean else (out, S, n)


# ---- bounds ----------------------------------------------------------------------------------------------------------------
def abs_bound(X):
    return C0 * U * abs_feature(X) + TINY


def log1p_bound(X):
    return C1 * U * log1p_abs_feature(X) + TINY


def _mvn_bound(L, mean, frames):
    return (C1 * U + (frames + 4.0) * EPS64) * (L + mean) + U * np.abs(L - mean) + TINY


def mvn_bound(X):
    L = log1p_abs_feature(X)
    return _mvn_bound(L, np.mean(L, axis=-2, keepdims=True), L.shape[-2])


def mvn_causal_bound(X, S=None, n=None, forgetting=1.0, frames_before=0):
    L = log1p_abs_feature(X)
    means = mvn_causal_feature(X, S, n, forgetting, with_mean=True)[3]
    frames = frames_before + 1.0 + np.arange(L.shape[-2])[:, None]
    return _mvn_bound(L, means, frames)


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound; inf when anything is not finite or a shape differs"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape or not np.isfinite(got).all():
        return float("inf")
    return float(np.max(np.abs(got - ref) / bound)) if got.size else 0.0


def held(got, ref, bound, what):
    w = worst(got, ref, bound)
    print(f"specfeat {what}: worst error / bound = {w:.3f}")
    assert w <= 1.0, f"{what}: worst error / bound = {w}"
    return w


# ---- the float32 restatement (what the kernels compute, in numpy) ----------------------------------------------------------
def restatement32(X, kind, S=None, n=None, forgetting=1.0, defect=None):
    """kind 'abs' | 'log1p' | 'mvn' -> float32 [..., T, F]; 'causal' -> (out, S, n).  defect plants one mistake (the
    CPU test's planted defects): 'mean_f', 'next_frame', 'count', 'forget_S_only', 'log', 'sum32', 'drop_state'."""
    X = np.asarray(X).astype(np.complex64)
    re, im = X.real.astype(np.float32), X.imag.astype(np.float32)
    a = np.sqrt(re * re + im * im)
    assert a.dtype == np.float32
    if kind == "abs":
        return a
    with np.errstate(divide="ignore"):
        L = np.log(a) if defect == "log" else np.log1p(a)
    assert L.dtype == np.float32
    if kind == "log1p":
        return L
    Ld = L.astype(np.float64)
    if kind == "mvn":
        if defect == "mean_f":
            return (Ld - Ld.mean(axis=-1, keepdims=True)).astype(np.float32)
        S_ = np.zeros(Ld.shape[:-2] + Ld.shape[-1:])
        for t in range(Ld.shape[-2]):
            S_ = S_ + Ld[..., t, :]
        return (Ld - (S_ / Ld.shape[-2])[..., None, :]).astype(np.float32)
    assert kind == "causal", kind
    lead, (T, F) = Ld.shape[:-2], Ld.shape[-2:]
    acc = np.float32 if defect == "sum32" else np.float64
    S = np.zeros(lead + (F,), acc) if S is None or defect == "drop_state" else np.array(S, dtype=acc)
    n = np.zeros(lead) if n is None or defect == "drop_state" else np.array(n, dtype=np.float64)
    alpha = acc(forgetting)
    out = np.empty(Ld.shape, np.float32)
    for t in range(T):
        S = alpha * S + L[..., t, :].astype(acc)
        if defect == "next_frame" and t + 1 < T:
            S = S + L[..., t + 1, :].astype(acc)
        n = (1.0 if defect == "forget_S_only" else forgetting) * n + 1.0
        cnt = n + 1.0 if defect == "count" else n
        out[..., t, :] = (Ld[..., t, :] - S.astype(np.float64) / cnt[..., None]).astype(np.float32)
        if defect == "next_frame" and t + 1 < T:
            S = S - L[..., t + 1, :].astype(acc)
    return out, S.astype(np.float64), n
