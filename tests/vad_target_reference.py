"""float64 references, error bound, checkers and planted defects for the VAD losses' device-built targets (helper module,
not collected): the STFT-magnitude activity of tssep/train/loss.py:312-327 and the sample -> frame gather that
tssep/util/utils.py:11-77 amounts to.

The chain under test:   X = stft(x)   a[r,t] = sum_f |X[r,t,f]|   ratio = a / max_t a   vad = ratio > thr.

ERROR BOUND OF a.  A float32 FFT of n points satisfies ||dZ||_2 <= log2(n) eta ||Z||_2 / (1 - log2(n) eta) with
eta = mu + gamma_4 (sqrt2 + mu) per radix-2 stage (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2); with
twiddles rounded once (mu = u) and gamma_4 ~ 4u that is eta ~ 6.7 u, u = 2^-24.  The kernels transform z = x_even + i x_odd
(size / 2 points: log2(size) - 1 radix-2 stages' worth; higher radices do fewer roundings) and split the result,
X_k = alpha_k Z_k + beta_k conj(Z_{n-k}) with |alpha|^2 + |beta|^2 = 1, so ||dX||_2 <= sqrt2 ||dZ||_2 over the size / 2 + 1
bins while ||Z||_2 = ||X_full||_2 / sqrt2 <= ||X||_2: sqrt2 * 6.7 u < 10 u per stage.  What remains -- the product with a
float32 window (two roundings per sample, sqrt2 * 2u on the spectrum by Parseval) and the split pass's own arithmetic
(~ 4u) -- is less than one more stage of 10 u.  Hence

    ||dX||_2 <= C_FFT log2(size) u ||X||_2,        C_FFT = 10,

and with ||.||_1 <= sqrt(F) ||.||_2 and ||.||_2 <= ||.||_1 over the F bins of a frame

    | sum_f |X32| - a64 | <= sqrt(F) C_FFT log2(size) u a64.

The modulus sqrtf(re^2 + im^2) adds at most 3u per bin (two products, a sum, a correctly rounded root) and the sum of F
non-negative terms -- ceil(F / 64) + 1 per lane, 6 levels across the wave -- at most (F / 64 + 8) u, both relative to a:

    |a - a64| <= (sqrt(F) C_FFT log2(size) + F / 64 + 11) u a64  =:  rel_bound(size, F) a64.

1024 / 513 bins: 2.3e3 u = 1.4e-4.  A frame of zeros has a64 = 0 and must give exactly 0.

DECISION BAND.  ratio = a / m carries the error of both: a frame is UNDECIDED when |ratio64 - thr| <= 2 rel_bound thr;
every other frame must be decided as the float64 chain decides it.  A row with m = 0 has ratio NaN: never undecided,
decided inactive."""
import math

import numpy as np
import torch

from oracle import stft as ostft

U32 = 2.0 ** -24
C_FFT = 10.0
MAX_UNDECIDED_SHARE = 1e-3


def rel_bound(size, F):
    return (math.sqrt(F) * C_FFT * math.log2(size) + F / 64 + 11) * U32


def mag_bound(a64, size, F):
    return rel_bound(size, F) * np.asarray(a64, dtype=np.float64)


# ---- the float64 chain ------------------------------------------------------------------------------------------------
def stft64(x, size=1024, shift=256, window="hann", window_length=None, pad=True, fading=True):
    return ostft.stft(np.asarray(x, dtype=np.float64), size=size, shift=shift, window=window, window_length=window_length,
                      pad=pad, fading=fading)


def frame_mag64(X):
    return np.abs(np.asarray(X)).astype(np.float64).sum(-1)


def ratio64(a64):
    with np.errstate(invalid="ignore", divide="ignore"):
        return a64 / np.amax(a64, axis=-1, keepdims=True)


def decide64(a64, thr):
    """loss.py:319-321 in float64: NaN (a silent row) compares false."""
    with np.errstate(invalid="ignore"):
        return ratio64(a64) > thr


def undecided(a64, thr, rel):
    with np.errstate(invalid="ignore"):
        return np.abs(ratio64(a64) - thr) <= 2 * rel * thr


def decide32(a32, thr):
    """The reference's own expression on a float32 tensor: what the device decisions must equal bit for bit."""
    a = torch.as_tensor(np.asarray(a32, dtype=np.float32))
    return ((a / torch.amax(a, dim=-1, keepdim=True)) > thr).numpy()


def gather_loop(vad, window_length, shift, fading):
    """Vad[r,t] = vad[r, i(t)], i(t) = (t + 1) shift + window_length // 2 - lead - 1; 0 where i(t) lies outside [0, N)."""
    vad = np.asarray(vad).astype(bool)
    R, N = vad.shape
    pad = window_length - shift
    lead = 0 if fading in (None, False) else (pad // 2 if fading == "half" else pad)
    n = N + (0 if fading in (None, False) else (pad if fading == "half" else 2 * pad))
    T = int(math.ceil((n - window_length + shift) / shift))
    out = np.zeros((R, T), dtype=bool)
    for r in range(R):
        for t in range(T):
            i = (t + 1) * shift + window_length // 2 - lead - 1
            if 0 <= i < N:
                out[r, t] = vad[r, i]
    return out


# ---- checkers (the GPU tests run the kernels' results through these; the CPU tests the planted defects) ------------------
def check_mag(a, a64, size, F, name="a"):
    a, a64 = np.asarray(a, dtype=np.float64), np.asarray(a64, dtype=np.float64)
    assert a.shape == a64.shape, (name, a.shape, a64.shape)
    err, tol = np.abs(a - a64), mag_bound(a64, size, F)
    bad = err > tol
    assert not bad.any(), (f"{name}: {int(bad.sum())}/{bad.size} outside the bound; worst err/bound "
                           f"{float(np.max(err[bad] / np.maximum(tol[bad], 1e-300))):.3g} at "
                           f"{np.unravel_index(int(np.argmax(err - tol)), err.shape)}")
    return float(np.max(np.where(a64 > 0, err / np.where(a64 > 0, a64, 1), 0.0)))         # the worst relative error, to print


def check_decisions(vad, a64, thr, rel, name="vad"):
    """vad (0 / 1) against the float64 decisions outside the band -> the undecided share (asserted <= 0.1 %)."""
    vad = np.asarray(vad)
    assert vad.shape == a64.shape, (name, vad.shape, a64.shape)
    assert np.isin(vad, (0, 1)).all(), name
    und = undecided(a64, thr, rel)
    want = decide64(a64, thr)
    bad = (vad.astype(bool) != want) & ~und
    assert not bad.any(), f"{name}: {int(bad.sum())} decisions differ outside the band, first at {np.argwhere(bad)[0]}"
    share = float(und.mean())
    assert share <= MAX_UNDECIDED_SHARE, f"{name}: {share:.3%} of the frames undecided"
    return share


def check_exact_decisions(vad, a32, thr, name="vad"):
    want = decide32(a32, thr)
    got = np.asarray(vad)
    assert got.shape == want.shape and np.isin(got, (0, 1)).all(), name
    bad = got.astype(bool) != want
    assert not bad.any(), f"{name}: {int(bad.sum())} decisions differ from torch's float32 formula, first at {np.argwhere(bad)[0]}"


def check_gather(Vad, vad, window_length, shift, fading, name="Vad"):
    want = gather_loop(vad, window_length, shift, fading)
    got = np.asarray(Vad)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isin(got, (0, 1)).all(), name
    assert np.array_equal(got.astype(bool), want), f"{name}: first difference at {np.argwhere(got.astype(bool) != want)[0]}"


# ---- constructed inputs ---------------------------------------------------------------------------------------------
def envelope_signal(rows, N, seed):
    """Gaussian noise under a per-row on / off envelope: runs of 300 - 3000 samples, active amplitude 0.2 - 1.0 (per run),
    inactive 1e-3 -> float32 [rows, N]."""
    rng = np.random.RandomState(seed)
    x = rng.randn(rows, N)
    env = np.empty((rows, N))
    for r in range(rows):
        n, on = 0, bool(rng.rand() < 0.5)
        while n < N:
            length = int(rng.randint(300, 3001))
            env[r, n:n + length] = rng.uniform(0.2, 1.0) if on else 1e-3
            n, on = n + length, not on
    return (x * env).astype(np.float32)


def special_rows(x):
    """The generator's rows with the edge cases the kernels must survive written over some of them (>= 5 rows): row 1 all
    zeros (an absent speaker), row 2 one non-zero sample, row 3 scaled by 1e-6, row 4 by 1e+6."""
    x = x.copy()
    if x.shape[0] >= 5:
        x[1] = 0
        x[2] = 0
        x[2, (2 * x.shape[1]) // 3 + 5] = 0.7
        x[3] *= np.float32(1e-6)
        x[4] *= np.float32(1e6)
    return x


# the fused chain's cases: every plan and path of tssep_stft_framemag_fwd (tests/test_gpu_vad_target_kernels.py runs them on
# the device, tests/test_vad_target_reference.py holds the float64 reference alone to the undecided share on each)
FUSED_CASES = [
    # name,                 size, shift, window,     window_length, fading, pad,  rows, N,    seed, offset
    ("1024_odd_N",          1024, 256, "hann",     None, True,   True,  5, 4099, 1, 0),   # slow path; rows T = 100: a part-filled
    ("1024_aligned",        1024, 256, "hann",     None, True,   True,  5, 4096, 2, 0),   # last workgroup; the fast path
    ("1024_offset_1_float", 1024, 256, "hann",     None, True,   True,  5, 4096, 2, 1),   # N even, the buffer 4-byte aligned
    ("1024_no_fading",      1024, 256, "blackman", None, False,  True,  5, 4099, 3, 0),
    ("1024_short_row",      1024, 256, "hann",     None, True,   True,  1, 300,  4, 0),   # shorter than a window
    ("512_128",             512,  128, "hann",     None, True,   True,  5, 3001, 5, 0),   # the general plan
    ("400_200_hann",        400,  200, "hann",     None, True,   True,  5, 2500, 6, 0),
    ("wl800_half_nopad",    1024, 256, "blackman", 800,  "half", False, 5, 4099, 7, 0),   # through STFT.frame_activity
]
THRESHOLD = 0.05


def fused_case(case):
    """-> (x float32 [rows, N], stft keyword arguments, a64 [rows, T], F)"""
    name, size, shift, window, wl, fading, pad, rows, N, seed, _ = case
    x = special_rows(envelope_signal(rows, N, seed))
    kw = dict(size=size, shift=shift, window=window, window_length=wl, pad=pad, fading=fading)
    return x, kw, frame_mag64(stft64(x, **kw)), size // 2 + 1


def product_tie(thr, search=4096):
    """(a, m) float32 with fl(a / m) > thr but not a > fl(thr m), or the other way round: where the rewritten comparison
    `a > thr m` decides differently from the reference's division."""
    thr = np.float32(thr)
    rng = np.random.RandomState(0)
    for _ in range(search):
        m = np.float32(rng.uniform(0.5, 1000.0))
        p = np.float32(thr * m)
        for a in (np.nextafter(p, np.float32(0)), p, np.nextafter(p, np.float32(np.inf))):
            if bool(np.float32(a / m) > thr) != bool(a > p):
                return np.float32(a), m
    raise AssertionError("no tie found")


# ---- planted defects: each returns what a wrong kernel would have produced -----------------------------------------------
def defect_nyquist_dropped(X):
    return np.abs(X[..., :-1]).sum(-1)


def defect_dc_twice(X):
    return np.abs(X).sum(-1) + np.abs(X[..., 0])


def defect_re_plus_im(X):
    return (np.abs(X.real) + np.abs(X.imag)).sum(-1)


def defect_batch_max(a, thr):
    a = np.asarray(a, dtype=np.float32)
    return (a / a.max() > np.float32(thr))


def defect_greater_equal(a, thr):
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (a / a.max(-1, keepdims=True)) >= np.float32(thr)


def defect_product(a, thr):
    a = np.asarray(a, dtype=np.float32)
    return a > (np.float32(thr) * a.max(-1, keepdims=True)).astype(np.float32)


def defect_silent_active(a, thr):
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        r = a / a.max(-1, keepdims=True)
    return ~(r <= np.float32(thr))                 # a NaN ratio passes


def defect_gather_off_by_one(vad, wl, sh, fading):
    v = np.asarray(vad).astype(bool)
    return gather_loop(np.concatenate([v[:, 1:], np.zeros_like(v[:, :1])], -1), wl, sh, fading)     # reads i + 1


def defect_half_as_full(vad, wl, sh, fading):
    want = gather_loop(vad, wl, sh, fading)
    full = gather_loop(vad, wl, sh, True)
    out = np.zeros_like(want)
    n = min(want.shape[-1], full.shape[-1])
    out[:, :n] = full[:, :n]
    return out
