"""The checker of the WPE kernels (tests/test_gpu_wpe.py), tested without a GPU: a float64 numpy restatement of the
definition in DESIGN 4.5 (nara_wpe's wpe_v8 -> wpe_v6 with psd_context = 0, [recalled]: nara_wpe is not installed), the same
lines one step above float64 (np.longdouble where it has a 64-bit significand, mpmath otherwise: the helpers of
tests/test_mvdr_reference.py, complex numbers as pairs of real arrays), per-stage references with their bounds, and the
input generators.  U = 2^-53.

DEFINITION, one bin, Y [D, T], K = taps * D:
    Yt[tau*D + d, t] = Y[d, t - delay - tau]  (zero where that index is negative);   X = Y;   `iterations` times:
    p[t] = mean_d |X[d,t]|^2;  eps = 1e-10 max_t p[t];  li[t] = 1 / max(p[t], eps)
    R = sum_t li[t] Yt[:,t] Yt[:,t]^H,  P = sum_t li[t] Yt[:,t] Y[:,t]^H   (t >= delay + taps - 1 only for 'valid')
    R G = P;   X = Y - G^H Yt  at all frames

BOUNDS (componentwise on re and im; gamma_n(k) = k U / (1 - k U); nothing fitted to a kernel's output).
  power         |li^ - li| <= gamma_n(D + 5) li: each |x|^2 is two products and a sum of positive terms (2), D - 1 further
                additions of positive terms, the division by D (1), eps = 1e-10 pmax (1; the maximum is monotone, so it
                carries the relative error of its arguments and adds none), the reciprocal (1), the reference rounded to
                float64 (1).
  correlations  stats_bound of the MVDR file with the weight li: |err| <= gamma_n(n + 4 + c) sum_t li |Yt_i| |Yt_j| +
                n 2^-1074 for n frames summed in c chunks (weight 1, two products and their sum 2, n additions, c joins).
  solve         Cholesky R = L L^H with P eliminated alongside, then L^H G = W (Higham, Accuracy and Stability, Thm 10.3 /
                10.4 with the constants of complex arithmetic as in the MVDR file): every entry of L L^H is a chain of at
                most K multiply-subtracts (C_MUL = 2 sqrt 2 for the product, one per subtraction), the square root and the
                division by it (2): |R - L^ L^^H| <= (K + C_MUL + 2) U |L^| |L^^H|; each substitution the same chain with one
                division: (K + C_MUL + 1) U.  Together  |P - R G^| <= GAMMA_C(K) |L| |L^H| |G^|,
                GAMMA_C = g / (1 - g), g = (3 K + 3 C_MUL + 4) U.  K = 60: 192.5 U = 2.1e-14.  |L| |L^H| is taken from the
                extended factor of the same float64 R (second-order difference to the computed one).
  filter        |err| <= gamma_n(K + 3) (|Y| + sum_i |G_i| |Yt_i|) + 2^-1074: per term a product (2 roundings in gamma
                units: 2 products and their sum), K subtractions, the reference rounded to float64.
  whole call    no fixed tolerance is honest at cond(R) 1e11: the error of ANY float64 solve is cond(R) U.  The GPU result
                is held to  max|X_gpu - X_ext| <= 8 max|X_f64 - X_ext|,  X_f64 the float64 restatement below (LAPACK's
                zgesv) on the same input: its own distance from the extended result IS the error of float64 at that
                condition; 8 covers the different elimination (Cholesky) and summation order.

GENERATORS (seeded).  `white`: complex Gaussian.  `reverberant`: a sparse source through D exponentially decaying
convolutive transfer functions of 24 frames plus sensor noise at -40 dB -- late reverberation that the taps can predict, so
that the iterations sharpen li and R loses rank numerically.  Conditions reached (this file, D = 6, taps = 10, delay = 2,
T = 200, 8 bins; test_generators_reach_the_conditions_of_array_data prints them):
    white        cond(R) 1.1e1 .. 1.8e1 at iteration 1,  2.4e1 .. 1.1e3 at iteration 3;  |X_f64 - X_ext| 3.7e-15 .. 5.6e-14
    reverberant  cond(R) 1.1e5 .. 3.1e5 at iteration 1,  4.0e7 .. 2.7e12 at iteration 3; |X_f64 - X_ext| 1.1e-9 .. 1.2e-4
    (of an output of modulus about 1), so 8 x that is the tolerance the GPU result meets on the same bins.

PLANTED DEFECTS (test_planted_defects_exceed_the_whole_call_bound), the float64 restatement with one defect against
8 max|X_f64 - X_ext| on the same input, worst over the bins; the clean run is 1/8 by construction:
    taps reaching across the segment start 7.7e+3   eps from the global maximum 7.0   R without li 4.4e+3
"""
import numpy as np
import pytest

import test_mvdr_reference as M
from test_mvdr_reference import U, C_MUL, DENORM, xr, xf, xc, xcf, cmul, gamma_n

WPE_TCHUNK = 256          # frames per chunk of wpe_corr_kernel (csrc/wpe.hip: TCHUNK)
MARGIN = 8.0


def chol_gamma(K):
    g = (3.0 * K + 3.0 * C_MUL + 4.0) * U
    return g / (1.0 - g)


# ---- the definition ------------------------------------------------------------------------------------------------------
def tilde(Y, taps, delay):
    """Y [D, T, ...] (any dtype) -> Yt [taps * D, T, ...]: row tau * D + d at frame t is Y[d, t - delay - tau], else zero"""
    D, T = Y.shape[:2]
    Yt = np.zeros((taps * D,) + Y.shape[1:], dtype=Y.dtype)
    if Y.dtype == object:
        Yt[...] = xr(np.zeros(1))[0]
    for tau in range(taps):
        sh = delay + tau
        if sh < T:
            Yt[tau * D:(tau + 1) * D, sh:] = Y[:, :T - sh]
    return Yt


def stat_range(T, taps, delay, mode):
    assert mode in ("full", "valid"), mode
    return slice(delay + taps - 1, T) if mode == "valid" else slice(0, T)


def power_float64(X, defect=None):
    p = np.mean(np.abs(X) ** 2, axis=0)                         # [T, F]
    eps = 1e-10 * (p.max() if defect == "global_eps" else p.max(0))
    return 1.0 / np.maximum(p, eps)


def wpe_float64(Y, taps=10, delay=2, iterations=3, mode="full", defect=None, Yt=None, trace=None):
    """Y [D, T, F] complex128 -> X [D, T, F].  Yt: a tilde matrix to use instead of tilde(Y) (the `across` defect hands in
    one that reaches in front of the slice).  trace: a list that receives (li, R, P, G) of every iteration."""
    Y = np.asarray(Y, dtype=np.complex128)
    D, T, F = Y.shape
    Yt = tilde(Y, taps, delay) if Yt is None else Yt
    sl = stat_range(T, taps, delay, mode)
    X = Y.copy()
    for _ in range(iterations):
        li = power_float64(X, defect)
        w = np.ones_like(li[sl]) if defect == "no_lambda" else li[sl]
        R = np.einsum("tf,itf,jtf->fij", w, Yt[:, sl], Yt[:, sl].conj())
        P = np.einsum("tf,itf,dtf->fid", w, Yt[:, sl], Y[:, sl].conj())
        G = np.linalg.solve(R, P)
        X = Y - np.einsum("fid,itf->dtf", G.conj(), Yt)
        if trace is not None:
            trace.append((li, R, P, G))
    return X


def channelwise_float64(Y, **kw):
    """ChannelWiseWPE: '1 t (d f)'"""
    D, T, F = Y.shape
    return wpe_float64(Y.transpose(1, 0, 2).reshape(1, T, D * F), **kw).reshape(T, D, F).transpose(1, 0, 2)


# ---- the same in extended precision ---------------------------------------------------------------------------------------
def _x0(shape):
    a = np.empty(shape, dtype=xr(np.zeros(1)).dtype)
    a[...] = xr(np.zeros(1))[0]
    return a


def power_extended(X):
    """X pair [D, T, F] -> li extended [T, F]"""
    D = X[0].shape[0]
    p = (X[0] * X[0] + X[1] * X[1]).sum(0) / xr(np.array(float(D)))
    eps = xr(np.array(1e-10)) * p.max(0)
    m = np.where(np.asarray(p > eps, dtype=bool), p, eps)
    return xr(np.ones(1))[0] / m


def correlations_extended(Y, Yt, li, sl):
    """Y pair [D, T, F], Yt pair [K, T, F], li extended [T, F] -> (R pair [F, K, K], P pair [F, K, D]) and, in float64,
    SR = sum_t li |Yt_i| |Yt_j|, SP = sum_t li |Yt_i| |Y_d|"""
    K, F, D = Yt[0].shape[0], Yt[0].shape[2], Y[0].shape[0]
    Rr, Ri, Pr, Pi = _x0((F, K, K)), _x0((F, K, K)), _x0((F, K, D)), _x0((F, K, D))
    ytr, yti, yr, yi, w = Yt[0][:, sl], Yt[1][:, sl], Y[0][:, sl], Y[1][:, sl], li[sl]
    for i in range(K):
        ar, ai = w * ytr[i], w * yti[i]
        pr, pi = cmul((ar[None], ai[None]), (ytr, -yti))
        Rr[:, i, :], Ri[:, i, :] = pr.sum(1).T, pi.sum(1).T
        pr, pi = cmul((ar[None], ai[None]), (yr, -yi))
        Pr[:, i, :], Pi[:, i, :] = pr.sum(1).T, pi.sum(1).T
    ma, my, wf = np.hypot(xf(ytr), xf(yti)), np.hypot(xf(yr), xf(yi)), np.abs(xf(w))
    SR = np.einsum("tf,itf,jtf->fij", wf, ma, ma)
    SP = np.einsum("tf,itf,dtf->fid", wf, ma, my)
    return (Rr, Ri), (Pr, Pi), SR, SP


def cholesky_solve_extended(R, P):
    """R pair [F, K, K] (its lower triangle and real diagonal are read), P pair [F, K, D] -> G pair [F, K, D], L complex128
    [F, K, K] (lower), bad [F]: a pivot that is not positive"""
    Ar, Ai, Br, Bi = R[0].copy(), R[1].copy(), P[0].copy(), P[1].copy()
    F, K = Ar.shape[:2]
    one = xr(np.ones(1))[0]
    bad = np.zeros(F, dtype=bool)
    for k in range(K):
        d = Ar[:, k, k].copy()
        nb = ~np.asarray(d > 0, dtype=bool)
        bad |= nb
        d[nb] = one
        s = np.sqrt(d) if d.dtype != object else np.frompyfunc(lambda v: v.sqrt(), 1, 1)(d)
        Ar[:, k, k], Ai[:, k, k] = s, 0 * s
        Ar[:, k + 1:, k] /= s[:, None]
        Ai[:, k + 1:, k] /= s[:, None]
        Br[:, k] /= s[:, None]
        Bi[:, k] /= s[:, None]
        if k + 1 < K:
            lr, li_ = Ar[:, k + 1:, k], Ai[:, k + 1:, k]
            ur, ui = cmul((lr[:, :, None], li_[:, :, None]), (lr[:, None, :], -li_[:, None, :]))
            Ar[:, k + 1:, k + 1:] -= ur
            Ai[:, k + 1:, k + 1:] -= ui
            wr, wi = cmul((lr[:, :, None], li_[:, :, None]), (Br[:, k, None, :], Bi[:, k, None, :]))
            Br[:, k + 1:] -= wr
            Bi[:, k + 1:] -= wi
    for k in range(K - 1, -1, -1):
        s = Ar[:, k, k]
        Br[:, k] /= s[:, None]
        Bi[:, k] /= s[:, None]
        if k:
            gr, gi = cmul((Ar[:, k, :k, None], -Ai[:, k, :k, None]), (Br[:, k, None, :], Bi[:, k, None, :]))
            Br[:, :k] -= gr
            Bi[:, :k] -= gi
    L = np.tril(xf(Ar) + 1j * xf(Ai))
    return (Br, Bi), L, bad


def filter_extended(Y, Yt, G):
    """X = Y - G^H Yt: Y pair [D, T, F], Yt pair [K, T, F], G pair [F, K, D] -> X pair [D, T, F]"""
    K, D = Yt[0].shape[0], Y[0].shape[0]
    Xr, Xi = Y[0].copy(), Y[1].copy()
    for d in range(D):
        gr, gi = G[0][:, :, d].T[:, None, :], G[1][:, :, d].T[:, None, :]          # [K, 1, F]
        pr, pi = cmul((gr, -gi), Yt)
        Xr[d] -= pr.sum(0)
        Xi[d] -= pi.sum(0)
    return Xr, Xi


def wpe_extended(Y, taps=10, delay=2, iterations=3, mode="full"):
    """-> X complex128 [D, T, F] rounded from the extended run, bad [F]"""
    Y = np.asarray(Y, dtype=np.complex128)
    T = Y.shape[1]
    Yx = xc(Y)
    Ytx = (tilde(Yx[0], taps, delay), tilde(Yx[1], taps, delay))
    sl = stat_range(T, taps, delay, mode)
    X = Yx
    bad = np.zeros(Y.shape[2], dtype=bool)
    for _ in range(iterations):
        li = power_extended(X)
        R, P, _, _ = correlations_extended(Yx, Ytx, li, sl)
        G, _, b = cholesky_solve_extended(R, P)
        bad |= b
        X = filter_extended(Yx, Ytx, G)
    return xcf(X), bad


# ---- per-stage references for the GPU tests --------------------------------------------------------------------------------
def power_reference(X):
    """X complex128 [D, T, F] -> li float64 [T, F] rounded from extended, relative bound"""
    return xf(power_extended(xc(X))), gamma_n(X.shape[0] + 5)


def correlations_reference(Y, li, taps, delay, mode):
    """Y [D, T, F], li float64 [T, F] as the kernel is handed it -> R [F, K, K], P [F, K, D] complex128 (rounded), and the
    bounds on each component for T frames summed in ceil(T / WPE_TCHUNK) chunks"""
    T = Y.shape[1]
    Yx = xc(Y)
    Ytx = (tilde(Yx[0], taps, delay), tilde(Yx[1], taps, delay))
    R, P, SR, SP = correlations_extended(Yx, Ytx, xr(li), stat_range(T, taps, delay, mode))
    c = (T + WPE_TCHUNK - 1) // WPE_TCHUNK
    return xcf(R), xcf(P), M.stats_bound(SR, T, joined=c + 1), M.stats_bound(SP, T, joined=c + 1)


def solve_ratio(R, P, G_hat):
    """worst |P - R G^| / (GAMMA_C |L| |L^H| |G^|) per system; R [F, K, K] float64-valued Hermitian, as handed to the kernel"""
    K = R.shape[-1]
    _, L, bad = cholesky_solve_extended(xc(R), xc(P))
    assert not bad.any()
    Rx, Gx, Px = xc(R), xc(G_hat), xc(P)
    rr, ri = Px[0].copy(), Px[1].copy()
    for k in range(K):
        tr, ti = cmul((Rx[0][:, :, k, None], Rx[1][:, :, k, None]), (Gx[0][:, k, None, :], Gx[1][:, k, None, :]))
        rr, ri = rr - tr, ri - ti
    res = np.maximum(np.abs(xf(rr)), np.abs(xf(ri)))
    bound = chol_gamma(K) * (np.abs(L) @ np.abs(np.swapaxes(L, -2, -1)) @ np.abs(G_hat))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where((res == 0) & (bound == 0), 0.0, res / bound)
    r = np.where(np.isfinite(G_hat).all((-2, -1), keepdims=True), r, np.inf)
    return np.nan_to_num(r, nan=np.inf).max((-2, -1))


def filter_reference(Y, G, taps, delay):
    """Y [D, T, F], G [F, K, D] complex128 -> X complex128 (rounded), bound [D, T, F]"""
    Yx = xc(Y)
    Ytx = (tilde(Yx[0], taps, delay), tilde(Yx[1], taps, delay))
    X = xcf(filter_extended(Yx, Ytx, xc(G)))
    S = np.abs(Y) + np.einsum("fid,itf->dtf", np.abs(G), np.abs(tilde(Y, taps, delay)))
    return X, gamma_n(taps * Y.shape[0] + 3) * S + DENORM


def whole_call_bound(Y, **kw):
    """-> X_ext, the tolerance MARGIN * max|X_f64 - X_ext| per bin [F]"""
    X_ext, bad = wpe_extended(Y, **kw)
    assert not bad.any()
    return X_ext, MARGIN * np.abs(wpe_float64(Y, **kw) - X_ext).max((0, 1))


# ---- generators ------------------------------------------------------------------------------------------------------------
def _crandn(rs, *shape):
    return rs.standard_normal(shape) + 1j * rs.standard_normal(shape)


def white(D, T, F, seed):
    return _crandn(np.random.RandomState(seed), D, T, F)


def reverberant(D, T, F, seed, rir=24, decay=0.8, noise=1e-2):
    """a sparse source through D decaying convolutive transfer functions of `rir` frames per bin + sensor noise"""
    rs = np.random.RandomState(seed)
    s = _crandn(rs, T + rir, F) * (rs.random_sample((T + rir, F)) < 0.6)
    h = _crandn(rs, D, rir, F) * (decay ** np.arange(rir))[None, :, None]
    Y = np.zeros((D, T, F), dtype=np.complex128)
    for q in range(rir):
        Y += h[:, q, None, :] * s[None, rir - q:rir - q + T, :]
    Y /= np.sqrt(np.mean(np.abs(Y) ** 2))
    return Y + noise * _crandn(rs, D, T, F)


GENERATORS = {"white": white, "reverberant": reverberant}


def levels(Y, seed):
    """bins of very different level and a few silent frames: the per-bin eps differs from a global one and takes effect"""
    rs = np.random.RandomState(seed)
    Y = Y * (10.0 ** rs.uniform(-4, 0, Y.shape[2]))[None, None, :]
    Y[:, rs.choice(np.arange(4, Y.shape[1]), 3, replace=False), :] = 0.0
    return Y


# ---- tests of the above on the CPU -------------------------------------------------------------------------------------------
def test_tilde_layout_by_hand():
    Y = (np.arange(1, 11).reshape(2, 5) * (1 + 0j))[:, :, None]            # Y[0] = 1..5, Y[1] = 6..10
    Yt = tilde(Y, taps=2, delay=1)[:, :, 0].real
    assert np.array_equal(Yt, [[0, 1, 2, 3, 4], [0, 6, 7, 8, 9], [0, 0, 1, 2, 3], [0, 0, 6, 7, 8]])
    assert np.array_equal(tilde(Y, taps=1, delay=0), Y)
    Yt = tilde(Y[:1], taps=3, delay=2)[:, :, 0].real
    assert np.array_equal(Yt, [[0, 0, 1, 2, 3], [0, 0, 0, 1, 2], [0, 0, 0, 0, 1]])
    assert np.array_equal(tilde(Y, taps=2, delay=7), np.zeros((4, 5, 1)))
    ext = tilde(xr(Y.real), taps=2, delay=1)
    assert np.array_equal(xf(ext), tilde(Y, 2, 1).real)


def test_valid_drops_exactly_the_frames_with_incomplete_history():
    Y = white(2, 30, 3, 1)
    taps, delay = 3, 1
    tf, tv = [], []
    wpe_float64(Y, taps, delay, 1, "full", trace=tf)
    wpe_float64(Y, taps, delay, 1, "valid", trace=tv)
    Yt, li = tilde(Y, taps, delay), tf[0][0]
    head = np.einsum("tf,itf,jtf->fij", li[:delay + taps - 1], Yt[:, :delay + taps - 1], Yt[:, :delay + taps - 1].conj())
    assert np.abs(head).max() > 0.1
    assert np.abs(tf[0][1] - tv[0][1] - head).max() < 1e-12
    assert (Yt[:, delay + taps - 1] != 0).all() and (Yt[-1, delay + taps - 2] == 0).all()
    assert stat_range(30, taps, delay, "valid") == slice(3, 30)


def test_eps_takes_effect_on_a_silent_frame():
    Y = white(2, 40, 3, 2)
    Y[:, 7] = 0.0
    li = power_float64(Y)
    pmax = np.mean(np.abs(Y) ** 2, axis=0).max(0)
    assert np.array_equal(li[7], 1.0 / (1e-10 * pmax)) and np.isfinite(li).all()
    assert (li[8] < 1e3).all()
    assert np.isfinite(wpe_float64(Y, 3, 1, 2)).all()
    lx, g = power_reference(Y)
    assert (np.abs(li - lx) <= g * lx).all()


@pytest.mark.parametrize("gen", GENERATORS)
@pytest.mark.parametrize("D,taps,delay,mode", [(1, 1, 0, "full"), (2, 3, 1, "valid"), (6, 10, 2, "full")])
def test_float64_restatement_against_extended(gen, D, taps, delay, mode):
    Y = GENERATORS[gen](D, taps * D + delay + 40, 3, 5)
    tr = []
    its = 2 if delay else 1         # delay 0 predicts a frame from itself: X = 0 after one iteration, nothing to iterate on
    X = wpe_float64(Y, taps, delay, its, mode, trace=tr)
    X_ext, bad = wpe_extended(Y, taps, delay, its, mode)
    assert not bad.any()
    c = np.linalg.cond(tr[-1][1]).max()
    err = np.abs(X - X_ext).max()
    print(gen, D, taps, "cond", c, "err", err)
    assert err <= 64 * taps * D * c * U * np.abs(Y).max()
    # the stage references on the first iteration's quantities
    li, R, P, G = tr[0]
    lx, g = power_reference(Y)
    assert (np.abs(li - lx) <= g * lx).all()
    Rx, Px, bR, bP = correlations_reference(Y, li, taps, delay, mode)
    assert (np.abs((R - Rx).real) <= bR).all() and (np.abs((R - Rx).imag) <= bR).all()
    assert (np.abs((P - Px).real) <= bP).all() and (np.abs((P - Px).imag) <= bP).all()
    Xf, bX = filter_reference(Y, G, taps, delay)
    X1 = Y - np.einsum("fid,itf->dtf", G.conj(), tilde(Y, taps, delay))
    assert (np.abs((X1 - Xf).real) <= bX).all() and (np.abs((X1 - Xf).imag) <= bX).all()


def test_extended_cholesky_solves_and_flags():
    Y = reverberant(3, 60, 4, 3)
    tr = []
    wpe_float64(Y, 4, 1, 1, trace=tr)
    _, R, P, _ = tr[0]
    R = M._herm(R)
    G, L, bad = cholesky_solve_extended(xc(R), xc(P))
    assert not bad.any()
    assert np.abs(L @ np.swapaxes(L.conj(), -2, -1) - R).max() <= 1e-12 * np.abs(R).max()
    Gf = xcf(G)
    assert solve_ratio(R, P, Gf).max() <= 1.0                          # the rounded extended solution
    assert solve_ratio(R, P, np.linalg.solve(R, P)).max() <= 1.0       # LAPACK
    Gb = Gf.copy()
    Gb[:, 0, 0] *= 1 + 1e-9
    assert solve_ratio(R, P, Gb).min() > 1.0
    R[2] = 0
    assert np.array_equal(cholesky_solve_extended(xc(R), xc(P))[2], [False, False, True, False])


def test_channelwise_is_per_channel_single_channel_wpe():
    """the reference's doctest identity (enhancer.py:355-358)"""
    Y = reverberant(3, 40, 5, 4)
    want = np.concatenate([wpe_float64(Y[d:d + 1], 10, 2, 3) for d in range(3)])
    assert np.array_equal(channelwise_float64(Y, taps=10, delay=2, iterations=3), want)


def _conds(gen, F=8):
    Y = GENERATORS[gen](6, 200, F, 11)
    tr = []
    X = wpe_float64(Y, 10, 2, 3, trace=tr)
    X_ext, bad = wpe_extended(Y, 10, 2, 3)
    assert not bad.any()
    return np.linalg.cond(tr[0][1]), np.linalg.cond(tr[2][1]), np.abs(X - X_ext).max((0, 1))


def test_generators_reach_the_conditions_of_array_data():
    c1, c3, e = _conds("white")
    print("white cond it1", c1.min(), c1.max(), "it3", c3.min(), c3.max(), "err", e.min(), e.max())
    assert c3.max() < 1e4 and e.max() < 1e-12
    c1, c3, e = _conds("reverberant")
    print("reverberant cond it1", c1.min(), c1.max(), "it3", c3.min(), c3.max(), "err", e.min(), e.max())
    assert c1.min() > 1e4 and c3.max() > 1e10 and c3.min() > 1e7
    # complex64 (U = 6e-8) loses the result there: float64 itself is already this far away
    assert e.max() > 1e-8


@pytest.mark.parametrize("defect", ("across", "global_eps", "no_lambda"))
def test_planted_defects_exceed_the_whole_call_bound(defect):
    taps, delay, s, e = 10, 2, 30, 230
    full = levels(reverberant(6, 230, 4, 21), 22)
    Y = full[:, s:e]
    X_ext, tol = whole_call_bound(Y, taps=taps, delay=delay, iterations=3)
    clean = np.abs(wpe_float64(Y, taps, delay, 3) - X_ext).max((0, 1))
    assert (clean <= tol).all()
    if defect == "across":
        bad = wpe_float64(Y, taps, delay, 3, Yt=tilde(full, taps, delay)[:, s:e])
    else:
        bad = wpe_float64(Y, taps, delay, 3, defect=defect)
    r = np.abs(bad - X_ext).max((0, 1)) / tol
    print(defect, "worst / tolerance", r.max(), "bins outside", int((r > 1).sum()), "of", r.size)
    assert r.max() > 1.0, (defect, r.max())


def test_chunk_constant_restates_the_source():
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "csrc",
                            "wpe.hip")).read()
    assert int(re.search(r"constexpr int TCHUNK = (\d+);", src).group(1)) == WPE_TCHUNK
