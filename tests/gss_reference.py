"""float64 numpy reference of the guided cACGMM, written over the definition: loops over blocks, classes
and matrix entries; every bin is carried along as the last axis (the bins never meet).  `order` permutes the frame
order of the sums over frames and nothing else: the change of the result between the orders is the reference's own
sensitivity to the summation order, the yardstick of the GPU tests.  `_defect` plants one deliberate mistake (the CPU
tests show that each moves the result by more than the GPU tests allow).  Also the scene generator of the tests."""
import numpy as np

TINY = np.finfo(np.float64).tiny
ORDERS = ("forward", "reversed", "even_odd")
DEFECTS = ("no_D", "plus_ld", "prior_start_only", "stale_pi", "no_q_weight", "q_one")


def frame_order(T, order):
    t = np.arange(T)
    if order == "forward":
        return t
    if order == "reversed":
        return t[::-1].copy()
    if order == "even_odd":
        return np.concatenate([t[0::2], t[1::2]])
    raise ValueError(order)


def _fsum(x, perm):
    """sum over the frames (axis 0) of x [T, F], one frame after the other in the order `perm`"""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], dtype=x.dtype)
    return np.cumsum(x[perm], axis=0)[-1]          # a running sum: strictly sequential in the permuted order


def _fit(Y, act, iterations, load, weights, order, _defect=None, solve="substitution"):
    """one problem per bin: Y [D, T, F], act [K, T] -> gamma [K + 1, T, F]"""
    D, T, F = Y.shape
    K = act.shape[0]
    C = K + 1
    perm = frame_order(T, order)
    a = np.concatenate([np.asarray(act) != 0, np.ones((1, T), dtype=bool)], axis=0)            # [C, T]
    with np.errstate(all="ignore"):
        n2 = np.zeros((T, F))
        for d in range(D):
            n2 = n2 + (Y[d].real * Y[d].real + Y[d].imag * Y[d].imag)
        nrm = np.sqrt(n2)
        ok = np.isfinite(nrm) & (nrm > 0)
        yh = np.where(ok[None], Y / np.where(ok, nrm, 1.0)[None], 0.0)                           # [D, T, F]
    on = a[:, :, None] & ok[None]                                                                # [C, T, F]
    gamma = np.where(on, 1.0 / a.sum(0)[None, :, None], 0.0)
    q = np.ones((C, T, F))
    n_prev = None
    for it in range(iterations):
        n = np.stack([_fsum(gamma[c], perm) for c in range(C)])                                  # [C, F]
        ntot = np.zeros(F)
        for c in range(C):
            ntot = ntot + n[c]
        logp = np.full((C, T, F), -np.inf)
        for c in range(C):
            full = n[c] > 0                                                                      # [F]
            if not full.any():
                continue
            with np.errstate(all="ignore"):
                w = gamma[c] if _defect == "no_q_weight" else gamma[c] / q[c]
                B = np.zeros((D, D, F), dtype=np.complex128)
                for i in range(D):
                    for j in range(i + 1):
                        B[i, j] = (D / n[c]) * _fsum(w * yh[i] * np.conj(yh[j]), perm)
                        if i == j:
                            B[i, j] = B[i, j].real
                tr = np.zeros(F)
                for i in range(D):
                    tr = tr + B[i, i].real
                B = B * D / tr
                for i in range(D):
                    B[i, i] = B[i, i].real + load
                # Cholesky B = L L^H on the lower triangle
                L = np.zeros_like(B)
                ld = np.zeros(F)
                for j in range(D):
                    if solve == "extended_pivot":
                        # the pivot's cancellation carried one step above float64, rounded once (what a fused
                        # multiply-add chain approaches): another correct evaluation of the same formula
                        d = B[j, j].real.astype(np.longdouble)
                        for k in range(j):
                            d = d - (L[j, k].real.astype(np.longdouble) ** 2 + L[j, k].imag.astype(np.longdouble) ** 2)
                        d = d.astype(np.float64)
                    else:
                        d = B[j, j].real.copy()
                        for k in range(j):
                            d = d - (L[j, k].real ** 2 + L[j, k].imag ** 2)
                    ljj = np.sqrt(d)
                    L[j, j] = ljj
                    ld = ld + np.log(ljj)
                    for i in range(j + 1, D):
                        x = B[i, j].copy()
                        for k in range(j):
                            x = x - L[i, k] * np.conj(L[j, k])
                        L[i, j] = x / ljj
                ld = 2.0 * ld
                # v = L^-1 yh, q = |v|^2: by forward substitution, or (solve="inverse") as the product with X = L^-1
                v = np.zeros((D, T, F), dtype=np.complex128)
                qc = np.zeros((T, F))
                if solve == "inverse":
                    X = np.zeros_like(L)
                    for j in range(D):
                        X[j, j] = 1.0 / L[j, j]
                        for i in range(j + 1, D):
                            x = np.zeros(F, dtype=np.complex128)
                            for k in range(j, i):
                                x = x + L[i, k] * X[k, j]
                            X[i, j] = -x / L[i, i]
                else:
                    assert solve in ("substitution", "extended_pivot"), solve
                for i in range(D):
                    if solve == "inverse":
                        x = np.zeros((T, F), dtype=np.complex128)
                        for k in range(i + 1):
                            x = x + X[i, k][None] * yh[k]
                        v[i] = x
                    else:
                        x = yh[i].copy()
                        for k in range(i):
                            x = x - L[i, k][None] * v[k]
                        v[i] = x / L[i, i][None]
                    qc = qc + (v[i].real ** 2 + v[i].imag ** 2)
                qc = np.maximum(qc, TINY)
                if _defect == "q_one":
                    qc = np.ones((T, F))
                if weights == "bin":
                    src = n_prev if (_defect == "stale_pi" and n_prev is not None) else n
                    logpi = np.log(src[c] / src.sum(0))
                else:
                    logpi = np.zeros(F)
                lp = logpi[None] + (ld if _defect == "plus_ld" else -ld)[None] \
                    - (1 if _defect == "no_D" else D) * np.log(qc)
            prior = ok if _defect == "prior_start_only" else on[c]
            logp[c] = np.where(prior & full[None], lp, -np.inf)
            q[c] = np.where(full[None], qc, q[c])
        with np.errstate(all="ignore"):
            mx = logp.max(axis=0)                                                                # [T, F]
            e = np.where(np.isfinite(logp) & np.isfinite(mx)[None], np.exp(logp - mx[None]), 0.0)
            s = np.zeros((T, F))
            for c in range(C):
                s = s + e[c]
            gamma = np.where(s[None] > 0, e / np.where(s > 0, s, 1.0)[None], 0.0)
        n_prev = n
    return gamma


def guided_cacgmm_reference(Y, act, iterations=20, load=1e-6, weights="bin", blocks=None, order="forward",
                            _defect=None, solve="substitution"):
    """Y [D, T, F] complex128, act [K, T] of 0 / 1 -> gamma [K + 1, T, F] float64.  blocks: rows (s_fit, e_fit, s_out,
    e_out); every block is fitted on Y[:, s_fit:e_fit] and read on [s_out, e_out)."""
    Y = np.asarray(Y, dtype=np.complex128)
    act = np.asarray(act)
    D, T, F = Y.shape
    if blocks is None:
        blocks = [(0, T, 0, T)]
    out = np.zeros((act.shape[0] + 1, T, F))
    for sf, ef, so, eo in np.asarray(blocks).tolist():
        g = _fit(Y[:, sf:ef], act[:, sf:ef], iterations, load, weights, order, _defect, solve)
        out[:, so:eo] = g[:, so - sf:eo - sf]
    return out


def activity_pattern(K, T):
    """K = 2: speaker 0 on [0, 3T/5), speaker 1 on [2T/5, T) (T = 200: 120 and 80); otherwise speaker k on a window of
    2T / (K + 1) frames starting at k T / (K + 1): neighbours overlap by half."""
    act = np.zeros((K, T), dtype=np.uint8)
    if K == 2:
        act[0, :(3 * T) // 5] = 1
        act[1, (2 * T) // 5:] = 1
    elif K == 1:
        act[0, :max(1, (3 * T) // 5)] = 1
    else:
        for k in range(K):
            s = (k * T) // (K + 1)
            act[k, s:max(s + 1, ((k + 2) * T) // (K + 1))] = 1
    return act


def scene(seed, D=6, K=2, T=200, F=5, act=None):
    """-> (Y [D, T, F], act [K, T], on [K, T, F] bool, images [K, D, T, F]): K speakers with random steering vectors,
    each present in half of the tf points of its activity, noise 20 dB below a unit source."""
    rng = np.random.default_rng(seed)
    steer = rng.standard_normal((K, D, F)) + 1j * rng.standard_normal((K, D, F))
    act = activity_pattern(K, T) if act is None else np.asarray(act)
    on = (rng.random((K, T, F)) < 0.5) * act[:, :, None]
    S = (rng.standard_normal((K, T, F)) + 1j * rng.standard_normal((K, T, F))) * on
    images = steer[:, :, None, :] * S[:, None, :, :]
    noise = rng.standard_normal((D, T, F)) + 1j * rng.standard_normal((D, T, F))
    Y = images.sum(0) + 10 ** (-20 / 20) * noise
    return Y, act, on.astype(bool), images


def recovery(gamma, on):
    """fraction of the tf points with exactly one speaker or none present whose argmax_c gamma names that class"""
    K = on.shape[0]
    cnt = on.sum(0)
    truth = np.where(cnt == 0, K, on.argmax(0))
    sel = cnt <= 1
    return float((gamma.argmax(0)[sel] == truth[sel]).mean())


def spread(Y, act, iterations, **kw):
    """the largest change of the reference between its three summation orders"""
    g = [guided_cacgmm_reference(Y, act, iterations, order=o, **kw) for o in ORDERS]
    return max(float(np.abs(g[0] - x).max()) for x in g[1:]), g[0]


# ------------------------------------------------------------------------------------------ the GPU tests' cases
# Shared by tests/test_gpu_gss.py (kernel against reference) and tests/test_gss_reference.py (every planted defect moves
# the reference by more than the allowance at these shapes).  The kernel's tile is 64 frames and its chunk 256 = 4 * 64:
# T = 63, 64, 65 straddle the tile, T = 300 the chunk.  (D, K, T, F, variant), a sparse cover of D in {1, 2, 6, 8} x
# K in {1, 2, 8} x T in {1, 2, 63, 64, 65, 300} x F in {1, 5, 130}.
# T = 1 and T = 2 are paired with D = 1.  A sum of two terms has no order, so the yardstick is 0 by construction there and
# the allowance is the bare 4 * 2^-52.  With D >= 2 and fewer frames than channels every B_c is rank deficient before
# the load, its condition is D / load ~ 1e6, and two correct float64 evaluations (fused or unfused products, L^-1 as a
# product or as a substitution) differ by ~1e-13 in gamma without the order yardstick seeing any of it.  That shape has
# a test of its own (RANK_DEFICIENT_CASE, test_gpu_gss.py) against `rounding_yardstick` below, which perturbs more than
# the order: the reference itself moves by 1.4e-13 there when its channels are reversed.
MARGIN = 16.0
FLOOR = 4 * 2.0 ** -52
SEEDS = (0, 1, 2, 3)
RANK_DEFICIENT_CASE = (2, 2, 2, 5, "plain")
ONE_ITERATION_CASES = (
    (1, 1, 1, 1, "plain"), (1, 2, 2, 5, "plain"), (1, 2, 64, 5, "plain"), (2, 8, 65, 1, "plain"),
    (6, 2, 63, 5, "plain"), (6, 2, 64, 130, "plain"), (8, 8, 65, 5, "plain"), (6, 8, 300, 5, "plain"),
    (8, 1, 300, 1, "plain"), (6, 1, 300, 130, "plain"), (8, 2, 300, 5, "plain"),
    (6, 2, 65, 5, "silent_speaker"), (6, 2, 65, 5, "zero_frame"), (6, 2, 65, 5, "noise_only"),
)
TWENTY_ITERATION_CASES = (
    (6, 2, 200, 5, "plain"), (1, 1, 1, 1, "plain"), (2, 2, 64, 5, "plain"), (8, 8, 65, 5, "plain"),
    (6, 2, 300, 5, "zero_frame"),
)


def case_scene(case, seed):
    """-> (Y, act, on) of a case: the scene of `seed` at the case's shape with its variant applied"""
    D, K, T, F, variant = case
    Y, act, on, _ = scene(seed, D, K, T, F)
    if variant == "silent_speaker":
        act = act.copy()
        act[-1] = 0
    elif variant == "zero_frame":
        Y = Y.copy()
        Y[:, T // 2] = 0
    elif variant == "noise_only":
        act = np.zeros_like(act)
    else:
        assert variant == "plain", variant
    return Y, act, on


_YARDSTICKS = {}


def yardstick(case, iterations):
    """-> (the largest change of the reference over its three orders and the seeds 0-3 at this case, {seed: forward
    gamma}).  Computed once per (case, iterations); the arrays are read-only."""
    key = (case, iterations)
    if key not in _YARDSTICKS:
        worst, refs = 0.0, {}
        for seed in SEEDS:
            Y, act, _ = case_scene(case, seed)
            s, g = spread(Y, act, iterations)
            g.setflags(write=False)
            worst, refs[seed] = max(worst, s), g
        _YARDSTICKS[key] = (worst, refs)
    return _YARDSTICKS[key]


def allowance(case, iterations):
    return MARGIN * yardstick(case, iterations)[0] + FLOOR


def rounding_yardstick(case, iterations):
    """For a shape where the order yardstick is blind (T <= 2: a sum of two terms has no order): the largest change of
    the reference, seeds 0-3, under everything that changes its roundings and nothing else -- the three orders, L^-1 yh as
    a product with the explicit inverse, the Cholesky pivots carried in extended precision, the channels reversed, and
    every frame rescaled by a positive factor (gamma is invariant to both).  -> (yardstick, {seed: forward gamma})"""
    key = (case, iterations, "rounding")
    if key not in _YARDSTICKS:
        worst, refs = 0.0, {}
        for seed in SEEDS:
            Y, act, _ = case_scene(case, seed)
            scale = np.random.default_rng(1000 + seed).uniform(0.1, 10.0, size=(1,) + Y.shape[1:])
            s, g = spread(Y, act, iterations)
            for Yv, kw in ((Y, dict(solve="inverse")), (Y, dict(solve="extended_pivot")), (Y[::-1], {}), (Y * scale, {})):
                s = max(s, float(np.abs(guided_cacgmm_reference(Yv, act, iterations, **kw) - g).max()))
            g.setflags(write=False)
            worst, refs[seed] = max(worst, s), g
        _YARDSTICKS[key] = (worst, refs)
    return _YARDSTICKS[key]
