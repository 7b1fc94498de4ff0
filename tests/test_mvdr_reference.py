"""The extended-precision checker of the MVDR kernels (tests/test_gpu_mvdr_kernels.py), tested without a GPU: references,
bound functions and input generators of the three stages of csrc/mvdr.hip (statistics, per-bin solve, filtering) and of the
segment-wise statistics.  The kernels work in float64, so the references work one step above it: np.longdouble where it has
a 64-bit significand, mpmath (113 bits) otherwise -- `backend()` decides, everything extended goes through `xr` / `xf`, and
complex numbers are pairs (re, im) of real arrays so that both back ends run the same lines.  U = 2^-53.

Layout (`pack_hermitian`): per (b, chunk, k, m) D*D rows of F doubles: rows 0..D-1 the real diagonal, then for every pair
i < j in row-major order the rows Re M[i,j], Im M[i,j].  m = 0 is the target PSD X, m = 1 the interference PSD A.

SOLVE.  The kernels eliminate [A | X] with row exchanges (pivot: the FIRST maximum of |re| + |im| in the column, LAPACK's
rule), then substitute backwards; Phi = A^-1 X.  `lu_reference` does the same in extended precision and returns Phi, the
factors L, U of P A, the exchange record and the flag "a pivot column was exactly zero".  Bound, componentwise (Higham,
Accuracy and Stability, Thm 9.4 with the constants of this code):
    |X - A Phi^| <= GAMMA(D) (|L| |U| |Phi^|),   GAMMA(D) = g / (1 - g),  g = (3 (D - 1) + 2 C_DIV + C_MUL) U
  * a complex product (4 products, 2 sums; an FMA only removes roundings) is (1 + e), |e| <= C_MUL U, C_MUL = 2 sqrt 2
    (Higham Lemma 3.5: sqrt 2 gamma_2); a complex sum (1 + e), |e| <= U.
  * crecip(a), |a.x| >= |a.y|: r = a.y / a.x (1 rounding), den = a.x + a.y r (2, no cancellation: both terms have the sign
    of a.x), 1 / den (1), -r / den (1 more): each component within 5 U relative.  The quotient is then a complex product
    with that reciprocal: C_DIV = 5 + 2 sqrt 2 where a true division would cost one rounding.
  * elimination: every entry of L U = P A is a chain of at most D multiply-subtracts: a term carries its product (C_MUL)
    and at most D - 1 subtractions, the last one of a multiplier carries the reciprocal (C_DIV) instead:
    |P A - L^ U^| <= (D - 1 + C_DIV) U |L^| |U^|.
  * the right-hand side is eliminated alongside (unit diagonal, no division): |dL| <= (D - 1 + C_MUL) U |L^|; the
    back substitution multiplies by crecip(u_ii): |dU| <= (D - 1 + C_DIV) U |U^|.  Thm 9.4 adds the three.
  Under the |re| + |im| rule a pivot is the largest of its column in the 1-norm of (re, im), not in modulus, so the
  multipliers satisfy |l| <= sqrt 2, not 1 (7 / (3 + 4i) has modulus 1.4: the `ties` generator).  Nothing above assumes
  |l| <= 1: the multipliers enter through |L| itself, and `test_multipliers_stay_below_sqrt2` holds the reference to sqrt 2.
  |L| |U| is taken from the reference's factors: the theorem states it for the computed ones, which differ in second order.
  The forward error may only be asserted through the condition of A: |Phi^ - Phi| <= |A^-1| (backward bound)
  (`forward_bound`); a fixed rtol against LAPACK means nothing at cond 1e9.
  D = 6: GAMMA = 33.5 U = 3.7e-15.

STATISTICS.  One chunk of n frames: |err| <= GAMMA_n(n + 4) sum_t |w| |y_i| |y_j| + n 2^-1074: per term two products and
their sum (2; |a.x b.x| + |a.y b.y| <= |a| |b|), the weight (1), 1 - w for M = 1 (1), then at most n additions; joining c
chunks adds c - 1.  2^-1074 per term: subnormal masks put products below the normal range.  GAMMA_n(k) = k U / (1 - k U).
Segment statistics add the slices joined, the two roundings of (1 / len) * sum, and the error of the weight itself where it
is a power: x * x in the mask's type is what numpy computes too; pow / powf are OpenCL's 16 ulp of the mask's type.

APPLY.  Each component of sum_d w_d y_d: 2 products, their sum, D additions: GAMMA_n(D + 2) sum_d |w_d| |y_d|; the mask
product adds one rounding.

SENSITIVITY (test_planted_defects_exceed_the_bound).  The same elimination in float64 with one defect passes through the
solve bound on `graded` + `rank1`, D = 6; the clean float64 run stays below 1.  Worst |residual| / bound:
    clean 0.05 (0.14 at D = 2)   no row exchanges 1.0e+08   exchange not applied to X 3.0e+12
    exchange on columns >= p of X only 8.6e+12   one upper-triangle imaginary part with the wrong sign 1.5e+14
    back substitution one term short 2.7e+14
No exchanges is still a valid elimination, and on a positive definite matrix a backward stable one (growth factor 1): no
residual can tell it from the real thing there.  It shows on the indefinite half of `rank1` (65 of 260 systems outside),
and on `indefinite`, whose zero diagonal makes it divide by zero."""
import math

import numpy as np
import pytest

U = 2.0 ** -53
C_MUL = 2.0 * math.sqrt(2.0)
C_DIV = 5.0 + 2.0 * math.sqrt(2.0)
DENORM = 2.0 ** -1074
POW_ULPS = 16.0
GAINS = (0.05, 0.3, 1.0, 3.0, 10.0, 30.0, 0.1, 100.0)
_FORCE = [None]         # the tests of the fallback put "mpmath" here


# ---- extended precision ------------------------------------------------------------------------------------------------
def backend():
    if _FORCE[0]:
        return _FORCE[0]
    return "longdouble" if np.finfo(np.longdouble).eps <= 2.0 ** -63 else "mpmath"


def xr(a):
    """float array -> extended real array (exact)"""
    a = np.asarray(a)
    if backend() == "longdouble":
        return a.astype(np.longdouble)
    import mpmath
    mpmath.mp.prec = 113
    return np.frompyfunc(lambda v: mpmath.mpf(float(v)), 1, 1)(a.astype(np.float64)).astype(object)


def xf(a):
    """extended -> float64"""
    return np.asarray(a, dtype=np.float64)


def xc(z):
    """complex128 array -> extended pair"""
    z = np.asarray(z)
    return xr(z.real), xr(z.imag)


def xcf(p):
    return xf(p[0]) + 1j * xf(p[1])


def cmul(a, b):
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def cdiv(a, b):
    den = b[0] * b[0] + b[1] * b[1]
    return (a[0] * b[0] + a[1] * b[1]) / den, (a[1] * b[0] - a[0] * b[1]) / den


def gamma_n(k):
    return k * U / (1.0 - k * U)


def solve_gamma(D):
    g = (3.0 * (D - 1) + 2.0 * C_DIV + C_MUL) * U
    return g / (1.0 - g)


# ---- layout ------------------------------------------------------------------------------------------------------------
def pack_hermitian(M):
    """[..., F, D, D] complex -> [..., D*D, F] float64 rows (diagonal; Re, Im of the strict upper triangle row by row)"""
    M = np.asarray(M)
    D = M.shape[-1]
    rows = [M[..., i, i].real for i in range(D)]
    for i in range(D):
        for j in range(i + 1, D):
            rows += [M[..., i, j].real, M[..., i, j].imag]
    return np.ascontiguousarray(np.stack(rows, -2), dtype=np.float64)


def unpack_hermitian(rows, D):
    """[..., D*D, F] -> [..., F, D, D] complex128, the lower triangle the conjugate of the upper"""
    rows = np.asarray(rows)
    M = np.zeros(rows.shape[:-2] + (rows.shape[-1], D, D), dtype=np.complex128)
    p = 0
    for i in range(D):
        M[..., i, i] = rows[..., i, :]
        for j in range(i + 1, D):
            v = rows[..., D + 2 * p, :] + 1j * rows[..., D + 2 * p + 1, :]
            M[..., i, j], M[..., j, i] = v, v.conj()
            p += 1
    return M


def make_plan(B, K, T, F):
    """the chunking of the statistics pass (make_plan of mvdr.hip, the same double arithmetic) -> chunks, tchunk"""
    nf = (F + 63) // 64
    per_chunk = B * nf * ((K + 3) // 4)
    cmax = min((T + 15) // 16, 256)
    best_c, best = 1, 1e300
    for c in range(1, cmax + 1):
        frames = (T + c - 1) // c
        rounds = (per_chunk * c + 511) // 512
        cost = float(rounds) * float(frames + 8) + 0.5 * float(c)
        if cost < best:
            best, best_c = cost, c
    tchunk = (T + best_c - 1) // best_c
    return (T + tchunk - 1) // tchunk, tchunk


def apply_plan(B, K, T, F):
    """launch_apply's chunking -> achunks, tchunk"""
    tiles = B * ((F + 63) // 64) * ((K + 3) // 4)
    c = max(1, min((4096 + tiles - 1) // tiles, (T + 15) // 16))
    tchunk = (T + c - 1) // c
    return (T + tchunk - 1) // tchunk, tchunk


def seg_slices(S, F):
    return max(1, min(16, (4096 + S * ((F + 63) // 64) - 1) // (S * ((F + 63) // 64))))


# ---- the reference elimination -------------------------------------------------------------------------------------------
DEFECTS = ("noswap", "x_noswap", "x_partial", "sign", "short")


def lu_reference(A, X, extended=True, defect=None):
    """A, X [n, D, D] complex128 -> dict(phi (pair, [n, D, D]), L, U complex128, piv [n, D] the row chosen at every step,
    singular [n]).  extended=False: the same lines in float64 (for the planted defects)."""
    A, X = np.asarray(A, dtype=np.complex128), np.asarray(X, dtype=np.complex128)
    n, D = A.shape[0], A.shape[-1]
    conv = xr if extended else (lambda a: np.array(a, dtype=np.float64))
    if defect == "sign" and D > 1:
        A = A.copy()
        A[:, 0, 1] = A[:, 0, 1].conj()
    Wr, Wi, Yr, Yi = conv(A.real), conv(A.imag), conv(X.real), conv(X.imag)
    one, zero = conv(np.ones(1))[0], conv(np.zeros(1))[0]
    idx = np.arange(n)
    piv = np.zeros((n, D), dtype=np.int64)
    singular = np.zeros(n, dtype=bool)
    for p in range(D):
        score = np.abs(Wr[:, p:, p]) + np.abs(Wi[:, p:, p])
        best = np.zeros(n, dtype=np.int64)
        for i in range(1, D - p):                                   # the FIRST maximum: strictly larger only
            best = np.where(score[idx, i] > score[idx, best], i, best)
        singular |= np.asarray(score[idx, best] == 0, dtype=bool)
        q = p + best if defect != "noswap" else np.full(n, p)
        piv[:, p] = q
        for M in (Wr, Wi):
            t = M[idx, p].copy()
            M[idx, p] = M[idx, q]
            M[idx, q] = t
        if defect != "x_noswap":
            c0 = p if defect == "x_partial" else 0
            for M in (Yr, Yi):
                t = M[idx, p, c0:].copy()
                M[idx, p, c0:] = M[idx, q, c0:]
                M[idx, q, c0:] = t
        dr, di = Wr[:, p, p].copy(), Wi[:, p, p].copy()
        z = np.asarray((dr == 0) & (di == 0), dtype=bool)
        dr[z] = one
        if p + 1 < D:
            l = cdiv((Wr[:, p + 1:, p], Wi[:, p + 1:, p]), (dr[:, None], di[:, None]))
            Wr[:, p + 1:, p], Wi[:, p + 1:, p] = l
            l = (l[0][:, :, None], l[1][:, :, None])
            ur, ui = cmul(l, (Wr[:, p, None, p + 1:], Wi[:, p, None, p + 1:]))
            Wr[:, p + 1:, p + 1:] -= ur
            Wi[:, p + 1:, p + 1:] -= ui
            yr, yi = cmul(l, (Yr[:, p, None, :], Yi[:, p, None, :]))
            Yr[:, p + 1:] -= yr
            Yi[:, p + 1:] -= yi
    for i in range(D - 1, -1, -1):
        sr, si = Yr[:, i].copy(), Yi[:, i].copy()
        for q in range(i + 1, D - 1 if defect == "short" and i < D - 1 else D):
            tr, ti = cmul((Wr[:, i, q, None], Wi[:, i, q, None]), (Yr[:, q], Yi[:, q]))
            sr, si = sr - tr, si - ti
        dr, di = Wr[:, i, i].copy(), Wi[:, i, i].copy()
        z = np.asarray((dr == 0) & (di == 0), dtype=bool)
        dr[z] = one
        Yr[:, i], Yi[:, i] = cdiv((sr, si), (dr[:, None], di[:, None]))
    W = xf(Wr) + 1j * xf(Wi)
    return dict(phi=(Yr, Yi), L=np.tril(W, -1) + np.eye(D), U=np.triu(W), piv=piv, singular=singular, zero=zero)


def residual(A, X, phi_hat):
    """X - A phi_hat in extended precision -> float64 |.| of the real and of the imaginary part, [n, D, D] each"""
    Ar, Ai = xc(A)
    Pr, Pi = xc(phi_hat)
    Rr, Ri = xc(X)
    D = np.asarray(A).shape[-1]
    for k in range(D):
        tr, ti = cmul((Ar[:, :, k, None], Ai[:, :, k, None]), (Pr[:, None, k, :], Pi[:, None, k, :]))
        Rr, Ri = Rr - tr, Ri - ti
    return np.abs(xf(Rr)), np.abs(xf(Ri))


def solve_bound(lu, phi_hat):
    """GAMMA(D) (|L| |U| |phi_hat|), rows in the order of A (the factors are those of P A: the exchanges are undone)"""
    n, D = lu["piv"].shape
    b = solve_gamma(D) * (np.abs(lu["L"]) @ np.abs(lu["U"]) @ np.abs(np.asarray(phi_hat)))
    idx = np.arange(n)
    for p in range(D - 1, -1, -1):
        q = lu["piv"][:, p]
        t = b[idx, p].copy()
        b[idx, p] = b[idx, q]
        b[idx, q] = t
    return b


def solve_ratio(A, X, phi_hat, lu=None):
    """worst |X - A phi_hat| / bound per system (0 / 0 counts as 0), over the regular systems"""
    lu = lu or lu_reference(A, X)
    rr, ri = residual(A, X, phi_hat)
    b = solve_bound(lu, phi_hat)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.maximum(rr, ri) / b
    r = np.where((b == 0) & (np.maximum(rr, ri) == 0), 0.0, r)
    r = np.where(np.isfinite(np.asarray(phi_hat)).all((-2, -1), keepdims=True), r, np.inf)
    return np.where(lu["singular"], 0.0, np.nan_to_num(r, nan=np.inf).max((-2, -1)))


def forward_bound(A, lu, phi_hat):
    """|A^-1| (backward bound): what |phi_hat - Phi| may be"""
    D = A.shape[-1]
    inv = xcf(lu_reference(A, np.broadcast_to(np.eye(D, dtype=np.complex128), A.shape))["phi"])
    return np.abs(inv) @ solve_bound(lu, phi_hat)


# ---- generators (seeded) -----------------------------------------------------------------------------------------------
def cyclic_gains(D, rs):
    """GAINS[:D] in descending order sent through a random single D-cycle: selection by size exchanges at every step"""
    g = np.sort(np.array(GAINS[:D]))[::-1]
    order = rs.permutation(D)                       # the cycle order[0] -> order[1] -> ... -> order[0]
    out = np.empty(D)
    out[order] = g[np.roll(order, -1)]
    return out


def graded_mixture(D, T, F, seed, K=2, offset=0.0):
    """Two correlated sources on D channels of unequal gain (a random cyclic arrangement of GAINS per bin), a noise floor of
    1e-3 before the gain, speaker masks from the sources' shares -> Y [D, T, F] complex128, masks [K, T, F] float64."""
    rs = np.random.RandomState(seed)
    S = (rs.standard_normal((2, T, F)) + 1j * rs.standard_normal((2, T, F))) * (rs.random_sample((2, T, F)) < 0.7)
    h = np.exp(2j * np.pi * rs.random_sample((D, 2, F))) * (0.5 + rs.random_sample((D, 2, F)))
    noise = 1e-3 * (rs.standard_normal((D, T, F)) + 1j * rs.standard_normal((D, T, F)))
    g = np.stack([cyclic_gains(D, rs) for _ in range(F)], -1)                      # [D, F]
    Y = g[:, None, :] * (np.einsum("dsf,stf->dtf", h, S) + noise) + offset
    p = np.abs(S) ** 2 + 1e-3
    share = p[0] / (p[0] + p[1])
    masks = np.stack([share if k % 2 == 0 else 1 - share for k in range(K)])
    masks = masks * (0.5 + 0.5 * rs.random_sample((K, 1, F)))
    return Y, masks


def psd_float64(w, Y):
    """sum_t w[t, f] Y[:, t, f] Y[:, t, f]^H -> [F, D, D]"""
    return np.einsum("tf,dtf,etf->fde", w, Y, Y.conj())


def _herm(M):
    M = (M + np.swapaxes(M.conj(), -2, -1)) / 2
    i = np.arange(M.shape[-1])
    M[..., i, i] = M[..., i, i].real
    return M


def _crandn(rs, *shape):
    return rs.standard_normal(shape) + 1j * rs.standard_normal(shape)


def gen_graded(D, n, seed):
    F = (n + 1) // 2
    Y, m = graded_mixture(D, max(24, 3 * D), F, seed)
    A = np.concatenate([psd_float64(1 - m[k], Y) for k in (0, 1)])[:n]
    X = np.concatenate([psd_float64(m[k], Y) for k in (0, 1)])[:n]
    return _herm(A), _herm(X)


def gen_rank1(D, n, seed, lo=3.0, hi=12.0, mixed=True):
    """A = Q diag(+-(1 .. 1 / cond)) Q^H, cond log-uniform over 1e3 .. 1e12 (evenly spread, shuffled); X = a a^H + 1e-6 I.
    The first half of the systems is positive definite; the second half (mixed) has eigenvalues of both signs: on a
    positive definite matrix elimination WITHOUT exchanges is backward stable too (growth factor 1), so only an
    indefinite one can tell a kernel that never exchanges rows from one that does."""
    rs = np.random.RandomState(seed)
    Q = np.linalg.qr(_crandn(rs, n, D, D))[0]
    cond = 10.0 ** rs.permutation(np.linspace(lo, hi, n))
    lam = cond[:, None] ** (-np.arange(D) / max(D - 1, 1))
    if mixed and D > 1:
        sign = np.where(rs.random_sample((n, D)) < 0.5, -1.0, 1.0)
        sign[:, 0], sign[:, 1] = 1.0, -1.0
        sign[:n // 2] = 1.0
        lam = lam * sign
    A = _herm(np.einsum("nij,nj,nkj->nik", Q, lam, Q.conj()))
    if mixed and D > 1:
        A[n // 2:, 0, 0] *= 2.0 ** -24              # ... and a leading entry far below its column
    a = _crandn(rs, n, D)
    return A, _herm(a[:, :, None] * a[:, None, :].conj() + 1e-6 * np.eye(D))


def gen_indefinite(D, n, seed):
    """Hermitian, not PSD, zero diagonal (D = 1: a negative number): no elimination without exchanges"""
    rs = np.random.RandomState(seed)
    A = _herm(_crandn(rs, n, D, D))
    i = np.arange(D)
    A[:, i, i] = 0.0 if D > 1 else -1.0 - rs.random_sample((n, 1))
    X = _herm(_crandn(rs, n, D, D))
    X[:, i, i] -= 0.25 * D                          # traces of either sign
    return A, X


def gen_ties(D, n, seed):
    """column 0 below a diagonal of 5: 3+4i, 4+3i, 7, -7, 7i, ... all with |re| + |im| = 7; the first one wins"""
    rs = np.random.RandomState(seed)
    A = _herm(np.round(4 * _crandn(rs, n, D, D)))
    tie = [3 + 4j, 4 + 3j, 7, -7, 7j, -4 + 3j, 3 - 4j]
    A[:, 0, 0] = 5
    for i in range(1, D):
        A[:, i, i] += 40
        A[:, i, 0] = tie[i - 1]
        A[:, 0, i] = np.conj(tie[i - 1])
    return A, _herm(_crandn(rs, n, D, D))


def gen_exactsing(D, n, seed):
    """every third system singular with entries 0, +-2, 4, so that the elimination is exact and meets an exact zero pivot:
    the zero matrix, a zero row and column, two equal rows; the rest regular -> A, X, singular [n] bool"""
    rs = np.random.RandomState(seed)
    A, X = gen_rank1(D, n, seed, 0.5, 2.0, mixed=False)
    sing = np.zeros(n, dtype=bool)
    for s in range(0, n, 3):
        kind = (s // 3) % 3 if D > 1 else 0
        M = np.diag(np.full(D, 4.0)).astype(np.complex128)
        if kind == 0:
            M[:] = 0
        elif kind == 1:
            j = rs.randint(D)
            M[j, j] = 0
        else:
            i = rs.randint(D - 1)
            M[i:i + 2, i:i + 2] = [[2, 2], [2, 2]] if s % 2 else [[2, 2j], [-2j, 2]]
        A[s], sing[s] = M, True
    return A, X, sing


def gen_scaled(D, n, seed, e):
    A, X = gen_graded(D, n, seed)
    return np.ldexp(A.real, e) + 1j * np.ldexp(A.imag, e), np.ldexp(X.real, e) + 1j * np.ldexp(X.imag, e)


REGULAR = {"graded": gen_graded, "rank1": gen_rank1, "indefinite": gen_indefinite, "ties": gen_ties}


# ---- statistics and filtering --------------------------------------------------------------------------------------------
def stats_reference(Y, w0, w1, t0, t1):
    """Y [D, T, F], w0, w1 [T, F] (any float type, taken exactly) over frames [t0, t1) -> (pair [2, F, D, D] extended,
    S [2, F, D, D] float64 = sum_t |w| |y_i| |y_j|)"""
    Yr, Yi = xc(Y[:, t0:t1])
    D, F = Y.shape[0], Y.shape[2]
    out_r = np.empty((2, F, D, D), dtype=Yr.dtype)
    out_i = np.empty((2, F, D, D), dtype=Yr.dtype)
    S = np.empty((2, F, D, D))
    mod = np.abs(Y[:, t0:t1])
    for m, w in enumerate((w0, w1)):
        w = np.asarray(w)
        wx = xr(w[t0:t1].astype(np.float64)) if w.dtype in (np.float32, np.float64) else w[t0:t1]    # else: extended already
        wa = np.abs(xf(wx))
        for i in range(D):
            for j in range(D):
                pr, pi = cmul((Yr[i], Yi[i]), (Yr[j], -Yi[j]))
                out_r[m, :, i, j] = (wx * pr).sum(0) if t1 > t0 else xr(np.zeros(F))
                out_i[m, :, i, j] = (wx * pi).sum(0) if t1 > t0 else xr(np.zeros(F))
                S[m, :, i, j] = (wa * mod[i] * mod[j]).sum(0)
    return (out_r, out_i), S


def stats_bound(S, n, joined=0, extra=0.0):
    """n frames in the chunk, `joined` further additions, `extra` a relative error of the weights themselves"""
    return (gamma_n(n + 4 + joined) + extra) * S + max(n, 1) * DENORM


def apply_reference(Y, w, mask=None, masking_eps=0.0):
    """Y [D, T, F], w [D, F] complex128 (the stored conj(bf)), mask [T, F] or None -> (enh complex128 [T, F] rounded from
    extended, bound [T, F] per component)"""
    Yr, Yi = xc(Y)
    wr, wi = xc(w)
    D = Y.shape[0]
    er, ei = cmul((wr[:, None], wi[:, None]), (Yr, Yi))
    e = xcf((er.sum(0), ei.sum(0)))
    S = (np.abs(w)[:, None] * np.abs(Y)).sum(0)
    if mask is None:
        return e, gamma_n(D + 2) * S + DENORM
    mk = np.maximum(np.asarray(mask, dtype=np.float64), masking_eps)
    ex = xcf((er.sum(0) * xr(mk), ei.sum(0) * xr(mk)))
    return ex, gamma_n(D + 3) * S * mk + DENORM


def segment_weights(masks, k, mode, dist_eps, power):
    """the two weights of speaker k the way ClassicBF_np forms them, in the masks' own type: masks [K, T, F] ->
    w_target, w_distortion [T, F] float64 (exact values of that type), relative error allowed for the power"""
    mt = masks.dtype.type
    tgt = masks[k]
    if mode == "sum_cross_talker":
        dist = np.zeros_like(tgt)
        for j in range(masks.shape[0]):
            if j != k:
                dist = dist + masks[j]
        dist = np.maximum(dist, mt(dist_eps))
    else:
        dist = np.maximum(mt(1) - tgt, mt(0))
    extra = 0.0
    if power == 2:
        tgt, dist = tgt * tgt, dist * dist
    elif power != 1:
        tgt, dist = tgt ** mt(power), dist ** mt(power)
        extra = (POW_ULPS + 1) * 2.0 * float(np.finfo(masks.dtype).eps) / 2
    return tgt.astype(np.float64), dist.astype(np.float64), extra


# ---- tests of the above on the CPU ---------------------------------------------------------------------------------------
N_CPU = 130


def test_backend_is_extended():
    assert backend() in ("longdouble", "mpmath")
    one = xr(np.ones(1))
    assert xf((one + xr(np.array([2.0 ** -60]))) - one)[0] == 2.0 ** -60


def test_mpmath_fallback_agrees_with_longdouble():
    """both back ends through the same lines: Phi of a few graded systems agrees to the shorter significand"""
    A, X = gen_graded(4, 6, 3)
    try:
        _FORCE[0] = "mpmath"
        a = lu_reference(A, X)
        pa = xcf(a["phi"])
        ra = residual(A, X, pa)
        _FORCE[0] = "longdouble"
        b = lu_reference(A, X)
        rb = residual(A, X, pa)                     # of the same float64 matrix
    finally:
        _FORCE[0] = None
    assert (a["piv"] == b["piv"]).all() and a["phi"][0].dtype == object
    assert (np.maximum(*ra) <= solve_bound(a, pa)).all()       # Phi rounded to float64: a backward error of U at most
    if np.finfo(np.longdouble).eps <= 2.0 ** -63:
        assert np.abs(pa - xcf(b["phi"])).max() <= 1e-6 * np.abs(pa).max()
        for x, y in zip(ra, rb):
            assert (np.abs(x - y) <= 2.0 ** -60 * (np.abs(A) @ np.abs(pa))).all()


@pytest.mark.parametrize("D", range(1, 9))
def test_pack_roundtrip_and_positions(D):
    rs = np.random.RandomState(D)
    M = _herm(_crandn(rs, 2, 5, D, D))
    rows = pack_hermitian(M)
    assert rows.shape == (2, D * D, 5) and rows.dtype == np.float64
    assert np.array_equal(unpack_hermitian(rows, D), M)
    assert np.array_equal(rows[:, D - 1], M[..., D - 1, D - 1].real)
    if D > 2:       # pair (1, 2) follows the D - 1 pairs of row 0
        assert np.array_equal(rows[:, D + 2 * (D - 1) + 1], M[..., 1, 2].imag)


@pytest.mark.parametrize("D", range(2, 9))
def test_graded_exchanges_rows_at_every_step(D):
    A, X = gen_graded(D, N_CPU, 100 + D)
    lu = lu_reference(A, X)
    assert not lu["singular"].any()
    swapped = lu["piv"] != np.arange(D)
    print(D, "exchanges per system", swapped.sum(1).mean(), "cond", np.linalg.cond(A).min(), np.linalg.cond(A).max())
    for p in range(D - 1):
        assert swapped[:, p].mean() >= 0.5, (D, p, swapped[:, p].mean())
        assert set(lu["piv"][:, p]) >= set(range(p + 1, D)), (D, p, set(lu["piv"][:, p]))


def test_graded_is_as_ill_conditioned_as_array_data():
    A, _ = gen_graded(6, N_CPU, 106)
    c = np.linalg.cond(A)
    assert c.min() > 1e7 and c.max() < 1e13, (c.min(), c.max())


@pytest.mark.parametrize("D", (2, 6, 8))
def test_rank1_spreads_the_condition(D):
    A, X = gen_rank1(D, N_CPU, 7)
    c = np.log10(np.linalg.cond(A))
    assert c.min() < 3.5 and c.max() > 11.5 and set(np.floor(c).astype(int)) >= set(range(3, 12)), (c.min(), c.max())
    assert (np.linalg.matrix_rank(X - 1e-6 * np.eye(D), tol=1e-9) == 1).all()


@pytest.mark.parametrize("D", range(1, 9))
def test_indefinite_needs_the_exchanges_and_ties_take_the_first(D):
    A, X = gen_indefinite(D, 40, D)
    lu = lu_reference(A, X)
    assert not lu["singular"].any() and (np.linalg.eigvalsh(A).min(1) < 0).all()
    tr = np.trace(xcf(lu["phi"]), axis1=-2, axis2=-1).real
    assert D == 1 or ((tr < 0).any() and (tr > 0).any())
    if D > 1:
        assert (lu["piv"][:, 0] != 0).all()
        A, X = gen_ties(D, 40, D)
        lu = lu_reference(A, X)
        assert (lu["piv"][:, 0] == 1).all() and not lu["singular"].any()
        if D > 3:
            assert np.abs(lu["L"][:, :, 0]).max() == pytest.approx(1.4)


@pytest.mark.parametrize("D", range(1, 9))
def test_exactsing_count_is_known(D):
    A, X, sing = gen_exactsing(D, 40, 50 + D)
    lu = lu_reference(A, X)
    assert np.array_equal(lu["singular"], sing) and sing.sum() == 14
    assert np.array_equal(lu_reference(A, X, extended=False)["singular"], sing)         # exact in float64 too


def test_multipliers_stay_below_sqrt2():
    worst = 0.0
    for D in (3, 6, 8):
        for name, gen in REGULAR.items():
            lu = lu_reference(*gen(D, 60, 11))
            worst = max(worst, np.abs(np.tril(lu["L"], -1)).max())
    assert 1.0 < worst <= math.sqrt(2.0) * (1 + 1e-12), worst


@pytest.mark.parametrize("D", range(1, 9))
def test_clean_reference_against_lapack(D):
    A, X = gen_rank1(D, 50, 9, 0.0, 2.0)
    lu = lu_reference(A, X)
    want = np.linalg.solve(A, X)
    assert np.abs(xcf(lu["phi"]) - want).max() <= 1e-11 * np.abs(want).max()
    P = np.abs(lu["L"] @ lu["U"])
    assert np.abs(np.sort(P.reshape(50, -1), 1) - np.sort(np.abs(A).reshape(50, -1), 1)).max() < 1e-12   # L U = P A
    assert solve_ratio(A, X, xcf(lu["phi"]), lu).max() <= 1.0


def _sensitivity_set(D=6):
    a, b = gen_graded(D, N_CPU, 100 + D), gen_rank1(D, N_CPU, 7)
    return np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])


def test_float64_elimination_passes_the_bound():
    for D in (2, 6, 8):
        A, X = _sensitivity_set(D)
        r = solve_ratio(A, X, xcf(lu_reference(A, X, extended=False)["phi"]))
        print("clean float64, D =", D, r.max())
        assert r.max() <= 1.0, r.max()


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_exceed_the_bound(defect):
    A, X = _sensitivity_set()
    with np.errstate(all="ignore"):
        bad = xcf(lu_reference(A, X, extended=False, defect=defect)["phi"])
    r = solve_ratio(A, X, bad)
    print(defect, "worst", r.max(), "systems outside", int((r > 1).sum()), "of", r.size)
    assert r.max() > 1.0, (defect, r.max())


def test_forward_bound_covers_float64_and_follows_the_condition():
    A, X = _sensitivity_set()
    lu = lu_reference(A, X)
    got = xcf(lu_reference(A, X, extended=False)["phi"])
    fb = forward_bound(A, lu, got)
    err = np.abs(got - xcf(lu["phi"]))
    assert (err <= fb).all()
    rel = fb.max((-2, -1)) / np.abs(got).max((-2, -1))
    c = np.linalg.cond(A)
    assert rel[c > 1e10].min() > 1e-9 > rel[c < 1e5].max() * 1e-3       # an rtol of 1e-8 could not be asserted everywhere


def test_statistics_and_apply_bounds_hold_for_float64_numpy():
    Y, m = graded_mixture(5, 13, 7, 4, offset=40.0)
    w0 = m[0].astype(np.float32)
    w0[0], w0[1], w0[2] = 0.0, 1.0, 1e-42
    w1 = 1.0 - w0.astype(np.float64)
    ref, S = stats_reference(Y, w0, w1, 2, 13)
    got = np.stack([psd_float64(w.astype(np.float64)[2:], Y[:, 2:]) for w in (w0, w1)])
    b = stats_bound(S, 11)
    assert (np.abs(got.real - xf(ref[0])) <= b).all() and (np.abs(got.imag - xf(ref[1])) <= b).all()
    assert b.max() < 1e-11 * np.abs(got).max()
    short = np.stack([psd_float64(w.astype(np.float64)[2:12], Y[:, 2:12]) for w in (w0, w1)])      # a frame missing
    assert (np.abs(short.real - xf(ref[0])) > b).any()
    w = _crandn(np.random.RandomState(1), 5, 7)
    e, eb = apply_reference(Y, w, m[0], 0.4)
    got = np.einsum("df,dtf->tf", w, Y) * np.maximum(m[0], 0.4)
    assert (np.abs(got.real - e.real) <= eb).all() and (np.abs(got.imag - e.imag) <= eb).all()
    assert (np.abs((got / np.maximum(m[0], 0.4) * m[0]).real - e.real) > eb).any()                  # the clamp missing


def test_plans_restate_the_host_code():
    from tssep_amd import _lib
    L = _lib.lib()
    for B, K, D, T, F in [(1, 1, 2, 1, 1), (1, 3, 3, 17, 65), (3, 9, 6, 70, 129), (1, 8, 6, 96, 65), (1, 4, 4, 300, 129),
                          (2, 8, 6, 1878, 513)]:
        chunks, tchunk = make_plan(B, K, T, F)
        assert L.tssep_mvdr_partial_bytes(B, K, D, T, F) == B * chunks * K * 2 * D * D * F * 8
        assert (chunks - 1) * tchunk < T <= chunks * tchunk
    assert make_plan(1, 1, 16, 1) == (1, 16) and make_plan(1, 1, 64, 1)[0] == 4
    assert seg_slices(1, 17) == 16 and seg_slices(4096, 1) == 1 and seg_slices(600, 1) == 7
