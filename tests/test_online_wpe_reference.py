"""The recursive WPE of DESIGN 4.19 restated in numpy -- the checker of tests/test_gpu_online_wpe.py, tested without a
GPU -- and what the Python layers refuse on the arguments alone.

`online_wpe_reference` runs, for every (b, f) and frame by frame (K = taps * D, yt[tau*D + d] = y_{t-delay-tau}[d] with
zeros in front of the stream, a = forgetting, c = power_context),

    p = sum_{s=t-c..t} sum_d |y_s[d]|^2 / (D (c + 1))      pmax = max(pmax, p) over the finite p
    pmax == 0: x = y, nothing is updated                   lam = max(p, 1e-10 pmax)
    x = y - G^H yt  (the output)       u = Q yt       den = a lam + Re(yt^H u)
    not (0 < den < inf): info += 1, nothing is updated     k = u / den
    Q = (Q - k u^H) / a  (lower triangle, mirrored, real diagonal; Q_0 = I / load)         G = G + k x^H

in float64 (extended=False) or one step above it (extended=True: np.longdouble or mpmath, `backend()` of
tests/test_mvdr_reference.py; complex numbers are pairs).  The state it returns and takes is the kernel's: Q is zeros while
pmax == 0, and a state of zeros is a fresh stream.

COMPARISON (`errors`, `yardsticks`): the error of an output element is |x - ext| / (|y_d| + sum_i |G_id| |yt_i|) (|ext|
itself will not do: a dereverberated frame is a cancellation), that of G_id is |g - ext| / max_i |G_id| (the column's
largest modulus), that of Q_ij is |q - ext| / sqrt(Q_ii Q_jj) (Q is positive definite); 0 / 0 = 0.  The yardsticks of a set
of inputs are the largest such errors of the float64 run against the extended run, a yardstick below 2^-52 (one rounding
on the element's scale) counts as 2^-52, and the kernel may be FACTOR = 8 times that far from the extended run at any
element (another but fixed summation order, fused multiply-adds, a product with 1 / a where the restatement divides).

The restatement itself is tied to the offline definition by `identity_residuals` (Q_T R_T = I, R_T G_T = P_T after 300
frames; the measured residuals are in test_recursion_solves_the_normal_equations's docstring)."""
import functools
import os

import numpy as np
import pytest
import torch

from test_mvdr_reference import backend, xf, xr

DEFECTS = ("posterior", "delay", "no_a", "no_conj", "stale_power", "a_first")
FACTOR = 8.0
FLOOR = 2.0 ** -52


def _conv(extended):
    return xr if extended else (lambda a: np.array(a, dtype=np.float64))


def _b(a):
    return np.asarray(a, dtype=bool)


def _finite(a):
    return np.isfinite(xf(a))


def fresh_state(B, D, F, taps, delay, power_context, extended):
    conv = _conv(extended)
    K, R = taps * D, max(delay + taps - 1, power_context)
    z = lambda *s: conv(np.zeros(s))
    return dict(Q=(z(B, F, K, K), z(B, F, K, K)), G=(z(B, F, K, D), z(B, F, K, D)),
                ring=np.zeros((B, F, R, D), dtype=np.complex128), pmax=z(B, F), info=np.zeros(B, dtype=np.int64))


def online_wpe_reference(Y, state=None, taps=10, delay=2, forgetting=0.99, load=1.0, power_context=0, extended=True,
                         defect=None):
    """Y [B,D,T,F] complex, state what an earlier call returned -> (x pair (re, im) [B,D,T,F] in the run's precision,
    state: dict(Q pair [B,F,K,K], G pair [B,F,K,D], ring complex128 [B,F,R,D], pmax [B,F], info int [B]),
    aux: dict(scale float64 [B,D,T,F], what an error of x is measured against; lam [T] of [B,F]; ok bool [T,B,F]))."""
    Y = np.asarray(Y, dtype=np.complex128)
    B, D, T, F = Y.shape
    K, c = taps * D, power_context
    R = max(delay + taps - 1, c)
    conv = _conv(extended)
    num = lambda v: conv(np.array([v]))[0]
    a, one, zero = num(forgetting), num(1.0), num(0.0)
    st = fresh_state(B, D, F, taps, delay, c, extended) if state is None else state
    pmax = st["pmax"].copy()
    eye = np.eye(K, dtype=bool)
    low = np.tril(np.ones((K, K), dtype=bool), -1)
    started = _b(pmax != 0)[..., None, None]
    Qr = np.where(started, st["Q"][0], np.where(eye, one / num(load), zero))
    Qi = np.where(started, st["Q"][1], zero)
    Gr, Gi = st["G"][0].copy(), st["G"][1].copy()
    info = st["info"].copy()
    # frames [B,F,1 + R + T,D]: one frame of zeros (the delay defect reaches it), the ring, the call
    hist = np.concatenate([np.zeros((B, F, 1, D), dtype=np.complex128), st["ring"], Y.transpose(0, 3, 2, 1)], axis=2)
    hr, hi = conv(hist.real), conv(hist.imag)
    habs = np.abs(hist)
    out_r, out_i = conv(np.zeros((B, D, T, F))), conv(np.zeros((B, D, T, F)))
    scale = np.zeros((B, D, T, F))
    lams, oks = [], []
    dl = delay + (1 if defect == "delay" else 0)
    pw = 1 if defect == "stale_power" else 0
    tsum = lambda M, axis: sum(np.take(M, i, axis=axis) for i in range(M.shape[axis]))       # a fixed order, any dtype
    with np.errstate(all="ignore"):
        for n in range(T):
            at = 1 + R + n
            lag = [max(at - dl - tau, 0) for tau in range(taps)]
            yr = np.concatenate([hr[:, :, l] for l in lag], axis=-1)                          # [B,F,K]
            yi = np.concatenate([hi[:, :, l] for l in lag], axis=-1)
            ya = np.concatenate([habs[:, :, l] for l in lag], axis=-1)
            cr, ci = hr[:, :, at], hi[:, :, at]                                               # y_t [B,F,D]
            p = zero
            for s in range(c, -1, -1):
                fr = max(at - pw - s, 0)
                for d in range(D):
                    p = p + (hr[:, :, fr, d] * hr[:, :, fr, d] + hi[:, :, fr, d] * hi[:, :, fr, d])
            p = p / num(float(D * (c + 1)))
            up = _b(p > pmax) & _finite(p)
            pmax = np.where(up, p, pmax)
            silent = _b(pmax == 0)
            flo = num(1e-10) * pmax
            lam = np.where(_b(p < flo), flo, p)

            def filt(Gr, Gi):
                xr_ = cr - tsum(Gr * yr[..., None] + Gi * yi[..., None], 2)                   # y - sum_i conj(G_id) yt_i
                xi_ = ci - tsum(Gr * yi[..., None] - Gi * yr[..., None], 2)
                sil = silent[..., None]
                return np.where(sil, cr, xr_), np.where(sil, ci, xi_)

            x_r, x_i = filt(Gr, Gi)
            ur = tsum(Qr * yr[..., None, :] - Qi * yi[..., None, :], 3)                      # [B,F,K]
            ui = tsum(Qr * yi[..., None, :] + Qi * yr[..., None, :], 3)
            den = (lam if defect == "no_a" else a * lam) + tsum(yr * ur + yi * ui, 2)
            ok = ~silent & _b(den > 0) & _finite(den)
            info += (~silent & ~ok).sum(axis=1)
            sden = np.where(ok, den, one)[..., None]
            kr, ki = ur / sden, ui / sden
            Nr = kr[..., :, None] * ur[..., None, :] + ki[..., :, None] * ui[..., None, :]    # k_i conj(u_j)
            Ni = ki[..., :, None] * ur[..., None, :] - kr[..., :, None] * ui[..., None, :]
            if defect == "a_first":
                Nr, Ni = Qr / a - Nr, Qi / a - Ni
            else:
                Nr, Ni = (Qr - Nr) / a, (Qi - Ni) / a
            Nr = np.where(low | eye, Nr, np.swapaxes(Nr, -1, -2))
            Ni = np.where(eye, zero, np.where(low, Ni, -np.swapaxes(Ni, -1, -2)))
            if defect == "no_conj":                                                          # k_i x_d
                dGr = kr[..., None] * x_r[..., None, :] - ki[..., None] * x_i[..., None, :]
                dGi = kr[..., None] * x_i[..., None, :] + ki[..., None] * x_r[..., None, :]
            else:                                                                            # k_i conj(x_d)
                dGr = kr[..., None] * x_r[..., None, :] + ki[..., None] * x_i[..., None, :]
                dGi = ki[..., None] * x_r[..., None, :] - kr[..., None] * x_i[..., None, :]
            sc = np.abs(hist[:, :, at]) + (np.hypot(xf(Gr), xf(Gi)) * ya[..., None]).sum(2)
            okk = ok[..., None, None]
            Qr, Qi = np.where(okk, Nr, Qr), np.where(okk, Ni, Qi)
            Gr, Gi = np.where(okk, Gr + dGr, Gr), np.where(okk, Gi + dGi, Gi)
            if defect == "posterior":
                x_r, x_i = filt(Gr, Gi)
            out_r[:, :, n], out_i[:, :, n] = x_r.transpose(0, 2, 1), x_i.transpose(0, 2, 1)
            scale[:, :, n] = np.where(silent[..., None], np.abs(hist[:, :, at]), sc).transpose(0, 2, 1)
            lams.append(lam)
            oks.append(ok)
    none = _b(pmax == 0)[..., None, None]
    new = dict(Q=(np.where(none, zero, Qr), np.where(none, zero, Qi)), G=(Gr, Gi),
               ring=np.ascontiguousarray(hist[:, :, 1 + T:]), pmax=pmax, info=info)
    return (out_r, out_i), new, dict(scale=scale, lam=lams, ok=np.array(oks).reshape(T, B, F))


# ---- the kernel's layout -------------------------------------------------------------------------------------------------
def tri_index(K):
    i, j = np.tril_indices(K)
    return i, j                                     # row by row: (i, j) at i (i + 1) / 2 + j


def pack_state(state):
    """the reference's state -> the kernel's five arrays (Q packed lower triangle [B,F,K(K+1)/2], G, ring, pmax, info)"""
    Q = xf(state["Q"][0]) + 1j * xf(state["Q"][1])
    i, j = tri_index(Q.shape[-1])
    return (Q[..., i, j], xf(state["G"][0]) + 1j * xf(state["G"][1]), state["ring"], xf(state["pmax"]),
            state["info"].astype(np.int32))


def unpack_q(tri, K):
    tri = np.asarray(tri)
    i, j = tri_index(K)
    Q = np.zeros(tri.shape[:-1] + (K, K), dtype=np.complex128)
    Q[..., j, i] = np.conj(tri)
    Q[..., i, j] = tri
    return Q


def _ratio(err, scale):
    with np.errstate(all="ignore"):
        r = err / scale
    r = np.where(err == 0, 0.0, r)
    return np.nan_to_num(r, nan=np.inf, posinf=np.inf)


def errors(X, Q, G, ref):
    """X complex [B,D,T,F], Q complex [B,F,K,K], G complex [B,F,K,D]; ref = online_wpe_reference(..., extended=True)
    -> the worst (output, G, Q) errors on the scales of the module docstring"""
    (er, ei), st, aux = ref
    ext = xf(er) + 1j * xf(ei)
    X, Q, G = np.asarray(X), np.asarray(Q), np.asarray(G)
    eo = _ratio(np.where(np.isfinite(X), np.abs(X - ext), np.inf), aux["scale"])
    Ge = xf(st["G"][0]) + 1j * xf(st["G"][1])
    eg = _ratio(np.where(np.isfinite(G), np.abs(G - Ge), np.inf), np.abs(Ge).max(axis=2, keepdims=True))
    Qe = xf(st["Q"][0]) + 1j * xf(st["Q"][1])
    dq = np.sqrt(np.abs(np.einsum("...ii->...i", Qe)))
    eq = _ratio(np.where(np.isfinite(Q), np.abs(Q - Qe), np.inf), dq[..., :, None] * dq[..., None, :])
    return float(eo.max()), float(eg.max()), float(eq.max())


def yardsticks(f64, ref):
    """the float64 run's own errors against the extended run, none below one rounding"""
    (xr_, xi_), st, _ = f64
    e = errors(xf(xr_) + 1j * xf(xi_), xf(st["Q"][0]) + 1j * xf(st["Q"][1]), xf(st["G"][0]) + 1j * xf(st["G"][1]), ref)
    return tuple(max(v, FLOOR) for v in e)


def held(X, Q, G, ref, ys, what):
    """(X, Q, G) against the extended run -> the three errors over their yardsticks"""
    e = errors(X, Q, G, ref)
    r = tuple(v / y for v, y in zip(e, ys))
    print(f"{what}: output {e[0]:.3g} = {r[0]:.3g} x the yardstick {ys[0]:.3g}; G {e[1]:.3g} = {r[1]:.3g} x {ys[1]:.3g}; "
          f"Q {e[2]:.3g} = {r[2]:.3g} x {ys[2]:.3g}")
    return r


def frames(B, D, T, F, seed):
    """Frames with a history: white complex noise under a slow envelope plus a decaying echo of the frames before, rounded
    to complex64 values (every input type of the kernel sees the same numbers) -> [B,D,T,F] complex128"""
    rs = np.random.RandomState(seed)
    Y = (rs.standard_normal((B, D, T, F)) + 1j * rs.standard_normal((B, D, T, F))) * \
        (0.3 + rs.random_sample((B, 1, T, F)) * 2.0)
    for t in range(1, T):
        Y[:, :, t] += 0.5 * Y[:, ::-1, t - 1]
    return Y.astype(np.complex64).astype(np.complex128)


SHAPES = ((1, 1, 0), (2, 3, 2), (3, 4, 1), (6, 10, 2), (8, 10, 3))      # (D, taps, delay): K = 1, 6, 12, 60, 80


@functools.lru_cache(maxsize=None)
def gpu_case(D, taps, delay, forgetting=1.0, power_context=0, B=2, F=5, T=None):
    """A case of tests/test_gpu_online_wpe.py -> Y, kw, the extended reference, the yardsticks (output, G, Q)"""
    T = delay + taps + 3 if T is None else T
    Y = frames(B, D, T, F, seed=100 * D + taps)
    kw = dict(taps=taps, delay=delay, forgetting=forgetting, load=0.5, power_context=power_context)
    ref = online_wpe_reference(Y, extended=True, **kw)
    return Y, kw, ref, yardsticks(online_wpe_reference(Y, extended=False, **kw), ref)


# ---- the reference itself ------------------------------------------------------------------------------------------------
def test_backend_is_extended():
    assert backend() in ("longdouble", "mpmath")


def _csolve(Ar, Ai, Br, Bi):
    """Gaussian elimination without exchanges (A is Hermitian positive definite) on pairs of any precision: A [K,K],
    B [K,M] -> X pair with A X = B"""
    Ar, Ai, Br, Bi = Ar.copy(), Ai.copy(), Br.copy(), Bi.copy()
    K = Ar.shape[0]
    for k in range(K):
        den = Ar[k, k] * Ar[k, k] + Ai[k, k] * Ai[k, k]
        fr = (Ar[k + 1:, k] * Ar[k, k] + Ai[k + 1:, k] * Ai[k, k]) / den
        fi = (Ai[k + 1:, k] * Ar[k, k] - Ar[k + 1:, k] * Ai[k, k]) / den
        for (Mr, Mi) in ((Ar, Ai), (Br, Bi)):
            rr, ri = Mr[k].copy(), Mi[k].copy()
            Mr[k + 1:] = Mr[k + 1:] - (fr[:, None] * rr[None] - fi[:, None] * ri[None])
            Mi[k + 1:] = Mi[k + 1:] - (fr[:, None] * ri[None] + fi[:, None] * rr[None])
    Xr, Xi = Br.copy(), Bi.copy()
    for k in range(K - 1, -1, -1):
        sr = Br[k] - sum(Ar[k, j] * Xr[j] - Ai[k, j] * Xi[j] for j in range(k + 1, K))
        si = Bi[k] - sum(Ar[k, j] * Xi[j] + Ai[k, j] * Xr[j] for j in range(k + 1, K))
        den = Ar[k, k] * Ar[k, k] + Ai[k, k] * Ai[k, k]
        Xr[k], Xi[k] = (sr * Ar[k, k] + si * Ai[k, k]) / den, (si * Ar[k, k] - sr * Ai[k, k]) / den
    return Xr, Xi


def _cmm(Ar, Ai, Br, Bi):
    f = lambda P, Q: sum(P[:, j, None] * Q[None, j] for j in range(P.shape[1]))
    return f(Ar, Br) - f(Ai, Bi), f(Ar, Bi) + f(Ai, Br)


def _resid(Rr, Ri, Xr, Xi, Pr, Pi):
    """the normwise relative residual max |R X - P| / (max |R| max |X| K + max |P|), in float64"""
    Mr, Mi = _cmm(Rr, Ri, Xr, Xi)
    res = np.hypot(xf(Mr - Pr), xf(Mi - Pi)).max()
    return res / (np.hypot(xf(Rr), xf(Ri)).max() * np.hypot(xf(Xr), xf(Xi)).max() * Rr.shape[0] +
                  np.hypot(xf(Pr), xf(Pi)).max())


def identity_residuals(Y, kw, extended):
    """One (b, f) stream Y [1,D,T,1]: R_T = a^T load I + sum_t a^(T-t) yt yt^H / lam_t, P_T = sum_t a^(T-t) yt y^H / lam_t
    from the frames and the run's own lam_t -> the residuals of (Q_T R_T = I, R_T G_T = P_T) of the recursion and of a direct
    solve in the same precision: ((rec_Q, rec_G), (direct_Q, direct_G))"""
    conv = _conv(extended)
    num = lambda v: conv(np.array([v]))[0]
    _, st, aux = online_wpe_reference(Y, extended=extended, **kw)
    assert aux["ok"].all()
    D, T = Y.shape[1], Y.shape[2]
    taps, delay, a = kw["taps"], kw["delay"], num(kw["forgetting"])
    K = taps * D
    y = Y[0, :, :, 0].T                                                                   # [T,D]
    Rr, Ri = conv(np.eye(K)) * num(kw["load"]), conv(np.zeros((K, K)))
    Pr, Pi = conv(np.zeros((K, D))), conv(np.zeros((K, D)))
    for t in range(T):
        yt = np.concatenate([y[t - delay - tau] if t - delay - tau >= 0 else np.zeros(D) for tau in range(taps)])
        tr, ti, cr, ci = conv(yt.real), conv(yt.imag), conv(y[t].real), conv(y[t].imag)
        lam = aux["lam"][t][0, 0]
        Rr = a * Rr + (tr[:, None] * tr[None] + ti[:, None] * ti[None]) / lam              # yt_i conj(yt_j)
        Ri = a * Ri + (ti[:, None] * tr[None] - tr[:, None] * ti[None]) / lam
        Pr = a * Pr + (tr[:, None] * cr[None] + ti[:, None] * ci[None]) / lam              # yt_i conj(y_d)
        Pi = a * Pi + (ti[:, None] * cr[None] - tr[:, None] * ci[None]) / lam
    Ir, Ii = conv(np.eye(K)), conv(np.zeros((K, K)))
    rec = (_resid(Rr, Ri, st["Q"][0][0, 0], st["Q"][1][0, 0], Ir, Ii),
           _resid(Rr, Ri, st["G"][0][0, 0], st["G"][1][0, 0], Pr, Pi))
    direct = (_resid(Rr, Ri, *_csolve(Rr, Ri, Ir, Ii), Ir, Ii), _resid(Rr, Ri, *_csolve(Rr, Ri, Pr, Pi), Pr, Pi))
    return rec, direct


@pytest.mark.parametrize("extended", (False, True))
@pytest.mark.parametrize("D,taps,delay", ((1, 1, 0), (2, 3, 2), (8, 10, 3)))
def test_recursion_solves_the_normal_equations(D, taps, delay, extended):
    """After T = 300 frames Q_T R_T = I and R_T G_T = P_T: the recursion is the offline definition (R G = P) with
    exponential weights and a loaded start, and this test of the restatement does not read the restatement's Q or G to
    form R and P.  The bound is FACTOR x the residual a direct elimination of the same system leaves in the same
    precision, on the normwise scale of `_resid`; a direct residual below one rounding of the precision counts as one.
    Measured (recursion / direct), float64: K = 1: Q 5.6e-17 / 5.6e-17, G 7.1e-17 / 0; K = 6: Q 7.3e-17 / 2.9e-17,
    G 1.1e-16 / 3.6e-17; K = 80: Q 2.7e-17 / 6.4e-18, G 4.9e-17 / 9.0e-18; extended (longdouble): K = 1: Q 2.7e-20 / 0,
    G 7.0e-20 / 0; K = 6: Q 6.4e-20 / 1.4e-20, G 7.2e-20 / 1.8e-20; K = 80: Q 1.5e-20 / 3.8e-21, G 3.5e-20 / 4.2e-21.  The
    recursion leaves 1 to 5.4 x what the direct solve leaves in float64; at K = 80 every direct residual on this scale
    (which carries the factor K) lies below one rounding of its precision, so there the floor is what binds, and the
    recursion stays below one rounding too."""
    Y = frames(1, D, 300, 1, seed=7 + D)
    kw = dict(taps=taps, delay=delay, forgetting=0.98, load=0.5, power_context=0)
    rec, direct = identity_residuals(Y, kw, extended)
    unit = float(np.finfo(np.longdouble).eps) / 2 if extended and backend() == "longdouble" else \
        (2.0 ** -113 if extended else 2.0 ** -53)
    print(f"K={taps * D} extended={extended}: Q {rec[0]:.3g} / {direct[0]:.3g}, G {rec[1]:.3g} / {direct[1]:.3g}")
    for r, d in zip(rec, direct):
        assert r <= FACTOR * max(d, unit), (rec, direct)


@pytest.mark.parametrize("extended", (False, True))
def test_split_invariance_of_the_reference(extended):
    D, taps, delay = 2, 3, 2
    T = 9
    Y = frames(2, D, T, 3, seed=11)
    kw = dict(taps=taps, delay=delay, forgetting=0.9, load=0.5, power_context=1, extended=extended)
    whole, sw, _ = online_wpe_reference(Y, **kw)
    for splits in ((1,) * T, (1, T - 1), (2, 1, 6), (delay + 1, T - delay - 1)):        # (2, 1, ..) ends inside the delay line
        parts, st, pos = [], None, 0
        for n in splits:
            x, st, _ = online_wpe_reference(Y[:, :, pos:pos + n], st, **kw)
            parts.append(x)
            pos += n
        assert pos == T
        for q in (0, 1):
            assert np.array_equal(np.concatenate([p[q] for p in parts], axis=2), whole[q]), splits
            assert np.array_equal(st["Q"][q], sw["Q"][q]) and np.array_equal(st["G"][q], sw["G"][q]), splits
        assert np.array_equal(st["ring"], sw["ring"]) and np.array_equal(st["pmax"], sw["pmax"])


def test_silent_start_of_the_reference():
    Y = frames(2, 2, 8, 3, seed=12)
    Y0 = np.concatenate([np.zeros_like(Y[:, :, :3]), Y], axis=2)
    kw = dict(taps=3, delay=1, forgetting=0.95, load=0.5, extended=False)
    lead, s0, _ = online_wpe_reference(Y0[:, :, :3], **kw)
    assert all((np.asarray(v) == 0).all() for v in pack_state(s0)) and (lead[0] == 0).all() and (lead[1] == 0).all()
    late, s1, _ = online_wpe_reference(Y0[:, :, 3:], s0, **kw)
    fresh, s2, _ = online_wpe_reference(Y, **kw)
    assert np.array_equal(late[0], fresh[0]) and np.array_equal(late[1], fresh[1])
    assert all(np.array_equal(p, q) for p, q in zip(pack_state(s1), pack_state(s2)))
    assert s2["info"].sum() == 0


def ar_observation(seed, D=2, taps=3, delay=1, T=400, F=4):
    """y_t = s_t + sum_tau C_tau^H y_{t-delay-tau}: a white source under a time-varying envelope, |C| small enough for a
    stable process -> Y [1,D,T,F], S [1,D,T,F]"""
    rs = np.random.RandomState(seed)
    C = 0.12 * (rs.standard_normal((taps, F, D, D)) + 1j * rs.standard_normal((taps, F, D, D)))
    env = 0.2 + np.abs(np.sin(np.arange(T) / 17.0 + rs.uniform(0, 6.0)))
    S = (rs.standard_normal((T, F, D)) + 1j * rs.standard_normal((T, F, D))) * env[:, None, None]
    Y = np.zeros((T, F, D), dtype=np.complex128)
    for t in range(T):
        Y[t] = S[t]
        for tau in range(taps):
            if t - delay - tau >= 0:
                Y[t] += np.einsum("fij,fi->fj", np.conj(C[tau]), Y[t - delay - tau])
    return Y.transpose(2, 0, 1)[None], S.transpose(2, 0, 1)[None]


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_dereverberation_of_an_autoregressive_observation(seed):
    """The late reverberation left over the second half, |x - s|^2 / |y - s|^2, is below 0.5.  Measured on these
    observations (|C_tau| entries of standard deviation 0.17, max |Y| 4.6 to 5.4): 0.19, 0.26, 0.19."""
    Y, S = ar_observation(seed)
    assert np.abs(Y).max() < 50 * np.abs(S).max()                                          # the process is stable
    (xr_, xi_), st, _ = online_wpe_reference(Y, taps=3, delay=1, forgetting=0.99, load=1.0, extended=False)
    X = xf(xr_) + 1j * xf(xi_)
    h = Y.shape[2] // 2
    left = (np.abs(X - S)[:, :, h:] ** 2).sum() / (np.abs(Y - S)[:, :, h:] ** 2).sum()
    print(f"seed {seed}: max |Y| {np.abs(Y).max():.3g}, late reverberation left {left:.3g}")
    assert left < 0.5 and st["info"].sum() == 0


@pytest.mark.parametrize("D,taps,delay", ((2, 3, 2), (6, 10, 2)))
def test_yardsticks_are_finite_and_planted_defects_exceed_them(D, taps, delay):
    """On the GPU test's own inputs the float64 run's distances from the extended one are finite, and each planted defect
    lies beyond FACTOR x a yardstick in the output, in G or in Q."""
    Y, kw, ref, ys = gpu_case(D, taps, delay, forgetting=0.9, power_context=2)
    print(f"D={D} taps={taps}: yardsticks output {ys[0]:.3g}, G {ys[1]:.3g}, Q {ys[2]:.3g}")
    assert all(FLOOR <= y < 1e-9 for y in ys), ys
    for defect in DEFECTS:
        (br, bi), st, _ = online_wpe_reference(Y, extended=False, defect=defect, **kw)
        r = held(xf(br) + 1j * xf(bi), xf(st["Q"][0]) + 1j * xf(st["Q"][1]), xf(st["G"][0]) + 1j * xf(st["G"][1]), ref, ys,
                 f"  {defect}")
        assert max(r) > FACTOR, (defect, r)
    (br, bi), st, _ = online_wpe_reference(Y, extended=False, **kw)
    r = held(xf(br) + 1j * xf(bi), xf(st["Q"][0]) + 1j * xf(st["Q"][1]), xf(st["G"][0]) + 1j * xf(st["G"][1]), ref, ys,
             "  none")
    assert max(r) <= 1.0


def test_pack_roundtrip():
    _, kw, ref, _ = gpu_case(2, 3, 2)
    tri, G, ring, pmax, info = pack_state(ref[1])
    Q = unpack_q(tri, 6)
    assert tri.shape == (2, 5, 21) and np.array_equal(Q, xf(ref[1]["Q"][0]) + 1j * xf(ref[1]["Q"][1]))
    assert np.array_equal(Q, np.conj(np.swapaxes(Q, -1, -2))) and ring.shape == (2, 5, 4, 2) and info.dtype == np.int32


# ---- refusals: CPU tensors, nothing is launched ----------------------------------------------------------------------
def _y(D=3, T=4, F=5, B=1, dtype=torch.complex64):
    return torch.randn(B, D, T, F, dtype=dtype)


def test_online_wpe_refusals():
    from tssep_amd import hip_ops
    assert hip_ops.online_wpe_check(_y(), taps=2) == (1, 3, 4, 5)
    with pytest.raises(TypeError, match="complex64 or complex128"):
        hip_ops.online_wpe(_y().real)
    with pytest.raises(ValueError, match="9 channels"):
        hip_ops.online_wpe(_y(D=9), taps=1)
    with pytest.raises(ValueError, match=r"taps \* channels = 27 \* 3 = 81"):
        hip_ops.online_wpe(_y(), taps=27)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="forgetting"):
            hip_ops.online_wpe(_y(), taps=2, forgetting=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="load"):
            hip_ops.online_wpe(_y(), taps=2, load=bad)
    with pytest.raises(ValueError, match="power_context"):
        hip_ops.online_wpe(_y(), taps=2, power_context=-1)
    with pytest.raises(ValueError, match="delay"):
        hip_ops.online_wpe(_y(), taps=2, delay=257)
    with pytest.raises(NotImplementedError, match="evaluation-time"):
        hip_ops.online_wpe(_y().requires_grad_(), taps=2)
    with pytest.raises(ValueError, match=r"\[B,D,Tc,F\]"):
        hip_ops.online_wpe(_y()[0], taps=2)


def _state(B=1, D=3, F=5, taps=2, delay=2, pc=0):
    from tssep_amd import hip_ops
    return hip_ops.OnlineWPEState(*(torch.zeros(s, dtype=dt) for s, dt in
                                    hip_ops.online_wpe_state_shapes(B, D, F, taps, delay, pc)))


def test_online_wpe_state_mismatch_is_named():
    from tssep_amd import hip_ops
    assert hip_ops.online_wpe_check(_y(), _state(), taps=2) == (1, 3, 4, 5)
    with pytest.raises(ValueError, match=r"state\.Q is torch\.complex128 \(1, 5, 3\)"):       # the state of a 1-channel stream
        hip_ops.online_wpe(_y(), _state(D=1), taps=2)
    with pytest.raises(ValueError, match=r"state\.ring is .*\(1, 5, 5, 3\)"):                # another power_context
        hip_ops.online_wpe(_y(), _state(pc=5), taps=2)
    with pytest.raises(ValueError, match=r"state\.ring"):                                    # another delay
        hip_ops.online_wpe(_y(), _state(delay=1), taps=2)
    with pytest.raises(ValueError, match=r"state\.pmax is torch\.float32"):
        hip_ops.online_wpe(_y(), _state()._replace(pmax=torch.zeros(1, 5)), taps=2)
    with pytest.raises(ValueError, match=r"state\.info"):
        hip_ops.online_wpe(_y(B=2), _state(B=2)._replace(info=torch.zeros(1, dtype=torch.int32)), taps=2)
    with pytest.raises(ValueError, match="OnlineWPEState"):
        hip_ops.online_wpe(_y(), torch.zeros(3), taps=2)


def test_size_query_is_host_only():
    from tssep_amd import _lib, hip_ops
    L = _lib.lib()
    for B, D, F, taps, delay, pc in ((1, 6, 513, 10, 2, 0), (2, 1, 5, 1, 0, 0), (2, 8, 5, 10, 3, 7), (1, 2, 3, 4, 256, 256)):
        want = sum(int(np.prod(s)) * torch.empty(0, dtype=dt).element_size()
                   for s, dt in hip_ops.online_wpe_state_shapes(B, D, F, taps, delay, pc))
        assert L.tssep_wpe_online_state_bytes(B, D, F, taps, delay, pc) == want
    for bad in ((1, 9, 5, 1, 0, 0), (1, 8, 5, 11, 0, 0), (1, 2, 5, 2, 257, 0), (1, 2, 5, 2, 0, 257), (1, 2, 5, 0, 0, 0),
                (1, 2, 5, 2, 0, -1)):
        assert L.tssep_wpe_online_state_bytes(*bad) == 0, bad


def test_enhancers_refuse_on_the_arguments():
    from tssep_amd.train import enhancer
    w = enhancer.OnlineWPE()
    assert (w.taps, w.delay, w.forgetting, w.load, w.power_context) == (10, 2, 0.99, 1.0, 0)
    with pytest.raises(TypeError, match="complex128 is required"):
        w(torch.zeros(3, 4, 5, dtype=torch.complex64))
    with pytest.raises(ValueError, match="9 channels"):
        w(np.zeros((9, 4, 5), dtype=np.complex128))
    with pytest.raises(NotImplementedError, match="evaluation-time"):
        w(torch.zeros(3, 4, 5, dtype=torch.complex128).requires_grad_())
    with pytest.raises(ValueError, match="forgetting"):
        enhancer.OnlineWPE(forgetting=0.0)(torch.zeros(3, 4, 5, dtype=torch.complex128))
    masks, Y = torch.rand(1, 2, 1, 4, 5), _y()
    with pytest.raises(NotImplementedError, match="OnlineWPE"), torch.no_grad():
        enhancer.OnlineMVDR(pre_wpe=enhancer.WPE())(masks, {"Observation": Y, "reference_channel": 0}, None)
    with pytest.raises(ValueError, match=r"taps \* channels"), torch.no_grad():
        enhancer.OnlineMVDR(pre_wpe=enhancer.OnlineWPE(taps=27))(masks, {"Observation": Y, "reference_channel": 0}, None)
    with pytest.raises(ValueError, match="the pair"):
        enhancer.OnlineMVDR(pre_wpe=w).chunk(masks, Y, torch.zeros(1, 2, 2, 9, 5, dtype=torch.float64), 0)


def test_configurable_round_trip_and_unchanged_defaults():
    from tssep_amd import configurable
    from tssep_amd.train import enhancer
    bf = enhancer.OnlineMVDR()
    assert bf.pre_wpe is None
    assert bf._kwargs() == dict(forgetting=1.0, diag_load=1e-6, eps=None, masking=False, masking_eps=0.0)
    assert enhancer.OnlineWPE.get_config() == {"factory": "tssep.train.enhancer.OnlineWPE", "taps": 10, "delay": 2,
                                               "forgetting": 0.99, "load": 1.0, "power_context": 0}
    cfg = enhancer.OnlineMVDR.get_config({"forgetting": 0.97, "pre_wpe": {"factory": "tssep.train.enhancer.OnlineWPE",
                                                                         "taps": 5, "power_context": 1}})
    assert cfg["pre_wpe"] == {"factory": "tssep.train.enhancer.OnlineWPE", "taps": 5, "delay": 2, "forgetting": 0.99,
                              "load": 1.0, "power_context": 1}
    made = configurable.Configurable.from_config(cfg)
    assert isinstance(made, enhancer.OnlineMVDR) and made.forgetting == 0.97 and isinstance(made.pre_wpe, enhancer.OnlineWPE)
    assert made.pre_wpe._kwargs() == dict(taps=5, delay=2, forgetting=0.99, load=1.0, power_context=1)
    assert enhancer.OnlineMVDR.get_config()["pre_wpe"] is None


def _model(enh):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import feature_extractor as fe, loss, model, net
    f = fe.ConcaternatedSTFTFeatures(
        fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True), size=1024, shift=256, window="hann")
    me = net.MaskEstimator_v2(combination="mul", ts_vad=3, rnn_typ="lstm", random_speaker_order=False, idim=553, odim=513,
                              units=8, projs=12, layers=3)
    return model.Model(fe=f, reader=DummyReader(), mask_estimator=me, enhancer=enh, loss=loss.LogMAE())


def test_model_online_accepts_the_pair():
    from tssep_amd.train import enhancer, online
    sep = _model(enhancer.OnlineMVDR(pre_wpe=enhancer.OnlineWPE(taps=4))).online(torch.zeros(2, 3, 513), reference_channel=1)
    assert isinstance(sep, online.OnlineSeparator) and sep._bf.pre_wpe.taps == 4 and sep._psd is None
    assert _model(enhancer.OnlineMVDR()).online(torch.zeros(2, 3, 513))._bf.pre_wpe is None


def test_toy_overlay_resolves():
    from tssep_amd.train import enhancer, online, run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
    yamls = ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_online_wpe.yaml")
    cfg = run.build_config([os.path.join(exp, y) for y in yamls] + ["eg.trainer.storage_dir=/tmp/unused"])
    model = Experiment.from_config(cfg["eg"]).trainer.model
    assert isinstance(model.enhancer, enhancer.OnlineMVDR) and isinstance(model.enhancer.pre_wpe, enhancer.OnlineWPE)
    assert model.enhancer.pre_wpe.taps == 10 and model.fe.causal and model.mask_estimator.rnn_typ == "lstm"
    assert isinstance(model.online(torch.zeros(1, 4, 513), reference_channel=1), online.OnlineSeparator)
