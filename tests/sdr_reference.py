"""float64 restatement of the SDR / SI-SDR loss (tssep_amd.train.loss.SDR, csrc/sdrloss.hip; semantics in DESIGN.md 4.15)
and the error bounds the CPU and the GPU tests share.  Per utterance b, estimate row i against target row j:

    a_i = sum e_i^2,  b_j = sum t_j^2,  c_ij = sum e_i t_j                        (sums over the N samples)
    scale-invariant: alpha = c / (b + eps), s = alpha c, n = a - s;   plain: s = b, n = max(a - 2 c + b, 0)
    D = n + tau s + eps,  tau = 10^(-sdr_max / 10) or 0
    value = 10 log10((s + eps) / D) dB,  cost = -value / K,  loss[b] = sum_i cost[b, i, perm_b(i)]
    gradient (perm fixed, t = tgt[b, perm(i)], g = gout[b] 20 / (K ln 10)):  dest = P e + Q t,
        scale-invariant P = g / D, Q = -g alpha (1 / (s + eps) + (1 - tau) / D);  plain P = g / D = -Q, 0 where n was clamped

Bounds.  The statistics kernel keeps float32 only in the per-lane chain acc = fma(x, y, acc) of at most ROUNDINGS =
SDR_CHUNK / 256 = 32 terms (the count its comment states; the products are exact inside the fma); wave tree, cross-wave
sum, stored partials and the chunk loop are float64 (2^-53 per operation: below 1e-6 of the float32 term, covered by
SLACK).  So, as tests/pit_reference.py derives its own, per statistic x = sum of terms:
    |dx| <= ROUNDINGS u sum |terms|        (u = 2^-24; for a and b the terms are non-negative)
propagated to first order:
    scale-invariant: dalpha = dc / (b + eps) + |c| db / (b + eps)^2,  ds = |alpha| dc + |c| dalpha,  dn = da + ds
    plain:           ds = db,  dn = da + 2 dc + db                    (the clamp moves n towards its true range)
    dD = dn + tau ds
    |dvalue| <= (10 / ln 10) (ds / (s + eps) + dD / D)  +  u |value|   (the final float32 rounding)
    |dcost|  <= |dvalue| / K  +  u |cost|
    dP = |P| dD / D,   dQ = g (dalpha |X| + |alpha| (ds / (s + eps)^2 + |1 - tau| dD / D^2)),  X = 1 / (s + eps) + (1 - tau) / D
    |ddest| <= |e| dP + |t| dQ + 3 u (|P e| + |Q t|)     (P, Q rounded once; fl(Q t); the fused multiply-add)
perm[b, i] is the TARGET row matched to estimate row i, found by brute force over itertools.permutations(range(K))."""
import numpy as np
import torch

import pit_reference as PR

U = 2.0 ** -24
CHUNK = 8192                   # SDR_CHUNK
ROUNDINGS = CHUNK // 256       # float32 roundings on the longest path into a statistic
SLACK = 1.0 + 1e-6             # the float64 operations behind the lane chain
LOG = 10.0 / np.log(10.0)


def tau_of(sdr_max):
    return 0.0 if sdr_max is None else 10.0 ** (-float(sdr_max) / 10.0)


def stats(est, tgt):
    """est, tgt [B, K, N] -> dict of float64 c [B,K,K], a [B,K], b [B,K] and cabs = sum |e_i t_j| [B,K,K]."""
    e, t = np.asarray(est, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    return dict(c=np.einsum("bin,bjn->bij", e, t), cabs=np.einsum("bin,bjn->bij", np.abs(e), np.abs(t)),
                a=(e * e).sum(-1), b=(t * t).sum(-1))


def flat_stats(st):
    """-> [B, K*K + 2K] in the kernels' layout: c_ij at i*K + j, then a_i, then b_j."""
    B, K = st["a"].shape
    return np.concatenate([st["c"].reshape(B, K * K), st["a"], st["b"]], axis=1)


def stat_bounds(st, roundings=ROUNDINGS):
    """-> the same layout: |dx| <= roundings u sum |terms|."""
    B, K = st["a"].shape
    return roundings * U * SLACK * np.concatenate([st["cabs"].reshape(B, K * K), st["a"], st["b"]], axis=1)


def decibels(c, a, b, scale_invariant=True, sdr_max=None, eps=1e-8, alpha_eps=True):
    """Broadcasting c, a, b -> dict(alpha, s, n, D, value, clamped).  alpha_eps=False: alpha = c / b, a planted defect."""
    tau = tau_of(sdr_max)
    c, a, b = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (c, a, b)))
    with np.errstate(divide="ignore", invalid="ignore"):
        if scale_invariant:
            alpha = c / (b + eps if alpha_eps else b)
            s = alpha * c
            n = a - s
        else:
            alpha = np.ones_like(c)
            s = b
            n = a - 2.0 * c + b
        clamped = n < 0
        n = np.where(clamped, 0.0, n)
        D = n + tau * s + eps
        value = 10.0 * np.log10((s + eps) / D)
    return dict(alpha=alpha, s=s, n=n, D=D, value=value, clamped=clamped, tau=tau, eps=eps)


def pair_values(st, scale_invariant=True, sdr_max=None, eps=1e-8, **kw):
    """-> decibels(...) on the K x K pairs: every array [B, K, K]."""
    return decibels(st["c"], st["a"][:, :, None], st["b"][:, None, :], scale_invariant, sdr_max, eps, **kw)


def value_terms(st, scale_invariant=True, sdr_max=None, eps=1e-8, roundings=ROUNDINGS):
    """-> (pair_values, dict of the propagated errors dalpha, ds, dD, dvalue), all [B, K, K]."""
    v = pair_values(st, scale_invariant, sdr_max, eps)
    r = roundings * U * SLACK
    dc, da, db = r * st["cabs"], r * st["a"][:, :, None], r * st["b"][:, None, :]
    b = st["b"][:, None, :]
    if scale_invariant:
        dalpha = dc / (b + eps) + np.abs(st["c"]) * db / (b + eps) ** 2
        ds = np.abs(v["alpha"]) * dc + np.abs(st["c"]) * dalpha
        dn = da + ds
    else:
        dalpha = np.zeros_like(dc)
        ds = db + np.zeros_like(dc)
        dn = da + 2.0 * dc + db
    dD = dn + v["tau"] * ds
    dvalue = LOG * (ds / (v["s"] + eps) + dD / v["D"]) + U * np.abs(v["value"])
    return v, dict(dalpha=dalpha, ds=ds, dD=dD, dvalue=dvalue)


def loss(est, tgt, scale_invariant=True, sdr_max=None, eps=1e-8, pit=False):
    """-> dict(value, dvalue, cost [B,K,K], perm [B,K], values [B,K] matched dB, loss [B], gap [B]).  The assignment is taken
    on the float32 rounding of the float64 costs (tssep_pit_assign's rule); gap = runner-up - optimum of the permutation
    sums of the costs, in float64 (inf for K = 1 or pit=False)."""
    st = stats(est, tgt)
    v, d = value_terms(st, scale_invariant, sdr_max, eps)
    K = v["value"].shape[-1]
    cost = -v["value"] / K
    perm, _ = PR.assign(cost.astype(np.float32), pit)
    matched = np.take_along_axis(v["value"], perm[..., None], axis=2)[..., 0]
    sums = np.sort(PR.permutation_sums(cost, np.float64), axis=1)
    gap = sums[:, 1] - sums[:, 0] if pit and sums.shape[1] > 1 else np.full(len(sums), np.inf)
    return dict(stats=st, value=v["value"], dvalue=d["dvalue"], cost=cost, perm=perm, values=matched,
                loss=-matched.sum(-1) / K, gap=gap)


def coefficients(st, perm, scale_invariant=True, sdr_max=None, eps=1e-8, tau_in_gradient=True, inv_k=True, alpha_eps=True,
                 roundings=ROUNDINGS):
    """P, Q [B, K] of dest = gout (P e_i + Q t_perm(i)) (gout excluded) and their bounds dP, dQ.  tau_in_gradient=False,
    inv_k=False, alpha_eps=False: planted defects (the factor (1 - tau) dropped; 1/K dropped; alpha = c / b)."""
    perm = np.asarray(perm)
    B, K = perm.shape
    take = lambda x: np.take_along_axis(x, perm[..., None], axis=2)[..., 0]      # noqa: E731
    c, cabs, a, b = take(st["c"]), take(st["cabs"]), st["a"], np.take_along_axis(st["b"], perm, axis=1)
    v = decibels(c, a, b, scale_invariant, sdr_max, eps, alpha_eps=alpha_eps)
    tau, s, D, alpha = v["tau"], v["s"], v["D"], v["alpha"]
    g = 20.0 / ((K if inv_k else 1) * np.log(10.0))
    r = roundings * U * SLACK
    dc, da, db = r * cabs, r * a, r * b
    if scale_invariant:
        X = 1.0 / (s + eps) + ((1.0 - tau) if tau_in_gradient else 1.0) / D
        P, Q = g / D, -g * alpha * X
        dalpha = dc / (b + eps) + np.abs(c) * db / (b + eps) ** 2
        ds = np.abs(alpha) * dc + np.abs(c) * dalpha
        dD = da + ds + tau * ds
        dP = np.abs(P) * dD / D
        dQ = g * (dalpha * np.abs(X) + np.abs(alpha) * (ds / (s + eps) ** 2 + abs(1.0 - tau) * dD / D ** 2))
    else:
        P = np.where(v["clamped"], 0.0, g / D)
        Q = -P
        dD = da + 2.0 * dc + db + tau * db
        dP = dQ = np.abs(P) * dD / D
    return P, Q, dP, dQ


def grad(est, tgt, perm, scale_invariant=True, sdr_max=None, eps=1e-8, gout=None, inverse_perm=False, **defects):
    """The closed-form gradient in float64 -> (dest [B,K,N], its element-wise bound).  inverse_perm: the target rows taken
    through the inverse permutation, a planted defect."""
    e, t = np.asarray(est, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    perm = np.asarray(perm)
    used = PR.inverse(perm) if inverse_perm else perm
    P, Q, dP, dQ = coefficients(stats(e, t), used, scale_invariant, sdr_max, eps, **defects)
    go = np.ones(len(e)) if gout is None else np.asarray(gout, dtype=np.float64)
    tm = np.take_along_axis(t, used[..., None], axis=1)
    pe, qt = P[..., None] * e, Q[..., None] * tm
    dest = go[:, None, None] * (pe + qt)
    bound = np.abs(go)[:, None, None] * (np.abs(e) * dP[..., None] + np.abs(tm) * dQ[..., None]
                                         + 3 * U * (np.abs(pe) + np.abs(qt)))
    return dest, bound


def autograd(est, tgt, perm, scale_invariant=True, sdr_max=None, eps=1e-8, gout=None):
    """The plain formula in float64 torch and its autograd gradient -> (value [B,K] matched dB, loss [B], d(sum gout loss)/d est)."""
    e = torch.tensor(np.asarray(est), dtype=torch.float64, requires_grad=True)
    t = torch.as_tensor(np.asarray(tgt), dtype=torch.float64)
    idx = torch.as_tensor(np.asarray(perm), dtype=torch.int64)[..., None].expand_as(t)
    tm = torch.gather(t, 1, idx)
    a, b, c = (e * e).sum(-1), (tm * tm).sum(-1), (e * tm).sum(-1)
    tau = tau_of(sdr_max)
    if scale_invariant:
        s = c / (b + eps) * c
        n = a - s
    else:
        s = b
        n = torch.clamp(a - 2 * c + b, min=0)
    value = 10 * torch.log10((s + eps) / (n + tau * s + eps))
    lo = -value.mean(-1)
    g = torch.ones_like(lo) if gout is None else torch.as_tensor(np.asarray(gout), dtype=torch.float64)
    (lo * g).sum().backward()
    return value.detach().numpy(), lo.detach().numpy(), e.grad.numpy()


# ------------------------------------------------------------------------------------------------ checkers
def _check(what, got, ref, bound):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bad = ~(err <= bound)                                # (a NaN fails)
    ratio = err / np.maximum(bound, 1e-300)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} outside the bound, worst {float(np.nanmax(ratio[bad])):.3g} x"
    return float(ratio.max()) if ratio.size else 0.0


def check_stats(got, st, diag_only=False, roundings=ROUNDINGS):
    """got [B, K*K + 2K] (or chunk partials summed by the caller) against the float64 statistics -> worst error / bound."""
    ref, bound = flat_stats(st), stat_bounds(st, roundings)
    if diag_only:
        B, K = st["a"].shape
        off = np.concatenate([~np.eye(K, dtype=bool).reshape(-1), np.zeros(2 * K, dtype=bool)])
        assert np.all(np.asarray(got)[:, off] == 0), "diag_only: an off-diagonal c entry was written"
        ref, bound = np.where(off, 0.0, ref), np.where(off, 0.0, bound)
    return _check("statistics", got, ref, bound)


def check_values(value, cost, ref, diag_only=False):
    """value, cost [B,K,K] float32 against loss(...)'s dict -> worst error / bound of the two."""
    K = ref["value"].shape[-1]
    want_v, want_c = ref["value"], ref["cost"]
    bv = ref["dvalue"]
    bc = bv / K + U * np.abs(want_c)
    if diag_only:
        eye = np.eye(K, dtype=bool)[None]
        assert np.all(np.asarray(value)[:, ~eye[0]] == 0) and np.all(np.asarray(cost)[:, ~eye[0]] == 0)
        want_v, want_c, bv, bc = (np.where(eye, x, 0.0) for x in (want_v, want_c, bv, bc))
    return max(_check("value", value, want_v, bv), _check("cost", cost, want_c, bc))


def check_backward(got, est, tgt, perm, scale_invariant, sdr_max, eps, gout):
    ref, bound = grad(est, tgt, perm, scale_invariant, sdr_max, eps, gout)
    return _check("gradient", got, ref, bound)


def planted(B, K, N, level_db, seed, scale=1.0):
    """tgt ~ N(0, scale^2), est = tgt + noise with the noise orthogonalised against its target row and scaled so that
    the plain SDR and the SI-SDR of every matched row are level_db (up to eps) -> float32 (est, tgt)."""
    rng = np.random.RandomState(seed)
    tgt = scale * rng.randn(B, K, N)
    noise = rng.randn(B, K, N)
    noise -= (noise * tgt).sum(-1, keepdims=True) / (tgt * tgt).sum(-1, keepdims=True) * tgt
    noise *= np.sqrt((tgt * tgt).sum(-1, keepdims=True) / (noise * noise).sum(-1, keepdims=True)) * 10.0 ** (-level_db / 20.0)
    return (tgt + noise).astype(np.float32), tgt.astype(np.float32)
