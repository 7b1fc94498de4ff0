"""The checker of the MVDR backward (tests/test_gpu_mvdr_backward.py), tested without a GPU: the analytic backward of
TorchBF.__call__ in extended precision, stage by stage, a torch float64 restatement of that call for autograd, input
generators, and the layout of the backward's workspace.  Extended numbers are those of tests/test_mvdr_reference.py (`R`):
pairs (re, im) of np.longdouble (or mpmath) arrays.

Forward, per (k, f), y_t in C^D:  Phi_s = sum_t m_s y y^H, Phi_n = sum_t m_n y y^H (m_n = 1 - m_s for M = 1, formed
exactly), P = Phi_n^-1 Phi_s, lam = Re tr P, c = max(lam, eps), w = P[:, ref] / c, e = w^H y, enh = e g,
g = max(m_s, masking_eps) with masking, else 1.
Backward for G = d(loss)/d(enh), torch's convention (dL = Re sum conj(G) d enh):
  stage 1   gw = sum_t conj(G g) y_t
  stage 2   gP = (gw / c) e_ref^T + gc I, gc = -Re(gw^H P[:, ref]) / c^2 if lam >= eps else 0;
            Z = Phi_n^-H gP;  Hs = herm(Z), Hn = herm(-Z P^H)
  stage 3   dm_s = Re(y^H Hs y) + [m_s >= masking_eps] Re(conj(e) G),  dm_n = Re(y^H Hn y);  M = 1: dm = dm_s - dm_n
`extended_backward` returns every stage.  test_extended_backward_matches_autograd holds it to CPU autograd of the
restatement on every shape of the GPU file's grid (GRID; one batch element, at most 9 bins); test_planted_defects_fail shows that the comparison sees a dropped -Z P^H term,
a missing conjugate in gw, `>` for `>=` at the masking clamp (masks exactly at masking_eps) and the trace term kept when
lam < eps.

Workspace of the backward (tssep_mvdr_bwd_workspace_bytes): doubles [B][chunks][K][2 D][F] (rows Re gw_d, Im gw_d; chunks
of R.make_plan), rounded up to 16 bytes, then [B][K][M][D D][F] packed Hermitian (R.pack_hermitian)."""
import math

import numpy as np
import pytest
import torch

import test_mvdr_reference as R

TINY = float(np.finfo(np.float64).tiny)
DEFECTS = ("no_zph", "gw_conj", "clamp_gt", "trace_kept")


# ---- extended helpers ----------------------------------------------------------------------------------------------------
def xsolve(A, Bm):
    """A, Bm pairs of extended [n, D, D] / [n, D, C] -> A^-1 Bm (pair), Gaussian elimination with partial pivoting"""
    Ar, Ai, Br, Bi = A[0].copy(), A[1].copy(), Bm[0].copy(), Bm[1].copy()
    n, D = Ar.shape[0], Ar.shape[1]
    idx = np.arange(n)
    for p in range(D):
        score = R.xf(np.abs(Ar[:, p:, p]) + np.abs(Ai[:, p:, p]))
        q = p + np.argmax(score, axis=1)
        for Mx in (Ar, Ai, Br, Bi):
            t = Mx[idx, p].copy()
            Mx[idx, p] = Mx[idx, q]
            Mx[idx, q] = t
        if p + 1 < D:
            l = R.cdiv((Ar[:, p + 1:, p], Ai[:, p + 1:, p]), (Ar[:, p, p, None], Ai[:, p, p, None]))
            l = (l[0][:, :, None], l[1][:, :, None])
            ur, ui = R.cmul(l, (Ar[:, p, None, :], Ai[:, p, None, :]))
            Ar[:, p + 1:] -= ur
            Ai[:, p + 1:] -= ui
            br, bi = R.cmul(l, (Br[:, p, None, :], Bi[:, p, None, :]))
            Br[:, p + 1:] -= br
            Bi[:, p + 1:] -= bi
    for i in range(D - 1, -1, -1):
        sr, si = Br[:, i].copy(), Bi[:, i].copy()
        for q in range(i + 1, D):
            tr, ti = R.cmul((Ar[:, i, q, None], Ai[:, i, q, None]), (Br[:, q], Bi[:, q]))
            sr, si = sr - tr, si - ti
        Br[:, i], Bi[:, i] = R.cdiv((sr, si), (Ar[:, i, i, None], Ai[:, i, i, None]))
    return Br, Bi


def xmatmul(a, b, conj_b_transposed=False):
    """pairs [n, D, E] x [n, E, C] -> [n, D, C];  conj_b_transposed: a b^H with b [n, C, E]"""
    if conj_b_transposed:
        b = (np.swapaxes(b[0], -2, -1), -np.swapaxes(b[1], -2, -1))
    E = a[0].shape[-1]
    out_r = out_i = 0
    for q in range(E):
        tr, ti = R.cmul((a[0][:, :, q, None], a[1][:, :, q, None]), (b[0][:, None, q, :], b[1][:, None, q, :]))
        out_r, out_i = out_r + tr, out_i + ti
    return out_r, out_i


def xherm(z):
    two = R.xr(np.full(1, 2.0))[0]
    return (z[0] + np.swapaxes(z[0], -2, -1)) / two, (z[1] - np.swapaxes(z[1], -2, -1)) / two


def xquad(H, Yr, Yi):
    """Re(y_t^H H y_t): H pair [F, D, D], Y [D, T, F] extended -> [T, F]"""
    D = Yr.shape[0]
    q = 0
    for i in range(D):
        for j in range(D):
            pr, pi = R.cmul((Yr[i], -Yi[i]), (Yr[j], Yi[j]))            # conj(y_i) y_j
            q = q + H[0][None, :, i, j] * pr - H[1][None, :, i, j] * pi
    return q


def extended_solve_stage(X, A, gw, ref, eps, M, defect=None):
    """X (target), A (interference) pairs [n, D, D] (R.xc of a complex128 array), gw pair [n, D] ->
    dict(P, lam, c, Hs, Hn), pairs"""
    n, D = X[0].shape[0], X[0].shape[-1]
    P = xsolve(A, X)
    lam = sum(P[0][:, i, i] for i in range(D))
    open_ = np.asarray(lam >= R.xr(np.full(1, eps))[0], dtype=bool)
    c = np.where(open_, lam, R.xr(np.full(1, eps))[0])
    if defect == "trace_kept":
        open_ = np.ones_like(open_)
    u = (gw[0] / c[:, None], gw[1] / c[:, None])
    dot = (gw[0] * P[0][:, :, ref] + gw[1] * P[1][:, :, ref]).sum(1)
    gc = np.where(open_, -dot / (c * c), R.xr(np.zeros(1))[0])
    gPr, gPi = R.xr(np.zeros((n, D, D))), R.xr(np.zeros((n, D, D)))
    gPr[:, :, ref], gPi[:, :, ref] = u
    for i in range(D):
        gPr[:, i, i] = gPr[:, i, i] + gc
    AH = (np.swapaxes(A[0], -2, -1).copy(), -np.swapaxes(A[1], -2, -1))
    Zm = xsolve(AH, (gPr, gPi))
    ZP = xmatmul(Zm, P, conj_b_transposed=True)
    Hs, Hn = xherm(Zm), xherm((-ZP[0], -ZP[1]))
    if defect == "no_zph":
        Hn = (Hn[0] * 0, Hn[1] * 0)
    mod = lambda z: float(np.max(np.hypot(R.xf(z[0]), R.xf(z[1]))))      # noqa: E731
    return dict(P=P, lam=lam, c=c, Hs=Hs, Hn=Hn, scale=(mod(Zm), mod(ZP)))


def extended_gw(Y, mask_s, G, masking, meps, defect=None):
    """Y [D, T, F] complex128, mask_s [T, F] (exact), G [T, F] complex128 -> gw pair [F, D]"""
    Yr, Yi = R.xc(Y)
    g = R.xr(np.maximum(np.asarray(mask_s, dtype=np.float64), meps)) if masking else R.xr(np.ones(mask_s.shape))
    Gr, Gi = R.xc(G)
    Ger, Gei = Gr * g, (Gi if defect == "gw_conj" else -Gi) * g                     # conj(Ge)
    pr, pi = R.cmul((Ger[None], Gei[None]), (Yr, Yi))
    return pr.sum(1).T, pi.sum(1).T


def extended_dmask(Y, mask_s, G, w, Hs, Hn, M, masking, meps, defect=None):
    """w pair [F, D] (the beamformer, not conjugated), Hs, Hn pairs [F, D, D] -> dmask extended [M, T, F]"""
    Yr, Yi = R.xc(Y)
    if M == 1:
        out = [xquad((Hs[0] - Hn[0], Hs[1] - Hn[1]), Yr, Yi)]
    else:
        out = [xquad(Hs, Yr, Yi), xquad(Hn, Yr, Yi)]
    if masking:
        er, ei = R.cmul((w[0].T[:, None, :], -w[1].T[:, None, :]), (Yr, Yi))
        er, ei = er.sum(0), ei.sum(0)
        Gr, Gi = R.xc(G)
        m64 = np.asarray(mask_s, dtype=np.float64)
        on = (m64 > meps) if defect == "clamp_gt" else (m64 >= meps)
        out[0] = out[0] + np.where(on, er * Gr + ei * Gi, R.xr(np.zeros(1))[0])
    return np.stack(out)


def extended_backward(Y, masks, G, ref, eps, masking, meps, defect=None):
    """One batch element: Y [D, T, F] complex128, masks [K, M, T, F] float32 | float64, G [K, T, F] complex128 ->
    dict(gw pair [K, F, D], Hs, Hn pairs [K, F, D, D], dmask extended [K, M, T, F], lam float64 [K, F], w pair [K, F, D],
    scale: what the errors of a stage are measured against -- the largest |gw|, |Z|, |Z P^H| (herm(Z) may cancel to
    nothing: at D = 1 without masking the whole gradient is zero) and, for dmask, D max|y|^2 (max|Z| + max|Z P^H|) plus
    the largest masking term)"""
    K, M, T, F = masks.shape
    D = Y.shape[0]
    meps = float(np.asarray(meps, dtype=masks.dtype))          # torch.clamp compares in the mask's dtype
    out = dict(gw=[], Hs=[], Hn=[], dmask=[], lam=[], w=[])
    zs = zp = 0.0
    for k in range(K):
        w0 = masks[k, 0]
        w1 = masks[k, 1] if M == 2 else R.xr(np.ones(1))[0] - R.xr(w0.astype(np.float64))
        (Sr, Si), _ = R.stats_reference(Y, w0, w1, 0, T)
        gw = extended_gw(Y, w0, G[k], masking, meps, defect)
        st = extended_solve_stage((Sr[0], Si[0]), (Sr[1], Si[1]), gw, ref, eps, M, defect)      # the statistics stay extended
        w = (st["P"][0][:, :, ref] / st["c"][:, None], st["P"][1][:, :, ref] / st["c"][:, None])
        zs, zp = max(zs, st["scale"][0]), max(zp, st["scale"][1])
        out["gw"].append(gw)
        out["Hs"].append(st["Hs"])
        out["Hn"].append(st["Hn"])
        out["w"].append(w)
        out["lam"].append(R.xf(st["lam"]))
        out["dmask"].append(extended_dmask(Y, w0, G[k], w, st["Hs"], st["Hn"], M, masking, meps, defect))
    res = {key: (np.stack([v[0] for v in out[key]]), np.stack([v[1] for v in out[key]])) for key in ("gw", "Hs", "Hn", "w")}
    res["dmask"], res["lam"] = np.stack(out["dmask"]), np.stack(out["lam"])
    y2 = float(np.max(np.abs(Y))) ** 2
    mterm = float(np.max(np.abs(R.xcf(res["w"])))) * D * math.sqrt(y2) * float(np.max(np.abs(G))) if masking else 0.0
    res["scale"] = dict(gw=float(np.max(np.abs(R.xcf(res["gw"])))), Hs=zs, Hn=zp, dmask=D * y2 * (zs + zp) + mterm)
    return res


# ---- the torch float64 restatement ---------------------------------------------------------------------------------------
def torch_bf(masks, Y, ref, eps=None, masking=False, masking_eps=0.0, keep=None):
    """TorchBF.__call__ restated: masks [..., K, M, T, F] real, Y [..., D, T, F] complex128 -> enh [..., K, T, F].
    keep: a dict that receives the intermediate tensors whose gradients are the stages (bf, psd_s, psd_n)."""
    mc = masks.to(torch.complex128)
    outer = Y.unsqueeze(-3) * Y.conj().unsqueeze(-4)                               # [..., d, D, t, f]

    def psd(m):                                                                     # m [..., K, T, F]
        return torch.einsum("...ktf,...dDtf->...kfdD", m, outer)
    if masks.shape[-3] == 2:
        psd_s, psd_n = psd(mc[..., 0, :, :]), psd(mc[..., 1, :, :])
    elif masks.shape[-3] == 1:
        psd_s, psd_n = psd(mc[..., 0, :, :]), psd(1 - mc[..., 0, :, :])
    else:
        raise ValueError(masks.shape)
    phi = torch.linalg.solve(psd_n, psd_s)
    lam = torch.diagonal(phi, dim1=-2, dim2=-1).sum(-1).real
    eps = torch.finfo(lam.dtype).tiny if eps is None else eps
    bf = (phi / torch.clamp(lam, min=eps)[..., None, None])[..., ref]
    if keep is not None:
        for name, t in (("bf", bf), ("psd_s", psd_s), ("psd_n", psd_n)):
            t.retain_grad()
            keep[name] = t
    enh = torch.einsum("...kfd,...dtf->...ktf", bf.conj(), Y)
    if masking:
        enh = enh * torch.clamp(masks[..., :, 0, :, :], min=masking_eps)
    return enh


def autograd_backward(Y, masks, G, ref, eps, masking, meps):
    """CPU autograd of the restatement -> dict(gw [K, F, D], Hs, Hn [K, F, D, D] complex128, dmask in the masks' dtype)"""
    m = torch.tensor(masks, requires_grad=True)
    keep = {}
    enh = torch_bf(m, torch.tensor(Y), ref, eps, masking, meps, keep)
    enh.backward(torch.tensor(G))

    def herm(t):
        t = t.detach().numpy()
        return (t + np.swapaxes(t.conj(), -2, -1)) / 2
    return dict(gw=keep["bf"].grad.numpy(), Hs=herm(keep["psd_s"].grad), Hn=herm(keep["psd_n"].grad),
                dmask=m.grad.numpy(), enh=enh.detach().numpy())


# ---- generators ----------------------------------------------------------------------------------------------------------
def make_case(K, M, D, T, F, f64, seed, masking_eps=None):
    """A well-conditioned system: Y complex Gaussian [D, T, F] with gains 0.5 .. 2 per channel (T >= 2 D frames keep Phi_n
    regular), masks in (0.05, 0.95), G complex Gaussian.  masking_eps: a third of the target masks are put exactly at it,
    the rest lie on both sides."""
    rs = np.random.RandomState(seed)
    Y = R._crandn(rs, D, T, F) * (0.5 + 1.5 * rs.random_sample((D, 1, F)))
    masks = (0.05 + 0.9 * rs.random_sample((K, M, T, F))).astype(np.float64 if f64 else np.float32)
    if masking_eps is not None:
        at = rs.random_sample((K, T, F)) < 1 / 3
        masks[:, 0][at] = masks.dtype.type(masking_eps)
    G = R._crandn(rs, K, T, F)
    return Y, masks, G


def eps_around(lam, side):
    """eps below every trace ('open': None, the reference's tiny) or above every trace ('clamped')"""
    return None if side == "open" else 2.0 * float(np.max(lam)) + 1.0


def bwd_layout(B, K, M, D, T, F):
    """-> chunks, tchunk, doubles of the gw partials (rounded up to 16 bytes), doubles of the whole workspace"""
    chunks, tchunk = R.make_plan(B, K, T, F)
    ngw = (B * chunks * K * 2 * D * F * 8 + 15) // 16 * 2
    return chunks, tchunk, ngw, ngw + B * K * M * D * D * F


def chunked_T(B, K, F):
    """the first T that make_plan splits into more than one chunk"""
    return next(T for T in range(17, 4096) if R.make_plan(B, K, T, F)[0] > 1)


# The grid of tests/test_gpu_mvdr_backward.py: B, K, M, D, T (None: chunked_T), F, f64, ref_last, masking, eps side
GRID = [(1, 1, 1, 1, 2, 63, True, False, False, "open"), (2, 3, 2, 2, 4, 63, False, True, True, "open"),
        (1, 5, 1, 6, 12, 65, True, True, True, "open"), (1, 3, 2, 7, 14, 130, True, False, False, "open"),
        (1, 1, 1, 8, 37, 65, False, True, True, "clamped"), (2, 3, 2, 6, 37, 63, True, False, True, "clamped"),
        (1, 5, 2, 2, 37, 130, False, False, False, "open"), (2, 5, 2, 1, 37, 1, True, False, True, "open"),
        (1, 3, 1, 6, None, 65, False, False, True, "open"), (2, 5, 2, 8, None, 1, True, True, False, "open"),
        (1, 3, 2, 7, None, 63, False, True, True, "clamped")]


def shape_of(case):
    """-> B, K, M, D, T, F, f64, ref, masking, eps side"""
    B, K, M, D, T, F, f64, ref_last, masking, side = case
    T = chunked_T(B, K, F) if T is None else T
    return B, K, M, D, T, F, f64, (D - 1 if ref_last else 0), masking, side


MEPS = 0.4


def max_rel(got, want, scale):
    """max-norm error relative to the stage's scale"""
    return float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / max(scale, 1e-300)


def compare(ext, ag, masks):
    """errors of `ag` (a dict like autograd_backward's) against the extended stages, relative to each stage's scale; dmask
    against the extended result rounded to the masks' dtype"""
    sc = ext["scale"]
    d = {key: max_rel(ag[key], R.xcf(ext[key]), sc[key]) for key in ("gw", "Hs", "Hn") if key in ag}
    d["dmask"] = max_rel(ag["dmask"].astype(np.float64), R.xf(ext["dmask"]).astype(masks.dtype).astype(np.float64),
                         sc["dmask"])
    return d


def tol(masks):
    return dict(gw=1e-12, Hs=1e-10, Hn=1e-10, dmask=1e-10 if masks.dtype == np.float64 else 3e-7)


# ---- tests ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GRID)
def test_extended_backward_matches_autograd(case):
    """every shape of the GPU file's grid, one batch element of it and at most 9 of its bins (the arithmetic is per bin and
    per batch element, and slow here; the GPU file runs all of them)"""
    B, K, M, D, T, F, f64, ref, masking, side = shape_of(case)
    F = min(F, 9)
    Y, masks, G = make_case(K, M, D, T, F, f64, 11 + D, MEPS if masking else None)
    lam = extended_backward(Y, masks, G, ref, TINY, masking, MEPS)["lam"]
    eps = eps_around(lam, side)
    ext = extended_backward(Y, masks, G, ref, TINY if eps is None else eps, masking, MEPS)
    ag = autograd_backward(Y, masks, G, ref, eps, masking, MEPS)
    err = compare(ext, ag, masks)
    print(case, err)
    if side == "clamped":
        assert (lam < eps).all()
    if D == 1 and not masking:
        assert np.abs(R.xf(ext["dmask"])).max() <= 1e-15 * ext["scale"]["dmask"]        # w = 1: no gradient
    for key, t in tol(masks).items():
        assert err[key] <= t, (key, err[key])
    assert ag["dmask"].dtype == masks.dtype


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defects_fail(defect):
    K, M, D, T, F = 2, 2, 3, 9, 5
    Y, masks, G = make_case(K, M, D, T, F, True, 5, MEPS)
    assert (masks[:, 0] == MEPS).any() and (masks[:, 0] < MEPS).any() and (masks[:, 0] > MEPS).any()
    lam = extended_backward(Y, masks, G, 1, TINY, True, MEPS)["lam"]
    eps = eps_around(lam, "clamped") if defect == "trace_kept" else None
    ag = autograd_backward(Y, masks, G, 1, eps, True, MEPS)
    clean = compare(extended_backward(Y, masks, G, 1, eps or TINY, True, MEPS), ag, masks)
    bad = compare(extended_backward(Y, masks, G, 1, eps or TINY, True, MEPS, defect=defect), ag, masks)
    print(defect, clean, bad)
    assert all(clean[k] <= t for k, t in tol(masks).items())
    assert any(bad[k] > 1e3 * t for k, t in tol(masks).items()), bad


def test_workspace_layout_is_host_only():
    from tssep_amd import _lib
    L = _lib.lib()
    for B, K, M, D, T, F in [(1, 1, 1, 1, 2, 1), (2, 3, 2, 6, 37, 65), (1, 5, 1, 8, 300, 130), (1, 3, 2, 7, 64, 63),
                             (2, 8, 1, 6, 1878, 513)]:
        chunks, tchunk, ngw, total = bwd_layout(B, K, M, D, T, F)
        assert L.tssep_mvdr_bwd_workspace_bytes(B, K, M, D, T, F) == 8 * total
        assert L.tssep_mvdr_partial_bytes(B, K, D, T, F) == B * chunks * K * 2 * D * D * F * 8      # the same chunks
    assert L.tssep_mvdr_bwd_workspace_bytes(1, 3, 2, 9, 37, 65) == 0             # more than 8 channels
    assert L.tssep_mvdr_bwd_workspace_bytes(1, 0, 2, 6, 37, 65) == 0
    assert L.tssep_mvdr_bwd_workspace_bytes(1, 3, 3, 6, 37, 65) == 0             # M is 1 or 2


def test_differentiable_keyword():
    from tssep_amd.train import enhancer as E
    assert E.TorchBF(differentiable=True).differentiable is True and E.TorchBF().differentiable is False
    m = torch.rand(2, 1, 8, 3, requires_grad=True)
    Y = torch.randn(3, 8, 3, dtype=torch.complex128)
    with pytest.raises(NotImplementedError, match="differentiable=True"):       # raised before anything touches a device
        E.TorchBF()(m, {"Observation": Y, "reference_channel": 0}, None)
    with pytest.raises(NotImplementedError, match="Observation"):
        E.TorchBF(differentiable=True)(m, {"Observation": Y.clone().requires_grad_(), "reference_channel": 0}, None)


def test_a_step_through_torch_bf_is_never_captured():
    """GraphedStep's decision, on the host: with a TorchBF enhancer every step is routed to the eager path (the trainer's
    `usable` says no, a direct call falls back, a capture refuses); any other enhancer leaves the graph path open."""
    from tssep_amd.train import enhancer as E, graph

    class Stub(torch.nn.Module):
        def __init__(self, enhancer):
            super().__init__()
            self.enhancer = enhancer

    assert graph.host_sync_reason(Stub(E.Masking())) is None and graph.host_sync_reason(Stub(None)) is None
    for bf in (E.TorchBF(differentiable=True), E.TorchBF()):
        assert "hipGraph" in graph.host_sync_reason(Stub(bf))
    ex = {"observation": torch.zeros(1, 8), "auxInput": torch.zeros(1, 2, 3)}
    step = graph.GraphedStep(Stub(E.TorchBF(differentiable=True)), optimizer=None)
    assert step.eager_reason and not step.usable(ex)
    with pytest.raises(RuntimeError, match="runs eagerly"):
        step._capture(ex)
    calls = []
    step._host_side_targets = lambda e: e
    step._eager = lambda e: calls.append(e) or ("out", "summary")
    assert step(ex) == ("out", "summary") and calls == [ex] and step.eager_steps == 1 and step.replays == 0
    assert graph.GraphedStep(Stub(E.Masking()), optimizer=None).eager_reason is None
