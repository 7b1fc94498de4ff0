"""The float64 references and element-wise bounds of the explicit_vad gated kernels (tests/test_gpu_gated_kernels.py),
tested without a GPU.  The functions below run on the device of their inputs; here they run on the CPU at B = 2, K = 3,
N = 1500 (T = 9; F = 513 is fixed for the fused pair): they are anchored against oracle/stft.py plus torch autograd in
float64, the fp32 rounding of their own outputs must lie inside the bounds in every element, and the same outputs with
nine defects planted must fall outside them.  Nothing here is compared with the code under test.

Logit rows hold F + 1 floats: the frame's VAD logit v at column 0, the mask logits l_f behind it.  g = sigmoid(v),
s_f = sigmoid(l_f), mm_f = s_f (1 - s_f), gg = g (1 - g).

    forward   mask_f = s_f g,  est_f = obs_f mask_f,  y = istft(est)
    backward  D = adjoint transform of dy, or of coef[b] sign(est - tgt) with coef = gout / (N ln10 sums) (LogMAE) or
              gout / N (MAE);  dm_f = Re(conj(obs_f) D_f)  (unfused: + dmask_f);
              d(l_f) = dm_f g mm_f;  d(v) = gg (sum_f dm_f s_f [+ dvmask]) [+ gbce[b] (g - vad[b, k, t]) / (K T)]
    gate BCE  l = max(x, 0) - x y + log1p(exp(-|x|)) on x = v, loss[b] = mean over (k, t); backward rows:
              gout[b] (sigmoid(x) - y) / (K T) at column 0, zeros behind it

Bounds, U = 2^-24, first order; every tolerance is multiplied by 1 + 2^-8 at the end, which covers the products of two
relative errors (each at most 2^-9 for |logit| <= 1e4), and gets + 2^-126 (TINY): v_exp_f32 / v_rcp_f32 and OCML at
its range ends may flush a subnormal result, and a product that lands below the normal range is rounded absolutely.
  * sigmoidf_mask: e(x) = |s^ - s| <= U s (8 + 2 |x|) + TINY (test_gpu_stft_kernels.py, test_gpu_streaming_kernels.py);
    kept absolute, so a 1 - g that rounds to 0 in fp32 is covered by e(v) and not by a relative error of gg.
  * mask = fl(s^ g^): g e(l_f) + s_f e(v) + U s_f g.  est: |obs_f| (that + U mask_f), the product with each component.
  * y: the transform's FFT_C L U ||frame||_2 and overlap-add terms of ref_istft (test_gpu_stft_kernels.py), plus the
    spectrum's own error through the inverse transform: a frame's sample error is at most the 2-norm of the frame's
    error, ||irfft(E)||_2 <= sqrt(2 / size) ||E||_2 for a half spectrum E (Parseval), E_f = the bound of est_f above.
  * D: (FFT_C L U + rel) fro per frame (ref_rfft), rel = 8 U for the loss modes' coefficient (test_gpu_stft_kernels.py).
    dm_f: |obs_f| tol(D) (Cauchy-Schwarz over the two components) + 3 U of the dot product's two terms.
  * d(l_f) = fl(fl(fl(dm^ g^) s^) fl(1 - s^)): three products and the subtraction, 4 U, and |s^ (1 - s^) - mm| <= e(l_f)
    (|1 - s - s^| <= 1):  e(dm) g mm + |dm| (g (e(l_f) + 4 U mm) + e(v) mm).
  * the d(v) sum S = sum_f dm_f s_f in the kernel's fixed order: lane l adds its bins l, l + 64, ... (the fused kernel:
    eight, and lane 0 the Nyquist bin as a ninth), ceil(F / 64) adds at most, then the six steps of the shuffle tree,
    and each product is rounded once where it is not contracted: c = ceil(F / 64) + 6 + 1 (16 at F = 513), every
    term passes through at most c roundings: c U sum_f |dm_f s_f|.  Propagated: sum_f (e(dm_f) s_f + |dm_f| e(l_f)).
    The unfused kernel adds dvmask: + U |S|.
  * d(v) = fl(fl(S^ g^) fl(1 - g^)): |S| (e(v) + 3 U gg) + gg e(S)  (|g^ (1 - g^) - gg| <= e(v), two products and the
    subtraction).
  * the BCE fold gbce (sigmoidf_acc(v) - vad) inv_kt: sigmoid_err(.., fast=False) of test_recurrence_reference.py (OCML
    expf within 3 ulp, the sum, the IEEE division), the subtraction, inv_kt = fl(1 / (K T)) (K T < 2^24 is exact) and
    two products: |gbce| / (K T) (e_acc + 4 U |g - vad|); the final addition U |d(v)|.  tssep_gatebce_bwd divides by
    K T instead (one product, one division, the subtraction): inside the same 4 U.
  * gate BCE rows: U (|x y| + |max(x, 0) - x y| + |l|) for the product, the subtraction and the last addition,
    3 ulp of expf through log1p (derivative 1 / (1 + E) <= 1): 6 U E / (1 + E), E = exp(-|x|), and 2 ulp of log1pf
    (the OpenCL full-profile limits, which OCML honours): 4 U log1p(E).  The mean over K T rows: the sum of the rows'
    bounds plus (K T / 256 + 16) U sum |l| (a thread's running sum of K T / 256 rows, the wave and workgroup
    reductions, the division), over K T.
  * the partial sums of |y - tgt|: check_partials of test_gpu_stft_kernels.py, (hops per chunk + 16) U sum |y - tgt|.

The planted defects (DEFECTS) are caught at the sizes of the GPU file too, not only here, because of how the inputs are
drawn (make_inputs, used by both files): rows are scaled by 10^u with u in [-3, 3], so some rows' transform terms are
1e-6 of others' and the fold term (about 1 / (2 K T), K T <= 1 280 there) dominates their d(v); vad is an independent
coin per (b, k, t), so speakers of an utterance differ; gate logits are 3 randn, so g is far from 1 in most frames and
column F differs from column 0; the permutation of utterance 0 is a rotation by one, so perm != iperm whenever
K >= 3; ties est == tgt are planted, among them one whole frame's support; |logit| ~ 3 makes a bf16 rounding 2^-9 relative, a hundred times the
frame bound.  The Nyquist bin and a lane's share of bins carry 1 / 513 and 8 / 513 of a frame's d(v) terms against a
bound of about 513 x 1e-5 of their typical size -- most frames exceed it."""
import math

import pytest
import torch

from oracle import stft as ostft
from test_gpu_stft_kernels import FFT_C, Ratios, check_partials, fft_rel, ref_istft, ref_rfft, windows64, within  # noqa: F401
from test_recurrence_reference import TINY, sigmoid_err

U = 2.0 ** -24
F = 513
SIZE, SHIFT, PAD = 1024, 256, 768
SECOND = 1 + 2.0 ** -8
LOSS_REL = 8 * U            # the loss modes' coefficient (test_gpu_stft_kernels.py)
MODES = ("dy", "logmae", "mae")


def frames(N):
    return ostft.num_frames(N, SIZE, SHIFT, fading=True)


def chain(Fb):
    """roundings a term of the d(v) sum passes through, at most"""
    return -(-Fb // 64) + 6 + 1


def mask_err(x, s):
    """|sigmoidf_mask(x) - s|, absolute, at the fp32 argument x (s = sigmoid(x) in float64)"""
    return U * s * (8 + 2 * x.abs()) + TINY


def finish(tol):
    return tol * SECOND + TINY


def _ola(seg):
    r, T, size = seg.shape
    length = (T - 1) * SHIFT + size
    return torch.nn.functional.fold(seg.transpose(1, 2), output_size=(1, length), kernel_size=(1, size),
                                    stride=(1, SHIFT)).reshape(r, length)


# ------------------------------------------------------------------------------------------------------------ forward
def ref_gate(lg):
    """lg [..., F + 1] float64 -> g, e(v) [...], s, e(l) [..., F]"""
    v, l = lg[..., 0], lg[..., 1:]
    g, s = torch.sigmoid(v), torch.sigmoid(l)
    return g, mask_err(v, g), s, mask_err(l, s)


def ref_mask(lg, gate_col=0):
    """-> mask [..., F], its bound, vmask [...], its bound"""
    g, eg, s, es = ref_gate(lg)
    if gate_col:
        g = torch.sigmoid(lg[..., gate_col])
    m = s * g[..., None]
    return m, g[..., None] * es + s * eg[..., None] + U * m, g, eg


def ref_unfused_fwd(lg, obs):
    """lg [b, K, T, F + 1] float64, obs [b, T, F] complex128 -> {name: (ref, tol)} of mask, vmask and est (est as
    [..., 2] reals)"""
    m, em, g, eg = ref_mask(lg)
    o = obs[:, None]
    est = torch.view_as_real(o * m)
    e_est = (o.abs() * (em + U * m))[..., None].expand_as(est)
    return {"mask": (m, finish(em)), "vmask": (g, finish(eg)), "est": (est, finish(e_est))}


def ref_fused_fwd(lg, obs, ws64, N, gate_col=0):
    """-> (y [b K, N], tol [b K, N]) of istft(obs sigmoid(l) sigmoid(v))"""
    b, K, T, _ = lg.shape
    m, em, _, _ = ref_mask(lg, gate_col)
    o = obs[:, None]
    e_frame = (o.abs() * (em + U * m)).reshape(b * K, T, -1).norm(dim=-1) * math.sqrt(2.0 / SIZE)
    y, tol = ref_istft((o * m).reshape(b * K, T, -1), ws64, SIZE, SHIFT, PAD, N)
    extra = _ola(ws64.abs() * e_frame[..., None].expand(-1, -1, SIZE))[..., PAD:PAD + N]
    return y, finish(tol + extra)


# ----------------------------------------------------------------------------------------------------------- backward
def loss_dy(est, tgt, coef, tie=0.0):
    """the loss modes' frame samples: coef[row] sign(est - tgt) from the fp32 est and tgt [rows, N]; `tie` at est == tgt"""
    d = est.double() - tgt.double()
    sg = torch.where(d == 0, torch.full_like(d, tie), torch.sign(d))
    return sg * coef[:, None]


def loss_coef(mode, gout, sums, N, K):
    """coef [B K] float64 of the fp32 gout [B] and sums [B]"""
    c = gout.double() / (N * math.log(10) * sums.double()) if mode == "logmae" else gout.double() / N
    return c.repeat_interleave(K)


def ref_dm(dy, obs, ws64, T, K, rel=0.0):
    """dy [b K, N] float64 -> dm [b, K, T, F] = Re(conj(obs) D) and the bound of the kernel's dm"""
    D, fro = ref_rfft(dy, ws64, SIZE, SHIFT, PAD, T, adjoint=True)
    b = obs.shape[0]
    D = D.view(b, K, T, -1)
    tol_d = ((fft_rel(SIZE) + rel) * fro).view(b, K, T, 1)
    o = obs[:, None]
    dm = o.real * D.real + o.imag * D.imag
    terms = (o.real * D.real).abs() + (o.imag * D.imag).abs()
    return dm, o.abs() * tol_d + 3 * U * terms


def ref_fold(lg, vad, gbce, defect=None):
    """the gate BCE's gradient of column 0: gbce[b] (sigmoid(v) - vad[b, k, t]) / (K T) [b, K, T] and its bound"""
    b, K, T, Fb1 = lg.shape
    v = lg[..., 0]
    g = torch.sigmoid(v)
    if defect == "vad_by_utterance":
        vad = vad.reshape(-1, T)[:b][:, None].expand(b, K, T)
    kt = K * T * (Fb1 - 1 if defect == "fold_over_ktf" else 1)
    diff = g - vad
    gb = gbce.double()[:, None, None]
    return gb * diff / kt, gb.abs() / kt * (sigmoid_err(v, g, False) + 4 * U * diff.abs())


def ref_head_bwd(lg, dm, e_dm, dvm=None, fold=None, defect=None):
    """lg [b, K, T, F + 1], dm and its bound [b, K, T, F], dvm [b, K, T] (the unfused kernel's dvmask), fold = (ref, tol)
    of ref_fold -> (d(logit) [b, K, T, F + 1], tol)."""
    g, eg, s, es = ref_gate(lg)
    Fb = s.shape[-1]
    if defect == "gate_from_column_F":
        g = torch.sigmoid(lg[..., Fb])
    mm, gg = s * (1 - s), g * (1 - g)
    g1, eg1 = g[..., None], eg[..., None]
    dl = dm * g1 * mm
    t_dl = e_dm * g1 * mm + dm.abs() * (g1 * (es + 4 * U * mm) + eg1 * mm)
    terms = dm * s
    if defect == "no_nyquist":
        terms = terms[..., :-1]
    elif defect == "no_lane_5":
        terms = terms.clone()
        terms[..., 5::64] = 0
    S, A = terms.sum(-1), terms.abs().sum(-1)
    e_S = chain(Fb) * U * A + (e_dm * s + dm.abs() * es).sum(-1)
    if dvm is not None:
        S = S + dvm
        e_S = e_S + U * S.abs()
    dv = S * gg
    t_dv = S.abs() * (eg + 3 * U * gg) + gg * e_S
    if fold is not None:
        dv = dv + fold[0]
        t_dv = t_dv + fold[1] + U * dv.abs()
    if defect == "no_gate_in_dl":
        dl = dm * mm
    return torch.cat([dv[..., None], dl], -1), finish(torch.cat([t_dv[..., None], t_dl], -1))


def ref_fused_bwd(mode, x, tgt, gout, sums, lg, obs, ws64, vad=None, gbce=None, defect=None):
    """The fused backward.  mode 'dy': x [b K, N] is dy; 'logmae' / 'mae': x is the kernel's fp32 estimate, tgt the
    target, gout and sums [b] fp32.  lg [b, K, T, F + 1] float64 of the fp32 logits, obs [b, T, F] complex128."""
    b, K, T, _ = lg.shape
    N = x.shape[-1]
    if defect == "bf16_logits":
        lg = torch.cat([lg[..., :1], lg[..., 1:].float().bfloat16().double()], -1)
    if mode == "dy":
        dy, rel = x.double(), 0.0
    else:
        dy, rel = loss_dy(x, tgt, loss_coef(mode, gout, sums, N, K), tie=1.0 if defect == "tie_gets_coef" else 0.0), LOSS_REL
    dm, e_dm = ref_dm(dy, obs, ws64, T, K, rel)
    fold = ref_fold(lg, vad.double(), gbce, defect) if vad is not None else None
    return ref_head_bwd(lg, dm, e_dm, fold=fold, defect=defect)


def ref_unfused_bwd(dest, dmask, dvm, lg, obs):
    """tssep_maskhead_gated_bwd: dest [b, K, T, F] complex128, dmask [b, K, T, F], dvm [b, K, T], each or None"""
    shape = lg.shape[:-1] + (lg.shape[-1] - 1,)
    dm = torch.zeros(shape, dtype=torch.float64, device=lg.device)
    e_dm = torch.zeros_like(dm)
    if dest is not None:
        o = obs[:, None]
        dm = o.real * dest.real + o.imag * dest.imag
        e_dm = 3 * U * ((o.real * dest.real).abs() + (o.imag * dest.imag).abs())
    if dmask is not None:
        dm = dm + dmask
        e_dm = e_dm + U * dm.abs()
    return ref_head_bwd(lg, dm, e_dm, dvm=dvm)


def bt_store(d, pos):
    """[B, K, T, C] -> the bt_major layout [B T, K C]: speaker k of utterance b at position pos[b, k] (None: k)"""
    B, K, T, C = d.shape
    out = torch.empty(B, T, K, C, dtype=d.dtype, device=d.device)
    if pos is None:
        out.copy_(d.transpose(1, 2))
    else:
        out[torch.arange(B, device=d.device)[:, None], :, pos.long()] = d
    return out.view(B * T, K * C)


def bt_load(x, pos, K):
    """the inverse of bt_store -> [B, K, T, C]"""
    B = pos.shape[0]
    v = x.view(B, -1, K, x.shape[-1] // K)
    return v[torch.arange(B, device=x.device)[:, None], :, pos.long()]


# ----------------------------------------------------------------------------------------------------------- gate BCE
def ref_bce_rows(x, y):
    """x, y [...] float64 -> the per-row loss and its bound"""
    a, p = x.clamp(min=0), x * y
    E = torch.exp(-x.abs())
    L = torch.log1p(E)
    l = a - p + L
    return l, U * (p.abs() + (a - p).abs() + l.abs() + 6 * E / (1 + E) + 4 * L) + TINY


def ref_bce(x, y):
    """x, y [B, K, T] float64 -> loss [B] and its bound (the mean over (k, t))"""
    l, e = ref_bce_rows(x, y)
    kt = x.shape[1] * x.shape[2]
    return l.sum((1, 2)) / kt, finish((e.sum((1, 2)) + (kt / 256 + 16) * U * l.abs().sum((1, 2))) / kt)


def ref_bce_bwd(x, y, gout):
    """-> column 0 of the backward's rows [B, K, T] and its bound (ref_fold with ld = 1)"""
    ref, tol = ref_fold(x[..., None], y, gout)
    return ref, finish(tol)


# ------------------------------------------------------------------------------------------------------------- inputs
def row_scale(n, g, device):
    return 10.0 ** (torch.rand(n, device=device, generator=g) * 6 - 3)


def make_inputs(B, K, N, seed, device="cpu"):
    """The inputs of a fused case, fp32 as the kernels take them: rows scaled by 10^u, u in [-3, 3]; logits 3 randn; vad
    a coin per (b, k, t); utterance b's permutation is the rotation by 1 + b, no involution at b = 0 for K >= 3 (so
    perm != iperm)."""
    g = torch.Generator(device=device).manual_seed(seed)
    T = frames(N)
    d = dict(B=B, K=K, N=N, T=T)
    d["logit"] = torch.randn(B, K, T, F + 1, device=device, generator=g).mul_(3)
    obs = torch.randn(B, T, F, device=device, generator=g, dtype=torch.complex64)
    d["obs"] = obs * row_scale(B, g, device)[:, None, None]
    d["tgt"] = torch.randn(B * K, N, device=device, generator=g) * (0.01 * row_scale(B, g, device).repeat_interleave(K))[:, None]
    d["dy"] = torch.randn(B * K, N, device=device, generator=g) * row_scale(B * K, g, device)[:, None]
    d["vad"] = (torch.rand(B, K, T, device=device, generator=g) > 0.5).float()
    d["gbce"] = torch.rand(B, device=device, generator=g) + 0.5
    d["gout"] = torch.rand(B, device=device, generator=g) + 0.5
    d["sums"] = torch.rand(B, device=device, generator=g) * 10 ** (torch.rand(B, device=device, generator=g) * 4 - 2) + 0.01
    perm = (torch.arange(K, device=device)[None] + 1 + torch.arange(B, device=device)[:, None]) % K
    d["perm"] = perm.int()
    d["iperm"] = torch.argsort(perm, dim=1).int()
    return d


def plant_ties(est, tgt, T_frame=4, seed=0):
    """tgt with tgt[i] = est[i] at a few hundred random positions and over the whole support of frame T_frame of row 0
    (samples [256 t - 768, 256 t + 256)): that frame's D is exactly 0."""
    g = torch.Generator().manual_seed(seed)
    tgt = tgt.clone()
    rows, N = est.shape
    idx = torch.randint(0, rows * N, (300,), generator=g).to(est.device)
    tgt.view(-1)[idx] = est.reshape(-1)[idx]
    lo, hi = max(0, 256 * T_frame - PAD), min(N, 256 * T_frame + 256)
    tgt[0, lo:hi] = est[0, lo:hi]
    return tgt


# -------------------------------------------------------------------------------------------------------------- tests
DEFECTS = ["no_gate_in_dl", "no_nyquist", "no_lane_5", "fold_over_ktf", "vad_by_utterance", "perm_for_iperm",
           "gate_from_column_F", "tie_gets_coef", "bf16_logits"]


def outside(got32, ref, tol):
    """elements of the fp32 tensor outside the bound (NaN counts)"""
    return int((~((got32.double() - ref).abs() <= tol)).sum())


@pytest.fixture(scope="module")
def case():
    B, K, N = 2, 3, 1500
    d = make_inputs(B, K, N, seed=1)
    assert d["T"] == 9
    _, ws = windows64(SIZE, SHIFT)
    d["ws64"] = ws
    d["lg"] = d["logit"].double()
    d["o128"] = d["obs"].to(torch.complex128)
    y, tol = ref_fused_fwd(d["lg"], d["o128"], ws, N)
    d["y"], d["y_tol"] = y, tol
    d["est"] = y.float()
    d["tgt_ties"] = plant_ties(d["est"], d["tgt"])
    return d


def test_references_match_the_oracle_and_autograd():
    """The gated references against oracle/stft.py's istft and torch autograd in float64: the forward, every mode of
    the fused backward with the BCE fold, the unfused pair with all three incoming gradients, and the gate BCE."""
    B, K, N = 2, 3, 1500
    d = make_inputs(B, K, N, seed=2)
    T = d["T"]
    _, ws = windows64(SIZE, SHIFT)
    o = d["obs"].to(torch.complex128)
    l64 = d["logit"].double().requires_grad_()
    gate = torch.sigmoid(l64[..., 0])
    mask = torch.sigmoid(l64[..., 1:]) * gate[..., None]
    est = o[:, None] * mask
    y = ostft.istft(est, size=SIZE, shift=SHIFT, window="hann", num_samples=N).reshape(B * K, N)
    yr, _ = ref_fused_fwd(l64.detach(), o, ws, N)
    assert float((yr - y.detach()).abs().max()) <= 1e-12 * float(y.detach().abs().max())
    vad, gb, gout = d["vad"].double(), d["gbce"].double(), d["gout"].double()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(l64[..., 0], vad, reduction="none").mean((-1, -2))
    lb, _ = ref_bce(l64.detach()[..., 0], vad)
    assert float((lb - bce.detach()).abs().max()) <= 1e-12
    (db,) = torch.autograd.grad((bce * gb).sum(), l64, retain_graph=True)
    rb, _ = ref_bce_bwd(l64.detach()[..., 0], vad, d["gbce"])
    assert float((rb - db[..., 0]).abs().max()) <= 1e-12 * float(db.abs().max()) and not bool(db[..., 1:].any())
    tgt = d["tgt"].double()
    mae = (y - tgt).abs().mean(-1).view(B, K).sum(-1)                 # [B]: the argument of the log, the kernel's `sums`
    for mode in MODES:
        if mode == "dy":
            loss, x = (y * d["dy"].double()).sum(), d["dy"]
        else:
            loss, x = ((torch.log10(mae) if mode == "logmae" else mae) * gout).sum(), y.detach()
        (dl,) = torch.autograd.grad(loss + (bce * gb).sum(), l64, retain_graph=True)
        if mode == "dy":
            dyv = x.double()
        else:                                                        # (float64 est and sums: the formula, not its rounding)
            c = gout / (N * math.log(10) * mae.detach()) if mode == "logmae" else gout / N
            dyv = torch.sign(x - tgt) * c.repeat_interleave(K)[:, None]
        dm, e_dm = ref_dm(dyv, o, ws, T, K)
        ref, _ = ref_head_bwd(l64.detach(), dm, e_dm, fold=ref_fold(l64.detach(), vad, d["gbce"]))
        assert float((ref - dl).abs().max()) <= 1e-11 * float(dl.abs().max()), mode
    g = torch.Generator().manual_seed(5)
    dest = torch.randn(B, K, T, F, generator=g, dtype=torch.complex128)
    dmask = torch.randn(B, K, T, F, generator=g, dtype=torch.float64)
    dvm = torch.randn(B, K, T, generator=g, dtype=torch.float64)
    s_ = (torch.view_as_real(est) * torch.view_as_real(dest)).sum() + (mask * dmask).sum() + (gate * dvm).sum()
    (dl,) = torch.autograd.grad(s_, l64)
    ref, _ = ref_unfused_bwd(dest, dmask, dvm, l64.detach(), o)
    assert float((ref - dl).abs().max()) <= 1e-12 * float(dl.abs().max())
    fw = ref_unfused_fwd(l64.detach(), o)
    assert torch.equal(fw["mask"][0], mask.detach()) and torch.equal(fw["vmask"][0], gate.detach())
    assert float((fw["est"][0] - torch.view_as_real(est.detach())).abs().max()) == 0.0


def test_bt_major_store_and_load_are_inverse():
    d = make_inputs(3, 4, 1500, seed=3)
    x = torch.randn(3, 4, d["T"], 5)
    assert bool((d["perm"] != d["iperm"]).any())
    assert torch.equal(bt_load(bt_store(x, d["iperm"]), d["iperm"], 4), x)
    assert torch.equal(bt_store(x, None).view(3, d["T"], 4, 5).transpose(1, 2), x)
    b, k = 1, 2                                   # speaker k of utterance b lies at position iperm[b, k]
    assert torch.equal(bt_store(x, d["iperm"]).view(3, d["T"], 4, 5)[b, :, int(d["iperm"][b, k])], x[b, k])


def test_clean_rounding_is_inside_every_bound(case):
    """The fp32 rounding of each reference output is inside its bound in every element."""
    d = case
    counts = {"fwd y": outside(d["y"].float(), d["y"], d["y_tol"])}
    for name, (ref, tol) in ref_unfused_fwd(d["lg"], d["o128"]).items():
        counts["unfused " + name] = outside(ref.float(), ref, tol)
    for mode in MODES:
        for fold in (False, True):
            ref, tol = ref_fused_bwd(mode, d["dy"] if mode == "dy" else d["est"], d["tgt_ties"], d["gout"], d["sums"],
                                     d["lg"], d["o128"], d["ws64"], d["vad"] if fold else None, d["gbce"])
            counts[f"bwd {mode} fold={fold}"] = outside(ref.float(), ref, tol)
    lb, tb = ref_bce(d["lg"][..., 0], d["vad"].double())
    counts["bce"] = outside(lb.float(), lb, tb)
    rb, tb = ref_bce_bwd(d["lg"][..., 0], d["vad"].double(), d["gbce"])
    counts["bce bwd"] = outside(rb.float(), rb, tb)
    for k, v in counts.items():
        print(f"clean fp32 rounding outside the bound  {k}: {v}")
    assert not any(counts.values()), counts


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_falls_outside_the_bounds(case, defect):
    """Each defect, applied to the reference's own output and rounded to fp32, leaves the bounds of the clean one."""
    d = case
    K = d["K"]
    if defect == "gate_from_column_F":            # the forward reads the same wrong column
        bad, _ = ref_fused_fwd(d["lg"], d["o128"], d["ws64"], d["N"], gate_col=F)
        n = outside(bad.float(), d["y"], d["y_tol"])
        print(f"planted {defect} (forward): {n} of {bad.numel()} elements outside the bound")
        assert n > 0
    mode = "dy" if defect in ("no_gate_in_dl", "no_nyquist", "no_lane_5", "gate_from_column_F") else "logmae"
    args = (mode, d["dy"] if mode == "dy" else d["est"], d["tgt_ties"], d["gout"], d["sums"], d["lg"], d["o128"], d["ws64"],
            d["vad"], d["gbce"])
    ref, tol = ref_fused_bwd(*args)
    if defect == "perm_for_iperm":
        assert bool((d["perm"] != d["iperm"]).any())
        got = bt_load(bt_store(ref.float(), d["perm"]), d["iperm"], K)
        clean = bt_load(bt_store(ref.float(), d["iperm"]), d["iperm"], K)
    else:
        got, _ = ref_fused_bwd(*args, defect=defect)
        got, clean = got.float(), ref.float()
    assert outside(clean, ref, tol) == 0
    n = outside(got, ref, tol)
    print(f"planted {defect}: {n} of {got.numel()} elements outside the bound")
    assert n > 0
    if defect == "tie_gets_coef":                  # the all-tie frame: exactly 0 behind column 0, the fold alone at it
        fr = ref[0, 0, 4]
        fold, _ = ref_fold(d["lg"], d["vad"].double(), d["gbce"])
        assert not bool(fr[1:].any()) and float(fr[0]) == float(fold[0, 0, 4])
        assert bool(got[0, 0, 4, 1:].any())
