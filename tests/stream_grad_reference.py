"""Restatements for training on a stream: the chunked overlap-add with carry as a float64 forward (the one
of tests/online_reference.py), its adjoint written from the gradient signal g, the whole-utterance adjoint, and the checker
tests/test_gpu_stream_grad_kernels.py uses, with the defects it has to reject.

One call of Tc frames, per row.  g holds Tc + 3 hops of 256 samples:
    hop h < skip: zeros;   skip <= h < Tc: dy[(h - skip) 256 ...], zeros from sample N on;   Tc <= h: d_ola_out[h - Tc]
    dEst[i]     = adjoint-frame(g[256 i .. 256 i + 1024))   (synthesis window, rfft, interior bins x 2/1024, DC / Nyquist
                  x 1/1024)
    d_ola_in[j] = g[hop j], j = 0, 1, 2
    dlogit      = Re(conj(obs) dEst) m (1 - m);   gated rows: d(l_f) = dm_f g s_f (1 - s_f), d(v) = g (1 - g) sum_f dm_f s_f
"""
import math

import numpy as np
import torch

import online_reference as OR

U = OR.U
SIZE, SHIFT, PEND = OR.SIZE, OR.SHIFT, OR.PEND
F = SIZE // 2 + 1
FFT_C = 8                                # the FFT error constant of tests/test_gpu_stft_kernels.py
FFT_REL = FFT_C * (math.ceil(math.log2(SIZE)) + 2) * U

# what the GPU file runs: utterances of 7 and 11 pushed hops + a ragged rest, by these pushes
RESTS = (0, 1, 37, 255)
PATTERNS = {7: [(7,), (1,) * 7, (1, 6), (3, 4)], 11: [(2, 2, 7), (4, 1, 6)]}
ROWS = [(1, 1), (2, 1), (1, 3), (2, 3)]                  # (B, K)
DEFECTS = ("carry_late", "skip_kept", "ola_from_dy", "beyond_N", "gate_missing")


def cases():
    """(pushed hops, pushes, rest) of every stream the GPU file splits."""
    return [(hops, p, r) for hops, pats in PATTERNS.items() for p in pats for r in RESTS]


def steps_of(pushes, N):
    from tssep_amd.train.online import schedule
    return schedule(pushes, N, SHIFT, SIZE)


# ------------------------------------------------------------------------------------------------------ the forward
def tail_forward(logit, obs, ola, skip, N=None, X=None):
    """One call of the streaming tail in the dtype of its input, differentiable by autograd: logit [B,K,Tc,F(+1)] and obs
    [B,Tc,F] (or X [rows,Tc,F] as it is) -> (y [rows, n], the carry behind [rows, 768])."""
    spec = X if X is not None else OR.masked(logit, obs)
    return OR.istft_stream(spec, ola, skip, N)


# ------------------------------------------------------------------------------------------------------ the adjoint
def gradient_signal(dy, d_ola_out, rows, Tc, skip, N, defect=None, dtype=torch.float64):
    """g [rows, Tc + 3, 256].  dy [rows, N] or None (N == 0), d_ola_out [rows, 768] or None (zeros).
    defects: 'carry_late' -- the carry's gradient at hop Tc - 1 + j; 'skip_kept' -- the skip hops hold the samples a
    negative offset wraps to (dy from its start) instead of zeros; 'beyond_N' -- the ragged last hop filled past sample N
    with what lies behind the row (here: ones); 'skip_first' -- the skip hops zeroed where they are the carry's (skip > Tc:
    shows only under a carry gradient that is not chained from a later call, which is zero there)."""
    g = torch.zeros(rows, Tc + 3, SHIFT, dtype=dtype)
    hops = max(Tc - skip, 0)
    if hops and N:
        body = torch.zeros(rows, hops * SHIFT, dtype=dtype)
        if defect == "beyond_N":
            body += 1.0
        body[:, :N] = dy.to(dtype)
        g[:, skip:Tc] = body.reshape(rows, hops, SHIFT)
        if defect == "skip_kept":
            g[:, :min(skip, hops)] = body.reshape(rows, hops, SHIFT)[:, :min(skip, hops)]
    if d_ola_out is not None:
        c = d_ola_out.to(dtype).reshape(rows, 3, SHIFT)
        if defect == "carry_late":
            g[:, Tc - 1:Tc + 2] += c
        else:
            g[:, Tc:] = c                                 # (whatever skip is: with skip > Tc the hops Tc .. skip - 1 are the carry's)
        if defect == "skip_first":
            g[:, :skip] = 0
    return g


def adjoint_frames(g, dtype=torch.float64):
    """g [rows, H, 256] -> (dEst [rows, H - 3, F] complex, fro [rows, H - 3]): the adjoint of the inverse STFT per frame
    and the 2-norm of each frame's full spectrum at the adjoint's scale (the yardstick of the FFT's error)."""
    rows = g.shape[0]
    _, ws = OR.windows("hann", dtype)
    seg = g.reshape(rows, -1).unfold(-1, SIZE, SHIFT) * ws
    fro = seg.norm(dim=-1) * math.sqrt(SIZE) * (2.0 / SIZE)
    D = torch.fft.rfft(seg, dim=-1) * (2.0 / SIZE)
    D[..., 0] *= 0.5
    D[..., -1] *= 0.5
    return D, fro


def head_backward(D, logit, obs, defect=None):
    """dEst [B*K, T, F] -> d(logit), the shape of logit (plain [B,K,T,F], gated [B,K,T,F+1] with d(v) at column 0).
    defect 'gate_missing': d(v) without the factor g (1 - g)."""
    B, K, T, Fl = logit.shape
    D = D.reshape(B, K, T, F)
    o = obs.to(D.dtype)[:, None]
    dm = o.real * D.real + o.imag * D.imag
    lg = logit.to(dm.dtype)
    if Fl == F:
        m = torch.sigmoid(lg)
        return dm * m * (1 - m)
    s, gm = torch.sigmoid(lg[..., 1:]), torch.sigmoid(lg[..., :1])
    dv = (dm * s).sum(-1, keepdim=True)
    if defect != "gate_missing":
        dv = dv * gm * (1 - gm)
    return torch.cat([dv, dm * gm * s * (1 - s)], dim=-1)


def tail_backward(dy, d_ola_out, Tc, skip, N, logit=None, obs=None, rows=None, defect=None):
    """The adjoint of one call, float64 -> (dlogit, or dX [rows, Tc, F] when logit is None; d_ola_in [rows, 768]).
    defect 'ola_from_dy': d_ola_in read from dy alone, so a call of Tc < 3 frames does not pass d_ola_out through."""
    rows = rows if logit is None else logit.shape[0] * logit.shape[1]
    g = gradient_signal(dy, d_ola_out, rows, Tc, skip, N, defect)
    D, _ = adjoint_frames(g)
    d_in = g[:, :3].clone()
    if defect == "ola_from_dy":
        d_in[:, Tc:] = 0
    out = D if logit is None else head_backward(D, logit, obs, defect)
    return out, d_in.reshape(rows, PEND)


def whole_backward(dy, T, logit=None, obs=None):
    """The whole-utterance adjoint, float64: dy [rows, N] over T frames, full fading (768 zeros in front)."""
    rows, N = dy.shape
    g = torch.zeros(rows, (T + 3) * SHIFT, dtype=torch.float64)
    g[:, PEND:PEND + N] = dy.double()
    D, _ = adjoint_frames(g.reshape(rows, T + 3, SHIFT))
    return D if logit is None else head_backward(D, logit, obs)


def stream_backward(dy, steps, logit=None, obs=None, rows=None, carry=True, defect=None):
    """The calls of a stream last first, each d_ola_in handed on as the earlier call's d_ola_out (carry=False: NULL for
    every call -- each chunk truncated) -> (the concatenated dlogit / dX, [d_ola_in per call])."""
    outs, d_ola, carries = [], None, []
    t_hi, n_hi = sum(s.frames for s in steps), sum(s.samples for s in steps)
    for st in reversed(steps):
        t_lo, n_lo = t_hi - st.frames, n_hi - st.samples
        lg = None if logit is None else logit[:, :, t_lo:t_hi]
        ob = None if obs is None else obs[:, t_lo:t_hi]
        d, d_in = tail_backward(dy[:, n_lo:n_hi] if st.samples else None, d_ola if carry else None, st.frames, st.skip,
                                st.samples, lg, ob, rows, defect)
        outs.insert(0, d)
        carries.insert(0, d_in)
        d_ola, t_hi, n_hi = d_in, t_lo, n_lo
    return torch.cat(outs, dim=-2), carries


# ------------------------------------------------------------------------------------------------------ the checker
def bounds(g, logit=None, obs=None):
    """float64 reference and tolerance of one call's dX / dlogit from its gradient signal g: the measure of
    tests/test_gpu_stft_kernels.py::test_fused_mask_istft_at_training_sizes (`_dlogit_ref` there), restated.
      dEst: FFT_REL fro per frame;   plain: (|o| tol_d + 3 U terms) mm + |dot| (dm + 3 U mm), dm = U m (8 + 2 |l|).
    Gated rows (this file's own, the same reasoning with the gate as one more rounded factor): with ds = U s (8 + 2 |l|),
    dg = U gm (8 + 2 |v|) the factor gm s (1 - s) carries gm ds + s (1 - s) dg + 4 U gm s (1 - s); d(v) sums 513 terms
    dot_f s_f in 15 roundings (9 per lane, 6 across the wave: 16 U sum |dot_f s_f|) and carries the gate's g (1 - g)."""
    D, fro = adjoint_frames(g)
    tol_d = (FFT_REL * fro)[..., None]
    if logit is None:
        return D, tol_d.expand(*D.shape).unsqueeze(-1).expand(*D.shape, 2)
    B, K, T, Fl = logit.shape
    D, tol_d = D.reshape(B, K, T, F), tol_d.reshape(B, K, T, 1)
    o = obs.to(torch.complex128)[:, None]
    dot = o.real * D.real + o.imag * D.imag
    terms = (o.real * D.real).abs() + (o.imag * D.imag).abs()
    tdot = o.abs() * tol_d + 3 * U * terms
    lg = logit.double()
    if Fl == F:
        m = torch.sigmoid(lg)
        mm = m * (1 - m)
        dm = U * m * (8 + 2 * lg.abs())
        return dot * mm, tdot * mm + dot.abs() * (dm + 3 * U * mm)
    l, v = lg[..., 1:], lg[..., :1]
    s, gm = torch.sigmoid(l), torch.sigmoid(v)
    ss, gg = s * (1 - s), gm * (1 - gm)
    ds, dg = U * s * (8 + 2 * l.abs()), U * gm * (8 + 2 * v.abs())
    ref_l = dot * gm * ss
    tol_l = tdot * gm * ss + dot.abs() * (gm * ds + ss * dg + 4 * U * gm * ss)
    tot = (dot * s).sum(-1, keepdim=True)
    tol_tot = (tdot * s + dot.abs() * (ds + U * s)).sum(-1, keepdim=True) + 16 * U * (dot * s).abs().sum(-1, keepdim=True)
    ref_v = tot * gg
    tol_v = tol_tot * gg + tot.abs() * (dg + 3 * U * gg)
    return torch.cat([ref_v, ref_l], -1), torch.cat([tol_v, tol_l], -1)


def within(got, ref, tol, what):
    """|got - ref| <= tol element-wise, NaN / Inf in `got` fails -> the worst err / tol."""
    if got.is_complex():
        got = torch.view_as_real(got)
    if ref.is_complex():
        ref = torch.view_as_real(ref)
    err = (got.double().cpu() - ref).abs()
    tol = torch.broadcast_to(tol, err.shape)
    ok = err <= tol
    if not bool(ok.all()):
        bad = ~ok
        idx = np.unravel_index(int(bad.reshape(-1).nonzero()[0]), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the tolerance; first at {idx}: got "
                             f"{float(got[idx]):.9g}, want {float(ref[idx]):.9g}, tol {float(tol[idx]):.3g}")
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())


def check_call(d, d_ola_in, dy, d_ola_out, Tc, skip, N, logit=None, obs=None, rows=None, what=""):
    """The checker of one call: d (dlogit / dX) inside the bounds of the float64 adjoint, d_ola_in the exact copy of hops
    0, 1, 2 of g -> the worst err / tol (a list of candidates d: one each).  AssertionError otherwise."""
    rows = rows if logit is None else logit.shape[0] * logit.shape[1]
    g = gradient_signal(dy, d_ola_out, rows, Tc, skip, N)
    ref, tol = bounds(g, logit, obs)
    if isinstance(d, (list, tuple)):                  # several candidates for the same frames: one ratio each
        worst = [within(x, ref, tol, f"{what} d[{i}]") for i, x in enumerate(d)]
    else:
        worst = within(d, ref, tol, f"{what} d")
    if d_ola_in is not None:
        want = g[:, :3].reshape(rows, PEND)
        assert torch.equal(d_ola_in.double().cpu(), want), f"{what}: d_ola_in is not the copy of hops 0, 1, 2 of g"
    return worst


def inputs(B, K, T, gated, seed):
    """logit [B,K,T,F(+1)] (the VAD logits of gated rows away from saturation, so the gate's factor matters), obs [B,T,F]"""
    gen = torch.Generator().manual_seed(seed)
    logit = torch.randn(B, K, T, F + int(gated), generator=gen) * 3
    if gated:
        logit[..., 0] = torch.randn(B, K, T, generator=gen)
    obs = torch.randn(B, T, F, generator=gen, dtype=torch.complex64)
    return logit, obs


def pos_zero(t):
    """-0 -> +0 (the carry-first sum of the forward and an empty descriptor's zeros may differ in the sign of a zero)"""
    return t + 0.0
