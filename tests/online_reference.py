"""Restatements for the online path: causal feature statistics, a tail-carrying STFT and a carry-first
inverse STFT in the dtype of their input (float64: the reference; float32: the independent implementation the checker
is tried on), and the checker tests/test_gpu_online_kernels.py uses, with the defects it has to reject.

Semantics: causal(X)[t] == noncausal(X[:t+1])[t] per utterance -- no formula is new, only the frames the statistics span.
"""
import math

import numpy as np
import torch

from oracle import stft as ostft

U = 2.0 ** -24
SIZE, SHIFT = 1024, 256
PEND = SIZE - SHIFT                    # samples of the STFT tail = floats of the overlap-add carry


# ---------------------------------------------------------------------------------------------------------- features
def fresh_state(B, like):
    s = torch.zeros(B, 2, dtype=like.dtype if not like.is_complex() else like.real.dtype, device=like.device)
    s[:, 1] = -math.inf
    return s


def raw_db(X, fb):
    """10 log10(clamp(mel, 1e-10)) [B, T, n_mels] in the real dtype of X."""
    return 10.0 * torch.log10(torch.clamp((X.abs() ** 2) @ fb.to(X.real.dtype), min=1e-10))


def causal_features(X, fb=None, dct=None, top_db=80.0, state=None, defect=None):
    """X complex [B, T, F] (a chunk of each utterance) -> (mfcc [B,T,n_mfcc] or None, log1p [B,T,F], state [B,2]): running
    maxima by torch.cummax, the current frame included, seeded by `state` = {max |X|, max dB} (None: a fresh stream).
    defect (the checker must reject each): 'batch_floor' -- the dB floor from the running maximum over the BATCH;
    'exclude_current' -- running maxima over t' < t; 'nan_zero' -- no guard where the norm is 0."""
    B, T, _ = X.shape
    rdt = X.real.dtype
    state = fresh_state(B, X) if state is None else state.to(rdt)
    a = X.abs()

    def running(frame_max, seed):
        r = torch.cummax(torch.cat([seed[:, None], frame_max], dim=1), dim=1).values
        return (r[:, :-1] if defect == "exclude_current" else r[:, 1:]), r[:, -1]

    norm, s_a = running(a.amax(-1), state[:, 0])
    scaled = a * ((np.e - 1) / norm[..., None])
    log1p = torch.log1p(scaled)
    if defect != "nan_zero":
        log1p = torch.where(norm[..., None] > 0, log1p, torch.zeros_like(log1p))
    mfcc, s_d = None, state[:, 1]
    if fb is not None:
        db = raw_db(X, fb)
        top, s_d = running(db.amax(-1), state[:, 1])
        if defect == "batch_floor":
            top = top.amax(0, keepdim=True).expand_as(top)
        mfcc = torch.maximum(db, (top - top_db)[..., None]) @ dct.to(rdt)
    return mfcc, log1p, torch.stack([s_a, s_d], dim=1)


def chunked(fn, X, chunks, drop_state=False):
    """fn(X chunk, state) -> (*outputs, state) over the chunks of the frame axis; drop_state: the planted defect of a state
    lost between the calls."""
    outs, state, t0 = [], None, 0
    for n in chunks:
        *o, state = fn(X[:, t0:t0 + n], None if drop_state else state)
        outs.append(o)
        t0 += n
    assert t0 == X.shape[1]
    return [None if o[0] is None else torch.cat(o, dim=1) for o in zip(*outs)] + [state]


def filter_width(fb):
    """Bins of every mel filter's support [lo, hi): pass 1 sums over it."""
    nz = fb != 0
    F = fb.shape[0]
    ar = torch.arange(F, device=fb.device, dtype=torch.float64)[:, None]
    return torch.where(nz.any(0), (ar * nz).amax(0) - torch.where(nz, ar, float(F)).amin(0) + 1, 0.0)


def feature_bounds(X, fb, dct, top_db=80.0):
    """float64 reference and tolerance of the causal features, tests/test_gpu_streaming_kernels.py::test_feat_fwd's bounds
    restated per frame:  err_db = 10/ln10 (width/4 + 8) U + 4 U |db|, the floor carrying the RUNNING maximum of err_db;
    tol = err_db @ |dct| + (n_mels + 2) U (|db'| @ |dct|);  log1p: 8 U a / (1 + a) + 2 U ref.
    -> (mfcc_ref, mfcc_tol) or (None, None), (log1p_ref, log1p_tol)."""
    X64 = X.to(torch.complex128)
    mf = (None, None)
    if fb is not None:
        fb64, dct64 = fb.double(), dct.double()
        db = raw_db(X64, fb64)
        top = torch.cummax(db.amax(-1), dim=1).values
        dbf = torch.maximum(db, (top - top_db)[..., None])
        err = 10 / math.log(10) * (filter_width(fb64) / 4 + 8) * U + 4 * U * db.abs()
        err = torch.maximum(err, torch.cummax(err.amax(-1), dim=1).values[..., None])
        mf = (dbf @ dct64, err @ dct64.abs() + (fb.shape[1] + 2) * U * (dbf.abs() @ dct64.abs()))
    _, ref, _ = causal_features(X64)
    a = torch.expm1(ref)
    return mf, (ref, 8 * U * a / (1 + a) + 2 * U * ref)


def check_features(mfcc, log1p, X, fb, dct, what):
    """The checker: finite, inside the bounds -> the worst ratio error / tolerance.  AssertionError otherwise."""
    (mref, mtol), (lref, ltol) = feature_bounds(X, fb, dct)
    worst = 0.0
    for name, got, ref, tol in (("mfcc", mfcc, mref, mtol), ("log1p", log1p, lref, ltol)):
        if ref is None:
            continue
        assert got.shape == ref.shape, (what, name, got.shape, ref.shape)
        assert bool(torch.isfinite(got).all()), f"{what} {name}: NaN or Inf"
        err = (got.double() - ref).abs()
        bad = err > tol
        assert not bool(bad.any()), (f"{what} {name}: {int(bad.sum())}/{bad.numel()} outside the tolerance, first at "
                                     f"{tuple(int(i) for i in bad.nonzero()[0])}, worst error {float(err.max()):.3g}")
        worst = max(worst, float((err / tol.clamp(min=1e-300)).max()))
    return worst


def feature_input(B, T, F, seed, device="cpu"):
    """Frames spanning 60 dB.  Utterance 2 % B rises strictly -- one frame pattern times a growing scale, so every frame
    moves both maxima and the loudest frame is the last; utterance 1 % B has its loudest frame (|X| and dB) at t = 0;
    utterance 0 starts with two all-zero frames (applied last: with B = 2 it is the rising one as well).  B = 1: the zero
    prefix, then the loudest frame at t = 2, nothing rising (a dropped state would not show on a rising utterance)."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(B, T, F, generator=g, dtype=torch.complex64) * (10 ** (-3 * torch.rand(B, T, 1, generator=g)))
    if B > 1:
        X[2 % B] = torch.randn(F, generator=g, dtype=torch.complex64) * (1e-3 * 10 ** (3 * torch.arange(T) / max(T - 1, 1)))[:, None]
    X[1 % B, 0 if B > 1 else 2] = torch.randn(F, generator=g, dtype=torch.complex64) * 10
    X[0, :2] = 0
    return X.to(device)


# ------------------------------------------------------------------------------------------------- STFT / inverse STFT
def windows(window, dtype, device="cpu"):
    w = torch.as_tensor(ostft.analysis_window(window, SIZE)).to(dtype)
    ws = torch.as_tensor(ostft.synthesis_window(window, SIZE, SHIFT)).to(dtype)
    return w.to(device), ws.to(device)


def stft_stream(x_new, tail, window="hann", stale=False):
    """The frames a push completes: x_new [rows, Tc * 256] behind tail [rows, 768] (None: zeros) -> (X [rows, Tc, 513],
    the new tail).  stale: the planted defect of a tail that lags one hop behind."""
    rows, n = x_new.shape
    assert n % SHIFT == 0 and n > 0
    if tail is None:
        tail = torch.zeros(rows, PEND, dtype=x_new.dtype, device=x_new.device)
    cat = torch.cat([tail, x_new], dim=1)
    w, _ = windows(window, x_new.dtype, x_new.device)
    X = torch.fft.rfft(cat.unfold(-1, SIZE, SHIFT) * w, dim=-1)
    assert X.shape[1] == n // SHIFT
    return X, (cat[:, -PEND - SHIFT:-SHIFT] if stale else cat[:, -PEND:]).clone()


def frames_to_segments(X, window="hann"):
    _, ws = windows(window, X.real.dtype, X.device)
    return torch.fft.irfft(X, n=SIZE, dim=-1) * ws


def istft_whole(X, N, window="hann"):
    """Hop h = ((f_h[768:] + f_{h+1}[512:768]) + f_{h+2}[256:512]) + f_{h+3}[:256], oldest frame first, in the dtype of X;
    frames past the last read as zeros.  -> [rows, N]"""
    seg = frames_to_segments(X, window)
    rows, T, _ = seg.shape
    hops = -(-N // SHIFT)
    seg = torch.cat([seg, seg.new_zeros(rows, max(hops + 3 - T, 0), SIZE)], dim=1)
    q = seg.reshape(rows, -1, 4, SHIFT)
    y = ((q[:, 0:hops, 3] + q[:, 1:hops + 1, 2]) + q[:, 2:hops + 2, 1]) + q[:, 3:hops + 3, 0]
    return y.reshape(rows, -1)[:, :N]


def istft_stream(X, ola, skip, N=None, window="hann", carry="first"):
    """The hops the stream's next Tc frames complete, the carry [rows, 768] (None: zeros) added FIRST, then the call's
    frames in order -> (y [rows, (Tc - skip) * 256] or its first N samples, the new carry).  carry: 'first' |
    'last' (planted defect: the call's frames first, the carry on top) | 'drop' (planted defect: no carry)."""
    seg = frames_to_segments(X, window)
    rows, Tc, _ = seg.shape
    q = seg.reshape(rows, Tc, 4, SHIFT)
    pend = torch.zeros(rows, 3, SHIFT, dtype=seg.dtype, device=seg.device)
    if ola is not None and carry != "drop":
        pend = ola.reshape(rows, 3, SHIFT).clone()
    out = []
    late = [p.clone() for p in pend.unbind(1)] if carry == "last" else None
    if carry == "last":
        pend = torch.zeros_like(pend)
    slots = list(pend.unbind(1)) + [None]            # partial sums of the hops pending, oldest hop first
    born = [-3, -2, -1, 0]                           # (which of them began with a carry: index < 0)
    for t in range(Tc):
        slots[3] = None
        for j in range(4):                           # frame t adds quarter j to the hop pending at position j
            slots[j] = q[:, t, j] if slots[j] is None else slots[j] + q[:, t, j]
        done = slots.pop(0)
        if late is not None and born[0] < 0:
            done = done + late[born[0] + 3]
        born = born[1:] + [t + 1]
        out.append(done)
        slots.append(None)
    if late is not None:
        for j in range(3):
            if born[j] < 0:
                slots[j] = slots[j] + late[born[j] + 3]
    y = torch.stack(out, dim=1)[:, skip:].reshape(rows, -1)
    return (y if N is None else y[:, :N]), torch.stack(slots[:3], dim=1).reshape(rows, PEND)


def masked(logit, obs):
    """sigmoid(logit) * obs per speaker: logit [B,K,T,F] (gated: [B,K,T,F+1], the VAD logit at column 0), obs [B,T,F]
    -> [B*K, T, F]"""
    F = obs.shape[-1]
    m = torch.sigmoid(logit[..., -F:])
    if logit.shape[-1] == F + 1:
        m = m * torch.sigmoid(logit[..., :1])
    return (m * obs[:, None]).reshape(-1, obs.shape[-2], F)


def run_stream(x, pushes, window="hann", mask=None, **defects):
    """x [rows, N] through stft_stream / istft_stream by the pushes (frames each) + flush of tests' schedule ->
    (X [rows, T, 513] of all frames, y [rows, N], the steps).  mask(X chunk, t0) -> the spectrum to invert."""
    from tssep_amd.train.online import schedule
    rows, N = x.shape
    steps = schedule(pushes, N, SHIFT, SIZE)
    tail = ola = None
    Xs, ys, pos, seen = [], [], 0, 0
    for i, st in enumerate(steps):
        last = i == len(steps) - 1
        xn = x[:, pos:pos + st.frames * SHIFT]
        if last:
            xn = torch.cat([xn, x.new_zeros(rows, st.frames * SHIFT - xn.shape[1])], dim=1)
        Xc, tail = stft_stream(xn, tail, window, stale=defects.get("stale", False))
        assert Xc.shape[1] == st.frames
        Yc = Xc if mask is None else mask(Xc, seen)
        y, ola = istft_stream(Yc, ola, st.skip, st.samples if last else None, window, carry=defects.get("carry", "first"))
        assert y.shape[1] == st.samples, (y.shape, st)
        Xs.append(Xc)
        ys.append(y)
        pos, seen = pos + st.frames * SHIFT, seen + st.frames
    return torch.cat(Xs, dim=1), torch.cat(ys, dim=1), steps
