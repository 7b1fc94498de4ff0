"""The online entry points of the C ABI on a real MI355X, called directly, every output pre-filled with NaN:
tssep_feat_causal_fwd against the float64 restatement within tests/online_reference.py's bounds and bit for bit across
chunkings and against tssep_feat_fwd where the two coincide; tssep_stft_stream_fwd, tssep_istft_stream_fwd and
tssep_mask_istft_stream_fwd bit for bit (torch.equal) against the whole-signal entry points; the guards."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import online_reference as OR  # noqa: E402
from test_online_reference import FEATURE_CASES, tables  # noqa: E402

DEV = "cuda"
NAN = float("nan")
E_SHAPE, E_ALIGN, E_UNSUPPORTED, E_NULL = -1, -2, -3, -5
WORST = {}


def L():
    from tssep_amd import _lib
    return _lib.lib()


def H():
    from tssep_amd import hip_ops
    return hip_ops


def p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def hann():
    from tssep_amd import functional as Fn
    return Fn.windows("hann", 1024, 256, torch.device(DEV), 1024)


# ---------------------------------------------------------------------------------------------------------- features
def feat_causal(X, fb, dct, n_mfcc, state=None):
    """-> (out [B,T,n_mfcc+F], state_out [B,2]) of one call; X complex64 [B,T,F] on the device"""
    B, T, F = X.shape
    n_mels = fb.shape[1] if n_mfcc else 0
    D = n_mfcc + F
    ld = (D + 3) // 4 * 4
    out, state_out = nans(B, T, ld), nans(B, 2)
    ws = nans(int(L().tssep_feat_causal_workspace_bytes(B, T, n_mels, F)) // 4 + 4)
    Xr = torch.view_as_real(X.contiguous())
    rc = L().tssep_feat_causal_fwd(p(Xr), B, T, F, p(fb), p(dct), n_mels, n_mfcc, 80.0, p(state), p(state_out), p(out), ld,
                                   p(ws), stream())
    assert rc == 0, rc
    return out[..., :D], state_out


def feat_chunked(X, fb, dct, n_mfcc, chunks):
    outs, state, t0 = [], None, 0
    for n in chunks:
        o, state = feat_causal(X[:, t0:t0 + n].contiguous(), fb, dct, n_mfcc, state)
        outs.append(o)
        t0 += n
    assert t0 == X.shape[1]
    return torch.cat(outs, dim=1), state


@pytest.mark.parametrize("B,T,F,n_mels,n_mfcc", FEATURE_CASES)
def test_feat_causal_fwd(B, T, F, n_mels, n_mfcc):
    """(3, 37): crosses a 16-frame pass-1 block raggedly; (5, 205): 65 blocks; F = 201; n_mfcc = 0: plain log1p.  Against
    float64 within the restated bounds, then the chunkings bit for bit."""
    Xc = OR.feature_input(B, T, F, seed=B * 100 + T)
    X = Xc.to(DEV)
    fb, dct = tables(F, n_mels, n_mfcc)
    fbd, dctd = (fb.to(DEV), dct.to(DEV)) if n_mfcc else (None, None)
    out, state = feat_causal(X, fbd, dctd, n_mfcc)
    torch.cuda.synchronize()
    mfcc = out[..., :n_mfcc].cpu() if n_mfcc else None
    WORST[(B, T, F)] = OR.check_features(mfcc, out[..., n_mfcc:].cpu(), Xc, fb, dct, f"feat_causal_fwd {(B, T, F)}")
    print(f"feat_causal_fwd {(B, T, F, n_mels, n_mfcc)}: worst error / tolerance {WORST[(B, T, F)]:.3g}")
    assert bool((out[0, :2, n_mfcc:] == 0).all())                     # the zero prefix: 0, not NaN
    # the state: the maxima themselves
    a = X.abs().amax((1, 2))
    assert torch.equal(state[:, 0], a)
    assert bool(torch.isfinite(state[:, 1]).all()) if n_mfcc else bool((state[:, 1] == -float("inf")).all())
    for chunks in ((T,), (1,) * T, (5, 1, T - 6), (16, 16, T - 32)):
        if min(chunks) < 1:
            continue
        o2, s2 = feat_chunked(X, fbd, dctd, n_mfcc, chunks)
        assert torch.equal(o2, out), (chunks, float((o2 - out).abs().max()))
        assert torch.equal(s2, state), chunks


def test_feat_causal_fwd_against_the_whole_utterance_kernel():
    """Where the two definitions coincide the bits do: with B = 1 the last frame's statistics span the utterance, and an
    utterance whose loudest frame (|X| and dB) is the first has its final statistics from t = 0 on."""
    T, F = 37, 513
    fb, dct = (t.to(DEV) for t in tables(F, 40, 40))
    X = OR.feature_input(3, T, F, seed=7).to(DEV)
    for b in range(3):
        xb = X[b:b + 1].contiguous()
        whole, _ = H().feat_fwd(xb, fb, dct, 40, top_db=80.0, statistics_axis="tf")
        got, _ = feat_causal(xb, fb, dct, 40)
        assert torch.equal(got[:, -1], whole[:, -1]), b
        if b == 1:                                                    # loudest first
            assert torch.equal(got, whole)
        else:
            assert not torch.equal(got, whole)
    plain, _ = H().feat_fwd(X[1:2].contiguous(), None, None, 0, statistics_axis="tf")
    got, _ = feat_causal(X[1:2].contiguous(), None, None, 0)
    assert torch.equal(got, plain)


# ---------------------------------------------------------------------------------------------------- streaming STFT
def stft_stream(x_new, tail):
    rows, n = x_new.shape
    w, _ = hann()
    Tc = n // 256
    X, tail_out = nans(rows, Tc, 513, 2), nans(rows, 768)
    rc = L().tssep_stft_stream_fwd(p(x_new), rows, n, p(tail), p(tail_out), 1024, 256, p(w), p(H().fft_tables(1024, x_new.device)),
                                   p(X), Tc, stream())
    assert rc == 0, rc
    return torch.view_as_complex(X), tail_out


@pytest.mark.parametrize("N", (2381, 2304))
@pytest.mark.parametrize("pushes", ((1, 1, 3, 4), (9,)))
def test_stft_stream_fwd(N, pushes):
    from tssep_amd.train.online import schedule
    rows = 3
    g = torch.Generator(device=DEV).manual_seed(N)
    x = torch.randn(rows, N, device=DEV, generator=g)
    w, _ = hann()
    X_ref = H().stft_fwd(x, w, 1024, 256, True)
    steps = schedule(pushes, N)
    xz = torch.cat([x, x.new_zeros(rows, sum(s.frames for s in steps) * 256 - N)], dim=1)      # the flush: zero-extended
    padded = torch.cat([x.new_zeros(rows, 768), xz], dim=1)
    tail, Xs, pos = None, [], 0
    for s in steps:
        Xc, tail = stft_stream(xz[:, pos:pos + s.frames * 256].contiguous(), tail)
        pos += s.frames * 256
        assert torch.equal(tail, padded[:, pos:pos + 768]), (s, "the tail")
        Xs.append(Xc)
    X = torch.cat(Xs, dim=1)
    assert X.shape == X_ref.shape and X.shape[1] == 9 + (4 if N % 256 else 3)
    assert torch.equal(torch.view_as_real(X), torch.view_as_real(X_ref))


# ------------------------------------------------------------------------------------------------- streaming inverse
def istft_stream(form, frames, obs, ola, skip, n, last, K):
    """form 'plain': frames = X complex [rows, Tc, 513]; 'masked' / 'gated': frames = logit [B, K, Tc, 513 (+ 1)]"""
    _, ws = hann()
    tw = H().fft_tables(1024, torch.device(DEV))
    rows = frames.shape[0] if form == "plain" else frames.shape[0] * K
    Tc = frames.shape[-2]
    y, ola_out = nans(rows, n), nans(rows, 768)
    fr = frames.contiguous()                      # (held until the call returns: a pointer keeps no tensor alive)
    if form == "plain":
        rc = L().tssep_istft_stream_fwd(p(torch.view_as_real(fr)), rows, Tc, 1024, 256, p(ws), p(tw), p(ola), p(ola_out), skip,
                                        last, p(y) if n else None, n, stream())
    else:
        ob = torch.view_as_real(obs.contiguous())
        rc = L().tssep_mask_istft_stream_fwd(p(fr), int(form == "gated"), p(ob), frames.shape[0], K, Tc, 1024, 256, p(ws), p(tw),
                                             p(ola), p(ola_out), skip, last, p(y) if n else None, n, stream())
    assert rc == 0, (rc, form, Tc, skip, n, last)
    return y, ola_out


@pytest.mark.parametrize("form", ("plain", "masked", "gated"))
@pytest.mark.parametrize("T", (13, 70))
def test_istft_stream_fwd(form, T):
    """rows = 2 x 3; T = 70: the second push holds more hops than one workgroup walks (64).  First pushes of 1, 2, 3 and 4
    frames, N ragged and whole, against the whole-utterance entry point of the same form."""
    B, K = 2, 3
    g = torch.Generator(device=DEV).manual_seed(T)
    _, ws = hann()
    obs = torch.view_as_complex(torch.randn(B, T, 513, 2, device=DEV, generator=g))
    if form == "plain":
        frames = torch.view_as_complex(torch.randn(B * K, T, 513, 2, device=DEV, generator=g))
    else:
        frames = torch.randn(B, K, T, 513 + (form == "gated"), device=DEV, generator=g) * 2
    for N in ((T - 3) * 256 - 100, (T - 3) * 256):
        if form == "plain":
            y_ref, _ = H().istft_fwd(frames, ws, N)
        else:
            y_ref, _ = H().mask_istft_fwd(frames, obs, ws, N)
            y_ref = y_ref.reshape(B * K, N)
        for first in (1, 2, 3, 4):
            for pushes in ((first, T - first), (first, 1, 1, T - first - 2)):
                ola, ys, t0, out = None, [], 0, 0
                for i, n_fr in enumerate(pushes):
                    last = i == len(pushes) - 1
                    skip = max(0, 3 - t0)
                    n = max(n_fr - skip, 0) * 256
                    if last:
                        n = N - out
                    y, ola = istft_stream(form, frames[..., t0:t0 + n_fr, :], obs[:, t0:t0 + n_fr], ola, skip, n, int(last), K)
                    ys.append(y)
                    t0, out = t0 + n_fr, out + n
                y = torch.cat(ys, dim=1)
                assert y.shape == y_ref.shape
                assert torch.equal(y, y_ref), (form, T, N, pushes, float((y - y_ref).abs().max()))


# --------------------------------------------------------------------------------------------------------------- guards
def test_guards_refuse_before_any_launch():
    w, ws = hann()
    tw = H().fft_tables(1024, torch.device(DEV))
    x, tail_in, tail_out, X = torch.zeros(2, 512 + 1, device=DEV)[:, :512].contiguous(), torch.zeros(2, 768, device=DEV), nans(2, 768), nans(2, 2, 513, 2)
    buf = torch.zeros(2 * 512 + 2, device=DEV)

    def stft(x_=x, n=512, ti=tail_in, to=tail_out, size=1024, shift=256, Tc=2, X_=X, xoff=0):
        return L().tssep_stft_stream_fwd(p(x_, xoff), 2, n, p(ti), p(to), size, shift, p(w), p(tw), p(X_), Tc, stream())

    assert stft(X_=None) == E_NULL and stft(to=None) == E_NULL
    assert stft(Tc=0, n=0) == E_SHAPE and stft(n=500) == E_SHAPE and stft(ti=tail_out) == E_SHAPE
    assert stft(x_=buf, xoff=4) == E_ALIGN
    assert stft(size=512, shift=128, n=256) == E_UNSUPPORTED
    Xs = torch.zeros(2, 4, 513, 2, device=DEV)
    ola_in, ola_out, y = torch.zeros(2, 768, device=DEV), nans(2, 768), nans(2, 256)

    def inv(X_=Xs, Tc=4, size=1024, shift=256, oi=ola_in, oo=ola_out, skip=3, last=0, y_=y, n=256, xoff=0):
        return L().tssep_istft_stream_fwd(p(X_, xoff), 2, Tc, size, shift, p(ws), p(tw), p(oi), p(oo), skip, last, p(y_), n, stream())

    assert inv(X_=None) == E_NULL and inv(oo=None) == E_NULL and inv(y_=None) == E_NULL
    assert inv(Tc=0) == E_SHAPE and inv(n=200) == E_SHAPE and inv(n=512) == E_SHAPE and inv(skip=4) == E_SHAPE
    assert inv(oi=ola_out) == E_SHAPE and inv(last=1, n=0) == E_SHAPE
    assert inv(xoff=4) == E_ALIGN
    assert inv(size=2048, shift=512) == E_UNSUPPORTED
    lg, ob = torch.zeros(1, 2, 4, 513, device=DEV), torch.zeros(1, 4, 513, 2, device=DEV)

    def minv(lg_=lg, ob_=ob, K=2, oi=ola_in, oo=ola_out, n=256, off=0):
        return L().tssep_mask_istft_stream_fwd(p(lg_), 0, p(ob_, off), 1, K, 4, 1024, 256, p(ws), p(tw), p(oi), p(oo), 3, 0, p(y), n, stream())

    assert minv(lg_=None) == E_NULL and minv(ob_=None) == E_NULL and minv(K=0) == E_SHAPE and minv(oi=ola_out) == E_SHAPE
    assert minv(off=4) == E_ALIGN
    Xf = torch.zeros(2, 3, 513, 2, device=DEV)
    out, st, ws_f = nans(2, 3, 516), nans(2, 2), nans(int(L().tssep_feat_causal_workspace_bytes(2, 3, 0, 513)) // 4 + 4)

    def feat(X_=Xf, T=3, si=None, so=st, out_=out, w_=ws_f, woff=0, ld=516):
        return L().tssep_feat_causal_fwd(p(X_), 2, T, 513, None, None, 0, 0, 80.0, p(si), p(so), p(out_), ld, p(w_, woff), stream())

    assert feat(X_=None) == E_NULL and feat(out_=None) == E_NULL and feat(w_=None) == E_NULL
    assert feat(T=0) == E_SHAPE and feat(ld=512) == E_SHAPE and feat(si=st) == E_SHAPE
    assert feat(woff=4) == E_ALIGN
    assert L().tssep_feat_causal_workspace_bytes(0, 3, 0, 513) == 0
    torch.cuda.synchronize()
    for t in (tail_out, X, ola_out, y, out, st):                    # nothing was launched: every output is still NaN
        assert bool(torch.isnan(t).all())
    assert stft() == 0 and inv() == 0 and minv() == 0 and feat() == 0
    torch.cuda.synchronize()
    for t in (tail_out, X, ola_out, y, out[..., :513], st[:, 0]):
        assert not bool(torch.isnan(t).any())


def test_zz_report():
    for k, v in sorted(WORST.items()):
        print(f"feat_causal_fwd {k}: worst error / tolerance {v:.3g}")
