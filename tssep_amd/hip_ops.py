"""Tensor-level wrappers over the C ABI (include/tssep_hip.h).

PyTorch is used for device memory and the current HIP stream only; every computation below
is a call into libtssep_hip.so.  Nothing here falls back to ATen math.
"""
import collections
import ctypes
import functools
import itertools
import math

import numpy as np
import torch

from . import _lib
from ._lib import GemmArgs, LstmSizes, check


# ---- optional live kernel timing (bench.py): HIP events on the launch stream -----------------
KERNEL_TIMING = False
KERNEL_TIMERS = {}      # name -> list of (start_event, end_event)
KERNEL_FLOPS = {}       # name -> algorithmic FLOPs accumulated over the timed launches
KERNEL_BYTES = {}       # name -> algorithmic HBM bytes accumulated over the timed launches


class _timed:
    def __init__(self, name, flops=0, nbytes=0):
        self.name, self.flops, self.nbytes = name, flops, nbytes

    def __enter__(self):
        if KERNEL_TIMING:
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)
            self.s.record()
        return self

    def __exit__(self, *a):
        if KERNEL_TIMING:
            self.e.record()
            KERNEL_TIMERS.setdefault(self.name, []).append((self.s, self.e))
            KERNEL_FLOPS[self.name] = KERNEL_FLOPS.get(self.name, 0) + self.flops
            KERNEL_BYTES[self.name] = KERNEL_BYTES.get(self.name, 0) + self.nbytes


KERNEL_OWN_BYTES = {}   # name -> bytes the kernel that actually runs must move (fused kernels: not the unfused chain's)


def _own_bytes(name, nbytes):
    if KERNEL_TIMING:
        KERNEL_OWN_BYTES[name] = KERNEL_OWN_BYTES.get(name, 0) + nbytes


def kernel_time_summary():
    torch.cuda.synchronize()
    return {k: (len(v), sum(s.elapsed_time(e) for s, e in v)) for k, v in KERNEL_TIMERS.items()}


def _addr(t):
    """Device address of a tensor, or of (tensor, float_offset); None stays None."""
    if isinstance(t, tuple):
        return t[0].data_ptr() + 4 * t[1]
    return t.data_ptr() if t is not None else None


def _p(t):
    """`_addr` as the pointer argument of a C entry point."""
    a = _addr(t)
    return ctypes.c_void_p(a) if a is not None else None


def _device_of(t):
    """Device of a tensor, or of (tensor, float_offset)."""
    return (t[0] if isinstance(t, tuple) else t).device


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _f32(t):
    assert t.is_cuda and t.dtype == torch.float32, (t.device, t.dtype)
    return t


def round_up(x, m):
    return (x + m - 1) // m * m


def rows_view(t):
    """Return (tensor, ld) of a 2-D-like fp32 tensor whose rows are 16-byte aligned.
    Accepts [..., C] with unit inner stride and uniform row stride; copies into a padded
    buffer otherwise (layout glue only)."""
    _f32(t)
    c = t.shape[-1]
    t2 = t.reshape(-1, c) if t.is_contiguous() else t
    if t2.dim() == 2 and t2.stride(1) == 1 and t2.stride(0) % 4 == 0 and t2.data_ptr() % 16 == 0 \
            and (t2.shape[0] == 1 or t2.stride(0) >= c):
        return t2, t2.stride(0)
    ld = round_up(c, 4)
    buf = torch.zeros(t.numel() // c, ld, device=t.device, dtype=torch.float32)
    buf[:, :c] = t.reshape(-1, c)
    return buf, ld


def padded(rows, cols, device, zero=True):
    """[rows, cols] view of a buffer with leading dimension round_up(cols, 4).  zero: the pad columns get a defined
    value here (consumers read whole 16-byte groups); False where the producer writes them itself."""
    ld = round_up(cols, 4)
    buf = torch.empty(rows, ld, device=device, dtype=torch.float32)
    if zero and ld != cols:   # only the pad columns (the producers write the rest)
        buf[:, cols:].zero_()
    return buf, ld


# ----------------------------------------------------------------------------- probes
def probe_xcc(nblocks=256):
    out = torch.full((nblocks,), -1, device="cuda", dtype=torch.int32)
    check(_lib.lib().tssep_probe_xcc(_p(out), nblocks, _stream()), "probe_xcc")
    return out


def probe_clock(heavy=True, nblocks=1024, iters=200000):
    """-> (shader MHz, MFMA TFLOP/s of the probe) under that load."""
    out = torch.zeros(2 * nblocks, device="cuda", dtype=torch.int64)
    check(_lib.lib().tssep_probe_clock(_p(out), nblocks, iters, int(heavy), _stream()), "probe_clock")
    o = out.cpu().view(nblocks, 2).double()
    mhz = float((o[:, 0] / o[:, 1]).mean() * 100.0)
    return mhz


def probe_mfma():
    L = _lib.lib()
    o4 = torch.zeros(64, 4, device="cuda")
    o32 = torch.zeros(2, 64, 16, device="cuda")
    check(L.tssep_probe_mfma(_p(o4), _p(o32), _stream()), "probe_mfma")
    return o4.cpu(), o32.cpu()


# ------------------------------------------------------------------------------- STFT
_TABLES = {}


def fft_tables(size, device):
    key = (size, str(device))
    if key not in _TABLES:
        L = _lib.lib()
        n = 2 * (size // 2 + size // 2 + 1)
        host = np.zeros(n, dtype=np.float32)
        check(L.tssep_fft_twiddles(size, host.ctypes.data_as(ctypes.c_void_p)), "fft_twiddles")
        _TABLES[key] = torch.from_numpy(host).to(device)
    return _TABLES[key]


def stft_frames(N, size=1024, shift=256, window_length=None, pad=True, fading=True):
    return int(_lib.lib().tssep_stft_frames(N, size, shift, window_length or size, int(pad),
                                            int(fading)))


def stft_fwd(x, window, size=1024, shift=256, fading=True, T=None):
    """x [rows, N] -> complex64 [rows, T, size//2+1].  fading: size - shift zeros in front (True) or none (False);
    T: frame count when it is not the padded, full-window one (pad=False, window_length < size: the caller's
    feature extractor computes it; frames that reach past the signal read zeros)."""
    L = _lib.lib()
    x = _f32(x).contiguous()
    rows, N = x.shape
    if T is None:
        T = stft_frames(N, size, shift, None, True, fading)
    X = torch.empty(rows, T, size // 2 + 1, 2, device=x.device, dtype=torch.float32)
    check(L.tssep_stft_fwd(_p(x), rows, N, size, shift, int(fading), _p(window),
                           _p(fft_tables(size, x.device)), _p(X), T, _stream()), "stft_fwd")
    return torch.view_as_complex(X)


def stft_framemag(x, window, size=1024, shift=256, fading=True, T=None):
    """x [rows, N] -> a [rows, T] float32, a[r,t] = sum_f |stft_fwd(x)[r,t,f]| without the spectrum (arguments as stft_fwd)."""
    L = _lib.lib()
    x = _f32(x).contiguous()
    rows, N = x.shape
    if T is None:
        T = stft_frames(N, size, shift, None, True, fading)
    a = torch.empty(rows, T, device=x.device, dtype=torch.float32)
    with _timed("stft_framemag", 0, 4 * rows * (N + T)):
        check(L.tssep_stft_framemag_fwd(_p(x), rows, N, size, shift, int(fading), _p(window),
                                        _p(fft_tables(size, x.device)), _p(a), T, _stream()), "stft_framemag")
    return a


def framemag(X):
    """X [rows, T, F] complex64 or float32 -> a [rows, T] float32, a[r,t] = sum_f |X[r,t,f]|."""
    assert X.is_cuda and X.dim() == 3 and X.dtype in (torch.complex64, torch.float32), (X.device, X.shape, X.dtype)
    X = X.contiguous()
    rows, T, F = X.shape
    cplx = X.is_complex()
    a = torch.empty(rows, T, device=X.device, dtype=torch.float32)
    with _timed("framemag", 0, 4 * rows * T * ((2 if cplx else 1) * F + 1)):
        check(_lib.lib().tssep_framemag_fwd(_p(torch.view_as_real(X) if cplx else X), int(cplx), rows, T, F, _p(a),
                                            _stream()), "framemag")
    return a


def vad_from_mag(a, threshold):
    """a [rows, T] -> float32 [rows, T] of 0 / 1: a / amax(a, -1, keepdim=True) > threshold (loss.py:319-321), the decisions
    of that torch expression on a float32 tensor bit for bit."""
    a = _f32(a).contiguous()
    rows, T = a.shape
    vad = torch.empty_like(a)
    with _timed("vad_from_mag", 0, 8 * rows * T):
        check(_lib.lib().tssep_vad_from_mag(_p(a), rows, T, float(threshold), _p(vad), _stream()), "vad_from_mag")
    return vad


_FADING_CODE = {None: 0, False: 0, True: 1, "full": 1, "half": 2}


def vad_frames(vad, window_length, shift, fading=True):
    """Sample activity vad [rows, N] (bool or uint8 as they are, any other dtype through `!= 0`) -> frame activity
    float32 [rows, T], T = the padded frame count: util.utils.stft_vad as a gather on the device."""
    assert vad.is_cuda and vad.dim() == 2, (vad.device, vad.shape)
    if vad.dtype == torch.bool:
        v = vad.contiguous().view(torch.uint8)
    elif vad.dtype == torch.uint8:
        v = vad.contiguous()
    else:
        v = (vad != 0).view(torch.uint8)
    rows, N = v.shape
    pad = window_length - shift
    n = N + {0: 0, 1: 2 * pad, 2: pad}[_FADING_CODE[fading]]
    T = -(-(n - window_length + shift) // shift)               # utils.samples_to_stft_frames(pad=True)
    out = torch.empty(rows, max(T, 0), device=v.device, dtype=torch.float32)
    if T <= 0:
        return out
    with _timed("vad_frames", 0, rows * T * 5):
        check(_lib.lib().tssep_vad_frames(_p(v), rows, N, int(window_length), int(shift), _FADING_CODE[fading], _p(out), T,
                                          _stream()), "vad_frames")
    return out


def istft_fwd(X, wsyn, N, size=1024, shift=256, fading=True, tgt=None):
    """X complex64 [rows, T, F] -> y [rows, N] (+ per-chunk sums of |y - tgt| when tgt given)"""
    L = _lib.lib()
    Xr = torch.view_as_real(X.contiguous())
    rows, T = X.shape[0], X.shape[1]
    y = torch.empty(rows, N, device=X.device, dtype=torch.float32)
    part = None
    if tgt is not None:
        nch = int(L.tssep_istft_chunks(N))
        part = torch.empty(rows, nch, device=X.device, dtype=torch.float32)
        tgt = _f32(tgt).contiguous()
    check(L.tssep_istft_fwd(_p(Xr), rows, T, size, shift, int(fading), _p(wsyn),
                            _p(fft_tables(size, X.device)), _p(y), N, _p(tgt), _p(part),
                            _stream()), "istft_fwd")
    return y, part


def istft_bwd(dy, wsyn, T, size=1024, shift=256, fading=True):
    L = _lib.lib()
    dy = _f32(dy).contiguous()
    rows, N = dy.shape
    dX = torch.empty(rows, T, size // 2 + 1, 2, device=dy.device, dtype=torch.float32)
    check(L.tssep_istft_bwd(_p(dy), rows, N, size, shift, int(fading), _p(wsyn),
                            _p(fft_tables(size, dy.device)), _p(dX), T, _stream()), "istft_bwd")
    return torch.view_as_complex(dX)


def _tail_rows(logit, obs):
    """The fused tail's row layout -> (B, K, T, F, gated): logit [B,K,T,F] (plain) or [B,K,T,F+1] with the VAD logit at
    column 0 (explicit_vad: gated), obs complex64 [B,T,F].  The one place that decides it."""
    B, K, T, Fl = logit.shape
    F = obs.shape[-1]
    assert Fl - F in (0, 1), f"mask_istft: logit rows of {Fl} columns for {F} bins (F: plain rows, F + 1: gated rows)"
    assert tuple(obs.shape) == (B, T, F) and obs.dtype == torch.complex64, (tuple(logit.shape), tuple(obs.shape), obs.dtype)
    return B, K, T, F, Fl == F + 1


def mask_istft_fwd(logit, obs, wsyn, N, size=1024, shift=256, fading=True, tgt=None):
    """logit [B,K,T,F], obs complex64 [B,T,F] -> y [B,K,N] = istft(sigmoid(logit) * obs), neither the mask
    nor the masked STFT is materialised (+ per-chunk sums of |y - tgt| when tgt [B,K,N] is given).
    explicit_vad: logit [B,K,T,F+1] (VAD logit at column 0) -> y = istft(sigmoid(l) sigmoid(v) * obs)."""
    L = _lib.lib()
    B, K, T, F, gated = _tail_rows(logit, obs)
    assert tgt is None or tuple(tgt.shape) == (B, K, N), (tuple(tgt.shape), (B, K, N))
    logit = _f32(logit).contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    y = torch.empty(B, K, N, device=logit.device, dtype=torch.float32)
    part = None
    if tgt is not None:
        part = torch.empty(B * K, int(L.tssep_istft_chunks(N)), device=logit.device, dtype=torch.float32)
        tgt = _f32(tgt).contiguous()
    if gated:
        entry, name, timer = L.tssep_mask_istft_gated_fwd, "mask_istft_gated_fwd", _timed(
            "maskhead_gated_fwd", 0, B * T * (4 * K * (F + 1) + 8 * F) + 4 * B * K * N)
    else:
        # roofline bookkeeping: the UNFUSED mask head's algorithmic bytes, whatever is moved; the fused kernel's
        # OWN bytes (logit + observation in, samples out, target in when the loss sums ride along) are kept beside them
        _own_bytes("maskhead_fwd", B * T * (4 * K * F + 8 * F) + 4 * B * K * N * (2 if tgt is not None else 1))
        entry, name, timer = L.tssep_mask_istft_fwd, "mask_istft_fwd", _timed("maskhead_fwd", 0, B * T * (16 * K * F + 8 * F))
    with timer:
        check(entry(_p(logit), _p(obs_r), B, K, T, size, shift, int(fading), _p(wsyn), _p(fft_tables(size, logit.device)),
                    _p(y), N, _p(tgt), _p(part), _stream()), name)
    return y, part


def mask_istft_bwd(dy, logit, obs, wsyn, size=1024, shift=256, fading=True, loss=None, vad=None, iperm=None,
                   bt_major=False):
    """dy [B,K,N] -> dlogit (the shape of logit) through the iSTFT adjoint and the mask head's backward.
    loss = (est, tgt, sums or None, gout): the loss gradient is formed inside the kernel from the estimate
    and the target instead of being read from `dy` (LogMAE; sums None: MAE).  bt_major: the result is laid
    out [B*T, K*F] with speaker k at position iperm[b, k] -- what the final Linear's backward reads.
    Gated rows only: vad = (Vad [B,K,T], gout_vad [B]) adds the gate column's BCE gradient in the same store."""
    L = _lib.lib()
    B, K, T, F, gated = _tail_rows(logit, obs)
    assert vad is None or gated, "mask_istft_bwd: vad= needs gated logit rows (F + 1 columns, the VAD logit at column 0)"
    Fl = logit.shape[-1]
    logit = _f32(logit).contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    dlogit = torch.empty(B * T, K * Fl, device=logit.device, dtype=torch.float32) if bt_major else torch.empty_like(logit)
    if loss is None:
        x, tgt, sums, gout = _f32(dy).contiguous(), None, None, None
    else:
        x, tgt, sums, gout = (_f32(loss[0]).contiguous(), _f32(loss[1]).contiguous(),
                              _f32(loss[2]).contiguous() if loss[2] is not None else None, _f32(loss[3]).contiguous())
    assert tuple(x.shape[:2]) == (B, K) and (tgt is None or tgt.shape == x.shape), (tuple(x.shape), B, K)
    assert (gout is None or gout.numel() == B) and (sums is None or sums.numel() == B)
    N = x.shape[-1]
    tail = (size, shift, int(fading), _p(wsyn), _p(fft_tables(size, logit.device)))
    if gated:
        v = gv = None
        if vad is not None:
            v, gv = _f32(vad[0]).contiguous(), _f32(vad[1]).contiguous()
            assert tuple(v.shape) == (B, K, T) and gv.numel() == B, (tuple(v.shape), (B, K, T), gv.numel())
        with _timed("maskhead_gated_bwd", 0, B * T * (8 * K * Fl + 8 * F) + 4 * B * K * N):
            check(L.tssep_mask_istft_gated_bwd(_p(x), _p(tgt), _p(sums), _p(gout), _p(v), _p(gv), _p(logit), _p(obs_r),
                                               B, K, N, *tail, _p(iperm), int(bt_major), _p(dlogit), T, _stream()),
                  "mask_istft_gated_bwd")
        return dlogit
    _own_bytes("maskhead_bwd", B * T * (8 * K * F + 8 * F) + 4 * B * K * N * (1 if loss is None else 2))
    with _timed("maskhead_bwd", 0, B * T * (16 * K * F + 8 * F)):
        if loss is None and not bt_major:
            check(L.tssep_mask_istft_bwd(_p(x), _p(logit), _p(obs_r), B, K, N, *tail, _p(dlogit), T, _stream()),
                  "mask_istft_bwd")
        else:
            check(L.tssep_mask_istft_bwd_loss(_p(x), _p(tgt), _p(sums), _p(gout), _p(logit), _p(obs_r), B, K, N, *tail,
                                              _p(iperm), int(bt_major), _p(dlogit), T, _stream()), "mask_istft_bwd_loss")
    return dlogit


# --------------------------------------------------------------------------- features
STAT_AXES = {"tf": 0, "t": 1, "f": 2}


def feat_fwd(X, fb, dct, n_mfcc, top_db=80.0, statistics_axis="tf"):
    """X complex64 [B,T,F] -> (view [B,T,n_mfcc+F], ld)."""
    L = _lib.lib()
    Xr = torch.view_as_real(X.contiguous())
    B, T, F = X.shape
    n_mels = fb.shape[1] if n_mfcc else 0
    if n_mfcc:
        fb, dct = _f32(fb).contiguous(), _f32(dct).contiguous()
    D = n_mfcc + F
    ld = round_up(D, 4)
    out = torch.empty(B, T, ld, device=X.device, dtype=torch.float32)
    if ld != D:
        out[..., D:].zero_()
    stat = STAT_AXES[statistics_axis]
    ws = torch.empty(int(L.tssep_feat_workspace_bytes(B, T, max(n_mels, 1), F, stat)) // 4 + 4,
                     device=X.device, dtype=torch.float32)
    check(L.tssep_feat_fwd(_p(Xr), B, T, F, _p(fb) if n_mfcc else None,
                           _p(dct) if n_mfcc else None, n_mels, n_mfcc, float(top_db), stat, _p(out),
                           ld, _p(ws), _stream()), "feat_fwd")
    return out[..., :D], ld


def feat_causal_fwd(X, fb, dct, n_mfcc, top_db=80.0, state=None):
    """feat_fwd('tf') with causal statistics: X complex64 [B,Tc,F], a chunk of each utterance's frames -> (view
    [B,Tc,n_mfcc+F], ld, state_out).  state [B,2] = {running max |X|, running max dB} in front of the chunk (None: a fresh
    stream); state_out is a new tensor, the state behind it."""
    L = _lib.lib()
    Xr = torch.view_as_real(X.contiguous())
    B, T, F = X.shape
    n_mels = fb.shape[1] if n_mfcc else 0
    if n_mfcc:
        fb, dct = _f32(fb).contiguous(), _f32(dct).contiguous()
    if state is not None:
        state = _f32(state).contiguous()
        assert tuple(state.shape) == (B, 2), (tuple(state.shape), B)
    D = n_mfcc + F
    ld = round_up(D, 4)
    out = torch.empty(B, T, ld, device=X.device, dtype=torch.float32)
    if ld != D:
        out[..., D:].zero_()
    state_out = torch.empty(B, 2, device=X.device, dtype=torch.float32)
    ws = torch.empty(int(L.tssep_feat_causal_workspace_bytes(B, T, n_mels, F)) // 4 + 4, device=X.device,
                     dtype=torch.float32)
    with _timed("feat_causal", 0, B * T * (16 * F + 4 * D)):
        check(L.tssep_feat_causal_fwd(_p(Xr), B, T, F, _p(fb) if n_mfcc else None, _p(dct) if n_mfcc else None, n_mels,
                                      n_mfcc, float(top_db), _p(state), _p(state_out), _p(out), ld, _p(ws), _stream()),
              "feat_causal_fwd")
    return out[..., :D], ld, state_out


SPECFEAT_KINDS = {"abs": 0, "log1p": 1, "mvn": 2}      # tssep_specfeat_fwd's `kind`
SPECFEAT_MAX_BINS = 1025


def _specfeat_args(name, X, out, col0):
    """Shared argument work of the two spectral-feature calls -> (X as float32 pairs, B, T, F, the [B,T,>= col0 + F] buffer,
    its row pitch).  `out` None: a fresh buffer whose padding columns are zeroed (as feat_fwd's)."""
    if not isinstance(X, torch.Tensor) or X.dim() != 3 or X.dtype != torch.complex64:
        got = f"{X.dtype} {tuple(X.shape)}" if isinstance(X, torch.Tensor) else type(X).__name__
        raise ValueError(f"{name}: X is complex64 [B,T,F], got {got}")
    assert X.is_cuda, X.device
    B, T, F = X.shape
    col0 = int(col0)
    if out is None:
        if col0:
            raise ValueError(f"{name}: col0 = {col0} names a column of `out`, and no `out` was given")
        ld = round_up(F, 4)
        out = torch.empty(B, T, ld, device=X.device, dtype=torch.float32)
        if ld != F:
            out[..., F:].zero_()
    else:
        ok = isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.dim() == 3
        if not ok or tuple(out.shape[:2]) != (B, T) or col0 < 0 or col0 + F > out.shape[2] or out.stride(2) != 1 \
                or out.stride(1) < out.shape[2] or (B > 1 and out.stride(0) != T * out.stride(1)):
            got = f"{out.dtype} {tuple(out.shape)} strides {out.stride()}" if isinstance(out, torch.Tensor) else type(out).__name__
            raise ValueError(f"{name}: out is a float32 [B = {B}, T = {T}, >= col0 + F = {col0} + {F}] buffer with unit "
                             f"column stride and one row pitch, got {got}")
    return torch.view_as_real(X.contiguous()), B, T, F, out, out.stride(1)


def specfeat_fwd(X, kind, out=None, col0=0):
    """X complex64 [B,T,F] -> view [B,T,F]: kind 0 | 'abs' = |X|, 1 | 'log1p' = log1p|X|, 2 | 'mvn' = log1p|X| minus its
    mean over the T frames.  out / col0: write columns [col0, col0 + F) of an existing float32 [B,T,ld] buffer (or a view
    of one) and return that view -- no copy, nothing else of the buffer is touched."""
    L = _lib.lib()
    kind = SPECFEAT_KINDS.get(kind, kind)
    Xr, B, T, F, out, ld = _specfeat_args("specfeat_fwd", X, out, col0)
    nws = int(L.tssep_specfeat_workspace_bytes(B, T, F, int(kind)))
    ws = torch.empty(nws // 8, device=X.device, dtype=torch.float64) if nws else None
    with _timed("specfeat", 0, B * T * F * (12 if kind != 2 else 20)):
        check(L.tssep_specfeat_fwd(_p(Xr), B, T, F, int(kind), _p((out, int(col0))), ld, _p(ws), _stream()), "specfeat_fwd")
    return out[..., int(col0):int(col0) + F]


def specfeat_causal_state_check(state, B, F):
    """A carried state of `specfeat_causal_fwd` is float64 [B, F + 1]: say what arrived instead."""
    if state is None:
        return
    if not isinstance(state, torch.Tensor) or state.dtype != torch.float64 or tuple(state.shape) != (B, F + 1):
        got = f"{state.dtype} {tuple(state.shape)}" if isinstance(state, torch.Tensor) else type(state).__name__
        raise ValueError(f"specfeat_causal_fwd: state is {got}, what a call with B = {B}, F = {F} carries is torch.float64 "
                         f"{(B, F + 1)}: the sums S[b, f] and the weight n[b] (did the batch or the FFT size change between "
                         "the calls of a stream, or was the state of another feature passed?)")


def specfeat_causal_fwd(X, state=None, forgetting=1.0, out=None, col0=0):
    """The running-mean form of kind 2 on the next Tc frames of a stream: X complex64 [B,Tc,F], state what the call before
    returned (None: a fresh stream) -> (view [B,Tc,F], state_out float64 [B, F + 1], a new tensor).  Per frame
    S = a S + L, n = a n + 1, out = L - S / n with a = forgetting in (0, 1]; outputs and state do not depend on how the
    frames are split over calls.  out / col0 as in `specfeat_fwd`."""
    L = _lib.lib()
    if not 0.0 < float(forgetting) <= 1.0:
        raise ValueError(f"specfeat_causal_fwd: forgetting = {forgetting} lies outside (0, 1]")
    Xr, B, T, F, out, ld = _specfeat_args("specfeat_causal_fwd", X, out, col0)
    specfeat_causal_state_check(state, B, F)
    if state is not None:
        assert state.is_cuda, state.device
        state = state.contiguous()
    state_out = torch.empty(B, F + 1, device=X.device, dtype=torch.float64)
    with _timed("specfeat_causal", 0, B * T * F * 12 + 16 * B * (F + 1)):
        check(L.tssep_specfeat_causal_fwd(_p(Xr), B, T, F, float(forgetting), _p(state), _p(state_out),
                                          _p((out, int(col0))), ld, _stream()), "specfeat_causal_fwd")
    return out[..., int(col0):int(col0) + F], state_out


# ----------------------------------------------------------------------------- online
def stft_stream_fwd(x_new, tail, window, size=1024, shift=256):
    """The frames a push completes: x_new [rows, Tc * shift] behind tail [rows, size - shift] (None: a fresh stream, the
    leading fade) -> (X complex64 [rows, Tc, size//2+1] with stft_fwd's bits for those frames, the new tail)."""
    L = _lib.lib()
    x_new = _f32(x_new).contiguous()
    rows, n = x_new.shape
    Tc = n // shift
    if tail is not None:
        tail = _f32(tail).contiguous()
        assert tuple(tail.shape) == (rows, size - shift), (tuple(tail.shape), rows, size - shift)
    tail_out = torch.empty(rows, size - shift, device=x_new.device, dtype=torch.float32)
    X = torch.empty(rows, Tc, size // 2 + 1, 2, device=x_new.device, dtype=torch.float32)
    check(L.tssep_stft_stream_fwd(_p(x_new), rows, n, _p(tail), _p(tail_out), size, shift, _p(window),
                                  _p(fft_tables(size, x_new.device)), _p(X), Tc, _stream()), "stft_stream_fwd")
    return torch.view_as_complex(X), tail_out


def _stream_hops(Tc, skip, shift, N):
    """(samples of y, last) for a call of Tc frames whose first `skip` hops are not stored; N: the samples that remain of
    the utterance (the final call), None: whole hops."""
    full = max(Tc - skip, 0) * shift
    return (full, 0) if N is None else (min(int(N), full), 1)


def istft_stream_fwd(X, wsyn, ola, skip, N=None, size=1024, shift=256):
    """The hops the stream's next frames complete: X complex64 [rows, Tc, F], ola [rows, size - shift] the carry in front
    (None: a fresh stream), skip = max(0, 3 - frames seen before) -> (y [rows, (Tc - skip) * shift], or its first N
    samples in the utterance's final call; the carry behind)."""
    L = _lib.lib()
    Xr = torch.view_as_real(X.contiguous())
    rows, Tc = X.shape[0], X.shape[1]
    n, last = _stream_hops(Tc, skip, shift, N)
    ola = None if ola is None else _f32(ola).contiguous()
    y = torch.empty(rows, n, device=X.device, dtype=torch.float32)
    ola_out = torch.empty(rows, size - shift, device=X.device, dtype=torch.float32)
    check(L.tssep_istft_stream_fwd(_p(Xr), rows, Tc, size, shift, _p(wsyn), _p(fft_tables(size, X.device)),
                                   _p(ola), _p(ola_out), int(skip), last,
                                   _p(y) if n else None, n, _stream()), "istft_stream_fwd")
    return y, ola_out


def mask_istft_stream_fwd(logit, obs, wsyn, ola, skip, N=None, size=1024, shift=256):
    """mask_istft_fwd on the stream's next frames: logit [B,K,Tc,F] (gated: [B,K,Tc,F+1]), obs complex64 [B,Tc,F], ola
    [B*K, size - shift] or None -> (y [B,K,n], the carry behind); arguments as istft_stream_fwd."""
    L = _lib.lib()
    B, K, Tc, F, gated = _tail_rows(logit, obs)
    logit = _f32(logit).contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    n, last = _stream_hops(Tc, skip, shift, N)
    ola = None if ola is None else _f32(ola).contiguous()
    y = torch.empty(B, K, n, device=logit.device, dtype=torch.float32)
    ola_out = torch.empty(B * K, size - shift, device=logit.device, dtype=torch.float32)
    with _timed("maskhead_stream", 0, B * Tc * (4 * K * logit.shape[-1] + 8 * F) + 4 * B * K * n):
        check(L.tssep_mask_istft_stream_fwd(_p(logit), int(gated), _p(obs_r), B, K, Tc, size, shift, _p(wsyn),
                                            _p(fft_tables(size, logit.device)),
                                            _p(ola), _p(ola_out), int(skip), last,
                                            _p(y) if n else None, n, _stream()), "mask_istft_stream_fwd")
    return y, ola_out


def _stream_grads(dy, d_ola_out, rows, Tc, skip, N, size, shift, device, want_ola):
    """The gradient arguments of a stream backward: dy [rows, n] or None (the call completed no sample, or nobody used
    them: zeros), d_ola_out [rows, size - shift] or None (the kernel's NULL) -> (dy, d_ola_out, n, last, d_ola_in)."""
    n, last = _stream_hops(Tc, skip, shift, N)
    if dy is None:
        dy = torch.zeros(rows, n, device=device, dtype=torch.float32) if n else None
    else:
        assert dy.numel() == rows * n, (tuple(dy.shape), rows, n)
        dy = _f32(dy).contiguous().reshape(rows, n)
    if d_ola_out is not None:
        d_ola_out = _f32(d_ola_out).contiguous()
        assert tuple(d_ola_out.shape) == (rows, size - shift), (tuple(d_ola_out.shape), rows, size - shift)
    d_ola_in = torch.empty(rows, size - shift, device=device, dtype=torch.float32) if want_ola else None
    return dy, d_ola_out, n, last, d_ola_in


def istft_stream_bwd(dy, d_ola_out, wsyn, Tc, skip, N=None, size=1024, shift=256, want_ola=True):
    """The backward of istft_stream_fwd(X [rows, Tc, F], ...) with the same skip and N: dy [rows, n] (None: zeros),
    d_ola_out [rows, size - shift] the gradient of the carry behind the call (None: the stream is cut there) ->
    (dX complex64 [rows, Tc, F], d_ola_in or None).  `rows` is read from dy, or from d_ola_out when dy is None."""
    L = _lib.lib()
    ref = dy if dy is not None else d_ola_out
    rows, device = ref.shape[0], ref.device
    dy, d_ola_out, n, last, d_ola_in = _stream_grads(dy, d_ola_out, rows, Tc, skip, N, size, shift, device, want_ola)
    F = size // 2 + 1
    dX = torch.empty(rows, Tc, F, 2, device=device, dtype=torch.float32)
    with _timed("maskhead_stream_bwd", 0, 8 * rows * Tc * F + 4 * rows * n):
        check(L.tssep_istft_stream_bwd(_p(dy) if n else None, _p(d_ola_out), rows, Tc, size, shift, _p(wsyn),
                                       _p(fft_tables(size, device)), int(skip), last, n, _p(dX), _p(d_ola_in), _stream()),
              "istft_stream_bwd")
    return torch.view_as_complex(dX), d_ola_in


def mask_istft_stream_bwd(dy, d_ola_out, logit, obs, wsyn, skip, N=None, size=1024, shift=256, want_ola=True):
    """The backward of mask_istft_stream_fwd(logit, obs, ...) with the same skip and N: dy [B,K,n] (None: zeros),
    d_ola_out [B*K, size - shift] (None: the stream is cut behind this call) -> (dlogit, the shape of logit; d_ola_in
    [B*K, size - shift] or None).  obs gets no gradient."""
    L = _lib.lib()
    B, K, Tc, F, gated = _tail_rows(logit, obs)
    logit = _f32(logit).contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    dy, d_ola_out, n, last, d_ola_in = _stream_grads(dy, d_ola_out, B * K, Tc, skip, N, size, shift, logit.device, want_ola)
    dlogit = torch.empty_like(logit)
    if TAIL_LOG is not None:
        TAIL_LOG.append(dict(kernel="maskhead_stream_bwd", B=B, K=K, T=Tc, F=F, gated=bool(gated), skip=int(skip), N=n,
                             carry=d_ola_out is not None))
    with _timed("maskhead_stream_bwd", 0, B * Tc * (8 * K * logit.shape[-1] + 8 * F) + 4 * B * K * n):
        check(L.tssep_mask_istft_stream_bwd(_p(dy) if n else None, _p(d_ola_out), _p(logit), int(gated), _p(obs_r), B, K, Tc,
                                            size, shift, _p(wsyn), _p(fft_tables(size, logit.device)), int(skip), last, n,
                                            _p(dlogit), _p(d_ola_in), _stream()), "mask_istft_stream_bwd")
    return dlogit, d_ola_in


# ------------------------------------------------------------------------------- GEMM
# Arithmetic of the non-recurrent GEMMs: "bf16x3" = split-bf16 on the bf16 MFMA with fp32 accumulation (fp32-class
# accuracy: masks 3e-6 from the CPU oracle, see gemm_bf16x3.hip) -- the DEFAULT since round 5: what bench.py measures is
# what `python -m tssep_amd.exp.run_tssep` trains with; "f32" = exact fp32 MFMA (the reference's GEMM arithmetic).  The
# recurrence kernel (exact fp32 or split-bf16) is chosen separately by recurrence_plan().
# This module reads NO environment variable: every policy attribute below has its default here and is set -- recorded
# in config.yaml / log/runtime.json -- through tssep_amd.train.runtime (`eg.runtime.*`, `bench.py --runtime k=v`).
GEMM_PRECISION = "bf16x3"
_PREC = {"f32": 0, "bf16x3": 1, "bf16": 3}      # "bf16": the plain-bf16 side line (tssep_gemm_args.precision = 3)


def _gemm_args(A, lda, B, ldb, C, ldc, M, N, K, a_kmajor=False, b_kmajor=False, bias=None, act=0,
               accumulate=False, b_kshift=0, kperiod=0, remap=None, splitk=1, split_stride=0,
               b_ones_col=False, aux=None):
    g = GemmArgs()
    g.A, g.B, g.C = _addr(A), _addr(B), _addr(C)
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = lda, ldb, ldc
    g.a_kmajor, g.b_kmajor = int(a_kmajor), int(b_kmajor)
    g.b_kshift, g.kperiod = b_kshift, kperiod
    g.bias = _addr(bias)
    g.act, g.accumulate = act, int(accumulate)
    if remap is not None:
        g.c_remap = 2 if remap.get("narrow") else 1      # (2: the 4-byte-per-lane store, the reference of the tests)
        g.c_T, g.c_K = remap["T"], remap.get("K", 1)
        g.c_sb, g.c_sk, g.c_st = remap["sb"], remap.get("sk", 0), remap["st"]
        g.c_cm, g.c_co = remap.get("cm", 0), remap.get("co", 0)
        perm = remap.get("perm")
        g.c_perm = _addr(perm)
        g.c_perm_ld = remap.get("perm_ld", 0)
    g.splitk, g.c_split_stride = splitk, split_stride
    g.precision = _PREC[GEMM_PRECISION]
    g.b_ones_col = int(b_ones_col)
    if act == 2:        # tanh backward folded into the store: aux = (tensor, ld) of the tanh OUTPUT, indexed like C
        assert aux is not None and splitk <= 1
        g.aux, g.ldaux = _addr(aux[0]), aux[1]
    return g


# Kernel ids of include/tssep_hip.h (TSSEP_GEMM_*).  The library chooses by itself; tests, the shape sweep and the
# A/B tools may name kernels to be tried first: GEMM_PREFER = ("stream", "tall2") launches the first one of them that
# covers the request (asked through tssep_gemm_plan) and the library's own choice when none does.
GEMM_KERNEL_NAMES = {}      # id -> name, as the library's candidate table names them (tssep_gemm_kernel_name; "?" past the last)
while (_name := _lib.lib().tssep_gemm_kernel_name(len(GEMM_KERNEL_NAMES))) != b"?":
    GEMM_KERNEL_NAMES[len(GEMM_KERNEL_NAMES)] = _name.decode()
GEMM_KERNELS = {name: kid for kid, name in GEMM_KERNEL_NAMES.items()}
GEMM_PREFER = ()
GEMM_LOG = None          # a list: (kernel name, M, N, K) of every launch is appended (tests)
RECURRENCE_LOG = None    # a list: dict(kernel, direction, N, T, H, groups) of every recurrence launch (Trainer: the kernel plan)
TAIL_LOG = None          # a list: dict(kernel, ...) of every fused two-mask tail launch (mask_map_fwd / _bwd; the kernel plan)


def _log_recurrence(kernel, direction, N, T, H, groups=0):
    if RECURRENCE_LOG is not None:
        RECURRENCE_LOG.append(dict(kernel=kernel, direction=direction, sequences=N, frames=T, units=H, groups=groups))


class prefer_gemm_kernels:
    """``with prefer_gemm_kernels("big"): ...`` -- see GEMM_PREFER."""

    def __init__(self, *names):
        self.names = tuple(n for n in names if n)

    def __enter__(self):
        global GEMM_PREFER
        self.old, GEMM_PREFER = GEMM_PREFER, self.names
        return self

    def __exit__(self, *exc):
        global GEMM_PREFER
        GEMM_PREFER = self.old
        return False


def gemm_plan(g, force="auto"):
    """-> name of the kernel tssep_gemm_f32_on(g, force) would launch, or None when `force` does not cover g."""
    kid = ctypes.c_int32(0)
    rc = _lib.lib().tssep_gemm_plan(ctypes.byref(g), GEMM_KERNELS[force], ctypes.byref(kid))
    return GEMM_KERNEL_NAMES[kid.value] if rc == 0 else None


def gemm_descriptor(g):
    """The request without its pointers (what the dispatcher's choice depends on): tools/sweep_gemm_shapes.py replays it."""
    d = {f: getattr(g, f) for f, _ in GemmArgs._fields_ if f not in ("A", "B", "C", "bias", "c_perm", "aux")}
    d.update(bias=bool(g.bias), perm=bool(g.c_perm), has_aux=bool(g.aux))
    return d


def _launch_gemm(g):
    kid = 0
    for name in GEMM_PREFER:
        if gemm_plan(g, name) is not None:
            kid = GEMM_KERNELS[name]
            break
    if GEMM_LOG is not None:
        GEMM_LOG.append((gemm_plan(g, GEMM_KERNEL_NAMES[kid]), g.M, g.N, g.K, gemm_descriptor(g)))
    L = _lib.lib()
    check(L.tssep_gemm_f32_on(ctypes.byref(g), kid, _stream()) if kid else L.tssep_gemm_f32(ctypes.byref(g), _stream()),
          "gemm_f32")


def gemm(A, lda, B, ldb, C, ldc, M, N, K, **kw):
    """C = epilogue(op(A) x op(B)); see include/tssep_hip.h.  A, B, C: tensors (or (tensor,
    float_offset) tuples) whose data pointers are used as given.  Keywords: a_kmajor, b_kmajor, bias, act,
    accumulate, b_kshift, kperiod, remap, splitk, split_stride, b_ones_col, aux."""
    g = _gemm_args(A, lda, B, ldb, C, ldc, M, N, K, **kw)
    with _timed("gemm_" + GEMM_PRECISION, 2 * M * N * K, 4 * (M * K + N * K + M * N * (2 if kw.get("accumulate") else 1))):
        _launch_gemm(g)


def transposed(w, rows, cols):
    """[rows, >= cols] weight view -> contiguous [cols, round_up(rows, 4)] copy (layout glue): the
    dgrad GEMMs then read BOTH operands k-contiguous with 16-byte loads (the k-major path reads
    4 bytes per lane: 242 vs ~300 TFLOP/s on the K = 2400 shapes)."""
    ld = round_up(rows, 4)
    if ld == rows:
        return w[:rows, :cols].t().contiguous(), ld
    out = torch.zeros(cols, ld, device=w.device, dtype=torch.float32)
    out[:, :rows] = w[:rows, :cols].t()
    return out, ld


def _wgrad_splits(g):
    """The split count the library recommends for the weight-gradient request `g` (it follows the kernel it picks)."""
    S = int(_lib.lib().tssep_gemm_wgrad_splits(ctypes.byref(g)))
    if S < 1:
        check(S, "gemm_wgrad_splits")
    return S


def pick_splitk(M, N, K, shifted=False, ones_col=False):
    """Split count the library recommends for the weight gradient dW[M,N] = dY[K,M]^T X[K,N] (host-only query on
    a description of the request: tools and tests; `wgrad` asks with the real arguments)."""
    g = GemmArgs()
    g.A = g.B = 0x1000
    g.M, g.N, g.K = M, N, K
    g.lda, g.ldb, g.ldc = round_up(M, 4), round_up(N, 4), round_up(N, 4)
    g.a_kmajor = g.b_kmajor = 1
    if shifted:
        g.b_kshift, g.kperiod = -1, 253
    g.b_ones_col = int(ones_col)
    g.precision = _PREC[GEMM_PRECISION]
    return _wgrad_splits(g)


# Opt-in arithmetic of the weight gradients (bench.py's `two_product_wgrad` side line): 2 = the dY_lo * X_hi product is
# dropped (tssep_gemm_args.precision = 2); an argument of the call, not an environment variable of the library.
WGRAD_PRODUCTS = 3


def wgrad(dY, ld_dy, X, ld_x, M, N, R, b_kshift=0, kperiod=0, with_colsum=False, splitk=None):
    """dW[M,N] = dY[R,M]^T X[R,N] by split-K partials -> (partials [S, M*N], S).
    with_colsum (split-bf16 GEMM only): partials are [S, M, round_up(N+1, 4)] and column N holds
    the column sums of dY (the bias gradient), from a virtual all-ones column of X.
    The split count is the library's (tssep_gemm_wgrad_splits: it follows the kernel the library picks)."""
    Nc = N + 1 if with_colsum else N
    ldp = round_up(Nc, 4) if with_colsum else N      # 16-byte rows keep the vector epilogue
    g = _gemm_args(dY, ld_dy, X, ld_x, X, ldp, M, Nc, R, a_kmajor=True, b_kmajor=True, b_kshift=b_kshift,
                   kperiod=kperiod, splitk=8, split_stride=M * ldp, b_ones_col=with_colsum)
    if (WGRAD_PRODUCTS == 2 and GEMM_PRECISION == "bf16x3") or GEMM_PRECISION == "bf16":
        g.precision = 2      # (the plain-bf16 side line: dY as plain bf16 in the weight gradients, X keeps hi + lo)
    S = splitk or _wgrad_splits(g)
    part = torch.empty(S, M * ldp, device=_device_of(dY), dtype=torch.float32)
    g.C, g.splitk = part.data_ptr(), S
    with _timed("gemm_" + GEMM_PRECISION, 2 * M * Nc * R, 4 * (M * R + N * R + S * M * ldp)):
        _launch_gemm(g)
    return part, S


def fused_colsum():
    """Whether weight-gradient GEMMs can also produce the bias gradient (b_ones_col)."""
    return GEMM_PRECISION in ("bf16x3", "bf16")


def reduce_splits(part, S, count, dst, accumulate=False):
    check(_lib.lib().tssep_reduce_splits(_p(part), S, count, count, _p(dst), int(accumulate),
                                         _stream()), "reduce_splits")


def reduce_splits_bias(part, S, M, N, ldp, dw, db, accumulate=False):
    """partials [S, M, ldp] of wgrad(..., with_colsum=True) -> dw [M, N] (dense) and db [M] (column N)."""
    check(_lib.lib().tssep_reduce_splits_bias(_p(part), S, M * ldp, M, N, ldp, _p(dw), N, _p(db), int(accumulate),
                                              _stream()), "reduce_splits_bias")


def colsum(A, lda, M, N, out=None, accumulate=False):
    L = _lib.lib()
    dev = _device_of(A)
    if out is None:
        out = torch.empty(N, device=dev, dtype=torch.float32)
    ws = torch.empty(int(L.tssep_colsum_workspace_bytes(M, N)) // 4, device=dev,
                     dtype=torch.float32)
    check(L.tssep_colsum_f32(_p(A), M, N, lda, _p(out), int(accumulate), _p(ws),
                             _stream()), "colsum")
    return out


# ---- derived weight layouts, cached across the micro-steps of a virtual minibatch ------------------
# Packed / transposed weight copies (lstm_pack, the W-stationary packs, dgrad transposes) are functions of
# the parameters only.  With virtual_minibatch_size = v (the reference's default is 12,
# tssep/train/experiment.py:135) the parameters change once per v forward/backward passes, so the copies
# are rebuilt once per optimizer step instead of once per pass.  Validity: a parameter changes either
# through torch (its ``_version`` counter moves: load_state_dict, copy_) or through the fused Adam kernel
# (raw pointer: ``weights_changed()`` is called by the optimizer).  Never used while a stream is being
# captured: a graph must contain the pack kernels, the weights differ at every replay.
# The ``.data`` rule: a write that reaches the storage past the parameter object -- ``p.data.copy_(...)``, any torch
# operation on ``optimizer.flat_param`` (whose views the parameters' ``.data`` are), a collective into it -- moves
# neither signal (``p._version`` counts writes through ``p`` itself only).  Whoever writes that way calls
# ``weights_changed()`` afterwards (train/trainer.py: adopt_rank0_state); a layout built before such a write would
# otherwise serve the forward after it.
WEIGHTS_VERSION = 0


def weights_changed():
    global WEIGHTS_VERSION
    WEIGHTS_VERSION += 1


_BUILDER_SEQ = itertools.count()      # order of first use: a build may read what an earlier one made
_PREPARED = None                      # while a step is being captured: (id(params[0]), tag) -> (event, value, stream, waiters)
PREPARED_HITS = 0                     # layouts handed out from there (tests)
PREPARE_DERIVED = True                # False: every layout is built where it is first used (A/B, tools)
_DERIVED_SEEN = None                  # while `record_derived` is open: (id(params[0]), tag) of every layout asked for


class record_derived:
    """``with record_derived() as seen:`` -- the layouts a step asks `derived` for (train/graph.py records them over the
    warm-up passes of ONE input signature and prepares exactly those in its graph: a builder another signature registered --
    the 32-sequence packs of a small validation batch, say -- is not rebuilt in every replay for nobody)."""

    def __enter__(self):
        global _DERIVED_SEEN
        self.old, _DERIVED_SEEN = _DERIVED_SEEN, set()
        return _DERIVED_SEEN

    def __exit__(self, *exc):
        global _DERIVED_SEEN
        _DERIVED_SEEN = self.old
        return False


def derived(tag, params, build):
    """build() -> any structure of tensors derived from `params`; memoised until a parameter changes.
    The memo lives ON the first parameter object (it dies with the module: a recycled device address of
    another model can never hit it) and is stamped with every parameter's address and version, the global
    update counter and the stream it was built on.  A `build` must reach everything it reads THROUGH the
    parameters (or through `derived` again): `prepare_derived` calls it at the start of a later step."""
    key = (id(params[0]), tag)
    if _DERIVED_SEEN is not None:
        _DERIVED_SEEN.add(key)
    if _PREPARED is not None:
        hit = _PREPARED.get(key)
        if hit is not None:
            global PREPARED_HITS
            PREPARED_HITS += 1
            ev, val, built_on, waited = hit
            cur = torch.cuda.current_stream().cuda_stream
            if cur != built_on and cur not in waited:      # (never a stream on its own event, never twice: one edge each)
                torch.cuda.current_stream().wait_event(ev)
                waited.add(cur)
            return val
    builders = params[0].__dict__.setdefault("_tssep_builders", {})      # on the parameter, like the memo below
    if tag not in builders:
        builders[tag] = (next(_BUILDER_SEQ), build)
    if torch.cuda.is_current_stream_capturing():
        return build()
    memo = params[0].__dict__.setdefault("_tssep_derived", {})
    stamp = (WEIGHTS_VERSION, torch.cuda.current_stream().cuda_stream,
             tuple((id(p), p.data_ptr(), p._version) for p in params))
    hit = memo.get(tag)
    if hit is not None and hit[0] == stamp:
        return hit[1]
    val = build()
    memo[tag] = (stamp, val)
    return val


class prepare_derived:
    """Context of ONE step that is being captured into a hipGraph (train/graph.py): the derived weight layouts the
    previous (warm-up) steps asked for -- gate / projection packs, the W-stationary packs, the dgrad transposes; functions
    of the parameters only -- are built at the START of the step on the side stream, as a branch of the graph beside the
    STFT / feature kernels, instead of one small kernel after the other in front of the recurrences they feed
    (8 utterances per GPU: ~25 launches of 4-20 us, 0.2 ms of a 7.8-ms step).  `derived` hands out the prepared value
    after making the consumer's stream wait for the event behind it.  Outside a capture the memo above does the job."""

    def __init__(self, parameters, device, only=None):
        """only: a set of (id(parameter), tag) -- what `record_derived` saw -- restricts the branch to those layouts."""
        self.builds = sorted((seq, id(p), tag, build) for p in parameters
                             for tag, (seq, build) in p.__dict__.get("_tssep_builders", {}).items()
                             if only is None or (id(p), tag) in only)
        self.device = device

    def __enter__(self):
        global _PREPARED
        assert _PREPARED is None
        main = torch.cuda.current_stream(self.device)
        side = side_stream(self.device)
        if side is main or not PREPARE_DERIVED or not torch.cuda.is_current_stream_capturing():
            return self
        prepared = {}
        side.wait_stream(main)
        _PREPARED = prepared            # builds that go through `derived` again find what is already there
        try:
            with torch.cuda.stream(side):
                for _, pid, tag, build in self.builds:
                    val = build()
                    ev = torch.cuda.Event()
                    ev.record(side)
                    prepared[(pid, tag)] = (ev, val, side.cuda_stream, set())
        except BaseException:
            _PREPARED = None
            raise
        return self

    def __exit__(self, *exc):
        global _PREPARED
        _PREPARED = None
        return False


# ------------------------------------------------------------------------------ BLSTM
def lstm_pack(params, H, I):
    """params: 8 tensors (w_ih, w_hh, b_ih, b_hh forward, then reverse), torch layout; or the 4 of one direction of time
    (typ = 'lstm') -> the [dir = 0] half of the same layouts, through the library's one-direction entry points."""
    L = _lib.lib()
    sizes, pack = ("lstm1_pack_sizes", "lstm1_pack") if len(params) // 4 == 1 else ("lstm_pack_sizes", "lstm_pack")
    ld_i = round_up(I, 4)
    sz = LstmSizes()
    check(getattr(L, "tssep_" + sizes)(H, I, ld_i, ctypes.byref(sz)), sizes)
    dev = params[0].device
    buf = torch.empty(sz.wih_p + round_up(sz.bias_p, 4) + sz.whh_f + sz.whh_b, device=dev,
                      dtype=torch.float32)
    o1 = sz.wih_p
    o2 = o1 + round_up(sz.bias_p, 4)
    o3 = o2 + sz.whh_f
    wih_p, bias_p, whh_f, whh_b = buf[:o1], buf[o1:o1 + sz.bias_p], buf[o2:o3], buf[o3:]
    ps = [_f32(p.detach()).contiguous() for p in params]
    check(getattr(L, "tssep_" + pack)(*[_p(p) for p in ps], H, I, ld_i, _p(wih_p), _p(bias_p), _p(whh_f),
                                      _p(whh_b), _stream()), pack)
    return dict(wih_p=wih_p, bias_p=bias_p, whh_f=whh_f, whh_b=whh_b, ld_i=ld_i, _keep=(buf, ps))


lstm1_pack = lstm_pack      # (a name of its own: the callers of one direction ask for it, and the tests watch each name)


def gru_pack(params, H, I):
    """params: the 4 tensors of one direction of time (w_ih [3H, I], w_hh [3H, H], b_ih, b_hh; torch.nn.GRU's layout, rows
    r, z, n) or the 8 of two (forward, then reverse) -> the four-slot layouts of gru.hip, in lstm_pack's dictionary: every
    unit has the slots (r, z, n, q), so every size is the LSTM's."""
    L = _lib.lib()
    nd = len(params) // 4
    ld_i = round_up(I, 4)
    sz = LstmSizes()
    check(L.tssep_gru_pack_sizes(nd, H, I, ld_i, ctypes.byref(sz)), "gru_pack_sizes")
    buf = torch.empty(sz.wih_p + round_up(sz.bias_p, 4) + sz.whh_f + sz.whh_b, device=params[0].device, dtype=torch.float32)
    o1 = sz.wih_p
    o2 = o1 + round_up(sz.bias_p, 4)
    o3 = o2 + sz.whh_f
    wih_p, bias_p, whh_f, whh_b = buf[:o1], buf[o1:o1 + sz.bias_p], buf[o2:o3], buf[o3:]
    ps = [_f32(p.detach()).contiguous() for p in params]
    ptrs = [_p(p) for p in ps] + [None] * (8 - len(ps))
    check(L.tssep_gru_pack(nd, *ptrs, H, I, ld_i, _p(wih_p), _p(bias_p), _p(whh_f), _p(whh_b), _stream()), "gru_pack")
    return dict(wih_p=wih_p, bias_p=bias_p, whh_f=whh_f, whh_b=whh_b, ld_i=ld_i, _keep=(buf, ps))


_ERR = {}


def _err_flag(device):
    device = torch.device(device)
    if device.index is None:      # "cuda" and "cuda:0" must name the SAME flag (a check on the wrong key sees nothing)
        device = torch.device("cuda", torch.cuda.current_device())
    key = str(device)
    if key not in _ERR:
        # [0] error flag, [1] launch epoch of the W-stationary kernels (library-maintained), [2..3] spare
        _ERR[key] = torch.zeros(4, device=device, dtype=torch.int32)
    return _ERR[key]


def cluster_error_code(device="cuda"):
    """Synchronising read-and-clear of the cluster kernels' timeout flag: 0 = no launch gave up."""
    f = _err_flag(device)
    v = int(f[0].item())
    if v:
        f[0].zero_()
    return v


def check_cluster_errors(device="cuda"):
    """Synchronising check of the cluster kernels' timeout flag (tests / end of a bench run)."""
    v = cluster_error_code(device)
    if v:
        raise RuntimeError(f"cluster recurrence kernel timed out waiting for a peer (code {v})")


@functools.lru_cache(maxsize=None)      # (asked once per layer and step, by both layer types)
def n_cus(device):
    return torch.cuda.get_device_properties(device).multi_processor_count


_WARNED = set()


def _warn_once(key, msg):
    if key not in _WARNED:
        _WARNED.add(key)
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


# recurrence policy (train/runtime.py: recurrence, onchip16, onchip16_groups, onchip16_min_n, onchip16_bwd,
# onchip16_bwd_groups), read by recurrence_plan alone
RECURRENCE = "auto"      # "auto" | "stream" (lstm.hip) | "cluster" (lstm_cluster.hip) | "onchip" (lstm_onchip.hip)
ONCHIP16 = True          # interleaved kernels: groups of 16 sequences in rotation
ONCHIP16_GROUPS = 0      # 1 | 2 | 4: forced group count where it divides the number of 16-sequence groups (A/B)
ONCHIP16_MIN_N = 1       # (a one-group step is 3.5 us against 5.2: the latency regime gains too)
ONCHIP16_BWD = True
ONCHIP16_BWD_GROUPS = 2  # at most: a backward phase is paced by its three barriers and the publish (7.1 against 7.8 ms
                         # per launch at 3 072 sequences with four -- profiles/r3_onchip16_backward.jsonl)

KEEP_XBUF = None         # a list: the exchange buffers of the interleaved launches are appended (trace builds, tools)


def recurrence_plan(N, T, H, cus, directions=2, cell="lstm"):
    """-> {"fwd": (kernel, groups), "bwd": (kernel, groups)}: the kernel of each direction of time of a BLSTM layer over
    N sequences of T frames with H units, on a device of `cus` compute units.  directions = 1 (typ = 'lstm'): the
    streaming kernels instantiated for one direction, with a state, ("stream1_f32", 0) both ways -- the only recurrence
    of one direction there is, so no policy switch is read and nothing is announced.  kernel: "stream_f32" (lstm.hip),
    "cluster_f32" (lstm_cluster.hip), "onchip32_bf16x3" or "onchip16_bf16x3" (lstm_onchip.hip); groups: 16-sequence groups
    in rotation per cluster of the interleaved kernels, 0 for the others.  ms per launch on MI355X at H=300, T=253
    (profiles/r2_recurrence_microbench.jsonl, forward / backward):
      on-chip bf16x3 (compact granules)  1.34 / 1.32 (8 sequences), 1.58 / 1.53 (32), 1.85 / 1.74 (256),
                                         2.26 / 2.14 (768 = one resident round of 48 XCD-local clusters x
                                         32 sequences x 1 direction), 4.3 / 4.1 (1536), 8.4 / 8.1 (3072)
      fp32 cluster                       1.50 / 1.34 (8), 1.50 / 1.57 (32), 7.8 / 21.5 (768)
      streaming fp32                     4.75 / 6.0 (<= 512), 5.3 / 6.2 (768), 17.0 / 18.7 (3072)
    Policy: the on-chip kernels for every N where they exist (H >= 128, T up to the 32-bit offset limit
    tssep_lstm_onchip_max_steps: 14 913 frames = 238 s at H = 300 for the 16-sequence kernels, 7 215 for the 32-sequence
    ones); the interleaved ones where tssep_blstm_onchip16_groups gives groups, backward for H = 257...320 only.  Round 1
    sent backward launches of <= 32 sequences to the fp32 cluster kernel, which the compact granules overtook.  The fp32
    W-stationary (cluster) and streaming kernels remain selectable (RECURRENCE) as the exact-fp32 recurrences, and
    streaming is the path for H the W-stationary kernels do not support -- a fallback for a SUPPORTED H (sequence too
    long) is announced, never silent.
    cell = "gru" (torch.nn.GRU containers): gru.hip's streaming kernels, ("stream_gru_f32", 0) for two directions and
    ("stream1_gru_f32", 0) for one, both ways -- the only GRU recurrences there are, so no policy switch is read."""
    if cell == "gru":
        return dict.fromkeys(("fwd", "bwd"), ("stream1_gru_f32" if directions == 1 else "stream_gru_f32", 0))
    assert cell == "lstm", cell
    if directions == 1:
        return dict.fromkeys(("fwd", "bwd"), ("stream1_f32", 0))
    return {direction: _plan_direction(N, T, H, cus, direction == "bwd") for direction in ("fwd", "bwd")}


def _onchip16_groups(N, H, cus, backward):
    """16-sequence groups per cluster of the interleaved kernel of one direction (0: the 32-sequence kernel serves it)"""
    g = int(_lib.lib().tssep_blstm_onchip16_groups(N, H, cus)) if ONCHIP16 else 0
    if g and ONCHIP16_GROUPS in (1, 2, 4) and ((N + 15) // 16) % ONCHIP16_GROUPS == 0:
        g = ONCHIP16_GROUPS
    elif N < ONCHIP16_MIN_N:
        g = 0
    if backward:
        g = min(g, ONCHIP16_BWD_GROUPS) if ONCHIP16_BWD and 256 < H <= 320 else 0
    return g


def _plan_direction(N, T, H, cus, backward):
    L = _lib.lib()
    g = _onchip16_groups(N, H, cus, backward)
    limit = int(L.tssep_lstm_onchip_max_steps(H, 16 if g else 32))
    h_ok = bool(L.tssep_lstm_onchip_supported(H))
    onchip_ok = h_ok and T <= limit
    if h_ok and not onchip_ok and RECURRENCE in ("auto", "onchip") and H >= 128:
        _warn_once(("onchip_T", H, backward), f"tssep_amd: {T} frames per sequence exceed the W-stationary "
                   f"recurrence's {limit} at H = {H}: the streaming fp32 kernel runs instead (about 3x slower)")
    want = RECURRENCE if RECURRENCE in ("stream", "cluster", "onchip") else "onchip" if H >= 128 else "stream"
    if want == "cluster" and L.tssep_lstm_cluster_supported(H):
        return "cluster_f32", 0
    if want == "onchip" and onchip_ok:
        return ("onchip16_bf16x3", g) if g else ("onchip32_bf16x3", 0)
    return "stream_f32", 0


def _w16(name, restype, argtypes):
    """Entry point of the four-wave variant of the interleaved forward: EXPERIMENT build only since ABI 4 (rejected in
    round 5: 1.4-1.8x slower at every size) -- `make -C tssep_amd/csrc exp`, TSSEP_HIP_LIB=.../libtssep_hip_exp.so."""
    L = _lib.lib()
    if not hasattr(L, name):
        raise RuntimeError(f"{name}: the four-wave workgroups exist in the experiment build only (make exp, TSSEP_HIP_LIB)")
    fn = getattr(L, name)
    fn.restype, fn.argtypes = restype, argtypes
    return fn


_VP, _I64, _I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int


def recurrence_packs(plan, w_hh_f, w_hh_r, H, lstm_pk=None, memo=False, waves=8):
    """-> {direction: the W_hh layout its planned kernel reads} for the directions of `plan` (recurrence_plan's, or a part
    of it).  The streaming kernels read lstm_pack's (`lstm_pk`; the GRU ones gru_pack's), the W-stationary ones a layout of their own, built once
    here where both directions read it: through `derived` on (w_hh_f, w_hh_r) with memo=True -- the tags prepare_derived
    builds at the start of a captured step --, anew otherwise.  waves = 4: the layout of the four-wave interleaved
    forward (experiment build, `_w16`)."""
    L = _lib.lib()

    def operands():
        return _f32(w_hh_f.detach()).contiguous(), _f32(w_hh_r.detach()).contiguous()

    def both(packer, floats):      # one launch packs the two directions
        nf, nb = int(floats(H, 0)), int(floats(H, 1))
        buf = torch.empty(nf + nb, device=w_hh_f.device, dtype=torch.float32)
        a, b = operands()
        check(packer(_p(a), _p(b), H, _p(buf[:nf]), _p(buf[nf:]), _stream()), packer.__name__[6:])
        return buf[:nf], buf[nf:]

    def one(packer, floats, *extra):
        buf = torch.empty(int(floats), device=w_hh_f.device, dtype=torch.float32)
        a, b = operands()
        check(packer(_p(a), _p(b), H, *extra, _p(buf), _stream()), packer.__name__[6:])
        return buf

    def layout(kernel, bwd):      # -> (derived tag, build, which of the built pair or None)
        if kernel == "cluster_f32":
            return "pack_cluster", lambda: both(L.tssep_lstm_pack_cluster, L.tssep_lstm_cluster_pack_floats), int(bwd)
        if kernel == "onchip32_bf16x3":
            return "pack_onchip", lambda: both(L.tssep_lstm_pack_onchip, L.tssep_lstm_onchip_pack_floats), int(bwd)
        if bwd:
            return "pack_onchip16_bwd", lambda: one(L.tssep_lstm_pack_onchip16_bwd, L.tssep_lstm_onchip16_bwd_pack_floats(H)), None
        if waves != 4:
            return "pack_onchip16", lambda: one(L.tssep_lstm_pack_onchip16, L.tssep_lstm_onchip16_pack_floats(H)), None
        return "pack_onchip16_w4", lambda: one(_w16("tssep_lstm_pack_onchip16w", _I, [_VP, _VP, _I, _I, _VP, _VP]),
                                               _w16("tssep_lstm_onchip16w_pack_floats", _I64, [_I, _I])(H, waves), waves), None

    built, out = {}, {}
    for direction, (kernel, _) in plan.items():
        if kernel in ("stream_f32", "stream1_f32", "stream_gru_f32", "stream1_gru_f32"):      # (lstm_pack's / gru_pack's)
            out[direction] = lstm_pk["whh_b" if direction == "bwd" else "whh_f"]
            continue
        tag, build, which = layout(kernel, direction == "bwd")
        if tag not in built:
            built[tag] = derived(tag, [w_hh_f, w_hh_r], build) if memo else build()
        out[direction] = built[tag] if which is None else built[tag][which]
    return out


# kernel -> (C entry points forward / backward, _timed name, algorithmic HBM bytes per cell forward / backward: gates in /
# activations out 16 + 16, c 4, h 4; activations 16, c 4 + 4, dh 4 in, d(gates) 16 out)
_RECURRENCE_KERNELS = {
    "stream_f32": (("tssep_blstm_fwd", "tssep_blstm_bwd"), "blstm", (0, 0)),
    "stream1_f32": (("tssep_lstm1_fwd", "tssep_lstm1_bwd"), "lstm1", (0, 0)),
    "stream_gru_f32": (("tssep_gru_fwd", "tssep_gru_bwd"), "gru", (0, 0)),
    "stream1_gru_f32": (("tssep_gru1_fwd", "tssep_gru1_bwd"), "gru1", (0, 0)),
    "cluster_f32": (("tssep_blstm_cluster_fwd", "tssep_blstm_cluster_bwd"), "blstm_cluster", (0, 0)),
    "onchip32_bf16x3": (("tssep_blstm_onchip_fwd", "tssep_blstm_onchip_bwd"), "blstm_onchip", (40, 44)),
    "onchip16_bf16x3": (("tssep_blstm_onchip16_fwd", "tssep_blstm_onchip16_bwd"), "blstm_onchip", (40, 44)),
}


def recurrence_launch(planned, direction, gates, cell, h, ldo, dstride, whh, N, T, H, ms=2, layout=0, waves=8,
                      state=(None,) * 4):
    """One direction of time ("fwd" | "bwd") of a BLSTM layer on planned = (kernel, groups), recurrence_plan's: h is hout
    (written forward) or dhout (read backward; d(gates) replace the gates in place), whh the layout recurrence_packs gave
    for the same kernel and direction.  ms (cluster), layout (on-chip kernels) and waves = 4 (the interleaved forward's
    four-wave workgroups, experiment build: `_w16`) go to the kernel as they are.
    "stream1_f32" (one direction: gates [N,T,H,4], cell [N,T,H], h columns 0..H-1 of [N,T,ldo]; no dstride) takes
    state = (h0, c0, hT, cT) forward: h0 / c0 [N,H] the initial state (both or neither; None = zeros), hT / cT [N,H]
    receive the state after the last frame.  Backward it starts from a zero state, or takes state = (c0, dhT, dcT, dh0,
    dc0), each [N,H] or None: the state the forward started from, the gradient arriving for (hT, cT), and where the
    gradient of (h0, c0) goes (tssep_lstm1_bwd_state; all None is the launch without a state, logged under one name).
    The GRU kernels ("stream_gru_f32", "stream1_gru_f32"; gates hold the slots (r, z, n, q)) have no cell tensor: forward
    `cell` is ignored (None), backward it is the forward's hout, which they read for h_prev; state = (h0, None, hT, None)
    forward, (h0, dhT, dh0) backward on "stream1_gru_f32" (tssep_gru1_bwd_state)."""
    kernel, groups = planned
    if kernel in ("stream_gru_f32", "stream1_gru_f32"):
        return _gru_launch(kernel, direction, gates, cell, h, ldo, dstride, whh, N, T, H, state)
    bwd = direction == "bwd"
    entry, timed, cell_bytes = _RECURRENCE_KERNELS[kernel]
    entry = entry[bwd]
    w4 = kernel == "onchip16_bf16x3" and not bwd and waves == 4
    _log_recurrence(kernel + ("_w4" if w4 else ""), direction, N, T, H, groups)
    L = _lib.lib()
    D = 1 if kernel == "stream1_f32" else 2
    flops, nbytes = 2 * D * N * T * 4 * H * H, N * T * D * H * cell_bytes[bwd]
    if D == 1:
        for s in state:
            assert s is None or (s.is_contiguous() and tuple(s.shape) == (N, H) and _f32(s) is s), (N, H)
        with_state = bwd and any(s is not None for s in state)
        if with_state:
            assert len(state) == 5, "backward: state = (c0, dhT, dcT, dh0, dc0)"
            entry += "_state"
        args = (_p(gates), _p(cell), _p(h), ldo, _p(whh), *(map(_p, state) if with_state or not bwd else ()))
    else:
        assert not bwd or all(s is None for s in state), "a state needs one direction of time"
        args = (_p(gates), _p(cell), _p(h), ldo, dstride, _p(whh))
    if kernel in ("stream_f32", "stream1_f32"):
        with _timed(f"{timed}_{direction}", flops, nbytes):
            check(getattr(L, entry)(*args, N, T, H, _stream()), entry[6:])
        return
    fence_comm(gates.device)
    cus = n_cus(gates.device)
    fn = getattr(L, entry)
    if kernel == "cluster_f32":
        words, tail = int(L.tssep_lstm_cluster_xbuf_bytes(N, H, int(bwd), cus, ms)) // 8 + 1, (ms,)
    elif kernel == "onchip32_bf16x3":
        words, tail = int(L.tssep_lstm_onchip_xbuf_bytes(N, H, int(bwd))) // 8 + 2, (layout,)
    elif bwd:
        words, tail = int(L.tssep_lstm_onchip16_bwd_xbuf_bytes(N, H)) // 8 + 2, (layout, groups)
    elif not w4:
        words, tail = int(L.tssep_lstm_onchip16_xbuf_bytes(N, H)) // 8 + 2, (layout, groups)
    else:
        words = int(_w16("tssep_lstm_onchip16w_xbuf_bytes", _I64, [_I64, _I, _I])(N, H, waves)) // 8 + 2
        tail = (layout, groups, waves)
        fn = _w16("tssep_blstm_onchip16w_fwd", _I, [_VP, _VP, _VP, _I64, _I64, _VP, _VP, _VP, _I64, _I64, _I, _I, _I, _I, _I, _VP])
    xbuf = torch.empty(words, device=gates.device, dtype=torch.int64)
    if KEEP_XBUF is not None and kernel == "onchip16_bf16x3":
        KEEP_XBUF.append(xbuf)
    with _timed(f"{timed}_{direction}", flops, nbytes):
        check(fn(*args, _p(xbuf), _p(_err_flag(gates.device)), N, T, H, cus, *tail, _stream()), entry[6:])


def _gru_launch(kernel, direction, gates, hout, h, ldo, dstride, whh, N, T, H, state):
    bwd = direction == "bwd"
    entry, timed, _ = _RECURRENCE_KERNELS[kernel]
    entry = entry[bwd]
    _log_recurrence(kernel, direction, N, T, H, 0)
    one = kernel == "stream1_gru_f32"
    D = 1 if one else 2
    if bwd and any(s is not None for s in state):
        assert one, "a state needs one direction of time"
        bstate = tuple(state)
        assert len(bstate) == 3, "backward: state = (h0, dhT, dh0)"
        h0 = hT = None
    else:
        bstate = ()
        h0, c0, hT, cT = state if not bwd else (None,) * 4
        assert c0 is None and cT is None, "a GRU carries h alone"
        assert one or (h0 is None and hT is None), "a state needs one direction of time"
    for s in (h0, hT) + bstate:
        assert s is None or (s.is_contiguous() and tuple(s.shape) == (N, H) and _f32(s) is s), (N, H)
    args = [_p(gates)] + ([_p(hout)] if bwd else []) + [_p(h), ldo] + ([] if one else [dstride]) + [_p(whh)]
    if one and not bwd:
        args += [_p(h0), _p(hT)]
    if bstate:
        entry += "_state"
        args += [_p(s) for s in bstate]
    with _timed(f"{timed}_{direction}", 2 * D * N * T * 4 * H * H, 0):
        check(getattr(_lib.lib(), entry)(*args, N, T, H, _stream()), entry[6:])


# Each recurrence kernel by name (the kernel tests and tools): the plan, the packs and the launcher above on one fixed
# kernel and direction.  device: whose CU count decides the groups -- the current device's when None, no interleaved
# kernels without a GPU.
def _cus(device):
    if device is None:
        if not torch.cuda.is_available():
            return 0
        device = torch.device("cuda", torch.cuda.current_device())
    return n_cus(device)


def recurrence_kernel(N, H, backward, T=0, device=None):
    """-> "stream" | "cluster" | "onchip": the family of the kernel recurrence_plan gives that direction"""
    return _plan_direction(N, T, H, _cus(device), backward)[0].split("_")[0].rstrip("0123456789")


def onchip16_groups(N, H, device):
    return _onchip16_groups(N, H, n_cus(device), False)


def onchip16_bwd_groups(N, H, device):
    return _onchip16_groups(N, H, n_cus(device), True)


def lstm_pack_cluster(w_hh_f, w_hh_r, H):
    return tuple(recurrence_packs(dict.fromkeys(("fwd", "bwd"), ("cluster_f32", 0)), w_hh_f, w_hh_r, H).values())


def lstm_pack_onchip(w_hh_f, w_hh_r, H):
    return tuple(recurrence_packs(dict.fromkeys(("fwd", "bwd"), ("onchip32_bf16x3", 0)), w_hh_f, w_hh_r, H).values())


def lstm_pack_onchip16(w_hh_f, w_hh_r, H, waves=8):
    return recurrence_packs({"fwd": ("onchip16_bf16x3", 0)}, w_hh_f, w_hh_r, H, waves=waves)["fwd"]


def lstm_pack_onchip16_bwd(w_hh_f, w_hh_r, H):
    return recurrence_packs({"bwd": ("onchip16_bf16x3", 0)}, w_hh_f, w_hh_r, H)["bwd"]


def blstm_fwd(gates, cell, hout, ldo, dstride, whh_f, N, T, H):
    recurrence_launch(("stream_f32", 0), "fwd", gates, cell, hout, ldo, dstride, whh_f, N, T, H)


def blstm_bwd(gates, cell, dhout, ldo, dstride, whh_b, N, T, H):
    recurrence_launch(("stream_f32", 0), "bwd", gates, cell, dhout, ldo, dstride, whh_b, N, T, H)


def lstm1_fwd(gates, cell, hout, ldo, whh_f, N, T, H, h0=None, c0=None, hT=None, cT=None):
    recurrence_launch(("stream1_f32", 0), "fwd", gates, cell, hout, ldo, 0, whh_f, N, T, H, state=(h0, c0, hT, cT))


def lstm1_bwd(gates, cell, dhout, ldo, whh_b, N, T, H, c0=None, dhT=None, dcT=None, dh0=None, dc0=None):
    """c0 / dhT / dcT / dh0 / dc0 [N,H]: the carried state's side of the backward (recurrence_launch); all None: none"""
    recurrence_launch(("stream1_f32", 0), "bwd", gates, cell, dhout, ldo, 0, whh_b, N, T, H,
                      state=(c0, dhT, dcT, dh0, dc0))


def blstm_cluster_fwd(gates, cell, hout, ldo, dstride, whh_cf, N, T, H, ms=2):
    recurrence_launch(("cluster_f32", 0), "fwd", gates, cell, hout, ldo, dstride, whh_cf, N, T, H, ms=ms)


def blstm_cluster_bwd(gates, cell, dhout, ldo, dstride, whh_cb, N, T, H, ms=2):
    recurrence_launch(("cluster_f32", 0), "bwd", gates, cell, dhout, ldo, dstride, whh_cb, N, T, H, ms=ms)


def blstm_onchip_fwd(gates, cell, hout, ldo, dstride, wf, N, T, H, layout=0):
    recurrence_launch(("onchip32_bf16x3", 0), "fwd", gates, cell, hout, ldo, dstride, wf, N, T, H, layout=layout)


def blstm_onchip_bwd(gates, cell, dhout, ldo, dstride, wb, N, T, H, layout=0):
    recurrence_launch(("onchip32_bf16x3", 0), "bwd", gates, cell, dhout, ldo, dstride, wb, N, T, H, layout=layout)


def blstm_onchip16_fwd(gates, cell, hout, ldo, dstride, wf16, N, T, H, groups, layout=0, waves=8):
    """wf16: the pack made for the SAME `waves` (lstm_pack_onchip16); waves = 4: experiment build only (`_w16`)."""
    recurrence_launch(("onchip16_bf16x3", groups), "fwd", gates, cell, hout, ldo, dstride, wf16, N, T, H, layout=layout,
                      waves=waves)


def blstm_onchip16_bwd(gates, cell, dhout, ldo, dstride, wb16, N, T, H, groups, layout=0):
    recurrence_launch(("onchip16_bf16x3", groups), "bwd", gates, cell, dhout, ldo, dstride, wb16, N, T, H, layout=layout)


def lstm_unpack(src, ld, nsplit, split_stride, H, ncols, dst_f, dst_r, accumulate=False):
    check(_lib.lib().tssep_lstm_unpack(_p(src), ld, nsplit, split_stride, H, ncols, _p(dst_f),
                                       _p(dst_r), int(accumulate), _stream()), "lstm_unpack")


def lstm1_unpack(src, ld, nsplit, split_stride, H, ncols, dst, accumulate=False):
    check(_lib.lib().tssep_lstm1_unpack(_p(src), ld, nsplit, split_stride, H, ncols, _p(dst), int(accumulate),
                                        _stream()), "lstm1_unpack")


def gru_fwd(gates, hout, ldo, dstride, whh_f, N, T, H, directions=2, h0=None, hT=None):
    """directions = 1: gates [N,T,H,4], hout columns 0..H-1, dstride unused; h0 / hT [N,H] the carried state"""
    recurrence_launch(("stream1_gru_f32" if directions == 1 else "stream_gru_f32", 0), "fwd", gates, None, hout, ldo,
                      dstride, whh_f, N, T, H, state=(h0, None, hT, None))


def gru_bwd(gates, hout, dhout, ldo, dstride, whh_b, N, T, H, directions=2, h0=None, dhT=None, dh0=None):
    """h0 / dhT / dh0 [N,H], directions = 1: the carried state's side of the backward; all None: none"""
    recurrence_launch(("stream1_gru_f32" if directions == 1 else "stream_gru_f32", 0), "bwd", gates, hout, dhout, ldo,
                      dstride, whh_b, N, T, H, state=(h0, dhT, dh0))


def gru1_bwd(gates, hout, dhout, ldo, whh_b, N, T, H, h0=None, dhT=None, dh0=None):
    gru_bwd(gates, hout, dhout, ldo, 0, whh_b, N, T, H, directions=1, h0=h0, dhT=dhT, dh0=dh0)


GRU_IH, GRU_HH = 0, 1      # TSSEP_GRU_IH / TSSEP_GRU_HH: the slots (0, 1, 2) / (0, 1, 3) of a packed row quadruple


def gru_unpack(src, ld, nsplit, split_stride, H, ncols, which, dst_f, dst_r=None, accumulate=False):
    """packed (dir, unit, slot) rows -> torch's [3H, ncols] rows (r, z, n) of one (dst_r None) or two directions"""
    check(_lib.lib().tssep_gru_unpack(1 if dst_r is None else 2, _p(src), ld, nsplit, split_stride, H, ncols, which,
                                      _p(dst_f), _p(dst_r), int(accumulate), _stream()), "gru_unpack")


# ---- side stream for weight gradients ---------------------------------------------------------
# Weight-gradient GEMMs are off the critical path of backward (nothing downstream reads them):
# with a GradBucket attached they are accumulated straight into the flat gradient buffer on a
# second HIP stream, overlapping the T-sequential recurrences of the layers still to come.
_SIDE = {}
OVERLAP_WGRAD = True
FOLD_TANH = True         # Tanh backward inside the consumer's d(input) GEMM store
FOLD_TAIL = 1            # LogMAE / MAE backward and the logit un-map inside the fused tail's backward (0: off; 2: the loss only, 3: the un-map only -- experiments)
SIDE_STREAM = True
SIDE_STREAM_MAX_SEQS = 512   # layers with more sequences (x 253 frames) stay on the compute stream: beyond this the GEMMs of the two streams only slow each other
ACTIVE_SINK = 0          # which gradient bucket the running micro-batch accumulates into
GRAPH_STEP = "auto"      # Trainer: hipGraph replay of forward + loss + backward ("auto": batches of <= GRAPH_MAX_UTTERANCES utterances)
GRAPH_MAX_UTTERANCES = 32


BUCKETED_ALLREDUCE = False     # per-layer gradient segments reduced during the backward (distributed.GradBucket; default off)
COMM_PENDING = {}              # str(device) -> the communication stream with gradient reductions in flight


def fence_comm(device):
    """In front of every W-stationary recurrence launch: an RCCL kernel must not run beside it (include/tssep_hip.h:
    the clusters need all their workgroups resident) -- the compute stream waits for the reductions queued so far."""
    st = COMM_PENDING.pop(str(torch.device(device) if not isinstance(device, torch.device) else device), None)
    if st is not None:
        torch.cuda.current_stream(device).wait_stream(st)


def side_stream(device, rows=0):
    """The weight-gradient stream paired with the CURRENT stream (one per compute stream).  Measured
    (batch sweep, MI355X): +7 % at batch 64, +2 % at 192, 0 at 384 -- where the uncontended GEMMs
    run at 213 instead of 124 TFLOP/s --, -0.6 % for the 768-sequence layers of batch 768, so layers
    with more than 512 sequences stay on the compute stream."""
    cur = torch.cuda.current_stream(device)
    if not SIDE_STREAM or rows > SIDE_STREAM_MAX_SEQS * 253:
        return cur
    key = (str(device), cur.cuda_stream)
    if key not in _SIDE:
        _SIDE[key] = torch.cuda.Stream(device=device)
    return _SIDE[key]


def forget_side_stream(stream):
    """Drop the side stream paired with `stream`.  torch hands streams out of a pool, so a NEW stream can carry the handle
    of one that was paired earlier; until it forks itself it must not join that old side stream (a captured step's waits
    would depend on how many streams the process has made)."""
    _SIDE.pop((str(stream.device), stream.cuda_stream), None)


def join_side_stream(device=None):
    """Make the current stream wait for the gradient work queued on ITS side stream (the pairing is per
    compute stream, so a stream that is being captured into a hipGraph only ever joins the stream it
    forked itself)."""
    cur = torch.cuda.current_stream(device)
    st = _SIDE.get((str(cur.device), cur.cuda_stream))
    if st is not None:
        cur.wait_stream(st)


# ------------------------------------------------------------------------ elementwise
def tanh_bwd(dy, y, rows, P, K, T, combined):
    dz = torch.empty(rows, P, device=dy.device, dtype=torch.float32)
    check(_lib.lib().tssep_tanh_bwd(_p(dy), _p(y), _p(dz), rows, P, K, T, int(combined),
                                    _stream()), "tanh_bwd")
    return dz


# ---- dropout in front of a Tanh (csrc/dropout.hip, csrc/dropout_philox.h) ----------------------------------------
# The mask is a pure function of {seed, draw, logical element index, p}.  {seed, draw} lives in DEVICE memory, one
# int64[2] per device: every active site's forward copies it into a tensor of its own (`used`, kept for the backward) and
# counts the draw up, on the device -- so nothing about a mask is frozen into a captured graph.  The tensor is created
# once and only ever written in place (captured graphs hold its address).
_DROPOUT_STATE = {}


def _as_i64(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >= (1 << 63) else v


def _cuda_device(device=None):
    dev = torch.device("cuda" if device is None else device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def dropout_state(device=None):
    """The device's {seed, draw} tensor; seeded from torch.initial_seed() when first asked for."""
    dev = _cuda_device(device)
    st = _DROPOUT_STATE.get(dev.index)
    if st is None:
        st = _DROPOUT_STATE[dev.index] = torch.tensor([_as_i64(torch.initial_seed()), 0], dtype=torch.int64, device=dev)
    return st


def manual_seed(seed, device=None):
    """Seed the dropout masks of `device` (default: the current one) and start counting draws from 0 again."""
    set_state((seed, 0), device)


def get_state(device=None):
    """-> (seed, draw) of the device's dropout stream as Python ints (one host sync)."""
    seed, draw = dropout_state(device).tolist()
    return seed, draw


def set_state(state, device=None):
    seed, draw = state
    st = dropout_state(device)
    st.copy_(torch.tensor([_as_i64(seed), _as_i64(draw)], dtype=torch.int64))


def dropout_draw(device=None):
    """One draw for one site: -> `used`, the {seed, draw} its forward and backward kernels read."""
    st = dropout_state(device)
    used = torch.empty(2, dtype=torch.int64, device=st.device)
    check(_lib.lib().tssep_dropout_draw(_p(st), _p(used), _stream()), "dropout_draw")
    return used


def dropout_tanh_fwd(z, y, rows, P, ld, K, T, combined, p, used):
    """y = keep ? tanh(z / (1 - p)) : 0; y may be z.  combined: both are the speaker-combined [B,T,K*P] (ld unused)."""
    assert used.dtype == torch.int64 and used.is_cuda and used.numel() == 2, (used.dtype, used.shape)
    check(_lib.lib().tssep_dropout_tanh_fwd(_p(_f32(z)), _p(_f32(y)), rows, P, ld, K, T, int(bool(combined)), float(p),
                                            _p(used), _stream()), "dropout_tanh_fwd")
    return y


def dropout_tanh_bwd(dy, y, rows, P, K, T, combined, p, used):
    """tanh_bwd with the mask of `used`: -> dz dense rows (b,k,t) x P."""
    assert used.dtype == torch.int64 and used.is_cuda and used.numel() == 2, (used.dtype, used.shape)
    dz = torch.empty(rows, P, device=dy.device, dtype=torch.float32)
    check(_lib.lib().tssep_dropout_tanh_bwd(_p(_f32(dy)), _p(_f32(y)), _p(dz), rows, P, K, T, int(bool(combined)),
                                            float(p), _p(used), _stream()), "dropout_tanh_bwd")
    return dz


def philox4x32_10_host(ctr, key):
    """Philox4x32-10 on the host (no GPU): 4 counter words, 2 key words -> 4 output words."""
    c, k, o = (ctypes.c_uint32 * 4)(*ctr), (ctypes.c_uint32 * 2)(*key), (ctypes.c_uint32 * 4)()
    check(_lib.lib().tssep_philox4x32_10_host(c, k, o), "philox4x32_10_host")
    return [int(v) for v in o]


def dropout_keep_host(seed, draw, first, n, p):
    """The mask {seed, draw} for the logical elements first .. first + n - 1, on the host (no GPU): uint8 [n], 1 = keep."""
    keep = np.empty(max(int(n), 0), dtype=np.uint8)
    buf = keep.ctypes.data_as(ctypes.c_void_p) if keep.size else (ctypes.c_uint8 * 1)()
    check(_lib.lib().tssep_dropout_keep_host(_as_i64(seed), _as_i64(draw), int(first), int(n), float(p), buf),
          "dropout_keep_host")
    return keep


def cond_frames(T, Ta, stride):
    """Frame-wise embeddings: frame t reads embedding row t // stride, so there are ceil(T / stride) rows.  Ta = 0 is the
    utterance-level embedding (one row per speaker).  Raises ValueError before anything is launched."""
    if not Ta:
        return
    if not isinstance(stride, int) or isinstance(stride, bool) or stride < 1:
        raise ValueError(f"aux_stride={stride!r}: a positive number of frames per embedding row")
    if Ta != -(-T // stride):
        raise ValueError(f"frame-wise embeddings: {Ta} rows for {T} frames at aux_stride={stride} "
                         f"(ceil(T / aux_stride) = {-(-T // stride)} rows are needed)")


def _cond_level(Ta, stride):
    """The one place that tells the two embedding levels apart: -> (t, level).  t is the infix of entry points and labels,
    "" for utterance-level embeddings (Ta = 0) and "_t" for frame-wise ones; level holds the trailing arguments the "_t"
    entry points take, (Ta, stride), or nothing."""
    return ("_t", (Ta, stride)) if Ta else ("", ())


def _entry(name):
    """-> (the bound tssep_<name>, its check label)"""
    return getattr(_lib.lib(), "tssep_" + name), name


def cond_fwd(pre, ld_pre, aux, B, K, T, F, trials, combination, Ta=0, stride=1, auxinfo=None):
    """-> (xs view [B*trials*K*T, W], ld, (aux rows, ld_aux)).  aux [B, K, E], or frame-wise [B, K, Ta, E] with
    Ta = ceil(T / stride) > 0.  The kernels take aux as 16-byte addressable rows: an aux whose E is no multiple of 4 is
    copied into padded rows first (rows_view: one pass over aux per call, layout glue); auxinfo = rows_view(aux) made by the
    caller skips that."""
    cond_frames(T, Ta, stride)
    t, level = _cond_level(Ta, stride)
    aux2, ld_aux = auxinfo if auxinfo is not None else rows_view(aux)
    E = aux.shape[-1]
    W = F if combination == "mul" else F + E
    # (the 16-byte path of cond_mul_fwd_kernel writes the pad columns itself: products of the inputs' zero pads)
    writes_pads = combination == "mul" and F <= 1024 and ld_pre % 4 == 0 and ld_pre >= round_up(F, 4) \
        and pre.data_ptr() % 16 == 0 and aux2.data_ptr() % 16 == 0
    xs, ld = padded(B * trials * K * T, W, pre.device, zero=not writes_pads)
    if combination == "mul":
        assert E == F, (E, F)
        fn, label = _entry(f"cond_mul{t}_fwd")
        check(fn(_p(pre), ld_pre, _p(aux2), ld_aux, _p(xs), ld, B, K, T, F, trials, *level, _stream()), label)
    else:
        fn, label = _entry(f"cond_cat{t}_fwd")
        check(fn(_p(pre), ld_pre, _p(aux2), ld_aux, _p(xs), ld, B, K, T, F, E, trials, *level, _stream()), label)
    return xs, ld, (aux2, ld_aux)


def cond_bwd(dxs, ld_dxs, auxinfo, B, K, T, F, trials, combination, Ta=0, stride=1):
    L = _lib.lib()
    aux2, ld_aux = auxinfo
    # (cond_mul_bwd_v4_kernel sums the pad columns too: zero in both inputs)
    writes_pads = combination == "mul" and ld_dxs % 4 == 0 and ld_dxs >= round_up(F, 4) and dxs.data_ptr() % 16 == 0 \
        and aux2.data_ptr() % 16 == 0
    dpre, ld = padded(B * T, F, dxs.device, zero=not writes_pads)
    if combination == "mul":
        t, level = _cond_level(Ta, stride)
        fn, label = _entry(f"cond_mul{t}_bwd")
        check(fn(_p(dxs), ld_dxs, _p(aux2), ld_aux, _p(dpre), ld, B, K, T, F, trials, *level, _stream()), label)
    else:                                   # (d(pre) of cat does not read the embedding: one entry point for both)
        check(L.tssep_cond_cat_bwd(_p(dxs), ld_dxs, _p(dpre), ld, B, K, T, F, trials, _stream()),
              "cond_cat_bwd")
    return dpre, ld


# ---- learned speaker embeddings (csrc/aux.hip) --------------------------------------------------------------------
def cond_aux_bwd(dxs, ld_dxs, pre, ld_pre, B, K, T, F, E, trials, combination, Ta=0, stride=1):
    """d(conditioning) / d(embedding) -> d_aux [B, K, C] (C = F for mul, E for cat), or [B, K, Ta, C] for frame-wise
    embeddings (Ta > 0).  A launch of its own, made only when the embedding requires a gradient (pre: the pre-net rows
    the forward multiplied with; None for cat)."""
    t, level = _cond_level(Ta, stride)
    mul = combination == "mul"
    C = F if mul else E
    fn, label = _entry(f"cond_aux{t}_bwd_workspace_bytes")
    nbytes = int(fn(B, K, T, F, 0 if mul else E, *level))
    # frame-wise: -1 refuses the shapes and 0 asks for no workspace; the utterance level always needs one
    if nbytes < 0 or (nbytes == 0 and not Ta):
        check(-1, label)
    ws = torch.empty(nbytes // 4, device=dxs.device, dtype=torch.float32) if nbytes else None
    d_aux = torch.empty(B, K, *level[:1], C, device=dxs.device, dtype=torch.float32)
    with _timed(f"cond_aux{t}_bwd", 0, 4 * (B * trials * K * T * C + (B * T * F if mul else 0) + d_aux.numel())):
        if mul:
            fn, label = _entry(f"cond_mul_aux{t}_bwd")
            check(fn(_p(_f32(dxs)), ld_dxs, _p(_f32(pre)), ld_pre, _p(d_aux), C, _p(ws), B, K, T, F, trials, *level,
                     _stream()), label)
        else:
            fn, label = _entry(f"cond_cat_aux{t}_bwd")
            check(fn(_p(_f32(dxs)), ld_dxs, _p(d_aux), C, _p(ws), B, K, T, F, E, trials, *level, _stream()), label)
    return d_aux


INSTNORM_AXES = {-1: 0, -2: 1}      # statistics along the last axis (one per row) / along the time axis (one per column)


def instnorm_fwd(x, axis, mode, unbiased=False):
    """x [..., n, C] -> (y like x, mean, rscale, (xv, ld)): InstanceNorm (mode 0) / InstanceNorm_v2 (mode 1)."""
    n, C = (x.shape[-2], x.shape[-1]) if x.dim() >= 2 else (1, x.shape[-1])
    R = x.numel() // (n * C)
    xv, ld = rows_view(x)
    y = torch.empty(R * n, C, device=x.device, dtype=torch.float32)
    stats = torch.empty(2, R * n if axis == 0 else R * C, device=x.device, dtype=torch.float32)
    check(_lib.lib().tssep_instnorm_fwd(_p(xv), ld, _p(y), C, _p(stats[0]), _p(stats[1]), R, n, C, axis, mode,
                                        int(bool(unbiased)), _stream()), "instnorm_fwd")
    return y.view(x.shape), stats[0], stats[1], (xv, ld)


def instnorm_bwd(dy, xinfo, mean, rscale, shape, axis, mode, unbiased=False):
    xv, ld = xinfo
    n, C = (shape[-2], shape[-1]) if len(shape) >= 2 else (1, shape[-1])
    R = int(np.prod(shape)) // (n * C)
    dv, ld_d = rows_view(dy)
    dx = torch.empty(R * n, C, device=dy.device, dtype=torch.float32)
    check(_lib.lib().tssep_instnorm_bwd(_p(dv), ld_d, _p(xv), ld, _p(mean), _p(rscale), _p(dx), C, R, n, C, axis, mode,
                                        int(bool(unbiased)), _stream()), "instnorm_bwd")
    return dx.view(shape)


def relu_fwd(y, ld, rows, C):
    """y = max(y, 0) in place on the rows of a [rows, ld] buffer."""
    check(_lib.lib().tssep_relu_fwd(_p(_f32(y)), ld, rows, C, _stream()), "relu_fwd")
    return y


def relu_bwd(dy, ld_dy, y, ld_y, rows, C):
    """-> (dx, ld): dx = y > 0 ? dy : 0 in a padded buffer."""
    dx, ld = padded(rows, C, dy.device, zero=True)
    check(_lib.lib().tssep_relu_bwd(_p(_f32(dy)), ld_dy, _p(_f32(y)), ld_y, _p(dx), ld, rows, C, _stream()), "relu_bwd")
    return dx, ld


def segment_rows(lengths, device):
    """Prefix of the packed rows -> int64 [S+1] on the device: built on the host once, one copy."""
    lengths = [int(n) for n in lengths]
    assert lengths and min(lengths) > 0, lengths
    return torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)).to(device)


def segment_mean_fwd(h, ld_h, row0, S, C, relu=False):
    """-> (out, ld): out[s] = mean over the rows row0[s] .. row0[s+1] - 1 of h (relu: of max(h, 0))."""
    assert row0.dtype == torch.int64 and row0.is_cuda and row0.numel() == S + 1, (row0.dtype, row0.shape)
    out, ld = padded(S, C, h.device, zero=True)
    check(_lib.lib().tssep_segment_mean_fwd(_p(_f32(h)), ld_h, _p(row0), _p(out), ld, S, C, int(bool(relu)), _stream()),
          "segment_mean_fwd")
    return out, ld


def segment_mean_bwd(dout, ld_dout, h, ld_h, row0, S, N, C, relu=False):
    """-> (dh, ld) over the N packed rows: dout[s] / len_s broadcast (relu: masked with h > 0)."""
    assert row0.dtype == torch.int64 and row0.is_cuda and row0.numel() == S + 1, (row0.dtype, row0.shape)
    dh, ld = padded(N, C, dout.device, zero=True)
    check(_lib.lib().tssep_segment_mean_bwd(_p(_f32(dout)), ld_dout, _p(h) if h is not None else None, ld_h, _p(row0),
                                            _p(dh), ld, S, C, int(bool(relu)), _stream()), "segment_mean_bwd")
    return dh, ld


# -------------------------------------------------------------------------- mask head
def maskhead_fwd(logit, obs):
    """logit [B,K,T,F] fp32, obs complex64 [B,T,F] -> mask [B,K,T,F], est complex64 [B,K,T,F]"""
    B, K, T, F = logit.shape
    logit = _f32(logit).contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    mask = torch.empty_like(logit)
    est = torch.empty(B, K, T, F, 2, device=logit.device, dtype=torch.float32)
    with _timed("maskhead_fwd", 0, B * T * (16 * K * F + 8 * F)):
        check(_lib.lib().tssep_maskhead_fwd(_p(logit), _p(obs_r), _p(mask), _p(est), B, K, T, F,
                                            _stream()), "maskhead_fwd")
    return mask, torch.view_as_complex(est)


def maskhead_bwd(dest, dmask, mask, obs):
    B, K, T, F = mask.shape
    dest_r = torch.view_as_real(dest.contiguous())
    obs_r = torch.view_as_real(obs.contiguous())
    dlogit = torch.empty_like(mask)
    if dmask is not None:
        dmask = _f32(dmask).contiguous()
    with _timed("maskhead_bwd", 0, B * T * (16 * K * F + 8 * F)):
        check(_lib.lib().tssep_maskhead_bwd(_p(dest_r), _p(dmask), _p(mask), _p(obs_r), _p(dlogit),
                                            B, K, T, F, _stream()), "maskhead_bwd")
    return dlogit


def maskhead_gated_fwd(logit, obs, with_est=True):
    """explicit_vad: logit [B,K,T,F+1] (VAD logit at column 0), obs complex64 [B,T,F] -> mask [B,K,T,F] =
    sigmoid(l) sigmoid(v), est complex64 [B,K,T,F] = obs * mask (None without with_est), vmask [B,K,T] = sigmoid(v)"""
    B, K, T, F1 = logit.shape
    assert tuple(obs.shape) == (B, T, F1 - 1) and obs.dtype == torch.complex64, (tuple(logit.shape), tuple(obs.shape))
    logit = _f32(logit).contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    mask = torch.empty(B, K, T, F1 - 1, device=logit.device, dtype=torch.float32)
    vmask = torch.empty(B, K, T, device=logit.device, dtype=torch.float32)
    est = torch.empty(B, K, T, F1 - 1, 2, device=logit.device, dtype=torch.float32) if with_est else None
    check(_lib.lib().tssep_maskhead_gated_fwd(_p(logit), _p(obs_r), _p(mask), _p(est), _p(vmask), B, K, T, F1 - 1,
                                              _stream()), "maskhead_gated_fwd")
    return mask, (torch.view_as_complex(est) if est is not None else None), vmask


def maskhead_gated_bwd(dest, dmask, dvmask, logit, obs):
    """-> dlogit [B,K,T,F+1]; dest (complex64), dmask [B,K,T,F] and dvmask [B,K,T] may each be None."""
    B, K, T, F1 = logit.shape
    assert tuple(obs.shape) == (B, T, F1 - 1) and obs.dtype == torch.complex64, (tuple(logit.shape), tuple(obs.shape))
    for t_, shape in ((dest, (B, K, T, F1 - 1)), (dmask, (B, K, T, F1 - 1)), (dvmask, (B, K, T))):
        assert t_ is None or tuple(t_.shape) == shape, (tuple(t_.shape), shape)
    assert dest is None or dest.dtype == torch.complex64
    logit = _f32(logit).contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    dest_r = torch.view_as_real(dest.contiguous()) if dest is not None else None
    dmask = _f32(dmask).contiguous() if dmask is not None else None
    dvmask = _f32(dvmask).contiguous() if dvmask is not None else None
    dlogit = torch.empty_like(logit)
    check(_lib.lib().tssep_maskhead_gated_bwd(_p(dest_r), _p(dmask), _p(dvmask), _p(logit), _p(obs_r), _p(dlogit),
                                              B, K, T, F1 - 1, _stream()), "maskhead_gated_bwd")
    return dlogit


def mask_mul_fwd(mask, obs):
    B, K, T, F = mask.shape
    est = torch.empty(B, K, T, F, 2, device=mask.device, dtype=torch.float32)
    check(_lib.lib().tssep_mask_mul_fwd(_p(_f32(mask).contiguous()),
                                        _p(torch.view_as_real(obs.contiguous())), _p(est), B, K, T,
                                        F, _stream()), "mask_mul_fwd")
    return torch.view_as_complex(est)


def mask_mul_bwd(dest, obs):
    B, K, T, F = dest.shape
    dmask = torch.empty(B, K, T, F, device=dest.device, dtype=torch.float32)
    check(_lib.lib().tssep_mask_mul_bwd(_p(torch.view_as_real(dest.contiguous())),
                                        _p(torch.view_as_real(obs.contiguous())), _p(dmask), B, K,
                                        T, F, _stream()), "mask_mul_bwd")
    return dmask


# ----------------------------------------------------------------------------- beamformer
def mvdr_souden(masks, obs, reference_channel, eps=None, masking=False, masking_eps=0.0,
                check_singular=True, return_state=False):
    """TorchBF('mvdr_souden'), tssep/train/enhancer.py:215-265.
    masks [B,K,M,T,F] fp32|fp64 (M = 1|2), obs [B,D,T,F] complex128 -> enh [B,K,T,F] complex128.
    eps None = torch.finfo(float64).tiny, as the reference.  Raises torch.linalg.LinAlgError for a
    singular interference PSD like torch.linalg.solve does (one host sync; check_singular=False
    skips it).  return_state=True: (enh, state), state what mvdr_souden_bwd needs -- the workspace
    of this call (reduced statistics, wconj) and the arguments as the kernels saw them."""
    L = _lib.lib()
    assert masks.is_cuda and obs.is_cuda, (masks.device, obs.device)
    assert obs.dtype == torch.complex128, obs.dtype
    if masks.dtype not in (torch.float32, torch.float64):
        masks = masks.to(torch.float64)
    B, K, M, T, F = masks.shape
    Bo, D, To, Fo = obs.shape
    assert (B, T, F) == (Bo, To, Fo), (masks.shape, obs.shape)
    if M not in (1, 2):
        raise ValueError(masks.shape)
    masks = masks.contiguous()
    obs_r = torch.view_as_real(obs.contiguous())
    ws_bytes = L.tssep_mvdr_workspace_bytes(B, K, D, T, F)
    if ws_bytes <= 0:
        raise RuntimeError(f"mvdr_souden: unsupported shape masks {tuple(masks.shape)} "
                           f"obs {tuple(obs.shape)} (at most 8 channels)")
    ws = torch.empty(ws_bytes // 8 + 2, device=obs.device, dtype=torch.float64)
    info = torch.empty(1, device=obs.device, dtype=torch.int32)
    enh = torch.empty(B, K, T, F, 2, device=obs.device, dtype=torch.float64)
    eps = float(torch.finfo(torch.float64).tiny) if eps is None else float(eps)
    # torch.clamp(mask, min=masking_eps) compares in the mask's dtype (enhancer.py:261-263)
    masking_eps = float(torch.tensor(float(masking_eps), dtype=masks.dtype))
    msz = masks.element_size()
    nbytes = B * T * F * (32 * D + K * M * msz + 16 * K + (K * msz if masking else 0))
    with _timed("mvdr_souden", 0, nbytes):
        check(L.tssep_mvdr_souden_fwd(_p(obs_r), _p(masks), int(masks.dtype == torch.float64),
                                      _p(enh), _p(ws), _p(info), B, K, M, D, T, F,
                                      int(reference_channel), eps, int(bool(masking)),
                                      float(masking_eps), _stream()), "mvdr_souden")
    if check_singular:
        n = int(info.item())
        if n:
            raise torch.linalg.LinAlgError(
                f"mvdr_souden: the solver failed because the interference PSD matrix is singular "
                f"({n} of {B * K * F} (batch, speaker, frequency) systems)")
    if return_state:
        return torch.view_as_complex(enh), dict(ws=ws, masks=masks, obs_r=obs_r, ref=int(reference_channel), eps=eps,
                                                masking=int(bool(masking)), masking_eps=float(masking_eps))
    return torch.view_as_complex(enh)


def mvdr_bwd_workspace(B, K, M, D, T, F, device):
    """The backward's workspace (tssep_mvdr_bwd_workspace_bytes: the gw partials, then the packed Hermitian matrices)."""
    nbytes = _lib.lib().tssep_mvdr_bwd_workspace_bytes(B, K, M, D, T, F)
    if nbytes <= 0:
        raise RuntimeError(f"mvdr_souden_bwd: unsupported shape B={B} K={K} M={M} D={D} T={T} F={F} (at most 8 channels)")
    return torch.empty(nbytes // 8, device=device, dtype=torch.float64)


def mvdr_souden_bwd(genh, state):
    """d(loss)/d(masks) of mvdr_souden: genh [B,K,T,F] complex128 = d(loss)/d(enh), `state` from
    mvdr_souden(..., return_state=True) -> dmask [B,K,M,T,F] in the masks' dtype.  Three HIP stages
    (csrc/mvdr.hip: gw over time, the per-bin solve, the quadratic forms over time); no host sync."""
    L = _lib.lib()
    masks, obs_r = state["masks"], state["obs_r"]
    B, K, M, T, F = masks.shape
    D = obs_r.shape[1]
    assert genh.is_cuda and genh.dtype == torch.complex128 and tuple(genh.shape) == (B, K, T, F), (genh.dtype, genh.shape)
    g_r = torch.view_as_real(genh.contiguous())
    ws = mvdr_bwd_workspace(B, K, M, D, T, F, masks.device)
    dmask = torch.empty_like(masks)
    msz = masks.element_size()
    nbytes = B * T * F * (32 * D + 16 * K * (2 if state["masking"] else 1) + K * M * msz + (K * msz if state["masking"] else 0))
    with _timed("mvdr_souden_bwd", 0, nbytes):
        check(L.tssep_mvdr_souden_bwd(_p(obs_r), _p(masks), int(masks.dtype == torch.float64), _p(g_r), _p(state["ws"]),
                                      _p(ws), _p(dmask), B, K, M, D, T, F, state["ref"], state["eps"], state["masking"],
                                      state["masking_eps"], _stream()), "mvdr_souden_bwd")
    return dmask


def online_mvdr_check(masks, Y, state=None, reference_channel=0, forgetting=1.0, diag_load=1e-6):
    """What `online_mvdr` refuses, from the arguments alone (CPU tensors do: nothing is launched) -> masks [B,K,Tc,F]."""
    if masks.dim() == 5:
        if masks.shape[2] != 1:
            raise NotImplementedError(f"online_mvdr with nmask = {masks.shape[2]} (masks {tuple(masks.shape)}): the "
                                      "recursion takes one mask per speaker, the interference is 1 - mask")
        masks = masks[:, :, 0]
    if masks.dim() != 4 or Y.dim() != 4:
        raise ValueError(f"online_mvdr: masks [B,K,1,Tc,F] or [B,K,Tc,F] and Y [B,D,Tc,F], got {tuple(masks.shape)} and "
                         f"{tuple(Y.shape)}")
    B, K, T, F = masks.shape
    Bo, D, To, Fo = Y.shape
    if (B, T, F) != (Bo, To, Fo):
        raise ValueError(f"online_mvdr: masks {tuple(masks.shape)} and Y {tuple(Y.shape)} differ in batch, frames or bins")
    if min(B, K, T, F, D) < 1 or D > 8:
        raise ValueError(f"online_mvdr: empty axis or more than 8 channels: masks {tuple(masks.shape)}, Y {tuple(Y.shape)}")
    if Y.dtype not in (torch.complex64, torch.complex128):
        raise TypeError(f"online_mvdr: Y is {Y.dtype}, complex64 or complex128 is required")
    if masks.is_complex():
        raise TypeError(f"online_mvdr: masks are {masks.dtype}")
    if not 0 <= int(reference_channel) < D:
        raise ValueError(f"online_mvdr: reference_channel = {reference_channel} of {D} channels")
    if not 0.0 < float(forgetting) <= 1.0:
        raise ValueError(f"online_mvdr: forgetting = {forgetting} lies outside (0, 1]")
    if not float(diag_load) >= 0.0:
        raise ValueError(f"online_mvdr: diag_load = {diag_load} is negative")
    if state is not None and (state.dtype != torch.float64 or tuple(state.shape) != (B, K, 2, D * D, F)):
        raise ValueError(f"online_mvdr: state is {state.dtype} {tuple(state.shape)}, what a call with K = {K} speakers, "
                         f"D = {D} channels and F = {F} bins carries is float64 {(B, K, 2, D * D, F)} (a channel or "
                         "speaker mismatch between the calls of a stream?)")
    return masks


def online_mvdr(masks, Y, state=None, reference_channel=0, forgetting=1.0, diag_load=1e-6, eps=None, masking=False,
                masking_eps=0.0):
    """The frame-recursive MVDR of DESIGN 4.18 on the next Tc frames of a stream: masks [B,K,1,Tc,F] or [B,K,Tc,F] fp32 |
    fp64, Y [B,D,Tc,F] complex64 | complex128, state what the call before returned (None: a fresh stream) ->
    (enh [B,K,Tc,F] complex128, the new state: float64 [B,K,2,D*D,F], the packed Hermitian Phi_s and Phi_n).  masking_eps
    is compared in the masks' dtype, as in mvdr_souden; eps None = torch.finfo(float64).tiny.  One launch, no host sync; output and state do not depend on how the frames are split over calls."""
    masks = online_mvdr_check(masks, Y, state, reference_channel, forgetting, diag_load)
    L = _lib.lib()
    assert masks.is_cuda and Y.is_cuda and (state is None or state.is_cuda), (masks.device, Y.device)
    if masks.dtype not in (torch.float32, torch.float64):
        masks = masks.to(torch.float64)
    masks = masks.contiguous()
    B, K, T, F = masks.shape
    D = Y.shape[1]
    y_r = torch.view_as_real(Y.contiguous())
    state = None if state is None else state.contiguous()
    assert L.tssep_mvdr_online_state_bytes(B, K, D, F) == 8 * B * K * 2 * D * D * F
    state_out = torch.empty(B, K, 2, D * D, F, device=Y.device, dtype=torch.float64)
    enh = torch.empty(B, K, T, F, 2, device=Y.device, dtype=torch.float64)
    eps = float(torch.finfo(torch.float64).tiny) if eps is None else float(eps)
    masking_eps = float(torch.tensor(float(masking_eps), dtype=masks.dtype))      # compared in the mask's dtype, as mvdr_souden
    nbytes = B * T * F * (y_r.element_size() * 2 * D + K * (masks.element_size() + 16)) + 32 * B * K * D * D * F
    with _timed("mvdr_online", 0, nbytes):
        check(L.tssep_mvdr_online_fwd(_p(y_r), int(Y.dtype == torch.complex128), _p(masks),
                                      int(masks.dtype == torch.float64), _p(state), _p(state_out), _p(enh), B, K, D, T, F,
                                      int(reference_channel), float(forgetting), float(diag_load), eps,
                                      int(bool(masking)), masking_eps, _stream()), "mvdr_online")
    return torch.view_as_complex(enh), state_out


DISTORTION_MODES = {"sum_cross_talker": 0, "one_minus": 1}


def segment_table(segments, device):
    """[(k, s, e), ...] or an int tensor [S,3] -> int32 [S,3] on `device` (a device tensor of that
    form passes through untouched: nothing is copied, the call stays capturable)."""
    if isinstance(segments, torch.Tensor):
        tab = segments
    else:
        tab = torch.tensor([tuple(int(v) for v in row) for row in segments], dtype=torch.int32).reshape(-1, 3)
    assert tab.dim() == 2 and tab.shape[1] == 3, tab.shape
    return tab.to(device=device, dtype=torch.int32).contiguous()


def _segment_args(masks, obs, segments):
    assert masks.is_cuda and obs.is_cuda, (masks.device, obs.device)
    assert obs.dtype == torch.complex128, obs.dtype
    if masks.dtype not in (torch.float32, torch.float64):
        masks = masks.to(torch.float64)
    K, M, T, F = masks.shape
    D, To, Fo = obs.shape
    assert (T, F) == (To, Fo), (masks.shape, obs.shape)
    if M != 1:
        raise NotImplementedError(f"segment_mvdr: masks {tuple(masks.shape)}: one mask per speaker (M = 1), the "
                                  f"distortion mask comes from the other speakers' masks")
    tab = segment_table(segments, obs.device)
    S = tab.shape[0]
    assert S > 0, "segment_mvdr: empty segment table"
    ws_bytes = _lib.lib().tssep_mvdr_segments_workspace_bytes(K, S, D, T, F)
    if ws_bytes <= 0:
        raise RuntimeError(f"segment_mvdr: unsupported shape masks {tuple(masks.shape)} obs {tuple(obs.shape)} "
                           f"with {S} segments (at most 8 channels)")
    ws = torch.empty(ws_bytes // 8 + 2, device=obs.device, dtype=torch.float64)
    return masks.contiguous(), torch.view_as_real(obs.contiguous()), tab, ws, (K, S, D, T, F)


def segment_psd(masks, obs, segments, mode="sum_cross_talker", distortion_eps=1e-4, mask_power=1,
                psd_real=True):
    """The statistics stage of segment_mvdr alone: (target, distortion) PSDs [S,2,F,D,D] complex128 of
    _get_psd (tssep/train/enhancer.py:268-289) for every row of the segment table."""
    masks, obs_r, tab, ws, (K, S, D, T, F) = _segment_args(masks, obs, segments)
    check(_lib.lib().tssep_mvdr_segments_psd(_p(obs_r), _p(masks), int(masks.dtype == torch.float64), _p(tab),
                                             _p(ws), K, S, D, T, F, DISTORTION_MODES[mode],
                                             float(distortion_eps), float(mask_power), int(bool(psd_real)),
                                             _stream()), "segment_psd")
    rows = ws[:S * 2 * D * D * F].view(S, 2, D * D, F)
    psd = torch.zeros(S, 2, F, D, D, device=obs.device, dtype=torch.complex128)
    p = 0
    for i in range(D):
        psd[..., i, i] = rows[:, :, i]
        for j in range(i + 1, D):
            v = torch.complex(rows[:, :, D + 2 * p], rows[:, :, D + 2 * p + 1])
            psd[..., i, j], psd[..., j, i] = v, v.conj()
            p += 1
    return psd


def segment_mvdr(masks, obs, segments, mode="sum_cross_talker", distortion_eps=1e-4, mask_power=1,
                 eps=None, masking=False, masking_eps=0.0, psd_real=True, check_singular=True,
                 out=None, obs_seg=None, row0=None, check_table=False):
    """ClassicBF_np('mvdr_souden', segment_bf=True), tssep/train/enhancer.py:451-590: one Souden MVDR
    per row (speaker, start, end) of `segments` from the statistics of that interval, the distortion
    mask from the other speakers' masks (mode), filtered over the interval; zero elsewhere.
    masks [K,1,T,F] fp32|fp64, obs [D,T,F] complex128 -> [K,T,F] complex128 (written into `out`
    when given).  segments: [(k, s, e), ...] or an int32 [S,3] tensor (on the device: no copy, no
    sync).  A constant number of launches whatever S is.  Raises torch.linalg.LinAlgError naming
    the (speaker, start, end) segments with a singular distortion PSD (one host read;
    check_singular=False skips it, the call is then free of host syncs and capturable).
    obs_seg [D,N,F] with row0 [S+1] (what `wpe` returns for the (s, e) columns of the same table): every row takes
    its statistics and its filter input from its own packed frames instead of obs[:, s:e].
    check_table: the table travels to the host in the copy of the singular check and a row outside [0, K) x [0, T] or
    an empty one raises ValueError: a device-born table is checked without a host read of its own (the kernels ignore
    such rows, no access leaves the buffers)."""
    L = _lib.lib()
    masks, obs_r, tab, ws, (K, S, D, T, F) = _segment_args(masks, obs, segments)
    if (obs_seg is None) != (row0 is None):
        raise ValueError("segment_mvdr: obs_seg and row0 come together")
    if obs_seg is not None:
        assert obs_seg.is_cuda and obs_seg.dtype == torch.complex128 and obs_seg.is_contiguous(), obs_seg.dtype
        assert obs_seg.dim() == 3 and obs_seg.shape[0] == D and obs_seg.shape[2] == F, (obs_seg.shape, obs.shape)
        assert row0.is_cuda and row0.dtype == torch.int64 and row0.shape == (S + 1,), (row0.dtype, row0.shape)
    info = torch.empty(S, device=obs.device, dtype=torch.int32)
    if out is None:
        out = torch.empty(K, T, F, device=obs.device, dtype=torch.complex128)
    assert out.shape == (K, T, F) and out.dtype == torch.complex128 and out.is_contiguous(), out.shape
    eps = float(torch.finfo(torch.float64).tiny) if eps is None else float(eps)
    msz = masks.element_size()
    nbytes = T * F * (K * msz + 16 * K) + 2 * T * F * 16 * D
    tail = (K, S, D, T, F, DISTORTION_MODES[mode], float(distortion_eps), float(mask_power), int(bool(psd_real)),
            eps, int(bool(masking)), float(masking_eps), _stream())
    with _timed("segment_mvdr", 0, nbytes):
        if obs_seg is None:
            check(L.tssep_mvdr_segments_fwd(_p(obs_r), _p(masks), int(masks.dtype == torch.float64), _p(tab),
                                            _p(torch.view_as_real(out)), _p(ws), _p(info), *tail), "segment_mvdr")
        else:
            check(L.tssep_mvdr_segments_fwd_obs(_p(torch.view_as_real(obs_seg)), _p(row0), obs_seg.shape[1],
                                                _p(masks), int(masks.dtype == torch.float64), _p(tab),
                                                _p(torch.view_as_real(out)), _p(ws), _p(info), *tail),
                  "segment_mvdr (packed observation)")
    if check_singular:
        host = (torch.cat([info, tab.reshape(-1)]) if check_table else info).cpu().numpy()
        bad = host[:S]
        if check_table:
            r = host[S:].reshape(S, 3)
            wrong = (r[:, 0] < 0) | (r[:, 0] >= K) | (r[:, 1] < 0) | (r[:, 2] > T) | (r[:, 1] >= r[:, 2])
            if wrong.any():
                raise ValueError(f"segment_mvdr: rows {[tuple(int(v) for v in x) for x in r[wrong][:8]]} of the segment "
                                 f"table lie outside speakers [0, {K}) x frames [0, {T}] or are empty")
        if bad.any():
            rows = tab.cpu().numpy()
            failed = [tuple(int(v) for v in rows[i]) for i in bad.nonzero()[0]]
            raise torch.linalg.LinAlgError(
                f"segment_mvdr: the solver failed because the distortion PSD matrix is singular in "
                f"{len(failed)} of {S} segments (speaker, start, end): {failed}")
    return out


# ------------------------------------------------------ masks -> segment table (csrc/segments.hip)
def segments_capacity(K, T):
    """Rows of the table buffer of activity_segments: K * ceil(T / 2); 0 for a shape the kernels refuse.  Host only."""
    return int(_lib.lib().tssep_segments_capacity(int(K), int(T)))


def mask_activity(masks):
    """masks [K, M, T, F] -> activity float32 [K, T] = fl32(sum_f masks[k, 0, t, f]) / fl32(F): mask index 0 (the target
    mask when M = 2), read by stride -- index 1 is never touched and nothing is copied.  One pass over K*T*F*4 bytes, the
    sum in float32 in a fixed order (two calls give the same bits), one correctly rounded division.  float64 masks are
    cast to float32 once, here, before the pass (mask index 0 only); any other dtype is refused."""
    assert masks.is_cuda and masks.dim() == 4, (masks.device, masks.shape)
    if masks.dtype == torch.float64:
        masks = masks[:, :1].to(torch.float32)
    m = _f32(masks.detach()).contiguous()
    K, M, T, F = m.shape
    act = torch.empty(K, T, device=m.device, dtype=torch.float32)
    with _timed("mask_activity", 0, 4 * K * T * (F + 1)):
        check(_lib.lib().tssep_mask_activity(_p(m), K, M, T, F, _p(act), _stream()), "mask_activity")
    return act


def check_segment_params(dilation=1, erosion=1, min_frames=1):
    """ValueError for an even or non-positive window or min_frames < 1: on the host, before any launch."""
    for name, w in (("dilation", dilation), ("erosion", erosion)):
        if int(w) != w or w < 1 or w % 2 == 0:
            raise ValueError(f"{name}={w!r}: the window is an odd number of frames >= 1")
    if int(min_frames) != min_frames or min_frames < 1:
        raise ValueError(f"min_frames={min_frames!r}: at least 1")


def activity_segments(activity, threshold=0.5, dilation=1, erosion=1, min_frames=1, return_count=False):
    """activity float32 [K, T] -> the segment table int32 [S, 3] of segment_mvdr, rows (k, s, e) sorted by k then s, on
    the device: b = activity > threshold (strict, in float32; NaN is inactive), binary dilation then erosion with odd
    windows clipped to the row, maximal runs, runs shorter than min_frames dropped.  Nine launches whatever
    T, the content and the number of runs; the same table on every call.
    The result is a view of the capacity buffer [K * ceil(T / 2), 3] cut to the count.  Reading that count is the ONE
    host synchronisation of the route masks -> table: S is a tensor shape.  return_count=True returns
    (buffer, count) instead, count an int32 [1] device tensor, with no synchronisation; rows past the count are
    undefined."""
    check_segment_params(dilation, erosion, min_frames)
    a = _f32(activity.detach()).contiguous()
    assert a.dim() == 2, a.shape
    K, T = a.shape
    cap = segments_capacity(K, T)
    if cap <= 0:
        raise RuntimeError(f"activity_segments: unsupported shape {tuple(a.shape)}")
    table = torch.empty(cap, 3, device=a.device, dtype=torch.int32)
    count = torch.empty(1, device=a.device, dtype=torch.int32)
    ws = torch.empty(9 * cap + 16, device=a.device, dtype=torch.int32)
    with _timed("activity_segments", 0, 12 * K * T):
        check(_lib.lib().tssep_activity_segments(_p(a), K, T, float(threshold), int(dilation), int(erosion),
                                                 int(min_frames), _p(table), _p(count), _p(ws), _stream()),
              "activity_segments")
    if return_count:
        return table, count
    return table[:int(count.item())]


# ----------------------------------------------------------------------------- WPE
WPE_MAX_CHANNELS, WPE_MAX_ROWS, WPE_MAX_DELAY = 8, 80, 256


def wpe_check_args(D, taps, delay, iterations, statistics_mode):
    """The limits of csrc/wpe.hip, checked on the host before anything touches the device."""
    if statistics_mode not in ("full", "valid"):
        raise ValueError(f"wpe: statistics_mode {statistics_mode!r}: 'full' or 'valid'")
    if int(taps) != taps or int(delay) != delay or int(iterations) != iterations:
        raise ValueError(f"wpe: taps, delay and iterations are integers, got {(taps, delay, iterations)}")
    if not 1 <= D <= WPE_MAX_CHANNELS:
        raise ValueError(f"wpe: {D} channels: the kernels are built for 1 to {WPE_MAX_CHANNELS}")
    if taps < 1 or taps * D > WPE_MAX_ROWS:
        raise ValueError(f"wpe: taps * channels = {taps} * {D} = {taps * D}: the per-bin systems are built for 1 to "
                         f"{WPE_MAX_ROWS} rows (the matrix lives in LDS)")
    if not 0 <= delay <= WPE_MAX_DELAY:
        raise ValueError(f"wpe: delay {delay}: 0 to {WPE_MAX_DELAY}")
    if iterations < 1:
        raise ValueError(f"wpe: iterations {iterations}: at least 1")


def wpe_rows(segments, T):
    """[(s, e), ...] (or an int tensor [S,2]; it is read on the host: the packed size is a host number) ->
    list of (s, e) ints, each inside [0, T]."""
    if isinstance(segments, torch.Tensor):
        segments = segments.detach().cpu().tolist()
    rows = [(int(s), int(e)) for s, e in segments]
    for s, e in rows:
        if not 0 <= s <= e <= T:
            raise ValueError(f"wpe: row ({s}, {e}) is not inside [0, {T}]")
    return rows


def wpe_validate(obs, segments, taps, delay, iterations, statistics_mode):
    """Every host-side refusal of `wpe` (dtype, limits, rows inside [0, T], the rank rule) -> rows, (D, T, F)"""
    if obs.dtype != torch.complex128:
        raise TypeError(f"wpe: {obs.dtype}: the observation must be complex128 (the per-bin systems reach condition "
                        f"numbers of 1e11 on reverberant data; complex64 loses the whole result there)")
    assert obs.dim() == 3, obs.shape
    D, T, F = obs.shape
    wpe_check_args(D, taps, delay, iterations, statistics_mode)
    rows = wpe_rows([(0, T)] if segments is None else segments, T)
    if not rows:
        raise ValueError("wpe: empty segment table")
    hist = delay + (taps - 1 if statistics_mode == "valid" else 0)
    short = [r for r in rows if r[1] - r[0] - hist < taps * D]
    if short:
        raise ValueError(f"wpe: {len(short)} of {len(rows)} rows (start, end) have fewer than taps * channels = "
                         f"{taps * D} frames behind the first {hist}: the correlation matrix cannot have full rank there: "
                         f"{short}")
    return rows, (D, T, F)


_WPE_TABLES = {}        # (device, rows) -> (table int32 [S,2], row0 int64 [S+1]) on the device


def wpe_table(rows, device):
    """[(s, e), ...] -> (int32 [S,2] table, int64 [S+1] prefix of the row lengths) on `device`.  The pair is kept: a
    later call with the same rows copies nothing from the host, so it neither synchronises nor breaks a capture."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, tuple(rows))
    hit = _WPE_TABLES.get(key)
    if hit is None:
        if len(_WPE_TABLES) >= 64:
            _WPE_TABLES.pop(next(iter(_WPE_TABLES)))
        r0 = np.concatenate([[0], np.cumsum([e - s for s, e in rows])]).astype(np.int64)
        hit = (torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 2).to(device), torch.from_numpy(r0).to(device))
        _WPE_TABLES[key] = hit
    return hit


def wpe(obs, segments=None, taps=10, delay=2, iterations=3, statistics_mode="full", check_singular=True, row0=None,
        N=None, _rows=None):
    """WPE dereverberation (nara_wpe's wpe_v8 with psd_context=0; csrc/wpe.hip).  obs [D,T,F] complex128 on the
    device.  segments None: the whole array -> [D,T,F].  segments [(s, e), ...]: every row dereverberated as if
    obs[:, s:e] were the whole array (rows may overlap or repeat) -> (obs_seg [D,N,F], row0 int64 [S+1] on the
    device), row i at obs_seg[:, row0[i]:row0[i+1]].  A fixed number of launches per iteration whatever the table
    holds.  Rows too short for a full-rank correlation matrix raise ValueError before any launch; a factorisation
    that meets a pivot that is not positive raises torch.linalg.LinAlgError naming the (start, end) rows (one host
    read; check_singular=False skips it).
    Host traffic: a table given as a list is copied to the device the first time it is seen (wpe_table keeps the last
    64), so with check_singular=False every later call with the same rows is free of host transfers.  A table that is
    already on the device goes in as `segments` int32 [S,2] with `row0` int64 [S+1] and the host number N = row0[S]
    (what wpe_table returns): nothing is read back.  The rows of a device table are NOT checked on the host: a row
    outside [0, T] is clamped by the kernels, and a row too short for the rank rule does not raise ValueError but shows
    as LinAlgError, or with check_singular=False as NaN in its packed frames.
    Capture: a graph keeps only the pointers of the table and of row0.  A captured call must therefore pass the device
    table (segments, row0, N) and the caller keeps those tensors alive as long as the graph; a list table lives in
    wpe_table's store only until 64 other tables have displaced it.
    Memory: the workspace holds li [N,F], R [S,F,K,K], P, G and the chunk partials for all rows at once, K = taps * D:
    16 F (S K (K + 2 D) + 16 tiles (N / 256 + S)) bytes, tiles = K / 4 (K / 4 + 1) / 2 + K / 4 (D + 3) / 4 -- 0.12 GB
    for one 30-s utterance at K = 60, 5.5 GB for 80 rows; it is allocated per call (torch's caching allocator)."""
    if isinstance(segments, torch.Tensor) and row0 is not None:
        if obs.dtype != torch.complex128:
            raise TypeError(f"wpe: {obs.dtype}: the observation must be complex128")
        assert obs.dim() == 3, obs.shape
        D, T, F = obs.shape
        wpe_check_args(D, taps, delay, iterations, statistics_mode)
        if N is None:
            raise ValueError("wpe: a device table comes with row0 and the host number N = row0[S]")
        assert segments.is_cuda and segments.dtype == torch.int32 and segments.dim() == 2 and segments.shape[1] == 2 \
            and segments.is_contiguous(), (segments.dtype, segments.shape)
        S = segments.shape[0]
        assert row0.is_cuda and row0.dtype == torch.int64 and row0.shape == (S + 1,), (row0.dtype, row0.shape)
        tab, N, rows = segments, int(N), None
    else:
        if row0 is not None or N is not None:
            raise ValueError("wpe: row0 and N come with a device table")
        # _rows: what wpe_validate returned to a caller that had to refuse before moving obs to the device
        rows, (D, T, F) = _rows or wpe_validate(obs, segments, taps, delay, iterations, statistics_mode)
        tab, row0 = wpe_table(rows, obs.device)
        S, N = len(rows), sum(e - s for s, e in rows)
    assert obs.is_cuda, obs.device
    ws_bytes = _lib.lib().tssep_wpe_workspace_bytes(S, N, D, T, F, int(taps), int(delay))
    if ws_bytes <= 0:
        raise RuntimeError(f"wpe: unsupported shape obs {(D, T, F)} with {S} rows, taps {taps}, delay {delay}")
    ws = torch.empty(ws_bytes // 8 + 2, device=obs.device, dtype=torch.float64)
    obs_r = torch.view_as_real(obs.contiguous())
    info = torch.empty(S, device=obs.device, dtype=torch.int32)
    out = torch.empty(D, N, F, device=obs.device, dtype=torch.complex128)
    K = taps * D
    flops = iterations * N * F * 8 * (K * (K + 1) // 2 + 2 * K * D)
    with _timed("wpe", flops, 0):
        check(_lib.lib().tssep_wpe_fwd(_p(obs_r), _p(tab), _p(row0), _p(torch.view_as_real(out)), _p(ws), _p(info),
                                       S, N, D, T, F, int(taps), int(delay), int(iterations),
                                       int(statistics_mode == "valid"), _stream()), "wpe")
    if check_singular:
        bad = info.cpu().numpy()
        if bad.any():
            rows = rows if rows is not None else [tuple(r) for r in tab.cpu().tolist()]
            failed = [rows[i] for i in bad.nonzero()[0]]
            raise torch.linalg.LinAlgError(
                f"wpe: the factorisation of the correlation matrix met a pivot that is not positive in "
                f"{len(failed)} of {S} rows (start, end): {failed}")
    return out if segments is None else (out, row0)


WPE_MAX_POWER_CONTEXT = 256
OnlineWPEState = collections.namedtuple("OnlineWPEState", "Q G ring pmax info")
OnlineWPEState.__doc__ = """What a stream of `online_wpe` carries: Q [B,F,K(K+1)/2] complex128 (the lower triangle of the
inverse correlation matrix, row by row), G [B,F,K,D] complex128, ring [B,F,R,D] complex128 (the last
R = max(delay + taps - 1, power_context) frames, oldest first), pmax [B,F] float64, info [B] int32 (the frames whose update
was refused, counted over the stream).  All zeros: a fresh stream."""


def online_wpe_state_shapes(B, D, F, taps, delay, power_context):
    K = taps * D
    R = max(delay + taps - 1, power_context)
    return OnlineWPEState(((B, F, K * (K + 1) // 2), torch.complex128), ((B, F, K, D), torch.complex128),
                          ((B, F, R, D), torch.complex128), ((B, F), torch.float64), ((B,), torch.int32))


def online_wpe_check(Y, state=None, taps=10, delay=2, forgetting=0.99, load=1.0, power_context=0):
    """What `online_wpe` refuses, from the arguments alone (CPU tensors do: nothing is launched) -> (B, D, Tc, F)."""
    if not isinstance(Y, torch.Tensor) or Y.dim() != 4:
        raise ValueError(f"online_wpe: Y [B,D,Tc,F], got {tuple(Y.shape) if isinstance(Y, torch.Tensor) else type(Y)}")
    if Y.dtype not in (torch.complex64, torch.complex128):
        raise TypeError(f"online_wpe: Y is {Y.dtype}, complex64 or complex128 is required")
    B, D, T, F = Y.shape
    if int(taps) != taps or int(delay) != delay or int(power_context) != power_context:
        raise ValueError(f"online_wpe: taps, delay and power_context are integers, got {(taps, delay, power_context)}")
    if min(B, T, F) < 1:
        raise ValueError(f"online_wpe: empty axis: Y {tuple(Y.shape)}")
    if not 1 <= D <= WPE_MAX_CHANNELS:
        raise ValueError(f"online_wpe: {D} channels: the kernel is built for 1 to {WPE_MAX_CHANNELS}")
    if taps < 1 or taps * D > WPE_MAX_ROWS:
        raise ValueError(f"online_wpe: taps * channels = {taps} * {D} = {taps * D}: the inverse correlation matrix is built "
                         f"for 1 to {WPE_MAX_ROWS} rows (it lives in LDS)")
    if not 0 <= delay <= WPE_MAX_DELAY:
        raise ValueError(f"online_wpe: delay {delay}: 0 to {WPE_MAX_DELAY}")
    if not 0 <= power_context <= WPE_MAX_POWER_CONTEXT:
        raise ValueError(f"online_wpe: power_context {power_context}: 0 to {WPE_MAX_POWER_CONTEXT} frames")
    if not 0.0 < float(forgetting) <= 1.0:
        raise ValueError(f"online_wpe: forgetting = {forgetting} lies outside (0, 1]")
    if not 0.0 < float(load) < float("inf"):
        raise ValueError(f"online_wpe: load = {load} is not positive and finite (Q starts as I / load)")
    if Y.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("online_wpe is evaluation-time only: Y requires grad and the recursion has no backward "
                                  "(call it under torch.no_grad())")
    if state is not None:
        want = online_wpe_state_shapes(B, D, F, int(taps), int(delay), int(power_context))
        if not isinstance(state, tuple) or len(state) != len(want):
            raise ValueError(f"online_wpe: state is {type(state).__name__}, not the OnlineWPEState an earlier call returned")
        for name, t, (shape, dtype) in zip(OnlineWPEState._fields, state, want):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != shape:
                got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"online_wpe: state.{name} is {got}, what a call with B = {B}, D = {D}, F = {F}, taps = "
                                 f"{taps}, delay = {delay}, power_context = {power_context} carries is {dtype} {shape} "
                                 "(did the channels or the parameters change between the calls of a stream?)")
    return B, D, T, F


def online_wpe(Y, state=None, taps=10, delay=2, forgetting=0.99, load=1.0, power_context=0):
    """The recursive WPE of DESIGN 4.19 on the next Tc frames of a stream: Y [B,D,Tc,F] complex64 | complex128, state what
    the call before returned (None: a fresh stream) -> (X [B,D,Tc,F] complex128, the new `OnlineWPEState`).  The output of a
    frame uses the filter of the frames before it.  One launch, no host sync (state.info stays on the device: read it
    when the stream allows); output and state do not depend on how the frames are split over calls."""
    B, D, T, F = online_wpe_check(Y, state, taps, delay, forgetting, load, power_context)
    L = _lib.lib()
    assert Y.is_cuda and (state is None or all(t.is_cuda for t in state)), Y.device
    taps, delay, pc = int(taps), int(delay), int(power_context)
    y_r = torch.view_as_real(Y.detach().contiguous())
    shapes = online_wpe_state_shapes(B, D, F, taps, delay, pc)
    new = OnlineWPEState(*(torch.empty(shape, device=Y.device, dtype=dtype) for shape, dtype in shapes))
    assert L.tssep_wpe_online_state_bytes(B, D, F, taps, delay, pc) == sum(t.numel() * t.element_size() for t in new)
    old = [None] * 5 if state is None else [t.contiguous() for t in state]
    # (an empty tensor has no address: the ring of delay = 0, taps = 1, power_context = 0 holds no frame)
    ptr = lambda t: _p(t) if t is not None and t.numel() else None
    X = torch.empty(B, D, T, F, device=Y.device, dtype=torch.complex128)
    K = taps * D
    nbytes = B * F * (T * D * (y_r.element_size() * 2 + 16) + 32 * (K * (K + 1) // 2 + K * D + shapes.ring[0][2] * D))
    with _timed("wpe_online", B * F * T * 8 * (K * K + K * (K + 1) // 2 + 2 * K * D), nbytes):
        check(L.tssep_wpe_online_fwd(_p(y_r), int(Y.dtype == torch.complex128), *(ptr(t) for t in old),
                                     *(ptr(t) for t in new), _p(torch.view_as_real(X)), B, D, T, F, taps, delay, pc,
                                     float(forgetting), float(load), _stream()), "wpe_online")
    return X, new


# ------------------------------------------------- guided source separation (csrc/gss.hip)
GSS_MAX_CHANNELS, GSS_MAX_SPEAKERS, GSS_MAX_BLOCKS, GSS_CHUNK = 8, 8, 65535, 256
GSS_WEIGHTS = {"bin": 0, "uniform": 1}


def gss_uniform_blocks(T, block=None, context=0):
    """The block table of GSS(block, context): rows (s_fit, e_fit, s_out, e_out), out ranges of `block` frames, each
    fitted with `context` more frames on either side, clipped to [0, T).  block None: the single row (0, T, 0, T)."""
    if int(T) != T or T < 1:
        raise ValueError(f"gss: T = {T!r}: at least one frame")
    T = int(T)
    if block is None:
        if context not in (0, None):
            raise ValueError(f"gss: context={context!r} without block: the whole recording is one fit")
        return np.array([[0, T, 0, T]], dtype=np.int32)
    if int(block) != block or block < 1:
        raise ValueError(f"gss: block={block!r}: a positive number of frames, or None")
    if int(context) != context or context < 0:
        raise ValueError(f"gss: context={context!r}: a number of frames >= 0")
    block, context = int(block), int(context)
    return np.array([[max(0, s - context), min(T, s + block + context), s, min(T, s + block)]
                     for s in range(0, T, block)], dtype=np.int32)


def gss_blocks_check(blocks, T):
    """blocks None | rows (s_fit, e_fit, s_out, e_out) -> int32 [P, 4] numpy, or ValueError: every row has
    0 <= s_fit <= s_out < e_out <= e_fit <= T and the out ranges, in the order given, tile [0, T)."""
    if blocks is None:
        return gss_uniform_blocks(T)
    if isinstance(blocks, torch.Tensor):
        if blocks.is_cuda:
            raise ValueError("gss: the block table is built on the host (a list or an array of rows), it is checked there")
        blocks = blocks.numpy()
    arr = np.asarray(blocks)
    if arr.ndim != 2 or arr.shape[1] != 4 or arr.shape[0] < 1:
        raise ValueError(f"gss: blocks {arr.shape}: rows (s_fit, e_fit, s_out, e_out)")
    if not np.issubdtype(arr.dtype, np.integer):
        if not np.all(np.isfinite(arr)) or not np.all(arr == np.floor(arr)):
            raise ValueError("gss: the block table holds integers")
    if arr.shape[0] > GSS_MAX_BLOCKS:
        raise ValueError(f"gss: {arr.shape[0]} blocks: at most {GSS_MAX_BLOCKS}")
    arr = arr.astype(np.int64)
    at = 0
    for sf, ef, so, eo in arr.tolist():
        if not (0 <= sf <= so < eo <= ef <= T):
            raise ValueError(f"gss: block ({sf}, {ef}, {so}, {eo}) breaks 0 <= s_fit <= s_out < e_out <= e_fit <= {T}")
        if so != at:
            raise ValueError(f"gss: the out ranges must tile [0, {T}): the block ({sf}, {ef}, {so}, {eo}) starts its out "
                             f"range at {so}, the one before ended at {at}")
        at = eo
    if at != T:
        raise ValueError(f"gss: the out ranges must tile [0, {T}): they end at {at}")
    return arr.astype(np.int32)


def guided_cacgmm_check(obs, activity, iterations=20, load=1e-6, weights="bin", blocks=None, out_dtype=torch.float32):
    """What `guided_cacgmm` refuses, from the arguments alone (CPU tensors do: nothing is launched)
    -> (D, K, T, F, block table int32 [P, 4] numpy)."""
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3:
        raise ValueError(f"guided_cacgmm: obs [D,T,F], got "
                         f"{tuple(obs.shape) if isinstance(obs, torch.Tensor) else type(obs)}")
    if obs.dtype != torch.complex128:
        raise TypeError(f"guided_cacgmm: obs is {obs.dtype}, complex128 is required (all arithmetic is float64)")
    if not isinstance(activity, torch.Tensor) or activity.dim() != 2:
        raise ValueError(f"guided_cacgmm: activity [K,T], got "
                         f"{tuple(activity.shape) if isinstance(activity, torch.Tensor) else type(activity)}")
    if activity.is_complex():
        raise TypeError(f"guided_cacgmm: activity is {activity.dtype}: 0 / 1 entries")
    D, T, F = obs.shape
    K, Ta = activity.shape
    if min(T, F) < 1:
        raise ValueError(f"guided_cacgmm: empty axis: obs {tuple(obs.shape)}")
    if Ta != T:
        raise ValueError(f"guided_cacgmm: activity {tuple(activity.shape)} does not match the {T} frames of obs")
    if not 1 <= D <= GSS_MAX_CHANNELS:
        raise ValueError(f"guided_cacgmm: {D} channels: the kernels are built for 1 to {GSS_MAX_CHANNELS}")
    if not 1 <= K <= GSS_MAX_SPEAKERS:
        raise ValueError(f"guided_cacgmm: {K} speakers: the kernels are built for 1 to {GSS_MAX_SPEAKERS} (plus noise)")
    if isinstance(iterations, bool) or int(iterations) != iterations or iterations < 1:
        raise ValueError(f"guided_cacgmm: iterations = {iterations!r}: an integer >= 1")
    if not 0.0 < float(load) < float("inf"):
        raise ValueError(f"guided_cacgmm: load = {load} is not positive and finite (it keeps every B_c positive definite)")
    if weights not in GSS_WEIGHTS:
        raise ValueError(f"guided_cacgmm: weights {weights!r}: 'bin' or 'uniform'")
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"guided_cacgmm: out_dtype {out_dtype}: float32 or float64")
    if not activity.is_cuda and not bool(((activity == 0) | (activity == 1)).all()):
        raise ValueError("guided_cacgmm: the activity holds only 0 and 1 (soft priors are not built)")
    if obs.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("guided_cacgmm is evaluation-time only: obs requires grad and the EM has no backward")
    return D, K, T, F, gss_blocks_check(blocks, T)


_GSS_TABLES = {}        # (device, table bytes) -> int32 [P,4] on the device


def _gss_table(tab, device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device, tab.tobytes())
    hit = _GSS_TABLES.get(key)
    if hit is None:
        if len(_GSS_TABLES) >= 64:
            _GSS_TABLES.pop(next(iter(_GSS_TABLES)))
        hit = _GSS_TABLES[key] = torch.from_numpy(tab).to(device)
    return hit


def gss_fma_per_frame_class(D):
    """fp64 FMAs per (frame, class, iteration): the triangular product L^-1 yh and its squared norm (4 ntri + 2 D) and
    the weighted outer product's lower triangle (6 ntri), ntri = D (D + 1) / 2."""
    ntri = D * (D + 1) // 2
    return 10 * ntri + 2 * D


def guided_cacgmm(obs, activity, iterations=20, load=1e-6, weights="bin", blocks=None, out_dtype=torch.float32):
    """The guided cACGMM of DESIGN 4.24: obs [D,T,F] complex128 and activity [K,T] of 0 / 1 on the device ->
    gamma [K+1,T,F] (class K: noise), the posteriors after `iterations` EM steps with the activities as hard priors.
    blocks: host rows (s_fit, e_fit, s_out, e_out) whose out ranges tile [0, T) (None: one fit over everything).
    2 * iterations + 2 launches whatever the table, T and the content; no host sync (a block table seen before is not
    copied again); float64 arithmetic in a fixed order: two calls give the same bits; out_dtype float32 is the rounding
    of the float64 result.  No default is tuned.  The values of a device activity are not read by the host: anything
    non-zero counts as 1."""
    D, K, T, F, tab = guided_cacgmm_check(obs, activity, iterations, load, weights, blocks, out_dtype)
    assert obs.is_cuda and activity.is_cuda, (obs.device, activity.device)
    L = _lib.lib()
    P = tab.shape[0]
    fit = (tab[:, 1] - tab[:, 0]).astype(np.int64)
    max_fit, sum_fit = int(fit.max()), int(fit.sum())
    ws_bytes = L.tssep_gss_workspace_bytes(P, D, K, T, F, max_fit)
    if ws_bytes <= 0:
        raise RuntimeError(f"guided_cacgmm: unsupported shape obs {(D, T, F)} with {K} speakers and {P} blocks")
    ws = torch.empty(ws_bytes // 8 + 2, device=obs.device, dtype=torch.float64)
    act = (activity.detach() != 0).to(torch.uint8).contiguous()
    obs_r = torch.view_as_real(obs.detach().contiguous())
    out = torch.empty(K + 1, T, F, device=obs.device, dtype=out_dtype)
    C, nent = K + 1, D * (D + 1) // 2 + 1
    chunks = int(((fit + GSS_CHUNK - 1) // GSS_CHUNK).sum())
    flops = 2 * int(iterations) * sum_fit * F * C * gss_fma_per_frame_class(D)
    nbytes = 32 * D * T * F + out.element_size() * C * T * F \
        + (int(iterations) + 1) * 16 * D * sum_fit * F + int(iterations) * 2 * 16 * chunks * F * C * nent
    with _timed("gss_fit", flops, nbytes):
        check(L.tssep_gss_fit(_p(obs_r), _p(act), _p(_gss_table(tab, obs.device)), _p(out),
                              int(out_dtype == torch.float64), _p(ws), P, D, K, T, F, max_fit, int(iterations),
                              float(load), GSS_WEIGHTS[weights], _stream()), "guided_cacgmm")
    return out


def segments_to_activity(table, K, T):
    """The segment table int32 [S,3] of rows (k, s, e) on the device -> activity uint8 [K,T], 1 inside the rows.  A row
    outside speakers [0, K) x frames [0, T] or an empty one is ignored, as segment_mvdr ignores it.  No host read."""
    assert isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.int32, (type(table),)
    assert table.dim() == 2 and table.shape[1] == 3, table.shape
    if int(K) != K or K < 1 or int(T) != T or T < 1:
        raise ValueError(f"segments_to_activity: K = {K!r}, T = {T!r}: both at least 1")
    tab = table.contiguous()
    S = tab.shape[0]
    act = torch.empty(int(K), int(T), device=tab.device, dtype=torch.uint8)
    with _timed("segments_to_activity", 0, 12 * S + int(K) * int(T)):
        check(_lib.lib().tssep_segments_to_activity(_p(tab) if S else None, S, int(K), int(T), _p(act), _stream()),
              "segments_to_activity")
    return act


# ----------------------------------------------------------------------------- losses
def logmae_fwd(est, tgt):
    L = _lib.lib()
    B, K, N = est.shape
    est, tgt = _f32(est).contiguous(), _f32(tgt).contiguous()
    loss = torch.empty(B, device=est.device, dtype=torch.float32)
    sums = torch.empty(B, device=est.device, dtype=torch.float32)
    ws = torch.empty(int(L.tssep_logmae_workspace_bytes(B, K, N)) // 4, device=est.device,
                     dtype=torch.float32)
    check(L.tssep_logmae_fwd(_p(est), _p(tgt), B, K, N, _p(loss), _p(sums), _p(ws), _stream()),
          "logmae_fwd")
    return loss, sums


def logmae_finalize(part, B, K, N):
    L = _lib.lib()
    loss = torch.empty(B, device=part.device, dtype=torch.float32)
    sums = torch.empty(B, device=part.device, dtype=torch.float32)
    check(L.tssep_logmae_finalize(_p(part), B, K, part.shape[-1], N, _p(loss), _p(sums),
                                  _stream()), "logmae_finalize")
    return loss, sums


def logmae_bwd(est, tgt, sums, gout):
    B, K, N = est.shape
    dest = torch.empty_like(est)
    check(_lib.lib().tssep_logmae_bwd(_p(est), _p(tgt), _p(sums), _p(_f32(gout).contiguous()), B,
                                      K, N, _p(dest), _stream()), "logmae_bwd")
    return dest


PIT_MAX_K = 8      # the assignment enumerates K! permutations (8! = 40 320); the C entry points answer TSSEP_E_SHAPE beyond


def _check_pit_k(K):
    if K > PIT_MAX_K:
        raise NotImplementedError(f"pairwise-cost losses (pit=True, MSE) take at most {PIT_MAX_K} speakers, got K = {K}: "
                                  f"the assignment enumerates K! permutations")


def pair_cost_fwd(est, tgt, p=1, diag_only=False):
    """est, tgt [B,K,N] -> chunk partials [B, nchunks, K, K] of sum_n |est[b,i,n] - tgt[b,j,n]|^p in ONE pass over both
    (diag_only: only i == j, the rest 0)."""
    L = _lib.lib()
    B, K, N = est.shape
    _check_pit_k(K)
    est, tgt = _f32(est).contiguous(), _f32(tgt).contiguous()
    part = torch.empty(B, int(L.tssep_pair_cost_chunks(N)), K, K, device=est.device, dtype=torch.float32)
    assert part.numel() * 4 == L.tssep_pair_cost_workspace_bytes(B, K, N)
    with _timed("pair_cost", B * K * (K if not diag_only else 1) * N * 2, 2 * B * K * N * 4):
        check(L.tssep_pair_cost_fwd(_p(est), _p(tgt), B, K, N, int(p), int(bool(diag_only)), _p(part), _stream()),
              "pair_cost_fwd")
    return part


def pit_assign(part, N, pit=True, log=False, want_cost=True):
    """part [B, nchunks, K, K] (a cost matrix [B,K,K]: pass part = cost[:, None], N = 1) ->
    (cost [B,K,K] or None, perm int32 [B,K], sums [B], loss [B]); all on the device, no host sync."""
    B, nchunks, K, K2 = part.shape
    assert K == K2, part.shape
    _check_pit_k(K)
    part = _f32(part).contiguous()
    dev = part.device
    cost = torch.empty(B, K, K, device=dev, dtype=torch.float32) if want_cost else None
    perm = torch.empty(B, K, device=dev, dtype=torch.int32)
    sums = torch.empty(B, device=dev, dtype=torch.float32)
    loss = torch.empty(B, device=dev, dtype=torch.float32)
    check(_lib.lib().tssep_pit_assign(_p(part), B, K, nchunks, int(N), int(bool(pit)), int(bool(log)), _p(cost),
                                      _p(perm), _p(sums), _p(loss), _stream()), "pit_assign")
    return cost, perm, sums, loss


def pair_loss_bwd(est, tgt, perm, sums, gout, p=1):
    """d(loss)/d(est) of a pairwise-cost loss; perm None: identity, sums None: no logarithm.  tgt is read through perm in
    place (never gathered)."""
    B, K, N = est.shape
    _check_pit_k(K)
    est, tgt = _f32(est).contiguous(), _f32(tgt).contiguous()
    if perm is not None:
        assert perm.dtype == torch.int32 and tuple(perm.shape) == (B, K) and perm.is_contiguous(), (perm.dtype, perm.shape)
    dest = torch.empty_like(est)
    check(_lib.lib().tssep_pair_loss_bwd(_p(est), _p(tgt), _p(perm), _p(sums), _p(_f32(gout).contiguous()), B, K, N,
                                         int(p), _p(dest), _stream()), "pair_loss_bwd")
    return dest


# SDR / SI-SDR (sdrloss.hip): statistics as float64 chunk partials -> value / cost -> pit_assign -> backward
def sdr_tau(sdr_max):
    """The soft threshold tau = 10^(-sdr_max / 10) (0: none)."""
    return 0.0 if sdr_max is None else 10.0 ** (-float(sdr_max) / 10.0)


def _sdr_nstat(K):
    return K * K + 2 * K


def sdr_stats_fwd(est, tgt, diag_only=False):
    """est, tgt [B,K,N] -> float64 chunk partials [B, nchunks, K*K + 2K] of c_ij = sum e_i t_j, a_i = sum e_i^2,
    b_j = sum t_j^2 in ONE pass over both (diag_only: only c_ii, the other c entries 0)."""
    L = _lib.lib()
    B, K, N = est.shape
    _check_pit_k(K)
    assert tuple(tgt.shape) == (B, K, N), (tuple(tgt.shape), (B, K, N))
    est, tgt = _f32(est).contiguous(), _f32(tgt).contiguous()
    part = torch.empty(B, int(L.tssep_sdr_chunks(N)), _sdr_nstat(K), device=est.device, dtype=torch.float64)
    assert 0 < part.numel() * 8 == L.tssep_sdr_workspace_bytes(B, K, N)
    with _timed("sdr_stats", B * N * 2 * ((K if diag_only else K * K) + 2 * K), 2 * B * K * N * 4):
        check(L.tssep_sdr_stats_fwd(_p(est), _p(tgt), B, K, N, int(bool(diag_only)), _p(part), _stream()),
              "sdr_stats_fwd")
    return part


def sdr_cost(part, K, scale_invariant=True, sdr_max=None, eps=1e-8, diag_only=False):
    """part [B, nchunks, K*K + 2K] float64 -> (stat float64 [B, K*K + 2K], value dB [B,K,K], cost = -value / K [B,K,K]);
    cost[:, None] is what pit_assign takes with N = 1."""
    B, nchunks, ns = part.shape
    _check_pit_k(K)
    assert ns == _sdr_nstat(K) and part.dtype == torch.float64 and part.is_cuda, (part.shape, part.dtype, K)
    part = part.contiguous()
    stat = torch.empty(B, ns, device=part.device, dtype=torch.float64)
    value = torch.empty(B, K, K, device=part.device, dtype=torch.float32)
    cost = torch.empty_like(value)
    with _timed("sdr_cost", 0, part.numel() * 8 + stat.numel() * 8 + 2 * value.numel() * 4):
        check(_lib.lib().tssep_sdr_cost(_p(part), B, K, nchunks, int(bool(scale_invariant)), sdr_tau(sdr_max), float(eps),
                                        int(bool(diag_only)), _p(stat), _p(value), _p(cost), _stream()), "sdr_cost")
    return stat, value, cost


def sdr_bwd(est, tgt, perm, stat, gout, scale_invariant=True, sdr_max=None, eps=1e-8):
    """d(loss)/d(est) = gout[b] (P e_i + Q tgt[b, perm[b,i]]) with P, Q from stat (sdr_cost's); perm None: identity.
    tgt is read through perm in place."""
    B, K, N = est.shape
    _check_pit_k(K)
    est, tgt = _f32(est).contiguous(), _f32(tgt).contiguous()
    assert tuple(stat.shape) == (B, _sdr_nstat(K)) and stat.dtype == torch.float64 and stat.is_contiguous(), \
        (stat.shape, stat.dtype)
    gout = _f32(gout).contiguous()
    assert gout.numel() == B, (gout.shape, B)
    dest = torch.empty_like(est)
    with _timed("sdr_bwd", 3 * B * K * N, 3 * B * K * N * 4):
        check(_lib.lib().tssep_sdr_bwd(_p(est), _p(tgt), _p(_spec_perm(perm, B, K)), _p(stat), _p(gout), B, K, N,
                                       int(bool(scale_invariant)), sdr_tau(sdr_max), float(eps), _p(dest), _stream()),
              "sdr_bwd")
    return dest


def sdr_forward(est, tgt, scale_invariant=True, sdr_max=None, eps=1e-8, pit=False):
    """The three forward launches -> (loss [B], perm int32 [B,K], values dB [B,K] of the matched pairs, stat)."""
    K = est.shape[-2]
    part = sdr_stats_fwd(est, tgt, diag_only=not pit)
    stat, value, cost = sdr_cost(part, K, scale_invariant, sdr_max, eps, diag_only=not pit)
    _, perm, _, loss = pit_assign(cost[:, None], 1, pit=pit, log=False, want_cost=False)
    values = torch.gather(value, 2, perm.long()[..., None])[..., 0]
    return loss, perm, values, stat


def sdr(est, tgt, scale_invariant=True, sdr_max=None, eps=1e-8, pit=False):
    """The metric: est, tgt [B,K,N] -> (values dB [B,K], values[b, i] = estimate row i against target row perm[b, i];
    perm int32 [B,K], the best assignment with pit, else the identity).  No gradient, no host sync."""
    with torch.no_grad():
        _, perm, values, _ = sdr_forward(est, tgt, scale_invariant, sdr_max, eps, pit)
    return values, perm


# FreqMSE (specloss.hip): cost[b,i,j] = sum_t mean_f |E_i - S_j|^2 as chunk partials over T; pit_assign(part, N=F) finishes
def _spec_target(tgt, shape):
    assert tgt.is_cuda and tgt.dtype == torch.complex64 and tuple(tgt.shape) == tuple(shape), \
        (tgt.device, tgt.dtype, tuple(tgt.shape), tuple(shape))
    return torch.view_as_real(tgt.contiguous())


def _spec_part(B, K, T, F, device):
    L = _lib.lib()
    part = torch.empty(B, int(L.tssep_specmse_chunks(T)), K, K, device=device, dtype=torch.float32)
    assert 0 < part.numel() * 4 <= L.tssep_specmse_workspace_bytes(B, K, T, F)
    return part


def _spec_perm(perm, B, K):
    if perm is not None:
        assert perm.dtype == torch.int32 and tuple(perm.shape) == (B, K) and perm.is_contiguous(), (perm.dtype, perm.shape)
    return perm


def mask_specmse_fwd(logit, obs, tgt, diag_only=False):
    """logit [B,K,T,F] fp32, obs [B,T,F] complex64, tgt [B,K,T,F] complex64 -> chunk partials [B, nchunks, K, K] of
    sum_{t,f} |sigmoid(logit_i) obs - tgt_j|^2 in one pass over the three (diag_only: only i == j, the rest 0); neither
    the mask nor the estimate is written."""
    B, K, T, F = logit.shape
    _check_pit_k(K)
    assert tuple(obs.shape) == (B, T, F) and obs.dtype == torch.complex64, (tuple(obs.shape), obs.dtype, (B, T, F))
    logit, obs_r, tgt_r = _f32(logit).contiguous(), torch.view_as_real(obs.contiguous()), _spec_target(tgt, logit.shape)
    part = _spec_part(B, K, T, F, logit.device)
    with _timed("mask_specmse_fwd", 0, B * T * F * (12 * K + 8)):
        check(_lib.lib().tssep_mask_specmse_fwd(_p(logit), _p(obs_r), _p(tgt_r), B, K, T, F, int(bool(diag_only)),
                                                _p(part), _stream()), "mask_specmse_fwd")
    return part


def mask_specmse_bwd(logit, obs, tgt, perm, gout, iperm=None, bt_major=False):
    """-> d(loss)/d(logit) = gout[b] (2/F) Re(conj(m Y - t) Y) m (1 - m), t = tgt[b, perm[b,k]] read in place (perm None:
    identity).  bt_major: laid out [B*T, K*F] with speaker k at position iperm[b, k] -- what the final Linear's backward
    reads (as mask_istft_bwd)."""
    B, K, T, F = logit.shape
    _check_pit_k(K)
    assert tuple(obs.shape) == (B, T, F) and obs.dtype == torch.complex64, (tuple(obs.shape), obs.dtype, (B, T, F))
    logit, obs_r, tgt_r = _f32(logit).contiguous(), torch.view_as_real(obs.contiguous()), _spec_target(tgt, logit.shape)
    gout = _f32(gout).contiguous()
    assert gout.numel() == B, (gout.shape, B)
    dlogit = torch.empty(B * T, K * F, device=logit.device, dtype=torch.float32) if bt_major else torch.empty_like(logit)
    with _timed("mask_specmse_bwd", 0, B * T * F * (16 * K + 8)):
        check(_lib.lib().tssep_mask_specmse_bwd(_p(logit), _p(obs_r), _p(tgt_r), _p(_spec_perm(perm, B, K)), _p(gout),
                                                B, K, T, F, _p(iperm), int(bool(bt_major)), _p(dlogit), _stream()),
              "mask_specmse_bwd")
    return dlogit


def _spec_est(est):
    assert est.is_cuda and est.dtype in (torch.complex64, torch.complex128) and est.dim() == 4, (est.device, est.dtype, est.shape)
    return torch.view_as_real(est.contiguous()), int(est.dtype == torch.complex128)


def specmse_fwd(est, tgt, diag_only=False):
    """est [B,K,T,F] complex64 | complex128, tgt [B,K,T,F] complex64 -> chunk partials [B, nchunks, K, K]"""
    B, K, T, F = est.shape
    _check_pit_k(K)
    est_r, f64 = _spec_est(est)
    tgt_r = _spec_target(tgt, est.shape)
    part = _spec_part(B, K, T, F, est.device)
    with _timed("specmse_fwd", 0, B * K * T * F * (16 + 8 * f64)):
        check(_lib.lib().tssep_specmse_fwd(_p(est_r), f64, _p(tgt_r), B, K, T, F, int(bool(diag_only)), _p(part),
                                           _stream()), "specmse_fwd")
    return part


def specmse_bwd(est, tgt, perm, gout):
    """-> d(loss)/d(est) = gout[b] (2/F) (est - tgt[b, perm[b,k]]) in est's dtype (perm None: identity)"""
    B, K, T, F = est.shape
    _check_pit_k(K)
    est_r, f64 = _spec_est(est)
    tgt_r = _spec_target(tgt, est.shape)
    gout = _f32(gout).contiguous()
    assert gout.numel() == B, (gout.shape, B)
    dest = torch.empty_like(est_r)
    check(_lib.lib().tssep_specmse_bwd(_p(est_r), f64, _p(tgt_r), _p(_spec_perm(perm, B, K)), _p(gout), B, K, T, F,
                                       _p(dest), _stream()), "specmse_bwd")
    return torch.view_as_complex(dest)


def vadbce_fwd(logit, vad):
    L = _lib.lib()
    B, K, T, F = logit.shape
    logit, vad = _f32(logit).contiguous(), _f32(vad).contiguous()
    loss = torch.empty(B, device=logit.device, dtype=torch.float32)
    xmean = torch.empty(B, K, T, device=logit.device, dtype=torch.float32)
    ws = torch.empty(B * K * T, device=logit.device, dtype=torch.float32)
    check(L.tssep_vadbce_fwd(_p(logit), _p(vad), B, K, T, F, _p(loss), _p(xmean), _p(ws),
                             _stream()), "vadbce_fwd")
    return loss, xmean


def vadbce_bwd(xmean, vad, gout, F):
    B, K, T = xmean.shape
    dlogit = torch.empty(B, K, T, F, device=xmean.device, dtype=torch.float32)
    check(_lib.lib().tssep_vadbce_bwd(_p(xmean), _p(_f32(vad).contiguous()),
                                      _p(_f32(gout).contiguous()), B, K, T, F, _p(dlogit),
                                      _stream()), "vadbce_bwd")
    return dlogit


def logit_map_fwd(raw, perm, iperm, B, trials, K, T, F, Fr, spk_rows):
    out = torch.empty(B, K, T, F, device=raw.device, dtype=torch.float32)
    check(_lib.lib().tssep_logit_map_fwd(_p(raw), _p(perm), _p(iperm), B, trials, K, T, F, Fr,
                                         int(spk_rows), _p(out), _stream()), "logit_map_fwd")
    return out


def logit_map_bwd(dout, perm, iperm, B, trials, K, T, F, Fr, spk_rows):
    n = B * trials * K * T * Fr
    draw = torch.empty(n, device=dout.device, dtype=torch.float32)
    check(_lib.lib().tssep_logit_map_bwd(_p(_f32(dout).contiguous()), _p(perm), _p(iperm), B,
                                         trials, K, T, F, Fr, int(spk_rows), _p(draw), _stream()),
          "logit_map_bwd")
    return draw


def mask_map_fwd(raw, perm, iperm, B, trials, K, M, T, F, Fr, spk_rows):
    """The fused two-mask tail: raw GEMM output -> (logit, mask), both [B,K,M,T,F] fp32, in one launch (the logit map
    with M masks per speaker + the mask head's sigmoid; include/tssep_hip.h)."""
    logit = torch.empty(B, K, M, T, F, device=raw.device, dtype=torch.float32)
    mask = torch.empty_like(logit)
    n = B * K * M * T
    if TAIL_LOG is not None:
        TAIL_LOG.append(dict(kernel="mask_map_fwd", B=B, K=K, M=M, T=T, F=F, Fr=Fr, trials=trials, spk_rows=int(spk_rows)))
    with _timed("mask_map_fwd", 0, 4 * n * (trials * Fr + 2 * F)):
        check(_lib.lib().tssep_mask_map_fwd(_p(_f32(raw)), _p(perm), _p(iperm), B, trials, K, M, T, F, Fr, int(spk_rows),
                                            _p(logit), _p(mask), _stream()), "mask_map_fwd")
    return logit, mask


def mask_map_bwd(dmask, mask, dlogit, perm, iperm, B, trials, K, M, T, F, Fr, spk_rows):
    """dmask, the saved mask and (or None) dlogit, all [B,K,M,T,F] -> draw in the raw layout [B*trials*K*M*T*Fr], one
    launch: (dmask s (1 - s) [+ dlogit]) [/ trials], summed over f for Fr == 1."""
    assert tuple(mask.shape) == (B, K, M, T, F) and mask.is_contiguous(), (tuple(mask.shape), (B, K, M, T, F))
    assert tuple(dmask.shape) == tuple(mask.shape), (tuple(dmask.shape), tuple(mask.shape))
    assert dlogit is None or tuple(dlogit.shape) == tuple(mask.shape), tuple(dlogit.shape)
    n = B * K * M * T
    draw = torch.empty(n * trials * Fr, device=mask.device, dtype=torch.float32)
    if TAIL_LOG is not None:
        TAIL_LOG.append(dict(kernel="mask_map_bwd", B=B, K=K, M=M, T=T, F=F, Fr=Fr, trials=trials, spk_rows=int(spk_rows),
                             dlogit=dlogit is not None))
    with _timed("mask_map_bwd", 0, 4 * n * ((2 if dlogit is None else 3) * F + trials * Fr)):
        check(_lib.lib().tssep_mask_map_bwd(_p(_f32(dmask).contiguous()), _p(_f32(mask)),
                                            _p(_f32(dlogit).contiguous()) if dlogit is not None else None,
                                            _p(perm), _p(iperm), B, trials, K, M, T, F, Fr, int(spk_rows), _p(draw),
                                            _stream()), "mask_map_bwd")
    return draw


def gatebce_fwd(logit, vad):
    """SignalAndVADSigmoidBCE's BCE on the gate column of logit [B,K,T,F+1] against vad [B,K,T] -> loss [B]"""
    B, K, T, F1 = logit.shape
    assert tuple(vad.shape) == (B, K, T), (tuple(vad.shape), (B, K, T))
    logit, vad = _f32(logit).contiguous(), _f32(vad).contiguous()
    loss = torch.empty(B, device=logit.device, dtype=torch.float32)
    ws = torch.empty(B * K * T, device=logit.device, dtype=torch.float32)
    check(_lib.lib().tssep_gatebce_fwd(_p(logit), F1, _p(vad), B, K, T, _p(loss), _p(ws), _stream()), "gatebce_fwd")
    return loss


def gatebce_bwd(logit, vad, gout):
    """-> dlogit [B,K,T,F+1]: the BCE gradient at column 0, zeros elsewhere"""
    B, K, T, F1 = logit.shape
    assert tuple(vad.shape) == (B, K, T) and gout.numel() == B, (tuple(vad.shape), (B, K, T), gout.numel())
    logit = _f32(logit).contiguous()
    dlogit = torch.empty_like(logit)
    check(_lib.lib().tssep_gatebce_bwd(_p(logit), F1, _p(_f32(vad).contiguous()), _p(_f32(gout).contiguous()),
                                       B, K, T, _p(dlogit), _stream()), "gatebce_bwd")
    return dlogit
