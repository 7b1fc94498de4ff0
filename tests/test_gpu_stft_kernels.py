"""The STFT kernels (stft.hip: the 1024 / 256 plan and the fused mask -> iSTFT tail; stft_generic.hip: every other plan) at
training sizes and past their grid caps, against float64 restatements of the same operations computed on the device.

Caps and boundaries, and the cases that cross them:

    rfft_generic_kernel       16 384 blocks x 4 waves = 65 536 frames per sweep, one wave per frame: 400 / 200 at
                              768 x 64 000 (246 528 frames, 3.8 sweeps), 512 / 128 at 330 rows (165 990, ragged last sweep),
                              960 / 240 at 620 rows (167 400; 480 = 4 4 2 3 5, an odd number of Stockham stages, radices
                              3 and 5), 4096 / 512 at 1 320 rows (174 240), 400 / 200 without fading (pad_left = 0)
    istft_generic_kernel      65 536 output hops per sweep: the same cases (400 / 200: 245 760 hops)
    4096 / 512                147 456 bytes of LDS, above the 64 KB default: the hipFuncSetAttribute opt-in; the plan must
                              be advertised (tssep_stft_plan == 2)
    rfft_frames_kernel        no cap; 768 rows (training), 2 100 rows (the spectrum exceeds 2^31 bytes), N = 480 000,
                              odd N = 64 001 (the clamped 4-byte load path)
    istft_kernel              grid (chunks, rows): N = 480 000 has 1 875 hops in 30 chunks of 63, the last one 48 (short)
    fused mask tail           cfg3 B = 768, K = 4 (3 072 rows); B = 1 100, K = 4 (logit 2.28 GB > 2^31 bytes);
                              cfg5 B = 4, K = 8, N = 480 000 -- per-utterance observation rows and loss coefficients,
                              per-chunk |y - tgt| partials, the bt_major layout with a non-identity iperm
    inverse row limit         grid.y <= 65 535 rows: 65 535 rows compute, 65 536 raise

References: frames by unfold, the float64 windows of oracle/stft.py, torch.fft in float64, overlap-add by fold, row chunk
by row chunk; each is anchored against oracle/stft.py in float64 on the CPU (test_device_references_match_the_oracle).
Every row is scaled by 10^u, u uniform in [-3, 3], and every output is pre-filled with NaN (the C ABI is called directly):
a row read as zeros, a dropped frame or an unwritten element fails.

Tolerances (U = 2^-24), per frame or per output sample, never per tensor:
  * a size-point FFT in fp32 has ||X^ - X||_2 <= L eta ||X||_2 with L binary levels and eta ~ mu + gamma_4 (sqrt 2 + mu)
    ~ 6.7 U per level for twiddles rounded to fp32 (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2);
    with eta = C U, C = 8, and L = ceil(log2 size) + 2 (the size / 2-point transform, the real split pass, the window
    product and the rounded window or scale).  Each element's error is at most the frame's error norm, so a forward bin
    gets C L U ||X_t||_2, with ||X_t||_2 = sqrt(size) ||window * frame||_2 (Parseval, the full spectrum).  The adjoint of
    the inverse is the same transform scaled by 2 / size.
  * inverse: output sample n sums the <= ceil(size / shift) frames that cover it; each contributes |wsyn[j]| (C L U
    ||x_t||_2 + (ceil(size / shift) + 2) U |x_t[j]|), x_t = irfft(X_t) (the transform, then the window product, the
    1 / NH scale and the overlap-add roundings), summed by the same overlap-add as the reference itself.
  * fused tail: the mask is the hardware exp2 / rcp sigmoid, |m^ - m| <= U m (8 + 2 |logit|) (as in
    test_gpu_streaming_kernels.py); its relative error, maximised over a frame's bins, adds to that frame's C L U.  The
    backward d(logit) = Re(conj(obs) d) m (1 - m) adds |obs| tol(d) m (1 - m), 3 U of the dot product's terms, and
    |Re(conj(obs) d)| (|m^ - m| + 3 U m (1 - m)) for the rounded m (1 - m) and the two products.
  * per-chunk sums of |y - tgt|, against the float64 sums of the kernel's own samples (themselves checked above) over
    the kernel's chunk bounds: (hops per chunk + 16) U sum |y - tgt| (the rounded differences, each thread's running
    sum of one sample per hop, then the wave and workgroup reductions).
The worst err / tol of every check is printed (pytest -rP)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import stft as ostft  # noqa: E402

U = 2.0 ** -24
GIB = 1 << 30
DEV = "cuda"
NAN = float("nan")
FFT_C = 8

GEN_SWEEP = 16384 * 4            # stft_generic.hip: frames (forward) or output hops (inverse) per sweep of the capped grid
ROW_LIMIT = 65535                # stft.hip istft_kernel: rows on grid.y
HCB_MAX = 64                     # stft.hip: hops per chunk of the 1024 / 256 inverse, at most
ELEMS = 1 << 25                  # float64 elements per frame tensor of a reference chunk (256 MB)

# (size, shift, rows, N, fading)
GENERIC_CASES = [
    (400, 200, 768, 64000, True),
    (512, 128, 330, 64000, True),
    (960, 240, 620, 64000, True),
    (4096, 512, 1320, 64000, True),
    (400, 200, 768, 64000, False),
]
# (rows, N) of the 1024 / 256 plan
PLAN1_CASES = [(768, 64000), (2100, 64000), (8, 480000), (300, 64001)]
# (B, K, N) of the fused tail
FUSED_CASES = [(768, 4, 64000), (1100, 4, 64000), (4, 8, 480000)]


def H():
    from tssep_amd import hip_ops
    return hip_ops


def L():
    from tssep_amd import _lib
    return _lib.lib()


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def row_scale(rows, g):
    """10^u per row, u uniform in [-3, 3]."""
    return 10.0 ** (torch.rand(rows, device=DEV, generator=g) * 6 - 3)


def levels(size):
    return math.ceil(math.log2(size)) + 2


def fft_rel(size):
    return FFT_C * levels(size) * U


def within(got, ref, tol, name):
    """|got - ref| <= tol element-wise; ref and tol float64.  NaN or Inf in `got` fails.  -> max err / tol."""
    if got.is_complex():
        got = torch.view_as_real(got)
    if ref.is_complex():
        ref = torch.view_as_real(ref)
    err = (got.double() - ref).abs()
    tol = torch.broadcast_to(tol, err.shape)
    ok = err <= tol
    if not bool(ok.all()):
        bad = ~ok
        i = int(bad.reshape(-1).nonzero()[0])
        idx = np.unravel_index(i, err.shape)
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the tolerance; first at {idx}: "
                             f"got {float(got[idx]):.9g}, want {float(ref[idx]):.9g}, tol {float(tol[idx]):.3g}")
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())


class Ratios:
    """The worst err / tol of each named check."""

    def __init__(self):
        self.r = {}

    def add(self, name, v):
        self.r[name] = max(self.r.get(name, 0.0), v)

    def report(self, case):
        for k, v in self.r.items():
            print(f"max err/tol  {case}  {k}: {v:.3g}")


@pytest.fixture(autouse=True)
def _device_memory_cap():
    """The GPU is shared: every test here stays under 16 GB of device memory at its peak."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 * GIB, f"peak device memory {peak / GIB:.1f} GiB"


def frames_of(N, size, shift, fading):
    return ostft.num_frames(N, size, shift, fading=fading)


def generic_hops(N, size, shift, fading):
    pad = size - shift if fading else 0
    return (pad + N + shift - 1) // shift - pad // shift


def radices(size):
    """stft_generic.hip make_plan: the Stockham stages of the size / 2-point transform."""
    rest, out = size // 2, []
    for r in (4, 2, 3, 5):
        while rest % r == 0 and rest > 1:
            out.append(r)
            rest //= r
    assert rest == 1
    return out


def plan1_chunks(N):
    hops = -(-N // 256)
    nch = -(-hops // HCB_MAX)
    return nch, -(-hops // nch)


def test_the_cases_run_past_the_grid_caps():
    """Each cap and boundary of the module docstring is crossed by a case of this file."""
    for size, shift, rows, N, fading in GENERIC_CASES:
        T = frames_of(N, size, shift, fading)
        assert rows * T >= 2.5 * GEN_SWEEP and rows * generic_hops(N, size, shift, fading) >= 2.5 * GEN_SWEEP
    assert any((rows * frames_of(N, s, sh, f)) % GEN_SWEEP for s, sh, rows, N, f in GENERIC_CASES)   # ragged last sweep
    assert frames_of(64000, 400, 200, True) * 768 == 246528 and generic_hops(64000, 400, 200, True) * 768 == 245760
    stages = [radices(s) for s, *_ in GENERIC_CASES]
    assert any(len(r) % 2 for r in stages) and any(len(r) % 2 == 0 for r in stages)
    assert any(3 in r for r in stages) and any(5 in r for r in stages)
    assert (2048 + 8 * 2048) * 8 == 147456 > 64 * 1024 and any(s == 4096 for s, *_ in GENERIC_CASES)
    assert any(not f for *_, f in GENERIC_CASES)
    assert any(rows == 768 for rows, _ in PLAN1_CASES)
    assert any(rows * frames_of(N, 1024, 256, True) * 513 * 8 > 2 ** 31 for rows, N in PLAN1_CASES)
    assert any(N % 2 for _, N in PLAN1_CASES)
    assert plan1_chunks(480000) == (30, 63) and 1875 - 29 * 63 == 48
    assert any(N == 480000 for _, N in PLAN1_CASES) and any(N == 480000 for *_, N in FUSED_CASES)
    assert any(B * K >= 3072 for B, K, _ in FUSED_CASES)
    assert any(B * K * frames_of(N, 1024, 256, True) * 513 * 4 > 2 ** 31 for B, K, N in FUSED_CASES)


# --------------------------------------------------------------------------------------------------------- references
def windows64(size, shift):
    wa = torch.as_tensor(ostft.analysis_window("hann", size), dtype=torch.float64)
    ws = torch.as_tensor(ostft.synthesis_window("hann", size, shift), dtype=torch.float64)
    return wa, ws


def windows32(size, shift):
    wa, ws = windows64(size, shift)
    return wa.float().to(DEV), ws.float().to(DEV)


def ref_rfft(x64, w64, size, shift, pad_left, T, adjoint=False):
    """x [r, N] float64 -> (X [r, T, size/2+1] complex128, fro [r, T]): the spectra of the windowed frames (pad_left zeros
    in front, zeros behind) and the 2-norm of each frame's full size-point spectrum.  adjoint: the adjoint of the inverse
    STFT (interior bins x 2 / size, DC and Nyquist x 1 / size; fro x 2 / size)."""
    N = x64.shape[-1]
    need = (T - 1) * shift + size
    xp = torch.nn.functional.pad(x64, (pad_left, max(0, need - pad_left - N)))[..., :need]
    seg = xp.unfold(-1, size, shift) * w64
    fro = seg.norm(dim=-1) * math.sqrt(size)
    X = torch.fft.rfft(seg, dim=-1)
    del seg
    if adjoint:
        X *= 2.0 / size
        X[..., 0] *= 0.5
        X[..., -1] *= 0.5
        fro = fro * (2.0 / size)
    return X, fro


def _ola(seg, shift):
    r, T, size = seg.shape
    length = (T - 1) * shift + size
    return torch.nn.functional.fold(seg.transpose(1, 2), output_size=(1, length), kernel_size=(1, size),
                                    stride=(1, shift)).reshape(r, length)


def ref_istft(X, ws64, size, shift, pad_left, N, rel=None):
    """X [r, T, F] complex128 -> (y [r, N], tol [r, N]): irfft (imaginary parts of DC and Nyquist ignored), synthesis
    window, overlap-add, samples [pad_left, pad_left + N).  rel [r, T]: an extra relative error of each frame's spectrum."""
    X = X.clone()
    X[..., 0] = X[..., 0].real.to(X.dtype)
    X[..., -1] = X[..., -1].real.to(X.dtype)
    seg = torch.fft.irfft(X, n=size, dim=-1)
    del X
    b = fft_rel(size) * seg.norm(dim=-1, keepdim=True)
    if rel is not None:
        b = b + rel[..., None] * seg.norm(dim=-1, keepdim=True)
    c = -(-size // shift)
    tol = _ola(ws64.abs() * (b + (c + 2) * U * seg.abs()), shift)[..., pad_left:pad_left + N]
    y = _ola(seg * ws64, shift)[..., pad_left:pad_left + N]
    return y, tol


def _row_chunk(T, size):
    return max(1, ELEMS // (T * size))


def check_rfft(got, x, w64, size, shift, pad_left, name, ratios, adjoint=False, rel=0.0):
    """got [rows, T, F] complex64 from x [rows, N] fp32: per-frame tolerance."""
    rows, T = got.shape[:2]
    w64 = w64.to(DEV)
    per = _row_chunk(T, size)
    for lo in range(0, rows, per):
        hi = min(rows, lo + per)
        X, fro = ref_rfft(x[lo:hi].double(), w64, size, shift, pad_left, T, adjoint)
        ratios.add(name, within(got[lo:hi], X, ((fft_rel(size) + rel) * fro)[..., None, None], name))


def check_istft(got, X, ws64, size, shift, pad_left, name, ratios, tgt=None, part=None, hcb=None):
    """got [rows, N] from X [rows, T, F] complex64: per-sample tolerance; with tgt, the per-chunk partial sums too."""
    rows, N = got.shape
    T = X.shape[1]
    ws64 = ws64.to(DEV)
    per = _row_chunk(T, size)
    for lo in range(0, rows, per):
        hi = min(rows, lo + per)
        y, tol = ref_istft(X[lo:hi].to(torch.complex128), ws64, size, shift, pad_left, N)
        ratios.add(name, within(got[lo:hi], y, tol, name))
        if part is not None:
            check_partials(part[lo:hi], got[lo:hi], tgt[lo:hi], hcb, name + " |y - tgt| partials", ratios)


def check_partials(part, y, tgt, hcb, name, ratios):
    """part [r, chunks] against sum |y - tgt| over samples [c hcb 256, (c + 1) hcb 256) of the kernel's y."""
    N = y.shape[-1]
    nch = part.shape[-1]
    span = hcb * 256
    assert (nch - 1) * span < N <= nch * span
    a = torch.nn.functional.pad((y.double() - tgt.double()).abs(), (0, nch * span - N)).view(-1, nch, span).sum(-1)
    ratios.add(name, within(part, a, (hcb + 16) * U * a, name))


def test_device_references_match_the_oracle():
    """The device references above against oracle/stft.py (pinned to the upstream doctest numbers) in float64 on the
    CPU, for every plan of this file: forward, inverse and the adjoint of the inverse (autograd of the oracle)."""
    g = torch.Generator().manual_seed(3)
    plans = [(1024, 256, True)] + [(s, sh, f) for s, sh, _, _, f in GENERIC_CASES]
    for size, shift, fading in plans:
        N = 9001
        pad = size - shift if fading else 0
        T = frames_of(N, size, shift, fading)
        assert T == H().stft_frames(N, size, shift, None, True, fading)
        wa, ws = windows64(size, shift)
        x = torch.randn(3, N, generator=g, dtype=torch.float64)
        X, _ = ref_rfft(x.to(DEV), wa.to(DEV), size, shift, pad, T)
        Xo = ostft.stft(x, size=size, shift=shift, window="hann", fading=fading)
        assert X.shape == Xo.shape
        assert float((X.cpu() - Xo).abs().max()) <= 1e-12 * float(Xo.abs().max()), (size, shift, fading, "stft")
        Y = torch.randn(3, T, size // 2 + 1, generator=g, dtype=torch.complex128)
        y, _ = ref_istft(Y.to(DEV), ws.to(DEV), size, shift, pad, N)
        Yg = Y.clone().requires_grad_()
        yo = ostft.istft(Yg, size=size, shift=shift, window="hann", fading=fading, num_samples=N)
        dy = torch.randn(3, N, generator=g, dtype=torch.float64)
        (yo * dy).sum().backward()
        yo = yo.detach()
        assert y.shape == yo.shape
        assert float((y.cpu() - yo).abs().max()) <= 1e-12 * float(yo.abs().max()), (size, shift, fading, "istft")
        dX, _ = ref_rfft(dy.to(DEV), ws.to(DEV), size, shift, pad, T, adjoint=True)
        gr = Yg.grad
        assert float((dX.cpu() - gr).abs().max()) <= 1e-12 * float(gr.abs().max()), (size, shift, fading, "adjoint")


# ------------------------------------------------------------------------------------------------- C ABI, NaN outputs
def _p(t):
    return H()._p(t)


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def abi_rfft(x, window, size, shift, fading, T, adjoint=False):
    """tssep_stft_fwd (or tssep_istft_bwd) into a NaN-filled [rows, T, F] complex64."""
    rows, N = x.shape
    X = torch.full((rows, T, size // 2 + 1, 2), NAN, device=DEV)
    fn = L().tssep_istft_bwd if adjoint else L().tssep_stft_fwd
    _ok(fn(_p(x), rows, N, size, shift, int(fading), _p(window), _p(H().fft_tables(size, DEV)), _p(X), T,
           H()._stream()), "istft_bwd" if adjoint else "stft_fwd")
    return torch.view_as_complex(X)


def abi_istft(X, wsyn, N, size, shift, fading, tgt=None):
    rows, T = X.shape[:2]
    y = torch.full((rows, N), NAN, device=DEV)
    part = torch.full((rows, int(L().tssep_istft_chunks(N))), NAN, device=DEV) if tgt is not None else None
    _ok(L().tssep_istft_fwd(_p(torch.view_as_real(X)), rows, T, size, shift, int(fading), _p(wsyn),
                            _p(H().fft_tables(size, DEV)), _p(y), N, _p(tgt), _p(part), H()._stream()), "istft_fwd")
    return y, part


def abi_mask_istft(logit, obs, wsyn, N, tgt=None):
    B, K, T, F = logit.shape
    y = torch.full((B * K, N), NAN, device=DEV)
    part = torch.full((B * K, int(L().tssep_istft_chunks(N))), NAN, device=DEV) if tgt is not None else None
    _ok(L().tssep_mask_istft_fwd(_p(logit), _p(torch.view_as_real(obs)), B, K, T, 1024, 256, 1, _p(wsyn),
                                 _p(H().fft_tables(1024, DEV)), _p(y), N, _p(tgt), _p(part), H()._stream()),
        "mask_istft_fwd")
    return y, part


def abi_mask_istft_bwd(dy, logit, obs, wsyn):
    B, K, T, F = logit.shape
    dl = torch.full((B, K, T, F), NAN, device=DEV)
    _ok(L().tssep_mask_istft_bwd(_p(dy), _p(logit), _p(torch.view_as_real(obs)), B, K, dy.shape[-1], 1024, 256, 1,
                                 _p(wsyn), _p(H().fft_tables(1024, DEV)), _p(dl), T, H()._stream()), "mask_istft_bwd")
    return dl


def abi_mask_istft_bwd_loss(est, tgt, sums, gout, logit, obs, wsyn, iperm, bt_major):
    B, K, T, F = logit.shape
    dl = torch.full((B * T, K * F) if bt_major else (B, K, T, F), NAN, device=DEV)
    _ok(L().tssep_mask_istft_bwd_loss(_p(est), _p(tgt), _p(sums), _p(gout), _p(logit), _p(torch.view_as_real(obs)),
                                      B, K, est.shape[-1], 1024, 256, 1, _p(wsyn), _p(H().fft_tables(1024, DEV)),
                                      _p(iperm), int(bt_major), _p(dl), T, H()._stream()), "mask_istft_bwd_loss")
    return dl


# ------------------------------------------------------------------------------------------------------- general plan
@pytest.mark.parametrize("size,shift,rows,N,fading", GENERIC_CASES)
def test_generic_plan_past_the_cap(size, shift, rows, N, fading):
    """stft_generic.hip: tssep_stft_fwd, tssep_istft_bwd (adjoint: s_in / s_edge) and tssep_istft_fwd past 2.5 sweeps
    of the capped grid -- every wave handles several frames or hops, reusing its LDS lines."""
    assert L().tssep_stft_plan(size, shift) == 2
    g = gen(size + shift + int(fading))
    pad = size - shift if fading else 0
    T = frames_of(N, size, shift, fading)
    wa64, ws64 = windows64(size, shift)
    wa, ws = windows32(size, shift)
    r = Ratios()
    x = torch.randn(rows, N, device=DEV, generator=g) * row_scale(rows, g)[:, None]
    X = abi_rfft(x, wa, size, shift, fading, T)
    check_rfft(X, x, wa64, size, shift, pad, "stft_fwd", r)
    del X
    dX = abi_rfft(x, ws, size, shift, fading, T, adjoint=True)
    check_rfft(dX, x, ws64, size, shift, pad, "istft_bwd", r, adjoint=True)
    del dX, x
    Y = torch.randn(rows, T, size // 2 + 1, device=DEV, generator=g, dtype=torch.complex64)
    Y *= row_scale(rows, g)[:, None, None]
    y, _ = abi_istft(Y, ws, N, size, shift, fading)
    check_istft(y, Y, ws64, size, shift, pad, "istft_fwd", r)
    r.report(f"{size}/{shift} rows={rows} N={N} fading={fading}")


# ----------------------------------------------------------------------------------------------------- 1024 / 256 plan
@pytest.mark.parametrize("rows,N", PLAN1_CASES)
def test_plan_1024_at_training_sizes(rows, N):
    """stft.hip: tssep_stft_fwd, tssep_istft_fwd with the |y - tgt| partials of every chunk, tssep_istft_bwd."""
    assert L().tssep_stft_plan(1024, 256) == 1
    g = gen(rows + N)
    T = frames_of(N, 1024, 256, True)
    wa64, ws64 = windows64(1024, 256)
    wa, ws = windows32(1024, 256)
    nch, hcb = plan1_chunks(N)
    assert int(L().tssep_istft_chunks(N)) == nch
    r = Ratios()
    x = torch.randn(rows, N, device=DEV, generator=g) * row_scale(rows, g)[:, None]
    X = abi_rfft(x, wa, 1024, 256, True, T)
    check_rfft(X, x, wa64, 1024, 256, 768, "stft_fwd", r)
    del X
    dX = abi_rfft(x, ws, 1024, 256, True, T, adjoint=True)
    check_rfft(dX, x, ws64, 1024, 256, 768, "istft_bwd", r, adjoint=True)
    del dX
    Y = torch.randn(rows, T, 513, device=DEV, generator=g, dtype=torch.complex64)
    s = row_scale(rows, g)
    Y *= s[:, None, None]
    del x
    tgt = torch.randn(rows, N, device=DEV, generator=g) * (0.05 * s)[:, None]
    y, part = abi_istft(Y, ws, N, 1024, 256, True, tgt=tgt)
    check_istft(y, Y, ws64, 1024, 256, 768, "istft_fwd", r, tgt=tgt, part=part, hcb=hcb)
    r.report(f"1024/256 rows={rows} N={N}")


# ------------------------------------------------------------------------------------------------------- fused tail
def _fused_refs(logit, obs, ws64, N, lo, hi):
    """Utterances [lo, hi): (y_ref [rows, N], tol [rows, N]) of istft(sigmoid(logit) obs)."""
    lg = logit[lo:hi].double()
    K, T = lg.shape[1], lg.shape[2]
    est = obs[lo:hi].to(torch.complex128)[:, None] * torch.sigmoid(lg)
    rel = U * (9 + 2 * lg.abs().amax(-1))                  # the mask's relative error and the product's, per frame
    del lg
    return ref_istft(est.reshape(-1, T, 513), ws64, 1024, 256, 768, N, rel.reshape(-1, T))


def _dlogit_ref(dy64, logit, obs, ws64, lo, hi, rel=0.0):
    """d(logit) [b, K, T, F] and its tolerance for the frame samples dy64 [(hi - lo) K, N]."""
    lg = logit[lo:hi].double()
    b, K, T, F = lg.shape
    D, fro = ref_rfft(dy64, ws64, 1024, 256, 768, T, adjoint=True)
    D = D.view(b, K, T, F)
    tol_d = ((fft_rel(1024) + rel) * fro).view(b, K, T, 1)
    o = obs[lo:hi].to(torch.complex128)[:, None]
    dot = o.real * D.real + o.imag * D.imag
    terms = (o.real * D.real).abs() + (o.imag * D.imag).abs()
    m = torch.sigmoid(lg)
    mm = m * (1 - m)
    dm = U * m * (8 + 2 * lg.abs())
    ref = dot * mm
    tol = (o.abs() * tol_d + 3 * U * terms) * mm + dot.abs() * (dm + 3 * U * mm)
    return ref, tol


@pytest.mark.parametrize("B,K,N", FUSED_CASES)
def test_fused_mask_istft_at_training_sizes(B, K, N):
    """tssep_mask_istft_fwd (+ per-chunk |y - tgt| partials), tssep_mask_istft_bwd and tssep_mask_istft_bwd_loss (LogMAE
    into the bt_major layout with a non-identity iperm; MAE into [B, K, T, F]; no target: dy itself, bt_major)."""
    g = gen(B * K + N)
    T = frames_of(N, 1024, 256, True)
    F = 513
    rows = B * K
    _, ws64 = windows64(1024, 256)
    ws64 = ws64.to(DEV)
    _, ws = windows32(1024, 256)
    nch, hcb = plan1_chunks(N)
    r = Ratios()
    logit = torch.randn(B, K, T, F, device=DEV, generator=g).mul_(3)
    obs = torch.randn(B, T, F, device=DEV, generator=g, dtype=torch.complex64)
    obs *= row_scale(B, g)[:, None, None]
    tgt = torch.randn(rows, N, device=DEV, generator=g) * (0.01 * row_scale(B, g).repeat_interleave(K))[:, None]
    y, part = abi_mask_istft(logit, obs, ws, N, tgt=tgt)
    bper = max(1, _row_chunk(T, 1024) // K)
    for lo in range(0, B, bper):
        hi = min(B, lo + bper)
        yr, tol = _fused_refs(logit, obs, ws64, N, lo, hi)
        r.add("mask_istft_fwd", within(y[lo * K:hi * K], yr, tol, "mask_istft_fwd"))
        check_partials(part[lo * K:hi * K], y[lo * K:hi * K], tgt[lo * K:hi * K], hcb, "mask_istft_fwd |y - tgt| partials",
                       r)
        del yr, tol

    def compare(got, dy_of, name, rel=0.0, iperm=None):
        for lo in range(0, B, bper):
            hi = min(B, lo + bper)
            ref, tol = _dlogit_ref(dy_of(lo, hi), logit, obs, ws64, lo, hi, rel)
            if iperm is None:
                gv = got.view(B, K, T, F)[lo:hi] if got.dim() == 4 else got.view(B, T, K, F)[lo:hi].transpose(1, 2)
            else:                                        # speaker k of utterance b at position iperm[b, k]
                gv = got.view(B, T, K, F)[lo:hi].transpose(1, 2)
                gv = gv[torch.arange(hi - lo, device=DEV)[:, None], iperm[lo:hi].long()]
            r.add(name, within(gv, ref, tol, name))
            del ref, tol, gv

    dy = torch.randn(rows, N, device=DEV, generator=g) * row_scale(rows, g)[:, None]
    dl = abi_mask_istft_bwd(dy, logit, obs, ws)
    compare(dl, lambda lo, hi: dy[lo * K:hi * K].double(), "mask_istft_bwd")
    del dl

    # the loss gradient formed in the kernel: gout[b] sign(est - tgt) / (N ln10 sums[b]) (LogMAE), gout[b] sign / N (MAE)
    est = y
    sums = torch.rand(B, device=DEV, generator=g) * 10 ** (torch.rand(B, device=DEV, generator=g) * 4 - 2) + 0.01
    gout = torch.rand(B, device=DEV, generator=g) + 0.5
    iperm = torch.argsort(torch.rand(B, K, device=DEV, generator=g), dim=1).int()
    assert K == 1 or bool((iperm != torch.arange(K, device=DEV)).any())

    def lossgrad(coef):
        return lambda lo, hi: (torch.sign(est[lo * K:hi * K].double() - tgt[lo * K:hi * K].double())
                               * coef[lo:hi].repeat_interleave(K)[:, None])

    coef = gout.double() / (N * math.log(10) * sums.double())
    dl = abi_mask_istft_bwd_loss(est, tgt, sums, gout, logit, obs, ws, iperm, True)
    compare(dl, lossgrad(coef), "mask_istft_bwd_loss LogMAE bt_major iperm", rel=8 * U, iperm=iperm)
    del dl
    dl = abi_mask_istft_bwd_loss(est, tgt, None, gout, logit, obs, ws, None, False)
    compare(dl, lossgrad(gout.double() / N), "mask_istft_bwd_loss MAE", rel=8 * U)
    del dl
    dl = abi_mask_istft_bwd_loss(dy, None, None, None, logit, obs, ws, None, True)
    compare(dl, lambda lo, hi: dy[lo * K:hi * K].double(), "mask_istft_bwd_loss dy bt_major")
    r.report(f"fused B={B} K={K} N={N}")


# ------------------------------------------------------------------------------------------------------- row limit
def test_inverse_row_limit():
    """istft_kernel puts rows on grid.y: 65 535 rows compute (unfused and fused), 65 536 raise through the wrappers."""
    g = gen(65535)
    N = 300
    T = frames_of(N, 1024, 256, True)
    _, ws64 = windows64(1024, 256)
    _, ws = windows32(1024, 256)
    r = Ratios()
    Y = torch.randn(ROW_LIMIT, T, 513, device=DEV, generator=g, dtype=torch.complex64)
    Y *= row_scale(ROW_LIMIT, g)[:, None, None]
    y, _ = abi_istft(Y, ws, N, 1024, 256, True)
    check_istft(y, Y, ws64, 1024, 256, 768, "istft_fwd 65 535 rows", r)
    del Y, y
    with pytest.raises(RuntimeError, match="istft_fwd"):
        H().istft_fwd(torch.zeros(ROW_LIMIT + 1, T, 513, device=DEV, dtype=torch.complex64), ws, N)
    B, K = 13107, 5
    assert B * K == ROW_LIMIT
    logit = torch.randn(B, K, T, 513, device=DEV, generator=g).mul_(3)
    obs = torch.randn(B, T, 513, device=DEV, generator=g, dtype=torch.complex64)
    obs *= row_scale(B, g)[:, None, None]
    y, _ = abi_mask_istft(logit, obs, ws, N)
    bper = max(1, _row_chunk(T, 1024) // K)
    for lo in range(0, B, bper):
        hi = min(B, lo + bper)
        yr, tol = _fused_refs(logit, obs, ws64.to(DEV), N, lo, hi)
        r.add("mask_istft_fwd 65 535 rows", within(y[lo * K:hi * K], yr, tol, "mask_istft_fwd 65 535 rows"))
    del logit, obs, y
    with pytest.raises(RuntimeError, match="mask_istft_fwd"):
        H().mask_istft_fwd(torch.zeros(16384, 4, T, 513, device=DEV), torch.zeros(16384, T, 513, device=DEV,
                                                                                   dtype=torch.complex64), ws, N)
    r.report("row limit")


def test_twiddle_tables():
    """tssep_fft_twiddles: [size/2] exp(-2 pi i k / (size/2)), then [size/2 + 1] exp(-2 pi i k / size), each rounded
    once to fp32."""
    import ctypes
    for size in (1024, 400, 512, 960, 4096):
        nh = size // 2
        host = np.zeros(2 * (2 * nh + 1), dtype=np.float32)
        _ok(L().tssep_fft_twiddles(size, host.ctypes.data_as(ctypes.c_void_p)), "fft_twiddles")
        k1, k2 = np.arange(nh), np.arange(nh + 1)
        ref = np.concatenate([np.exp(-2j * np.pi * k1 / nh), np.exp(-2j * np.pi * k2 / size)])
        ref = np.stack([ref.real, ref.imag], -1).reshape(-1)
        assert np.all(np.abs(host.astype(np.float64) - ref) <= U * np.abs(ref)), size
