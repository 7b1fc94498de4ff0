"""The kernels behind the VAD losses' device-built targets on a real MI355X, at the smallest shapes at which each can go
wrong: the fused frame magnitudes (both FFT plans, every load path) against float64 within the derived bound, framemag
on a spectrum in memory, the decisions bit-equal to torch's float32 formula, the sample -> frame gather equal to the host
stft_vad, and the fused chain's decisions against float64 outside the undecided band.  The references, the bound and the
band: tests/vad_target_reference.py."""
import numpy as np
import pytest
import torch

import vad_target_reference as R

pytestmark = pytest.mark.gpu

T_ = torch.as_tensor
THR = R.THRESHOLD


def _fused(case):
    """One case through the device -> (a [rows, T] numpy, vad [rows, T] numpy, the device tensors a, vad)."""
    from tssep_amd import functional as Fn, hip_ops as H
    from tssep_amd.train.feature_extractor import STFT
    name, size, shift, window, wl, fading, pad, rows, N, seed, offset = case
    x, kw, a64, F = R.fused_case(case)
    if wl is not None or fading == "half" or not pad:
        fe = STFT(size=size, shift=shift, window_length=wl, pad=pad, fading=fading, window=window)
        xd = T_(x).cuda()
        vad = fe.frame_activity(xd, THR)
        lead, tail = fe._fade()
        w, _ = fe._windows(xd.device)
        a = H.stft_framemag(torch.nn.functional.pad(xd, (lead, tail)), w, size, shift, False, T=fe.frames(N))
    else:
        buf = torch.zeros(rows * N + 2, device="cuda")
        xd = buf[offset:offset + rows * N].view(rows, N)
        xd.copy_(T_(x))
        assert xd.data_ptr() % 8 == (4 if offset else 0)
        w, _ = Fn.windows(window, size, shift, xd.device, size)
        a = H.stft_framemag(xd, w, size, shift, bool(fading), T=a64.shape[-1])
        vad = H.vad_from_mag(a, THR)
    return x, kw, a64, F, a, vad


@pytest.mark.parametrize("case", R.FUSED_CASES, ids=[c[0] for c in R.FUSED_CASES])
def test_fused_frame_magnitudes_and_decisions_against_float64(case):
    from tssep_amd import functional as Fn, hip_ops as H
    x, kw, a64, F, a, vad = _fused(case)
    size, shift = kw["size"], kw["shift"]
    assert tuple(a.shape) == a64.shape and a.dtype == torch.float32
    worst = R.check_mag(a.cpu().numpy(), a64, size, F, name=case[0])
    print(f"{case[0]}: worst relative error of a {worst:.3g} (bound {R.rel_bound(size, F):.3g})")
    if x.shape[0] >= 5:
        assert float(a[1].abs().max()) == 0.0                                  # a frame of zeros gives exactly 0
    # the decisions: bit-equal to torch's formula on the same a, and the float64 chain's outside the band
    R.check_exact_decisions(vad.cpu().numpy(), a.cpu().numpy(), THR, name=case[0])
    share = R.check_decisions(vad.cpu().numpy(), a64, THR, R.rel_bound(size, F), name=case[0])
    print(f"{case[0]}: undecided share {share:.4%}")
    # the same bits on every run
    _, _, _, _, a2, vad2 = _fused(case)
    assert torch.equal(a, a2) and torch.equal(vad, vad2)
    # and, within the bound, framemag of the spectrum stft_fwd wrote for the same frames
    if kw["window_length"] is None and kw["pad"]:
        w, _ = Fn.windows(kw["window"], size, shift, a.device, size)
        X = H.stft_fwd(T_(x).cuda(), w, size, shift, bool(kw["fading"]), T=a64.shape[-1])
        am = H.framemag(X)
        R.check_mag(am.cpu().numpy(), a64, size, F, name=case[0] + " (materialised)")
        tol = 2 * R.mag_bound(a64, size, F)
        assert (np.abs(am.cpu().numpy().astype(np.float64) - a.cpu().numpy()) <= tol).all()


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("F", [1, 201, 257, 513])
@pytest.mark.parametrize("T", [1, 5])
def test_framemag(F, T, cplx):
    from tssep_amd import hip_ops as H
    g = torch.Generator().manual_seed(F * 10 + T)
    rows = 3
    re = torch.randn(rows, T, F, generator=g)
    re[1, 0] = 0                                                               # a frame of zeros
    X = torch.complex(re, torch.randn(rows, T, F, generator=g) * (re != 0)) if cplx else re
    a = H.framemag(X.cuda())
    assert tuple(a.shape) == (rows, T) and a.dtype == torch.float32
    a64 = X.to(torch.complex128 if cplx else torch.float64).abs().sum(-1).numpy()
    # no transform here: 3u per modulus and (F / 64 + 8) u for the sum, relative to a (vad_target_reference's second term)
    tol = (F / 64 + 11) * R.U32 * a64
    assert (np.abs(a.cpu().numpy().astype(np.float64) - a64) <= tol).all(), float(np.abs(a.cpu().numpy() - a64).max())
    assert float(a[1, 0]) == 0.0
    assert torch.equal(a, H.framemag(X.cuda()))


def _mag_rows(T, seed):
    """Rows of frame magnitudes with every decision the kernel can get wrong."""
    rng = np.random.RandomState(seed)
    thr = np.float32(THR)
    a = rng.uniform(0.0, 1.0, size=(9, T)).astype(np.float32) ** 4            # most frames below, some above the threshold
    a[0, 0] = 3.0                                                               # the maximum in the first frame
    a[1, -1] = 2.5                                                              # ... in the last
    a[2] = 0.0                                                                  # a silent row: 0 / 0 compares false
    a[3] = a[3, 0] + 1e-3                                                       # all equal: a == m everywhere, ratio 1
    a[4, :] = thr                                                               # ties: a / m exactly thr with m = 1 ...
    a[4, T // 2] = 1.0
    if T > 2:
        a[4, 0] = np.nextafter(thr, np.float32(1))                              # ... and one ulp above it
    a_t, m_t = R.product_tie(thr)                                              # where a > thr m would decide otherwise
    a[5] = np.minimum(a[5], 0.5) * m_t
    a[5, -1] = m_t
    a[5, 0] = a_t
    a[6] *= np.float32(1e-30)                                                  # tiny and huge rows: the division scales out
    a[7] *= np.float32(1e30)
    return a


@pytest.mark.parametrize("T", [1, 63, 64, 65, 1000, 5000])
def test_vad_from_mag_is_bit_equal_to_torch(T):
    from tssep_amd import hip_ops as H
    a = _mag_rows(T, seed=T)
    ad = T_(a).cuda()
    vad = H.vad_from_mag(ad, THR)
    assert vad.dtype == torch.float32 and tuple(vad.shape) == a.shape
    R.check_exact_decisions(vad.cpu().numpy(), a, THR)
    # torch on the device, the expression of loss.py:319-321 itself
    want = ((ad / torch.amax(ad, dim=-1, keepdim=True)) > THR).float()
    assert torch.equal(vad, want)
    assert not bool(vad[2].any()) and bool(vad[3].all())
    assert torch.equal(vad, H.vad_from_mag(ad, THR))
    # another threshold, passed as a double and compared as a float
    assert torch.equal(H.vad_from_mag(ad, 0.3), ((ad / torch.amax(ad, dim=-1, keepdim=True)) > 0.3).float())


GRID = [(wl, sh, fading) for fading in (True, False, "half") for wl, sh in [(8, 2), (16, 4), (1024, 256), (64, 16)]]


@pytest.mark.parametrize("wl,sh,fading", GRID)
def test_vad_frames_equals_host_stft_vad(wl, sh, fading):
    from tssep_amd import hip_ops as H
    from tssep_amd.util.utils import stft_vad, stft_vad_device
    rows = 7
    for N in (1, 255, 256, 257, 4099):
        lead2 = 0 if fading is False else (wl - sh) * (1 if fading == "half" else 2)
        if N + lead2 + sh <= wl:
            continue                                                           # no frame at all (the host code has none either)
        rng = np.random.RandomState(N + wl)
        v = np.repeat(rng.rand(rows, -(-N // 37)) < 0.5, 37, axis=-1)[:, :N]
        v[0] = True                                                            # all active
        v[1] = False                                                           # all silent
        v[2] = False
        v[2, N // 2] = True                                                    # a single-sample run
        want = stft_vad(v, wl, sh, fading)
        for dtype in (torch.bool, torch.uint8, torch.float32):
            got = H.vad_frames(T_(v).to(dtype).cuda(), wl, sh, fading)
            assert got.dtype == torch.float32 and got.is_cuda
            np.testing.assert_array_equal(got.cpu().numpy(), want.astype(np.float32))
        R.check_gather(got.cpu().numpy(), v, wl, sh, fading)
        # the public route: util.utils.stft_vad_device on a CUDA tensor, leading dimensions kept
        pub = stft_vad_device(T_(v).cuda().view(1, rows, N), wl, sh, fading)
        assert pub.is_cuda and pub.dtype == torch.float32 and tuple(pub.shape) == (1, rows, want.shape[-1])
        np.testing.assert_array_equal(pub[0].cpu().numpy(), want.astype(np.float32))
        np.testing.assert_array_equal(stft_vad(T_(v), wl, sh, fading).numpy(), want.astype(np.float32))
