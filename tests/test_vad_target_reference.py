"""The float64 references of tests/vad_target_reference.py against what pins them (the reference's recorded doctest
numbers, util.utils.stft_vad, oracle.stft_vad), the checkers against planted defects, and the GPU tests' signal generator
against the undecided share -- all on the CPU."""
import numpy as np
import pytest
import torch

import vad_target_reference as R
from oracle import loss as oloss, stft_vad as ovad

GRID = [(wl, sh, fading) for fading in (True, False, "half") for wl, sh in [(8, 2), (16, 4), (1024, 256), (64, 16)]]


def test_references_reproduce_the_recorded_doctest_numbers(golden):
    """tests/golden/kat_loss.npz: bce / bce10 / bce1 recorded from the reference's
    VADSigmoidBCE(target='Speaker_reverberation_early') on a REAL [2, 100, 257] target (loss.py:286-299)."""
    k = golden("kat_loss")
    torch.manual_seed(0)
    target = torch.rand((2, 100, 257))
    estimate = target + 0.5 * torch.rand((2, 100, 257))
    a64 = R.frame_mag64(target.numpy())
    assert not R.undecided(a64, 0.05, R.rel_bound(512, 257)).any()
    vad = torch.as_tensor(R.decide64(a64, 0.05)).double()
    assert tuple(vad.shape) == (2, 100)
    np.testing.assert_array_equal(vad.numpy().astype(bool), R.decide32(a64.astype(np.float32), 0.05))
    for name, est in (("bce", estimate), ("bce10", ((abs(target) > 0.05).float() - 0.5) * 10),
                      ("bce1", ((abs(target) > 0.05).float() - 0.5) * 1)):
        got = oloss.vad_sigmoid_bce(est.double(), vad)
        assert float(got) == pytest.approx(float(k[name]), rel=1e-6, abs=1e-7), name
    assert float(k["bce"]) == pytest.approx(0.3867, abs=5e-5) and float(k["bce10"]) == pytest.approx(0.0111, abs=5e-5)


@pytest.mark.parametrize("wl,sh,fading", GRID)
def test_gather_equals_stft_vad(wl, sh, fading):
    from tssep_amd.util.utils import stft_vad
    rng = np.random.RandomState(wl + sh)
    for N, density in [(5 * wl + 3, 0.5), (wl - 1, 0.3), (2 * wl, 0.9), (1, 1.0), (sh + 1, 0.5)]:
        if N + (0 if fading is False else (wl - sh) // (2 if fading == "half" else 1) * (1 if fading == "half" else 2)) + sh <= wl:
            continue                                          # (no frame at all: not a case of the reference either)
        v = np.repeat(rng.rand(4, -(-N // 7)) < density, 7, axis=-1)[:, :N]
        want = stft_vad(v, wl, sh, fading)
        np.testing.assert_array_equal(R.gather_loop(v, wl, sh, fading), want)
        np.testing.assert_array_equal(ovad.stft_vad(v, wl, sh, fading), want)
        R.check_gather(want, v, wl, sh, fading)


def test_magnitude_checker_catches_planted_defects():
    x = R.envelope_signal(3, 3000, 11)
    X = R.stft64(x)
    a64 = R.frame_mag64(X)
    R.check_mag(a64.astype(np.float32), a64, 1024, 513)                       # float32 rounding of the truth passes
    for defect in (R.defect_nyquist_dropped, R.defect_dc_twice, R.defect_re_plus_im):
        with pytest.raises(AssertionError, match="outside the bound"):
            R.check_mag(defect(X), a64, 1024, 513)
    with pytest.raises(AssertionError, match="outside the bound"):           # a frame of zeros must give exactly 0
        R.check_mag(np.full((1, 2), 1e-30), np.zeros((1, 2)), 1024, 513)


def test_decision_checkers_catch_planted_defects():
    thr = np.float32(0.05)
    # maximum over the batch instead of the row: a quiet row loses its activity
    a = np.stack([np.linspace(0.0, 1.0, 50), 0.01 * np.linspace(0.0, 1.0, 50) + 1e-5]).astype(np.float32)
    a64 = a.astype(np.float64)
    R.check_exact_decisions(R.decide32(a, thr), a, thr)
    R.check_decisions(R.decide32(a, thr), a64, float(thr), R.rel_bound(1024, 513))
    with pytest.raises(AssertionError):
        R.check_exact_decisions(R.defect_batch_max(a, thr), a, thr)
    with pytest.raises(AssertionError, match="outside the band"):
        R.check_decisions(R.defect_batch_max(a, thr), a64, float(thr), R.rel_bound(1024, 513))
    # >= instead of >: a / m exactly the float32 threshold
    tie = np.array([[1.0, thr, 0.0, np.nextafter(thr, np.float32(1))]], dtype=np.float32)
    assert R.decide32(tie, thr).tolist() == [[True, False, False, True]]
    with pytest.raises(AssertionError, match="float32 formula"):
        R.check_exact_decisions(R.defect_greater_equal(tie, thr), tie, thr)
    # a > thr m instead of a / m > thr: a tie where the two roundings disagree
    a_t, m_t = R.product_tie(thr)
    prod = np.array([[m_t, a_t]], dtype=np.float32)
    assert R.defect_product(prod, thr).tolist() != R.decide32(prod, thr).tolist()
    with pytest.raises(AssertionError, match="float32 formula"):
        R.check_exact_decisions(R.defect_product(prod, thr), prod, thr)
    # a silent row (0 / 0 = NaN compares false) reported active
    silent = np.array([[0.0, 0.0, 0.0], [1.0, 0.5, 0.0]], dtype=np.float32)
    assert R.decide32(silent, thr)[0].tolist() == [False] * 3
    with pytest.raises(AssertionError, match="float32 formula"):
        R.check_exact_decisions(R.defect_silent_active(silent, thr), silent, thr)
    with pytest.raises(AssertionError, match="outside the band"):
        R.check_decisions(R.defect_silent_active(silent, thr), silent.astype(np.float64), float(thr), 1e-4)
    # more than 0.1 % of the frames inside the band is a failure of the case, not a licence
    near = np.full((1, 100), 1.0)
    near[0, 1:] = 0.05 * (1 + 1e-5)
    with pytest.raises(AssertionError, match="undecided"):
        R.check_decisions(np.ones((1, 100)), near, 0.05, 1e-4)


@pytest.mark.parametrize("wl,sh,fading", GRID)
def test_gather_checker_catches_planted_defects(wl, sh, fading):
    N = 5 * wl + 3
    v = np.eye(N, dtype=bool)[sh // 2::sh][:40]               # one-hot rows: a shifted index moves or loses the frame
    v = np.concatenate([v, np.ones((1, N), bool), np.zeros((1, N), bool)])
    R.check_gather(R.gather_loop(v, wl, sh, fading), v, wl, sh, fading)
    hit = np.eye(N, dtype=bool)[[(t + 1) * sh + wl // 2 - (0 if fading is False else (wl - sh) // (2 if fading == "half" else 1)) - 1
                                 for t in range(3, 8)]]
    assert R.gather_loop(hit, wl, sh, fading).sum() == 5
    with pytest.raises(AssertionError, match="first difference"):
        R.check_gather(R.defect_gather_off_by_one(hit, wl, sh, fading), hit, wl, sh, fading)
    if fading == "half":
        with pytest.raises(AssertionError):
            R.check_gather(R.defect_half_as_full(hit, wl, sh, fading), hit, wl, sh, fading)


@pytest.mark.parametrize("case", R.FUSED_CASES, ids=[c[0] for c in R.FUSED_CASES])
def test_generated_signals_stay_decidable(case):
    """Every seeded case of the GPU tests: the float64 reference alone leaves at most 0.1 % of the frames undecided, and a
    float32 torch restatement of the chain stays inside the bound of a and flips no decision outside the band."""
    x, kw, a64, F = R.fused_case(case)
    rel = R.rel_bound(kw["size"], F)
    und = R.undecided(a64, R.THRESHOLD, rel)
    assert und.mean() <= R.MAX_UNDECIDED_SHARE, (case[0], int(und.sum()), und.size)
    from oracle import stft as ostft
    X32 = ostft.stft(torch.as_tensor(x), **kw)
    assert X32.dtype == torch.complex64
    a32 = X32.abs().sum(-1).numpy()
    worst = R.check_mag(a32, a64, kw["size"], F, name=case[0])
    assert worst < rel
    vad32 = R.decide32(a32, R.THRESHOLD)
    R.check_decisions(vad32, a64, R.THRESHOLD, rel, name=case[0])
    if x.shape[0] >= 5:
        assert not vad32[1].any() and a32[1].max() == 0                        # the absent speaker
        assert vad32[2].any() and not vad32[2].all()                           # the single sample: the frames that hold it
