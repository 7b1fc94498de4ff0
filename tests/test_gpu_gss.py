"""The guided cACGMM kernels (csrc/gss.hip) against the float64 reference of tests/gss_reference.py.

ALLOWANCE.  The kernel and the reference differ in the order of their sums over frames (the kernel: frames ascending
inside a chunk of 256, chunks ascending), in fused multiply-adds, in OCML's exp / log against libm's (a few ulp each;
D <= 8 multiplies the one in D log q) and in L^-1 applied as a product where the reference substitutes forward.  None of
that is measured on the kernel: the yardstick is the largest change of the REFERENCE over its three summation orders and
the seeds 0-3 at the case's shape (several seeds, not one draw), and an element of gamma may be
MARGIN x yardstick + 4 * 2^-52 away, MARGIN = 16.  Every test prints its worst error / yardstick before it asserts
(measured on an MI355X: 1.25 at worst after one iteration, 2.92 after twenty; DESIGN 4.24 has the table).

The frame counts 63, 64, 65 straddle the kernel's tile of 64 frames, 300 its chunk of 256 = 4 * 64."""
import ctypes

import numpy as np
import pytest
import torch

import gss_reference as R
from tssep_amd import _lib, hip_ops as H
from tssep_amd.train import enhancer, feature_extractor as fe

pytestmark = pytest.mark.gpu
MAIN = (6, 2, 200, 5, "plain")


def _gpu(Y, act, iterations, **kw):
    kw.setdefault("out_dtype", torch.float64)
    g = H.guided_cacgmm(torch.from_numpy(np.ascontiguousarray(Y)).cuda(), torch.from_numpy(np.ascontiguousarray(act)).cuda(),
                        iterations, **kw)
    return g.cpu().numpy()


def _against_reference(case, iterations):
    yard, refs = R.yardstick(case, iterations)
    allow = R.allowance(case, iterations)
    worst, got = 0.0, {}
    for seed in R.SEEDS:
        Y, act, _ = R.case_scene(case, seed)
        got[seed] = _gpu(Y, act, iterations)
        assert got[seed].shape == refs[seed].shape and np.isfinite(got[seed]).all()
        worst = max(worst, float(np.abs(got[seed] - refs[seed]).max()))
    print(f"case {case} x {iterations}: worst |error| {worst:.3e}, yardstick {yard:.3e}, "
          f"error / yardstick {worst / yard if yard else float('inf') if worst else 0.0:.2f}, allowance {allow:.3e}")
    assert worst <= allow
    return got


@pytest.mark.parametrize("case", R.ONE_ITERATION_CASES, ids=lambda c: "-".join(map(str, c)))
def test_one_iteration(case):
    got = _against_reference(case, 1)
    D, K, T, F, variant = case
    for seed, g in got.items():
        _, act, _ = R.case_scene(case, seed)
        assert (g[:-1][act == 0] == 0).all()
        if variant == "zero_frame":
            assert (g[:, T // 2] == 0).all()
        if variant == "noise_only":
            assert (g[-1] == 1).all()


@pytest.mark.parametrize("case", R.TWENTY_ITERATION_CASES, ids=lambda c: "-".join(map(str, c)))
def test_twenty_iterations(case):
    got = _against_reference(case, 20)
    if case == MAIN:
        for seed, g in got.items():
            _, _, on = R.case_scene(case, seed)
            rec = R.recovery(g, on)
            print(f"seed {seed}: recovery {rec:.4f}")
            assert rec >= 0.95


@pytest.mark.parametrize("iterations", [1, 20])
def test_two_frames_of_two_channels(iterations):
    """D = 2, T = 2: speaker 0 owns one frame, its B_c is a rank-one matrix plus the load, condition D / load = 2e6.  The
    order yardstick is 0 by construction here (a sum of two terms has no order) while the second Cholesky pivot is what a
    cancellation leaves of 1e-6, so the shape has a yardstick of its own, R.rounding_yardstick: the largest change of the
    reference under everything that changes its roundings only (the orders, L^-1 as a product, the pivots carried in
    extended precision, the channels reversed, every frame rescaled), seeds 0-3 -- 1.4e-13 after one iteration (the
    channel reversal at seed 3), 6.8e-18 after twenty (the posteriors have gone to 0 / 1).  Same form of allowance, same
    margin.  Measured on the kernel: 2.6e-13 (one iteration, seed 3 as well), 1.4e-17 (twenty)."""
    case = R.RANK_DEFICIENT_CASE
    yard, refs = R.rounding_yardstick(case, iterations)
    allow = R.MARGIN * yard + R.FLOOR
    worst = 0.0
    for seed in R.SEEDS:
        Y, act, _ = R.case_scene(case, seed)
        g = _gpu(Y, act, iterations)
        worst = max(worst, float(np.abs(g - refs[seed]).max()))
        assert np.abs(g.sum(0) - 1).max() <= 4 * 2.0 ** -52 and (g[:-1][act == 0] == 0).all()
    print(f"case {case} x {iterations}: worst |error| {worst:.3e}, rounding yardstick {yard:.3e}, "
          f"error / yardstick {worst / yard:.2f}, allowance {allow:.3e}")
    assert worst <= allow


def test_weights_uniform_and_load():
    """the two keywords reach the kernel: against the reference with the same values, same form of allowance"""
    case = (6, 2, 65, 5, "plain")
    Y, act, _ = R.case_scene(case, 0)
    for kw in (dict(weights="uniform"), dict(load=1e-2)):
        yard, ref = R.spread(Y, act, 3, **kw)
        err = np.abs(_gpu(Y, act, 3, **kw) - ref).max()
        print(kw, err, yard)
        assert err <= R.MARGIN * yard + R.FLOOR
        assert np.abs(ref - R.guided_cacgmm_reference(Y, act, 3)).max() > 1e-6


# ------------------------------------------------------------------------------------------------ bits and splits
def test_same_bits_and_float32_is_the_rounding():
    Y, act, _ = R.case_scene((6, 2, 300, 5, "plain"), 0)
    a, b = _gpu(Y, act, 5), _gpu(Y, act, 5)
    assert np.array_equal(a, b)
    f32 = _gpu(Y, act, 5, out_dtype=torch.float32)
    assert f32.dtype == np.float32 and np.array_equal(f32, a.astype(np.float32))


def test_blocks_equal_separate_calls_on_their_slices():
    Y, act, _ = R.case_scene((6, 2, 300, 5, "plain"), 1)
    table = H.gss_uniform_blocks(300, 100, 30)
    assert len(table) == 3
    g = _gpu(Y, act, 4, blocks=table)
    for sf, ef, so, eo in table.tolist():
        part = _gpu(Y[:, sf:ef], act[:, sf:ef], 4)
        assert np.array_equal(g[:, so:eo], part[:, so - sf:eo - sf])
    assert np.array_equal(_gpu(Y, act, 4, blocks=[(0, 300, 0, 300)]), _gpu(Y, act, 4))
    assert not np.array_equal(g, _gpu(Y, act, 4))


def test_segments_to_activity():
    K, T = 3, 300
    rows = [(0, 0, 10), (0, 5, 40), (1, 299, 300), (2, 64, 257), (3, 0, 10), (-1, 0, 10), (1, -1, 5), (1, 290, 301),
            (2, 20, 20), (2, 30, 25)]
    want = np.zeros((K, T), dtype=np.uint8)
    for k, s, e in rows:
        if 0 <= k < K and 0 <= s < e <= T:
            want[k, s:e] = 1
    got = H.segments_to_activity(torch.tensor(rows, dtype=torch.int32).cuda(), K, T)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    empty = H.segments_to_activity(torch.zeros(0, 3, dtype=torch.int32).cuda(), K, T)
    assert not empty.any()


# ------------------------------------------------------------------------------------------------ the chain
STFT = dict(size=64, shift=16)           # F = 33: the general FFT plan


def _si_sdr(stft, spec, image):
    """SI-SDR [K] in dB of the time signals of spec [K, T, F] against those of image [K, T, F] (hip_ops.sdr)"""
    est = stft.istft(spec.to(torch.complex64))
    tgt = stft.istft(image.to(torch.complex64))
    return H.sdr(est[None], tgt[None])[0][0].double().cpu().numpy()


def test_chain():
    """GSS()(Y, dia, numpy_out=True) -> inverse STFT -> SI-SDR of every speaker against their image at channel 0 inside
    their activity, against the same beamformer fed the float64 reference's masks.
    SLACK.  The reference chain's own spread over the three summation orders, times MARGIN, plus a floor for the float32
    tail both chains share (the masks reach the beamformer as float32, the inverse STFT and hip_ops.sdr run in float32):
    SI-SDR is 10 log10 of a ratio of float32 energies over N ~ 3200 samples, each good to ~sqrt(N) 2^-24 ~ 3e-6
    relative, and the distortion energy is what is left of a cancellation that amplifies this by the SDR ratio itself,
    <= 1e3 at 30 dB: 3e-3 relative, 0.013 dB -> floor 0.05 dB."""
    D, K, T, F = 6, 2, 200, 33
    Y, act, on, images = R.scene(0, D, K, T, F)
    stft = fe.STFT(window="hann", **STFT)
    Yd = torch.from_numpy(Y).cuda()
    dia = [act[k] for k in range(K)]
    gate = torch.from_numpy(act.astype(np.float64)).cuda()[:, :, None]
    image0 = torch.from_numpy(np.ascontiguousarray(images[:, 0])).cuda() * gate
    raw = _si_sdr(stft, Yd[0][None] * gate, image0)

    gss = enhancer.GSS()
    out = gss(Yd, dia, numpy_out=True)
    assert out.shape == (K, T, F) and out.dtype == torch.complex128
    assert (out[torch.from_numpy(act == 0).cuda()] == 0).all()
    got = _si_sdr(stft, out, image0)

    bf = enhancer.ClassicBF_np(distortion_mask=enhancer.enhancer_distortion_mask.SumCrossTalker())
    ref = []
    for order in R.ORDERS:
        m = torch.from_numpy(R.guided_cacgmm_reference(Y, act, order=order)).to(torch.float32).cuda()[:, None]
        ref.append(_si_sdr(stft, bf(m, Yd, dia + [[]], numpy_out=True)[:K], image0))
    spread = max(np.abs(ref[0] - r).max() for r in ref[1:])
    slack = R.MARGIN * spread + 0.05
    print(f"SI-SDR dB: channel 0 {raw}, kernel chain {got}, reference chain {ref[0]}; improvement kernel {got - raw}, "
          f"reference {ref[0] - raw}; reference spread {spread:.2e} dB, slack {slack:.3f} dB")
    assert (got >= ref[0] - slack).all()
    assert (ref[0] - raw > 3).all()                       # the scene is one the reference masks help on
    assert (got - raw >= 0.5 * (ref[0] - raw)).all()

    # the same from a [K, T] tensor and from the device segment table
    assert torch.equal(gss(Yd, torch.from_numpy(act).cuda(), numpy_out=True), out)
    table = torch.tensor([(k, s, e) for k in range(K) for s, e in enhancer.normalized_intervals(act[k], T)],
                         dtype=torch.int32).cuda()
    assert torch.equal(gss(Yd, table, numpy_out=True, K=K), out)
    masks = gss.masks(Yd, table, K=K)
    assert masks.shape == (K + 1, 1, T, F) and masks.dtype == torch.float32
    views = gss(Yd, dia)
    assert len(views) == K and all(torch.equal(v, out[k, s:e]) for k in range(K) for (s, e), v in views[k].items())

    wpe = enhancer.GSS(pre_wpe=enhancer.WPE(taps=2, iterations=1))(Yd, dia, numpy_out=True)
    assert wpe.shape == out.shape and torch.isfinite(torch.view_as_real(wpe)).all()
    assert (wpe - out).abs().max() > 1e-6 * out.abs().max()


def test_masks_take_fewer_than_six_channels():
    Y, act, _ = R.case_scene((2, 2, 65, 5, "plain"), 0)
    m = enhancer.GSS(iterations=1).masks(Y, [act[0], act[1]])
    assert m.shape == (3, 1, 65, 5) and m.is_cuda and m.dtype == torch.float32
    # float32 masks of values <= 1: half an ulp of rounding (2^-25 at most) on either side of the float64 allowance
    want = R.guided_cacgmm_reference(Y, act, 1)
    assert np.abs(m[:, 0].cpu().numpy().astype(np.float64) - want).max() <= 2.0 ** -24


# ------------------------------------------------------------------------------------------------ guards
def test_guards_return_codes_and_launch_nothing():
    """D = 9, K = 9: TSSEP_E_UNSUPPORTED (-3); load = 0, iterations = 0: TSSEP_E_SHAPE (-1) -- the entry returns before its
    first launch: the output keeps its fill.  The Python layer raises ValueError for the same before it gets there."""
    L = _lib.lib()
    T, F = 8, 3
    obs = torch.zeros(9, T, F, 2, dtype=torch.float64, device="cuda")
    act = torch.ones(9, T, dtype=torch.uint8, device="cuda")
    blocks = torch.tensor([[0, T, 0, T]], dtype=torch.int32, device="cuda")
    out = torch.full((10, T, F), -7.0, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def fit(D, K, iterations, load):
        return L.tssep_gss_fit(p(obs), p(act), p(blocks), p(out), 1, p(ws), 1, D, K, T, F, T, iterations, load, 0,
                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

    assert fit(9, 2, 1, 1e-6) == -3
    assert fit(6, 9, 1, 1e-6) == -3
    assert fit(6, 2, 1, 0.0) == -1
    assert fit(6, 2, 1, -1.0) == -1
    assert fit(6, 2, 0, 1e-6) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    Yc = torch.zeros(9, T, F, dtype=torch.complex128, device="cuda")
    with pytest.raises(ValueError):
        H.guided_cacgmm(Yc, act[:2], 1)
    with pytest.raises(ValueError):
        H.guided_cacgmm(Yc[:6], act, 1)
    with pytest.raises(ValueError):
        H.guided_cacgmm(Yc[:6], act[:2], 1, load=0.0)
