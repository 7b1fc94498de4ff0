"""The frame-recursive MVDR of DESIGN 4.18 restated in numpy -- the checker of tests/test_gpu_online_mvdr.py, tested
without a GPU -- and what the Python layers refuse on the arguments alone.

`online_reference` runs, for every (b, k, f) and frame by frame,

    Phi_s = a Phi_s + m y y^H      Phi_n = a Phi_n + (1 - m) y y^H      l = delta Re tr(Phi_s + Phi_n) / D
    phi = solve(Phi_n + l I, Phi_s)      w = phi[:, ref] / max(Re tr phi, eps)      enh = w^H y  (* max(m, masking_eps))

with the statistics, the loading, the scaling and the filtering in float64 (extended=False) or one step above it
(extended=True: np.longdouble or mpmath, `backend()` of tests/test_mvdr_reference.py; complex numbers are pairs).  The
solve is `lu_reference` of that file, the elimination the kernels restate; it takes complex128, so the extended run
hands it the correctly rounded statistics of the frame and keeps everything around it extended.  A bin whose trace is
exactly zero gives zero and is not solved.

COMPARISON (`errors`, `yardsticks`): the error of an output element is |x - ext| / sum_d |w_d| |y_d| (the scale of the
filtering's own bound in tests/test_mvdr_reference.py; |ext| itself will not do, a beamformer's output is a cancellation
wherever it nulls an interferer), that of a state element (i, j) is |x - ext| / sqrt(T_ii T_jj), T = Phi_s + Phi_n (the
Cauchy-Schwarz scale of a sum of y_i conj(y_j)); 0 / 0 = 0.  The yardsticks of a set of inputs are the largest such errors
of the float64 run, and the kernel may be 8 times that far from the extended run at any element (a different but fixed
summation order of the rank-one updates, fused multiply-adds).  The planted defects below must exceed 8 x a yardstick:
three show in the output; the forgetting factor applied after the update scales both PSDs alike, which no MVDR output
can see -- it shows in the state, and the GPU test compares the state too."""
import numpy as np
import pytest
import torch

from test_mvdr_reference import backend, forward_bound, graded_mixture, lu_reference, pack_hermitian, xc, xcf, xf, xr

DEFECTS = ("stale", "load_n", "alpha_after", "conj")
FACTOR = 8.0


def _conv(extended):
    return xr if extended else (lambda a: np.array(a, dtype=np.float64))


def online_reference(Y, masks, state=None, ref=0, forgetting=1.0, diag_load=1e-6, eps=None, masking=False,
                     masking_eps=0.0, extended=True, defect=None):
    """Y [B,D,T,F] complex, masks [B,K,T,F] real, state what an earlier call returned -> (enh pair (re, im) [B,K,T,F],
    state: the pair (re, im) of [2: Phi_s, Phi_n][B,K,F,D,D] in the run's precision, scale float64 [B,K,T,F]:
    sum_d |w_d| |y_d| (times the masking factor), what an error of enh is measured against)."""
    Y, m = np.asarray(Y, dtype=np.complex128), np.asarray(masks, dtype=np.float64)
    B, D, T, F = Y.shape
    K = m.shape[1]
    conv = _conv(extended)
    num = lambda v: conv(np.array([v]))[0]
    a, delta, one = num(forgetting), num(diag_load), num(1.0)
    eps = num(np.finfo(np.float64).tiny if eps is None else eps)
    if state is None:
        Sr, Si = conv(np.zeros((2, B, K, F, D, D))), conv(np.zeros((2, B, K, F, D, D)))
    else:
        Sr, Si = state[0].copy(), state[1].copy()
    out_r, out_i = conv(np.zeros((B, K, T, F))), conv(np.zeros((B, K, T, F)))
    scale = np.zeros((B, K, T, F))
    eye = np.eye(D, dtype=bool)
    n = B * K * F
    with np.errstate(all="ignore"):
        for t in range(T):
            yr, yi = (conv(p.transpose(0, 2, 1)) for p in (Y[:, :, t].real, Y[:, :, t].imag))              # [B,F,D]
            Pr = (yr[..., :, None] * yr[..., None, :] + yi[..., :, None] * yi[..., None, :])[:, None]      # y_i conj(y_j)
            Pi = (yi[..., :, None] * yr[..., None, :] - yr[..., :, None] * yi[..., None, :])[:, None]
            w0 = conv(m[:, :, t])[..., None, None]
            w = (w0, one - w0)
            used = (Sr.copy(), Si.copy()) if defect == "stale" else None
            for q in (0, 1):
                if defect == "alpha_after":
                    Sr[q], Si[q] = a * (Sr[q] + w[q] * Pr), a * (Si[q] + w[q] * Pi)
                else:
                    Sr[q], Si[q] = a * Sr[q] + w[q] * Pr, a * Si[q] + w[q] * Pi
            Ur, Ui = used if used is not None else (Sr, Si)
            diag = lambda M: M[..., eye].sum(-1) if False else sum(M[..., i, i] for i in range(D))
            tr = diag(Ur[0]) + diag(Ur[1])                                                                   # [B,K,F]
            load = delta * (diag(Ur[1]) if defect == "load_n" else tr) / num(float(D))
            live = xf(tr).reshape(n) != 0
            Ar, Ai = Ur[1].copy(), Ui[1].copy()
            for i in range(D):
                Ar[..., i, i] = Ar[..., i, i] + load
            A = (xf(Ar) + 1j * xf(Ai)).reshape(n, D, D)
            X = (xf(Ur[0]) + 1j * xf(Ui[0])).reshape(n, D, D)
            A[~live] = np.eye(D)
            phr, phi = lu_reference(A, X, extended=extended)["phi"]
            lam = sum(phr[:, i, i] for i in range(D))
            lam = np.where(np.asarray(lam < eps, dtype=bool), eps, lam)
            wr, wi = phr[:, :, ref] / lam[:, None], phi[:, :, ref] / lam[:, None]                            # [n,D]
            ysr = np.broadcast_to(yr[:, None], (B, K, F, D)).reshape(n, D)
            ysi = np.broadcast_to(yi[:, None], (B, K, F, D)).reshape(n, D)
            er = sum(wr[:, d] * ysr[:, d] + wi[:, d] * ysi[:, d] for d in range(D))                          # conj(w) y
            ei = sum(wr[:, d] * ysi[:, d] - wi[:, d] * ysr[:, d] for d in range(D))
            if defect == "conj":
                ei = -ei                                                                                     # w conj(y)
            sc = sum(np.hypot(xf(wr[:, d]), xf(wi[:, d])) * np.hypot(xf(ysr[:, d]), xf(ysi[:, d])) for d in range(D))
            if masking:
                g = conv(np.maximum(m[:, :, t], masking_eps)).reshape(n)
                er, ei, sc = er * g, ei * g, sc * xf(g)
            scale[:, :, t] = np.where(live, sc, 0.0).reshape(B, K, F)
            zero = num(0.0)
            er, ei = np.where(live, er, zero), np.where(live, ei, zero)
            out_r[:, :, t], out_i[:, :, t] = er.reshape(B, K, F), ei.reshape(B, K, F)
    return (out_r, out_i), (Sr, Si), scale


def packed_state(state):
    """the reference's state -> float64 [B,K,2,D*D,F], the kernel's layout"""
    M = xf(state[0]) + 1j * xf(state[1])                      # [2,B,K,F,D,D]
    return np.moveaxis(pack_hermitian(M), 0, 2)              # [2,B,K,D*D,F] -> [B,K,2,D*D,F]


def _ratio(err, scale):
    with np.errstate(all="ignore"):
        r = err / scale
    r = np.where(err == 0, 0.0, r)
    return np.nan_to_num(r, nan=np.inf, posinf=np.inf)


def state_scale(state):
    """sqrt(T_ii T_jj) per packed row, T = Phi_s + Phi_n of the (extended) reference -> [B,K,1,D*D,F]"""
    T = xf(state[0][0] + state[0][1])                                       # [B,K,F,D,D]
    D = T.shape[-1]
    s = np.sqrt(np.stack([T[..., i, i] for i in range(D)], -1))            # [B,K,F,D]
    rows = [s[..., i] ** 2 for i in range(D)]
    for i in range(D):
        for j in range(i + 1, D):
            rows += [s[..., i] * s[..., j]] * 2
    return np.stack(rows, -2)[:, :, None]


def errors(enh, state, ref):
    """enh complex [B,K,T,F], state float64 [B,K,2,D*D,F] (the kernel's layout), ref = online_reference(..., extended=True)
    -> (worst output error, worst state error) on the scales of the module docstring"""
    ext, ext_state, scale = ref
    enh, state = np.asarray(enh), np.asarray(state)
    eo = _ratio(np.where(np.isfinite(enh), np.abs(enh - xcf(ext)), np.inf), scale)
    es = _ratio(np.where(np.isfinite(state), np.abs(state - packed_state(ext_state)), np.inf), state_scale(ext_state))
    return float(eo.max()), float(es.max())


def yardsticks(f64, ref):
    """the float64 run's own errors against the extended run"""
    return errors(xcf(f64[0]), packed_state(f64[1]), ref)


def array_inputs(D, T, F, seed, B=2, K=3, lo=0.05, hi=0.95):
    """graded_mixture-style array data per batch element, masks mapped into [lo, hi] -> Y [B,D,T,F], masks [B,K,T,F]"""
    Ys, ms = zip(*(graded_mixture(D, T, F, seed + 17 * b, K=K) for b in range(B)))
    m = np.stack(ms)
    return np.stack(Ys), lo + (hi - lo) * (m - m.min()) / (m.max() - m.min())


def _random(D, T, F, seed, B=2, K=3):
    rs = np.random.RandomState(seed)
    Y = rs.standard_normal((B, D, T, F)) + 1j * rs.standard_normal((B, D, T, F))
    return Y, 0.1 + 0.8 * rs.random_sample((B, K, T, F))


# ---- the reference itself ------------------------------------------------------------------------------------------------
def test_backend_is_extended():
    assert backend() in ("longdouble", "mpmath")


@pytest.mark.parametrize("D", (2, 6))
def test_last_frame_is_torch_bf(D):
    """forgetting = 1, diag_load = 0: the filter of frame T - 1 is TorchBF's.  Both sides solve the same system up to the
    rounding of the statistics (T + 4 roundings per entry, below the GAMMA(D) of the solve bound: its |L| |U| |phi|
    dominates |A| |phi| and |X|), so each lies within 2 x forward_bound of the exact phi and the two within 4 x of each
    other; the bound on phi goes through w = phi[:, ref] / tr phi and enh = w^H y to first order."""
    from oracle import enhancer as oe
    T, F, ref = 12, 9, 1
    Y, m = _random(D, T, F, seed=3 + D)
    (er, ei), state, _ = online_reference(Y, m, ref=ref, forgetting=1.0, diag_load=0.0, extended=False)
    got = er[:, :, T - 1] + 1j * ei[:, :, T - 1]      # (the frames in front of D - 1 are singular without loading)
    want = oe.torch_bf(m[:, :, None], Y, ref)[:, :, T - 1]
    S = xf(state[0]) + 1j * xf(state[1])
    n = S[0].size // (D * D)
    A, X = S[1].reshape(n, D, D), S[0].reshape(n, D, D)
    lu = lu_reference(A, X)
    phi = xcf(lu["phi"])
    fb = forward_bound(A, lu, phi)
    lam = np.trace(phi, axis1=-2, axis2=-1).real
    dw = fb[:, :, ref] / lam[:, None] + np.abs(phi[:, :, ref]) * np.trace(fb, axis1=-2, axis2=-1)[:, None] / lam[:, None] ** 2
    y = np.broadcast_to(np.abs(Y[:, None, :, T - 1]).transpose(0, 1, 3, 2), (2, 3, F, D)).reshape(n, D)
    bound = 4.0 * (dw * y).sum(-1).reshape(2, 3, F)
    err = np.abs(got - want)
    print(f"D={D}: worst |online - TorchBF| / bound = {(err / bound).max():.3g}")
    assert np.isfinite(want).all() and (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("extended", (False, True))
def test_chunk_invariance_of_the_reference(extended):
    Y, m = array_inputs(3, 7, 5, seed=2)
    kw = dict(ref=1, forgetting=0.9, diag_load=1e-3, extended=extended)
    whole, sw, _ = online_reference(Y, m, **kw)
    parts, st, pos = [], None, 0
    for c in (1, 2, 4):
        e, st, _ = online_reference(Y[:, :, pos:pos + c], m[:, :, pos:pos + c], st, **kw)
        parts.append(e)
        pos += c
    for q in (0, 1):
        assert np.array_equal(np.concatenate([p[q] for p in parts], axis=2), whole[q])
        assert np.array_equal(st[q], sw[q])


def test_silent_start_and_full_masks():
    Y, m = array_inputs(4, 8, 6, seed=5)
    Y[:, :, :3] = 0
    e, st, _ = online_reference(Y, m, diag_load=1e-6, extended=False)
    e = e[0] + 1j * e[1]
    assert (e[:, :, :3] == 0).all() and np.isfinite(e).all() and np.abs(e[:, :, 3:]).min() > 0
    _, s3, _ = online_reference(Y[:, :, :3], m[:, :, :3], extended=False)
    assert (s3[0] == 0).all() and (s3[1] == 0).all()
    late, _, _ = online_reference(Y[:, :, 3:], m[:, :, 3:], diag_load=1e-6, extended=False)
    assert np.array_equal(late[0] + 1j * late[1], e[:, :, 3:])
    # m = 1 everywhere: Phi_n is zero, the loading alone carries the solve
    Y, m = array_inputs(4, 6, 6, seed=6)
    e, _, _ = online_reference(Y, np.ones_like(m), diag_load=1e-6, extended=False)
    assert np.isfinite(e[0]).all() and np.isfinite(e[1]).all()


def test_masking_factor():
    Y, m = array_inputs(3, 5, 6, seed=7, lo=0.0, hi=0.9)
    plain, _, _ = online_reference(Y, m, diag_load=1e-3, extended=False)
    for meps in (0.0, 0.3):
        mk, _, _ = online_reference(Y, m, diag_load=1e-3, masking=True, masking_eps=meps, extended=False)
        g = np.maximum(m, meps)
        assert np.array_equal(mk[0], plain[0] * g) and np.array_equal(mk[1], plain[1] * g)
    assert (m < 0.3).any()


# (masking_eps is compared in the mask's dtype, as TorchBF's clamp does: 0.25 is the same number in float32 and float64)
CASES = dict(plain=dict(), forgetting=dict(forgetting=0.9), masking=dict(masking=True, masking_eps=0.25))


def gpu_case(D, name, T=7, F=70, B=2, K=3):
    """A case of tests/test_gpu_online_mvdr.py: the inputs (Y with complex64 values, masks with float32 values, so that
    every input type of the kernel sees the same numbers), the keywords, the extended reference and the yardsticks
    (output, state) -> Y, masks, kw, ref, yardsticks"""
    Y, m = array_inputs(D, T, F, seed=40 + D, B=B, K=K)
    Y = Y.astype(np.complex64).astype(np.complex128)
    m = m.astype(np.float32).astype(np.float64)
    kw = dict(ref=1 if D > 1 else 0, diag_load=1e-3, **CASES[name])
    ref = online_reference(Y, m, extended=True, **kw)
    return Y, m, kw, ref, yardsticks(online_reference(Y, m, extended=False, **kw), ref)


def held(enh, state, ref, ys, what):
    """The comparison of the GPU test: (enh, state) within FACTOR x the yardsticks of the extended run -> the two ratios"""
    eo, es = errors(enh, state, ref)
    ro, rs = eo / ys[0], es / ys[1]
    print(f"{what}: output {eo:.3g} = {ro:.3g} x the yardstick {ys[0]:.3g}; state {es:.3g} = {rs:.3g} x {ys[1]:.3g}")
    return ro, rs


@pytest.mark.parametrize("D", (2, 6, 7))
def test_yardsticks_are_finite_and_planted_defects_exceed_them(D):
    """On the GPU test's own inputs (fewer bins here) the float64 run's distances from the extended one are finite and
    not zero, and each planted defect lies beyond FACTOR x a yardstick, in the output or in the state."""
    Y, m, kw, ref, ys = gpu_case(D, "forgetting", F=12)
    print(f"D={D}: yardsticks (float64 against extended) output {ys[0]:.3g}, state {ys[1]:.3g}")
    assert 0 < ys[0] < 1e-6 and 0 < ys[1] < 1e-14, ys
    for defect in DEFECTS:
        bad = online_reference(Y, m, extended=False, defect=defect, **kw)
        ro, rs = held(xcf(bad[0]), packed_state(bad[1]), ref, ys, f"  {defect}")
        assert max(ro, rs) > FACTOR, (defect, ro, rs)
        assert (rs > FACTOR) == (defect == "alpha_after") and (ro > FACTOR) == (defect != "alpha_after"), (defect, ro, rs)


# ---- refusals: CPU tensors, nothing is launched ----------------------------------------------------------------------
def _cpu_args(D=3, K=2, T=4, F=5, M=None):
    masks = torch.rand(1, K, T, F) if M is None else torch.rand(1, K, M, T, F)
    return masks, torch.randn(1, D, T, F, dtype=torch.complex64)


def test_online_mvdr_refusals():
    from tssep_amd import hip_ops
    masks, Y = _cpu_args(M=2)
    with pytest.raises(NotImplementedError, match="nmask = 2"):
        hip_ops.online_mvdr(masks, Y)
    masks, Y = _cpu_args()
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="forgetting"):
            hip_ops.online_mvdr(masks, Y, forgetting=bad)
    with pytest.raises(ValueError, match="diag_load"):
        hip_ops.online_mvdr(masks, Y, diag_load=-1e-6)
    with pytest.raises(ValueError, match="differ"):
        hip_ops.online_mvdr(masks, Y[..., :4])
    with pytest.raises(ValueError, match="state"):                               # the state of a 2-channel stream
        hip_ops.online_mvdr(masks, Y, state=torch.zeros(1, 2, 2, 4, 5, dtype=torch.float64))
    with pytest.raises(ValueError, match="reference_channel"):
        hip_ops.online_mvdr(masks, Y, reference_channel=3)
    with pytest.raises(ValueError, match="8 channels"):
        hip_ops.online_mvdr(*_cpu_args(D=9))
    with pytest.raises(TypeError):
        hip_ops.online_mvdr(masks, Y.real)


def test_enhancer_refuses_gradients_and_two_masks():
    from tssep_amd.train import enhancer
    bf = enhancer.OnlineMVDR()
    assert (bf.forgetting, bf.diag_load, bf.eps, bf.masking, bf.masking_eps) == (1.0, 1e-6, None, False, 0.0)
    masks, Y = _cpu_args(M=1)
    with pytest.raises(NotImplementedError, match="evaluation-time"):
        bf(masks.requires_grad_(), {"Observation": Y, "reference_channel": 0}, None)
    masks, Y = _cpu_args(M=2)
    with pytest.raises(NotImplementedError, match="nmask = 2"), torch.no_grad():
        bf(masks, {"Observation": Y, "reference_channel": 0}, None)
    with pytest.raises(ValueError, match="forgetting"), torch.no_grad():
        enhancer.OnlineMVDR(forgetting=0.0)(_cpu_args(M=1)[0], {"Observation": Y, "reference_channel": 0}, None)


def _model(enh):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import feature_extractor as fe, loss, model, net
    f = fe.ConcaternatedSTFTFeatures(
        fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True), size=1024, shift=256, window="hann")
    me = net.MaskEstimator_v2(combination="mul", ts_vad=3, rnn_typ="lstm", random_speaker_order=False, idim=553, odim=513,
                              units=8, projs=12, layers=3)
    return model.Model(fe=f, reader=DummyReader(), mask_estimator=me, enhancer=enh, loss=loss.LogMAE())


def test_model_online_accepts_online_mvdr_only():
    from tssep_amd.train import enhancer, online
    aux = torch.zeros(2, 3, 513)
    with pytest.raises(NotImplementedError, match="only Masking has a streaming tail"):
        _model(enhancer.TorchBF()).online(aux)
    sep = _model(enhancer.OnlineMVDR(forgetting=0.95)).online(aux, reference_channel=2)
    assert isinstance(sep, online.OnlineSeparator) and sep._ref == 2 and sep._bf.forgetting == 0.95
    assert _model(enhancer.Masking()).online(aux)._bf is None
    with pytest.raises(ValueError, match=r"\[B, D, n\]"):
        sep.push(torch.zeros(2, 256))


def test_toy_overlay_resolves():
    import os
    from tssep_amd.train import enhancer, online, run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
    yamls = ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_online_mvdr.yaml")
    cfg = run.build_config([os.path.join(exp, y) for y in yamls] + ["eg.trainer.storage_dir=/tmp/unused"])
    model = Experiment.from_config(cfg["eg"]).trainer.model
    assert isinstance(model.enhancer, enhancer.OnlineMVDR) and model.enhancer.diag_load == 1e-6
    assert model.fe.causal and model.mask_estimator.rnn_typ == "lstm" and model.mask_estimator.nmask == 1
    assert isinstance(model.online(torch.zeros(1, 4, 513), reference_channel=1), online.OnlineSeparator)
