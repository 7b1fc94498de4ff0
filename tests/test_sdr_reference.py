"""CPU checks of the SDR / SI-SDR reference (tests/sdr_reference.py) and of the host side of tssep_amd.train.loss.SDR:
the closed-form gradient against float64 autograd of the plain formula, the invariances and limiting values, planted
defects that the shared checkers must catch at the bounds they use, and what constructs or is refused."""
import os

import numpy as np
import pytest
import torch

import pit_reference as PR
import sdr_reference as R

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
LEVELS = (-10, 0, 20, 40)
MODES = [(True, None), (True, 30.0), (False, None), (False, 30.0)]
Q3 = np.array([[1, 2, 0], [2, 0, 1]])          # 3-cycles: the inverse differs from the permutation


def _take(t, q):
    return np.take_along_axis(t, np.asarray(q)[..., None], axis=1)


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("scale_invariant,sdr_max", MODES)
@pytest.mark.parametrize("level", LEVELS)
def test_closed_form_gradient_against_float64_autograd(scale_invariant, sdr_max, level):
    est, tgt = R.planted(2, 3, 500, level, seed=level + 100)
    tgt = _take(tgt, R.PR.inverse(Q3))                  # est row i belongs to tgt row Q3[b, i]
    gout = np.array([0.7, -1.3])
    eps = 1e-6
    value, lo, want = R.autograd(est, tgt, Q3, scale_invariant, sdr_max, eps, gout)
    got, _ = R.grad(est, tgt, Q3, scale_invariant, sdr_max, eps, gout)
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max()
    ref = R.loss(est, tgt, scale_invariant, sdr_max, eps, pit=True)
    assert np.array_equal(ref["perm"], Q3)
    assert np.allclose(ref["values"], value, rtol=0, atol=1e-9) and np.allclose(ref["loss"], lo, rtol=0, atol=1e-9)
    want_level = level if sdr_max is None else -10 * np.log10(10 ** (-level / 10) + 10 ** (-sdr_max / 10))
    assert np.all(np.abs(value - want_level) < 1e-2), (value, want_level)      # (the planted level itself)


def test_invariances_and_limiting_values():
    est, tgt = R.planted(2, 2, 400, 7.0, seed=3)
    eps = 1e-8
    pv = R.pair_values(R.stats(est, tgt), True, None, eps)
    v, v3 = pv["value"], R.pair_values(R.stats(3.0 * est.astype(np.float64), tgt), True, None, eps)["value"]
    # e -> 3 e, scale-invariant: s and D scale by 9, so only the two eps terms move the value
    assert np.all(np.abs(v - v3) <= R.LOG * eps * (1 / pv["s"] + 1 / pv["D"]) + 1e-9)
    assert np.abs(v - v3)[:, np.eye(2, dtype=bool)].max() < 1e-8
    p = R.pair_values(R.stats(tgt, tgt), False, None, 1.0)      # (eps = 1: far above the float64 residue of a - 2 c + b)
    b = R.stats(tgt, tgt)["b"]
    eye = np.eye(2, dtype=bool)
    assert np.allclose(p["value"][:, eye], 10 * np.log10((b + 1.0) / 1.0), rtol=0, atol=1e-9)      # e = t, plain
    for si in (True, False):
        for e in (est, tgt, 100 * tgt):
            assert np.all(R.pair_values(R.stats(e, tgt), si, 20.0, eps)["value"] < 20.0)   # under sdr_max
    silent = np.zeros_like(tgt)
    for si in (True, False):
        a = R.stats(est, silent)["a"][:, :, None]
        got = R.pair_values(R.stats(est, silent), si, None, eps)["value"]
        assert np.all(np.isfinite(got)) and np.allclose(got, 10 * np.log10(eps / (a + eps)), rtol=1e-12)
        both = R.pair_values(R.stats(silent, silent), si, None, eps)
        assert np.all(both["value"] == 0)
        dest, _ = R.grad(est, silent, np.tile(np.arange(2), (2, 1)), si, None, eps)
        assert np.all(np.isfinite(dest)) and np.all(dest * est >= 0)       # pushes the estimate's energy down


def test_nan_is_not_swallowed_by_the_clamp():
    est, tgt = R.planted(1, 2, 50, 5.0, seed=1)
    est[0, 1, 7] = np.nan
    for si in (True, False):
        v = R.pair_values(R.stats(est, tgt), si, None, 1e-8)["value"]
        assert np.isnan(v[0, 1]).all() and np.isfinite(v[0, 0]).all()


# ------------------------------------------------------------------------------------------------ planted defects
def _f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("scale_invariant,sdr_max", [(True, 30.0), (False, 30.0)])
@pytest.mark.parametrize("level", LEVELS)
def test_checkers_catch_planted_defects(scale_invariant, sdr_max, level):
    """Each defect is applied to the float64 reference itself (rounded to float32 as the kernels' outputs are), so the
    defect is all that separates it from what the checker expects; the clean reference must pass the same checker."""
    B, K, N = 2, 3, 4099
    est, tgt = R.planted(B, K, N, level, seed=7 * level + 150)
    tgt = _take(tgt, PR.inverse(Q3))
    eps = 1e-2 * float((tgt.astype(np.float64) ** 2).sum(-1).min())       # (an eps that matters: alpha without it differs)
    gout = np.array([1.0, -0.5])
    ref = R.loss(est, tgt, scale_invariant, sdr_max, eps, pit=True)
    assert np.array_equal(ref["perm"], Q3) and np.all(ref["gap"] > 4 * K * ref["dvalue"].max() / K)
    clean, _ = R.grad(est, tgt, Q3, scale_invariant, sdr_max, eps, gout)
    R.check_values(_f32(ref["value"]), _f32(ref["cost"]), ref)
    R.check_backward(_f32(clean), est, tgt, Q3, scale_invariant, sdr_max, eps, gout)

    def caught(fn):
        with pytest.raises(AssertionError, match="outside the bound"):
            fn()

    # 1 / K dropped: cost = -value, and the gradient K times as large
    caught(lambda: R.check_values(_f32(ref["value"]), _f32(-ref["value"]), ref))
    caught(lambda: R.check_backward(_f32(R.grad(est, tgt, Q3, scale_invariant, sdr_max, eps, gout, inv_k=False)[0]),
                                    est, tgt, Q3, scale_invariant, sdr_max, eps, gout))
    # the permutation applied in the inverse direction
    caught(lambda: R.check_backward(_f32(R.grad(est, tgt, Q3, scale_invariant, sdr_max, eps, gout, inverse_perm=True)[0]),
                                    est, tgt, Q3, scale_invariant, sdr_max, eps, gout))
    if scale_invariant:
        # tau missing from the gradient: Q without its factor (1 - tau)
        caught(lambda: R.check_backward(_f32(R.grad(est, tgt, Q3, True, sdr_max, eps, gout, tau_in_gradient=False)[0]),
                                        est, tgt, Q3, True, sdr_max, eps, gout))
        # alpha = c / b, without eps
        bad = R.pair_values(ref["stats"], True, sdr_max, eps, alpha_eps=False)["value"]
        caught(lambda: R.check_values(_f32(bad), _f32(-bad / K), ref))
        caught(lambda: R.check_backward(_f32(R.grad(est, tgt, Q3, True, sdr_max, eps, gout, alpha_eps=False)[0]),
                                        est, tgt, Q3, True, sdr_max, eps, gout))
    else:
        # tau missing from the plain gradient: D without tau s
        no_tau, _ = R.grad(est, tgt, Q3, False, None, eps, gout)
        caught(lambda: R.check_backward(_f32(no_tau), est, tgt, Q3, False, sdr_max, eps, gout))


def _emulate_row_stats(x, y, tree):
    """sum x y as the statistics kernel forms it on its 16-byte path, on the CPU: per chunk of 8192 samples lane l owns the
    samples 1024 it + 4 l + q and chains them in float32 (fused multiply-add: the product exact, one rounding per add);
    then the xor butterfly over the 64 lanes of a wave, (w0 + w1) + (w2 + w3), and the chunks in ascending order -- in
    `tree` (float64: the kernel; float32: the planted defect)."""
    n = len(x)
    nch = -(-n // R.CHUNK)
    X = np.zeros(nch * R.CHUNK, dtype=np.float32)
    Y = np.zeros_like(X)
    X[:n], Y[:n] = x, y
    X, Y = (v.reshape(nch, R.CHUNK // 1024, 256, 4).astype(np.float64) for v in (X, Y))
    acc = np.zeros((nch, 256), dtype=np.float32)
    for it in range(R.CHUNK // 1024):
        for q in range(4):
            acc = (acc.astype(np.float64) + X[:, it, :, q] * Y[:, it, :, q]).astype(np.float32)
    v = acc.astype(tree).reshape(nch, 4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, :, lanes ^ o]).astype(tree)
    w = v[:, :, 0]
    part = ((w[:, 0] + w[:, 1]).astype(tree) + (w[:, 2] + w[:, 3]).astype(tree)).astype(tree)
    s = tree(0)
    for c in range(nch):
        s = tree(s + part[c])
    return float(s)


def test_float32_chunk_sums_are_caught_at_40_db():
    """One loud chunk in front of 63 quiet ones, est at 40 dB: in float64 the statistics sit inside the bound of the 32
    float32 roundings of the lane chain; with float32 partials and a float32 chunk loop every quiet chunk falls below half
    an ulp of the running sum and is lost -- 63 roundings in one direction, which the bound of 32 does not cover."""
    rng = np.random.RandomState(40)
    nch = 64
    t = rng.randn(nch * R.CHUNK)
    loud = (t[:R.CHUNK] ** 2).sum()
    t[:R.CHUNK] *= np.sqrt(1.05 * 2.0 ** 20 / loud)
    for c in range(1, nch):                                  # each quiet chunk: 0.9 of half an ulp of 2^20 ... 2^21
        seg = t[c * R.CHUNK:(c + 1) * R.CHUNK]
        seg *= np.sqrt(0.9 * 0.0625 / (seg ** 2).sum())
    noise = rng.randn(len(t)) * np.abs(t)
    noise -= (noise * t).sum() / (t * t).sum() * t
    noise *= np.sqrt((t * t).sum() / (noise * noise).sum()) * 1e-2
    est, tgt = (t + noise).astype(np.float32)[None, None], t.astype(np.float32)[None, None]
    st = R.stats(est, tgt)
    level = R.pair_values(st, True, None, 1e-8)["value"][0, 0, 0]
    assert abs(level - 40) < 0.1, level
    e, g = est[0, 0], tgt[0, 0]
    emulate = lambda tree: np.array([[_emulate_row_stats(e, g, tree), _emulate_row_stats(e, e, tree),      # noqa: E731
                                      _emulate_row_stats(g, g, tree)]])
    worst = R.check_stats(emulate(np.float64), st)
    assert worst < 1
    with pytest.raises(AssertionError, match="statistics.*outside the bound"):
        R.check_stats(emulate(np.float32), st)


# ------------------------------------------------------------------------------------------------ host behaviour
def test_constructor_and_refusals():
    from tssep_amd.train import loss
    lo = loss.SDR()
    assert isinstance(lo, loss.TimeDomain) and lo.name == "SDR" and not lo.fused_tail and not loss.SDR(pit=True).fused_tail
    assert (lo.pit, lo.scale_invariant, lo.sdr_max, lo.eps) == (False, True, None, 1e-8)
    assert lo.permutation is None and lo.values is None
    assert lo.targets() == ("speaker_reverberation_early_ch0",) and loss.SDR(target="x").targets() == ("x",)
    assert loss.SDR(sdr_max=30).sdr_max == 30.0 and loss.SDR(scale_invariant=False).scale_invariant is False
    for eps in (0.0, -1e-8, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            loss.SDR(eps=eps)
    for sdr_max in (float("inf"), float("-inf"), float("nan"), "30"):
        with pytest.raises(ValueError, match="sdr_max"):
            loss.SDR(sdr_max=sdr_max)


def test_more_than_eight_speakers_are_refused_before_any_launch():
    """K = 9 raises in Python, on CPU tensors: no kernel, no library call."""
    from tssep_amd import functional as Fn, hip_ops as H
    from tssep_amd.train import loss
    e = torch.zeros(2, 9, 16)
    for lo in (loss.SDR(), loss.SDR(pit=True), loss.SDR(scale_invariant=False)):
        with pytest.raises(NotImplementedError, match="8"):
            lo(e, e)
        with pytest.raises(NotImplementedError, match="8"):
            lo(e[0], e[0])
    for fn in (lambda: Fn.sdr_loss(e, e), lambda: H.sdr(e, e), lambda: H.sdr_stats_fwd(e, e),
               lambda: H.sdr_cost(torch.zeros(2, 1, 99, dtype=torch.float64), 9),
               lambda: H.sdr_bwd(e, e, None, torch.zeros(2, 99, dtype=torch.float64), torch.ones(2))):
        with pytest.raises(NotImplementedError, match="8"):
            fn()
    with pytest.raises(AssertionError):
        loss.SDR()(torch.zeros(2, 3, 16), torch.zeros(2, 3, 15))


def test_config_round_trip_and_overlay(tmp_path):
    from tssep_amd import configurable
    from tssep_amd.train import loss, run
    from tssep_amd.train.experiment import Experiment
    assert configurable.resolve("tssep.train.loss.SDR") is loss.SDR
    assert configurable.factory_path(loss.SDR) == "tssep.train.loss.SDR"
    cfg = loss.SDR.get_config({"pit": True, "sdr_max": 25.0})
    assert cfg == {"factory": "tssep.train.loss.SDR", "target": "speaker_reverberation_early_ch0", "pit": True,
                   "scale_invariant": True, "sdr_max": 25.0, "eps": 1e-8}
    lo = configurable.Configurable.from_config(cfg)
    assert isinstance(lo, loss.SDR) and lo.pit is True and lo.sdr_max == 25.0
    full = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_sdr.yaml")]
                            + [f"eg.trainer.storage_dir={tmp_path}"])
    m = Experiment.from_config(full["eg"]).trainer.model
    assert isinstance(m.loss, loss.SDR) and m.loss.pit is False and m.loss.scale_invariant and m.loss.sdr_max == 30.0
    assert not m.loss.fused_tail and m.loss.targets() == ("speaker_reverberation_early_ch0",)


def test_joint_loss_takes_sdr_and_refuses_its_pit():
    from tssep_amd.train import loss
    lo = loss.SignalAndVADSigmoidBCE(signal_loss=loss.SDR(target="x", sdr_max=30.0))
    assert lo.targets() == ("Vad", "x") and isinstance(lo.signal_loss, loss.SDR) and not lo.signal_loss.fused_tail
    with pytest.raises(NotImplementedError, match="permutation"):
        loss.SignalAndVADSigmoidBCE(signal_loss=loss.SDR(pit=True))
