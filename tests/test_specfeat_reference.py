"""The float64 definitions and bounds of tests/specfeat_reference.py, and the host side of the spectral features
(AbsSTFT, Log1pAbsSTFT, MVNLog1pAbsSTFT, NoFeatureSTFT), without a device: the definitions against closed
forms, the running mean against the whole-utterance mean, the checker on the float32 restatement (which must pass) and on
seven planted defects (each of which must fail, at shapes of the GPU file where the defect changes anything at all: T >= 2,
F >= 2, a state in front), then constructor keywords, errors, config round trips and the ABI."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import specfeat_reference as R

DOCTEST = np.array([[1, 5], [3 + 4j, -5]], dtype=np.complex64)        # feature_extractor.py:117-122
LN2, LN3, LN6 = math.log(2.0), math.log(3.0), math.log(6.0)
FE = "tssep.train.feature_extractor."


# ---- definitions -----------------------------------------------------------------------------------------------------------
def test_definitions_against_closed_forms():
    np.testing.assert_allclose(R.abs_feature(DOCTEST), [[1, 5], [5, 5]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(R.log1p_abs_feature(DOCTEST), [[LN2, LN6], [LN6, LN6]], rtol=0, atol=1e-15)
    np.testing.assert_allclose(R.mvn_feature(DOCTEST), [[-LN3 / 2, 0], [LN3 / 2, 0]], rtol=0, atol=1e-15)
    # the reference's doctest output as printed (8 digits)
    np.testing.assert_allclose(R.mvn_feature(DOCTEST), [[-0.54930614, 0.0], [0.54930614, 0.0]], rtol=0, atol=5e-9)


def test_causal_against_whole_utterance_and_chunked():
    X = R.make_input(3, 70, 5, seed=1)
    out, S, n = R.mvn_causal_feature(X)
    assert np.all(out[:, 0] == 0) and np.all(n == 70)
    np.testing.assert_allclose(out[:, -1], R.mvn_feature(X)[:, -1], rtol=0, atol=1e-12)
    for alpha in (1.0, 0.97):
        whole = R.mvn_causal_feature(X, forgetting=alpha)
        for split in ((70,), (1,) * 70, (1, 1, 3, 65), (64, 6)):
            S_, n_, pos, outs = None, None, 0, []
            for c in split:
                o, S_, n_ = R.mvn_causal_feature(X[:, pos:pos + c], S_, n_, alpha)
                outs.append(o)
                pos += c
            assert np.array_equal(np.concatenate(outs, axis=1), whole[0])
            assert np.array_equal(S_, whole[1]) and np.array_equal(n_, whole[2])
    # the weight with forgetting: the geometric sum
    np.testing.assert_allclose(R.mvn_causal_feature(X, forgetting=0.97)[2], (1 - 0.97 ** 70) / 0.03, rtol=1e-12)


# ---- the checker -----------------------------------------------------------------------------------------------------------
SHAPES = [(B, T, F) for B in R.BS for T in R.TS for F in R.FS]


def test_restatement_passes_every_bound():
    w = dict(abs=0.0, log1p=0.0, mvn=0.0, causal=0.0, causal97=0.0)
    for B, T, F in SHAPES:
        X = R.make_input(B, T, F)
        w["abs"] = max(w["abs"], R.worst(R.restatement32(X, "abs"), R.abs_feature(X), R.abs_bound(X)))
        w["log1p"] = max(w["log1p"], R.worst(R.restatement32(X, "log1p"), R.log1p_abs_feature(X), R.log1p_bound(X)))
        w["mvn"] = max(w["mvn"], R.worst(R.restatement32(X, "mvn"), R.mvn_feature(X), R.mvn_bound(X)))
        for key, alpha in (("causal", 1.0), ("causal97", 0.97)):
            got = R.restatement32(X, "causal", forgetting=alpha)
            ref = R.mvn_causal_feature(X, forgetting=alpha)
            w[key] = max(w[key], R.worst(got[0], ref[0], R.mvn_causal_bound(X, forgetting=alpha)))
            np.testing.assert_allclose(got[1], ref[1], rtol=2 * R.C1 * R.U, atol=R.TINY)
            np.testing.assert_allclose(got[2], ref[2], rtol=1e-13)
    print("restatement32, worst error / bound:", {k: round(v, 3) for k, v in w.items()})
    assert all(0.0 < v <= 1.0 for v in w.values()), w


def _state(X0, alpha):
    _, S, n = R.mvn_causal_feature(X0, forgetting=alpha)
    return S, n


@pytest.mark.parametrize("defect", ["mean_f", "next_frame", "count", "forget_S_only", "log", "drop_state"])
def test_planted_defects_are_refused(defect):
    B, T, F = 3, 70, 5
    X0, X = R.make_input(B, 9, F, seed=2), R.make_input(B, T, F)
    alpha = 0.97
    S, n = _state(X0, alpha)
    if defect == "mean_f":
        good, bad = R.restatement32(X, "mvn"), R.restatement32(X, "mvn", defect=defect)
        ref, bound = R.mvn_feature(X), R.mvn_bound(X)
    elif defect == "log":
        good, bad = R.restatement32(X, "log1p"), R.restatement32(X, "log1p", defect=defect)
        ref, bound = R.log1p_abs_feature(X), R.log1p_bound(X)
    else:
        good = R.restatement32(X, "causal", S, n, alpha)[0]
        bad = R.restatement32(X, "causal", S, n, alpha, defect=defect)[0]
        ref, bound = R.mvn_causal_feature(X, S, n, alpha)[0], R.mvn_causal_bound(X, S, n, alpha, frames_before=9)
    assert R.worst(good, ref, bound) <= 1.0
    assert R.worst(bad, ref, bound) > 1.0, defect
    with pytest.raises(AssertionError, match="worst error / bound"):
        R.held(bad, ref, bound, defect)


def test_float32_running_sum_is_refused_at_200000_frames():
    """one (b, f), 2 10^5 frames of L ~ 1: the float64 chain passes, the float32 sum leaves the bound"""
    rng = np.random.RandomState(5)
    X = (rng.uniform(0.5, 4.0, size=(1, 200_000, 1)) * np.exp(2j * np.pi * rng.uniform(size=(1, 200_000, 1)))).astype(np.complex64)
    ref, bound = R.mvn_causal_feature(X)[0], R.mvn_causal_bound(X)
    assert R.worst(R.restatement32(X, "causal")[0], ref, bound) <= 1.0
    assert R.worst(R.restatement32(X, "causal", defect="sum32")[0], ref, bound) > 1.0


def test_worst_refuses_nan_and_shape():
    X = R.make_input(1, 2, 5)
    ref, bound = R.abs_feature(X), R.abs_bound(X)
    got = R.restatement32(X, "abs").copy()
    assert R.worst(got, ref, bound) <= 1.0 and R.worst(got[:, :1], ref, bound) == float("inf")
    got[0, 0, 0] = np.nan
    assert R.worst(got, ref, bound) == float("inf")


# ---- host logic ------------------------------------------------------------------------------------------------------------
def test_constructor_keywords_and_output_size():
    from tssep_amd.train import feature_extractor as fe
    base = ["size", "shift", "window_length", "pad", "fading", "output_size", "window"]
    want = {fe.AbsSTFT: base + ["causal"], fe.Log1pAbsSTFT: base + ["causal"],
            fe.MVNLog1pAbsSTFT: base + ["norm_means", "norm_vars", "eps", "causal", "forgetting"],
            fe.NoFeatureSTFT: base + ["causal"]}
    for cls, names in want.items():
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[1:] == names, (cls, list(p))
        assert p["window"].default == "blackman" and p["causal"].default is False and p["size"].default == 1024
    p = inspect.signature(fe.MVNLog1pAbsSTFT.__init__).parameters
    assert (p["norm_means"].default, p["norm_vars"].default, p["eps"].default, p["forgetting"].default) == (True, False, 1e-20, 1.0)
    for cls in (fe.AbsSTFT, fe.Log1pAbsSTFT, fe.MVNLog1pAbsSTFT):
        assert cls().output_size == 513 and cls(size=512, shift=128).output_size == 257 and cls(output_size=7).output_size == 7
        assert cls().causal is False and cls(causal=True).causal is True
    assert issubclass(fe.MVNLog1pAbsSTFT, fe.Log1pAbsSTFT) and issubclass(fe.Log1pAbsSTFT, fe.AbsSTFT)
    assert fe.NoFeatureSTFT().output_size == 0 and fe.NoFeatureSTFT(output_size=0).output_size == 0
    with pytest.raises(AssertionError):
        fe.NoFeatureSTFT(output_size=513)
    X = torch.zeros(2, 3, 513, dtype=torch.complex64)
    assert tuple(fe.NoFeatureSTFT().stft_to_feature(X).shape) == (2, 3, 0)


def test_errors_without_a_device():
    from tssep_amd.train import feature_extractor as fe
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="forgetting"):
            fe.MVNLog1pAbsSTFT(causal=True, forgetting=bad)
    with pytest.raises(ValueError, match="causal=True"):
        fe.MVNLog1pAbsSTFT(forgetting=0.99)
    assert fe.MVNLog1pAbsSTFT(causal=True, forgetting=0.99).forgetting == 0.99
    X = torch.zeros(2, 3, 513, dtype=torch.complex64)
    for cls in (fe.AbsSTFT, fe.Log1pAbsSTFT, fe.MVNLog1pAbsSTFT):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cls().stft_to_feature(X)
        with pytest.raises(RuntimeError, match="at most 1025"):
            cls(size=2052, shift=256)
    # the reference's errors, at the call (feature_extractor.py:160-166), before anything touches a device
    Xm = X.to("meta")
    for kw in (dict(norm_vars=True), dict(norm_means=False)):
        m = fe.MVNLog1pAbsSTFT(**kw)                   # (constructing is fine, as in the reference)
        with pytest.raises(NotImplementedError):
            m._feature(Xm, None)
    from tssep_amd import hip_ops as H
    with pytest.raises(ValueError, match=r"float32 \(2, 514\)"):
        H.specfeat_causal_state_check(torch.zeros(2, 514), 2, 513)
    with pytest.raises(ValueError, match=r"float64 \(2, 2\)"):
        H.specfeat_causal_state_check(torch.zeros(2, 2, dtype=torch.float64), 2, 513)
    H.specfeat_causal_state_check(torch.zeros(2, 514, dtype=torch.float64), 2, 513)
    H.specfeat_causal_state_check(None, 2, 513)


@pytest.mark.parametrize("name", ["AbsSTFT", "Log1pAbsSTFT", "MVNLog1pAbsSTFT", "NoFeatureSTFT"])
def test_configurable_round_trips(name):
    from tssep_amd.configurable import Configurable
    from tssep_amd.train import feature_extractor as fe
    cfg = Configurable.get_config({"factory": FE + name, "window": "hann"})
    assert cfg["factory"] == FE + name and cfg["window"] == "hann" and cfg["causal"] is False
    obj = Configurable.from_config(cfg)
    assert type(obj) is getattr(fe, name) and obj.window == "hann"
    assert Configurable.get_config(cfg) == cfg
    # as fe2 of the concatenation: the STFT options and `causal` reach both parts
    extra = {"forgetting": 0.999} if name == "MVNLog1pAbsSTFT" else {}
    cfg = Configurable.get_config({"factory": FE + "ConcaternatedSTFTFeatures", "window": "hann", "causal": True,
                                   "fe1": {"factory": FE + "TorchMFCC"}, "fe2": {"factory": FE + name, **extra}})
    assert cfg["fe2"]["factory"] == FE + name and cfg["fe2"]["causal"] is True and cfg["fe1"]["causal"] is True
    assert cfg["fe2"]["window"] == "hann" and cfg["fe1"]["size"] == 1024
    cat = Configurable.from_config(cfg)
    assert type(cat.fe2) is getattr(fe, name) and cat.causal is True and cat.fe2.causal is True
    assert cat.output_size == 40 + (0 if name == "NoFeatureSTFT" else 513)
    if extra:
        assert cat.fe2.forgetting == 0.999


def test_toy_overlays_resolve():
    import os
    from tssep_amd.train import feature_extractor as fe, run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
    for overlay, causal, alpha in (("toy_tssep_mvn.yaml", False, 1.0), ("toy_tssep_online_mvn.yaml", True, 0.999)):
        yamls = ("toy_common.yaml", "toy_tssep.yaml", overlay)
        cfg = run.build_config([os.path.join(exp, y) for y in yamls] + ["eg.trainer.storage_dir=/tmp/unused"])
        c2 = cfg["eg"]["trainer"]["model"]["fe"]["fe2"]
        assert c2["factory"] == FE + "MVNLog1pAbsSTFT" and "statistics_axis" not in c2 and c2["window"] == "hann"
        model = Experiment.from_config(cfg["eg"]).trainer.model
        obj = model.fe
        assert type(obj.fe2) is fe.MVNLog1pAbsSTFT and type(obj.fe1) is fe.TorchMFCC
        assert obj.causal is causal and obj.fe2.causal is causal and obj.fe1.causal is causal
        assert obj.fe2.forgetting == alpha and obj.output_size == 553 and obj.fe2.window == "hann"
        assert (model.mask_estimator.rnn_typ == "lstm") is causal
        if causal:
            assert model.online(torch.zeros(1, 4, 513)).fe is obj
    # the rule that drops toy_common.yaml's `statistics_axis` leaves every key the new class takes, and touches nothing when
    # the factory stays
    dst = {"a": {"factory": FE + "Log1pMaxNormAbsSTFT", "size": 512, "statistics_axis": "tf"}}
    run._deep_update(dst, {"a": {"factory": FE + "MVNLog1pAbsSTFT"}})
    assert dst["a"] == {"factory": FE + "MVNLog1pAbsSTFT", "size": 512}
    dst = {"a": {"factory": FE + "Log1pMaxNormAbsSTFT", "bogus": 1}}
    run._deep_update(dst, {"a": {"factory": FE + "Log1pMaxNormAbsSTFT", "size": 512}})
    assert dst["a"] == {"factory": FE + "Log1pMaxNormAbsSTFT", "bogus": 1, "size": 512}


def test_entry_points_declared_exported_and_wrapped():
    from tssep_amd import _lib, hip_ops
    protos = _lib.parse_header()
    assert len(protos["tssep_specfeat_workspace_bytes"][1]) == 4 and protos["tssep_specfeat_workspace_bytes"][0] is ctypes.c_int64
    assert len(protos["tssep_specfeat_fwd"][1]) == 9 and len(protos["tssep_specfeat_causal_fwd"][1]) == 10
    assert protos["tssep_specfeat_causal_fwd"][1][4] is ctypes.c_double
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("tssep_specfeat_workspace_bytes", "tssep_specfeat_fwd", "tssep_specfeat_causal_fwd"):
        assert hasattr(dll, name), name
    assert dll.tssep_abi_version() == 4
    assert "tssep_specfeat_fwd" in inspect.getsource(hip_ops.specfeat_fwd)
    assert "tssep_specfeat_causal_fwd" in inspect.getsource(hip_ops.specfeat_causal_fwd)
    assert list(inspect.signature(hip_ops.specfeat_fwd).parameters) == ["X", "kind", "out", "col0"]
    assert list(inspect.signature(hip_ops.specfeat_causal_fwd).parameters) == ["X", "state", "forgetting", "out", "col0"]


def test_guards_return_before_any_launch():
    """Shape, kind, forgetting, overlap and alignment guards answer on the arguments alone: no device is touched."""
    from tssep_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p
    SHAPE, ALIGN, UNSUP, NULL = -1, -2, -3, -5
    assert L.tssep_specfeat_workspace_bytes(3, 70, 513, 2) == 3 * 513 * 8
    assert L.tssep_specfeat_workspace_bytes(3, 70, 513, 0) == 0 and L.tssep_specfeat_workspace_bytes(3, 70, 513, 1) == 0
    assert L.tssep_specfeat_workspace_bytes(3, 70, 1026, 2) == 0
    fwd = lambda B, T, F, kind, ld, X=64, out=64, ws=64: L.tssep_specfeat_fwd(p(X), B, T, F, kind, p(out), ld, p(ws), None)
    assert fwd(1, 1, 1026, 1, 1026) == SHAPE and fwd(1, 0, 5, 1, 5) == SHAPE and fwd(0, 1, 5, 1, 5) == SHAPE
    assert fwd(1, 1, 0, 1, 5) == SHAPE and fwd(1, 2, 5, 1, 4) == SHAPE
    assert fwd(1, 2, 5, 3, 5) == UNSUP and fwd(1, 2, 5, -1, 5) == UNSUP
    assert fwd(1, 2, 5, 1, 5, X=None) == NULL and fwd(1, 2, 5, 2, 5, ws=None) == NULL
    assert fwd(1, 2, 5, 1, 5, X=68) == ALIGN and fwd(1, 2, 5, 1, 5, out=66) == ALIGN and fwd(1, 2, 5, 2, 5, ws=68) == ALIGN
    assert fwd(1 << 40, 2, 5, 1, 5) == SHAPE and fwd(4, 1 << 40, 1025, 1, 1025) == SHAPE       # (the grids)
    cz = lambda B, T, F, a, si, so, ld=None, out=64: L.tssep_specfeat_causal_fwd(p(64), B, T, F, a, p(si), p(so), p(out),
                                                                                  F if ld is None else ld, None)
    assert cz(1, 0, 5, 1.0, None, None) == SHAPE and cz(1, 1, 1026, 1.0, None, None) == SHAPE
    for a in (0.0, -1.0, 1.0 + 1e-12, float("nan")):
        assert cz(1, 1, 5, a, None, None) == SHAPE
    nb = 2 * 6 * 8
    assert cz(2, 1, 5, 1.0, 4096, 4096) == SHAPE and cz(2, 1, 5, 1.0, 4096, 4096 + nb - 8) == SHAPE
    assert cz(2, 1, 5, 1.0, 4096 + nb - 8, 4096) == SHAPE
    assert cz(2, 1, 5, 1.0, 4100, None) == ALIGN and cz(2, 1, 5, 1.0, None, 4100) == ALIGN
    assert cz(2, 1, 5, 1.0, None, None, out=66) == ALIGN and cz(2, 1, 5, 1.0, None, None, ld=4) == SHAPE
