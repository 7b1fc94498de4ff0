"""The online path without a GPU: the causal statistics' defining property against the oracle, the
tail-carrying STFT and the carry-first inverse against oracle/stft.py in float64, the checker of
tests/test_gpu_online_kernels.py on an independent float32 implementation and on the defects it has to reject, and the
host logic (constructors, config propagation, every refusal of Model.online, the overlay)."""
import os

import numpy as np
import pytest
import torch

import online_reference as OR
from oracle import features as ofeat
from oracle import stft as ostft
from tssep_amd.train.online import schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXP = os.path.join(ROOT, "tssep_amd", "exp")
# the cases of tests/test_gpu_online_kernels.py
FEATURE_CASES = [(3, 37, 513, 40, 40), (5, 205, 513, 40, 40), (2, 21, 201, 40, 40), (1, 5, 513, 0, 0)]
STREAM_N = (256 * 9 + 77, 256 * 9)
PATTERNS = ((9,), (1,) * 9, (1, 1, 3, 4), (2, 1, 6))
WORST = {}


def tables(F, n_mels, n_mfcc, dtype=torch.float32):
    if not n_mfcc:
        return None, None
    fb, dct = ofeat.mfcc_tables(size=2 * (F - 1), n_mels=n_mels, n_mfcc=n_mfcc)
    return fb.to(dtype), dct.to(dtype)


# ------------------------------------------------------------------------------------------- the defining property
@pytest.mark.parametrize("seed", range(4))
def test_causal_statistics_are_the_noncausal_ones_of_the_prefix(seed):
    """causal(X)[t] == oracle noncausal(X[:t+1])[t] per utterance, to 1e-12: 'tf' log1p and the 2-D (per-utterance)
    amplitude_to_db_power + DCT.  A batch of 3 has three floors, not the batch's."""
    B, T, F = 3, 9, 513
    X = OR.feature_input(B, T, F, seed).to(torch.complex128)
    fb, dct = tables(F, 40, 40, torch.float64)
    mfcc, log1p, state = OR.causal_features(X, fb, dct)
    for b in range(B):
        for t in range(T):
            if float(X[b, :t + 1].abs().max()) == 0:
                assert bool((log1p[b, t] == 0).all())            # digital silence so far: 0, not NaN
            else:
                ref = ofeat.log1p_max_norm_abs(X[b, :t + 1], "tf")[t]
                assert float((log1p[b, t] - ref).abs().max()) <= 1e-12, (b, t)
            mel = (X[b, :t + 1].abs() ** 2) @ fb                 # (torch_mfcc itself forms the power in float32)
            ref = (ofeat.amplitude_to_db_power(mel.t(), 80.0).t() @ dct)[t]      # 2-D: the floor of this utterance alone
            assert float((mfcc[b, t] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), (b, t)
    assert bool(torch.isfinite(log1p).all()) and bool((log1p[0, :2] == 0).all())
    batch, _, _ = OR.causal_features(X, fb, dct, defect="batch_floor")
    assert float((batch - mfcc).abs().max()) > 1.0               # the batch floor is another feature, by dBs
    # the state is the pair of maxima -- exact, whatever the chunking (the element-wise functions and the BLAS product
    # behind it may round differently for another number of rows here)
    db = OR.raw_db(X, fb)
    assert torch.equal(state, torch.stack([X.abs().amax((1, 2)), db.amax((1, 2))], dim=1))
    for chunks in ((T,), (1,) * T, (5, 1, T - 6)):
        m2, l2, s2 = OR.chunked(lambda x, s: OR.causal_features(x, fb, dct, state=s), X, chunks)
        assert torch.equal(s2, state), chunks
        assert float((l2 - log1p).abs().max()) <= 1e-12 and float((m2 - mfcc).abs().max()) <= 1e-12 * float(mfcc.abs().max()), chunks


# --------------------------------------------------------------------------------------- float64 stream against oracle
@pytest.mark.parametrize("N", STREAM_N)
@pytest.mark.parametrize("pushes", PATTERNS)
def test_float64_stream_reproduces_the_oracle(N, pushes):
    rng = np.random.RandomState(N + len(pushes))
    rows, K = 2, 3
    x = torch.as_tensor(rng.randn(rows, N))
    logit = torch.as_tensor(rng.randn(rows, K, ostft.num_frames(N), 513) * 2)
    X_ref = ostft.stft(x)
    T = X_ref.shape[1]
    X, y, steps = OR.run_stream(x, pushes)
    assert [s.frames for s in steps] == list(pushes) + [T - sum(pushes)] and steps[-1].frames == (4 if N % 256 else 3)
    assert sum(s.samples for s in steps) == N and X.shape[1] == T == sum(s.frames for s in steps)
    seen = 0
    for s in steps[:-1]:
        assert s.samples == max(seen + s.frames - 3, 0) * 256 - max(seen - 3, 0) * 256
        seen += s.frames
    assert float((X - X_ref).abs().max()) <= 1e-12 * float(X_ref.abs().max())
    y_ref = ostft.istft(X_ref, num_samples=N)
    assert y.shape == y_ref.shape and float((y - y_ref).abs().max()) <= 1e-12
    assert float((y - x).abs().max()) <= 1e-12                  # (and the analysis / synthesis pair reconstructs)
    assert float((OR.istft_whole(X_ref, N) - y_ref).abs().max()) <= 1e-12
    # the masked form, one mask per speaker
    for k in range(K):
        _, yk, _ = OR.run_stream(x, pushes, mask=lambda Xc, t0: torch.sigmoid(logit[:, k, t0:t0 + Xc.shape[1]]) * Xc)
        ref = ostft.istft(torch.sigmoid(logit[:, k]) * X_ref, num_samples=N)
        assert float((yk - ref).abs().max()) <= 1e-12
    est = OR.masked(logit, X_ref)
    assert est.shape == (rows * K, T, 513) and float((est[K + 1] - torch.sigmoid(logit[1, 1]) * X_ref[1]).abs().max()) <= 1e-14


def test_schedule():
    assert [tuple(s) for s in schedule((1, 1, 3, 4), 256 * 9 + 77)] == [(1, 3, 0), (1, 2, 0), (3, 1, 512), (4, 0, 1024), (4, 0, 256 * 3 + 77)]
    assert [tuple(s) for s in schedule((9,), 256 * 9)] == [(9, 3, 1536), (3, 0, 768)]
    assert [tuple(s) for s in schedule((), 100)] == [(4, 3, 100)]
    assert [tuple(s) for s in schedule((1,), 256)] == [(1, 3, 0), (3, 2, 256)]
    for bad in (((2,), 256), ((1,), 600), ((0, 1), 256)):
        with pytest.raises(ValueError):
            schedule(*bad)


# -------------------------------------------------------------- the GPU file's checker and the defects it has to reject
@pytest.mark.parametrize("B,T,F,n_mels,n_mfcc", FEATURE_CASES)
def test_feature_checker_passes_fp32_and_rejects_planted_defects(B, T, F, n_mels, n_mfcc):
    X = OR.feature_input(B, T, F, seed=B * 100 + T)
    fb, dct = tables(F, n_mels, n_mfcc)
    mfcc, log1p, _ = OR.causal_features(X, fb, dct)                      # torch float32, cummax: independent of the kernels
    WORST[(B, T, F)] = OR.check_features(mfcc, log1p, X, fb, dct, "fp32 cummax")
    assert WORST[(B, T, F)] < 1.0
    chunks = (5, 1, T - 6) if T > 6 else (1,) * T
    m2, l2, _ = OR.chunked(lambda x, s: OR.causal_features(x, fb, dct, state=s), X, chunks)
    OR.check_features(m2, l2, X, fb, dct, "fp32 cummax, chunked")
    defects = ["exclude_current", "nan_zero"] + (["batch_floor"] if n_mfcc and B > 1 else [])
    for defect in defects:
        m3, l3, _ = OR.causal_features(X, fb, dct, defect=defect)
        with pytest.raises(AssertionError):
            OR.check_features(m3, l3, X, fb, dct, defect)
    m4, l4, _ = OR.chunked(lambda x, s: OR.causal_features(x, fb, dct, state=s), X, chunks, drop_state=True)
    with pytest.raises(AssertionError):
        OR.check_features(m4, l4, X, fb, dct, "a state dropped between chunks")


@pytest.mark.parametrize("N", (2381, 2304))
def test_stream_checker_is_bit_equality_and_rejects_planted_defects(N):
    """float32: the stream equals the whole-signal transform bit for bit (the GPU file's check, torch.equal), and a carry
    added last, a carry dropped or a sample tail one hop stale do not."""
    rng = np.random.RandomState(N)
    x = torch.as_tensor(rng.randn(3, N).astype(np.float32))
    X_ref = ostft.stft(x)
    y_ref = OR.istft_whole(X_ref, N)
    for pushes in ((1, 1, 3, 4), (9,), (1,) * 9, (2, 1, 6)):
        X, y, _ = OR.run_stream(x, pushes)
        assert torch.equal(X, X_ref) and torch.equal(y, y_ref), pushes
    for pushes in ((1, 1, 3, 4), (2, 1, 6)):
        for defect in (dict(carry="last"), dict(carry="drop"), dict(stale=True)):
            X, y, _ = OR.run_stream(x, pushes, **defect)
            assert not (torch.equal(X, X_ref) and torch.equal(y, y_ref)), (pushes, defect)


def test_zz_report():
    for k, v in sorted(WORST.items()):
        print(f"fp32 cummax features {k}: worst error / tolerance {v:.3g}")


# ------------------------------------------------------------------------------------------------------ host logic
def _fe(parts=True, **kw):
    from tssep_amd.train import feature_extractor as fe
    return fe.ConcaternatedSTFTFeatures(fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=parts),
                                        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=parts),
                                        size=1024, shift=256, window="hann", **kw)


def _model(fe=None, enh=None, **me):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, loss, model, net
    kw = dict(idim=553, odim=513, units=8, projs=12, combination="mul", aux_net_output_size=513, ts_vad=3,
              output_resolution="tf", rnn_typ="lstm", random_speaker_order=False)
    kw.update(me)
    return model.Model(fe=_fe() if fe is None else fe, reader=DummyReader(), mask_estimator=net.MaskEstimator_v2(**kw),
                       enhancer=enh or enhancer.Masking(), loss=loss.LogMAE())


def test_constructors_and_config_propagation():
    from tssep_amd.train import feature_extractor as fe
    assert fe.Log1pMaxNormAbsSTFT().causal is False and fe.TorchMFCC().causal is False and _fe(False).causal is False
    assert fe.Log1pMaxNormAbsSTFT(causal=True).causal and fe.TorchMFCC(causal=True, log_mels=True).causal
    assert fe.Log1pMaxNormAbsSTFT(causal=True, statistics_axis="f").causal
    with pytest.raises(NotImplementedError, match="statistics_axis='t'"):
        fe.Log1pMaxNormAbsSTFT(causal=True, statistics_axis="t")
    assert _fe(True).causal and _fe(True, causal=True).causal
    mixed = fe.ConcaternatedSTFTFeatures(fe.TorchMFCC(size=1024, shift=256, causal=True), fe.Log1pMaxNormAbsSTFT())
    assert mixed.causal is False
    with pytest.raises(ValueError, match="causal parts"):
        _fe(False, causal=True)
    parts = {"fe1": {"factory": fe.TorchMFCC}, "fe2": {"factory": fe.Log1pMaxNormAbsSTFT}}
    cfg = fe.ConcaternatedSTFTFeatures.get_config({**parts, "causal": True})
    assert cfg["causal"] is True and cfg["fe1"]["causal"] is True and cfg["fe2"]["causal"] is True
    obj = fe.ConcaternatedSTFTFeatures.from_config(cfg)
    assert obj.causal and obj.fe1.causal and obj.fe2.causal
    cfg = fe.ConcaternatedSTFTFeatures.get_config(parts)
    assert cfg["causal"] is False and cfg["fe1"]["causal"] is False and not fe.ConcaternatedSTFTFeatures.from_config(cfg).causal
    # a carried state belongs to causal statistics; CPU tensors: refused before anything is launched
    X = torch.zeros(1, 4, 513, dtype=torch.complex64)
    for f in (fe.Log1pMaxNormAbsSTFT(), fe.TorchMFCC(size=1024, shift=256), _fe(False)):
        with pytest.raises(ValueError, match="causal"):
            f.stft_to_feature(X, state=torch.zeros(1, 2))
    for f, what in ((fe.STFT(size=512, shift=128), "size / shift"), (fe.STFT(window_length=800), "window_length"),
                    (fe.STFT(fading="half"), "fading"), (fe.STFT(pad=False), "pad")):
        with pytest.raises(NotImplementedError, match=what):
            f.stft_chunk(torch.zeros(1, 256))
        with pytest.raises(NotImplementedError, match=what):
            f.istft_chunk(X)


def test_model_online_refusals():
    from tssep_amd.train import enhancer, feature_extractor as fe
    aux = torch.zeros(2, 3, 513)
    sep = _model().online(aux)                                      # nothing is launched by the constructor
    assert sep.frames == 0 and not sep.closed and sep.last is None
    with pytest.raises(ValueError, match="on the device"):
        sep.push(torch.zeros(2, 512))                               # a CPU tensor
    with pytest.raises(ValueError, match="rnn_typ='lstm'"):
        _model(rnn_typ="blstm").online(aux)
    with pytest.raises(ValueError, match="utterance-wide statistics"):
        _model(fe=_fe(False)).online(aux)
    with pytest.raises(NotImplementedError, match="enhancer"):
        _model(enh=enhancer.TorchBF()).online(aux)
    with pytest.raises(NotImplementedError, match="nmask"):
        _model(nmask=2, enh=enhancer.TorchBF()).online(aux)          # (Masking itself refuses two masks in Model)
    with pytest.raises(NotImplementedError, match="output_resolution"):
        _model(output_resolution="t").online(aux)
    odd = fe.ConcaternatedSTFTFeatures(fe.TorchMFCC(size=1024, shift=256, fading="half", causal=True),
                                       fe.Log1pMaxNormAbsSTFT(fading="half", causal=True), fading="half")
    with pytest.raises(NotImplementedError, match="fading"):
        _model(fe=odd).online(aux)
    with pytest.raises(NotImplementedError, match="frame-wise aux"):
        _model().online(torch.zeros(2, 3, 5, 513))
    with pytest.raises(NotImplementedError, match="input_normalizer"):
        m = _model()
        m.mask_estimator.input_normalizer = torch.nn.Identity()
        m.online(aux)


def test_toy_online_overlay_resolves():
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    yamls = ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_online.yaml")
    cfg = run.build_config([os.path.join(EXP, y) for y in yamls] + ["eg.trainer.storage_dir=/tmp/unused"])
    fe = Experiment.get_config(cfg["eg"])["trainer"]["model"]["fe"]
    assert fe["causal"] is True and fe["fe1"]["causal"] is True and fe["fe2"]["causal"] is True
    model = Experiment.from_config(cfg["eg"]).trainer.model
    assert model.fe.causal and model.fe.fe1.causal and model.fe.fe2.causal and model.mask_estimator.rnn_typ == "lstm"
    assert model.online(torch.zeros(1, 4, 513)).fe is model.fe
    plain = run.build_config([os.path.join(EXP, y) for y in yamls[:2]] + ["eg.trainer.storage_dir=/tmp/unused"])
    ref = Experiment.from_config(plain["eg"]).trainer.model
    assert not ref.fe.causal and not ref.fe.fe1.causal and not ref.fe.fe2.causal
    with pytest.raises(ValueError):
        ref.online(torch.zeros(1, 4, 513))
