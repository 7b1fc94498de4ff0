"""AbsSTFT, Log1pAbsSTFT, MVNLog1pAbsSTFT on a real MI355X, from the classes up to the toy model: the classes
against the float64 definitions within the bounds of tests/specfeat_reference.py; the concatenation with TorchMFCC placed
into one buffer without a copy (launch log = the entry-point names `hip_ops.check` sees, torch.concat / torch.cat forbidden
while it runs); the existing pair TorchMFCC + Log1pMaxNormAbsSTFT with the launches it had before these classes existed
(tests/golden/specfeat_existing_pair_launches.json, recorded from a run of the commit before them); Model.forward, eager
against captured training, and Model.online in pushes."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import specfeat_reference as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "specfeat_existing_pair_launches.json")
B, K, N = 2, 3, 256 * 11 + 100
WIDTHS = dict(idim=553, odim=513, units=8, projs=12, layers=3)
PATTERNS = ((11,), (1,) * 11, (4, 1, 6))
STFT_KW = dict(size=1024, shift=256, window="hann")


def _spectrum(lead=(2, 1), T=11, F=513, seed=7):
    X = R.make_input(int(np.prod(lead)), T, F, seed=seed).reshape(*lead, T, F)
    return X, torch.as_tensor(X).cuda()


@contextlib.contextmanager
def launches(forbid_concat=True):
    """-> the list of entry points checked while the block runs; torch.concat / torch.cat raise inside it"""
    from tssep_amd import hip_ops as H
    log, old = [], (H.check, torch.concat, torch.cat)

    def check_(status, what):
        log.append(what)
        return old[0](status, what)

    def no_cat(*a, **k):
        raise AssertionError("a concatenation (a copy kernel) on the placed path")

    H.check = check_
    if forbid_concat:
        torch.concat = torch.cat = no_cat
    try:
        yield log
    finally:
        H.check, torch.concat, torch.cat = old


# ---- the classes -----------------------------------------------------------------------------------------------------------
def test_classes_within_bounds_any_leading_dimensions():
    from tssep_amd.train import feature_extractor as fe
    X, Xd = _spectrum()
    table = ((fe.AbsSTFT, R.abs_feature, R.abs_bound), (fe.Log1pAbsSTFT, R.log1p_abs_feature, R.log1p_bound),
             (fe.MVNLog1pAbsSTFT, R.mvn_feature, R.mvn_bound))
    for cls, ref, bound in table:
        for causal in (False, True):
            if cls is fe.MVNLog1pAbsSTFT and causal:
                continue
            obj = cls(causal=causal)
            out = obj.stft_to_feature(Xd)
            assert tuple(out.shape) == (2, 1, 11, 513) and out.dtype == torch.float32
            R.held(out.cpu().numpy(), ref(X), bound(X), f"{cls.__name__} causal={causal} 4-D")
            one = obj.stft_to_feature(Xd[1, 0])                      # 2-D: one utterance
            assert tuple(one.shape) == (11, 513) and torch.equal(one, out[1, 0])
            assert torch.equal(obj.stft_to_feature(Xd.to(torch.complex128)), out)
            if causal:                                               # no statistics: a state passes through untouched
                token = object()
                o, s = obj.stft_to_feature(Xd, token, True)
                assert s is token and torch.equal(o, out)
            else:
                assert obj.stft_to_feature(Xd, None, True)[1] is None
                with pytest.raises(ValueError, match="a carried state belongs to causal statistics"):
                    obj.stft_to_feature(Xd, torch.zeros(2, 514, dtype=torch.float64, device="cuda"))
    for kw in (dict(norm_vars=True), dict(norm_means=False)):
        with pytest.raises(NotImplementedError):
            fe.MVNLog1pAbsSTFT(**kw).stft_to_feature(Xd)
    sig = torch.as_tensor(np.random.RandomState(0).randn(2, 3000).astype(np.float32)).cuda()
    m = fe.MVNLog1pAbsSTFT()
    assert torch.equal(m(sig), m.stft_to_feature(m.stft(sig))) and tuple(m(sig).shape) == (2, m.frames(3000), 513)


@pytest.mark.parametrize("alpha", [1.0, 0.97])
def test_causal_mvn_class_in_pushes(alpha):
    from tssep_amd.train import feature_extractor as fe
    X, Xd = _spectrum()
    obj = fe.MVNLog1pAbsSTFT(causal=True, forgetting=alpha)
    whole, state = obj.stft_to_feature(Xd, None, True)
    assert tuple(whole.shape) == (2, 1, 11, 513) and state.dtype == torch.float64 and tuple(state.shape) == (2, 514)
    R.held(whole.cpu().numpy(), R.mvn_causal_feature(X, forgetting=alpha)[0], R.mvn_causal_bound(X, forgetting=alpha),
           f"MVNLog1pAbsSTFT causal a={alpha}")
    assert bool((whole[..., 0, :] == 0).all()) and torch.equal(obj.stft_to_feature(Xd), whole)
    for pushes in PATTERNS:
        st, pos, outs = None, 0, []
        for c in pushes:
            o, st = obj.stft_to_feature(Xd[..., pos:pos + c, :], st, True)
            outs.append(o)
            pos += c
        assert torch.equal(torch.cat(outs, dim=-2), whole) and torch.equal(st, state), pushes
    with pytest.raises(ValueError, match=r"float32 \(2, 2\)"):
        obj.stft_to_feature(Xd, torch.zeros(2, 2, device="cuda"))                      # (Log1pMaxNormAbsSTFT's state)


# ---- the concatenation -----------------------------------------------------------------------------------------------------
def _pair(second, causal, **kw):
    from tssep_amd.train import feature_extractor as fe
    return fe.ConcaternatedSTFTFeatures(fe.TorchMFCC(output_size=40, causal=causal, **STFT_KW),
                                        getattr(fe, second)(causal=causal, **STFT_KW, **kw), **STFT_KW).cuda()


@pytest.mark.parametrize("second", ["MVNLog1pAbsSTFT", "Log1pAbsSTFT", "AbsSTFT"])
@pytest.mark.parametrize("causal", [False, True])
def test_concatenation_is_placed_without_a_copy(second, causal):
    _, Xd = _spectrum(lead=(3,), T=11)
    cat = _pair(second, causal)
    assert cat.causal is causal and cat.output_size == 553
    with launches() as log:
        out, state = cat.stft_to_feature(Xd, None, True)
    first = "feat_causal_fwd" if causal else "feat_fwd"
    assert log == [first, "specfeat_causal_fwd" if causal and second == "MVNLog1pAbsSTFT" else "specfeat_fwd"], log
    # one [B, T, ld] buffer holds both parts
    assert tuple(out.shape) == (3, 11, 553) and out.stride() == (11 * 556, 556, 1)
    assert out.untyped_storage().nbytes() == 3 * 11 * 556 * 4
    base = torch.as_strided(out, (3, 11, 556), (11 * 556, 556, 1))
    assert bool((base[..., 553:] == 0).all())
    if causal:
        s1, s2 = state
        mf, t1 = cat.fe1.stft_to_feature(Xd, None, True)
        sp, t2 = cat.fe2.stft_to_feature(Xd, None, True)
        assert torch.equal(s1, t1) and (torch.equal(s2, t2) if second == "MVNLog1pAbsSTFT" else s2 is None and t2 is None)
    else:
        assert state is None
        mf, sp = cat.fe1.stft_to_feature(Xd), cat.fe2.stft_to_feature(Xd)
    assert torch.equal(out[..., :40], mf) and torch.equal(out[..., 40:], sp)
    one = cat.stft_to_feature(Xd[0])             # 2-D: one utterance (the MFCC's dB floor then spans that utterance alone)
    assert tuple(one.shape) == (11, 553) and torch.equal(one[:, 40:], out[0, :, 40:])
    if causal and second == "MVNLog1pAbsSTFT":
        # in pushes: the pair of states carries both parts
        for pushes in PATTERNS[1:]:
            st, pos, outs = None, 0, []
            for c in pushes:
                with launches() as log:
                    o, st = cat.stft_to_feature(Xd[:, pos:pos + c], st, True)
                assert log == ["feat_causal_fwd", "specfeat_causal_fwd"]
                outs.append(o)
                pos += c
            assert torch.equal(torch.cat(outs, dim=-2), out) and torch.equal(st[0], state[0]) and torch.equal(st[1], state[1])
        with pytest.raises(ValueError, match="the pair"):
            cat.stft_to_feature(Xd, torch.zeros(3, 2, device="cuda"))
    if not causal:
        with pytest.raises(ValueError, match="a carried state belongs to causal statistics"):
            cat.stft_to_feature(Xd, (None, None))


def existing_pair_launches():
    """what TorchMFCC + Log1pMaxNormAbsSTFT launches, causal and not (also run by the recorder on the parent commit)"""
    from tssep_amd import hip_ops as H
    _, Xd = _spectrum(lead=(3,), T=11)
    got = {}
    for causal in (False, True):
        cat = _pair("Log1pMaxNormAbsSTFT", causal)
        log, old = [], H.check
        H.check = lambda status, what: (log.append(what), old(status, what))[1]
        try:
            out, state = cat.stft_to_feature(Xd, None, True)
        finally:
            H.check = old
        got["causal" if causal else "whole"] = dict(
            launches=log, state=None if state is None else [str(state.dtype), list(state.shape)], shape=list(out.shape))
    return got


def test_existing_pair_keeps_its_branch_state_and_launches():
    want = json.load(open(GOLDEN))
    assert existing_pair_launches() == want
    assert want["whole"]["launches"] == ["feat_fwd"] and want["causal"]["launches"] == ["feat_causal_fwd"]
    assert want["causal"]["state"] == ["torch.float32", [3, 2]]


# ---- the toy model ---------------------------------------------------------------------------------------------------------
def _model(causal, seed=5, forgetting=1.0, **me):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, loss, model, net
    torch.manual_seed(seed)
    kw = dict(combination="mul", ts_vad=K, random_speaker_order=False, **WIDTHS)
    if causal:
        kw["rnn_typ"] = "lstm"
    kw.update(me)
    fe = _pair("MVNLog1pAbsSTFT", causal, **(dict(forgetting=forgetting) if causal else {}))
    return model.Model(fe=fe, reader=DummyReader(), mask_estimator=net.MaskEstimator_v2(**kw), enhancer=enhancer.Masking(),
                       loss=loss.LogMAE()).cuda().eval()


@pytest.mark.parametrize("causal", [False, True])
def test_model_forward_input_is_the_feature_of_its_observation(causal):
    from test_gpu_dropout import _batch
    model = _model(causal)
    ex = _batch(2, K, 5000, seed=3)
    out = model(ex)
    assert bool(torch.isfinite(out.logit).all())
    X = ex["Observation"][:, 0].cpu().numpy()
    inp = ex["Input"]
    assert tuple(inp.shape) == (2, X.shape[1], 553) and inp.dtype == torch.float32
    if causal:
        ref, bound = R.mvn_causal_feature(X)[0], R.mvn_causal_bound(X)
    else:
        ref, bound = R.mvn_feature(X), R.mvn_bound(X)
    R.held(inp[..., 40:].cpu().numpy(), ref, bound, f"Model.forward Input causal={causal}")
    assert torch.equal(inp[..., :40], model.fe.fe1.stft_to_feature(ex["Observation"][:, 0]))


@pytest.mark.parametrize("causal", [False, True])
def test_training_eager_and_graphed_bit_identical(tmp_path, causal):
    from test_gpu_dropout import _batch
    from tssep_amd.train import runtime
    from tssep_amd.train.optimizer import Adam
    from tssep_amd.train.trainer import Trainer
    data = [_batch(2, K, 5000 if i % 2 else 7300, seed=41 + i) for i in range(4)]

    class Dataset(list):
        def __iter__(self):
            return (dict(ex) for ex in list.__iter__(self))

    runs = {}
    for mode in ("off", "on"):
        with runtime.applied(graph_step=mode):
            np.random.seed(78)
            tr = Trainer(_model(causal, seed=6, forgetting=0.97).train(), tmp_path / mode, Adam(gradient_clipping=10.0, lr=1e-3),
                         summary_trigger=(1, "iteration"), checkpoint_trigger=(1000, "iteration"), stop_trigger=(4, "iteration"),
                         virtual_minibatch_size=1)
            hist = tr.train(Dataset(data), device=0)
            torch.cuda.synchronize()
            hf = json.loads((tmp_path / mode / "log" / "history.json").read_text())
            runs[mode] = ([l for _, l in hist], tr.optimizer.flat_param.clone(), hf)
    l_off, p_off, _ = runs["off"]
    l_on, p_on, h_on = runs["on"]
    assert len(l_off) == 4 and all(np.isfinite(l_off))
    assert h_on.get("graph_replays", 0) >= 1 and h_on["graphs"] == 2, h_on
    assert l_on == l_off, [(i, a, b) for i, (a, b) in enumerate(zip(l_on, l_off)) if a != b]
    assert torch.equal(p_on, p_off), float((p_on - p_off).abs().max())


# ---- online ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pushes", PATTERNS)
def test_online_separator_with_the_running_mean(pushes):
    from test_gpu_online import _signal
    from tssep_amd.train.online import schedule
    model = _model(True, forgetting=0.97)
    fe = model.fe
    x, aux = _signal()
    sep = model.online(aux, record=True)
    steps = schedule(pushes, N)
    ys, pos = [], 0
    for s in steps[:-1]:
        y = sep.push(x[:, pos:pos + s.frames * 256])
        assert tuple(y.shape) == (B, K, s.samples), (y.shape, s)
        ys.append(y)
        pos += s.frames * 256
    ys.append(sep.flush(x[:, pos:]))
    y = torch.cat(ys, dim=-1)
    Obs, Inp, logit = (torch.cat([r[k] for r in sep.record], dim=-2) for k in ("Observation", "Input", "logit"))
    assert tuple(y.shape) == (B, K, N) and bool(torch.isfinite(y).all()) and sep.frames == fe.frames(N)
    X = fe.stft(x)
    assert torch.equal(torch.view_as_real(Obs), torch.view_as_real(X))
    feat = fe.stft_to_feature(X)
    assert torch.equal(Inp, feat) and bool(torch.isfinite(feat).all())
    Xh = X.cpu().numpy()
    R.held(feat[..., 40:].cpu().numpy(), R.mvn_causal_feature(Xh, forgetting=0.97)[0], R.mvn_causal_bound(Xh, forgetting=0.97),
           f"online features {pushes[:3]}")
    assert torch.equal(y, fe.masked_istft(logit, X, num_samples=N))
