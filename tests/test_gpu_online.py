"""Model.online on a real MI355X: a toy causal model (idim 553, units 8, projs 12, K = 3, B = 2,
N = 256 * 11 + 100) fed in pushes (11), (1 x 11), (4, 1, 6) + flush.  The frames and features the separator formed are
those of the whole signal bit for bit; its audio is fe.masked_istft of its own concatenated chunk logits bit for bit; the
chunk logits stay inside what tests/test_gpu_causal_estimator.py allows forward_chunk against the float64 restatement of
the whole utterance (its `reference` and `held`, imported).  explicit_vad once.  Training with the causal features: eager,
and through GraphedStep bit-identical to the eager trainer."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_causal_estimator as CE  # noqa: E402

B, K, N = 2, 3, 256 * 11 + 100
WIDTHS = dict(idim=553, odim=513, units=8, projs=12, layers=3)
PATTERNS = ((11,), (1,) * 11, (4, 1, 6))
CE.ROWS.setdefault("online-toy", (B, WIDTHS, dict(combination="mul", ts_vad=K), False))      # a row for CE.reference


def _fe():
    from tssep_amd.train import feature_extractor as fe
    return fe.ConcaternatedSTFTFeatures(
        fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True), size=1024, shift=256, window="hann")


def _model(seed=5, **me):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, loss, model, net
    torch.manual_seed(seed)
    kw = dict(combination="mul", ts_vad=K, rnn_typ="lstm", random_speaker_order=False, **WIDTHS)
    kw.update(me)
    return model.Model(fe=_fe(), reader=DummyReader(), mask_estimator=net.MaskEstimator_v2(**kw), enhancer=enhancer.Masking(),
                       loss=loss.LogMAE()).cuda().eval()


def _signal(seed=3):
    rng = np.random.RandomState(seed)
    x = rng.randn(B, N).astype(np.float32) * np.linspace(0.05, 1.0, N, dtype=np.float32)      # the level rises: the state moves
    x[0, :300] = 0                                                                            # digital silence first
    aux = (rng.randn(B, K, 513) + 0.5).astype(np.float32)
    return torch.as_tensor(x).cuda(), torch.as_tensor(aux).cuda()


def _stream(model, x, aux, pushes):
    """-> (audio [B,K,N], Observation, Input, logit rows of all frames, the separator)"""
    from tssep_amd.train.online import schedule
    sep = model.online(aux, record=True)
    steps = schedule(pushes, N)
    ys, pos = [], 0
    for s in steps[:-1]:
        y = sep.push(x[:, pos:pos + s.frames * 256])
        assert tuple(y.shape) == (B, K, s.samples), (y.shape, s)
        ys.append(y)
        pos += s.frames * 256
    assert 0 < N - pos < 256
    y = sep.flush(x[:, pos:])
    assert tuple(y.shape) == (B, K, steps[-1].samples) and sep.frames == model.fe.frames(N)
    ys.append(y)
    with pytest.raises(RuntimeError, match="closed"):
        sep.push(x[:, :256])
    cat = {k: torch.cat([r[k] for r in sep.record], dim=-2) for k in ("Observation", "Input", "logit")}
    return torch.cat(ys, dim=-1), cat["Observation"], cat["Input"], cat["logit"], sep


@pytest.mark.parametrize("pushes", PATTERNS)
def test_online_separator(pushes):
    from tssep_amd import hip_ops
    model = _model()
    fe, me = model.fe, model.mask_estimator
    x, aux = _signal()
    y, Obs, Inp, logit, sep = _stream(model, x, aux, pushes)
    assert tuple(y.shape) == (B, K, N) and bool(torch.isfinite(y).all())
    X = fe.stft(x)
    assert torch.equal(torch.view_as_real(Obs), torch.view_as_real(X))
    feat = fe.stft_to_feature(X)
    assert torch.equal(Inp, feat) and bool((feat[0, 0, 40:] == 0).all()) and bool(torch.isfinite(feat).all())
    assert torch.equal(y, fe.masked_istft(logit, X, num_samples=N))
    last = sep.last
    n_last = sep.record[-1]["logit"].shape[-2]
    assert torch.equal(last.logit[:, :, 0], sep.record[-1]["logit"]) and tuple(last.mask.shape) == (B, K, 1, n_last, 513)
    # the chunk logits against the float64 restatement of the WHOLE utterance, under forward_chunk's own bounds
    state = {k: v.detach().cpu().clone() for k, v in me.state_dict().items()}
    rng = np.random.RandomState(11)
    T = X.shape[-2]
    inp = dict(xs=feat.cpu().numpy(), aux=aux.cpu().numpy(), w={n: rng.randn(B, K, 1, T, 513).astype(np.float32) for n in ("mask", "logit")})
    r64, r32 = (CE.reference("online-toy", state, inp, None, dt) for dt in (torch.float64, torch.float32))
    got = {"logit": logit.unsqueeze(2).cpu(), "mask": torch.sigmoid(logit).unsqueeze(2).cpu()}
    assert got["logit"].shape == r64["logit"].shape
    CE.held(got, r64, r32, hip_ops.GEMM_PRECISION, f"online {pushes[:3]}", names=("logit",))
    whole = me(feat, aux)
    CE.held({"logit": whole.logit.detach().cpu()}, r64, r32, hip_ops.GEMM_PRECISION, "forward", names=("logit",))


def test_online_separator_explicit_vad_and_unbatched():
    model = _model(explicit_vad=True)
    fe = model.fe
    x, aux = _signal()
    y, Obs, _, logit, sep = _stream(model, x, aux, (4, 1, 6))
    assert logit.shape[-1] == 514 and sep.last.logit is None and tuple(sep.last.vad_mask.shape)[:2] == (B, K)
    est, _ = fe.masked_istft(logit, Obs, num_samples=N)
    assert torch.equal(y, est)
    # one un-batched stream: entry 0 of the batch, [K, m] per call
    model = _model()
    one = model.online(aux[0])
    ys = [one.push(x[0, :1024]), one.push(x[0, 1024:2816]), one.flush(x[0, 2816:])]
    assert [tuple(t.shape) for t in ys] == [(K, 256), (K, 1792), (K, N - 2048)]
    bat = model.online(aux[:1])                                     # (the same rows in every GEMM: the same bits)
    yb = [bat.push(x[:1, :1024]), bat.push(x[:1, 1024:2816]), bat.flush(x[:1, 2816:])]
    assert torch.equal(torch.cat(ys, dim=-1), torch.cat(yb, dim=-1)[0])


def test_training_with_causal_features_eager_and_graphed(tmp_path):
    """Model.forward with a causal fe runs under autograd, and the trainer's captured step is bit-identical to the eager
    trainer over 4 iterations (the causal feature launches are captured as they stand: no host sync, no allocation by the
    library)."""
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
            tr = Trainer(_model(seed=6).train(), tmp_path / mode, Adam(gradient_clipping=10.0, lr=1e-3),
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
