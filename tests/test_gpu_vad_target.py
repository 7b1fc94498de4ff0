"""The VAD losses on device-built targets, on a real MI355X: the reference's doctest numbers through the magnitude target,
loss and gradient against the float64 chain, a Model step with the ungated and the gated loss and with a caller's spectrum,
a captured step against the eager one, the gather for a device-resident `vad`, and the toy overlay.  References,
bound and band: tests/vad_target_reference.py."""
import os
import types

import numpy as np
import pytest
import torch

import vad_target_reference as R
from oracle import loss as oloss

pytestmark = pytest.mark.gpu

from test_gpu_kernels import close  # noqa: E402

T_ = torch.as_tensor
TARGET = "Speaker_reverberation_early_ch0"
KEY = TARGET.lower()


def test_reference_doctest_numbers_on_the_device(golden):
    """loss.py:286-299 through loss.VADSigmoidBCE(target='Speaker_reverberation_early') on CUDA tensors (a REAL target, as
    the doctest passes); tolerance: the one test_gpu_kernels.py::test_losses gives the 'Vad' BCE."""
    from tssep_amd.train import loss
    k = golden("kat_loss")
    torch.manual_seed(0)
    target = torch.rand((2, 100, 257))
    estimate = target + 0.5 * torch.rand((2, 100, 257))
    lo = loss.VADSigmoidBCE(pit=False, target="Speaker_reverberation_early")
    tgt = target.cuda()
    prepared = lo.prepare_target(tgt)
    assert tuple(prepared.shape) == (2, 100) and prepared.is_cuda and prepared.dtype == torch.float32
    assert torch.equal(prepared.cpu(), lo.prepare_target(target))             # the CPU path is the reference's formula
    for name, est in (("bce", estimate), ("bce10", ((abs(target) > 0.05).float() - 0.5) * 10),
                      ("bce1", ((abs(target) > 0.05).float() - 0.5) * 1)):
        close(lo(est.cuda(), tgt), T_(k[name]), rtol=1e-5, atol=1e-6, name=name)
    with pytest.raises(AssertionError):                                       # loss.py:334-339
        lo(estimate.cuda()[..., :5], tgt)


class _Stub(torch.nn.Module):
    """What from_ex_out asks of a model: the feature extractor and a device."""

    def __init__(self, fe):
        super().__init__()
        self.fe = fe
        self.p = torch.nn.Parameter(torch.zeros(1))


@pytest.fixture(scope="module")
def chain():
    """B = 2, K = 3, N = 4099 and the float64 chain on it, computed once: (x [B,K,N] float32, vad64 [B,K,T] float64)."""
    B, K, N = 2, 3, 4099
    x = R.envelope_signal(B * K, N, seed=31).reshape(B, K, N)
    x[1, 2] = 0                                                                # an absent speaker
    a64 = R.frame_mag64(R.stft64(x, window="hann"))
    assert not R.undecided(a64, 0.05, R.rel_bound(1024, 513)).any()            # every frame decidable: no band in the tests
    vad64 = R.decide64(a64, 0.05).astype(np.float64)
    assert 0.2 < vad64.mean() < 0.95 and not vad64[1, 2].any()
    return x, vad64


@pytest.mark.parametrize("res,F", [("tf", 513), ("t", 1)])
def test_loss_and_gradient_against_the_float64_chain(chain, res, F):
    from tssep_amd.train import feature_extractor as fe, loss
    x, vad64 = chain
    B, K, T = vad64.shape
    g = torch.Generator().manual_seed(5 + F)
    logit = (torch.randn(B, K, 1, T, F, generator=g) * 2).requires_grad_()
    gout = torch.rand(B, generator=g) + 0.5
    ref = oloss.vad_sigmoid_bce(logit.double().squeeze(-3), T_(vad64))
    (ref * gout.double()).sum().backward()
    m = _Stub(fe.STFT(size=1024, shift=256, window="hann")).cuda()
    lo = loss.VADSigmoidBCE(target=TARGET)
    ld = logit.detach().cuda().requires_grad_()
    ex = {KEY: T_(x).cuda()}
    value = lo.from_ex_out(ex, types.SimpleNamespace(logit=ld), m, None)
    (value * gout.cuda()).sum().backward()
    assert TARGET not in ex                                                   # that key stays a spectrum's
    act = lo.frame_activity(ex, m)
    assert np.array_equal(act.cpu().numpy(), vad64.astype(np.float32))
    close(value, ref, rtol=1e-5, atol=1e-6, name="bce")
    close(ld.grad, logit.grad, rtol=1e-4, atol=1e-9, name="d logit")


def _model(lo, explicit_vad, res="tf", K=3, seed=4):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, model, net
    torch.manual_seed(seed)
    return model.Model(
        fe=fe.ConcaternatedSTFTFeatures(
            fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=12, projs=10, combination="mul",
                                            aux_net_output_size=513, ts_vad=K, output_resolution=res,
                                            random_speaker_order=False, explicit_vad=explicit_vad),
        enhancer=enhancer.Masking(), loss=lo).cuda()


def _batch(x, seed=0):
    B, K, N = x.shape
    rng = np.random.RandomState(seed)
    obs = x.sum(1, keepdims=True) + 0.01 * rng.randn(B, 1, N).astype(np.float32)
    return {"observation": T_(obs).cuda(), "auxInput": T_(rng.rand(B, K, 513).astype(np.float32)).cuda(),
            "reference_channel": 0, KEY: T_(x).cuda(), "dataset": ["m"] * B}


def _step(m, ex):
    m.zero_grad()
    out = m(ex)
    summary = m.review(ex, out)
    summary["loss"].backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    return out, summary, grads


@pytest.mark.parametrize("res", ["t", "tf"])
def test_model_step_with_the_ungated_loss(chain, res):
    from tssep_amd.train import loss
    x, vad64 = chain
    m = _model(loss.VADSigmoidBCE(target=TARGET), explicit_vad=False, res=res)
    ex = _batch(x)
    out, summary, _ = _step(m, ex)
    act = m.loss.frame_activity(ex, m)
    assert np.array_equal(act.cpu().numpy(), vad64.astype(np.float32))
    assert TARGET not in ex
    ref = oloss.vad_sigmoid_bce(out.logit.detach().cpu().double().squeeze(-3), T_(vad64)).sum()
    close(summary["loss"], ref, rtol=1e-5, atol=1e-6, name="loss")
    # a spectrum supplied by the caller: the same activity (no frame of these inputs lies in the band), the same loss
    ex2 = _batch(x)
    ex2[TARGET] = m.fe.stft(ex2[KEY])
    spectrum = ex2[TARGET]
    _, summary2, _ = _step(m, ex2)
    assert ex2[TARGET] is spectrum and spectrum.is_complex()
    assert torch.equal(m.loss.frame_activity(ex2, m), act)
    assert torch.equal(summary2["loss"], summary["loss"])


def test_model_step_with_the_gated_loss(chain):
    from tssep_amd import functional as Fn
    from tssep_amd.train import loss
    x, vad64 = chain
    lo = loss.SignalAndVADSigmoidBCE(target=TARGET, signal_loss=loss.LogMAE())
    m = _model(lo, explicit_vad=True)
    ex = _batch(x)
    out, summary, grads = _step(m, ex)
    act = lo.frame_vad(ex, m)
    assert np.array_equal(act.cpu().numpy(), vad64.astype(np.float32)) and TARGET not in ex
    # the BCE rode in the fused gated tail, and from_ex_out took it from there
    assert not out.materialised and out._gate_bce is not None and out._gate_bce[1] is act
    alone = Fn.gate_bce(out._gated.detach(), act)
    close(out._gate_bce[0], alone, rtol=1e-6, atol=1e-7, name="fused bce")
    ref = oloss.vad_sigmoid_bce(out.vad_logit.detach().cpu().double().squeeze(-2)[..., None], T_(vad64))
    close(alone, ref, rtol=1e-5, atol=1e-6, name="gate bce")
    signal = loss.LogMAE()(out.time_estimate.detach(), ex[KEY])
    close(summary["loss"], (alone + signal).sum(), rtol=1e-5, atol=1e-6, name="joint loss")
    # the materialised route (someone looked at the mask): same loss, same gradients
    ex2 = _batch(x)
    m.zero_grad()
    out2 = m(ex2)
    assert out2.mask is not None
    s2 = m.review(ex2, out2)
    s2["loss"].backward()
    close(s2["loss"], summary["loss"], rtol=1e-5, atol=1e-6, name="materialised loss")
    for k, p in m.named_parameters():
        if p.grad is not None:
            close(p.grad, grads[k], rtol=1e-3, atol=1e-4 * float(grads[k].abs().max()) + 1e-9, name="d" + k)


@pytest.mark.parametrize("gated", [False, True])
def test_captured_step_equals_the_eager_step(gated):
    """Three steps with different data through GraphedStep: the target kernels are nodes of the graph (a host
    synchronisation inside the step would fail the capture), losses and gradients equal the eager steps' bit for bit."""
    from tssep_amd.train import loss
    from tssep_amd.train.graph import GraphedStep
    from tssep_amd.train.optimizer import Adam
    lo = loss.SignalAndVADSigmoidBCE(target=TARGET, signal_loss=loss.LogMAE()) if gated else loss.VADSigmoidBCE(target=TARGET)
    m = _model(lo, explicit_vad=gated, res="tf" if gated else "t")
    opt = Adam(gradient_clipping=10.0)
    opt.set_parameters(m.parameters())
    exs = [_batch(R.envelope_signal(6, 4099, seed=40 + i).reshape(2, 3, 4099), seed=i) for i in range(3)]
    want = []
    for e in exs:
        opt.zero_grad()
        e = dict(e)
        out = m(e)
        value = m.review(e, out)["loss"]
        value.backward()
        opt.bucket.sync()
        torch.cuda.synchronize()
        want.append((value.detach().clone(), opt.bucket.flat.clone(), lo.frame_vad(e, m).clone() if gated
                     else lo.frame_activity(e, m).clone()))
    assert not torch.equal(want[0][2], want[1][2])
    g = GraphedStep(m, opt)
    assert g.usable(exs[0])
    g(dict(exs[0]))                                                            # warm-up, capture, first replay
    for i in (1, 2, 0):
        _, summary = g(dict(exs[i]))
        torch.cuda.synchronize()
        assert torch.equal(summary["loss"].detach(), want[i][0]), (i, float(summary["loss"]), float(want[i][0]))
        assert torch.equal(opt.bucket.flat, want[i][1]), (i, float((opt.bucket.flat - want[i][1]).abs().max()))
    assert g.replays == 4 and g.eager_steps == 0 and len(g._graphs) == 1


def test_vad_target_from_a_device_resident_sample_activity():
    """`vad` on the device: stft_vad_device (the gather) gives the values of stft_vad, which keeps its host route, and
    VADSigmoidBCE(target='Vad') on the gathered Vad has the bits of the loss on the Vad prepared on the host."""
    from tssep_amd.train import feature_extractor as fe, loss
    from tssep_amd.util.utils import stft_vad, stft_vad_device
    B, K, N = 2, 3, 4099
    rng = np.random.RandomState(8)
    vad = np.repeat(rng.rand(B, K, -(-N // 500)) < 0.5, 500, axis=-1)[..., :N]
    host = stft_vad(vad, 1024, 256, True)
    dev = stft_vad_device(T_(vad).cuda(), 1024, 256, True)
    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == host.shape
    np.testing.assert_array_equal(dev.cpu().numpy(), host.astype(np.float32))
    assert torch.equal(stft_vad_device(T_(vad).float().cuda(), 1024, 256, True), dev)
    assert torch.equal(stft_vad(T_(vad).cuda(), 1024, 256, True), dev)         # the host route, same values and device
    with pytest.raises(TypeError):
        stft_vad_device(T_(vad), 1024, 256, True)
    m = _Stub(fe.STFT(size=1024, shift=256, window="hann")).cuda()
    lo = loss.VADSigmoidBCE()
    logit = (torch.randn(B, K, 1, host.shape[-1], 1, generator=torch.Generator().manual_seed(2)) * 2).cuda()
    out = types.SimpleNamespace(logit=logit)
    from_device = lo.from_ex_out({"Vad": dev}, out, m, None)
    from_host = lo.from_ex_out({"vad": T_(vad).cuda()}, out, m, None)
    assert torch.equal(from_device, from_host)


def test_toy_magnitude_overlays_train(tmp_path):
    """tssep_amd/exp/toy_tsvad_magnitude.yaml, then its gated counterpart initialised from it: a few iterations each with
    finite losses."""
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")

    def toy(*yamls, overrides=()):
        cfg = run.build_config([os.path.join(exp, y) for y in yamls] + list(overrides))
        return Experiment.from_config(cfg["eg"])

    def train(m):
        assert m.loss.target == TARGET
        ds = m.prepare_train_dataset(torch.device("cuda"), batch_size=1, prefetch=False)
        losses = []
        for i, ex in enumerate(ds):
            if i == 3:
                break
            m.zero_grad()
            out = m(ex)
            summary = m.review(ex, out)
            summary["loss"].backward()
            losses.append(float(summary["loss"]))
            assert float(m.loss.frame_vad(ex, m).mean() if hasattr(m.loss, "frame_vad") else
                         m.loss.frame_activity(ex, m).mean()) > 0
        assert len(losses) == 3 and all(np.isfinite(losses)), losses

    vad = toy("toy_common.yaml", "toy_tsvad.yaml", "toy_tsvad_magnitude.yaml",
              overrides=[f"eg.trainer.storage_dir={tmp_path / 'v'}"])
    train(vad.trainer.model.cuda())
    ck = tmp_path / "vad.pth"
    torch.save({"model": vad.trainer.model.state_dict()}, ck)
    sep = toy("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_explicit_vad.yaml", "toy_tssep_explicit_vad_magnitude.yaml",
              overrides=[f"eg.trainer.storage_dir={tmp_path / 's'}", f"eg.init_ckpt.init_ckpt={ck}",
                         "eg.trainer.stop_trigger=[3,iteration]"])
    sep.init_ckpt(sep)
    train(sep.trainer.model.cuda())
