"""FreqMSE end to end on a real MI355X: the toy model (toy_common.yaml + toy_tssep.yaml + toy_tssep_freqmse.yaml, B = 2,
K = 8) through Model.review on both routes -- the fused spectral tail (logits, Observation and target spectrum in one
kernel each way, no inverse STFT) and the materialised one (``out.stft_estimate`` touched first: mask head, then
functional.spec_mse) -- against the float64 references of tests/spectral_reference.py within their bounds; the folds of
``fold_tail``; the lazy ``time_estimate``; graph replay; the complex128 estimate of TorchBF; and an existing route
left as it was.

One override, as in test_gpu_tail_routes.py: ``num_averaged_permutations=1`` (the head offers its link for a single trial
only).  The targets are the model's own time estimates, relabelled by a rotation and with noise added, so that the best
permutation is decided by a wide gap -- asserted against the forward bound, not assumed."""
import os

import numpy as np
import pytest
import torch

import spectral_reference as R

pytestmark = pytest.mark.gpu

from test_gpu_explicit_vad import _batch  # noqa: E402

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
B, K = 2, 8
SAMPLES = (4096, 3001)
SIGNAL, SPECTRUM = "speaker_reverberation_early_ch0", "Speaker_reverberation_early_ch0"


def _config(tmp, *overlays, overrides=()):
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", *overlays)]
                           + [f"eg.trainer.storage_dir={tmp}", *overrides])
    return Experiment.from_config(cfg["eg"])


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from tssep_amd.train import loss
    torch.manual_seed(17)
    m = _config(tmp_path_factory.mktemp("freqmse"), "toy_tssep_freqmse.yaml",
                overrides=["eg.trainer.model.mask_estimator.num_averaged_permutations=1"]).trainer.model.cuda()
    assert isinstance(m.loss, loss.FreqMSE) and m.loss.target == SPECTRUM
    m.train()
    return m


@pytest.fixture(scope="module")
def batches(model):
    """per signal length: the example (made once, never written); target row j = the model's estimate of speaker
    (j + 1 + b) % K plus noise"""
    out = {}
    for N in SAMPLES:
        ex = _batch(B, K, N, seed=N)
        with torch.no_grad():
            np.random.seed(5)
            probe = dict(ex)
            o = model(probe)
            model.review(probe, o)
            est = o.time_estimate.detach().clone()
        rot = (torch.arange(K)[None] + 1 + torch.arange(B)[:, None]) % K
        g = torch.Generator().manual_seed(N + 1)
        tgt = est[torch.arange(B)[:, None], rot.cuda()] + 0.2 * est.std() * torch.randn(B, K, N, generator=g).cuda()
        ex[SIGNAL] = tgt.contiguous()
        ex.pop("Vad", None)
        out[N] = (ex, torch.argsort(rot, dim=1).int().cuda())          # estimate i belongs to target row inverse(rot)[i]
    return out


def _chunk_frames():
    from tssep_amd import _lib
    return 2 ** 20 // _lib.lib().tssep_specmse_chunks(2 ** 20)


def _step(m, ex0, pit, route="fused", fold_tail=0, hook=False):
    """one eager step -> dict(loss [B], total, grads, out, ex, dlogit (with hook), perm)"""
    from tssep_amd.train import runtime
    m.loss.pit, m.loss.permutation = pit, None
    got = {}
    with runtime.applied(fold_tail=fold_tail):
        m.zero_grad()
        np.random.seed(5)                                   # (random_speaker_order draws the permutation from numpy)
        ex = dict(ex0)
        out = m(ex)
        logit4 = out._fusable[0]
        if hook:
            logit4.register_hook(lambda g: got.__setitem__("dlogit", g.detach().clone()))
        if route == "materialised":
            assert out.stft_estimate.dtype == torch.complex64 and out.materialised
        summary = m.review(ex, out)
        got["fused"] = getattr(out, "_spec_loss", None) is not None
        got["materialised_after_review"] = out.materialised
        summary["loss"].backward()
        torch.cuda.synchronize()
    got.update(loss=torch.stack([s.detach() for s in summary["scalars"]["e_FreqMSE"]]), total=summary["loss"].detach().clone(),
               grads={k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, out=out, ex=ex,
               perm=m.loss.permutation, logit=logit4.detach(), obs=out._fusable[1])
    assert len(got["grads"]) > 10 and all(bool(torch.isfinite(g).all()) for g in got["grads"].values())
    return got


def _reference(got, pit, fused):
    """float64 loss [B] and d(logit) with their bounds, from the step's own logits, Observation and target spectrum"""
    lg, o, S = got["logit"].double(), got["obs"].to(torch.complex128), got["ex"][SPECTRUM].to(torch.complex128)
    E, e_E = R.ref_estimate(lg, o)
    ct = _chunk_frames()
    # (the materialised route's estimate is the mask head's fl(m^ Y_c), the fused kernel's own: the same e_E either way)
    cost, tol = R.ref_costs(E, S, e_E, ct=ct, diag_only=not pit)
    loss, t_loss, perm, gap = R.ref_loss(cost, tol, pit)
    assert bool((gap >= 100 * t_loss).all()), (gap.tolist(), t_loss.tolist())
    gout = torch.ones(lg.shape[0], device=lg.device)
    dl, t_dl = R.ref_mask_bwd(lg, o, S, perm if pit else None, gout, unfused=not fused)
    return loss, t_loss, perm, dl, t_dl


@pytest.mark.parametrize("pit", [False, True], ids=["plain", "pit"])
@pytest.mark.parametrize("N", SAMPLES)
def test_both_routes_against_float64(model, batches, N, pit):
    ex0, want_perm = batches[N]
    runs = {}
    for route in ("fused", "materialised"):
        got = runs[route] = _step(model, ex0, pit, route, fold_tail=0, hook=True)
        assert got["fused"] is (route == "fused")
        assert got["ex"][SPECTRUM].dtype == torch.complex64 and tuple(got["ex"][SPECTRUM].shape) == tuple(got["logit"].shape)
        loss, t_loss, perm, dl, t_dl = _reference(got, pit, route == "fused")
        R.within(got["loss"], loss, t_loss, f"{route} loss N={N} pit={pit}")
        if pit:
            assert torch.equal(got["perm"], perm) and torch.equal(perm, want_perm), (got["perm"].tolist(), perm.tolist())
            assert got["perm"].dtype == torch.int32 and not got["perm"].requires_grad
        else:
            assert got["perm"] is None
        R.within(got["dlogit"], dl, t_dl, f"{route} d(logit) N={N} pit={pit}")
    # the two routes' parameter gradients: the project's in-run gradient bar, 1e-3 of each tensor's largest entry
    a, b = runs["fused"]["grads"], runs["materialised"]["grads"]
    assert set(a) == set(b)
    for k in a:
        assert float((a[k] - b[k]).abs().max()) <= 1e-3 * float(b[k].abs().max()), k


@pytest.mark.parametrize("pit", [False, True], ids=["plain", "pit"])
def test_every_fold_gives_the_unfolded_gradients_bit_for_bit(model, batches, pit):
    for N in SAMPLES:
        ref = _step(model, batches[N][0], pit, fold_tail=0)
        assert ref["fused"] and getattr(ref["out"]._fusable[0], "_tssep_head_link", None) is None
        for fold in (1, 2, 3):
            got = _step(model, batches[N][0], pit, fold_tail=fold)
            assert got["fused"]
            assert getattr(got["out"]._fusable[0], "_tssep_head_link", None) is not None, "the head offered no link"
            assert torch.equal(got["loss"], ref["loss"]) and set(got["grads"]) == set(ref["grads"])
            for k in ref["grads"]:
                assert torch.equal(got["grads"][k], ref["grads"][k]), (N, fold, k)


def test_time_estimate_is_computed_on_first_read(model, batches):
    N = SAMPLES[1]
    got = _step(model, batches[N][0], False)
    out = got["out"]
    assert got["fused"] and got["materialised_after_review"] is False and not out.materialised
    assert "<lazy>" in repr(out)
    with torch.no_grad():
        te = out.time_estimate
        assert out.materialised and tuple(te.shape) == (B, K, N)
        assert torch.equal(te, model.fe.istft(out.stft_estimate, num_samples=N))
        assert out.time_estimate is te
        again = out.fresh()
        assert not again.materialised and torch.equal(again.time_estimate, te) and again.time_estimate is not te
    out.time_estimate = None                                   # the setter: user code may still assign
    assert out.time_estimate is None


def test_graphed_step_replays_the_eager_steps(model, batches):
    from tssep_amd import hip_ops
    from tssep_amd.train.graph import GraphedStep
    from tssep_amd.train.optimizer import Adam
    m = model
    m.loss.pit, m.loss.permutation = True, None
    N = SAMPLES[0]
    ex0, _ = batches[N]
    exs = [dict(ex0)]
    for s in (1, 2):                                           # other relabellings of the same targets
        e = dict(ex0)
        e[SIGNAL] = torch.roll(ex0[SIGNAL], s, dims=1).contiguous()
        exs.append(e)
    opt = Adam(gradient_clipping=10.0)
    opt.set_parameters(m.parameters())
    start = opt.flat_param.clone()

    def restart():
        opt.flat_param.copy_(start)
        opt.exp_avg.zero_(), opt.exp_avg_sq.zero_()
        opt.step_count = 0
        hip_ops.weights_changed()

    want = []
    for i, e in enumerate(exs):
        np.random.seed(60 + i)
        opt.zero_grad()
        e = dict(e)
        out = m(e)
        value = m.review(e, out)["loss"]
        assert getattr(out, "_spec_loss", None) is not None
        value.backward()
        opt.step()
        torch.cuda.synchronize()
        want.append((value.detach().clone(), m.loss.permutation.clone(), opt.flat_param.clone()))
    # (the speaker order drawn for these steps is not the one the targets were made under: only that the choice moves)
    assert not torch.equal(want[0][1], want[1][1]) and not torch.equal(want[1][1], want[2][1])
    restart()
    g = GraphedStep(m, opt)
    assert g.usable(exs[0])
    for i in (0, 1, 2):
        np.random.seed(60 + i)
        _, summary = g(dict(exs[i]))
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(summary["loss"].detach(), want[i][0]), (i, float(summary["loss"]), float(want[i][0]))
        assert torch.equal(m.loss.permutation, want[i][1]), i
        assert torch.equal(opt.flat_param, want[i][2]), (i, float((opt.flat_param - want[i][2]).abs().max()))
    assert g.replays == 3 and g.eager_steps == 0 and len(g._graphs) == 1
    restart()
    m.loss.pit = False


def test_complex128_estimate_of_the_beamformer(tmp_path):
    """FreqMSE over TorchBF(differentiable=True) with nmask = 2: the generic pair's complex128 entry points"""
    from tssep_amd.train import enhancer as E, loss
    from test_gpu_two_mask import D, K as K3, N as N3, SMALL
    torch.manual_seed(3)
    m = _config(tmp_path, "toy_tssep_two_mask.yaml", "toy_tssep_freqmse.yaml", overrides=SMALL).trainer.model.cuda()
    assert isinstance(m.enhancer, E.TorchBF) and m.enhancer.differentiable and m.mask_estimator.nmask == 2
    assert isinstance(m.loss, loss.FreqMSE)
    ex = next(iter(m.prepare_train_dataset(torch.device("cuda"), batch_size=1, prefetch=False)))
    mix = ex["observation"][0, 0, :N3]
    g = torch.Generator(device="cpu").manual_seed(3)
    obs = torch.stack([a * torch.roll(mix, d) for a, d in ((1.0, 0), (0.8, 3), (0.6, 7))])
    obs = obs + 0.05 * mix.abs().max() * torch.randn(D, N3, generator=g).to(obs)
    ex = dict(ex, observation=obs[None], auxInput=ex["auxInput"][:, :K3].contiguous(), reference_channel=0)
    ex[SIGNAL] = ex[SIGNAL][:, :K3, :N3].contiguous()
    m.zero_grad()
    np.random.seed(5)
    out = m(ex)
    summary = m.review(ex, out)
    summary["loss"].backward()
    torch.cuda.synchronize()
    assert getattr(out, "_spec_loss", None) is None and out.stft_estimate.dtype == torch.complex128
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.any()) for x in grads)
    est = out.stft_estimate.detach()
    S = ex[SPECTRUM].to(torch.complex128)
    assert est.shape == S.shape and est.shape[0] == 1
    cost, tol = R.ref_costs(est, S, None, ct=_chunk_frames(), diag_only=True)
    ref, t_ref, _, _ = R.ref_loss(cost, tol, False)
    R.within(summary["loss"].detach().reshape(1), ref, t_ref, "FreqMSE on the beamformer's complex128 estimate")


def test_logmae_step_is_what_it_was(model, batches):
    """An existing route beside the new code: a LogMAE step before and after FreqMSE steps on the same model -- the same
    loss bits and gradients, on the fused time-domain tail (and never through the spectral one)."""
    from tssep_amd.train import loss
    m = model
    spectral = m.loss
    ex0 = dict(batches[SAMPLES[0]][0])

    def logmae_step():
        m.zero_grad()
        np.random.seed(5)
        ex = dict(ex0)
        out = m(ex)
        total = m.review(ex, out)["loss"]
        assert getattr(out, "_spec_loss", None) is None and SPECTRUM not in ex
        assert getattr(out.time_estimate, "_tssep_loss_link", None) is not None
        total.backward()
        torch.cuda.synchronize()
        return total.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    try:
        m.loss = loss.LogMAE().cuda()
        before = logmae_step()
        m.loss = spectral
        _step(m, ex0, True, fold_tail=1)
        m.loss = loss.LogMAE().cuda()
        after = logmae_step()
    finally:
        m.loss = spectral
    assert torch.equal(before[0], after[0]) and set(before[1]) == set(after[1])
    for k in before[1]:
        assert torch.equal(before[1][k], after[1][k]), k
