"""The hand-offs around the fused tail (functional: head -> mask / iSTFT -> LogMAE / MAE) on a real MI355X, route by route.

``fold_tail`` = 1 folds the loss gradient into the tail's backward and writes d(logit) where the final Linear's backward
reads it; 2 folds the loss only, 3 the layout only, 0 neither.  A second consumer of the time estimate, or of the head's
logit rows, makes the consumer of a link fall back to the unfused kernels for the linked part and add it.  Every route
must give the gradients of ``fold_tail`` = 0 bit for bit: the folded kernel forms the loss gradient with the arithmetic of
``tssep_logmae_bwd``, the bt-major store is a permutation of the [B,K,T,F] one, and a fallback adds the same two terms
autograd would have added.

The model is the toy experiment's (toy_common.yaml + toy_tssep.yaml, + toy_tssep_explicit_vad.yaml for the gated rows) with
one override, ``num_averaged_permutations=1``: the head offers its link only for a single trial, and a test of the link
routes with two trials would pass without taking one."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_explicit_vad import _batch  # noqa: E402

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
B, K = 2, 8
SAMPLES = (4096, 3001)          # even: aligned sample pairs; odd: the kernel's clamped 4-byte loads
LOSSES = {"plain": ("LogMAE", "MAE"), "gated": ("LogMAE", "MAE", "joint")}
ROUTES = ("single", "estimate", "logit")
CASES = [(rows, loss, route) for rows in LOSSES for loss in LOSSES[rows] for route in ROUTES]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    out = {}
    for rows, overlays in (("plain", ()), ("gated", ("toy_tssep_explicit_vad.yaml",))):
        torch.manual_seed(17)
        cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml") + overlays] + [
            f"eg.trainer.storage_dir={tmp_path_factory.mktemp(rows)}",
            "eg.trainer.model.mask_estimator.num_averaged_permutations=1"])
        out[rows] = Experiment.from_config(cfg["eg"]).trainer.model.cuda()
    return out


@pytest.fixture(scope="module")
def batches():
    """per signal length: the example and the fixed weights of the extra terms (made once, never written)"""
    out = {}
    for N in SAMPLES:
        ex = _batch(B, K, N, seed=N)
        g = torch.Generator().manual_seed(N + 1)
        T = ex["Vad"].shape[-1]
        out[N] = (ex, torch.randn(B, K, N, generator=g).cuda(), torch.randn(B, K, 1, T, 1, generator=g).cuda())
    return out


def _loss(name):
    from tssep_amd.train import loss
    if name == "joint":
        return loss.SignalAndVADSigmoidBCE(signal_loss=loss.LogMAE())
    return getattr(loss, name)()


def _step(m, rows, route, batch, fold_tail, check_links=False):
    """one eager step -> (loss, {parameter: gradient})"""
    from tssep_amd.train import runtime
    ex0, w_est, w_logit = batch
    with runtime.applied(fold_tail=fold_tail):
        m.zero_grad()
        np.random.seed(5)                                   # (random_speaker_order draws the permutation from numpy)
        ex = dict(ex0)
        out = m(ex)
        total = m.review(ex, out)["loss"]
        if check_links:
            assert not out.materialised
            assert getattr(out._fusable[0], "_tssep_head_link", None) is not None, "the head offered no link"
            assert getattr(out.time_estimate, "_tssep_loss_link", None) is not None, "the tail offered no loss link"
        if route == "estimate":
            total = total + (out.time_estimate * w_est).sum()
        elif route == "logit":
            rows_ = out.logit if rows == "plain" else out.vad_logit[..., None]      # [B,K,1,T,F] / [B,K,1,T,1]
            total = total + (rows_ * w_logit).sum()
        total.backward()
        torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads.values())
    return total.detach().clone(), grads


def _same(a, b, what):
    assert torch.equal(a[0], b[0]), (what, "loss", float(a[0]), float(b[0]))
    assert set(a[1]) == set(b[1])
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), (what, k, float((a[1][k] - b[1][k]).abs().max()))


@pytest.mark.parametrize("rows,loss_name,route", CASES, ids=["-".join(c) for c in CASES])
def test_every_fold_gives_the_unfolded_gradients_bit_for_bit(models, batches, rows, loss_name, route):
    m = models[rows]
    m.loss = _loss(loss_name).cuda()
    for N in SAMPLES:
        ref = _step(m, rows, route, batches[N], 0)
        for fold in (1, 2, 3):
            got = _step(m, rows, route, batches[N], fold, check_links=(fold == 1 and route == "single"))
            _same(got, ref, f"N={N} fold_tail={fold}")
        if (rows, loss_name, route) == ("plain", "LogMAE", "single"):
            _same(_step(m, rows, route, batches[N], 0), ref, f"N={N} second run")
            # (and the extra terms are not inert: another route gives other gradients)
            other = _step(m, rows, "estimate", batches[N], 0)
            assert any(not torch.equal(other[1][k], ref[1][k]) for k in ref[1])
