"""nmask = 2 end to end on the device: MaskEstimator_v2(nmask=2) against the CPU oracle, a toy Model trained through
TorchBF(differentiable=True) against CPU autograd of a float64 restatement, the toy overlay through the Trainer, and the
nmask = 1 step unchanged.  Toy sizes as in test_gpu_mvdr_backward.py::test_toy_model_end_to_end: units 10, projs 12,
K = 3, three channels, N = 16000."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import net as onet  # noqa: E402
from test_gpu_kernels import close  # noqa: E402
from test_gpu_mvdr_backward import restated_istft  # noqa: E402
import test_mvdr_backward_reference as Bk  # noqa: E402
import test_two_mask_reference as R  # noqa: E402

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
K, D, N = 3, 3, 16000
SMALL = ["eg.trainer.model.mask_estimator.units=10", "eg.trainer.model.mask_estimator.projs=12",
         f"eg.trainer.model.mask_estimator.ts_vad={K}"]


@pytest.mark.parametrize("ts_vad,res,nap", [(False, "tf", 1), (False, "t", 1), (K, "tf", 1), (K, "t", 1), (K, "tf", 2)])
@pytest.mark.parametrize("gemm", ["f32", "bf16x3"])
def test_two_mask_estimator_against_the_oracle(ts_vad, res, nap, gemm):
    """mask and logit [B, K, 2, T, F] of MaskEstimator_v2(nmask=2) against oracle.net.mask_estimator_forward(nmask=2) on
    the same weights and permutations.  Tolerances: those of the nmask = 1 parity test for the same GEMM arithmetic,
    tests/test_gpu_modules.py:72-73 (logit rtol 1e-3, atol 5e-6 a; mask rtol 1e-3, atol 2e-6 a; a = 1 for exact fp32
    GEMMs, 10 for split-bf16, line 60)."""
    from tssep_amd import hip_ops
    from tssep_amd.train.net import MaskEstimator_v2
    a = 1 if gemm == "f32" else 10
    B, T = 2, 63
    torch.manual_seed(11)
    me = MaskEstimator_v2(idim=553, odim=513, units=10, projs=12, combination="mul", aux_net_output_size=513, nmask=2,
                          ts_vad=ts_vad, output_resolution=res, num_averaged_permutations=nap).cuda()
    g = torch.Generator().manual_seed(12)
    feat = torch.randn(B, T, 553, generator=g)
    aux = torch.rand(B, K, 513, generator=g)
    old = hip_ops.GEMM_PRECISION
    hip_ops.GEMM_PRECISION = gemm
    try:
        np.random.seed(5)
        out = me(feat.cuda(), aux.cuda())
    finally:
        hip_ops.GEMM_PRECISION = old
    np.random.seed(5)
    perm = me.draw_permutations(B, K)[0]
    p = {"mask_estimator." + k: v.detach().cpu().double() for k, v in me.state_dict().items()}
    ref = onet.mask_estimator_forward(p, feat.double(), aux.double(), odim=513, nmask=2, combination="mul", ts_vad=ts_vad,
                                      output_resolution=res, num_averaged_permutations=nap, perm=perm)
    assert tuple(out.logit.shape) == tuple(out.mask.shape) == (B, K, 2, T, 513) == tuple(ref["logit"].shape)
    assert float((ref["logit"][:, :, 0] - ref["logit"][:, :, 1]).abs().max()) > 1e-3            # two different masks
    close(out.logit, ref["logit"].float(), rtol=1e-3, atol=5e-6 * a, name="logit")
    close(out.mask, ref["mask"].float(), rtol=1e-3, atol=2e-6 * a, name="mask")
    # an unbatched example takes the same route
    np.random.seed(5)
    one = me(feat[0].cuda(), aux[0].cuda())
    assert tuple(one.logit.shape) == tuple(one.mask.shape) == (K, 2, T, 513) and tuple(one.embedding.shape) == (K, 1, 513)


def _toy_model(tmp_path, *overlays, overrides=()):
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", *overlays)]
                           + [f"eg.trainer.storage_dir={tmp_path}", *SMALL, *overrides])
    return Experiment.from_config(cfg["eg"])


def _three_channels(m, ex):
    tgt_key = m.loss.target
    mix = ex["observation"][0, 0, :N]
    g = torch.Generator(device="cpu").manual_seed(3)
    obs = torch.stack([a * torch.roll(mix, d) for a, d in ((1.0, 0), (0.8, 3), (0.6, 7))])          # delayed, scaled copies
    obs = obs + 0.05 * mix.abs().max() * torch.randn(D, N, generator=g).to(obs)                    # + noise per channel
    ex = dict(ex, observation=obs[None], auxInput=ex["auxInput"][:, :K].contiguous(), reference_channel=0)
    ex[tgt_key] = ex[tgt_key][:, :K, :N].contiguous()
    return ex


def test_toy_model_end_to_end(tmp_path, monkeypatch):
    """Model.forward + review + backward with nmask = 2, TorchBF(differentiable=True), LogMAE: the loss, d(loss)/d(logit)
    [1, K, 2, T, F] and the final Linear's weight gradient against CPU autograd of the float64 restatement
    torch_bf(sigmoid(l), Y, 0) -> istft -> LogMAE, l = the restated tail of the final Linear (test_two_mask_reference.py)
    on the HIP path's own input of that Linear.  Bars: loss 1e-4 max(1, |loss|), gradients 1e-3 of the largest entry."""
    from tssep_amd import functional as Fn
    from tssep_amd.train import enhancer as E
    m = _toy_model(tmp_path, "toy_tssep_two_mask.yaml").trainer.model.cuda()
    me = m.mask_estimator
    assert isinstance(m.enhancer, E.TorchBF) and m.enhancer.differentiable and me.nmask == 2
    ex = _three_channels(m, next(iter(m.prepare_train_dataset(torch.device("cuda"), batch_size=1, prefetch=False))))
    tgt_key = m.loss.target
    box = {}
    head_masks, map_bwd = Fn.head_masks, Fn.H.mask_map_bwd

    def keep_head(x, linear, perm, iperm, *geo, **kw):
        box.update(h=x.detach(), perm=perm, iperm=iperm, geo=geo, kw=kw)
        return head_masks(x, linear, perm, iperm, *geo, **kw)

    def keep_draw(dmask, mask, dlogit, *a):
        box["dlogit_in"] = dlogit
        box["draw"] = map_bwd(dmask, mask, dlogit, *a)
        return box["draw"]
    monkeypatch.setattr(Fn, "head_masks", keep_head)
    monkeypatch.setattr(Fn.H, "mask_map_bwd", keep_draw)
    m.zero_grad()
    out = m(ex)
    assert tuple(out.mask.shape) == tuple(out.logit.shape) == (1, K, 2, out.mask.shape[-2], 513)
    summary = m.review(ex, out)
    summary["loss"].backward()
    assert ex["Observation"].dtype == torch.complex64 and out.stft_estimate.dtype == torch.complex128
    assert tuple(out.time_estimate.shape) == (1, K, N) and box["dlogit_in"] is None          # nobody else used the logit
    B, Kk, M, T, F, trials, Fr = box["geo"]
    spk_rows = int(box["kw"]["spk_rows"])
    assert (B, Kk, M, F, Fr, spk_rows) == (1, K, 2, 513, 513, 0) and trials == me.num_averaged_permutations
    perm, iperm = box["perm"].cpu(), box["iperm"].cpu()
    # d(loss)/d(logit) of the HIP chain: every trial's raw run holds d(logit) / trials of its speaker
    got = R.unpermute(R.raw_to_trials(box["draw"].double().cpu(), B, trials, K, M, T, Fr, spk_rows).sum(1), iperm)
    # the restatement, from the final Linear's input
    lin = me._linear
    w64 = lin.weight.detach().double().cpu().requires_grad_()
    b64 = lin.bias.detach().double().cpu()
    raw = box["h"].double().cpu().reshape(-1, w64.shape[1]) @ w64.t() + b64
    l64, mask64 = R.ref_fwd(raw.reshape(-1), iperm, B, trials, K, M, T, F, Fr, spk_rows)
    l64.retain_grad()
    close(out.logit, l64.detach().float(), rtol=1e-3, atol=5e-5, name="logit of the step")
    Y = ex["Observation"].to(torch.complex128).cpu()                              # [1, D, T, F]
    enh = Bk.torch_bf(torch.sigmoid(l64), Y, 0)
    wsyn = Fn.windows("hann", 1024, 256, torch.device("cuda"))[1].double().cpu()
    est = restated_istft(enh, wsyn, 1024, 256, N)
    loss = torch.log10((est - ex[tgt_key].double().cpu()).abs().mean(-1).sum(-1)).sum()
    loss.backward()
    want = l64.grad
    hip_loss = float(summary["loss"].detach())
    err = float((got - want).abs().max()) / float(want.abs().max())
    gw = lin.weight.grad.double().cpu()
    err_w = float((gw - w64.grad).abs().max()) / float(w64.grad.abs().max())
    print(f"two-mask toy model: loss HIP {hip_loss:.8g}, float64 restatement {float(loss):.8g}; d(loss)/d(logit) max error "
          f"{err:.3g} of the largest entry ({float(want.abs().max()):.3g}); d(loss)/d(W) {err_w:.3g} of "
          f"{float(w64.grad.abs().max()):.3g}")
    assert tuple(got.shape) == tuple(want.shape) == (1, K, 2, T, F) and float(want.abs().max()) > 0
    assert abs(hip_loss - float(loss)) <= 1e-4 * max(1.0, abs(float(loss)))
    assert err <= 1e-3
    assert err_w <= 1e-3
    rows = gw.view(K, 2, F, -1)                                                   # '(spk mask freq)' rows of the Linear
    assert bool(rows[:, 0].any()) and bool(rows[:, 1].any())
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    # evaluation: the default TorchBF under no_grad takes the same masks
    m.enhancer.differentiable = False
    with torch.no_grad():
        ev = m(dict(ex))
        assert tuple(ev.stft_estimate.shape) == (1, K, T, F) and ev.stft_estimate.dtype == torch.complex128


class _Dataset(list):
    def __iter__(self):
        return (dict(ex) for ex in list.__iter__(self))


def _train(tmp_path, *overlays, iterations):
    from tssep_amd.train import runtime
    eg = _toy_model(tmp_path, *overlays, overrides=[f"eg.trainer.stop_trigger=[{iterations},iteration]",
                                                    "eg.trainer.summary_trigger=[1,iteration]",
                                                    "eg.trainer.checkpoint_trigger=[1000,iteration]"])
    tr = eg.trainer
    m = tr.model.cuda()
    data = []
    for i, ex in enumerate(m.prepare_train_dataset(torch.device("cuda"), batch_size=1, prefetch=False)):
        data.append(_three_channels(m, ex))
        if len(data) == iterations:
            break
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    with runtime.applied(**eg.runtime):
        np.random.seed(9)
        hist = tr.train(_Dataset(data), device=0)
        torch.cuda.synchronize()
    return tr, m, before, hist


def test_trainer_with_the_two_mask_overlay(tmp_path):
    """Three iterations with toy_tssep_two_mask.yaml: finite losses, every parameter changes, the GraphedStep sends every
    step down the eager path (TorchBF's singular check is a host sync), and the first step's kernel plan lists the fused
    tail's two launches."""
    tr, m, before, hist = _train(tmp_path, "toy_tssep_two_mask.yaml", iterations=3)
    losses = [l for _, l in hist]
    assert len(losses) == 3 and all(np.isfinite(losses)), losses
    same = [k for k, v in m.named_parameters() if torch.equal(v.detach(), before[k])]
    assert not same, same
    g = tr.graph_step
    assert g is not None and g.eager_reason is not None and "TorchBF" in g.eager_reason and g.replays == 0 and not g._graphs
    h = json.loads((tmp_path / "log" / "history.json").read_text())
    assert h["iteration"] == 3 and h.get("graph_replays", 0) == 0
    plan = json.loads((tmp_path / "log" / "kernel_plan.json").read_text())
    assert [e["kernel"] for e in plan["tail"]] == ["mask_map_fwd", "mask_map_bwd"], plan["tail"]
    assert all(e["M"] == 2 and e["K"] == K and e["F"] == 513 for e in plan["tail"])


def test_one_mask_step_runs_no_mask_map_launch(tmp_path):
    """nmask = 1 (toy_tssep.yaml as it is): the recorded kernel plan of the first step has no fused two-mask launch."""
    from tssep_amd.train import enhancer as E
    tr, m, _, hist = _train(tmp_path, iterations=1)
    assert m.mask_estimator.nmask == 1 and isinstance(m.enhancer, E.Masking) and np.isfinite(hist[0][1])
    assert tr.kernel_plan["tail"] == []
    plan = json.loads((tmp_path / "log" / "kernel_plan.json").read_text())
    assert plan["tail"] == [] and sum(plan["gemm"].values()) > 0
