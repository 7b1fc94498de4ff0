"""loss.SDR end to end on a real MI355X, on the toy Model of the PIT tests: the parameter gradients against the same formula
written in torch on out.time_estimate, relabelled targets under pit=True, the metric hip_ops.sdr, graph capture and replay
with the permutation and the values recomputed, and the joint loss of an explicit_vad estimator.

Tolerances.  A loss value: the K matched values each within the bound of tests/sdr_reference.py (dvalue), over K, plus the
K - 1 float32 adds of tssep_pit_assign.  Parameter gradients: both runs push a d(time_estimate) through the SAME backward
kernels, which are linear in it; the two d(time_estimate) differ element-wise by at most the backward bound of
sdr_reference.grad (the torch formula runs in float64 and is rounded once: + 2^-24), i.e. by rho = |bound|_2 / |dy|_2 in
relative L2 norm (2e-3 on the toy batch at 14 dB: P e and Q t nearly cancel there, and the bound is the worst case of 32
aligned roundings).  A linear map amplifies a relative perturbation only where its result cancels; the backward chain is
given a factor 4 for that, and 2^-20 for its own float32 roundings on two different inputs:
    |dg|_max <= 4 (rho + 2^-20) |g|_max   per parameter tensor
-- below the 2.5 % by which a gradient without tau would differ at sdr_max = 30.  Seen on the MI355X: 1e-3 of it."""
import numpy as np
import pytest
import torch

import pit_reference as PR
import sdr_reference as R
from test_gpu_pit import TARGET, _step, _take, toy  # noqa: F401  (toy: the module-scoped fixture, instantiated here)

pytestmark = pytest.mark.gpu

T_ = torch.as_tensor
MODES = [(True, None), (True, 30.0), (False, None), (False, 30.0)]


def _loss_bound(ref, perm):
    K = perm.shape[-1]
    dv = np.take_along_axis(ref["dvalue"], perm[..., None], axis=2)[..., 0]
    cost = np.take_along_axis(ref["cost"], perm[..., None], axis=2)[..., 0]
    return dv.sum(-1) / K + (K + 1) * R.U * np.abs(cost).sum(-1)


def _torch_sdr(loss_module, scale_invariant, sdr_max, eps):
    """The plain formula in float64 torch as a time-domain loss module that Model.review routes as it routes MSE."""
    tau = R.tau_of(sdr_max)

    class TorchSDR(loss_module.TimeDomain):
        power = 2                                          # (not an L1 loss: never formed by the fused tail)

        def loss_fn(self, estimate, target):
            e, t = estimate.double(), target.double()
            a, b, c = (e * e).sum(-1), (t * t).sum(-1), (e * t).sum(-1)
            if scale_invariant:
                s = c / (b + eps) * c
                n = a - s
            else:
                s = b
                n = torch.clamp(a - 2 * c + b, min=0)
            return (-(10 * torch.log10((s + eps) / (n + tau * s + eps))).mean(-1)).float()

    return TorchSDR()


@pytest.mark.parametrize("scale_invariant,sdr_max", MODES)
def test_parameter_gradients_against_the_formula_in_torch(toy, scale_invariant, sdr_max):
    from tssep_amd.train import loss
    m, ex, tgt, _ = toy
    B, K, N = tgt.shape
    eps = 1e-8
    batch = dict(ex, **{TARGET: tgt})
    m.loss = loss.SDR(scale_invariant=scale_invariant, sdr_max=sdr_max, eps=eps)
    got, out, ggot = _step(m, batch)
    assert getattr(out.time_estimate, "_tssep_loss_link", None) is None          # the fused tail did not form the loss
    values = m.loss.values.cpu().numpy()
    assert m.loss.permutation is None and tuple(values.shape) == (B, K)
    est = out.time_estimate.detach().cpu().numpy()
    m.loss = _torch_sdr(loss, scale_invariant, sdr_max, eps)
    want, _, gwant = _step(m, batch)
    m.loss = loss.LogMAE()
    ident = np.tile(np.arange(K), (B, 1))
    ref = R.loss(est, tgt.cpu().numpy(), scale_invariant, sdr_max, eps, pit=False)
    assert np.all(np.abs(values - ref["values"]) <= np.take_along_axis(ref["dvalue"], ident[..., None], axis=2)[..., 0])
    bound = float(_loss_bound(ref, ident).sum())
    assert abs(got - float(ref["loss"].sum())) <= bound + B * R.U * abs(got), (got, ref["loss"].sum(), bound)
    assert abs(got - want) <= bound + 2 * B * R.U * abs(got), (got, want, bound)
    dy, dy_bound = R.grad(est, tgt.cpu().numpy(), ident, scale_invariant, sdr_max, eps)
    rho = float(np.linalg.norm(dy_bound + R.U * np.abs(dy)) / np.linalg.norm(dy))
    tol = 4 * (rho + 2.0 ** -20)
    assert set(ggot) == set(gwant) and len(ggot) > 10
    worst = 0.0
    for k in gwant:
        scale = float(gwant[k].abs().max())
        err = float((ggot[k] - gwant[k]).abs().max())
        worst = max(worst, err / max(scale, 1e-30) / tol)
        assert err <= tol * scale, (k, err, scale, tol)
    print(f"sdr model gradients si={scale_invariant} sdr_max={sdr_max}: level {values.mean():.2f} dB, rho {rho:.3g}, "
          f"worst error / tolerance {worst:.4f}")


@pytest.mark.parametrize("scale_invariant,sdr_max", [(True, None), (False, 30.0)])
@pytest.mark.parametrize("K,N", [(2, 1000), (3, 4099), (8, 8200)])
def test_relabelled_targets_against_plain_targets(K, N, scale_invariant, sdr_max):
    """pit=True on tgt[:, q] equals pit=False on tgt; .permutation == inverse(q); .values line up with the estimates;
    hip_ops.sdr returns the same values and permutation; tgt gets no gradient; [K, N] input is squeezed back."""
    from tssep_amd import hip_ops as H
    from tssep_amd.train import loss
    B = 3
    e0, t0 = R.planted(B, K, N, 10.0, seed=K * N)
    tgt, est0 = T_(t0).cuda(), T_(e0).cuda()
    rng = np.random.RandomState(K + N)
    q = np.stack([rng.permutation(K) for _ in range(B)])
    w = T_(np.array([1.0, -2.0, 0.5], dtype=np.float32)).cuda()
    res = {}
    for pit in (False, True):
        lo = loss.SDR(pit=pit, scale_invariant=scale_invariant, sdr_max=sdr_max)
        est = est0.clone().requires_grad_()
        t = (_take(tgt, q) if pit else tgt.clone()).requires_grad_()
        val = lo(est, t)
        assert tuple(val.shape) == (B,)
        (val * w).sum().backward()
        assert t.grad is None
        assert not lo.values.requires_grad and tuple(lo.values.shape) == (B, K)
        res[pit] = (val.detach().cpu().numpy(), est.grad.cpu().numpy(), lo.permutation, lo.values.cpu().numpy())
        mv, mp = H.sdr(est.detach(), t.detach(), scale_invariant, sdr_max, 1e-8, pit=pit)
        assert torch.equal(mv, lo.values) and not mv.requires_grad
        assert torch.equal(mp, lo.permutation) if pit else np.array_equal(mp.cpu().numpy(), np.tile(np.arange(K), (B, 1)))
    ref = R.loss(e0, _take(tgt, q).cpu().numpy(), scale_invariant, sdr_max, 1e-8, pit=True)
    assert np.array_equal(ref["perm"], PR.inverse(q)) and np.all(ref["gap"] > 4 * K * ref["dvalue"].max())
    assert res[False][2] is None
    perm = res[True][2]
    assert perm.dtype == torch.int32 and not perm.requires_grad and tuple(perm.shape) == (B, K)
    assert np.array_equal(perm.cpu().numpy(), PR.inverse(q))
    bound = _loss_bound(ref, ref["perm"])
    assert np.all(np.abs(res[True][0] - ref["loss"]) <= bound) and np.all(np.abs(res[False][0] - ref["loss"]) <= bound)
    # the same pairs are matched: the same statistics in another column of the K x K accumulators, the same coefficients
    assert np.array_equal(res[True][3], res[False][3]) and np.array_equal(res[True][1], res[False][1])
    R.check_backward(res[True][1], e0, _take(tgt, q).cpu().numpy(), PR.inverse(q), scale_invariant, sdr_max, 1e-8,
                     w.cpu().numpy())
    lo = loss.SDR(pit=True, scale_invariant=scale_invariant, sdr_max=sdr_max)
    one = lo(est0[1], _take(tgt, q)[1])
    assert one.dim() == 0 and tuple(lo.permutation.shape) == (K,) and tuple(lo.values.shape) == (K,)
    assert float(one) == float(res[True][0][1]) and np.array_equal(lo.permutation.cpu().numpy(), PR.inverse(q)[1])
    assert np.array_equal(lo.values.cpu().numpy(), res[True][3][1])


def test_loss_graph_replay_recomputes_permutation_and_values(toy):
    """forward + loss + backward of SDR(pit=True) captured with torch.cuda.graph: each of 4 replays equals its eager run
    bit for bit, and permutation and values follow the contents of the static target buffer."""
    from tssep_amd.train import loss
    _, _, tgt, (qa, qb) = toy
    base = (tgt + 0.01 * torch.randn_like(tgt)).detach()
    lo = loss.SDR(pit=True, sdr_max=30.0)

    def eager(t):
        est = base.clone().requires_grad_()
        v = lo(est, t)
        v.sum().backward()
        torch.cuda.synchronize()
        return v.detach().clone(), lo.permutation.clone(), lo.values.clone(), est.grad.clone()

    want = [eager(_take(tgt, q)) for q in (qa, qb)]
    s_est, s_tgt = base.clone().requires_grad_(), _take(tgt, qa).clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lo(s_est, s_tgt).sum().backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    s_est.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_val = lo(s_est, s_tgt)
        s_val.sum().backward()
    s_perm, s_values = lo.permutation, lo.values
    for q, (v, perm, values, grad) in zip((qa, qb, qa, qb), want + want):
        s_tgt.copy_(_take(tgt, q))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_val.detach(), v) and torch.equal(s_est.grad, grad)
        assert torch.equal(s_perm, perm) and np.array_equal(s_perm.cpu().numpy(), PR.inverse(q))
        assert torch.equal(s_values, values)
    assert not np.array_equal(PR.inverse(qa), PR.inverse(qb))


def test_graphed_step_with_sdr(toy):
    """The whole training step through GraphedStep: capturable without a host sync, and each of 4 replays reports the
    permutation and the values of ITS targets and the eager step's loss and gradients, bit for bit."""
    from tssep_amd.train import loss
    from tssep_amd.train.graph import GraphedStep
    from tssep_amd.train.optimizer import Adam
    m, ex, tgt, (qa, qb) = toy
    m.loss = loss.SDR(pit=True)
    opt = Adam(gradient_clipping=10.0)
    opt.set_parameters(m.parameters())
    exs = [dict(ex, **{TARGET: _take(tgt, q)}) for q in (qa, qb)]
    want = []
    for e in exs:
        opt.zero_grad()
        out = m(dict(e))
        value = m.review(dict(e), out)["loss"]
        value.backward()
        opt.bucket.sync()
        torch.cuda.synchronize()
        want.append((value.detach().clone(), m.loss.permutation.clone(), m.loss.values.clone(), opt.bucket.flat.clone()))
    g = GraphedStep(m, opt)
    assert g.usable(exs[0])
    g(dict(exs[0]))                                                # warm-up, capture, first replay
    for i in (1, 0, 1, 0):
        _, summary = g(dict(exs[i]))
        torch.cuda.synchronize()
        diff = float((opt.bucket.flat - want[i][3]).abs().max())
        print(f"graphed sdr step {i}: loss {float(summary['loss'])!r} eager {float(want[i][0])!r}, gradient difference {diff:.3g}")
        assert torch.equal(m.loss.permutation, want[i][1]) and torch.equal(m.loss.values, want[i][2])
        assert float(summary["loss"]) == float(want[i][0])
        assert torch.equal(opt.bucket.flat, want[i][3])
    assert g.replays == 5 and g.eager_steps == 0 and len(g._graphs) == 1
    assert not torch.equal(want[0][1], want[1][1])
    m.loss = loss.LogMAE()


def test_joint_loss_on_an_explicit_vad_estimator():
    """SignalAndVADSigmoidBCE(signal_loss=SDR()) through Model.review: the loss is the sum of its two terms computed
    separately (the SDR of out.time_estimate; the BCE of out.vad_logit against Vad), and every parameter gets a finite
    gradient.  Tolerance: the BCE is reduced by two different kernels, K T < 128 float32 terms each."""
    from test_gpu_explicit_vad import _batch, _model
    from tssep_amd.train import loss
    m = _model(random_speaker_order=False)
    m.loss = loss.SignalAndVADSigmoidBCE(signal_loss=loss.SDR(sdr_max=30.0))
    m.train()
    B, K, N = 2, 4, 7000
    ex0 = _batch(B, K, N, seed=3)
    m.zero_grad()
    ex = dict(ex0)
    out = m(ex)
    assert out.logit is None
    total = m.review(ex, out)["loss"]
    total.backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert len(grads) > 10 and all(bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().max()) > 0 for g in grads)
    with torch.no_grad():
        sdr_term = loss.SDR(sdr_max=30.0)(out.time_estimate.detach(), ex0[TARGET])
        bce_term = loss.VADSigmoidBCE()._bce(torch.squeeze(out.vad_logit.detach()[..., None], dim=-3).contiguous(), ex0["Vad"])
    a, b = float(sdr_term.sum()), float(bce_term.sum())
    assert abs(float(total) - (a + b)) <= 128 * R.U * (abs(a) + abs(b)), (float(total), a, b)
    assert tuple(m.loss.signal_loss.values.shape) == (B, K) and m.loss.signal_loss.permutation is None
