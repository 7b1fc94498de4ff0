"""pit=True end to end on a real MI355X: the loss modules on relabelled targets, Model.review with the stand-alone
permutation-invariant loss against the fused pit=False tail, and graph replay with the permutation recomputed.

Tolerance of a loss value against the same loss computed another way (the issue's): the relative bound of the matched
cost sum, rel = (r + K - 1) 2^-24 with r the roundings of the pair-cost reduction (test_gpu_pit_kernels.roundings),
propagated through log10 as an absolute rel / ln10, plus 4 * 2^-24 * max(|loss|, 1) for log10f and the final rounding;
MAE / MSE (no logarithm): rel * |loss| instead of rel / ln10."""
import numpy as np
import pytest
import torch

import pit_reference as R
from test_gpu_pit_kernels import roundings

pytestmark = pytest.mark.gpu

T_ = torch.as_tensor
LOSSES = {"LogMAE": (1, True), "MAE": (1, False), "MSE": (2, False)}


def tolerance(value, p, log, K, N):
    rel = (roundings(p, N) + K - 1) * R.U
    value = np.abs(np.asarray(value, dtype=np.float64))
    return (rel / np.log(10) if log else rel * value) + 4 * R.U * np.maximum(value, 1)


def _take(t, q):
    """t [B, K, ...] with its rows reordered per utterance: out[b, j] = t[b, q[b, j]]."""
    idx = T_(q).to(t.device)
    return torch.gather(t, 1, idx.view(*idx.shape, *([1] * (t.dim() - 2))).expand(-1, -1, *t.shape[2:])).contiguous()


@pytest.mark.parametrize("name", list(LOSSES))
@pytest.mark.parametrize("K,N", [(2, 1000), (3, 4099), (8, 8200)])
def test_relabelled_targets_against_plain_targets(name, K, N):
    """pit=True on tgt[:, q] equals pit=False on tgt; .permutation == inverse(q); tgt gets no gradient."""
    from tssep_amd.train import loss
    p, log = LOSSES[name]
    B = 3
    rng = np.random.RandomState(K * N)
    tgt = T_(rng.randn(B, K, N).astype(np.float32)).cuda()
    q = np.stack([rng.permutation(K) for _ in range(B)])
    noise = T_(rng.randn(B, K, N).astype(np.float32)).cuda()
    res = {}
    for pit in (False, True):
        lo = getattr(loss, name)(pit=pit)
        est = (tgt + 0.3 * noise).requires_grad_()
        t = (_take(tgt, q) if pit else tgt.clone()).requires_grad_()
        val = lo(est, t)
        assert tuple(val.shape) == (B,)
        w = T_(np.array([1.0, -2.0, 0.5], dtype=np.float32)).cuda()
        (val * w).sum().backward()
        assert t.grad is None
        res[pit] = (val.detach().cpu().numpy(), est.grad.cpu().numpy(), lo.permutation)
    ref = R.loss((tgt + 0.3 * noise).cpu().numpy(), _take(tgt, q).cpu().numpy(), p, log, pit=True)
    assert np.all(ref["gap"] > 1e-3)
    assert res[False][2] is None
    perm = res[True][2]
    assert perm.dtype == torch.int32 and not perm.requires_grad and tuple(perm.shape) == (B, K)
    assert np.array_equal(perm.cpu().numpy(), R.inverse(q)) and np.array_equal(ref["perm"], R.inverse(q))
    tol = tolerance(ref["loss"], p, log, K, N)
    assert np.all(np.abs(res[True][0] - res[False][0]) <= tol), (res[True][0], res[False][0], tol)
    assert np.all(np.abs(res[True][0] - ref["loss"]) <= tol)
    # the same pairs are matched, so the gradients are the same up to the coefficient's sums
    scale = np.abs(res[False][1]).max()
    assert np.abs(res[True][1] - res[False][1]).max() <= 1e-5 * scale
    # one utterance, [K, N]: squeezed back
    lo = getattr(loss, name)(pit=True)
    one = lo(tgt[1] + 0.3 * noise[1], _take(tgt, q)[1])
    assert one.dim() == 0 and tuple(lo.permutation.shape) == (K,)
    assert float(one) == float(res[True][0][1]) and np.array_equal(lo.permutation.cpu().numpy(), R.inverse(q)[1])


def test_functional_forms():
    from tssep_amd import functional as Fn
    torch.manual_seed(0)                                         # the doctests of tssep/train/loss.py:183-216
    target = torch.rand(2, 10000)
    estimate = target + 0.5 * torch.rand(2, 10000)
    e, t = estimate[None].cuda(), target[None].cuda()
    assert float(Fn.mse(e, t)) == pytest.approx(0.1673, abs=5e-5)
    assert float(Fn.mse(e, t, pit=True)) == float(Fn.mse(e, t))
    assert float(Fn.mae(e, t, pit=True)) == pytest.approx(0.5018, abs=5e-5)
    assert float(Fn.log_mae(e, t.flip(1), pit=True)) == pytest.approx(np.log10(0.5018), abs=5e-5)
    loss, perm = Fn.pair_loss(e, t.flip(1), p=2, pit=True)
    assert perm.tolist() == [[1, 0]] and float(loss) == float(Fn.mse(e, t))


# ------------------------------------------------------------------------------------------------ the toy Model
def _model(loss_module):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, model, net
    torch.manual_seed(2)
    m = model.Model(
        fe=fe.ConcaternatedSTFTFeatures(
            fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=16, projs=24, combination="mul",
                                            aux_net_output_size=513, ts_vad=3, output_resolution="tf",
                                            random_speaker_order=False),
        enhancer=enhancer.Masking(), loss=loss_module).cuda()
    m.train()
    return m


TARGET = "speaker_reverberation_early_ch0"


@pytest.fixture(scope="module")
def toy():
    """The model, a batch whose targets sit next to the model's own estimates (so that the matching is decided by a
    wide gap, asserted), and two relabellings of them."""
    from tssep_amd.train import loss
    B, K, N = 2, 3, 3000
    m = _model(loss.LogMAE())
    rng = np.random.RandomState(9)
    src = 0.1 * rng.randn(B, K, N).astype(np.float32)
    ex = dict(observation=T_(src.sum(1, keepdims=True) + 0.01 * rng.rand(B, 1, N).astype(np.float32)).cuda(),
              auxInput=T_(rng.rand(B, K, 513).astype(np.float32)).cuda(), reference_channel=0, dataset=["p"] * B)
    with torch.no_grad():
        probe = dict(ex, **{TARGET: T_(src).cuda()})
        out = m(probe)
        m.review(probe, out)
        est = out.time_estimate.detach().clone()
    tgt = est + 0.2 * est.std() * T_(rng.randn(B, K, N).astype(np.float32)).cuda()
    ref = R.loss(est.cpu().numpy(), tgt.cpu().numpy(), 1, True, pit=True)
    assert np.array_equal(ref["perm"], np.tile(np.arange(K), (B, 1))) and np.all(ref["gap"] > 1e-3), ref["gap"]
    qa, qb = np.array([[1, 2, 0], [2, 1, 0]]), np.array([[0, 2, 1], [1, 0, 2]])
    return m, ex, tgt, (qa, qb)


def _step(m, ex):
    m.zero_grad()
    out = m(dict(ex))
    ex = dict(ex)
    value = m.review(ex, out)["loss"]
    value.backward()
    torch.cuda.synchronize()
    return float(value), out, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}


def test_model_review_with_pit_against_the_fused_plain_tail(toy):
    from tssep_amd.train import loss
    m, ex, tgt, (qa, _) = toy
    B, K, N = tgt.shape
    m.loss = loss.LogMAE()
    plain, out, gplain = _step(m, dict(ex, **{TARGET: tgt}))
    assert getattr(out.time_estimate, "_tssep_loss_link", None) is not None      # the fused tail formed the loss
    m.loss = loss.LogMAE(pit=True)
    pit, out, gpit = _step(m, dict(ex, **{TARGET: _take(tgt, qa)}))
    assert getattr(out.time_estimate, "_tssep_loss_link", None) is None          # ... and here it did not
    assert np.array_equal(m.loss.permutation.cpu().numpy(), R.inverse(qa))
    # (the summed loss of B utterances: B tolerances)
    assert abs(pit - plain) <= B * float(tolerance(plain / B, 1, True, K, N)), (pit, plain)
    assert set(gpit) == set(gplain) and len(gpit) > 10
    for k in gplain:
        assert float((gpit[k] - gplain[k]).abs().max()) <= 1e-3 * float(gplain[k].abs().max()), k
    # MSE (never fused) runs through review too
    m.loss = loss.MSE(pit=True)
    mse, _, gm = _step(m, dict(ex, **{TARGET: _take(tgt, qa)}))
    assert np.isfinite(mse) and np.array_equal(m.loss.permutation.cpu().numpy(), R.inverse(qa))
    assert all(bool(torch.isfinite(g).all()) for g in gm.values())
    m.loss = loss.LogMAE()


def test_loss_graph_replay_recomputes_the_permutation(toy):
    """forward + loss + backward of LogMAE(pit=True) captured with torch.cuda.graph: every replay equals its eager run bit
    for bit, and the permutation follows the contents of the static target buffer."""
    from tssep_amd.train import loss
    _, _, tgt, (qa, qb) = toy
    B, K, N = tgt.shape
    base = (tgt + 0.01 * torch.randn_like(tgt)).detach()
    lo = loss.LogMAE(pit=True)

    def eager(t):
        est = base.clone().requires_grad_()
        v = lo(est, t)
        v.sum().backward()
        torch.cuda.synchronize()
        return v.detach().clone(), lo.permutation.clone(), est.grad.clone()

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
    s_perm = lo.permutation
    for q, (v, perm, grad) in zip((qa, qb, qa), want + want[:1]):
        s_tgt.copy_(_take(tgt, q))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s_val.detach(), v) and torch.equal(s_est.grad, grad)
        assert torch.equal(s_perm, perm) and np.array_equal(s_perm.cpu().numpy(), R.inverse(q))
    assert not np.array_equal(R.inverse(qa), R.inverse(qb))


def test_graphed_step_with_pit(toy):
    """The whole training step through GraphedStep (forward + review + backward as one hipGraph): capturable without a
    host sync, and each replay reports the permutation of ITS targets and the eager step's loss."""
    from tssep_amd.train import loss
    from tssep_amd.train.graph import GraphedStep
    from tssep_amd.train.optimizer import Adam
    m, ex, tgt, (qa, qb) = toy
    m.loss = loss.LogMAE(pit=True)
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
        want.append((float(value), m.loss.permutation.clone(), opt.bucket.flat.clone()))
    g = GraphedStep(m, opt)
    assert g.usable(exs[0])
    g(dict(exs[0]))                                                # warm-up, capture, first replay
    for i in (1, 0, 1):
        _, summary = g(dict(exs[i]))
        torch.cuda.synchronize()
        assert float(summary["loss"]) == pytest.approx(want[i][0], rel=1e-6)
        assert torch.equal(m.loss.permutation, want[i][1])
        assert float((opt.bucket.flat - want[i][2]).abs().max()) <= 1e-5 * float(want[i][2].abs().max())
    assert g.replays == 4 and g.eager_steps == 0 and len(g._graphs) == 1
    assert not torch.equal(want[0][1], want[1][1])
    m.loss = loss.LogMAE()
