"""dropout > 0 on a real MI355X: the masked Tanh kernels (csrc/dropout.hip) against the host-side mask function and
float64, the inactive path (eval, p = 0) against today's, the module path against the materialised chain
(layer -> mask from the host -> torch.tanh, autograd), the train / eval switch, hipGraph replay and the toy experiment."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_kernels import close  # noqa: E402

T_ = torch.as_tensor
GRID_SWEEP = 4096 * 256            # dropout.hip grid_for (the same cap as elementwise.hip): items per sweep of the grid
EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")


def H():
    from tssep_amd import hip_ops
    return hip_ops


@pytest.fixture(params=["f32", "bf16x3"])
def gemm_mode(request):
    old = H().GEMM_PRECISION
    H().GEMM_PRECISION = request.param
    yield request.param
    H().GEMM_PRECISION = old


def host_keep(used, n, p):
    seed, draw = used.tolist()
    return torch.from_numpy(H().dropout_keep_host(seed, draw, 0, n, p).astype(np.bool_))


def logical(y, rows, P, K, T, combined):
    """[rows, P] in logical order (rows (b,k,t)) of a plain (possibly padded) or speaker-combined buffer."""
    if combined:
        B = rows // (K * T)
        return y.view(B, T, K, P).permute(0, 2, 1, 3).reshape(rows, P)
    return y[:, :P]


def physical(v, rows, P, ld, K, T, combined):
    """The buffer a [rows, P] logical tensor lives in: [B T, K P] (combined) or [rows, ld] with zero pad columns."""
    if combined:
        B = rows // (K * T)
        return v.view(B, K, T, P).permute(0, 2, 1, 3).reshape(B * T, K * P).contiguous()
    buf = torch.zeros(rows, ld, device=v.device, dtype=v.dtype)
    buf[:, :P] = v
    return buf


# (rows = B K T, P, ld, K, T, combined): 16-byte path dense / padded, scalar path (P = 6), the combined layout with K = 4 on
# both paths, and two sizes of 2.55 sweeps of the capped grid in float4 items (the tanh_bwd size of test_gpu_streaming_kernels)
LAYOUTS = [
    (5 * 37, 320, 320, 1, 37, False), (50, 8, 12, 1, 50, False), (77, 6, 8, 1, 77, False), (3 * 4 * 7, 8, 0, 4, 7, True),
    (3 * 4 * 7, 6, 0, 4, 7, True), (33 * 4 * 253, 320, 320, 4, 253, False), (33 * 4 * 253, 320, 0, 4, 253, True),
]


def test_sizes_wrap_the_capped_grid():
    assert 33 * 4 * 253 * 320 >= 2.5 * 4 * GRID_SWEEP
    assert sum(1 for r, P, *_ in LAYOUTS if r * P >= 2.5 * 4 * GRID_SWEEP) == 2


@pytest.mark.parametrize("rows,P,ld,K,T,combined", LAYOUTS)
def test_device_mask_is_the_host_mask(rows, P, ld, K, T, combined):
    """z = 1 everywhere, so y != 0 <=> keep: the device's mask against tssep_dropout_keep_host, bit for bit."""
    h, p = H(), 0.3
    h.manual_seed(1234)
    z = physical(torch.ones(rows, P, device="cuda"), rows, P, ld, K, T, combined)
    if not combined and ld != P:
        z[:, P:] = 7.0                                     # pad columns: not the kernel's to touch
    used0 = h.dropout_draw()
    used = h.dropout_draw()
    assert used0.tolist() == [1234, 0] and used.tolist() == [1234, 1] and h.get_state() == (1234, 2)
    y = torch.full_like(z, -1.0)
    h.dropout_tanh_fwd(z, y, rows, P, ld, K, T, combined, p, used)
    keep = host_keep(used, rows * P, p).view(rows, P)
    got = logical(y, rows, P, K, T, combined).cpu()
    assert torch.equal(got != 0, keep)
    want = torch.tanh(torch.tensor(1.0 / (1 - p), dtype=torch.float64))
    assert float((got.double()[keep] - want).abs().max()) <= 5e-7 and bool((got[~keep] == 0).all())
    if not combined and ld != P:
        assert bool((y[:, P:] == -1.0).all())
    h.dropout_tanh_fwd(z, z, rows, P, ld, K, T, combined, p, used)       # in place: the same result
    assert torch.equal(logical(z, rows, P, K, T, combined), logical(y, rows, P, K, T, combined))
    if not combined and ld != P:
        assert bool((z[:, P:] == 7.0).all())
    # p = 0 keeps everything, p = 1 nothing; another draw is another mask
    for pp, expect in ((0.0, True), (1.0, False)):
        h.dropout_tanh_fwd(torch.ones_like(y), y, rows, P, ld, K, T, combined, pp, used)
        assert bool(((logical(y, rows, P, K, T, combined) != 0) == expect).all())
    h.dropout_tanh_fwd(torch.ones_like(y), y, rows, P, ld, K, T, combined, p, used0)
    assert not torch.equal(logical(y, rows, P, K, T, combined).cpu() != 0, keep)


def test_status_codes():
    h = H()
    used = h.dropout_draw()
    z = torch.ones(8, 8, device="cuda")
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="invalid shape"):
            h.dropout_tanh_fwd(z, z, 8, 8, 8, 1, 8, False, bad, used)
        with pytest.raises(RuntimeError, match="invalid shape"):
            h.dropout_tanh_bwd(z, z, 8, 8, 1, 8, False, bad, used)
    with pytest.raises(RuntimeError, match="invalid shape"):
        h.dropout_tanh_fwd(z, z, 8, 8, 4, 1, 8, False, 0.3, used)        # ld < P
    with pytest.raises(RuntimeError, match="invalid shape"):
        h.dropout_tanh_fwd(z, z, 8, 8, 8, 3, 2, True, 0.3, used)         # rows not B K T


VALUE_LAYOUTS = [l for l in LAYOUTS if l[0] * l[1] < 2.5 * 4 * GRID_SWEEP] + [LAYOUTS[-1]]


@pytest.mark.parametrize("p", [0.3, 0.5])
@pytest.mark.parametrize("rows,P,ld,K,T,combined", VALUE_LAYOUTS)
def test_forward_and_backward_values_against_float64(rows, P, ld, K, T, combined, p):
    """Forward: |y - where(keep, tanh(z / (1 - p)), 0)| <= 5e-7 (gemm_tanh's documented 3e-7 plus the fp32 rounding of
    z / (1 - p) through a slope <= 1), dropped elements exactly 0.  Backward: within 1e-6 of the tensor's largest entry of
    where(keep, dy (1 - y^2) / (1 - p), 0) in float64 (three fp32 products), dropped elements exactly 0.  Two forwards, then
    the two backwards: each finds its own forward's mask."""
    h = H()
    h.manual_seed(99)
    g = torch.Generator().manual_seed(rows + P)
    res = []
    for _ in range(2):
        z = torch.randn(rows, P, generator=g) * 2
        dy = torch.randn(rows, P, generator=g)
        zb = physical(z.cuda(), rows, P, ld, K, T, combined)
        used = h.dropout_draw()
        yb = h.dropout_tanh_fwd(zb, torch.empty_like(zb).fill_(-1.0), rows, P, ld, K, T, combined, p, used)
        res.append((z, dy, yb, used))
    masks = []
    for z, dy, yb, used in res:
        keep = host_keep(used, rows * P, p).view(rows, P)
        masks.append(keep)
        y = logical(yb, rows, P, K, T, combined).cpu()
        want = torch.where(keep, torch.tanh(z.double() / (1 - p)), torch.zeros((), dtype=torch.float64))
        err = float((y.double() - want).abs().max())
        print(f"forward rows={rows} P={P} combined={combined} p={p}: max abs err {err:.3e}")
        assert bool((y[~keep] == 0).all())
        assert err <= 5e-7
        # backward: dy and y dense rows (plain) or the combined buffers, as for tssep_tanh_bwd
        dyb = physical(dy.cuda(), rows, P, P, K, T, combined)
        yd = yb if combined else yb[:, :P].contiguous()
        dz = h.dropout_tanh_bwd(dyb, yd, rows, P, K, T, combined, p, used).cpu()
        want = torch.where(keep, dy.double() * (1 - y.double() ** 2) / (1 - p), torch.zeros((), dtype=torch.float64))
        err = float((dz.double() - want).abs().max())
        print(f"backward rows={rows} P={P} combined={combined} p={p}: max abs err {err:.3e}, largest entry "
              f"{float(want.abs().max()):.3e}")
        assert bool((dz[~keep] == 0).all())
        assert err <= 1e-6 * float(want.abs().max())
    assert not torch.equal(masks[0], masks[1])


# ------------------------------------------------------------------------------------------------- the inactive path
def _clone_weights(dst, src):
    dst.load_state_dict(src.state_dict())
    return dst.cuda()


def _run_logged(fn):
    h = H()
    h.GEMM_LOG = []
    try:
        out = fn()
    finally:
        log, h.GEMM_LOG = h.GEMM_LOG, None
    return out, log


def _grads(m):
    return {k: p.grad.clone() for k, p in m.named_parameters()}


def test_rnnp_packed_eval_and_p0_are_todays_path(gemm_mode):
    from tssep_amd.train.rnnp import RNNP_packed
    h = H()
    torch.manual_seed(3)
    ref = RNNP_packed(7, 3, 5, 8, 0).cuda().train()
    x = torch.randn(3, 11, 7).cuda()
    gy = torch.randn(3, 11, 8).cuda()

    def step(m):
        m.zero_grad()
        xx = x.clone().requires_grad_()
        y = m(xx)
        (y * gy).sum().backward()
        return y.detach().clone(), xx.grad.clone(), _grads(m)

    want, log0 = _run_logged(lambda: step(ref))
    before = h.get_state()
    for m in (_clone_weights(RNNP_packed(7, 3, 5, 8, 0.3), ref).eval(), _clone_weights(RNNP_packed(7, 3, 5, 8, 0.0), ref).train()):
        got, log = _run_logged(lambda: step(m))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert all(torch.equal(got[2][k], want[2][k]) for k in want[2])
        assert log == log0
    assert h.get_state() == before                         # nothing was drawn


@pytest.mark.parametrize("projs", [6, 8])
@pytest.mark.parametrize("ts_vad", [False, 4])
@pytest.mark.parametrize("combination", ["mul", "cat"])
def test_mask_estimator_eval_and_p0_are_todays_path(combination, ts_vad, projs, gemm_mode):
    """A dropout = 0.3 module in .eval() and a dropout = 0.0 module in .train() run the dropout = 0 module's launches --
    the same GEMM requests on the same kernels (act = 1 stores, the Tanh fold at projs = 8) -- and give its outputs and
    parameter gradients bit for bit."""
    from tssep_amd.train.net import MaskEstimator_v2
    h = H()
    kw = dict(idim=12, odim=9, layers=3, units=5, projs=projs, combination=combination, aux_net_output_size=7,
              ts_vad=ts_vad, random_speaker_order=True)
    torch.manual_seed(4)
    ref = MaskEstimator_v2(dropout=0, **kw).cuda().train()
    B, K, T = 2, 4, 13
    xs = torch.randn(B, T, 12).cuda()
    aux = torch.rand(B, K, 9 if combination == "mul" else 7).cuda()
    gm = None

    def step(m):
        nonlocal gm
        m.zero_grad()
        np.random.seed(8)
        out = m(xs, aux)
        if gm is None:
            gm = torch.randn(out.mask.shape, generator=torch.Generator().manual_seed(1)).cuda()
        (out.mask * gm).sum().backward()
        return out.mask.detach().clone(), out.logit.detach().clone(), _grads(m)

    want, log0 = _run_logged(lambda: step(ref))
    assert any(d["act"] == 1 for *_, d in log0) and any(d["act"] == 2 for *_, d in log0) == (projs == 8 and h.FOLD_TANH)
    before = h.get_state()
    for m in (_clone_weights(MaskEstimator_v2(dropout=0.3, **kw), ref).eval(),
              _clone_weights(MaskEstimator_v2(dropout=0.0, **kw), ref).train()):
        got, log = _run_logged(lambda: step(m))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert all(torch.equal(got[2][k], want[2][k]) for k in want[2])
        assert log == log0
    assert h.get_state() == before


# --------------------------------------------------------------------------- module path = materialised chain
class _record_draws:
    """Keeps the `used` tensor of every dropout_draw made inside the block, in order."""

    def __enter__(self):
        h = H()
        self.orig, self.used = h.dropout_draw, []

        def draw(device=None):
            u = self.orig(device)
            self.used.append(u)
            return u
        h.dropout_draw = draw
        return self.used

    def __exit__(self, *exc):
        H().dropout_draw = self.orig
        return False


def _masked_tanh(z, used, p):
    """torch.tanh(z keep / (1 - p)) with the host's mask for `used`; z: [rows, P] logical."""
    keep = host_keep(used, z.numel(), p).view(z.shape).to(z.device)
    return torch.tanh(z * keep / (1 - p))


def _compare(tag, got, want, a, log_only=()):
    """The bars of ::test_rnnp_packed_against_reference_fixture for the arithmetic (a = 1: f32, 10: bf16x3): the chain's
    Tanh is torch's, an implementation independent of the kernels', as the fixture's is."""
    y, dx, dp = got
    y_, dx_, dp_ = want
    print(f"{tag}: output max abs err {float((y - y_).abs().max()):.3e} (scale {float(y_.abs().max()):.3e})")
    close(y, y_, rtol=1e-4 * a, atol=2e-6 * a, name=tag + " output")
    if dx is not None:
        close(dx, dx_, rtol=1e-3, atol=2e-6 * a, name=tag + " dx")
    worst = max(dp_, key=lambda k: float((dp[k] - dp_[k]).abs().max()) / float(dp_[k].abs().max()))
    print(f"{tag}: gradients, worst max abs err / scale: d{worst} {float((dp[worst] - dp_[worst]).abs().max()):.3e} / "
          f"{float(dp_[worst].abs().max()):.3e}")
    for k in dp_:
        close(dp[k], dp_[k], rtol=1e-3, atol=5e-6 * a, name=f"{tag} d{k}")


@pytest.mark.parametrize("cdim,hdim", [(5, 6), (5, 8), (300, 320)])
def test_rnnp_packed_training_equals_materialised_chain(cdim, hdim, gemm_mode):
    from tssep_amd import functional as Fn
    from tssep_amd.train.rnnp import RNNP_packed
    a, p = (1 if gemm_mode == "f32" else 10), 0.3
    torch.manual_seed(5)
    idim = 7 if cdim == 5 else 40
    m = RNNP_packed(idim, 3, cdim, hdim, p).cuda().train()
    N, T = 3, 11
    x = torch.randn(N, T, idim).cuda()
    gy = torch.randn(N, T, hdim).cuda()
    xx = x.clone().requires_grad_()
    with _record_draws() as used:
        y = m(xx)
    assert len(used) == 2                                  # the two inner sites; none behind the last layer
    (y * gy).sum().backward()
    got = (y.detach().clone(), xx.grad.clone(), _grads(m))
    m.zero_grad()
    xx = x.clone().requires_grad_()
    hcur = xx.reshape(N * T, idim)
    for i in range(3):
        z = Fn.rnnp_layer(hcur, m.net[4 * i], m.net[4 * i + 1], N, T, act=0)
        hcur = _masked_tanh(z, used[i], p) if i < 2 else z
    y2 = hcur.reshape(N, T, hdim)
    (y2 * gy).sum().backward()
    _compare(f"RNNP_packed {cdim}/{hdim} {gemm_mode}", got, (y2.detach(), xx.grad, _grads(m)), a)
    assert float((got[0] - m.eval()(x).detach()).abs().max()) > 1e-3      # and dropout did something


@pytest.mark.parametrize("units,projs", [(5, 6), (5, 8), (300, 320)])
def test_post_net_training_equals_materialised_chain(units, projs, gemm_mode):
    """MaskEstimator_v2(ts_vad = 4) in training mode: the site behind birnn0 works on rows (b,k,t), the one behind birnn1
    on the speaker-combined tensor [B, T, K P] -- with the mask of the LOGICAL rows (b,k,t) in both."""
    from tssep_amd import functional as Fn
    from tssep_amd.train.net import MaskEstimator_v2
    a, p = (1 if gemm_mode == "f32" else 10), 0.3
    torch.manual_seed(6)
    idim, odim = (12, 9) if units == 5 else (40, 16)
    me = MaskEstimator_v2(idim=idim, odim=odim, layers=3, units=units, projs=projs, dropout=p, combination="mul",
                          ts_vad=4, random_speaker_order=False).cuda().train()
    B, K, T = 2, 4, 11
    xs = torch.randn(B, T, idim).cuda()
    aux = torch.rand(B, K, odim).cuda()
    with _record_draws() as used:
        logit, _ = me.logits(xs, aux)
    assert len(used) == 2
    gl = torch.randn(logit.shape, generator=torch.Generator().manual_seed(2)).cuda()
    (logit * gl).sum().backward()
    got = (logit.detach().clone(), None, _grads(me))
    me.zero_grad()
    pre = me.pre_net.forward_rows(xs.reshape(B * T, idim), B, T)
    hcur = Fn.condition(pre, aux.contiguous(), B, K, T, 1, "mul")
    b0, b1, b2 = me._birnns
    hcur = _masked_tanh(b0.forward_rows(hcur, B * K, T), used[0], p)
    hcur = _masked_tanh(b1.forward_rows(hcur, B * K, T), used[1], p)
    hcur = hcur.view(B, K, T, projs).permute(0, 2, 1, 3).reshape(B * T, K * projs)       # net.py:608-611
    hcur = b2.forward_rows(hcur, B, T)
    logit2 = Fn.head(hcur, me._linear, None, None, B, K, T, odim, 1, odim, spk_rows=False)
    (logit2 * gl).sum().backward()
    _compare(f"post-net {units}/{projs} {gemm_mode}", got, (logit2.detach(), None, _grads(me)), a)


# ------------------------------------------------------------------------------------ train / eval, fresh masks
def _model(units=12, projs=12, dropout=0.1, seed=21, shuffle=False):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net
    torch.manual_seed(seed)
    return model.Model(
        fe=fe.ConcaternatedSTFTFeatures(
            fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=units, projs=projs, dropout=dropout, combination="mul",
                                            aux_net_output_size=513, ts_vad=4, output_resolution="tf",
                                            random_speaker_order=shuffle, num_averaged_permutations=1),
        enhancer=enhancer.Masking(), loss=loss.LogMAE())


def _batch(B, K, N, seed):
    rng = np.random.RandomState(seed)
    tgt = 0.1 * rng.randn(B, K, N).astype(np.float32)
    return dict(observation=T_(tgt.sum(1, keepdims=True) + 0.01 * rng.rand(B, 1, N).astype(np.float32)).cuda(),
                auxInput=T_(rng.rand(B, K, 513).astype(np.float32)).cuda(),
                speaker_reverberation_early_ch0=T_(tgt).cuda(), reference_channel=0, dataset=["d"] * B)


def test_train_eval_switch_fresh_masks_and_reseeding(tmp_path):
    from tssep_amd.train.optimizer import Adam
    from tssep_amd.train.trainer import Trainer
    h = H()
    m = _model(dropout=0.3).cuda().train()
    ex = _batch(2, 4, 6000, seed=1)
    sites = 2                                               # layers - 1 post-net sites; the pre-net has a single layer

    def step():
        m.zero_grad()
        e = dict(ex)
        out = m(e)
        loss = m.review(e, out)["loss"]
        loss.backward()
        return float(loss.detach()), out.time_estimate.detach().clone(), [q.grad.clone() for q in m.parameters() if q.grad is not None]

    h.manual_seed(42)
    a = step()
    assert h.get_state() == (42, sites)
    b = step()
    assert h.get_state() == (42, 2 * sites)
    assert not torch.equal(a[1], b[1]) and a[0] != b[0]    # fresh masks on the same input
    h.manual_seed(42)
    c = step()                                              # reseeded: the first step again, bit for bit
    assert c[0] == a[0] and torch.equal(c[1], a[1]) and all(torch.equal(x, y) for x, y in zip(c[2], a[2]))
    h.set_state((42, sites))
    d = step()
    assert d[0] == b[0] and torch.equal(d[1], b[1]) and all(torch.equal(x, y) for x, y in zip(d[2], b[2]))
    # one site switched off by itself: one draw per forward
    m.mask_estimator._dropouts[0].eval()
    before = h.get_state()
    step()
    assert h.get_state() == (before[0], before[1] + 1)
    m.train()
    # eval: no draws, equal outputs
    m.eval()
    before = h.get_state()

    def evaluate():
        e = dict(ex)
        with torch.no_grad():
            out = m(e)
            loss = float(m.review(e, out)["loss"])
        return loss, out.time_estimate.clone()

    e1, e2 = evaluate(), evaluate()
    assert e1[0] == e2[0] and torch.equal(e1[1], e2[1]) and h.get_state() == before
    tr = Trainer(m, tmp_path, Adam(lr=1e-3))
    tr.register_validation_hook([_batch(2, 4, 6000, seed=2), _batch(1, 4, 5000, seed=3)])
    v1, v2 = tr.validate(), tr.validate()
    assert v1 == v2 and np.isfinite(v1) and h.get_state() == before and m.training


# ---------------------------------------------------------------------------------------------------- graph replay
def test_trainer_graph_step_is_bit_identical_to_the_eager_trainer(tmp_path):
    """::test_trainer_graph_step_is_bit_identical_to_the_eager_trainer of test_gpu_modules with dropout = 0.1: the passes a
    capture needs draw masks too, and the dropout state is put back after them, so the run through graphs consumes the
    same draws as the eager run -- losses of every iteration and the final parameters are bit-identical."""
    from tssep_amd.train import runtime
    from tssep_amd.train.optimizer import Adam
    from tssep_amd.train.trainer import Trainer
    h = H()
    data = [_batch(2, 4, 5000 if i % 2 else 7300, seed=31 + i) for i in range(4)]

    class Dataset(list):
        def __iter__(self):
            return (dict(ex) for ex in list.__iter__(self))

    runs = {}
    for mode in ("off", "on"):
        with runtime.applied(graph_step=mode):
            np.random.seed(77)
            h.manual_seed(2024)
            tr = Trainer(_model(units=24, projs=24, dropout=0.1, shuffle=True), tmp_path / mode,
                         Adam(gradient_clipping=10.0, lr=1e-3), summary_trigger=(1, "iteration"),
                         checkpoint_trigger=(1000, "iteration"), stop_trigger=(8, "iteration"), virtual_minibatch_size=2)
            hist = tr.train(Dataset(data), device=0)
            torch.cuda.synchronize()
            hf = json.loads((tmp_path / mode / "log" / "history.json").read_text())
            runs[mode] = ([l for _, l in hist], tr.optimizer.flat_param.clone(), hf, h.get_state())
    l_off, p_off, _, s_off = runs["off"]
    l_on, p_on, h_on, s_on = runs["on"]
    assert len(l_off) == 8 and all(np.isfinite(l_off))
    assert s_off == (2024, 16) and s_on == s_off            # two sites x eight iterations, captures included
    assert h_on.get("graph_replays", 0) == 7 and h_on["graphs"] == 2, h_on
    assert l_on == l_off, [(i, a, b) for i, (a, b) in enumerate(zip(l_on, l_off)) if a != b]
    assert torch.equal(p_on, p_off), float((p_on - p_off).abs().max())


def test_graph_replays_draw_fresh_masks():
    from tssep_amd.train import runtime
    from tssep_amd.train.graph import GraphedStep
    from tssep_amd.train.optimizer import Adam
    h = H()
    m = _model(units=16, projs=16, dropout=0.3).cuda().train()
    opt = Adam(gradient_clipping=10.0)
    opt.set_parameters(m.parameters())
    ex = _batch(2, 4, 5000, seed=5)
    with runtime.applied(side_stream=False):
        g = GraphedStep(m, opt)
        h.manual_seed(7)
        g(dict(ex))                                         # warm-up, capture (state put back), first replay
        assert h.get_state() == (7, 2)
        l1 = float(g(dict(ex))[1]["loss"])
        l2 = float(g(dict(ex))[1]["loss"])
        assert h.get_state() == (7, 6) and l1 != l2         # identical inputs, fresh masks
        h.set_state((7, 2))
        l1_again = float(g(dict(ex))[1]["loss"])
        assert l1_again == l1
        # the eager step with the same state computes the replay's loss
        h.set_state((7, 2))
        opt.zero_grad()
        e = dict(ex)
        l1_eager = float(m.review(e, m(e))["loss"])
    assert l1_eager == pytest.approx(l1, rel=1e-6)
    assert g.replays == 4 and len(g._graphs) == 1
    m.eval()                                                # another signature: the sites are off
    with runtime.applied(side_stream=False):
        before = h.get_state()
        la = float(g(dict(ex))[1]["loss"])
        lb = float(g(dict(ex))[1]["loss"])
    assert la == lb and h.get_state() == before and len(g._graphs) == 2


# ------------------------------------------------------------------------------------------------- toy experiment
def test_toy_experiment_with_the_dropout_overlay(tmp_path):
    """run_tssep with toy_tssep_dropout.yaml: trains its iterations with finite losses, validates, checkpoints; the checkpoint
    carries the dropout state and a resumed run goes on drawing where the first one stopped."""
    import subprocess
    import sys
    import yaml
    from tssep_amd.exp import run_tssep
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tsvad.yaml")]
                           + [f"eg.trainer.storage_dir={tmp_path / 'v'}"])
    ck = tmp_path / "vad.pth"
    torch.save({"model": Experiment.from_config(cfg["eg"]).trainer.model.state_dict()}, ck)
    fast = ["eg.trainer.stop_trigger=[3,iteration]", "eg.trainer.checkpoint_trigger=[3,iteration]",
            "eg.trainer.summary_trigger=[1,iteration]"]
    sep_dir = run_tssep.main(configs=tuple(os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml",
                                                                          "toy_tssep_dropout.yaml")),
                             storage_dir=tmp_path / "tssep", checkpoint=ck, overrides=fast)
    frozen = yaml.safe_load((sep_dir / "config.yaml").read_text())
    assert frozen["eg"]["trainer"]["model"]["mask_estimator"]["dropout"] == 0.1
    layers = frozen["eg"]["trainer"]["model"]["mask_estimator"]["layers"]
    hist = json.loads((sep_dir / "log" / "history.json").read_text())
    assert hist["iteration"] == 3 and len(hist["loss"]) == 3 and all(np.isfinite(l) for _, l in hist["loss"])
    sd = torch.load(sep_dir / "checkpoints" / "ckpt_latest.pth", map_location="cpu")
    seed, draw = sd["dropout_state"]
    assert draw >= 3 * (layers - 1)                         # (+ the pre-flight test run's forward, if the experiment makes one)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-m", "tssep_amd.train.run", "with", "config.yaml",
                    "eg.trainer.stop_trigger=[4,iteration]", "eg.trainer.checkpoint_trigger=[4,iteration]"],
                   cwd=sep_dir, check=True, env=dict(os.environ, PYTHONPATH=root))
    sd4 = torch.load(sep_dir / "checkpoints" / "ckpt_latest.pth", map_location="cpu")
    assert sd4["iteration"] == 4
    assert tuple(sd4["dropout_state"]) == (seed, draw + (layers - 1))      # resumed: one more training step's draws
