"""MaskEstimator_v2 conditioned on frame-wise speaker embeddings (aux [B, K, Ta, E], `aux_stride`; the reference's
aux_time = "time" branch, tssep/train/net.py:862-894) on a real MI355X, in both GEMM arithmetics:

  1. a time-constant 4-D aux against the same module and seed with the 3-D aux: logit, mask and every parameter gradient
     bit for bit (the frame-wise kernels keep their neighbours' row decomposition, summation order and access widths)
  2. a time-varying aux at aux_stride 1 and 4 against the float64 restatement (tests/framewise_reference.py): masks,
     parameter gradients and d(aux), with the measure and bars of tests/test_rnnp_layer_reference.py taken against the
     fp32 restatement of the same case
  3. aux_normalizer = InstanceNorm(dim = -1 / -2) on the 4-D tensor (dim -2 is the time axis), Output.embedding's shape, an
     un-batched xs with [K, Ta, E]
  4. a Model step with a 4-D auxInput through GraphedStep: three replays, losses and flat gradients bit for bit the
     eager steps'
  5. what is refused, before anything is launched: aux_net on a 4-D aux, Ta != ceil(T / aux_stride); and a 3-D aux makes
     none of the new calls

Case 2 prints every tensor's figures and its ratio to the fp32 restatement's own error (pytest -rP); the bar is MARGIN = 8,
times SPLIT_RATIO for the split-bf16 GEMMs.  Its docstring says why it runs at units 64 / projs 48.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import framewise_reference as R  # noqa: E402
import test_aux_kernel_reference as AR  # noqa: E402
from test_rnnp_layer_reference import MARGIN, SPLIT_RATIO, bounds, errors  # noqa: E402

T_ = torch.as_tensor
U = 2.0 ** -24
Bn, Kn, Tn, IDIM, ODIM = 2, 4, 9, 7, 6


@pytest.fixture(params=["f32", "bf16x3"])
def gemm_mode(request):
    from tssep_amd import hip_ops
    old = hip_ops.GEMM_PRECISION
    hip_ops.GEMM_PRECISION = request.param
    yield request.param
    hip_ops.GEMM_PRECISION = old


def _estimator(combination, nap, seed=12, units=5, projs=6, idim=IDIM, odim=ODIM, **kw):
    from tssep_amd.train import net
    torch.manual_seed(seed)
    E = odim if combination == "mul" else 5
    me = net.MaskEstimator_v2(idim=idim, odim=odim, layers=3, units=units, projs=projs, combination=combination,
                              aux_net_output_size=E, ts_vad=Kn if nap > 1 else False, num_averaged_permutations=nap, **kw).cuda()
    return me, E


def _run(me, xs, aux, gm, seed=21):
    """forward + backward of sum(mask gm) -> (Output, {name: grad}, d(aux) or None)"""
    me.zero_grad(set_to_none=True)
    np.random.seed(seed)
    out = me(xs, aux)
    (out.mask * gm).sum().backward()
    torch.cuda.synchronize()
    return out, {k: q.grad.clone() for k, q in me.named_parameters()}, (aux.grad.clone() if aux.requires_grad else None)


# -------------------------------------------------------------------------------------------------------------- case 1
@pytest.mark.parametrize("nap", [1, 2])
@pytest.mark.parametrize("combination", ["mul", "cat"])
def test_time_constant_aux_gives_the_bits_of_the_utterance_level_aux(combination, nap, gemm_mode):
    me, E = _estimator(combination, nap, random_speaker_order=True)
    assert me.aux_stride == 1 and me.random_speaker_order
    rng = np.random.RandomState(1)
    xs = T_(rng.randn(Bn, Tn, IDIM).astype(np.float32)).cuda()
    a3 = T_((rng.randn(Bn, Kn, E) + 0.5).astype(np.float32)).cuda()
    gm = T_(rng.randn(Bn, Kn, 1, Tn, ODIM).astype(np.float32)).cuda()
    a4 = a3[:, :, None].expand(Bn, Kn, Tn, E).contiguous()
    o3, g3, _ = _run(me, xs, a3, gm)
    o4, g4, _ = _run(me, xs, a4, gm)
    assert o3.embedding.shape == (Bn, Kn, 1, E) and o4.embedding.shape == (Bn, Kn, Tn, E)
    assert torch.equal(o4.logit, o3.logit) and torch.equal(o4.mask, o3.mask)
    assert set(g3) == set(g4) and all(v.abs().max() > 0 for v in g3.values())
    for k in g3:
        assert torch.equal(g4[k], g3[k]), (k, float((g4[k] - g3[k]).abs().max()))
    # the shuffle moved whole [Ta, E] blocks: the embedding that entered the conditioning is the shuffled one
    assert torch.equal(o4.embedding[:, :, 0], o3.embedding[:, :, 0])


# -------------------------------------------------------------------------------------------------------------- case 2
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("nap", [1, 2])
@pytest.mark.parametrize("combination", ["mul", "cat"])
def test_time_varying_aux_against_the_restatement(combination, nap, stride, gemm_mode):
    """B = 2, K = 4, T = 9 (stride 4: buckets of 4, 4 and 1 frames) at units 64, projs 48, idim 40, odim 32, not at the toy
    width of case 1.  The measure divides a tensor's error by the fp32 restatement's own error for that tensor.  At the toy
    width a tensor's largest error is one or two roundings and moves with the seed
    (tests/test_rnnp_layer_reference.py), and this case takes the maximum over 41 tensors of a model four layers deep:
    tools/survey_framewise_ratio.py (profiles/framewise_ratio_survey.jsonl: 8 seeds x {mul, cat} x {1, 2} trials, fp32) found
    the worst ratio of a run above MARGIN = 8 in 8 of 64 frame-wise runs (strides 1 and 4; up to 15.1) and in 1 of 32 runs
    with a 3-D aux on the launches of the parent commit (13.3) at units 5 / projs 6, in 1 of 64 (8.15) and 0 of 32 at
    units 24 / projs 20, every time in a weight or bias gradient of an RNNP layer -- tensors that see the frame-wise
    kernels only through the forward product, which is exact, and d(pre), which is inside its bound; the mask's ratio
    stayed below 1.4 and d(aux)'s below 3.6 in every frame-wise run.  At this width every tensor's error is a sum of
    many roundings, and the same survey gave at most 6.2 over all 96 runs (frame-wise 6.0)."""
    IDIM, ODIM = 40, 32
    me, E = _estimator(combination, nap, units=64, projs=48, idim=IDIM, odim=ODIM, random_speaker_order=True,
                       aux_stride=stride)
    Ta = R.frames_of(Tn, stride)
    rng = np.random.RandomState(2 + stride)
    xs = rng.randn(Bn, Tn, IDIM).astype(np.float32)
    aux = (rng.randn(Bn, Kn, Ta, E) + 0.5).astype(np.float32)
    gm = rng.randn(Bn, Kn, 1, Tn, ODIM).astype(np.float32)
    aux_d = T_(aux).cuda().requires_grad_()
    out, grads, d_aux = _run(me, T_(xs).cuda(), aux_d, T_(gm).cuda(), seed=31)
    assert out.embedding.shape == (Bn, Kn, Ta, E) and d_aux.shape == aux.shape
    np.random.seed(31)
    perm = type(me).draw_permutations(Bn, Kn)[0]
    kw = dict(odim=ODIM, aux_stride=stride, combination=combination, ts_vad=Kn if nap > 1 else False,
              num_averaged_permutations=nap, perm=perm)
    ref = {}
    for dtype in (torch.float64, torch.float32):
        p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in me.state_dict().items()}
        a = T_(aux).to(dtype).requires_grad_()
        o = R.mask_estimator_forward(p, T_(xs).to(dtype), a, **kw)
        (o["mask"] * T_(gm).to(dtype)).sum().backward()
        ref[dtype] = {"mask": o["mask"].detach(), "d aux": a.grad, **{"d " + k: p[k].grad for k, _ in me.named_parameters()}}
    got = {"mask": out.mask.detach().cpu(), "d aux": d_aux.cpu(), **{"d " + k: v.cpu() for k, v in grads.items()}}
    split = gemm_mode == "bf16x3"
    bad = []
    for k, r64 in ref[torch.float64].items():
        e, b, own = errors(got[k], r64), bounds(ref[torch.float32][k], r64, split), errors(ref[torch.float32][k], r64)
        ratio = max(e[0] / max(own[0], U), e[1] / max(own[1], U))
        print(f"{combination} nap={nap} stride={stride} {gemm_mode} {k:42s} norm {e[0]:.3g} (<= {b[0]:.3g}) elem {e[1]:.3g} "
              f"(<= {b[1]:.3g}) ratio to the fp32 restatement {ratio:.3g}")
        if not (e[0] <= b[0] and e[1] <= b[1]):
            bad.append(k)
    assert MARGIN == 8.0 and SPLIT_RATIO > 700 and not bad, bad


# -------------------------------------------------------------------------------------------------------------- case 3
@pytest.mark.parametrize("dim", [-1, -2])
def test_aux_normalizer_on_the_4d_aux_and_unbatched_input(dim, gemm_mode):
    from tssep_amd.train import net
    stride = 2
    Ta = R.frames_of(Tn, stride)
    me, E = _estimator("mul", 1, random_speaker_order=False, aux_stride=stride, aux_normalizer=net.InstanceNorm(dim=dim))
    rng = np.random.RandomState(5)
    xs = T_(rng.randn(Bn, Tn, IDIM).astype(np.float32)).cuda()
    aux = T_((rng.randn(Bn, Kn, Ta, E) * 2 + 1.0).astype(np.float32)).cuda()
    with torch.no_grad():
        out = me(xs, aux)
    assert out.embedding.shape == aux.shape and out.mask.shape == (Bn, Kn, 1, Tn, ODIM)
    # on 4-D input dim -2 is the time axis (one statistic per (b, k, column)), dim -1 one per (b, k, frame)
    y64, tol = AR.ref_instnorm(aux, torch.zeros_like(aux), dim, 0, False)["y"]
    r, nonfinite = AR.within_class(out.embedding, y64, tol, f"InstanceNorm(dim={dim}) on [B, K, Ta, E]")
    print(f"InstanceNorm(dim={dim}) on the 4-D aux: worst err/bound {r:.3g}")
    assert nonfinite == 0
    want = {dt: R.mask_estimator_forward({k: v.detach().cpu().to(dt) for k, v in me.state_dict().items()}, xs.cpu().to(dt),
                                         y64.cpu().to(dt), odim=ODIM, aux_stride=stride, combination="mul")["mask"]
            for dt in (torch.float64, torch.float32)}
    e, b = errors(out.mask.cpu(), want[torch.float64]), bounds(want[torch.float32], want[torch.float64], gemm_mode == "bf16x3")
    print(f"mask behind InstanceNorm(dim={dim}): norm {e[0]:.3g} (<= {b[0]:.3g}) elem {e[1]:.3g} (<= {b[1]:.3g})")
    assert e[0] <= b[0] and e[1] <= b[1], (e, b)
    # un-batched: xs [T, idim] with aux [K, Ta, E] is entry 0 of the batch of one
    with torch.no_grad():
        one, batch = me(xs[1], aux[1]), me(xs[1:2], aux[1:2])
    assert one.embedding.shape == (Kn, Ta, E) and one.mask.shape == (Kn, 1, Tn, ODIM)
    assert torch.equal(one.mask, batch.mask[0]) and torch.equal(one.embedding, batch.embedding[0])
    assert torch.equal(batch.mask[0], out.mask[1])


# -------------------------------------------------------------------------------------------------------------- case 4
def test_captured_step_with_a_4d_auxinput_replays_the_eager_step(gemm_mode):
    from tssep_amd import hip_ops
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net
    from tssep_amd.train.graph import GraphedStep
    from tssep_amd.train.optimizer import Adam
    stride, B, K, N = 4, 2, 4, 5000
    torch.manual_seed(4)
    m = model.Model(
        fe=fe.ConcaternatedSTFTFeatures(
            fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=12, projs=16, combination="mul", aux_net_output_size=513,
                                            ts_vad=K, output_resolution="tf", random_speaker_order=True, aux_stride=stride),
        enhancer=enhancer.Masking(), loss=loss.LogMAE()).cuda()
    m.train()
    opt = Adam(gradient_clipping=10.0)
    opt.set_parameters(m.parameters())
    exs = []
    for i in range(3):
        rng = np.random.RandomState(50 + i)
        tgt = 0.1 * rng.randn(B, K, N).astype(np.float32)
        obs = T_(tgt.sum(1, keepdims=True) + 0.01 * rng.rand(B, 1, N).astype(np.float32)).cuda()
        frames = hip_ops.stft_frames(N)
        Ta = R.frames_of(frames, stride)
        assert Ta > 1 and Ta != K and frames % stride            # a partial last bucket; (B, K) are not the trailing axes
        exs.append(dict(observation=obs, auxInput=T_(rng.rand(B, K, Ta, 513).astype(np.float32)).cuda(),
                        speaker_reverberation_early_ch0=T_(tgt).cuda(), reference_channel=0, dataset=["f"] * B))
    want = []
    for i, e in enumerate(exs):
        np.random.seed(60 + i)
        opt.zero_grad()
        e = dict(e)
        out = m(e)
        assert out.embedding.shape == e["auxInput"].shape
        value = m.review(e, out)["loss"]
        value.backward()
        opt.bucket.sync()
        torch.cuda.synchronize()
        want.append((value.detach().clone(), opt.bucket.flat.clone()))
    assert not torch.equal(want[0][1], want[1][1]) and bool(torch.isfinite(want[0][1]).all())
    g = GraphedStep(m, opt)
    assert g.usable(exs[0])
    for i in (0, 1, 2):
        np.random.seed(60 + i)
        _, summary = g(dict(exs[i]))
        torch.cuda.synchronize()
        assert torch.equal(summary["loss"].detach(), want[i][0]), (i, float(summary["loss"]), float(want[i][0]))
        assert torch.equal(opt.bucket.flat, want[i][1]), (i, float((opt.bucket.flat - want[i][1]).abs().max()))
    assert g.replays == 3 and g.eager_steps == 0 and len(g._graphs) == 1


# -------------------------------------------------------------------------------------------------------------- case 5
def test_refusals_come_before_any_launch(monkeypatch):
    from tssep_amd import functional as Fn
    from tssep_amd.train import net

    def refuse(*a, **k):
        raise AssertionError("a launch on a refused input")
    me, E = _estimator("mul", 1, aux_stride=2)
    lin, _ = _estimator("mul", 1, aux_net=net.Linear(3, ODIM))
    monkeypatch.setattr(Fn, "condition", refuse)
    monkeypatch.setattr(Fn, "affine", refuse)
    monkeypatch.setattr(Fn, "instance_norm", refuse)
    for mod in (me, lin):
        monkeypatch.setattr(mod.pre_net, "forward_rows", refuse)
        monkeypatch.setattr(mod, "_speaker_permutations", refuse)
    xs = torch.randn(Bn, Tn, IDIM, device="cuda")
    with pytest.raises(NotImplementedError, match="aux_net=Linear on frame-wise embeddings"):
        lin(xs, torch.randn(Bn, Kn, Tn, 3, device="cuda"))
    for Ta in (R.frames_of(Tn, 2) - 1, R.frames_of(Tn, 2) + 1, Tn):
        with pytest.raises(ValueError, match="aux_stride=2"):
            me(xs, torch.randn(Bn, Kn, Ta, E, device="cuda"))
    with pytest.raises(ValueError):
        me(xs, torch.randn(Bn + 1, Kn, R.frames_of(Tn, 2), E, device="cuda"))
    with pytest.raises(ValueError):
        me(xs, torch.randn(Bn, Kn, 1, R.frames_of(Tn, 2), E, device="cuda"))
    for bad in (0, -1, 2.0, True):
        with pytest.raises(ValueError, match="aux_stride"):
            net.MaskEstimator_v2(idim=IDIM, odim=ODIM, units=5, projs=6, combination="mul", aux_stride=bad)
    # aux_stride is the frame rate of a frame-wise aux: an utterance-level aux beside aux_stride != 1 is refused, not ignored
    with pytest.raises(ValueError, match="aux_stride=2 with one embedding per speaker and utterance"):
        me(xs, torch.randn(Bn, Kn, E, device="cuda"))
    cfg = net.MaskEstimator_v2.get_config({"aux_stride": 3, "combination": "mul"})
    assert cfg["aux_stride"] == 3 and net.MaskEstimator_v2.get_config()["aux_stride"] == 1


def test_a_3d_aux_makes_none_of_the_new_calls(monkeypatch):
    from tssep_amd import _lib

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called for an utterance-level embedding")
        return f
    for name in ("tssep_cond_mul_t_fwd", "tssep_cond_mul_t_bwd", "tssep_cond_cat_t_fwd", "tssep_cond_aux_t_bwd_workspace_bytes",
                 "tssep_cond_mul_aux_t_bwd", "tssep_cond_cat_aux_t_bwd"):
        assert callable(getattr(_lib.lib(), name))
        monkeypatch.setattr(_lib.lib(), name, refuse(name))
    for comb in ("mul", "cat"):
        me, E = _estimator(comb, 2, aux_normalizer=None)
        aux = torch.randn(Bn, Kn, E, device="cuda", requires_grad=True)
        out = me(torch.randn(Bn, Tn, IDIM, device="cuda"), aux)
        out.mask.sum().backward()
        assert aux.grad is not None and out.embedding.shape == (Bn, Kn, 1, E)
    with pytest.raises(AssertionError, match="tssep_cond_mul_t_fwd called"):
        me4, E = _estimator("mul", 1)
        me4(torch.randn(Bn, Tn, IDIM, device="cuda"), torch.randn(Bn, Kn, Tn, E, device="cuda"))


def test_graphed_step_leaves_unbatched_framewise_input_to_the_eager_path():
    """[K, Ta, E] beside an un-batched observation has the rank of [B, K, E]: GraphedStep does not guess, it is not usable."""
    from tssep_amd.train.graph import GraphedStep
    g = GraphedStep.__new__(GraphedStep)
    g.eager_reason, g.model = None, object()
    obs, aux = torch.zeros(1, 5000, device="cuda"), torch.zeros(4, 6, 513, device="cuda")
    assert GraphedStep._unbatched_framewise(dict(observation=obs, auxInput=aux))
    assert not g.usable(dict(observation=obs, auxInput=aux))
    assert g.usable(dict(observation=obs[None], auxInput=aux)) and g.usable(dict(observation=obs, auxInput=aux[0]))
    assert g.usable(dict(observation=obs[None], auxInput=aux[None]))
    with pytest.raises(RuntimeError, match="un-batched frame-wise auxInput"):
        g._capture(dict(observation=obs, auxInput=aux))


def test_a_recycled_stream_handle_forgets_its_side_stream():
    """hip_ops pairs one side stream with every compute stream, keyed by the stream's handle; torch recycles handles.
    forget_side_stream (GraphedStep calls it on its fresh capture stream) drops the pairing, for that stream only."""
    from tssep_amd import hip_ops as H
    s, other = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        side = H.side_stream(s.device)
    with torch.cuda.stream(other):
        side_other = H.side_stream(other.device)
    key = (str(s.device), s.cuda_stream)
    assert H._SIDE[key] is side and side is not side_other
    H.forget_side_stream(s)
    assert key not in H._SIDE and H._SIDE[(str(other.device), other.cuda_stream)] is side_other
    H.forget_side_stream(s)                                  # nothing to forget: no error
    with torch.cuda.stream(s):
        H.join_side_stream()                                 # nothing to join
        assert H.side_stream(s.device) is not None and key in H._SIDE
    H.forget_side_stream(s)
    H.forget_side_stream(other)
