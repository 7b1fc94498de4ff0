"""MaskEstimator_v2(rnn_typ='lstm') -- every recurrent layer in one direction of time -- on a real MI355X against
tests/estimator_reference.py::estimator_forward (imported, unchanged) run with a ONE-direction torch layer
(torch.nn.LSTM(bidirectional=False) + Linear): float64 is the reference, the same in float32 the yardstick.  The measure
is tests/test_estimator_reference.py's (`compare`): per tensor the normwise and the element-wise error against float64
within MARGIN x the float32 run's own, x SPLIT_RATIO under split-bf16 GEMMs.  Forward, every parameter gradient, d(xs) and
d(aux).  Then forward_chunk over chunks (23), (1 x 23), (5, 1, 17) against the SAME float64 outputs under the same bounds
(random_speaker_order on: one permutation for the whole utterance, read from the state; AuxNet enrolments: the embedding
computed once), the default model's bits, the trainer through hipGraph replay and the kernel plan it writes."""
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import estimator_reference as ER  # noqa: E402
import test_estimator_reference as TR  # noqa: E402
from test_causal_reference import CATTRS, causal_module_params, causal_modules, chunkings  # noqa: E402
from test_rnnp_layer_reference import MARGIN, SPLIT_RATIO  # noqa: E402

T_ = torch.as_tensor
B_, K_, T_FRAMES = 2, 4, 23
TOY = dict(idim=40, odim=32, units=64, projs=48, layers=3)
WIDE = dict(idim=96, odim=80, units=300, projs=320, layers=3)
E_CAT = 18
WORST = {}

# name -> (batch, widths, constructor keywords beyond the widths, AuxNet enrolments)
ROWS = {
    "mul-spk": (B_, TOY, dict(combination="mul", ts_vad=False), False),
    "cat-tsvad-2trials": (B_, TOY, dict(combination="cat", ts_vad=K_, num_averaged_permutations=2, aux_net_output_size=E_CAT), False),
    "explicit-vad": (B_, TOY, dict(combination="mul", ts_vad=K_, explicit_vad=True), False),
    "two-masks": (B_, TOY, dict(combination="mul", ts_vad=False, nmask=2), False),
    "resolution-t": (B_, TOY, dict(combination="cat", ts_vad=K_, output_resolution="t", aux_net_output_size=E_CAT), False),
    "auxnet": (B_, TOY, dict(combination="mul", ts_vad=K_), True),
    "production-width": (1, WIDE, dict(combination="mul", ts_vad=K_), False),
}


@pytest.fixture(params=["f32", "bf16x3"])
def gemm_mode(request):
    from tssep_amd import hip_ops
    old = hip_ops.GEMM_PRECISION
    hip_ops.GEMM_PRECISION = request.param
    yield request.param
    hip_ops.GEMM_PRECISION = old


class OneDirectionTorchLayer:
    """The RNNP layer by torch.nn.LSTM(bidirectional=False) + torch.nn.Linear in `dtype` under autograd (the `layer` of
    estimator_forward).  The containers are kept; grads() names their gradients."""

    def __init__(self, dtype):
        self.dtype, self.made = dtype, {}

    def __call__(self, x, p, prefix):
        params = [p[prefix + "net.0." + a] for a in CATTRS] + [p[prefix + "net.1.weight"], p[prefix + "net.1.bias"]]
        lstm, lin = causal_modules([t.detach() for t in params], dtype=self.dtype)
        self.made[prefix] = (lstm, lin)
        y = lin(lstm(x.reshape(-1, x.shape[-2], x.shape[-1]))[0])
        return y.reshape(*x.shape[:-1], y.shape[-1])

    def grads(self):
        out = {}
        for prefix, (lstm, lin) in self.made.items():
            names = ["net.0." + a for a in CATTRS] + ["net.1.weight", "net.1.bias"]
            out.update({prefix + n: t.grad for n, t in zip(names, causal_module_params(lstm, lin))})
        return out


def build(name, shuffle, seed=0, **more):
    from tssep_amd.train import net
    B, widths, kw, auxnet = ROWS[name]
    kw = dict(kw, **more)
    torch.manual_seed(300 + seed)
    E = kw.get("aux_net_output_size") or widths["odim"]
    if auxnet:
        kw["aux_net"], kw["aux_net_output_size"] = net.AuxNet(E), E
    return net.MaskEstimator_v2(rnn_typ="lstm", random_speaker_order=shuffle, **widths, **kw).train()


def outputs_of(name):
    return ("mask", "vad_mask", "vad_logit") if ROWS[name][2].get("explicit_vad") else ("mask", "logit")


def inputs(name, seed=0):
    B, widths, kw, auxnet = ROWS[name]
    rng = np.random.RandomState(600 + seed)
    E = kw.get("aux_net_output_size") or widths["odim"]
    xs = (rng.randn(B, T_FRAMES, widths["idim"]) * 1.5 + 0.3).astype(np.float32)
    if auxnet:
        lens = [[TR.ENROLMENT[(b * K_ + k) % len(TR.ENROLMENT)] for k in range(K_)] for b in range(B)]
        aux = [[(rng.randn(n, E) * 0.7 + 0.2).astype(np.float32) for n in lb] for lb in lens]
    else:
        aux = (rng.randn(B, K_, E) + 0.5).astype(np.float32)
    shape = (B, K_, kw.get("nmask", 1), T_FRAMES, widths["odim"])
    w = {n: rng.randn(*(shape if n in ("mask", "logit") else shape[:4])).astype(np.float32) for n in outputs_of(name)}
    return dict(xs=xs, aux=aux, w=w)


def reference(name, state, inp, perm, dtype):
    """estimator_forward on the weights `state` with the one-direction torch layer, forward and backward of the weighted
    sum over every differentiable output -> {output, "embedding", "d <parameter>", "d xs", "d aux" (a tensor aux)}"""
    B, widths, kw, auxnet = ROWS[name]
    p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in state.items()}
    xs = T_(inp["xs"]).to(dtype).requires_grad_()
    if auxnet:
        aux, leaf = [[T_(s).to(dtype) for s in sb] for sb in inp["aux"]], None
    else:
        aux = leaf = T_(inp["aux"]).to(dtype).requires_grad_()
    layer = OneDirectionTorchLayer(dtype)
    out = ER.estimator_forward(p, xs, aux, odim=widths["odim"], combination=kw["combination"], ts_vad=kw["ts_vad"],
                               output_resolution=kw.get("output_resolution", "tf"), nmask=kw.get("nmask", 1),
                               explicit_vad=kw.get("explicit_vad", False), num_averaged_permutations=kw.get("num_averaged_permutations", 1),
                               layers=widths["layers"], perm=perm, aux_net="auxnet" if auxnet else None, layer=layer)
    sum((out[n] * T_(inp["w"][n]).to(dtype)).sum() for n in outputs_of(name)).backward()
    res = {n: out[n].detach() for n in outputs_of(name)}
    res["embedding"] = out["embedding"].detach()
    grads = {k: v.grad for k, v in p.items()}
    grads.update(layer.grads())
    assert not [k for k, v in grads.items() if v is None]
    res.update({"d " + k: v for k, v in grads.items()})
    res["d xs"] = xs.grad
    if leaf is not None:
        res["d aux"] = leaf.grad
    return res


def device_inputs(name, inp, grad=True):
    xs = T_(inp["xs"]).cuda().requires_grad_(grad)
    if ROWS[name][3]:
        return xs, [[T_(s).cuda() for s in sb] for sb in inp["aux"]], None
    aux = T_(inp["aux"]).cuda().requires_grad_(grad)
    return xs, aux, aux


def held(got, r64, r32, gemm_mode, what, names=None):
    ratios, bad = TR.compare(got, r64, r32, gemm_mode == "bf16x3", what, names)
    worst = max(ratios, key=ratios.get)
    print(f"{what}: worst ratio {ratios[worst]:.3g} ({worst})")
    WORST[(what.split()[0], gemm_mode)] = max(WORST.get((what.split()[0], gemm_mode), 0.0), ratios[worst])
    assert MARGIN == 8.0 and SPLIT_RATIO > 700 and not bad, bad


@pytest.mark.parametrize("name", list(ROWS))
def test_row_against_the_float64_restatement(name, gemm_mode):
    from tssep_amd import hip_ops as h
    shuffle = name in ("cat-tsvad-2trials", "explicit-vad", "auxnet")
    me = build(name, shuffle).cuda()
    state = {k: v.detach().cpu().clone() for k, v in me.state_dict().items()}
    assert not any(k.endswith("_reverse") for k in state)
    inp = inputs(name)
    xs, aux, leaf = device_inputs(name, inp)
    perm = None
    if shuffle:
        np.random.seed(81)
        perm = me.draw_permutations(xs.shape[0], K_)[0]
        np.random.seed(81)                                     # what the module's own draw gives behind the same seed
    h.RECURRENCE_LOG = []
    try:
        out = me(xs, aux)
        sum((getattr(out, n) * T_(inp["w"][n]).cuda()).sum() for n in outputs_of(name)).backward()
        torch.cuda.synchronize()
    finally:
        log, h.RECURRENCE_LOG = h.RECURRENCE_LOG, None
    layers = ROWS[name][1]["layers"] + 1
    assert [e["kernel"] for e in log] == ["stream1_f32"] * (2 * layers) and [e["direction"] for e in log] == ["fwd"] * layers + ["bwd"] * layers
    got = {n: getattr(out, n).detach().cpu() for n in outputs_of(name)}
    got["embedding"] = out.embedding.detach().cpu()
    for k, q in me.named_parameters():
        assert q.grad is not None, k
        got["d " + k] = q.grad.cpu()
    got["d xs"] = xs.grad.cpu()
    if leaf is not None:
        got["d aux"] = leaf.grad.cpu()
    r64, r32 = (reference(name, state, inp, perm, dt) for dt in (torch.float64, torch.float32))
    assert set(got) == set(r64), set(got) ^ set(r64)
    for k in got:
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
    held(got, r64, r32, gemm_mode, f"{name} {gemm_mode}")


@pytest.mark.parametrize("name", ["mul-spk", "cat-tsvad-2trials", "explicit-vad", "two-masks", "resolution-t", "auxnet", "production-width"])
def test_forward_chunk_against_the_float64_restatement(name, gemm_mode):
    """chunks of any lengths, each started from the state the previous call returned, against the float64 outputs of the
    WHOLE utterance; random_speaker_order on: the permutation is drawn once and read from the state"""
    from tssep_amd import hip_ops as h
    from tssep_amd.train import net
    me = build(name, True).cuda().eval()
    state_dict = {k: v.detach().cpu().clone() for k, v in me.state_dict().items()}
    inp = inputs(name)
    xs, aux, _ = device_inputs(name, inp, grad=False)
    names = outputs_of(name)
    ref, first = {}, None
    for chunks in chunkings(T_FRAMES):
        np.random.seed(82)
        draws = []
        mlp = net.AuxNet.forward
        net.AuxNet.forward = lambda self, *a, **k: (draws.append(1), mlp(self, *a, **k))[1]
        h.RECURRENCE_LOG = []
        try:
            state, outs, t0 = None, [], 0
            for n in chunks:
                out, state = me.forward_chunk(xs[:, t0:t0 + n], aux if state is None else None, state)
                assert state.frames == t0 + n and len(state.layers) == ROWS[name][1]["layers"] + 1
                outs.append(out)
                t0 += n
            torch.cuda.synchronize()
        finally:
            log, h.RECURRENCE_LOG = h.RECURRENCE_LOG, None
            net.AuxNet.forward = mlp
        assert len(draws) == int(ROWS[name][3]), "the embedding is computed once, at the first chunk"
        assert all(e["kernel"] == "stream1_f32" and e["direction"] == "fwd" for e in log) and len(log) == len(chunks) * len(state.layers)
        perm = state.perm.cpu().numpy()
        if first is None:
            first = perm
            assert sorted(perm[0].tolist()) == list(range(K_))
            ref = {dt: reference(name, state_dict, inp, perm, dt) for dt in (torch.float64, torch.float32)}
        assert np.array_equal(perm, first)                      # the same seed: the same single draw, whatever the chunking
        got = {n_: torch.cat([getattr(o, n_) for o in outs], dim=-2 if n_ in ("mask", "logit") else -1).cpu() for n_ in names}
        assert not any(t.requires_grad for t in got.values())
        for k in names:
            assert got[k].shape == ref[torch.float64][k].shape, (k, got[k].shape)
        assert torch.equal(outs[0].embedding.cpu(), outs[-1].embedding.cpu())
        held(got, ref[torch.float64], ref[torch.float32], gemm_mode, f"{name} {gemm_mode} chunks {chunks[:3]}", names=names)
    # one frame, un-batched: entry 0 of the batch of one
    np.random.seed(82)
    a0 = aux[0] if ROWS[name][3] else aux[0]
    one, st1 = me.forward_chunk(xs[0, :1], a0)
    np.random.seed(82)
    bat, st2 = me.forward_chunk(xs[:1, :1], aux[:1])
    for n_ in names:
        assert torch.equal(getattr(one, n_), getattr(bat, n_)[0]), n_


def test_the_default_model_is_the_model_without_the_keyword(gemm_mode):
    from tssep_amd import hip_ops as h
    from tssep_amd.train import net
    kw = dict(combination="mul", ts_vad=K_, random_speaker_order=False, **TOY)
    runs = []
    for extra in ({}, dict(rnn_typ="blstm")):
        torch.manual_seed(9)
        me = net.MaskEstimator_v2(**kw, **extra).cuda().train()
        inp = inputs("mul-spk")
        xs, aux = T_(inp["xs"]).cuda().requires_grad_(), T_(inp["aux"]).cuda()
        h.RECURRENCE_LOG = []
        try:
            out = me(xs, aux)
            (out.mask * T_(inp["w"]["mask"]).cuda()).sum().backward()
            torch.cuda.synchronize()
        finally:
            log, h.RECURRENCE_LOG = h.RECURRENCE_LOG, None
        runs.append((list(me.state_dict()), repr(me), log, out.mask.detach(), out.logit.detach(), xs.grad, [q.grad for q in me.parameters()]))
    a, b = runs
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and not any(e["kernel"] == "stream1_f32" for e in a[2])
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
    assert all(torch.equal(x, y) for x, y in zip(a[6], b[6]))


# ---- the trainer: hipGraph replay and the kernel plan ------------------------------------------------------------------------
def _model(units=24, projs=24, seed=21):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net
    torch.manual_seed(seed)
    return model.Model(
        fe=fe.ConcaternatedSTFTFeatures(
            fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=units, projs=projs, combination="mul",
                                            aux_net_output_size=513, ts_vad=4, output_resolution="tf", rnn_typ="lstm",
                                            random_speaker_order=True, num_averaged_permutations=1),
        enhancer=enhancer.Masking(), loss=loss.LogMAE())


def test_trainer_graph_step_is_bit_identical_to_the_eager_trainer(tmp_path):
    """tests/test_gpu_dropout.py::test_trainer_graph_step_is_bit_identical_to_the_eager_trainer on a causal model: the
    one-direction launches have no exchange buffer, no spin and no error flag, so they are captured as they stand; losses of
    every iteration and the final parameters are bit-identical, and the kernel plan names the kernel."""
    from test_gpu_dropout import _batch
    from tssep_amd.train import runtime
    from tssep_amd.train.optimizer import Adam
    from tssep_amd.train.trainer import Trainer
    data = [_batch(2, 4, 5000 if i % 2 else 7300, seed=31 + i) for i in range(4)]

    class Dataset(list):
        def __iter__(self):
            return (dict(ex) for ex in list.__iter__(self))

    runs = {}
    for mode in ("off", "on"):
        with runtime.applied(graph_step=mode):
            np.random.seed(77)
            tr = Trainer(_model(), tmp_path / mode, Adam(gradient_clipping=10.0, lr=1e-3), summary_trigger=(1, "iteration"),
                         checkpoint_trigger=(1000, "iteration"), stop_trigger=(8, "iteration"), virtual_minibatch_size=2)
            hist = tr.train(Dataset(data), device=0)
            torch.cuda.synchronize()
            hf = json.loads((tmp_path / mode / "log" / "history.json").read_text())
            plan = json.loads((tmp_path / mode / "log" / "kernel_plan.json").read_text())
            runs[mode] = ([l for _, l in hist], tr.optimizer.flat_param.clone(), hf, plan)
    l_off, p_off, _, plan_off = runs["off"]
    l_on, p_on, h_on, plan_on = runs["on"]
    assert len(l_off) == 8 and all(np.isfinite(l_off))
    assert h_on.get("graph_replays", 0) == 7 and h_on["graphs"] == 2, h_on
    assert l_on == l_off, [(i, a, b) for i, (a, b) in enumerate(zip(l_on, l_off)) if a != b]
    assert torch.equal(p_on, p_off), float((p_on - p_off).abs().max())
    for plan in (plan_off, plan_on):
        rec = plan["recurrence"]
        assert rec and all(r["kernel"] == "stream1_f32" for r in rec), rec
        assert {r["direction"] for r in rec} == {"fwd", "bwd"}      # (one entry per distinct launch shape and direction)


def test_toy_experiment_with_the_causal_overlay(tmp_path):
    """run_tssep with toy_tssep_causal.yaml, initialised from a causal TS-VAD model's checkpoint (InitCheckPointVAD2Sep grows
    the head; nothing in it knows the layer type): trains its iterations with finite losses and writes a kernel plan that
    names stream1_f32 and nothing else"""
    import os
    import yaml
    from tssep_amd.exp import run_tssep
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
    cfg = run.build_config([os.path.join(exp, y) for y in ("toy_common.yaml", "toy_tsvad.yaml", "toy_tssep_causal.yaml")]
                           + [f"eg.trainer.storage_dir={tmp_path / 'v'}"])
    vad = Experiment.from_config(cfg["eg"]).trainer.model
    assert vad.mask_estimator.rnn_typ == "lstm"
    ck = tmp_path / "vad.pth"
    torch.save({"model": vad.state_dict()}, ck)
    fast = ["eg.trainer.stop_trigger=[3,iteration]", "eg.trainer.checkpoint_trigger=[3,iteration]",
            "eg.trainer.summary_trigger=[1,iteration]"]
    sep_dir = run_tssep.main(configs=tuple(os.path.join(exp, y) for y in ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_causal.yaml")),
                             storage_dir=tmp_path / "tssep", checkpoint=ck, overrides=fast)
    frozen = yaml.safe_load((sep_dir / "config.yaml").read_text())
    assert frozen["eg"]["trainer"]["model"]["mask_estimator"]["rnn_typ"] == "lstm"
    hist = json.loads((sep_dir / "log" / "history.json").read_text())
    assert hist["iteration"] == 3 and len(hist["loss"]) == 3 and all(np.isfinite(l) for _, l in hist["loss"])
    plan = json.loads((sep_dir / "log" / "kernel_plan.json").read_text())
    assert plan["recurrence"] and all(r["kernel"] == "stream1_f32" for r in plan["recurrence"]), plan["recurrence"]
    sd = torch.load(sep_dir / "checkpoints" / "ckpt_latest.pth", map_location="cpu")
    assert not any(k.endswith("_reverse") for k in sd["model"])


def test_zz_report():
    for (what, mode_), v in sorted(WORST.items()):
        print(f"{what:20s} {mode_:7s} worst ratio to the fp32 run {v:.3g}")
