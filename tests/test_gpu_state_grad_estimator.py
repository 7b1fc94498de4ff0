"""MaskEstimator_v2.train_chunk -- forward_chunk's contract with gradients -- on a real MI355X: a tiny causal estimator
(the option sets of tests/test_causal_reference.py's ESTIMATORS at tests/test_gpu_causal_estimator.py's toy widths), T = 23
as chunks (5, 1, 17), random_speaker_order on.

detach=False (full BPTT over chunks, one backward at the end): outputs, every parameter gradient, d(xs) and d(aux) against
tests/estimator_reference.py::estimator_forward's float64 WHOLE-utterance run, under test_gpu_causal_estimator.held's
measure (MARGIN x the float32 run's own error, x SPLIT_RATIO under split-bf16 GEMMs).
detach=True (truncated BPTT, backward after every chunk): against the same float64 restatement with every recurrent layer
run over the same chunks and its state detached at the same places.  d(aux) is left out there: the embedding a later chunk
reads is detached too, which the whole-utterance restatement cannot express (a parameter gradient does not pass through it:
the embedding of these models is the input itself).
The permutation is drawn once and the embedding computed once, whatever `detach`; the refusals are forward_chunk's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import estimator_reference as ER  # noqa: E402
import test_gpu_causal_estimator as CE  # noqa: E402
from test_causal_reference import ESTIMATORS  # noqa: E402
from test_gpu_causal_estimator import K_, T_, T_FRAMES, TOY, gemm_mode, held  # noqa: E402,F401  (gemm_mode: the fixture)

CHUNKS = (5, 1, 17)
# (the helpers of test_gpu_causal_estimator look their row up by name: the rows of this file are added under names of their own)
NAMES = {}
for _kw in (ESTIMATORS[0], ESTIMATORS[3]):
    _name = f"state-grad-{_kw['combination']}-{_kw['ts_vad']}"
    CE.ROWS.setdefault(_name, (CE.B_, TOY, dict(_kw), False))
    NAMES[_name] = _kw


class ChunkedTorchLayer(CE.OneDirectionTorchLayer):
    """the one-direction torch layer run over CHUNKS, the state handed over DETACHED: truncated BPTT in torch"""

    def __call__(self, x, p, prefix):
        from test_causal_reference import CATTRS, causal_modules
        params = [p[prefix + "net.0." + a] for a in CATTRS] + [p[prefix + "net.1.weight"], p[prefix + "net.1.bias"]]
        lstm, lin = causal_modules([t.detach() for t in params], dtype=self.dtype)
        self.made[prefix] = (lstm, lin)
        x3 = x.reshape(-1, x.shape[-2], x.shape[-1])
        ys, state, t0 = [], None, 0
        for n in CHUNKS:
            h, state = lstm(x3[:, t0:t0 + n], state)
            state = tuple(s.detach() for s in state)
            ys.append(lin(h))
            t0 += n
        y = torch.cat(ys, 1)
        return y.reshape(*x.shape[:-1], y.shape[-1])


def reference(name, state, inp, perm, dtype, detached):
    """test_gpu_causal_estimator.reference; detached: with the chunked, detached layer (and without d aux)"""
    if not detached:
        return CE.reference(name, state, inp, perm, dtype)
    B, widths, kw, _ = CE.ROWS[name]
    p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in state.items()}
    xs = T_(inp["xs"]).to(dtype).requires_grad_()
    aux = T_(inp["aux"]).to(dtype)
    layer = ChunkedTorchLayer(dtype)
    out = ER.estimator_forward(p, xs, aux, odim=widths["odim"], combination=kw["combination"], ts_vad=kw["ts_vad"],
                               output_resolution="tf", nmask=1, explicit_vad=False, num_averaged_permutations=1,
                               layers=widths["layers"], perm=perm, aux_net=None, layer=layer)
    sum((out[n] * T_(inp["w"][n]).to(dtype)).sum() for n in CE.outputs_of(name)).backward()
    res = {n: out[n].detach() for n in CE.outputs_of(name)}
    res["embedding"] = out["embedding"].detach()
    grads = {k: v.grad for k, v in p.items()}
    grads.update(layer.grads())
    assert not [k for k, v in grads.items() if v is None]
    res.update({"d " + k: v for k, v in grads.items()})
    res["d xs"] = xs.grad
    return res


@pytest.mark.parametrize("detach", [False, True], ids=["full", "detached"])
@pytest.mark.parametrize("name", list(NAMES))
def test_train_chunk_against_the_float64_restatement(name, detach, gemm_mode):
    from tssep_amd import hip_ops as h
    from tssep_amd.train import net
    me = CE.build(name, True).cuda()
    assert me.training and sum(CHUNKS) == T_FRAMES
    weights = {k: v.detach().cpu().clone() for k, v in me.state_dict().items()}
    inp = CE.inputs(name)
    xs, aux, leaf = CE.device_inputs(name, inp)
    names = CE.outputs_of(name)
    np.random.seed(83)
    calls = dict(perm=0, emb=0)
    draw, emb = net.MaskEstimator_v2._speaker_permutations, net.MaskEstimator_v2._embedding
    net.MaskEstimator_v2._speaker_permutations = lambda self, *a: (calls.__setitem__("perm", calls["perm"] + 1), draw(self, *a))[1]
    net.MaskEstimator_v2._embedding = lambda self, *a: (calls.__setitem__("emb", calls["emb"] + 1), emb(self, *a))[1]
    h.RECURRENCE_LOG = []
    try:
        state, outs, t0, total = None, [], 0, 0.0
        for n in CHUNKS:
            out, state = me.train_chunk(xs[:, t0:t0 + n], aux if state is None else None, state, detach=detach)
            assert isinstance(state, net.ChunkState) and state.frames == t0 + n and len(state.layers) == TOY["layers"] + 1
            in_graph = [s.requires_grad for hc in state.layers for s in hc]
            assert in_graph == [not detach] * len(in_graph), "detach decides whether the state stays in the graph"
            assert state.embedding.requires_grad == (not detach)
            loss = sum((getattr(out, k) * T_(inp["w"][k][..., t0:t0 + n, :]).cuda()).sum() for k in names)
            if detach:
                loss.backward()          # truncated BPTT: after every chunk
            else:
                total = total + loss
            outs.append(out)
            t0 += n
        if not detach:
            total.backward()
        torch.cuda.synchronize()
    finally:
        log, h.RECURRENCE_LOG = h.RECURRENCE_LOG, None
        net.MaskEstimator_v2._speaker_permutations, net.MaskEstimator_v2._embedding = draw, emb
    assert calls == dict(perm=1, emb=1), "the permutation is drawn once and the embedding computed once"
    assert all(e["kernel"] == "stream1_f32" for e in log) and len(log) == 2 * len(CHUNKS) * len(state.layers)
    perm = state.perm.cpu().numpy()
    assert sorted(perm[0].tolist()) == list(range(K_))
    got = {k: torch.cat([getattr(o, k) for o in outs], dim=-2).detach().cpu() for k in names}
    got["embedding"] = outs[0].embedding.detach().cpu()
    assert torch.equal(outs[0].embedding, outs[-1].embedding)
    for k, q in me.named_parameters():
        assert q.grad is not None, k
        got["d " + k] = q.grad.cpu()
    got["d xs"] = xs.grad.cpu()
    if not detach:
        got["d aux"] = leaf.grad.cpu()
    r64, r32 = (reference(name, weights, inp, perm, dt, detach) for dt in (torch.float64, torch.float32))
    assert set(got) == set(r64), set(got) ^ set(r64)
    for k in got:
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
    held(got, r64, r32, gemm_mode, f"{name}-{'detached' if detach else 'full'} {gemm_mode}")
    if detach:      # and the truncated gradient is not the full one: far outside the bound against the whole utterance
        full = CE.reference(name, weights, inp, perm, torch.float64)
        k = "d pre_net.net.0.weight_hh_l0"
        far = float((r64[k] - full[k]).abs().max() / full[k].abs().max())
        print(f"{name}: truncated against full {k}: {far:.3g}")
        assert far > 1e-2, far


def test_train_chunk_refuses_what_forward_chunk_refuses():
    from tssep_amd.train import net
    base = dict(idim=8, layers=2, units=5, projs=12, combination="mul")
    xs, aux = torch.zeros(2, 3, 8, device="cuda"), torch.zeros(2, 4, 8, device="cuda")
    with pytest.raises(ValueError, match="reads the future"):
        net.MaskEstimator_v2(**base).cuda().train_chunk(xs, aux)
    with pytest.raises(NotImplementedError, match="span the utterance"):
        net.MaskEstimator_v2(rnn_typ="lstm", input_normalizer=net.InstanceNorm(), **base).cuda().train_chunk(xs, aux)
    m = net.MaskEstimator_v2(rnn_typ="lstm", **base).cuda()
    with pytest.raises(NotImplementedError, match="frame-wise"):
        m.train_chunk(xs, torch.zeros(2, 4, 3, 8, device="cuda"))
    with pytest.raises(ValueError, match="Tc >= 1"):
        m.train_chunk(xs[:, :0], aux)
    with pytest.raises(TypeError):
        m.train_chunk(xs, aux, state=object())
    # forward_chunk itself is what it was: without gradients, a state out of the graph
    out, state = m.forward_chunk(xs, aux)
    assert not out.mask.requires_grad and not any(s.requires_grad for hc in state.layers for s in hc)
