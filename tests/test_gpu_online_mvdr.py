"""The frame-recursive MVDR on a real MI355X: hip_ops.online_mvdr against the extended-precision restatement
of tests/test_online_mvdr_reference.py under that file's comparison (output AND state within 8 x the float64 restatement's
own distance), bit-identity across the ways a stream can be split into calls, the silent-start rule, the enhancer class
and the separator `Model.online` builds on it.

Shapes: B = 2, K = 3, F = 70 (two bin tiles, the second ragged), T = 7, reference_channel = 1; D = 2 / 6 the smallest /
largest register-resident elimination, D = 7 the LDS one.  One wave serves one (b, k, 64 bins): the K workgroups of a tile
are the kernel's only grouping, and the launch rounds the tiles up to the 8 XCDs, so B * ceil(F / 64) = 4, 2 or 9 tiles
cover a ragged round, and F = 513 with K = 8 a second round on the bin axis.

Measured on an MI355X (worst error / yardstick, the same for every input type): output 1.40 (D = 2), 1.66 (D = 6), 1.25
(D = 7); state 0.77, 1.00, 1.00; forgetting 0.9: 1.01 / 0.70 / 1.16; F = 513, K = 8: 1.02; the bound is 8."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_online_mvdr_reference as R  # noqa: E402

B, K, F, T = 2, 3, 70, 7
MDT = {"f32": torch.float32, "f64": torch.float64}
YDT = {"c64": torch.complex64, "c128": torch.complex128}


@functools.lru_cache(maxsize=None)
def case(D, name, **shape):
    return R.gpu_case(D, name, **{"T": T, "F": F, "B": B, "K": K, **shape})


def _dev(Y, m, mdt="f64", ydt="c128"):
    return torch.as_tensor(m).to(MDT[mdt]).cuda(), torch.as_tensor(Y).to(YDT[ydt]).cuda()


def _kernel(Y, m, kw, mdt="f64", ydt="c128", splits=None, state=None):
    """-> (enh [B,K,T,F] complex128, state) of the frames pushed in `splits`"""
    from tssep_amd import hip_ops
    masks, obs = _dev(Y, m, mdt, ydt)
    kw = dict(kw)
    ref = kw.pop("ref")
    outs, pos = [], 0
    for c in splits or (Y.shape[2],):
        e, state = hip_ops.online_mvdr(masks[:, :, pos:pos + c], obs[:, :, pos:pos + c], state, ref, **kw)
        assert e.dtype == torch.complex128 and tuple(e.shape) == (m.shape[0], m.shape[1], c, m.shape[3])
        outs.append(e)
        pos += c
    assert pos == Y.shape[2]
    return torch.cat(outs, dim=2), state


def _check(D, name, what, mdt="f64", ydt="c128", **shape):
    Y, m, kw, ref, ys = case(D, name, **shape)
    enh, state = _kernel(Y, m, kw, mdt, ydt)
    ro, rs = R.held(enh.cpu().numpy(), state.cpu().numpy(), ref, ys, f"D={D} {what}")
    assert ro <= R.FACTOR and rs <= R.FACTOR, (ro, rs)


@pytest.mark.parametrize("ydt", tuple(YDT))
@pytest.mark.parametrize("mdt", tuple(MDT))
@pytest.mark.parametrize("D", (2, 6, 7))
def test_kernel_against_extended_reference(D, mdt, ydt):
    _check(D, "plain", f"{mdt} {ydt}", mdt, ydt)


@pytest.mark.parametrize("name", ("forgetting", "masking"))
@pytest.mark.parametrize("D", (2, 6, 7))
def test_forgetting_and_masking_against_reference(D, name):
    _check(D, name, name, "f32", "c64")


def test_one_batch_element_five_speakers():
    """K = 5 workgroups per tile, B * nf = 2 tiles of a round of 8"""
    _check(6, "plain", "B=1 K=5", "f32", "c64", B=1, K=5)


def test_second_round_on_the_bin_axis():
    _check(6, "plain", "F=513 K=8 T=2", "f32", "c64", B=1, K=8, F=513, T=2)


@pytest.mark.parametrize("D", (2, 6, 7))
def test_splits_give_the_same_bits(D):
    Y, m, kw, _, _ = case(D, "forgetting")
    whole, sw = _kernel(Y, m, kw, "f32", "c64", (7,))
    for splits in ((1, 2, 4), (3, 4), (1,) * 7):
        e, s = _kernel(Y, m, kw, "f32", "c64", splits)
        assert torch.equal(torch.view_as_real(e), torch.view_as_real(whole)), splits
        assert torch.equal(s, sw), splits


@pytest.mark.parametrize("D", (2, 7))
def test_silent_leading_chunk(D):
    Y, m, kw, _, _ = case(D, "plain")
    Y0 = np.concatenate([np.zeros_like(Y[:, :, :3]), Y], axis=2)
    m0 = np.concatenate([m[:, :, :3], m], axis=2)
    lead, s0 = _kernel(Y0[:, :, :3], m0[:, :, :3], kw)
    assert bool((torch.view_as_real(lead) == 0).all()) and bool((s0 == 0).all())
    late, s1 = _kernel(Y0[:, :, 3:], m0[:, :, 3:], kw, state=s0)
    fresh, s2 = _kernel(Y, m, kw)
    assert torch.equal(torch.view_as_real(late), torch.view_as_real(fresh)) and torch.equal(s1, s2)
    assert bool(torch.isfinite(torch.view_as_real(late)).all())
    both, s3 = _kernel(Y0, m0, kw, splits=(10,))                    # the silence and the signal in one call
    assert torch.equal(torch.view_as_real(both[:, :, 3:]), torch.view_as_real(fresh)) and torch.equal(s3, s2)
    assert bool((torch.view_as_real(both[:, :, :3]) == 0).all())


def test_enhancer_on_a_whole_utterance_is_the_chunked_kernel():
    from tssep_amd.train import enhancer
    Y, m, kw, _, _ = case(6, "forgetting")
    bf = enhancer.OnlineMVDR(forgetting=0.9, diag_load=1e-3)
    masks, obs = _dev(Y, m, "f32", "c64")
    with torch.no_grad():
        whole = bf(masks[:, :, None], {"Observation": obs, "reference_channel": 1}, None)
        one = bf(masks[0, :, None], {"Observation": obs[0], "reference_channel": 1}, None)
    chunks, _ = _kernel(Y, m, kw, "f32", "c64", (2, 5))
    assert torch.equal(torch.view_as_real(whole), torch.view_as_real(chunks))
    assert torch.equal(torch.view_as_real(one), torch.view_as_real(whole[0]))
    with pytest.raises(NotImplementedError, match="evaluation-time"):
        bf(masks[:, :, None].clone().requires_grad_(), {"Observation": obs, "reference_channel": 1}, None)


def test_capture_and_replay():
    from tssep_amd import hip_ops
    D = 6
    Y, m, kw, _, _ = case(D, "forgetting")
    kw = dict(kw)
    ref = kw.pop("ref")
    masks, obs = _dev(Y, m, "f32", "c64")
    sm, so = torch.zeros_like(masks[:, :, :3]), torch.zeros_like(obs[:, :, :3])
    ss = torch.zeros(B, K, 2, D * D, F, device="cuda", dtype=torch.float64)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hip_ops.online_mvdr(sm, so, ss, ref, **kw)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ge, gs = hip_ops.online_mvdr(sm, so, ss, ref, **kw)
    state = None
    for pos in (0, 3):                                              # two replays on fresh input, the state carried
        sm.copy_(masks[:, :, pos:pos + 3])
        so.copy_(obs[:, :, pos:pos + 3])
        ss.copy_(state if state is not None else torch.zeros_like(ss))
        g.replay()
        e, state = hip_ops.online_mvdr(masks[:, :, pos:pos + 3], obs[:, :, pos:pos + 3], state, ref, **kw)
        assert torch.equal(torch.view_as_real(ge), torch.view_as_real(e)) and torch.equal(gs, state), pos


# ---- the separator ---------------------------------------------------------------------------------------------------------
SB, SK, SD, SN = 2, 3, 3, 256 * 8 + 100
WIDTHS = dict(idim=553, odim=513, units=8, projs=12, layers=3)


def _model(enh, seed=5, **me):
    """(the `_model()` shapes of tests/test_online_reference.py / test_gpu_online.py)"""
    from tssep_amd.data import DummyReader
    from tssep_amd.train import feature_extractor as fe, loss, model, net
    torch.manual_seed(seed)
    f = fe.ConcaternatedSTFTFeatures(
        fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True), size=1024, shift=256, window="hann")
    kw = dict(combination="mul", ts_vad=SK, rnn_typ="lstm", random_speaker_order=False, **WIDTHS)
    kw.update(me)
    return model.Model(fe=f, reader=DummyReader(), mask_estimator=net.MaskEstimator_v2(**kw), enhancer=enh,
                       loss=loss.LogMAE()).cuda().eval()


def _signal(seed=3):
    rng = np.random.RandomState(seed)
    src = rng.randn(SB, 1, SN) * np.linspace(0.05, 1.0, SN)
    x = (src * rng.uniform(0.5, 1.5, (SB, SD, 1)) + 0.1 * rng.randn(SB, SD, SN)).astype(np.float32)
    x[0, :, :300] = 0                                                                    # digital silence first
    aux = (rng.randn(SB, SK, 513) + 0.5).astype(np.float32)
    return torch.as_tensor(x).cuda(), torch.as_tensor(aux).cuda()


def _push_all(sep, x, pushes):
    ys, pos = [], 0
    for p in pushes:
        ys.append(sep.push(x[..., pos:pos + p * 256]))
        pos += p * 256
    ys.append(sep.flush(x[..., pos:]))
    return torch.cat(ys, dim=-1)


@pytest.mark.parametrize("explicit_vad", (False, True))
def test_online_separator_with_online_mvdr(explicit_vad):
    """Pushes of 2, 5 and 1 hops and a ragged flush.  The chunk trunk's logits are not the whole-utterance forward's bits
    (its GEMMs see other row counts; tests/test_gpu_online.py holds them to the float64 restatement instead), so the
    comparison starts where it first can: from the masks the stream formed, the audio is
    fe.istft(OnlineMVDR()(masks, whole-utterance STFT)) bit for bit."""
    from tssep_amd.train import enhancer
    ref = 1
    model = _model(enhancer.OnlineMVDR(), explicit_vad=explicit_vad)
    fe = model.fe
    x, aux = _signal()
    sep = model.online(aux, record=True, reference_channel=ref)
    y = _push_all(sep, x, (2, 5, 1))
    assert tuple(y.shape) == (SB, SK, SN) and bool(torch.isfinite(y).all()) and sep.frames == fe.frames(SN)
    X = fe.stft(x)                                                                       # [B, D, T, F]
    Obs = torch.cat([r["Observation"] for r in sep.record], dim=-2)
    assert torch.equal(torch.view_as_real(Obs), torch.view_as_real(X))
    feat = torch.cat([r["Input"] for r in sep.record], dim=-2)
    assert torch.equal(feat, fe.stft_to_feature(X[:, ref].contiguous()))
    masks = torch.cat([r["mask"] for r in sep.record], dim=-2)
    assert tuple(masks.shape) == (SB, SK, 1, X.shape[-2], 513)
    with torch.no_grad():
        enh = model.enhancer(masks, {"Observation": X, "reference_channel": ref}, model)
        want = fe.istft(enh, num_samples=SN)
    assert torch.equal(torch.view_as_real(torch.cat([r["Estimate"] for r in sep.record], dim=-2)), torch.view_as_real(enh))
    assert torch.equal(y, want)
    # the whole-utterance forward with this enhancer runs the same recursion on its own masks
    with torch.no_grad():
        whole = model.mask_estimator(feat, aux)
        est = model.enhancer(whole.mask, {"Observation": X, "reference_channel": ref}, model)
    assert tuple(est.shape) == tuple(enh.shape) and bool(torch.isfinite(torch.view_as_real(est)).all())
    # one un-batched stream: entry 1 of the batch
    one = model.online(aux[1], reference_channel=ref)
    y1 = _push_all(one, x[1], (2, 5, 1))
    bat = model.online(aux[1:], reference_channel=ref)
    assert torch.equal(y1, _push_all(bat, x[1:], (2, 5, 1))[0])
    with pytest.raises(ValueError, match=r"\[B, D, n\]"):
        model.online(aux).push(x[0, 0, :256])


def test_masking_stream_is_what_it_was():
    """The Masking route ignores reference_channel and still is fe.masked_istft of its own chunk logits, bit for bit."""
    from tssep_amd.train import enhancer
    model = _model(enhancer.Masking())
    fe = model.fe
    x, aux = _signal()
    x = x[:, 0].contiguous()
    seps = [model.online(aux, record=True), model.online(aux, record=True, reference_channel=2)]
    ys = [_push_all(s, x, (2, 5, 1)) for s in seps]
    assert torch.equal(ys[0], ys[1]) and tuple(ys[0].shape) == (SB, SK, SN)
    logit = torch.cat([r["logit"] for r in seps[0].record], dim=-2)
    assert torch.equal(ys[0], fe.masked_istft(logit, fe.stft(x), num_samples=SN))
    assert set(seps[0].record[0]) == {"Observation", "Input", "logit"} and seps[0]._psd is None
