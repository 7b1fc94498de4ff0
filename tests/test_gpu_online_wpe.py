"""The recursive WPE on a real MI355X: hip_ops.online_wpe against the extended-precision restatement of
tests/test_online_wpe_reference.py under that file's comparison (output, G and Q within 8 x the float64 restatement's own
distance), bit-identity across the ways a stream can be split into calls, the silent-start rule, a NaN frame, the enhancer
classes and the separator `Model.online` builds on them.

Shapes: B = 2, F = 5 (ten workgroups), T = delay + taps + 3 (the ring wraps and every tap slot holds data);
(D, taps, delay) = (1, 1, 0) the smallest system and no ring at all, (2, 3, 2) K = 6, (3, 4, 1) K = 12, ragged against any
tiling by 8 or 16, (6, 10, 2) K = 60 the production shape, (8, 10, 3) K = 80 the LDS limit (above 64 KB); B = 2, F = 513,
T = 2 at K = 6 for the grid.

Measured on an MI355X: the worst error is 2.34 x its yardstick (Q at K = 60 with forgetting 0.9), the bound is 8; the
table is in the docstring of test_kernel_against_extended_reference."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_online_mvdr as M  # noqa: E402
import test_online_wpe_reference as R  # noqa: E402

YDT = {"c64": torch.complex64, "c128": torch.complex128}
MODES = {"plain": dict(forgetting=1.0, power_context=0), "forget_context": dict(forgetting=0.9, power_context=2)}


def _bits(a, b):
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.shape == b.shape and (a.numel() == 0 or torch.equal(a, b))


def _same(xa, sa, xb, sb):
    return _bits(xa, xb) and all(_bits(p, q) for p, q in zip(sa, sb))


def _kernel(Y, kw, ydt="c128", splits=None, state=None):
    """-> (X [B,D,T,F] complex128, state) of the frames pushed in `splits`"""
    from tssep_amd import hip_ops
    obs = torch.as_tensor(Y).to(YDT[ydt]).cuda()
    outs, pos = [], 0
    for c in splits or (Y.shape[2],):
        x, state = hip_ops.online_wpe(obs[:, :, pos:pos + c], state, **kw)
        assert x.dtype == torch.complex128 and tuple(x.shape) == (Y.shape[0], Y.shape[1], c, Y.shape[3])
        outs.append(x)
        pos += c
    assert pos == Y.shape[2]
    return torch.cat(outs, dim=2), state


def _check(shape, mode, ydt, **dims):
    D, taps, delay = shape
    Y, kw, ref, ys = R.gpu_case(D, taps, delay, **MODES[mode], **dims)
    X, st = _kernel(Y, kw, ydt)
    r = R.held(X.cpu().numpy(), R.unpack_q(st.Q.cpu().numpy(), D * taps), st.G.cpu().numpy(), ref, ys,
               f"{shape} {mode} {ydt}")
    assert max(r) <= R.FACTOR, r
    _, _, ring, pmax, info = R.pack_state(ref[1])
    assert np.array_equal(st.ring.cpu().numpy(), ring) and np.array_equal(st.info.cpu().numpy(), info)
    # pmax is one of the p: a sum of 2 D (c + 1) squares and a division, every operation within one rounding
    n = 2 * D * (kw["power_context"] + 1) + 2
    assert np.all(np.abs(st.pmax.cpu().numpy() - pmax) <= n * 2.0 ** -53 * pmax)


@pytest.mark.parametrize("ydt", tuple(YDT))
@pytest.mark.parametrize("mode", tuple(MODES))
@pytest.mark.parametrize("shape", R.SHAPES)
def test_kernel_against_extended_reference(shape, mode, ydt):
    """Measured on an MI355X (output / G / Q over their yardsticks, the same for c64 and c128; plain | forget_context):
    (1, 1, 0) 0.31 / 0.57 / 1.00 | 0.36 / 0.54 / 1.00;    (2, 3, 2) 0.75 / 1.11 / 0.52 | 1.07 / 0.80 / 1.40;
    (3, 4, 1) 0.77 / 0.74 / 0.69 | 1.10 / 1.05 / 1.91;    (6, 10, 2) 0.64 / 0.67 / 0.80 | 0.64 / 0.91 / 2.34;
    (8, 10, 3) 0.63 / 0.66 / 0.90 | 0.89 / 0.78 / 2.04.   Q with forgetting < 1 carries the kernel's product with 1 / a
    where the restatement divides by a.  The bound is 8."""
    _check(shape, mode, ydt)


def test_every_bin_of_a_wide_grid():
    """B = 2, F = 513: 1026 workgroups, four per CU.  T = 2 does not reach past the delay: the taps stay zero and the output is
    the input exactly; what is compared is Q.  Measured: Q 0.81 x its yardstick (2^-52, the floor)."""
    _check((2, 3, 2), "forget_context", "c64", B=2, F=513, T=2)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_splits_give_the_same_bits(shape):
    D, taps, delay = shape
    Y, kw, _, _ = R.gpu_case(D, taps, delay, **MODES["forget_context"])
    T = Y.shape[2]
    whole, sw = _kernel(Y, kw, "c64", (T,))
    for splits in ((1,) * T, (1, T - 1), (delay + 1, T - delay - 1)):
        x, s = _kernel(Y, kw, "c64", splits)
        assert _same(x, s, whole, sw), splits


@pytest.mark.parametrize("shape", ((2, 3, 2), (8, 10, 3)))
def test_silent_leading_chunk(shape):
    D, taps, delay = shape
    Y, kw, _, _ = R.gpu_case(D, taps, delay, **MODES["forget_context"])
    Y0 = np.concatenate([np.zeros_like(Y[:, :, :3]), Y], axis=2)
    lead, s0 = _kernel(Y0[:, :, :3], kw)
    assert bool((torch.view_as_real(lead) == 0).all())
    assert all(bool((t == 0).all()) for t in (torch.view_as_real(s0.Q), torch.view_as_real(s0.G),
                                               torch.view_as_real(s0.ring), s0.pmax, s0.info))
    late, s1 = _kernel(Y0[:, :, 3:], kw, state=s0)
    fresh, s2 = _kernel(Y, kw)
    assert _same(late, s1, fresh, s2) and bool(torch.isfinite(torch.view_as_real(late)).all())
    both, s3 = _kernel(Y0, kw)                                      # the silence and the signal in one call
    assert _same(both[:, :, 3:], s3, fresh, s2) and bool((torch.view_as_real(both[:, :, :3]) == 0).all())
    assert int(s2.info.sum()) == 0 and float(s2.pmax.min()) > 0


def test_nan_frame_is_counted_and_leaves():
    """One NaN in Y: the frames whose power or whose delayed frames hold it are refused and counted (as the restatement
    counts them), Q and G stay finite, the output is finite again once the NaN has left the ring, and no other
    (batch element, bin) sees any of it."""
    D, taps, delay, T = 2, 3, 2, 14
    Y, kw, _, _ = R.gpu_case(D, taps, delay, T=T)
    bad = Y.copy()
    bad[1, 1, 3, 2] = np.nan
    _, rs, _ = R.online_wpe_reference(bad, extended=False, **kw)
    assert rs["info"].tolist() == [0, 1 + taps]
    for splits in ((T,), (4, 3, 7)):
        X, st = _kernel(bad, kw, "c128", splits)
        clean, sc = _kernel(Y, kw, "c128", splits)
        assert st.info.tolist() == rs["info"].tolist() and sc.info.tolist() == [0, 0]
        assert bool(torch.isfinite(torch.view_as_real(st.Q)).all()) and bool(torch.isfinite(torch.view_as_real(st.G)).all())
        assert bool(torch.isfinite(st.pmax).all())
        gone = 3 + delay + taps                                       # the first frame whose taps no longer reach frame 3
        assert bool(torch.isfinite(torch.view_as_real(X[:, :, gone:])).all())
        assert bool(torch.isnan(torch.view_as_real(X[1, :, 3, 2])).any())
        keep = torch.ones(2, 5, dtype=torch.bool)
        keep[1, 2] = False
        keep = keep.cuda()
        assert torch.equal(torch.view_as_real(X.permute(0, 3, 1, 2)[keep]), torch.view_as_real(clean.permute(0, 3, 1, 2)[keep]))
        assert torch.equal(torch.view_as_real(st.Q[keep]), torch.view_as_real(sc.Q[keep]))


def test_online_wpe_class_on_a_whole_utterance_is_the_chunked_kernel():
    from tssep_amd.train import enhancer
    D, taps, delay = 3, 4, 1
    Y, kw, _, _ = R.gpu_case(D, taps, delay, **MODES["forget_context"])
    w = enhancer.OnlineWPE(**kw)
    chunks, _ = _kernel(Y[1:], kw, "c128", (2, Y.shape[2] - 2))
    whole = w(torch.as_tensor(Y[1]).cuda())
    assert whole.is_cuda and _bits(whole, chunks[0])
    host = w(Y[1])
    assert isinstance(host, np.ndarray) and np.array_equal(host, chunks[0].cpu().numpy())
    x, s = w.chunk(torch.as_tensor(Y).to(torch.complex64).cuda())
    assert _same(x, s, *_kernel(Y, kw, "c64"))


def test_online_mvdr_with_pre_wpe_is_the_two_kernels():
    from tssep_amd import hip_ops
    from tssep_amd.train import enhancer
    D, taps, delay = 3, 4, 1
    Y, kw, _, _ = R.gpu_case(D, taps, delay, **MODES["forget_context"])
    B, _, T, F = Y.shape
    obs = torch.as_tensor(Y).to(torch.complex64).cuda()
    masks = torch.rand(B, 2, 1, T, F, generator=torch.Generator().manual_seed(1)).cuda()
    bf = enhancer.OnlineMVDR(forgetting=0.95, diag_load=1e-3, pre_wpe=enhancer.OnlineWPE(**kw))
    X, _ = hip_ops.online_wpe(obs, **kw)
    want, psd = hip_ops.online_mvdr(masks, X, None, 1, forgetting=0.95, diag_load=1e-3)
    with torch.no_grad():
        whole = bf(masks, {"Observation": obs, "reference_channel": 1}, None)
        one = bf(masks[1], {"Observation": obs[1], "reference_channel": 1}, None)
    assert _bits(whole, want) and _bits(one, want[1])
    parts, state = [], None
    for lo, hi in ((0, 3), (3, 4), (4, T)):
        e, state, xd = bf.chunk(masks[..., lo:hi, :], obs[:, :, lo:hi], state, 1, with_observation=True)
        assert _bits(xd, X[:, :, lo:hi])
        parts.append(e)
    assert _bits(torch.cat(parts, dim=2), want) and isinstance(state, tuple) and len(state) == 2
    assert isinstance(state[0], hip_ops.OnlineWPEState) and torch.equal(state[1], psd)
    plain = enhancer.OnlineMVDR(forgetting=0.95, diag_load=1e-3)
    e, s = plain.chunk(masks, obs, None, 1)
    assert isinstance(s, torch.Tensor) and _bits(e, hip_ops.online_mvdr(masks, obs, None, 1, forgetting=0.95, diag_load=1e-3)[0])


def test_online_separator_with_the_pair():
    """Pushes of 2, 5 and 1 hops and a ragged flush, as tests/test_gpu_online_mvdr.py compares its stream: from the masks
    the stream formed, the audio is fe.istft(enhancer(masks, whole-utterance STFT)) bit for bit, and the recorded
    dereverberated frames are OnlineWPE's on the whole STFT."""
    from tssep_amd.train import enhancer
    ref = 1
    wpe = enhancer.OnlineWPE(taps=4, delay=2, forgetting=0.98, load=0.5, power_context=1)
    model = M._model(enhancer.OnlineMVDR(pre_wpe=wpe))
    fe = model.fe
    x, aux = M._signal()
    sep = model.online(aux, record=True, reference_channel=ref)
    y = M._push_all(sep, x, (2, 5, 1))
    assert tuple(y.shape) == (M.SB, M.SK, M.SN) and bool(torch.isfinite(y).all()) and sep.frames == fe.frames(M.SN)
    X = fe.stft(x)
    assert _bits(torch.cat([r["Observation"] for r in sep.record], dim=-2), X)
    masks = torch.cat([r["mask"] for r in sep.record], dim=-2)
    with torch.no_grad():
        enh = model.enhancer(masks, {"Observation": X, "reference_channel": ref}, model)
        want = fe.istft(enh, num_samples=M.SN)
    assert _bits(torch.cat([r["Estimate"] for r in sep.record], dim=-2), enh)
    assert torch.equal(y, want)
    der = torch.cat([r["Dereverberated"] for r in sep.record], dim=-2)
    assert _bits(der, wpe.chunk(X)[0]) and not _bits(der, X.to(torch.complex128))
    assert isinstance(sep._psd, tuple) and int(sep._psd[0].info.sum()) == 0
    # without pre_wpe the record and the state are what they were
    plain = M._model(enhancer.OnlineMVDR()).online(aux, record=True, reference_channel=ref)
    plain.push(x[..., :512])
    assert set(plain.record[0]) == {"Observation", "Input", "logit", "mask", "Estimate"} and isinstance(plain._psd, torch.Tensor)
