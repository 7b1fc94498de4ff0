"""Training on a stream without a GPU: the float64 adjoint of the chunked overlap-add with carry against
float64 autograd of the chunked forward, against the whole-utterance adjoint (carry handed on) and against the zeroed-dy
statement (NULL carry); the checker of tests/test_gpu_stream_grad_kernels.py on the defects it has to reject, at that
file's shapes; the ABI (declared, exported, wrapped, in the kernel plan, the guards that return before any launch) and
the refusals of Model.online(grad=True)."""
import ctypes
import inspect

import pytest
import torch

import stream_grad_reference as SG

SHIFT, PEND, F = SG.SHIFT, SG.PEND, SG.F
NAMES = ("tssep_istft_stream_bwd", "tssep_mask_istft_stream_bwd")


def same(a, b):
    """Equal up to the rounding of a float64 FFT (the library's batched transform is not bit-reproducible across batch
    sizes; the GPU file asserts the kernels' bits)."""
    return float((a - b).abs().max()) <= 1e-13 * max(float(b.abs().max()), 1e-300)


def rand(*shape, seed=0, dtype=torch.float64):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=dtype)


# ---- one call against autograd -------------------------------------------------------------------------------------------
CALLS = [(7, 3, None), (1, 3, None), (2, 1, None), (1, 0, None), (4, 0, 3 * 256 + 37), (6, 0, 5 * 256 + 1), (5, 2, 2 * 256 + 255),
         (3, 3, None)]       # (Tc, skip, N of a final call)


@pytest.mark.parametrize("form", ["plain", "gated", "X"])
@pytest.mark.parametrize("Tc,skip,N", CALLS)
def test_adjoint_is_autograd_of_the_chunked_forward(form, Tc, skip, N):
    B, K = 2, 2
    rows = B * K
    logit, obs = SG.inputs(B, K, Tc, form == "gated", seed=Tc * 7 + skip)
    logit, obs = logit.double().requires_grad_(True), obs.to(torch.complex128)
    X = (rand(rows, Tc, F, seed=5) + 1j * rand(rows, Tc, F, seed=6)).requires_grad_(True)
    ola = rand(rows, PEND, seed=1).requires_grad_(True)
    y, ola_out = SG.tail_forward(logit, obs, ola, skip, N, X=X if form == "X" else None)
    n = y.shape[1]
    assert n == (max(Tc - skip, 0) * SHIFT if N is None else N)
    dy, d_out = rand(rows, n, seed=2), rand(rows, PEND, seed=3)
    leaf = X if form == "X" else logit
    want, want_ola = torch.autograd.grad([y, ola_out], [leaf, ola], [dy, d_out], retain_graph=True)
    got, got_ola = SG.tail_backward(dy if n else None, d_out, Tc, skip, n, None if form == "X" else logit.detach(), obs, rows)
    assert torch.equal(got_ola, want_ola)                                # (a copy: exact)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-12 * scale
    # a carry nobody differentiates is a zero carry
    want0, = torch.autograd.grad([y], [leaf], [dy]) if n else (torch.zeros_like(want),)
    got0, _ = SG.tail_backward(dy if n else None, None, Tc, skip, n, None if form == "X" else logit.detach(), obs, rows)
    assert float((got0 - want0).abs().max()) <= 1e-12 * max(scale, 1e-300)


# ---- the two statements the GPU file asserts bit for bit --------------------------------------------------------------------
def _utterance(hops, rest, B, K, gated, seed):
    N = hops * SHIFT + rest
    T = -(-N // SHIFT) + 3
    logit, obs = SG.inputs(B, K, T, gated, seed)
    dy = rand(B * K, N, seed=seed + 1)
    return N, T, logit.double(), obs.to(torch.complex128), dy


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("hops,pushes,rest", SG.cases())
def test_chunks_with_the_carry_handed_on_are_the_whole_utterance(hops, pushes, rest, gated):
    N, T, logit, obs, dy = _utterance(hops, rest, 1, 3, gated, seed=hops + rest)
    steps = SG.steps_of(pushes, N)
    assert sum(s.frames for s in steps) == T
    got, carries = SG.stream_backward(dy, steps, logit, obs)
    assert same(got, SG.whole_backward(dy, T, logit, obs))                 # the same 1024 values per frame
    assert not bool(carries[0].any())                                       # in front of the stream: the leading fade
    gX, _ = SG.stream_backward(dy, steps, rows=3)
    assert same(gX, SG.whole_backward(dy, T))


@pytest.mark.parametrize("hops,pushes,rest", SG.cases())
def test_null_carry_is_a_zeroed_dy(hops, pushes, rest):
    N, T, logit, obs, dy = _utterance(hops, rest, 2, 1, False, seed=hops + rest + 50)
    steps = SG.steps_of(pushes, N)
    got, _ = SG.stream_backward(dy, steps, logit, obs, carry=False)
    t, n = 0, 0
    for st in steps:
        n += st.samples
        cut = dy.clone()
        cut[:, n:] = 0                                                     # behind the chunk's last completed sample
        want = SG.whole_backward(cut, T, logit, obs)[:, :, t:t + st.frames]
        assert same(got[:, :, t:t + st.frames], want), (st, t)
        t += st.frames
    assert not same(got, SG.whole_backward(dy, T, logit, obs))              # (truncation is visible: every stream has two calls)


# ---- the checker and the defects it has to reject ----------------------------------------------------------------------------
def _checked_stream(hops, pushes, rest, B, K, gated, defect, cast=torch.float32):
    """A candidate (the float64 adjoint with `defect`, rounded to float32) through the checker, call by call, with the
    CORRECT carry gradients as inputs -> (calls that passed, calls it rejected)."""
    N, T, logit, obs, dy = _utterance(hops, rest, B, K, gated, seed=3 * hops + rest)
    logit32, obs32, dy32 = logit.float(), obs.to(torch.complex64), dy.float()
    steps = SG.steps_of(pushes, N)
    d_ola, t_hi, n_hi, ok, bad = None, T, N, 0, 0
    for st in reversed(steps):
        t_lo, n_lo = t_hi - st.frames, n_hi - st.samples
        lg, ob = logit32[:, :, t_lo:t_hi], obs32[:, t_lo:t_hi]
        dyc = dy32[:, n_lo:n_hi] if st.samples else None
        d, d_in = SG.tail_backward(dyc, d_ola, st.frames, st.skip, st.samples, lg, ob, defect=defect)
        try:
            SG.check_call(d.to(cast), d_in.to(cast), dyc, d_ola, st.frames, st.skip, st.samples, lg, ob, what=str(st))
            ok += 1
        except AssertionError:
            bad += 1
        d_ola = SG.tail_backward(dyc, d_ola, st.frames, st.skip, st.samples, lg, ob)[1].float()
        t_hi, n_hi = t_lo, n_lo
    return ok, bad


@pytest.mark.parametrize("B,K", SG.ROWS)
def test_checker_accepts_the_rounded_adjoint(B, K):
    for gated in (False, True):
        for hops, pushes, rest in SG.cases():
            ok, bad = _checked_stream(hops, pushes, rest, B, K, gated, None)
            assert bad == 0 and ok == len(pushes) + 1, (hops, pushes, rest, gated)


@pytest.mark.parametrize("defect", SG.DEFECTS)
def test_checker_rejects_planted_defects(defect):
    """Each defect is caught at the GPU file's shapes -- in every (B, K), and in every stream where it can show at all:
    carry_late and ola_from_dy need a call with a carry behind it (more than one call; ola_from_dy a call of Tc < 3 that
    is not the last), skip_kept a completed hop in the first call... so the count is asserted per defect, not per case."""
    gated = defect == "gate_missing"
    for B, K in SG.ROWS:
        caught = []
        for hops, pushes, rest in SG.cases():
            _, bad = _checked_stream(hops, pushes, rest, B, K, gated, defect)
            if bad:
                caught.append((hops, pushes, rest))
        assert caught, (defect, B, K)
        if defect == "gate_missing":
            assert len(caught) == len(SG.cases())
        if defect == "beyond_N":                       # every ragged rest shows it, a whole last hop cannot
            assert {c[2] for c in caught} == {1, 37, 255}
        if defect == "ola_from_dy":                    # the streams with a push of fewer than three frames
            assert {(1,) * 7, (2, 2, 7), (4, 1, 6)} <= {c[1] for c in caught} <= {(1,) * 7, (1, 6), (2, 2, 7), (4, 1, 6)}
        if defect == "carry_late":
            assert len(caught) == len(SG.cases())      # (the flush behind the pushes always carries)
        if defect == "skip_kept":                      # the streams whose first calls complete a hop behind skipped ones
            assert {(7,), (1, 6), (2, 2, 7), (4, 1, 6)} <= {c[1] for c in caught}


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("Tc,skip", [(1, 3), (1, 2), (2, 3)])
def test_checker_rejects_skip_over_carry_under_a_random_carry_gradient(Tc, skip, gated):
    """skip > Tc: the hops Tc .. skip - 1 of g are d_ola_out's.  A carry gradient chained from a later call is zero there,
    so the streams above cannot see a kernel that zeroes them; a random one does (the GPU file's single-call test)."""
    B, K = 2, 3
    logit, obs = SG.inputs(B, K, Tc, gated, seed=Tc + skip)
    d_out = rand(B * K, PEND, seed=4).float()
    n = max(Tc - skip, 0) * SHIFT
    assert n == 0
    good, good_in = SG.tail_backward(None, d_out, Tc, skip, 0, logit, obs)
    SG.check_call(good.float(), good_in.float(), None, d_out, Tc, skip, 0, logit, obs)
    bad, bad_in = SG.tail_backward(None, d_out, Tc, skip, 0, logit, obs, defect="skip_first")
    with pytest.raises(AssertionError, match="outside the tolerance"):
        SG.check_call(bad.float(), good_in.float(), None, d_out, Tc, skip, 0, logit, obs)
    with pytest.raises(AssertionError, match="d_ola_in"):
        SG.check_call(good.float(), bad_in.float(), None, d_out, Tc, skip, 0, logit, obs)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_wrapped_and_planned():
    from tssep_amd import _lib, functional, hip_ops
    from tssep_amd.train import feature_extractor, runtime
    protos = _lib.parse_header()
    assert len(protos["tssep_istft_stream_bwd"][1]) == 14 and len(protos["tssep_mask_istft_stream_bwd"][1]) == 18
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(dll, name), name
    assert "tssep_istft_stream_bwd" in inspect.getsource(hip_ops.istft_stream_bwd)
    src = inspect.getsource(hip_ops.mask_istft_stream_bwd)
    assert "tssep_mask_istft_stream_bwd" in src and '_timed("maskhead_stream_bwd"' in src and "TAIL_LOG" in src
    assert '_timed("maskhead_stream_bwd"' in inspect.getsource(hip_ops.istft_stream_bwd)
    plan = runtime.summarise_plan([], [], [dict(kernel="maskhead_stream_bwd", B=2, K=2, T=4)])
    assert plan["tail"][0]["kernel"] == "maskhead_stream_bwd"
    assert callable(functional.mask_istft_stream) and callable(functional.istft_stream)
    for fn in (feature_extractor.STFT.masked_istft_chunk, feature_extractor.STFT.istft_chunk):
        assert inspect.signature(fn).parameters["differentiable"].default is False


def test_guards_return_before_any_launch():
    """Plan, shape, overlap and alignment guards answer on the arguments alone: no device is needed (or touched)."""
    from tssep_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)
    base += (-base) % 64

    def p(off=0):
        return ctypes.c_void_p(base + off)

    def masked(dy=p(), dout=p(1024 * 4), size=1024, shift=256, B=1, K=1, Tc=4, skip=3, last=0, N=256, din=p(8192), lg=p(), ob=p()):
        return L.tssep_mask_istft_stream_bwd(dy, dout, lg, 0, ob, B, K, Tc, size, shift, p(), p(), skip, last, N, p(), din, None)

    def plain(dy=p(), dout=p(1024 * 4), size=1024, shift=256, rows=1, Tc=4, skip=3, last=0, N=256, din=p(8192), dX=p()):
        return L.tssep_istft_stream_bwd(dy, dout, rows, Tc, size, shift, p(), p(), skip, last, N, dX, din, None)

    OKAY, SHAPE, ALIGN, UNSUP, NULL = 0, -1, -2, -3, -5
    for f in (masked, plain):
        assert f(size=512, shift=128) == UNSUP and f(shift=512) == UNSUP
        assert f(N=255) == SHAPE and f(N=257) == SHAPE and f(last=1, N=0) == SHAPE and f(last=1, N=257) == SHAPE
        assert f(skip=4) == SHAPE and f(skip=-1) == SHAPE and f(Tc=0) == SHAPE and f(Tc=(1 << 20) + 1, N=0) == SHAPE
        assert f(Tc=2, skip=3, N=256) == SHAPE                     # (a call of two frames behind skip = 3 completes nothing)
        assert f(din=p(1024 * 4)) == SHAPE and f(din=p(1024 * 4 + 3068)) == SHAPE and f(dout=p(8192 - 3068)) == SHAPE
        assert f(dy=None) == NULL
        assert f(dout=p(1024 * 4 + 4)) == ALIGN and f(dy=p(2)) == ALIGN and f(din=p(8192 + 2)) == ALIGN
    assert masked(B=0) == SHAPE and masked(K=0) == SHAPE and plain(rows=0) == SHAPE
    assert masked(lg=None) == NULL and masked(ob=None) == NULL and plain(dX=None) == NULL
    assert masked(ob=p(4)) == ALIGN and plain(dX=p(4)) == ALIGN


# ---- Model.online(grad=True) -----------------------------------------------------------------------------------------------
def _model(enh):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import feature_extractor as fe, loss, model, net
    f = fe.ConcaternatedSTFTFeatures(
        fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True), size=1024, shift=256, window="hann")
    me = net.MaskEstimator_v2(combination="mul", ts_vad=3, rnn_typ="lstm", random_speaker_order=False, idim=553, odim=513,
                              units=8, projs=12, layers=3)
    return model.Model(fe=f, reader=DummyReader(), mask_estimator=me, enhancer=enh, loss=loss.LogMAE())


def test_model_online_grad_refusals():
    from tssep_amd.train import enhancer, online
    aux = torch.zeros(2, 3, 513)
    with pytest.raises(NotImplementedError, match="grad=True.*OnlineMVDR.*evaluation-time"):
        _model(enhancer.OnlineMVDR()).online(aux, grad=True)
    with pytest.raises(NotImplementedError, match="only Masking has a streaming tail"):
        _model(enhancer.TorchBF()).online(aux, grad=True)
    sep = _model(enhancer.Masking()).online(aux, grad=True, detach=False)
    assert isinstance(sep, online.OnlineSeparator) and sep.grad and not sep.detach
    sep = _model(enhancer.Masking()).online(aux)
    assert not sep.grad and sep.detach                                   # the inference path, as it was
    assert isinstance(_model(enhancer.OnlineMVDR()).online(aux), online.OnlineSeparator)
    with pytest.raises(ValueError, match="pushed hops"):
        online.stream_loss_step(_model(enhancer.Masking()), torch.zeros(2, 1000), torch.zeros(2, 3, 1000), aux,
                                lambda y, t: (y - t).abs().mean((1, 2)), pushes=(1,))
