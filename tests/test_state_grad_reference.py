"""tests/state_grad_reference.py on the CPU (no GPU): the float64 loops with a state on both sides equal torch.nn.LSTM /
torch.nn.GRU under autograd; a sequence run as chunks with the state kept in the graph has the whole sequence's gradient,
and with the state detached it has not (by at least 100 x the bound the GPU layer test applies, at that test's own case);
the fp32 loops pass the per-element bounds and the same loops with a defect planted fail them, at the shapes of
tests/test_gpu_state_grad_kernels.py; and the host side of the feature -- the two entry points in the header, in the built
library and behind hip_ops, the new keywords, and every refusal that held without them."""
import inspect

import pytest
import torch

import gru_reference as G
import state_grad_reference as S
from test_causal_reference import lstm1_loop
from test_rnnp_layer_reference import bounds, errors, failures, report

F64, F32 = torch.float64, torch.float32
case = S.make_case


def close(a, b, tol=1e-11):
    e = errors(a, b)
    return e[0] <= tol, e


# ---- the loops are the layer torch differentiates ----------------------------------------------------------------------------
@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dims,combine", [((3, 5, 7, 5, 6), 0), ((4, 3, 8, 4, 8), 2), ((1, 1, 7, 5, 6), 0), ((9, 7, 8, 12, 8), 0)])
def test_loops_equal_torch_autograd_with_a_state_in_the_loss(dims, combine, act, gru):
    N, T = dims[:2]
    x, params, dy, dlast, state = case(*dims, gru, 0, combine)
    got = S.layer(x, params, dy, dlast, state, N, T, F64, gru, act, combine)
    ref = S.torch_layer(x, params, dy, dlast, state, N, T, F64, gru, act, combine)
    assert set(got) == set(ref) and ("c0" in got) == (not gru)
    for k in ref:
        ok, e = close(got[k], ref[k])
        assert ok, (k, e)
    # and a state of None is the zero state
    zero = tuple(torch.zeros_like(s) for s in state)
    a, b = S.layer(x, params, dy, dlast, None, N, T, F64, gru, act, combine), S.layer(x, params, dy, dlast, zero, N, T, F64, gru, act, combine)
    assert all(torch.equal(a[k], b[k]) for k in a)


CHUNKINGS = S.CHUNKINGS


@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("chunks", CHUNKINGS, ids=lambda c: "-".join(map(str, c[:3])))
def test_chunks_with_an_undetached_state_have_the_whole_gradient(chunks, gru):
    N, T, I, H, hdim = 3, 23, 7, 5, 6
    x, params, dy, dlast, state = case(N, T, I, H, hdim, gru, 1)
    whole = S.torch_layer(x, params, dy, dlast, state, N, T, F64, gru, 1)
    for fn in (S.layer, S.torch_layer):
        got = fn(x, params, dy, dlast, state, N, T, F64, gru, 1, chunks=chunks)
        for k in whole:
            ok, e = close(got[k], whole[k])
            assert ok, (fn.__name__, k, e)


@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
def test_detached_chunks_are_the_truncated_gradient_of_autograd(gru):
    N, T, I, H, hdim = 3, 23, 7, 5, 6
    x, params, dy, dlast, state = case(N, T, I, H, hdim, gru, 1)
    got = S.layer(x, params, dy, dlast, state, N, T, F64, gru, 1, chunks=[5, 1, 17], detach=True)
    ref = S.torch_layer(x, params, dy, dlast, state, N, T, F64, gru, 1, chunks=[5, 1, 17], detach=True)
    for k in ref:
        ok, e = close(got[k], ref[k])
        assert ok, (k, e)


@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("name", list(S.CHUNK_CASES))
def test_truncation_is_far_outside_the_bound_of_the_gpu_test(name, gru):
    """At the cases tests/test_gpu_state_grad_layer.py runs as chunks, dW_hh (and dW_ih, dx) of the detached run differ
    from the full one by at least 100 x that test's bound under fp32 GEMMs -- measured: more than 20000 x --, so an
    implementation that ignores `detach`, either way, cannot pass.  Under split-bf16 GEMMs the bound is 770.6 times wider,
    8 x 770.6 x 5e-7 = 3e-3 of the tensor at 300 units, and no factor on W_hh moves the truncated gradient 100 x that far
    from the full one (state_grad_reference.WHH_SCALE_WIDE lists what was measured: 101 at best, where the figure depends
    on the host's fp32 summation order): there the distance is asserted at 25 x the bound, measured 82 - 309."""
    full, trunc = S.chunk_reference(name, gru)[-1], S.chunk_reference(name, gru, detach=True)[-1]
    for k in ("w_hh", "w_ih", "x"):
        e = errors(trunc[F64][k], full[F64][k])[0]
        for split, factor in ((False, 100.0), (True, 25.0)):
            b = max(bounds(full[F32][k], full[F64][k], split)[0], bounds(trunc[F32][k], trunc[F64][k], split)[0])
            print(name, "gru" if gru else "lstm", k, "split" if split else "fp32", "truncated against full", e, "bound", b, "ratio", e / b)
            assert e >= factor * b, (k, split, e, b)


# ---- the per-element bounds: the fp32 loops pass, planted defects fail --------------------------------------------------------
KERNEL_SHAPES = [(1, 1, 5), (8, 2, 64), (9, 7, 65), (9, 7, 300), (8, 1, 300), (1, 2, 65)]      # of the GPU kernel file


def kernel_case(N, T, H, gru, seed=0):
    """saved activations of a float64 forward from a nonzero state, and the backward's inputs: fp32 values"""
    gen = torch.Generator().manual_seed(6000 + seed)
    whh = (G.make_gru_whh(H, 1, gen, "cpu") if gru else [(torch.rand(4 * H, H, generator=gen) * 2 - 1) * H ** -0.5])[0]
    gin = torch.randn(N, T, H, 4, generator=gen)
    h0, c0 = torch.rand(N, H, generator=gen) * 2 - 1, torch.randn(N, H, generator=gen)
    dh, dhT, dcT = (torch.randn(*s, generator=gen) for s in ((N, T, H), (N, H), (N, H)))
    if gru:
        A, h = G.gru_forward_loop(gin.unsqueeze(2), [whh], H, F64, h0=h0)
        return dict(whh=whh, A=A[:, :, 0].float(), h=h[:, :, 0].float(), h0=h0, dh=dh, dhT=dhT)
    A, c, _, _ = lstm1_loop(gin, whh, H, F64, (h0, c0))
    return dict(whh=whh, A=A.float(), c=c.float(), c0=c0, dh=dh, dhT=dhT, dcT=dcT)


def run_lstm(k, H, dtype, defect=None):
    D, dh0, dc0 = S.lstm1_backward_loop(k["A"], k["c"], k["dh"], k["whh"], H, dtype, k["c0"], k["dhT"], k["dcT"], defect)
    return S.check_lstm1_backward(k["A"], k["c"], k["dh"], D, k["whh"], H, k["c0"], k["dhT"], k["dcT"], dh0, dc0)


def run_gru(k, H, dtype, defect=None):
    Dg, dh0 = S.gru1_backward_loop(k["A"], k["h"], k["dh"], k["whh"], H, dtype, k["h0"], k["dhT"], defect)
    return S.check_gru1_backward(k["A"], k["h"], k["dh"], Dg, k["whh"], H, k["h0"], k["dhT"], dh0)


@pytest.mark.parametrize("N,T,H", KERNEL_SHAPES)
def test_fp32_loops_pass_the_bounds_and_float64_loops_by_far(N, T, H):
    for gru, run in ((False, run_lstm), (True, run_gru)):
        k = kernel_case(N, T, H, gru)
        w32, w64 = run(k, H, F32), run(k, H, F64)
        print("gru" if gru else "lstm", (N, T, H), "fp32:", w32, "float64:", w64)
        assert w32.ok() and w32.count == N * T * H * 4, str(w32)
        assert set(w32.ratio) == ({"dgates", "dh0"} if gru else {"dgates", "dh0", "dc0"})
        assert all(v < 1e-3 for v in w64.ratio.values()), str(w64)
        assert w32.median("dgates") < 1e-4 and w32.median("dh0") < 1e-4


@pytest.mark.parametrize("N,T,H", KERNEL_SHAPES)
@pytest.mark.parametrize("defect", S.LSTM_DEFECTS)
def test_planted_lstm_defects_fail_the_bounds(defect, N, T, H):
    w = run_lstm(kernel_case(N, T, H, False), H, F32, defect)
    print(defect, (N, T, H), w, w.outside)
    assert not w.ok(), str(w)
    if defect == "dc0_before_f":
        assert w.ratio["dc0"] > 1 and w.ratio["dgates"] <= 1 and w.ratio["dh0"] <= 1


@pytest.mark.parametrize("N,T,H", KERNEL_SHAPES)
@pytest.mark.parametrize("defect", S.GRU_DEFECTS)
def test_planted_gru_defects_fail_the_bounds(defect, N, T, H):
    w = run_gru(kernel_case(N, T, H, True), H, F32, defect)
    print(defect, (N, T, H), w, w.outside)
    assert not w.ok(), str(w)
    if defect == "dh0_without_carry":
        assert w.ratio["dh0"] > 1 and w.ratio["dgates"] <= 1


@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("shape", S.LAYER_CASES, ids=lambda s: "x".join(map(str, s)))
def test_the_missing_h0_term_of_dwhh_fails_the_layer_measure(shape, gru):
    """under both GEMM arithmetics' bounds, and nothing but dW_hh moves"""
    N, T, I, H, hdim, combine = shape
    x, params, dy, dlast, state, ref = S.layer_reference(shape, gru, 1)
    with torch.no_grad():
        bad = S.layer(x, params, dy, dlast, state, N, T, F32, gru, 1, combine, defect="dwhh_h0_missing")
    for split in (False, True):
        assert failures(report(bad, ref[F64], ref[F32], split)) == ["w_hh"], split
        assert failures(report(ref[F32], ref[F64], ref[F32], split)) == []


# ---- the host side -----------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_wrapped():
    from tssep_amd import _lib, hip_ops as h
    protos = _lib.parse_header()
    assert len(protos["tssep_lstm1_bwd_state"][1]) == 14 and len(protos["tssep_gru1_bwd_state"][1]) == 12
    assert len(protos["tssep_lstm1_bwd"][1]) == 9 and len(protos["tssep_gru1_bwd"][1]) == 9, "the old entry points stay"
    L = _lib.lib()
    assert hasattr(L, "tssep_lstm1_bwd_state") and hasattr(L, "tssep_gru1_bwd_state") and L.tssep_abi_version() == 4
    for fn, names in ((h.lstm1_bwd, ("c0", "dhT", "dcT", "dh0", "dc0")), (h.gru1_bwd, ("h0", "dhT", "dh0")),
                      (h.gru_bwd, ("h0", "dhT", "dh0"))):
        sig = inspect.signature(fn).parameters
        assert all(sig[n].default is None for n in names), (fn.__name__, list(sig))
    assert "state" in inspect.signature(h.recurrence_launch).parameters
    # a null pointer where the guards look first: declined on the host, nothing is launched (no GPU here)
    assert L.tssep_lstm1_bwd_state(None, None, None, 8, None, None, None, None, None, None, 2, 3, 5, None) == -5
    assert L.tssep_gru1_bwd_state(None, None, None, 8, None, None, None, None, 2, 3, 5, None) == -5


def test_the_new_keywords_exist_and_default_to_off():
    from tssep_amd import functional as Fn
    from tssep_amd.train.net import MaskEstimator_v2
    from tssep_amd.train.rnnp import RNNP_packed
    assert inspect.signature(Fn.rnnp_layer).parameters["state_grad"].default is False
    assert inspect.signature(RNNP_packed.forward).parameters["state_grad"].default is False
    assert inspect.signature(RNNP_packed.forward_rows).parameters["state_grad"].default is False
    sig = inspect.signature(MaskEstimator_v2.train_chunk).parameters
    assert list(sig) == ["self", "xs", "aux", "state", "detach"] and sig["state"].default is None and sig["detach"].default is True
    assert list(inspect.signature(RNNP_packed.__init__).parameters) == ["self", "idim", "elayers", "cdim", "hdim", "dropout", "typ",
                                                                        "return_states"]


def test_refusals_hold_without_the_keyword_and_for_two_directions():
    """CPU tensors: every refusal is raised on the arguments alone"""
    from tssep_amd import functional as Fn
    from tssep_amd.train.net import InstanceNorm, MaskEstimator_v2
    from tssep_amd.train.rnnp import RNNP_packed
    x, state = torch.zeros(6, 7), (torch.zeros(2, 5), torch.zeros(2, 5))
    lstm, gru = torch.nn.LSTM(7, 5, batch_first=True), torch.nn.GRU(7, 5, batch_first=True)
    lin = torch.nn.Linear(5, 6)
    for kw in ({}, dict(state_grad=False)):
        with pytest.raises(RuntimeError, match="without gradients"):
            Fn.rnnp_layer(x, lstm, lin, 2, 3, state=state, **kw)
        with pytest.raises(RuntimeError, match="without gradients"):
            Fn.rnnp_layer(x, gru, lin, 2, 3, state=state[0], **kw)
    for two in (torch.nn.LSTM(7, 5, bidirectional=True, batch_first=True), torch.nn.GRU(7, 5, bidirectional=True, batch_first=True)):
        for kw in (dict(state_grad=True), dict(state=state, state_grad=True), dict(return_state=True, state_grad=True)):
            with pytest.raises(NotImplementedError, match="bidirectional"):
                Fn.rnnp_layer(x, two, torch.nn.Linear(10, 6), 2, 3, **kw)
    with pytest.raises(ValueError, match="h0"):
        Fn.rnnp_layer(x, gru, lin, 2, 3, state=state, state_grad=True)
    with pytest.raises(ValueError, match="h0, c0"):
        Fn.rnnp_layer(x, lstm, lin, 2, 3, state=state[:1], state_grad=True)
    m = RNNP_packed(7, 2, 5, 6, 0, typ="lstm", return_states=True)
    xs, st = torch.zeros(2, 3, 7), [(torch.zeros(1, 2, 5), torch.zeros(1, 2, 5))] * 2
    with pytest.raises(RuntimeError, match="without gradients"):
        m(xs, prev_state=st)
    with pytest.raises(ValueError, match="one .h, c. per layer"):
        m(xs, prev_state=st[:1], state_grad=True)
    with pytest.raises(ValueError, match="return_states"):
        RNNP_packed(7, 2, 5, 6, 0, typ="lstm")(xs, prev_state=st, state_grad=True)
    with pytest.raises(NotImplementedError, match="typ='lstm'"):
        RNNP_packed(7, 2, 5, 6, 0).forward_rows(torch.zeros(6, 7), 2, 3, states=[], state_grad=True)
    base = dict(idim=8, layers=2, units=5, projs=12, combination="mul")
    xe, aux = torch.zeros(2, 3, 8), torch.zeros(2, 4, 8)
    for detach in (True, False):
        with pytest.raises(ValueError, match="reads the future"):
            MaskEstimator_v2(**base).train_chunk(xe, aux, detach=detach)
        with pytest.raises(NotImplementedError, match="span the utterance"):
            MaskEstimator_v2(rnn_typ="lstm", input_normalizer=InstanceNorm(), **base).train_chunk(xe, aux, detach=detach)
        me = MaskEstimator_v2(rnn_typ="lstm", **base)
        with pytest.raises(NotImplementedError, match="frame-wise"):
            me.train_chunk(xe, torch.zeros(2, 4, 3, 8), detach=detach)
        with pytest.raises(ValueError, match="Tc >= 1"):
            me.train_chunk(torch.zeros(2, 0, 8), aux, detach=detach)
        with pytest.raises(TypeError):
            me.train_chunk(xe, aux, state=object(), detach=detach)
    with pytest.raises(ValueError, match="rnn_typ"):
        MaskEstimator_v2(rnn_typ="gru", **base)
