"""functional.rnnp_layer on ONE-direction containers (typ='lstm': functional._RNNP over one direction of time) on a real MI355X
against the float64 restatement of tests/test_causal_reference.py -- the two-direction restatement with the reverse half of
the projection zeroed.  Measure and bound are tests/test_rnnp_layer_reference.py's (`assert_within`): per tensor the
normwise and the element-wise error against float64, each within MARGIN x the same figure of the fp32 restatement of the
same case under GEMM_PRECISION = "f32", and that x C_SPLIT / U under "bf16x3".  The recurrence is the exact-fp32 streaming
kernel under both.  Every case has a fixed seed; NaN or Inf anywhere fails.  The carried state (chunks of frames, each
started from the previous chunk's last frame, under no_grad) is held to the same float64 outputs under the same bounds."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_causal_reference import (CNAMES, LAYER_SHAPES, STATE_SHAPE, causal_layer, causal_module_params,  # noqa: E402
                                   causal_modules, causal_reference, causal_two_layers, chunked_forward, chunkings, make_causal_case,
                                   make_causal_params)
from test_rnnp_layer_reference import assert_within, bounds, combine_rows, errors, round_up  # noqa: E402
from tssep_amd import functional as Fn, hip_ops as H  # noqa: E402
from tssep_amd.distributed import GradBucket  # noqa: E402
from tssep_amd.train import runtime  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
RATIOS = {}          # (mode, tensor) -> the largest error / (the fp32 restatement's error) this run saw (test_zz_report)
TOY, TOY_COMBINED, ALIGN = LAYER_SHAPES[0], LAYER_SHAPES[1], LAYER_SHAPES[2]


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request):
    """both GEMM arithmetics, hence both values of fused_colsum(); restored afterwards"""
    with runtime.applied(gemm_precision=request.param):
        assert H.fused_colsum() == (request.param == "bf16x3")
        yield request.param


def is_split():
    return H.GEMM_PRECISION != "f32"


@contextlib.contextmanager
def logged():
    """-> dict(recurrence=[...], splits=[S of every wgrad], unpack=[accumulate of every lstm1_unpack], packs=[...],
    tanh=[one entry per stand-alone Tanh backward], two=[every call of a two-direction entry point])"""
    seen = dict(recurrence=[], splits=[], unpack=[], packs=[], tanh=[], two=[])
    wgrad, unpack, pack, tanh_bwd, unpack2, pack2 = H.wgrad, H.lstm1_unpack, H.lstm1_pack, H.tanh_bwd, H.lstm_unpack, H.lstm_pack

    def tanh_(*a, **k):
        seen["tanh"].append(1)
        return tanh_bwd(*a, **k)

    def wgrad_(*a, **k):
        part, S = wgrad(*a, **k)
        seen["splits"].append(S)
        return part, S

    def unpack_(*a, accumulate=False):
        seen["unpack"].append(bool(accumulate))
        return unpack(*a, accumulate=accumulate)

    def pack_(*a, **k):
        seen["packs"].append(1)
        return pack(*a, **k)

    def two_(*a, **k):
        seen["two"].append(1)
        raise AssertionError("a two-direction entry point on the causal route")

    old_log = H.RECURRENCE_LOG
    H.wgrad, H.lstm1_unpack, H.lstm1_pack, H.tanh_bwd, H.RECURRENCE_LOG = wgrad_, unpack_, pack_, tanh_, seen["recurrence"]
    H.lstm_unpack = H.lstm_pack = two_
    try:
        yield seen
    finally:
        H.wgrad, H.lstm1_unpack, H.lstm1_pack, H.tanh_bwd, H.RECURRENCE_LOG = wgrad, unpack, pack, tanh_bwd, old_log
        H.lstm_unpack, H.lstm_pack = unpack2, pack2


def collect(y, xg, lstm, lin):
    torch.cuda.synchronize()
    out = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in zip(CNAMES, causal_module_params(lstm, lin))}
    out["y"] = y.detach().cpu()
    out["x"] = xg.grad.detach().cpu() if xg is not None and xg.grad is not None else None
    return out


def run_layer(x, params, dy, N, T, act, combine, x_grad=True, passes=1, sinks=False, frozen=None, dy_dev=None):
    """-> (outputs on the host, the bucket or None).  sinks: a GradBucket owns the gradients before the first backward."""
    lstm, lin = causal_modules(params, device=DEV)
    assert not lstm.bidirectional
    if frozen:
        getattr(lstm, frozen).requires_grad_(False)
    bucket = GradBucket(causal_module_params(lstm, lin)) if sinks else None
    xg = x.to(DEV).clone().requires_grad_(x_grad)
    for _ in range(passes):
        y = Fn.rnnp_layer(xg, lstm, lin, N, T, act=act, combine=combine)
        y.backward(dy.to(DEV) if dy_dev is None else dy_dev)
    if bucket is not None:
        bucket.sync()            # the side stream's weight gradients, BEFORE anything reads the bucket
    return collect(y, xg, lstm, lin), bucket


def note(mode_, rep):
    for k, v in rep.items():
        key = (mode_, k.split(".")[-1])
        RATIOS[key] = max(RATIOS.get(key, 0.0), v["ratio"])


def ident(s):
    return "x".join(map(str, s))


# ---- the layer against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=ident)
def test_layer_matches_float64(shape, act, mode):
    N, T, I, Hh, hdim, combine = shape
    x, params, dy, ref = causal_reference(shape, 0, act)
    with logged() as seen:
        got, _ = run_layer(x, params, dy, N, T, act, combine)
    assert [(e["kernel"], e["direction"], e["sequences"], e["frames"], e["units"]) for e in seen["recurrence"]] == \
        [("stream1_f32", "fwd", N, T, Hh), ("stream1_f32", "bwd", N, T, Hh)], seen["recurrence"]
    # three weight-gradient GEMMs (projection, dW_hh, dW_ih + bias), three unpacks through autograd, ONE pack
    assert len(seen["splits"]) == 3 and seen["unpack"] == [False] * 3 and len(seen["packs"]) == 1, seen
    assert got["y"].shape == ref[F64]["y"].shape
    print(ident(shape), "splits", seen["splits"], "split-bf16" if is_split() else "fp32")
    note(mode, assert_within(got, ref[F64], ref[F32], is_split(), what=f"{ident(shape)} act={act} {mode}"))


# ---- the three ways a gradient leaves the layer ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [TOY, TOY_COMBINED, ALIGN, LAYER_SHAPES[3]], ids=ident)
def test_sinks_accumulate_twice_the_autograd_gradient(shape, mode):
    """GradBucket sinks on the side stream (`direct`): two backward passes leave exactly 2 x the float64 gradient, within
    the bound scaled by 2.  Hp != Hh: the projection gradient is cut to [hdim, Hh] and added; Hp == Hh: the emitter writes
    the sinks itself (reduce_splits_bias under fused_colsum)."""
    N, T, I, Hh, hdim, combine = shape
    x, params, dy, ref = causal_reference(shape, 0, 1)
    assert H.OVERLAP_WGRAD
    calls = dict(bias=0)
    rsb = H.reduce_splits_bias
    H.reduce_splits_bias = lambda *a, **k: (calls.__setitem__("bias", calls["bias"] + 1), rsb(*a, **k))[1]
    try:
        with logged() as seen:
            got, bucket = run_layer(x, params, dy, N, T, 1, combine, passes=2, sinks=True)
    finally:
        H.reduce_splits_bias = rsb
    assert seen["unpack"] == [True] * 8, seen["unpack"]        # the direct path, both passes (four unpacks each)
    assert calls["bias"] == (2 if (round_up(Hh, 4) == Hh and H.fused_colsum()) else 0), calls
    what = f"{ident(shape)} sinks x2 {mode}"
    note(mode, assert_within(got, ref[F64], ref[F32], is_split(), names=[*CNAMES, "x"], scale=2.0, what=what))
    note(mode, assert_within(got, ref[F64], ref[F32], is_split(), names=["y"], what=what))
    plain, _ = run_layer(x, params, dy, N, T, 1, combine)
    for k in CNAMES:      # sink against autograd return, directly: 2 x, within the two results' bounds together
        b = bounds(ref[F32][k], ref[F64][k], is_split())
        e = errors(got[k], 2 * plain[k].double())
        assert e[0] <= 2 * b[0] and e[1] <= 2 * b[1], (k, e, b)


def test_frozen_parameter_falls_back_to_autograd_returns(mode):
    N, T, I, Hh, hdim, combine = TOY
    x, params, dy, ref = causal_reference(TOY, 0, 1)
    with logged() as seen:
        got, bucket = run_layer(x, params, dy, N, T, 1, combine, sinks=True, frozen="bias_hh_l0")
    assert seen["unpack"] == [False] * 3, seen["unpack"]
    assert got["b_hh"] is None
    names = [k for k in CNAMES if k != "b_hh"]
    note(mode, assert_within(got, ref[F64], ref[F32], is_split(), names=["y", "x"] + names, what=f"frozen {mode}"))
    assert float(bucket.flat.abs().max()) > 0            # and they did arrive in the bucket


@pytest.mark.parametrize("shape", [TOY, TOY_COMBINED], ids=ident)
def test_input_without_gradient(shape, mode):
    N, T, I, Hh, hdim, combine = shape
    x, params, dy, ref = causal_reference(shape, 0, 1)
    got, _ = run_layer(x, params, dy, N, T, 1, combine, x_grad=False)
    assert got["x"] is None
    note(mode, assert_within(got, ref[F64], ref[F32], is_split(), names=["y", *CNAMES], what=f"{ident(shape)} no dx {mode}"))


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", [TOY, TOY_COMBINED], ids=ident)
def test_output_gradient_is_not_contiguous(shape, act, mode):
    N, T, I, Hh, hdim, combine = shape
    x, params, dy, ref = causal_reference(shape, 0, act)
    dyt = dy.to(DEV).t().contiguous().t()              # the same values, column-major
    assert not dyt.is_contiguous()
    got, _ = run_layer(x, params, dy, N, T, act, combine, dy_dev=dyt)
    note(mode, assert_within(got, ref[F64], ref[F32], is_split(), what=f"{ident(shape)} dy^T {mode}"))


# ---- two stacked layers: the Tanh backward folded into the consumer's d(input) GEMM -----------------------------------------
CHAINS = {"toy": (8, 5, 7, 5, 8), "w32": (32, 7, 321, 300, 320)}
_CHAIN = {}


def chain_reference(name, K):
    key = (name, K)
    if key not in _CHAIN:
        N, T, I, Hh, hdim = CHAINS[name]
        gen = torch.Generator().manual_seed(77)
        p0, p1 = make_causal_params(I, Hh, hdim, gen), make_causal_params((K or 1) * hdim, Hh, hdim, gen)
        x = torch.randn(N * T, I, generator=gen)
        dy = torch.randn(N // (K or 1) * T, hdim, generator=gen)
        _CHAIN[key] = (x, p0, p1, dy, {dt: causal_two_layers(x, p0, p1, dy, N, T, K, dt) for dt in (F64, F32)})
    return _CHAIN[key]


@pytest.mark.parametrize("name,K", [("toy", 0), ("toy", 4), ("w32", 0), ("w32", 4)])
def test_two_layers_with_the_tanh_fold(name, K, mode):
    """in_tanh = 1 / in_tanh = K behind a combined producer, against the float64 chain through tanh; then unfolded (the
    activation has retain_grad): both inside the bound AND within one bound of each other"""
    N, T, I, Hh, hdim = CHAINS[name]
    x, p0, p1, dy, ref = chain_reference(name, K)
    B = N // (K or 1)
    split = is_split()

    def run(retain):
        l0, q0 = causal_modules(p0, device=DEV)
        l1, q1 = causal_modules(p1, device=DEV)
        xg = x.to(DEV).clone().requires_grad_()
        h = Fn.rnnp_layer(xg, l0, q0, N, T, act=1, combine=K, dz_given=True)
        assert getattr(h, "_tssep_tanh_link", None) is not None
        if retain:
            h.retain_grad()
        y = Fn.rnnp_layer(h, l1, q1, B, T, in_tanh=(K or 1))
        y.backward(dy.to(DEV))
        out = {"1." + k: v for k, v in collect(y, None, l1, q1).items() if k in CNAMES}
        out.update({"0." + k: v for k, v in collect(y, xg, l0, q0).items() if k in CNAMES})
        out.update(y=y.detach().cpu(), x=xg.grad.cpu(), h=h.detach().cpu())
        if retain:
            out["dh"] = h.grad.cpu()
        return out

    with logged() as seen:
        folded = run(False)
    assert seen["tanh"] == [], "the fold was not taken"
    names = [k for k in ref[F64] if k != "dh"]
    note(mode, assert_within(folded, ref[F64], ref[F32], split, names=names, what=f"{name} K={K} folded {mode}"))
    with logged() as seen:
        plain = run(True)
    assert seen["tanh"] == [1], "a watched activation: the producer runs its own Tanh backward"
    note(mode, assert_within(plain, ref[F64], ref[F32], split, what=f"{name} K={K} unfolded {mode}"))
    for k in names:
        b = bounds(ref[F32][k], ref[F64][k], split)
        e = errors(folded[k], plain[k].double())
        print(f"{k}: folded against unfolded {e[0]:.3g} (<= {b[0]:.3g})")
        assert e[0] <= b[0] and e[1] <= b[1], (k, e, b)


# ---- an active dropout site behind the layer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [TOY, TOY_COMBINED, LAYER_SHAPES[3]], ids=ident)
def test_active_dropout_site(shape, mode):
    """y = keep ? tanh(z / (1 - p)) : 0 with the mask the host computes for the {seed, draw} the forward drew: the SAME mask
    in the backward (every gradient against the float64 layer fed dz = dy (1 - y^2) keep / (1 - p)), a fresh one next call"""
    import numpy as np
    N, T, I, Hh, hdim, combine = shape
    p = 0.3
    x, params, dy = make_causal_case(N, T, I, Hh, hdim, 9, combine)
    lstm, lin = causal_modules(params, device=DEV)
    used, draw = [], H.dropout_draw
    H.dropout_draw = lambda device=None: (used.append(draw(device)), used[-1])[1]
    try:
        xg = x.to(DEV).clone().requires_grad_()
        y = Fn.rnnp_layer(xg, lstm, lin, N, T, act=1, combine=combine, dropout_p=p)
        y.backward(dy.to(DEV))
        got = collect(y, xg, lstm, lin)
        with torch.no_grad():
            y2 = Fn.rnnp_layer(x.to(DEV), lstm, lin, N, T, act=1, combine=combine, dropout_p=p).cpu()
    finally:
        H.dropout_draw = draw
    assert len(used) == 2 and used[0].tolist() != used[1].tolist()
    seed, d = used[0].tolist()
    keep = torch.from_numpy(H.dropout_keep_host(seed, d, 0, N * T * hdim, p).astype(np.bool_)).view(N * T, hdim)   # logical rows (n, t)
    lay = (lambda t: combine_rows(t, N, T, combine)) if combine else (lambda t: t)
    ref = {}
    for dt in (F64, F32):
        z = causal_layer(x, params, dy, N, T, dt, 0, 0)["y"]                     # rows (n, t), no activation
        scale = keep.to(dt) / (1 - p)
        yr = torch.tanh(z * scale)
        dyr = dy.to(dt) if not combine else dy.to(dt).view(N // combine, T, combine, hdim).permute(0, 2, 1, 3).reshape(N * T, hdim)
        ref[dt] = causal_layer(x, params, dyr * (1 - yr * yr) * scale, N, T, dt, 0, 0)
        ref[dt]["y"] = lay(yr)
    note(mode, assert_within(got, ref[F64], ref[F32], is_split(), what=f"{ident(shape)} dropout {mode}"))
    dropped = lay(~keep)
    assert bool((got["y"][dropped] == 0).all()) and float(dropped.float().mean()) > 0.1
    assert not torch.equal(y2, got["y"]), "the next call drew the same mask"


# ---- the carried state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
def test_chunks_with_a_carried_state_match_float64(act, mode):
    N, T, I, Hh, hdim, combine = STATE_SHAPE
    x, params, dy, ref = causal_reference(STATE_SHAPE, 0, act)
    lstm, lin = causal_modules(params, device=DEV)
    x3 = x.to(DEV).view(N, T, I)
    with torch.no_grad():
        whole, last = Fn.rnnp_layer(x3.reshape(N * T, I), lstm, lin, N, T, act=act, return_state=True)
    final = {dt: dict(zip(("hT", "cT"), chunked_forward(x, params, N, T, [T], dt, act)[1])) for dt in (F64, F32)}
    note(mode, assert_within({"hT": last[0].cpu(), "cT": last[1].cpu()}, final[F64], final[F32], is_split(), what=f"final state {mode}"))
    for chunks in chunkings(T):
        state, ys, t0 = None, [], 0
        with logged() as seen, torch.no_grad():
            for n in chunks:
                y, state = Fn.rnnp_layer(x3[:, t0:t0 + n].reshape(N * n, I), lstm, lin, N, n, act=act, state=state, return_state=True)
                assert tuple(state[0].shape) == tuple(state[1].shape) == (N, Hh)
                ys.append(y.view(N, n, hdim))
                t0 += n
        assert [e["frames"] for e in seen["recurrence"]] == chunks and all(e["kernel"] == "stream1_f32" for e in seen["recurrence"])
        got = {"y": torch.cat(ys, 1).reshape(N * T, hdim).cpu()}
        note(mode, assert_within(got, ref[F64], ref[F32], is_split(), names=["y"], what=f"chunks {chunks[:3]}.. act={act} {mode}"))
        # the state after the last chunk is the whole sequence's last frame (the input GEMM of another row count may round
        # differently, so this is the measure again, not an equality: tests/test_gpu_causal_kernels.py has the equality)
        got = {"hT": state[0].cpu(), "cT": state[1].cpu()}
        note(mode, assert_within(got, final[F64], final[F32], is_split(), what=f"chunks {chunks[:3]}.. final state {mode}"))
    lstm2, lin2 = causal_modules(params, device=DEV)
    with pytest.raises(RuntimeError, match="without gradients"):
        Fn.rnnp_layer(x3.reshape(N * T, I), lstm2, lin2, N, T, state=last)


def test_final_state_under_autograd_carries_no_gradient(mode):
    N, T, I, Hh, hdim, combine = TOY
    x, params, dy, ref = causal_reference(TOY, 0, 1)
    lstm, lin = causal_modules(params, device=DEV)
    xg = x.to(DEV).clone().requires_grad_()
    y, (hT, cT) = Fn.rnnp_layer(xg, lstm, lin, N, T, act=1, return_state=True)
    assert y.requires_grad and not hT.requires_grad and not cT.requires_grad
    y.backward(dy.to(DEV))
    note(mode, assert_within(collect(y, xg, lstm, lin), ref[F64], ref[F32], is_split(), what=f"return_state {mode}"))


def test_rnnp_packed_states_round_trip(mode):
    """RNNP_packed(typ='lstm', return_states=True): (h, states) with one (h_n, c_n) [1, N, cdim] per layer, accepted back as
    prev_state.  The layers' numerics are held to float64 above; this is the plumbing: a state that is dropped, or handed
    to another layer, moves tanh-sized outputs by 0.01 - 0.1, so 1e-3 (far above any rounding of three toy layers in
    either arithmetic: split-bf16 products carry 2^-16) separates right from wrong."""
    from tssep_amd.train.rnnp import RNNP_packed
    torch.manual_seed(3)
    m = RNNP_packed(7, 3, 5, 8, 0.0, typ="lstm", return_states=True).to(DEV).eval()
    x = torch.randn(4, 9, 7, device=DEV)
    with torch.no_grad():
        y, states = m(x)
        assert y.shape == (4, 9, 8) and len(states) == 3 and all(tuple(s.shape) == (1, 4, 5) for hc in states for s in hc)
        ya, sa = m(x[:, :4])
        yb, sb = m(x[:, 4:], prev_state=sa)
    for (h1, c1), (h2, c2) in zip(states, sb):
        assert float((h1 - h2).abs().max()) <= 1e-3 and float((c1 - c2).abs().max()) <= 1e-3
    assert float((torch.cat([ya, yb], 1) - y).abs().max()) <= 1e-3
    with torch.no_grad():
        dropped = m(x[:, 4:])[0]
    assert float((dropped - y[:, 4:]).abs().max()) > 1e-2, "a dropped state must show"
    with pytest.raises(RuntimeError, match="without gradients"):
        m(x, prev_state=states)
    # against torch's own modules (the containers ARE torch.nn.LSTM / Linear)
    with torch.no_grad():
        h = x
        for layer in m.net:
            h = layer(h)[0] if isinstance(layer, torch.nn.LSTM) else layer(h)
    assert float((h - y).abs().max()) <= 1e-3


def test_zz_report():
    """the largest error / (the fp32 restatement's error) per tensor this run saw (pytest -rP)"""
    for (mode_, name), v in sorted(RATIOS.items()):
        print(f"{mode_:7s} {name:8s} {v:.3g}")
