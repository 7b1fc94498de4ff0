"""functional.rnnp_layer on torch.nn.GRU + Linear containers (one direction of time, and two) on a real
MI355X, in both GEMM arithmetics, against torch.nn.GRU + Linear (+ Tanh) in float64 on the CPU.  Shapes are
tests/test_causal_reference.py's LAYER_SHAPES (what tests/test_gpu_causal_layer.py runs for typ = 'lstm'); measure and
bound are tests/test_rnnp_layer_reference.py's (`errors` / `bounds` / `assert_within`), unchanged: per tensor the normwise and
the element-wise error against float64, each within MARGIN x the same figure of the fp32 restatement of the same case
(tests/gru_reference.py `layer`: the same formulas in torch fp32, pinned to torch.nn.GRU in tests/test_gru_reference.py)
under GEMM_PRECISION = "f32", and that x C_SPLIT / U under "bf16x3".  The recurrence is the exact-fp32 streaming kernel
under both.

Does the four-slot layout change a term of the bound?  No.  The input GEMM's zero slot is a row of zeros times x plus
b_hn: an exact value (0 + b_hn), no error term of its own; in d(input) the slot's column of wih_p^T is zero, so whatever
da_q holds contributes exact zeros.  The separate bias gradients are two column sums over the same partials (slots
(r, z, n) and (r, z, q)): each is the sum the LSTM's shared bias gradient is, over another column.  The bound formula
stays as that file has it.

Measured on an MI355X (pytest -rP, test_zz_report), the largest error / (the fp32 restatement's error) per tensor over the
file: under "f32" (allowed 8) y 5.1, x 3.2, dh 5.1, w_ih 3.2, w_hh 2.2, b_ih 4.4, b_hh 2.9, w_proj 3.4, b_proj 5.1, hT 0.87;
under "bf16x3" (allowed 8 x 770.6 = 6165) y 112, x 108, w_ih 115, w_hh 149, b_ih 177, b_hh 176, w_proj 167, b_proj 56, hT 14."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import gru_reference as G  # noqa: E402
from test_causal_reference import LAYER_SHAPES, STATE_SHAPE, chunkings  # noqa: E402
from test_rnnp_layer_reference import assert_within, bounds, combine_rows, errors  # noqa: E402
from tssep_amd import functional as Fn, hip_ops as H  # noqa: E402
from tssep_amd.distributed import GradBucket  # noqa: E402
from tssep_amd.train import runtime  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
RATIOS = {}          # (mode, D, tensor) -> the largest error / (the fp32 restatement's error) this run saw (test_zz_report)
TOY, TOY_COMBINED, ALIGN, WIDE, FULL = LAYER_SHAPES
_REF = {}


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request):
    """both GEMM arithmetics, hence both values of fused_colsum(); restored afterwards"""
    with runtime.applied(gemm_precision=request.param):
        assert H.fused_colsum() == (request.param == "bf16x3")
        yield request.param


def is_split():
    return H.GEMM_PRECISION != "f32"


def reference(shape, D, seed, act):
    """-> x, params, dy, {float64: torch.nn.GRU + Linear (+ Tanh) under autograd, float32: the restatement}; computed once"""
    key = (shape, D, seed, act)
    if key not in _REF:
        N, T, I, Hh, hdim, combine = shape
        x, params, dy = G.make_layer_case(N, T, I, Hh, hdim, D, seed, combine)
        with torch.no_grad():
            r32 = G.layer(x, params, dy, N, T, F32, act, combine)
        _REF[key] = (x, params, dy, {F64: G.torch_layer(x, params, dy, N, T, F64, act, combine), F32: r32})
    return _REF[key]


@contextlib.contextmanager
def logged():
    """-> dict(recurrence=[...], splits=[S of every wgrad], unpack=[(which, accumulate) of every gru_unpack], packs=[...],
    tanh=[one entry per stand-alone Tanh backward]); an LSTM pack or unpack on a GRU layer raises"""
    seen = dict(recurrence=[], splits=[], unpack=[], packs=[], tanh=[])
    keep = {n: getattr(H, n) for n in ("wgrad", "gru_unpack", "gru_pack", "tanh_bwd", "lstm_unpack", "lstm1_unpack",
                                       "lstm_pack", "lstm1_pack", "RECURRENCE_LOG")}

    def tanh_(*a, **k):
        seen["tanh"].append(1)
        return keep["tanh_bwd"](*a, **k)

    def wgrad_(*a, **k):
        part, S = keep["wgrad"](*a, **k)
        seen["splits"].append(S)
        return part, S

    def unpack_(src, ld, nsplit, stride, Hh, ncols, which, *dst, accumulate=False):
        seen["unpack"].append((which, bool(accumulate)))
        return keep["gru_unpack"](src, ld, nsplit, stride, Hh, ncols, which, *dst, accumulate=accumulate)

    def pack_(*a, **k):
        seen["packs"].append(1)
        return keep["gru_pack"](*a, **k)

    def lstm_(*a, **k):
        raise AssertionError("an LSTM entry point on a GRU layer")

    H.wgrad, H.gru_unpack, H.gru_pack, H.tanh_bwd, H.RECURRENCE_LOG = wgrad_, unpack_, pack_, tanh_, seen["recurrence"]
    H.lstm_unpack = H.lstm1_unpack = H.lstm_pack = H.lstm1_pack = lstm_
    try:
        yield seen
    finally:
        for n, v in keep.items():
            setattr(H, n, v)


def collect(y, xg, gru, lin):
    torch.cuda.synchronize()
    D = 2 if gru.bidirectional else 1
    out = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in zip(G.layer_names(D), G.module_params(gru, lin))}
    out["y"] = y.detach().cpu()
    out["x"] = xg.grad.detach().cpu() if xg is not None and xg.grad is not None else None
    return out


def run_layer(x, params, dy, N, T, act, combine, x_grad=True, passes=1, sinks=False, frozen=None):
    """-> (outputs on the host, the bucket or None).  sinks: a GradBucket owns the gradients before the first backward."""
    gru, lin = G.gru_modules(params, device=DEV)
    if frozen:
        getattr(gru, frozen).requires_grad_(False)
    bucket = GradBucket(G.module_params(gru, lin)) if sinks else None
    xg = x.to(DEV).clone().requires_grad_(x_grad)
    for _ in range(passes):
        y = Fn.rnnp_layer(xg, gru, lin, N, T, act=act, combine=combine)
        y.backward(dy.to(DEV))
    if bucket is not None:
        bucket.sync()            # the side stream's weight gradients, BEFORE anything reads the bucket
    return collect(y, xg, gru, lin), bucket


def note(mode_, D, rep):
    for k, v in rep.items():
        key = (mode_, D, k.split(".")[-1])
        RATIOS[key] = max(RATIOS.get(key, 0.0), v["ratio"])


def ident(s):
    return "x".join(map(str, s))


def kernel_of(D):
    return "stream1_gru_f32" if D == 1 else "stream_gru_f32"


# ---- the layer against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", LAYER_SHAPES, ids=ident)
def test_layer_matches_float64(shape, act, D, mode):
    N, T, I, Hh, hdim, combine = shape
    x, params, dy, ref = reference(shape, D, 0, act)
    with logged() as seen:
        got, _ = run_layer(x, params, dy, N, T, act, combine)
    assert [(e["kernel"], e["direction"], e["sequences"], e["frames"], e["units"]) for e in seen["recurrence"]] == \
        [(kernel_of(D), "fwd", N, T, Hh), (kernel_of(D), "bwd", N, T, Hh)], seen["recurrence"]
    # the projection's, D dW_hh and the dW_ih + bias weight-gradient GEMMs; four unpacks through autograd (W_hh, W_ih,
    # b_ih, b_hh: the two biases are unpacked apart), ONE pack
    assert len(seen["splits"]) == 2 + D and len(seen["packs"]) == 1, seen
    assert seen["unpack"] == [(H.GRU_HH, False), (H.GRU_IH, False), (H.GRU_IH, False), (H.GRU_HH, False)], seen["unpack"]
    assert got["y"].shape == ref[F64]["y"].shape and set(got) == set(ref[F64])
    note(mode, D, assert_within(got, ref[F64], ref[F32], is_split(), what=f"{ident(shape)} D={D} act={act} {mode}"))
    for sfx in ("", "_r")[:D]:      # the n rows of the two bias gradients differ (by the factor r), the others do not
        a, b = got["b_ih" + sfx], got["b_hh" + sfx]
        assert torch.equal(a[:2 * Hh], b[:2 * Hh]) and not torch.equal(a[2 * Hh:], b[2 * Hh:])


# ---- the three ways a gradient leaves the layer ------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("shape", [TOY, TOY_COMBINED, ALIGN, WIDE], ids=ident)
def test_sinks_accumulate_twice_the_autograd_gradient(shape, D, mode):
    """GradBucket sinks on the side stream (`direct`): two backward passes leave exactly 2 x the float64 gradient, within
    the bound scaled by 2"""
    N, T, I, Hh, hdim, combine = shape
    x, params, dy, ref = reference(shape, D, 0, 1)
    assert H.OVERLAP_WGRAD
    with logged() as seen:
        got, bucket = run_layer(x, params, dy, N, T, 1, combine, passes=2, sinks=True)
    assert seen["unpack"] == [(H.GRU_HH, True), (H.GRU_IH, True), (H.GRU_IH, True), (H.GRU_HH, True)] * 2, seen["unpack"]
    names = G.layer_names(D)
    what = f"{ident(shape)} D={D} sinks x2 {mode}"
    note(mode, D, assert_within(got, ref[F64], ref[F32], is_split(), names=[*names, "x"], scale=2.0, what=what))
    note(mode, D, assert_within(got, ref[F64], ref[F32], is_split(), names=["y"], what=what))
    plain, _ = run_layer(x, params, dy, N, T, 1, combine)
    for k in names:      # sink against autograd return, directly: 2 x, within the two results' bounds together
        b = bounds(ref[F32][k], ref[F64][k], is_split())
        e = errors(got[k], 2 * plain[k].double())
        assert e[0] <= 2 * b[0] and e[1] <= 2 * b[1], (k, e, b)


@pytest.mark.parametrize("D", [1, 2])
def test_frozen_parameter_falls_back_to_autograd_returns(D, mode):
    N, T, I, Hh, hdim, combine = TOY
    x, params, dy, ref = reference(TOY, D, 0, 1)
    with logged() as seen:
        got, bucket = run_layer(x, params, dy, N, T, 1, combine, sinks=True, frozen="bias_hh_l0")
    assert [a for _, a in seen["unpack"]] == [False] * 4, seen["unpack"]
    assert got["b_hh"] is None
    names = [k for k in G.layer_names(D) if k != "b_hh"]
    note(mode, D, assert_within(got, ref[F64], ref[F32], is_split(), names=["y", "x"] + names, what=f"frozen D={D} {mode}"))
    assert float(bucket.flat.abs().max()) > 0            # and they did arrive in the bucket


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("shape", [TOY, TOY_COMBINED], ids=ident)
def test_input_without_gradient(shape, D, mode):
    N, T, I, Hh, hdim, combine = shape
    x, params, dy, ref = reference(shape, D, 0, 1)
    got, _ = run_layer(x, params, dy, N, T, 1, combine, x_grad=False)
    assert got["x"] is None
    note(mode, D, assert_within(got, ref[F64], ref[F32], is_split(), names=["y", *G.layer_names(D)],
                                what=f"{ident(shape)} D={D} no dx {mode}"))


# ---- two stacked layers: the Tanh backward folded into the consumer's d(input) GEMM -----------------------------------------
# (N, T, I, H, hdim).  "toy" is the chain tests/test_gpu_causal_layer.py runs for typ = 'lstm'.  Its bound here is MARGIN x the
# fp32 restatement's own error at that shape taken over twelve seeds (gru_reference.chain_yardstick, where the reason is
# written down), not over the one draw of the case: measured on an MI355X against the one-draw yardstick, dW_hh of layer 0
# at D = 2, K = 4 under "f32" stood at 9.04 element-wise (normwise 1.8; every other tensor below 2.8) -- on the element
# (n rows, unit 0, k = 2) whose value is 0.001 of the tensor's largest, where torch.nn.GRU in fp32 on the same host stood at
# 4.58 and, at K = 0, at 11.08 on another tensor; on another host the same torch run gives 1.73 and 3.66, and the
# restatement's own figure for that tensor 4.2e-6 instead of 1.0e-6.  Over eleven other seeds the kernels' worst one-draw
# ratio was 5.5 (D = 2) and 5.1 (D = 1), torch's 6.2.  Nothing GRU-specific shows in the n rows: the three row blocks'
# errors are 0.4, 1.3 and 5.9 e-7 of the largest element against the restatement's 0.3, 1.2 and 3.3.
# Against the yardstick over seeds that element stands at 3.85 and it is the toy chain's worst under "f32" (109 under "bf16x3",
# allowed 6165).  "w64" and "w32" keep that file's one-draw bound.
CHAINS = {"toy": (8, 5, 7, 5, 8), "w64": (8, 5, 40, 64, 48), "w32": (32, 7, 321, 300, 320)}
_CHAIN = {}


def chain_reference(name, K, D):
    key = (name, K, D)
    if key not in _CHAIN:
        N, T, I, Hh, hdim = CHAINS[name]
        x, p0, p1, dy = G.chain_case(N, T, I, Hh, hdim, K, D)
        with torch.no_grad():
            r32 = G.two_layers(x, p0, p1, dy, N, T, K, F32)
        ref = {F64: G.two_layers(x, p0, p1, dy, N, T, K, F64, by_torch=True), F32: r32}
        if name == "toy":
            ref["yardstick"] = G.chain_yardstick(N, T, I, Hh, hdim, K, D)
        _CHAIN[key] = (x, p0, p1, dy, ref)
    return _CHAIN[key]


def chain_within(got, ref, split, names=None, what=""):
    """assert_within, or -- the toy chain -- the same report and assertion on the yardstick over seeds"""
    if "yardstick" not in ref:
        return assert_within(got, ref[F64], ref[F32], split, names=names, what=what)
    rep = G.yardstick_report(got, ref[F64], ref["yardstick"], split, names)
    for k, v in rep.items():
        print(f"{what} {k:9s} norm {v['norm']:.3g} (<= {v['bound_norm']:.3g}) elem {v['elem']:.3g} (<= {v['bound_elem']:.3g}) "
              f"ratio to the yardstick over seeds {v['ratio']:.3g}")
    bad = [k for k, v in rep.items() if not (v["norm"] <= v["bound_norm"] and v["elem"] <= v["bound_elem"])]
    assert not bad, (what, {k: rep[k] for k in bad})
    return rep


def chain_bounds(ref, k, split):
    if "yardstick" not in ref:
        return bounds(ref[F32][k], ref[F64][k], split)
    v = G.yardstick_report({k: ref[F64][k]}, ref[F64], ref["yardstick"], split, [k])[k]
    return v["bound_norm"], v["bound_elem"]


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("name,K", [("toy", 0), ("toy", 4), ("w64", 0), ("w64", 4), ("w32", 0), ("w32", 4)])
def test_two_layers_with_the_tanh_fold(name, K, D, mode):
    """in_tanh = 1 / in_tanh = K behind a combined producer, against the float64 chain through tanh; then unfolded (the
    activation has retain_grad): both inside the bound AND within one bound of each other"""
    N, T, I, Hh, hdim = CHAINS[name]
    x, p0, p1, dy, ref = chain_reference(name, K, D)
    B = N // (K or 1)
    split = is_split()
    names_ = G.layer_names(D)

    def run(retain):
        l0, q0 = G.gru_modules(p0, device=DEV)
        l1, q1 = G.gru_modules(p1, device=DEV)
        xg = x.to(DEV).clone().requires_grad_()
        h = Fn.rnnp_layer(xg, l0, q0, N, T, act=1, combine=K, dz_given=True)
        assert getattr(h, "_tssep_tanh_link", None) is not None
        if retain:
            h.retain_grad()
        y = Fn.rnnp_layer(h, l1, q1, B, T, in_tanh=(K or 1))
        y.backward(dy.to(DEV))
        out = {"1." + k: v for k, v in collect(y, None, l1, q1).items() if k in names_}
        out.update({"0." + k: v for k, v in collect(y, xg, l0, q0).items() if k in names_})
        out.update(y=y.detach().cpu(), x=xg.grad.cpu(), h=h.detach().cpu())
        if retain:
            out["dh"] = h.grad.cpu()
        return out

    with logged() as seen:
        folded = run(False)
    assert seen["tanh"] == [], "the fold was not taken"
    names = [k for k in ref[F64] if k != "dh"]
    note(mode, D, chain_within(folded, ref, split, names=names, what=f"{name} K={K} D={D} folded {mode}"))
    with logged() as seen:
        plain = run(True)
    assert seen["tanh"] == [1], "a watched activation: the producer runs its own Tanh backward"
    note(mode, D, chain_within(plain, ref, split, what=f"{name} K={K} D={D} unfolded {mode}"))
    for k in names:
        b = chain_bounds(ref, k, split)
        e = errors(folded[k], plain[k].double())
        assert e[0] <= b[0] and e[1] <= b[1], (k, e, b)


# ---- an active dropout site behind the layer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("shape", [TOY, TOY_COMBINED, WIDE], ids=ident)
def test_active_dropout_site(shape, D, mode):
    """y = keep ? tanh(z / (1 - p)) : 0 with the mask the host computes for the {seed, draw} the forward drew: the SAME mask
    in the backward (every gradient against the float64 layer fed dz = dy (1 - y^2) keep / (1 - p)), a fresh one next call"""
    import numpy as np
    N, T, I, Hh, hdim, combine = shape
    p = 0.3
    x, params, dy = G.make_layer_case(N, T, I, Hh, hdim, D, 9, combine)
    gru, lin = G.gru_modules(params, device=DEV)
    used, draw = [], H.dropout_draw
    H.dropout_draw = lambda device=None: (used.append(draw(device)), used[-1])[1]
    try:
        xg = x.to(DEV).clone().requires_grad_()
        y = Fn.rnnp_layer(xg, gru, lin, N, T, act=1, combine=combine, dropout_p=p)
        y.backward(dy.to(DEV))
        got = collect(y, xg, gru, lin)
        with torch.no_grad():
            y2 = Fn.rnnp_layer(x.to(DEV), gru, lin, N, T, act=1, combine=combine, dropout_p=p).cpu()
    finally:
        H.dropout_draw = draw
    assert len(used) == 2 and used[0].tolist() != used[1].tolist()
    seed, d = used[0].tolist()
    keep = torch.from_numpy(H.dropout_keep_host(seed, d, 0, N * T * hdim, p).astype(np.bool_)).view(N * T, hdim)   # logical rows (n, t)
    lay = (lambda t: combine_rows(t, N, T, combine)) if combine else (lambda t: t)
    ref = {}
    for dt, fn in ((F64, G.torch_layer), (F32, G.layer)):
        with torch.no_grad():
            z = G.layer_forward(x, params, N, T, dt)["y"]                                # rows (n, t), no activation
        scale = keep.to(dt) / (1 - p)
        yr = torch.tanh(z * scale)
        dyr = dy.to(dt) if not combine else dy.to(dt).view(N // combine, T, combine, hdim).permute(0, 2, 1, 3).reshape(N * T, hdim)
        with torch.set_grad_enabled(dt == F64):
            ref[dt] = dict(fn(x, params, dyr * (1 - yr * yr) * scale, N, T, dt, 0, 0))
        ref[dt]["y"] = lay(yr)
    note(mode, D, assert_within(got, ref[F64], ref[F32], is_split(), what=f"{ident(shape)} D={D} dropout {mode}"))
    dropped = lay(~keep)
    assert bool((got["y"][dropped] == 0).all()) and float(dropped.float().mean()) > 0.1
    assert not torch.equal(y2, got["y"]), "the next call drew the same mask"


# ---- the carried state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
def test_chunks_with_a_carried_state_match_float64(act, mode):
    N, T, I, Hh, hdim, combine = STATE_SHAPE
    x, params, dy, ref = reference(STATE_SHAPE, 1, 0, act)
    gru, lin = G.gru_modules(params, device=DEV)
    x3 = x.to(DEV).view(N, T, I)
    with torch.no_grad():
        whole, last = Fn.rnnp_layer(x3.reshape(N * T, I), gru, lin, N, T, act=act, return_state=True)
        g64, _ = G.gru_modules(params, dtype=F64)
        final = {F64: {"hT": g64(x.double().view(N, T, I))[1][0]}, F32: {"hT": G.chunked_forward(x, params, N, T, [T], F32, act)[1]}}
    assert torch.is_tensor(last) and tuple(last.shape) == (N, Hh), "a GRU's state is one tensor"
    note(mode, 1, assert_within({"hT": last.cpu()}, final[F64], final[F32], is_split(), what=f"final state {mode}"))
    for chunks in chunkings(T):
        state, ys, t0 = None, [], 0
        with logged() as seen, torch.no_grad():
            for n in chunks:
                y, state = Fn.rnnp_layer(x3[:, t0:t0 + n].reshape(N * n, I), gru, lin, N, n, act=act, state=state, return_state=True)
                assert tuple(state.shape) == (N, Hh)
                ys.append(y.view(N, n, hdim))
                t0 += n
        assert [e["frames"] for e in seen["recurrence"]] == chunks and all(e["kernel"] == "stream1_gru_f32" for e in seen["recurrence"])
        got = {"y": torch.cat(ys, 1).reshape(N * T, hdim).cpu()}
        note(mode, 1, assert_within(got, ref[F64], ref[F32], is_split(), names=["y"], what=f"chunks {chunks[:3]}.. act={act} {mode}"))
        note(mode, 1, assert_within({"hT": state.cpu()}, final[F64], final[F32], is_split(), what=f"chunks {chunks[:3]}.. final state {mode}"))
    gru2, lin2 = G.gru_modules(params, device=DEV)
    with pytest.raises(RuntimeError, match="without gradients"):
        Fn.rnnp_layer(x3.reshape(N * T, I), gru2, lin2, N, T, state=last)
    two, lin_two = torch.nn.GRU(I, Hh, bidirectional=True, batch_first=True).to(DEV), torch.nn.Linear(2 * Hh, hdim).to(DEV)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        Fn.rnnp_layer(x3.reshape(N * T, I), two, lin_two, N, T, state=last)


def test_final_state_under_autograd_carries_no_gradient(mode):
    N, T, I, Hh, hdim, combine = TOY
    x, params, dy, ref = reference(TOY, 1, 0, 1)
    gru, lin = G.gru_modules(params, device=DEV)
    xg = x.to(DEV).clone().requires_grad_()
    y, hT = Fn.rnnp_layer(xg, gru, lin, N, T, act=1, return_state=True)
    assert y.requires_grad and torch.is_tensor(hT) and not hT.requires_grad
    y.backward(dy.to(DEV))
    note(mode, 1, assert_within(collect(y, xg, gru, lin), ref[F64], ref[F32], is_split(), what=f"return_state {mode}"))


# ---- the kernel plan -------------------------------------------------------------------------------------------------------
def test_lstm_layers_record_the_kernels_they_recorded(mode):
    """a 'blstm' and an 'lstm' layer beside the GRU ones: the plan of an LSTM layer is recurrence_plan's without a cell
    argument -- the streaming kernels at the toy width, the W-stationary ones at H = 300 -- and lstm_pack's layouts"""
    from test_causal_reference import causal_modules, make_causal_case
    from test_rnnp_layer_reference import make_case, modules
    cus = H.n_cus(torch.device(DEV, torch.cuda.current_device()))
    names = {}
    for shape in (TOY, WIDE):
        N, T, I, Hh, hdim, combine = shape
        log = H.RECURRENCE_LOG = []
        try:
            for kind in ("blstm", "lstm", "bgru", "gru"):
                if kind == "blstm":
                    x, params, dy = make_case(N, T, I, Hh, hdim, 0, combine)
                    rnn, lin = modules(params, device=DEV)
                elif kind == "lstm":
                    x, params, dy = make_causal_case(N, T, I, Hh, hdim, 0, combine)
                    rnn, lin = causal_modules(params, device=DEV)
                else:
                    x, params, dy = G.make_layer_case(N, T, I, Hh, hdim, 2 if kind == "bgru" else 1, 0, combine)
                    rnn, lin = G.gru_modules(params, device=DEV)
                start = len(log)
                Fn.rnnp_layer(x.to(DEV).requires_grad_(), rnn, lin, N, T, act=1, combine=combine).backward(dy.to(DEV))
                torch.cuda.synchronize()
                names[(Hh, kind)] = [(e["kernel"], e["direction"]) for e in log[start:]]
        finally:
            H.RECURRENCE_LOG = None
        plan = H.recurrence_plan(N, T, Hh, cus)
        assert names[(Hh, "blstm")] == [(plan["fwd"][0], "fwd"), (plan["bwd"][0], "bwd")]
        assert names[(Hh, "lstm")] == [("stream1_f32", "fwd"), ("stream1_f32", "bwd")]
        assert names[(Hh, "bgru")] == [("stream_gru_f32", "fwd"), ("stream_gru_f32", "bwd")]
        assert names[(Hh, "gru")] == [("stream1_gru_f32", "fwd"), ("stream1_gru_f32", "bwd")]
    assert names[(5, "blstm")] == [("stream_f32", "fwd"), ("stream_f32", "bwd")]
    assert all(k.startswith("onchip") for k, _ in names[(300, "blstm")]), names[(300, "blstm")]


def test_zz_report():
    """the largest error / (the fp32 restatement's error) per tensor this run saw (pytest -rP; the bound is 8 under f32,
    8 x 770.6 under bf16x3; the module docstring has an MI355X's figures)"""
    for (mode_, D, name), v in sorted(RATIOS.items()):
        print(f"{mode_:7s} D={D} {name:8s} {v:.3g}")
