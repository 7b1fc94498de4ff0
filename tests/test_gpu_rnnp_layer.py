"""functional.rnnp_layer -- one BLSTM + projection layer, forward and the 200 lines of backward orchestration -- and the
`derived` layout memo of hip_ops, on a real MI355X against the float64 restatement of tests/test_rnnp_layer_reference.py.

Measure and bound are that file's (`assert_within`): per tensor the normwise and the element-wise error against float64,
each within MARGIN x the same figure of the fp32 restatement of the same case under GEMM_PRECISION = "f32", and that
x C_SPLIT / U under "bf16x3".  The recurrence plan does not follow GEMM_PRECISION: at production width the W-stationary
split-bf16 recurrences run under "f32" too, and are held to the fp32 bound there all the same (they need 6.2 of the 8;
DESIGN.md section 4.4).  Every case has a fixed seed; NaN or Inf anywhere fails (the measure
returns inf).  What each case took -- recurrence families, split counts, fused_colsum -- is asserted from host-side queries
in `test_zz_every_branch_is_reachable_at_these_shapes`, and per case from the launch logs."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_rnnp_layer_reference import (NAMES, SHAPES, assert_within, bounds, errors, layer, make_case,  # noqa: E402
                                       make_params, module_params, modules, reference, round_up, two_layers)
from tssep_amd import _lib, functional as Fn, hip_ops as H  # noqa: E402
from tssep_amd.distributed import GradBucket  # noqa: E402
from tssep_amd.train import runtime  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
RATIOS = {}          # (mode, tensor) -> the largest error / (the fp32 restatement's error) this run saw (test_zz_report)

# recurrence routing of the production-width shapes: tests/test_gpu_recurrence_kernels.py::test_through_the_plan
SETTINGS = {"w32": dict(recurrence="cluster"), "w3072": dict(onchip16_bwd=False)}
FAMILY = {"w32": ("cluster_f32", "cluster_f32"), "w768": ("onchip16_bf16x3", "onchip16_bf16x3"),
          "w768_combined": ("onchip16_bf16x3", "onchip16_bf16x3"), "w3072": ("onchip16_bf16x3", "onchip32_bf16x3")}


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request):
    """both GEMM arithmetics, hence both values of fused_colsum(); restored afterwards"""
    with runtime.applied(gemm_precision=request.param):
        assert H.fused_colsum() == (request.param == "bf16x3")
        yield request.param


def _cus():
    return H.n_cus(torch.device("cuda", torch.cuda.current_device()))


def is_split(*layers):
    """which of the two bounds the case is held to: the GEMM arithmetic decides (module docstring)"""
    return H.GEMM_PRECISION != "f32"


@contextlib.contextmanager
def logged():
    """-> dict(recurrence=[...], splits=[S of every wgrad], unpack=[accumulate of every lstm_unpack], packs=[...],
    tanh=[one entry per stand-alone Tanh backward])"""
    seen = dict(recurrence=[], splits=[], unpack=[], packs=[], tanh=[])
    wgrad, unpack, pack, tanh_bwd = H.wgrad, H.lstm_unpack, H.lstm_pack, H.tanh_bwd

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

    old_log = H.RECURRENCE_LOG
    H.wgrad, H.lstm_unpack, H.lstm_pack, H.tanh_bwd, H.RECURRENCE_LOG = wgrad_, unpack_, pack_, tanh_, seen["recurrence"]
    try:
        yield seen
    finally:
        H.wgrad, H.lstm_unpack, H.lstm_pack, H.tanh_bwd, H.RECURRENCE_LOG = wgrad, unpack, pack, tanh_bwd, old_log


def collect(y, xg, lstm, lin):
    torch.cuda.synchronize()
    H.check_cluster_errors()
    out = {k: (p.grad.detach().cpu() if p.grad is not None else None) for k, p in zip(NAMES, module_params(lstm, lin))}
    out["y"] = y.detach().cpu()
    out["x"] = xg.grad.detach().cpu() if xg is not None and xg.grad is not None else None
    return out


def run_layer(x, params, dy, N, T, act, combine, x_grad=True, passes=1, sinks=False, frozen=None):
    """-> (outputs on the host, the bucket or None).  sinks: a GradBucket owns the gradients before the first backward."""
    lstm, lin = modules(params, device=DEV)
    if frozen:
        getattr(lstm, frozen).requires_grad_(False)
    bucket = GradBucket(module_params(lstm, lin)) if sinks else None
    xg = x.to(DEV).clone().requires_grad_(x_grad)
    for _ in range(passes):
        y = Fn.rnnp_layer(xg, lstm, lin, N, T, act=act, combine=combine)
        y.backward(dy.to(DEV))
    if bucket is not None:
        bucket.sync()            # the side stream's weight gradients, BEFORE anything reads the bucket
    return collect(y, xg, lstm, lin), bucket


def note(mode_, rep):
    for k, v in rep.items():
        key = (mode_, k.split(".")[-1])
        RATIOS[key] = max(RATIOS.get(key, 0.0), v["ratio"])


# ---- the layer against float64: shapes x act x combine ---------------------------------------------------------------------
LAYER_CASES = [("pad", 0), ("pad", 1), ("pad_combined", 0), ("pad_combined", 1), ("align", 1), ("w32", 1), ("w768", 0), ("w768", 1),
               ("w768_combined", 0), ("w768_combined", 1), ("w3072", 1)]


@pytest.mark.parametrize("shape,act", LAYER_CASES)
def test_layer_matches_float64(shape, act, mode):
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy, ref = reference(shape, 0, act)
    with runtime.applied(**SETTINGS.get(shape, {})), logged() as seen:
        split = is_split((N, T, Hh))
        plan = H.recurrence_plan(N, T, Hh, _cus())
        got, _ = run_layer(x, params, dy, N, T, act, combine)
    assert [e["kernel"] for e in seen["recurrence"]] == [plan["fwd"][0], plan["bwd"][0]], (seen["recurrence"], plan)
    if shape in FAMILY:
        assert (plan["fwd"][0], plan["bwd"][0]) == FAMILY[shape], plan
    else:
        assert plan["fwd"][0] == plan["bwd"][0] == "stream_f32"
    assert split == (mode == "bf16x3")
    assert len(seen["splits"]) == 4 and seen["unpack"] == [False] * 3 and len(seen["packs"]) == 1, seen
    assert got["y"].shape == ref[F64]["y"].shape
    print(shape, "splits", seen["splits"], "plan", plan, "split-bf16" if split else "fp32")
    note(mode, assert_within(got, ref[F64], ref[F32], split, what=f"{shape} act={act} {mode}"))


# ---- the three ways a gradient leaves the layer ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["pad", "pad_combined", "align", "w768"])
def test_sinks_accumulate_twice_the_autograd_gradient(shape, mode):
    """GradBucket sinks on the side stream (`direct`): two backward passes leave exactly 2 x the float64 gradient, within
    the bound scaled by 2; the same case through autograd leaves 1 x.  pad: Hp != Hh (_proj_unlayout + add_); align,
    w768: Hp == Hh -- reduce_splits_bias under fused_colsum (bf16x3), reduce_splits + colsum without (f32)."""
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy, ref = reference(shape, 0, 1)
    split = is_split((N, T, Hh))
    assert H.OVERLAP_WGRAD
    calls = dict(bias=0, plain=0)
    rsb = H.reduce_splits_bias
    H.reduce_splits_bias = lambda *a, **k: (calls.__setitem__("bias", calls["bias"] + 1), rsb(*a, **k))[1]
    try:
        with logged() as seen:
            got, bucket = run_layer(x, params, dy, N, T, 1, combine, passes=2, sinks=True)
    finally:
        H.reduce_splits_bias = rsb
    assert seen["unpack"] == [True] * 8, seen["unpack"]        # the direct path, both passes (four unpacks each)
    assert calls["bias"] == (2 if (round_up(Hh, 4) == Hh and H.fused_colsum()) else 0), calls
    note(mode, assert_within(got, ref[F64], ref[F32], split, names=NAMES, scale=2.0, what=f"{shape} sinks x2 {mode}"))
    note(mode, assert_within(got, ref[F64], ref[F32], split, names=["y"], what=f"{shape} sinks {mode}"))
    # dx comes back through autograd and accumulates there: 2 x as well
    note(mode, assert_within(got, ref[F64], ref[F32], split, names=["x"], scale=2.0, what=f"{shape} sinks x2 {mode}"))
    plain, _ = run_layer(x, params, dy, N, T, 1, combine)
    for k in NAMES:      # sink against autograd return, directly: 2 x, within the two results' bounds together
        b = bounds(ref[F32][k], ref[F64][k], split)
        e = errors(got[k], 2 * plain[k].double())
        assert e[0] <= 2 * b[0] and e[1] <= 2 * b[1], (k, e, b)


def test_frozen_parameter_falls_back_to_autograd_returns(mode):
    """one parameter without a sink: nothing is accumulated directly, autograd adds into the bucket's views, the frozen
    one gets nothing and the others stay right"""
    N, T, I, Hh, hdim, combine = SHAPES["pad"]
    x, params, dy, ref = reference("pad", 0, 1)
    with logged() as seen:
        got, bucket = run_layer(x, params, dy, N, T, 1, combine, sinks=True, frozen="bias_hh_l0")
    assert seen["unpack"] == [False] * 3, seen["unpack"]
    assert got["b_hh"] is None
    names = [k for k in NAMES if k != "b_hh"]
    note(mode, assert_within(got, ref[F64], ref[F32], is_split((N, T, Hh)), names=["y", "x"] + names, what=f"frozen {mode}"))
    assert float(bucket.flat.abs().max()) > 0            # and they did arrive in the bucket


@pytest.mark.parametrize("shape", ["pad", "pad_combined"])
def test_input_without_gradient(shape, mode):
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy, ref = reference(shape, 0, 1)
    got, _ = run_layer(x, params, dy, N, T, 1, combine, x_grad=False)
    assert got["x"] is None
    note(mode, assert_within(got, ref[F64], ref[F32], is_split((N, T, Hh)), names=["y", *NAMES], what=f"{shape} no dx {mode}"))


@pytest.mark.parametrize("shape,act", [("pad", 1), ("pad_combined", 0), ("w32", 1)])
def test_input_is_a_strided_view_of_a_padded_buffer(shape, act, mode):
    """ld_x > round_up(I, 4): x is the first I columns of a wider buffer whose columns past the 16-byte group of x hold
    other data (3.0), which must neither be read nor receive a gradient"""
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy, ref = reference(shape, 0, act)
    ld = round_up(I, 4) + 8
    buf = torch.zeros(N * T, ld, device=DEV)
    buf[:, :I] = x.to(DEV)
    buf[:, round_up(I, 4):] = 3.0
    buf.requires_grad_()
    lstm, lin = modules(params, device=DEV)
    with runtime.applied(**SETTINGS.get(shape, {})):
        split = is_split((N, T, Hh))
        xv = buf[:, :I]
        assert H.rows_view(xv)[1] == ld
        y = Fn.rnnp_layer(xv, lstm, lin, N, T, act=act, combine=combine)
        y.backward(dy.to(DEV))
        got = collect(y, buf, lstm, lin)
    assert float(got["x"][:, I:].abs().max()) == 0.0
    got["x"] = got["x"][:, :I]
    note(mode, assert_within(got, ref[F64], ref[F32], split, what=f"{shape} strided x {mode}"))


@pytest.mark.parametrize("shape,act", [("pad", 0), ("pad", 1), ("pad_combined", 0), ("pad_combined", 1)])
def test_output_gradient_is_not_contiguous(shape, act, mode):
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy, ref = reference(shape, 0, act)
    dyt = dy.to(DEV).t().contiguous().t()              # the same values, column-major
    assert not dyt.is_contiguous()
    lstm, lin = modules(params, device=DEV)
    xg = x.to(DEV).clone().requires_grad_()
    y = Fn.rnnp_layer(xg, lstm, lin, N, T, act=act, combine=combine)
    y.backward(dyt)
    note(mode, assert_within(collect(y, xg, lstm, lin), ref[F64], ref[F32], is_split((N, T, Hh)), what=f"{shape} dy^T {mode}"))


# ---- two stacked layers: the Tanh backward folded into the consumer's d(input) GEMM -----------------------------------------
CHAINS = {"toy": (8, 5, 7, 5, 8), "w768": (768, 7, 321, 300, 320)}
_CHAIN = {}


def chain_reference(name, K):
    key = (name, K)
    if key not in _CHAIN:
        N, T, I, Hh, hdim = CHAINS[name]
        gen = torch.Generator().manual_seed(77)
        p0, p1 = make_params(I, Hh, hdim, gen), make_params((K or 1) * hdim, Hh, hdim, gen)
        x = torch.randn(N * T, I, generator=gen)
        dy = torch.randn(N // (K or 1) * T, hdim, generator=gen)
        _CHAIN[key] = (x, p0, p1, dy, {dt: two_layers(x, p0, p1, dy, N, T, K, dt) for dt in (F64, F32)})
    return _CHAIN[key]


@pytest.mark.parametrize("name,K", [("toy", 0), ("toy", 4), ("w768", 0), ("w768", 4)])
def test_two_layers_with_the_tanh_fold(name, K, mode):
    """in_tanh = 1 / in_tanh = K behind a combined producer, against the float64 chain through tanh; then unfolded (the
    activation has retain_grad): both inside the bound AND within one bound of each other"""
    N, T, I, Hh, hdim = CHAINS[name]
    x, p0, p1, dy, ref = chain_reference(name, K)
    B = N // (K or 1)
    split = is_split((N, T, Hh), (B, T, Hh))

    def run(retain):
        l0, q0 = modules(p0, device=DEV)
        l1, q1 = modules(p1, device=DEV)
        xg = x.to(DEV).clone().requires_grad_()
        h = Fn.rnnp_layer(xg, l0, q0, N, T, act=1, combine=K, dz_given=True)
        assert getattr(h, "_tssep_tanh_link", None) is not None
        if retain:
            h.retain_grad()
        y = Fn.rnnp_layer(h, l1, q1, B, T, in_tanh=(K or 1))
        y.backward(dy.to(DEV))
        out = {"1." + k: v for k, v in collect(y, None, l1, q1).items() if k in NAMES}
        out.update({"0." + k: v for k, v in collect(y, xg, l0, q0).items() if k in NAMES})
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


# ---- the time shift of dW_hh -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["pad", "w32"])
def test_boundary_pairing_probe(shape, mode):
    """dy lives on ONE sequence; its neighbours get inputs four times as large (saturated h).  dgates_t of that sequence
    must pair with ITS h_{t-1} / h_{t+1} and with nothing at its first / last frame: a wrong period would add a
    neighbour's row, an O(1) error of dW_hh here."""
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy = make_case(N, T, I, Hh, hdim, 31)
    n = N // 2
    x = x.view(N, T, I).clone()
    x[n - 1] *= 4
    x[n + 1] *= 4
    x = x.reshape(N * T, I)
    only = torch.zeros_like(dy.view(N, T, hdim))
    only[n] = dy.view(N, T, hdim)[n]
    dy = only.reshape(N * T, hdim)
    ref = {dt: layer(x, params, dy, N, T, dt, 1, 0) for dt in (F64, F32)}
    with runtime.applied(**SETTINGS.get(shape, {})):
        split = is_split((N, T, Hh))
        got, _ = run_layer(x, params, dy, N, T, 1, 0)
    note(mode, assert_within(got, ref[F64], ref[F32], split, what=f"{shape} probe {mode}"))


# ---- the layout memo -------------------------------------------------------------------------------------------------------
MEMO = (4, 5, 8, 4, 8)          # N, T, I, Hh, hdim


class Memo:
    """one small layer on the device, its forward and the float64 restatement on whatever its weights are NOW"""

    def __init__(self, seed=3):
        self.N, self.T, I, Hh, hdim = MEMO
        self.x, params, self.dy = make_case(self.N, self.T, I, Hh, hdim, seed)
        self.lstm, self.lin = modules(params, device=DEV)
        self.xd = self.x.to(DEV)

    def params(self):
        return module_params(self.lstm, self.lin)

    def forward(self, grad=False):
        with torch.enable_grad() if grad else torch.no_grad():
            return Fn.rnnp_layer(self.xd, self.lstm, self.lin, self.N, self.T, act=1)

    def check(self, y, old=None, what=""):
        torch.cuda.synchronize()
        now = [p.detach().cpu() for p in self.params()]
        r64, r32 = (layer(self.x, now, self.dy, self.N, self.T, dt, 1, 0) for dt in (F64, F32))
        assert_within({"y": y.detach().cpu()}, r64, r32, is_split((self.N, self.T, MEMO[3])), names=["y"], what=what)
        if old is not None:      # and the weights did move: far more than any bound
            assert errors(y.detach().cpu(), old.detach().cpu().double())[0] > 1e-2, what


def test_memo_hits_within_a_step_and_across_micro_steps():
    m = Memo()
    with logged() as seen:
        y = m.forward(grad=True)
        assert len(seen["packs"]) == 1
        y.backward(m.dy.to(DEV))
        assert len(seen["packs"]) == 1, "the backward rebuilt the gate pack"
        y2 = m.forward(grad=True)
        assert len(seen["packs"]) == 1, "the second micro-step rebuilt the gate pack"
    m.check(y2, what="second micro-step")
    assert torch.equal(y, y2)


@pytest.mark.parametrize("route", ["no_grad_mul", "load_state_dict", "set_parameters", "adam_step", "other_stream"])
def test_memo_follows_the_weights(route):
    from tssep_amd.train.optimizer import Adam
    m = Memo()
    y0 = m.forward()
    m.check(y0, what="before")
    with logged() as seen:
        if route == "no_grad_mul":
            with torch.no_grad():
                for p in m.params():
                    p.mul_(1.5)
        elif route == "load_state_dict":
            other = Memo(seed=4)
            m.lstm.load_state_dict(other.lstm.state_dict())
            m.lin.load_state_dict(other.lin.state_dict())
        elif route == "set_parameters":      # re-homes p.data: same values at new addresses -> rebuilt, same output
            ptrs = [p.data_ptr() for p in m.params()]
            opt = Adam(lr=0.1)
            opt.set_parameters(m.params())
            assert all(a != p.data_ptr() for a, p in zip(ptrs, m.params()))
        elif route == "adam_step":           # the fused kernel writes through the raw pointer of the flat buffer
            opt = Adam(lr=0.1)
            opt.set_parameters(m.params())
            y = m.forward(grad=True)
            y.backward(m.dy.to(DEV))
            n = len(seen["packs"])
            opt.step()
            y1 = m.forward()
            assert len(seen["packs"]) == n + 1
            m.check(y1, old=y0, what=route)
            return
        if route == "other_stream":
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                y1 = m.forward()
            torch.cuda.current_stream().wait_stream(s)
        else:
            y1 = m.forward()
        assert len(seen["packs"]) == 1, (route, "the gate pack was not rebuilt")
    if route in ("set_parameters", "other_stream"):
        m.check(y1, what=route)
        assert errors(y1.cpu(), y0.cpu().double())[0] <= 1e-6
    else:
        m.check(y1, old=y0, what=route)


def test_memo_dies_with_its_module():
    """a second module whose parameters may reuse the first one's freed addresses never sees its packs"""
    m = Memo(seed=5)
    y0 = m.forward()
    torch.cuda.synchronize()
    freed = {p.data_ptr() for p in m.params()}
    y0 = y0.cpu()
    del m
    m2 = Memo(seed=6)
    print("addresses reused:", len(freed & {p.data_ptr() for p in m2.params()}))
    with logged() as seen:
        y1 = m2.forward()
    assert len(seen["packs"]) == 1
    m2.check(y1, what="second module")
    assert errors(y1.cpu(), y0.double())[0] > 1e-2


def test_trainer_shaped_write_into_flat_param(monkeypatch):
    """forward -> rank 0's parameters arrive in `optimizer.flat_param` -> forward.  The write moves neither validity signal
    (hip_ops.derived: the `.data` rule); trainer.adopt_rank0_state declares the layouts stale, and the second forward runs
    on the new weights.  The same for a `p.data.copy_` followed by weights_changed()."""
    from tssep_amd import distributed
    from tssep_amd.train import trainer
    from tssep_amd.train.optimizer import Adam
    m = Memo()
    opt = Adam(lr=0.1)
    opt.set_parameters(m.params())
    y0 = m.forward()
    versions = [p._version for p in m.params()]

    def arrives(t, src=0):
        if t is opt.flat_param:
            t.mul_(-1.5)
        return t
    monkeypatch.setattr(distributed, "broadcast_", arrives)
    trainer.adopt_rank0_state(opt)
    assert versions == [p._version for p in m.params()]          # (what makes this a blind spot of the stamp)
    y1 = m.forward()
    m.check(y1, old=y0, what="after the broadcast")
    with torch.no_grad():
        m.lin.weight.data.copy_(m.lin.weight.data * 2)
    H.weights_changed()
    m.check(m.forward(), old=y1, what="after p.data.copy_ + weights_changed")


# ---- what the shapes reach, from the host alone ------------------------------------------------------------------------------
def _wgrad_splits(M, Ncols, R, ld_dy, ld_x, shift=0, T=0, ones=False):
    """the split count `hip_ops.wgrad` would ask the library for (tssep_gemm_wgrad_splits; no launch)"""
    Nc = Ncols + 1 if ones else Ncols
    ldp = round_up(Nc, 4) if ones else Ncols
    d = torch.empty(4, device=DEV)
    g = H._gemm_args(d, ld_dy, d, ld_x, d, ldp, M, Nc, R, a_kmajor=True, b_kmajor=True, b_kshift=shift, kperiod=T, splitk=8,
                     split_stride=M * ldp, b_ones_col=ones)
    S = int(_lib.lib().tssep_gemm_wgrad_splits(H.ctypes.byref(g)))
    assert S >= 1, S
    return S


def test_zz_every_branch_is_reachable_at_these_shapes(mode):
    cus = _cus()
    fams = set()
    for shape, want in FAMILY.items():
        N, T, I, Hh, hdim, _ = SHAPES[shape]
        with runtime.applied(**SETTINGS.get(shape, {})):
            plan = H.recurrence_plan(N, T, Hh, cus)
        assert (plan["fwd"][0], plan["bwd"][0]) == want, (shape, plan)
        fams |= {plan["fwd"][0], plan["bwd"][0]}
    assert fams == {"cluster_f32", "onchip16_bf16x3", "onchip32_bf16x3"}
    N, T, I, Hh, hdim, _ = SHAPES["pad"]
    assert H.recurrence_plan(N, T, Hh, cus)["fwd"][0] == "stream_f32"
    splits = {}
    for shape in ("pad", "w32", "w768", "w3072"):
        N, T, I, Hh, hdim, _ = SHAPES[shape]
        R, Hp, fused = N * T, round_up(Hh, 4), H.fused_colsum()
        splits[shape] = (_wgrad_splits(hdim, 2 * Hp, R, round_up(hdim, 4), 2 * Hp),
                         _wgrad_splits(4 * Hh, Hh, R, 8 * Hh, 2 * Hp, shift=-1, T=T),
                         _wgrad_splits(8 * Hh, I, R, 8 * Hh, round_up(I, 4), ones=fused))
    print(mode, splits)
    flat = [S for v in splits.values() for S in v]
    assert any(S == 1 for S in flat) and any(S > 1 for S in flat), splits
    assert I % 4 and round_up(I, 4) != I


def test_zz_report():
    """the largest ratio to the fp32 restatement's own error per arithmetic and tensor this run saw (pytest -rP)"""
    for (m, k), v in sorted(RATIOS.items()):
        print(f"{m:7s} {k:8s} {v:.3g}")
