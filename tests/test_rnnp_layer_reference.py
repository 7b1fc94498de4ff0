"""One RNNP layer (BLSTM + projection (+ Tanh), functional._RNNP) restated in plain torch, and the error measure of
tests/test_gpu_rnnp_layer.py, both tested here without a GPU.

The restatement.  `layer_forward` / `layer_gradients` take x as rows (n, t), the eight LSTM tensors in torch's layout
and w_proj, b_proj, in any dtype: float64 is the reference, float32 ("same formulas, torch fp32, natural summation
order") is the yardstick.  The recurrence is the time loop of tests/test_recurrence_reference.py.  Every gradient is
written as the explicit sum it is, with no autograd:

    dz        = dy (1 - y^2)   (act = 1)   |   dy   (act = 0),          rows (n, t) after undoing the `combine` layout
    d b_proj  = sum_r dz[r, :]                     d w_proj[j, c] = sum_r dz[r, j] hcat[r, c],  hcat = [h_fwd | h_rev]
    dh[r, c]  = sum_j dz[r, j] w_proj[j, c]        D = the BPTT of the recurrence on dh   (d pre-activations)
    d w_ih_d[g, i] = sum_{n,t} D_d[n, t, g] x[n, t, i]
    d b_ih_d[g] = d b_hh_d[g] = sum_{n,t} D_d[n, t, g]
    d w_hh_f[g, k] = sum_n sum_{t >= 1}    D_f[n, t, g] h_f[n, t - 1, k]        (nothing at t = 0)
    d w_hh_r[g, k] = sum_n sum_{t <= T-2}  D_r[n, t, g] h_r[n, t + 1, k]        (nothing at t = T - 1)
    dx[r, i]  = sum_d sum_g D_d[r, g] w_ih_d[g, i]

It is pinned against torch.nn.LSTM(bidirectional).double() + Linear + Tanh under autograd (<= 1e-12 relative) and against
the reference project's own fixture tests/golden/rnnp.npz.

The error measure.  Per tensor two figures against float64 (`errors`): the normwise error |got - ref|_inf / |ref|_inf and
the element-wise error max_i |got - ref|_i / (|ref_i| + FLOOR |ref|_inf).  A non-finite `got` gives inf.  The bound of
either figure is MARGIN x the same figure of the fp32 restatement of the SAME case (never below the one rounding U every
fp32 result carries), x SPLIT_RATIO = C_SPLIT / U where the GEMMs of the case are split-bf16 (2^-16 per product
instead of 2^-24; derived in tests/test_gpu_gemm_kernels.py).  Nothing in the bound comes from a kernel.

MARGIN.  What may an fp32 implementation of the same formulas need over the restatement?  Here that question is put to an
independent one -- torch.nn.LSTM + Linear + Tanh in fp32 under autograd (other kernels, other summation orders) -- over
SEEDS at the GPU file's shapes: `test_margin_covers_an_independent_fp32_implementation` prints the ratio per tensor and
requires it inside MARGIN.  The worst seen is 4.05 (dW_ih at the toy width, where a tensor's largest error is one or two
roundings and moves with the seed; 2.3 at production width): MARGIN = 8, the power of two above it, which is also the
largest margin the measure is allowed before a ratio counts as a finding.

The teeth.  `CORRUPTIONS` plants, in the float64 gradients, each defect the layer's orchestration could have (a
boundary row of the neighbouring sequence in dW_hh, the directions swapped, the bias read from column I - 1, b_hh left
zero, a split-K partial dropped, the padding column of the hidden width leaking into dW_proj, the Tanh factor missing):
each must be rejected by the measure at the GPU file's shapes under the WIDER of the two bounds (split-bf16), and the
fp32 restatement itself must pass the NARROWER with the margin to spare."""
import pytest
import torch

from test_gpu_gemm_kernels import C_SPLIT, U
from test_recurrence_reference import _shift, lstm_backward_loop, lstm_forward_loop

NAMES = ("w_ih", "w_hh", "b_ih", "b_hh", "w_ih_r", "w_hh_r", "b_ih_r", "b_hh_r", "w_proj", "b_proj")
LSTM_ATTRS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
              "bias_ih_l0_reverse", "bias_hh_l0_reverse")
MARGIN = 8.0
FLOOR = 2.0 ** -4                 # element-wise: an element below |ref|_inf / 16 is held to the error of one of that size
SPLIT_RATIO = C_SPLIT / U         # 770.6: split-bf16 product error over the fp32 rounding
SEEDS = (0, 1, 2, 3, 4)
MAX_SPLITS = 128                  # (more partials than the library's split-K rule gives at these shapes: 80 at most)


def round_up(x, m):
    return (x + m - 1) // m * m


# ---- layouts ---------------------------------------------------------------------------------------------------------
def combine_rows(y, N, T, K):
    """rows (b, k, t) x hdim -> rows (b, t) x (k, hdim): the projection's `combine=K` store"""
    hd = y.shape[-1]
    return y.reshape(N // K, K, T, hd).permute(0, 2, 1, 3).reshape(N // K * T, K * hd)


def uncombine_rows(yc, N, T, K):
    """the inverse of combine_rows"""
    hd = yc.shape[-1] // K
    return yc.reshape(N // K, T, K, hd).permute(0, 2, 1, 3).reshape(N * T, hd)


def _gate_rows(D, d):
    """[N, T, 2, H, 4] -> direction d as [N, T, 4H] in torch's row order (gate * H + unit)"""
    N, T, _, H, _ = D.shape
    return D[:, :, d].transpose(2, 3).reshape(N, T, 4 * H)


# ---- the restatement -------------------------------------------------------------------------------------------------
def layer_forward(x, params, N, T, dtype, act=0, combine=0):
    """-> dict: y (the layer's output in the requested variant), y_rows (rows (n, t), after the activation) and what the
    gradients need (x, A, c, h [N, T, 2, H], hcat [N T, 2 H])"""
    p = [t.to(dtype) for t in params]
    x = x.to(dtype).reshape(N * T, -1)
    H = p[1].shape[1]
    gin = torch.stack([(x @ p[4 * d].t() + (p[4 * d + 2] + p[4 * d + 3])).view(N, T, 4, H).transpose(2, 3) for d in (0, 1)], 2)
    A, c, h = lstm_forward_loop(gin, [p[1], p[5]], H, dtype)
    hcat = h.reshape(N * T, 2 * H)
    z = hcat @ p[8].t() + p[9]
    y_rows = torch.tanh(z) if act else z
    y = combine_rows(y_rows, N, T, combine) if combine else y_rows
    return dict(x=x, A=A, c=c, h=h, hcat=hcat, y_rows=y_rows, y=y, N=N, T=T, H=H, act=act, combine=combine, p=p)


def layer_terms(fw, dy):
    """-> dz rows (n, t), D [N, T, 2, H, 4], Dg = per direction [N, T, 4H], hprev [N, T, 2, H] (h_{t-1} forward, h_{t+1}
    reverse, zeros at each sequence's first / last frame)"""
    N, T, H, p = fw["N"], fw["T"], fw["H"], fw["p"]
    dtype = fw["x"].dtype
    dy = dy.to(dtype)
    dy = uncombine_rows(dy, N, T, fw["combine"]) if fw["combine"] else dy.reshape(N * T, -1)
    dz = dy * (1 - fw["y_rows"] ** 2) if fw["act"] else dy
    dh = (dz @ p[8]).view(N, T, 2, H)
    D = lstm_backward_loop(fw["A"], fw["c"], dh, [p[1], p[5]], H, dtype)
    return dict(dz=dz, D=D, Dg=[_gate_rows(D, d) for d in (0, 1)], hprev=_shift(fw["h"], 1, -1))


def layer_gradients(fw, dy, terms=None):
    """-> {"x": dx rows (n, t), "w_ih": ..., "b_proj": ...}: the closed-form gradients listed in the module docstring"""
    tm = terms or layer_terms(fw, dy)
    x3 = fw["x"].view(fw["N"], fw["T"], -1)
    p = fw["p"]
    out = {"b_proj": tm["dz"].sum(0), "w_proj": torch.einsum("rj,rc->jc", tm["dz"], fw["hcat"])}
    dx = 0
    for d, sfx in ((0, ""), (1, "_r")):
        Dg = tm["Dg"][d]
        out["w_ih" + sfx] = torch.einsum("ntg,nti->gi", Dg, x3)
        out["w_hh" + sfx] = torch.einsum("ntg,ntk->gk", Dg, tm["hprev"][:, :, d])
        out["b_ih" + sfx] = Dg.sum((0, 1))
        out["b_hh" + sfx] = Dg.sum((0, 1))
        dx = dx + torch.einsum("ntg,gi->nti", Dg, p[4 * d])
    out["x"] = dx.reshape(fw["N"] * fw["T"], -1)
    return out


def layer(x, params, dy, N, T, dtype, act=0, combine=0):
    """-> the layer's outputs {"y", "x", the ten parameter names} in `dtype`"""
    fw = layer_forward(x, params, N, T, dtype, act, combine)
    out = layer_gradients(fw, dy)
    out["y"] = fw["y"]
    return out


def two_layers(x, p0, p1, dy, N, T, K, dtype):
    """Layer 0 (act = 1, combine = K or 0) feeding layer 1 (act = 0, N / K sequences): the chain through tanh.
    -> {"y", "h", "dh", "x", "0.<name>", "1.<name>"}"""
    Kc = K or 1
    f0 = layer_forward(x, p0, N, T, dtype, 1, K)
    f1 = layer_forward(f0["y"], p1, N // Kc, T, dtype, 0, 0)
    g1 = layer_gradients(f1, dy)
    g0 = layer_gradients(f0, g1["x"])
    out = {"y": f1["y"], "h": f0["y"], "dh": g1["x"], "x": g0["x"]}
    out.update({"0." + k: g0[k] for k in NAMES})
    out.update({"1." + k: g1[k] for k in NAMES})
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------
def make_params(I, Hh, hdim, gen, device="cpu"):
    """the ten tensors with torch.nn.LSTM's / Linear's initial ranges"""
    def uni(bound, *shape):
        return (torch.rand(*shape, generator=gen, device=device) * 2 - 1) * bound
    b = Hh ** -0.5
    lstm = [t for _ in (0, 1) for t in (uni(b, 4 * Hh, I), uni(b, 4 * Hh, Hh), uni(b, 4 * Hh), uni(b, 4 * Hh))]
    bp = (2 * Hh) ** -0.5
    return lstm + [uni(bp, hdim, 2 * Hh), uni(bp, hdim)]


def make_case(N, T, I, Hh, hdim, seed, combine=0, device="cpu"):
    """-> x rows (n, t) [N T, I], the ten parameters, dy in the output's layout: fp32 values, fixed seed"""
    gen = torch.Generator(device=device).manual_seed(1000 + seed)
    params = make_params(I, Hh, hdim, gen, device)
    x = torch.randn(N * T, I, generator=gen, device=device)
    K = combine or 1
    dy = torch.randn(N // K * T, K * hdim, generator=gen, device=device)
    return x, params, dy


def modules(params, device="cpu", dtype=torch.float32):
    """the ten tensors in torch.nn.LSTM / Linear containers"""
    I, Hh, hdim = params[0].shape[1], params[1].shape[1], params[8].shape[0]
    lstm = torch.nn.LSTM(I, Hh, bidirectional=True, batch_first=True)
    lin = torch.nn.Linear(2 * Hh, hdim)
    with torch.no_grad():
        for a, t in zip(LSTM_ATTRS, params[:8]):
            getattr(lstm, a).copy_(t)
        lin.weight.copy_(params[8])
        lin.bias.copy_(params[9])
    return lstm.to(device=device, dtype=dtype), lin.to(device=device, dtype=dtype)


def module_params(lstm, lin):
    return [getattr(lstm, a) for a in LSTM_ATTRS] + [lin.weight, lin.bias]


def torch_layer(x, params, dy, N, T, dtype, act=0, combine=0):
    """the same layer by torch.nn.LSTM + Linear (+ Tanh) under autograd"""
    lstm, lin = modules(params, dtype=dtype)
    xr = x.to(dtype).view(N, T, -1).clone().requires_grad_()
    z = lin(lstm(xr)[0]).reshape(N * T, -1)
    y = torch.tanh(z) if act else z
    y = combine_rows(y, N, T, combine) if combine else y
    (y * dy.to(dtype)).sum().backward()
    out = {k: t.grad for k, t in zip(NAMES, module_params(lstm, lin))}
    out.update(y=y.detach(), x=xr.grad.reshape(N * T, -1))
    return out


# ---- the error measure -------------------------------------------------------------------------------------------------
def errors(got, ref):
    """-> (normwise, element-wise) error of `got` against the float64 `ref`; inf for a NaN / Inf in `got`"""
    ref = ref.double()
    got = got.double().reshape(ref.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf"), float("inf")
    d = (got - ref).abs()
    m = float(ref.abs().max())
    if m == 0.0:
        z = 0.0 if float(d.max()) == 0.0 else float("inf")
        return z, z
    return float(d.max()) / m, float((d / (ref.abs() + FLOOR * m)).max())


def bounds(ref32, ref64, split):
    """-> (normwise, element-wise) bound of one tensor: MARGIN x the fp32 restatement's own figures (at least U)"""
    s = MARGIN * (SPLIT_RATIO if split else 1.0)
    return tuple(s * max(e, U) for e in errors(ref32, ref64))


def report(got, ref64, ref32, split, names=None, scale=1.0):
    """-> {name: dict(norm, elem, bound_norm, bound_elem, ratio)}: ratio = the larger of error / (the restatement's own
    error), what DESIGN.md records.  scale: `got` is compared with scale x ref (two accumulated backward passes)."""
    out = {}
    for k in names or ref64.keys():
        r64, r32 = ref64[k].double() * scale, ref32[k].double() * scale
        e, y = errors(got[k], r64), errors(r32, r64)
        b = bounds(r32, r64, split)
        out[k] = dict(norm=e[0], elem=e[1], bound_norm=b[0], bound_elem=b[1],
                      ratio=max(e[0] / max(y[0], U), e[1] / max(y[1], U)))
    return out


def failures(rep):
    return [k for k, v in rep.items() if not (v["norm"] <= v["bound_norm"] and v["elem"] <= v["bound_elem"])]


def assert_within(got, ref64, ref32, split, names=None, scale=1.0, what=""):
    """prints every figure, then asserts; -> the report"""
    rep = report(got, ref64, ref32, split, names, scale)
    for k, v in rep.items():
        print(f"{what} {k:9s} norm {v['norm']:.3g} (<= {v['bound_norm']:.3g}) elem {v['elem']:.3g} (<= {v['bound_elem']:.3g}) "
              f"ratio to the fp32 restatement {v['ratio']:.3g}")
    bad = failures(rep)
    assert not bad, (what, {k: rep[k] for k in bad})
    return rep


# ---- planted defects ---------------------------------------------------------------------------------------------------
def _drop_split(rows_a, rows_b, S):
    """sum over rows of a^T b with the last of S row slabs left out"""
    R = rows_a.shape[0]
    keep = R - -(-R // S)
    return torch.einsum("rg,ri->gi", rows_a[:keep], rows_b[:keep])


def corrupt(name, fw, dy, grads):
    """-> (the gradients with defect `name` planted, the tensors it must show in)"""
    g = dict(grads)
    tm = layer_terms(fw, dy)
    N, T, H = fw["N"], fw["T"], fw["H"]
    I = fw["x"].shape[1]
    R = N * T
    if name == "boundary_row_of_the_neighbour":      # kperiod ignored: h_{t-1} of frame 0 is the last frame of sequence n - 1
        flat = fw["h"][:, :, 0].reshape(R, H)
        prev = torch.cat([torch.zeros_like(flat[:1]), flat[:-1]])
        g["w_hh"] = torch.einsum("rg,rk->gk", tm["Dg"][0].reshape(R, 4 * H), prev)
        return g, ["w_hh"]
    if name == "boundary_row_of_the_neighbour_reverse":
        flat = fw["h"][:, :, 1].reshape(R, H)
        nxt = torch.cat([flat[1:], torch.zeros_like(flat[:1])])
        g["w_hh_r"] = torch.einsum("rg,rk->gk", tm["Dg"][1].reshape(R, 4 * H), nxt)
        return g, ["w_hh_r"]
    if name == "directions_swapped":
        g["w_hh"], g["w_hh_r"] = grads["w_hh_r"], grads["w_hh"]
        return g, ["w_hh", "w_hh_r"]
    if name == "bias_from_column_I_minus_1":
        for sfx in ("", "_r"):
            g["b_ih" + sfx] = g["b_hh" + sfx] = grads["w_ih" + sfx][:, I - 1]
        return g, ["b_ih", "b_hh", "b_ih_r", "b_hh_r"]
    if name == "b_hh_zero":
        g["b_hh"], g["b_hh_r"] = torch.zeros_like(grads["b_hh"]), torch.zeros_like(grads["b_hh_r"])
        return g, ["b_hh", "b_hh_r"]
    if name == "split_dropped_w_ih":        # the bias gradient rides in the same partials
        S = min(MAX_SPLITS, R)
        g["w_ih"] = _drop_split(tm["Dg"][0].reshape(R, -1), fw["x"], S)
        g["b_ih"] = g["b_hh"] = tm["Dg"][0].reshape(R, -1)[:R - -(-R // S)].sum(0)
        return g, ["w_ih", "b_ih", "b_hh"]
    if name == "split_dropped_w_hh":
        # (the forward direction: the last row of the last slab pairs with h_{T-2}; the reverse's pairs with nothing)
        g["w_hh"] = _drop_split(tm["Dg"][0].reshape(R, -1), tm["hprev"][:, :, 0].reshape(R, H), min(MAX_SPLITS, R))
        return g, ["w_hh"]
    if name == "split_dropped_w_proj":
        g["w_proj"] = _drop_split(tm["dz"], fw["hcat"], min(MAX_SPLITS, R))
        return g, ["w_proj"]
    if name == "padding_column_leaks":      # dW_proj in the padded layout [hdim, 2 Hp], un-laid-out as if Hp were Hh
        Hp = round_up(H, 4)
        assert Hp != H, "only where the hidden width is padded"
        dwp = torch.zeros(grads["w_proj"].shape[0], 2 * Hp, dtype=grads["w_proj"].dtype)
        dwp[:, :H], dwp[:, Hp:Hp + H] = grads["w_proj"][:, :H], grads["w_proj"][:, H:]
        g["w_proj"] = dwp[:, :2 * H].clone()
        return g, ["w_proj"]
    if name == "tanh_factor_missing":       # the folded path: dz taken as dy
        assert fw["act"] == 1
        plain = dict(fw, act=0)
        return dict(layer_gradients(plain, dy)), ["x", *NAMES]
    raise KeyError(name)


CORRUPTIONS = ("boundary_row_of_the_neighbour", "boundary_row_of_the_neighbour_reverse", "directions_swapped",
               "bias_from_column_I_minus_1", "b_hh_zero", "split_dropped_w_ih", "split_dropped_w_hh", "split_dropped_w_proj",
               "padding_column_leaks", "tanh_factor_missing")

# the shapes of the GPU file: name -> (N, T, I, Hh, hdim, combine)
SHAPES = {
    "pad": (6, 5, 7, 5, 6, 0),
    "pad_combined": (8, 5, 7, 5, 6, 4),
    "align": (6, 7, 8, 8, 8, 0),            # Hp == Hh at toy width (the reduce_splits_bias path)
    "w32": (32, 7, 321, 300, 320, 0),
    "w768": (768, 7, 321, 300, 320, 0),
    "w768_combined": (768, 7, 321, 300, 320, 4),
    "w3072": (3072, 7, 321, 256, 320, 0),
}
_CACHE = {}


def reference(shape, seed, act, dtypes=(torch.float64, torch.float32)):
    """-> (x, params, dy, {dtype: layer outputs}) of SHAPES[shape], computed once per process"""
    key = (shape, seed, act)
    if key not in _CACHE:
        N, T, I, Hh, hdim, combine = SHAPES[shape]
        x, params, dy = make_case(N, T, I, Hh, hdim, seed, combine)
        _CACHE[key] = (x, params, dy, {dt: layer(x, params, dy, N, T, dt, act, combine) for dt in dtypes})
    return _CACHE[key]


# ---- tests: the restatement is the layer -------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("dims,combine", [((3, 5, 7, 5, 6), 0), ((4, 3, 8, 4, 8), 0), ((4, 3, 8, 4, 8), 2), ((4, 5, 7, 5, 6), 2)])
def test_restatement_equals_torch_lstm_in_float64(dims, combine, act):
    N, T, I, Hh, hdim = dims
    x, params, dy = make_case(N, T, I, Hh, hdim, 7, combine)
    mine = layer(x, params, dy, N, T, torch.float64, act, combine)
    ref = torch_layer(x, params, dy, N, T, torch.float64, act, combine)
    assert mine["y"].shape == ((N // combine * T, combine * hdim) if combine else (N * T, hdim))
    for k in ("y", "x") + NAMES:
        e = errors(mine[k], ref[k])[0]
        print(k, e)
        assert e <= 1e-12, (k, e)


def test_two_layer_chain_equals_autograd_through_tanh():
    N, T, I, Hh, hdim, K = 4, 3, 8, 4, 8, 2
    gen = torch.Generator().manual_seed(5)
    p0, p1 = make_params(I, Hh, hdim, gen), make_params(K * hdim, Hh, hdim, gen)
    x = torch.randn(N * T, I, generator=gen)
    dy = torch.randn(N // K * T, hdim, generator=gen)
    mine = two_layers(x, p0, p1, dy, N, T, K, torch.float64)
    l0, q0 = modules(p0, dtype=torch.float64)
    l1, q1 = modules(p1, dtype=torch.float64)
    xr = x.double().view(N, T, I).requires_grad_()
    h = combine_rows(torch.tanh(q0(l0(xr)[0])).reshape(N * T, hdim), N, T, K)
    h.retain_grad()
    y = q1(l1(h.view(N // K, T, K * hdim))[0]).reshape(-1, hdim)
    (y * dy.double()).sum().backward()
    want = {"y": y.detach(), "h": h.detach(), "dh": h.grad, "x": xr.grad.reshape(N * T, I)}
    want.update({"0." + k: t.grad for k, t in zip(NAMES, module_params(l0, q0))})
    want.update({"1." + k: t.grad for k, t in zip(NAMES, module_params(l1, q1))})
    for k, w in want.items():
        assert errors(mine[k], w)[0] <= 1e-12, k


def test_restatement_against_the_reference_fixture(golden):
    """tests/golden/rnnp.npz: the reference project's RNNP_packed(7, 1, 5, 6, 0) in fp32, forward and every gradient.
    An fp32 realisation of the layer from another code base: it passes the fp32 bound of the measure."""
    g = golden("rnnp")
    keys = ["net.0." + a for a in LSTM_ATTRS] + ["net.1.weight", "net.1.bias"]
    params = [torch.as_tensor(g["p." + k]) for k in keys]
    for tag, (N, T) in (("x3", (3, 9)), ("x4", (6, 9)), ("x2", (1, 9))):
        x, dy = torch.as_tensor(g[tag]).reshape(N * T, 7), torch.as_tensor(g[tag + "_g"]).reshape(N * T, 6)
        r64, r32 = (layer(x, params, dy, N, T, dt) for dt in (torch.float64, torch.float32))
        got = {"y": torch.as_tensor(g[tag + "_y"]), "x": torch.as_tensor(g[tag + "_dx"])}
        got.update({n: torch.as_tensor(g[f"{tag}_dp.{k}"]) for n, k in zip(NAMES, keys)})
        assert_within(got, r64, r32, split=False, what=tag)


# ---- tests: the measure ------------------------------------------------------------------------------------------------
CPU_SHAPES = ("pad", "pad_combined", "align", "w32", "w768_combined")


@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_margin_covers_an_independent_fp32_implementation(shape):
    """torch.nn.LSTM + Linear + Tanh in fp32 under autograd against the fp32 restatement's own error, over SEEDS: inside
    MARGIN.  (The wide shapes take one seed: their maxima run over 10^5 elements and move little.)"""
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    worst = {}
    wide = N * T * Hh >= 10000
    for seed in (SEEDS[:1] if wide else SEEDS):
        for act in ((1,) if wide else (0, 1)):
            x, params, dy, ref = reference(shape, seed, act)
            got = torch_layer(x, params, dy, N, T, torch.float32, act, combine)
            rep = report(got, ref[torch.float64], ref[torch.float32], split=False)
            for k, v in rep.items():
                worst[k] = max(worst.get(k, 0.0), v["ratio"])
    print(shape, " ".join(f"{k}={v:.2f}" for k, v in worst.items()))
    assert max(worst.values()) <= MARGIN, worst


@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_fp32_restatement_is_inside_the_bound_with_the_margin_to_spare(shape):
    x, params, dy, ref = reference(shape, 0, 1)
    rep = report(ref[torch.float32], ref[torch.float64], ref[torch.float32], split=False)
    for k, v in rep.items():
        assert v["norm"] * MARGIN <= v["bound_norm"] * (1 + 1e-12) and v["elem"] * MARGIN <= v["bound_elem"] * (1 + 1e-12), (k, v)
        assert v["bound_norm"] < 1e-4, (k, v)       # and the bound is not vacuous: fp32-sized at every shape


# (the padding column exists only where Hh is no multiple of 4)
DEFECT_CASES = [(s, c) for s in CPU_SHAPES for c in CORRUPTIONS if c != "padding_column_leaks" or SHAPES[s][3] % 4]


@pytest.mark.parametrize("shape,name", DEFECT_CASES)
def test_planted_defects_are_rejected(shape, name):
    """each defect, planted in the float64 gradients, fails the measure under the WIDER (split-bf16) bound in every
    tensor it touches"""
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy, ref = reference(shape, 0, 1)
    fw = layer_forward(x, params, N, T, torch.float64, 1, combine)
    bad, touched = corrupt(name, fw, dy, ref[torch.float64])
    bad["y"] = ref[torch.float64]["y"]
    rep = report(bad, ref[torch.float64], ref[torch.float32], split=True)
    failed = failures(rep)
    print(name, shape, {k: (f"{rep[k]['norm']:.3g}", f"{rep[k]['bound_norm']:.3g}") for k in touched})
    assert set(touched) <= set(failed), (name, touched, failed, {k: rep[k] for k in touched})
    assert set(failed) <= set(touched), (name, failed)       # and nothing else moved
