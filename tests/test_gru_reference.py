"""The float64 GRU references of tests/gru_reference.py, tested without a GPU.

1. The loops against torch.  The packed four-slot layer (pack_reference -> the input product -> gru_forward_loop ->
   gru_backward_loop -> the weight-gradient products -> unpack_reference) equals torch.nn.GRU in float64, the output and the
   autograd gradients of the input and of every parameter, for one and two directions: they state the same formula, so the
   tolerance is float64 rounding (1e-12 relative to the largest element).  db_ih and db_hh differ on the n rows.
2. The checkers pass an fp32 loop of the same formula and fail each of five planted defects, at the shapes
   tests/test_gpu_gru_kernels.py uses.
3. The host side: the GRU entry points are declared, exported, wrapped and planned; functional.rnnp_layer takes a
   torch.nn.GRU container, whose state is one tensor, and refuses what it refuses for an LSTM (this part fails on the parent).
4. The restated layer (GRU + projection (+ Tanh), chains, chunks) equals torch.nn.GRU + Linear + Tanh in float64.
"""
import pytest
import torch

import gru_reference as G

SHAPES = [(9, 7, 300), (8, 2, 65), (1, 1, 5), (9, 7, 64)]      # of the GPU file's grid: its largest, its smallest, two between


def _gru(I, H, D, seed):
    torch.manual_seed(seed)
    return torch.nn.GRU(I, H, batch_first=True, bidirectional=D == 2).double()


def _params(gru, D):
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    return [getattr(gru, n + sfx) for sfx in ("", "_reverse")[:D] for n in names]


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("n,T,I,H", [(3, 6, 7, 5), (2, 1, 4, 9), (2, 5, 3, 16)])
def test_loops_equal_torch_gru_in_float64(n, T, I, H, D):
    gru = _gru(I, H, D, 3)
    gen = torch.Generator().manual_seed(4)
    x = torch.randn(n, T, I, generator=gen, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(n, T, D * H, generator=gen, dtype=torch.float64)
    y, _ = gru(x)
    want = torch.autograd.grad(y, [x, *_params(gru, D)], dy)
    with torch.no_grad():
        h, dx, grads = G.layer_gradients(x.detach(), [p.detach() for p in _params(gru, D)], dy.view(n, T, D, H), H)

    def close(a, b, what):
        tol = 1e-12 * max(1.0, float(b.abs().max()))
        assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)
    close(h.reshape(n, T, D * H), y.detach(), "h")
    close(dx, want[0], "dx")
    for i, (g, w) in enumerate(zip(grads, want[1:])):
        close(g, w, f"parameter {i}")
    for d in range(D):      # the two biases stop sharing a gradient on the n rows (and only there)
        db_ih, db_hh = want[1 + 4 * d + 2], want[1 + 4 * d + 3]
        close(db_ih[:2 * H], db_hh[:2 * H], "db r, z")
        assert float((db_ih[2 * H:] - db_hh[2 * H:]).abs().max()) > 1e-3
        assert float((grads[4 * d + 2][2 * H:] - grads[4 * d + 3][2 * H:]).abs().max()) > 1e-3


def test_loops_carry_an_initial_state_like_torch():
    n, T, I, H = 3, 5, 4, 6
    gru = _gru(I, H, 1, 5)
    gen = torch.Generator().manual_seed(6)
    x, h0 = torch.randn(n, T, I, generator=gen, dtype=torch.float64), torch.randn(n, H, generator=gen, dtype=torch.float64)
    with torch.no_grad():
        y, _ = gru(x, h0[None])
        ps = [p.detach() for p in _params(gru, 1)]
        wih_p, bias_p = G.pack_reference(ps, H)
        gin = (x.reshape(n * T, I) @ wih_p.t() + bias_p).view(n, T, 1, H, 4)
        _, h = G.gru_forward_loop(gin, ps[1::4], H, torch.float64, h0=h0)
    assert float((h[:, :, 0] - y).abs().max()) < 1e-12


def test_pack_reference_layout():
    H, I = 3, 2
    ps = [torch.arange(3 * H * I, dtype=torch.float64).view(3 * H, I) + 1, torch.zeros(3 * H, H),
          torch.arange(3 * H, dtype=torch.float64) + 100, torch.arange(3 * H, dtype=torch.float64) + 1000]
    wih_p, bias_p = G.pack_reference(ps, H)
    w = wih_p.view(H, 4, I)
    assert torch.equal(w[:, 0], ps[0][:H]) and torch.equal(w[:, 1], ps[0][H:2 * H]) and torch.equal(w[:, 2], ps[0][2 * H:])
    assert float(w[:, 3].abs().max()) == 0.0
    b = bias_p.view(H, 4)
    assert torch.equal(b[:, 0], ps[2][:H] + ps[3][:H]) and torch.equal(b[:, 1], ps[2][H:2 * H] + ps[3][H:2 * H])
    assert torch.equal(b[:, 2], ps[2][2 * H:]) and torch.equal(b[:, 3], ps[3][2 * H:])
    blocks = G.hh_blocks(torch.arange(3 * H * H, dtype=torch.float64).view(3 * H, H) + 1, H, torch.float64)
    assert float(blocks[2].abs().max()) == 0.0 and float(blocks[3][0, 0]) == 2 * H * H + 1


# ---- the checkers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    N, T, H = request.param
    gen = torch.Generator().manual_seed(29)
    whh = G.make_gru_whh(H, 2, gen, "cpu")
    gin = torch.randn(N, T, 2, H, 4, generator=gen)
    dh = torch.randn(N, T, 2, H, generator=gen)
    return N, T, H, whh, gin, dh


def _forward(case, defect=None):
    N, T, H, whh, gin, _ = case
    A, h = G.gru_forward_loop(gin, whh, H, torch.float32, defect=defect)
    return G.check_forward(gin, A, G.packed(h, 2 * H + 3, H + 2), whh, H, H + 2)


def _backward(case, defect=None):
    N, T, H, whh, gin, dh = case
    A, h = G.gru_forward_loop(gin, whh, H, torch.float64)
    A, h = A.float(), h.float()
    Dg = G.gru_backward_loop(A, h, dh, whh, H, torch.float32, defect=defect)
    return G.check_backward(A, G.packed(h, 2 * H + 3, H + 2), G.packed(dh, 2 * H + 3, H + 2), Dg, whh, H, H + 2)


def test_fp32_loop_passes_the_bounds(case):
    N, T, H = case[:3]
    f, b = _forward(case), _backward(case)
    print(N, T, H, f, b)
    assert f.ok() and f.count == N * T * 2 * H, str(f)
    assert b.ok() and b.count == N * T * 2 * H * 4, str(b)


def test_bounds_are_not_vacuous(case):
    """the median bound of every output is below 1e-5 (H = 300: one fmaf chain of 300 terms)"""
    f, b = _forward(case), _backward(case)
    for w, names in ((f, ("act", "h")), (b, ("dgates",))):
        for name in names:
            assert w.median(name) < 1e-5, (name, w.median(name))


@pytest.mark.parametrize("defect", ["bhn_outside", "z_swapped"])
def test_planted_forward_defects_fail_the_bounds(case, defect):
    w = _forward(case, defect)
    print(defect, w, w.outside)
    assert not w.ok() and w.ratio["h"] > 1, str(w)


@pytest.mark.parametrize("defect", ["daq_without_r", "hprev_first_frame"])
def test_planted_backward_defects_fail_the_bounds(case, defect):
    w = _backward(case, defect)
    print(defect, w, w.outside)
    assert not w.ok() and w.ratio["dgates"] > 1, str(w)


@pytest.mark.parametrize("N,T,H", SHAPES)
def test_db_hh_taken_from_slot_2_is_caught(N, T, H):
    """the comparison the layer tests make -- the parameter gradient against float64 autograd -- sees the wrong slot"""
    I = 4
    gru = _gru(I, H, 2, 8)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(N, T, I, generator=gen, dtype=torch.float64)
    dy = torch.randn(N, T, 2, H, generator=gen, dtype=torch.float64)
    ps = [p.detach() for p in _params(gru, 2)]
    with torch.no_grad():
        good = G.layer_gradients(x, ps, dy, H)[2]
        bad = G.layer_gradients(x, ps, dy, H, defect="hh_from_slot_2")[2]
    for d in (0, 1):
        g, b = good[4 * d + 3], bad[4 * d + 3]
        assert torch.equal(g[:2 * H], b[:2 * H])
        err = float((g[2 * H:] - b[2 * H:]).abs().max())
        assert err > 1e-3 * float(g.abs().max()), err      # (an fp32 path's error is 1e-6 of it)


# ---- the host side, without a GPU -----------------------------------------------------------------------------------------
def test_entry_points_are_declared_and_planned():
    """(fails on the parent commit) the header declares the GRU entry points, the library exports them, hip_ops wraps them
    and recurrence_plan names the two kernels without reading a policy switch; the LSTM plans are what they were"""
    from tssep_amd import _lib, hip_ops as h
    protos = _lib.parse_header()
    names = {"tssep_gru_pack_sizes", "tssep_gru_pack", "tssep_gru_fwd", "tssep_gru_bwd", "tssep_gru1_fwd", "tssep_gru1_bwd",
             "tssep_gru_unpack"}
    assert names <= set(protos) and all(hasattr(_lib.lib(), n) for n in names)
    assert _lib.lib().tssep_abi_version() == 4
    assert all(callable(getattr(h, n)) for n in ("gru_pack", "gru_fwd", "gru_bwd", "gru_unpack")) and (h.GRU_IH, h.GRU_HH) == (0, 1)
    for want in ("stream", "cluster", "onchip", "auto"):
        old, h.RECURRENCE = h.RECURRENCE, want
        try:
            assert h.recurrence_plan(768, 253, 300, 256, directions=2, cell="gru") == dict.fromkeys(("fwd", "bwd"), ("stream_gru_f32", 0))
            assert h.recurrence_plan(768, 253, 300, 256, directions=1, cell="gru") == dict.fromkeys(("fwd", "bwd"), ("stream1_gru_f32", 0))
            assert h.recurrence_plan(768, 253, 300, 256, directions=1) == dict.fromkeys(("fwd", "bwd"), ("stream1_f32", 0))
            assert h.recurrence_plan(768, 253, 300, 256) == h.recurrence_plan(768, 253, 300, 256, 2, cell="lstm")
        finally:
            h.RECURRENCE = old
    sz = _lib.LstmSizes()
    import ctypes
    assert _lib.lib().tssep_gru_pack_sizes(2, 300, 321, 324, ctypes.byref(sz)) == 0 and sz.bias_p == 2 * 4 * 300
    assert _lib.lib().tssep_gru_pack_sizes(1, 513, 7, 8, ctypes.byref(sz)) == -3


def test_rnnp_layer_takes_a_gru_container_and_its_single_tensor_state():
    from tssep_amd import functional as Fn
    x = torch.zeros(6, 7)
    one, two = torch.nn.GRU(7, 5, batch_first=True), torch.nn.GRU(7, 5, batch_first=True, bidirectional=True)
    with pytest.raises(RuntimeError, match="without gradients"):      # gradients are enabled here; nothing is launched
        Fn.rnnp_layer(x, one, torch.nn.Linear(5, 6), 2, 3, state=torch.zeros(2, 5))
    with torch.no_grad(), pytest.raises(ValueError, match="h0"):
        Fn.rnnp_layer(x, one, torch.nn.Linear(5, 6), 2, 3, state=(torch.zeros(2, 5), torch.zeros(2, 5)))
    with torch.no_grad(), pytest.raises(NotImplementedError):
        Fn.rnnp_layer(x, two, torch.nn.Linear(10, 6), 2, 3, state=torch.zeros(2, 5))


# ---- the restated layer -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("act,combine", [(0, 0), (1, 0), (1, 4)])
def test_restated_layer_equals_torch_gru_linear_tanh(act, combine, D):
    N, T, I, H, hdim = 8, 5, 7, 5, 6
    x, params, dy = G.make_layer_case(N, T, I, H, hdim, D, 0, combine)
    with torch.no_grad():
        mine = G.layer(x, params, dy, N, T, torch.float64, act, combine)
    want = G.torch_layer(x, params, dy, N, T, torch.float64, act, combine)
    assert set(mine) == set(want) == {"y", "x", *G.layer_names(D)}
    for k in want:
        tol = 1e-12 * max(1.0, float(want[k].abs().max()))
        assert float((mine[k] - want[k]).abs().max()) <= tol, k


@pytest.mark.parametrize("D,K", [(1, 0), (1, 4), (2, 4)])
def test_restated_chain_and_chunks_equal_torch(D, K):
    N, T, I, H, hdim = 8, 5, 7, 5, 8
    gen = torch.Generator().manual_seed(77)
    p0, p1 = G.make_layer_params(I, H, hdim, D, gen), G.make_layer_params((K or 1) * hdim, H, hdim, D, gen)
    x, dy = torch.randn(N * T, I, generator=gen), torch.randn(N // (K or 1) * T, hdim, generator=gen)
    with torch.no_grad():
        mine = G.two_layers(x, p0, p1, dy, N, T, K, torch.float64)
    want = G.two_layers(x, p0, p1, dy, N, T, K, torch.float64, by_torch=True)
    for k in want:
        assert float((mine[k] - want[k]).abs().max()) <= 1e-12 * max(1.0, float(want[k].abs().max())), k
    if D == 1:
        with torch.no_grad():
            whole = G.layer_forward(x, p0, N, T, torch.float64, 1)
            for chunks in ([T], [1] * T, [2, 3]):
                y, hT = G.chunked_forward(x, p0, N, T, chunks, torch.float64, 1)
                assert float((y - whole["y"]).abs().max()) < 1e-12 and float((hT - whole["h"][:, -1, 0]).abs().max()) < 1e-12


# ---- the toy chain's yardstick -----------------------------------------------------------------------------------------------
TOY_CHAIN = (8, 5, 7, 5, 8)


def test_one_draw_is_no_yardstick_at_five_units():
    """The fp32 restatement's own element-wise error for ONE tensor of the toy chain, seed by seed: the figure the one-draw
    bound of tests/test_rnnp_layer_reference.py multiplies by MARGIN = 8 moves by more than that margin's half between draws
    of the same shape (measured: 9.5 x over six seeds for dW_hh of layer 0 at D = 2, K = 4; up to 24 x for other tensors),
    and MARGIN x the least of them would refuse the restatement itself at another seed."""
    from test_rnnp_layer_reference import MARGIN, errors
    fig = []
    for seed in G.YARDSTICK_SEEDS:
        x, p0, p1, dy = G.chain_case(*TOY_CHAIN, 4, 2, seed)
        with torch.no_grad():
            r32 = G.two_layers(x, p0, p1, dy, 8, 5, 4, torch.float32)
        r64 = G.two_layers(x, p0, p1, dy, 8, 5, 4, torch.float64, by_torch=True)
        fig.append(errors(r32["0.w_hh"], r64["0.w_hh"])[1])
    print("dW_hh of layer 0, element-wise, seed by seed:", " ".join(f"{v:.2e}" for v in fig))
    assert max(fig) / min(fig) > MARGIN / 2, fig
    yard = G.chain_yardstick(*TOY_CHAIN, 4, 2)
    assert yard["0.w_hh"][1] == max(fig) and all(a > 0 and b > 0 for a, b in yard.values())


@pytest.mark.parametrize("D,K", [(2, 4), (1, 0)])
def test_the_yardstick_over_seeds_keeps_its_teeth(D, K):
    """under the WIDER bound (split-bf16 is not used here: the fp32 one) the float64 chain passes with the margin to spare,
    the fp32 restatement and torch's own fp32 GRU pass, and planted defects of a part in a thousand are refused"""
    x, p0, p1, dy = G.chain_case(*TOY_CHAIN, K, D)
    yard = G.chain_yardstick(*TOY_CHAIN, K, D)
    r64 = G.two_layers(x, p0, p1, dy, 8, 5, K, torch.float64, by_torch=True)
    with torch.no_grad():
        r32 = G.two_layers(x, p0, p1, dy, 8, 5, K, torch.float32)
    t32 = G.two_layers(x, p0, p1, dy, 8, 5, K, torch.float32, by_torch=True)

    def bad(got):
        rep = G.yardstick_report(got, r64, yard, False)
        return [k for k, v in rep.items() if not (v["norm"] <= v["bound_norm"] and v["elem"] <= v["bound_elem"])]
    assert bad(r64) == [] and bad(r32) == [] and bad(t32) == []
    H = 5
    wrong = dict(r64)
    wrong["0.w_hh"] = r64["0.w_hh"].clone()
    wrong["0.w_hh"][2 * H:] *= 1.001                     # the n rows (slot q's): a part in a thousand
    assert bad(wrong) == ["0.w_hh"]
    wrong = dict(r64)
    wrong["1.b_hh"] = r64["1.b_ih"]                      # b_hh's n rows taken from slot 2
    assert bad(wrong) == ["1.b_hh"]
    wrong = dict(r64)
    wrong["x"] = r64["x"] * (1 + 2e-4)
    assert bad(wrong) == ["x"]
