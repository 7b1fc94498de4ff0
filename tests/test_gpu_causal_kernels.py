"""The one-direction streaming recurrence (tssep_lstm1_fwd / _bwd: lstm.hip's kernels instantiated for ONE direction of
time, with an initial and a final state) against float64, through the checkers of tests/test_recurrence_reference.py
unchanged and the `Case` of tests/test_gpu_recurrence_kernels.py (inputs, NaN / sentinel fills, bounds, printing).

1. Step by step.  A bidirectional case's pre-activations gin [N, T, 2, H, 4] are run as TWO one-direction launches: the
   new kernel on gin[:, :, 0] with W_hh of direction 0, and on the time-flipped gin[:, :, 1] with W_hh of direction 1; the
   second result is flipped back and the two are stacked to [N, T, 2, H, 4] -- exactly what the two-direction kernel would
   have written, so check_forward / check_backward (fam = "stream": exact fp32, OCML activations) apply as they are.  Every
   output is written over NaN; the pad columns of the launches' own hout [N, T, Hp + 4] hold a sentinel before and after,
   those of dhout NaN.
2. Whole sequences at (40, 64, 300) against the float64 loop: at most whole_sequence_multiple("stream", H) = 4 times the
   fp32 torch loop's error plus 4 U max|ref|.
3. The state is complete (equalities, bit for bit): at (9, 7, 300) launches split 1|6, 3|4, 6|1 and seven launches of one
   frame, each started from the previous launch's hT, cT, give the gates, cell and hout of the single launch; a null
   state equals an all-zero one; hT / cT are the last frame of hout / cell.
4. Guards: every refused argument set returns its code from the C entry point before any launch.

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report): act 0.49, cell 0.52, h 0.20,
d(gates) 0.49; whole sequences, kernel error / fp32 torch error (allowed 4): act 1.19, cell 0.96, h 0.95, d(gates) 0.96."""
import pytest
import torch

from tssep_amd import _lib, hip_ops as Hop
from test_recurrence_reference import U, _dirs, lstm_backward_loop, lstm_forward_loop, whole_sequence_multiple
from test_gpu_recurrence_kernels import Case, DEV, GIB, NAN, SENT, WORST

pytestmark = pytest.mark.gpu
E_SHAPE, E_ALIGN, E_UNSUPPORTED, E_NULL = -1, -2, -3, -5
EXTRA = 4           # pad columns of the launches' own hout / dhout beyond Hp


@pytest.fixture(autouse=True)
def _device_memory_cap():
    """The GPU is shared: every test here stays under 16 GB of device memory at its peak."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 * GIB, f"peak device memory {peak / GIB:.1f} GiB"


def pack1(whh, H):
    """lstm1_pack of one direction's W_hh (the input weights play no part in the recurrence)"""
    z = torch.zeros(4 * H, 4, device=DEV)
    b = torch.zeros(4 * H, device=DEV)
    return Hop.lstm1_pack([z, whh, b, b], H, 4)


def one_direction_launch(case):
    """-> the `launch` hook of Case.forward / Case.backward: two one-direction launches in place of a two-direction one"""
    N, T, H = case.N, case.T, case.H
    ld1 = case.Hp + EXTRA
    packs = [pack1(w, H) for w in case.whh]

    def launch(fam, bwd, var, gates, cell, h):
        for d in (0, 1):
            flip = (lambda x: x.flip(1)) if d else (lambda x: x)
            g = flip(gates[:, :, d]).contiguous()
            cols = slice(d * case.dstride, d * case.dstride + H)
            if bwd:
                c = flip(cell[:, :, d]).contiguous()
                dh = torch.full((N, T, ld1), NAN, device=DEV)
                dh[..., :H] = flip(h[..., cols])
                Hop.lstm1_bwd(g, c, dh, ld1, packs[d]["whh_b"], N, T, H)
            else:
                c = torch.full((N, T, H), NAN, device=DEV)
                ho = torch.full((N, T, ld1), NAN, device=DEV)
                ho[..., H:] = SENT
                Hop.lstm1_fwd(g, c, ho, ld1, packs[d]["whh_f"], N, T, H)
                assert bool((ho[..., H:] == SENT).all()), "pad columns of hout were written"
                cell[:, :, d] = flip(c)
                h[..., cols] = flip(ho[..., :H])
            gates[:, :, d] = flip(g)
        torch.cuda.synchronize()
    return launch


def _rename(before):
    """the figures Case recorded under ("stream", ...) during one of this file's checks belong to the one-direction kernel"""
    for key in [k for k in WORST if k[0] == "stream"]:
        v = WORST.pop(key)
        WORST[("stream1",) + key[1:]] = max(WORST.get(("stream1",) + key[1:], 0.0), v)
    WORST.update(before)


def _both(c):
    before = {k: v for k, v in WORST.items() if k[0] == "stream"}
    for k in before:
        del WORST[k]
    try:
        launch = one_direction_launch(c)
        out = c.forward("stream", None, launch), c.backward("stream", None, launch)
    finally:
        _rename(before)
    return out


SHAPES = [(1, 1, 5), (1, 5, 5), (8, 7, 300), (9, 7, 300), (9, 3, 303), (9, 5, 305), (9, 5, 512), (17, 2, 12), (3072, 5, 300)]


@pytest.mark.parametrize("N,T,H", SHAPES)
def test_one_direction_step_by_step(N, T, H):
    _both(Case(N, T, H, seed=1))


def test_saturated_gates_and_a_growing_cell_state():
    _both(Case(9, 33, 300, seed=2, klass="big"))


def test_whole_sequences_against_a_float64_loop():
    N, T, H = 40, 64, 300
    c = Case(N, T, H, seed=11)
    M = whole_sequence_multiple("stream", H)
    assert M == 4.0
    gin = torch.cat([c.gin(*b) for b in c.blocks])
    (A, cell, hout), (As, cs, dhout, D) = _both(c)
    ref = lstm_forward_loop(gin, c.whh, H, torch.float64)
    t32 = lstm_forward_loop(gin, c.whh, H, torch.float32)
    dh = _dirs(dhout, H, c.dstride)
    pairs = [(n, k, r, t) for n, k, r, t in zip(("act", "cell", "h"), (A, cell, _dirs(hout, H, c.dstride)), ref, t32)]
    pairs.append(("dgates", D, lstm_backward_loop(As, cs, dh, c.whh, H, torch.float64),
                  lstm_backward_loop(As, cs, dh, c.whh, H, torch.float32)))
    for name, k, r, t in pairs:
        ek, et = float((k.double() - r).abs().max()), float((t.double() - r).abs().max())
        floor = 4 * U * float(r.abs().max())
        print(f"stream1 H={H} {name}: kernel {ek:.3g}, fp32 torch {et:.3g}, ratio {ek / et:.3g} (allowed {M:.3g})")
        WORST[("stream1", "whole", name)] = ek / et
        assert ek <= M * et + floor, (name, ek, et, M)


# ---- the state -------------------------------------------------------------------------------------------------------
def _run(gin, pk, N, T, H, ld, state=None, zeros=False):
    """one launch over gin [N, T, H, 4] -> (gates, cell, hout[..., :H], hT, cT), everything written over NaN"""
    g = gin.contiguous().clone()
    cell = torch.full((N, T, H), NAN, device=DEV)
    hout = torch.full((N, T, ld), NAN, device=DEV)
    hout[..., H:] = SENT
    hT, cT = torch.full((N, H), NAN, device=DEV), torch.full((N, H), NAN, device=DEV)
    if zeros:
        state = (torch.zeros(N, H, device=DEV), torch.zeros(N, H, device=DEV))
    h0, c0 = state if state is not None else (None, None)
    Hop.lstm1_fwd(g, cell, hout, ld, pk["whh_f"], N, T, H, h0, c0, hT, cT)
    torch.cuda.synchronize()
    assert bool((hout[..., H:] == SENT).all())
    return g, cell, hout[..., :H].contiguous(), hT, cT


@pytest.mark.parametrize("N,T,H", [(9, 7, 300), (3, 7, 5)])
def test_the_state_is_complete(N, T, H):
    gen = torch.Generator(device=DEV).manual_seed(5)
    whh = (torch.rand(4 * H, H, device=DEV, generator=gen) * 2 - 1) * H ** -0.5
    pk = pack1(whh, H)
    gin = torch.randn(N, T, H, 4, device=DEV, generator=gen)
    ld = Hop.round_up(H, 4) + EXTRA
    whole = _run(gin, pk, N, T, H, ld)
    assert all(bool(torch.isfinite(x).all()) for x in whole)
    assert torch.equal(whole[3], whole[2][:, -1]) and torch.equal(whole[4], whole[1][:, -1]), "hT / cT: the last frame"
    again = _run(gin, pk, N, T, H, ld, zeros=True)
    assert all(torch.equal(a, b) for a, b in zip(whole, again)), "a null state is an all-zero state"
    for split in ([1, 6], [3, 4], [6, 1], [1] * 7):
        state, parts, t0 = None, [], 0
        for n in split:
            out = _run(gin[:, t0:t0 + n], pk, N, n, H, ld, state)
            state = (out[3], out[4])
            assert torch.equal(out[3], out[2][:, -1]) and torch.equal(out[4], out[1][:, -1])
            parts.append(out[:3])
            t0 += n
        for name, i in (("gates", 0), ("cell", 1), ("hout", 2)):
            got = torch.cat([p[i] for p in parts], 1)
            assert torch.equal(got, whole[i]), (split, name, float((got - whole[i]).abs().max()))
        assert torch.equal(state[0], whole[3]) and torch.equal(state[1], whole[4]), split


def test_pack_is_the_forward_half_of_the_two_direction_pack():
    """lstm1_pack's four layouts are the [dir = 0] halves of lstm_pack's, and lstm1_unpack inverts the gate-row order"""
    H, I = 13, 7
    gen = torch.Generator(device=DEV).manual_seed(3)
    ps = [torch.randn(*s, device=DEV, generator=gen) for s in ((4 * H, I), (4 * H, H), (4 * H,), (4 * H,))] * 2
    two, one = Hop.lstm_pack(ps, H, I), Hop.lstm1_pack(ps[:4], H, I)
    for k in ("wih_p", "bias_p", "whh_f", "whh_b"):
        assert torch.equal(one[k], two[k][:one[k].numel()]), k
    back = torch.full((4 * H, I), NAN, device=DEV)
    Hop.lstm1_unpack(one["wih_p"], one["ld_i"], 1, 0, H, I, back)
    assert torch.equal(back, ps[0])
    Hop.lstm1_unpack(one["wih_p"], one["ld_i"], 1, 0, H, I, back, accumulate=True)
    assert torch.equal(back, 2 * ps[0])


# ---- guards ----------------------------------------------------------------------------------------------------------
def test_guards_decline_before_anything_is_launched():
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    p, odd, s = Hop._p(buf), Hop._p((buf, 1)), Hop._stream()
    N, T, H, ld = 2, 3, 5, 8

    def fwd(gates=p, cell=p, hout=p, ldo=ld, whh=p, h0=None, c0=None, hT=None, cT=None, N=N, T=T, H=H):
        return L.tssep_lstm1_fwd(gates, cell, hout, ldo, whh, h0, c0, hT, cT, N, T, H, s)

    def bwd(gates=p, cell=p, dhout=p, ldo=ld, whh=p, N=N, T=T, H=H):
        return L.tssep_lstm1_bwd(gates, cell, dhout, ldo, whh, N, T, H, s)

    for fn, names in ((fwd, ("gates", "cell", "hout", "whh")), (bwd, ("gates", "cell", "dhout", "whh"))):
        for name in names:
            assert fn(**{name: None}) == E_NULL, (fn.__name__, name)
        for dim in ("N", "T", "H"):
            for v in (0, -1):
                assert fn(**{dim: v}) == E_SHAPE, (fn.__name__, dim, v)
        assert fn(ldo=H - 1) == E_SHAPE
        assert fn(gates=odd) == E_ALIGN and fn(whh=odd) == E_ALIGN
        assert fn(H=513, ldo=516) == E_UNSUPPORTED
    assert fwd(h0=p) == E_NULL and fwd(c0=p) == E_NULL, "h0 without c0"
    sz = _lib.LstmSizes()
    import ctypes
    assert L.tssep_lstm1_pack_sizes(5, 7, 8, None) == E_NULL
    assert L.tssep_lstm1_pack_sizes(0, 7, 8, ctypes.byref(sz)) == E_SHAPE
    assert L.tssep_lstm1_pack_sizes(5, 7, 7, ctypes.byref(sz)) == E_SHAPE
    assert L.tssep_lstm1_pack_sizes(513, 7, 8, ctypes.byref(sz)) == E_UNSUPPORTED
    assert L.tssep_lstm1_pack_sizes(5, 7, 8, ctypes.byref(sz)) == 0 and sz.wih_p == 4 * 5 * 8 and sz.bias_p == 20
    assert L.tssep_lstm1_pack(p, p, p, None, 5, 7, 8, p, p, p, p, s) == E_NULL
    assert L.tssep_lstm1_pack(p, p, p, p, 5, 7, 8, p, p, odd, p, s) == E_ALIGN
    assert L.tssep_lstm1_pack(p, p, p, p, 513, 7, 8, p, p, p, p, s) == E_UNSUPPORTED
    assert L.tssep_lstm1_unpack(None, 8, 1, 0, 5, 7, p, 0, s) == E_NULL
    assert L.tssep_lstm1_unpack(p, 8, 0, 0, 5, 7, p, 0, s) == E_SHAPE
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "a refused call wrote"


def test_launches_are_logged_for_the_kernel_plan():
    H = 5
    pk = pack1(torch.zeros(4 * H, H, device=DEV), H)
    log = Hop.RECURRENCE_LOG = []
    try:
        g, c, h = torch.zeros(2, 3, H, 4, device=DEV), torch.zeros(2, 3, H, device=DEV), torch.zeros(2, 3, 8, device=DEV)
        Hop.lstm1_fwd(g, c, h, 8, pk["whh_f"], 2, 3, H)
        Hop.lstm1_bwd(g, c, h, 8, pk["whh_b"], 2, 3, H)
    finally:
        Hop.RECURRENCE_LOG = None
    assert [(e["kernel"], e["direction"], e["sequences"], e["frames"], e["units"]) for e in log] == \
        [("stream1_f32", "fwd", 2, 3, H), ("stream1_f32", "bwd", 2, 3, H)]


def test_zz_report():
    """the largest error / bound of every output this run saw (pytest -rP)"""
    for (fam, direction, name), v in sorted(WORST.items()):
        if fam == "stream1":
            print(f"{fam:8s} {direction:6s} {name:7s} {v:.3g}")
