"""The GRU streaming recurrences (tssep_gru_fwd / _bwd, tssep_gru1_fwd / _bwd: gru.hip's kernels for two directions of time
and for one, the latter with an initial and a final state), their pack and their gradient unpack, against the float64
references and the bounds of tests/gru_reference.py (derivations there).

1. Step by step, forward and backward, ND = 1 and ND = 2: N in {1, 8, 9} (the 8-sequence workgroup boundary), T in {1, 2, 7},
   H in {5, 64, 65, 300} (below one MFMA block with H % 4 != 0; the NB / NBB boundary; the model's size), H = 321, 449 and
   512 (NB = 6 and 8, the largest accepted width), and one case of
   saturated gates (pre-activations of +-30).  Every output is written over NaN; the pad columns of hout hold a sentinel
   before and after, those of dhout NaN.  ND = 1 also from a non-zero initial state.
2. The ND = 2 launch equals, bit for bit, two ND = 1 launches, the second on the time-flipped tensors.
3. Whole sequences at (40, 64, 300) against the float64 loop: at most whole_sequence_multiple("stream", H) = 4 times the
   error of the fp32 torch loop of the same formula plus 4 U max|ref|.
4. The state is complete (equalities, bit for bit): at (9, 7, 300) and (3, 7, 5) launches split 1|6, 3|4, 6|1 and seven
   launches of one frame, each started from the previous launch's hT, give the gates and hout of the single launch; a null
   h0 equals zeros; hT is the last frame of hout.
5. Pack and unpack: the packed layouts against gru_reference.pack_reference / hh_blocks, bit for bit; pack -> unpack
   round-trips torch's matrices with which = ih / hh; the zero slots are zero and bias_p's slot 3 is b_hn.
6. Guards: every refused argument set returns its code from the C entry point before any launch; the launches are logged.

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report): ND = 1 act 0.41, h 0.55,
d(gates) 0.32; ND = 2 act 0.42, h 0.48, d(gates) 0.37; whole sequences, kernel error / fp32 torch error (allowed 4): ND = 1
act 0.87, h 0.85, d(gates) 1.11; ND = 2 act 0.93, h 1.07, d(gates) 1.06."""
import ctypes

import pytest
import torch

import gru_reference as G
from tssep_amd import _lib, hip_ops as Hop
from test_recurrence_reference import U, whole_sequence_multiple
from test_gpu_recurrence_kernels import DEV, GIB, NAN, SENT

pytestmark = pytest.mark.gpu
E_SHAPE, E_ALIGN, E_UNSUPPORTED, E_NULL = -1, -2, -3, -5
EXTRA = 4           # pad columns of hout / dhout beyond the directions' blocks
WORST = {}          # (nd, direction, output) -> largest error / bound of this run


@pytest.fixture(autouse=True)
def _device_memory_cap():
    """The GPU is shared: every test here stays under 16 GB of device memory at its peak."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 * GIB, f"peak device memory {peak / GIB:.1f} GiB"


def pack(whh, H):
    """gru_pack of the directions' W_hh (the input weights play no part in the recurrence)"""
    z, b = torch.zeros(3 * H, 4, device=DEV), torch.zeros(3 * H, device=DEV)
    return Hop.gru_pack([t for w in whh for t in (z, w, b, b)], H, 4)


class Case:
    """Inputs of one launch over D directions.  klass "sat": every pre-activation is +30 or -30."""

    def __init__(self, N, T, H, D, seed=0, klass="randn"):
        self.N, self.T, self.H, self.D = N, T, H, D
        gen = torch.Generator(device=DEV).manual_seed(1000 * seed + 7 * N + 3 * T + H + D)
        self.whh = G.make_gru_whh(H, D, gen, DEV)
        self.gin = torch.randn(N, T, D, H, 4, device=DEV, generator=gen)
        if klass == "sat":
            self.gin = 30.0 * torch.sign(self.gin)
        self.dh = torch.randn(N, T, D, H, device=DEV, generator=gen)
        self.h0 = torch.randn(N, H, device=DEV, generator=gen) if D == 1 else None
        self.Hp = Hop.round_up(H, 4)
        self.dstride, self.ldo = self.Hp, D * self.Hp + EXTRA
        self.pk = pack(self.whh, H)

    def pads(self, h):
        """the columns of an hout-layout tensor that belong to no direction"""
        keep = torch.ones(self.ldo, dtype=torch.bool, device=DEV)
        for d in range(self.D):
            keep[d * self.dstride:d * self.dstride + self.H] = False
        return h[..., keep]

    def forward(self, h0=None):
        """-> (gates, hout) of one launch, everything written over NaN, sentinels in hout's pad columns"""
        N, T, H, D = self.N, self.T, self.H, self.D
        gates = self.gin.clone()
        hout = torch.full((N, T, self.ldo), SENT, device=DEV)
        for d in range(D):
            hout[..., d * self.dstride:d * self.dstride + H] = NAN
        Hop.gru_fwd(gates, hout, self.ldo, self.dstride, self.pk["whh_f"], N, T, H, directions=D, h0=h0)
        torch.cuda.synchronize()
        assert bool((self.pads(hout) == SENT).all()), "pad columns of hout were written"
        return gates, hout

    def backward(self, A, hout):
        """-> (dhout as read, d(gates)) of one launch on the saved A, hout"""
        N, T, H, D = self.N, self.T, self.H, self.D
        dhout = G.packed(self.dh, self.ldo, self.dstride, fill=NAN)
        Dg = A.clone()
        Hop.gru_bwd(Dg, hout, dhout, self.ldo, self.dstride, self.pk["whh_b"], N, T, H, directions=D)
        torch.cuda.synchronize()
        return dhout, Dg

    def check(self, h0=None):
        N, T, H, D = self.N, self.T, self.H, self.D
        A, hout = self.forward(h0)
        wf = G.check_forward(self.gin, A, hout, self.whh, H, self.dstride, h0=h0)
        print(f"gru{D} fwd N={N} T={T} H={H}: {wf}")
        assert wf.ok() and wf.count == N * T * D * H, str(wf)
        out = [A, hout]
        if h0 is None:      # (the backward assumes a zero initial state)
            dhout, Dg = self.backward(A, hout)
            wb = G.check_backward(A, hout, torch.nan_to_num(dhout), Dg, self.whh, H, self.dstride)
            print(f"gru{D} bwd N={N} T={T} H={H}: {wb}")
            assert wb.ok() and wb.count == N * T * D * H * 4, str(wb)
            out += [dhout, Dg]
            wf.ratio.update(wb.ratio)
        for name, v in wf.ratio.items():
            WORST[(D, "step", name)] = max(WORST.get((D, "step", name), 0.0), v)
        return out


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("H", [5, 64, 65, 300])
@pytest.mark.parametrize("T", [1, 2, 7])
@pytest.mark.parametrize("N", [1, 8, 9])
def test_step_by_step(N, T, H, D):
    Case(N, T, H, D, seed=1).check()


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("N,T,H", [(9, 2, 512), (9, 2, 449), (8, 1, 321)])
def test_step_by_step_past_the_model_width(N, T, H, D):
    """the instantiations NB = 8 at the largest H the entry points accept (the backward's 133 KB of LDS), NB = 8 with
    H % 4 != 0 and a ragged last block, and NB = 6, the first past H = 320"""
    Case(N, T, H, D, seed=5).check()


@pytest.mark.parametrize("D", [1, 2])
def test_saturated_gates(D):
    Case(9, 7, 300, D, seed=2, klass="sat").check()


@pytest.mark.parametrize("N,T,H", [(9, 7, 300), (3, 2, 5)])
def test_one_direction_from_an_initial_state(N, T, H):
    c = Case(N, T, H, 1, seed=3)
    c.check(h0=c.h0)


@pytest.mark.parametrize("N,T,H", [(9, 7, 300), (8, 2, 65), (1, 1, 5), (9, 7, 64)])
def test_two_directions_equal_two_one_direction_launches(N, T, H):
    c = Case(N, T, H, 2, seed=4)
    A, hout = c.forward()
    dhout, Dg = c.backward(A, hout)
    ld1 = c.Hp + EXTRA
    for d in (0, 1):
        flip = (lambda x: x.flip(1)) if d else (lambda x: x)
        pk = pack([c.whh[d]], H)
        cols = slice(d * c.dstride, d * c.dstride + H)
        g = flip(c.gin[:, :, d]).contiguous()
        ho = torch.full((N, T, ld1), SENT, device=DEV)
        ho[..., :H] = NAN
        Hop.gru_fwd(g, ho, ld1, 0, pk["whh_f"], N, T, H, directions=1)
        assert bool((ho[..., H:] == SENT).all()), "pad columns of hout were written"
        assert torch.equal(flip(g), A[:, :, d]) and torch.equal(flip(ho[..., :H]), hout[..., cols]), ("forward", d)
        dh = torch.full((N, T, ld1), NAN, device=DEV)
        dh[..., :H] = flip(dhout[..., cols])
        Hop.gru_bwd(g, ho, dh, ld1, 0, pk["whh_b"], N, T, H, directions=1)
        assert torch.equal(flip(g), Dg[:, :, d]), ("backward", d)


@pytest.mark.parametrize("D", [1, 2])
def test_whole_sequences_against_a_float64_loop(D):
    N, T, H = 40, 64, 300
    c = Case(N, T, H, D, seed=11)
    M = whole_sequence_multiple("stream", H)
    assert M == 4.0
    A, hout, dhout, Dg = c.check()
    h = G.dirs(hout, H, c.dstride, D)
    ref = G.gru_forward_loop(c.gin, c.whh, H, torch.float64)
    t32 = G.gru_forward_loop(c.gin, c.whh, H, torch.float32)
    pairs = [(n, k, r, t) for n, k, r, t in zip(("act", "h"), (A, h), ref, t32)]
    pairs.append(("dgates", Dg, G.gru_backward_loop(A, h, c.dh, c.whh, H, torch.float64),
                  G.gru_backward_loop(A, h, c.dh, c.whh, H, torch.float32)))
    for name, k, r, t in pairs:
        ek, et = float((k.double() - r).abs().max()), float((t.double() - r).abs().max())
        floor = 4 * U * float(r.abs().max())
        print(f"gru{D} H={H} {name}: kernel {ek:.3g}, fp32 torch {et:.3g}, ratio {ek / et:.3g} (allowed {M:.3g})")
        WORST[(D, "whole", name)] = ek / et
        assert ek <= M * et + floor, (name, ek, et, M)


# ---- the state -------------------------------------------------------------------------------------------------------
def _run(gin, pk, N, T, H, ld, h0=None, zeros=False):
    """one launch over gin [N, T, H, 4] -> (gates, hout[..., :H], hT), everything written over NaN"""
    g = gin.contiguous().clone()
    hout = torch.full((N, T, ld), NAN, device=DEV)
    hout[..., H:] = SENT
    hT = torch.full((N, H), NAN, device=DEV)
    if zeros:
        h0 = torch.zeros(N, H, device=DEV)
    Hop.gru_fwd(g, hout, ld, 0, pk["whh_f"], N, T, H, directions=1, h0=h0, hT=hT)
    torch.cuda.synchronize()
    assert bool((hout[..., H:] == SENT).all())
    return g, hout[..., :H].contiguous(), hT


@pytest.mark.parametrize("N,T,H", [(9, 7, 300), (3, 7, 5)])
def test_the_state_is_complete(N, T, H):
    gen = torch.Generator(device=DEV).manual_seed(5)
    pk = pack(G.make_gru_whh(H, 1, gen, DEV), H)
    gin = torch.randn(N, T, H, 4, device=DEV, generator=gen)
    ld = Hop.round_up(H, 4) + EXTRA
    whole = _run(gin, pk, N, T, H, ld)
    assert all(bool(torch.isfinite(x).all()) for x in whole)
    assert torch.equal(whole[2], whole[1][:, -1]), "hT: the last frame"
    again = _run(gin, pk, N, T, H, ld, zeros=True)
    assert all(torch.equal(a, b) for a, b in zip(whole, again)), "a null state is an all-zero state"
    for split in ([1, 6], [3, 4], [6, 1], [1] * 7):
        state, parts, t0 = None, [], 0
        for n in split:
            out = _run(gin[:, t0:t0 + n], pk, N, n, H, ld, state)
            state = out[2]
            assert torch.equal(out[2], out[1][:, -1])
            parts.append(out[:2])
            t0 += n
        for name, i in (("gates", 0), ("hout", 1)):
            got = torch.cat([p[i] for p in parts], 1)
            assert torch.equal(got, whole[i]), (split, name, float((got - whole[i]).abs().max()))
        assert torch.equal(state, whole[2]), split


# ---- pack and unpack ---------------------------------------------------------------------------------------------------
def _layout_f(blocks, H):
    """[4 slots, H, H] -> whh_f [wave 4][kq][i NB][lane 64][4] of one direction (include/tssep_hip.h)"""
    NB, KQ3 = ((H + 15) // 16 + 3) // 4, (((H + 3) // 4 + 2) // 3) * 3
    pad = torch.zeros(4, 4 * NB * 16, 4 * KQ3, device=blocks.device)
    pad[:, :H, :H] = blocks
    # [slot, wave, i, ub, kq, e] -> [wave, kq, i, ub, slot, e]
    return pad.view(4, 4, NB, 16, KQ3, 4).permute(1, 4, 2, 3, 0, 5).reshape(-1)


def _layout_b(blocks, H):
    """[4 slots, H(row kk), H(unit)] -> whh_b [slot 4][kq][ubb NBB][lane 64][4] = W_slot[4 kq + e][ubb 64 + lane]"""
    NBB, KQ3 = (H + 63) // 64, (((H + 3) // 4 + 2) // 3) * 3
    pad = torch.zeros(4, 4 * KQ3, NBB * 64, device=blocks.device)
    pad[:, :H, :H] = blocks
    # [slot, kq, e, ubb, lane] -> [slot, kq, ubb, lane, e]
    return pad.view(4, KQ3, 4, NBB, 64).permute(0, 1, 3, 4, 2).reshape(-1)


@pytest.mark.parametrize("D", [1, 2])
@pytest.mark.parametrize("H,I", [(13, 7), (65, 8), (300, 5)])
def test_pack_and_unpack(H, I, D):
    gen = torch.Generator(device=DEV).manual_seed(3)
    ps = [torch.randn(*s, device=DEV, generator=gen) for _ in range(D) for s in ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,))]
    pk = Hop.gru_pack(ps, H, I)
    ld_i = pk["ld_i"]
    wih_ref, bias_ref = G.pack_reference(ps, H)
    wih_p = pk["wih_p"].view(D * 4 * H, ld_i)
    assert torch.equal(wih_p[:, :I], wih_ref) and float(wih_p[:, I:].abs().max() if ld_i > I else 0.0) == 0.0
    assert torch.equal(pk["bias_p"], bias_ref)
    assert float(wih_p.view(D, H, 4, ld_i)[:, :, 3].abs().max()) == 0.0, "slot 3 of wih_p"
    for d in range(D):
        assert torch.equal(pk["bias_p"].view(D, H, 4)[d, :, 3], ps[4 * d + 3][2 * H:]), "bias_p slot 3 is b_hn"
        blocks = G.hh_blocks(ps[4 * d + 1], H, torch.float32)
        f, b = _layout_f(blocks, H), _layout_b(blocks, H)
        assert torch.equal(pk["whh_f"].view(D, -1)[d], f) and torch.equal(pk["whh_b"].view(D, -1)[d], b), d
        assert float(pk["whh_b"].view(D, 4, -1)[d, 2].abs().max()) == 0.0, "slot 2 of the BPTT layout"
        lanes = pk["whh_f"].view(D, -1, 64, 4)[d]
        assert float(lanes[:, 2::4].abs().max()) == 0.0, "slot 2 of the forward layout"
    # unpack: the input side reads the slots (0, 1, 2), the hidden side (0, 1, 3); the other slot's row is junk
    src = torch.randn(D * 4 * H, ld_i, device=DEV, generator=gen)
    for which, name in ((Hop.GRU_IH, "ih"), (Hop.GRU_HH, "hh")):
        want = G.unpack_reference(src[:, :I].contiguous(), H, name)
        dst = [torch.full((3 * H, I), NAN, device=DEV) for _ in range(D)]
        Hop.gru_unpack(src, ld_i, 1, 0, H, I, which, *dst)
        assert all(torch.equal(a, b) for a, b in zip(dst, want)), name
        Hop.gru_unpack(src, ld_i, 1, 0, H, I, which, *dst, accumulate=True)
        assert all(torch.equal(a, 2 * b) for a, b in zip(dst, want)), name
    # round trips: W_ih through wih_p, b_hh's n rows and W_hh through a [D 4H, H] matrix of the four blocks
    back = [torch.full((3 * H, I), NAN, device=DEV) for _ in range(D)]
    Hop.gru_unpack(pk["wih_p"], ld_i, 1, 0, H, I, Hop.GRU_IH, *back)
    assert all(torch.equal(back[d], ps[4 * d]) for d in range(D))
    rows = torch.cat([G.hh_blocks(ps[4 * d + 1], H, torch.float32).permute(1, 0, 2).reshape(4 * H, H) for d in range(D)])
    rows.view(D, H, 4, H)[:, :, 2] = NAN                  # never read
    back = [torch.full((3 * H, H), NAN, device=DEV) for _ in range(D)]
    Hop.gru_unpack(rows, H, 1, 0, H, H, Hop.GRU_HH, *back)
    assert all(torch.equal(back[d], ps[4 * d + 1]) for d in range(D))
    # the split-K reduction: two splits summed
    two = torch.stack([src, 2 * src])
    dst = [torch.full((3 * H, I), NAN, device=DEV) for _ in range(D)]
    Hop.gru_unpack(two, ld_i, 2, src.numel(), H, I, Hop.GRU_HH, *dst)
    want = G.unpack_reference(src[:, :I].contiguous(), H, "hh")
    assert all(torch.equal(a, b + 2 * b) for a, b in zip(dst, want))


# ---- guards ----------------------------------------------------------------------------------------------------------
def test_guards_decline_before_anything_is_launched():
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    p, odd, s = Hop._p(buf), Hop._p((buf, 1)), Hop._stream()
    N, T, H, ld = 2, 3, 5, 20

    def fwd2(gates=p, hout=p, ldo=ld, dstride=8, whh=p, N=N, T=T, H=H):
        return L.tssep_gru_fwd(gates, hout, ldo, dstride, whh, N, T, H, s)

    def bwd2(gates=p, hout=p, dhout=p, ldo=ld, dstride=8, whh=p, N=N, T=T, H=H):
        return L.tssep_gru_bwd(gates, hout, dhout, ldo, dstride, whh, N, T, H, s)

    def fwd1(gates=p, hout=p, ldo=ld, whh=p, h0=None, hT=None, N=N, T=T, H=H):
        return L.tssep_gru1_fwd(gates, hout, ldo, whh, h0, hT, N, T, H, s)

    def bwd1(gates=p, hout=p, dhout=p, ldo=ld, whh=p, N=N, T=T, H=H):
        return L.tssep_gru1_bwd(gates, hout, dhout, ldo, whh, N, T, H, s)

    for fn, names in ((fwd2, ("gates", "hout", "whh")), (bwd2, ("gates", "hout", "dhout", "whh")),
                      (fwd1, ("gates", "hout", "whh")), (bwd1, ("gates", "hout", "dhout", "whh"))):
        for name in names:
            assert fn(**{name: None}) == E_NULL, (fn.__name__, name)
        for dim in ("N", "T", "H"):
            for v in (0, -1):
                assert fn(**{dim: v}) == E_SHAPE, (fn.__name__, dim, v)
        assert fn(ldo=H - 1) == E_SHAPE
        assert fn(gates=odd) == E_ALIGN and fn(whh=odd) == E_ALIGN
    for fn in (fwd2, bwd2):
        assert fn(dstride=H - 1) == E_SHAPE and fn(ldo=8 + H - 1) == E_SHAPE
        assert fn(H=513, dstride=516, ldo=1032) == E_UNSUPPORTED
    for fn in (fwd1, bwd1):
        assert fn(H=513, ldo=516) == E_UNSUPPORTED
    sz = _lib.LstmSizes()
    ref = ctypes.byref(sz)
    assert L.tssep_gru_pack_sizes(1, 5, 7, 8, None) == E_NULL
    for args in ((0, 5, 7, 8), (3, 5, 7, 8), (1, 0, 7, 8), (1, 5, 0, 8), (1, 5, 7, 7), (2, 5, 7, 6)):
        assert L.tssep_gru_pack_sizes(*args, ref) == E_SHAPE, args
    assert L.tssep_gru_pack_sizes(1, 513, 7, 8, ref) == E_UNSUPPORTED
    assert L.tssep_gru_pack_sizes(1, 5, 7, 8, ref) == 0 and sz.wih_p == 4 * 5 * 8 and sz.bias_p == 20
    assert L.tssep_gru_pack_sizes(2, 5, 7, 8, ref) == 0 and sz.wih_p == 2 * 4 * 5 * 8 and sz.bias_p == 40
    assert L.tssep_gru_pack(1, p, p, p, None, None, None, None, None, 5, 7, 8, p, p, p, p, s) == E_NULL
    assert L.tssep_gru_pack(2, p, p, p, p, p, p, p, None, 5, 7, 8, p, p, p, p, s) == E_NULL
    assert L.tssep_gru_pack(1, p, p, p, p, None, None, None, None, 5, 7, 8, p, p, odd, p, s) == E_ALIGN
    assert L.tssep_gru_pack(1, p, p, p, p, None, None, None, None, 513, 7, 8, p, p, p, p, s) == E_UNSUPPORTED
    assert L.tssep_gru_pack(3, p, p, p, p, p, p, p, p, 5, 7, 8, p, p, p, p, s) == E_SHAPE
    assert L.tssep_gru_unpack(1, None, 8, 1, 0, 5, 7, 0, p, None, 0, s) == E_NULL
    assert L.tssep_gru_unpack(2, p, 8, 1, 0, 5, 7, 0, p, None, 0, s) == E_NULL
    assert L.tssep_gru_unpack(1, p, 8, 0, 0, 5, 7, 0, p, None, 0, s) == E_SHAPE
    assert L.tssep_gru_unpack(1, p, 8, 1, 0, 5, 7, 2, p, None, 0, s) == E_SHAPE, "which"
    assert L.tssep_gru_unpack(0, p, 8, 1, 0, 5, 7, 0, p, None, 0, s) == E_SHAPE
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "a refused call wrote"


def test_launches_are_logged_for_the_kernel_plan():
    H = 5
    log = Hop.RECURRENCE_LOG = []
    try:
        for D in (1, 2):
            pk = pack([torch.zeros(3 * H, H, device=DEV)] * D, H)
            g, h = torch.zeros(2, 3, D, H, 4, device=DEV), torch.zeros(2, 3, 16, device=DEV)
            Hop.gru_fwd(g, h, 16, 8, pk["whh_f"], 2, 3, H, directions=D)
            Hop.gru_bwd(g, h, h.clone(), 16, 8, pk["whh_b"], 2, 3, H, directions=D)
    finally:
        Hop.RECURRENCE_LOG = None
    assert [(e["kernel"], e["direction"], e["sequences"], e["frames"], e["units"]) for e in log] == \
        [("stream1_gru_f32", "fwd", 2, 3, H), ("stream1_gru_f32", "bwd", 2, 3, H),
         ("stream_gru_f32", "fwd", 2, 3, H), ("stream_gru_f32", "bwd", 2, 3, H)]
    cus = Hop.n_cus(torch.device(DEV, torch.cuda.current_device()))
    assert Hop.recurrence_plan(768, 253, 300, cus, directions=1, cell="gru") == dict.fromkeys(("fwd", "bwd"), ("stream1_gru_f32", 0))
    assert Hop.recurrence_plan(768, 253, 300, cus, directions=2, cell="gru") == dict.fromkeys(("fwd", "bwd"), ("stream_gru_f32", 0))
    assert Hop.recurrence_plan(768, 253, 300, cus, directions=1) == Hop.recurrence_plan(768, 253, 300, cus, 1, cell="lstm")


def test_zz_report():
    """the largest error / bound of every output this run saw (pytest -rP; the module docstring has an MI355X's figures)"""
    for (nd, kind, name), v in sorted(WORST.items()):
        print(f"gru{nd} {kind:6s} {name:7s} {v:.3g}")
