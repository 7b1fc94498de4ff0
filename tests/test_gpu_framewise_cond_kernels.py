"""The conditioning kernels for frame-wise embeddings -- tssep_cond_mul_t_fwd / _bwd, tssep_cond_cat_t_fwd,
tssep_cond_mul_aux_t_bwd / tssep_cond_cat_aux_t_bwd (csrc/elementwise.hip, csrc/aux.hip) -- through the C ABI, element by
element against the float64 restatements and bounds of tests/framewise_reference.py, computed on the device.

    base cases     B = 2, K = 3, T = 7; trials in {1, 2}; stride in {1, 2, 3, 7, 8} (8 > T: Ta = 1); mul F in {5, 8, 1028}
                   (4-byte path when dense, 16-byte path, behind the forward's 16-byte limit of 1024), cat F = 5 with
                   E in {3, 4, 100}; four layouts: rows padded to 4 floats, 4 floats wider, dense (ld = width), and every
                   pointer one float behind a 16-byte boundary
    past the grid  T = 2741 (prime): 32 892 forward rows and 16 446 one-frame buckets for each of the four d(aux) kernels (a
                   pass is 16 384 waves), 1 052 544 float4 items and 1 058 026 floats of d(pre), 1 052 544 elements of the cat
                   forward and 1 049 760 elements of the d(aux) reduce kernel (a pass is 1 048 576)
    outputs        start as NaN with a sentinel in their pad columns; the 16-byte mul kernels write the pad columns of a row
                   rounded to 4 floats (products of the inputs' zero pads), as their utterance-level neighbours do; nothing
                   else may be touched; the d(aux) kernels get NaN in every input column they must not read
    workspace      d(aux) with buckets longer than 16 frames (T = 40, strides 17, 33, 40; a shorter last bucket): the two-launch
                   path in its 16-byte and 4-byte forms, mul and cat, a NaN-filled workspace, two runs with the same bits
    stride >= T    forward and d(pre) against tssep_cond_mul_fwd / _bwd / tssep_cond_cat_fwd on the same buffers: bit for bit;
                   a time-constant aux at strides 1 and 3 as well; d(aux) inside the bound, two runs bit for bit alike
    bad shapes     Ta != ceil(T / stride), stride < 1: TSSEP_E_SHAPE from all entry points, nothing written
"""
import math

import pytest
import torch

import framewise_reference as R
from test_gpu_aux_kernels import NAN, buf, load, pads_untouched
from test_gpu_stft_kernels import Ratios

pytestmark = pytest.mark.gpu

DEV = "cuda"
E_SHAPE = -1
B, K, T = 2, 3, 7
STRIDES = (1, 2, 3, 7, 8)
LAYOUTS = ("padded", "wide", "dense", "offset")
MUL_F = (5, 8, 1028)
CAT_FE = ((5, 3), (5, 4), (5, 100))
WAVE_PASS, ITEM_PASS = 4096 * 4, 4096 * 256        # grid_for: one pass of a wave-per-row kernel, of a thread-per-item kernel
# (mul, B, K, trials, T, F, E, stride, layout)
PAST = [(True, 2, 3, 2, 2741, 8, 8, 1, "padded"), (True, 2, 3, 1, 2741, 768, 768, 3, "padded"),
        (True, 2, 3, 1, 2741, 193, 193, 17, "dense"), (False, 2, 3, 1, 2741, 60, 4, 5, "padded"),
        # the other three instantiations of the d(aux) kernel past one pass of waves, and the two-launch path with its
        # reduce kernel past one pass of items
        (True, 2, 3, 1, 2741, 5, 5, 1, "dense"), (False, 2, 3, 1, 2741, 60, 4, 1, "padded"), (False, 2, 3, 1, 2741, 5, 3, 1, "offset"),
        (True, 2, 3, 1, 2741, 1080, 1080, 17, "padded")]
# the two-launch d(aux) path: buckets longer than the 16 frames one wave adds -> workspace + reduce kernel
LONG_T, LONG_STRIDES = 40, (17, 33, 40)           # buckets of 17 + 17 + 6, 33 + 7, 40 frames: 2, 3 and 3 chunks
LONG_SHAPES = [(True, 5, 5), (True, 8, 8), (False, 5, 3), (False, 5, 4), (False, 5, 100)]

WORST = Ratios()


def H():
    from tssep_amd import hip_ops
    return hip_ops


def L():
    from tssep_amd import _lib
    return _lib.lib()


def _p(t):
    return H()._p(t)


def r4(n):
    return (n + 3) // 4 * 4


def layout(width, how):
    """-> (ld, offset in floats)"""
    return {"padded": (r4(width), 0), "wide": (r4(width) + 4, 0), "dense": (width, 0), "offset": (r4(width), 1)}[how]


def is_vec(*lds_offs, width):
    return all(ld % 4 == 0 and ld >= r4(width) and off == 0 for ld, off in lds_offs)


class Case:
    """One shape in one layout: the inputs in device buffers, the float64 references and bounds."""

    def __init__(self, mul, B, K, trials, T, F, E, stride, how, seed, const=False, data=None):
        self.mul, self.dims, self.stride, self.how = mul, (B, K, trials, T, F, E), stride, how
        self.Ta = R.frames_of(T, stride)
        self.C, self.W = (F, F) if mul else (E, F + E)
        pre, aux, dxs = data or R.inputs(B, K, trials, T, F, E, mul, stride, seed, DEV)
        if const:
            aux = aux[:, :, :1].expand(-1, -1, self.Ta, -1).contiguous()
        self.pre, self.aux, self.dxs = pre, aux, dxs
        (self.ld_p, self.o_p), (self.ld_a, self.o_a), (self.ld_x, self.o_x) = layout(F, how), layout(self.C, how), layout(self.W, how)
        self.pv = load(pre.view(B * T, F), self.ld_p, offset=self.o_p)
        self.av = load(aux.reshape(B * K * self.Ta, self.C), self.ld_a, offset=self.o_a)
        self.rows = B * trials * K * T

    def dxs_view(self, pad=0.0):
        v = load(self.dxs.view(self.rows, self.W), self.ld_x, pad=pad, offset=self.o_x)
        if pad != 0.0 and not self.mul:
            F = self.dims[4]
            v[:, F // 4 * 4:F] = pad
        return v

    def fwd(self, utterance=False):
        B, K, trials, T, F, E = self.dims
        xs = buf(self.rows, self.ld_x, self.W, offset=self.o_x)
        s = H()._stream()
        tail = () if utterance else (self.Ta, self.stride)
        if self.mul:
            f = L().tssep_cond_mul_fwd if utterance else L().tssep_cond_mul_t_fwd
            rc = f(_p(self.pv), self.ld_p, _p(self.av), self.ld_a, _p(xs), self.ld_x, B, K, T, F, trials, *tail, s)
        else:
            f = L().tssep_cond_cat_fwd if utterance else L().tssep_cond_cat_t_fwd
            rc = f(_p(self.pv), self.ld_p, _p(self.av), self.ld_a, _p(xs), self.ld_x, B, K, T, F, E, trials, *tail, s)
        assert rc == 0, rc
        return xs

    def dpre(self, utterance=False):
        """mul only (d(pre) of cat does not read the embedding: tssep_cond_cat_bwd serves it)"""
        B, K, trials, T, F, E = self.dims
        dv = self.dxs_view()
        out = buf(B * T, self.ld_p, F, offset=self.o_p)
        tail = () if utterance else (self.Ta, self.stride)
        f = L().tssep_cond_mul_bwd if utterance else L().tssep_cond_mul_t_bwd
        rc = f(_p(dv), self.ld_x, _p(self.av), self.ld_a, _p(out), self.ld_p, B, K, T, F, trials, *tail, H()._stream())
        assert rc == 0, rc
        return out

    def daux(self):
        """dxs and pre carry NaN in every column the kernels must not read; d_aux has ld = C + 1 and starts as NaN, and so
        does the workspace"""
        B, K, trials, T, F, E = self.dims
        dv = self.dxs_view(pad=NAN)
        pv = load(self.pre.view(B * T, F), self.ld_p, pad=NAN, offset=self.o_p) if self.mul else None
        nbytes = int(L().tssep_cond_aux_t_bwd_workspace_bytes(B, K, T, F, 0 if self.mul else E, self.Ta, self.stride))
        assert nbytes >= 0 and (nbytes == 0) == (min(self.stride, T) <= 16), nbytes
        ws = torch.full((nbytes // 4,), NAN, device=DEV) if nbytes else None
        out = buf(B * K * self.Ta, self.C + 1, self.C)
        s = H()._stream()
        if self.mul:
            rc = L().tssep_cond_mul_aux_t_bwd(_p(dv), self.ld_x, _p(pv), self.ld_p, _p(out), self.C + 1, _p(ws), B, K, T, F, trials,
                                              self.Ta, self.stride, s)
        else:
            rc = L().tssep_cond_cat_aux_t_bwd(_p(dv), self.ld_x, _p(out), self.C + 1, _p(ws), B, K, T, F, E, trials, self.Ta,
                                              self.stride, s)
        assert rc == 0, rc
        assert pads_untouched(out, self.C)
        return out[:, :self.C].reshape(B, K, self.Ta, self.C), (dv, pv)

    # ---- checks
    def check_fwd(self, xs):
        B, K, trials, T, F, E = self.dims
        want = R.cond_fwd(self.pre, self.aux, self.mul, trials, self.stride).float().view(self.rows, self.W)
        assert torch.equal(xs[:, :self.W], want), (self.dims, self.stride, self.how, int((xs[:, :self.W] != want).sum()))
        vec = self.mul and F <= 1024 and is_vec((self.ld_p, self.o_p), (self.ld_a, self.o_a), (self.ld_x, self.o_x), width=F)
        self.check_pads(xs, self.W, vec)

    def check_pads(self, out, width, vec):
        if vec:                  # the row rounded to 4 floats is written: products / sums of the inputs' zero pads
            assert bool((out[:, width:r4(width)] == 0).all()) and pads_untouched(out, r4(width)), (self.dims, self.how)
        else:
            assert pads_untouched(out, width), (self.dims, self.how)

    def check_dpre(self, out, name):
        B, K, trials, T, F, E = self.dims
        ref, tol = R.cond_dpre(self.dxs, self.aux, True, self.stride)
        WORST.add(name, R.worst(out[:, :F].reshape(B, T, F), ref, tol))
        self.check_pads(out, F, is_vec((self.ld_p, self.o_p), (self.ld_a, self.o_a), (self.ld_x, self.o_x), width=F))

    def check_daux(self, got, name):
        B, K, trials, T, F, E = self.dims
        ref, tol = R.cond_daux(self.dxs, self.pre if self.mul else None, E, self.stride)
        WORST.add(name, R.worst(got, ref, tol))


def test_the_cases_cover_what_they_claim():
    assert WAVE_PASS == 16384 and ITEM_PASS == 1048576 and set(STRIDES) == {1, 2, 3, 7, 8} and max(STRIDES) > T
    assert [R.frames_of(T, s) for s in STRIDES] == [7, 4, 3, 1, 1] and T % 2 and T % 3
    assert layout(5, "dense") == (5, 0) and not is_vec(layout(5, "dense"), width=5) and is_vec(layout(8, "dense"), width=8)
    assert is_vec(layout(5, "padded"), width=5) and is_vec(layout(5, "wide"), width=5) and not is_vec(layout(8, "offset"), width=8)
    assert max(MUL_F) > 1024 and {e for _, e in CAT_FE} == {3, 4, 100}
    m, Bp, Kp, tr, Tp, F, E, s, how = PAST[0]
    assert Bp * tr * Kp * Tp > 2 * WAVE_PASS and Bp * Kp * R.frames_of(Tp, s) > WAVE_PASS and s == 1          # forward rows; d(aux) waves
    m, Bp, Kp, tr, Tp, F, E, s, how = PAST[1]
    assert m and Bp * Tp * F // 4 > ITEM_PASS and is_vec(layout(F, how), width=F)                              # d(pre), 16-byte
    m, Bp, Kp, tr, Tp, F, E, s, how = PAST[2]
    assert m and Bp * Tp * F > ITEM_PASS and not is_vec(layout(F, how), width=F) and s > 16                    # d(pre), 4-byte
    m, Bp, Kp, tr, Tp, F, E, s, how = PAST[3]
    assert not m and Bp * tr * Kp * Tp * (F + E) > ITEM_PASS                                                   # cat forward
    assert all(c[4] == 2741 and all(2741 % q for q in range(2, 53)) for c in PAST)
    # d(aux): every instantiation (16-byte / 4-byte x mul / cat) has more wave units than one pass at one-frame buckets
    kinds = set()
    for m, Bp, Kp, tr, Tp, F, E, s, how in (PAST[0], *PAST[4:7]):
        W = F if m else F + E
        vec = is_vec(layout(W, how), width=W) and (not m or is_vec(layout(F, how), width=F))
        assert s == 1 and Bp * Kp * Tp > WAVE_PASS
        kinds.add((vec, m))
    assert kinds == {(True, True), (False, True), (True, False), (False, False)}
    m, Bp, Kp, tr, Tp, F, E, s, how = PAST[7]
    assert m and s > 16 and Bp * Kp * R.frames_of(Tp, s) * F > ITEM_PASS and is_vec(layout(F, how), width=F)     # reduce kernel
    assert [R.frames_of(LONG_T, s) for s in LONG_STRIDES] == [3, 2, 1] and all(s > 16 for s in LONG_STRIDES)
    assert LONG_T % 17 == 6 and LONG_T % 33 == 7          # a shorter last bucket: its chunks behind the end store zeros


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("F", MUL_F)
def test_mul_base_cases(F, how):
    for trials in (1, 2):
        for stride in STRIDES:
            c = Case(True, B, K, trials, T, F, F, stride, how, seed=F + 10 * stride + trials)
            c.check_fwd(c.fwd())
            c.check_dpre(c.dpre(), f"d(pre) mul   F={F}")
            got, _ = c.daux()
            c.check_daux(got, f"d(aux) mul   F={F}")


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("F,E", CAT_FE)
def test_cat_base_cases(F, E, how):
    for trials in (1, 2):
        for stride in STRIDES:
            c = Case(False, B, K, trials, T, F, E, stride, how, seed=E + 10 * stride + trials)
            c.check_fwd(c.fwd())
            got, _ = c.daux()
            c.check_daux(got, f"d(aux) cat   E={E}")


@pytest.mark.parametrize("mul,Bp,Kp,trials,Tp,F,E,stride,how", PAST)
def test_past_one_pass_of_the_grid(mul, Bp, Kp, trials, Tp, F, E, stride, how):
    c = Case(mul, Bp, Kp, trials, Tp, F, E, stride, how, seed=Tp + F)
    c.check_fwd(c.fwd())
    if mul:
        c.check_dpre(c.dpre(), "d(pre) mul   past the grid")
    got, _ = c.daux()
    c.check_daux(got, f"d(aux) {'mul' if mul else 'cat'}   past the grid")


@pytest.mark.parametrize("how", LAYOUTS)
@pytest.mark.parametrize("mul,F,E", LONG_SHAPES)
def test_d_aux_through_the_workspace(mul, F, E, how):
    """Buckets longer than 16 frames: the partial kernel writes [chunk][(b, s, ta)][window] into a NaN-filled workspace
    and the reduce kernel picks the C columns out of the window (for cat the window starts at F & ~3, before column F).
    T = 40 at strides 17, 33 and 40: a shorter last bucket whose trailing chunks hold no frame and must store zeros, and
    one bucket of all frames.  Inside the bound, two runs bit for bit alike, through hip_ops as through the C ABI."""
    for trials in (1, 2):
        for stride in LONG_STRIDES:
            c = Case(mul, B, K, trials, LONG_T, F, E, stride, how, seed=7 * F + E + stride + trials)
            got, (dv, pv) = c.daux()
            vec = is_vec((c.ld_x, c.o_x), width=c.W) and (not mul or is_vec((c.ld_p, c.o_p), width=F))
            assert vec == (how in ("padded", "wide") or (how == "dense" and c.W % 4 == 0 and (not mul or F % 4 == 0)))
            c.check_daux(got, f"d(aux) {'mul' if mul else 'cat'}   workspace, {'16' if vec else '4'}-byte")
            again, _ = c.daux()
            assert torch.equal(got, again)
            comb = "mul" if mul else "cat"
            assert torch.equal(H().cond_aux_bwd(dv, c.ld_x, pv, c.ld_p if mul else 0, B, K, LONG_T, F, E, trials, comb, c.Ta, stride), got)


@pytest.mark.parametrize("how", ["padded", "dense"])
@pytest.mark.parametrize("mul,F,E", [(True, 5, 5), (True, 8, 8), (True, 1028, 1028), (False, 5, 3), (False, 5, 100)])
def test_time_constant_against_the_utterance_level_entry_points(mul, F, E, how):
    """stride >= T (7 and 8: one row per speaker, the very buffers the utterance-level entry points take) and a
    time-constant aux at strides 1 and 3: the forward and d(pre) have the neighbours' bits; d(aux) at stride >= T is the
    utterance-level sum within the bound, the same bits in two runs, and through hip_ops as through the C ABI."""
    for trials in (1, 2):
        for stride in (1, 3, 7, 8):
            c = Case(mul, B, K, trials, T, F, E, stride, how, seed=3 * F + stride + trials, const=True)
            u = c if c.Ta == 1 else Case(mul, B, K, trials, T, F, E, T, how, seed=0,
                                         data=(c.pre, c.aux[:, :, :1].contiguous(), c.dxs))
            assert torch.equal(u.aux[:, :, 0], c.aux[:, :, 0]) and torch.equal(u.dxs, c.dxs) and u.Ta == 1
            xs, xs_u = c.fwd(), u.fwd(utterance=True)
            assert torch.equal(xs[:, :c.W], xs_u[:, :c.W]), (stride, trials)
            if mul:
                d, d_u = c.dpre(), u.dpre(utterance=True)
                assert torch.equal(d[:, :F], d_u[:, :F]), (stride, trials)
            if c.Ta == 1:
                got, (dv, pv) = c.daux()
                c.check_daux(got, f"d(aux) {'mul' if mul else 'cat'}   stride >= T")
                again, _ = c.daux()
                assert torch.equal(got, again)
                if how == "padded":
                    comb = "mul" if mul else "cat"
                    args = (dv, c.ld_x, pv, c.ld_p if mul else 0, B, K, T, F, E, trials, comb)
                    assert torch.equal(H().cond_aux_bwd(*args, c.Ta, stride), got)
                    ref3, tol3 = R.cond_daux(c.dxs, c.pre if mul else None, E, stride)
                    WORST.add("d(aux) utterance-level entry point", R.worst(H().cond_aux_bwd(*args).view(B, K, 1, c.C), ref3, tol3))


def test_hip_ops_wrappers_make_the_same_calls():
    """hip_ops.cond_fwd / cond_bwd with (Ta, stride): the C ABI's bits, and ValueError before a launch on a bad shape."""
    for mul, F, E in ((True, 8, 8), (False, 5, 3)):
        comb = "mul" if mul else "cat"
        c = Case(mul, B, K, 2, T, F, E, 3, "padded", seed=77)
        xs, ld, info = H().cond_fwd(c.pv, c.ld_p, c.aux, B, K, T, F, 2, comb, c.Ta, 3)
        assert torch.equal(xs[:, :c.W], c.fwd()[:, :c.W])
        if mul:
            dpre, _ = H().cond_bwd(c.dxs_view(), c.ld_x, info, B, K, T, F, 2, comb, c.Ta, 3)
            assert torch.equal(dpre[:, :F], c.dpre()[:, :F])
        for Ta, stride in ((c.Ta + 1, 3), (c.Ta, 2), (c.Ta, 0), (c.Ta, -3), (c.Ta, 3.0)):
            with pytest.raises(ValueError, match="aux_stride"):
                H().cond_fwd(c.pv, c.ld_p, c.aux, B, K, T, F, 2, comb, Ta, stride)


def test_bad_shapes_are_refused_before_any_launch():
    s = H()._stream()
    a = torch.zeros(256, device=DEV)
    p = _p(a)
    for Ta, stride in ((3, 2), (5, 2), (0, 2), (7, 0), (7, -1), (1, 6), (2, 7), (2, 8)):          # T = 7
        assert stride < 1 or Ta != R.frames_of(7, stride)
        assert L().tssep_cond_mul_t_fwd(p, 8, p, 8, p, 8, 1, 2, 7, 8, 1, Ta, stride, s) == E_SHAPE
        assert L().tssep_cond_mul_t_bwd(p, 8, p, 8, p, 8, 1, 2, 7, 8, 1, Ta, stride, s) == E_SHAPE
        assert L().tssep_cond_cat_t_fwd(p, 4, p, 4, p, 8, 1, 2, 7, 4, 4, 1, Ta, stride, s) == E_SHAPE
        assert L().tssep_cond_mul_aux_t_bwd(p, 8, p, 8, p, 8, p, 1, 2, 7, 8, 1, Ta, stride, s) == E_SHAPE
        assert L().tssep_cond_cat_aux_t_bwd(p, 8, p, 4, p, 1, 2, 7, 4, 4, 1, Ta, stride, s) == E_SHAPE
        assert L().tssep_cond_aux_t_bwd_workspace_bytes(1, 2, 7, 8, 0, Ta, stride) == -1
    assert L().tssep_cond_mul_t_fwd(p, 8, p, 8, p, 8, 1, 2, 7, 8, 3, 4, 2, s) == E_SHAPE                 # trials > K
    assert L().tssep_cond_cat_aux_t_bwd(p, 8, p, 4, p, 1, 2, 7, 4, 0, 1, 4, 2, s) == E_SHAPE             # E = 0
    assert L().tssep_cond_mul_aux_t_bwd(p, 7, p, 8, p, 8, p, 1, 2, 7, 8, 1, 4, 2, s) == E_SHAPE          # ld < F
    assert L().tssep_cond_mul_aux_t_bwd(p, 8, p, 8, p, 8, None, 1, 2, 40, 8, 1, 2, 20, s) == -5          # a workspace is needed
    assert L().tssep_cond_aux_t_bwd_workspace_bytes(1, 2, 7, 8, 0, 4, 2) == 0
    assert L().tssep_cond_aux_t_bwd_workspace_bytes(1, 2, 40, 8, 0, 2, 20) == 2 * 1 * 2 * 2 * 8 * 4
    torch.cuda.synchronize()
    assert not bool(a.any())


def test_zz_report():
    """The worst err / bound of every group of this file (pytest -rP)."""
    for k in sorted(WORST.r):
        print(f"max err/bound  {k}: {WORST.r[k]:.3g}")
    assert all(math.isfinite(v) and v <= 1.0 for v in WORST.r.values())
