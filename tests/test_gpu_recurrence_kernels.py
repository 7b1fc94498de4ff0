"""The four BLSTM recurrence families (lstm.hip: streaming fp32; lstm_cluster.hip: W-stationary fp32; lstm_onchip.hip: the
32-sequence and the interleaved 16-sequence split-bf16 kernels) one step at a time against float64, launched through the
by-name wrappers of hip_ops, every launch followed by check_cluster_errors().  The reference and bound functions live in
tests/test_recurrence_reference.py, which also tests them without a GPU.  C_SPLIT, LAMBDA and U are those of
tests/test_gpu_gemm_kernels.py.

1. Forward, step-wise.  Inputs: fp32 pre-activations gin [N, T, 2, H, 4] (generated directly: no input GEMM) and
   W_hh ~ U(-H^-1/2, H^-1/2).  One launch writes the activations A, cell and hout over NaN.  In float64, all t at once:
   from the KERNEL's own h and c of the previous step (zero at the start), a = gin + h_prev W_hh^T, the four activations,
   c = f c_prev + i g, h = o tanh(c); every element of every step is compared with what the kernel stored.  Bounds:
     * pre-activation.  e_a = (C + LAMBDA sqrt(n) U) (|h_prev| |W_hh|^T) + U |a|.  Split-bf16 kernels: C = C_SPLIT,
       n = 3 H + 16 (three products per term, up to 16 partial sums joined); exact-fp32 ones: C = 0, n = H + 16.  The last
       term is the addition of gin.  The on-chip kernels read h_prev from compact exchange granules that keep 16
       significant bits (relative 2^-17); such a value splits into bf16 hi + lo exactly, so the operand error stays below
       the 2^-16 |x| that the derivation of C_SPLIT already allows for e_x: no further term.
     * activations.  e_act = f'(a) e_a + max|f''| / 2 e_a^2 + e_f (sigmoid: f' = s (1 - s), |f''| / 2 <= 0.0482; tanh:
       f' = 1 - y^2, |f''| / 2 <= 0.385), e_f the function's own absolute error, plus U |f| for the store:
         - streaming, cluster: 1 / (1 + expf(-x)) and tanhf of OCML, which honours OpenCL's full-profile limits (exp 3 ulp,
           tanh 5 ulp; 1 ulp <= 2 U relative): sigmoid s ((1 - s) 6 U + 2 U) (expf enters s with weight 1 - s; the sum and
           the correctly rounded division add U each), tanh 10 U |y|;
         - fast_sigmoid = rcp(1 + exp2(fl(-log2e x))): the rounded constant and product put (1 +- 2 U) on the argument,
           i.e. 2 U |x| relative on the exponential; v_exp_f32 1 ulp = 2 U; the sum U; v_rcp_f32 2 U:
           s ((1 - s) (2 U |x| + 2 U) + 3 U);
         - fast_tanh = 1 - 2 r, r = rcp(1 + E), E = exp2(fl(2 log2e x)): E carries 4 U |x| + 2 U with weight
           E / (1 + E) = (1 + y) / 2, r 3 U more, 2 r = 1 - y, the subtraction U |y|:
           (1 - y) ((1 + y) / 2 (4 U |x| + 2 U) + 3 U) + U |y| -- an ABSOLUTE error of 4 U near x = 0;
         - every one plus 2^-126: the units may flush a subnormal result.
     * c: e_c = e_f |c_prev| + e_i |g| + e_g i + e_i e_g + 2 U (|f c_prev| + |i g|) + U |c| (two products, the sum, the
       store); h: tanh at the kernel's c, e_tc = (1 - tc^2) e_c + 0.385 e_c^2 + e_tanh, e_h = e_o |tc| + o e_tc + e_o e_tc
       + 2 U |h|.
   At H = 300 the median bounds are 3e-6 (A), 6e-6 (cell), 4e-6 (h) for fp32 and four times that for split bf16; W_hh
   rounded to bf16 exceeds them 66 / 11 times (fp32 / split-bf16 bound), a reduction cut at k = 288 10^4 / 10^3 times
   (tests/test_recurrence_reference.py).

2. The activation bounds on their own: T = 1 launches (h_-1 = 0: A is the plain function of gin) whose pre-activations
   run through the 163 841 multiples of 2^-12 in [-20, 20] and +-30, +-88, +-100, +-1e4, +-0, +-2^-126, +-2^-125, every
   value in every gate.  Within the bounds of 1 (e_a = 0), finite, and exactly 0, 1 or +-1 where float64 rounds to them.

3. Backward, step-wise.  Saved A and cell: the float64 forward loop rounded to fp32; dhout ~ randn.  In float64:
   dh_t = dhout_t + D_next W_hh from the KERNEL's own D of the next step; dc_t = dh_t o_t (1 - tanh^2 c_t) + f_next dc_next
   by an elementwise scan; the four gate gradients.  Bounds:
     * e_dh = (C + C_X + LAMBDA sqrt(n) U) (|D_next| |W_hh|) + U |dh|, n = 3 * 4H + 16 (split) or 4H + 16: the sum runs
       over the 4H gate columns, in up to 16 partial sums (4 waves in lstm.hip, the workgroups of a cluster in the
       reduce-scatter).  C_X = 2^-17 for the on-chip kernels only: each partial sum crosses in a 24-bit granule.
     * local term p = dh o (1 - tc^2): e_p = e_dh o (1 - tc^2) + |dh| o (2 |tc| e_tanh + e_tanh^2 + U) + 3 U |p|.
     * carried dc: E_t = e_p + f_next E_next + U |f_next dc_next| + U |dc_t|, scanned alongside.
     * gates: E times the other factors; d_g adds U |dc i| (1 - g^2 cancels), d_o = dh tc o (1 - o) takes e_dh and e_tanh;
       5 U |d| for the products and the store.

4. Whole sequences, T <= 64: the kernel against a plain float64 time loop, at most M times the error of the same loop in
   fp32 torch (torch.nn.LSTM's arithmetic, computed here) plus 4 U max|ref|.  M = 4 for the exact-fp32 families (two
   realisations of one bound: 2; OCML's 3 - 5 ulp functions against 1 ulp: 2); for split bf16 M = 4 (C_SPLIT + LAMBDA
   sqrt(3 H + 16) U) / (LAMBDA sqrt(H + 16) U) = 26.1 at H = 300.

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report):
    family     A      cell   h      d(gates)  activations alone   whole sequence: kernel error / fp32 torch error (allowed)
    streaming  0.50   0.51   0.23   0.49      0.50                A 1.19  cell 0.96  h 0.95  d(gates) 0.96  (4)
    cluster    0.50   0.54   0.23   0.49      0.50                A 0.52  cell 0.91  h 0.91  d(gates) 1.38  (4)
    32-seq.    0.56   0.55   0.55   0.56      0.52                A 10.5  cell 11.5  h 14.7  d(gates) 8.33  (26.1)
    interl.    0.56   0.55   0.56   0.56      0.52                A 10.2  cell 11.6  h 14.3  d(gates) 10.4  (26.1; 27.4 at H = 260)
The headline launches (3 072 x 253 x 300, two groups): A 0.55, cell 0.54, h 0.51 forward, d(gates) 0.56 backward.

Pad columns of hout (Hp != H, or ldo > 2 Hp) hold a sentinel before every forward launch and must hold it afterwards; the
backward's dhout holds NaN there."""
import warnings

import pytest
import torch

from tssep_amd import _lib, hip_ops as Hop
from tssep_amd.train import runtime
from test_recurrence_reference import (FAMILIES, U, Worst, _blocks, activation_grid, check_backward, check_forward,
                                       lstm_backward_loop, lstm_forward_loop, make_whh, sigmoid_err, tanh_err,
                                       whole_sequence_multiple, _dirs)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = 12345.5
GIB = 1 << 30
E_SHAPE, E_UNSUPPORTED = -1, -3
WORST = {}          # (family, direction, output) -> largest error / bound of this run
KERNEL_FAMILY = {"stream_f32": "stream", "cluster_f32": "cluster", "onchip32_bf16x3": "onchip32", "onchip16_bf16x3": "onchip16"}


@pytest.fixture(autouse=True)
def _device_memory_cap():
    """The GPU is shared: every test here stays under 16 GB of device memory at its peak."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 * GIB, f"peak device memory {peak / GIB:.1f} GiB"


def _record(fam, direction, w):
    for k, v in w.ratio.items():
        WORST[(fam, direction, k)] = max(WORST.get((fam, direction, k), 0.0), v)


class Case:
    """Inputs of one launch.  klass "big": pre-activations scaled by 20 and a forget-gate bias of +6 (saturated gates, a
    cell state that grows over the sequence)."""

    def __init__(self, N, T, H, seed=0, klass="randn", ldo_extra=0):
        self.N, self.T, self.H, self.seed, self.klass = N, T, H, seed, klass
        self.Hp = Hop.round_up(H, 4)
        self.dstride, self.ldo = self.Hp, 2 * self.Hp + ldo_extra
        gen = torch.Generator(device=DEV).manual_seed(1000 + seed)
        self.whh = make_whh(H, gen, DEV)
        self.blocks = _blocks(N, T)
        self._packs = {}

    def gin(self, n0, n1):
        assert (n0, n1) in self.blocks
        gen = torch.Generator(device=DEV).manual_seed(self.seed * 1000003 + n0)
        x = torch.randn(n1 - n0, self.T, 2, self.H, 4, device=DEV, generator=gen)
        if self.klass == "big":
            x *= 20
            x[..., 1] += 6
        return x

    def saved(self, group):
        """A, cell of the float64 forward loop over a few consecutive blocks, rounded to fp32"""
        A, c, _ = lstm_forward_loop(torch.cat([self.gin(*b) for b in group]), self.whh, self.H, torch.float64)
        return A.float(), c.float()

    def saved_again(self):
        """-> (n0, n1) -> A of that block, recomputed group by group (a launch overwrites A; a copy of 7 GB is too much)"""
        groups = [self.blocks[i:i + 4] for i in range(0, len(self.blocks), 4)]
        held = {}

        def A_of(n0, n1):
            grp = groups[self.blocks.index((n0, n1)) // 4]
            if held.get("first") != grp[0][0]:
                held.clear()
                held.update(first=grp[0][0], A=self.saved(grp)[0])
            return held["A"][n0 - grp[0][0]:n1 - grp[0][0]]
        return A_of

    def pad_mask(self):
        m = torch.ones(self.ldo, dtype=torch.bool, device=DEV)
        for d in (0, 1):
            m[d * self.dstride:d * self.dstride + self.H] = False
        return m

    def pack(self, fam, bwd):
        key = fam if fam != "onchip16" else (fam, bwd)
        if key not in self._packs:
            wf, wr = self.whh
            if fam == "stream":
                z = torch.zeros(4 * self.H, 4, device=DEV)
                b = torch.zeros(4 * self.H, device=DEV)
                pk = Hop.lstm_pack([z, wf, b, b, z, wr, b, b], self.H, 4)
                self._packs[key] = (pk["whh_f"], pk["whh_b"], pk)
            elif fam == "cluster":
                self._packs[key] = Hop.lstm_pack_cluster(wf, wr, self.H)
            elif fam == "onchip32":
                self._packs[key] = Hop.lstm_pack_onchip(wf, wr, self.H)
            elif bwd:
                self._packs[key] = (None, Hop.lstm_pack_onchip16_bwd(wf, wr, self.H))
            else:
                self._packs[key] = (Hop.lstm_pack_onchip16(wf, wr, self.H), None)
        return self._packs[key][int(bwd)]

    def launch(self, fam, bwd, var, gates, cell, h):
        N, T, H = self.N, self.T, self.H
        args = (gates, cell, h, self.ldo, self.dstride, self.pack(fam, bwd), N, T, H)
        if fam == "stream":
            (Hop.blstm_bwd if bwd else Hop.blstm_fwd)(*args)
        elif fam == "cluster":
            (Hop.blstm_cluster_bwd if bwd else Hop.blstm_cluster_fwd)(*args, var)
        elif fam == "onchip32":
            (Hop.blstm_onchip_bwd if bwd else Hop.blstm_onchip_fwd)(*args, var)
        else:
            (Hop.blstm_onchip16_bwd if bwd else Hop.blstm_onchip16_fwd)(*args, var)
        Hop.check_cluster_errors()

    # ---- the two step-wise checks ------------------------------------------------------------------------------------
    def forward(self, fam, var, launch=None):
        N, T, H = self.N, self.T, self.H
        gates = torch.empty(N, T, 2, H, 4, device=DEV)
        for n0, n1 in self.blocks:
            gates[n0:n1] = self.gin(n0, n1)
        cell = torch.full((N, T, 2, H), NAN, device=DEV)
        hout = torch.full((N, T, self.ldo), NAN, device=DEV)
        pad = self.pad_mask()
        hout[..., pad] = SENT
        (launch or self.launch)(fam, False, var, gates, cell, hout)
        if bool(pad.any()):
            assert bool((hout[..., pad] == SENT).all()), "pad columns of hout were written"
        w = check_forward(self.gin, gates, cell, hout, self.whh, H, self.dstride, fam)
        print(f"{fam} fwd N={N} T={T} H={H} var={var} {self.klass}: {w}")
        _record(fam, "fwd", w)
        assert w.count == N * T * 2 * H and w.ok(), (str(w), w.outside)
        return gates, cell, hout

    def backward(self, fam, var, launch=None):
        N, T, H = self.N, self.T, self.H
        gates = torch.empty(N, T, 2, H, 4, device=DEV)
        cell = torch.empty(N, T, 2, H, device=DEV)
        for i in range(0, len(self.blocks), 4):
            grp = self.blocks[i:i + 4]
            gates[grp[0][0]:grp[-1][1]], cell[grp[0][0]:grp[-1][1]] = self.saved(grp)
        A = gates.clone() if gates.numel() < (1 << 28) else self.saved_again()
        gen = torch.Generator(device=DEV).manual_seed(77 + self.seed)
        dhout = torch.randn(N, T, self.ldo, device=DEV, generator=gen)
        dhout[..., self.pad_mask()] = NAN
        (launch or self.launch)(fam, True, var, gates, cell, dhout)
        w = check_backward(A, cell, dhout, gates, self.whh, H, self.dstride, fam)
        print(f"{fam} bwd N={N} T={T} H={H} var={var} {self.klass}: {w}")
        _record(fam, "bwd", w)
        assert w.count == N * T * 2 * H * 4 and w.ok(), (str(w), w.outside)
        return A, cell, dhout, gates


# ---- sections 1 and 3: the cases ---------------------------------------------------------------------------------------
STREAM = [(1, 5, 5), (9, 7, 300), (9, 3, 303), (9, 5, 305), (9, 5, 512), (1, 1, 300), (3072, 5, 300)]
CLUSTER = [(1, 1, 33, 0), (70, 2, 257, 2), (1000, 5, 304, 4), (70, 7, 304, 0), (1, 7, 257, 4), (1000, 2, 33, 2), (70, 5, 300, 4)]
# (785 sequences: 50 work items, between the 48 XCD-local and the 51 packed clusters of 256 CUs at five workgroups each;
# 1601 and 3072: 102 and 192 items, several resident rounds, 1601 with one sequence in its last item)
ONCHIP32 = [(1, 1, 129, 0), (31, 2, 192, 8), (33, 7, 257, 0), (159, 7, 301, 8), (160, 7, 304, 0), (160, 2, 129, 8), (1, 7, 304, 8),
            (33, 1, 301, 0), (785, 7, 300, 0), (1601, 2, 301, 0), (1601, 7, 192, 8), (3072, 7, 257, 0)]
ONCHIP16_FWD = [(1, 1, 128, 1), (15, 2, 256, 1), (16, 3, 260, 1), (17, 5, 300, 2), (64, 5, 304, 4), (64, 3, 128, 2), (32, 5, 256, 2),
                (17, 1, 304, 1), (64, 7, 256, 4), (64, 2, 128, 4), (16, 5, 300, 1), (3088, 5, 300, 1), (3072, 2, 260, 4), (32, 253, 304, 2),
                (16, 2100, 300, 1)]
ONCHIP16_BWD = [(64, 5, 300, 4), (32, 3, 260, 1), (32, 2, 304, 2), (1, 1, 260, 1), (15, 2, 300, 1), (16, 3, 304, 1), (17, 5, 260, 2), (64, 5, 304, 4), (17, 1, 300, 1),
                (3088, 5, 300, 1), (3072, 2, 260, 4), (32, 253, 300, 2), (16, 2100, 300, 1)]


@pytest.mark.parametrize("N,T,H", STREAM)
def test_streaming_step_by_step(N, T, H):
    c = Case(N, T, H, seed=1)
    c.forward("stream", None)
    c.backward("stream", None)


@pytest.mark.parametrize("N,T,H,ms", CLUSTER)
def test_cluster_step_by_step(N, T, H, ms):
    c = Case(N, T, H, seed=2)
    c.forward("cluster", ms)
    c.backward("cluster", ms)


@pytest.mark.parametrize("N,T,H,layout", ONCHIP32)
def test_onchip32_step_by_step(N, T, H, layout):
    c = Case(N, T, H, seed=3)
    c.forward("onchip32", layout)
    c.backward("onchip32", layout)


@pytest.mark.parametrize("N,T,H,groups", ONCHIP16_FWD)
def test_interleaved_forward_step_by_step(N, T, H, groups):
    Case(N, T, H, seed=4).forward("onchip16", groups)


@pytest.mark.parametrize("N,T,H,groups", ONCHIP16_BWD)
def test_interleaved_backward_step_by_step(N, T, H, groups):
    Case(N, T, H, seed=5).backward("onchip16", groups)


@pytest.mark.parametrize("fam,N,T,H,var", [("stream", 9, 33, 300, None), ("cluster", 70, 33, 300, 2), ("onchip32", 33, 33, 300, 0),
                                           ("onchip16", 64, 33, 300, 2)])
def test_saturated_gates_and_a_growing_cell_state(fam, N, T, H, var):
    c = Case(N, T, H, seed=6, klass="big")
    _, cell, _ = c.forward(fam, var)
    assert float(cell.abs().max()) > 2          # (one step from zero gives |c| <= 1: the inputs do make c grow)
    c.backward(fam, var)


@pytest.mark.parametrize("fam,N,T,H,var", [("stream", 9, 5, 303, None), ("cluster", 70, 5, 257, 2), ("onchip32", 33, 5, 301, 0),
                                           ("onchip32", 33, 5, 300, 8), ("onchip16", 32, 5, 300, 2)])
def test_a_wider_row_of_hout_stays_untouched(fam, N, T, H, var):
    """ldo = 2 Hp + 8: the eight extra columns keep the sentinel (forward) and are never read (backward: NaN)"""
    c = Case(N, T, H, seed=7, ldo_extra=8)
    c.forward(fam, var)
    c.backward(fam, var)


def test_the_headline_size_forward():
    """3 072 x 253 x 300 on the group count the library picks: the multi-round, all-XCD schedule of the timed step"""
    N, T, H = 3072, 253, 300
    g = Hop.onchip16_groups(N, H, torch.device("cuda", 0))
    assert g
    Case(N, T, H, seed=8).forward("onchip16", g)


def test_the_headline_size_backward():
    N, T, H = 3072, 253, 300
    g = Hop.onchip16_bwd_groups(N, H, torch.device("cuda", 0))
    assert g
    Case(N, T, H, seed=9).backward("onchip16", g)


# ---- section 2 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,H,var", [("stream", 300, None), ("cluster", 300, 0), ("onchip32", 300, 0), ("onchip16", 300, 1)])
def test_activations_over_their_whole_range(fam, H, var):
    x = activation_grid().to(DEV)
    G = x.numel()
    N = -(-G // (2 * H))
    c = Case(N, 1, H, seed=10)
    j = torch.arange(N * 2 * H, device=DEV)
    gin = torch.stack([x[(j + g * (G // 4)) % G] for g in range(4)], -1).view(N, 1, 2, H, 4)
    c.gin = lambda n0, n1: gin[n0:n1]
    A, _, _ = c.forward(fam, var)
    fast = FAMILIES[fam]["fast"]
    a = gin.double()
    s, y = torch.sigmoid(a), torch.tanh(a[..., 2])
    ref = s.clone()
    ref[..., 2] = y
    err = sigmoid_err(a, s, fast)
    err[..., 2] = tanh_err(a[..., 2], y, fast)
    assert bool(torch.isfinite(A).all())
    r = (A.double() - ref).abs() / (err + U * ref.abs())
    print(f"{fam}: activations alone, error / bound = {float(r.max()):.3g}")
    WORST[(fam, "fwd", "activation sweep")] = float(r.max())
    assert float(r.max()) <= 1
    r32 = ref.float()
    for v in (0.0, 1.0, -1.0):
        m = r32 == v
        assert bool(m.any()) and bool((A[m] == v).all()), v


# ---- section 4 -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,N,T,H,var", [("stream", 40, 64, 300, None), ("cluster", 40, 64, 300, 2), ("onchip32", 40, 64, 300, 0),
                                           ("onchip16", 48, 64, 300, 1), ("onchip16", 48, 64, 260, 1)])
def test_whole_sequences_against_a_float64_loop(fam, N, T, H, var):
    c = Case(N, T, H, seed=11)
    M = whole_sequence_multiple(fam, H)
    gin = torch.cat([c.gin(*b) for b in c.blocks])
    A, cell, hout = c.forward(fam, var)
    ref = lstm_forward_loop(gin, c.whh, H, torch.float64)
    t32 = lstm_forward_loop(gin, c.whh, H, torch.float32)
    got = (A, cell, _dirs(hout, H, c.dstride))
    pairs = [(n, k, r, t) for n, k, r, t in zip(("act", "cell", "h"), got, ref, t32)]
    if fam != "onchip16" or H > 256:
        As, cs, dhout, D = c.backward(fam, var)
        dh = _dirs(dhout, H, c.dstride)
        pairs.append(("dgates", D, lstm_backward_loop(As, cs, dh, c.whh, H, torch.float64),
                      lstm_backward_loop(As, cs, dh, c.whh, H, torch.float32)))
    for name, k, r, t in pairs:
        ek, et = float((k.double() - r).abs().max()), float((t.double() - r).abs().max())
        floor = 4 * U * float(r.abs().max())
        print(f"{fam} H={H} {name}: kernel {ek:.3g}, fp32 torch {et:.3g}, ratio {ek / et:.3g} (allowed {M:.3g})")
        key = (fam, "whole", name)
        WORST[key] = max(WORST.get(key, 0.0), ek / et)
        assert ek <= M * et + floor, (name, ek, et, M)


# ---- guards ------------------------------------------------------------------------------------------------------------
def _guard_call(entry, N, T, H, groups=None):
    """the C entry point on argument values alone: every guard under test returns before anything is launched"""
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    Hp = Hop.round_up(H, 4)
    p = Hop._p(buf)
    tail = (0,) if groups is None else (0, groups)
    return getattr(L, entry)(p, p, p, 2 * Hp, Hp, p, p, Hop._p(Hop._err_flag(DEV)), N, T, H, Hop.n_cus(torch.device("cuda", 0)),
                             *tail, Hop._stream())


def test_guards_decline_before_anything_is_launched():
    L = _lib.lib()
    cus = Hop.n_cus(torch.device("cuda", 0))
    for entry in ("tssep_blstm_onchip_fwd", "tssep_blstm_onchip_bwd"):
        assert _guard_call(entry, 32, 3, 305) == E_UNSUPPORTED
        assert _guard_call(entry, 32, int(L.tssep_lstm_onchip_max_steps(300, 32)) + 1, 300) == E_SHAPE
    for entry in ("tssep_blstm_onchip16_fwd", "tssep_blstm_onchip16_bwd"):
        assert _guard_call(entry, 16, 3, 321, 1) == E_UNSUPPORTED
        assert _guard_call(entry, 16, 3, 258, 1) == E_UNSUPPORTED
        assert _guard_call(entry, 16, int(L.tssep_lstm_onchip_max_steps(300, 16)) + 1, 300, 1) == E_SHAPE
    torch.cuda.synchronize()
    Hop.check_cluster_errors()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        plan = Hop.recurrence_plan(16, int(L.tssep_lstm_onchip_max_steps(300, 16)) + 1, 300, cus)
        assert plan["fwd"][0] == "stream_f32" and plan["bwd"][0] == "stream_f32", plan
        # H = 256: the backward runs on the 32-sequence kernel, whose limit is the lower one
        plan = Hop.recurrence_plan(16, int(L.tssep_lstm_onchip_max_steps(256, 32)) + 1, 256, cus)
        assert plan["fwd"][0] == "onchip16_bf16x3" and plan["bwd"][0] == "stream_f32", plan
    assert Hop.recurrence_plan(16, 5, 305, cus) == {"fwd": ("stream_f32", 0), "bwd": ("stream_f32", 0)}
    assert Hop.recurrence_plan(16, 5, 304, cus)["fwd"][0].startswith("onchip")


# ---- through the plan, as functional._RNNP launches ------------------------------------------------------------------
@pytest.mark.parametrize("N,T,H,settings", [(3072, 7, 256, dict(onchip16_bwd=False)), (768, 7, 300, {}), (32, 7, 300, dict(recurrence="cluster")),
                                            (9, 7, 300, dict(recurrence="stream")), (40, 5, 303, {})])
def test_through_the_plan(N, T, H, settings):
    with runtime.applied(**settings):
        c = Case(N, T, H, seed=12)
        cus = Hop.n_cus(torch.device("cuda", 0))
        plan = Hop.recurrence_plan(N, T, H, cus)
        wf, wr = c.whh
        c.pack("stream", False)
        whh = Hop.recurrence_packs(plan, wf, wr, H, c._packs["stream"][2])
        log = Hop.RECURRENCE_LOG = []

        def launch(fam, bwd, var, gates, cell, h):
            d = "bwd" if bwd else "fwd"
            Hop.recurrence_launch(plan[d], d, gates, cell, h, c.ldo, c.dstride, whh[d], N, T, H)
            Hop.check_cluster_errors()

        try:
            c.forward(KERNEL_FAMILY[plan["fwd"][0]], None, launch)
            c.backward(KERNEL_FAMILY[plan["bwd"][0]], None, launch)
        finally:
            Hop.RECURRENCE_LOG = None
    print(plan)
    assert [(e["kernel"], e["groups"]) for e in log] == [plan["fwd"], plan["bwd"]], (log, plan)
    if "recurrence" in settings:
        assert plan["fwd"][0].startswith(settings["recurrence"])
    if settings.get("onchip16_bwd") is False:
        assert plan["bwd"] == ("onchip32_bf16x3", 0) and plan["fwd"][0] == "onchip16_bf16x3"


def test_through_the_plan_in_one_direction():
    """directions=1 (typ='lstm'): plan -> packs -> launch is the one-direction streaming kernel with its state, and leaves
    the bits of the by-name wrappers lstm1_fwd / lstm1_bwd on copies of the same buffers"""
    N, T, H = 6, 5, 5
    ld = Hop.round_up(H, 4)
    gen = torch.Generator().manual_seed(12)
    whh = ((torch.rand(4 * H, H, generator=gen) * 2 - 1) * H ** -0.5).to(DEV)
    gates0, dh0 = torch.randn(N * T, 4 * H, generator=gen).to(DEV), torch.randn(N * T, ld, generator=gen).to(DEV)
    h0, c0 = (0.5 * torch.randn(N, H, generator=gen).to(DEV) for _ in range(2))
    pk = Hop.lstm1_pack([torch.zeros(4 * H, 4, device=DEV), whh, torch.zeros(4 * H, device=DEV), torch.zeros(4 * H, device=DEV)], H, 4)
    plan = Hop.recurrence_plan(N, T, H, Hop.n_cus(torch.device("cuda", 0)), directions=1)
    assert plan == {"fwd": ("stream1_f32", 0), "bwd": ("stream1_f32", 0)}
    whh_of = Hop.recurrence_packs(plan, whh, whh, H, pk)
    assert whh_of["fwd"] is pk["whh_f"] and whh_of["bwd"] is pk["whh_b"]

    def run(fwd, bwd):
        g, cell, hout, dh = gates0.clone(), torch.zeros(N, T, H, device=DEV), torch.zeros(N * T, ld, device=DEV), dh0.clone()
        hT, cT = (torch.zeros(N, H, device=DEV) for _ in range(2))
        fwd(g, cell, hout, (h0, c0, hT, cT))
        act = g.clone()
        bwd(g, cell, dh)
        torch.cuda.synchronize()
        return dict(act=act, cell=cell, hout=hout, hT=hT, cT=cT, dgates=g)

    log = Hop.RECURRENCE_LOG = []
    try:
        got = run(lambda g, c, h, st: Hop.recurrence_launch(plan["fwd"], "fwd", g, c, h, ld, ld, whh_of["fwd"], N, T, H, state=st),
                  lambda g, c, dh: Hop.recurrence_launch(plan["bwd"], "bwd", g, c, dh, ld, ld, whh_of["bwd"], N, T, H))
    finally:
        Hop.RECURRENCE_LOG = None
    want = run(lambda g, c, h, st: Hop.lstm1_fwd(g, c, h, ld, pk["whh_f"], N, T, H, *st),
               lambda g, c, dh: Hop.lstm1_bwd(g, c, dh, ld, pk["whh_b"], N, T, H))
    assert [(e["kernel"], e["direction"], e["groups"]) for e in log] == [("stream1_f32", "fwd", 0), ("stream1_f32", "bwd", 0)], log
    for k in got:
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], want[k]), k
    assert float(got["hT"].abs().max()) > 0 and float(got["dgates"].abs().max()) > 0      # (the launches wrote)


def test_zz_report():
    """the largest error / bound of every family, direction and output this run saw (pytest -rP)"""
    for (fam, direction, name), v in sorted(WORST.items()):
        print(f"{fam:9s} {direction:5s} {name:18s} {v:.3g}")
