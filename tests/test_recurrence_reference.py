"""The float64 step-wise checker of the BLSTM recurrence kernels (tests/test_gpu_recurrence_kernels.py), tested without a
GPU: the reference and bound functions below run on any device; here they run on the CPU at H = 300, T = 64, N = 4 against
a plain fp32 time loop (torch.nn.LSTM's arithmetic), which must pass every bound, and against the same loop with five
defects planted, each of which must fail them.  The derivations are in the docstring of the GPU file; the functions are
named after its sections.

Tensors (include/tssep_hip.h): gates [N, T, 2, H, 4] (gate order i, f, g, o), cell [N, T, 2, H], hout / dhout
[N, T, ldo] with direction d in columns d * dstride .. + H; W_hh in torch's layout [4H, H] per direction."""
import math

import pytest
import torch

from test_gpu_gemm_kernels import C_SPLIT, LAMBDA, U

TINY = 2.0 ** -126          # v_exp_f32 / v_rcp_f32 (and OCML at its range ends) may flush a subnormal result
C_EXCH = 2.0 ** -17         # a value rounded to the 24 bits of a compact exchange granule (lstm_onchip.hip)
ULP = 2.0 * U               # one unit in the last place, relative, at worst
EXP_ULPS, TANH_ULPS = 3.0, 5.0      # OpenCL full-profile limits, which OCML's expf / tanhf honour
SIG_D2, TANH_D2 = 0.0482, 0.385     # max |f''| / 2: 1 / (12 sqrt 3), 2 / (3 sqrt 3)
PARTIALS = 16               # partial sums of one reduction joined at the end, at most (waves, workgroups of a cluster)
ROWS = 16384                # (sequence, frame, direction) rows of one block of the references

# family -> split: split-bf16 products (C_SPLIT, three products per term); fast: v_exp_f32 / v_rcp_f32 activations;
# exch: partial dh sums cross workgroups in compact granules (the forward's h is covered by C_SPLIT, see the GPU file)
FAMILIES = {
    "stream": dict(split=False, fast=False, exch=False),
    "cluster": dict(split=False, fast=False, exch=False),
    "onchip32": dict(split=True, fast=True, exch=True),
    "onchip16": dict(split=True, fast=True, exch=True),
    "torch": dict(split=False, fast=False, exch=False),
}


# ---- section 1: bounds -------------------------------------------------------------------------------------------------
def dot_factor(fam, terms, backward=False):
    """the factor of (|x| |W|) in the error of a dot product of `terms` terms on family `fam`"""
    f = FAMILIES[fam]
    n = (3 if f["split"] else 1) * terms + PARTIALS
    return (C_SPLIT if f["split"] else 0.0) + (C_EXCH if backward and f["exch"] else 0.0) + LAMBDA * math.sqrt(n) * U


def sigmoid_err(x, s, fast):
    """absolute error of the kernel's sigmoid at the exact argument x (s = sigmoid(x), float64)"""
    if fast:    # rcp(1 + exp2(fl(-log2e x))): argument 2 U |x|, exp2 1 ulp, the sum U, rcp 1 ulp
        rel = (1 - s) * (2 * U * x.abs() + ULP) + U + ULP
    else:       # 1 / (1 + expf(-x)): expf EXP_ULPS, the sum U, the division U
        rel = (1 - s) * EXP_ULPS * ULP + 2 * U
    return s * rel + TINY


def tanh_err(x, y, fast):
    """absolute error of the kernel's tanh at the exact argument x (y = tanh(x), float64)"""
    if fast:    # 1 - 2 r, r = rcp(1 + E), E = exp2(fl(2 log2e x)): E / (1 + E) = (1 + y) / 2, 2 r = 1 - y
        return (1 - y) * ((1 + y) / 2 * (4 * U * x.abs() + ULP) + U + ULP) + U * y.abs() + TINY
    return TANH_ULPS * ULP * y.abs() + TINY


def _through(e, d1, d2, own):
    """an argument error e through a function with derivative d1 (|f''| / 2 <= d2), plus the function's own error"""
    return d1 * e + d2 * e * e + own


def _shift(x, d0, d1):
    """x [n, T, 2, ...] -> the previous step's x in each direction's time order (d0 / d1: +1 previous, -1 next)"""
    out = torch.zeros_like(x)
    for d, s in ((0, d0), (1, d1)):
        if s > 0:
            out[:, 1:, d] = x[:, :-1, d]
        else:
            out[:, :-1, d] = x[:, 1:, d]
    return out


def _w_fwd(whh, H, dtype):
    """[2, H(k), 4H(unit * 4 + gate)]"""
    return torch.stack([w.to(dtype).view(4, H, H).permute(2, 1, 0).reshape(H, 4 * H) for w in whh])


def _w_bwd(whh, H, dtype):
    """[2, 4H(unit * 4 + gate), H(k)]"""
    return torch.stack([w.to(dtype).view(4, H, H).permute(1, 0, 2).reshape(4 * H, H) for w in whh])


def _dirs(h, H, dstride):
    """hout / dhout [n, T, ldo] -> [n, T, 2, H]"""
    return torch.stack([h[..., d * dstride:d * dstride + H] for d in (0, 1)], 2)


class Worst:
    """largest error / bound per output, the elements outside, the median bound, non-finite outputs"""

    def __init__(self):
        self.ratio, self.outside, self.count, self.nonfinite, self.medians = {}, {}, 0, 0, {}

    def add(self, name, got, ref, bound):
        fin = torch.isfinite(got)
        self.nonfinite += int((~fin).sum())
        r = ((got.double() - ref).abs() / bound)
        r = torch.where(fin, r, torch.full_like(r, float("inf")))
        self.ratio[name] = max(self.ratio.get(name, 0.0), float(r.max()))
        self.outside[name] = self.outside.get(name, 0) + int((r > 1).sum())
        self.medians.setdefault(name, []).append(float(bound.median()))

    def ok(self):
        return self.nonfinite == 0 and all(v <= 1 for v in self.ratio.values())

    def median(self, name):
        return sorted(self.medians[name])[len(self.medians[name]) // 2]

    def __str__(self):
        return " ".join(f"{k}={v:.3g}" for k, v in self.ratio.items()) + (f" NONFINITE={self.nonfinite}" if self.nonfinite else "")


def _blocks(N, T):
    nb = max(1, ROWS // (2 * T))
    return [(n0, min(N, n0 + nb)) for n0 in range(0, N, nb)]


def _of(x, n0, n1):
    return x(n0, n1) if callable(x) else x[n0:n1]


def check_forward(gin, A, cell, hout, whh, H, dstride, fam, worst=None):
    """Section 1.  gin: the pre-activations the launch read (a tensor, or a function (n0, n1) -> that block); A, cell,
    hout: what it wrote.  Every element of every step against the float64 step from the kernel's own previous h, c."""
    worst = worst or Worst()
    fast = FAMILIES[fam]["fast"]
    N, T = A.shape[:2]
    wk = _w_fwd(whh, H, torch.float64)
    kf = dot_factor(fam, H)
    for n0, n1 in _blocks(N, T):
        n = n1 - n0
        g = _of(gin, n0, n1).double()
        hk, ck, Ak = _dirs(hout[n0:n1], H, dstride), cell[n0:n1], A[n0:n1]
        hp, cp = _shift(hk.double(), 1, -1), _shift(ck.double(), 1, -1)
        hp2 = hp.permute(2, 0, 1, 3).reshape(2, n * T, H)
        rec = torch.bmm(hp2, wk).view(2, n, T, H, 4).permute(1, 2, 0, 3, 4)
        S = torch.bmm(hp2.abs(), wk.abs()).view(2, n, T, H, 4).permute(1, 2, 0, 3, 4)
        a = g + rec
        ea = kf * S + U * a.abs()
        sg, th = torch.sigmoid(a), torch.tanh(a[..., 2])
        ref = sg.clone()
        ref[..., 2] = th
        eact = _through(ea, sg * (1 - sg), SIG_D2, sigmoid_err(a, sg, fast))
        eact[..., 2] = _through(ea[..., 2], 1 - th * th, TANH_D2, tanh_err(a[..., 2], th, fast))
        worst.add("act", Ak, ref, eact + U * ref.abs())
        i, f, gg, o = ref.unbind(-1)
        ei, ef, eg, eo = eact.unbind(-1)
        c = f * cp + i * gg
        ec = ef * cp.abs() + ei * gg.abs() + eg * i + ei * eg + 2 * U * ((f * cp).abs() + (i * gg).abs())
        worst.add("cell", ck, c, ec + U * c.abs() + TINY)
        tc = torch.tanh(c)
        etc = _through(ec, 1 - tc * tc, TANH_D2, tanh_err(c, tc, fast))
        h = o * tc
        eh = eo * tc.abs() + o * etc + eo * etc + 2 * U * h.abs() + TINY
        worst.add("h", hk, h, eh)
        worst.count += h.numel()
    return worst


def check_backward(A, cell, dhout, D, whh, H, dstride, fam, worst=None, blocks=None):
    """Section 3.  A (a tensor or a function of a block), cell, dhout: what the launch read; D: the d(pre-activations)
    it wrote.  dh from the kernel's own D of the next step, the carried dc by a float64 scan with its error alongside."""
    worst = worst or Worst()
    fast = FAMILIES[fam]["fast"]
    N, T = D.shape[:2]
    wb = _w_bwd(whh, H, torch.float64)
    kf = dot_factor(fam, 4 * H, backward=True)
    for n0, n1 in blocks or _blocks(N, T):
        n = n1 - n0
        a = _of(A, n0, n1).double()
        i, f, g, o = a.unbind(-1)
        c = cell[n0:n1].double()
        cp = _shift(c, 1, -1)
        Dk = D[n0:n1]
        Dn = _shift(Dk.double(), -1, 1).permute(2, 0, 1, 3, 4).reshape(2, n * T, 4 * H)
        rec = torch.bmm(Dn, wb).view(2, n, T, H).permute(1, 2, 0, 3)
        S = torch.bmm(Dn.abs(), wb.abs()).view(2, n, T, H).permute(1, 2, 0, 3)
        dh = _dirs(dhout[n0:n1], H, dstride).double() + rec
        edh = kf * S + U * dh.abs()
        tc = torch.tanh(c)
        etc = tanh_err(c, tc, fast)
        omt = 1 - tc * tc
        p = dh * o * omt
        ep = edh * o * omt + dh.abs() * o * (2 * tc.abs() * etc + etc * etc + U) + 3 * U * p.abs()
        fn = _shift(f, -1, 1)
        dc, E = torch.empty_like(p), torch.empty_like(p)
        for d, order in ((0, range(T - 1, -1, -1)), (1, range(T))):
            dcn = torch.zeros_like(p[:, 0, d])
            En = torch.zeros_like(dcn)
            for t in order:
                carried = fn[:, t, d] * dcn
                dcn = p[:, t, d] + carried
                En = ep[:, t, d] + fn[:, t, d] * En + U * carried.abs() + U * dcn.abs()
                dc[:, t, d], E[:, t, d] = dcn, En
        ref = torch.stack([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
        err = torch.stack([E * (g * i * (1 - i)).abs(), E * (cp * f * (1 - f)).abs(), E * i * (1 - g * g) + U * (dc * i).abs(),
                           edh * (tc * o * (1 - o)).abs() + dh.abs() * etc * o * (1 - o)], -1)
        worst.add("dgates", Dk, ref, err + 5 * U * ref.abs() + TINY)
        worst.count += ref.numel()
    return worst


# ---- section 4: plain time loops -----------------------------------------------------------------------------------
def lstm_forward_loop(gin, whh, H, dtype):
    """-> A [n, T, 2, H, 4], c, h [n, T, 2, H] of the recurrence in `dtype` (torch.nn.LSTM's arithmetic)"""
    g = gin.to(dtype)
    n, T = g.shape[:2]
    wk = _w_fwd(whh, H, dtype)
    A, C, Hh = torch.empty_like(g), torch.empty_like(g[..., 0]), torch.empty_like(g[..., 0])
    h = torch.zeros(2, n, H, dtype=dtype, device=g.device)
    c = torch.zeros(n, 2, H, dtype=dtype, device=g.device)
    for s in range(T):
        ts = (s, T - 1 - s)
        a = torch.stack([g[:, ts[0], 0], g[:, ts[1], 1]], 1) + torch.bmm(h, wk).view(2, n, H, 4).transpose(0, 1)
        act = torch.sigmoid(a)
        act[..., 2] = torch.tanh(a[..., 2])
        c = act[..., 1] * c + act[..., 0] * act[..., 2]
        hn = act[..., 3] * torch.tanh(c)
        for d in (0, 1):
            A[:, ts[d], d], C[:, ts[d], d], Hh[:, ts[d], d] = act[:, d], c[:, d], hn[:, d]
        h = hn.transpose(0, 1).contiguous()
    return A, C, Hh


def lstm_backward_loop(A, cell, dh_in, whh, H, dtype, wrong_f=False):
    """-> D [n, T, 2, H, 4] from saved A, cell [n, T, 2, H] and dh_in [n, T, 2, H].  wrong_f: the planted defect -- the
    carried dc is scaled by the forget gate of the step it arrives at instead of the one it leaves."""
    a, c, dh_in = A.to(dtype), cell.to(dtype), dh_in.to(dtype)
    n, T = a.shape[:2]
    wb = _w_bwd(whh, H, dtype)
    D = torch.empty_like(a)
    Dn = torch.zeros(2, n, 4 * H, dtype=dtype, device=a.device)
    dcc = torch.zeros(n, 2, H, dtype=dtype, device=a.device)
    zero = torch.zeros(n, H, dtype=dtype, device=a.device)
    for s in range(T):
        ts = (T - 1 - s, s)
        prev = (ts[0] - 1, ts[1] + 1)
        at = torch.stack([a[:, ts[0], 0], a[:, ts[1], 1]], 1)
        ct = torch.stack([c[:, ts[0], 0], c[:, ts[1], 1]], 1)
        last = s + 1 == T
        cp = torch.stack([zero if last else c[:, prev[0], 0], zero if last else c[:, prev[1], 1]], 1)
        dh = torch.stack([dh_in[:, ts[0], 0], dh_in[:, ts[1], 1]], 1) + torch.bmm(Dn, wb).transpose(0, 1)
        i, f, g, o = at.unbind(-1)
        tc = torch.tanh(ct)
        dc = dh * o * (1 - tc * tc) + dcc
        if wrong_f and not last:
            dcc = dc * torch.stack([a[:, prev[0], 0, :, 1], a[:, prev[1], 1, :, 1]], 1)
        else:
            dcc = dc * f
        d = torch.stack([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
        for k in (0, 1):
            D[:, ts[k], k] = d[:, k]
        Dn = d.transpose(0, 1).reshape(2, n, 4 * H)
    return D


def whole_sequence_multiple(fam, H):
    """Section 4: how many times the error of the fp32 torch loop a kernel's error over a whole sequence may be."""
    exact = 4.0     # two realisations of one error bound (2) x OCML's 3 - 5 ulp functions against libm's 1 (2)
    return exact * dot_factor(fam, H) / dot_factor("torch", H)


def make_whh(H, gen, device):
    b = H ** -0.5
    return [(torch.rand(4 * H, H, generator=gen, device=device) * 2 - 1) * b for _ in (0, 1)]


def packed(h4, ldo, dstride, fill=0.0):
    """[n, T, 2, H] -> hout layout [n, T, ldo]"""
    n, T, _, H = h4.shape
    out = torch.full((n, T, ldo), fill, dtype=h4.dtype, device=h4.device)
    for d in (0, 1):
        out[..., d * dstride:d * dstride + H] = h4[:, :, d]
    return out


# ---- section 6: the checker on the CPU -------------------------------------------------------------------------------
H6, T6, N6 = 300, 64, 4


@pytest.fixture(scope="module")
def cpu_case():
    gen = torch.Generator().manual_seed(29)
    whh = make_whh(H6, gen, "cpu")
    gin = torch.randn(N6, T6, 2, H6, 4, generator=gen)
    dh = torch.randn(N6, T6, 2, H6, generator=gen)
    return whh, gin, dh


def _forward(gin, whh_used, whh_true, fam="torch"):
    A, c, h = lstm_forward_loop(gin, whh_used, H6, torch.float32)
    return check_forward(gin, A, c, packed(h, 2 * H6, H6), whh_true, H6, H6, fam)


def test_fp32_torch_loop_passes_the_forward_bounds(cpu_case):
    whh, gin, _ = cpu_case
    for fam in FAMILIES:
        w = _forward(gin, whh, whh, fam)
        print(fam, w)
        assert w.ok() and w.count == N6 * T6 * 2 * H6, (fam, str(w))


def test_forward_bounds_are_not_vacuous(cpu_case):
    """the median bound of every output, on every family, is below 1e-4 at H = 300"""
    whh, gin, _ = cpu_case
    for fam in FAMILIES:
        w = _forward(gin, whh, whh, fam)
        for name in ("act", "cell", "h"):
            print(fam, name, w.median(name))
            assert w.median(name) < 1e-4, (fam, name, w.median(name))


def _bf16(w):
    return w.bfloat16().float()


def _cut(w):
    w = w.clone()
    w.view(4, H6, H6)[:, :, 288:] = 0
    return w


def _unit_missing(w):
    w = w.clone()
    w.view(4, H6, H6)[:, :, 299] = 0
    return w


def _o_row_zero(w):
    w = w.clone()
    w.view(4, H6, H6)[3, 299, :] = 0
    return w


@pytest.mark.parametrize("defect", [_bf16, _cut, _unit_missing, _o_row_zero], ids=lambda f: f.__name__.strip("_"))
@pytest.mark.parametrize("fam", ["stream", "onchip16"])
def test_planted_forward_defects_fail_the_bounds(cpu_case, defect, fam):
    whh, gin, _ = cpu_case
    w = _forward(gin, [defect(x) for x in whh], whh, fam)
    print(defect.__name__, fam, w, w.outside)
    assert not w.ok() and w.ratio["act"] > 1 and w.ratio["h"] > 1, str(w)


def _saved(cpu_case):
    whh, gin, dh = cpu_case
    A, c, _ = lstm_forward_loop(gin, whh, H6, torch.float64)
    return whh, A.float(), c.float(), dh


def test_fp32_torch_loop_passes_the_backward_bounds(cpu_case):
    whh, A, c, dh = _saved(cpu_case)
    D = lstm_backward_loop(A, c, dh, whh, H6, torch.float32)
    for fam in FAMILIES:
        w = check_backward(A, c, packed(dh, 2 * H6, H6), D, whh, H6, H6, fam)
        print(fam, w, w.median("dgates"))
        assert w.ok() and w.count == N6 * T6 * 2 * H6 * 4, (fam, str(w))


@pytest.mark.parametrize("defect", ["bf16", "cut", "unit_missing", "wrong_f"])
@pytest.mark.parametrize("fam", ["stream", "onchip16"])
def test_planted_backward_defects_fail_the_bounds(cpu_case, defect, fam):
    whh, A, c, dh = _saved(cpu_case)
    used = {"bf16": _bf16, "cut": _cut, "unit_missing": _unit_missing}.get(defect, lambda w: w)
    D = lstm_backward_loop(A, c, dh, [used(w) for w in whh], H6, torch.float32, wrong_f=defect == "wrong_f")
    w = check_backward(A, c, packed(dh, 2 * H6, H6), D, whh, H6, H6, fam)
    print(defect, fam, w, w.outside)
    assert not w.ok(), str(w)


def test_whole_sequence_multiples():
    """single digit for the exact-fp32 families; the split-bf16 ones: the ratio of the section 1 factors, computed"""
    assert whole_sequence_multiple("stream", 300) == 4.0
    m = whole_sequence_multiple("onchip16", 300)
    want = 4.0 * (C_SPLIT + LAMBDA * math.sqrt(916) * U) / (LAMBDA * math.sqrt(316) * U)
    assert abs(m - want) < 1e-12 and 4.0 < m < 40.0, m


def activation_grid():
    """Section 2: the multiples of 2^-12 in [-20, 20] and the special arguments"""
    grid = torch.arange(-20 * 4096, 20 * 4096 + 1, dtype=torch.float64) / 4096
    sn = 2.0 ** -126
    special = torch.tensor([30.0, 88.0, 100.0, 1e4, 0.0, sn, 2 * sn], dtype=torch.float64)
    return torch.cat([grid, special, -special]).float()


def test_activation_grid_avoids_the_rounding_ties():
    """Where float64 sigmoid / tanh round to 0, 1 or -1 in fp32 the kernels must return exactly that: no grid point may
    sit so close to where the rounding changes that an error inside the bound could flip it."""
    x = activation_grid().double()
    assert bool((x.float().double() == x).all()) and x.numel() > 160000
    for y in (torch.sigmoid(x), torch.tanh(x).abs()):
        gap = (1 - y - 2.0 ** -25).abs() / 2.0 ** -25      # distance of 1 - y from the tie below 1, relative
        # (tanh_err / (1 - y) <= (4 U 20 + 2 ULP + U) + U / (1 - y) at |x| <= 20: the last term is the final rounding
        # itself, the rest is 85 U = 5.1e-6 of 1 - y)
        assert float(gap.min()) > 1e-5, float(gap.min())
