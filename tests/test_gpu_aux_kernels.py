"""The speaker-embedding kernels of csrc/aux.hip -- tssep_cond_mul_aux_bwd / tssep_cond_cat_aux_bwd, tssep_instnorm_fwd /
_bwd (both axes), tssep_relu_fwd / _bwd, tssep_segment_mean_fwd / _bwd -- past their grid caps and at the long-form
shape, against the float64 references of tests/test_aux_kernel_reference.py computed on the device, element by element
within the bounds restated there.  Every output the C ABI is given directly starts as NaN, with a sentinel in its pad
columns; all inputs come from seeded generators.  tests/test_gpu_auxnet.py keeps the small-shape stage tests.

Sizes (test_the_cases_run_past_the_grid_caps):
    instance norm, last axis   40 963 rows (2.5 sweeps of 16 384 rows, 3 mod 4: a partial last block) as [1, 40963, C], and
                               the 40 964 rows of [7, 5852, C] through the C ABI with ld_y = ld_dx = C + 3; C in {5, 100, 513}
                               (idle lanes; an input ld of 516); the three (mode, unbiased) pairs
    instance norm, time axis   [3072, 3, 513] (27 648 workgroups, n < 4) and [2, 1878, 553] (a long column sum)
    ReLU                       20 481 rows x 513: 2.64 M float4 items at ld = 516 / 520 (2.5 sweeps of 1 048 576), the 4-byte
                               kernels through ld = 513 and through a base pointer one float behind a 16-byte boundary
    segment mean               3 072 sequences of 1 ... 17 rows, then 1 878 and 5 000 rows; C in {10, 513}; plain and fused ReLU
    d_aux                      mul (1282, 4, 1, 65, 513): 2.63 M reduce elements, two chunks, the second of one frame; both
                               combinations at (1, 8, 8, 1878, 513, 100): 30 chunks, trials = K; the 4-byte kernels through a
                               misaligned pre / dxs; a cat window that starts before F and ends at ld; NaN in every pad column
    edge values                NaN, +-Inf, +-0, +-2^-149, +-2^-126, a constant row and column in the first sweep and behind the
                               second (last-axis norm, ReLU), in single sequences (segment mean), one column (time-axis norm)

Finding, fixed in aux.hip: with `fmaxf(v, 0.f)` the ReLU kernels and the ReLU fused into the segment mean turned a NaN
into 0, where torch.nn.ReLU keeps it, and the masks `y > 0` stopped the gradient at a NaN activation, where torch's
threshold_backward (zero where result <= 0) passes it.  Against the library as it was, on an MI355X, test_relu failed on
all four paths (forward: 4 elements, got 0.0, want nan) and test_segment_mean[*-True] on 2 of 30 740 elements (got 0.2086,
want nan); nothing else in this file depended on the kernels' change.  The kernels now keep NaN (`v > 0 || v != v`) and pass
the gradient unless the activation is <= 0; finite inputs give the bits they gave before.

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report); the whole file takes about 5 s:
    d_aux            reduce past its sweep 0.115   long form mul 0.0016, cat 0.00079   path switches 16-byte 0.017, 4-byte 0.034
    instnorm rows    y 0.071   mean 0.999   rscale 0.040   dx 0.037
    instnorm time    y 0.092   mean 1.00    rscale 0.063   dx 0.052      ([3072, 3, 513])
    relu             0 differing elements
    segment mean     plain 0.40   fused ReLU 0.45      backward 0.99 (one rounding)
(mean: the bound is the one rounding of the mean, which a value just above a power of two uses up; the long forms sit far
below 1 because the bound adds 160 roundings' worth of sum|terms| where the errors of 15 000 terms mostly cancel.)
"""
import math

import pytest
import torch

import test_aux_kernel_reference as R
from test_aux_kernel_reference import ITEM_SWEEP, ROW_SWEEP, SUB, TINY_N, same, within_class
from test_gpu_stft_kernels import Ratios

pytestmark = pytest.mark.gpu

GIB = 1 << 30
DEV = "cuda"
NAN = float("nan")
INF = float("inf")
SENT = -777.0                     # pad columns: a value ReLU would change
E_SHAPE, E_UNSUPPORTED, E_NULL = -1, -3, -5      # include/tssep_hip.h

ROWS = 40963
ROW_LAYOUT = (7, 5852)            # 40 964 rows, trimmed to ROWS for the [1, ROWS, C] run
WIDTHS = (5, 100, 513)
MODES = [(0, False), (0, True), (1, False)]
TIME_CASES = [(3072, 3, 513), (2, 1878, 553)]
RELU_CASE = (20481, 513)
RELU_PATHS = {"v4": (516, 0), "v4_ld520": (520, 0), "scalar_ld513": (513, 0), "scalar_offset": (516, 1)}     # (ld, offset of y)
SEG_COUNT, SEG_LONG, SEG_WIDTHS = 3072, (1878, 5000), (10, 513)
# (combination, B, K, trials, T, F, E)
D_AUX_REDUCE = ("mul", 1282, 4, 1, 65, 513, 513)
D_AUX_LONG = [("mul", 1, 8, 8, 1878, 513, 513), ("cat", 1, 8, 8, 1878, 513, 100)]
# (combination, shape, ld_dxs, offset of dxs, offset of pre, 16-byte kernels?)
D_AUX_PATHS = [("mul", (2, 3, 2, 67, 513, 513), 516, 0, 1, False), ("mul", (2, 3, 2, 67, 513, 513), 516, 1, 0, False),
               ("cat", (2, 3, 2, 67, 513, 7), 520, 0, 0, True), ("cat", (2, 3, 2, 67, 513, 7), 524, 1, 0, False),
               ("cat", (2, 3, 2, 67, 513, 100), 616, 0, 0, True)]

WORST = Ratios()


def H():
    from tssep_amd import hip_ops
    return hip_ops


def L():
    from tssep_amd import _lib
    return _lib.lib()


def _p(t):
    return H()._p(t)


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def note(entry, check, v):
    WORST.add(f"{entry:<22}{check}", v)


@pytest.fixture(autouse=True)
def _device_memory_cap():
    """The GPU is shared: every test here stays under 16 GB of device memory at its peak."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 * GIB, f"peak device memory {peak / GIB:.1f} GiB"


def test_the_cases_run_past_the_grid_caps():
    assert ROW_SWEEP == 16384 and ITEM_SWEEP == 1048576
    assert ROWS >= 2.5 * ROW_SWEEP and ROWS % 4 == 3 and ROW_LAYOUT[0] * ROW_LAYOUT[1] == ROWS + 1
    assert set(WIDTHS) == {5, 100, 513} and (513 + 3) // 4 * 4 == 516 and len(MODES) == 3
    assert TIME_CASES[0][1] < 4 and TIME_CASES[0][0] * -(-TIME_CASES[0][2] // 64) == 27648 and TIME_CASES[1][1] == 1878
    rows, C = RELU_CASE
    assert rows * ((C + 3) // 4) >= 2.5 * ITEM_SWEEP and rows * C >= 2.5 * ITEM_SWEEP
    for ld, off in RELU_PATHS.values():          # the ABI's switch: every ld a multiple of 4 and every base on 16 bytes
        assert (ld % 4 == 0 and off == 0) == (ld in (516, 520) and off == 0)
    assert {k for k, (ld, off) in RELU_PATHS.items() if ld % 4 or off} == {"scalar_ld513", "scalar_offset"}
    lengths = R.segment_lengths(SEG_COUNT, SEG_LONG)
    assert set(lengths[:SEG_COUNT]) == set(range(1, 18)) and lengths[-2:] == [1878, 5000] and max(lengths) > 300
    comb, B, K, trials, T, F, E = D_AUX_REDUCE
    assert comb == "mul" and B * K * F >= 2.5 * ITEM_SWEEP and -(-T // 64) == 2 and T % 64 == 1
    assert B * trials * K * T * 516 * 4 < 0.75 * GIB
    for comb, B, K, trials, T, F, E in D_AUX_LONG:
        assert (K, trials, T) == (8, 8, 1878) and -(-T // 64) == 30
    assert {c[0] for c in D_AUX_LONG} == {"mul", "cat"}
    for comb, shape, ld, od, op, vec in D_AUX_PATHS:
        F, E = shape[4], shape[5]
        W = F if comb == "mul" else F + E
        c0 = 0 if comb == "mul" else F // 4 * 4
        assert vec == (ld % 4 == 0 and od == 0 and op == 0 and ld >= (W + 3) // 4 * 4) and ld >= W and (comb == "mul" or c0 < F)
    assert any(c == "cat" and ld == s[4] + s[5] and ld % 4 == 0 and s[4] % 2 for c, s, ld, _, _, _ in D_AUX_PATHS)
    assert any(c == "mul" and od == 0 and op == 1 for c, _, _, od, op, _ in D_AUX_PATHS)


# ------------------------------------------------------------------------------------------------- buffers, NaN outputs
def buf(rows, ld, C, fill=NAN, pad=SENT, offset=0):
    """[rows, ld] view whose first element lies `offset` floats behind a 16-byte boundary: `fill` in the C data columns,
    `pad` behind them"""
    base = torch.full((rows * ld + offset + 4,), pad, device=DEV)
    v = base[offset:offset + rows * ld].view(rows, ld)
    assert v.data_ptr() % 16 == 4 * offset
    v[:, :C] = fill
    return v


def load(a, ld, pad=0.0, offset=0):
    v = buf(a.shape[0], ld, a.shape[1], pad=pad, offset=offset)
    v[:, :a.shape[1]] = a
    return v


def pads_untouched(v, C, pad=SENT):
    return v.shape[1] == C or bool((v[:, C:] == pad).all())


def check(entry, name, got, ref, tol, nonfinite=None):
    r, n = within_class(got, ref.reshape(got.shape), tol.reshape(got.shape) if tol.numel() == got.numel() else tol,
                        f"{entry} {name}")
    note(entry, name, r)
    if nonfinite is not None:
        assert (n > 0) == nonfinite, (entry, name, n)
    return n


# ------------------------------------------------------------------------------------------- instance norm, last axis
def abi_instnorm(x, ld_x, dy, ld_dy, R_, n, C, axis, mode, unbiased, ld_out):
    rows, stats = R_ * n, (R_ * n if axis == 0 else R_ * C)
    y, dx = buf(rows, ld_out, C), buf(rows, ld_out, C)
    mean, rscale = torch.full((stats,), NAN, device=DEV), torch.full((stats,), NAN, device=DEV)
    _ok(L().tssep_instnorm_fwd(_p(x), ld_x, _p(y), ld_out, _p(mean), _p(rscale), R_, n, C, axis, mode, int(unbiased),
                               H()._stream()), "instnorm_fwd")
    _ok(L().tssep_instnorm_bwd(_p(dy), ld_dy, _p(x), ld_x, _p(mean), _p(rscale), _p(dx), ld_out, R_, n, C, axis, mode,
                               int(unbiased), H()._stream()), "instnorm_bwd")
    return y, mean, rscale, dx


@pytest.mark.parametrize("mode,unbiased", MODES)
@pytest.mark.parametrize("C", WIDTHS)
def test_instnorm_rows(C, mode, unbiased):
    """y, mean, rscale and dx of 40 963 rows through hip_ops ([1, 40963, C]: the third sweep ends in a block of three
    rows) and of all 40 964 through the C ABI as [7, 5852, C] with ld_y = ld_dx = C + 3 (the pads keep their sentinel),
    the two bit for bit alike.  Sequence 0 has |mean| / std ~ 200, centred lines carry a planted zero, and the edge values
    sit in rows 40 - 55 (first sweep) and 32 968 - 32 983 (behind the second): those rows are NaN exactly where the
    reference is, every other row meets its bound."""
    Rr, n = ROW_LAYOUT
    x = R.instnorm_input(Rr, n, C, 0, seed=1000 + C, device=DEV).view(Rr * n, C)
    for base in (40, 2 * ROW_SWEEP + 200):
        R.plant_edge_rows(x, base)
    dy = torch.randn(Rr * n, C, device=DEV, generator=R.gen(C, DEV))
    ref = R.ref_instnorm(x, dy, -1, mode, unbiased)
    assert int(torch.isnan(ref["y"][0]).all(1).sum()) == 8 and int(torch.isnan(ref["y"][0]).sum()) == 8 * C
    xt, dt = x[:ROWS].view(1, ROWS, C), dy[:ROWS].view(1, ROWS, C)
    y, mean, rscale, xinfo = H().instnorm_fwd(xt, 0, mode, unbiased)
    assert xinfo[1] == (C + 3) // 4 * 4
    dx = H().instnorm_bwd(dt, xinfo, mean, rscale, (1, ROWS, C), 0, mode, unbiased)
    got = {"y": y.view(ROWS, C), "mean": mean.view(ROWS, 1), "rscale": rscale.view(ROWS, 1), "dx": dx.view(ROWS, C)}
    for k, (rf, tol) in ref.items():
        check("instnorm rows", k, got[k], rf[:ROWS], tol[:ROWS], nonfinite=True)
    ldx = (C + 3) // 4 * 4
    y2, mean2, rscale2, dx2 = abi_instnorm(load(x, ldx), ldx, load(dy, ldx), ldx, Rr, n, C, 0, mode, unbiased, C + 3)
    assert pads_untouched(y2, C) and pads_untouched(dx2, C)
    got2 = {"y": y2[:, :C], "mean": mean2.view(-1, 1), "rscale": rscale2.view(-1, 1), "dx": dx2[:, :C]}
    for k, (rf, tol) in ref.items():
        check("instnorm rows", k, got2[k], rf, tol, nonfinite=True)
        assert bool(same(got2[k][:ROWS], got[k]).all()), k


# ------------------------------------------------------------------------------------------- instance norm, time axis
@pytest.mark.parametrize("mode,unbiased", MODES)
@pytest.mark.parametrize("Rr,n,C", TIME_CASES)
def test_instnorm_time(Rr, n, C, mode, unbiased):
    """[3072, 3, 513]: one workgroup per (sequence, 64 columns), three of four waves without a row to store; [2, 1878, 553]:
    118 additions per accumulator, a constant column and a column with one NaN in sequence 1 (NaN down those two columns
    and nowhere else)."""
    x = R.instnorm_input(Rr, n, C, 1, seed=n * 1000 + C, device=DEV)
    edges = n > 100
    if edges:
        x[1, :, 5] = 1.5
        x[1, 17, 9] = NAN
    dy = torch.randn(Rr, n, C, device=DEV, generator=R.gen(C + n, DEV))
    ref = R.ref_instnorm(x, dy, -2, mode, unbiased)
    assert int(torch.isnan(ref["y"][0]).sum()) == (2 * n if edges else 0)
    y, mean, rscale, xinfo = H().instnorm_fwd(x, 1, mode, unbiased)
    dx = H().instnorm_bwd(dy, xinfo, mean, rscale, (Rr, n, C), 1, mode, unbiased)
    got = {"y": y, "mean": mean.view(Rr, 1, C), "rscale": rscale.view(Rr, 1, C), "dx": dx}
    for k, (rf, tol) in ref.items():
        check("instnorm time", k, got[k], rf, tol, nonfinite=edges)
    ldx = (C + 3) // 4 * 4
    y2, mean2, rscale2, dx2 = abi_instnorm(load(x.view(Rr * n, C), ldx), ldx, load(dy.view(Rr * n, C), ldx), ldx, Rr, n, C, 1,
                                           mode, unbiased, C + 3)
    assert pads_untouched(y2, C) and pads_untouched(dx2, C)
    assert bool(same(y2[:, :C], y.view(Rr * n, C)).all()) and bool(same(dx2[:, :C], dx.view(Rr * n, C)).all())
    assert bool(same(mean2, mean.reshape(-1)).all()) and bool(same(rscale2, rscale.reshape(-1)).all())


# ---------------------------------------------------------------------------------------------------------------- ReLU
@pytest.mark.parametrize("path", list(RELU_PATHS))
def test_relu(path):
    """Forward (in place) and backward, exact against torch.relu and its autograd on the same data: NaN stays NaN and
    the gradient passes at a NaN activation.  The edge values sit in rows 3 - 18 and 20 451 - 20 466 (behind the second
    sweep of float4 items, which ends in row 16 257).  The 16-byte kernels may rewrite the pad columns 513 - 515; columns
    from 516 on, and every pad column on the 4-byte path, keep their sentinel."""
    rows, C = RELU_CASE
    ld, off = RELU_PATHS[path]
    g = R.gen(ld + off, DEV)
    x = torch.randn(rows, C, device=DEV, generator=g)
    dy = torch.randn(rows, C, device=DEV, generator=g)
    for base in (3, rows - 30):
        R.plant_edge_rows(x, base)
        x[base + 1, 7] = -NAN
    assert (rows - 30) * ((C + 3) // 4) > 2 * ITEM_SWEEP
    want_y, want_dx = R.ref_relu(x, dy)
    assert int(torch.isnan(want_y).sum()) == 4 and int(torch.isinf(want_y).sum()) == 2
    yb = load(x, ld, pad=SENT, offset=off)
    H().relu_fwd(yb, ld, rows, C)
    ok = same(yb[:, :C], want_y)
    assert bool(ok.all()), (path, "forward", int((~ok).sum()), yb[:, :C][~ok][:4].tolist(), want_y[~ok][:4].tolist())
    keep = C if (ld % 4 or off) else (C + 3) // 4 * 4
    assert pads_untouched(yb, keep), (path, "forward pads")
    dyb = load(dy, ld, pad=SENT)
    dxb = buf(rows, ld, C)
    _ok(L().tssep_relu_bwd(_p(dyb), ld, _p(yb), ld, _p(dxb), ld, rows, C, H()._stream()), "relu_bwd")
    ok = same(dxb[:, :C], want_dx)
    assert bool(ok.all()), (path, "backward", int((~ok).sum()), dxb[:, :C][~ok][:4].tolist(), want_dx[~ok][:4].tolist())
    assert pads_untouched(dxb, keep), (path, "backward pads")
    nan_at = torch.isnan(want_y)
    assert torch.equal(dxb[:, :C][nan_at], dy[nan_at])
    note("relu", "differing elements", 0.0)


# -------------------------------------------------------------------------------------------------------- segment mean
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", SEG_WIDTHS)
def test_segment_mean(C, relu):
    """3 074 sequences (1 ... 17 rows, then 1 878 and 5 000): the forward within (ceil(len / 16) + 7) U sum|terms| / len, the
    backward within one rounding, two runs bit for bit alike.  Edge values in single sequences: a NaN, an Inf and a -Inf
    each poison one column of one sequence (with the fused ReLU: NaN stays, -Inf becomes 0); +-2^-149 and +-2^-126 sit in
    sequences of one row, whose mean is the value itself."""
    lengths = R.segment_lengths(SEG_COUNT, SEG_LONG)
    S, N = len(lengths), sum(lengths)
    g = R.gen(C + relu, DEV)
    h = torch.randn(N, C, device=DEV, generator=g)
    dout = torch.randn(S, C, device=DEV, generator=g)
    row0 = H().segment_rows(lengths, DEV)
    b = row0.tolist()
    assert lengths[0] == lengths[17] == lengths[34] == 1 and lengths[5] == 6
    h[b[5] + 2, 1], h[b[7] + 1, 2], h[b[8], 3] = NAN, INF, -INF
    h[b[0], 4], h[b[17], 5], h[b[17], 6], h[b[34], 4], h[b[34], 5], h[b[34], 6] = SUB, -TINY_N, -0.0, -SUB, TINY_N, 0.0
    h[b[20] + 1] = 3.25
    h[b[21]:b[22], 7] = 1.5
    h[b[S - 1] + 4000, 2], h[b[S - 2] + 7, 3], h[b[S - 2] + 1500, 3] = NAN, INF, -INF
    ref, tol = R.ref_segment_mean(h, lengths, relu)
    assert int(torch.isnan(ref).sum()) == (2 if relu else 3) and int(torch.isinf(ref).sum()) == (2 if relu else 2)
    ld = (C + 3) // 4 * 4
    hv = load(h, ld)
    out = buf(S, ld + 4, C)
    _ok(L().tssep_segment_mean_fwd(_p(hv), ld, _p(row0), _p(out), ld + 4, S, C, int(relu), H()._stream()), "segment_mean_fwd")
    assert pads_untouched(out, C)
    name = "fused ReLU" if relu else "plain"
    check("segment mean", name, out[:, :C], ref, tol, nonfinite=True)
    again, _ = H().segment_mean_fwd(hv, ld, row0, S, C, relu=relu)
    assert bool(same(again[:, :C], out[:, :C]).all())
    assert float(out[0, 4]) == SUB and float(out[34, 5]) == TINY_N and float(out[17, 5]) == (0.0 if relu else -TINY_N)
    dh = buf(N, ld + 4, C)
    dv = load(dout, ld)
    _ok(L().tssep_segment_mean_bwd(_p(dv), ld, _p(hv) if relu else None, ld, _p(row0), _p(dh), ld + 4, S, C, int(relu),
                                   H()._stream()), "segment_mean_bwd")
    assert pads_untouched(dh, C)
    refb, tolb = R.ref_segment_mean_bwd(dout, h, lengths, relu)
    check("segment mean bwd", name, dh[:, :C], refb, tolb, nonfinite=False)
    if relu:
        assert float(dh[b[5] + 2, 1]) != 0 and float(dh[b[8], 3]) == 0          # the gradient passes at the NaN, not at -Inf


# ---------------------------------------------------------------------------------------------------------------- d_aux
def run_d_aux(comb, B, K, trials, T, F, E, ld, off_dxs=0, off_pre=0, seed=0):
    """dxs and pre with NaN in every pad column and, for cat, in the columns of the 16-byte window before F; d_aux and the
    workspace start as NaN.  -> (d_aux [B, K, C], the reference and its bound, the wrapper's arguments)"""
    mul = comb == "mul"
    C, W = (F, F) if mul else (E, F + E)
    dxs, pre = R.d_aux_inputs(B, K, trials, T, F, E, mul, seed, DEV)
    dv = load(dxs, ld, pad=NAN, offset=off_dxs)
    del dxs
    if not mul:
        dv[:, F // 4 * 4:F] = NAN
    ldp = (F + 3) // 4 * 4
    pv = load(pre, ldp, pad=NAN, offset=off_pre) if mul else None
    nbytes = int(L().tssep_cond_aux_bwd_workspace_bytes(B, K, T, F, 0 if mul else E))
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), NAN, device=DEV)
    out = buf(B * K, C + 1, C)
    if mul:
        rc = L().tssep_cond_mul_aux_bwd(_p(dv), ld, _p(pv), ldp, _p(out), C + 1, _p(ws), B, K, T, F, trials, H()._stream())
    else:
        rc = L().tssep_cond_cat_aux_bwd(_p(dv), ld, _p(out), C + 1, _p(ws), B, K, T, F, E, trials, H()._stream())
    _ok(rc, f"cond_{comb}_aux_bwd")
    assert pads_untouched(out, C)
    d5 = dv.view(B, trials, K, T, ld)[..., (0 if mul else F):(0 if mul else F) + C]
    ref, tol = R.ref_d_aux(d5, pv.view(B, T, ldp)[..., :F] if mul else None)
    return out[:, :C].reshape(B, K, C), ref, tol, (dv, ld, pv, ldp if mul else 0, B, K, T, F, E, trials, comb)


def test_d_aux_reduce_kernel_past_its_sweep():
    """mul, B K C = 2 630 664 reduce elements (2.5 sweeps), 15 384 x 2 partial workgroups, the second chunk one frame."""
    comb, B, K, trials, T, F, E = D_AUX_REDUCE
    got, ref, tol, _ = run_d_aux(comb, B, K, trials, T, F, E, 516, seed=1)
    check("d_aux", "reduce past its sweep", got, ref, tol, nonfinite=False)


@pytest.mark.parametrize("comb,B,K,trials,T,F,E", D_AUX_LONG)
def test_d_aux_long_form(comb, B, K, trials, T, F, E):
    """K = trials = 8, T = 1878: 30 chunks, every rotation of the speakers, 64-bit row offsets up to 120 192 rows."""
    ld = (F + 3) // 4 * 4 if comb == "mul" else (F + E + 3) // 4 * 4
    got, ref, tol, args = run_d_aux(comb, B, K, trials, T, F, E, ld, seed=2)
    check("d_aux", f"long form {comb}", got, ref, tol, nonfinite=False)
    assert torch.equal(H().cond_aux_bwd(*args), got)


@pytest.mark.parametrize("comb,shape,ld,off_dxs,off_pre,vec", D_AUX_PATHS)
def test_d_aux_path_switches(comb, shape, ld, off_dxs, off_pre, vec):
    """The 4-byte kernels through a pre (mul) or a dxs one float behind a 16-byte boundary while everything else is
    aligned; the cat window [512, 520) that starts before F = 513 and ends exactly at ld = F + E; the window [512, 616)
    at E = 100.  NaN in every column nobody may read."""
    B, K, trials, T, F, E = shape
    got, ref, tol, args = run_d_aux(comb, B, K, trials, T, F, E, ld, off_dxs, off_pre, seed=3)
    check("d_aux", f"path switches {'16-byte' if vec else '4-byte'}", got, ref, tol, nonfinite=False)
    assert torch.equal(H().cond_aux_bwd(*args), got)


# --------------------------------------------------------------------------------------------------------- status codes
def test_status_codes_without_a_launch():
    """Every refusal of aux.hip's argument checks, which come before any launch."""
    s = H()._stream()
    a = torch.zeros(64, device=DEV)
    i64 = torch.zeros(4, dtype=torch.int64, device=DEV)
    p, q = _p(a), _p(i64)
    mulf, catf = L().tssep_cond_mul_aux_bwd, L().tssep_cond_cat_aux_bwd
    # (dxs, ld_dxs, pre, ld_pre, d_aux, ld_daux, ws, B, K, T, F, trials) / (dxs, ld_dxs, d_aux, ld_daux, ws, B, K, T, F, E, trials)
    assert mulf(p, 8, p, 8, p, 8, p, 1, 2, 2, 8, 3, s) == E_SHAPE                       # trials > K
    assert catf(p, 12, p, 4, p, 1, 2, 2, 8, 4, 3, s) == E_SHAPE
    assert mulf(p, 7, p, 8, p, 8, p, 1, 2, 2, 8, 1, s) == E_SHAPE                       # ld < C
    assert mulf(p, 8, p, 7, p, 8, p, 1, 2, 2, 8, 1, s) == E_SHAPE
    assert mulf(p, 8, p, 8, p, 7, p, 1, 2, 2, 8, 1, s) == E_SHAPE
    assert catf(p, 11, p, 4, p, 1, 2, 2, 8, 4, 1, s) == E_SHAPE
    assert catf(p, 12, p, 3, p, 1, 2, 2, 8, 4, 1, s) == E_SHAPE
    assert mulf(p, 8, p, 8, p, 8, p, 1, 2, 65536 * 64, 8, 1, s) == E_SHAPE              # 65 536 chunks
    assert catf(p, 12, p, 4, p, 1, 2, 65536 * 64, 8, 4, 1, s) == E_SHAPE
    assert catf(p, 8, p, 4, p, 1, 2, 2, 8, 0, 1, s) == E_SHAPE                          # E = 0
    assert mulf(None, 8, p, 8, p, 8, p, 1, 2, 2, 8, 1, s) == E_NULL
    assert mulf(p, 8, None, 8, p, 8, p, 1, 2, 2, 8, 1, s) == E_NULL
    assert mulf(p, 8, p, 8, None, 8, p, 1, 2, 2, 8, 1, s) == E_NULL
    assert mulf(p, 8, p, 8, p, 8, None, 1, 2, 2, 8, 1, s) == E_NULL
    assert catf(None, 12, p, 4, p, 1, 2, 2, 8, 4, 1, s) == E_NULL and catf(p, 12, None, 4, p, 1, 2, 2, 8, 4, 1, s) == E_NULL
    assert catf(p, 12, p, 4, None, 1, 2, 2, 8, 4, 1, s) == E_NULL
    assert L().tssep_cond_aux_bwd_workspace_bytes(0, 2, 2, 8, 0) == 0
    fwd, bwd = L().tssep_instnorm_fwd, L().tssep_instnorm_bwd
    for axis, mode, unb in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (1, 1, -1)):
        assert fwd(p, 8, p, 8, p, p, 1, 2, 8, axis, mode, unb, s) == E_UNSUPPORTED
        assert bwd(p, 8, p, 8, p, p, p, 8, 1, 2, 8, axis, mode, unb, s) == E_UNSUPPORTED
    for axis in (0, 1):
        assert fwd(p, 7, p, 8, p, p, 1, 2, 8, axis, 0, 0, s) == E_SHAPE and fwd(p, 8, p, 7, p, p, 1, 2, 8, axis, 0, 0, s) == E_SHAPE
        assert fwd(p, 8, p, 8, p, p, 0, 2, 8, axis, 0, 0, s) == E_SHAPE
        for k in range(3):
            ld = [8, 8, 8]
            ld[k] = 7
            assert bwd(p, ld[0], p, ld[1], p, p, p, ld[2], 1, 2, 8, axis, 0, 0, s) == E_SHAPE
        for k in range(4):
            ptr = [p, p, p, p]
            ptr[k] = None
            assert fwd(ptr[0], 8, ptr[1], 8, ptr[2], ptr[3], 1, 2, 8, axis, 0, 0, s) == E_NULL
        for k in range(5):
            ptr = [p, p, p, p, p]
            ptr[k] = None
            assert bwd(ptr[0], 8, ptr[1], 8, ptr[2], ptr[3], ptr[4], 8, 1, 2, 8, axis, 0, 0, s) == E_NULL
    assert L().tssep_relu_fwd(None, 8, 2, 8, s) == E_NULL and L().tssep_relu_fwd(p, 7, 2, 8, s) == E_SHAPE
    assert L().tssep_relu_fwd(p, 8, 0, 8, s) == E_SHAPE
    for k in range(3):
        ptr, ld = [p, p, p], [8, 8, 8]
        ptr[k] = None
        assert L().tssep_relu_bwd(ptr[0], 8, ptr[1], 8, ptr[2], 8, 2, 8, s) == E_NULL
        ld[k] = 7
        assert L().tssep_relu_bwd(p, ld[0], p, ld[1], p, ld[2], 2, 8, s) == E_SHAPE
    sf, sb = L().tssep_segment_mean_fwd, L().tssep_segment_mean_bwd
    assert sf(None, 8, q, p, 8, 1, 8, 0, s) == E_NULL and sf(p, 8, None, p, 8, 1, 8, 0, s) == E_NULL
    assert sf(p, 8, q, None, 8, 1, 8, 0, s) == E_NULL
    assert sf(p, 7, q, p, 8, 1, 8, 0, s) == E_SHAPE and sf(p, 8, q, p, 7, 1, 8, 0, s) == E_SHAPE and sf(p, 8, q, p, 8, 0, 8, 0, s) == E_SHAPE
    assert sb(None, 8, p, 8, q, p, 8, 1, 8, 0, s) == E_NULL and sb(p, 8, p, 8, None, p, 8, 1, 8, 0, s) == E_NULL
    assert sb(p, 8, p, 8, q, None, 8, 1, 8, 0, s) == E_NULL and sb(p, 8, None, 8, q, p, 8, 1, 8, 1, s) == E_NULL
    assert sb(p, 7, p, 8, q, p, 8, 1, 8, 0, s) == E_SHAPE and sb(p, 8, p, 8, q, p, 7, 1, 8, 0, s) == E_SHAPE
    assert sb(p, 8, p, 7, q, p, 8, 1, 8, 1, s) == E_SHAPE
    torch.cuda.synchronize()
    assert not bool(a.any()) and not bool(i64.any())


def test_zz_report():
    """The worst err / bound of every kernel and case group of this file (pytest -rP)."""
    for k in sorted(WORST.r):
        print(f"max err/bound  {k}: {WORST.r[k]:.3g}")
    assert all(math.isfinite(v) and v <= 1.0 for v in WORST.r.values())
