"""The float64 references and element-wise bounds of the speaker-embedding kernels (csrc/aux.hip; the GPU side is
tests/test_gpu_aux_kernels.py), tested without a GPU.  The references restate the definitions -- InstanceNorm,
InstanceNorm_v2, AuxNet's ReLU and padded_sequence_reduction of the reference's net.py (tests/aux_reference.py), and the
conditioning sum d_aux[b, s, c] = sum_tr sum_t dxs[(b, tr, (s - tr) mod K, t), c0 + c] (* pre[(b, t), c] for mul) -- and
run on the device of their inputs.  Here they run on the CPU at reduced size: they are anchored against
tests/aux_reference.py and torch autograd, numpy fp32 emulations of each kernel's summation order must stay inside the
bounds, and the same outputs with eight defects planted must fall outside them.  Nothing here is compared with the code
under test.

Bounds (U = 2^-24), the ones derived in tests/test_gpu_auxnet.py, restated as functions:
  * d_aux: (d + 2) U sum|terms|, d = trials min(16, ceil(T / 4)) + 3 + ceil(T / 64) - 1 (a wave's running sum over its
    frames of a 64-frame chunk, trial after trial; the four waves; the chunks).
  * instance norm over N values, c = 4 (log2 N + 4):
      forward   |y - y64| <= c U (|y| + (|x| + |mean|) / std)
      backward  e_y = the forward bound, rel_r = c U (1 + (max|x| + |mean|) / std), r = 1 / std, b = sum(dy y) / dof:
                |dx - dx64| <= c U r (|dy| + mean|dy| + |y| sum|dy y| / dof) + r (e_y |b| + |y| sum(|dy| e_y) / dof)
                               + rel_r (|dx64| + 2 r |y| |b|)
      rscale    rel_r r (the relative error of r the backward bound is built on)
      mean      U |mean| + 2 (N + 8) 2^-53 mean|x|: the kernels add the N values in double, divide in double and round
                once; the second term covers that double sum and the float64 reference's own (any order of N additions
                is within (N - 1) 2^-53 sum|x|).
  * segment mean: (ceil(len / 16) + 7) U sum|terms| / len; its backward dout / len: one rounding, U |dout / len|.
  * ReLU forward and backward: exact, torch.relu and its autograd on the same fp32 data (NaN stays NaN, and the
    gradient passes where the activation is NaN: threshold_backward zeroes where result <= 0 only).

Input generators (shared with the GPU file): instnorm_input puts |mean| / std ~ 200 into sequence 0 (randn 0.5 + 100),
randn 5 - 5 into sequence 1, and centres every eighth reduction line of the sequences behind 0 to mean 1e-5 with one
element exactly 0: there the forward bound is 2 c U |mean| / std ~ 6e-11, which one rounding of the mean (6e-13)
meets and a chain of fp32 additions (1e-8) does not.

Measured here (pytest -rP), worst err / bound of the fp32 emulations at the reduced sizes:
    d_aux 0.058 (mul), 0.028 (cat)      instance norm y 0.072  mean 0.998  rscale 0.046  dx 0.034
    segment mean 0.20 (plain), 0.26 (ReLU)   segment-mean backward 0.92 (one rounding)   ReLU exact
(the mean's bound is one rounding, which a mean just above a power of two uses up.)
Planted defects, elements outside the bound (or unequal, for the exact comparisons) of the checked output:
    second sweep shifted by one block   instance norm y, the reduced d_aux, ReLU: more than 0.9 of the moved elements
    last partial chunk dropped          d_aux 108 of 108 (mul) and 48 of 48 (cat) at T = 65, one frame in the last chunk
    rotation (s + tr) mod K             d_aux 78 of 78 (mul), 42 of 42 (cat) at trials = 2, K = 3; all at trials = K = 8
    mean as an fp32 chain               the planted zero of every centred line: 5 of 5 (last axis, N = 513 and 100), up to
                                        358 times the bound; 9 of 9 (time axis, N = 150), up to 605 times
    uncentred variance                  on sequence 0: 5 752 of 21 033 elements (N = 513), 1 598 of 4 100 (N = 100), 102 of
                                        205 (N = 5), 6 356 of 10 500 (time axis, N = 150): the elements with |y| above ~0.5
    dof off by one                      46 189 of 63 099 elements (N = 513), 11 628 of 12 300 (N = 100), all at N = 5 and 3
    mean over the padded length         41 of 41 sequences shorter than the longest
    ReLU mask from the gradient         336 of 650 elements
"""
import math

import numpy as np
import pytest
import torch

import aux_reference as A

U = 2.0 ** -24
ROW_SWEEP = 4096 * 4             # aux.hip grid_for(rows, 4): rows one sweep of the row-wise norm covers
ITEM_SWEEP = 4096 * 256          # aux.hip grid_for(n): items (floats, float4s, reduce elements) per sweep
TCH = 64                         # frames per chunk of the d_aux partials
f32, f64 = np.float32, np.float64


def gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


# ------------------------------------------------------------------------------------------------------- comparison
def within_class(got, ref, tol, name):
    """Every element of the fp32 `got` has the class of the float64 `ref` (NaN, +Inf, -Inf, finite; the sign of a zero
    is not compared) and, where ref is finite, |got - ref| <= tol.  -> (max err / tol over the finite elements, number
    of non-finite reference elements)."""
    g = got.double()
    fin = torch.isfinite(ref)
    ok = torch.where(fin, torch.isfinite(g) & ((g - ref).abs() <= torch.broadcast_to(tol, ref.shape)),
                     torch.where(torch.isnan(ref), torch.isnan(g), g == ref))
    if not bool(ok.all()):
        bad = ~ok
        i = int(bad.reshape(-1).nonzero()[0])
        idx = np.unravel_index(i, tuple(ref.shape))
        t = torch.broadcast_to(tol, ref.shape)
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the tolerance or of another class; "
                             f"first at {idx}: got {float(g[idx]):.9g}, want {float(ref[idx]):.9g}, tol {float(t[idx]):.3g}")
    err = (g - ref).abs()
    ratio = torch.where(fin & (err > 0), err / tol, torch.zeros_like(err))
    return float(ratio.max()), int((~fin).sum())


def outside(got, ref, tol):
    """number of elements that within_class would refuse"""
    g = got.double()
    fin = torch.isfinite(ref)
    ok = torch.where(fin, torch.isfinite(g) & ((g - ref).abs() <= torch.broadcast_to(tol, ref.shape)),
                     torch.where(torch.isnan(ref), torch.isnan(g), g == ref))
    return int((~ok).sum())


def same(got, ref):
    """exact: equal, or both NaN (the sign of a zero is not compared)"""
    return (got == ref) | (torch.isnan(got) & torch.isnan(ref))


# ------------------------------------------------------------------------------------------------------------ d_aux
def d_aux_depth(trials, T):
    return trials * min(16, -(-T // 4)) + 3 + (-(-T // TCH) - 1)


def d_aux_inputs(B, K, trials, T, F, E, mul, seed, device="cpu"):
    """-> dxs [B trials K T, W], pre [B T, F] fp32 (W = F for mul, F + E for cat)"""
    g = gen(seed, device)
    dxs = torch.randn(B * trials * K * T, F if mul else F + E, device=device, generator=g)
    pre = torch.randn(B * T, F, device=device, generator=g) + 0.5
    return dxs, pre


def ref_d_aux(d5, p3, defect=None):
    """d5 [B, trials, K, T, C] fp32 (a view of the C columns of dxs that count), p3 [B, T, C] fp32 or None (cat)
    -> (d_aux [B, K, C] float64, its bound)"""
    B, trials, K, T, C = d5.shape
    want = torch.zeros(B, K, C, dtype=torch.float64, device=d5.device)
    mag = torch.zeros_like(want)
    Tu = T - T % TCH if defect == "drop_last_chunk" and T % TCH else T
    for s in range(K):
        for tr in range(trials):
            k = (s + tr) % K if defect == "rotation" else (s - tr) % K
            terms = d5[:, tr, k, :Tu].double()
            if p3 is not None:
                terms = terms * p3[:, :Tu].double()
            want[:, s] += terms.sum(1)
            mag[:, s] += terms.abs().sum(1)
    return want, (d_aux_depth(trials, T) + 2) * U * mag


def emu_d_aux(d5, p3):
    """The kernels' order in fp32 (numpy): per 64-frame chunk wave w adds the frames t0 + w, t0 + w + 4, ... of trial 0,
    then of trial 1, ... into one accumulator (each product rounded first), wave 0 adds the four waves in ascending
    order, the reduce kernel adds the chunks in ascending order."""
    B, trials, K, T, C = d5.shape
    out = None
    for t0 in range(0, T, TCH):
        t1 = min(T, t0 + TCH)
        red = []
        for w in range(4):
            acc = np.zeros((B, K, C), f32)
            for tr in range(trials):
                k = (np.arange(K) - tr) % K
                for t in range(t0 + w, t1, 4):
                    term = d5[:, tr, k, t]
                    acc = acc + (term * p3[:, None, t] if p3 is not None else term)
            red.append(acc)
        part = ((red[0] + red[1]) + red[2]) + red[3]
        out = part if out is None else out + part
    assert out.dtype == f32
    return out


def shift_second_sweep(a, sweep, block):
    """The defect of a grid-stride loop whose second pass starts one block late: items [sweep, 2 sweep) of a (along
    axis 0) come from [sweep + block, 2 sweep + block)."""
    n = a.shape[0]
    assert n >= 2 * sweep + block
    out = a.clone()
    out[sweep:2 * sweep] = a[sweep + block:2 * sweep + block]
    return out


# ---------------------------------------------------------------------------------------------------- instance norm
def instnorm_c(N):
    return 4 * (math.log2(N) + 4)


def instnorm_input(R, n, C, axis, seed, device="cpu"):
    """fp32 [R, n, C] (axis 0: statistics over C, one line per row; axis 1: over n, one line per (sequence, column)).
    Sequence 0: randn 0.5 + 100, |mean| / std ~ 200; sequence 1: randn 5 - 5; every eighth line (from the third) of the
    sequences behind 0, if it holds at least 8 values: mean 1e-5 and one element exactly 0."""
    g = gen(seed, device)
    x = torch.randn(R, n, C, device=device, generator=g, dtype=torch.float64)
    x[0] = x[0] * 0.5 + 100.0
    if R > 1:
        x[1] = x[1] * 5 - 5
    N = C if axis == 0 else n
    if N >= 8 and R > 1:
        v = x[1:] if axis == 0 else x[1:].transpose(1, 2)          # [R - 1, lines, N] views
        lines = torch.arange(3, v.shape[1], 8, device=device)
        j = (lines % N)[None, :, None].expand(R - 1, -1, 1)
        c = torch.randn(R - 1, lines.numel(), N, device=device, generator=g, dtype=torch.float64)
        c.scatter_(2, j, 0.0)
        c += (1e-5 * N - c.sum(2, keepdim=True)) / (N - 1)
        c.scatter_(2, j, 0.0)
        v[:, lines] = c
    return x.float()


def centred_lines(R, n, C, axis):
    """-> (line indices within a sequence, position of the planted zero in each) of instnorm_input"""
    N = C if axis == 0 else n
    lines = torch.arange(3, n if axis == 0 else C, 8)
    return (lines, lines % N) if (N >= 8 and R > 1) else (lines[:0], lines[:0])


def ref_instnorm(x, dy, dim, mode, unbiased):
    """x, dy fp32 -> {name: (float64 reference, bound)} of y, mean, rscale, dx for statistics along `dim`.
    mode 0: (x - mean) / std with N - unbiased in std's denominator (InstanceNorm); mode 1: the centred x over
    ||x - mean|| / sqrt(N) (InstanceNorm_v2); dx = r (dy - mean(dy) - y sum(dy y) / dof) is their gradient."""
    x, g = x.double(), dy.double()
    N = x.shape[dim]
    dof = N - 1 if (mode == 0 and unbiased) else N
    kw = dict(dim=dim, keepdim=True)
    # (a true division by a tensor: x.mean and a division by a Python number multiply by 1 / N on the device, which
    # misses the exact mean of a constant line)
    m = x.sum(**kw) / torch.full((), N, dtype=torch.float64, device=x.device)
    xc = x - m
    s = ((xc * xc).sum(**kw) / dof).sqrt() if mode == 0 else torch.linalg.norm(xc, **kw) / math.sqrt(N)
    y, r = xc / s, 1.0 / s
    c = instnorm_c(N)
    e_y = c * U * (y.abs() + (x.abs() + m.abs()) / s)
    b = (g * y).sum(**kw) / dof
    dx = r * (g - g.mean(**kw) - y * b)
    rel_r = c * U * (1 + (x.abs().amax(**kw) + m.abs()) / s)
    e_dx = c * U * r * (g.abs() + g.abs().mean(**kw) + y.abs() * (g * y).abs().sum(**kw) / dof) \
        + r * (e_y * b.abs() + y.abs() * (g.abs() * e_y).sum(**kw) / dof) + rel_r * (dx.abs() + 2 * r * y.abs() * b.abs())
    e_m = U * m.abs() + 2 * (N + 8) * 2.0 ** -53 * x.abs().mean(**kw)
    return {"y": (y, e_y), "mean": (m, e_m), "rscale": (r, rel_r * r), "dx": (dx, e_dx)}


def _wave_sum64(t):
    """t float64 [..., C] -> [..., 1]: lane l adds its columns l, l + 64, ... in ascending order, then the xor tree"""
    C = t.shape[-1]
    pad = np.zeros(t.shape[:-1] + (-C % 64,), f64)
    v = np.concatenate([t, pad], -1).reshape(t.shape[:-1] + (-1, 64))
    v = np.cumsum(v, axis=-2)[..., -1, :]
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return v[..., :1]


def _time_sum(t, dtype):
    """t [..., n, C] -> [..., 1, C]: wave w, accumulator u add the rows w + 4 u (mod 16) in ascending order; the four
    accumulators pairwise, then the four waves in ascending order (aux.hip time_sum)"""
    t = t.astype(dtype)
    waves = []
    for w in range(4):
        acc = []
        for u in range(4):
            rows = t[..., w + 4 * u::16, :]
            acc.append(np.cumsum(rows, axis=-2, dtype=dtype)[..., -1:, :] if rows.shape[-2]
                       else np.zeros(t.shape[:-2] + (1, t.shape[-1]), dtype))
        waves.append((acc[0] + acc[1]) + (acc[2] + acc[3]))
    out = ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert out.dtype == dtype
    return out


def emu_instnorm(x, dy, axis, mode, unbiased, defect=None):
    """The kernels in numpy: statistics accumulated in double in the kernel's order and rounded once, everything else
    fp32.  x, dy fp32 arrays [R, n, C] -> y, mean, rscale, dx (fp32).  defect: 'mean_chain' (the mean as a running fp32
    sum), 'uncentred' (sum x^2 - N mean^2 in fp32), 'dof' (biased and unbiased swapped)."""
    assert x.dtype == f32 and dy.dtype == f32
    ax = -1 if axis == 0 else -2
    N = x.shape[ax]
    summ = _wave_sum64 if axis == 0 else (lambda t: _time_sum(t, f64))
    if defect == "dof":
        unbiased = not unbiased
    if defect == "mean_chain":
        m = np.take(np.cumsum(x, axis=ax, dtype=f32), [-1], axis=ax) / f32(N)
    else:
        m = (summ(x.astype(f64)) / f64(N)).astype(f32)
    if defect == "uncentred":
        ss = np.sum(x * x, axis=ax, keepdims=True, dtype=f32) - f32(N) * m * m
    else:
        d = (x - m).astype(f64)
        ss = summ(d * d).astype(f32)
    dof = f32(N - (1 if (mode == 0 and unbiased) else 0))
    with np.errstate(all="ignore"):
        sc = np.sqrt(ss / dof) if mode == 0 else np.sqrt(ss) / np.sqrt(f32(N))
        y = (x - m) / sc
        r = f32(1) / sc
        yh = (x - m) * r
        a = (summ(dy.astype(f64)) / f64(N)).astype(f32)
        b = (summ(dy.astype(f64) * yh.astype(f64)) / f64(dof)).astype(f32)
        dx = r * ((dy - a) - yh * b)
    assert all(v.dtype == f32 for v in (y, m, r, dx))
    return {"y": y, "mean": m, "rscale": r, "dx": dx}


# -------------------------------------------------------------------------------------------- ReLU and segment mean
def ref_relu(x, dy):
    """torch.nn.ReLU and its autograd on the fp32 data themselves -> (y, dx)"""
    xg = x.detach().clone().requires_grad_()
    y = torch.relu(xg)
    (dx,) = torch.autograd.grad(y, xg, dy)
    return y.detach(), dx


def segment_ids(lengths, device="cpu"):
    return torch.repeat_interleave(torch.arange(len(lengths), device=device), torch.as_tensor(lengths, device=device))


def ref_segment_mean(h, lengths, relu, defect=None):
    """h fp32 [sum(lengths), C]: the mean over each sequence's own rows (padded_sequence_reduction, op = mean), of
    ReLU(h) with relu -> (out [S, C] float64, bound)"""
    v = torch.relu(h.double()) if relu else h.double()
    ids = segment_ids(lengths, h.device)
    lens = torch.as_tensor(lengths, dtype=torch.float64, device=h.device)[:, None]
    z = torch.zeros(len(lengths), h.shape[1], dtype=torch.float64, device=h.device)
    sums, mag = z.index_add(0, ids, v), z.index_add(0, ids, v.abs())
    div = lens.max() if defect == "padded_length" else lens
    return sums / div, ((lens / 16).ceil() + 7) * U * mag / lens


def ref_segment_mean_bwd(dout, h, lengths, relu):
    """-> (dh [sum(lengths), C] float64, bound): dout / len on every row of the sequence, through ReLU's autograd mask
    (zero where the activation is <= 0, so the gradient passes at a NaN)"""
    ids = segment_ids(lengths, dout.device)
    lens = torch.as_tensor(lengths, dtype=torch.float64, device=dout.device)[:, None]
    want = (dout.double() / lens)[ids]
    if relu:
        want = torch.where(h <= 0, torch.zeros_like(want), want)
    return want, U * want.abs()


def emu_segment_mean(h, lengths, relu):
    """numpy fp32 in the kernel's order (time_sum in fp32, one division)"""
    out, a = [], 0
    for n in lengths:
        seg = h[a:a + n]
        if relu:
            seg = np.where(seg < 0, f32(0), seg)
        out.append(_time_sum(seg, f32)[0] / f32(n))
        a += n
    return np.stack(out)


def segment_lengths(S, long=(1878, 5000)):
    """S lengths cycling through 1 ... 17, then the long ones"""
    return [1 + i % 17 for i in range(S)] + list(long)


# ------------------------------------------------------------------------------------------------------- edge values
SUB, TINY_N = 2.0 ** -149, 2.0 ** -126
EDGE_ROWS = 16                   # rows plant_edge_rows uses from `base` on


def plant_edge_rows(x2, base):
    """x2 fp32 [rows, C >= 5]: NaN, +-Inf, +-0, +-2^-149, +-2^-126, a constant row and a constant column (over one block
    of four rows) from row `base` on, every second row left as it is.  -> the rows that hold a NaN or an Inf and the
    constant row (the rows a per-row statistic turns into NaN)."""
    C = x2.shape[1]
    x2[base + 0, 1] = float("nan")
    x2[base + 2, 0] = float("inf")
    x2[base + 4, C - 1] = float("-inf")
    x2[base + 6, 0], x2[base + 6, 2] = 0.0, -0.0
    x2[base + 8, 0], x2[base + 8, 1], x2[base + 8, 3], x2[base + 8, 4] = SUB, -SUB, TINY_N, -TINY_N
    x2[base + 10] = 3.25
    x2[base + 12:base + 16, 3] = 1.5
    return [base + 0, base + 2, base + 4], base + 10


# ============================================================================================================ tests
D_AUX_SMALL = [(3, 4, 1, 65, 9, 4), (2, 3, 2, 67, 13, 7), (1, 8, 8, 130, 9, 4)]     # (B, K, trials, T, F, E)


def _d5(dxs, pre, B, K, trials, T, F, E, mul):
    d5 = dxs.view(B, trials, K, T, -1)[..., (0 if mul else F):(F if mul else F + E)]
    return d5, (pre.view(B, T, F) if mul else None)


@pytest.mark.parametrize("mul", [True, False])
def test_d_aux_reference_emulation_and_defects(mul):
    """The reference is the gradient of aux_reference.condition with respect to the embedding (autograd, float64); the
    fp32 emulation of the kernels' order stays inside the bound; the dropped last chunk and the reversed rotation fall
    outside it, and so does a reduce kernel whose second sweep starts one block late."""
    worst = 0.0
    for B, K, trials, T, F, E in D_AUX_SMALL:
        dxs, pre = d_aux_inputs(B, K, trials, T, F, E, mul, seed=T + F)
        d5, p3 = _d5(dxs, pre, B, K, trials, T, F, E, mul)
        ref, tol = ref_d_aux(d5, p3)
        aux = torch.randn(B, K, F if mul else E, dtype=torch.float64, generator=gen(1)).requires_grad_()
        xs = A.condition(pre.double().view(B, T, F), aux, "mul" if mul else "cat", trials)
        (want,) = torch.autograd.grad(xs, aux, dxs.double().view(xs.shape))
        assert float((ref - want).abs().max()) <= 1e-12 * float(want.abs().max())
        emu = torch.as_tensor(emu_d_aux(d5.numpy(), p3.numpy() if mul else None))
        r, nonfinite = within_class(emu, ref, tol, "d_aux emulation")
        assert nonfinite == 0
        worst = max(worst, r)
        assert outside(ref.float(), ref, tol) == 0
        if T % TCH:
            bad, _ = ref_d_aux(d5, p3, defect="drop_last_chunk")
            n = outside(bad.float(), ref, tol)
            print(f"d_aux {'mul' if mul else 'cat'} T={T}: last partial chunk dropped: {n} of {ref.numel()} outside")
            assert n > 0.9 * ref.numel()
        if trials > 1:
            bad, _ = ref_d_aux(d5, p3, defect="rotation")
            n = outside(bad.float(), ref, tol)
            print(f"d_aux {'mul' if mul else 'cat'} K={K} trials={trials}: rotation (s + tr): {n} of {ref.numel()} outside")
            assert n > 0.9 * ref.numel()
        flat, sweep, block = ref.float().reshape(-1), ref.numel() // 3, 2
        moved = shift_second_sweep(flat, sweep, block)
        assert outside(moved, ref.reshape(-1), tol.reshape(-1)) >= 0.9 * sweep
    print(f"d_aux {'mul' if mul else 'cat'} emulation: worst err/bound {worst:.3g}")
    assert worst <= 1.0


INSTNORM_SMALL = [(0, 3, 41, 5), (0, 3, 41, 100), (0, 3, 41, 513), (1, 40, 3, 70), (1, 2, 150, 70)]   # (axis, R, n, C)
MODES = [(0, False), (0, True), (1, False)]


@pytest.mark.parametrize("mode,unbiased", MODES)
def test_instnorm_reference_emulation_and_defects(mode, unbiased):
    """The reference is aux_reference.instance_norm / instance_norm_v2 and its autograd; the emulation (double
    statistics rounded once, fp32 elsewhere) stays inside all four bounds on instnorm_input; a chained fp32 mean fails
    at the planted zeros of the centred lines, an uncentred variance fails on sequence 0, a dof off by one fails
    everywhere, and a second sweep of rows shifted by one block fails."""
    worst = {}
    for axis, R, n, C in INSTNORM_SMALL:
        dim = -1 if axis == 0 else -2
        N = C if axis == 0 else n
        x = instnorm_input(R, n, C, axis, seed=n * 1000 + C)
        dy = torch.randn(R, n, C, generator=gen(C + n))
        ref = ref_instnorm(x, dy, dim, mode, unbiased)
        x64 = x.double().requires_grad_()
        y64 = A.instance_norm(x64, dim, unbiased) if mode == 0 else A.instance_norm_v2(x64, dim, dim)
        (dx64,) = torch.autograd.grad(y64, x64, dy.double())
        assert float((ref["y"][0] - y64.detach()).abs().max()) <= 1e-9
        assert float(((ref["dx"][0] - dx64).abs() / (dx64.abs() + 1e-3)).max()) <= 1e-9
        emu = emu_instnorm(x.numpy(), dy.numpy(), axis, mode, unbiased)
        for k, (rf, tol) in ref.items():
            got = torch.as_tensor(emu[k]).reshape(rf.shape)
            r, nonfinite = within_class(got, rf, tol, f"instnorm emulation {k} {(axis, R, n, C)}")
            assert nonfinite == 0
            worst[k] = max(worst.get(k, 0.0), r)
            assert outside(rf.float(), rf, tol) == 0, k
        yref, ytol = ref["y"]
        # the planted zeros: a chained fp32 mean
        lines, pos = centred_lines(R, n, C, axis)
        if lines.numel():
            bad = torch.as_tensor(emu_instnorm(x.numpy(), dy.numpy(), axis, mode, unbiased, defect="mean_chain")["y"])
            pick = (lambda t: t[2, lines, pos]) if axis == 0 else (lambda t: t[1, pos, lines])
            assert bool((pick(x) == 0).all())
            ratio = (pick(bad).double() - pick(yref)).abs() / pick(ytol)
            print(f"instnorm {(axis, R, n, C)} fp32-chain mean at the planted zeros: {int((ratio > 1).sum())} of {ratio.numel()} "
                  f"lines outside, up to {float(ratio.max()):.3g} x bound")
            assert N < 100 or bool((ratio > 1).all())
            assert outside(bad, yref, ytol) > 0 or N < 100
        bad = torch.as_tensor(emu_instnorm(x.numpy(), dy.numpy(), axis, mode, unbiased, defect="uncentred")["y"])
        n_out, n0 = outside(bad[0], yref[0], ytol[0]), yref[0].numel()
        print(f"instnorm {(axis, R, n, C)} uncentred variance on sequence 0: {n_out} of {n0} outside")
        assert n_out > 0.2 * n0          # (an error of a few ulp of sum x^2 ~ 1e4 N: rows with small |y| survive it)
        if mode == 0:
            bad = torch.as_tensor(emu_instnorm(x.numpy(), dy.numpy(), axis, mode, unbiased, defect="dof")["y"])
            n_out = outside(bad, yref, ytol)
            print(f"instnorm {(axis, R, n, C)} dof off by one: {n_out} of {yref.numel()} outside")
            assert n_out > 0.5 * yref.numel()          # (a relative 1 / (2 N) of y: elements with small |y| survive it)
        if axis == 0:                                    # 123 rows, a sweep of 32 rows, blocks of 4
            rows = torch.as_tensor(emu["y"]).reshape(R * n, C)
            moved = shift_second_sweep(rows, 32, 4)
            n_out = outside(moved, yref.reshape(R * n, C), ytol.reshape(R * n, C))
            assert n_out > 0.9 * 32 * C, n_out
    print(f"instnorm mode={mode} unbiased={unbiased} emulation: worst err/bound " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize("relu", [False, True])
def test_segment_mean_reference_emulation_and_defects(relu):
    """The reference against a plain loop over the sequences and its autograd; the fp32 emulation inside the bound; the
    mean over the padded length outside it for every sequence shorter than the longest."""
    lengths = segment_lengths(40, long=(150, 300))
    N, C = sum(lengths), 10
    h = torch.randn(N, C, generator=gen(3))
    dout = torch.randn(len(lengths), C, generator=gen(4))
    ref, tol = ref_segment_mean(h, lengths, relu)
    h64 = h.double().requires_grad_()
    v = torch.relu(h64) if relu else h64
    b = np.concatenate([[0], np.cumsum(lengths)])
    loop = torch.stack([v[a:e].mean(0) for a, e in zip(b[:-1], b[1:])])
    assert float((loop.detach() - ref).abs().max()) <= 1e-14
    (dh,) = torch.autograd.grad(loop, h64, dout.double())
    refb, tolb = ref_segment_mean_bwd(dout, h, lengths, relu)
    assert float((dh - refb).abs().max()) <= 1e-15
    emu = torch.as_tensor(emu_segment_mean(h.numpy(), lengths, relu))
    r, _ = within_class(emu, ref, tol, "segment mean emulation")
    rb, _ = within_class(refb.float(), refb, tolb, "segment mean backward, rounded")
    print(f"segment mean relu={relu}: emulation worst err/bound {r:.3g}; backward (one rounding) {rb:.3g}")
    bad, _ = ref_segment_mean(h, lengths, relu, defect="padded_length")
    wrong = (~((bad.float().double() - ref).abs() <= tol)).any(1)
    short = torch.as_tensor(lengths) < max(lengths)
    print(f"segment mean relu={relu}: mean over the padded length: {int(wrong.sum())} of {int(short.sum())} shorter sequences outside")
    assert torch.equal(wrong, short)


def test_relu_reference_and_the_mask_defect():
    """torch.relu keeps NaN, its gradient passes where the activation is NaN and nowhere else outside y > 0; a mask taken
    from the gradient's sign instead of the activation's is caught by the exact comparison."""
    x = torch.randn(50, 13, generator=gen(5))
    dy = torch.randn(50, 13, generator=gen(6))
    x[3, 4], x[7, 0], x[9, 1], x[11, 2], x[12, 3] = float("nan"), float("inf"), float("-inf"), -0.0, SUB
    y, dx = ref_relu(x, dy)
    assert math.isnan(float(y[3, 4])) and float(y[7, 0]) == math.inf and float(y[9, 1]) == 0 and float(y[12, 3]) == SUB
    assert float(dx[3, 4]) == float(dy[3, 4]) and float(dx[9, 1]) == 0 and float(dx[11, 2]) == 0 and float(dx[12, 3]) == float(dy[12, 3])
    fin = ~torch.isnan(x)
    assert torch.equal(dx[fin], (dy * (x > 0))[fin])
    # the activation, not the input, is what the backward kernel is given: the same mask
    y2, dx2 = ref_relu(y, dy)
    assert bool(same(y2, y).all()) and torch.equal(dx2, dx)
    bad = torch.where(dy > 0, dy, torch.zeros_like(dy))
    n = int((~same(bad, dx)).sum())
    print(f"ReLU mask from the gradient: {n} of {dx.numel()} elements differ")
    assert n > 0.3 * dx.numel()
    moved = shift_second_sweep(y.reshape(-1), 200, 3)
    assert int((~same(moved, y.reshape(-1))).sum()) > 100


def test_the_reference_carries_the_edge_values():
    """On the edge-value inputs of the GPU file the float64 references are NaN exactly where the definition says -- the
    rows (columns, for the time axis) that hold a NaN or an Inf and the constant ones -- and finite everywhere else, so
    every other row still has a bound to meet; the segment mean is NaN / Inf in the poisoned columns of single
    sequences only."""
    R, n, C = 3, 41, 100
    for mode, unbiased in MODES:
        x = instnorm_input(R, n, C, 0, seed=7)
        poisoned, const = plant_edge_rows(x.view(R * n, C), 60)
        dy = torch.randn(R, n, C, generator=gen(8))
        ref = ref_instnorm(x, dy, -1, mode, unbiased)
        nan_rows = sorted(poisoned + [const])
        for k in ("y", "dx"):
            rf, tol = (t.view(R * n, C) for t in ref[k])
            assert torch.isnan(rf).all(1).nonzero().flatten().tolist() == nan_rows, k
            keep = torch.ones(R * n, dtype=torch.bool)
            keep[nan_rows] = False
            assert bool(torch.isfinite(rf[keep]).all()) and bool((tol[keep] > 0).all()) and bool(torch.isfinite(tol[keep]).all())
        assert float(ref["rscale"][0].view(-1)[const]) == math.inf and float(ref["mean"][0].view(-1)[const]) == 3.25
        # the time axis: a constant column and a NaN in another, in sequence 1 only
        x = instnorm_input(2, 150, 70, 1, seed=9)
        x[1, :, 5] = 1.5
        x[1, 17, 9] = float("nan")
        rf = ref_instnorm(x, torch.randn(2, 150, 70, generator=gen(10)), -2, mode, unbiased)["y"][0]
        assert torch.isnan(rf).all(1).nonzero().tolist() == [[1, 5], [1, 9]] and int(torch.isnan(rf).sum()) == 300
    lengths = segment_lengths(40, long=(150,))
    h = torch.randn(sum(lengths), 10, generator=gen(11))
    b = np.concatenate([[0], np.cumsum(lengths)])
    h[b[5], 1], h[b[7], 2], h[b[8], 3] = float("nan"), float("inf"), float("-inf")
    h[b[0], 4], h[b[17], 5], h[b[17], 6] = SUB, -TINY_N, -0.0                      # sequences of one row: exact
    for relu in (False, True):
        ref, tol = ref_segment_mean(h, lengths, relu)
        assert torch.isnan(ref).nonzero().tolist() == [[5, 1]]
        assert torch.isinf(ref).nonzero().tolist() == ([[7, 2]] if relu else [[7, 2], [8, 3]])
        assert float(ref[0, 4]) == SUB and float(ref[17, 5]) == (0.0 if relu else -TINY_N)
        dh, _ = ref_segment_mean_bwd(torch.ones(len(lengths), 10), h, lengths, relu)
        assert bool(torch.isfinite(dh).all()) and float(dh[b[5], 1]) == 1 / lengths[5]
        assert float(dh[b[8], 3]) == (0.0 if relu else 1 / lengths[8])


def test_the_bound_functions_restate_the_stage_tests():
    """d and c at the shapes whose values tests/test_gpu_auxnet.py writes out."""
    assert d_aux_depth(2, 300) == 2 * 16 + 3 + 4 and d_aux_depth(1, 5) == 2 + 3 + 0 and d_aux_depth(8, 1878) == 128 + 3 + 29
    assert instnorm_c(512) == 4 * 13 and ROW_SWEEP == 16384 and ITEM_SWEEP == 1048576
    lens = torch.tensor([1.0, 16.0, 17.0, 300.0])
    assert ((lens / 16).ceil() + 7).tolist() == [8, 8, 9, 26]          # ceil(len / 16) + 5, + 2
