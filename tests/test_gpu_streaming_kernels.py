"""The streaming kernels (elementwise.hip, maskhead.hip, feat.hip, optim.hip) past their grid caps, against float64
restatements of the same operations computed on the device.

Every one of these kernels caps its grid and then grid-strides; some carry state from one sweep to the next
(maskhead.hip Pos::advance), merge partial results through slots (feat.hip's 64 dB-maximum slots, the colsum slabs,
the Adam partial sums) or switch between a 16-byte and a scalar path.  The cases below run at least 2.5 sweeps of each
kernel, at the training shapes (cfg3: B = 768, K = 4, T = 253, F = 513; cfg5: 1 x 8 x 1878 x 513), and take both
branches of every path switch.  Per-sweep counts (items per sweep of the capped grid):

    grid_for (elementwise.hip)        4096 blocks x 256 = 1 048 576 items; 16 384 rows for cond_mul_fwd and
                                      logit_map_bwd_tf (one wave per row / run)
    stream_grid (maskhead.hip)        2048 blocks: forward 2 097 152 elements, backward 4 194 304, mask_mul 524 288
    sumsq_partial / adam_step         524 288 elements

Tolerances follow from fp32 rounding (U = 2^-24): element-wise results a few U of the result; sums c * U * sum|terms|
with c the longest chain of roundings in the kernel's summation order.  Reductions whose inputs are multiples of 1/16
small enough that every partial sum is an fp32 number are compared exactly: any order of summation is exact there."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import features as ofeat, loss as oloss  # noqa: E402

U = 2.0 ** -24
GIB = 1 << 30
DEV = "cuda"

FWD_SWEEP, BWD_SWEEP, MUL_SWEEP = 2048 * 4 * 256, 2048 * 4 * 512, 2048 * 256      # maskhead.hip stream_grid
GRID_SWEEP, ROW_SWEEP = 4096 * 256, 4096 * 4                                       # elementwise.hip grid_for
ADAM_SWEEP = 512 * 1024                                                            # optim.hip (both kernels)


def H():
    from tssep_amd import hip_ops
    return hip_ops


def L():
    from tssep_amd import _lib
    return _lib.lib()


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def randn(*shape, g, dtype=torch.float32):
    return torch.randn(*shape, device=DEV, dtype=dtype, generator=g)


def rand(*shape, g):
    return torch.rand(*shape, device=DEV, generator=g)


def grid16(*shape, g):
    """Multiples of 1/16 in [-1/2, 1/2]: sums of up to 2^20 of them are exact in fp32 in any order."""
    return torch.randint(-8, 9, shape, device=DEV, generator=g).float() / 16


def within(got, ref, tol, name):
    """|got - ref| <= tol element-wise; ref and tol float64 (or scalars).  NaN or Inf in `got` fails."""
    if got.is_complex():
        got = torch.view_as_real(got)
    if isinstance(ref, torch.Tensor) and ref.is_complex():
        ref = torch.view_as_real(ref)
    err = (got.double() - ref).abs()
    ok = err <= tol
    if not bool(ok.all()):
        bad = ~ok
        i = int(bad.reshape(-1).nonzero()[0])
        idx = np.unravel_index(i, err.shape)
        r = torch.broadcast_to(torch.as_tensor(ref, device=err.device), err.shape)[idx]
        t = torch.broadcast_to(torch.as_tensor(tol, device=err.device), err.shape)[idx]
        raise AssertionError(f"{name}: {int(bad.sum())}/{bad.numel()} elements outside the tolerance; first at {idx}: "
                             f"got {float(got[idx]):.9g}, want {float(r):.9g}, tol {float(t):.3g}")


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
    """Each per-sweep count is exceeded at least 2.5 times by a case of this file (the case lists are below)."""
    sizes = [B * K * T * F for B, K, T, F in MH_SHAPES]
    assert max(sizes) >= 2.5 * max(FWD_SWEEP, BWD_SWEEP, MUL_SWEEP)
    assert any(n % 2 and n >= 2.5 * BWD_SWEEP for n in sizes)                                 # odd: the scalar tail
    assert any(K * T * F > BWD_SWEEP for B, K, T, F in MH_SHAPES)
    assert any(K * T * F < MUL_SWEEP and B * K * T * F > 2.5 * BWD_SWEEP for B, K, T, F in MH_SHAPES)
    for K, trials in COND_KT:
        assert _cond_B(K, trials, 253) * trials * K * 253 >= 2.5 * ROW_SWEEP                  # cond_mul_fwd, logit_map
    assert 33 * 4 * 253 * 320 >= 2.5 * 4 * GRID_SWEEP                                         # tanh_bwd, float4 items
    assert 2700000 >= 2.5 * GRID_SWEEP                                                        # reduce_splits
    assert 9000 * 321 >= 2.5 * GRID_SWEEP                                                     # reduce_splits_bias
    assert 1310723 >= 2.5 * ADAM_SWEEP and 1310723 % 4 == 3                                    # sumsq_partial, adam_step


def test_workspace_queries():
    """The size queries the wrappers allocate workspaces by."""
    lib = L()
    assert lib.tssep_colsum_workspace_bytes(777216, 300) == 128 * 300 * 4                  # colsum_workspace_bytes
    for n in (1, 4095, 4096, 4097, 480000):
        assert lib.tssep_logmae_chunks(n) == -(-n // 4096)                                # logmae_chunks
        assert lib.tssep_logmae_workspace_bytes(3, 5, n) == 15 * -(-n // 4096) * 4        # logmae_workspace_bytes
    assert lib.tssep_vadbce_workspace_bytes(2, 8, 1878) == 2 * 8 * 1878 * 4                # vadbce_workspace_bytes
    assert lib.tssep_adam_workspace_bytes() == 512 * 4                                     # adam_workspace_bytes
    small = lib.tssep_feat_workspace_bytes(8, 253, 40, 513, 0)                             # feat_workspace_bytes
    assert small >= 8 * 253 * 40 * 4 + 40 * 1032 * 4
    assert lib.tssep_feat_workspace_bytes(8, 253, 40, 513, 1) >= small + (8 * 513 - 8) * 4   # per-(utterance, bin) maxima
    assert lib.tssep_feat_workspace_bytes(8, 253, 40, 513, 3) == 0


# ------------------------------------------------------------------------------------------------------------ mask head
MH_SHAPES = [
    (1, 8, 1878, 513),     # cfg5 chunk; K*T*F = 7.7 M > the forward's and the backward's stride
    (16, 4, 253, 513),     # cfg3 slice
    (64, 1, 253, 513),     # K = 1: every utterance boundary is a speaker boundary
    (33, 3, 253, 513),     # odd total 12 854 241 > 2.5 backward sweeps; K*T*F = 389 367: a step wraps 5-10 utterances
    (2, 8, 1878, 513),     # K*T*F = 7.7 M > stride, total 15.4 M > 2.5 backward sweeps
    (3, 5, 17, 9),         # tiny, odd
]


@pytest.mark.parametrize("B,K,T,F", MH_SHAPES)
def test_maskhead_and_mask_mul(B, K, T, F):
    """maskhead_fwd / maskhead_bwd (with and without dmask), mask_mul_fwd / mask_mul_bwd: the observation bin of every
    flat element is b*T*F + (e mod T*F), carried across sweeps by Pos::advance."""
    g = gen(11)
    logit = randn(B, K, T, F, g=g) * 4
    obs = randn(B, T, F, g=g, dtype=torch.complex64)
    dest = randn(B, K, T, F, g=g, dtype=torch.complex64)
    dmask = randn(B, K, T, F, g=g)
    h = H()
    x64 = torch.view_as_real(obs).double()[:, None]                  # [B, 1, T, F, 2]
    xa = logit.double()

    mask, est = h.maskhead_fwd(logit, obs)
    m_ref = torch.sigmoid(xa)
    # hardware exp2 / rcp sigmoid: the rounded exp2 argument costs |x| U relative in exp, (1 - m) of that in m
    within(mask, m_ref, U * m_ref * (6 + 2 * (xa.abs() + 1)), "maskhead_fwd mask")
    m64 = mask.double()
    e_ref = x64 * m64[..., None]                                     # one rounded product per component
    within(est, e_ref, U * e_ref.abs(), "maskhead_fwd est (observation bin)")
    del e_ref, m_ref

    d64 = torch.view_as_real(dest).double()
    terms = (x64 * d64).abs().sum(-1)
    dot = (x64 * d64).sum(-1)
    mm = m64 * (1 - m64)
    for dm in (None, dmask):
        got = h.maskhead_bwd(dest, dm, mask, obs)
        s = dot if dm is None else dot + dm.double()
        st = terms if dm is None else terms + dm.double().abs()
        within(got, s * mm, 8 * U * st * mm, f"maskhead_bwd dmask={dm is not None}")
        del got

    pm = rand(B, K, T, F, g=g)
    est2 = h.mask_mul_fwd(pm, obs)
    e_ref = x64 * pm.double()[..., None]
    within(est2, e_ref, U * e_ref.abs(), "mask_mul_fwd")
    del est2, e_ref
    within(h.mask_mul_bwd(dest, obs), dot, 3 * U * terms, "mask_mul_bwd")


# --------------------------------------------------------------------------------------------------------- conditioning
def _cond_B(K, trials, T, rows=int(2.5 * ROW_SWEEP)):
    return -(-rows // (trials * K * T))


def _pre_buffer(B, T, F, layout, g):
    """pre [B*T, ld] (zero pad columns) in the layout under test: 'vec' 16-byte rows, 'odd' odd leading dimension,
    'offset' a view one float past a 16-byte boundary.  -> (pre view, ld, pre64 [B, T, F])"""
    ld = F + 2 if layout == "odd" and (F + 2) % 2 else (F + 3 if layout == "odd" else (F + 3) // 4 * 4)
    flat = torch.zeros(B * T * ld + 1, device=DEV)
    base = flat[1:] if layout == "offset" else flat[:-1]
    pre = base.view(B * T, ld)
    pre[:, :F] = randn(B * T, F, g=g)
    return pre, ld, pre[:, :F].double().view(B, T, F)


def _grad_buffer(rows, W, ld, layout, g):
    flat = torch.zeros(rows * ld + 1, device=DEV)
    d = (flat[1:] if layout == "offset" else flat[:-1]).view(rows, ld)
    d[:, :W] = randn(rows, W, g=g)
    return d


def _poison(*sizes):
    """NaN-filled blocks handed back to the caching allocator: outputs the wrappers leave to a kernel are allocated from
    them, so a pad column the kernel should have written stays NaN."""
    p = [torch.full((n,), float("nan"), device=DEV) for n in sizes]
    del p


def _check_cond(B, K, T, F, E, trials, comb, layout, seed, bchunk=64):
    g = gen(seed)
    h = H()
    pre, ld_pre, pre64 = _pre_buffer(B, T, F, layout, g)
    aux = rand(B, K, E, g=g)
    rows = B * trials * K * T
    W = F if comb == "mul" else F + E
    ldx = (W + 3) // 4 * 4
    _poison(rows * ldx, B * T * ((F + 3) // 4 * 4))
    xs, ld, info = h.cond_fwd(pre, ld_pre, aux, B, K, T, F, trials, comb)
    assert ld == ldx
    fwd = "cond_mul_fwd" if comb == "mul" else "cond_cat_fwd"
    bwd = "cond_mul_bwd" if comb == "mul" else "cond_cat_bwd"
    tag = f"{comb} K={K} trials={trials} F={F} {layout}"
    assert bool((xs[:, W:] == 0).all()), f"{fwd} {tag}: pad columns not zero"
    idx = ((torch.arange(K)[None, :] + torch.arange(trials)[:, None]) % K).to(DEV)      # trial tr: speaker (k + tr) % K
    a64 = aux.double()
    xs4 = xs.view(B, trials, K, T, ld)
    for b0 in range(0, B, bchunk):
        b1 = min(B, b0 + bchunk)
        p = pre64[b0:b1, None, None]                                   # [b, 1, 1, T, F]
        a = a64[b0:b1][:, idx][:, :, :, None]                          # [b, trials, K, 1, E]
        if comb == "mul":
            ref = p * a
            within(xs4[b0:b1, ..., :W], ref, U * ref.abs(), f"{fwd} {tag}")
        else:
            ref = torch.cat([p.expand(-1, trials, K, T, F), a.expand(-1, -1, -1, T, E)], -1)
            within(xs4[b0:b1, ..., :W], ref, 0.0, f"{fwd} {tag}")
    del xs, xs4

    dl = ldx + 1 if layout == "odd" else ldx
    dxs = _grad_buffer(rows, W, dl, layout, g)
    _poison(B * T * ((F + 3) // 4 * 4))
    dpre, ldp = h.cond_bwd(dxs, dl, info, B, K, T, F, trials, comb)
    assert bool((dpre[:, F:] == 0).all()), f"{bwd} {tag}: pad columns not zero"
    d5 = dxs.view(B, trials, K, T, dl)
    dp = dpre.view(B, T, ldp)
    for b0 in range(0, B, bchunk):
        b1 = min(B, b0 + bchunk)
        d = d5[b0:b1, ..., :F].double()
        if comb == "mul":
            prod = d * a64[b0:b1][:, idx][:, :, :, None, :F]
        else:
            prod = d
        ref = prod.sum((1, 2))
        within(dp[b0:b1, :, :F], ref, (trials * K + 1) * U * prod.abs().sum((1, 2)), f"{bwd} {tag}")


COND_KT = [(1, 1), (4, 1), (4, 2), (4, 4), (8, 1), (8, 2), (8, 8)]


@pytest.mark.parametrize("comb", ["mul", "cat"])
@pytest.mark.parametrize("K,trials", COND_KT)
def test_conditioning(comb, K, trials):
    """cond_mul_fwd / cond_mul_bwd / cond_cat_fwd / cond_cat_bwd at F = 513 over >= 2.5 x 16 384 rows (E = 600 > F for
    'cat'), 16-byte layouts: the pad columns the 16-byte kernels write must come out zero."""
    T = 253
    _check_cond(_cond_B(K, trials, T), K, T, 513, 513 if comb == "mul" else 600, trials, comb, "vec", 100 + 10 * K + trials)


@pytest.mark.parametrize("comb,layout,F", [("mul", "odd", 513), ("mul", "offset", 513), ("mul", "vec", 1100),
                                           ("cat", "odd", 513), ("cat", "offset", 513)])
def test_conditioning_scalar_paths(comb, layout, F):
    """The scalar branches: odd leading dimensions, a view one float off 16 bytes, F > 1024 (cond_mul_fwd)."""
    K, trials, T = 4, 2, 253
    _check_cond(_cond_B(K, trials, T), K, T, F, F if comb == "mul" else 600, trials, comb, layout, 7)


def test_conditioning_at_cfg3():
    """cfg3 batch 768, 'mul', one trial: 777 216 rows (47 sweeps of cond_mul_fwd)."""
    _check_cond(768, 4, 253, 513, 513, 1, "mul", "vec", 5)


# --------------------------------------------------------------------------------------------------------- tanh backward
@pytest.mark.parametrize("B,P,combined,offset", [
    (33, 320, False, False), (33, 320, True, False),        # 16-byte path, 10.7 M elements = 2.5 sweeps of float4
    (33, 300, False, False), (33, 300, True, False),
    (33, 321, False, False), (33, 321, True, False),        # scalar path (P % 4), 10.1 sweeps
    (33, 320, True, True),                                  # scalar path (a view one float off 16 bytes)
    (768, 320, True, False),                                # cfg3: 248.7 M elements
])
def test_tanh_bwd(B, P, combined, offset):
    K, T = 4, 253
    rows = B * K * T
    g = gen(21 + P)
    n = rows * P
    shape = (B, T, K, P) if combined else (B, K, T, P)
    fy, fd = torch.empty(n + 1, device=DEV), torch.empty(n + 1, device=DEV)
    y = (fy[1:] if offset else fy[:n]).view(shape)
    dy = (fd[1:] if offset else fd[:n]).view(shape)
    y.copy_(torch.tanh(randn(*shape, g=g) * 2))
    dy.copy_(randn(*shape, g=g))
    dz = H().tanh_bwd(dy, y, rows, P, K, T, combined).view(B, K, T, P)
    for b0 in range(0, B, 96):
        b1 = min(B, b0 + 96)
        yy, dd = y[b0:b1].double(), dy[b0:b1].double()
        if combined:
            yy, dd = yy.transpose(1, 2), dd.transpose(1, 2)
        y2 = yy * yy
        within(dz[b0:b1], dd * (1 - y2), 3 * U * dd.abs() * (y2 + (1 - y2).abs()), f"tanh_bwd P={P} combined={combined}")


# ------------------------------------------------------------------------------------------------------------ reductions
@pytest.mark.parametrize("M,N,lda,accumulate", [
    (777216, 300, 304, False),    # cfg3 rows, N % 64 != 0
    (777216, 64, 64, True),
    (1, 300, 300, False),         # fewer rows than the 128 slabs
    (127, 130, 131, True),
    (129, 513, 516, False),
    (50000, 1, 3, True),
])
def test_colsum(M, N, lda, accumulate):
    """colsum_f32 (two-pass: 128 slabs, then reduce_splits) on multiples of 1/16: exact in any summation order."""
    g = gen(31)
    A = grid16(M, lda, g=g)
    if lda > N:
        A[:, N:] = float("nan")                                     # columns past N must not be read
    init = grid16(N, g=g) * 64
    out = init.clone()
    H().colsum(A, lda, M, N, out=out, accumulate=accumulate)
    ref = A[:, :N].double().sum(0) + (init.double() if accumulate else 0)
    within(out, ref, 0.0, f"colsum_f32 M={M} N={N}")


def test_colsum_rounding():
    """colsum_f32 on normal data: c U sum|a| with c the longest addition chain: M / 128 rows per slab over 4 row
    lanes x 4 partial sums, their combination, then the 128 slabs added in sequence."""
    g = gen(32)
    M, N = 777216, 77
    A = randn(M, N, g=g)
    out = H().colsum(A, N, M, N)
    c = M / (128 * 16) + 8 + 128 + 4
    within(out, A.double().sum(0), c * U * A.double().abs().sum(0), "colsum_f32 (randn)")


@pytest.mark.parametrize("S,count,accumulate", [(1, 2700000, False), (8, 2700000, True), (8, 1000, False)])
def test_reduce_splits(S, count, accumulate):
    g = gen(33)
    part = grid16(S, count, g=g)
    init = grid16(count, g=g)
    dst = init.clone()
    H().reduce_splits(part, S, count, dst, accumulate)
    within(dst, part.double().sum(0) + (init.double() if accumulate else 0), 0.0, "reduce_splits")


@pytest.mark.parametrize("S,M,N,ldp,accumulate", [
    (1, 2400, 320, 324, False), (8, 2400, 320, 328, True),       # ldp > N + 1
    (8, 9000, 320, 321, True),                                   # M (N + 1) = 2.9 M: 2.8 sweeps
    (4, 1200, 513, 520, False), (1, 777, 301, 305, True),
])
def test_reduce_splits_bias(S, M, N, ldp, accumulate):
    """reduce_splits_bias: columns [0, N) of the split partials -> dw [M, N], column N -> db [M], columns past N never
    read; nothing outside dw and db written (guard bands around both)."""
    g = gen(34)
    part = grid16(S, M, ldp, g=g)
    part[:, :, N + 1:] = float("nan")
    G = 64
    wbuf = torch.full((M * N + 2 * G,), 1234.5, device=DEV)
    bbuf = torch.full((M + 2 * G,), -777.25, device=DEV)
    dw, db = wbuf[G:G + M * N].view(M, N), bbuf[G:G + M]
    w0, b0 = grid16(M, N, g=g), grid16(M, g=g) * 4
    dw.copy_(w0)
    db.copy_(b0)
    H().reduce_splits_bias(part, S, M, N, ldp, dw, db, accumulate)
    s = part[:, :, :N + 1].double().sum(0)
    acc = 1.0 if accumulate else 0.0
    within(dw, s[:, :N] + acc * w0.double(), 0.0, f"reduce_splits_bias dw S={S} acc={accumulate}")
    within(db, s[:, N] + acc * b0.double(), 0.0, f"reduce_splits_bias db S={S} acc={accumulate}")
    for buf, v in ((wbuf, 1234.5), (bbuf, -777.25)):
        assert bool((buf[:G] == v).all()) and bool((buf[-G:] == v).all()), "reduce_splits_bias wrote outside dw / db"


# ---------------------------------------------------------------------------------------------------------------- losses
@pytest.mark.parametrize("B,K,N", [(4, 3, 1), (4, 3, 4095), (4, 3, 4096), (4, 3, 4097), (2, 8, 480000),
                                   (768, 4, 64000),                # cfg3: 196.6 M elements
                                   (13107, 5, 7)])                 # B K = 65 535, the largest grid.y
def test_logmae(B, K, N):
    """logmae_fwd (+ logmae_finalize inside it), logmae_bwd for LogMAE and for plain MAE (sums = None); a tenth of the
    elements have est == tgt: their gradient is exactly 0."""
    g = gen(41)
    tgt = randn(B, K, N, g=g)
    est = tgt + 0.5 * randn(B, K, N, g=g)
    eq = rand(B, K, N, g=g) < 0.1
    est = torch.where(eq, tgt, est)
    gout = randn(B, g=g)
    h = H()
    loss, sums = h.logmae_fwd(est, tgt)
    nch = L().tssep_logmae_chunks(N)
    bc = max(1, (1 << 25) // (K * N))
    s_ref = torch.cat([(est[i:i + bc].double() - tgt[i:i + bc].double()).abs().mean(-1).sum(-1) for i in range(0, B, bc)])
    c = 1 + 24 + nch + K + 2           # |e - t|, 16 per lane + butterfly + block, chunks, speakers, / N
    within(sums, s_ref, c * U * s_ref, f"logmae_fwd sums N={N}")
    if B * K * N < 1e8:
        l_ref = oloss.log_mae(est.double(), tgt.double())
        within(loss, l_ref, 2 * U * l_ref.abs() + c * U / math.log(10), f"logmae_fwd loss N={N}")
    else:
        within(loss, torch.log10(s_ref), 2 * U * torch.log10(s_ref).abs() + c * U / math.log(10), f"logmae_fwd loss N={N}")
    s64 = sums.double()
    for mae in (False, True):
        dest = h.logmae_bwd(est, tgt, None if mae else sums, gout)
        coef = gout.double() / (N if mae else N * math.log(10) * s64)
        for b0 in range(0, B, 96):
            b1 = min(B, b0 + 96)
            sgn = torch.sign(est[b0:b1].double() - tgt[b0:b1].double())
            ref = sgn * coef[b0:b1, None, None]
            within(dest[b0:b1], ref, 4 * U * ref.abs(), f"logmae_bwd mae={mae} N={N}")
        assert bool((dest[eq] == 0).all())
        del dest


def test_logmae_grid_limit_and_finalize():
    """B K = 65 536 is rejected with the shape error (grid.y); logmae_finalize on given partial sums."""
    h = H()
    with pytest.raises(RuntimeError, match="invalid shape"):
        h.logmae_fwd(torch.zeros(16384, 4, 3, device=DEV), torch.zeros(16384, 4, 3, device=DEV))
    g = gen(42)
    B, K, N = 6, 8, 480000
    nch = L().tssep_logmae_chunks(N)
    part = rand(B * K, nch, g=g) * 4096
    loss, sums = h.logmae_finalize(part, B, K, N)
    ref = (part.double().sum(-1) / N).view(B, K).sum(-1)
    within(sums, ref, (nch + K + 2) * U * ref, "logmae_finalize sums")
    within(loss, torch.log10(ref), 2 * U * torch.log10(ref).abs() + (nch + K + 2) * U / math.log(10), "logmae_finalize")


@pytest.mark.parametrize("F", [1, 63, 64, 65, 513])
def test_vadbce(F):
    """vadbce_fwd / vadbce_bwd at T = 1878 (cfg5 frames), row means up to +-40: the log1p(exp(-|x|)) branch."""
    B, K, T = 2, 8, 1878
    g = gen(50 + F)
    x_row = (rand(B, K, T, 1, g=g) * 2 - 1) * 40
    logit = x_row + 0.5 * randn(B, K, T, F, g=g)
    vad = (rand(B, K, T, g=g) > 0.5).float()
    gout = randn(B, g=g)
    h = H()
    loss, xmean = h.vadbce_fwd(logit, vad)
    lg = logit.double()
    x_ref = lg.mean(-1)
    err_x = (F / 64 + 8) * U * lg.abs().sum(-1) / F + U * x_ref.abs()
    within(xmean, x_ref, err_x, f"vadbce_fwd xmean F={F}")
    y = vad.double()
    lrow = x_ref.clamp(min=0) - x_ref * y + torch.log1p(torch.exp(-x_ref.abs()))
    err_l = err_x + 4 * U * (x_ref.clamp(min=0) + (x_ref * y).abs() + torch.log1p(torch.exp(-x_ref.abs())))
    KT = K * T
    l_ref = oloss.vad_sigmoid_bce(lg, y)
    within(loss, l_ref, err_l.mean((1, 2)) + (KT / 256 + 10) * U * lrow.mean((1, 2)), f"vadbce_fwd loss F={F}")
    dl = h.vadbce_bwd(xmean, vad, gout, F)
    s = torch.sigmoid(xmean.double())
    k = (gout.double() / (KT * F))[:, None, None]
    ref = (k * (s - y))[..., None].expand(B, K, T, F)
    tol = (k.abs() * (4 * U * s + U * (s - y).abs()) + 3 * U * (k * (s - y)).abs())[..., None]
    within(dl, ref, tol, f"vadbce_bwd F={F}")


# ------------------------------------------------------------------------------------------------------------ logit map
def _map_restated(raw, iperm, B, trials, K, T, F, Fr, spk_rows):
    """The float64 restatement: raw GEMM layout -> [B, K, T, F]: trial tr holds speaker (k + tr) % K at position k,
    mean over the trials, speaker s to output row perm[b, s]."""
    if spk_rows:
        pos = raw.view(B, 1, K, T, Fr)
    else:
        pos = raw.view(B, trials, T, K, Fr).permute(0, 1, 3, 2, 4)             # [B, tr, K(pos), T, Fr]
    tr = torch.arange(trials, device=raw.device)[:, None]
    kpos = (torch.arange(K, device=raw.device)[None, :] - tr) % K             # [tr, s]
    spk = pos[:, tr, kpos].mean(1)                                            # [B, K(s), T, Fr]
    out = spk if iperm is None else torch.take_along_dim(spk, iperm.long()[:, :, None, None], 1)
    return out.expand(B, K, T, F)


@pytest.mark.parametrize("K,trials,Fr,spk_rows,perm", [
    (4, 1, 513, 0, True), (4, 2, 513, 0, True), (4, 4, 513, 0, True), (4, 1, 1, 0, True), (4, 2, 1, 0, True),
    (4, 4, 1, 0, True), (8, 1, 513, 0, True), (8, 2, 513, 0, True), (8, 8, 513, 0, True), (8, 1, 1, 0, True),
    (8, 2, 1, 0, True), (8, 8, 1, 0, True), (4, 1, 513, 1, True), (4, 1, 1, 1, True), (8, 1, 513, 1, True),
    (8, 1, 1, 1, True), (4, 2, 513, 0, False),
])
def test_logit_map(K, trials, Fr, spk_rows, perm):
    """logit_map_fwd / logit_map_bwd at F = 513 over >= 2.5 x 16 384 runs of F (logit_map_bwd_tf's per-sweep rows);
    the backward against autograd of the float64 restatement."""
    T, F = 253, 513
    B = -(-int(2.5 * ROW_SWEEP) // (trials * K * T))
    g = gen(60 + K + trials)
    raw = randn(B * trials * K * T * Fr, g=g)
    if perm:
        pm = torch.stack([torch.randperm(K, device=DEV, generator=g) for _ in range(B)]).int()
        ipm = torch.argsort(pm, -1).int()
    else:
        pm = ipm = None
    h = H()
    out = h.logit_map_fwd(raw, pm, ipm, B, trials, K, T, F, Fr, spk_rows)
    r64 = raw.double().requires_grad_()
    ref = _map_restated(r64, ipm, B, trials, K, T, F, Fr, spk_rows)
    tag = f"K={K} trials={trials} Fr={Fr} spk_rows={spk_rows}"
    if trials == 1:
        within(out, ref, 0.0, f"logit_map_fwd {tag}")
    else:
        mag = _map_restated(raw.double().abs(), ipm, B, trials, K, T, F, Fr, spk_rows)
        within(out, ref, (trials - 1) * U * mag, f"logit_map_fwd {tag}")
    del out
    dout = randn(B, K, T, F, g=g)
    draw = h.logit_map_bwd(dout, pm, ipm, B, trials, K, T, F, Fr, spk_rows)
    (gref,) = torch.autograd.grad(ref, r64, dout.double(), retain_graph=True)
    if Fr == F or F == 1:                       # a gather scaled by 1 / trials (a power of two): exact
        within(draw, gref, 0.0, f"logit_map_bwd {tag}")
    else:                                       # the sum over F of a run (logit_map_bwd_t)
        (gmag,) = torch.autograd.grad(ref, r64, dout.double().abs())
        within(draw, gref, (F / 64 + 8) * U * gmag, f"logit_map_bwd {tag}")


def test_logit_map_at_cfg3():
    """cfg3 batch 768 (num_averaged_permutations = 1): a permutation of 398.7 M elements both ways, exact."""
    B, K, T, F = 768, 4, 253, 513
    g = gen(69)
    raw = randn(B * T * K * F, g=g)
    pm = torch.stack([torch.randperm(K, device=DEV, generator=g) for _ in range(B)]).int()
    ipm = torch.argsort(pm, -1).int()
    h = H()
    out = h.logit_map_fwd(raw, pm, ipm, B, 1, K, T, F, F, 0)
    r4 = raw.view(B, T, K, F)
    for b0 in range(0, B, 128):
        b1 = min(B, b0 + 128)
        ref = _map_restated(r4[b0:b1], ipm[b0:b1], b1 - b0, 1, K, T, F, F, 0)
        assert torch.equal(out[b0:b1], ref), f"logit_map_fwd cfg3 utterances {b0}:{b1}"
    del out
    dout = randn(B, K, T, F, g=g)
    draw = h.logit_map_bwd(dout, pm, ipm, B, 1, K, T, F, F, 0).view(B, T, K, F)
    for b0 in range(0, B, 128):
        b1 = min(B, b0 + 128)
        # raw (b, t, k) holds speaker k, which went to output row perm[b, k]
        ref = torch.take_along_dim(dout[b0:b1], pm[b0:b1].long()[:, :, None, None], 1).transpose(1, 2)
        assert torch.equal(draw[b0:b1], ref), f"logit_map_bwd cfg3 utterances {b0}:{b1}"


# -------------------------------------------------------------------------------------------------------------- features
@pytest.mark.parametrize("B,T,F,n_mels,n_mfcc,axis", [
    (5, 205, 513, 40, 40, "tf"),        # 1 025 frames: 65 pass-1 blocks, the last one shares slot 0
    (767, 253, 513, 40, 40, "tf"),      # 194 051 frames (cfg3 batch 767): the last block writes slot 32
    (8, 253, 513, 40, 40, "t"),
    (8, 253, 513, 40, 40, "f"),
    (8, 253, 513, 80, 80, "tf"),        # n_mels > 64: the m0 loops of both passes
    (8, 253, 513, 160, 80, "tf"),       # n_mels > 128: pass 1 without the packed LDS filterbank
    (8, 253, 201, 160, 160, "tf"),      # 160 mels over 201 bins: low filters without a nonzero weight
    (8, 253, 201, 40, 40, "tf"),
    (8, 253, 257, 40, 40, "tf"),
    (8, 253, 1025, 40, 40, "tf"),
])
def test_feat_fwd(B, T, F, n_mels, n_mfcc, axis):
    """feat_fwd (MFCC with the batch-wide top_db floor + Log1pMaxNormAbsSTFT) against the oracle in float64.  The
    frames span 60 dB; the batch dB maximum sits in the LAST frame, so it reaches pass 2 only through the last block's
    slot of the 64-slot merge."""
    g = gen(70 + F + n_mels)
    X = randn(B, T, F, g=g, dtype=torch.complex64) * (10 ** (-3 * rand(B, T, 1, g=g)))
    X[-1, -1] = randn(F, g=g, dtype=torch.complex64) * 10
    fb, dct = ofeat.mfcc_tables(size=2 * (F - 1), n_mels=n_mels, n_mfcc=n_mfcc)
    out, _ = H().feat_fwd(X, fb.to(DEV), dct.to(DEV), n_mfcc, top_db=80.0, statistics_axis=axis)
    fb64, dct64 = fb.double().to(DEV), dct.double().to(DEV)
    # width of every filter's [lo, hi) support: pass 1 sums over it
    nz = fb64 != 0
    ar = torch.arange(F, device=DEV, dtype=torch.float64)[:, None]
    width = torch.where(nz.any(0), (ar * nz).amax(0) - torch.where(nz, ar, float(F)).amin(0) + 1, 0.0)
    mels, dbs = [], []
    for b0 in range(0, B, 64):
        x = X[b0:b0 + 64].to(torch.complex128)
        mels.append((x.abs() ** 2) @ fb64)                                        # [b, T, n_mels]
    mel = torch.cat(mels)
    del mels
    db_ref = ofeat.amplitude_to_db_power(mel.transpose(1, 2), 80.0).transpose(1, 2)      # 3-D: batch-wide floor
    raw_db = 10 * torch.log10(mel.clamp(min=1e-10))
    assert int(raw_db.reshape(-1, n_mels).amax(1).argmax()) == B * T - 1              # the planted maximum
    err_db = 10 / math.log(10) * (width / 4 + 8) * U + 4 * U * raw_db.abs()
    err_db = torch.maximum(err_db, err_db.max())                                       # the floor carries the max's error
    mf_ref = db_ref @ dct64
    tol = err_db @ dct64.abs() + (n_mels + 2) * U * (db_ref.abs() @ dct64.abs())
    within(out[..., :n_mfcc], mf_ref, tol, f"feat_fwd mfcc n_mels={n_mels} F={F}")
    empty = (~nz.any(0)).nonzero().flatten()
    if n_mfcc == n_mels:
        # orthonormal square DCT: the dB bands themselves; filters without a weight clamp to 1e-10 and take the floor
        assert len(empty) > 0
        floor = float(raw_db.max()) - 80.0
        assert bool((db_ref[..., empty] == floor).all())
        # (the fp32 DCT table is orthogonal to ~1e-7: both sides go through the same inverse)
        db_got = out[..., :n_mfcc].double() @ dct64.t()
        within(db_got[..., empty], (mf_ref @ dct64.t())[..., empty], (tol @ dct64.abs().t())[..., empty],
               f"feat_fwd floor of the empty filters {empty.tolist()}")
    del mel, db_ref, raw_db, mf_ref, tol
    for b0 in range(0, B, 64):
        x = X[b0:b0 + 64].to(torch.complex128)
        ref = ofeat.log1p_max_norm_abs(x, axis)
        a = torch.expm1(ref)
        within(out[b0:b0 + 64, :, n_mfcc:], ref, 8 * U * a / (1 + a) + 2 * U * ref,
               f"feat_fwd log1p-max-norm axis={axis} F={F}")


# ------------------------------------------------------------------------------------------------------------- optimizer
LR, BETAS, EPS, MAX_NORM = 1e-3, (0.9, 0.999), 1e-8, 10.0
GRAD_SCALES = [1e-2, 1e-3, 3e-2, 1e-3, 1e-2]     # norms ~ scale * sqrt(n): the steps alternate clipped / not clipped


def f32(x):
    return float(np.float32(x))


def _adam_reference(p0, m0, v0, g, step, wd, norm_got):
    """clip_grad_norm_ + torch.optim.Adam in float64 from the kernel's state before the step, with the fp32 values of
    the hyper-parameters the kernel receives -> (norm, p, m, v, and their tolerances)."""
    lr, b1, b2, eps, wd, mx = f32(LR), f32(BETAS[0]), f32(BETAS[1]), f32(EPS), f32(wd), f32(MAX_NORM)
    p = torch.nn.Parameter(p0.clone())
    p.grad = g.clone()
    norm = float(torch.nn.utils.clip_grad_norm_([p], mx))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[p] = dict(step=torch.tensor(float(step - 1), dtype=torch.float64), exp_avg=m0.clone(),
                        exp_avg_sq=v0.clone())
    opt.step()
    st = opt.state[p]
    # forward error of the kernel's fp32 arithmetic (optim.hip adam_step_kernel), term by term
    clip = min(1.0, mx / (norm + 1e-6))
    e_clip = (abs(norm_got - norm) / norm + 3 * U) if clip < 1 else 0.0
    g1 = g * clip
    e_g = g1.abs() * (e_clip + U)
    g2 = g1 + wd * p0
    if wd:
        e_g = e_g + 2 * U * ((wd * p0).abs() + g2.abs())
    e_m = (1 - b1) * e_g + 3 * U * (b1 * m0.abs() + (1 - b1) * g2.abs())
    v = st["exp_avg_sq"]
    e_v = (1 - b2) * 2 * g2.abs() * e_g + 4 * U * (b2 * v0 + (1 - b2) * g2 * g2)
    sv = v.sqrt()
    e_sv = torch.minimum(e_v / (2 * sv), e_v.sqrt()).nan_to_num(0.0) + U * sv
    s = 1 / math.sqrt(1 - b2 ** step)
    den = sv * s + eps
    e_den = s * e_sv + 5 * U * sv * s + U * den
    step_size = lr / (1 - b1 ** step)
    m = st["exp_avg"]
    upd = step_size * m / den
    e_p = step_size * (e_m / den + m.abs() * e_den / den ** 2) + 4 * U * upd.abs() + U * p.detach().abs()
    return norm, p.detach(), m, v, e_p, e_m, e_v


def _run_adam_steps(n, step_fn, state, wd, tail=0, live=None):
    """Five steps through `step_fn(step) -> norm`, each against the float64 reference started from the kernel's state
    before it.  live: 0 where the flat buffers have their zero gaps."""
    P, M, V, G = state
    g = gen(80 + n % 97)
    for it, sc in enumerate(GRAD_SCALES):
        G.copy_(randn(n, g=g) * sc)
        if live is not None:
            G.mul_(live)
        if tail:
            G[n - tail:n] = 2.0 * sc * math.sqrt(n)           # the scalar tail: 12/13 of the squared norm
        before = [t[:n].double() for t in (P, M, V)]
        gg = G[:n].double()
        norm_got = float(step_fn(it + 1))
        norm, p_ref, m_ref, v_ref, e_p, e_m, e_v = _adam_reference(*before, gg, it + 1, wd, norm_got)
        clipped = norm > MAX_NORM
        assert clipped == (it % 2 == 0), (it, norm)
        assert norm_got == pytest.approx(norm, rel=1e-5), f"step {it + 1}: gradient norm"
        within(M[:n], m_ref, e_m, f"adam exp_avg step {it + 1} wd={wd}")
        within(V[:n], v_ref, e_v, f"adam exp_avg_sq step {it + 1} wd={wd}")
        within(P[:n], p_ref, e_p, f"adam param step {it + 1} wd={wd}")


def _cfg3_mask_estimator_shapes():
    from tssep_amd.train import net
    me = net.MaskEstimator_v2(idim=553, odim=513, units=300, projs=320, combination="mul", aux_net_output_size=513,
                              ts_vad=4, output_resolution="tf", random_speaker_order=True, num_averaged_permutations=1)
    return [tuple(p.shape) for p in me.parameters() if p.requires_grad]


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fused_adam_on_the_cfg3_mask_estimator(wd):
    """train.optimizer.Adam (adam_step_guarded: sumsq_partial + adam_step over the flat buffers) on the 42 parameter
    tensors of the cfg3 mask estimator: 10 842 048 flat elements, 20.7 sweeps of both kernels."""
    from tssep_amd.train.optimizer import Adam
    shapes = _cfg3_mask_estimator_shapes()
    g = gen(90)
    params = [torch.nn.Parameter(randn(*s, g=g) * 0.1) for s in shapes]
    opt = Adam(gradient_clipping=MAX_NORM, lr=LR, betas=BETAS, eps=EPS, weight_decay=wd)
    opt.set_parameters(params)
    n = opt.flat_param.numel()
    assert n == 10842048, n
    live = torch.zeros(n, device=DEV)
    for prm, off in zip(params, opt._offsets):
        live[off:off + prm.numel()] = 1

    def step(_):
        return opt.step()
    _run_adam_steps(n, step, (opt.flat_param, opt.exp_avg, opt.exp_avg_sq, opt.bucket.flat), wd, live=live)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_step_odd_size(wd):
    """adam_step directly at n = 1 310 723 = 3 (mod 4), 2.5 sweeps: sumsq_partial's scalar tail holds most of the
    gradient norm."""
    n = 1310723
    g = gen(91)
    P = randn(n, g=g) * 0.1
    M, V = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    G = torch.zeros(n, device=DEV)
    norm = torch.zeros(1, device=DEV)
    ws = torch.empty(L().tssep_adam_workspace_bytes() // 4, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def step(k):
        from tssep_amd import _lib
        _lib.check(L().tssep_adam_step(p(P), p(M), p(V), p(G), n, k, MAX_NORM, LR, BETAS[0], BETAS[1], EPS, wd,
                                       p(norm), p(ws), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "adam_step")
        return norm
    _run_adam_steps(n, step, (P, M, V, G), wd, tail=3)
