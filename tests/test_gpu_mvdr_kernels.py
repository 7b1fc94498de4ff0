"""The MVDR kernels of csrc/mvdr.hip one stage at a time on an MI355X against extended precision: the statistics
(tssep_mvdr_psd), the per-bin solve (tssep_mvdr_weights: mvdr_reduce_kernel, mvdr_solve_kernel<D> in registers for D <= 6,
mvdr_weights_kernel in LDS for D = 7, 8), the filtering (tssep_mvdr_apply), their chain (hip_ops.mvdr_souden) and the
segment-wise pipeline (tssep_mvdr_segments_psd / _fwd), called through tssep_amd._lib.  References, bounds (derived in that
file's docstring, nothing fitted to a kernel's output) and input generators: tests/test_mvdr_reference.py.

1. Solve alone, on crafted partials.  The kernel's own Phi is recovered exactly: with eps = 2^k above every trace the
   stored weights are conj(Phi[:, ref]) 2^-k without a rounding, one call per ref.  |X - A Phi^| <= GAMMA(D) |L| |U| |Phi^|
   for D = 1..8 on graded, rank1, indefinite, ties and graded x 2^+-400; F in {1, 63, 64, 65, 130}, K in {1, 3, 5}, B in
   {1, 3}; more than one chunk: the sums of mvdr_reduce_kernel are read back bit for bit.  With the default eps, and with
   eps = 1e-2 and traces on both sides of it and below zero, the weights are conj(Phi^[:, ref]) / max(tr, eps) of the
   kernel's own Phi^ within the two roundings of 1 / lam and the product.  info: the exact count on exactsing, zero
   elsewhere, written over a sentinel.  A NaN or an Inf in one bin leaves every other bin bit-identical; 2^+-400 on A and X
   gives bit-identical weights; a 6 x 6 system as the leading block of an 8 x 8 one with an identity tail (LDS kernel) has
   the leading Phi of the register kernel within the bounds.
2. Statistics alone: every chunk partial against the extended sum over that chunk's own frames, NaN guard bands around
   the buffer, every element in between written.
3. Apply alone on crafted weights: the dot-product bound, the clamp of the mask, guard bands around enh.
4. The chain: the stages run by hand and hip_ops.mvdr_souden give the same bits; every stage within its bound.
5. Segments: statistics against the extended _get_psd; the whole pipeline on graded data with adjacent and overlapping
   rows (ClassicBF_np assigns out[k, s:e] row after row: the later row wins, and so does seg_map_kernel), the singular
   segment named exactly, rows that load_seg empties changing nothing.
   FOUND HERE: a row that load_seg empties had its zero statistics solved like any other, so its info slot counted F
   singular bins and hip_ops.segment_mvdr raised LinAlgError naming a row the header calls ignored.  seg_info_kernel
   (mvdr.hip) now puts that slot back to zero; test_segments_emptied_rows_change_nothing holds it.
   Nothing else was exposed: both exchange paths, the scaled case and overlapping rows were right.

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report):
                             D=1      D=2      D=3      D=4      D=5      D=6      D=7      D=8
    solve                    0.093    0.13     0.08     0.082    0.076    0.074    0.085    0.075
    solve, forward           0.098    0.13     0.046    0.062    0.035    0.023    0.014    0.013
    weights from Phi         0.92     1        1        1        1        1        1        1       (0.996 .. 0.9995: two roundings)
    statistics               0.35     0.38     0.54     0.55     0.49     0.46     0.56     0.43
    apply                    0.73     0.59     0.56     0.6      0.54     0.44     0.59     0.49
    chain: statistics        -        -        -        -        -        0.26     -        0.3
    chain: solve             -        -        -        -        -        0.045    -        0.029
    chain: solve, forward    -        -        -        -        -        0.011    -        0.0068
    segment statistics       -        0.28     0.052    -        -        0.19     0.22     0.2
    segments: solve          -        -        -        -        -        0.029    -        0.029
    segments: apply          -        -        -        -        -        0.25     -        0.13
The chain ran at cond(A) 8.6e10 .. 2.6e13 (graded) and 1.2e4 .. 2.3e13 (rank1), mvdr_souden bit-identical to the stages.
"""
import math

import numpy as np
import pytest
import torch

from tssep_amd import _lib, hip_ops as Hop
import test_mvdr_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
G = 64                      # guard band, in doubles
TINY = float(np.finfo(np.float64).tiny)
WORST = {}                  # (stage, D) -> largest error / bound of this run


def record(stage, D, ratio):
    ratio = float(np.max(ratio)) if np.size(ratio) else 0.0
    WORST[(stage, D)] = max(WORST.get((stage, D), 0.0), ratio)
    return ratio


def L():
    return _lib.lib()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def guarded(n):
    """n doubles between two NaN bands -> (whole buffer, the view in between)"""
    buf = torch.full((n + 2 * G,), NAN, dtype=torch.float64, device=DEV)
    return buf, buf[G:G + n]


def bands_intact(buf):
    return bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[-G:]).all())


def ratio_of(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / bound
    return np.nan_to_num(np.where((err == 0) & (bound == 0), 0.0, r), nan=np.inf)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- stage 1: the solve ------------------------------------------------------------------------------------------------
def partials_of(A, X, B, K, F):
    """A, X [B*K*F, D, D] -> one chunk of partials [B, 1, K, 2, D*D, F]"""
    D = A.shape[-1]
    part = np.empty((B, 1, K, 2, D * D, F))
    part[:, 0, :, 0] = R.pack_hermitian(X.reshape(B, K, F, D, D))
    part[:, 0, :, 1] = R.pack_hermitian(A.reshape(B, K, F, D, D))
    return part


def run_weights(part, D, T, ref, eps):
    """-> wconj [B, K, D, F] complex128, info, the partials after the call"""
    B, chunks, K, _, _, F = part.shape
    assert L().tssep_mvdr_partial_bytes(B, K, D, T, F) == part.size * 8
    pd = dev(part)
    buf, w = guarded(B * K * D * F * 2)
    info = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    st = L().tssep_mvdr_weights(pd.data_ptr(), w.data_ptr(), info.data_ptr(), B, K, D, T, F, ref, float(eps), None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(buf)
    wc = w.view(B, K, D, F, 2).cpu().numpy()
    return wc[..., 0] + 1j * wc[..., 1], int(info.item()), pd.cpu().numpy()


def recover_phi(part, D, T, trace_ref, regular=None):
    """the kernel's own Phi [B*K*F, D, D] (exact) and info"""
    B, _, K, _, _, F = part.shape
    k2 = int(math.ceil(math.log2(max(float(np.max(np.abs(trace_ref))), 2.0 ** -1000)))) + 3
    phi = np.empty((B, K, F, D, D), dtype=np.complex128)
    infos = set()
    for ref in range(D):
        w, info, _ = run_weights(part, D, T, ref, 2.0 ** k2)
        phi[..., ref] = np.ldexp(1.0, k2) * np.conj(w).transpose(0, 1, 3, 2)
        infos.add(info)
    phi = phi.reshape(B * K * F, D, D)
    tr = np.trace(phi, axis1=-2, axis2=-1).real
    assert not (tr[regular] >= 2.0 ** k2).any(), "eps was not above every trace: Phi is not recovered"
    return phi, infos


def trace_of(lu):
    return np.trace(R.xcf(lu["phi"]), axis1=-2, axis2=-1).real


def seq_trace(phi):
    lam = np.zeros(phi.shape[0])
    for i in range(phi.shape[-1]):
        lam = lam + phi[:, i, i].real
    return lam


def check_scaled_weights(phi, w, ref, eps, B, K, F, D):
    """w against conj(phi[:, ref]) / max(tr, eps): 1 / lam and the product, one rounding each"""
    lam = np.maximum(seq_trace(phi), eps)
    got = np.conj(w).transpose(0, 1, 3, 2).reshape(B * K * F, D)
    ok = np.isfinite(1.0 / lam)
    wr, wi = R.xc(phi[:, :, ref])
    lx = R.xr(lam)[:, None]
    want = R.xcf((wr / lx, wi / lx))
    bound = R.gamma_n(2) * np.maximum(np.abs(want.real), np.abs(want.imag)) + R.DENORM
    fin = np.abs(want) < 1e300
    err = np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag))
    return ratio_of(err[ok[:, None] & fin], np.broadcast_to(bound, err.shape)[ok[:, None] & fin]), lam


SHAPES1 = [(1, 1, 1), (1, 3, 63), (3, 1, 64), (1, 5, 65), (1, 3, 130)]     # B, K, F


@pytest.mark.parametrize("D", range(1, 9))
def test_solve_backward_error(D):
    gens = dict(R.REGULAR, scaled_up=lambda d, n, s: R.gen_scaled(d, n, s, 400),
                scaled_down=lambda d, n, s: R.gen_scaled(d, n, s, -400))
    for gi, (name, gen) in enumerate(gens.items()):
        for si, (B, K, F) in enumerate(SHAPES1):
            if name.startswith("scaled") and si not in (1, 4):
                continue
            n = B * K * F
            A, X = gen(D, n, 1000 * D + 10 * gi + si)
            lu = R.lu_reference(A, X)
            assert not lu["singular"].any()
            part = partials_of(A, X, B, K, F)
            phi, infos = recover_phi(part, D, 16, trace_of(lu))
            assert infos == {0}, (name, infos)
            r = record("solve", D, R.solve_ratio(A, X, phi, lu))
            fwd = record("solve, forward", D, ratio_of(np.abs(phi - R.xcf(lu["phi"])), R.forward_bound(A, lu, phi) +
                                                       2 * R.U * np.abs(phi)))
            print(f"D={D} {name} B={B} K={K} F={F}: residual / bound {r:.3g}, forward {fwd:.3g}, "
                  f"rows exchanged {float((lu['piv'] != np.arange(D)).sum(1).mean()):.2f} per system")
            assert r <= 1 and fwd <= 1, (name, B, K, F, r, fwd)
            if name in ("graded", "rank1") and si in (1, 3):
                for ref in {0, D - 1}:
                    w, info, _ = run_weights(part, D, 16, ref, TINY)
                    rr, lam = check_scaled_weights(phi, w, ref, TINY, B, K, F, D)
                    assert info == 0 and record("weights from Phi", D, rr) <= 1, (name, ref, rr.max())


@pytest.mark.parametrize("D", (1, 2, 6, 7, 8))
def test_trace_clamp(D):
    """eps = 1e-2, traces on both sides of it (graded, X rescaled per system) and below zero (indefinite)"""
    B, K, F = 1, 3, 65
    n = B * K * F
    A, X = R.gen_graded(D, n, 40 + D)
    tr = trace_of(R.lu_reference(A, X))
    X = X * (np.ldexp(1.0, np.round(np.log2(1e-2 / tr)).astype(int)) * np.where(np.arange(n) % 2, 2.0, 0.5))[:, None, None]
    for name, (A, X) in (("graded", (A, X)), ("indefinite", R.gen_indefinite(D, n, 41 + D))):
        part = partials_of(A, X, B, K, F)
        phi, _ = recover_phi(part, D, 16, trace_of(R.lu_reference(A, X)))
        w, info, _ = run_weights(part, D, 16, D // 2, 1e-2)
        rr, lam = check_scaled_weights(phi, w, D // 2, 1e-2, B, K, F, D)
        tr = seq_trace(phi)
        print(f"D={D} {name}: {int((tr < 1e-2).sum())} of {n} traces clamped, {int((tr < 0).sum())} negative; "
              f"error / bound {rr.max():.3g}")
        assert (tr < 1e-2).any() and (name == "indefinite") == bool((tr < 0).any())
        assert name == "indefinite" and D > 1 or (tr > 1e-2).any()
        assert info == 0 and record("weights from Phi", D, rr) <= 1


@pytest.mark.parametrize("D", range(1, 9))
def test_info_counts_the_singular_systems_exactly(D):
    B, K, F = 3, 3, 65
    A, X, sing = R.gen_exactsing(D, B * K * F, 60 + D)
    part = partials_of(A, X, B, K, F)
    w, info, _ = run_weights(part, D, 16, 0, TINY)
    assert info == int(sing.sum()) == 195, (info, int(sing.sum()))
    lu = R.lu_reference(A, X)
    ok = ~sing
    phi, infos = recover_phi(part, D, 16, trace_of(lu)[ok], ok)
    assert infos == {195}
    phi[sing] = 0
    assert record("solve", D, R.solve_ratio(A, X, phi, lu)) <= 1                 # the regular bins next to them
    A2, X2 = R.gen_rank1(D, B * K * F, 5)
    assert run_weights(partials_of(A2, X2, B, K, F), D, 16, 0, TINY)[1] == 0    # and back to zero on the next call


@pytest.mark.parametrize("D", (2, 6, 7, 8))
@pytest.mark.parametrize("poison", (NAN, float("inf")))
def test_a_poisoned_bin_stays_alone(D, poison):
    B, K, F = 1, 3, 130
    A, X = R.gen_graded(D, B * K * F, 70 + D)
    part = partials_of(A, X, B, K, F)
    base, _, _ = run_weights(part, D, 16, 0, TINY)
    bad = part.copy()
    bad[0, 0, 1, 1, D, 77] = poison                   # Re A[0, 1] of speaker 1, bin 77
    got, info, _ = run_weights(bad, D, 16, 0, TINY)
    other = np.ones((B, K, F), dtype=bool)
    other[0, 1, 77] = False
    assert np.array_equal(bits(got.transpose(0, 1, 3, 2)[other]), bits(base.transpose(0, 1, 3, 2)[other]))
    assert info == 0 and (np.isinf(poison) or np.isnan(got[0, 1, :, 77]).all())


@pytest.mark.parametrize("D", range(1, 9))
def test_powers_of_two_change_no_bit(D):
    B, K, F = 1, 3, 65
    n = B * K * F
    base = run_weights(partials_of(*R.gen_graded(D, n, 80 + D), B, K, F), D, 16, D - 1, TINY)[0]
    for e in (400, -400):
        got = run_weights(partials_of(*R.gen_scaled(D, n, 80 + D, e), B, K, F), D, 16, D - 1, TINY)[0]
        assert np.isfinite(got).all() and np.array_equal(bits(got), bits(base)), e


@pytest.mark.parametrize("B", (1, 3))
@pytest.mark.parametrize("D", (3, 6, 8))
def test_reduced_chunks_feed_the_solve(B, D):
    """T = 64: four chunks; every system split over them with mixed signs.  The sums the kernel leaves in chunk 0 are the
    float64 sums in chunk order, bit for bit, and Phi satisfies the bound for those sums."""
    K, F, T = 3, 65, 64
    n = B * K * F
    chunks = L().tssep_mvdr_partial_bytes(B, K, D, T, F) // (8 * n * 2 * D * D)
    assert chunks == R.make_plan(B, K, T, F)[0] == 4
    one = partials_of(*R.gen_graded(D, n, 90 + D), B, K, F)
    rs = np.random.RandomState(D)
    part = np.empty((B, chunks) + one.shape[2:])
    part[:, 1:] = rs.standard_normal(part[:, 1:].shape) * np.abs(one)
    part[:, 0] = one[:, 0] - part[:, 1:].sum(1)
    want = part[:, 0].copy()
    for c in range(1, chunks):
        want = want + part[:, c]
    _, info, after = run_weights(part, D, T, 0, TINY)
    assert info == 0 and np.array_equal(bits(after[:, 0]), bits(want))
    assert np.array_equal(bits(after[:, 1:]), bits(part[:, 1:]))
    X, A = (R.unpack_hermitian(want[:, :, m], D).reshape(n, D, D) for m in (0, 1))
    lu = R.lu_reference(A, X)
    phi, _ = recover_phi(part, D, T, trace_of(lu))
    assert record("solve", D, R.solve_ratio(A, X, phi, lu)) <= 1


def test_six_channels_inside_eight():
    B, K, F = 1, 3, 65
    n = B * K * F
    for name in ("graded", "rank1"):
        A6, X6 = R.REGULAR[name](6, n, 17)
        A8 = np.tile(np.eye(8, dtype=np.complex128), (n, 1, 1))
        X8 = A8.copy()
        A8[:, :6, :6], X8[:, :6, :6] = A6, X6
        lu6, lu8 = R.lu_reference(A6, X6), R.lu_reference(A8, X8)
        phi6, _ = recover_phi(partials_of(A6, X6, B, K, F), 6, 16, trace_of(lu6))
        phi8, _ = recover_phi(partials_of(A8, X8, B, K, F), 8, 16, trace_of(lu8))
        assert record("solve", 8, R.solve_ratio(A8, X8, phi8, lu8)) <= 1
        lead = phi8[:, :6, :6]
        r = R.solve_ratio(A6, X6, lead, lu6) * R.solve_gamma(6) / R.solve_gamma(8)      # the chains of D = 8
        f = ratio_of(np.abs(lead - phi6), R.forward_bound(A6, lu6, lead) + R.forward_bound(A6, lu6, phi6))
        print(f"{name}: leading block residual / bound {r.max():.3g}, against the register kernel {f.max():.3g}")
        assert record("solve", 8, r) <= 1 and record("solve, forward", 8, f) <= 1
        assert np.abs(phi8[:, 6:, :6]).max() == 0 and np.abs(phi8[:, :6, 6:]).max() == 0


# ---- stage 2: the statistics -------------------------------------------------------------------------------------------
def make_inputs(B, K, M, D, T, F, f64, seed, offset=0.0, gen=R.graded_mixture):
    """-> Y [B, D, T, F] complex128, masks [B, K, M, T, F] with exact 0, exact 1 and subnormals among them"""
    Ys, ms = [], []
    for b in range(B):
        Y, m = gen(D, T, F, seed + b, K=K, offset=offset)
        rs = np.random.RandomState(seed + 100 + b)
        m = np.stack([m] + [rs.random_sample(m.shape)] * (M - 1), 1)               # [K, M, T, F]
        Ys.append(Y)
        ms.append(m)
    masks = np.stack(ms).astype(np.float64 if f64 else np.float32)
    flat = masks.reshape(-1)
    flat[0::7], flat[1::7], flat[2::7] = 0.0, 1.0, (1e-310 if f64 else 1e-42)
    assert flat.size < 3 or flat[2] != 0
    return np.stack(Ys), masks


def run_psd(Y, masks):
    B, D, T, F = Y.shape
    K, M = masks.shape[1:3]
    nb = L().tssep_mvdr_partial_bytes(B, K, D, T, F)
    chunks, tchunk = R.make_plan(B, K, T, F)
    assert nb == B * chunks * K * 2 * D * D * F * 8
    buf, part = guarded(nb // 8)
    Yd, md = dev(Y), dev(masks)
    st = L().tssep_mvdr_psd(Yd.data_ptr(), md.data_ptr(), int(masks.dtype == np.float64), part.data_ptr(), B, K, M, D, T,
                            F, None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(buf)
    out = part.cpu().numpy().reshape(B, chunks, K, 2, D * D, F)
    assert not np.isnan(out).any(), "an element of the partials was not written"
    return out, chunks, tchunk


def check_partials(Y, masks, part, chunks, tchunk, stage="statistics"):
    B, D, T, F = Y.shape
    K, M = masks.shape[1:3]
    worst = 0.0
    for b in range(B):
        for k in range(K):
            w0 = masks[b, k, 0]
            w1 = masks[b, k, 1] if M == 2 else R.xr(np.ones(1))[0] - R.xr(w0.astype(np.float64))
            for c in range(chunks):
                t0, t1 = c * tchunk, min(T, (c + 1) * tchunk)
                ref, S = R.stats_reference(Y[b], w0, w1, t0, t1)
                got = np.stack([R.unpack_hermitian(part[b, c, k, m], D) for m in (0, 1)])
                bound = R.stats_bound(S, t1 - t0)
                err = np.maximum(np.abs(got.real - R.xf(ref[0])), np.abs(got.imag - R.xf(ref[1])))
                worst = max(worst, record(stage, D, ratio_of(err, bound)))
    return worst


# T, K, F, M, fp64 masks, B, offset: chunk lengths = 1, 2, 3 mod 4, one step, odd and even step counts, tail chunks
CASES2 = [(1, 1, 1, 1, False, 1, 0), (2, 3, 63, 2, True, 1, 40), (3, 4, 64, 1, False, 3, 0), (4, 5, 65, 2, False, 1, 40),
          (5, 8, 129, 1, True, 1, 0), (7, 9, 1, 2, False, 1, 40), (8, 1, 63, 1, True, 3, 0), (9, 3, 64, 2, False, 1, 40),
          (17, 4, 65, 1, True, 1, 0), (31, 5, 129, 2, False, 1, 40), (33, 8, 1, 1, False, 1, 0), (70, 9, 65, 2, True, 3, 40)]


@pytest.mark.parametrize("D", range(1, 9))
def test_statistics_chunk_by_chunk(D):
    seen = set()
    for i, (T, K, F, M, f64, B, offset) in enumerate(CASES2):
        Y, masks = make_inputs(B, K, M, D, T, F, f64, 200 + 20 * D + i, offset * (1 + 1j))
        part, chunks, tchunk = run_psd(Y, masks)
        seen |= {(min(T, (c + 1) * tchunk) - c * tchunk) for c in range(chunks)}
        r = check_partials(Y, masks, part, chunks, tchunk)
        print(f"D={D} T={T} K={K} F={F} M={M} fp64={f64} B={B}: {chunks} chunks of {tchunk}, error / bound {r:.3g}")
        assert r <= 1, (T, K, F, M, f64, B, r)
    steps = {(n + 3) // 4 for n in seen}
    assert {n % 4 for n in seen} == {0, 1, 2, 3} and {1, 2, 3, 4} <= steps, (seen, steps)


# ---- stage 3: the filtering --------------------------------------------------------------------------------------------
def run_apply(Y, w, masks, masking, meps):
    B, D, T, F = Y.shape
    K, M = masks.shape[1:3]
    buf, enh = guarded(B * K * T * F * 2)
    Yd, wd, md = dev(Y), dev(w), dev(masks)
    st = L().tssep_mvdr_apply(Yd.data_ptr(), wd.data_ptr(), md.data_ptr(), int(masks.dtype == np.float64), enh.data_ptr(),
                              B, K, M, D, T, F, int(masking), float(meps), None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(buf)
    e = enh.view(B, K, T, F, 2).cpu().numpy()
    assert not np.isnan(e).any(), "an element of enh was not written"
    return e[..., 0] + 1j * e[..., 1]


def check_apply(Y, w, masks, masking, meps, got, D, pairs=None):
    worst = 0.0
    for b, k in pairs or [(b, k) for b in range(Y.shape[0]) for k in range(w.shape[1])]:
        want, bound = R.apply_reference(Y[b], w[b, k], masks[b, k, 0] if masking else None, meps)
        err = np.maximum(np.abs(got[b, k].real - want.real), np.abs(got[b, k].imag - want.imag))
        worst = max(worst, record("apply", D, ratio_of(err, bound)))
    return worst


# B, K, T, F, M, fp64 masks, masking: one chunk, several, a short tail chunk, more than 4096 tiles
CASES3 = [(1, 1, 16, 1, 1, True, False), (1, 4, 70, 63, 2, False, True), (3, 5, 37, 65, 1, True, True),
          (1, 9, 35, 129, 2, False, False), (1, 5, 5, 64, 1, False, True), (456, 9, 2, 129, 1, False, True)]


@pytest.mark.parametrize("D", range(1, 9))
def test_apply_alone(D):
    plans = set()
    for i, (B, K, T, F, M, f64, masking) in enumerate(CASES3):
        if B > 3 and D not in (2, 7):
            continue
        rs = np.random.RandomState(300 + 10 * D + i)
        if B > 3:
            Y, masks = R._crandn(rs, B, D, T, F), rs.random_sample((B, K, M, T, F)).astype(np.float32)
            assert B * ((F + 63) // 64) * ((K + 3) // 4) > 4096
        else:
            Y, masks = make_inputs(B, K, M, D, T, F, f64, 300 + 10 * D + i)
        if M == 2:
            masks[:, :, 1] = NAN                      # the clamp reads mask 0
        meps = 0.4 if f64 else float(np.float32(0.4))
        assert (masks[:, :, 0] < meps).any() and (masks[:, :, 0] > meps).any()
        w = R._crandn(rs, B, K, D, F)
        got = run_apply(Y, w, masks, masking, meps)
        pairs = None if B <= 3 else [(0, 0), (B // 2, 4), (B - 1, K - 1)]
        r = check_apply(Y, w, masks, masking, meps, got, D, pairs)
        achunks, tchunk = R.apply_plan(B, K, T, F)
        plans.add((achunks, T - (achunks - 1) * tchunk < tchunk))
        print(f"D={D} B={B} K={K} T={T} F={F} M={M} masking={masking}: {achunks} chunks of {tchunk}, error / bound {r:.3g}")
        assert r <= 1
    assert {(1, False), (5, False), (3, True)} <= plans, plans


# ---- stage 4: the chain ------------------------------------------------------------------------------------------------
def rank1_mixture(D, T, F, seed, K=2, offset=0.0):
    """a target and an interferer (one point source each) over a floor of 10^-1.5 .. 10^-6 per bin: the target PSD is rank 1
    plus the floor, cond(A) spreads with the floor; two masks per speaker (M = 2), binary"""
    rs = np.random.RandomState(seed)
    act = rs.random_sample((2, T, F)) < 0.6
    S = R._crandn(rs, 2, T, F) * act
    h = np.exp(2j * np.pi * rs.random_sample((D, 2, F)))
    floor = 10.0 ** -(1.5 + 4.5 * rs.random_sample(F))
    Y = np.einsum("dsf,stf->dtf", h, S) + floor * R._crandn(rs, D, T, F)
    m0 = (act[0] & ~act[1]).astype(np.float64)
    return Y, np.stack([m0 if k % 2 == 0 else (act[1] & ~act[0]).astype(np.float64) for k in range(K)])


def chain(name, B, K, D, T, F, f64, masking, seed):
    M = 1 if name == "graded" else 2
    if name == "graded":
        Y, masks = make_inputs(B, K, M, D, T, F, f64, seed)
    else:
        Y = np.stack([rank1_mixture(D, T, F, seed + b)[0] for b in range(B)])
        m = np.stack([rank1_mixture(D, T, F, seed + b, K=K)[1] for b in range(B)])
        masks = np.stack([m, 1.0 - m + 1e-3], 2).astype(np.float64 if f64 else np.float32)
    ref, meps = D // 2, (0.3 if f64 else float(np.float32(0.3)))
    part, chunks, tchunk = run_psd(Y, masks)
    rs_ = check_partials(Y, masks, part, chunks, tchunk, "chain: statistics")
    w, info, after = run_weights(part, D, T, ref, TINY)
    n = B * K * F
    X, A = (R.unpack_hermitian(after[:, 0, :, m], D).reshape(n, D, D) for m in (0, 1))
    lu = R.lu_reference(A, X)
    assert info == 0 and not lu["singular"].any()
    phi, _ = recover_phi(part, D, T, trace_of(lu))
    rb = record("chain: solve", D, R.solve_ratio(A, X, phi, lu))
    rf = record("chain: solve, forward", D, ratio_of(np.abs(phi - R.xcf(lu["phi"])), R.forward_bound(A, lu, phi) +
                                                     2 * R.U * np.abs(phi)))
    rw = record("chain: weights from Phi", D, check_scaled_weights(phi, w, ref, TINY, B, K, F, D)[0])
    enh = run_apply(Y, w, masks, masking, meps)
    ra = check_apply(Y, w, masks, masking, meps, enh, D)
    got = Hop.mvdr_souden(dev(masks), dev(Y), ref, masking=masking, masking_eps=0.3)      # no LinAlgError
    same = np.array_equal(bits(got.cpu().numpy()), bits(enh))
    cond = np.linalg.cond(A)
    print(f"chain {name} B={B} K={K} D={D} T={T} F={F}: cond {cond.min():.2g} .. {cond.max():.2g}, statistics {rs_:.3g}, "
          f"solve {rb:.3g} (forward {rf:.3g}), weights {rw:.3g}, apply {ra:.3g}, mvdr_souden bit-identical: {same}")
    assert max(rs_, rb, rf, rw, ra) <= 1 and same
    return cond


@pytest.mark.parametrize("D", (6, 8))
@pytest.mark.parametrize("name", ("graded", "rank1"))
def test_chain(name, D):
    cond = chain(name, 2, 3, D, 40, 65, name == "rank1", name == "graded", 400 + D)
    assert cond.max() > 1e8


def test_chain_production_like():
    chain("graded", 1, 8, 6, 96, 65, False, False, 77)


# ---- stage 5: segments -------------------------------------------------------------------------------------------------
MODES = {"sum_cross_talker": 0, "one_minus": 1}


def seg_workspace(K, S, D, T, F):
    nbytes = L().tssep_mvdr_segments_workspace_bytes(K, S, D, T, F)
    C = R.seg_slices(S, F)
    pb = (C * S * 2 * D * D * F * 8 + 15) // 16 * 16
    assert nbytes == pb + S * D * F * 16 + (K * T * 4 + 15) // 16 * 16
    return nbytes // 8, pb // 8, C


def segment_reference(Y, masks, seg, mode, deps, power, psd_real, C):
    """-> psd [2, F, D, D] complex128 of the extended _get_psd, bound"""
    k, s, e = seg
    w0, w1, extra = R.segment_weights(masks[:, 0], k, mode, deps, power)
    ref, S = R.stats_reference(Y, w0, w1, s, e)
    n = R.xr(np.full(1, float(e - s)))[0]
    want = R.xf(ref[0] / n) + 1j * (0.0 if psd_real else 1.0) * R.xf(ref[1] / n)
    return want, R.stats_bound(S / (e - s), (e - s + C - 1) // C, joined=C + 1, extra=extra)


def run_segment_psd(Y, masks, table, mode, deps, power, psd_real):
    D, T, F = Y.shape
    K, S = masks.shape[0], len(table)
    nws, npart, C = seg_workspace(K, S, D, T, F)
    buf, ws = guarded(nws)
    Yd, md, tab = dev(Y), dev(masks), dev(np.asarray(table, dtype=np.int32))
    st = L().tssep_mvdr_segments_psd(Yd.data_ptr(), md.data_ptr(), int(masks.dtype == np.float64), tab.data_ptr(),
                                     ws.data_ptr(), K, S, D, T, F, MODES[mode], float(deps), float(power), int(psd_real),
                                     None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(buf)
    rows = ws[:S * 2 * D * D * F].cpu().numpy().reshape(S, 2, D * D, F)
    assert not np.isnan(rows).any()
    return rows, C


def seg_masks(K, T, F, f64, seed):
    rs = np.random.RandomState(seed)
    m = rs.random_sample((K, 1, T, F)).astype(np.float64 if f64 else np.float32)
    m.reshape(-1)[0::11] = 0.0
    return m


LENGTHS = (1, 2, 15, 16, 17, 79)


@pytest.mark.parametrize("mode,f64,power,psd_real,D", [
    ("sum_cross_talker", True, 1, True, 6), ("sum_cross_talker", False, 2, False, 8), ("sum_cross_talker", False, 0.5, True, 3),
    ("sum_cross_talker", True, 0.5, False, 6), ("one_minus", True, 2, True, 7), ("one_minus", False, 1, False, 2)])
def test_segment_statistics(mode, f64, power, psd_real, D):
    """S = 7: sixteen slices, empty ones where the segment is shorter; every length of LENGTHS, adjacent and overlapping"""
    K, T, F = (1 if mode == "one_minus" else 3), 130, 65
    Y = R.graded_mixture(D, T, F, 500 + D, offset=10 + 10j)[0]
    masks = seg_masks(K, T, F, f64, 501 + D)
    table, t = [], 0
    for i, n in enumerate(LENGTHS):
        table.append((i % K, t, t + n))
        t += n if i % 2 else max(n - 3, 1)
    table.append((K - 1, 5, 84))
    assert max(e for _, _, e in table) <= T
    rows, C = run_segment_psd(Y, masks, table, mode, 1e-4, power, psd_real)
    assert C == 16
    for i, seg in enumerate(table):
        got = np.stack([R.unpack_hermitian(rows[i, m], D) for m in (0, 1)])
        want, bound = segment_reference(Y, masks, seg, mode, 1e-4, power, psd_real, C)
        r = record("segment statistics", D, ratio_of(np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)), bound))
        assert r <= 1 and (not psd_real or (got.imag == 0).all()), (seg, r)
    print(f"{mode} fp64={f64} power={power} psd_real={psd_real} D={D}: worst {WORST[('segment statistics', D)]:.3g}")


@pytest.mark.parametrize("S,C", [(600, 7), (4096, 1)])
def test_segment_statistics_with_fewer_slices(S, C):
    K, D, T, F = 3, 2, 20, 1
    Y = R.graded_mixture(D, T, F, 520)[0]
    masks = seg_masks(K, T, F, False, 521)
    rs = np.random.RandomState(S)
    s = rs.randint(0, T, S)
    table = np.stack([rs.randint(0, K, S), s, np.minimum(T, s + 1 + rs.randint(0, T, S))], 1)
    rows, c = run_segment_psd(Y, masks, table, "sum_cross_talker", 1e-4, 2, False)
    assert c == C
    for i in range(0, S, max(1, S // 150)):
        got = np.stack([R.unpack_hermitian(rows[i, m], D) for m in (0, 1)])
        want, bound = segment_reference(Y, masks, tuple(table[i]), "sum_cross_talker", 1e-4, 2, False, C)
        r = record("segment statistics", D, ratio_of(np.maximum(np.abs(got.real - want.real), np.abs(got.imag - want.imag)), bound))
        assert r <= 1, (i, table[i], r)


def run_segments_fwd(Y, masks, table, deps, eps, masking=False, meps=0.0, psd_real=False):
    """-> enh [K, T, F], info [S], psd rows [S, 2, DD, F] (slice 0), wconj [S, D, F]"""
    D, T, F = Y.shape
    K, S = masks.shape[0], len(table)
    nws, npart, C = seg_workspace(K, S, D, T, F)
    wbuf, ws = guarded(nws)
    ebuf, enh = guarded(K * T * F * 2)
    info = torch.full((S,), 77, dtype=torch.int32, device=DEV)
    Yd, md, tab = dev(Y), dev(masks), dev(np.asarray(table, dtype=np.int32))
    st = L().tssep_mvdr_segments_fwd(Yd.data_ptr(), md.data_ptr(), int(masks.dtype == np.float64), tab.data_ptr(),
                                     enh.data_ptr(), ws.data_ptr(), info.data_ptr(), K, S, D, T, F, 0, float(deps), 1.0,
                                     int(psd_real), float(eps), int(masking), float(meps), None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(wbuf) and bands_intact(ebuf)
    e = enh.view(K, T, F, 2).cpu().numpy()
    rows = ws[:S * 2 * D * D * F].cpu().numpy().reshape(S, 2, D * D, F)
    w = ws[npart:npart + S * D * F * 2].cpu().numpy().reshape(S, D, F, 2)
    return e[..., 0] + 1j * e[..., 1], info.cpu().numpy(), rows, w[..., 0] + 1j * w[..., 1]


def fwd_inputs(D, seed=0):
    K, T, F = 2, 80, 65
    Y, m = R.graded_mixture(D, T, F, 600 + D + seed)
    return Y, np.ascontiguousarray(m[:, None]), K, T, F


TABLE5 = [(0, 0, 20), (0, 20, 45), (1, 5, 40), (1, 30, 70), (0, 50, 62), (1, 70, 80)]      # adjacent; overlapping


@pytest.mark.parametrize("D", (6, 8))
def test_segments_on_graded_data(D):
    Y, masks, K, T, F = fwd_inputs(D)
    S = len(TABLE5)
    _, info1, rows, w40 = run_segments_fwd(Y, masks, TABLE5, 1e-4, 2.0 ** 40)
    X, A = (R.unpack_hermitian(rows[:, m], D).reshape(S * F, D, D) for m in (0, 1))
    lu = R.lu_reference(A, X)
    exch = (lu["piv"] != np.arange(D)).sum(1)
    assert (info1 == 0).all() and not lu["singular"].any() and (exch[:4 * F] > 0).mean() > 0.9
    col = (np.ldexp(1.0, 40) * np.conj(w40)).transpose(0, 2, 1).reshape(S * F, D, 1)      # Phi^[:, 0]
    assert (np.abs(trace_of(lu)) < 2.0 ** 38).all()
    r = record("segments: solve", D, R.solve_ratio(A, X[:, :, :1], col, lu))
    enh, info, rows2, w = run_segments_fwd(Y, masks, TABLE5, 1e-4, TINY, masking=True, meps=0.25)
    assert (info == 0).all() and np.array_equal(bits(rows2), bits(rows))
    owner = -np.ones((K, T), dtype=int)
    for i, (k, s, e) in enumerate(TABLE5):
        owner[k, s:e] = i                               # out[k, s:e] = ... row after row: the later row wins
    assert (owner[1, 30:40] == 3).all()
    worst = 0.0
    for i, (k, s, e) in enumerate(TABLE5):
        want, bound = R.apply_reference(Y, w[i], masks[k, 0], 0.25)
        mine = owner[k] == i
        err = np.maximum(np.abs(enh[k].real - want.real), np.abs(enh[k].imag - want.imag))[mine]
        worst = max(worst, record("segments: apply", D, ratio_of(err, bound[mine])))
    assert np.array_equal(bits(enh[owner < 0]), np.zeros_like(bits(enh[owner < 0])))     # exactly zero outside
    print(f"D={D}: rows exchanged {exch.mean():.2f} per system, solve {r:.3g}, apply {worst:.3g}")
    assert r <= 1 and worst <= 1


def test_segments_singular_rows_are_named_exactly():
    """speaker 1 silent on frames 30..39 and distortion eps 0: the rows of speaker 0 inside have a zero distortion PSD in
    every bin, all others none"""
    D = 6
    Y, masks, K, T, F = fwd_inputs(D, 1)
    masks[1, 0, 30:40] = 0.0
    table = [(0, 0, 30), (0, 30, 40), (1, 25, 45), (0, 40, 80), (0, 32, 36)]
    _, info, _, _ = run_segments_fwd(Y, masks, table, 0.0, TINY)
    assert info.tolist() == [0, F, 0, 0, F], info
    with pytest.raises(torch.linalg.LinAlgError) as ei:
        Hop.segment_mvdr(dev(masks), dev(Y), [table[i] for i in (0, 1, 2, 3)], distortion_eps=0.0, psd_real=False)
    assert "(0, 30, 40)" in str(ei.value) and "1 of 4 segments" in str(ei.value), str(ei.value)


def test_segments_emptied_rows_change_nothing():
    D = 6
    Y, masks, K, T, F = fwd_inputs(D, 2)
    base, binfo, _, _ = run_segments_fwd(Y, masks, TABLE5, 1e-4, TINY)
    empty = [(-1, 0, 10), (K, 0, 10), (0, -5, -1), (1, T + 3, T + 9), (0, 30, 20), (1, 7, 7)]
    table, real = [], []
    for i, row in enumerate(TABLE5):
        table += [empty[i], row]
        real.append(2 * i + 1)
    got, info, rows, _ = run_segments_fwd(Y, masks, table, 1e-4, TINY)
    assert np.array_equal(bits(got), bits(base)) and np.array_equal(info[real], binfo)
    assert (info == 0).all(), info                      # an ignored row reports nothing (seg_info_kernel)
    assert (rows[[2 * i for i in range(len(empty))]] == 0).all()
    out = Hop.segment_mvdr(dev(masks), dev(Y), table, psd_real=False)          # ... and raises nothing
    assert np.array_equal(bits(out.cpu().numpy()), bits(base))


# ---- 6: the report -------------------------------------------------------------------------------------------------------
def test_zz_report():
    stages = sorted({s for s, _ in WORST})
    print("worst error / bound      " + "".join(f"D={d:<7d}" for d in range(1, 9)))
    for s in stages:
        print(f"{s:25s}" + "".join(f"{WORST[(s, d)]:<9.2g}" if (s, d) in WORST else "-        " for d in range(1, 9)))
    assert WORST and all(v <= 1 for v in WORST.values()), {k: v for k, v in WORST.items() if not v <= 1}
