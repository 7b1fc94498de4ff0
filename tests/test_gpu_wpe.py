"""The WPE kernels of csrc/wpe.hip on an MI355X, one stage at a time against extended precision (tssep_wpe_power,
_correlations, _solve, _filter through tssep_amd._lib), the whole call (hip_ops.wpe) against the float64 restatement's own
distance from the extended result, the segment table as a batch, the failure paths, and the module level (WPE,
ChannelWiseWPE, ClassicBF_np with pre_wpe / segment_wpe).  References, bounds (derived in that file's docstring, nothing
fitted to a kernel's output) and generators: tests/test_wpe_reference.py.

Stage cases: D in {1, 2, 6, 8}, (taps, delay) in {(1, 0), (3, 1), (10, 2)} (taps * D = 80 at D = 8), F in {1, 63, 64, 65,
130}, T in {taps * D + delay, 200, 257 = one chunk of 256 frames and a last chunk of one frame}, 'full' and 'valid', white
and reverberant data.  Every output buffer lies between NaN guard bands and starts as NaN: an element left unwritten fails
the comparison.

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report):
                                          D=1       D=2       D=6       D=8
    power                                 0.44      0.43      0.4       0.3
    correlations R                        0.14      0.21      0.26      0.17
    correlations P                        0.14      0.16      0.26      0.093
    solve                                 0.13      0.11      0.16      0.1
    filter                                0.33      0.33      0.19      0.24
    whole call / (8 x float64)            0.15      0.17      0.69      0.1
    segment_wpe slice / (8 x float64)     -         -         0.57      -
    segment_wpe composition / (8 x f64)   -         -         0.25      -
The stage cases reached cond(R) 1 .. 1.6e13 (reverberant, D = 8, taps = 10: 2.1e12 .. 1.6e13; D = 6, taps = 10: 3.7e11 ..
1.0e13), info 0 throughout.  Whole call, reverberant, D = 6, taps = 10, 3 iterations: the GPU result is 1.1e-4 from the
extended one in the worst bin where float64 numpy is 1.2e-4 away (tolerance 9.4e-4); white: 4.6e-14 against 5.6e-14.
"""
import numpy as np
import pytest
import torch

from tssep_amd import _lib, hip_ops as Hop
from tssep_amd.train import enhancer
from tssep_amd.train import enhancer_distortion_mask as dm
import test_wpe_reference as W

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GB = 64                     # guard band, in doubles
WORST = {}                  # (stage, D) -> largest error / bound of this run
SEG_RTOL, SEG_ATOL = 1e-9, 1e-12    # the bars of tests/test_gpu_segment_bf.py


def record(stage, D, ratio):
    ratio = float(np.max(ratio)) if np.size(ratio) else 0.0
    WORST[(stage, D)] = max(WORST.get((stage, D), 0.0), ratio)
    return ratio


def L():
    return _lib.lib()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def guarded(n):
    buf = torch.full((n + 2 * GB,), NAN, dtype=torch.float64, device=DEV)
    return buf, buf[GB:GB + n]


def bands_intact(buf):
    return bool(torch.isnan(buf[:GB]).all()) and bool(torch.isnan(buf[-GB:]).all())


def ratio_of(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / bound
    return np.nan_to_num(np.where((err == 0) & (bound == 0), 0.0, r), nan=np.inf)


def cratio(got, want, bound):
    return max(ratio_of(np.abs(got.real - want.real), bound).max(), ratio_of(np.abs(got.imag - want.imag), bound).max())


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64)


def cplx(t, *shape):
    a = t.view(*shape, 2).cpu().numpy()
    return a[..., 0] + 1j * a[..., 1]


# ---- stage by stage -------------------------------------------------------------------------------------------------------
#        D  taps delay T    F    generator       mode
CASES = [(1, 1, 0, 1, 1, "white", "full"),
         (1, 3, 1, 257, 130, "white", "full"),
         (1, 10, 2, 200, 1, "reverberant", "full"),
         (2, 1, 0, 200, 64, "white", "full"),
         (2, 3, 1, 7, 63, "white", "full"),
         (2, 3, 1, 200, 65, "reverberant", "valid"),
         (2, 10, 2, 257, 64, "white", "valid"),
         (6, 1, 0, 6, 130, "white", "full"),
         (6, 3, 1, 257, 63, "reverberant", "full"),
         (6, 10, 2, 62, 5, "white", "full"),
         (6, 10, 2, 200, 65, "reverberant", "full"),
         (8, 1, 0, 200, 63, "reverberant", "full"),
         (8, 3, 1, 25, 64, "white", "full"),
         (8, 10, 2, 82, 1, "white", "full"),
         (8, 10, 2, 257, 5, "reverberant", "full")]


def stage_buffers(D, T, F, taps, delay):
    ws_bytes = L().tssep_wpe_workspace_bytes(1, T, D, T, F, taps, delay)
    assert ws_bytes > 0 and ws_bytes % 16 == 0
    ws = torch.full((ws_bytes // 8,), NAN, dtype=torch.float64, device=DEV)
    tab = torch.tensor([[0, T]], dtype=torch.int32, device=DEV)
    row0 = torch.tensor([0, T], dtype=torch.int64, device=DEV)
    return ws, tab, row0


@pytest.mark.parametrize("D,taps,delay,T,F,gen,mode", CASES)
def test_stages_against_extended(D, taps, delay, T, F, gen, mode):
    K = taps * D
    Y = W.GENERATORS[gen](D, T, F, 100 * D + taps)
    if gen == "reverberant" and T > 20:
        Y[:, 9] = 0.0                                                  # a silent frame: eps takes effect
    ws, tab, row0 = stage_buffers(D, T, F, taps, delay)
    obs = dev(Y)
    op = torch.view_as_real(obs).data_ptr()
    valid = int(mode == "valid")

    # power: li from X = Y through the table, and from a packed estimate
    lbuf, lam = guarded(T * F)
    st = L().tssep_wpe_power(op, None, tab.data_ptr(), row0.data_ptr(), lam.data_ptr(), ws.data_ptr(), 1, T, D, T, F, None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(lbuf)
    li = lam.view(T, F).cpu().numpy()
    lx, g = W.power_reference(Y)
    record("power", D, ratio_of(np.abs(li - lx), g * lx))
    assert (np.abs(li - lx) <= g * lx).all()
    lbuf2, lam2 = guarded(T * F)
    st = L().tssep_wpe_power(op, op, tab.data_ptr(), row0.data_ptr(), lam2.data_ptr(), ws.data_ptr(), 1, T, D, T, F, None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(lbuf2) and np.array_equal(bits(lam2), bits(lam))

    # correlations from the kernel's own li
    rbuf, Rd = guarded(F * K * K * 2)
    pbuf, Pd = guarded(F * K * D * 2)
    st = L().tssep_wpe_correlations(op, lam.data_ptr(), tab.data_ptr(), row0.data_ptr(), Rd.data_ptr(), Pd.data_ptr(),
                                    ws.data_ptr(), 1, T, D, T, F, taps, delay, valid, None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(rbuf) and bands_intact(pbuf)
    Rg, Pg = cplx(Rd, F, K, K), cplx(Pd, F, K, D)
    Rx, Px, bR, bP = W.correlations_reference(Y, li, taps, delay, mode)
    record("correlations R", D, cratio(Rg, Rx, bR))
    record("correlations P", D, cratio(Pg, Px, bP))
    assert cratio(Rg, Rx, bR) <= 1.0 and cratio(Pg, Px, bP) <= 1.0
    assert np.array_equal(Rg, np.swapaxes(Rg.conj(), -2, -1)) and (Rg[:, np.arange(K), np.arange(K)].imag == 0).all()

    # solve: the kernel's own R and P; in 'valid' mode the minimal T leaves too few frames, those cases stop here
    sl = W.stat_range(T, taps, delay, mode)
    if sl.stop - sl.start - (0 if valid else delay) < K:
        return
    gbuf, Gd = guarded(K * D * F * 2)
    info = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    st = L().tssep_wpe_solve(Rd.data_ptr(), Pd.data_ptr(), Gd.data_ptr(), info.data_ptr(), 1, D, F, taps, None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(gbuf) and int(info.item()) == 0
    Gg = np.ascontiguousarray(cplx(Gd, K, D, F).transpose(2, 0, 1))                     # [F, K, D]
    r = W.solve_ratio(Rg, Pg, Gg)
    record("solve", D, r)
    print("cond(R)", np.linalg.cond(Rg).min(), np.linalg.cond(Rg).max(), "solve", r.max())
    assert r.max() <= 1.0

    # filter with the kernel's own G
    xbuf, Xd = guarded(D * T * F * 2)
    st = L().tssep_wpe_filter(op, Gd.data_ptr(), tab.data_ptr(), row0.data_ptr(), Xd.data_ptr(), ws.data_ptr(), 1, T, D, T,
                              F, taps, delay, None)
    torch.cuda.synchronize()
    assert st == 0 and bands_intact(xbuf)
    Xg = cplx(Xd, D, T, F)
    Xx, bX = W.filter_reference(Y, Gg, taps, delay)
    record("filter", D, cratio(Xg, Xx, bX))
    assert cratio(Xg, Xx, bX) <= 1.0


# ---- the whole call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,taps,delay,T,F,gen,mode,its", [
    (6, 10, 2, 200, 8, "white", "full", 3), (6, 10, 2, 200, 8, "reverberant", "full", 3),
    (2, 3, 1, 257, 5, "reverberant", "valid", 3), (8, 10, 2, 300, 3, "reverberant", "full", 2),
    (1, 10, 2, 80, 7, "reverberant", "full", 3), (6, 1, 0, 40, 3, "white", "full", 1)])
def test_whole_call_within_the_float64_error(D, taps, delay, T, F, gen, mode, its):
    Y = W.GENERATORS[gen](D, T, F, 11)
    kw = dict(taps=taps, delay=delay, iterations=its, mode=mode)
    X_ext, tol = W.whole_call_bound(Y, **kw)
    X = Hop.wpe(dev(Y), None, taps, delay, its, mode).cpu().numpy()
    err = np.abs(X - X_ext).max((0, 1))
    print(gen, D, "err", err.max(), "tolerance", tol.min(), tol.max(), "worst ratio", (err / tol).max())
    record("whole call / (8 x float64)", D, err / tol)
    assert (err <= tol).all()


# ---- the table is a batch -------------------------------------------------------------------------------------------------
ROWS = [(0, 40), (40, 80), (30, 90), (30, 90), (10, 50), (60, 110)]


def test_segments_are_a_batch_in_every_order():
    D, T, F, taps, delay = 2, 130, 5, 3, 1
    Y = W.reverberant(D, T, F, 5)
    obs = dev(Y)
    alone = {r: Hop.wpe(obs[:, r[0]:r[1]].contiguous(), None, taps, delay) for r in set(ROWS)}
    orders = [ROWS, ROWS[::-1], ROWS[2:] + ROWS[:2], [ROWS[i] for i in (3, 0, 5, 1, 4, 2)]]
    for rows in orders:
        seg, row0 = Hop.wpe(obs, rows, taps, delay)
        r0 = row0.cpu().numpy()
        assert r0.dtype == np.int64 and np.array_equal(r0, np.concatenate([[0], np.cumsum([e - s for s, e in rows])]))
        assert seg.shape == (D, r0[-1], F) and not torch.isnan(torch.view_as_real(seg)).any()
        for i, r in enumerate(rows):
            assert np.array_equal(bits(seg[:, r0[i]:r0[i + 1]]), bits(alone[r])), (rows, i)
    poisoned = obs.clone()
    poisoned[:, 110:] = complex(NAN, NAN)                             # frames of no row
    seg2, _ = Hop.wpe(poisoned, ROWS, taps, delay)
    seg, _ = Hop.wpe(obs, ROWS, taps, delay)
    assert np.array_equal(bits(seg2), bits(seg))
    whole = Hop.wpe(obs, [(0, T)], taps, delay)[0]
    assert np.array_equal(bits(whole), bits(Hop.wpe(obs, None, taps, delay)))


# ---- failure paths ---------------------------------------------------------------------------------------------------------
def test_singular_row_is_named_and_other_bins_are_untouched():
    D, T, F, taps, delay = 2, 120, 6, 3, 1
    rows = [(0, 40), (40, 80), (80, 120)]
    Y = W.white(D, T, F, 3)
    good = Hop.wpe(dev(Y), rows, taps, delay)[0]
    Yz = Y.copy()
    Yz[:, 40:80, 2] = 0.0
    with pytest.raises(torch.linalg.LinAlgError, match=r"1 of 3 rows \(start, end\): \[\(40, 80\)\]"):
        Hop.wpe(dev(Yz), rows, taps, delay)
    out, row0 = Hop.wpe(dev(Yz), rows, taps, delay, check_singular=False)          # no exception
    keep = [f for f in range(F) if f != 2]
    assert np.array_equal(bits(out[:, :, keep]), bits(good[:, :, keep]))
    assert np.array_equal(bits(out[:, :40, 2]), bits(good[:, :40, 2])) and torch.isnan(out[:, 40:80, 2].real).all()
    # info is written over a sentinel, by the stage and by the whole call
    ws_bytes = L().tssep_wpe_workspace_bytes(3, T, D, T, F, taps, delay)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
    tab = torch.tensor(rows, dtype=torch.int32, device=DEV)
    info = torch.full((3,), 77, dtype=torch.int32, device=DEV)
    seg = torch.empty(D, T, F, dtype=torch.complex128, device=DEV)
    obs = dev(Yz)
    st = L().tssep_wpe_fwd(torch.view_as_real(obs).data_ptr(), tab.data_ptr(), row0.data_ptr(),
                           torch.view_as_real(seg).data_ptr(), ws.data_ptr(), info.data_ptr(), 3, T, D, T, F, taps, delay,
                           1, 0, None)
    torch.cuda.synchronize()
    assert st == 0 and info.tolist() == [0, 1, 0]
    # a NaN in one bin
    Yn = Y.copy()
    Yn[1, 17, 4] = NAN
    outn = Hop.wpe(dev(Yn), rows, taps, delay, check_singular=False)[0]
    keep = [f for f in range(F) if f != 4]
    assert np.array_equal(bits(outn[:, :, keep]), bits(good[:, :, keep]))
    assert torch.isnan(outn[:, :40, 4].real).all() and np.array_equal(bits(outn[:, 40:, 4]), bits(good[:, 40:, 4]))
    with pytest.raises(torch.linalg.LinAlgError, match=r"\[\(0, 40\)\]"):
        Hop.wpe(dev(Yn), rows, taps, delay)
    with pytest.raises(ValueError, match=r"\[\(40, 46\)\]"):
        Hop.wpe(dev(Y), [(0, 40), (40, 46)], taps, delay)


# ---- module level ----------------------------------------------------------------------------------------------------------
def test_wpe_modules_numpy_torch_and_channelwise():
    Y = W.reverberant(3, 60, 5, 8)
    want = Hop.wpe(dev(Y), None, 10, 2, 3)
    a = enhancer.WPE()(Y)
    b = enhancer.WPE()(torch.from_numpy(Y))
    c = enhancer.WPE()(dev(Y), inplace=True)
    assert isinstance(a, np.ndarray) and a.dtype == np.complex128 and isinstance(b, torch.Tensor) and b.is_cuda
    assert np.array_equal(bits(a), bits(want)) and np.array_equal(bits(b), bits(want)) and np.array_equal(bits(c), bits(want))
    X_ext, tol = W.whole_call_bound(Y, taps=10, delay=2, iterations=3)
    assert (np.abs(a - X_ext).max((0, 1)) <= tol).all()
    # the reference's doctest identity (atol 1e-6 there)
    cw = enhancer.ChannelWiseWPE()(dev(Y))
    stacked = torch.cat([enhancer.WPE()(dev(Y[d:d + 1])) for d in range(3)])
    assert cw.shape == (3, 60, 5) and np.array_equal(bits(cw), bits(stacked))
    assert np.array_equal(bits(enhancer.ChannelWiseWPE()(Y)), bits(cw))
    assert not np.array_equal(bits(cw), bits(want))


def _toy(seed=0):
    """the shape of the reference's docstring (enhancer.py:374-420): 6 x 79 x 17, intervals 0:55 and 45:79"""
    rs = np.random.RandomState(seed)
    Y = W.reverberant(6, 79, 17, seed)
    masks = rs.random_sample((2, 1, 79, 17))
    return masks, Y, [[(0, 55)], [(45, 79)]]


def test_classic_bf_pre_wpe_is_wpe_then_bf():
    masks, Y, dia = _toy()
    wpe = enhancer.WPE(taps=3)
    plain = enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker())
    got = enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker(), pre_wpe=wpe)(dev(masks), dev(Y), dia, numpy_out=True)
    want = plain(dev(masks), wpe(dev(Y)), dia, numpy_out=True)
    assert np.array_equal(bits(got), bits(want))
    assert not np.array_equal(bits(got), bits(plain(dev(masks), dev(Y), dia, numpy_out=True)))
    whole = enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker(), pre_wpe=wpe)(
        dev(masks), dev(Y), None, segment_bf=False, numpy_out=True)
    assert np.array_equal(bits(whole), bits(plain(dev(masks), wpe(dev(Y)), None, segment_bf=False, numpy_out=True)))


def test_classic_bf_segment_wpe_is_wpe_per_slice_then_bf_on_that_slice():
    """The composition 'extended-reference WPE of the slice -> segment_mvdr on that slice' within the segment pipeline's
    bar (tests/test_gpu_segment_bf.py: rtol 1e-9, atol 1e-12) plus 8 x the float64 path's own distance, and its two links on
    their own, which are tighter: every packed slice is the extended-reference WPE of that slice within the whole-call
    bound, and the beamformer on the packed observation gives, for every row, the bits of segment_mvdr on the kernel's
    own slice alone."""
    masks, Y, dia = _toy(1)
    taps = 3
    bf = enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker(), segment_wpe=enhancer.WPE(taps=taps))
    out = bf(dev(masks), dev(Y), dia, numpy_out=True)
    assert out.shape == (2, 79, 17)
    seg, row0 = Hop.wpe(dev(Y), [(0, 55), (45, 79)], taps=taps)
    assert row0.tolist() == [0, 55, 89]
    for k, (s, e) in enumerate([(0, 55), (45, 79)]):
        sl = seg[:, row0[k]:row0[k + 1]].contiguous()
        X_ext, tol = W.whole_call_bound(Y[:, s:e], taps=taps, delay=2, iterations=3)
        err = np.abs(sl.cpu().numpy() - X_ext).max((0, 1))
        record("segment_wpe slice / (8 x float64)", 6, err / tol)
        assert (err <= tol).all()
        alone = Hop.segment_mvdr(dev(masks[:, :, s:e]), sl, [(k, 0, e - s)])
        assert np.array_equal(bits(out[k, s:e]), bits(alone[k]))
        want = Hop.segment_mvdr(dev(masks[:, :, s:e]), dev(X_ext), [(k, 0, e - s)])[k].cpu().numpy()
        got = out[k, s:e].cpu().numpy()
        # the beamformer amplifies the float64 error of the WPE slice by the condition of its PSDs, so the bar of the
        # segment pipeline alone (rtol 1e-9, atol 1e-12: same input on both sides) cannot hold here (measured 1.2e-8 of
        # 0.74); as for the whole call, the float64 restatement's slice through the same beamformer says what float64
        # costs at this condition, per bin, and the GPU gets 8 x that on top of the pipeline's own bar
        f64 = Hop.segment_mvdr(dev(masks[:, :, s:e]), dev(W.wpe_float64(Y[:, s:e], taps, 2, 3)), [(k, 0, e - s)])[k]
        own = np.abs(f64.cpu().numpy() - want).max(0)                                # [F]
        d = np.abs(got - want).max(0)
        lim = SEG_ATOL + SEG_RTOL * np.abs(want).max(0) + W.MARGIN * own
        print("row", (k, s, e), "max |out - composition|", d.max(), "float64 path", own.max(), "scale", np.abs(want).max())
        record("segment_wpe composition / (8 x float64)", 6, d / lim)
        assert (d <= lim).all()
        other = torch.cat([out[k, :s], out[k, e:]])
        assert not other.real.any() and not other.imag.any()
    per = bf(dev(masks), dev(Y), dia)
    assert np.array_equal(bits(per[1][(45, 79)]), bits(out[1, 45:79]))


def _golden_case(golden, case):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_segment_bf as mg
    g = golden("segment_bf")
    seed, K, D, T, F, power = (int(v) for v in g[case + "_cfg"][:6])
    masking, masking_eps, deps = bool(g[case + "_cfg"][6]), float(g[case + "_cfg"][7]), float(g[case + "_cfg"][8])
    Y, masks = mg.inputs(seed, K, D, T, F, str(g[case + "_mdtype"]))
    segments = [tuple(int(v) for v in row) for row in g[case + "_segments"]]
    kw = dict(mode="one_minus" if deps < 0 else "sum_cross_talker", distortion_eps=max(deps, 0.0), mask_power=power,
              masking=masking, masking_eps=masking_eps)
    return dev(Y), dev(masks), segments, kw


GOLDEN_CASES = ("doc64", "pow64", "doc32", "k8", "one")


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_existing_segment_entry_point_gives_the_bits_it_gave_before(golden, case):
    """tests/golden/segment_bf_gpu.npz holds what hip_ops.segment_mvdr (tssep_mvdr_segments_fwd) returned on an MI355X
    for every case of segment_bf.npz BEFORE seg_psd_kernel / seg_apply_kernel took their packed-observation flag
    (recorder: tests/golden/record_segment_bf_gpu.py): the unpacked instantiations must still give those bits."""
    Y, masks, segments, kw = _golden_case(golden, case)
    got = Hop.segment_mvdr(masks, Y, segments, **kw)
    assert np.array_equal(bits(got), bits(golden("segment_bf_gpu")[case + "_out"]))


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_packed_entry_point_on_the_sliced_observation_gives_the_same_bits(golden, case):
    """tssep_mvdr_segments_fwd_obs on the fixture's own tables (rows with s != 0, both distortion modes, mask_power,
    masking): obs_seg holds the slices obs[:, s:e] one after the other, so every row reads what the unpacked kernels
    read and must return their bits -- the recorded ones."""
    Y, masks, segments, kw = _golden_case(golden, case)
    obs_seg = torch.cat([Y[:, s:e] for _, s, e in segments], 1).contiguous()
    r0 = np.concatenate([[0], np.cumsum([e - s for _, s, e in segments])]).astype(np.int64)
    assert any(s != 0 for _, s, _ in segments)
    poisoned = torch.full_like(Y, complex(NAN, NAN))              # the unpacked observation is not read
    got = Hop.segment_mvdr(masks, poisoned, segments, obs_seg=obs_seg, row0=dev(r0), **kw)
    assert np.array_equal(bits(got), bits(golden("segment_bf_gpu")[case + "_out"]))


def test_capturable_without_the_singular_check():
    """check_singular=False: once the table is on the device (a list seen before, or a device table with row0 and N) the
    call copies nothing from or to the host -- it runs under torch's sync debug mode 'error', and it is captured in a
    graph and replayed twice, for the whole observation and for a table."""
    D, T, F, taps, delay = 2, 300, 70, 3, 1
    rows = [(0, 280), (10, 300), (100, 130)]
    obs = dev(W.reverberant(D, T, F, 6))
    eager_whole = Hop.wpe(obs, None, taps, delay)
    eager_rows, row0 = Hop.wpe(obs, rows, taps, delay)
    tab, r0 = Hop.wpe_table(rows, obs.device)
    assert r0.data_ptr() == row0.data_ptr()
    N = int(row0[-1].item())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = Hop.wpe(obs, None, taps, delay, check_singular=False)
        b, _ = Hop.wpe(obs, rows, taps, delay, check_singular=False)
        c, _ = Hop.wpe(obs, tab, taps, delay, check_singular=False, row0=row0, N=N)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert np.array_equal(bits(a), bits(eager_whole))
    assert np.array_equal(bits(b), bits(eager_rows)) and np.array_equal(bits(c), bits(eager_rows))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        Hop.wpe(obs, None, taps, delay, check_singular=False)
        Hop.wpe(obs, tab, taps, delay, check_singular=False, row0=row0, N=N)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    live = obs.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        gw = Hop.wpe(live, None, taps, delay, check_singular=False)
        gr, _ = Hop.wpe(live, tab, taps, delay, check_singular=False, row0=row0, N=N)
    for _ in range(2):
        gw.fill_(complex(NAN, NAN))
        gr.fill_(complex(NAN, NAN))
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bits(gw), bits(eager_whole)) and np.array_equal(bits(gr), bits(eager_rows))
    live.mul_(2.0)                                                # the graph reads its inputs anew
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(gw), bits(Hop.wpe(live, None, taps, delay)))


def test_zz_report():
    stages = sorted({s for s, _ in WORST})
    print("worst error / bound".ljust(38) + "".join(f"D={d}".ljust(10) for d in (1, 2, 6, 8)))
    for s in stages:
        print(s.ljust(38) + "".join((f"{WORST[(s, d)]:.2g}" if (s, d) in WORST else "-").ljust(10) for d in (1, 2, 6, 8)))
