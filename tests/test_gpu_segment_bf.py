"""Segment-wise MVDR (ClassicBF_np, hip_ops.segment_mvdr, tssep_mvdr_segments_*) on a real MI355X against the
reference fixture tests/golden/segment_bf.npz (the reference's _get_psd / SumCrossTalker / OneMinus, weights by
TorchBF's lines in float64 numpy) and against the whole-utterance kernels that were here before.
rtol=1e-9, atol=1e-12 throughout: the bars tests/test_gpu_modules.py holds TorchBF to."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_segment_bf as mg  # noqa: E402

RTOL, ATOL = 1e-9, 1e-12
CASES = list(mg.CASES)


def H():
    from tssep_amd import hip_ops
    return hip_ops


def close(got, want, name=""):
    got = torch.as_tensor(got).detach().cpu()
    want = torch.as_tensor(want).detach().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.is_complex():
        got, want = torch.view_as_real(got.contiguous()), torch.view_as_real(want.contiguous())
    err = (got.double() - want.double()).abs()
    print(f"{name}: max abs err {float(err.max()):.3e}, ref scale {float(want.abs().max()):.3e}")
    bad = err > ATOL + RTOL * want.double().abs()
    assert not bool(bad.any()), (
        f"{name}: {int(bad.sum())}/{bad.numel()} off; max abs err {float(err.max()):.3e} "
        f"at {np.unravel_index(int(err.argmax()), err.shape)}; ref scale {float(want.abs().max()):.3e}")


def load(golden, case):
    g = golden("segment_bf")
    seed, K, D, T, F, power = (int(v) for v in g[case + "_cfg"][:6])
    masking, masking_eps, deps = bool(g[case + "_cfg"][6]), float(g[case + "_cfg"][7]), float(g[case + "_cfg"][8])
    Y, masks = mg.inputs(seed, K, D, T, F, str(g[case + "_mdtype"]))
    np.testing.assert_array_equal(g[case + "_check"], [Y.sum().real, Y.sum().imag, masks.astype(np.float64).sum()])
    segments = [tuple(int(v) for v in row) for row in g[case + "_segments"]]
    kw = dict(mode="one_minus" if deps < 0 else "sum_cross_talker", distortion_eps=max(deps, 0.0),
              mask_power=power, masking=masking, masking_eps=masking_eps)
    return torch.as_tensor(Y).cuda(), torch.as_tensor(masks).cuda(), segments, kw, g


def enhancer_of(kw):
    from tssep_amd.train import enhancer, enhancer_distortion_mask as dm
    dist = dm.OneMinus() if kw["mode"] == "one_minus" else dm.SumCrossTalker(eps=kw["distortion_eps"])
    return enhancer.ClassicBF_np(masking=kw["masking"], masking_eps=kw["masking_eps"], distortion_mask=dist,
                                 mask_power=kw["mask_power"])


def dia_of(segments, K):
    return [[(s, e) for k, s, e in segments if k == i] for i in range(K)]


@pytest.mark.parametrize("case", CASES)
def test_dense_output_matches_the_reference_fixture(golden, case):
    """fp64 and fp32 masks alike: the fixture's expectation is computed from the same masks in their own dtype."""
    Y, masks, segments, kw, g = load(golden, case)
    got = enhancer_of(kw)(masks, Y, dia_of(segments, masks.shape[0]), numpy_out=True)
    assert got.is_cuda and got.dtype == torch.complex128
    close(got, g[case + "_out"], name=f"ClassicBF_np {case}")


@pytest.mark.parametrize("case", CASES)
def test_zero_outside_the_intervals_on_a_nan_buffer(golden, case):
    Y, masks, segments, kw, g = load(golden, case)
    K, _, T, F = masks.shape
    out = torch.full((K, T, F), complex(float("nan"), float("nan")), dtype=torch.complex128, device="cuda")
    got = H().segment_mvdr(masks, Y, segments, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    inside = torch.zeros(K, T, dtype=torch.bool)
    for k, s, e in segments:
        inside[k, s:e] = True
    raw = torch.view_as_real(got.cpu())
    assert bool((raw[~inside] == 0).all())                       # exactly zero, no NaN left
    assert bool(torch.isfinite(raw).all())
    close(got, g[case + "_out"], name=f"segment_mvdr {case}")


@pytest.mark.parametrize("case", ["doc64", "k8"])
def test_list_of_dicts_holds_the_dense_values(golden, case):
    Y, masks, segments, kw, g = load(golden, case)
    K = masks.shape[0]
    bf = enhancer_of(kw)
    dense = bf(masks, Y, dia_of(segments, K), numpy_out=True).cpu()
    ret = bf(masks, Y, dia_of(segments, K))
    assert isinstance(ret, list) and len(ret) == K
    assert sorted((k, s, e) for k, d in enumerate(ret) for s, e in d) == sorted(segments)
    for k, d in enumerate(ret):
        for (s, e), v in d.items():
            assert v.shape == (e - s, masks.shape[-1])
            assert torch.equal(torch.view_as_real(v.cpu()), torch.view_as_real(dense[k, s:e]))


@pytest.mark.parametrize("case", CASES)
def test_staged_psds_match_get_psd(golden, case):
    """tssep_mvdr_segments_psd against the arrays _get_psd returned, both planes; psd_real: imaginary part exactly
    zero here (the reference's is rounding noise of (psd + psd.T) / 2 around zero, inside atol)."""
    Y, masks, segments, kw, g = load(golden, case)
    got = H().segment_psd(masks, Y, segments, mode=kw["mode"], distortion_eps=kw["distortion_eps"],
                          mask_power=kw["mask_power"], psd_real=True)
    assert bool((got.imag == 0).all())
    close(got, g[case + "_psd"], name=f"psd {case}")


def cross_talker_plane(masks, eps):
    """SumCrossTalker with torch ops: ascending sum over the other speakers, in the mask's dtype."""
    K = masks.shape[0]
    planes = []
    for k in range(K):
        acc = torch.zeros_like(masks[0, 0])
        for j in range(K):
            if j != k:
                acc = acc + masks[j, 0]
        planes.append(torch.clamp(acc, min=eps))
    return torch.stack(planes)                                   # [K,T,F]


def test_whole_utterance_segments_equal_mvdr_souden():
    """One segment (k, 0, T) per speaker with psd_real=0 is TorchBF with the SumCrossTalker plane handed in: the
    1 / T of the segment PSDs cancels in phi."""
    K, D, T, F = 4, 6, 200, 70
    gen = torch.Generator().manual_seed(3)
    Y = torch.randn(D, T, F, dtype=torch.complex128, generator=gen).cuda()
    for dtype in (torch.float64, torch.float32):
        masks = torch.rand(K, 1, T, F, dtype=dtype, generator=gen).cuda()
        two = torch.stack([masks[:, 0], cross_talker_plane(masks, 1e-4)], dim=1)
        want = H().mvdr_souden(two[None], Y[None], 0)[0]
        got = H().segment_mvdr(masks, Y, [(k, 0, T) for k in range(K)], distortion_eps=1e-4, psd_real=False)
        close(got, want, name=f"segments (k,0,T) vs mvdr_souden {dtype}")


def seeded_diarization(K, T, per_speaker, seed):
    """about per_speaker disjoint intervals of 60-170 frames for every speaker"""
    rs = np.random.RandomState(seed)
    segments = []
    for k in range(K):
        t = int(rs.randint(0, 40))
        for _ in range(per_speaker):
            length = int(rs.randint(60, 170))
            if t + length > T:
                break
            segments.append((k, t, t + length))
            t += length + int(rs.randint(5, 60))
    return segments


def test_production_size_against_the_sliced_loop():
    """K=8, D=6, T=1878, F=513, about 80 segments, fp32 masks as the model emits them: one call against a loop of
    hip_ops.mvdr_souden on time slices with host-built two-plane masks (psd_real=0 on both sides; the slice's
    1 / len cancels in phi).  No segment may be left out of the comparison."""
    K, D, T, F = 8, 6, 1878, 513
    gen = torch.Generator().manual_seed(5)
    Y = torch.randn(D, T, F, dtype=torch.complex128, generator=gen).cuda()
    masks = torch.rand(K, 1, T, F, generator=gen).cuda()
    segments = seeded_diarization(K, T, 10, seed=5)
    assert 70 <= len(segments) <= 90, len(segments)
    got = H().segment_mvdr(masks, Y, segments, distortion_eps=1e-4, psd_real=False)
    dist = cross_talker_plane(masks, 1e-4)
    want = torch.zeros_like(got)
    left_out = []
    for k, s, e in segments:
        two = torch.stack([masks[k, 0, s:e], dist[k, s:e]])[None, None]
        try:
            want[k, s:e] = H().mvdr_souden(two, Y[None, :, s:e], 0)[0, 0]
        except torch.linalg.LinAlgError:
            left_out.append((k, s, e))
    assert len(left_out) <= 0, left_out
    close(got, want, name="production size vs sliced loop")


def test_singular_segment_is_named():
    """The distortion mask of speaker 0 is all zero on frames 10..14 (speaker 1 silent there, eps 0): that segment's
    distortion PSD is the zero matrix and the error names it, and only it."""
    K, D, T, F = 2, 6, 120, 9
    gen = torch.Generator().manual_seed(9)
    Y = torch.randn(D, T, F, dtype=torch.complex128, generator=gen).cuda()
    masks = torch.rand(K, 1, T, F, dtype=torch.float64, generator=gen)
    masks[1, 0, 10:14] = 0.0
    masks = masks.cuda()
    segments = [(0, 10, 14), (0, 30, 100), (1, 20, 90)]
    with pytest.raises(torch.linalg.LinAlgError) as ei:
        H().segment_mvdr(masks, Y, segments, distortion_eps=0.0)
    msg = str(ei.value)
    assert "(0, 10, 14)" in msg and "(0, 30, 100)" not in msg and "(1, 20, 90)" not in msg, msg
    assert "1 of 3 segments" in msg, msg
    from tssep_amd.train import enhancer, enhancer_distortion_mask as dm
    with pytest.raises(torch.linalg.LinAlgError, match=r"\(0, 10, 14\)"):
        enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker(eps=0.0))(
            masks, Y, [[(10, 14), (30, 100)], [(20, 90)]], numpy_out=True)
    ok = H().segment_mvdr(masks, Y, segments[1:], distortion_eps=0.0)          # the others alone are fine
    assert bool(torch.isfinite(torch.view_as_real(ok)).all())


def test_capturable_without_the_singular_check(golden):
    """check_singular=False: no host sync inside -- the call is captured in a graph and replayed twice."""
    Y, masks, segments, kw, g = load(golden, "doc64")
    K, _, T, F = masks.shape
    table = H().segment_table(segments, "cuda")
    out = torch.zeros(K, T, F, dtype=torch.complex128, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H().segment_mvdr(masks, Y, table, out=out, check_singular=False, **kw)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        H().segment_mvdr(masks, Y, table, out=out, check_singular=False, **kw)
    replays = []
    for _ in range(2):
        out.fill_(complex(float("nan"), float("nan")))
        graph.replay()
        torch.cuda.synchronize()
        replays.append(out.clone())
    assert torch.equal(torch.view_as_real(replays[0]), torch.view_as_real(replays[1]))
    assert torch.equal(torch.view_as_real(replays[0]), torch.view_as_real(eager))
    close(replays[0], g["doc64_out"], name="graph replay")
