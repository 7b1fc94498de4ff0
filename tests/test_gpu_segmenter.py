"""The chain masks -> ActivitySegmenter -> ClassicBF_np on a real MI355X: a device-born segment table gives the output
of the host interval lists derived from the reference (tests/segments_reference.py), bit for bit."""
import numpy as np
import pytest
import torch

import segments_reference as R

pytestmark = pytest.mark.gpu

K, T, F, D = 3, 200, 17, 6
PARAMS = dict(threshold=0.5, dilation=5, erosion=3, min_frames=8)      # min_frames 8: more frames than channels


def _inputs():
    """masks in multiples of 2^-10 (the float32 activity is exact, no decision is in doubt) whose mean over F follows a
    per-speaker on/off pattern with short gaps and spikes; a complex128 observation of six channels"""
    rs = np.random.RandomState(11)
    on = np.zeros((K, T), bool)
    for k in range(K):
        t = int(rs.randint(0, 12))
        while t < T:
            n = int(rs.randint(3, 40))
            on[k, t:t + n] = True
            t += n + int(rs.randint(1, 25))
    level = np.where(on, 0.75, 0.2)[:, None, :, None]
    m = np.clip(level + 0.2 * (rs.rand(K, 1, T, F) - 0.5), 0, 1)
    masks = (np.round(m * 1024) / 1024).astype(np.float32)
    Y = rs.randn(D, T, F) + 1j * rs.randn(D, T, F)
    return masks, Y


@pytest.fixture(scope="module")
def case():
    from tssep_amd.train.segmenter import ActivitySegmenter
    masks, Y = _inputs()
    want = R.segments(R.activity32_exact(masks), **PARAMS)
    assert len(want) >= 6 and len(set(want[:, 0].tolist())) == K, want          # every speaker, several intervals
    assert ((want[:, 2] - want[:, 1]) >= 8).all()
    dm, dY = torch.from_numpy(masks).cuda(), torch.from_numpy(Y).cuda()
    table = ActivitySegmenter(**PARAMS)(dm)
    return dm, dY, table, want


def _bf():
    from tssep_amd.train import enhancer, enhancer_distortion_mask as dm
    return enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker())


def test_table_is_the_reference_table(case):
    dm, dY, table, want = case
    assert table.is_cuda and table.dtype == torch.int32
    assert R.compare(table.shape[0], table.cpu().numpy(), want) is None
    from tssep_amd.train.segmenter import ActivitySegmenter
    assert ActivitySegmenter.intervals(table, K) == R.intervals(want, K)


def test_dense_output_equals_the_host_interval_lists(case):
    dm, dY, table, want = case
    got = _bf()(dm, dY, table, numpy_out=True)
    ref = _bf()(dm, dY, R.intervals(want, K), numpy_out=True)                # singular check passes: no LinAlgError
    assert got.shape == (K, T, F) and got.dtype == torch.complex128
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(ref))
    assert bool(torch.isfinite(torch.view_as_real(got)).all()) and float(got.abs().max()) > 0


def test_views_of_numpy_out_false_are_the_same(case):
    dm, dY, table, want = case
    dense = _bf()(dm, dY, table, numpy_out=True)
    got = _bf()(dm, dY, table)
    ref = _bf()(dm, dY, R.intervals(want, K))
    assert isinstance(got, list) and len(got) == K
    for k in range(K):
        assert list(got[k]) == list(ref[k]) == R.intervals(want, K)[k]
        for (s, e), v in got[k].items():
            assert v.shape == (e - s, F)
            assert torch.equal(torch.view_as_real(v), torch.view_as_real(ref[k][(s, e)]))
            assert torch.equal(torch.view_as_real(v), torch.view_as_real(dense[k, s:e]))


def test_table_with_segment_wpe_equals_the_host_interval_lists(case):
    """segment_wpe needs host numbers (the packed size): the table is read once and the rows are the lists' rows.
    min_frames = 20 here: taps * channels + delay = 13 frames is the least WPE takes, and a row needs some more than
    that for a system that is not singular to rounding."""
    from tssep_amd.train import enhancer, enhancer_distortion_mask as dist
    from tssep_amd.train.segmenter import ActivitySegmenter
    dm, dY, _, _ = case
    params = {**PARAMS, "min_frames": 20}
    want = R.segments(R.activity32_exact(dm.cpu().numpy()), **params)
    assert len(want) >= 6 and ((want[:, 2] - want[:, 1]) >= 20).all()
    table = ActivitySegmenter(**params)(dm)
    assert R.compare(table.shape[0], table.cpu().numpy(), want) is None
    bf = enhancer.ClassicBF_np(distortion_mask=dist.SumCrossTalker(),
                               segment_wpe=enhancer.WPE(taps=2, delay=1, iterations=1))
    got = torch.view_as_real(bf(dm, dY, table, numpy_out=True))
    ref = torch.view_as_real(bf(dm, dY, R.intervals(want, K), numpy_out=True))
    plain = torch.view_as_real(_bf()(dm, dY, table, numpy_out=True))
    print(f"finite {int(torch.isfinite(got).sum())}/{got.numel()}, max |got - ref| {float((got - ref).abs().max()):.3e}, "
          f"max |got - plain| {float((got - plain).abs().max()):.3e}")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, ref)
    assert not torch.equal(got, plain)                                       # the dereverberation took part


def test_empty_table_gives_zeros(case):
    dm, dY, table, want = case
    from tssep_amd.train.segmenter import ActivitySegmenter
    empty = ActivitySegmenter(threshold=2.0)(dm)
    assert empty.shape == (0, 3) and empty.dtype == torch.int32 and empty.is_cuda
    out = _bf()(dm, dY, empty, numpy_out=True)
    assert out.shape == (K, T, F) and out.dtype == torch.complex128 and not bool(out.any())
    assert _bf()(dm, dY, empty) == [{} for _ in range(K)]


@pytest.mark.parametrize("row", ((K, 10, 30), (0, 150, T + 1), (-1, 10, 30), (1, -2, 30)))
def test_rows_outside_the_utterance_are_refused(case, row):
    dm, dY, table, want = case
    bad = torch.cat([table, torch.tensor([row], dtype=torch.int32, device="cuda")])
    with pytest.raises(ValueError):
        _bf()(dm, dY, bad, numpy_out=True)
    with pytest.raises(ValueError):
        _bf()(dm, dY, bad)


def test_segmenter_round_trips_through_its_config():
    from tssep_amd.configurable import Configurable
    from tssep_amd.train.segmenter import ActivitySegmenter
    cfg = ActivitySegmenter.get_config(dict(dilation=81, erosion=41, min_frames=8))
    assert cfg == {"factory": "tssep.train.segmenter.ActivitySegmenter", "threshold": 0.5, "dilation": 81,
                   "erosion": 41, "min_frames": 8}
    seg = Configurable.from_config(cfg)
    assert isinstance(seg, ActivitySegmenter)
    assert (seg.threshold, seg.dilation, seg.erosion, seg.min_frames) == (0.5, 81, 41, 8)
    assert ActivitySegmenter.get_config(None)["dilation"] == 1                 # the neutral defaults
    with pytest.raises(ValueError):
        Configurable.from_config({**cfg, "dilation": 80})


def test_activity_and_the_masks_it_was_averaged_from_give_the_same_table(case):
    dm, dY, table, want = case
    from tssep_amd import hip_ops as H
    from tssep_amd.train.segmenter import ActivitySegmenter
    seg = ActivitySegmenter(**PARAMS)
    act = H.mask_activity(dm)
    assert act.shape == (K, T)
    assert torch.equal(seg(act), table)
    two = torch.cat([dm, 1 - dm], dim=1)                                      # M = 2: mask index 0 is the target mask
    assert torch.equal(seg(two), table)
    buf, count = seg(dm, return_count=True)
    assert buf.shape == (K * (T // 2), 3) and int(count.item()) == table.shape[0]
