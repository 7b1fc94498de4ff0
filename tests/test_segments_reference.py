"""CPU checks of the discretisation reference (tests/segments_reference.py) that the GPU tests compare against, of the
comparison function they use, and of the host-only part of the ABI (csrc/segments.hip)."""
import os
import re

import numpy as np
import pytest

import segments_reference as R
from tssep_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = ((1, 1), (3, 1), (1, 3), (5, 3), (3, 5), (81, 41))


def _activity(T, dilation):
    return R.edge_rows(T, dilation)


@pytest.mark.parametrize("T", (1, 2, 9, 64, 257))
def test_reference_agrees_with_scipy(T):
    nd = pytest.importorskip("scipy.ndimage")
    for d, e in WINDOWS + ((2 * T + 1, 1), (1, 2 * T + 1)):
        a = _activity(T, d)
        x = np.where(np.isnan(a), -np.inf, a.astype(np.float64))
        y = nd.maximum_filter1d(x, d, axis=1, mode="constant", cval=-np.inf)
        y = nd.minimum_filter1d(y, e, axis=1, mode="constant", cval=np.inf)
        want = R.table_from_bits(y > 0.5)
        got = R.segments(a, 0.5, d, e, 1)
        assert R.compare(len(got), got, want) is None, (T, d, e)
        bits = R.decide(a, 0.5)
        assert np.array_equal(R.dilate(bits, d), nd.binary_dilation(bits, np.ones((1, d), bool)))
        assert np.array_equal(R.erode(bits, e), nd.binary_erosion(bits, np.ones((1, e), bool), border_value=1))


@pytest.mark.parametrize("T", (1, 2, 7, 100, 300))
def test_bit_route_and_minmax_route_agree(T):
    for d, e in WINDOWS + ((2 * T + 1, 1),):
        for mf in (1, 2, 8):
            a = _activity(T, d)
            one, two = R.segments(a, 0.5, d, e, mf), R.segments_minmax(a, 0.5, d, e, mf)
            assert R.compare(len(two), two, one) is None, (T, d, e, mf)
            assert one.dtype == np.int32 and (len(one) == 0 or (0 <= one[:, 1]).all() and (one[:, 1] < one[:, 2]).all()
                                              and (one[:, 2] <= T).all())
            assert len(one) <= a.shape[0] * ((T + 1) // 2)


def test_reference_by_hand():
    a = np.array([[0, 1, 1, 0, 0, 1, 0, 0, 0, 1]], np.float32)
    assert R.segments(a).tolist() == [[0, 1, 3], [0, 5, 6], [0, 9, 10]]
    assert R.segments(a, dilation=3).tolist() == [[0, 0, 7], [0, 8, 10]]          # gap 2 = dilation - 1 closes, 3 does not
    assert R.segments(a, dilation=3, erosion=3).tolist() == [[0, 0, 6], [0, 9, 10]]   # no erosion from frame 0 and T
    assert R.segments(a, dilation=3, erosion=3, min_frames=2).tolist() == [[0, 0, 6]]
    assert R.segments(a, erosion=3).tolist() == []
    assert R.segments(np.float32([[0.5, np.nan, 0.6]])).tolist() == [[0, 2, 3]]     # == threshold and NaN: inactive
    assert R.segments(a, dilation=21).tolist() == [[0, 0, 10]]
    for bad in (dict(dilation=2), dict(erosion=0), dict(erosion=-3), dict(min_frames=0)):
        with pytest.raises(ValueError):
            R.segments(a, **bad)


def test_activity_models():
    rs = np.random.RandomState(0)
    m = (rs.randint(0, 1025, size=(3, 2, 7, 513)) / 1024.0).astype(np.float32)
    a32, a64 = R.activity32_exact(m), R.activity64(m)
    assert a32.dtype == np.float32 and a32.shape == (3, 7)
    assert (np.abs(a32 - a64) <= 2.0 ** -24 * a64).all()                   # one rounding: the division
    assert not np.array_equal(a64, R.activity64(m[:, ::-1]))                # mask index 1 differs and is not read


# ---- planted defects: each one must be caught by the comparison the GPU tests use -------------------------------
def _defect_case():
    T, d, e, mf = 300, 5, 3, 4
    a = _activity(T, d)
    return a, (0.5, d, e, mf), R.segments(a, 0.5, d, e, mf)


def test_compare_accepts_the_reference_itself():
    a, p, want = _defect_case()
    assert len(want) > 20
    assert R.compare(len(want), want, want) is None
    buf = np.concatenate([want, np.full((5, 3), -7, np.int32)])            # rows past the count are ignored
    assert R.compare(len(want), buf, want) is None


def test_defect_zero_padding_for_the_erosion():
    a, (thr, d, e, mf), want = _defect_case()
    bits = R.dilate(R.decide(a, thr), d)
    h = e // 2
    padded = np.concatenate([np.zeros((len(bits), h), bool), bits, np.zeros((len(bits), h), bool)], 1)
    eroded = np.stack([padded[:, t:t + e].all(1) for t in range(bits.shape[1])], 1)
    got = R.table_from_bits(eroded, mf)
    assert R.compare(len(got), got, want) is not None


def test_defect_greater_equal():
    a, (thr, d, e, mf), want = _defect_case()
    got = R.table_from_bits(R.closing(np.nan_to_num(a, nan=0.0) >= np.float32(thr), d, e), mf)
    assert R.compare(len(got), got, want) is not None


def test_defect_off_by_one_end():
    a, p, want = _defect_case()
    got = want.copy()
    got[len(got) // 2, 2] -= 1
    assert R.compare(len(got), got, want) is not None
    got = want.copy()
    got[:, 2] = np.minimum(got[:, 2] + 1, a.shape[1])
    assert R.compare(len(got), got, want) is not None


def test_defect_unsorted_table():
    a, p, want = _defect_case()
    got = want.copy()
    got[[3, 4]] = got[[4, 3]]
    assert R.compare(len(got), got, want) is not None
    assert R.compare(len(got), got[::-1].copy(), want) is not None


def test_defect_short_run_kept():
    a, (thr, d, e, mf), want = _defect_case()
    got = R.segments(a, thr, d, e, mf - 1)
    assert ((got[:, 2] - got[:, 1]) == mf - 1).any()                        # the case holds such a run
    assert R.compare(len(got), got, want) is not None


def test_defect_wrong_dtype_or_count():
    a, p, want = _defect_case()
    assert R.compare(len(want), want.astype(np.int64), want) is not None
    assert R.compare(len(want) - 1, want, want) is not None


# ---- the host-only part of the ABI --------------------------------------------------------------------------------
def test_segments_capacity_is_host_only():
    L = _lib.lib()
    for K, T in ((1, 1), (1, 2), (3, 7), (8, 1878), (4, 253), (19, 1025), (1, 37500), (2, 2 ** 30)):
        assert L.tssep_segments_capacity(K, T) == K * ((T + 1) // 2)
    for K, T in ((0, 5), (5, 0), (-1, 5), (5, -1), (1, 2 ** 30 + 1), (2 ** 20, 2 ** 20), (2 ** 40, 2)):
        assert L.tssep_segments_capacity(K, T) == 0


def test_header_declares_the_entry_points():
    protos = _lib.parse_header()
    for name in ("tssep_mask_activity", "tssep_activity_segments", "tssep_segments_capacity"):
        assert name in protos, name
    text = open(os.path.join(ROOT, "include", "tssep_hip.h")).read()
    assert re.search(r"int64_t\s+tssep_segments_capacity\(int64_t K, int64_t T\);", text)
    src = open(os.path.join(ROOT, "tssep_amd", "csrc", "segments.hip")).read()
    assert "atomic" not in src.replace("no atomics", "") and "asm" not in src


def test_host_refuses_bad_parameters_before_any_launch():
    """even or non-positive windows and min_frames < 1 raise on the host: no device, no tensor is touched"""
    from tssep_amd import hip_ops as H
    from tssep_amd.train.segmenter import ActivitySegmenter
    for bad in (dict(dilation=2), dict(dilation=0), dict(erosion=4), dict(erosion=-1), dict(min_frames=0)):
        with pytest.raises(ValueError):
            H.check_segment_params(**bad)
        with pytest.raises(ValueError):
            H.activity_segments(None, **bad)
        with pytest.raises(ValueError):
            ActivitySegmenter(**bad)
    H.check_segment_params(81, 41, 8)
