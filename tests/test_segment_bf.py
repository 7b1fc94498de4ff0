"""Host-side checks of the segment-wise beamformer ClassicBF_np (no GPU): constructor and config, refused
arguments, interval normalisation, the numpy distortion masks against the reference fixture, the workspace query."""
import os
import sys

import numpy as np
import pytest
import torch

from tssep_amd import _lib, configurable
from tssep_amd.train import enhancer, enhancer_distortion_mask as dm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_segment_bf as mg  # noqa: E402

CASES = list(mg.CASES)


def test_config_default_and_constructor():
    cfg = enhancer.ClassicBF_np.get_config()
    assert cfg == {"factory": "tssep.train.enhancer.ClassicBF_np", "bf": "mvdr_souden", "masking": False,
                   "masking_eps": 0,
                   "distortion_mask": {"factory": "tssep.train.enhancer_distortion_mask.SumCrossTalker",
                                       "eps": 0.0001},
                   "pre_wpe": None, "segment_wpe": None, "mask_power": 1}
    bf = enhancer.ClassicBF_np.new()
    assert repr(bf) == "ClassicBF_np()" and bf.name == "ClassicBF_np"
    assert isinstance(bf.distortion_mask, dm.SumCrossTalker) and bf.distortion_mask.eps == 1e-4
    assert enhancer.ClassicBF is enhancer.ClassicBF_np
    bf = enhancer.ClassicBF_np.new({"distortion_mask": {"factory": "tssep.train.enhancer_distortion_mask.OneMinus"},
                                    "mask_power": 2, "masking": True})
    assert isinstance(bf.distortion_mask, dm.OneMinus) and bf.mask_power == 2 and bf.masking is True


def test_factories_resolve_from_reference_names():
    assert configurable.resolve("tssep.train.enhancer.ClassicBF_np") is enhancer.ClassicBF_np
    assert configurable.resolve("tssep.train.enhancer.ClassicBF") is enhancer.ClassicBF_np
    assert configurable.resolve("tssep.train.enhancer_distortion_mask.SumCrossTalker") is dm.SumCrossTalker
    assert configurable.resolve("tssep.train.enhancer_distortion_mask.OneMinus") is dm.OneMinus
    assert configurable.factory_path(dm.SumCrossTalker) == "tssep.train.enhancer_distortion_mask.SumCrossTalker"
    bf = configurable.Configurable.from_config({
        "factory": "tssep.train.enhancer.ClassicBF_np",
        "distortion_mask": {"factory": "tssep.train.enhancer_distortion_mask.SumCrossTalker", "eps": 0.01}})
    assert isinstance(bf, enhancer.ClassicBF_np) and bf.distortion_mask.eps == 0.01


def _args(K=2, M=1, D=6, T=30, F=3):
    return torch.rand(K, M, T, F, dtype=torch.float64), torch.randn(D, T, F, dtype=torch.complex128)


@pytest.mark.parametrize("kw,call,match", [
    (dict(bf="ch0"), {}, "mvdr_souden"),
    (dict(bf="wmwf"), {}, "mvdr_souden"),
    (dict(pre_wpe=object()), {}, "WPE"),
    (dict(segment_wpe=object()), {}, "WPE"),
    (dict(), dict(segment_bf=False), "segment_bf=False"),
    (dict(distortion_mask=lambda m: m), {}, "distortion_mask"),
])
def test_unsupported_arguments_raise_with_the_reason(kw, call, match):
    kw.setdefault("distortion_mask", dm.SumCrossTalker())
    masks, Y = _args()
    with pytest.raises(NotImplementedError, match=match):
        enhancer.ClassicBF_np(**kw)(masks, Y, [[(0, 30)], [(0, 30)]], **call)


def test_reference_checks_are_kept():
    bf = enhancer.ClassicBF_np.new()
    masks, Y = _args(D=5)
    with pytest.raises(AssertionError):                       # mics >= 6
        bf(masks, Y, [[(0, 30)], [(0, 30)]])
    masks, Y = _args(M=2)
    with pytest.raises(NotImplementedError):                  # enhancer.py:481-483
        bf(masks, Y, [[(0, 30)], [(0, 30)]])
    masks, Y = _args()
    for call in (dict(), dict(segment_bf=False), dict(segment_bf=False, numpy_out=False)):
        with pytest.raises(AssertionError):                   # dia is None: segment_bf False and numpy_out True
            bf(masks, Y, None, **call)
    with pytest.raises(AssertionError):                       # not a list
        bf(masks, Y, np.ones((2, 30)), numpy_out=True)
    one = enhancer.ClassicBF_np(distortion_mask=dm.OneMinus())
    with pytest.raises(AssertionError):                       # OneMinus: one speaker
        one(masks, Y, [[(0, 30)], [(0, 30)]])


class _ArrayInterval:
    def __init__(self, pairs):
        self.normalized_intervals = tuple(pairs)


def test_interval_normalisation_from_all_three_forms():
    T = 79
    act = np.zeros(T, dtype=bool)
    act[3:31] = act[40:76] = True
    want = [(3, 31), (40, 76)]
    assert enhancer.normalized_intervals(_ArrayInterval(want), T) == want
    assert enhancer.normalized_intervals(act, T) == want
    assert enhancer.normalized_intervals(act.astype(np.float32), T) == want
    assert enhancer.normalized_intervals(torch.as_tensor(act), T) == want
    assert enhancer.normalized_intervals(want, T) == want
    assert enhancer.normalized_intervals(np.array(want), T) == want
    assert enhancer.normalized_intervals(np.ones(T), T) == [(0, T)]
    assert enhancer.normalized_intervals(np.zeros(T), T) == []
    assert enhancer.normalized_intervals([], T) == []
    assert enhancer.normalized_intervals([(0, 5), (5, 5), (5, 9), (20, 20)], T) == [(0, 5), (5, 9)]   # empty dropped


@pytest.mark.parametrize("bad", [
    [(0, 10), (9, 20)],          # overlap
    [(30, 40), (0, 10)],         # not sorted
    [(-1, 10)], [(70, 80)],      # outside [0, T]
    [(10, 5)],                   # end before start
    [(0.5, 10)],                 # not integral
])
def test_bad_intervals_are_rejected(bad):
    with pytest.raises(ValueError):
        enhancer.normalized_intervals(bad, 79)
    with pytest.raises(ValueError):
        enhancer.normalized_intervals(np.full(79, 2), 79)     # not a 0/1 array


@pytest.mark.parametrize("case", CASES)
def test_numpy_distortion_masks_reproduce_the_fixture(golden, case):
    g = golden("segment_bf")
    seed, K, D, T, F = (int(v) for v in g[case + "_cfg"][:5])
    deps = float(g[case + "_cfg"][8])
    Y, masks = mg.inputs(seed, K, D, T, F, str(g[case + "_mdtype"]))
    np.testing.assert_array_equal(g[case + "_check"], [Y.sum().real, Y.sum().imag, masks.astype(np.float64).sum()])
    fn = dm.OneMinus() if deps < 0 else dm.SumCrossTalker(eps=deps)
    got = fn(np.transpose(masks, (1, 0, 3, 2)))                # mask spk freq time
    assert got.shape == (2, K, F, T) and got.dtype == masks.dtype
    np.testing.assert_array_equal(got[0], np.transpose(masks[:, 0], (0, 2, 1)))
    np.testing.assert_array_equal(np.transpose(got[1], (0, 2, 1)), g[case + "_dist"])
    assert g[case + "_dist"].dtype == masks.dtype


def test_distortion_mask_doctests():
    """the two arrays of the reference's docstrings (enhancer_distortion_mask.py:11-34)"""
    np.testing.assert_array_equal(dm.OneMinus()(np.array([0, 0.5, 1])[None]), [[0., 0.5, 1.], [1., 0.5, 0.]])
    m = np.array([[0, 0.2, 0.8, 1, 0], [0.1, 0, 0.5, 1, 0], [1, 0.1, 1, 0.5, 0]])[None, :, :, None]
    got = np.squeeze(dm.SumCrossTalker(eps=0.01)(m))
    want = [[[0., 0.2, 0.8, 1., 0.], [0.1, 0., 0.5, 1., 0.], [1., 0.1, 1., 0.5, 0.]],
            [[1.1, 0.1, 1.5, 1.5, 0.01], [1., 0.3, 1.8, 1.5, 0.01], [0.1, 0.2, 1.3, 2., 0.01]]]
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-15)
    with pytest.raises(AssertionError):
        dm.SumCrossTalker()(np.zeros((2, 3, 4, 5)))


def test_workspace_query_is_host_only():
    """tssep_mvdr_segments_workspace_bytes needs no GPU; it covers the slice partials, the weights and the
    (speaker, frame) -> segment map, and answers 0 for a shape the kernels do not take."""
    L = _lib.lib()
    for K, S, D, T, F in ((3, 4, 6, 79, 17), (8, 80, 6, 1878, 513), (8, 8, 8, 1878, 513), (1, 1, 1, 1, 1)):
        n = L.tssep_mvdr_segments_workspace_bytes(K, S, D, T, F)
        assert n >= 8 * S * 2 * D * D * F + 16 * S * D * F + 4 * K * T and n % 16 == 0
    assert L.tssep_mvdr_segments_workspace_bytes(8, 80, 9, 1878, 513) == 0        # more than 8 channels
    assert L.tssep_mvdr_segments_workspace_bytes(8, 0, 6, 1878, 513) == 0
    assert L.tssep_mvdr_segments_workspace_bytes(0, 4, 6, 79, 17) == 0
    assert L.tssep_mvdr_segments_workspace_bytes(3, 4, 6, 0, 17) == 0
