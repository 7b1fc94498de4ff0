"""WPE / ChannelWiseWPE at the host boundary, without a GPU: configuration and factory names of the reference, the arguments
that are refused (each with its own exception, before anything touches a device) and the host-only workspace query."""
import numpy as np
import pytest
import torch

from tssep_amd import _lib, configurable, hip_ops as H
from tssep_amd.train import enhancer
from tssep_amd.train import enhancer_distortion_mask as dm


def test_config_and_factories_resolve_from_reference_names():
    assert configurable.resolve("tssep.train.enhancer.WPE") is enhancer.WPE
    assert configurable.resolve("tssep.train.enhancer.ChannelWiseWPE") is enhancer.ChannelWiseWPE
    assert issubclass(enhancer.ChannelWiseWPE, enhancer.WPE)
    assert enhancer.WPE.get_config() == {"factory": "tssep.train.enhancer.WPE", "taps": 10, "delay": 2, "iterations": 3,
                                         "psd_context": 0, "statistics_mode": "full"}
    bf = configurable.Configurable.from_config({
        "factory": "tssep.train.enhancer.ClassicBF_np",
        "pre_wpe": {"factory": "tssep.train.enhancer.WPE", "taps": 5},
        "segment_wpe": {"factory": "tssep.train.enhancer.ChannelWiseWPE", "statistics_mode": "valid"}})
    assert type(bf.pre_wpe) is enhancer.WPE and (bf.pre_wpe.taps, bf.pre_wpe.delay) == (5, 2)
    assert type(bf.segment_wpe) is enhancer.ChannelWiseWPE and bf.segment_wpe.statistics_mode == "valid"
    assert bf.pre_wpe.name == "WPE"


def _Y(D=2, T=60, F=3, dtype=np.complex128):
    rs = np.random.RandomState(0)
    return (rs.standard_normal((D, T, F)) + 1j * rs.standard_normal((D, T, F))).astype(dtype)


@pytest.mark.parametrize("kw,Y,exc,match", [
    (dict(psd_context=1), _Y(), NotImplementedError, "psd_context"),
    (dict(), _Y(dtype=np.complex64), TypeError, "complex128"),
    (dict(), _Y().real, TypeError, "complex128"),
    (dict(taps=1), _Y(D=9), ValueError, "9 channels"),
    (dict(taps=27), _Y(D=3, T=200), ValueError, "81"),
    (dict(delay=-1), _Y(), ValueError, "delay"),
    (dict(iterations=0), _Y(), ValueError, "iterations"),
    (dict(statistics_mode="half"), _Y(), ValueError, "statistics_mode"),
])
@pytest.mark.parametrize("as_torch", (False, True))
def test_refused_arguments_raise_with_the_reason(kw, Y, exc, match, as_torch):
    with pytest.raises(exc, match=match):
        enhancer.WPE(**kw)(torch.from_numpy(Y) if as_torch else Y)


def test_rows_too_short_for_full_rank_are_named_before_any_launch():
    Y = torch.from_numpy(_Y(D=2, T=60))
    with pytest.raises(ValueError, match=r"\[\(10, 17\)\]"):          # 7 - 2 < 3 * 2
        H.wpe(Y, [(0, 30), (10, 17), (5, 13)], taps=3, delay=2)
    with pytest.raises(ValueError, match=r"\(0, 9\)"):                # 'valid': the first delay + taps - 1 frames do not count
        H.wpe(Y, [(0, 9)], taps=3, delay=2, statistics_mode="valid")
    with pytest.raises(ValueError, match="inside"):
        H.wpe(Y, [(0, 61)], taps=3, delay=2)
    with pytest.raises(ValueError, match=r"\(0, 60\)"):
        enhancer.WPE()(_Y(D=6, T=60))                                 # 60 - 2 frames for 6 channels x 10 taps


def test_classic_bf_refuses_a_foreign_wpe_object():
    masks, Y = torch.rand(2, 1, 30, 3, dtype=torch.float64), torch.randn(6, 30, 3, dtype=torch.complex128)
    for name in ("pre_wpe", "segment_wpe"):
        with pytest.raises(NotImplementedError, match="WPE"):
            enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker(), **{name: object()})(masks, Y, [[(0, 30)]] * 2)
    with pytest.raises(AssertionError):                               # dia is None with segment_wpe (enhancer.py:487)
        enhancer.ClassicBF_np(distortion_mask=dm.SumCrossTalker(), segment_wpe=enhancer.WPE())(
            masks, Y, None, segment_bf=False, numpy_out=True)


def test_workspace_query_is_host_only():
    L = _lib.lib()
    for S, N, D, T, F, taps, delay in ((1, 1878, 6, 1878, 513, 10, 2), (80, 12000, 6, 1878, 513, 10, 2),
                                       (1, 7, 1, 7, 1, 1, 0), (3, 500, 8, 300, 65, 10, 256), (2, 90, 1, 90, 5, 80, 2)):
        ws = L.tssep_wpe_workspace_bytes(S, N, D, T, F, taps, delay)
        K = taps * D
        tiles = ((K + 3) // 4) * ((K + 3) // 4 + 1) // 2 + ((K + 3) // 4) * ((D + 3) // 4)
        # li, R, P, G and one chunk of partial tiles per row
        lower = 8 * N * F + 16 * S * F * (K * K + 2 * K * D) + 256 * S * F * tiles
        assert ws >= lower and ws % 16 == 0, (ws, lower)
    for bad in ((1, 100, 9, 100, 5, 1, 0), (1, 100, 3, 100, 5, 27, 0), (1, 100, 2, 100, 5, 0, 0), (1, 100, 2, 100, 5, 3, -1),
                (1, 100, 2, 100, 5, 3, 257), (0, 100, 2, 100, 5, 3, 2), (1, 0, 2, 100, 5, 3, 2), (1, 100, 2, 100, 0, 3, 2)):
        assert L.tssep_wpe_workspace_bytes(*bad) == 0, bad
