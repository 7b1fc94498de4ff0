"""Fixture of the segment-wise beamformer, ``segment_bf.npz``, from the REFERENCE functions (stubbed imports of
make_golden.py): ``_get_psd`` (tssep/train/enhancer.py:268-289) and ``SumCrossTalker`` / ``OneMinus``
(tssep/train/enhancer_distortion_mask.py), called the way ``ClassicBF_np.__call__`` calls them (:472-480, 526-530).

Per case ``c``: ``{c}_cfg`` (seed, K, D, T, F, mask_power, masking, masking_eps, distortion eps; -1 = OneMinus),
``{c}_mdtype``, ``{c}_segments`` [S,3] (speaker, start, end), ``{c}_check`` (sums of the inputs),
``{c}_dist`` the distortion masks [K,T,F], ``{c}_psd`` [S,2,F,D,D] the (target, distortion) PSDs those reference
functions return, ``{c}_out`` [K,T,F] the beamformed output.  pb_bss is absent, so the weights are composed in
float64 numpy from those PSDs with the lines of the reference's TorchBF (:250-258, reference channel 0 as in
:497-506): phi = solve(psd_dist, psd_tgt), bf = phi[:, 0] / max(Re tr phi, tiny).

The inputs are not stored (they would not fit the size of a committed fixture): ``inputs(cfg)`` below draws them
from numpy's frozen ``RandomState`` stream, the test calls the same function and checks ``{c}_check`` first.

Run from the repository root with the reference checkout at the path make_golden.py names:
    python tests/golden/make_golden_segment_bf.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# the doctest's activity (enhancer.py:381-382) plus one speaker with two intervals
DOCTEST = [[(0, 55)], [(45, 79)], [(3, 31), (40, 76)]]
EIGHT = [[(0, 30)], [(10, 40), (60, 96)], [(20, 50)], [(0, 24), (30, 60)], [(66, 96)], [(5, 45)], [(50, 90)],
         [(12, 36), (40, 64), (70, 96)]]
CASES = {
    # name: (seed, K, D, T, F, mask dtype, mask_power, masking, masking_eps, distortion eps | None = OneMinus, dia)
    "doc64": (11, 3, 6, 79, 17, "float64", 1, False, 0.0, 1e-4, DOCTEST),
    "pow64": (12, 3, 6, 79, 3, "float64", 2, True, 0.0, 1e-4, DOCTEST),
    "doc32": (13, 3, 7, 79, 3, "float32", 1, True, 0.3, 0.3, DOCTEST),
    "k8": (14, 8, 6, 96, 2, "float32", 2, False, 0.0, 2.0, EIGHT),
    "one": (15, 1, 6, 60, 2, "float64", 2, True, 0.1, None, [[(2, 30), (31, 58)]]),
}


def inputs(seed, K, D, T, F, mdtype):
    """-> Observation [D,T,F] complex128, masks [K,1,T,F] of mdtype; RandomState: the stream is frozen by numpy."""
    rs = np.random.RandomState(seed)
    Y = rs.standard_normal((D, T, F)) + 1j * rs.standard_normal((D, T, F))
    masks = rs.random_sample((K, 1, T, F)).astype(mdtype)
    return Y, masks


def main():
    sys.path.insert(0, HERE)
    from make_golden import _stub_imports, npz
    _stub_imports()
    from tssep.train.enhancer import _get_psd
    from tssep.train.enhancer_distortion_mask import OneMinus, SumCrossTalker

    arrs = {}
    for name, (seed, K, D, T, F, mdtype, power, masking, masking_eps, deps, dia) in CASES.items():
        Y, masks = inputs(seed, K, D, T, F, mdtype)
        obs = np.transpose(Y, (2, 0, 1))                                  # 'mic time freq -> freq mic time'
        m = np.transpose(masks, (1, 0, 3, 2))                             # 'spk mask time freq -> mask spk freq time'
        m = (OneMinus() if deps is None else SumCrossTalker(eps=deps))(m)
        assert m.dtype == np.dtype(mdtype) and m.shape == (2, K, F, T)
        out = np.zeros([K, T, F], dtype=np.complex128)
        segments, psds = [], []
        tiny = np.finfo(np.float64).tiny
        for k, ai in enumerate(dia):
            for s, e in ai:
                assert e - s >= 4 * D, (name, k, s, e)
                psd = _get_psd(m[:, k, :, s:e], obs[:, :, s:e], mask_power=power)        # [2,F,D,D]
                assert np.linalg.cond(psd[1]).max() < 1e8, (name, k, s, e, np.linalg.cond(psd[1]).max())
                phi = np.linalg.solve(psd[1], psd[0])
                lam = np.maximum(np.trace(phi, axis1=-2, axis2=-1).real, tiny)
                bf = phi[..., 0] / lam[:, None]                                           # [F,D]
                enh = np.einsum("fd,fdt->tf", bf.conj(), obs[:, :, s:e])
                if masking:
                    enh = enh * np.maximum(m[0, k, :, s:e].T, masking_eps)
                out[k, s:e] = enh
                segments.append((k, s, e))
                psds.append(psd)
        arrs.update({
            f"{name}_cfg": np.array([seed, K, D, T, F, power, float(masking), masking_eps,
                                     -1.0 if deps is None else deps]),
            f"{name}_mdtype": np.array(mdtype), f"{name}_segments": np.array(segments, dtype=np.int32),
            f"{name}_check": np.array([Y.sum().real, Y.sum().imag, masks.astype(np.float64).sum()]),
            f"{name}_dist": np.transpose(m[1], (0, 2, 1)), f"{name}_psd": np.stack(psds), f"{name}_out": out})
    npz("segment_bf", **arrs)
    size = os.path.getsize(os.path.join(HERE, "segment_bf.npz"))
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE)
                  if f.endswith(".npz") and f != "segment_bf.npz")
    assert size <= largest, (size, largest)


if __name__ == "__main__":
    main()
