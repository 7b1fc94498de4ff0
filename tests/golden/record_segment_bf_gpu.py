"""Fixture ``segment_bf_gpu.npz``: what ``hip_ops.segment_mvdr`` (tssep_mvdr_segments_fwd) returns ON AN MI355X for every
case of ``segment_bf.npz``, kept bit for bit.  It pins the unpacked segment kernels: tests/test_gpu_wpe.py compares the
existing entry point, and the packed one on the sliced observation, with these arrays exactly.

The committed file was recorded with the library built from the commit BEFORE seg_psd_kernel / seg_apply_kernel took their
packed-observation flag (c04657b, "Test MVDR kernels stage by stage against extended precision").  To record again -- only
when a change of the arithmetic of those kernels is intended -- check out and build the commit whose bits are to be kept and
run, on the GPU machine, from the repository root:
    python tests/golden/record_segment_bf_gpu.py [output.npz]
Per case ``c``: ``{c}_out`` [K,T,F] complex128.  The inputs come from ``make_golden_segment_bf.inputs`` as in the tests."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main(path):
    import make_golden_segment_bf as mg
    from tssep_amd import hip_ops as H
    g = dict(np.load(os.path.join(HERE, "segment_bf.npz"), allow_pickle=False))
    out = {}
    for case in mg.CASES:
        seed, K, D, T, F, power = (int(v) for v in g[case + "_cfg"][:6])
        masking, masking_eps, deps = bool(g[case + "_cfg"][6]), float(g[case + "_cfg"][7]), float(g[case + "_cfg"][8])
        Y, masks = mg.inputs(seed, K, D, T, F, str(g[case + "_mdtype"]))
        segments = [tuple(int(v) for v in row) for row in g[case + "_segments"]]
        res = H.segment_mvdr(torch.as_tensor(masks).cuda(), torch.as_tensor(Y).cuda(), segments,
                             mode="one_minus" if deps < 0 else "sum_cross_talker", distortion_eps=max(deps, 0.0),
                             mask_power=power, masking=masking, masking_eps=masking_eps).cpu().numpy()
        print(case, res.shape, "max |gpu - reference fixture|", np.abs(res - g[case + "_out"]).max())
        out[case + "_out"] = res
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "segment_bf_gpu.npz"))
