"""Micro-benchmark (GPU box): forward and backward of the mask-based MVDR beamformer (csrc/mvdr.hip) at an evaluation-sized
shape -- hip_ops.mvdr_souden with return_state=True and hip_ops.mvdr_souden_bwd, interleaved in one process, HIP events,
median of the rounds, with the algorithmic HBM bytes of each beside the time.  No number from this tool is quoted anywhere
yet: run it on an MI355X first.

    python tools/bench_mvdr_bwd.py [--rounds 7] [--reps 5] [-B 1] [-K 8] [-D 6] [-T 1878] [-F 513] [-M 1] [--masking]
                                   [--fp64-masks] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tssep_amd import hip_ops as h  # noqa: E402


def timeit(fn, reps):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    for name, default in (("B", 1), ("K", 8), ("D", 6), ("T", 1878), ("F", 513), ("M", 1)):
        ap.add_argument("-" + name, type=int, default=default)
    ap.add_argument("--masking", action="store_true")
    ap.add_argument("--fp64-masks", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)
    mdt = torch.float64 if a.fp64_masks else torch.float32
    masks = 0.05 + 0.9 * torch.rand(a.B, a.K, a.M, a.T, a.F, device=dev, generator=g, dtype=mdt)
    obs = torch.view_as_complex(torch.randn(a.B, a.D, a.T, a.F, 2, device=dev, generator=g, dtype=torch.float64))
    genh = torch.view_as_complex(torch.randn(a.B, a.K, a.T, a.F, 2, device=dev, generator=g, dtype=torch.float64))
    kw = dict(masking=a.masking, masking_eps=0.1)
    _, state = h.mvdr_souden(masks, obs, 0, return_state=True, **kw)
    msz = masks.element_size()
    per = a.B * a.T * a.F
    moved = dict(forward=per * (32 * a.D + a.K * a.M * msz + 16 * a.K + (a.K * msz if a.masking else 0)),
                 backward=per * (32 * a.D + 16 * a.K * (2 if a.masking else 1) + a.K * a.M * msz + (a.K * msz if a.masking else 0)))
    calls = dict(forward=lambda: h.mvdr_souden(masks, obs, 0, check_singular=False, return_state=True, **kw),
                 backward=lambda: h.mvdr_souden_bwd(genh, state))
    times = {k: [] for k in calls}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, fn in calls.items():
            times[k].append(timeit(fn, a.reps))
    res = dict(part="mvdr_souden forward / backward", rounds=a.rounds, reps=a.reps, B=a.B, K=a.K, D=a.D, T=a.T, F=a.F, M=a.M,
               masking=a.masking, mask_dtype=str(mdt))
    for k in calls:
        ms = statistics.median(times[k])
        res[k] = dict(ms=round(ms, 4), min_ms=round(min(times[k]), 4), max_ms=round(max(times[k]), 4), bytes=moved[k],
                      tb_per_s=round(moved[k] / ms / 1e9, 3))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
