"""masks -> segment table at evaluation size (csrc/segments.hip): four things timed interleaved in one
process, F = 513, at 8 speakers x 30 s (T = 1878), 4 speakers x 4 s (T = 253), one long row of 10 minutes (T = 37500) and
the 10-minute meeting of 8 speakers (0.6 GB of masks: more than the 256 MiB the memory-side cache holds, so THIS row is the
one that reads HBM; the three smaller tensors stay resident in that cache between launches):

  activity  hip_ops.mask_activity alone, HIP events around ONE launch (`_single`: at these sizes mostly the time to get
            a launch from Python to the device) and around --inner launches back to back (`_stream`, per launch), with
            the achieved bytes/s of the latter: K*T*(F+1)*4 bytes over the time, against 8 TB/s (spec) and 6.29 TB/s
            (the measured float4 copy rate of the part)
  mean      torch's masks[:, 0].mean(-1) alone, timed the same two ways: the activity pass's eager counterpart
  route     masks -> table on the device: mask_activity + activity_segments, the count read included (host clock)
  today     what users write without it: masks[:, 0].mean(-1) in torch, .cpu(), threshold, closing and runs in numpy
            (enhancer.normalized_intervals per speaker), hip_ops.segment_table back to the device (host clock)

    python tools/bench_segments.py [--reps 20] [--inner 20] [--out profiles/segments_microbench.jsonl]

Prints one JSON line per shape; nothing is tuned between the contestants: same tensors, same process, alternating."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tssep_amd import hip_ops as H                      # noqa: E402
from tssep_amd.train.enhancer import normalized_intervals   # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12
PARAMS = dict(threshold=0.5, dilation=81, erosion=41, min_frames=8)
SHAPES = (("8 speakers x 30 s", 8, 1878), ("4 speakers x 4 s", 4, 253), ("1 speaker x 10 min", 1, 37500),
          ("8 speakers x 10 min", 8, 37500))


def masks_like(K, T, F, seed):
    """sigmoid-like masks whose frame mean follows an on/off pattern of 0.3-3 s turns"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    on = torch.zeros(K, T, device="cuda")
    rs = np.random.RandomState(seed)
    for k in range(K):
        t = int(rs.randint(0, 60))
        while t < T:
            n = int(rs.randint(20, 190))
            on[k, t:t + n] = 1
            t += n + int(rs.randint(5, 120))
    m = torch.randn(K, 1, T, F, device="cuda", generator=g)
    return m.mul_(3).add_((4 * on - 2)[:, None, :, None]).sigmoid_()


def numpy_closing(bits, dilation, erosion):
    """sliding OR then sliding AND with clipped windows, by cumulative sums (the fast way to write it in numpy)"""
    def count(x, h):
        T = x.shape[1]
        c = np.concatenate([np.zeros((x.shape[0], 1), np.int64), np.cumsum(x, 1)], 1)
        lo, hi = np.maximum(np.arange(T) - h, 0), np.minimum(np.arange(T) + h + 1, T)
        return c[:, hi] - c[:, lo], hi - lo
    n, _ = count(bits, dilation // 2)
    d = n > 0
    n, w = count(d, erosion // 2)
    return n == w


def today(masks, threshold, dilation, erosion, min_frames):
    K, _, T, _ = masks.shape
    act = masks[:, 0].mean(-1).cpu().numpy()
    bits = numpy_closing(act > np.float32(threshold), dilation, erosion)
    rows = [(k, s, e) for k in range(K) for s, e in normalized_intervals(bits[k].astype(np.int8), T)
            if e - s >= min_frames]
    return H.segment_table(rows, masks.device)


def route(masks, **kw):
    return H.activity_segments(H.mask_activity(masks), **kw)


def events(fn, inner):
    """ms per launch of `inner` launches back to back between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20, help="launches back to back of the _stream timings")
    ap.add_argument("--F", type=int, default=513)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_segments needs a GPU"
    lines = []
    for name, K, T in SHAPES:
        F = args.F
        masks = masks_like(K, T, F, seed=K + T)
        a, b = route(masks, **PARAMS), today(masks, **PARAMS)                      # warm-up, and the two agree
        same = a.shape == b.shape and bool(torch.equal(a, b))
        act, mean = (lambda: H.mask_activity(masks)), (lambda: masks[:, 0].mean(-1))
        contestants = {"activity_single": lambda: events(act, 1), "mean_single": lambda: events(mean, 1),
                       "activity_stream": lambda: events(act, args.inner), "mean_stream": lambda: events(mean, args.inner),
                       "route": lambda: clock(lambda: route(masks, **PARAMS)),
                       "today": lambda: clock(lambda: today(masks, **PARAMS))}
        ms = {k: [] for k in contestants}
        for _ in range(args.reps):                                                  # interleaved
            for k, fn in contestants.items():
                ms[k].append(fn())
        nbytes = 4 * K * T * (F + 1)
        med = {k: float(np.median(v)) for k, v in ms.items()}
        line = {"what": "masks -> segment table", "shape": name, "K": K, "T": T, "F": F, **PARAMS,
                "segments": int(a.shape[0]), "tables_equal": same, "reps": args.reps, "inner": args.inner,
                **{f"{k}_ms_median": med[k] for k in ms}, **{f"{k}_ms_min": float(min(v)) for k, v in ms.items()},
                "activity_bytes": nbytes,
                **{f"{k}_TBps": nbytes / med[f"{k}_stream"] / 1e9 for k in ("activity", "mean")},
                "activity_share_of_8.0TBps_spec": nbytes / med["activity_stream"] / 1e-3 / HBM_SPEC,
                "activity_share_of_6.29TBps_copy": nbytes / med["activity_stream"] / 1e-3 / HBM_COPY}
        del masks
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
