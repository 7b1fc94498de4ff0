"""Micro-benchmark of the frame-recursive MVDR, one process:

1. hip_ops.online_mvdr on a single stream, B = 1, K = 8, D = 6, F = 513, fp32 masks and a complex64 observation (what the
   separator hands it), Tc = 1 and 16 frames per call with the state carried from call to call: device events around
   the call, 3 warm-ups, the median of 20 with min and max, and the same per frame.  The yardstick is the 16 ms a frame
   lasts (shift 256 at 16 kHz).
2. A whole 30-s utterance (T = 1878 frames) in one call -- what OnlineMVDR does on a validation example -- beside the
   offline hip_ops.mvdr_souden (complex128 observation, fp32 masks) on the same shape, alternating.  The ratio is reported,
   nothing is gated on it: the recursion solves one system per frame and bin, the offline pipeline one per bin.

    python tools/bench_online_mvdr.py [--out profiles/online_mvdr_microbench.jsonl] [--channels 6]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tssep_amd import hip_ops as h  # noqa: E402

WARMUP, REPS = 3, 20


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                spread_ms=round(max(ms) - min(ms), 4))


def alternate(calls):
    times = {k: [] for k in calls}
    for r in range(WARMUP + REPS):
        for k, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[k].append(s.elapsed_time(e))
    return {k: stats(v) for k, v in times.items()}


def inputs(B, K, D, T, F, seed=0):
    torch.manual_seed(seed)
    Y = torch.view_as_complex(torch.randn(B, D, T, F, 2, device="cuda"))
    masks = torch.rand(B, K, T, F, device="cuda") * 0.9 + 0.05
    return masks, Y


def stream(emit, D, B=1, K=8, F=513):
    for Tc in (1, 16):
        masks, Y = inputs(B, K, D, Tc, F)
        state = [h.online_mvdr(masks, Y)[1]]

        def call():
            state[0] = h.online_mvdr(masks, Y, state[0])[1]
        res = alternate({"online_mvdr": call})["online_mvdr"]
        emit(dict(what="stream", B=B, K=K, D=D, F=F, frames=Tc, masks="float32", Y="complex64", online_mvdr=res,
                  ms_per_frame=round(res["median_ms"] / Tc, 4), frame_ms_at_shift_256_16k=16.0,
                  within_a_frame=bool(res["median_ms"] <= 16.0 * Tc), waves=K * B * ((F + 63) // 64)))


def utterance(emit, D, B=1, K=8, F=513, T=1878):
    masks, Y = inputs(B, K, D, T, F, seed=1)
    Y128 = Y.to(torch.complex128)
    m5 = masks[:, :, None].contiguous()
    res = alternate({
        "online_mvdr": lambda: h.online_mvdr(masks, Y, diag_load=1e-6),
        "online_mvdr_c128": lambda: h.online_mvdr(masks, Y128, diag_load=1e-6),
        "mvdr_souden": lambda: h.mvdr_souden(m5, Y128, 0, check_singular=False),
    })
    emit(dict(what="utterance", B=B, K=K, D=D, F=F, frames=T, seconds=30, **res,
              ms_per_frame=round(res["online_mvdr"]["median_ms"] / T, 4),
              ratio_to_mvdr_souden=round(res["online_mvdr_c128"]["median_ms"] / res["mvdr_souden"]["median_ms"], 2),
              real_time_factor=round(res["online_mvdr"]["median_ms"] / 30e3, 5)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "online_mvdr_microbench.jsonl"))
    ap.add_argument("--channels", type=int, nargs="+", default=[6])
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(row):
            row = dict(device=torch.cuda.get_device_name(0), **row)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
        for D in args.channels:
            stream(emit, D)
            utterance(emit, D)


if __name__ == "__main__":
    main()
