"""Micro-benchmark of the guided cACGMM, one process: hip_ops.guided_cacgmm with D = 6 channels,
K = 2 and 8 speakers, T = 1875 (30 s) and 7500 (2 min) frames, F = 513, 20 iterations, once fitted over the whole
recording and once with GSS(block=1875, context=940)'s table.  Device events around one call, 3 warm-ups, the median of
20 with min, max and spread.

Beside every time goes the arithmetic it stands for: gss_fma_per_frame_class(D) fp64 FMAs per (frame, class, iteration)
-- the triangular product L^-1 yh with its squared norm, and the lower triangle of the weighted outer product -- over
the fitted frames (with a block table: the sum of the fit ranges, context included), the time that count would take at
the vector fp64 rate (78.6 TFLOP/s: half the 157.3 TFLOP/s fp32 vector rate, two flops per FMA), and the measured
fraction of that rate.  A record, not a bar: nothing is gated on it.

    python tools/bench_gss.py [--out profiles/gss_microbench.jsonl]
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
FP64_VECTOR_TFLOPS = 78.6
D, F, ITERATIONS = 6, 513, 20


def scene(K, T, seed=0):
    """K speakers with random steering vectors, speaker k active on a window of 2T / (K + 1) frames from k T / (K + 1)
    and present in half of its tf points, noise 20 dB below"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.view_as_complex(torch.randn(*s, 2, device="cuda", dtype=torch.float64, generator=g))
    act = torch.zeros(K, T, dtype=torch.uint8, device="cuda")
    for k in range(K):
        act[k, k * T // (K + 1):(k + 2) * T // (K + 1)] = 1
    on = (torch.rand(K, T, F, device="cuda", generator=g) < 0.5) & act.bool()[:, :, None]
    Y = 0.1 * rnd(D, T, F)
    steer = rnd(K, D, F)
    for k in range(K):
        Y += steer[k][:, None, :] * (rnd(T, F) * on[k])[None]
    return Y.contiguous(), act


def measure(fn):
    ms = []
    for r in range(WARMUP + REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if r >= WARMUP:
            ms.append(s.elapsed_time(e))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                spread_ms=round(max(ms) - min(ms), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "gss_microbench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gss.py measures on the GPU: none found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for K in (2, 8):
            for T in (1875, 7500):
                Y, act = scene(K, T)
                for block, context in ((None, 0), (1875, 940)):
                    table = h.gss_uniform_blocks(T, block, context)
                    fit = int((table[:, 1] - table[:, 0]).sum())
                    res = measure(lambda: h.guided_cacgmm(Y, act, ITERATIONS, blocks=table))
                    gamma = h.guided_cacgmm(Y, act, ITERATIONS, blocks=table)
                    fma = ITERATIONS * fit * F * (K + 1) * h.gss_fma_per_frame_class(D)
                    at_rate_ms = 2 * fma / (FP64_VECTOR_TFLOPS * 1e12) * 1e3
                    row = dict(device=torch.cuda.get_device_name(0), what="guided_cacgmm", D=D, K=K, T=T, F=F,
                               iterations=ITERATIONS, block=block, context=context, blocks=len(table), fitted_frames=fit,
                               launches=2 * ITERATIONS + 2, **res,
                               fma_per_frame_class_iteration=h.gss_fma_per_frame_class(D), fp64_gfma=round(fma / 1e9, 2),
                               ms_at_vector_fp64_rate=round(at_rate_ms, 4), vector_fp64_tflops=FP64_VECTOR_TFLOPS,
                               fraction_of_vector_fp64_rate=round(at_rate_ms / res["median_ms"], 4),
                               real_time_factor=round(res["median_ms"] / (T * 16.0), 6),
                               finite=bool(torch.isfinite(gamma).all()),
                               max_sum_error=float((gamma.double().sum(0) - 1).abs().max()))
                    print(json.dumps(row), flush=True)
                    f.write(json.dumps(row) + "\n")
                    f.flush()


if __name__ == "__main__":
    main()
