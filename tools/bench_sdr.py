"""Micro-benchmark (GPU box): the three launches of the SDR / SI-SDR loss (csrc/sdrloss.hip) -- tssep_sdr_stats_fwd,
tssep_sdr_cost (+ tssep_pit_assign), tssep_sdr_bwd -- against the L2 pair cost and its backward (tssep_pair_cost_fwd(p=2),
tssep_pair_loss_bwd), which move the same bytes, on the same tensors at B = 768, K = 8, N = 64 000, for pit=False (the
diagonal-only passes) and pit=True (all K x K pairs).  All variants run interleaved in one process, HIP events around
`reps` launches after a warm-up, inputs resident (1.6 GB each: past every cache); the median of the rounds is reported
with the ratio to the yardstick and the bytes/s of what the launch has to move (forward: the 2 B K N floats read;
backward: two reads and one write of B K N floats).  A statistics pass much slower than the L2 pair cost would mean the
float64 reduction leaked into the per-sample loop.

    python tools/bench_sdr.py [--rounds 7] [--reps 100] [--out FILE.jsonl]
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
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sdr.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    B, K, N = 768, 8, 64000
    g = torch.Generator(device=dev).manual_seed(0)
    tgt = torch.randn(B, K, N, device=dev, generator=g)
    est = tgt + 0.3 * torch.randn(B, K, N, device=dev, generator=g)
    gout = torch.ones(B, device=dev)
    lines = []
    for pit in (False, True):
        diag = not pit
        part = h.sdr_stats_fwd(est, tgt, diag_only=diag)
        stat, value, cost = h.sdr_cost(part, K, True, 30.0, 1e-8, diag_only=diag)
        _, perm, _, _ = h.pit_assign(cost[:, None], 1, pit=pit, log=False, want_cost=False)
        l2part = h.pair_cost_fwd(est, tgt, 2, diag_only=diag)
        _, l2perm, l2sums, _ = h.pit_assign(l2part, N, pit=pit, log=False, want_cost=False)
        torch.cuda.synchronize()
        assert bool((perm == torch.arange(K, device=dev, dtype=torch.int32)).all()) and torch.equal(perm, l2perm)
        runs = {
            "pair_cost_p2": (lambda: h.pair_cost_fwd(est, tgt, 2, diag_only=diag), None, 2),
            "sdr_stats": (lambda: h.sdr_stats_fwd(est, tgt, diag_only=diag), "pair_cost_p2", 2),
            "l2_assign": (lambda: h.pit_assign(l2part, N, pit=pit, log=False, want_cost=False), None, 0),
            "sdr_cost_assign": (lambda: h.pit_assign(h.sdr_cost(part, K, True, 30.0, 1e-8, diag_only=diag)[2][:, None], 1,
                                                     pit=pit, log=False, want_cost=False), "l2_assign", 0),
            "pair_loss_bwd_p2": (lambda: h.pair_loss_bwd(est, tgt, perm if pit else None, None, gout, 2), None, 3),
            "sdr_bwd": (lambda: h.sdr_bwd(est, tgt, perm if pit else None, stat, gout, True, 30.0, 1e-8),
                        "pair_loss_bwd_p2", 3),
        }
        times = {k: [] for k in runs}
        for fn, _, _ in runs.values():                 # warm-up of every variant
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):                      # interleaved: one window of each variant per round
            for k, (fn, _, _) in runs.items():
                times[k].append(timeit(fn, a.reps))
        res = dict(name="sdr_microbench", pit=pit, scale_invariant=True, sdr_max=30.0, B=B, K=K, N=N, rounds=a.rounds,
                   reps=a.reps, device=torch.cuda.get_device_name(0))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, (_, base, passes) in runs.items():
            res[f"{k}_ms"] = round(med[k], 4)
            res[f"{k}_min_max_ms"] = [round(min(times[k]), 4), round(max(times[k]), 4)]
            if passes:
                res[f"{k}_TBps"] = round(passes * B * K * N * 4 / (med[k] * 1e-3) / 1e12, 3)
            if base:
                res[f"{k}_over_{base}"] = round(med[k] / med[base], 4)
        print(json.dumps(res), flush=True)
        lines.append(res)
    if a.out:
        with open(a.out, "w") as f:
            for res in lines:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
