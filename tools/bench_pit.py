"""Micro-benchmark (GPU box): the pair-cost pass of pit=True (all K x K costs in one pass over est and tgt) against
tssep_logmae_fwd, the pit=False kernel that reads the same 2 B K N floats for the K matched pairs only, on identical
tensors at the cfg3 (K = 4) and cfg5 (K = 8) training shapes.  Variants: the full pair-cost launch alone, with the
assignment (tssep_pit_assign) behind it, and the diagonal-only launch of a pit=False MSE.  All run interleaved in one
process, HIP events around `reps` launches after a warm-up, inputs resident (1.5 GB per shape: past every cache); the
median of the rounds is reported with the ratio to tssep_logmae_fwd and the bytes/s of the 2 B K N floats.

    python tools/bench_pit.py [--rounds 9] [--reps 100] [--out FILE]
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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pit.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    results = []
    for name, B, K, N in (("cfg3", 768, 4, 64000), ("cfg5", 48, 8, 480000)):
        g = torch.Generator(device=dev).manual_seed(0)
        tgt = torch.randn(B, K, N, device=dev, generator=g)
        est = tgt + 0.3 * torch.randn(B, K, N, device=dev, generator=g)
        runs = {
            "logmae_fwd": lambda: h.logmae_fwd(est, tgt),
            "pair_cost": lambda: h.pair_cost_fwd(est, tgt, 1),
            "pair_cost_assign": lambda: h.pit_assign(h.pair_cost_fwd(est, tgt, 1), N, pit=True, log=True, want_cost=False),
            "pair_cost_p2": lambda: h.pair_cost_fwd(est, tgt, 2),
            "pair_cost_diag_p2": lambda: h.pair_cost_fwd(est, tgt, 2, diag_only=True),
        }
        # same answer first: the matched sum of the identity assignment is LogMAE's argument
        _, sums = h.logmae_fwd(est, tgt)
        _, perm, psums, _ = h.pit_assign(h.pair_cost_fwd(est, tgt, 1), N, pit=True, log=True, want_cost=False)
        torch.cuda.synchronize()
        assert bool((perm == torch.arange(K, device=dev, dtype=torch.int32)).all())
        rel = float(((psums - sums).abs() / sums).max())
        times = {k: [] for k in runs}
        for fn in runs.values():                       # warm-up of every variant at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):                      # interleaved: one window of each variant per round
            for k, fn in runs.items():
                times[k].append(timeit(fn, a.reps))
        nbytes = 2 * B * K * N * 4
        res = dict(name=name, B=B, K=K, N=N, rounds=a.rounds, reps=a.reps, bytes=nbytes, sums_rel_diff_vs_logmae=rel)
        base = statistics.median(times["logmae_fwd"])
        for k, v in times.items():
            med = statistics.median(v)
            res[f"{k}_ms"] = round(med, 4)
            res[f"{k}_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
            res[f"{k}_TBps"] = round(nbytes / (med * 1e-3) / 1e12, 3)
            if k != "logmae_fwd":
                res[f"{k}_over_logmae_fwd"] = round(med / base, 4)
        print(json.dumps(res), flush=True)
        results.append(res)
        del runs, est, tgt
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
