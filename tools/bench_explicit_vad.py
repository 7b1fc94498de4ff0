"""Micro-benchmark (GPU box): the gated fused tail of explicit_vad (logit rows of 514 floats, the VAD logit at column 0)
against the ungated one, forward (mask head + iSTFT + |est - tgt| sums) and backward (the training step's call: LogMAE
gradient formed in the kernel, d(logit) stored bt_major through iperm; the gated one with the gate BCE folded in), at
the cfg3 / cfg5 shapes.  The two variants run interleaved in one process, HIP events, inputs resident; the median of
the rounds is reported with the gated / ungated ratio.

    python tools/bench_explicit_vad.py [--rounds 7] [--reps 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tssep_amd import functional as Fn, hip_ops as h  # noqa: E402


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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    for name, B, K, N in (("cfg3", 768, 4, 64000), ("cfg5", 48, 8, 480000)):
        T, F = h.stft_frames(N), 513
        _, wsyn = Fn.windows("hann", 1024, 256, dev)
        g = torch.Generator(device=dev).manual_seed(0)
        obs = torch.randn(B, T, F, device=dev, dtype=torch.complex64, generator=g)
        tgt = torch.randn(B, K, N, device=dev, generator=g)
        vad = (torch.rand(B, K, T, device=dev, generator=g) > 0.5).float()
        gout = torch.ones(B, device=dev)
        iperm = torch.stack([torch.randperm(K, device=dev, generator=g) for _ in range(B)]).int()
        runs = {}
        for gated in (False, True, "nobce"):
            logit = torch.randn(B, K, T, F + int(bool(gated)), device=dev, generator=g)
            fwd = lambda l=logit: h.mask_istft_fwd(l, obs, wsyn, N, tgt=tgt)                    # noqa: E731
            y, _ = fwd()
            _, sums = h.logmae_fwd(y, tgt)
            va = (vad, gout) if gated is True else None     # ("nobce": without the BCE fold -- what the gate itself costs)
            bwd = lambda l=logit, y=y, s=sums, va=va: h.mask_istft_bwd(                          # noqa: E731
                None, l, obs, wsyn, loss=(y, tgt, s, gout), vad=va, iperm=iperm, bt_major=True)
            fwd(); bwd(); torch.cuda.synchronize()
            runs[gated] = (fwd, bwd, {"fwd": [], "bwd": []})
        for _ in range(a.rounds):                      # interleaved: ungated, gated, gated without the fold, ungated, ...
            for gated in (False, True, "nobce"):
                fwd, bwd, t = runs[gated]
                t["fwd"].append(timeit(fwd, a.reps))
                t["bwd"].append(timeit(bwd, a.reps))
        res = dict(name=name, B=B, K=K, T=T, N=N, rounds=a.rounds, reps=a.reps)
        for d in ("fwd", "bwd"):
            u = statistics.median(runs[False][2][d])
            v = statistics.median(runs[True][2][d])
            res[f"ungated_{d}_ms"], res[f"gated_{d}_ms"] = round(u, 4), round(v, 4)
            res[f"gated_over_ungated_{d}"] = round(v / u, 4)
            if d == "bwd":
                w = statistics.median(runs["nobce"][2][d])
                res["gated_nobce_bwd_ms"], res["gated_nobce_over_ungated_bwd"] = round(w, 4), round(w / u, 4)
            res[f"spread_{d}"] = [round(min(runs[g_][2][d]), 4) for g_ in (False, True)] + \
                                 [round(max(runs[g_][2][d]), 4) for g_ in (False, True)]
        print(json.dumps(res), flush=True)
        results.append(res)
        del runs, obs, tgt, vad
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
