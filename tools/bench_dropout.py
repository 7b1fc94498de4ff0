"""Micro-benchmark (GPU box): what dropout > 0 costs on the HIP path.

1. The two masked-Tanh kernels alone (csrc/dropout.hip) at the headline shape -- rows = 768 x 4 x 253, P = 320, plain and
   speaker-combined -- beside a device-to-device copy of the same bytes (forward: read + write one tensor; backward: the
   copy moves 2 of the pass's 3 tensors, so its RATE is what is compared) and beside `tssep_tanh_bwd`, the unmasked
   backward pass of the same traffic.  All interleaved in one process, HIP events, median of the rounds.
2. The training step at cfg3 (batch 768 x 4 s, bf16x3) with the sites active (p = 0.1) against the same model with its
   Dropout containers switched off (the launches of dropout = 0), alternating in one process.

    python tools/bench_dropout.py [--rounds 7] [--reps 5] [--batch 768] [--steps 3] [--no-step] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
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


def kernels(a, dev):
    B, K, T, P = a.batch, 4, 253, 320
    rows = B * K * T
    nbytes = rows * P * 4
    g = torch.Generator(device=dev).manual_seed(0)
    z = torch.randn(rows, P, device=dev, generator=g)
    y = torch.empty_like(z)
    dy = torch.randn(rows, P, device=dev, generator=g)
    used = h.dropout_draw(dev)
    out = []
    for combined in (False, True):
        calls = {
            "copy": (lambda: y.copy_(z), 2 * nbytes),
            "dropout_tanh_fwd": (lambda: h.dropout_tanh_fwd(z, y, rows, P, P, K, T, combined, 0.1, used), 2 * nbytes),
            "tanh_bwd": (lambda: h.tanh_bwd(dy, y, rows, P, K, T, combined), 3 * nbytes),
            "dropout_tanh_bwd": (lambda: h.dropout_tanh_bwd(dy, y, rows, P, K, T, combined, 0.1, used), 3 * nbytes),
        }
        times = {k: [] for k in calls}
        for fn, _ in calls.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):                      # interleaved: copy, forward, unmasked backward, backward, copy, ...
            for k, (fn, _) in calls.items():
                times[k].append(timeit(fn, a.reps))
        res = dict(part="kernels", layout="combined" if combined else "plain", rows=rows, P=P, p=0.1, rounds=a.rounds,
                   reps=a.reps)
        copy_rate = None
        for k, (_, moved) in calls.items():
            ms = statistics.median(times[k])
            rate = moved / ms / 1e9                    # TB/s
            copy_rate = rate if k == "copy" else copy_rate
            res[k] = dict(ms=round(ms, 4), min_ms=round(min(times[k]), 4), max_ms=round(max(times[k]), 4),
                          bytes=moved, tb_per_s=round(rate, 3), rate_over_copy=round(rate / copy_rate, 3))
        print(json.dumps(res), flush=True)
        out.append(res)
    return out


def step_time(a, dev):
    import bench
    from tssep_amd.train import runtime
    from tssep_amd.train.optimizer import Adam
    K, N = bench.WORKLOADS["cfg3"]["K"], bench.WORKLOADS["cfg3"]["N"]
    model = bench.build_model(K).to(dev).train()
    sites = model.mask_estimator._dropouts
    for d in sites:
        d.p = 0.1
    opt = Adam(gradient_clipping=10.0, lr=1e-4)
    opt.set_parameters(model.parameters())
    obs, aux, tgt = bench.synth_batch(a.batch, K, N, seed=0)
    ex0 = dict(observation=torch.as_tensor(obs).to(dev), auxInput=torch.as_tensor(aux).to(dev),
               speaker_reverberation_early_ch0=torch.as_tensor(tgt).to(dev), reference_channel=0,
               dataset=["bench"] * a.batch)

    def step():
        opt.zero_grad()
        ex = dict(ex0)
        model.review(ex, model(ex))["loss"].backward()
        opt.step()

    def switch(active):
        for d in sites:
            d.train(active)

    times = {False: [], True: []}
    with runtime.applied(gemm_precision="bf16x3"):
        for active in (False, True):                  # warm-up of both paths
            switch(active)
            np.random.seed(1)
            step()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for active in (False, True):
                switch(active)
                times[active].append(timeit(step, a.steps))
    off, on = statistics.median(times[False]), statistics.median(times[True])
    res = dict(part="step", workload="cfg3", batch=a.batch, arithmetic="bf16x3", rounds=a.rounds, steps=a.steps,
               dropout_0_ms=round(off, 3), dropout_0p1_ms=round(on, 3), cost_ms=round(on - off, 3),
               ratio=round(on / off, 4), spread_0=[round(min(times[False]), 3), round(max(times[False]), 3)],
               spread_0p1=[round(min(times[True]), 3), round(max(times[True]), 3)], sites=len(sites))
    print(json.dumps(res), flush=True)
    return [res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=768)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = kernels(a, dev)
    torch.cuda.empty_cache()
    if not a.no_step:
        results += step_time(a, dev)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
