"""Micro-benchmark (GPU box): the FreqMSE tail, forward + backward, at bench.py's headline shape (cfg3) and its
8-utterance shard (cfg4), read from bench.py's WORKLOADS.  Variants, interleaved in one process after a warm-up:

    fused     tssep_mask_specmse_fwd -> tssep_pit_assign;  tssep_mask_specmse_bwd            (pit=False: diag_only)
    fused_pit the same with the full K x K costs and the assignment (pit=True)
    unfused   tssep_maskhead_fwd -> tssep_specmse_fwd -> tssep_pit_assign;  tssep_specmse_bwd -> tssep_maskhead_bwd
    logmae    the LogMAE fused tail (tssep_mask_istft_fwd + finalize; tssep_mask_istft_bwd_loss), for scale

Reported per variant: the median ms per call (forward + backward) with the min / max of the rounds, the algorithmic
bytes of the FUSED FreqMSE tail -- forward 12 B K T F + 8 B T F read, backward the same read plus 4 B K T F written --
and the share of 8 TB/s those bytes amount to at that time (the kernels are bandwidth-bound: HBM streaming, a few
flops per byte).  The unfused chain moves more than the algorithmic bytes (it writes and re-reads mask, estimate and
d(estimate)); its share says how far it is from the same floor.

--step adds bench.py's whole eager training step (its model, its synthetic batch) with LogMAE and with FreqMSE on the same
weights, alternating, for scale: reported, not gated.

    python tools/bench_spectral.py [--rounds 9] [--reps 20] [--step] [--out profiles/spectral_microbench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from tssep_amd import functional as Fn, hip_ops as h  # noqa: E402

HBM_BYTES_PER_S = 8e12


def timeit(fn, reps):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def whole_step(bench, dev, rounds, reps):
    """bench.py's model, batch and eager training step (forward, review, backward, Adam) with LogMAE and with FreqMSE on the
    same weights, alternating: ms per step.  Reported, not gated."""
    import numpy as np
    from tssep_amd.train import loss
    from tssep_amd.train.optimizer import Adam
    lines = []
    for name in ("cfg4", "cfg3"):
        w = bench.WORKLOADS[name]
        B, K, N = w["batch"], w["K"], w["N"]
        model = bench.build_model(K).to(dev)
        model.train()
        opt = Adam(gradient_clipping=10.0, lr=1e-5)
        opt.set_parameters(model.parameters())
        obs, aux, tgt = bench.synth_batch(B, K, N, seed=0)
        ex0 = dict(observation=torch.as_tensor(obs).to(dev), auxInput=torch.as_tensor(aux).to(dev),
                   speaker_reverberation_early_ch0=torch.as_tensor(tgt).to(dev), reference_channel=0, dataset=["bench"] * B)
        losses = {"logmae": loss.LogMAE(), "freqmse": loss.FreqMSE(target="Speaker_reverberation_early_ch0")}
        np.random.seed(0)

        def step():
            opt.zero_grad()
            ex = dict(ex0)
            out = model(ex)
            model.review(ex, out)["loss"].backward()
            opt.step()

        times = {k: [] for k in losses}
        for k, lo in losses.items():
            model.loss = lo
            for _ in range(3):
                step()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k, lo in losses.items():
                model.loss = lo
                times[k].append(timeit(step, reps))
        res = dict(name=name, what="whole eager training step", B=B, K=K, N=N, rounds=rounds, reps=reps)
        for k, v in times.items():
            res[f"{k}_step_ms"] = round(statistics.median(v), 3)
            res[f"{k}_step_min_max_ms"] = [round(min(v), 3), round(max(v), 3)]
        print(json.dumps(res), flush=True)
        lines.append(res)
        del model, opt, ex0
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="also time bench.py's whole eager step with LogMAE and with FreqMSE")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_spectral.py measures on the GPU; there is none")
    import bench                                       # the shapes are bench.py's, not copies of them
    dev = torch.device("cuda", 0)
    F = bench.FBINS
    _, wsyn = Fn.windows("hann", 1024, 256, dev)
    lines = []
    for name in ("cfg3", "cfg4"):
        w = bench.WORKLOADS[name]
        B, K, N = w["batch"], w["K"], w["N"]
        T = h.stft_frames(N)
        g = torch.Generator(device=dev).manual_seed(0)
        logit = torch.randn(B, K, T, F, device=dev, generator=g)
        obs = torch.randn(B, T, F, device=dev, generator=g, dtype=torch.complex64)
        tgt = obs[:, None] * torch.sigmoid(logit + 0.5 * torch.randn(B, K, T, F, device=dev, generator=g))
        tgt_time = torch.randn(B, K, N, device=dev, generator=g)
        gout = torch.ones(B, device=dev)

        def fused(pit=False):
            part = h.mask_specmse_fwd(logit, obs, tgt, diag_only=not pit)
            _, perm, _, _ = h.pit_assign(part, F, pit=pit, log=False, want_cost=False)
            h.mask_specmse_bwd(logit, obs, tgt, perm if pit else None, gout)

        def unfused():
            mask, est = h.maskhead_fwd(logit, obs)
            h.pit_assign(h.specmse_fwd(est, tgt, diag_only=True), F, pit=False, log=False, want_cost=False)
            dest = h.specmse_bwd(est, tgt, None, gout)
            h.maskhead_bwd(dest, None, mask, obs)

        def logmae():
            y, part = h.mask_istft_fwd(logit, obs, wsyn, N, tgt=tgt_time)
            _, sums = h.logmae_finalize(part, B, K, N)
            h.mask_istft_bwd(None, logit, obs, wsyn, loss=(y, tgt_time, sums, gout))

        runs = {"fused": fused, "fused_pit": lambda: fused(True), "unfused": unfused, "logmae": logmae}
        for fn in runs.values():                       # warm-up of every variant at this shape
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):                      # interleaved: one window of each variant per round
            for k, fn in runs.items():
                times[k].append(timeit(fn, a.reps))
        fwd_bytes = 12 * B * K * T * F + 8 * B * T * F
        nbytes = 2 * fwd_bytes + 4 * B * K * T * F
        res = dict(name=name, B=B, K=K, T=T, F=F, rounds=a.rounds, reps=a.reps, algorithmic_bytes_fwd_bwd=nbytes,
                   bound="bandwidth (HBM streaming)")
        for k, v in times.items():
            med = statistics.median(v)
            res[f"{k}_ms"] = round(med, 4)
            res[f"{k}_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
            if k != "logmae":
                res[f"{k}_share_of_8TBps"] = round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 4)
        res["fused_over_unfused"] = round(res["fused_ms"] / res["unfused_ms"], 4)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del runs, logit, obs, tgt, tgt_time
        torch.cuda.empty_cache()
    if a.step:
        lines += whole_step(bench, dev, 3, 5)
    if a.out:
        with open(a.out, "w") as f:
            for res in lines:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
