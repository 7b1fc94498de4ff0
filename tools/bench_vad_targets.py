"""Micro-benchmark (GPU box): the VAD losses' targets built on the device, at the headline shape
(768 utterances x 4 speakers x 64 000 samples) and at the 8-speaker x 30 s shape.

(a) the magnitude target: the MATERIALISED chain stft_fwd -> framemag -> vad_from_mag (the spectrum [rows, T, 513]
    complex64 is written and read back once, as the reference's `fe.stft` + `prepare_target` do) against the FUSED chain
    stft_framemag -> vad_from_mag (the frame kernel sums the magnitudes of the bins it formed).  One process, warmed up,
    HIP events around `reps` launches, the two variants alternating per round; reported per chain: the median time, the
    algorithmic bytes, their share of 8 TB/s, and the peak of torch's allocator above the resident input.
(b) the frame activity `Vad` from a device-resident sample activity `vad`: the host route of util.utils.stft_vad
    (a synchronising device-to-host copy, numpy over B K N samples, the result copied back) against the gather kernel
    (util.utils.stft_vad_device); wall time per call including the synchronisation.

    python tools/bench_vad_targets.py [--rounds 7] [--reps 20] [--out FILE.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tssep_amd import functional as Fn, hip_ops as h  # noqa: E402
from tssep_amd.util import utils  # noqa: E402

PEAK_BPS = 8e12
THR = 0.05


def timeit(fn, reps):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def host_stft_vad(vad, window_length, shift, fading):
    """util.utils.stft_vad on a device tensor: copy to the host, numpy, copy back."""
    return utils.stft_vad(vad, window_length, shift, fading)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vad_targets.py measures on the GPU; there is none")
    dev = torch.device("cuda", 0)
    size, shift, F = 1024, 256, 513
    w, _ = Fn.windows("hann", size, shift, dev, size)
    lines = []
    for name, B, K, N in (("headline", 768, 4, 64000), ("8spk_30s", 48, 8, 480000)):
        rows = B * K
        T = h.stft_frames(N, size, shift)
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(rows, N, device=dev, generator=g)
        x *= (torch.rand(rows, -(-N // 4000), device=dev, generator=g) < 0.5).repeat_interleave(4000, dim=1)[:, :N] * 0.999 + 1e-3

        def materialised():
            return h.vad_from_mag(h.framemag(h.stft_fwd(x, w, size, shift, True, T=T)), THR)

        def fused():
            return h.vad_from_mag(h.stft_framemag(x, w, size, shift, True, T=T), THR)

        va, vb = materialised(), fused()
        torch.cuda.synchronize()
        differ = float((va != vb).float().mean())
        del va, vb
        runs = {"materialised": materialised, "fused": fused}
        for fn in runs.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(a.rounds):                      # alternating: one window of each variant per round
            for k, fn in runs.items():
                times[k].append(timeit(fn, a.reps))
        frames = rows * T
        nbytes = {"materialised": 4 * rows * N + 2 * 8 * frames * F + 4 * 4 * frames,      # x; X written and read; a w + r, vad
                  "fused": 4 * rows * N + 4 * 4 * frames}
        res = dict(bench="magnitude_target", name=name, B=B, K=K, N=N, T=T, rounds=a.rounds, reps=a.reps,
                   decisions_differing=differ)
        for k, v in times.items():
            med = statistics.median(v)
            res[f"{k}_ms"] = round(med, 4)
            res[f"{k}_min_max_ms"] = [round(min(v), 4), round(max(v), 4)]
            res[f"{k}_bytes"] = nbytes[k]
            res[f"{k}_share_of_8TBps"] = round(nbytes[k] / (med * 1e-3) / PEAK_BPS, 4)
            res[f"{k}_peak_bytes"] = peak_above(runs[k])
        res["fused_over_materialised"] = round(res["fused_ms"] / res["materialised_ms"], 4)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del runs, x
        torch.cuda.empty_cache()

        # (b) Vad from a device-resident vad
        vad = (torch.rand(B, K, -(-N // 4000), device=dev, generator=g) < 0.5).repeat_interleave(4000, dim=-1)[..., :N].contiguous()
        want = host_stft_vad(vad, size, shift, True)
        got = utils.stft_vad_device(vad, size, shift, True)
        torch.cuda.synchronize()
        assert torch.equal(want, got)
        wall = {"host": [], "gather": []}
        for _ in range(a.host_rounds):
            for k, fn, reps in (("host", lambda: host_stft_vad(vad, size, shift, True), 1),
                                ("gather", lambda: utils.stft_vad_device(vad, size, shift, True), a.reps)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                wall[k].append((time.perf_counter() - t0) / reps * 1e3)
        gather_dev = statistics.median(timeit(lambda: utils.stft_vad_device(vad, size, shift, True), a.reps) for _ in range(a.rounds))
        res = dict(bench="vad_frames", name=name, B=B, K=K, N=N, T=T,
                   host_wall_ms=round(statistics.median(wall["host"]), 3),
                   gather_wall_ms=round(statistics.median(wall["gather"]), 4), gather_device_ms=round(gather_dev, 4),
                   d2h_bytes=int(np.prod(vad.shape)), gather_bytes=5 * rows * T)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del vad, want, got
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
