"""Microbenchmark of the mask-based MVDR beamformer (TorchBF) on one MI355X:
HIP-event time of the whole pipeline and of each stage vs the algorithmic HBM bytes, and the CPU
oracle beside it on a frequency slice.  One JSON line per configuration.  The last line is the segment-wise
pipeline (ClassicBF_np, hip_ops.segment_mvdr) against the way to the same output without it: a loop of
hip_ops.mvdr_souden over time slices with host-built two-plane masks (--only-segments: that line alone)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tssep_amd import _lib, hip_ops as H  # noqa: E402

HBM_PEAK = 8000.0
F64_VECTOR_PEAK = 78.6        # TFLOP/s: 256 CUs x 4 SIMDs x 16 lanes x 2 flop x 2.4 GHz


def ev_ms(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def wall_ms(fn, iters):
    """median wall-clock time of fn (which may synchronise inside), device idle at both ends"""
    fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def segmented(args, L):
    """8 speakers x 30 s x 6 channels, F = 513, a seeded diarization of about 10 intervals per speaker."""
    K, D, T, F = 8, 6, 1878, 513
    g = torch.Generator().manual_seed(0)
    Y = torch.randn(D, T, F, dtype=torch.complex128, generator=g).cuda()
    m = torch.rand(K, 1, T, F, generator=g).cuda()
    rs = np.random.RandomState(0)
    segments = []
    for k in range(K):
        t = int(rs.randint(0, 40))
        for _ in range(10):
            n = int(rs.randint(60, 170))
            if t + n > T:
                break
            segments.append((k, t, t + n))
            t += n + int(rs.randint(5, 60))
    S = len(segments)
    table = H.segment_table(segments, "cuda")

    def one_call():
        return H.segment_mvdr(m, Y, table, distortion_eps=1e-4, psd_real=False)

    def loop():
        # SumCrossTalker with torch ops, then one whole-utterance beamformer per slice (one .item() each)
        dist = torch.stack([torch.clamp(sum(m[j, 0] for j in range(K) if j != k), min=1e-4) for k in range(K)])
        out = torch.zeros(K, T, F, dtype=torch.complex128, device="cuda")
        for k, s, e in segments:
            two = torch.stack([m[k, 0, s:e], dist[k, s:e]])[None, None]
            out[k, s:e] = H.mvdr_souden(two, Y[None, :, s:e], 0)[0, 0]
        return out

    a, b = one_call(), loop()
    err = float((a - b).abs().max() / b.abs().max())
    t_new, t_loop = wall_ms(one_call, args.iters), wall_ms(loop, max(3, args.iters // 4))
    # library launches only (kernels + the info memset); the loop's torch ops come on top of its count
    per_slice = [3 + 1 + (L.tssep_mvdr_partial_bytes(1, 1, D, e - s, F) > 8 * 2 * D * D * F) for _, s, e in segments]
    print(json.dumps({"config": "segment-wise: 8 spk, 6 ch, 30 s", "K": K, "D": D, "T": T, "F": F, "segments": S,
                      "frames_in_segments": int(sum(e - s for _, s, e in segments)),
                      "segment_mvdr_ms": round(t_new, 4), "sliced_loop_ms": round(t_loop, 4),
                      "loop_over_segment_mvdr": round(t_loop / t_new, 2), "segment_mvdr_launches": 6,
                      "sliced_loop_library_launches": int(sum(per_slice)), "segment_mvdr_host_syncs": 1,
                      "sliced_loop_host_syncs": S, "max_rel_diff": err,
                      "workspace_bytes": L.tssep_mvdr_segments_workspace_bytes(K, S, D, T, F)}), flush=True)
    assert t_new <= t_loop, "segment_mvdr is slower than the loop it replaces"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--only-segments", action="store_true")
    args = ap.parse_args()
    L = _lib.lib()
    if args.only_segments:
        return segmented(args, L)
    for name, (B, K, M, D, T, F) in {
            "cfg3 eval: 4 spk, 6 ch, 4 s": (1, 4, 2, 6, 253, 513),
            "cfg5 eval: 8 spk, 6 ch, 30 s": (1, 8, 2, 6, 1878, 513),
            "cfg5 eval, target mask only": (1, 8, 1, 6, 1878, 513),
            "8 x cfg5 eval batched": (8, 8, 2, 6, 1878, 513)}.items():
        g = torch.Generator().manual_seed(0)
        Y = torch.randn(B, D, T, F, dtype=torch.complex128, generator=g).cuda()
        m = torch.rand(B, K, M, T, F, generator=g).cuda()
        total = ev_ms(lambda: H.mvdr_souden(m, Y, 0, check_singular=False), args.iters)
        nb = L.tssep_mvdr_partial_bytes(B, K, D, T, F)
        part = torch.empty(nb // 8, dtype=torch.float64, device="cuda")
        w = torch.empty(B * K * D * F * 2, dtype=torch.float64, device="cuda")
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        enh = torch.empty(B, K, T, F, 2, dtype=torch.float64, device="cuda")
        Yr = torch.view_as_real(Y)
        st = torch.cuda.current_stream().cuda_stream
        t_psd = ev_ms(lambda: L.tssep_mvdr_psd(Yr.data_ptr(), m.data_ptr(), 0, part.data_ptr(),
                                               B, K, M, D, T, F, st), args.iters)
        t_w = ev_ms(lambda: L.tssep_mvdr_weights(part.data_ptr(), w.data_ptr(), info.data_ptr(), B, K,
                                                 D, T, F, 0, 1e-300, st), args.iters)
        t_app = ev_ms(lambda: L.tssep_mvdr_apply(Yr.data_ptr(), w.data_ptr(), m.data_ptr(), 0,
                                                 enh.data_ptr(), B, K, M, D, T, F, 0, 0.0, st),
                      args.iters)
        b_psd = B * T * F * (16 * D + 4 * K * M) + nb
        b_app = B * T * F * (16 * D + 16 * K)
        alg = B * T * F * (32 * D + 4 * K * M + 16 * K)
        row = {"config": name, "B": B, "K": K, "M": M, "D": D, "T": T, "F": F, "dtype": "c128",
               "total_ms": round(total, 4), "frames_per_s": round(B * T / total * 1e3, 1),
               "algorithmic_bytes": alg, "achieved_GBps": round(alg / total / 1e6, 1),
               "frac_of_hbm_peak": round(alg / total / 1e6 / HBM_PEAK, 4),
               "psd_ms": round(t_psd, 4), "psd_GBps": round(b_psd / t_psd / 1e6, 1),
               # statistics pass: 7 D^2 fp64 flop per (frame, bin, speaker) -- pair products once,
               # weighted into the target and the interference accumulators
               "psd_f64_tflops": round(B * T * F * K * 7 * D * D / t_psd / 1e9, 2),
               "psd_frac_of_f64_vector_peak": round(B * T * F * K * 7 * D * D / t_psd / 1e9 / F64_VECTOR_PEAK, 4),
               "weights_ms": round(t_w, 4), "apply_ms": round(t_app, 4),
               "apply_GBps": round(b_app / t_app / 1e6, 1),
               "apply_frac_of_hbm_peak": round(b_app / t_app / 1e6 / HBM_PEAK, 4),
               "psd_partial_bytes": nb}
        if not args.no_cpu and B == 1:
            from oracle import enhancer as oenh          # checker / CPU baseline only
            fs = 16
            mc, Yc = m[..., :fs].cpu().numpy(), Y[..., :fs].cpu().numpy()
            t0 = time.perf_counter()
            want = oenh.torch_bf(mc, Yc, 0)
            dt = time.perf_counter() - t0
            got = H.mvdr_souden(m, Y, 0)[..., :fs].cpu().numpy()
            row["cpu_oracle_frames_per_s"] = round(B * T / (dt * F / fs), 1)
            row["cpu_sample"] = f"{fs} of {F} bins, numpy complex128, scaled to {F}"
            row["max_rel_err_vs_oracle"] = float(np.abs(got - want).max() / np.abs(want).max())
        print(json.dumps(row), flush=True)
    segmented(args, L)


if __name__ == "__main__":
    main()
