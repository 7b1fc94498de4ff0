"""Micro-benchmark of the online path, one process, kernels alternating:

1. tssep_feat_causal_fwd beside the unchanged tssep_feat_fwd('tf') at (B, T, F, n_mels, n_mfcc) = (768, 253, 513, 40, 40),
   the training size: device events, 3 warm-ups, the median of 20 with min and max.  The causal call runs one more launch
   (the scan of the per-frame maxima); it should not be slower than tssep_feat_fwd by more than that kernel's own spread
   plus the scan.  The scan's own duration comes from a kernel trace of `--feat-only` (feat_scan_kernel in the statistics
   of `rocprofv3 --kernel-trace --stats -- python tools/bench_online.py --feat-only`); pass it with --scan-ms to have the
   condition evaluated in the row.
2. OnlineSeparator.push of 1, 8 and 64 frames at production width (idim 553, odim 513, units 300, projs 320, three post-net
   layers, B = 1, K = 4) beside MaskEstimator_v2.forward_chunk alone on the same frames: the host clock around a
   synchronise, state carried from call to call.  The difference is the cost of the two ends (streaming STFT + causal
   features in front, the fused mask head + streaming inverse STFT behind).  The yardstick is the 16 ms a frame lasts.

    python tools/bench_online.py [--out profiles/online_microbench.jsonl] [--feat-only] [--scan-ms X]
"""
import argparse
import json
import os
import statistics
import sys
import time

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


def features(emit, scan_ms=None, B=768, T=253, F=513):
    from tssep_amd.train import feature_extractor as fe
    torch.manual_seed(0)
    mf = fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40).cuda()
    X = torch.view_as_complex(torch.randn(B, T, F, 2, device="cuda")) * (10 ** (-3 * torch.rand(B, T, 1, device="cuda")))
    # (both wrappers allocate output and workspace per call, as the step does: the same in both intervals)
    res = alternate({
        "feat_fwd_tf": lambda: h.feat_fwd(X, mf.fb, mf.dct_mat, 40, 80.0, "tf"),
        "feat_causal_fwd": lambda: h.feat_causal_fwd(X, mf.fb, mf.dct_mat, 40, 80.0),
    })
    a, b = res["feat_causal_fwd"], res["feat_fwd_tf"]
    row = dict(what="features", B=B, T=T, F=F, n_mels=40, n_mfcc=40, feat_causal_fwd=a, feat_fwd_tf=b,
               difference_of_medians_ms=round(a["median_ms"] - b["median_ms"], 4), launches=dict(feat_fwd=3, feat_causal_fwd=4))
    if scan_ms is not None:
        row.update(scan_ms=scan_ms, condition="median(causal) <= median(feat_fwd) + spread(feat_fwd) + scan",
                   condition_met=bool(a["median_ms"] <= b["median_ms"] + b["spread_ms"] + scan_ms))
    emit(row)


def pushes(emit):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net
    torch.manual_seed(2)
    m = model.Model(
        fe=fe.ConcaternatedSTFTFeatures(fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
                                        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True),
                                        size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=300, projs=320, layers=3, combination="mul",
                                            aux_net_output_size=513, ts_vad=4, rnn_typ="lstm", random_speaker_order=False),
        enhancer=enhancer.Masking(), loss=loss.LogMAE()).cuda().eval()
    me = m.mask_estimator
    aux = torch.rand(1, 4, 513, device="cuda")
    for Tc in (1, 8, 64):
        x = torch.randn(1, Tc * 256, device="cuda") * 0.1
        xs = torch.randn(1, Tc, 553, device="cuda")
        sep = m.online(aux)
        sep.push(torch.randn(1, 4 * 256, device="cuda") * 0.1)        # past the stream's first three frames
        _, state = me.forward_chunk(xs, aux)
        calls, real = [0], h.check

        def counting(status, what):
            calls[0] += 1
            return real(status, what)
        h.check = counting
        try:
            sep.push(x)
        finally:
            h.check = real
        ms = {"push": [], "forward_chunk": []}
        for r in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = sep.push(x)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _, state = me.forward_chunk(xs, None, state)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if r >= WARMUP:
                ms["push"].append((t1 - t0) * 1e3)
                ms["forward_chunk"].append((t2 - t1) * 1e3)
        assert tuple(y.shape) == (1, 4, Tc * 256)
        p, f = stats(ms["push"]), stats(ms["forward_chunk"])
        emit(dict(what="push", B=1, K=4, frames=Tc, units=300, projs=320, push=p, forward_chunk=f,
                  two_ends_ms=round(p["median_ms"] - f["median_ms"], 4), ms_per_frame=round(p["median_ms"] / Tc, 4),
                  frame_ms_at_shift_256_16k=16.0, within_a_frame=bool(p["median_ms"] <= 16.0 * Tc),
                  entry_point_calls_per_push=calls[0], launches_of_the_two_ends=dict(stft_stream=2, feat_causal=4, mask_istft_stream=1),
                  gemm_precision=h.GEMM_PRECISION))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "online_microbench.jsonl"))
    ap.add_argument("--feat-only", action="store_true")
    ap.add_argument("--scan-ms", type=float, default=None)
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(row):
            row = dict(device=torch.cuda.get_device_name(0), **row)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
        features(emit, args.scan_ms)
        if not args.feat_only:
            torch.cuda.empty_cache()
            pushes(emit)


if __name__ == "__main__":
    main()
