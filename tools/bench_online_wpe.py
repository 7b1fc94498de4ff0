"""Micro-benchmark of the recursive WPE, one process:

1. hip_ops.online_wpe on a single stream, B = 1, F = 513, taps 10, delay 2, a complex64 observation (what the separator
   hands it), D = 6 (K = 60) and D = 8 (K = 80), Tc = 1 and 4 frames per call with the state carried from call to call:
   a device-event window holds CALLS calls, 3 warm-up windows, the median of 20 with min and max, per call and per frame.
   The yardstick is the 16 ms a frame lasts (shift 256 at 16 kHz).  The state's bytes (read and written once per call) go
   beside it, and their rate.
2. A whole 30-s utterance (T = 1878 frames) in one call -- what OnlineWPE does on a validation example -- beside the
   offline hip_ops.wpe with 1 and 3 iterations on the same utterance (complex128), alternating.  Nothing is gated on the
   ratio: the recursion updates one inverse per frame and bin, the offline pipeline solves one system per bin.
3. OnlineSeparator.push of one frame at production width (units 300, projs 320, K = 4 speakers, D = 6 channels) with
   OnlineMVDR alone -- the push of the commit before this one, the same launches -- and with pre_wpe=OnlineWPE(): a host
   clock around push + synchronise, alternating.

    python tools/bench_online_wpe.py [--out profiles/online_wpe_microbench.jsonl]
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

WARMUP, REPS, CALLS = 3, 20, 16
TAPS, DELAY = 10, 2


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                spread_ms=round(max(ms) - min(ms), 4))


def alternate(calls, per_window=1):
    times = {k: [] for k in calls}
    for r in range(WARMUP + REPS):
        for k, fn in calls.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(per_window):
                fn()
            e.record()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[k].append(s.elapsed_time(e) / per_window)
    return {k: stats(v) for k, v in times.items()}


def frames(B, D, T, F, seed=0, dtype=torch.complex64):
    torch.manual_seed(seed)
    Y = torch.view_as_complex(torch.randn(B, D, T, F, 2, device="cuda"))
    for t in range(1, min(T, 64)):
        Y[:, :, t] += 0.5 * Y[:, :, t - 1]
    return Y.to(dtype)


def stream(emit, D, B=1, F=513):
    K = TAPS * D
    for Tc in (1, 4):
        Y = frames(B, D, Tc, F)
        state = [h.online_wpe(frames(B, D, 16, F, seed=3), taps=TAPS, delay=DELAY)[1]]

        def call():
            state[0] = h.online_wpe(Y, state[0], taps=TAPS, delay=DELAY)[1]
        res = alternate({"online_wpe": call}, CALLS)["online_wpe"]
        state_bytes = sum(t.numel() * t.element_size() for t in state[0])
        emit(dict(what="stream", B=B, D=D, taps=TAPS, delay=DELAY, K=K, F=F, frames=Tc, Y="complex64", calls_per_window=CALLS,
                  online_wpe=res, ms_per_frame=round(res["median_ms"] / Tc, 4), frame_ms_at_shift_256_16k=16.0,
                  within_a_frame=bool(res["median_ms"] <= 16.0 * Tc), workgroups=B * F, state_mb=round(state_bytes / 1e6, 2),
                  state_in_and_out_gb_per_s=round(2 * state_bytes / (res["median_ms"] * 1e-3) / 1e9, 1),
                  info_refused=int(state[0].info.sum())))


def utterance(emit, D, F=513, T=1878):
    Y = frames(1, D, T, F, seed=1, dtype=torch.complex128)
    Y64 = Y.to(torch.complex64)
    obs = Y[0].contiguous()
    res = alternate({
        "online_wpe": lambda: h.online_wpe(Y64, taps=TAPS, delay=DELAY),
        "online_wpe_c128": lambda: h.online_wpe(Y, taps=TAPS, delay=DELAY),
        "wpe_1_iteration": lambda: h.wpe(obs, taps=TAPS, delay=DELAY, iterations=1, check_singular=False),
        "wpe_3_iterations": lambda: h.wpe(obs, taps=TAPS, delay=DELAY, iterations=3, check_singular=False),
    })
    K = TAPS * D
    flops = 513 * T * 8 * (K * K + K * (K + 1) // 2 + 2 * K * D)
    emit(dict(what="utterance", B=1, D=D, taps=TAPS, delay=DELAY, K=K, F=F, frames=T, seconds=30, **res,
              ms_per_frame=round(res["online_wpe"]["median_ms"] / T, 5),
              fp64_gflops=round(flops / (res["online_wpe"]["median_ms"] * 1e-3) / 1e9, 1),
              ratio_to_wpe_1_iteration=round(res["online_wpe_c128"]["median_ms"] / res["wpe_1_iteration"]["median_ms"], 2),
              ratio_to_wpe_3_iterations=round(res["online_wpe_c128"]["median_ms"] / res["wpe_3_iterations"]["median_ms"], 2),
              real_time_factor=round(res["online_wpe"]["median_ms"] / 30e3, 5)))


def pushes(emit, D=6, K=4):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net

    def build(enh):
        torch.manual_seed(2)
        return model.Model(
            fe=fe.ConcaternatedSTFTFeatures(fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
                                            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True),
                                            size=1024, shift=256, window="hann"),
            reader=DummyReader(),
            mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=300, projs=320, layers=3, combination="mul",
                                                aux_net_output_size=513, ts_vad=K, rnn_typ="lstm",
                                                random_speaker_order=False),
            enhancer=enh, loss=loss.LogMAE()).cuda().eval()
    aux = torch.rand(1, K, 513, device="cuda")
    seps = {"online_mvdr": build(enhancer.OnlineMVDR()).online(aux),
            "online_mvdr_pre_wpe": build(enhancer.OnlineMVDR(pre_wpe=enhancer.OnlineWPE(taps=TAPS, delay=DELAY))).online(aux)}
    torch.manual_seed(4)
    for s in seps.values():
        s.push(torch.randn(1, D, 8 * 256, device="cuda") * 0.1)          # past the stream's first frames
    x = torch.randn(1, D, 256, device="cuda") * 0.1
    ms = {k: [] for k in seps}
    for r in range(WARMUP + REPS):
        for k, s in seps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            y = s.push(x)
            torch.cuda.synchronize()
            if r >= WARMUP:
                ms[k].append((time.perf_counter() - t0) * 1e3)
        assert tuple(y.shape) == (1, K, 256)
    res = {k: stats(v) for k, v in ms.items()}
    emit(dict(what="push", B=1, K=K, D=D, frames=1, units=300, projs=320, taps=TAPS, delay=DELAY, **res,
              pre_wpe_adds_ms=round(res["online_mvdr_pre_wpe"]["median_ms"] - res["online_mvdr"]["median_ms"], 4),
              frame_ms_at_shift_256_16k=16.0, within_a_frame=bool(res["online_mvdr_pre_wpe"]["median_ms"] <= 16.0),
              gemm_precision=h.GEMM_PRECISION))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "online_wpe_microbench.jsonl"))
    ap.add_argument("--channels", type=int, nargs="+", default=[6, 8])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_online_wpe.py measures on the GPU: none found")
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
        pushes(emit)


if __name__ == "__main__":
    main()
