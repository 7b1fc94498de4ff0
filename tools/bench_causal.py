"""Micro-benchmark of the causal route, one process, kernels alternating:

1. tssep_lstm1_fwd / _bwd (one direction of time) beside the unchanged streaming tssep_blstm_fwd / _bwd (two directions)
   at (N, T, H) = (8 | 32 | 768 | 3072, 253, 300): device events, 3 warm-ups, the median of 20 with min and max (the
   run-to-run spread in this process).  A one-direction launch does the per-workgroup work of the two-direction one with
   half the workgroups: it must not be slower than the two-direction launch beyond that launch's own spread.
2. one causal RNNP layer (functional.rnnp_layer, forward + backward, I = hdim = 320) beside the BLSTM layer on the policy's
   W-stationary recurrences at 768 sequences of 253 frames (the headline batch).
3. MaskEstimator_v2.forward_chunk at production width (idim 553, odim 513, units 300, projs 320, three post-net layers),
   B = 1, K = 4, chunks of 1, 8 and 64 frames: the host clock around a synchronise, state carried from call to call.
   The yardstick is the 16 ms a frame lasts at shift 256 / 16 kHz.

    python tools/bench_causal.py [--out profiles/causal_microbench.jsonl] [--sizes 8,32,768,3072]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tssep_amd import functional as Fn, hip_ops as h  # noqa: E402

T, Hh, I, HDIM = 253, 300, 320, 320
WARMUP, REPS = 3, 20


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                spread_ms=round(max(ms) - min(ms), 4))


def alternate(calls, before=None):
    """calls: {name: fn}; WARMUP + REPS rounds, every round runs each call once in turn between two device events.
    before: {name: fn} run outside the timed interval (restores what the call overwrites)."""
    times = {k: [] for k in calls}
    for r in range(WARMUP + REPS):
        for k, fn in calls.items():
            if before and k in before:
                before[k]()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[k].append(s.elapsed_time(e))
    return {k: stats(v) for k, v in times.items()}


def kernels(N, emit):
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(I, Hh, bidirectional=True, batch_first=True).cuda()
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    two = h.lstm_pack([getattr(lstm, n) for n in names] + [getattr(lstm, n + "_reverse") for n in names], Hh, I)
    one = h.lstm1_pack([getattr(lstm, n) for n in names], Hh, I)
    g2 = torch.randn(N * T, 8 * Hh, device="cuda") * 0.5
    keep = g2.clone()
    cell2 = torch.empty(N, T, 2, Hh, device="cuda")
    h2 = torch.zeros(N, T, 2 * Hh, device="cuda")
    dh2 = torch.randn(N, T, 2 * Hh, device="cuda") * 0.1
    # the one-direction launch works in the first half of the same buffers (3 072 sequences: 7.5 GB of gates once, not twice)
    g1, cell1 = g2.view(-1)[:N * T * 4 * Hh], cell2.view(-1)[:N * T * Hh]
    h1, dh1 = h2.view(-1)[:N * T * Hh], dh2.view(-1)[:N * T * Hh]
    res = alternate({
        "blstm_fwd": lambda: h.blstm_fwd(g2, cell2, h2, 2 * Hh, Hh, two["whh_f"], N, T, Hh),
        "lstm1_fwd": lambda: h.lstm1_fwd(g1, cell1, h1, Hh, one["whh_f"], N, T, Hh),
    }, before={"blstm_fwd": lambda: g2.copy_(keep), "lstm1_fwd": lambda: g2.copy_(keep)})
    # backward: activations and cell states of a forward of each kind, restored before every call
    g2.copy_(keep)
    h.lstm1_fwd(g1, cell1, h1, Hh, one["whh_f"], N, T, Hh)
    A1, C1 = g1.clone(), cell1.clone()
    g2.copy_(keep)
    h.blstm_fwd(g2, cell2, h2, 2 * Hh, Hh, two["whh_f"], N, T, Hh)
    A2, C2 = keep.copy_(g2), cell2.clone()      # (the pre-activations are not needed again: their buffer keeps the activations)

    def put2():
        g2.copy_(A2)
        cell2.copy_(C2)

    def put1():
        g1.copy_(A1)
        cell1.copy_(C1)
    res.update(alternate({
        "blstm_bwd": lambda: h.blstm_bwd(g2, cell2, dh2, 2 * Hh, Hh, two["whh_b"], N, T, Hh),
        "lstm1_bwd": lambda: h.lstm1_bwd(g1, cell1, dh1, Hh, one["whh_b"], N, T, Hh),
    }, before={"blstm_bwd": lambda: (put1(), put2()), "lstm1_bwd": lambda: (put2(), put1())}))      # (the same copies in front of both)
    for d in ("fwd", "bwd"):
        a, b = res[f"lstm1_{d}"], res[f"blstm_{d}"]
        emit(dict(what=f"kernel_{d}", N=N, T=T, H=Hh, lstm1=a, blstm_stream=b,
                  ratio_of_medians=round(a["median_ms"] / b["median_ms"], 4),
                  not_slower_beyond_spread=bool(a["median_ms"] <= b["median_ms"] + b["spread_ms"])))


def layers(N, emit):
    torch.manual_seed(1)
    x = torch.randn(N * T, I, device="cuda")
    dy = torch.randn(N * T, HDIM, device="cuda")
    mods = {"lstm": (torch.nn.LSTM(I, Hh, batch_first=True).cuda(), torch.nn.Linear(Hh, HDIM).cuda()),
            "blstm": (torch.nn.LSTM(I, Hh, bidirectional=True, batch_first=True).cuda(), torch.nn.Linear(2 * Hh, HDIM).cuda())}
    log = h.RECURRENCE_LOG = []

    def step(kind):
        lstm, lin = mods[kind]
        xg = x.clone().requires_grad_()
        Fn.rnnp_layer(xg, lstm, lin, N, T, act=1).backward(dy)
    try:
        res = alternate({k: (lambda k=k: step(k)) for k in mods})
    finally:
        h.RECURRENCE_LOG = None
    h.check_cluster_errors()
    kernels_seen = sorted({f"{e['kernel']}/{e['direction']}" for e in log})
    emit(dict(what="layer_fwd_bwd", N=N, T=T, I=I, H=Hh, hdim=HDIM, gemm_precision=h.GEMM_PRECISION, causal=res["lstm"],
              blstm_policy=res["blstm"], recurrences=kernels_seen,
              ratio_of_medians=round(res["lstm"]["median_ms"] / res["blstm"]["median_ms"], 4)))


def chunks(emit):
    from tssep_amd.train.net import MaskEstimator_v2
    torch.manual_seed(2)
    me = MaskEstimator_v2(idim=553, odim=513, units=300, projs=320, layers=3, combination="mul", aux_net_output_size=513,
                          ts_vad=4, rnn_typ="lstm", random_speaker_order=False).cuda().eval()
    aux = torch.rand(1, 4, 513, device="cuda")
    for Tc in (1, 8, 64):
        xs = torch.randn(1, Tc, 553, device="cuda")
        _, state = me.forward_chunk(xs, aux)
        ms = []
        for r in range(WARMUP + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, state = me.forward_chunk(xs, None, state)
            torch.cuda.synchronize()
            if r >= WARMUP:
                ms.append((time.perf_counter() - t0) * 1e3)
        emit(dict(what="forward_chunk", B=1, K=4, frames=Tc, units=300, projs=320, idim=553, odim=513, host_clock=stats(ms),
                  ms_per_frame=round(statistics.median(ms) / Tc, 4), frame_ms_at_shift_256_16k=16.0,
                  gemm_precision=h.GEMM_PRECISION))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "causal_microbench.jsonl"))
    ap.add_argument("--sizes", default="8,32,768,3072")
    ap.add_argument("--layer-sizes", default="768")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(row):
            row = dict(device=torch.cuda.get_device_name(0), **row)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
        for N in [int(s) for s in args.sizes.split(",") if s]:
            kernels(N, emit)
            torch.cuda.empty_cache()
        for N in [int(s) for s in args.layer_sizes.split(",") if s]:
            layers(N, emit)
            torch.cuda.empty_cache()
        chunks(emit)


if __name__ == "__main__":
    main()
