"""Micro-benchmark of the GRU route, one process, kernels alternating:

1. tssep_gru1_fwd / _bwd beside tssep_lstm1_fwd / _bwd (the one-direction streaming recurrences of the two cells) at the
   same (N, T, H): (768, 253, 300), the headline batch, and (4, 1, 300), a one-frame launch over four sequences: device events, 3 warm-ups, the
   median of 20 with min and max (the run-to-run spread in this process).  Both
   stream the same W_hh bytes per step (four rows per unit; the GRU's slot 2 is a zero block) and the GRU has fewer
   transcendentals per cell (two sigmoids and one tanh against three and two).
2. one RNNP layer of each cell through functional.rnnp_layer (I = hdim = 320): forward + backward at the same sizes, and at
   (4, 1) the one-frame forward with a carried state, without gradients -- the call an online trunk makes per layer and
   frame.  The yardstick there is the 16 ms a frame lasts at shift 256 / 16 kHz.

    python tools/bench_gru.py [--out profiles/gru_microbench.jsonl] [--sizes 768x253,4x1]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tssep_amd import functional as Fn, hip_ops as h  # noqa: E402

Hh, I, HDIM = 300, 320, 320
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


def kernels(N, T, emit):
    torch.manual_seed(0)
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    lstm, gru = torch.nn.LSTM(I, Hh, batch_first=True).cuda(), torch.nn.GRU(I, Hh, batch_first=True).cuda()
    pl, pg = h.lstm1_pack([getattr(lstm, n) for n in names], Hh, I), h.gru_pack([getattr(gru, n) for n in names], Hh, I)
    keep = torch.randn(N * T, 4 * Hh, device="cuda") * 0.5
    gl, gg = keep.clone(), keep.clone()
    cell = torch.empty(N, T, Hh, device="cuda")
    hl, hg = torch.zeros(N, T, Hh, device="cuda"), torch.zeros(N, T, Hh, device="cuda")
    dh = torch.randn(N, T, Hh, device="cuda") * 0.1
    res = alternate({
        "lstm1_fwd": lambda: h.lstm1_fwd(gl, cell, hl, Hh, pl["whh_f"], N, T, Hh),
        "gru1_fwd": lambda: h.gru_fwd(gg, hg, Hh, 0, pg["whh_f"], N, T, Hh, directions=1),
    }, before={"lstm1_fwd": lambda: (gg.copy_(keep), gl.copy_(keep)), "gru1_fwd": lambda: (gl.copy_(keep), gg.copy_(keep))})
    # backward: the activations of a forward of each kind, restored before every call (the same copies in front of both)
    gl.copy_(keep)
    gg.copy_(keep)
    h.lstm1_fwd(gl, cell, hl, Hh, pl["whh_f"], N, T, Hh)
    h.gru_fwd(gg, hg, Hh, 0, pg["whh_f"], N, T, Hh, directions=1)
    Al, Ag = gl.clone(), gg.clone()
    res.update(alternate({
        "lstm1_bwd": lambda: h.lstm1_bwd(gl, cell, dh, Hh, pl["whh_b"], N, T, Hh),
        "gru1_bwd": lambda: h.gru_bwd(gg, hg, dh, Hh, 0, pg["whh_b"], N, T, Hh, directions=1),
    }, before={"lstm1_bwd": lambda: (gg.copy_(Ag), gl.copy_(Al)), "gru1_bwd": lambda: (gl.copy_(Al), gg.copy_(Ag))}))
    for d in ("fwd", "bwd"):
        a, b = res[f"gru1_{d}"], res[f"lstm1_{d}"]
        emit(dict(what=f"kernel_{d}", N=N, T=T, H=Hh, gru1=a, lstm1=b, ratio_of_medians=round(a["median_ms"] / b["median_ms"], 4),
                  not_slower_beyond_spread=bool(a["median_ms"] <= b["median_ms"] + b["spread_ms"])))


def layers(N, T, emit):
    """one RNNP layer on each cell through functional.rnnp_layer: forward + backward, and (N <= 8) the stateful one-chunk
    forward without gradients that an online trunk would call"""
    torch.manual_seed(1)
    x, dy = torch.randn(N * T, I, device="cuda"), torch.randn(N * T, HDIM, device="cuda")
    mods = {"gru": (torch.nn.GRU(I, Hh, batch_first=True).cuda(), torch.nn.Linear(Hh, HDIM).cuda()),
            "lstm": (torch.nn.LSTM(I, Hh, batch_first=True).cuda(), torch.nn.Linear(Hh, HDIM).cuda())}

    def step(kind):
        rnn, lin = mods[kind]
        Fn.rnnp_layer(x.clone().requires_grad_(), rnn, lin, N, T, act=1).backward(dy)
    res = alternate({k: (lambda k=k: step(k)) for k in mods})
    emit(dict(what="layer_fwd_bwd", N=N, T=T, I=I, H=Hh, hdim=HDIM, gemm_precision=h.GEMM_PRECISION, gru=res["gru"], lstm=res["lstm"],
              ratio_of_medians=round(res["gru"]["median_ms"] / res["lstm"]["median_ms"], 4)))
    if N > 8:
        return
    state = {}
    with torch.no_grad():
        for kind, (rnn, lin) in mods.items():
            state[kind] = Fn.rnnp_layer(x, rnn, lin, N, T, act=1, return_state=True)[1]

        def chunk(kind):
            rnn, lin = mods[kind]
            state[kind] = Fn.rnnp_layer(x, rnn, lin, N, T, act=1, state=state[kind], return_state=True)[1]
        res = alternate({k: (lambda k=k: chunk(k)) for k in mods})
    emit(dict(what="layer_chunk_with_state", N=N, T=T, I=I, H=Hh, hdim=HDIM, gemm_precision=h.GEMM_PRECISION, gru=res["gru"],
              lstm=res["lstm"], ratio_of_medians=round(res["gru"]["median_ms"] / res["lstm"]["median_ms"], 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "gru_microbench.jsonl"))
    ap.add_argument("--sizes", default="768x253,4x1")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(row):
            row = dict(device=torch.cuda.get_device_name(0), **row)
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
        for size in [s for s in args.sizes.split(",") if s]:
            N, T = (int(v) for v in size.split("x"))
            kernels(N, T, emit)
            torch.cuda.empty_cache()
            layers(N, T, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
