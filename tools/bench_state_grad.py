"""Micro-benchmark of the gradient through a carried state.  Device events, 3 warm-ups, the median of 20
with min and max (max - min: the run-to-run spread in the process), H = 300.

(a) the launch time with a null state: tssep_lstm1_bwd / tssep_gru1_bwd (all-null state arguments of the *_bwd_state entry
    points) at (768, 253) and (4, 1).  With --parent-root DIR, a built checkout of the parent commit, the same launches run
    from that tree and from this one in ALTERNATING child processes (each process one tree, two of each), and every pair row
    says whether the medians differ by more than the parent's own spread.
(b) the hand-over's cost: one RNNP layer (I = hdim = 320), forward + backward at 768 x 253 as one call against four chunks
    of 64 / 63 frames with the state kept in the graph (functional.rnnp_layer(state_grad=True)), LSTM and GRU.  A record.

    python tools/bench_state_grad.py [--parent-root DIR] [--out profiles/state_grad_microbench.jsonl]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Hh, I, HDIM = 300, 320, 320
WARMUP, REPS = 3, 20
SIZES = ((768, 253), (4, 1))


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                spread_ms=round(max(ms) - min(ms), 4))


def alternate(calls, before=None):
    """calls: {name: fn}; WARMUP + REPS rounds, every round runs each call once in turn between two device events.
    before: {name: fn} run outside the timed interval (restores what the call overwrites)."""
    import torch
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


def kernels(root):
    """(child process) the two backward launches without a state, from the tree at `root` -> one JSON row per size"""
    sys.path.insert(0, root)
    import torch
    from tssep_amd import hip_ops as h
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    for N, T in SIZES:
        torch.manual_seed(0)
        lstm, gru = torch.nn.LSTM(I, Hh, batch_first=True).cuda(), torch.nn.GRU(I, Hh, batch_first=True).cuda()
        pl, pg = h.lstm1_pack([getattr(lstm, n) for n in names], Hh, I), h.gru_pack([getattr(gru, n) for n in names], Hh, I)
        gl = torch.randn(N * T, 4 * Hh, device="cuda") * 0.5
        gg = gl.clone()
        cell = torch.empty(N, T, Hh, device="cuda")
        hl, hg = torch.zeros(N, T, Hh, device="cuda"), torch.zeros(N, T, Hh, device="cuda")
        dh = torch.randn(N, T, Hh, device="cuda") * 0.1
        h.lstm1_fwd(gl, cell, hl, Hh, pl["whh_f"], N, T, Hh)
        h.gru_fwd(gg, hg, Hh, 0, pg["whh_f"], N, T, Hh, directions=1)
        Al, Ag = gl.clone(), gg.clone()
        res = alternate({
            "lstm1_bwd": lambda: h.lstm1_bwd(gl, cell, dh, Hh, pl["whh_b"], N, T, Hh),
            "gru1_bwd": lambda: h.gru_bwd(gg, hg, dh, Hh, 0, pg["whh_b"], N, T, Hh, directions=1),
        }, before={"lstm1_bwd": lambda: (gg.copy_(Ag), gl.copy_(Al)), "gru1_bwd": lambda: (gl.copy_(Al), gg.copy_(Ag))})
        print(json.dumps(dict(N=N, T=T, **res)), flush=True)


def null_state_pairs(parent_root, emit):
    """(a): child processes, one tree each, alternating"""
    order = [("this", HERE)] if not parent_root else [("parent", parent_root), ("this", HERE)] * 2
    runs = {}
    for tag, root in order:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-kernels", root], check=True,
                             stdout=subprocess.PIPE, text=True).stdout
        for line in out.splitlines():
            row = json.loads(line)
            for k in ("lstm1_bwd", "gru1_bwd"):
                runs.setdefault((k, row["N"], row["T"]), {}).setdefault(tag, []).append(row[k])
    for (k, N, T), by in runs.items():
        row = dict(what="kernel_bwd_null_state", kernel=k, N=N, T=T, H=Hh, this=by["this"])
        if "parent" in by:
            mp = statistics.median(r["median_ms"] for r in by["parent"])
            mt = statistics.median(r["median_ms"] for r in by["this"])
            spread = max(r["spread_ms"] for r in by["parent"])
            row.update(parent=by["parent"], parent_median_ms=round(mp, 4), this_median_ms=round(mt, 4),
                       ratio_of_medians=round(mt / mp, 4), parent_spread_ms=spread,
                       differ_beyond_parent_spread=bool(abs(mt - mp) > spread))
        emit(row)


def hand_over(emit):
    """(b): one call against four chunks with an undetached state"""
    sys.path.insert(0, HERE)
    import torch
    from tssep_amd import functional as Fn, hip_ops as h
    N, T = SIZES[0]
    chunks = [64, 63, 63, 63]
    assert sum(chunks) == T
    torch.manual_seed(1)
    x, dy = torch.randn(N, T, I, device="cuda"), torch.randn(N * T, HDIM, device="cuda")
    for kind, cls in (("lstm", torch.nn.LSTM), ("gru", torch.nn.GRU)):
        rnn, lin = cls(I, Hh, batch_first=True).cuda(), torch.nn.Linear(Hh, HDIM).cuda()

        def whole():
            Fn.rnnp_layer(x.reshape(N * T, I).clone().requires_grad_(), rnn, lin, N, T, act=1).backward(dy)

        def chunked():
            xg = x.clone().requires_grad_()
            state, ys, t0 = None, [], 0
            for n in chunks:
                y, state = Fn.rnnp_layer(xg[:, t0:t0 + n].reshape(N * n, I), rnn, lin, N, n, act=1, state=state,
                                         return_state=True, state_grad=True)
                ys.append(y.view(N, n, HDIM))
                t0 += n
            torch.cat(ys, 1).reshape(N * T, HDIM).backward(dy)
        res = alternate({"whole": whole, "chunked": chunked})
        emit(dict(what="layer_fwd_bwd_hand_over", cell=kind, N=N, T=T, chunks=chunks, I=I, H=Hh, hdim=HDIM,
                  gemm_precision=h.GEMM_PRECISION, whole=res["whole"], chunked=res["chunked"],
                  ratio_of_medians=round(res["chunked"]["median_ms"] / res["whole"]["median_ms"], 4)))
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "state_grad_microbench.jsonl"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit, for (a)")
    ap.add_argument("--child-kernels", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child_kernels:
        return kernels(args.child_kernels)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(row):
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
        null_state_pairs(args.parent_root, emit)
        hand_over(emit)


if __name__ == "__main__":
    main()
