"""Micro-benchmark of the spectral feature kernels (csrc/specfeat.hip).  Section 4.20's protocol: one
process, the calls of a pair alternating, device events, 3 warm-ups, the median of 20 with min and max (max - min: the
run-to-run spread in the process), one JSON row per pair.

At (B, T, F) = (768, 253, 513), the C entry points on buffers allocated once (no allocation inside the timed region):
  kinds 0, 1 and 2 of tssep_specfeat_fwd, each against tssep_feat_fwd(n_mfcc = 0, stat_axis 0) -- the existing log1p-only
      call: the same bytes in and out, two passes (three launches);
  tssep_specfeat_causal_fwd against tssep_feat_causal_fwd(n_mfcc = 0).
At (4, 1, 513), one frame of a stream: every one of the above once more.

    python tools/bench_specfeat.py [--out profiles/specfeat_microbench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS = 3, 20
SIZES = ((768, 253, 513), (4, 1, 513))


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                spread_ms=round(max(ms) - min(ms), 4))


def alternate(calls):
    """calls: {name: fn}; WARMUP + REPS rounds, every round runs each call once in turn between two device events."""
    import torch
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "specfeat_microbench.jsonl"))
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import torch
    from tssep_amd import _lib, hip_ops as h
    L, p = _lib.lib(), h._p
    dev = torch.device("cuda")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(row):
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
        for B, T, F in SIZES:
            torch.manual_seed(T)
            X = torch.view_as_real(torch.view_as_complex(torch.randn(B, T, F, 2, device=dev)).contiguous())
            ld = h.round_up(F, 4)
            out = torch.zeros(B, T, ld, device=dev)
            ws_feat = torch.empty(int(L.tssep_feat_workspace_bytes(B, T, 1, F, 0)) // 4 + 4, device=dev)
            ws_fc = torch.empty(int(L.tssep_feat_causal_workspace_bytes(B, T, 0, F)) // 4 + 4, device=dev)
            ws_mvn = torch.empty(int(L.tssep_specfeat_workspace_bytes(B, T, F, 2)) // 8 + 1, device=dev, dtype=torch.float64)
            st32_in, st32_out = torch.zeros(B, 2, device=dev), torch.zeros(B, 2, device=dev)
            st_in, st_out = torch.zeros(B, F + 1, device=dev, dtype=torch.float64), torch.zeros(B, F + 1, device=dev, dtype=torch.float64)
            s = h._stream()

            def feat():
                assert L.tssep_feat_fwd(p(X), B, T, F, None, None, 0, 0, 80.0, 0, p(out), ld, p(ws_feat), s) == 0

            def kind(k):
                def run():
                    assert L.tssep_specfeat_fwd(p(X), B, T, F, k, p(out), ld, p(ws_mvn), s) == 0
                return run

            def feat_causal():
                assert L.tssep_feat_causal_fwd(p(X), B, T, F, None, None, 0, 0, 80.0, p(st32_in), p(st32_out), p(out), ld,
                                               p(ws_fc), s) == 0

            def causal():
                assert L.tssep_specfeat_causal_fwd(p(X), B, T, F, 0.999, p(st_in), p(st_out), p(out), ld, s) == 0

            gb = B * T * F * 12 / 1e9
            for k in (0, 1, 2):
                res = alternate({"specfeat": kind(k), "feat_fwd": feat})
                a, b = res["specfeat"], res["feat_fwd"]
                emit(dict(what=f"specfeat_fwd kind {k}", against="feat_fwd(n_mfcc=0, stat_axis=0)", B=B, T=T, F=F, **res,
                          ratio=round(a["median_ms"] / b["median_ms"], 4),
                          within_feat_plus_its_spread=bool(a["median_ms"] <= b["median_ms"] + b["spread_ms"]),
                          specfeat_gb_per_s=round(gb * (1 if k < 2 else 5 / 3) / (a["median_ms"] * 1e-3), 1)))
            res = alternate({"specfeat": causal, "feat_causal_fwd": feat_causal})
            a, b = res["specfeat"], res["feat_causal_fwd"]
            emit(dict(what="specfeat_causal_fwd", against="feat_causal_fwd(n_mfcc=0)", B=B, T=T, F=F, forgetting=0.999, **res,
                      ratio=round(a["median_ms"] / b["median_ms"], 4),
                      within_feat_plus_its_spread=bool(a["median_ms"] <= b["median_ms"] + b["spread_ms"]),
                      specfeat_gb_per_s=round(gb / (a["median_ms"] * 1e-3), 1)))
            del X, out, ws_feat, ws_fc, ws_mvn
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
