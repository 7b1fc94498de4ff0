"""WPE dereverberation at evaluation size: D = 6, taps = 10, delay = 2, 3 iterations, T = 1 878, F = 513 -- the whole
observation (pre_wpe) and a table of 8 speakers x 10 intervals (segment_wpe), against numpy on the host of the same box.
Prints one JSON line per measurement.

    python tools/bench_wpe.py [--reps 5] [--host-bins 64] [--stages] [--no-host]

--stages also runs every exported stage alone on the whole observation (HIP events around each), so that a run under
`rocprofv3 --kernel-trace --stats -- python tools/bench_wpe.py --stages --no-host` lists every kernel of the pipeline.
The host baseline is numpy with the products on BLAS (batched matmul of the weighted tilde matrix, LAPACK's solve per bin),
measured on --host-bins bins and scaled to F; `blas_threads` is what threadpoolctl reports, or null where it is not
installed (then OMP_NUM_THREADS of the environment is printed beside it)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from tssep_amd import _lib, hip_ops as H   # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(min(ts))


def wpe_numpy_blas(Y, taps, delay, iterations):
    """the definition with every product a batched matmul: Y [D, T, F] -> X [D, T, F]"""
    import test_wpe_reference as W
    Yf = np.ascontiguousarray(Y.transpose(2, 0, 1))                                   # [F, D, T]
    Yt = np.ascontiguousarray(W.tilde(Y, taps, delay).transpose(2, 0, 1))             # [F, K, T]
    YtH, YfH = Yt.conj().transpose(0, 2, 1), Yf.conj().transpose(0, 2, 1)
    X = Yf
    for _ in range(iterations):
        p = np.mean(X.real ** 2 + X.imag ** 2, axis=1)                                # [F, T]
        li = 1.0 / np.maximum(p, 1e-10 * p.max(1, keepdims=True))
        Z = Yt * li[:, None, :]
        G = np.linalg.solve(Z @ YtH, Z @ YfH)                                         # [F, K, D]
        X = Yf - G.conj().transpose(0, 2, 1) @ Yt
    return X.transpose(1, 2, 0)


def blas_threads():
    try:
        from threadpoolctl import threadpool_info
        return max((p.get("num_threads", 0) for p in threadpool_info()), default=None)
    except ImportError:
        return None


def stages(obs, taps, delay, reps):
    """every exported stage alone on the table [(0, T)], out of one workspace; HIP events around each"""
    L = _lib.lib()
    D, T, F = obs.shape
    K = taps * D
    tab, row0 = H.wpe_table([(0, T)], obs.device)
    ws = torch.empty(L.tssep_wpe_workspace_bytes(1, T, D, T, F, taps, delay) // 8 + 2, dtype=torch.float64, device="cuda")
    lam = torch.empty(T, F, dtype=torch.float64, device="cuda")
    R = torch.empty(F, K, K, 2, dtype=torch.float64, device="cuda")
    P = torch.empty(F, K, D, 2, dtype=torch.float64, device="cuda")
    G = torch.empty(K, D, F, 2, dtype=torch.float64, device="cuda")
    X = torch.empty(D, T, F, 2, dtype=torch.float64, device="cuda")
    info = torch.empty(1, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    o = p(torch.view_as_real(obs))
    calls = {
        "tssep_wpe_power": lambda: L.tssep_wpe_power(o, None, p(tab), p(row0), p(lam), p(ws), 1, T, D, T, F, None),
        "tssep_wpe_correlations": lambda: L.tssep_wpe_correlations(o, p(lam), p(tab), p(row0), p(R), p(P), p(ws), 1, T, D,
                                                                   T, F, taps, delay, 0, None),
        "tssep_wpe_solve": lambda: L.tssep_wpe_solve(p(R), p(P), p(G), p(info), 1, D, F, taps, None),
        "tssep_wpe_filter": lambda: L.tssep_wpe_filter(o, p(G), p(tab), p(row0), p(X), p(ws), 1, T, D, T, F, taps, delay,
                                                       None),
    }
    for name, call in calls.items():
        assert call() == 0, name
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            assert call() == 0, name
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        print(json.dumps({"what": "stage " + name, "ms_median": float(np.median(ms)), "ms_min": float(min(ms))}))
    assert int(info.item()) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-bins", type=int, default=64, help="bins of the numpy baseline (scaled to F)")
    ap.add_argument("--stages", action="store_true", help="also run every exported stage alone")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy baseline")
    ap.add_argument("--T", type=int, default=1878)
    ap.add_argument("--F", type=int, default=513)
    args = ap.parse_args()
    import test_wpe_reference as W
    D, taps, delay, its, T, F = 6, 10, 2, 3, args.T, args.F
    K = taps * D
    Y = W.reverberant(D, T, 8, 1)
    Y = np.tile(Y, (1, 1, (F + 7) // 8))[:, :, :F] * (1 + 0.01 * np.arange(F))[None, None, :]
    obs = torch.from_numpy(np.ascontiguousarray(Y)).cuda()
    flops = lambda n: its * n * F * 8 * (K * (K + 1) // 2 + 2 * K * D)      # noqa: E731
    med, best = timed(lambda: H.wpe(obs, None, taps, delay, its, check_singular=False), args.reps)
    print(json.dumps({"what": "wpe whole observation", "D": D, "taps": taps, "T": T, "F": F, "ms_median": med,
                      "ms_min": best, "tflops_fp64": flops(T) / med / 1e9}))
    rs = np.random.RandomState(0)
    rows = []
    for _ in range(8):
        starts = np.sort(rs.choice(np.arange(0, T - 260, 20), 10, replace=False))
        rows += [(int(s), int(min(T, s + rs.randint(80, 260)))) for s in starts]
    N = sum(e - s for s, e in rows)
    med, best = timed(lambda: H.wpe(obs, rows, taps, delay, its, check_singular=False), args.reps)
    print(json.dumps({"what": "wpe 8 x 10 segments", "rows": len(rows), "N": N, "ms_median": med, "ms_min": best,
                      "tflops_fp64": flops(N) / med / 1e9}))
    if args.stages:
        stages(obs, taps, delay, args.reps)
    if not args.no_host:
        nb = min(args.host_bins, F)
        wpe_numpy_blas(Y[:, :, :2], taps, delay, 1)
        t0 = time.perf_counter()
        Xh = wpe_numpy_blas(Y[:, :, :nb], taps, delay, its)
        host = (time.perf_counter() - t0) * 1e3 * F / nb
        Xg = H.wpe(obs, None, taps, delay, its).cpu().numpy()[:, :, :nb]
        print(json.dumps({"what": "numpy baseline on BLAS, whole observation (scaled from %d bins)" % nb, "ms": host,
                          "blas_threads": blas_threads(), "OMP_NUM_THREADS": os.environ.get("OMP_NUM_THREADS"),
                          "max_abs_diff_to_gpu": float(np.abs(Xh - Xg).max())}))


if __name__ == "__main__":
    main()
