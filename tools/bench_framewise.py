"""Micro-benchmark (GPU box): the conditioning kernels for frame-wise speaker embeddings (`tssep_cond_mul_t_fwd / _bwd`,
`tssep_cond_cat_t_fwd`, `tssep_cond_mul_aux_t_bwd`, `tssep_cond_cat_aux_t_bwd`) at aux_stride 1 and 16, beside their
utterance-level neighbours (`tssep_cond_mul_fwd / _bwd`, `tssep_cond_cat_fwd`, `tssep_cond_*_aux_bwd`) at the same B, K, T, F
and a device-to-device copy -- the shape of tools/bench_auxnet.py: B = 768, K = 8, trials = 2, T = 253, F = 513 (E = 100 for
cat).  Interleaved in one process, HIP events, median of the rounds with their spread; every launch is reported with its
algorithmic HBM bytes (include/tssep_hip.h) and the fraction of the 6.29 TB/s a float4 copy reaches (MI355X).
d(pre) of cat does not read the embedding (`tssep_cond_cat_bwd` serves both), so it is not timed twice.  The kernels are
timed on aux rows that are already 16-byte addressable; the padded copy `hip_ops.cond_fwd` makes of an aux whose width is no
multiple of 4 (F = 513) is reported as `pad_aux*`, an entry of its own (read + write of aux).

    python tools/bench_framewise.py [--rounds 7] [--reps 5] [--batch 768] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from tssep_amd import hip_ops as h  # noqa: E402

HBM_COPY_TB_S = 6.29
STRIDES = (1, 16)


def timeit(fn, reps):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def _report(shape, calls, a):
    times = {k: [] for k in calls}
    for fn, _ in calls.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, (fn, _) in calls.items():
            times[k].append(timeit(fn, a.reps))
    res = dict(part="framewise_cond", rounds=a.rounds, reps=a.reps, **shape)
    for k, (_, moved) in calls.items():
        ms = statistics.median(times[k])
        rate = moved / ms / 1e9
        res[k] = dict(ms=round(ms, 4), min_ms=round(min(times[k]), 4), max_ms=round(max(times[k]), 4), bytes=moved,
                      tb_per_s=round(rate, 3), fraction_of_hbm_copy_rate=round(rate / HBM_COPY_TB_S, 3))
    print(json.dumps(res), flush=True)
    return res


def run(a, dev, comb):
    B, K, trials, T, F, E = a.batch, 8, 2, 253, 513, 100
    mul = comb == "mul"
    W, C = (F, F) if mul else (F + E, E)
    rows = B * trials * K * T
    g = torch.Generator(device=dev).manual_seed(0)
    dxs, ld = h.padded(rows, W, dev, zero=True)
    dxs[:, :W].normal_(generator=g)
    pre, ldp = h.padded(B * T, F, dev, zero=True)
    pre[:, :F].normal_(generator=g)
    other = torch.empty_like(dxs)
    calls = {"copy": (lambda: other.copy_(dxs), 2 * dxs.numel() * 4)}
    for stride in (0,) + STRIDES:                   # 0: the utterance-level entry points
        Ta = -(-T // stride) if stride else 0
        n_aux = B * K * max(Ta, 1) * C
        aux = torch.rand(*((B, K, Ta, C) if stride else (B, K, C)), device=dev, generator=g)
        # the kernels are timed on aux rows that are already 16-byte addressable; the padding copy hip_ops.cond_fwd makes
        # per call when C % 4 != 0 (rows_view) is a launch sequence of its own below
        info = h.rows_view(aux)
        tag = f"_t_stride{stride}" if stride else ""
        kw = dict(Ta=Ta, stride=stride or 1)
        if info[0].data_ptr() != aux.data_ptr():
            calls[f"pad_aux{tag}"] = (lambda aux=aux: h.rows_view(aux), 4 * (n_aux + info[0].numel()))
        calls[f"cond_{comb}{tag}_fwd"] = (
            lambda aux=aux, kw=kw, info=info: h.cond_fwd(pre, ldp, aux, B, K, T, F, trials, comb, auxinfo=info, **kw),
            4 * (rows * W + B * T * F + n_aux))
        if mul:
            calls[f"cond_mul{tag}_bwd"] = (
                lambda info=info, kw=kw: h.cond_bwd(dxs, ld, info, B, K, T, F, trials, comb, **kw), 4 * (rows * F + n_aux + B * T * F))
        calls[f"cond_{comb}_aux{tag}_bwd"] = (
            lambda kw=kw: h.cond_aux_bwd(dxs, ld, pre if mul else None, ldp if mul else 0, B, K, T, F, E, trials, comb, **kw),
            4 * (rows * C + (B * T * F if mul else 0) + n_aux))
    return _report(dict(combination=comb, B=B, K=K, trials=trials, T=T, F=F, E=E, strides=list(STRIDES)), calls, a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=768)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = []
    for comb in ("mul", "cat"):
        results.append(run(a, dev, comb))
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
