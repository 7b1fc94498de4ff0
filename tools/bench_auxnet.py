"""Micro-benchmark (GPU box): the learned-embedding kernels (csrc/aux.hip) and what aux_net: Linear costs per step.

1. d(conditioning) / d(embedding) (`tssep_cond_mul_aux_bwd`, `tssep_cond_cat_aux_bwd`) at the headline shape -- B = 768,
   K = 8, trials = 2, T = 253, F = 513 (E = 100 for cat) -- beside the existing `tssep_cond_mul_bwd` over the same dxs (the
   same bytes: the yardstick) and a device-to-device copy.  Interleaved in one process, HIP events, median of the rounds;
   the achieved fraction of HBM bandwidth is bytes / time over the 6.29 TB/s a float4 copy reaches (MI355X).
2. Instance norm (both axes), ReLU and the segment mean at feature-sized shapes.
3. The step of the toy model (toy_common.yaml sizes, TS-SEP, LogMAE) with 100-dimensional speaker vectors through
   aux_net: Linear(100, 513) against the same model fed 513-dimensional fixed embeddings, alternating in one process.

    python tools/bench_auxnet.py [--rounds 7] [--reps 5] [--batch 768] [--step-batch 8] [--steps 5] [--no-step] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from tssep_amd import hip_ops as h  # noqa: E402

HBM_COPY_TB_S = 6.29


def timeit(fn, reps):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def _report(part, shape, calls, a):
    times = {k: [] for k in calls}
    for fn, _ in calls.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, (fn, _) in calls.items():
            times[k].append(timeit(fn, a.reps))
    res = dict(part=part, rounds=a.rounds, reps=a.reps, **shape)
    for k, (_, moved) in calls.items():
        ms = statistics.median(times[k])
        rate = moved / ms / 1e9
        res[k] = dict(ms=round(ms, 4), min_ms=round(min(times[k]), 4), max_ms=round(max(times[k]), 4), bytes=moved,
                      tb_per_s=round(rate, 3), fraction_of_hbm_copy_rate=round(rate / HBM_COPY_TB_S, 3))
    print(json.dumps(res), flush=True)
    return res


def d_aux(a, dev):
    B, K, trials, T, F, E = a.batch, 8, 2, 253, 513, 100
    rows = B * trials * K * T
    g = torch.Generator(device=dev).manual_seed(0)
    out = []
    for comb in ("mul", "cat"):
        W = F if comb == "mul" else F + E
        C = F if comb == "mul" else E
        dxs, ld = h.padded(rows, W, dev, zero=True)
        dxs[:, :W].normal_(generator=g)
        pre, ldp = h.padded(B * T, F, dev, zero=True)
        pre[:, :F].normal_(generator=g)
        aux = torch.rand(B, K, C, device=dev, generator=g)
        aux2, ld_aux = h.rows_view(aux)
        other = torch.empty_like(dxs)
        read = 4 * rows * C
        calls = {"copy": (lambda: other.copy_(dxs), 2 * dxs.numel() * 4)}
        if comb == "mul":
            calls["cond_mul_bwd"] = (lambda: h.cond_bwd(dxs, ld, (aux2, ld_aux), B, K, T, F, trials, "mul"),
                                     read + 4 * B * T * F + 4 * B * K * F)
            calls["cond_mul_aux_bwd"] = (lambda: h.cond_aux_bwd(dxs, ld, pre, ldp, B, K, T, F, E, trials, "mul"),
                                         read + 4 * B * T * F + 4 * B * K * F)
        else:
            calls["cond_cat_bwd"] = (lambda: h.cond_bwd(dxs, ld, (aux2, ld_aux), B, K, T, F, trials, "cat"),
                                     4 * rows * F + 4 * B * T * F)
            calls["cond_cat_aux_bwd"] = (lambda: h.cond_aux_bwd(dxs, ld, None, 0, B, K, T, F, E, trials, "cat"),
                                         read + 4 * B * K * E)
        out.append(_report("d_aux", dict(combination=comb, B=B, K=K, trials=trials, T=T, F=F, E=E), calls, a))
        del dxs, other
        torch.cuda.empty_cache()
    return out


def small_kernels(a, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    out = []
    R_, n, C = a.batch, 253, 553
    x = torch.randn(R_, n, C, device=dev, generator=g) + 3
    dy = torch.randn(R_, n, C, device=dev, generator=g)
    for axis in (0, 1):
        y, mean, rscale, xinfo = h.instnorm_fwd(x, axis, 0)
        calls = {"instnorm_fwd": (lambda: h.instnorm_fwd(x, axis, 0), 8 * x.numel()),
                 "instnorm_bwd": (lambda: h.instnorm_bwd(dy, xinfo, mean, rscale, tuple(x.shape), axis, 0), 12 * x.numel())}
        out.append(_report("instnorm", dict(axis=axis, R=R_, n=n, C=C), calls, a))
    N, C = a.batch * 8 * 100, 513                      # 100 enrolment frames for each of batch x 8 speakers
    hbuf, ld = h.padded(N, C, dev, zero=True)
    hbuf[:, :C].normal_(generator=g)
    gbuf = torch.randn_like(hbuf)
    S = a.batch * 8
    row0 = h.segment_rows([100] * S, dev)
    dout, ldd = h.padded(S, C, dev, zero=True)
    calls = {"relu_fwd": (lambda: h.relu_fwd(hbuf, ld, N, C), 8 * N * C),
             "relu_bwd": (lambda: h.relu_bwd(gbuf, ld, hbuf, ld, N, C), 12 * N * C),
             "segment_mean_fwd": (lambda: h.segment_mean_fwd(hbuf, ld, row0, S, C, relu=True), 4 * (N + S) * C),
             "segment_mean_bwd": (lambda: h.segment_mean_bwd(dout, ldd, hbuf, ld, row0, S, N, C, relu=True),
                                  4 * (S + 2 * N) * C)}
    out.append(_report("relu_segment_mean", dict(N=N, S=S, C=C), calls, a))
    return out


def step_time(a, dev):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net, runtime
    from tssep_amd.train.optimizer import Adam
    B, K, N = a.step_batch, 8, 5 * 16000

    def build(aux_net):
        torch.manual_seed(0)
        m = model.Model(
            fe=fe.ConcaternatedSTFTFeatures(
                fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
                fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
            reader=DummyReader(),
            mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=40, projs=42, combination="mul",
                                                aux_net=net.Linear(100, 513) if aux_net else None,
                                                aux_net_output_size=513, ts_vad=K, num_averaged_permutations=2),
            enhancer=enhancer.Masking(), loss=loss.LogMAE()).to(dev).train()
        opt = Adam(gradient_clipping=10.0, lr=1e-4)
        opt.set_parameters(m.parameters())
        return m, opt

    rng = np.random.RandomState(0)
    tgt = (rng.randn(B, K, N) * 0.1).astype(np.float32)
    obs = tgt.sum(1, keepdims=True) + 0.05 * rng.rand(B, 1, N).astype(np.float32)
    base = dict(observation=torch.as_tensor(obs).to(dev), speaker_reverberation_early_ch0=torch.as_tensor(tgt).to(dev),
                reference_channel=0, dataset=["bench"] * B)
    runs = {}
    for aux_net in (False, True):
        m, opt = build(aux_net)
        aux = torch.as_tensor(rng.rand(B, K, 100 if aux_net else 513).astype(np.float32)).to(dev)

        def step(m=m, opt=opt, aux=aux):
            opt.zero_grad()
            ex = dict(base, auxInput=aux)
            m.review(ex, m(ex))["loss"].backward()
            opt.step()
        runs[aux_net] = step
    times = {False: [], True: []}
    with runtime.applied(gemm_precision="bf16x3"):
        for k in (False, True):
            np.random.seed(1)
            runs[k]()
            runs[k]()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k in (False, True):
                times[k].append(timeit(runs[k], a.steps))
    off, on = statistics.median(times[False]), statistics.median(times[True])
    res = dict(part="step", model="toy_common sizes, TS-SEP, LogMAE, eager", batch=B, K=K, samples=N, arithmetic="bf16x3",
               rounds=a.rounds, steps=a.steps, fixed_embedding_ms=round(off, 3), aux_net_linear_ms=round(on, 3),
               cost_ms=round(on - off, 3), ratio=round(on / off, 4),
               spread_fixed=[round(min(times[False]), 3), round(max(times[False]), 3)],
               spread_aux_net=[round(min(times[True]), 3), round(max(times[True]), 3)])
    print(json.dumps(res), flush=True)
    return [res]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=768)
    ap.add_argument("--step-batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    results = d_aux(a, dev)
    results += small_kernels(a, dev)
    torch.cuda.empty_cache()
    if not a.no_step:
        results += step_time(a, dev)
    if a.out:
        with open(a.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
