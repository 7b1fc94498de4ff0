"""Micro-benchmark (GPU box): the fused two-mask tail (tssep_mask_map_fwd / _bwd) against the two-launch compositions of
the kernels that existed before it, on rows of the 4-speaker (K = 4, T = 253) and 8-speaker (K = 8, T = 1878) workloads,
F = 513, at M = 1 and M = 2 masks per speaker; and one toy-overlay training step with nmask = 2 beside nmask = 1, both
through TorchBF(differentiable=True).  Writes profiles/two_mask_head.json (DESIGN 4.9 quotes it).

    forward    fused: raw -> logit, mask                      composition: logit_map_fwd, then maskhead_fwd with obs = 0
    backward   fused: dmask, mask -> draw                     composition: maskhead_bwd with dest = 0, then logit_map_bwd

The M = 2 composition runs on the [B, K M, T, F] view (K M "speakers", the permutation expanded to perm[b, k] M + m):
what trials = 1 allows.  Bytes are the algorithmic HBM bytes of each launch (include/tssep_hip.h); the fraction is of the
8 TB/s the README uses.  Every timing is a window of `inner` calls between two device events after a warm-up; fused and
composed windows alternate, `reps` of each; the median and the spread (min, max) of the windows are recorded."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tssep_amd import hip_ops as h  # noqa: E402

PEAK = 8e12
F = 513


def window(fn, inner):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(inner):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / inner


def alternate(fns, reps, inner):
    """{name: [ms per call of every window]}; the candidates take turns, window by window"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window(fn, inner))
    return times


def stats(ms, nbytes):
    med = statistics.median(ms)
    return dict(ms=round(med, 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4), bytes=int(nbytes),
                TBps=round(nbytes / med / 1e9, 3), frac_of_8TBps=round(nbytes / (med * 1e-3) / PEAK, 3))


def tail(B, K, T, M, reps, inner):
    n = B * K * M * T * F
    g = torch.Generator(device="cuda").manual_seed(B + K + M)
    raw = torch.randn(n, device="cuda", generator=g)
    dmask = torch.randn(B, K, M, T, F, device="cuda", generator=g)
    pm = torch.stack([torch.randperm(K, device="cuda", generator=g) for _ in range(B)]).int()
    ipm = torch.argsort(pm, -1).int()
    # the [B, K M, T, F] view of the composition: "speaker" k M + m goes to row perm[b, k] M + m
    m_ = torch.arange(M, device="cuda", dtype=torch.int32)
    pm2 = (pm[:, :, None] * M + m_).reshape(B, K * M).contiguous()
    ipm2 = torch.argsort(pm2, -1).int()
    obs0 = torch.zeros(B, T, F, device="cuda", dtype=torch.complex64)
    dest0 = torch.zeros(B, K * M, T, F, device="cuda", dtype=torch.complex64)
    KM = K * M

    def fused_fwd():
        return h.mask_map_fwd(raw, pm, ipm, B, 1, K, M, T, F, F, 0)

    def composed_fwd():
        return h.maskhead_fwd(h.logit_map_fwd(raw, pm2, ipm2, B, 1, KM, T, F, F, 0), obs0)
    logit, mask = fused_fwd()
    mask_c, _ = composed_fwd()
    same_fwd = bool(torch.equal(mask.view(B, KM, T, F), mask_c))

    def fused_bwd():
        return h.mask_map_bwd(dmask, mask, None, pm, ipm, B, 1, K, M, T, F, F, 0)

    def composed_bwd():
        return h.logit_map_bwd(h.maskhead_bwd(dest0, dmask.view(B, KM, T, F), mask_c, obs0), pm2, ipm2, B, 1, KM, T, F, F, 0)
    a, b = fused_bwd(), composed_bwd()
    worst_bwd = float((a - b).abs().max() / b.abs().max())
    del a, b
    e4 = 4 * n
    # bytes per launch: fused fwd raw + logit + mask; composed fwd (raw + logit) + (logit + mask + the complex estimate, the
    # observation once per utterance); fused bwd dmask + mask + draw; composed bwd (complex dest + dmask + mask + dlogit,
    # the observation) + (dlogit + draw)
    nb = dict(fused_fwd=3 * e4, composed_fwd=2 * e4 + (4 * e4 + 8 * B * T * F),
              fused_bwd=3 * e4, composed_bwd=(5 * e4 + 8 * B * T * F) + 2 * e4)
    t = alternate(dict(fused_fwd=fused_fwd, composed_fwd=composed_fwd), reps, inner)
    t.update(alternate(dict(fused_bwd=fused_bwd, composed_bwd=composed_bwd), reps, inner))
    res = dict(B=B, K=K, T=T, F=F, M=M, elements=n, forward_mask_bit_identical=same_fwd,
               backward_max_rel_difference=worst_bwd, **{k: stats(v, nb[k]) for k, v in t.items()})
    for d in ("fwd", "bwd"):
        f_, c_ = res["fused_" + d], res["composed_" + d]
        # not slower than the composition by more than the run-to-run spread of the two
        spread = max(f_["ms_max"] - f_["ms_min"], c_["ms_max"] - c_["ms_min"])
        res[f"{d}_fused_over_composed"] = round(f_["ms"] / c_["ms"], 3)
        res[f"{d}_fused_not_slower_within_spread"] = bool(f_["ms"] <= c_["ms"] + spread)
    return res


def toy_step(nmask, steps, warmup):
    """ms per eager step (forward + review + backward) of the toy model, units 10 / projs 12, K = 3, three channels,
    N = 16000, TorchBF(differentiable=True) + LogMAE; nmask = 2: toy_tssep_two_mask.yaml"""
    import tempfile
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(ROOT, "tssep_amd", "exp")
    K, D, N = 3, 3, 16000
    yamls = ["toy_common.yaml", "toy_tssep.yaml"] + (["toy_tssep_two_mask.yaml"] if nmask == 2 else [])
    cfg = run.build_config([os.path.join(exp, y) for y in yamls] + [
        f"eg.trainer.storage_dir={tempfile.mkdtemp()}", "eg.trainer.model.mask_estimator.units=10",
        "eg.trainer.model.mask_estimator.projs=12", f"eg.trainer.model.mask_estimator.ts_vad={K}",
        "eg.trainer.model.enhancer.factory=tssep.train.enhancer.TorchBF", "eg.trainer.model.enhancer.differentiable=true"])
    m = Experiment.from_config(cfg["eg"]).trainer.model.cuda()
    assert m.mask_estimator.nmask == nmask
    ex = next(iter(m.prepare_train_dataset(torch.device("cuda"), batch_size=1, prefetch=False)))
    mix = ex["observation"][0, 0, :N]
    g = torch.Generator(device="cpu").manual_seed(3)
    obs = torch.stack([a * torch.roll(mix, d) for a, d in ((1.0, 0), (0.8, 3), (0.6, 7))])
    obs = obs + 0.05 * mix.abs().max() * torch.randn(D, N, generator=g).to(obs)
    ex = dict(ex, observation=obs[None], auxInput=ex["auxInput"][:, :K].contiguous(), reference_channel=0)
    ex[m.loss.target] = ex[m.loss.target][:, :K, :N].contiguous()
    np.random.seed(1)
    ms = []
    for i in range(warmup + steps):
        e = dict(ex)
        m.zero_grad()
        torch.cuda.synchronize()
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        m.review(e, m(e))["loss"].backward()
        t.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(s.elapsed_time(t))
    return dict(nmask=nmask, ms=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), ms_max=round(max(ms), 3), steps=steps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "two_mask_head.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--batch4", type=int, default=256, help="utterances of the 4-speaker rows (K = 4, T = 253)")
    ap.add_argument("--batch8", type=int, default=8, help="utterances of the 8-speaker rows (K = 8, T = 1878)")
    ap.add_argument("--toy-steps", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_two_mask.py measures on the GPU; there is no CPU path"
    res = dict(device=torch.cuda.get_device_name(0), reps=a.reps, inner=a.inner, peak_TBps=PEAK / 1e12, tail=[], toy_step=[])
    for name, (B, K, T) in (("4-speaker", (a.batch4, 4, 253)), ("8-speaker", (a.batch8, 8, 1878))):
        for M in (1, 2):
            r = dict(workload=name, **tail(B, K, T, M, a.reps, a.inner))
            res["tail"].append(r)
            print(json.dumps(r), flush=True)
    if a.toy_steps > 0:
        for nmask in (1, 2, 1, 2):                          # alternating, two rounds
            r = toy_step(nmask, a.toy_steps, 3)
            res["toy_step"].append(r)
            print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
