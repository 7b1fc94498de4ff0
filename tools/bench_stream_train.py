"""Micro-benchmark of training on a stream.  Section 4.20's protocol: device events, 3 warm-ups, the
median of 20 with min and max (max - min: the run-to-run spread in the process).

(a) tssep_mask_istft_stream_bwd -- one middle call of a stream (skip 0, a carry gradient behind it, d_ola_in wanted) -- at
    (B K, Tc) = (3072, 253), (8, 16) and (8, 1) against tssep_mask_istft_bwd at the same frame count (the whole-utterance
    entry point needs four frames: (8, 1) is set against T = 4, launch against launch).  With --parent-lib FILE, the parent
    commit's libtssep_hip.so, its tssep_mask_istft_bwd is bound beside this build's and timed in the same rounds, and the
    row says whether the stream launch differs from it by more than its own spread.
(b) one causal toy model (units 64, projs 48), B = 4, K = 4, N = 64000 (253 frames): zero_grad + forward + backward as one
    Model.forward step against online.stream_loss_step in 4 pushes, detached and undetached.  A record.

    python tools/bench_stream_train.py [--parent-lib FILE] [--out profiles/stream_train_microbench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP, REPS = 3, 20
SIZES = ((768, 4, 253), (2, 4, 16), (2, 4, 1))          # (B, K, Tc)


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


def parent_entry(parent_lib):
    """tssep_mask_istft_bwd of the parent commit's build, bound beside this build's library: -> fn(dy, logit, obs, wsyn)
    with hip_ops.mask_istft_bwd's work around the launch (the result's allocation, the pointers)"""
    import ctypes
    import torch
    from tssep_amd import _lib, hip_ops as h
    _lib.lib()                                              # (this build's first: torch's HIP runtime is the one both bind to)
    fn = ctypes.CDLL(os.path.abspath(parent_lib)).tssep_mask_istft_bwd
    fn.restype, fn.argtypes = _lib.parse_header()["tssep_mask_istft_bwd"]

    def run(dy, logit, obs, wsyn):
        B, K, T, _ = logit.shape
        dlogit = torch.empty_like(logit)
        obs_r = torch.view_as_real(obs)
        rc = fn(h._p(dy), h._p(logit), h._p(obs_r), B, K, dy.shape[-1], 1024, 256, 1, h._p(wsyn),
                h._p(h.fft_tables(1024, logit.device)), h._p(dlogit), T, h._stream())
        assert rc == 0, rc
        return dlogit
    return run


def kernels(parent_lib, emit):
    """(a): in one process, every round runs the stream backward, this build's whole-utterance backward and (with
    --parent-lib) the parent build's once in turn"""
    sys.path.insert(0, HERE)
    import torch
    from tssep_amd import functional as Fn, hip_ops as h
    dev = torch.device("cuda")
    ws = Fn.windows("hann", 1024, 256, dev, 1024)[1]
    parent = parent_entry(parent_lib) if parent_lib else None
    for B, K, Tc in SIZES:
        torch.manual_seed(Tc)
        T = max(Tc, 4)                                      # (the whole-utterance entry point needs four frames)
        logit = torch.randn(B, K, T, 513, device=dev) * 2
        obs = torch.view_as_complex(torch.randn(B, T, 513, 2, device=dev))
        dy_w = torch.randn(B, K, (T - 3) * 256, device=dev)
        lg, ob = logit[:, :, :Tc].contiguous(), obs[:, :Tc].contiguous()
        dy_s, carry = torch.randn(B, K, Tc * 256, device=dev), torch.randn(B * K, 768, device=dev)
        calls = {"stream": lambda: h.mask_istft_stream_bwd(dy_s, carry, lg, ob, ws, 0),
                 "stream_no_d_ola_in": lambda: h.mask_istft_stream_bwd(dy_s, carry, lg, ob, ws, 0, want_ola=False),
                 "whole": lambda: h.mask_istft_bwd(dy_w, logit, obs, ws)}
        if parent:
            calls["parent_whole"] = lambda: parent(dy_w, logit, obs, ws)
        res = alternate(calls)
        base = res["parent_whole" if parent else "whole"]
        row = dict(what="mask_istft_stream_bwd", rows=B * K, Tc=Tc, T_whole=T, **res,
                   launch_ratio_stream_to_whole=round(res["stream"]["median_ms"] / base["median_ms"], 4),
                   differ_beyond_whole_spread=bool(abs(res["stream"]["median_ms"] - base["median_ms"]) > base["spread_ms"]),
                   whole_is="parent build" if parent else "this build")
        if Tc == T:                                         # the same frames on both sides: a time per frame and row
            row.update(stream_ns_per_frame=round(1e6 * res["stream"]["median_ms"] / (B * K * Tc), 3),
                       whole_ns_per_frame=round(1e6 * base["median_ms"] / (B * K * T), 3))
        emit(row)
        del logit, obs, dy_w, lg, ob, dy_s
        torch.cuda.empty_cache()


def toy_step(emit):
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from tssep_amd import hip_ops as h
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net, online
    B, K, N = 4, 4, 64000
    pushes = (64, 62, 62, 62)
    torch.manual_seed(7)
    f = fe.ConcaternatedSTFTFeatures(
        fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40, causal=True),
        fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann", causal=True), size=1024, shift=256, window="hann")
    me = net.MaskEstimator_v2(idim=553, odim=513, units=64, projs=48, combination="mul", ts_vad=K, rnn_typ="lstm",
                              random_speaker_order=False)
    m = model.Model(fe=f, reader=DummyReader(), mask_estimator=me, enhancer=enhancer.Masking(), loss=loss.LogMAE()).cuda().train()
    rng = np.random.RandomState(1)
    tgt = 0.1 * rng.randn(B, K, N).astype(np.float32)
    ex = dict(observation=torch.as_tensor(tgt.sum(1, keepdims=True)).cuda(), auxInput=torch.as_tensor(rng.rand(B, K, 513).astype(np.float32)).cuda(),
              speaker_reverberation_early_ch0=torch.as_tensor(tgt).cuda(), reference_channel=0, dataset=["d"] * B)
    x, t, aux = ex["observation"][:, 0].contiguous(), ex["speaker_reverberation_early_ch0"], ex["auxInput"]

    def whole():
        m.zero_grad()
        e = dict(ex)
        m.review(e, m(e))["loss"].backward()

    def stream(detach):
        def run():
            m.zero_grad()
            online.stream_loss_step(m, x, t, aux, m.loss, pushes, detach=detach)
        return run
    res = alternate({"whole": whole, "stream_detached": stream(True), "stream_full": stream(False)})
    emit(dict(what="toy_step_fwd_bwd", B=B, K=K, N=N, frames=253, pushes=list(pushes), units=64, projs=48,
              gemm_precision=h.GEMM_PRECISION, **res,
              ratio_detached=round(res["stream_detached"]["median_ms"] / res["whole"]["median_ms"], 4),
              ratio_full=round(res["stream_full"]["median_ms"] / res["whole"]["median_ms"], 4)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "stream_train_microbench.jsonl"))
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libtssep_hip.so, for (a)")
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        def emit(row):
            print(json.dumps(row), flush=True)
            f.write(json.dumps(row) + "\n")
            f.flush()
        kernels(args.parent_lib, emit)
        toy_step(emit)


if __name__ == "__main__":
    main()
