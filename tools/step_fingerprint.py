"""What a training step launches, and the bits it leaves: the record a host-side refactor is held to.

    python tools/step_fingerprint.py --record tests/golden/step_fingerprint.json        # on an MI355X

Every case of CASES runs a piece of the step (one RNNP layer, the final Linear, the affine layers of the speaker
embeddings, two optimizer steps of a toy experiment) from fixed seeds.  While it runs, `Trace` keeps
  * the entry-point name of every `hip_ops.check` (one per launch), with the stream it went to: "main" = the stream that
    was current when the case began, "other" = any other;
  * every `torch.cuda.Stream.wait_stream`, as "wait:<waiter><-<waited>" in the same sequence;
  * `hip_ops.GEMM_LOG`, `RECURRENCE_LOG`, `TAIL_LOG` (cases D: the kernel plan the Trainer derives from them -- it owns
    the three logs during its first step).
After a synchronise and `check_cluster_errors` every output and gradient tensor is hashed (sha256 of dtype, shape, bytes).

--record runs every case twice.  Cases D -- whole steps -- then run twice more, each from an allocator cache whose free
blocks were filled with a value of the recorder's (`poison`: 0, then 2.5): a step that reads memory it never wrote gives
what its predecessor in the process left there, and must not pass for reproducible.  The traces must agree (anything else ends the run with exit status 2); the tensor hashes are
written when all runs agree, otherwise the case goes to "unstable" with the digests seen.  Cases A - C run fixed-order, atomic-free kernels: one of
them under "unstable" is a finding (exit status 1), not something to commit.
tests/test_gpu_step_fingerprint.py re-runs the cases against the committed file; a change that moves launches or kernels
on purpose records again with this tool.  --cases PREFIX[,PREFIX...] records the chosen cases only and leaves the other
entries of an existing file as they are (new cases beside a record that must not move).

The parent's Python beside the library of this tree: put the parent's `tssep_amd/` (and `include/`) first on PYTHONPATH
and name the library in TSSEP_HIP_LIB -- this file only appends its own tree to sys.path."""
import argparse
import collections
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path += [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tssep_amd import functional as Fn, hip_ops as H  # noqa: E402
from tssep_amd.train import runtime  # noqa: E402

DEV = "cuda"
EXP = os.path.join(ROOT, "tssep_amd", "exp")
HOST_ONLY = {"fft_twiddles"}      # a host table cached per process: no launch, and asked once however many cases run


class Trace:
    """``with Trace() as t:`` -> t.events (launches and waits in order), t.logs (the three launch logs)"""

    def __enter__(self):
        self.main = torch.cuda.current_stream().cuda_stream
        H.side_stream(torch.cuda.current_stream().device)      # exists from here on: GradBucket.sync joins it only if it does
        self.events = []
        self.logs = dict(gemm=[], recurrence=[], tail=[])
        self.old = (H.check, torch.cuda.Stream.wait_stream, H.GEMM_LOG, H.RECURRENCE_LOG, H.TAIL_LOG)
        check, wait = self.old[:2]

        def check_(status, what):
            if what not in HOST_ONLY:
                self.events.append(f"{what}@{self.role(torch.cuda.current_stream())}")
            return check(status, what)

        def wait_(stream, other):
            self.events.append(f"wait:{self.role(stream)}<-{self.role(other)}")
            return wait(stream, other)

        H.check, torch.cuda.Stream.wait_stream = check_, wait_
        H.GEMM_LOG, H.RECURRENCE_LOG, H.TAIL_LOG = self.logs["gemm"], self.logs["recurrence"], self.logs["tail"]
        return self

    def role(self, stream):
        return "main" if stream.cuda_stream == self.main else "other"

    def __exit__(self, *exc):
        H.check, torch.cuda.Stream.wait_stream, H.GEMM_LOG, H.RECURRENCE_LOG, H.TAIL_LOG = self.old
        return False


def sha(t):
    """sha256 of a tensor's dtype, shape and bytes (None: of nothing)"""
    h = hashlib.sha256()
    if t is not None:
        t = t.detach().cpu().contiguous()
        h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        h.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
    return h.hexdigest()


def _grads(names, params):
    return {k: (p.grad.detach().clone() if p.grad is not None else None) for k, p in zip(names, params)}


def _bucket(params, sinks):
    from tssep_amd.distributed import GradBucket
    return GradBucket(params) if sinks else None


# ---- A: one RNNP layer ---------------------------------------------------------------------------------------------------
Builders = collections.namedtuple("Builders", "NAMES SHAPES make_case make_params modules module_params")


def builders(causal):
    """the case builders of the two-direction layer (tests/test_rnnp_layer_reference.py) or of the causal one
    (tests/test_causal_reference.py: the first four of its LAYER_SHAPES, by name)"""
    if causal:
        import test_causal_reference as R
        shapes = dict(zip(("pad", "pad_combined", "align", "w32"), R.LAYER_SHAPES))
        return Builders(R.CNAMES, shapes, R.make_causal_case, R.make_causal_params, R.causal_modules, R.causal_module_params)
    import test_rnnp_layer_reference as R
    return Builders(R.NAMES, R.SHAPES, R.make_case, R.make_params, R.modules, R.module_params)


def rnnp(shape, act, prec, sinks, frozen=None, x_grad=True, dropout_p=0.0, causal=False):
    NAMES, SHAPES, make_case, _, modules, module_params = builders(causal)
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, dy = make_case(N, T, I, Hh, hdim, 0, combine)
    lstm, lin = modules(params, device=DEV)
    if frozen:
        getattr(lstm, frozen).requires_grad_(False)
    ps = module_params(lstm, lin)
    bucket = _bucket(ps, sinks)
    xg = x.to(DEV).requires_grad_(x_grad)
    with runtime.applied(gemm_precision=prec):
        if dropout_p:
            H.manual_seed(3)
        for _ in range(2 if sinks else 1):
            y = Fn.rnnp_layer(xg, lstm, lin, N, T, act=act, combine=combine, dropout_p=dropout_p)
            y.backward(dy.to(DEV))
    if bucket is not None:
        bucket.sync()
    return dict(_grads(NAMES, ps), y=y.detach(), x=xg.grad)


def chain(K, causal=False):
    """two stacked layers with the Tanh backward folded into the consumer's d(input) GEMM (K: the producer combines)"""
    NAMES, _, _, make_params, modules, module_params = builders(causal)
    N, T, I, Hh, hdim = 8, 5, 7, 5, 8
    Kc = K or 1
    gen = torch.Generator().manual_seed(77)
    p0, p1 = make_params(I, Hh, hdim, gen), make_params(Kc * hdim, Hh, hdim, gen)
    x = torch.randn(N * T, I, generator=gen)
    dy = torch.randn(N // Kc * T, hdim, generator=gen)
    l0, q0 = modules(p0, device=DEV)
    l1, q1 = modules(p1, device=DEV)
    xg = x.to(DEV).requires_grad_()
    h = Fn.rnnp_layer(xg, l0, q0, N, T, act=1, combine=K, dz_given=True)
    y = Fn.rnnp_layer(h, l1, q1, N // Kc, T, in_tanh=Kc)
    y.backward(dy.to(DEV))
    out = {"0." + k: v for k, v in _grads(NAMES, module_params(l0, q0)).items()}
    out.update({"1." + k: v for k, v in _grads(NAMES, module_params(l1, q1)).items()})
    return dict(out, y=y.detach(), h=h.detach(), x=xg.grad)


def state(shape, chunks, act):
    """The causal layer without gradients: the whole utterance with return_state, then the same frames in `chunks`, each
    started from the previous chunk's (hT, cT)."""
    _, SHAPES, make_case, _, modules, _ = builders(True)
    N, T, I, Hh, hdim, combine = SHAPES[shape]
    x, params, _ = make_case(N, T, I, Hh, hdim, 0, combine)
    lstm, lin = modules(params, device=DEV)
    x3 = x.to(DEV).view(N, T, I)
    with torch.no_grad():
        y, (hT, cT) = Fn.rnnp_layer(x3.reshape(N * T, I), lstm, lin, N, T, act=act, combine=combine, return_state=True)
        ys, last, t0 = [], None, 0
        for n in chunks:
            yc, last = Fn.rnnp_layer(x3[:, t0:t0 + n].reshape(N * n, I), lstm, lin, N, n, act=act, combine=combine,
                                     state=last, return_state=True)
            ys.append(yc.reshape(N // (combine or 1), n, -1))
            t0 += n
    assert t0 == T, (chunks, T)
    return dict(y=y, hT=hT, cT=cT, y_chunks=torch.cat(ys, 1), hT_chunks=last[0], cT_chunks=last[1])


# ---- B: the final Linear ---------------------------------------------------------------------------------------------------
def head(masks, trials, sinks):
    B, K, T, F, P = 2, 2, 5, 9, 12
    M = 2 if masks else 1
    gen = torch.Generator().manual_seed(11)
    lin = torch.nn.Linear(P, K * M * F)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(K * M * F, P, generator=gen) * 0.3)
        lin.bias.copy_(torch.randn(K * M * F, generator=gen) * 0.3)
    lin = lin.to(DEV)
    perm = torch.stack([torch.randperm(K, generator=gen) for _ in range(B)])
    perm_d, iperm_d = perm.int().to(DEV), perm.argsort(-1).int().to(DEV)
    x = torch.randn(B * trials * T, P, generator=gen).to(DEV).requires_grad_()
    shape = (B, K, M, T, F) if masks else (B, K, T, F)
    douts = [torch.randn(*shape, generator=gen).to(DEV) for _ in range(M)]
    bucket = _bucket([lin.weight, lin.bias], sinks)
    for _ in range(2 if sinks else 1):
        if masks:
            outs = Fn.head_masks(x, lin, perm_d, iperm_d, B, K, M, T, F, trials, F, False)
        else:
            outs = (Fn.head(x, lin, perm_d, iperm_d, B, K, T, F, trials, F, False),)
        torch.autograd.backward(outs, douts)
    if bucket is not None:
        bucket.sync()
    out = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    return dict(out, x=x.grad, **_grads(("w", "b"), (lin.weight, lin.bias)))


# ---- C: the affine layers of the learned speaker embeddings ----------------------------------------------------------------
def _linear(idim, odim, gen, bias=True):
    lin = torch.nn.Linear(idim, odim, bias=bias)
    with torch.no_grad():
        for p in lin.parameters():
            p.copy_(torch.randn(*p.shape, generator=gen) * 0.3)
    return lin.to(DEV)


def affine(bias, sinks):
    gen = torch.Generator().manual_seed(12)
    lin = _linear(7, 5, gen, bias)
    x = torch.randn(6, 7, generator=gen).to(DEV).requires_grad_()
    dy = torch.randn(6, 5, generator=gen).to(DEV)
    ps = list(lin.parameters())
    bucket = _bucket(ps, sinks)
    for _ in range(2 if sinks else 1):
        y = Fn.affine(x, lin.weight, lin.bias)
        y.backward(dy)
    if bucket is not None:
        bucket.sync()
    return dict(_grads(("w", "b"), ps), y=y.detach(), x=x.grad)


def aux_mlp(sinks):
    gen = torch.Generator().manual_seed(13)
    lengths = (4, 2, 5)                      # S = 3 ragged enrolment segments
    lins = [_linear(7, 8, gen), _linear(8, 8, gen), _linear(8, 5, gen)]
    x = torch.randn(sum(lengths), 7, generator=gen).to(DEV)
    dy = torch.randn(len(lengths), 5, generator=gen).to(DEV)
    row0 = H.segment_rows(list(lengths), torch.device(DEV))
    ps = [p for l in lins for p in (l.weight, l.bias)]
    bucket = _bucket(ps, sinks)
    for _ in range(2 if sinks else 1):
        y = Fn.aux_mlp(x, row0, len(lengths), lins)
        y.backward(dy)
    if bucket is not None:
        bucket.sync()
    return dict(_grads(("w1", "b1", "w2", "b2", "w3", "b3"), ps), y=y.detach())


# ---- D: two optimizer steps of the toy experiment -----------------------------------------------------------------------------
class _Dataset(list):
    def __iter__(self):
        return (dict(ex) for ex in list.__iter__(self))


def _three_channels(m, ex, K=3, D=3, N=16000):
    """TorchBF wants an array: delayed, scaled copies of the mixture plus noise per channel, K speakers, N samples"""
    key = m.loss.target
    mix = ex["observation"][0, 0, :N]
    g = torch.Generator(device="cpu").manual_seed(3)
    obs = torch.stack([a * torch.roll(mix, d) for a, d in ((1.0, 0), (0.8, 3), (0.6, 7))])
    obs = obs + 0.05 * mix.abs().max() * torch.randn(D, N, generator=g).to(obs)
    ex = dict(ex, observation=obs[None], auxInput=ex["auxInput"][:, :K].contiguous(), reference_channel=0)
    ex[key] = ex[key][:, :K, :N].contiguous()
    return ex


def toy(overlay, graph, trace):
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    two_mask = overlay == "toy_tssep_two_mask.yaml"
    small = ["eg.trainer.model.mask_estimator.units=10", "eg.trainer.model.mask_estimator.projs=12",
             "eg.trainer.model.mask_estimator.ts_vad=3"] if two_mask else []
    with tempfile.TemporaryDirectory() as tmp:
        torch.manual_seed(17)
        cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", *([overlay] if overlay else []))]
                               + [f"eg.trainer.storage_dir={tmp}", "eg.trainer.stop_trigger=[2,iteration]",
                                  "eg.trainer.summary_trigger=[1,iteration]", "eg.trainer.checkpoint_trigger=[1000,iteration]"]
                               + small)
        eg = Experiment.from_config(cfg["eg"])
        tr = eg.trainer
        m = tr.model.cuda()
        data = []
        for ex in m.prepare_train_dataset(torch.device("cuda"), batch_size=1, prefetch=False):
            data.append(_three_channels(m, ex) if two_mask else ex)
            if len(data) == 2:
                break
        with runtime.applied(dict(eg.runtime, graph_step=graph)):
            np.random.seed(9)
            H.manual_seed(3)
            hist = tr.train(_Dataset(data), device=0)
            torch.cuda.synchronize()
        trace.logs = tr.kernel_plan                 # (the Trainer took the three logs for its first step)
        assert len(hist) == 2 and tr.optimizer.step_count == 2, (hist, tr.optimizer.step_count)
        return dict(losses=torch.tensor([l for _, l in hist], dtype=torch.float64), flat_param=tr.optimizer.flat_param.detach().clone())


def poison(value):
    """Every block `torch.empty` will hand out next holds `value`: the cache is emptied, refilled with blocks of the small
    (< 1 MiB), the 20-MiB-segment and the large pool, written, and freed again."""
    torch.cuda.empty_cache()
    blocks = [torch.full((n // 4,), value, device=DEV) for n, count in ((1 << 19, 256), (9 << 20, 32), (64 << 20, 8))
              for _ in range(count)]
    torch.cuda.synchronize()
    del blocks


def _cases():
    c = collections.OrderedDict()
    for shape in ("pad", "pad_combined", "align", "w768"):
        for act in (0, 1):
            for prec in ("f32", "bf16x3"):
                for sinks in (False, True):
                    c[f"A/{shape}/act{act}/{prec}/{'sinks' if sinks else 'autograd'}"] = (rnnp, (shape, act, prec, sinks))
    c["A/pad/act1/bf16x3/frozen"] = (rnnp, ("pad", 1, "bf16x3", True, "bias_hh_l0"))
    c["A/pad/act1/bf16x3/no_dx"] = (rnnp, ("pad", 1, "bf16x3", False, None, False))
    c["A/two_layers/K0"] = (chain, (0,))
    c["A/two_layers/K4"] = (chain, (4,))
    c["A/align/act1/bf16x3/dropout"] = (rnnp, ("align", 1, "bf16x3", False, None, True, 0.5))
    for shape in ("pad", "pad_combined", "align", "w32"):
        for act in (0, 1) if shape != "w32" else (1,):
            for prec in ("f32", "bf16x3") if shape != "w32" else ("bf16x3",):
                for sinks in (False, True):
                    c[f"A/causal/{shape}/act{act}/{prec}/{'sinks' if sinks else 'autograd'}"] = (
                        rnnp, (shape, act, prec, sinks, None, True, 0.0, True))
    c["A/causal/pad/act1/bf16x3/frozen"] = (rnnp, ("pad", 1, "bf16x3", True, "bias_hh_l0", True, 0.0, True))
    c["A/causal/pad/act1/bf16x3/no_dx"] = (rnnp, ("pad", 1, "bf16x3", False, None, False, 0.0, True))
    c["A/causal/align/act1/bf16x3/dropout"] = (rnnp, ("align", 1, "bf16x3", False, None, True, 0.5, True))
    c["A/causal/two_layers/K0"] = (chain, (0, True))
    c["A/causal/two_layers/K4"] = (chain, (4, True))
    c["A/causal/state/plain"] = (state, ("align", [5, 1, 1], 0))
    c["A/causal/state/combined"] = (state, ("pad_combined", [3, 1, 1], 1))
    for sinks in (False, True):
        tag = "sinks" if sinks else "autograd"
        c[f"B/head_fast/{tag}"] = (head, (False, 1, sinks))
        c[f"B/head_logit_map/{tag}"] = (head, (False, 2, sinks))
        c[f"B/head_masks/{tag}"] = (head, (True, 1, sinks))
        c[f"C/affine_bias/{tag}"] = (affine, (True, sinks))
        c[f"C/affine_nobias/{tag}"] = (affine, (False, sinks))
        c[f"C/aux_mlp/{tag}"] = (aux_mlp, (sinks,))
    for overlay in (None, "explicit_vad", "auxnet", "two_mask", "dropout", "pit", "causal"):
        for graph in ("off", "on"):
            c[f"D/{overlay or 'plain'}/{'graph' if graph == 'on' else 'eager'}"] = (
                toy, (f"toy_tssep_{overlay}.yaml" if overlay else None, graph))
    return c


CASES = _cases()
_WARM = []


def run_case(name):
    """-> (fingerprint of the trace: dict(launches, trace), {tensor name: tensor}).  The first eager pair of toy steps of a
    process leaves other bits than every later one (with the weight gradients on the side stream only; found while
    recording), so one pair runs unrecorded before the first case D."""
    fn, args = CASES[name]
    if fn is toy and not _WARM:
        _WARM.append(toy(None, "off", argparse.Namespace()) is not None)
    torch.cuda.synchronize()
    with Trace() as t:
        tensors = fn(*args, t) if fn is toy else fn(*args)
        torch.cuda.synchronize()
        H.check_cluster_errors()
    digest = hashlib.sha256(json.dumps([t.events, t.logs], sort_keys=True, default=str).encode()).hexdigest()
    launches = t.events if not name.startswith("D/") else dict(sorted(collections.Counter(t.events).items()))
    return dict(launches=launches, trace=digest), tensors


def hashes(tensors):
    return {k: sha(v) for k, v in sorted(tensors.items())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--record", metavar="JSON", required=True)
    ap.add_argument("--cases", default="", help="comma-separated prefixes (default: every case)")
    args = ap.parse_args()
    pick = [p for p in args.cases.split(",") if p]
    out, unstable, moved = {}, {}, []
    if pick and os.path.exists(args.record):      # chosen cases only: the file's other entries stay as they are
        with open(args.record) as f:
            old = json.load(f)
        out, unstable = old["cases"], old["unstable"]
    names = [n for n in CASES if not pick or any(n.startswith(p) for p in pick)]
    seen = {n: [] for n in names}                      # name -> [(trace, tensor hashes)]
    for name in names:
        seen[name] += [(fp, hashes(t)) for fp, t in (run_case(name), run_case(name))]
    for name in names:
        for value in (0.0, 2.5) if name.startswith("D/") else ():
            poison(value)
            fp, t = run_case(name)
            seen[name].append((fp, hashes(t)))
    for name in names:
        fps, hs = [fp for fp, _ in seen[name]], [h for _, h in seen[name]]
        fp1, h1 = fps[0], hs[0]
        if any(fp != fp1 for fp in fps):
            moved.append(name)
            print(f"{name}: the runs launched differently\n  " + "\n  ".join(str(fp["launches"]) for fp in fps), flush=True)
            continue
        if all(h == h1 for h in hs):
            out[name] = dict(fp1, tensors=h1)
            unstable.pop(name, None)
        else:
            out[name] = fp1
            unstable[name] = sorted({hashlib.sha256(json.dumps(h).encode()).hexdigest() for h in hs})
            order = [json.dumps(h) for h in hs]
            print(f"{name}: UNSTABLE {[k for k in h1 if any(h[k] != h1[k] for h in hs)]}, results by run "
                  + "".join("ABCDEFGH"[sorted(set(order), key=order.index).index(o)] for o in order), flush=True)
        print(f"{name}: {len(fp1['launches'])} {'kinds of ' if name.startswith('D/') else ''}launches", flush=True)
    with open(args.record, "w") as f:
        json.dump(dict(cases=out, unstable=unstable), f, indent=0, sort_keys=True)
        f.write("\n")
    if moved:
        raise SystemExit(2)
    if any(not n.startswith("D/") for n in unstable):
        print("a fixed-order case did not reproduce: a finding, not a fingerprint", flush=True)
        raise SystemExit(1)


if __name__ == "__main__":
    main()
