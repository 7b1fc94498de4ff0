"""Survey (GPU box): how the whole-model error measure of tests/test_gpu_framewise_embeddings.py (case 2) behaves with the
width of the model.  For every seed, combination (mul / cat), number of averaged permutations (1 / 2) and kind of aux --
frame-wise at aux_stride 4 ("t4") and 1 ("t1"), and the utterance-level 3-D aux ("utt": the launches a model made before
frame-wise embeddings existed) -- one forward + backward of MaskEstimator_v2 (B = 2, K = 4, T = 9) is compared with the float64
restatement of tests/framewise_reference.py, and every tensor's error (mask, d(aux), every parameter gradient) is divided by
the error of the fp32 restatement of the same case (the measure of tests/test_rnnp_layer_reference.py, whose bar is
MARGIN = 8).  One JSON line per configuration: the worst ratio of each seed's run and the tensor it belongs to.

    python tools/survey_framewise_ratio.py [--widths 5,6,7,6 24,20,20,16 64,48,40,32] [--seeds 8] [--modes f32] [--out FILE]

(widths: units,projs,idim,odim).  DESIGN 4.12 quotes profiles/framewise_ratio_survey.jsonl.
"""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import framewise_reference as R  # noqa: E402
from test_rnnp_layer_reference import errors  # noqa: E402
from tssep_amd import hip_ops  # noqa: E402
from tssep_amd.train import net  # noqa: E402

U = 2.0 ** -24
B, K, T = 2, 4, 9
T_ = torch.as_tensor


def one_run(comb, nap, kind, seed, units, projs, idim, odim):
    """-> {tensor name: ratio to the fp32 restatement's own error}"""
    stride = 4 if kind == "t4" else 1
    E = odim if comb == "mul" else 5
    torch.manual_seed(100 + seed)
    me = net.MaskEstimator_v2(idim=idim, odim=odim, layers=3, units=units, projs=projs, combination=comb, aux_net_output_size=E,
                              ts_vad=K if nap > 1 else False, num_averaged_permutations=nap, random_speaker_order=True,
                              aux_stride=stride).cuda()
    rng = np.random.RandomState(seed)
    xs = rng.randn(B, T, idim).astype(np.float32)
    aux = (rng.randn(*((B, K, E) if kind == "utt" else (B, K, R.frames_of(T, stride), E))) + 0.5).astype(np.float32)
    gm = rng.randn(B, K, 1, T, odim).astype(np.float32)
    aux_d = T_(aux).cuda().requires_grad_()
    np.random.seed(31 + seed)
    out = me(T_(xs).cuda(), aux_d)
    (out.mask * T_(gm).cuda()).sum().backward()
    torch.cuda.synchronize()
    got = {"mask": out.mask.detach().cpu(), "d aux": aux_d.grad.cpu(), **{"d " + k: q.grad.cpu() for k, q in me.named_parameters()}}
    np.random.seed(31 + seed)
    perm = net.MaskEstimator_v2.draw_permutations(B, K)[0]
    ref = {}
    for dtype in (torch.float64, torch.float32):
        p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in me.state_dict().items()}
        a = T_(aux).to(dtype).requires_grad_()
        o = R.mask_estimator_forward(p, T_(xs).to(dtype), a, odim=odim, aux_stride=stride, combination=comb,
                                     ts_vad=K if nap > 1 else False, num_averaged_permutations=nap, perm=perm)
        (o["mask"] * T_(gm).to(dtype)).sum().backward()
        ref[dtype] = {"mask": o["mask"].detach(), "d aux": a.grad, **{"d " + k: p[k].grad for k, _ in me.named_parameters()}}
    ratios = {}
    for k, r64 in ref[torch.float64].items():
        e, own = errors(got[k], r64), errors(ref[torch.float32][k], r64)
        ratios[k] = max(e[0] / max(own[0], U), e[1] / max(own[1], U))
    return ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", nargs="+", default=["5,6,7,6", "24,20,20,16", "64,48,40,32"])
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--modes", nargs="+", default=["f32"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for width in a.widths:
        units, projs, idim, odim = (int(v) for v in width.split(","))
        for mode in a.modes:
            hip_ops.GEMM_PRECISION = mode
            for comb in ("mul", "cat"):
                for nap in (1, 2):
                    for kind in ("t4", "t1", "utt"):
                        worst, mask, d_aux = [], 0.0, 0.0
                        for seed in range(a.seeds):
                            r = one_run(comb, nap, kind, seed, units, projs, idim, odim)
                            k = max(r, key=r.get)
                            worst.append([round(r[k], 2), k])
                            mask, d_aux = max(mask, r["mask"]), max(d_aux, r["d aux"])
                        res = dict(units=units, projs=projs, idim=idim, odim=odim, arithmetic=mode, combination=comb,
                                   averaged_permutations=nap, aux=kind, worst_ratio=max(w[0] for w in worst),
                                   runs_above_8=sum(w[0] > 8 for w in worst), worst_mask_ratio=round(mask, 2),
                                   worst_d_aux_ratio=round(d_aux, 2), worst_per_seed=worst)
                        print(json.dumps(res), flush=True)
                        lines.append(res)
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
