"""tests/framewise_reference.py tested without a GPU: the float64 restatements of the conditioning on frame-wise
embeddings are anchored against torch autograd and, time-constant, against the utterance-level definitions
(tests/aux_reference.py, oracle.net.mask_estimator_forward); their fp32 forms stay inside the bounds; and every planted
defect of the time axis falls outside them.  Nothing here is compared with the code under test.

Measured here (pytest -rP): worst err / bound of the fp32 restatement d(pre) 0.91 (cat, trials = 1: two additions),
d(aux) 0.99 (mul, stride 1, trials = 1: the bound is the one rounding of the product).  What the planted defects must
leave outside the bound (unequal, for the exact forward) at B = 2, K = 3, T = 7, as asserted below:
    mod_ta             strides 2, 3: more than 0.3 of the forward's aux-fed elements and of d(pre) mul, 0.4 of d(aux); at
                       stride 1 and at stride >= T, t % Ta IS t // stride and nothing may change
    rotate_time        trials = 2: the same fractions at every stride (at Ta = 1 the time index has nothing to rotate, and
                       the speaker index, which the defect leaves unrotated, is what differs)
    drop_last_bucket   strides 2, 3 (T % stride != 0): every element of the last bucket of d(aux), and no other
    no_clamp           strides 2, 3, 8: every element of the last bucket but those of the last flat block, and no other
"""
import numpy as np
import pytest
import torch

import aux_reference as A
import framewise_reference as R
from oracle import net as onet

B, K, T = 2, 3, 7
STRIDES = (1, 2, 3, 7, 8)
SHAPES = [(True, 5, 5), (True, 8, 8), (False, 5, 3), (False, 8, 4)]           # (mul, F, E)


@pytest.mark.parametrize("mul,F,E", SHAPES)
@pytest.mark.parametrize("trials", [1, 2])
def test_the_restatements_against_autograd_and_the_utterance_level_definition(mul, F, E, trials):
    """cond_dpre / cond_daux are the gradients of cond_fwd (autograd, float64), at every stride; with a time-constant
    aux, cond_fwd is aux_reference.condition on the 3-D embedding and d(aux) summed over its rows is that one's gradient."""
    for stride in STRIDES:
        pre, aux, dxs = R.inputs(B, K, trials, T, F, E, mul, stride, seed=10 * stride + trials)
        p64, a64 = pre.double().requires_grad_(), aux.double().requires_grad_()
        xs = R.cond_fwd(p64, a64, mul, trials, stride)
        assert xs.shape == dxs.shape
        gp, ga = torch.autograd.grad(xs, (p64, a64), dxs.double())
        dpre, tol_p = R.cond_dpre(dxs, aux, mul, stride)
        daux, tol_a = R.cond_daux(dxs, pre if mul else None, E, stride)
        assert float((dpre - gp).abs().max()) <= 1e-13 * float(gp.abs().max())
        assert float((daux - ga).abs().max()) <= 1e-13 * float(ga.abs().max())
        assert bool((tol_a > 0).all()) and (mul or trials * K > 1) and bool((tol_p > 0).all())
        # time-constant: the utterance-level definition
        a3 = aux[:, :, 0].double().requires_grad_()
        const = a3[:, :, None].expand(B, K, R.frames_of(T, stride), a3.shape[-1])
        xs_t = R.cond_fwd(pre, const, mul, trials, stride)
        xs_u = A.condition(pre.double(), a3, "mul" if mul else "cat", trials)
        assert torch.equal(xs_t.reshape(xs_u.shape), xs_u)
        (g3,) = torch.autograd.grad(xs_u, a3, dxs.double().view(xs_u.shape))
        assert float((daux.sum(2) - g3).abs().max()) <= 1e-13 * float(g3.abs().max())


@pytest.mark.parametrize("mul,F,E", SHAPES)
@pytest.mark.parametrize("trials", [1, 2])
def test_the_fp32_restatement_is_inside_the_bounds(mul, F, E, trials):
    """torch fp32, natural order: the forward equals the rounded float64 result bit for bit, the two gradients stay
    inside their bounds at every stride (and at a longer T with buckets of 1, 5, 64 and 301 frames)."""
    w = {"dpre": 0.0, "daux": 0.0}
    for T_, strides in ((T, STRIDES), (301, (1, 5, 64, 400))):
        for stride in strides:
            pre, aux, dxs = R.inputs(B, K, trials, T_, F, E, mul, stride, seed=stride + 7)
            assert torch.equal(R.cond_fwd(pre, aux, mul, trials, stride, torch.float32),
                               R.cond_fwd(pre, aux, mul, trials, stride).float())
            ref, tol = R.cond_dpre(dxs, aux, mul, stride)
            w["dpre"] = max(w["dpre"], R.worst(R.cond_dpre(dxs, aux, mul, stride, torch.float32)[0], ref, tol))
            ref, tol = R.cond_daux(dxs, pre if mul else None, E, stride)
            w["daux"] = max(w["daux"], R.worst(R.cond_daux(dxs, pre if mul else None, E, stride, torch.float32)[0], ref, tol))
            assert R.outside(ref.float(), ref, tol) == 0
    print(f"fp32 restatement {'mul' if mul else 'cat'} trials={trials}: worst err/bound " + "  ".join(f"{k} {v:.3g}" for k, v in w.items()))


@pytest.mark.parametrize("mul,F,E", SHAPES)
@pytest.mark.parametrize("trials", [1, 2])
def test_planted_defects_fall_outside_the_bounds(mul, F, E, trials):
    """Each defect, planted in the float64 result and rounded to fp32, against the clean reference and its bound."""
    seen = set()
    for stride in STRIDES:
        pre, aux, dxs = R.inputs(B, K, trials, T, F, E, mul, stride, seed=100 + stride)
        Ta = R.frames_of(T, stride)
        xs = R.cond_fwd(pre, aux, mul, trials, stride).float()
        dpre, tol_p = R.cond_dpre(dxs, aux, mul, stride)
        daux, tol_a = R.cond_daux(dxs, pre if mul else None, E, stride)
        C = daux.shape[-1]
        for defect in R.DEFECTS:
            bad_x = R.cond_fwd(pre, aux, mul, trials, stride, defect=defect).float()
            bad_p = R.cond_dpre(dxs, aux, mul, stride, defect=defect)[0].float()
            bad_a = R.cond_daux(dxs, pre if mul else None, E, stride, defect=defect)[0].float()
            n_x = int((bad_x != xs).sum())
            n_p, n_a = R.outside(bad_p, dpre, tol_p), R.outside(bad_a, daux, tol_a)
            print(f"{'mul' if mul else 'cat'} trials={trials} stride={stride} {defect}: forward {n_x}/{xs.numel()} unequal, "
                  f"d(pre) {n_p}/{dpre.numel()}, d(aux) {n_a}/{daux.numel()} outside")
            changes_index = (defect == "mod_ta" and 1 < stride < T) or (defect == "rotate_time" and trials > 1)
            if changes_index:
                seen.add(defect)
                cols = xs.shape[-1] - (0 if mul else F)          # the columns that come from aux
                assert n_x > 0.3 * xs.numel() * cols / xs.shape[-1]
                assert n_a > 0.4 * daux.numel()
                assert (n_p > 0.3 * dpre.numel()) if mul else n_p == 0          # (d(pre) of cat does not read aux)
            elif defect in ("mod_ta", "rotate_time"):
                assert n_x == 0 and n_p == 0 and n_a == 0        # the same index: nothing may change
            elif defect == "drop_last_bucket":
                assert n_x == 0 and n_p == 0
                if T % stride:
                    seen.add(defect)
                    assert n_a == B * K * C and R.outside(bad_a[:, :, :Ta - 1], daux[:, :, :Ta - 1], tol_a[:, :, :Ta - 1]) == 0
                else:
                    assert n_a == 0
            else:                                                # no_clamp
                assert n_x == 0 and n_p == 0
                if Ta * stride > T:
                    seen.add(defect)
                    # every (b, s) whose blocks are not all the last flat block reads frames of a neighbour
                    assert n_a >= (B * K - 1) * C and R.outside(bad_a[:, :, :Ta - 1], daux[:, :, :Ta - 1], tol_a[:, :, :Ta - 1]) == 0
                else:
                    assert n_a == 0
    assert seen == set(R.DEFECTS) - ({"rotate_time"} if trials == 1 else set())


@pytest.mark.parametrize("combination", ["mul", "cat"])
@pytest.mark.parametrize("nap", [1, 2])
def test_time_constant_forward_equals_the_oracle(combination, nap):
    """framewise_reference.mask_estimator_forward with a time-constant 4-D aux, at strides 1, 4 and >= T, gives
    oracle.net.mask_estimator_forward on the 3-D aux exactly (logit and mask), with and without the speaker shuffle."""
    torch.manual_seed(3)
    Bn, Kn, Tn, idim, odim, units, projs = 2, 4, 9, 7, 6, 5, 6
    E = odim if combination == "mul" else 3
    first = odim if combination == "mul" else odim + E
    p = {}

    def rnnp_params(prefix, i, h, o):
        for sfx in ("", "_reverse"):
            p[prefix + "net.0.weight_ih_l0" + sfx] = torch.randn(4 * h, i, dtype=torch.float64) * 0.3
            p[prefix + "net.0.weight_hh_l0" + sfx] = torch.randn(4 * h, h, dtype=torch.float64) * 0.3
            p[prefix + "net.0.bias_ih_l0" + sfx] = torch.randn(4 * h, dtype=torch.float64) * 0.1
            p[prefix + "net.0.bias_hh_l0" + sfx] = torch.randn(4 * h, dtype=torch.float64) * 0.1
        p[prefix + "net.1.weight"] = torch.randn(o, 2 * h, dtype=torch.float64) * 0.3
        p[prefix + "net.1.bias"] = torch.randn(o, dtype=torch.float64) * 0.1

    ts_vad = Kn if nap > 1 else False
    rnnp_params("pre_net.", idim, units, odim)
    rnnp_params("post_net.birnn0.", first, units, projs)
    rnnp_params("post_net.birnn1.", projs, units, projs)
    rnnp_params("post_net.birnn2.", projs * (Kn if ts_vad else 1), units, projs)
    p["post_net.linear2.weight"] = torch.randn(odim * (Kn if ts_vad else 1), projs, dtype=torch.float64) * 0.3
    p["post_net.linear2.bias"] = torch.randn(odim * (Kn if ts_vad else 1), dtype=torch.float64) * 0.1
    xs = torch.randn(Bn, Tn, idim, dtype=torch.float64)
    a3 = torch.randn(Bn, Kn, E, dtype=torch.float64)
    kw = dict(odim=odim, combination=combination, ts_vad=ts_vad, num_averaged_permutations=nap, prefix="")
    for perm in (None, [np.random.RandomState(5 + b).permutation(Kn) for b in range(Bn)]):
        want = onet.mask_estimator_forward(p, xs, a3, random_speaker_order=perm is not None, perm=perm, **kw)
        for stride in (1, 4, Tn, Tn + 3):
            a4 = a3[:, :, None].expand(Bn, Kn, R.frames_of(Tn, stride), E)
            got = R.mask_estimator_forward(p, xs, a4, aux_stride=stride, perm=perm, **kw)
            assert torch.equal(got["logit"], want["logit"]) and torch.equal(got["mask"], want["mask"]), (stride, perm)
            assert got["embedding"].shape == a4.shape
        got3 = R.mask_estimator_forward(p, xs, a3, perm=perm, **kw)
        assert torch.equal(got3["logit"], want["logit"]) and torch.equal(got3["embedding"], want["embedding"])
    # time-varying: the rows really differ by frame, and a stride regroups them
    a4 = torch.randn(Bn, Kn, Tn, E, dtype=torch.float64)
    v = R.mask_estimator_forward(p, xs, a4, aux_stride=1, **kw)["logit"]
    c = R.mask_estimator_forward(p, xs, a4[:, :, :1].expand(-1, -1, Tn, -1), aux_stride=1, **kw)["logit"]
    assert float((v - c).abs().max()) > 1e-3
    with pytest.raises(AssertionError):
        R.mask_estimator_forward(p, xs, a4, aux_stride=2, **kw)
