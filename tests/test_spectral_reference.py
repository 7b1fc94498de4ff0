"""The float64 references and element-wise bounds of the FreqMSE kernels (tests/spectral_reference.py), tested without a
GPU and never compared with the code under test: they equal torch autograd in float64 (complex128), pit by brute force
over itertools.permutations; the fp32 rounding of their own outputs lies inside every bound; the same outputs with nine
defects planted fall outside.  And the condition the pit comparisons of the GPU files rest on is asserted here for every
shape and seed they use: the best and the second-best permutation sums are at least 100 forward bounds apart in every
utterance, so the expected permutation is never a coin toss."""
import itertools

import pytest
import torch

import spectral_reference as R
from spectral_reference import U, outside

CT = 4                      # a nominal chunk length for the CPU checks (the GPU file reads the kernel's own)
GPU_CASES = [(s, 100 + i) for i, s in enumerate(R.SHAPES)] + [((1, 3, 41, 7), 120), ((2, 8, 600, 3), 121)]


def _c128(d):
    return d["logit"].double(), d["obs"].to(torch.complex128), d["tgt"].to(torch.complex128)


@pytest.fixture(scope="module")
def case():
    d = R.make_inputs(2, 3, 9, 513, seed=101)
    d["lg"], d["o128"], d["S"] = _c128(d)
    return d


def test_references_equal_autograd_in_float64():
    for (B, K, T, Fb), seed in GPU_CASES[:5]:
        d = R.make_inputs(B, K, T, Fb, seed)
        lg, o, S = _c128(d)
        lg.requires_grad_()
        E = o[:, None] * torch.sigmoid(lg)
        E.retain_grad()
        diff = (E[:, :, None] - S[:, None]).abs() ** 2
        cost = diff.mean(-1).sum(-1)                                              # [B, K, K]
        rc, _ = R.ref_costs(E.detach(), S)
        assert float((rc - cost.detach()).abs().max()) <= 1e-12 * float(cost.detach().abs().max())
        rd, _ = R.ref_costs(E.detach(), S, diag_only=True)
        assert torch.equal(rd, rc * torch.eye(K, dtype=torch.float64))
        for pit in (False, True):
            perms = list(itertools.permutations(range(K))) if pit else [tuple(range(K))]
            onehot = torch.nn.functional.one_hot(torch.tensor(perms), K).double()                 # [nperm, K, K]
            sums = torch.einsum("bij,pij->bp", cost, onehot)                                      # [B, nperm]
            loss, best = sums.min(-1)
            rl, _, rp, _ = R.ref_loss(rc, torch.zeros_like(rc), pit)
            assert float((rl - loss.detach()).abs().max()) <= 1e-12 * float(loss.detach().abs().max())
            assert rp.tolist() == [list(perms[int(i)]) for i in best]
            (dl,) = torch.autograd.grad((loss * d["gout"].double()).sum(), lg, retain_graph=True)
            (dE,) = torch.autograd.grad((loss * d["gout"].double()).sum(), E, retain_graph=True)
            perm = rp if pit else None
            ref, _ = R.ref_mask_bwd(lg.detach(), o, S, perm, d["gout"])
            assert float((ref - dl).abs().max()) <= 1e-11 * max(float(dl.abs().max()), 1e-300), (B, K, T, Fb, pit)
            ref, _ = R.ref_spec_bwd(E.detach(), S, perm, d["gout"], True)
            assert float((ref - torch.view_as_real(dE)).abs().max()) <= 1e-12 * float(dE.abs().max())
        # a permutation that is given (the rotation of make_inputs): autograd of the loss with that pairing
        Sp = S[torch.arange(B)[:, None], d["perm"].long()]
        given = ((E - Sp).abs() ** 2).mean(-1).sum((-1, -2))
        (dl,) = torch.autograd.grad((given * d["gout"].double()).sum(), lg)
        ref, _ = R.ref_mask_bwd(lg.detach(), o, S, d["perm"], d["gout"])
        assert float((ref - dl).abs().max()) <= 1e-11 * max(float(dl.abs().max()), 1e-300)


def test_doctest_value_of_the_reference():
    """loss.py:258-269: 0.1673 for real [2, 10000] inputs -- the mean over the last axis, the sum over the other"""
    torch.manual_seed(0)
    target = torch.rand((2, 10000))
    estimate = target + 0.5 * torch.rand((2, 10000))
    E = estimate.to(torch.complex128)[None, :, None]                              # [B = 1, K = 2, T = 1, F]
    cost, _ = R.ref_costs(E, target.to(torch.complex128)[None, :, None])
    loss, _, _, _ = R.ref_loss(cost, torch.zeros_like(cost), False)
    assert abs(float(loss[0]) - 0.1673) < 5e-5


@pytest.mark.parametrize("shape,seed", GPU_CASES, ids=[str(s) for s, _ in GPU_CASES])
def test_best_permutation_is_clear_at_every_gpu_shape(shape, seed):
    """the condition of the pit comparisons: gap >= 100 forward bounds, for the fused and for both generic estimates"""
    d = R.make_inputs(*shape, seed)
    lg, o, S = _c128(d)
    E, e_E = R.ref_estimate(lg, o)
    for name, est, err in (("fused", E, e_E), ("c64", d["est"].to(torch.complex128), None), ("c128", d["est128"], None)):
        cost, tol = R.ref_costs(est, S, err, ct=1)                                # (ct = 1: the longest chunk sum)
        _, t_loss, perm, gap = R.ref_loss(cost, tol, True)
        assert bool((gap >= 100 * t_loss).all()), (name, shape, gap.tolist(), t_loss.tolist())
    if shape[1] >= 3:
        assert bool((d["perm"][0] != torch.argsort(d["perm"][0].long()).int()).any())
        assert bool((d["iperm"] != d["perm"]).any())


def test_clean_rounding_is_inside_every_bound(case):
    d = case
    E, e_E = R.ref_estimate(d["lg"], d["o128"])
    counts = {}
    for diag in (False, True):
        cost, tol = R.ref_costs(E, d["S"], e_E, ct=CT, diag_only=diag)
        counts[f"cost diag={diag}"] = outside(cost.float(), cost, tol)
        loss, t_loss, _, _ = R.ref_loss(cost, tol, not diag)
        counts[f"loss pit={not diag}"] = outside(loss.float(), loss, t_loss)
    for perm in (None, d["perm"]):
        ref, tol = R.ref_mask_bwd(d["lg"], d["o128"], d["S"], perm, d["gout"])
        counts[f"dlogit perm={perm is not None}"] = outside(ref.float(), ref, tol)
        ref, tol = R.ref_spec_bwd(d["est"].to(torch.complex128), d["S"], perm, d["gout"], False)
        counts[f"dest perm={perm is not None}"] = outside(ref.float(), ref, tol)
    for k, v in counts.items():
        print(f"clean fp32 rounding outside the bound  {k}: {v}")
    assert not any(counts.values()), counts


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_falls_outside_the_bounds(case, defect):
    d = case
    K = d["K"]
    E, e_E = R.ref_estimate(d["lg"], d["o128"])
    hits = {}
    if defect in ("mean_over_tf", "last_bin_dropped", "obs_of_utterance_0", "target_of_speaker_0"):      # forward defects
        cost, tol = R.ref_costs(E, d["S"], e_E, ct=CT)
        bad, _ = R.ref_costs(R.ref_estimate(d["lg"], d["o128"], defect)[0], d["S"], e_E, ct=CT, defect=defect)
        hits["cost"] = outside(bad.float(), cost, tol)
        assert outside(cost.float(), cost, tol) == 0 and hits["cost"] > 0, hits
    ref_l, tol_l = R.ref_mask_bwd(d["lg"], d["o128"], d["S"], d["perm"], d["gout"])
    bad, _ = R.ref_mask_bwd(d["lg"], d["o128"], d["S"], d["perm"], d["gout"], iperm=d["iperm"], defect=defect)
    assert outside(ref_l.float(), ref_l, tol_l) == 0
    hits["dlogit"] = outside(bad.float(), ref_l, tol_l)
    assert hits["dlogit"] > 0, hits
    if defect != "no_conj" and defect != "obs_of_utterance_0":                    # the generic pair has neither
        Eg = d["est"].to(torch.complex128)
        ref, tol = R.ref_spec_bwd(Eg, d["S"], d["perm"], d["gout"], False)
        bad, _ = R.ref_spec_bwd(Eg, d["S"], d["perm"], d["gout"], False, iperm=d["iperm"], defect=defect)
        hits["dest"] = outside(bad.float(), ref, tol)
        assert hits["dest"] > 0, hits
    if defect == "iperm_for_perm":                # and the store: perm where iperm belongs is another arrangement
        clean = R.bt_load(R.bt_store(ref_l.float(), d["iperm"]), d["iperm"], K)
        got = R.bt_load(R.bt_store(ref_l.float(), d["perm"]), d["iperm"], K)
        assert torch.equal(clean, ref_l.float()) and outside(got, ref_l, tol_l) > 0
    print(f"planted {defect}: elements outside the bound {hits}")


def test_chain_counts_the_kernel_order():
    # F = 513, T = 253, four frames per chunk: 2 * 9 lane adds + 6 + 2 + 64 chunk adds + the division
    assert R.chain(513, 253, 4) == 18 + 6 + 2 + 64 + 1
    assert R.chain(1, 1, 4) == 2 + 6 + 2 + 1 + 1
    assert U == 2.0 ** -24
