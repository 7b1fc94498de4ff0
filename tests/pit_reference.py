"""float64 restatement of the pairwise-cost losses (LogMAE, MAE, MSE with and without pit), written for this
repository's tests (padertorch's pit_loss is not a dependency; the semantics are pinned in DESIGN.md 4.10):

    C[b, i, j] = mean_n |est[b, i, n] - tgt[b, j, n]|^p                     (p = 1: MAE / LogMAE, p = 2: MSE)
    perm[b]    = the permutation minimising sum_i C[b, i, perm(i)]; the sum in float32 in ascending i, ties to the
                 first permutation in itertools.permutations(range(K)) order; pit=False: the identity
    sums[b]    = sum_i C[b, i, perm[b, i]],   loss[b] = log10(sums[b]) (LogMAE) or sums[b]

and the checkers the CPU and the GPU tests share.  perm[b, i] is the TARGET row matched to estimate row i."""
import itertools

import numpy as np
import torch

U = 2.0 ** -24            # unit roundoff of float32


def pair_costs(est, tgt, p):
    """est, tgt [B, K, N] (any float dtype) -> float64 C [B, K, K]."""
    e = torch.as_tensor(np.asarray(est), dtype=torch.float64)
    t = torch.as_tensor(np.asarray(tgt), dtype=torch.float64)
    out = torch.empty(e.shape[0], e.shape[1], e.shape[1], dtype=torch.float64)
    for i in range(e.shape[1]):                                    # (row by row: [B, K, N] temporaries only)
        d = (e[:, i, None, :] - t).abs()
        out[:, i] = (d if p == 1 else d * d).mean(-1)
    return out.numpy()


def permutation_table(K):
    return np.array(list(itertools.permutations(range(K))), dtype=np.int64).reshape(-1, K)


def permutation_sums(cost, dtype=np.float32):
    """cost [B, K, K] -> [B, K!]: sum_i cost[b, i, perm(i)] for every permutation, accumulated in `dtype` in ascending i."""
    cost = np.asarray(cost).astype(dtype)
    table = permutation_table(cost.shape[-1])
    s = cost[:, 0, table[:, 0]]
    for i in range(1, cost.shape[-1]):
        s = (s + cost[:, i, table[:, i]]).astype(dtype)
    return s


def assign(cost, pit=True, last_on_tie=False):
    """Brute force over all permutations -> (perm int64 [B, K], sums float32 [B]).  np.argmin takes the FIRST minimum
    (and the first NaN): the tie rule.  last_on_tie: the reversed rule, a planted defect for the tests."""
    cost = np.asarray(cost)
    K = cost.shape[-1]
    if not pit:
        s = permutation_sums(cost)[:, 0]
        return np.tile(np.arange(K), (cost.shape[0], 1)), s
    s = permutation_sums(cost)
    idx = s.shape[1] - 1 - np.argmin(s[:, ::-1], axis=1) if last_on_tie else np.argmin(s, axis=1)
    return permutation_table(K)[idx], s[np.arange(len(idx)), idx]


def relative_gap(cost):
    """(runner-up - optimum) / optimum of the permutation sums, in float64, per utterance (inf for K = 1)."""
    s = np.sort(permutation_sums(cost, np.float64), axis=1)
    return (s[:, 1] - s[:, 0]) / s[:, 0] if s.shape[1] > 1 else np.full(len(s), np.inf)


def inverse(perm):
    perm = np.asarray(perm)
    inv = np.empty_like(perm)
    np.put_along_axis(inv, perm, np.broadcast_to(np.arange(perm.shape[-1]), perm.shape), axis=-1)
    return inv


def loss(est, tgt, p=1, log=False, pit=False):
    """-> dict(cost float64 [B,K,K], perm [B,K], sums float64 [B], loss float64 [B], gap [B]).  The assignment is taken on
    the float32 rounding of the float64 costs, as the rule pins it; sums / loss are then the float64 values of it."""
    C = pair_costs(est, tgt, p)
    perm, _ = assign(C.astype(np.float32), pit)
    sums = np.take_along_axis(C, perm[..., None], axis=2)[..., 0].sum(-1)
    return dict(cost=C, perm=perm, sums=sums, loss=np.log10(sums) if log else sums, gap=relative_gap(C))


def grad(est, tgt, perm, p=1, log=False, gout=None):
    """d(sum_b gout[b] loss[b]) / d(est) by float64 autograd, the permutation held fixed -> float64 [B, K, N]."""
    e = torch.tensor(np.asarray(est), dtype=torch.float64, requires_grad=True)
    t = torch.as_tensor(np.asarray(tgt), dtype=torch.float64)
    idx = torch.as_tensor(np.asarray(perm), dtype=torch.int64)[..., None].expand_as(t)
    d = (e - torch.gather(t, 1, idx)).abs()                        # row i against tgt[perm[i]]
    s = (d if p == 1 else d * d).mean(-1).sum(-1)
    val = torch.log10(s) if log else s
    g = torch.ones_like(val) if gout is None else torch.as_tensor(np.asarray(gout), dtype=torch.float64)
    (val * g).sum().backward()
    return e.grad.numpy()


# ------------------------------------------------------------------------------------------------ checkers
def check_cost(got, ref, roundings):
    """|got - ref| <= roundings * 2^-24 * ref (all terms of a cost are non-negative).  -> worst error / bound."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    bound = roundings * U * ref
    err = np.abs(got - ref)
    bad = err > bound
    assert not bad.any(), f"cost: {int(bad.sum())} entries outside {roundings} roundings, worst " \
                          f"{float((err[bad] / np.maximum(bound[bad], 1e-300)).max()):.3g} x the bound"
    return float((err / np.maximum(bound, 1e-300)).max())


def check_assignment(cost32, perm, sums, loss_, pit, log):
    """The assignment on the float32 cost matrix the device itself reported is pinned exactly: the permutation, the
    float32 sum bit for bit, and the loss to the accuracy of log10f."""
    want_perm, want_sums = assign(cost32, pit)
    perm, sums, loss_ = np.asarray(perm), np.asarray(sums), np.asarray(loss_)
    assert np.array_equal(perm, want_perm), ("permutation", perm[(perm != want_perm).any(-1)][:4],
                                             want_perm[(perm != want_perm).any(-1)][:4])
    assert np.array_equal(sums.view(np.uint32), want_sums.astype(np.float32).view(np.uint32)), ("sums", sums, want_sums)
    want = np.log10(want_sums.astype(np.float64)) if log else want_sums.astype(np.float64)
    assert np.all(np.abs(loss_ - want) <= 4 * U * np.maximum(np.abs(want), 1)), ("loss", loss_, want)


def check_backward(got, est, tgt, perm, p, log, gout, coef_roundings, sums_rel):
    """Element-wise |got - ref| <= (coef_roundings * 2^-24 + sums_rel) |ref| against the float64 gradient, and exactly 0
    where the estimate equals its matched target.  -> worst error / bound."""
    ref = grad(est, tgt, perm, p, log, gout)
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    matched = np.take_along_axis(np.asarray(tgt), np.asarray(perm)[..., None], axis=1)
    zero = np.asarray(est) == matched
    assert np.all(got[zero] == 0), "a nonzero gradient where est == tgt"
    bound = (coef_roundings * U + sums_rel) * np.abs(ref)
    err = np.abs(got - ref)
    bad = err > bound
    assert not bad.any(), f"gradient: {int(bad.sum())} of {bad.size} elements outside the bound"
    return float((err / np.maximum(bound, 1e-300)).max())
