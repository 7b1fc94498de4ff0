"""CPU checks of tests/pit_reference.py, the float64 reference the GPU tests of the pairwise-cost losses compare with:
known answers (the MSE doctest of tssep/train/loss.py:183-190 and the MAE one of :194-216), the relabelling identity of
a permutation-invariant loss, and the checkers against planted defects -- a checker that accepts a transposed cost
matrix or an inverted permutation would let the kernels do the same."""
import itertools

import numpy as np
import pytest
import torch

import pit_reference as R


def _doctest_pair():
    torch.manual_seed(0)
    target = torch.rand(2, 10000)
    estimate = target + 0.5 * torch.rand(2, 10000)
    return estimate[None].numpy(), target[None].numpy()


@pytest.fixture(scope="module")
def planted():
    """est[b, k] = tgt[b, q[b, k]] + 0.3 noise, K = 3 with a 3-cycle among the q (its inverse differs from it)."""
    rng = np.random.RandomState(3)
    B, K, N = 3, 3, 400
    tgt = rng.randn(B, K, N).astype(np.float32)
    q = np.array([[1, 2, 0], [2, 0, 1], [0, 2, 1]])
    est = (np.take_along_axis(tgt, q[..., None], axis=1) + 0.3 * rng.randn(B, K, N)).astype(np.float32)
    return est, tgt, q


def test_known_answers():
    e, t = _doctest_pair()
    assert float(R.loss(e, t, p=2)["loss"][0]) == pytest.approx(0.1673, abs=5e-5)
    assert float(R.loss(e, t, p=1)["loss"][0]) == pytest.approx(0.5018, abs=5e-5)
    assert float(R.loss(e, t, p=1, log=True)["loss"][0]) == pytest.approx(np.log10(0.5018), abs=5e-5)
    # (not the mean over all elements, which is half of it)
    assert float(((e - t).astype(np.float64) ** 2).mean()) == pytest.approx(0.0837, abs=5e-5)
    for p in (1, 2):                                     # the estimate is nearest its own target: pit changes nothing
        a, b = R.loss(e, t, p=p), R.loss(e, t, p=p, pit=True)
        assert np.array_equal(b["perm"], [[0, 1]]) and a["loss"][0] == b["loss"][0]


def test_permutation_order_is_itertools():
    for K in (1, 2, 3, 4):
        assert R.permutation_table(K).tolist() == [list(p) for p in itertools.permutations(range(K))]
    assert R.permutation_table(8).shape == (40320, 8)
    q = np.array([[2, 0, 3, 1]])
    assert np.array_equal(np.take_along_axis(q, R.inverse(q), axis=1), [[0, 1, 2, 3]])


@pytest.mark.parametrize("p,log", [(1, True), (1, False), (2, False)])
def test_relabelled_targets_give_the_plain_loss(planted, p, log):
    """pit=True on tgt[:, q] equals pit=False on tgt, with perm == inverse(q)."""
    est, tgt, q = planted
    est = (tgt + 0.3 * np.random.RandomState(4).randn(*tgt.shape)).astype(np.float32)       # est[k] belongs to tgt[k]
    plain = R.loss(est, tgt, p, log, pit=False)
    relabelled = R.loss(est, np.take_along_axis(tgt, q[..., None], axis=1), p, log, pit=True)
    assert np.array_equal(relabelled["perm"], R.inverse(q))
    np.testing.assert_allclose(relabelled["loss"], plain["loss"], rtol=1e-14)
    assert np.all(relabelled["gap"] > 1e-3)


def test_planted_permutation_is_found_and_gradient_follows_it(planted):
    est, tgt, q = planted
    for p, log in ((1, True), (1, False), (2, False)):
        r = R.loss(est, tgt, p, log, pit=True)
        assert np.array_equal(r["perm"], q) and np.all(r["gap"] > 1e-3)
        g = R.grad(est, tgt, r["perm"], p, log)
        # closed forms of the issue: sign(e - t_perm) / (N ln10 sums) and 2 (e - t_perm) / N
        d = est.astype(np.float64) - np.take_along_axis(tgt, q[..., None], axis=1)
        N = est.shape[-1]
        want = np.sign(d) / N / (np.log(10) * r["sums"][:, None, None] if log else 1) if p == 1 else 2 * d / N
        np.testing.assert_allclose(g, want, rtol=1e-12, atol=1e-18)


def test_tie_rule():
    flat = np.full((1, 3, 3), 5.0, dtype=np.float32)
    assert R.assign(flat)[0].tolist() == [[0, 1, 2]]
    # rotations by one and by two are both optimal: the earlier one in itertools order, (1, 2, 0), wins
    c = np.full((1, 3, 3), 10.0, dtype=np.float32)
    for i in range(3):
        c[0, i, (i + 1) % 3] = c[0, i, (i + 2) % 3] = 1
    assert R.assign(c)[0].tolist() == [[1, 2, 0]]
    assert R.assign(c, last_on_tie=True)[0].tolist() == [[2, 0, 1]]
    assert R.assign(c, pit=False)[0].tolist() == [[0, 1, 2]] and float(R.assign(c, pit=False)[1][0]) == 30.0


def test_float32_sum_order_decides_ties():
    """The sums compared are float32 sums in ascending i: 2^24 + 1 + 1 stays 2^24, 1 + 1 + 2^24 does not."""
    big = 2.0 ** 24
    c = np.full((1, 3, 3), 4 * big, dtype=np.float32)
    c[0, 0, 0], c[0, 1, 1], c[0, 2, 2] = big, 1, 1                    # identity: (2^24 + 1) + 1 -> 2^24 in float32
    c[0, 0, 1], c[0, 1, 2], c[0, 2, 0] = 1, 1, big                    # (1, 2, 0): (1 + 1) + 2^24 = 2^24 + 2
    perm, s = R.assign(c)
    assert perm.tolist() == [[0, 1, 2]] and float(s[0]) == big
    assert R.permutation_sums(c, np.float64)[0, 0] == R.permutation_sums(c, np.float64)[0, 3] == big + 2


# ------------------------------------------------------------------------------ the checkers catch planted defects
def _device_like(est, tgt, p, log, pit=True):
    r = R.loss(est, tgt, p, log, pit)
    cost32 = r["cost"].astype(np.float32)
    perm, sums = R.assign(cost32, pit)
    return cost32, perm, sums, (np.log10(sums) if log else sums).astype(np.float32), r


def test_checkers_accept_the_rounded_reference(planted):
    est, tgt, _ = planted
    for p, log in ((1, True), (2, False)):
        cost32, perm, sums, loss_, r = _device_like(est, tgt, p, log)
        assert R.check_cost(cost32, r["cost"], roundings=1) <= 1
        R.check_assignment(cost32, perm, sums, loss_, True, log)
        g = R.grad(est, tgt, perm, p, log).astype(np.float32)
        assert R.check_backward(g, est, tgt, perm, p, log, None, coef_roundings=1, sums_rel=0) <= 1


def test_checker_catches_transposed_cost(planted):
    est, tgt, _ = planted
    cost32, _, _, _, r = _device_like(est, tgt, 1, False)
    with pytest.raises(AssertionError, match="cost"):
        R.check_cost(cost32.transpose(0, 2, 1), r["cost"], roundings=50)


def test_checker_catches_permutation_applied_to_est(planted):
    """min_perm sum_i |est[perm(i)] - tgt[i]| has the same value but reports the inverse permutation."""
    est, tgt, q = planted
    cost32, perm, sums, loss_, _ = _device_like(est, tgt, 1, True)
    wrong = R.assign(cost32.transpose(0, 2, 1))[0]
    assert np.array_equal(wrong, R.inverse(q)) and not np.array_equal(wrong, perm)
    with pytest.raises(AssertionError, match="permutation"):
        R.check_assignment(cost32, wrong, sums, loss_, True, True)


def test_checker_catches_inverse_permutation_in_backward(planted):
    est, tgt, q = planted
    for p in (1, 2):
        g = R.grad(est, tgt, R.inverse(q), p, False).astype(np.float32)
        with pytest.raises(AssertionError, match="gradient"):
            R.check_backward(g, est, tgt, q, p, False, None, coef_roundings=8, sums_rel=1e-6)


def test_checker_catches_reversed_tie_rule():
    c = np.full((2, 4, 4), 3.0, dtype=np.float32)
    perm, sums = R.assign(c, last_on_tie=True)
    assert perm.tolist() == [[3, 2, 1, 0]] * 2
    with pytest.raises(AssertionError, match="permutation"):
        R.check_assignment(c, perm, sums, sums, True, False)


def test_checker_catches_nonzero_gradient_at_equal_samples(planted):
    est, tgt, q = planted
    est = est.copy()
    est[0, 1, 7] = tgt[0, q[0, 1], 7]
    g = R.grad(est, tgt, q, 1, False).astype(np.float32)
    assert g[0, 1, 7] == 0
    R.check_backward(g, est, tgt, q, 1, False, None, coef_roundings=1, sums_rel=0)
    g[0, 1, 7] = 1e-30
    with pytest.raises(AssertionError, match="nonzero"):
        R.check_backward(g, est, tgt, q, 1, False, None, coef_roundings=1, sums_rel=0)
