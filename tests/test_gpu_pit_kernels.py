"""The pairwise-cost kernels of pit=True / MSE (csrc/elementwise.hip) through their C entry points on a real MI355X,
against tests/pit_reference.py (float64).

Pair cost: all terms are non-negative, so |C^ - C| <= r 2^-24 C with r the float32 roundings on the longest path of the
kernel's own reduction, counted from the code (``roundings`` below):
    the term             1 (e - t; p = 1)  or  2 (the rounded difference squared, the product fused into the add; p = 2)
    the lane's chain     PC_CHUNK / 256 = 32 adds (4 x 8 in the vector path, 32 in the scalar one)
    the wave tree        6
    the four waves       2            ((w0 + w1) + (w2 + w3))
    the chunk loop       nchunks      (tssep_pit_assign, in chunk order)
    the scale            2            (float(N), the division)
i.e. r = 43 + nchunks (p = 1), 44 + nchunks (p = 2); the matched sum adds K - 1.
Worst error / bound seen on the MI355X: 0.082 (K = 8, N = 16 392; 0.009 ... 0.082 over all 28 shapes, both p); the
backward's: 0.52 (p = 2, N = 255).

The assignment is pinned exactly on the cost matrix the device itself reports (permutation, float32 sum bit for bit);
on real data the planted permutation must come back, after the reference's own relative gap to the runner-up is
asserted to exceed 1e-3.  Backward: element-wise (coefficient roundings) 2^-24 + rel(sums), exactly 0 where e == t."""
import ctypes

import numpy as np
import pytest
import torch

import pit_reference as R

pytestmark = pytest.mark.gpu

CHUNK = 8192
T_ = torch.as_tensor


def roundings(p, N):
    return (1 if p == 1 else 2) + CHUNK // 256 + 6 + 2 + -(-N // CHUNK) + 2


# coefficient of the backward: p = 1: gout / (float(N) ln10 sums): ln10 as a float constant, two products, the division
# (4; MAE: the division alone); p = 2: the same on 2 gout (exact), times the rounded difference (+ 2)
COEF_ROUNDINGS = {1: 4, 2: 6}


def _signals(B, K, N, seed):
    g = np.random.RandomState(seed)
    return g.randn(B, K, N).astype(np.float32), g.randn(B, K, N).astype(np.float32)


def _forward(est, tgt, p, pit, log=False, diag_only=None):
    from tssep_amd import hip_ops as H
    part = H.pair_cost_fwd(est, tgt, p, diag_only=(not pit) if diag_only is None else diag_only)
    cost, perm, sums, loss = H.pit_assign(part, est.shape[-1], pit=pit, log=log)
    torch.cuda.synchronize()
    return part, cost.cpu().numpy(), perm.cpu().numpy(), sums.cpu().numpy(), loss.cpu().numpy()


@pytest.mark.parametrize("N", [1, 4, 255, 4099, 4100, 2 * CHUNK + 3, 2 * CHUNK + 8])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_pair_cost_against_float64(K, N):
    """B = 3; N below one vector, inside a chunk, past two chunks -- with N % 4 != 0 (scalar loads) and == 0 (16-byte
    loads); the full matrix and the diagonal-only pass; p = 1 and 2."""
    from tssep_amd import _lib
    e, t = _signals(3, K, N, seed=1000 * K + N)
    ec, tc = T_(e).cuda(), T_(t).cuda()
    assert _lib.lib().tssep_pair_cost_chunks(N) == -(-N // CHUNK)
    worst = 0.0
    for p in (1, 2):
        ref = R.pair_costs(e, t, p)
        r = roundings(p, N)
        part, cost, perm, sums, _ = _forward(ec, tc, p, pit=True)
        assert tuple(part.shape) == (3, -(-N // CHUNK), K, K)
        worst = max(worst, R.check_cost(cost, ref, r))
        R.check_assignment(cost, perm, sums, sums, True, False)
        _, dcost, dperm, dsums, _ = _forward(ec, tc, p, pit=False)
        eye = np.eye(K, dtype=bool)
        assert np.array_equal(dcost[:, eye], cost[:, eye]), "the diagonal-only pass is the full pass's diagonal"
        assert np.all(dcost[:, ~eye] == 0) and np.array_equal(dperm, np.tile(np.arange(K), (3, 1)))
        ref_diag = ref[:, eye].sum(-1)
        assert np.all(np.abs(dsums - ref_diag) <= (r + K - 1) * R.U * ref_diag)
    print(f"pair cost K={K} N={N}: worst error / bound {worst:.4f}")


def test_pair_cost_unaligned_base_takes_the_scalar_path():
    """N % 4 == 0 but the buffers start 4 bytes past a 16-byte boundary."""
    B, K, N = 2, 3, 520
    e, t = _signals(B, K, N, seed=5)
    buf_e, buf_t = torch.zeros(B * K * N + 1, device="cuda"), torch.zeros(B * K * N + 1, device="cuda")
    ec, tc = buf_e[1:].view(B, K, N), buf_t[1:].view(B, K, N)
    ec.copy_(T_(e)), tc.copy_(T_(t))
    assert ec.data_ptr() % 16 == 4 and ec.is_contiguous()
    for p in (1, 2):
        cost = _forward(ec, tc, p, pit=True)[1]
        R.check_cost(cost, R.pair_costs(e, t, p), roundings(p, N))
        aligned = _forward(T_(e).cuda(), T_(t).cuda(), p, pit=True)[1]
        R.check_cost(aligned, R.pair_costs(e, t, p), roundings(p, N))


def test_pair_cost_past_the_grid_cap():
    """B = 65 537 utterances (K = 2, N = 5): b shares the flat blockIdx.x, no 65 535 cap."""
    B, K, N = 65537, 2, 5
    e, t = _signals(B, K, N, seed=7)
    for p in (1, 2):
        _, cost, perm, sums, loss = _forward(T_(e).cuda(), T_(t).cuda(), p, pit=True, log=True)
        R.check_cost(cost, R.pair_costs(e, t, p), roundings(p, N))
        R.check_assignment(cost, perm, sums, loss, True, True)
        assert len(np.unique(perm, axis=0)) == 2


def _integer_cases(K):
    """Hand-made integer cost matrices (exact in float32) -> [B, K, K]."""
    ident = np.full((K, K), 10.0)
    ident[np.arange(K), np.arange(K)] = 1                     # the optimum is the first permutation
    last = np.full((K, K), 10.0)
    last[np.arange(K), K - 1 - np.arange(K)] = 1              # ... the last one, index K! - 1
    flat = np.full((K, K), 5.0)                               # all K! permutations tie
    rot = np.full((K, K), 10.0)                               # rotations by one and by two tie (K >= 3)
    for i in range(K):
        rot[i, (i + 1) % K] = rot[i, (i + 2) % K] = 1
    rng = np.random.RandomState(K)
    small = rng.randint(0, 3, size=(4, K, K)).astype(np.float64)      # few distinct values: many ties
    wide = rng.randint(0, 1000, size=(4, K, K)).astype(np.float64)
    return np.concatenate([np.stack([ident, last, flat, rot]), small, wide]).astype(np.float32)


@pytest.mark.parametrize("K", range(1, 9))
def test_assignment_on_integer_costs(K):
    from tssep_amd import hip_ops as H
    c = _integer_cases(K)
    want, want_sums = R.assign(c)
    table = R.permutation_table(K)
    assert want[0].tolist() == table[0].tolist() and want[1].tolist() == table[-1].tolist()
    assert want[2].tolist() == table[0].tolist() and want_sums[2] == 5 * K
    if K >= 3:
        assert want[3].tolist() == [(i + 1) % K for i in range(K)]
        s = R.permutation_sums(c[3:4])[0]
        assert (s == s.min()).sum() >= 2
    for pit in (True, False):
        cost, perm, sums, loss = H.pit_assign(T_(c).cuda()[:, None], 1, pit=pit, log=False)
        torch.cuda.synchronize()
        assert np.array_equal(cost.cpu().numpy(), c)
        R.check_assignment(c, perm.cpu().numpy(), sums.cpu().numpy(), loss.cpu().numpy(), pit, False)
        if pit:
            assert np.array_equal(perm.cpu().numpy(), want) and np.array_equal(sums.cpu().numpy(), want_sums)
        else:
            assert np.array_equal(perm.cpu().numpy(), np.tile(np.arange(K), (len(c), 1)))
            assert np.array_equal(sums.cpu().numpy(), c[:, np.arange(K), np.arange(K)].sum(-1))


def test_assignment_sums_chunks_in_order_and_scales():
    """part [B, 3, K, K] with N = 4: cost = ((p0 + p1) + p2) / 4 in float32."""
    from tssep_amd import hip_ops as H
    rng = np.random.RandomState(11)
    part = rng.rand(5, 3, 3, 3).astype(np.float32)
    cost, perm, sums, loss = H.pit_assign(T_(part).cuda(), 4, pit=True, log=True)
    want = ((part[:, 0] + part[:, 1]) + part[:, 2]) / np.float32(4)
    assert np.array_equal(cost.cpu().numpy(), want)
    R.check_assignment(want, perm.cpu().numpy(), sums.cpu().numpy(), loss.cpu().numpy(), True, True)


def test_nan_cost_reaches_the_loss():
    from tssep_amd import hip_ops as H
    c = _integer_cases(4)[4:6].copy()
    c[0, 2, 1] = np.nan
    _, perm, sums, loss = H.pit_assign(T_(c).cuda()[:, None], 1, pit=True, log=False)
    assert np.isnan(float(loss[0])) and np.isnan(float(sums[0])) and not np.isnan(float(loss[1]))
    assert sorted(perm[0].tolist()) == [0, 1, 2, 3]


@pytest.mark.parametrize("K", [2, 3, 8])
def test_assignment_on_real_data(K):
    """est[b, k] = tgt[b, q_b[k]] + 0.3 noise, N = 1000: the planted permutation is the unique optimum by a wide gap."""
    B, N = 3, 1000
    rng = np.random.RandomState(20 + K)
    tgt = rng.randn(B, K, N).astype(np.float32)
    q = np.stack([rng.permutation(K) for _ in range(B)])
    est = (np.take_along_axis(tgt, q[..., None], axis=1) + 0.3 * rng.randn(B, K, N)).astype(np.float32)
    for p, log in ((1, True), (1, False), (2, False)):
        ref = R.loss(est, tgt, p, log, pit=True)
        assert np.all(ref["gap"] > 1e-3), ref["gap"]
        assert np.array_equal(ref["perm"], q)
        _, cost, perm, sums, loss = _forward(T_(est).cuda(), T_(tgt).cuda(), p, pit=True, log=log)
        assert np.array_equal(perm, q)
        r = roundings(p, N)
        R.check_cost(cost, ref["cost"], r)
        R.check_assignment(cost, perm, sums, loss, True, log)
        assert np.all(np.abs(sums - ref["sums"]) <= (r + K - 1) * R.U * ref["sums"])


@pytest.mark.parametrize("p", [1, 2])
@pytest.mark.parametrize("N", [255, 4099])
def test_backward_against_float64(p, N):
    from tssep_amd import hip_ops as H
    B, K = 3, 3
    rng = np.random.RandomState(N + p)
    est, tgt = _signals(B, K, N, seed=N + p)
    q = np.array([[1, 2, 0], [2, 0, 1], [0, 2, 1]])
    gout = rng.randn(B).astype(np.float32)
    worst = 0.0
    for perm in (q, None):
        pm = q if perm is not None else np.tile(np.arange(K), (B, 1))
        e = est.copy()
        matched = np.take_along_axis(tgt, pm[..., None], axis=1)
        e[:, :, ::37] = matched[:, :, ::37]                       # samples where the estimate equals its target
        for log in (True, False):
            sums64 = np.take_along_axis(R.pair_costs(e, tgt, p), pm[..., None], axis=2)[..., 0].sum(-1)
            sums32 = sums64.astype(np.float32)                    # relative error <= 2^-24
            got = H.pair_loss_bwd(T_(e).cuda(), T_(tgt).cuda(), T_(perm.astype(np.int32)).cuda() if perm is not None else None,
                                  T_(sums32).cuda() if log else None, T_(gout).cuda(), p)
            torch.cuda.synchronize()
            worst = max(worst, R.check_backward(got.cpu().numpy(), e, tgt, pm, p, log, gout, COEF_ROUNDINGS[p],
                                                sums_rel=R.U if log else 0.0))
    print(f"backward p={p} N={N}: worst error / bound {worst:.4f}")


def test_backward_with_the_forward_sums():
    """sums as the forward leaves them: the bound widens by the cost bound (+ K - 1 for the matched sum)."""
    from tssep_amd import hip_ops as H
    B, K, N = 2, 4, 4099
    est, tgt = _signals(B, K, N, seed=9)
    ec, tc = T_(est).cuda(), T_(tgt).cuda()
    part = H.pair_cost_fwd(ec, tc, 1)
    _, perm, sums, _ = H.pit_assign(part, N, pit=True, log=True)
    got = H.pair_loss_bwd(ec, tc, perm, sums, torch.ones(B, device="cuda"), 1)
    R.check_backward(got.cpu().numpy(), est, tgt, perm.cpu().numpy(), 1, True, None, COEF_ROUNDINGS[1],
                     sums_rel=(roundings(1, N) + K - 1) * R.U)


def test_two_runs_are_bit_identical():
    e, t = _signals(3, 8, 2 * CHUNK + 3, seed=13)
    ec, tc = T_(e).cuda(), T_(t).cuda()
    for p in (1, 2):
        a = _forward(ec, tc, p, pit=True, log=True)
        b = _forward(ec, tc, p, pit=True, log=True)
        assert torch.equal(a[0], b[0])
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y)


def test_more_than_eight_speakers():
    """TSSEP_E_SHAPE (-1) from the C entry points, NotImplementedError from Python before any launch."""
    from tssep_amd import _lib, hip_ops as H
    L = _lib.lib()
    x = torch.zeros(1, 9, 16, device="cuda")
    part = torch.zeros(1, 1, 9, 9, device="cuda")
    perm = torch.zeros(1, 9, device="cuda", dtype=torch.int32)
    out = torch.zeros(16 * 9, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert L.tssep_pair_cost_fwd(P(x), P(x), 1, 9, 16, 1, 0, P(part), None) == -1
    assert L.tssep_pit_assign(P(part), 1, 9, 1, 16, 1, 0, None, P(perm), P(out), P(out), None) == -1
    assert L.tssep_pair_loss_bwd(P(x), P(x), None, None, P(out), 1, 9, 16, 1, P(out), None) == -1
    assert L.tssep_pair_cost_fwd(P(x), P(x), 1, 8, 16, 3, 0, P(part), None) == -1          # p is 1 or 2
    for fn in (lambda: H.pair_cost_fwd(x, x), lambda: H.pit_assign(part, 16), lambda: H.pair_loss_bwd(x, x, None, None, out[:1])):
        with pytest.raises(NotImplementedError):
            fn()
