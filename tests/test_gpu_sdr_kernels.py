"""The SDR / SI-SDR kernels (csrc/sdrloss.hip) through their entry points on a real MI355X, against tests/sdr_reference.py
(float64) within the bounds derived there from the kernel's stated float32 rounding count (32: the per-lane chain; all
behind it is float64).  The assignment and the loss are tssep_pit_assign's and are pinned exactly on the float32 cost
matrix the device itself reports (tests/pit_reference.check_assignment).
Worst error / bound seen on the MI355X: statistics 0.047 (K = 8, N = 4; 0.003 ... 0.047 over the 28 shapes, both passes);
values 0.023 over the four planted levels x four modes (the bound itself: 6e-5 dB at -10 and 0 dB, 3e-3 dB at 20 dB, 0.33 dB
at 40 dB without sdr_max, at K = 3, N = 16 392); backward 0.013."""
import ctypes

import numpy as np
import pytest
import torch

import pit_reference as PR
import sdr_reference as R

pytestmark = pytest.mark.gpu

CHUNK = R.CHUNK
T_ = torch.as_tensor
MODES = [(True, None), (True, 30.0), (False, None), (False, 30.0)]
LEVELS = (-10, 0, 20, 40)


def _signals(B, K, N, seed):
    g = np.random.RandomState(seed)
    return g.randn(B, K, N).astype(np.float32), g.randn(B, K, N).astype(np.float32)


def _stats(ec, tc, diag_only):
    from tssep_amd import hip_ops as H
    part = H.sdr_stats_fwd(ec, tc, diag_only=diag_only)
    torch.cuda.synchronize()
    return part


def _forward(ec, tc, scale_invariant, sdr_max, eps, pit):
    """-> part, stat, value, cost, perm, sums, loss as numpy arrays (part stays a tensor)."""
    from tssep_amd import hip_ops as H
    K = ec.shape[1]
    part = H.sdr_stats_fwd(ec, tc, diag_only=not pit)
    stat, value, cost = H.sdr_cost(part, K, scale_invariant, sdr_max, eps, diag_only=not pit)
    _, perm, sums, loss = H.pit_assign(cost[:, None], 1, pit=pit, log=False, want_cost=False)
    torch.cuda.synchronize()
    return (part,) + tuple(x.cpu().numpy() for x in (stat, value, cost, perm, sums, loss))


@pytest.mark.parametrize("N", [1, 4, 255, 4099, 4100, 2 * CHUNK + 3, 2 * CHUNK + 8])
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_statistics_against_float64(K, N):
    """B = 3; N below one vector, inside a chunk, past two chunks -- with N % 4 != 0 (scalar loads) and == 0 (16-byte
    loads); the full matrix and the diagonal-only pass; then the chunk sums of tssep_sdr_cost."""
    from tssep_amd import _lib, hip_ops as H
    e, t = _signals(3, K, N, seed=1000 * K + N)
    ec, tc = T_(e).cuda(), T_(t).cuda()
    L = _lib.lib()
    nchunks = -(-N // CHUNK)
    assert L.tssep_sdr_chunks(N) == nchunks
    assert L.tssep_sdr_workspace_bytes(3, K, N) == 3 * nchunks * (K * K + 2 * K) * 8
    st = R.stats(e, t)
    worst = 0.0
    for diag_only in (False, True):
        part = _stats(ec, tc, diag_only)
        assert tuple(part.shape) == (3, nchunks, K * K + 2 * K) and part.dtype == torch.float64
        worst = max(worst, R.check_stats(part.cpu().numpy().sum(1), st, diag_only=diag_only))
        stat = H.sdr_cost(part, K, diag_only=diag_only)[0]
        p = part.cpu().numpy()
        want = p[:, 0].copy()
        for c in range(1, nchunks):
            want += p[:, c]
        assert np.array_equal(stat.cpu().numpy(), want), "stat is the partials summed in chunk order, in float64"
    print(f"sdr statistics K={K} N={N}: worst error / bound {worst:.4f}")


def test_unaligned_base_takes_the_scalar_path():
    """N % 4 == 0 but the buffers start 4 bytes past a 16-byte boundary: statistics and backward."""
    from tssep_amd import hip_ops as H
    B, K, N = 2, 3, 520
    e, t = _signals(B, K, N, seed=5)
    buf_e, buf_t = torch.zeros(B * K * N + 1, device="cuda"), torch.zeros(B * K * N + 1, device="cuda")
    ec, tc = buf_e[1:].view(B, K, N), buf_t[1:].view(B, K, N)
    ec.copy_(T_(e)), tc.copy_(T_(t))
    assert ec.data_ptr() % 16 == 4 and ec.is_contiguous()
    st = R.stats(e, t)
    R.check_stats(_stats(ec, tc, False).cpu().numpy().sum(1), st)
    R.check_stats(_stats(T_(e).cuda(), T_(t).cuda(), False).cpu().numpy().sum(1), st)
    stat = T_(R.flat_stats(st)).cuda()
    gout = T_(np.array([1.0, -2.0], dtype=np.float32)).cuda()
    got = H.sdr_bwd(ec, tc, None, stat, gout, True, None, 1e-8)
    aligned = H.sdr_bwd(T_(e).cuda(), T_(t).cuda(), None, stat, gout, True, None, 1e-8)
    torch.cuda.synchronize()
    assert torch.equal(got, aligned)


def test_past_the_grid_cap():
    """B x nchunks = 65 537 workgroups of the statistics (K = 2, N = 5) and B x K rows of the backward: b shares the flat
    blockIdx.x, no 65 535 cap."""
    from tssep_amd import hip_ops as H
    B, K, N = 65537, 2, 5
    e, t = _signals(B, K, N, seed=7)
    ec, tc = T_(e).cuda(), T_(t).cuda()
    part, stat, value, cost, perm, sums, loss = _forward(ec, tc, True, None, 1e-8, True)
    st = R.stats(e, t)
    R.check_stats(stat, st)
    PR.check_assignment(cost, perm, sums, loss, True, False)
    assert len(np.unique(perm, axis=0)) == 2
    gout = torch.ones(B, device="cuda")
    got = H.sdr_bwd(ec, tc, T_(perm).cuda(), T_(stat).cuda(), gout, True, None, 1e-8)
    torch.cuda.synchronize()
    tail = slice(B - 4, B)                                     # the last rows sit past block 65 535
    R.check_backward(got.cpu().numpy()[tail], e[tail], t[tail], perm[tail], True, None, 1e-8, np.ones(4))


@pytest.mark.parametrize("scale_invariant,sdr_max", MODES)
@pytest.mark.parametrize("level", LEVELS)
def test_values_at_planted_levels(scale_invariant, sdr_max, level):
    """K = 3, N = 2 CHUNK + 8: estimates at -10 ... 40 dB of their own targets; the full matrix and the diagonal."""
    B, K, N = 2, 3, 2 * CHUNK + 8
    e, t = R.planted(B, K, N, level, seed=level + 300)
    ec, tc = T_(e).cuda(), T_(t).cuda()
    eps = 1e-8
    ref = R.loss(e, t, scale_invariant, sdr_max, eps, pit=True)
    want_level = level if sdr_max is None else -10 * np.log10(10 ** (-level / 10) + 10 ** (-sdr_max / 10))
    assert np.all(np.abs(ref["values"] - want_level) < 1e-2), (ref["values"], want_level)
    worst = 0.0
    for pit in (True, False):
        _, stat, value, cost, perm, sums, loss = _forward(ec, tc, scale_invariant, sdr_max, eps, pit)
        worst = max(worst, R.check_values(value, cost, ref, diag_only=not pit))
        PR.check_assignment(cost, perm, sums, loss, pit, False)
        assert np.array_equal(perm, np.tile(np.arange(K), (B, 1)))
        # (K matched costs, each within its bound; K - 1 float32 adds of them)
        bound = (np.diagonal(ref["dvalue"], axis1=1, axis2=2).sum(-1) / K
                 + (K + 1) * R.U * np.abs(np.diagonal(ref["cost"], axis1=1, axis2=2)).sum(-1))
        assert np.all(np.abs(loss - ref["loss"]) <= bound), (loss, ref["loss"], bound)
    diag = np.diagonal(ref["dvalue"], axis1=1, axis2=2)
    print(f"sdr values si={scale_invariant} sdr_max={sdr_max} level={level}: worst error / bound {worst:.4f}, "
          f"bound {diag.max():.3g} dB")


SKIPPED = []


@pytest.mark.parametrize("K", [2, 3, 8])
def test_assignment_on_permuted_targets(K):
    """est[b, k] = tgt[b, q_b[k]] + noise at 10 dB, N = 1000: the planted permutation is the optimum by more than the
    bound of the permutation sums, in every mode."""
    B, N = 3, 1000
    rng = np.random.RandomState(20 + K)
    e0, tgt = R.planted(B, K, N, 10.0, seed=40 + K)
    q = np.stack([rng.permutation(K) for _ in range(B)])
    est = np.take_along_axis(e0, q[..., None], axis=1)
    for scale_invariant, sdr_max in MODES:
        ref = R.loss(est, tgt, scale_invariant, sdr_max, 1e-8, pit=True)
        sum_bound = K * (ref["dvalue"].max() / K + R.U * np.abs(ref["cost"]).max()) + K * R.U * np.abs(ref["cost"]).sum((1, 2))
        if not (np.array_equal(ref["perm"], q) and np.all(ref["gap"] > 2 * sum_bound)):
            SKIPPED.append((K, scale_invariant, sdr_max))
            continue
        _, stat, value, cost, perm, sums, loss = _forward(T_(est).cuda(), T_(tgt).cuda(), scale_invariant, sdr_max, 1e-8, True)
        assert np.array_equal(perm, q)
        R.check_values(value, cost, ref)
        PR.check_assignment(cost, perm, sums, loss, True, False)
        from tssep_amd import hip_ops as H
        values, hperm = H.sdr(T_(est).cuda(), T_(tgt).cuda(), scale_invariant, sdr_max, 1e-8, pit=True)
        assert np.array_equal(hperm.cpu().numpy(), q) and not values.requires_grad
        assert np.array_equal(values.cpu().numpy(), np.take_along_axis(value, q[..., None], axis=2)[..., 0])
        assert np.all(np.abs(values.cpu().numpy() - ref["values"]) <= np.take_along_axis(ref["dvalue"], q[..., None], axis=2)[..., 0])


def test_no_assignment_case_was_skipped():
    assert SKIPPED == []


@pytest.mark.parametrize("scale_invariant,sdr_max", MODES)
@pytest.mark.parametrize("N", [255, 4099, CHUNK + 4])
def test_backward_against_float64(scale_invariant, sdr_max, N):
    """perm given and NULL, stat as the forward leaves it; levels 0 and 20 dB in one batch."""
    from tssep_amd import hip_ops as H
    B, K = 2, 3
    e0, t0 = R.planted(1, K, N, 0.0, seed=N)
    e1, t1 = R.planted(1, K, N, 20.0, seed=N + 1)
    e, tgt = np.concatenate([e0, e1]), np.concatenate([t0, t1])
    q = np.array([[1, 2, 0], [2, 0, 1]])
    gout = np.array([0.7, -1.3], dtype=np.float32)
    eps = 1e-8
    worst = 0.0
    for perm in (q, None):
        pm = q if perm is not None else np.tile(np.arange(K), (B, 1))
        t = np.take_along_axis(tgt, PR.inverse(pm)[..., None], axis=1)          # est row i belongs to t row pm[b, i]
        ec, tc = T_(e).cuda(), T_(t).cuda()
        stat = H.sdr_cost(H.sdr_stats_fwd(ec, tc), K, scale_invariant, sdr_max, eps)[0]
        got = H.sdr_bwd(ec, tc, T_(perm.astype(np.int32)).cuda() if perm is not None else None, stat, T_(gout).cuda(),
                        scale_invariant, sdr_max, eps)
        torch.cuda.synchronize()
        worst = max(worst, R.check_backward(got.cpu().numpy(), e, t, pm, scale_invariant, sdr_max, eps, gout))
    print(f"sdr backward si={scale_invariant} sdr_max={sdr_max} N={N}: worst error / bound {worst:.4f}")


def test_corrupt_permutation_falls_back_to_the_identity():
    from tssep_amd import hip_ops as H
    e, t = _signals(2, 3, 260, seed=3)
    ec, tc = T_(e).cuda(), T_(t).cuda()
    stat = H.sdr_cost(H.sdr_stats_fwd(ec, tc), 3)[0]
    gout = torch.ones(2, device="cuda")
    bad = T_(np.array([[7, -1, 100], [3, 1 << 30, -5]], dtype=np.int32)).cuda()
    assert torch.equal(H.sdr_bwd(ec, tc, bad, stat, gout), H.sdr_bwd(ec, tc, None, stat, gout))


def test_silent_rows():
    """A silent target: 10 log10(eps / (a + eps)), finite, and the gradient is P e with P > 0; both silent: 0 dB and a
    zero gradient; a silent estimate of a live target: finite."""
    from tssep_amd import hip_ops as H
    B, K, N = 1, 3, 1028
    e, t = _signals(B, K, N, seed=11)
    t[0, 0] = 0                                     # silent target, live estimate
    e[0, 1] = t[0, 1] = 0                           # both silent
    e[0, 2] = 0                                     # silent estimate, live target
    eps = 1e-8
    for scale_invariant, sdr_max in MODES:
        ref = R.loss(e, t, scale_invariant, sdr_max, eps, pit=False)
        _, stat, value, cost, perm, sums, loss = _forward(T_(e).cuda(), T_(t).cuda(), scale_invariant, sdr_max, eps, False)
        assert np.all(np.isfinite(value)) and np.all(np.isfinite(loss))
        R.check_values(value, cost, ref, diag_only=True)
        a = ref["stats"]["a"][0, 0]
        assert abs(value[0, 0, 0] - 10 * np.log10(eps / (a + eps))) <= ref["dvalue"][0, 0, 0]
        assert value[0, 1, 1] == 0
        got = H.sdr_bwd(T_(e).cuda(), T_(t).cuda(), None, T_(stat).cuda(), torch.ones(B, device="cuda"),
                        scale_invariant, sdr_max, eps).cpu().numpy()
        assert np.all(np.isfinite(got)) and np.all(got[0, 0] * e[0, 0] >= 0) and np.abs(got[0, 0]).max() > 0
        assert np.all(got[0, 1] == 0)
        R.check_backward(got, e, t, np.arange(K)[None], scale_invariant, sdr_max, eps, np.ones(B))


def test_nan_sample_reaches_the_loss():
    e, t = _signals(2, 3, 4100, seed=13)
    e[0, 1, 4000] = np.nan
    for scale_invariant, sdr_max in MODES:
        for pit in (True, False):
            _, stat, value, cost, perm, sums, loss = _forward(T_(e).cuda(), T_(t).cuda(), scale_invariant, sdr_max, 1e-8, pit)
            assert np.isnan(loss[0]) and np.isfinite(loss[1]), (scale_invariant, sdr_max, pit, loss)
            assert sorted(perm[0].tolist()) == [0, 1, 2]


def test_two_runs_are_bit_identical():
    from tssep_amd import hip_ops as H
    e, t = _signals(3, 8, 2 * CHUNK + 3, seed=13)
    ec, tc = T_(e).cuda(), T_(t).cuda()
    a = _forward(ec, tc, True, 30.0, 1e-8, True)
    b = _forward(ec, tc, True, 30.0, 1e-8, True)
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x.view(np.uint64 if x.dtype == np.float64 else np.uint32),
                              y.view(np.uint64 if y.dtype == np.float64 else np.uint32))
    gout = torch.ones(3, device="cuda")
    ga = H.sdr_bwd(ec, tc, T_(a[4]).cuda(), T_(a[1]).cuda(), gout, True, 30.0, 1e-8)
    gb = H.sdr_bwd(ec, tc, T_(a[4]).cuda(), T_(a[1]).cuda(), gout, True, 30.0, 1e-8)
    assert torch.equal(ga, gb)


def test_more_than_eight_speakers():
    """TSSEP_E_SHAPE (-1) from the C entry points; eps <= 0 is TSSEP_E_UNSUPPORTED (-3)."""
    from tssep_amd import _lib
    L = _lib.lib()
    x = torch.zeros(1, 9, 16, device="cuda")
    part = torch.zeros(1, 1, 99, device="cuda", dtype=torch.float64)
    out = torch.zeros(16 * 9, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    assert L.tssep_sdr_stats_fwd(P(x), P(x), 1, 9, 16, 0, P(part), None) == -1
    assert L.tssep_sdr_cost(P(part), 1, 9, 1, 1, 0.0, 1e-8, 0, P(part), P(out), P(out), None) == -1
    assert L.tssep_sdr_bwd(P(x), P(x), None, P(part), P(out), 1, 9, 16, 1, 0.0, 1e-8, P(out), None) == -1
    assert L.tssep_sdr_workspace_bytes(1, 9, 16) == 0 and L.tssep_sdr_workspace_bytes(1, 8, 16) == 80 * 8
    assert L.tssep_sdr_cost(P(part), 1, 8, 1, 1, 0.0, 0.0, 0, P(part), P(out), P(out), None) == -3
    assert L.tssep_sdr_bwd(P(x), P(x), None, P(part), P(out), 1, 8, 16, 1, 0.0, -1.0, P(out), None) == -3
