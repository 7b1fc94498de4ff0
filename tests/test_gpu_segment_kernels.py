"""csrc/segments.hip on a real MI355X against tests/segments_reference.py: tssep_mask_activity bit for bit where float32
sums are exact and within the derived bound gamma_F elsewhere; tssep_activity_segments by exact equality of count and
table."""
import ctypes

import numpy as np
import pytest
import torch

import segments_reference as R

pytestmark = pytest.mark.gpu

CHUNK = 256                      # frames per block of the edge stage (SEG_BLOCK in csrc/segments.hip)
ACT_ROWS_PER_SWEEP = 2048 * 4    # rows one launch of the activity kernel covers before its waves stride (ACT_GRID_CAP)


def H():
    from tssep_amd import hip_ops
    return hip_ops


def exact_masks(K, M, T, F, seed):
    """multiples of 2^-10 in [0, 1]: with F <= 513 every partial sum is exact in float32, in any order"""
    rs = np.random.RandomState(seed)
    m = (rs.randint(0, 1025, size=(K, M, T, F)) / 1024.0).astype(np.float32)
    if M == 2:
        m[:, 1] = (rs.randint(512, 1025, size=(K, T, F)) / 1024.0).astype(np.float32) * np.float32(0.5) + np.float32(0.5)
    return m


@pytest.mark.parametrize("M", (1, 2))
@pytest.mark.parametrize("F", (1, 3, 4, 257, 513))
def test_activity_bit_for_bit_on_exact_sums(F, M):
    for K in (1, 3):
        for T in (1, 7, 257):
            m = exact_masks(K, M, T, F, seed=F + 10 * T + K)
            want = R.activity32_exact(m)
            got = H().mask_activity(torch.from_numpy(m).cuda())
            assert got.dtype == torch.float32 and got.shape == (K, T)
            g = got.cpu().numpy()
            assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), (
                K, M, T, F, float(np.abs(g.astype(np.float64) - want).max()))


@pytest.mark.parametrize("offset", (1, 2, 3))
def test_activity_bit_for_bit_on_rows_off_the_16_byte_grid(offset):
    """a contiguous tensor whose storage starts `offset` floats past a 16-byte boundary: the scalar head does the work"""
    K, M, T, F = 2, 2, 9, 513
    m = exact_masks(K, M, T, F, seed=offset)
    buf = torch.zeros(m.size + 8, dtype=torch.float32, device="cuda")
    view = buf[offset:offset + m.size].view(K, M, T, F)
    view.copy_(torch.from_numpy(m))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
    got = H().mask_activity(view).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.activity32_exact(m).view(np.uint32))


@pytest.mark.parametrize("shape", ((2, 2, 33, 513), (1, 1, 5, 1000), (3, 1, 3000, 5), (2, 1, 4, 4099)))
def test_activity_within_the_derived_bound_and_reproducible(shape):
    """|a32 - a64| <= gamma_F a64, gamma_F = F u / (1 - F u), u = 2^-24: the terms are non-negative, so any summation
    order obeys gamma_{F-1} and the division adds one rounding.  Derived, not measured.  (3, 1, 3000, 5): 9000 rows, more
    than one sweep of the capped grid."""
    K, M, T, F = shape
    if shape == (3, 1, 3000, 5):
        assert K * T > ACT_ROWS_PER_SWEEP
    rs = np.random.RandomState(F)
    m = (1.0 / (1.0 + np.exp(-3.0 * rs.randn(K, M, T, F)))).astype(np.float32)
    a64 = R.activity64(m)
    d = torch.from_numpy(m).cuda()
    one, two = H().mask_activity(d), H().mask_activity(d)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))
    err = np.abs(one.cpu().numpy().astype(np.float64) - a64)
    print(f"{shape}: max err / a64 = {float((err / a64).max()):.3e}, bound {R.gamma(F):.3e}")
    assert (err <= R.gamma(F) * a64).all()


def test_activity_of_float64_masks_is_that_of_their_float32_cast():
    m = exact_masks(2, 2, 5, 257, seed=4)
    got = H().mask_activity(torch.from_numpy(m.astype(np.float64)).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.activity32_exact(m).view(np.uint32))


def test_activity_refuses_bad_shapes_before_any_launch():
    from tssep_amd import _lib
    L = _lib.lib()
    x = torch.zeros(64, device="cuda")
    p = ctypes.c_void_p(x.data_ptr())
    for K, M, T, F in ((0, 1, 4, 4), (1, 0, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (-1, 1, 4, 4)):
        assert L.tssep_mask_activity(p, K, M, T, F, p, None) == -1
    assert L.tssep_mask_activity(None, 1, 1, 4, 4, p, None) == -5


# ------------------------------------------------------------------------------------------------- segmentation
WINDOWS = lambda T: ((1, 1), (3, 1), (1, 3), (5, 3), (3, 5), (2 * T + 1, 1), (81, 41))      # noqa: E731
T_CASES = (1, 2, 255, 256, 257, 2 * CHUNK + 3, 1025)      # 515: past two chunks plus the one-frame halo


def pool(T, dilation):
    a = np.concatenate([R.edge_rows(T, dilation), R.edge_rows(T, dilation, seed=1)[-4:]])
    assert a.shape[0] == 19, a.shape
    return a


@pytest.mark.parametrize("T", T_CASES)
def test_segments_equal_the_reference_exactly(T):
    """count and table, every window, min_frames in {1, 2, 8}, K in {1, 3, 19}; the reference decides on the same
    float32 activity.  K = 19: the whole pool; K = 3 and K = 1: every group of three rows and every row alone."""
    h = H()
    calls = 0
    for d, e in WINDOWS(T):
        a = pool(T, d)
        dev = torch.from_numpy(a).cuda()
        closed = R.closing(R.decide(a, 0.5), d, e)
        row_runs = [R.runs(row) for row in closed]
        groups = [list(range(19))] + [list(range(i, i + 3)) for i in range(0, 18, 3)] + [[i] for i in range(19)]
        for mf in (1, 2, 8):
            for rows in groups:
                want = np.asarray([(k, s, t) for k, i in enumerate(rows) for s, t in row_runs[i] if t - s >= mf],
                                  dtype=np.int32).reshape(-1, 3)
                sub = dev[rows[0]:rows[-1] + 1]
                buf, count = h.activity_segments(sub, 0.5, d, e, mf, return_count=True)
                assert buf.shape == (len(rows) * ((T + 1) // 2), 3) and buf.dtype == torch.int32
                msg = R.compare(int(count.item()), buf.cpu().numpy(), want)
                assert msg is None, (T, d, e, mf, rows, msg)
                calls += 1
        # the public form: a view cut to the count; the whole reference route on the pool
        tab = h.activity_segments(dev, 0.5, d, e, 2)
        want = R.segments(a, 0.5, d, e, 2)
        assert R.compare(tab.shape[0], tab.cpu().numpy(), want) is None, (T, d, e)
    assert calls == 7 * 3 * 26


def test_segments_fill_the_capacity_and_repeat_bit_for_bit():
    """every row alternating: K * ceil(T / 2) runs, the buffer is full to its last row; two calls, one table"""
    K, T = 19, 1025
    a = np.full((K, T), 0.25, np.float32)
    a[:, ::2] = 0.75
    dev = torch.from_numpy(a).cuda()
    one = H().activity_segments(dev)
    two = H().activity_segments(dev)
    assert one.shape == (K * 513, 3) and one.shape[0] == H().segments_capacity(K, T)
    assert torch.equal(one, two)
    assert R.compare(one.shape[0], one.cpu().numpy(), R.segments(a)) is None
    assert H().activity_segments(dev, min_frames=2).shape == (0, 3)
    assert H().activity_segments(dev, dilation=3).cpu().tolist() == [[k, 0, T] for k in range(K)]


def test_threshold_is_strict_and_in_float32():
    thr = 0.3                                              # not a float32: compared as float32(0.3)
    t32 = np.float32(thr)
    a = np.array([[t32, np.nextafter(t32, np.float32(1)), np.nextafter(t32, np.float32(0)), np.nan, 1.0]], np.float32)
    tab = H().activity_segments(torch.from_numpy(a).cuda(), threshold=thr)
    assert tab.cpu().tolist() == [[0, 1, 2], [0, 4, 5]] == R.segments(a, thr).tolist()


def test_bad_parameters_are_refused_on_the_host_and_by_the_library():
    from tssep_amd import _lib
    h, L = H(), _lib.lib()
    a = torch.zeros(2, 16, device="cuda")
    for bad in (dict(dilation=2), dict(dilation=0), dict(erosion=4), dict(erosion=-3), dict(min_frames=0)):
        with pytest.raises(ValueError):
            h.activity_segments(a, **bad)
    cap = h.segments_capacity(2, 16)
    table = torch.full((cap, 3), -1, dtype=torch.int32, device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    ws = torch.zeros(9 * cap + 16, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for K, T, d, e, mf in ((0, 16, 1, 1, 1), (2, 0, 1, 1, 1), (2, 16, 2, 1, 1), (2, 16, 1, 0, 1), (2, 16, 1, 1, 0),
                           (2, 16, -1, 1, 1)):
        assert L.tssep_activity_segments(p(a), K, T, 0.5, d, e, mf, p(table), p(count), p(ws), None) == -1
    torch.cuda.synchronize()
    assert int(count.item()) == -1 and bool((table == -1).all())          # nothing was launched
