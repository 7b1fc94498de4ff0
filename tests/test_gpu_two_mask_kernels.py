"""tssep_mask_map_fwd / tssep_mask_map_bwd (the fused two-mask tail, elementwise.hip) element by element against the
float64 reference of tests/test_two_mask_reference.py, within its bounds (derived there).

Shapes: B = 2, T = 3, K in {3, 4}, M in {1, 2, 3}, F in {5, 65}, two settings at F = 513; every combination of raw layout
(speakers in rows / in columns), resolution ('tf' / 't'), trials in {1, 2, K} on the ts_vad rows, permutations off / on
and dlogit NULL / given.  At M = 1 the forward is bit-identical to tssep_logit_map_fwd and the mask head's sigmoid.  One
case runs 2.5 sweeps of the capped grid.  The inputs are drawn on the CPU (test_two_mask_reference.make_inputs), so the
reference file's CPU checks see the values the kernels see."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_two_mask_reference as R  # noqa: E402
from test_gpu_streaming_kernels import ROW_SWEEP, within  # noqa: E402

DEV = "cuda"


def H():
    from tssep_amd import hip_ops
    return hip_ops


def L():
    from tssep_amd import _lib
    return _lib.lib()


def forward(d):
    B, trials, K, M, T, F, Fr, spk_rows = R.geometry(d)
    return H().mask_map_fwd(d["raw"], d["perm"], d["iperm"], B, trials, K, M, T, F, Fr, spk_rows)


def backward(d, mask):
    B, trials, K, M, T, F, Fr, spk_rows = R.geometry(d)
    return H().mask_map_bwd(d["dmask"], mask, d["dlogit"], d["perm"], d["iperm"], B, trials, K, M, T, F, Fr, spk_rows)


def check_setting(s):
    d = R.case_of(s, device=DEV)
    geo = R.geometry(d)
    B, trials, K, M, T, F, Fr, spk_rows = geo
    tag = R.setting_id(s)
    logit, mask = forward(d)
    assert tuple(logit.shape) == tuple(mask.shape) == (B, K, M, T, F)
    raw64 = d["raw"].double()
    ref, _ = R.ref_fwd(raw64, d["iperm"], *geo)
    within(logit, ref, R.logit_tol(raw64, d["iperm"], *geo), f"logit {tag}")
    sig, tol = R.mask_tol(logit)
    within(mask, sig, tol, f"mask {tag}")
    draw = backward(d, mask)
    dref, dtol = R.ref_bwd(d["dmask"].double(), logit, None if d["dlogit"] is None else d["dlogit"].double(), d["perm"], *geo)
    assert draw.numel() == dref.numel() == B * trials * K * M * T * Fr
    within(draw, dref, dtol, f"draw {tag}")
    if M == 1:
        h = H()
        assert torch.equal(logit.view(B, K, T, F), h.logit_map_fwd(d["raw"], d["perm"], d["iperm"], B, trials, K, T, F, Fr,
                                                                   spk_rows)), f"logit != logit_map_fwd {tag}"
        head, _ = h.maskhead_fwd(logit.view(B, K, T, F), torch.zeros(B, T, F, device=DEV, dtype=torch.complex64))
        assert torch.equal(mask.view(B, K, T, F), head), f"mask != maskhead_fwd {tag}"
    return logit, ref


@pytest.mark.parametrize("group", R.GROUPS, ids=R.group_id)
def test_fused_pair_against_float64(group):
    """Every setting of the group: logit (exact at trials == 1, else (trials - 1) U mean |raw|, trials = 3 included), mask
    and draw within their bounds, the M = 1 bit-identities."""
    for s in R.settings_of(group):
        check_setting(s)


def test_past_the_grid_cap():
    """F = 5, M = 2: 2.5 sweeps of the capped grid.  Both launches walk one wave per run of F floats, four waves per
    workgroup, and grid_for caps the grid at 4096 workgroups: ROW_SWEEP = 16 384 runs per sweep (elementwise.hip).  The
    forward has B K M T runs, the backward B trials T K M; compared utterance slice by slice."""
    K, M, T, F = 3, 2, 3, 5
    B = -(-int(2.5 * ROW_SWEEP) // (K * M * T))
    assert ROW_SWEEP == 4096 * 4 and B * K * M * T >= 2.5 * ROW_SWEEP
    for tf, trials, spk_rows in ((True, 2, 0), (False, 1, 1)):
        d = R.make_inputs(B, K, M, T, F, F if tf else 1, trials, spk_rows, perm=True, seed=900 + trials, device=DEV)
        geo = R.geometry(d)
        logit, mask = forward(d)
        draw = backward(d, mask).view(B, -1)
        raw = d["raw"].view(B, -1)
        for b0 in range(0, B, 512):
            b1 = min(B, b0 + 512)
            g = (b1 - b0,) + geo[1:]
            pm, ipm = d["perm"][b0:b1], d["iperm"][b0:b1]
            r64 = raw[b0:b1].reshape(-1).double()
            ref, _ = R.ref_fwd(r64, ipm, *g)
            within(logit[b0:b1], ref, R.logit_tol(r64, ipm, *g), f"logit past the cap, utterances {b0}:{b1}")
            sig, tol = R.mask_tol(logit[b0:b1])
            within(mask[b0:b1], sig, tol, f"mask past the cap, utterances {b0}:{b1}")
            dref, dtol = R.ref_bwd(d["dmask"][b0:b1].double(), logit[b0:b1], d["dlogit"][b0:b1].double(), pm, *g)
            within(draw[b0:b1].reshape(-1), dref, dtol, f"draw past the cap, utterances {b0}:{b1}")


def test_error_codes_and_no_launch():
    """TSSEP_E_SHAPE (-1) for M = 0, TSSEP_E_UNSUPPORTED (-3) for speakers in rows with trials > 1, TSSEP_E_NULL (-5) for
    one of perm / iperm alone; nothing is launched: the outputs keep their fill."""
    lib = L()
    B, K, M, T, F = 2, 3, 2, 3, 5
    n = B * K * M * T * F
    raw = torch.randn(2 * n, device=DEV)
    out = [torch.full((n,), 7.0, device=DEV) for _ in range(3)]
    draw = torch.full((2 * n,), 7.0, device=DEV)
    pm = torch.zeros(B, K, dtype=torch.int32, device=DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731

    def fwd(perm, iperm, trials, M_, spk_rows):
        return lib.tssep_mask_map_fwd(p(raw), p(perm), p(iperm), B, trials, K, M_, T, F, F, spk_rows, p(out[0]), p(out[1]), st)

    def bwd(perm, iperm, trials, M_, spk_rows):
        return lib.tssep_mask_map_bwd(p(out[2]), p(out[2]), None, p(perm), p(iperm), B, trials, K, M_, T, F, F, spk_rows,
                                      p(draw), st)
    for call in (fwd, bwd):
        assert call(None, None, 1, 0, 0) == -1
        assert call(None, None, 1, -2, 1) == -1
        assert call(None, None, 2, M, 1) == -3
        assert call(pm, None, 1, M, 0) == -5
        assert call(None, pm, 1, M, 0) == -5
    assert lib.tssep_mask_map_fwd(None, None, None, B, 1, K, M, T, F, F, 0, p(out[0]), p(out[1]), st) == -5
    assert lib.tssep_mask_map_bwd(p(out[2]), None, None, None, None, B, 1, K, M, T, F, F, 0, p(draw), st) == -5
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in out) and bool((draw == 7.0).all())
    assert fwd(None, None, 1, M, 0) == 0 and bwd(None, None, 1, M, 0) == 0        # the same calls with good arguments launch
    torch.cuda.synchronize()
    assert not bool((out[0] == 7.0).any()) and not bool((draw[:n] == 7.0).all())
