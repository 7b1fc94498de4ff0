"""The four FreqMSE entry points (tssep_amd/csrc/specloss.hip) on a real MI355X against the float64 references of
tests/spectral_reference.py, within the bounds derived there -- element by element for the gradients.

Shapes: one element; F = 513 over three chunks; K = 8 (64 accumulators per lane); F = 65 (one bin past a wave); two
frames of five bins for three utterances; a T over eleven chunks; B K T = 9 600 frames at F = 3, past the 8 192 frames a
sweep of the backward's capped grid covers (frame_grid: 2 048 workgroups of four waves, one wave per frame).  Every shape
runs diag_only and pit, a given permutation (utterance 0: a rotation by one, perm != its inverse for K >= 3), bt_major 0 and
1, complex64 and complex128 estimates; the inputs carry an exact tie E == S over one whole frame and logit rows at +-30
(spectral_reference.make_inputs).  Forwards run twice and must give the same bits; perm and loss of tssep_pit_assign on
the partials must be the brute-force choice (its gap to the second best is asserted on the CPU, test_spectral_reference)."""
import pytest
import torch

import spectral_reference as R
from test_spectral_reference import GPU_CASES

pytestmark = pytest.mark.gpu

FRAME_SWEEP = 2048 * 4              # specloss.hip frame_grid: frames per sweep of mask_specmse_bwd_kernel
GRID_SWEEP = 4096 * 256             # common.h grid_for: elements per sweep of specmse_bwd_kernel
DEV = "cuda"


def H():
    from tssep_amd import hip_ops
    return hip_ops


def chunk_frames():
    from tssep_amd import _lib
    return 2 ** 20 // _lib.lib().tssep_specmse_chunks(2 ** 20)


def test_the_cases_cross_chunks_and_the_grid_cap():
    from tssep_amd import _lib
    shapes = [s for s, _ in GPU_CASES]
    assert any(_lib.lib().tssep_specmse_chunks(T) >= 3 and Fb == 513 for _, _, T, Fb in shapes)
    assert any(_lib.lib().tssep_specmse_chunks(T) >= 3 and T % chunk_frames() for _, _, T, _ in shapes)
    assert any(B * K * T > FRAME_SWEEP and Fb <= 8 for B, K, T, Fb in shapes)


@pytest.fixture(scope="module", params=GPU_CASES, ids=[str(s) for s, _ in GPU_CASES])
def case(request):
    """inputs on the device and the float64 references they share (computed once, never written)"""
    shape, seed = request.param
    d = R.make_inputs(*shape, seed, device=DEV)
    d["lg"], d["o128"], d["S"] = d["logit"].double(), d["obs"].to(torch.complex128), d["tgt"].to(torch.complex128)
    d["E"], d["e_E"] = R.ref_estimate(d["lg"], d["o128"])
    d["ct"] = chunk_frames()
    return d


def _finish(part, Fb, pit):
    cost, perm, sums, loss = H().pit_assign(part, Fb, pit=pit, log=False)
    torch.cuda.synchronize()
    return cost, perm, sums, loss


def _check_forward(d, launch, E, e_E, what):
    from tssep_amd import _lib
    B, K, T, Fb = d["B"], d["K"], d["T"], d["F"]
    for pit in (False, True):
        part = launch(diag_only=not pit)
        again = launch(diag_only=not pit)
        assert tuple(part.shape) == (B, _lib.lib().tssep_specmse_chunks(T), K, K)
        assert torch.equal(part, again), f"{what}: two runs of the forward differ"
        cost, perm, sums, loss = _finish(part, Fb, pit)
        ref, tol = R.ref_costs(E, d["S"], e_E, ct=d["ct"], diag_only=not pit)
        R.within(cost, ref, tol, f"{what} cost pit={pit}")
        if not pit:
            eye = torch.eye(K, dtype=torch.bool, device=DEV)
            assert not bool(part[..., ~eye].any()), "diag_only writes the other entries as 0"
        rl, t_loss, rp, gap = R.ref_loss(ref, tol, pit)
        assert bool((gap >= 100 * t_loss).all())
        assert torch.equal(perm, rp), (what, pit, perm.tolist(), rp.tolist())
        R.within(loss, rl, t_loss, f"{what} loss pit={pit}")
        assert torch.equal(loss, sums)


def test_fused_forward(case):
    d = case
    _check_forward(d, lambda diag_only: H().mask_specmse_fwd(d["logit"], d["obs"], d["tgt"], diag_only=diag_only),
                   d["E"], d["e_E"], "fused")


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_generic_forward(case, dtype):
    d = case
    est = d["est"] if dtype == "c64" else d["est128"]
    _check_forward(d, lambda diag_only: H().specmse_fwd(est, d["tgt"], diag_only=diag_only),
                   est.to(torch.complex128), None, dtype)


def test_diag_only_is_the_full_pass_diagonal(case):
    d = case
    K = d["K"]
    eye = torch.eye(K, dtype=torch.bool, device=DEV)
    full = H().mask_specmse_fwd(d["logit"], d["obs"], d["tgt"], diag_only=False)
    diag = H().mask_specmse_fwd(d["logit"], d["obs"], d["tgt"], diag_only=True)
    assert torch.equal(full[..., eye], diag[..., eye])


def _pit_perm(d, E, e_E):
    ref, tol = R.ref_costs(E, d["S"], e_E, ct=d["ct"])
    return R.ref_loss(ref, tol, True)[2]


def test_fused_backward(case):
    d = case
    B, K, T, Fb = d["B"], d["K"], d["T"], d["F"]
    for name, perm in (("identity", None), ("given", d["perm"]), ("pit", _pit_perm(d, d["E"], d["e_E"]))):
        ref, tol = R.ref_mask_bwd(d["lg"], d["o128"], d["S"], perm, d["gout"])
        got = H().mask_specmse_bwd(d["logit"], d["obs"], d["tgt"], perm, d["gout"])
        torch.cuda.synchronize()
        assert tuple(got.shape) == (B, K, T, Fb)
        R.within(got, ref, tol, f"dlogit perm={name}")
        for iperm in (None, d["iperm"]):
            bt = H().mask_specmse_bwd(d["logit"], d["obs"], d["tgt"], perm, d["gout"], iperm=iperm, bt_major=True)
            torch.cuda.synchronize()
            assert tuple(bt.shape) == (B * T, K * Fb)
            assert torch.equal(bt, R.bt_store(got, iperm)), f"bt_major store, perm={name}, iperm={iperm is not None}"
    # the saturated rows: exactly 0 where 1 - m rounds to 0, finite everywhere
    assert bool(torch.isfinite(got).all())
    if (B, K, T) != (1, 1, 1):
        assert not bool(got[0, 0, 0].any())


@pytest.mark.parametrize("dtype", ["c64", "c128"])
def test_generic_backward(case, dtype):
    d = case
    f64 = dtype == "c128"
    est = d["est128"] if f64 else d["est"]
    E = est.to(torch.complex128)
    for name, perm in (("identity", None), ("given", d["perm"]), ("pit", _pit_perm(d, E, None))):
        ref, tol = R.ref_spec_bwd(E, d["S"], perm, d["gout"], f64)
        got = H().specmse_bwd(est, d["tgt"], perm, d["gout"])
        torch.cuda.synchronize()
        assert got.dtype == est.dtype and got.shape == est.shape
        R.within(torch.view_as_real(got), ref, tol, f"dest {dtype} perm={name}")
    tie = torch.view_as_real(H().specmse_bwd(est, d["tgt"], None, d["gout"]))[0, 0, 0]
    assert not bool(tie.any()), "E == S over a whole frame: its gradient is exactly 0"


def test_generic_backward_past_the_grid_cap():
    """complex64, 3 x 4 x 171 x 513 = 1 052 676 elements: past one sweep of the capped grid (1 048 576)"""
    B, K, T, Fb = 3, 4, 171, 513
    assert B * K * T * Fb > GRID_SWEEP
    g = torch.Generator(device=DEV).manual_seed(9)
    est = torch.randn(B, K, T, Fb, device=DEV, generator=g, dtype=torch.complex64)
    tgt = torch.randn(B, K, T, Fb, device=DEV, generator=g, dtype=torch.complex64)
    gout = torch.rand(B, device=DEV, generator=g) + 0.5
    perm = ((torch.arange(K)[None] + 1 + torch.arange(B)[:, None]) % K).int().to(DEV)
    ref, tol = R.ref_spec_bwd(est.to(torch.complex128), tgt.to(torch.complex128), perm, gout, False)
    R.within(torch.view_as_real(H().specmse_bwd(est, tgt, perm, gout)), ref, tol, "dest past the grid cap")


def test_entry_points_refuse_what_the_header_says():
    from tssep_amd import _lib
    from tssep_amd.hip_ops import _p
    L = _lib.lib()
    x = torch.zeros(4096, device=DEV)
    i = torch.zeros(64, device=DEV, dtype=torch.int32)
    for B, K, T, Fb in ((1, 9, 2, 3), (0, 2, 2, 3), (1, 0, 2, 3), (1, 2, 0, 3), (1, 2, 2, 0)):
        assert L.tssep_mask_specmse_fwd(_p(x), _p(x), _p(x), B, K, T, Fb, 0, _p(x), None) == -1
        assert L.tssep_mask_specmse_bwd(_p(x), _p(x), _p(x), _p(i), _p(x), B, K, T, Fb, None, 0, _p(x), None) == -1
        for f64 in (0, 1):
            assert L.tssep_specmse_fwd(_p(x), f64, _p(x), B, K, T, Fb, 1, _p(x), None) == -1
            assert L.tssep_specmse_bwd(_p(x), f64, _p(x), None, _p(x), B, K, T, Fb, _p(x), None) == -1
    assert L.tssep_mask_specmse_fwd(None, _p(x), _p(x), 1, 1, 1, 1, 0, _p(x), None) == -5
    torch.cuda.synchronize()


def test_autograd_functions(case):
    """Fn.spec_mse / Fn.mask_spec_mse: the wrappers' loss, permutation and gradients are the entry points' (bit for bit)"""
    from tssep_amd import functional as Fn
    d = case
    for pit in (False, True):
        logit = d["logit"].clone().requires_grad_()
        loss, perm = Fn.mask_spec_mse(logit, d["obs"], d["tgt"], pit=pit)
        (loss * d["gout"]).sum().backward()
        part = H().mask_specmse_fwd(d["logit"], d["obs"], d["tgt"], diag_only=not pit)
        _, p2, _, l2 = _finish(part, d["F"], pit)
        assert torch.equal(loss.detach(), l2) and torch.equal(perm, p2) and not perm.requires_grad
        assert torch.equal(logit.grad, H().mask_specmse_bwd(d["logit"], d["obs"], d["tgt"], p2 if pit else None, d["gout"]))
        for est0 in (d["est"], d["est128"]):
            est = est0.clone().requires_grad_()
            loss, perm = Fn.spec_mse(est, d["tgt"], pit=pit)
            (loss * d["gout"]).sum().backward()
            _, p2, _, l2 = _finish(H().specmse_fwd(est0, d["tgt"], diag_only=not pit), d["F"], pit)
            assert torch.equal(loss.detach(), l2) and torch.equal(perm, p2)
            assert est.grad.dtype == est0.dtype
            assert torch.equal(est.grad, H().specmse_bwd(est0, d["tgt"], p2 if pit else None, d["gout"]))
