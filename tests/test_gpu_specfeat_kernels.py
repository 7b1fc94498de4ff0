"""tssep_specfeat_fwd / tssep_specfeat_causal_fwd (csrc/specfeat.hip) through hip_ops on a real MI355X, against
the float64 definitions and within the derived bounds of tests/specfeat_reference.py.  Shapes B in {1, 3} x T in {1, 2, 70}
x F in {1, 5, 513, 1025}: magnitudes over nine decades, a silent utterance, a silent frame.  Every output buffer is filled
with NaN before the call, so an element the kernel skips fails the bound and a column it must not touch is still NaN.
The worst error / bound of each kind is printed (`-s`) -- the figures of DESIGN 4.23."""
import numpy as np
import pytest
import torch

import specfeat_reference as R

pytestmark = pytest.mark.gpu

SHAPES = [(B, T, F) for B in R.BS for T in R.TS for F in R.FS]
_CACHE = {}


def case(B, T, F):
    """the input and its float64 features, computed once per shape and left unchanged"""
    key = (B, T, F)
    if key not in _CACHE:
        X = R.make_input(B, T, F)
        ref = dict(abs=(R.abs_feature(X), R.abs_bound(X)), log1p=(R.log1p_abs_feature(X), R.log1p_bound(X)),
                   mvn=(R.mvn_feature(X), R.mvn_bound(X)))
        for v in ref.values():
            for a in v:
                a.setflags(write=False)
        _CACHE[key] = (X, torch.as_tensor(X).cuda(), ref)
    return _CACHE[key]


def nan_buffer(B, T, F, col0=3):
    ld = -(-(F + 8) // 4) * 4
    return torch.full((B, T, ld), float("nan"), device="cuda"), ld, col0


def only_block_written(buf, col0, F):
    assert bool(torch.isnan(buf[..., :col0]).all()) and bool(torch.isnan(buf[..., col0 + F:]).all())
    assert bool(torch.isfinite(buf[..., col0:col0 + F]).all())


WORST = {}


@pytest.mark.parametrize("kind", ["abs", "log1p", "mvn"])
@pytest.mark.parametrize("B,T,F", SHAPES)
def test_kinds_within_bounds_and_placed(kind, B, T, F):
    from tssep_amd import hip_ops as H
    X, Xd, ref = case(B, T, F)
    buf, ld, col0 = nan_buffer(B, T, F)
    out = H.specfeat_fwd(Xd, kind, out=buf, col0=col0)
    assert out.data_ptr() == buf.data_ptr() + 4 * col0 and tuple(out.shape) == (B, T, F) and out.stride() == (T * ld, ld, 1)
    only_block_written(buf, col0, F)
    w = R.held(out.cpu().numpy(), *ref[kind], f"kind {kind} {(B, T, F)}")
    WORST[kind] = max(WORST.get(kind, 0.0), w)
    # a buffer of its own: the same bits, padding columns zeroed
    own = H.specfeat_fwd(Xd, H.SPECFEAT_KINDS[kind])
    assert torch.equal(own, out) and own.stride(1) == -(-F // 4) * 4
    base = torch.as_strided(own, (B, T, own.stride(1)), (T * own.stride(1), own.stride(1), 1))
    assert bool((base[..., F:] == 0).all())
    if kind == "mvn":
        again = H.specfeat_fwd(Xd, kind)
        assert torch.equal(again, own)                                     # run to run
        if B > 1:
            assert bool((out[1] == 0).all())                               # the silent utterance


@pytest.mark.parametrize("alpha", [1.0, 0.97])
@pytest.mark.parametrize("B,T,F", SHAPES)
def test_causal_within_bounds_and_placed(alpha, B, T, F):
    from tssep_amd import hip_ops as H
    X, Xd, _ = case(B, T, F)
    buf, ld, col0 = nan_buffer(B, T, F)
    out, state = H.specfeat_causal_fwd(Xd, None, alpha, out=buf, col0=col0)
    only_block_written(buf, col0, F)
    assert state.dtype == torch.float64 and tuple(state.shape) == (B, F + 1)
    ref, S, n = R.mvn_causal_feature(X, forgetting=alpha)
    w = R.held(out.cpu().numpy(), ref, R.mvn_causal_bound(X, forgetting=alpha), f"causal a={alpha} {(B, T, F)}")
    WORST[f"causal{alpha}"] = max(WORST.get(f"causal{alpha}", 0.0), w)
    assert bool((out[:, 0] == 0).all())                                    # the first frame of a fresh stream: exactly 0
    st = state.cpu().numpy()
    np.testing.assert_allclose(st[:, :F], S, rtol=2 * R.C1 * R.U, atol=R.TINY)
    np.testing.assert_allclose(st[:, F], n, rtol=1e-13)
    if alpha == 1.0:
        assert bool((state[:, F] == T).all())
        # the chain of kind 2's pass 1 is this one: the last frame has kind 2's bits
        assert torch.equal(out[:, -1], H.specfeat_fwd(Xd, "mvn")[:, -1])
    # a second chunk behind the state, against the float64 recursion continued from the float64 state
    out2, state2 = H.specfeat_causal_fwd(Xd, state, alpha)
    ref2 = R.mvn_causal_feature(X, S, n, alpha)[0]
    R.held(out2.cpu().numpy(), ref2, R.mvn_causal_bound(X, S, n, alpha, frames_before=T), f"causal chunk 2 a={alpha} {(B, T, F)}")
    assert state2.data_ptr() != state.data_ptr()


def test_zz_worst_figures():
    """(runs last in this file: what DESIGN 4.23 records)"""
    print("specfeat kernels, worst error / bound over all shapes:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


def _split_run(H, Xd, split, alpha):
    state, pos, outs = None, 0, []
    for c in split:
        o, state = H.specfeat_causal_fwd(Xd[:, pos:pos + c].contiguous(), state, alpha)
        outs.append(o)
        pos += c
    assert pos == Xd.shape[1]
    return torch.cat(outs, dim=1), state


@pytest.mark.parametrize("alpha", [1.0, 0.97])
@pytest.mark.parametrize("F", [5, 513])
def test_causal_split_invariance(alpha, F):
    from tssep_amd import hip_ops as H
    for T, splits in ((9, ((9,), (1,) * 9, (1, 1, 3, 4), (2, 1, 6))), (70, ((64, 6),))):
        _, Xd, _ = case(3, T, F) if T == 70 else (None, torch.as_tensor(R.make_input(3, T, F, seed=4)).cuda(), None)
        whole, state = H.specfeat_causal_fwd(Xd, None, alpha)
        for split in splits:
            got, st = _split_run(H, Xd, split, alpha)
            assert torch.equal(got, whole), (T, split)
            assert torch.equal(st, state), (T, split)


def test_kind1_is_the_L_of_the_causal_kernel():
    """out + S / n of the causal call is L up to the rounding of `out` (and of the float64 sum back): within U |out| + 2^-50 L
    of kind 1 -- and the two kernels call one routine (spec_log1p), which the source shows."""
    import os
    from tssep_amd import hip_ops as H
    X, Xd, _ = case(3, 70, 513)
    L1 = H.specfeat_fwd(Xd, "log1p").double()
    out, state = H.specfeat_causal_fwd(Xd, None, 1.0)
    # rebuild S / n per frame from kind 1 itself in float64 (the kernel's own chain: S += L, n = t + 1)
    mean = torch.cumsum(L1, dim=1) / torch.arange(1, 71, device="cuda", dtype=torch.float64)[None, :, None]
    err = (out.double() + mean - L1).abs()
    tol = R.U * out.double().abs() + 2.0 ** -45 * (L1 + mean) + R.TINY
    assert bool((err <= tol).all()), float((err / tol).max())
    total = L1.sum(dim=1)
    assert bool(((state[:, :513] - total).abs() <= 2.0 ** -45 * total + R.TINY).all())
    src = open(os.path.join(os.path.dirname(H.__file__), "csrc", "specfeat.hip")).read()
    assert src.count("log1pf(") == 1 and src.count("spec_log1p(xv") >= 2


def test_guards():
    from tssep_amd import _lib, hip_ops as H
    L = _lib.lib()
    X = torch.zeros(2, 3, 5, dtype=torch.complex64, device="cuda")
    with pytest.raises(RuntimeError, match="invalid shape"):
        H.specfeat_fwd(torch.zeros(1, 1, 1026, dtype=torch.complex64, device="cuda"), 1)
    with pytest.raises(RuntimeError, match="invalid shape"):
        H.specfeat_causal_fwd(torch.zeros(1, 1, 1026, dtype=torch.complex64, device="cuda"))
    with pytest.raises(RuntimeError, match="specfeat_causal_fwd failed"):
        H.specfeat_causal_fwd(torch.zeros(2, 0, 5, dtype=torch.complex64, device="cuda"))
    with pytest.raises(RuntimeError, match="unsupported"):
        H.specfeat_fwd(X, 3)
    with pytest.raises(ValueError, match=r"float32 \(2, 6\)"):
        H.specfeat_causal_fwd(X, torch.zeros(2, 6, device="cuda"))
    with pytest.raises(ValueError, match=r"float64 \(2, 5\)"):
        H.specfeat_causal_fwd(X, torch.zeros(2, 5, device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError, match="forgetting"):
        H.specfeat_causal_fwd(X, None, 0.0)
    with pytest.raises(ValueError, match="complex64"):
        H.specfeat_fwd(torch.zeros(2, 3, 5, device="cuda"), 1)
    with pytest.raises(ValueError, match="out is a float32"):
        H.specfeat_fwd(X, 1, out=torch.zeros(2, 3, 7, device="cuda"), col0=3)
    with pytest.raises(ValueError, match="col0"):
        H.specfeat_fwd(X, 1, col0=3)
    # overlapping states, on the C ABI (the wrapper always allocates a new one)
    Xr = torch.view_as_real(X)
    st = torch.zeros(2, 6, device="cuda", dtype=torch.float64)
    out = torch.full((2, 3, 5), float("nan"), device="cuda")
    p = H._p
    assert L.tssep_specfeat_causal_fwd(p(Xr), 2, 3, 5, 1.0, p(st), p(st), p(out), 5, H._stream()) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool((st == 0).all())
    # state_out NULL: outputs only
    assert L.tssep_specfeat_causal_fwd(p(Xr), 2, 3, 5, 1.0, p(st), None, p(out), 5, H._stream()) == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all())
