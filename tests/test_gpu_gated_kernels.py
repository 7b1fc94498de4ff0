"""The explicit_vad gated kernels -- tssep_mask_istft_gated_fwd / _bwd (stft.hip: istft_kernel<true, true>,
rfft_frames_kernel<true, true>), tssep_maskhead_gated_fwd / _bwd (maskhead.hip) and tssep_gatebce_fwd / _bwd
(elementwise.hip) -- against the float64 references of tests/test_gated_reference.py computed on the device, element by
element within the bounds derived there.  The C ABI is called directly; every output and every workspace that is read
back is pre-filled with NaN, bt_major outputs are allocated at their exact size, and any NaN or Inf fails (`within`).
Rows are scaled by 10^u, u in [-3, 3]; logits are 3 randn.

Sizes: the smallest at which each mechanism is exercised (test_the_cases_cross_the_boundaries).
    fused forward / backward   (2, 3, 6000) one chunk, B K T = 162 (not a multiple of the backward's 16 frames per
                               workgroup, T = 27 not a multiple of 4); (3, 4, 20001) 79 hops in chunks of 40 and 39, odd N:
                               the clamped scalar sample loads; (1, 8, 40000) three chunks, K = 8
    backward modes             dy, LogMAE, MAE x BCE fold on / off x [B, K, T, F + 1], bt_major, bt_major through a
                               non-identity iperm: seven combinations; est / tgt / logit / dlogit at a 4-byte offset give
                               bit-identical results; planted ties est == tgt, one frame made only of ties
    unfused pair               F = 513 at 20 500 frames (2.5 sweeps of frame_grid's 8 192, T = 1025 odd), F in {1, 63, 64,
                               65} (empty, partial, full and wrapped stride-64 loop); est NULL; dest, dmask, dvmask NULL
                               one by one and together
    gate BCE                   ld = 3 at 2 625 021 rows (2.5 sweeps of 1 048 576 rows; 7.9 M backward elements), ld = 514
    edge values                the multiples of 2^-6 in [-20, 20], +-30, +-88, +-100, +-1e4, +-0, +-2^-126 in the gate column
                               and in mask logits of distinct frames, through every kernel

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report); the whole file takes 7 - 12 s:
    mask_istft_gated_fwd    y 0.0043   |y - tgt| partials 0.040
    mask_istft_gated_bwd    d(v)   dy 0.030   LogMAE 0.048   MAE 0.048   with the BCE fold: dy 0.23   LogMAE 0.58   MAE 0.59
                            d(l_f) dy 0.064   LogMAE 0.066   MAE 0.066   (the same with the fold)
    maskhead_gated_fwd      mask 0.38   vmask 0.40   est 0.36
    maskhead_gated_bwd      d(v) 0.33   d(l_f) 0.53   on the float64 adjoint 0.26
    gatebce_fwd             rows 0.87   loss 0.049        gatebce_bwd   column 0 0.74
    fused against unfused   d(v) 0.00014   d(l_f) 0.0032
    edge values             mask_istft_gated_fwd y 0.012   mask_istft_gated_bwd d(v) 0.51, d(l_f) 0.51   maskhead_gated_fwd mask
                            0.39, vmask 0.44, est 0.51   maskhead_gated_bwd 0.51   gatebce_fwd rows 0.46, loss 0.012
                            gatebce_bwd column 0 0.69
(The transform terms are bounded by a frame's error norm, which one element reaches only if it carries the whole error:
y and the fused d(l_f) sit far below 1; the element-wise kernels sit near one half, a rounding's mean.)

Once, outside the suite: with the Nyquist term dropped from the fused kernel's d(v) sum, with inv_kt divided by F, and with
iperm read at a wrong speaker, test_fused_backward failed on d(v) in 37 of 81, 81 of 81 and 54 of 81 frames of its first
utterance.
"""
import math

import pytest
import torch

import test_gated_reference as R
from test_gated_reference import F, MODES, bt_load, frames, make_inputs, plant_ties
from test_gpu_stft_kernels import (Ratios, abi_istft, abi_mask_istft, abi_mask_istft_bwd, check_partials, plan1_chunks, windows32,
                                   windows64, within)

pytestmark = pytest.mark.gpu

GIB = 1 << 30
DEV = "cuda"
NAN = float("nan")
E_NULL = -5                      # include/tssep_hip.h
FRAME_SWEEP = 256 * 8 * 4        # maskhead.hip frame_grid: frames per sweep
ROW_SWEEP = 256 * 16 * 256       # elementwise.hip grid_for: rows / elements per sweep
BWD_FRAMES = 16                  # stft.hip rfft_frames_kernel: frames per workgroup (4 waves x 4 iterations)

FUSED_CASES = [(2, 3, 6000), (3, 4, 20001), (1, 8, 40000)]
# (F, B, K, T)
UNFUSED_CASES = [(513, 5, 4, 1025), (1, 2, 3, 701), (63, 2, 3, 701), (64, 2, 3, 701), (65, 2, 3, 701)]
BCE_CASES = [(3, 7, 3, 125001), (514, 2, 3, 27)]
# (mode, BCE fold, layout)
BWD_COMBOS = [("dy", False, "bktf"), ("dy", True, "bt"), ("logmae", True, "bt_iperm"), ("logmae", False, "bt"),
              ("mae", True, "bktf"), ("mae", False, "bt_iperm"), ("dy", True, "bt_iperm")]
EDGE = (2, 3, 230000)            # T = 902: 5 412 frames for the 2 573 edge values of the gate column

WORST = Ratios()                 # the file's table (test_zz_report)


def H():
    from tssep_amd import hip_ops
    return hip_ops


def L():
    from tssep_amd import _lib
    return _lib.lib()


def _p(t):
    return H()._p(t)


def _ok(rc, what):
    assert rc == 0, f"{what} returned {rc}"


def note(entry, check, v):
    WORST.add(f"{entry:<28}{check}", v)


@pytest.fixture(autouse=True)
def _device_memory_cap():
    """The GPU is shared: every test here stays under 16 GB of device memory at its peak."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 * GIB, f"peak device memory {peak / GIB:.1f} GiB"


def test_the_cases_cross_the_boundaries():
    hops = lambda N: -(-N // 256)                                                          # noqa: E731
    assert [frames(N) for _, _, N in FUSED_CASES] == [27, 82, 160]
    assert plan1_chunks(6000) == (1, 24) and plan1_chunks(20001) == (2, 40) and hops(20001) == 79 and 79 - 40 == 39
    assert plan1_chunks(40000) == (3, 53) and hops(40000) - 2 * 53 == 51
    assert any(N % 2 for _, _, N in FUSED_CASES) and any(K == 8 for _, K, _ in FUSED_CASES)
    assert any((B * K * frames(N)) % BWD_FRAMES and frames(N) % 4 for B, K, N in FUSED_CASES)
    assert {m for m, _, _ in BWD_COMBOS} == set(MODES) and {f for _, f, _ in BWD_COMBOS} == {False, True}
    assert {lay for _, _, lay in BWD_COMBOS} == {"bktf", "bt", "bt_iperm"} and len(BWD_COMBOS) >= 7
    assert all({f for m, f, _ in BWD_COMBOS if m == mode} == {False, True} for mode in MODES)
    Fb, B, K, T = UNFUSED_CASES[0]
    assert Fb == 513 and B * K * T == 20500 >= 2.5 * FRAME_SWEEP and T % 2 == 1 and FRAME_SWEEP == 8192
    assert {c[0] for c in UNFUSED_CASES[1:]} == {1, 63, 64, 65} and all(2000 < b * k * t < 8192 for _, b, k, t in UNFUSED_CASES[1:])
    ld, B, K, T = BCE_CASES[0]
    assert ld == 3 and B * K * T == 2625021 >= 2.5 * ROW_SWEEP and B * K * T * ld > 7.5 * ROW_SWEEP and K * T == 375003
    assert ROW_SWEEP == 1048576 and BCE_CASES[1][0] == 514
    assert len(edge_values()) == 2561 + 12 <= EDGE[0] * EDGE[1] * frames(EDGE[2]) // 2


# ------------------------------------------------------------------------------------------------- C ABI, NaN outputs
def off1(t):
    """a copy of t whose first element lies 4 bytes behind a 16-byte boundary"""
    buf = torch.full((t.numel() + 1,), NAN, device=DEV, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 8 == 4
    return v


def abi_gated_fwd(logit, obs, ws, N, tgt=None):
    B, K, T, _ = logit.shape
    y = torch.full((B * K, N), NAN, device=DEV)
    part = torch.full((B * K, int(L().tssep_istft_chunks(N))), NAN, device=DEV) if tgt is not None else None
    _ok(L().tssep_mask_istft_gated_fwd(_p(logit), _p(torch.view_as_real(obs)), B, K, T, 1024, 256, 1, _p(ws),
                                       _p(H().fft_tables(1024, DEV)), _p(y), N, _p(tgt), _p(part), H()._stream()),
        "mask_istft_gated_fwd")
    return y, part


def abi_gated_bwd(x, tgt, sums, gout, vad, gbce, logit, obs, ws, iperm=None, bt_major=False, offset=False):
    B, K, T, F1 = logit.shape
    dl = torch.full((B * T, K * F1) if bt_major else (B, K, T, F1), NAN, device=DEV)
    if offset:
        dl = off1(dl)
    _ok(L().tssep_mask_istft_gated_bwd(_p(x), _p(tgt), _p(sums), _p(gout), _p(vad), _p(gbce), _p(logit),
                                       _p(torch.view_as_real(obs)), B, K, x.shape[-1], 1024, 256, 1, _p(ws),
                                       _p(H().fft_tables(1024, DEV)), _p(iperm), int(bt_major), _p(dl), T, H()._stream()),
        "mask_istft_gated_bwd")
    return dl


def abi_unfused_fwd(logit, obs, with_est=True):
    B, K, T, F1 = logit.shape
    mask = torch.full((B, K, T, F1 - 1), NAN, device=DEV)
    vmask = torch.full((B, K, T), NAN, device=DEV)
    est = torch.full((B, K, T, F1 - 1, 2), NAN, device=DEV) if with_est else None
    _ok(L().tssep_maskhead_gated_fwd(_p(logit), _p(torch.view_as_real(obs)), _p(mask), _p(est), _p(vmask), B, K, T, F1 - 1,
                                     H()._stream()), "maskhead_gated_fwd")
    return mask, est, vmask


def abi_unfused_bwd(dest, dmask, dvm, logit, obs):
    B, K, T, F1 = logit.shape
    dl = torch.full((B, K, T, F1), NAN, device=DEV)
    _ok(L().tssep_maskhead_gated_bwd(_p(torch.view_as_real(dest)) if dest is not None else None, _p(dmask), _p(dvm),
                                     _p(logit), _p(torch.view_as_real(obs)), _p(dl), B, K, T, F1 - 1, H()._stream()),
        "maskhead_gated_bwd")
    return dl


def abi_bce_fwd(logit, ld, vad):
    B, K, T = vad.shape
    loss = torch.full((B,), NAN, device=DEV)
    ws = torch.full((B * K * T,), NAN, device=DEV)
    _ok(L().tssep_gatebce_fwd(_p(logit), ld, _p(vad), B, K, T, _p(loss), _p(ws), H()._stream()), "gatebce_fwd")
    return loss, ws.view(B, K, T)


def abi_bce_bwd(logit, ld, vad, gout):
    B, K, T = vad.shape
    dl = torch.full((B, K, T, ld), NAN, device=DEV)
    _ok(L().tssep_gatebce_bwd(_p(logit), ld, _p(vad), _p(gout), B, K, T, _p(dl), H()._stream()), "gatebce_bwd")
    return dl


def ws_pair():
    _, ws64 = windows64(1024, 256)
    _, ws = windows32(1024, 256)
    return ws64.to(DEV), ws


def per_utterance(B):
    """the references are computed utterance by utterance"""
    return [(b, b + 1) for b in range(B)]


# ------------------------------------------------------------------------------------------------------ fused forward
def check_fused_fwd(y, logit, obs, ws64, N, entry, name):
    K = logit.shape[1]
    for lo, hi in per_utterance(logit.shape[0]):
        ref, tol = R.ref_fused_fwd(logit[lo:hi].double(), obs[lo:hi].to(torch.complex128), ws64, N)
        note(entry, name, within(y[lo * K:hi * K], ref, tol, f"{entry} {name}"))


@pytest.mark.parametrize("B,K,N", FUSED_CASES)
def test_fused_forward(B, K, N):
    """tssep_mask_istft_gated_fwd with and without the target, the |y - tgt| partials of every chunk, the NULL pairing of
    tgt and abs_partial, and a logit at a 4-byte offset (bit-identical)."""
    d = make_inputs(B, K, N, seed=B * K + N, device=DEV)
    ws64, ws = ws_pair()
    nch, hcb = plan1_chunks(N)
    y, part = abi_gated_fwd(d["logit"], d["obs"], ws, N, tgt=d["tgt"])
    assert part.shape[1] == nch
    check_fused_fwd(y, d["logit"], d["obs"], ws64, N, "mask_istft_gated_fwd", "y")
    r = Ratios()
    check_partials(part, y, d["tgt"], hcb, "partials", r)
    note("mask_istft_gated_fwd", "|y - tgt| partials", r.r["partials"])
    y2, none = abi_gated_fwd(d["logit"], d["obs"], ws, N)
    assert none is None and torch.equal(y2, y)
    assert torch.equal(abi_gated_fwd(off1(d["logit"]), d["obs"], ws, N)[0], y)
    yn = torch.full((B * K, N), NAN, device=DEV)
    pn = torch.full((B * K, nch), NAN, device=DEV)
    for tgt, pp in ((d["tgt"], None), (None, pn)):
        rc = L().tssep_mask_istft_gated_fwd(_p(d["logit"]), _p(torch.view_as_real(d["obs"])), B, K, d["T"], 1024, 256, 1, _p(ws),
                                            _p(H().fft_tables(1024, DEV)), _p(yn), N, _p(tgt), _p(pp), H()._stream())
        assert rc == E_NULL, rc


# ----------------------------------------------------------------------------------------------------- fused backward
def read_layout(dl, layout, d):
    B, K, T = d["B"], d["K"], d["T"]
    if layout == "bktf":
        return dl.view(B, K, T, F + 1)
    if layout == "bt":
        assert tuple(dl.shape) == (B * T, K * (F + 1))
        return dl.view(B, T, K, F + 1).transpose(1, 2)
    return bt_load(dl, d["iperm"], K)


def run_bwd(d, ws, mode, fold, layout, est=None, tgt=None, logit=None, offset=False, sums="sums"):
    x = d["dy"] if mode == "dy" else (est if est is not None else d["est"])
    t = None if mode == "dy" else (tgt if tgt is not None else d["tgt_ties"])
    return abi_gated_bwd(x, t, d[sums] if mode == "logmae" else None, None if mode == "dy" else d["gout"],
                         d["vad"] if fold else None, d["gbce"] if fold else None, logit if logit is not None else d["logit"],
                         d["obs"], ws, d["iperm"] if layout == "bt_iperm" else None, layout != "bktf", offset=offset)


def check_fused_bwd(got, d, ws64, mode, fold, entry, name):
    """got [B, K, T, F + 1] -> the all-tie frame aside, every element within its bound; d(v) and d(l_f) reported apart"""
    K = d["K"]
    for lo, hi in per_utterance(d["B"]):
        rows = slice(lo * K, hi * K)
        ref, tol = R.ref_fused_bwd(mode, (d["dy"] if mode == "dy" else d["est"])[rows], d["tgt_ties"][rows], d["gout"][lo:hi],
                                   d["sums"][lo:hi], d["logit"][lo:hi].double(), d["obs"][lo:hi].to(torch.complex128), ws64,
                                   d["vad"][lo:hi] if fold else None, d["gbce"][lo:hi])
        note(entry, name + " d(v)", within(got[lo:hi, ..., 0], ref[..., 0], tol[..., 0], f"{entry} {name} d(v)"))
        note(entry, name + " d(l_f)", within(got[lo:hi, ..., 1:], ref[..., 1:], tol[..., 1:], f"{entry} {name} d(l_f)"))


@pytest.mark.parametrize("B,K,N", FUSED_CASES)
def test_fused_backward(B, K, N):
    """tssep_mask_istft_gated_bwd: dy, LogMAE and MAE (sums = NULL) with the BCE fold on and off into [B, K, T, F + 1],
    bt_major and bt_major through a non-identity iperm.  The loss modes read the kernel's own fp32 estimate; ties est ==
    tgt are planted, and the frame made only of ties has exact zeros behind column 0 and exactly the fold term at it."""
    d = make_inputs(B, K, N, seed=B * K + N, device=DEV)
    ws64, ws = ws_pair()
    T = d["T"]
    assert K < 3 or bool((d["iperm"] != torch.arange(K, device=DEV)).any()) and bool((d["iperm"] != d["perm"]).any())
    d["est"], _ = abi_gated_fwd(d["logit"], d["obs"], ws, N)
    d["tgt_ties"] = plant_ties(d["est"], d["tgt"])
    assert int((d["est"] == d["tgt_ties"]).sum()) >= 300
    zero_dy = dict(d, dy=torch.zeros_like(d["dy"]))
    fold_only = run_bwd(zero_dy, ws, "dy", True, "bktf")           # D = 0: exactly the kernel's fold term at column 0
    assert not bool(fold_only[..., 1:].any())
    got = {}
    for mode, fold, layout in BWD_COMBOS:
        dl = read_layout(run_bwd(d, ws, mode, fold, layout), layout, d)
        check_fused_bwd(dl, d, ws64, mode, fold, "mask_istft_gated_bwd", f"{mode}{' + BCE fold' if fold else ''}")
        if (mode, fold) in got:                                    # the layouts agree bit for bit
            assert torch.equal(got[mode, fold], dl), (mode, fold, layout)
        got[mode, fold] = dl.contiguous()
        if mode != "dy":
            fr = dl[0, 0, 4]
            assert not bool(fr[1:].any()), (mode, fold, "the all-tie frame")
            assert float(fr[0]) == (float(fold_only[0, 0, 4, 0]) if fold else 0.0), (mode, fold, "the all-tie frame's d(v)")
    # the clamped scalar sample loads (odd N takes them anyway; at even N through est / tgt at a 4-byte offset), logit and
    # dlogit at a 4-byte offset: bit-identical (the fixed summation order)
    ref = got["logmae", True]
    if N % 2 == 0:
        for est, tgt in ((off1(d["est"]), None), (None, off1(d["tgt_ties"])), (off1(d["est"]), off1(d["tgt_ties"]))):
            assert torch.equal(run_bwd(d, ws, "logmae", True, "bktf", est=est, tgt=tgt), ref)
        assert torch.equal(read_layout(abi_gated_bwd(off1(d["dy"]), None, None, None, None, None, d["logit"], d["obs"], ws), "bktf", d),
                           got["dy", False])
    assert torch.equal(run_bwd(d, ws, "logmae", True, "bktf", logit=off1(d["logit"]), offset=True), ref)
    assert torch.equal(run_bwd(d, ws, "logmae", True, "bktf"), ref)          # and run to run
    # the wrapper hands a non-contiguous `sums` to the kernel as a contiguous fp32 vector, like its other arguments
    strided = torch.stack([d["sums"], torch.full_like(d["sums"], NAN)], 1)[:, 0]
    assert not strided.is_contiguous() or B == 1
    w = H().mask_istft_bwd(None, d["logit"], d["obs"], ws, loss=(d["est"].view(B, K, N), d["tgt_ties"].view(B, K, N), strided,
                                                                  d["gout"]), vad=(d["vad"], d["gbce"]))
    assert torch.equal(w, ref)
    with pytest.raises(AssertionError):
        H().mask_istft_bwd(None, d["logit"], d["obs"], ws, loss=(d["est"].view(B, K, N), d["tgt_ties"].view(B, K, N),
                                                              d["sums"].double(), d["gout"]))


def test_fused_backward_agrees_with_the_unfused_head():
    """The two implementations of d(v): the fused backward in dy mode against tssep_maskhead_gated_bwd applied to the
    device-float64 adjoint rounded to fp32 -- within the sum of the two bounds (and the distance of the two references,
    which is the rounding of that adjoint)."""
    B, K, N = FUSED_CASES[0]
    d = make_inputs(B, K, N, seed=77, device=DEV)
    ws64, ws = ws_pair()
    T = d["T"]
    fused = run_bwd(d, ws, "dy", False, "bktf")
    lg, o = d["logit"].double(), d["obs"].to(torch.complex128)
    ref1, tol1 = R.ref_fused_bwd("dy", d["dy"], None, None, None, lg, o, ws64)
    D, _ = R.ref_rfft(d["dy"].double(), ws64, 1024, 256, 768, T, adjoint=True)
    dest = D.view(B, K, T, F).to(torch.complex64)
    unfused = abi_unfused_bwd(dest, None, None, d["logit"], d["obs"])
    ref2, tol2 = R.ref_unfused_bwd(dest.to(torch.complex128), None, None, lg, o)
    note("maskhead_gated_bwd", "on the float64 adjoint", within(unfused, ref2, tol2, "maskhead_gated_bwd on the adjoint"))
    tol = tol1 + tol2 + (ref1 - ref2).abs()
    note("fused against unfused", "d(v)", within(fused[..., 0], unfused[..., 0].double(), tol[..., 0], "fused / unfused d(v)"))
    note("fused against unfused", "d(l_f)", within(fused[..., 1:], unfused[..., 1:].double(), tol[..., 1:], "fused / unfused d(l_f)"))


# ------------------------------------------------------------------------------------------------------- unfused pair
def unfused_inputs(Fb, B, K, T, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rs = lambda n: R.row_scale(n, g, DEV)                                                    # noqa: E731
    logit = torch.randn(B, K, T, Fb + 1, device=DEV, generator=g).mul_(3)
    obs = torch.randn(B, T, Fb, device=DEV, generator=g, dtype=torch.complex64) * rs(B)[:, None, None]
    dest = torch.randn(B, K, T, Fb, device=DEV, generator=g, dtype=torch.complex64) * rs(B * K).view(B, K, 1, 1)
    dmask = torch.randn(B, K, T, Fb, device=DEV, generator=g) * rs(B * K).view(B, K, 1, 1)
    dvm = torch.randn(B, K, T, device=DEV, generator=g) * rs(B * K).view(B, K, 1)
    return logit, obs, dest, dmask, dvm


@pytest.mark.parametrize("Fb,B,K,T", UNFUSED_CASES)
def test_unfused_pair(Fb, B, K, T):
    """tssep_maskhead_gated_fwd (est given and NULL) and tssep_maskhead_gated_bwd with dest, dmask and dvmask all given, NULL
    one by one and NULL together (exact zeros); a logit at a 4-byte offset is bit-identical."""
    logit, obs, dest, dmask, dvm = unfused_inputs(Fb, B, K, T, seed=Fb + T)
    logit[0, 0, 1, 1:] = 1e4                        # s_f = 1 exactly: this frame's mask is the gate itself, bit for bit
    mask, est, vmask = abi_unfused_fwd(logit, obs)
    assert torch.equal(mask[0, 0, 1], vmask[0, 0, 1].expand(Fb))
    m2, none, v2 = abi_unfused_fwd(logit, obs, with_est=False)
    assert none is None and torch.equal(m2, mask) and torch.equal(v2, vmask)
    m3, e3, v3 = abi_unfused_fwd(off1(logit), obs)
    assert torch.equal(m3, mask) and torch.equal(e3, est) and torch.equal(v3, vmask)
    grads = {"all": (dest, dmask, dvm), "dest NULL": (None, dmask, dvm), "dmask NULL": (dest, None, dvm),
             "dvmask NULL": (dest, dmask, None)}
    dls = {k: abi_unfused_bwd(*v, logit, obs) for k, v in grads.items()}
    assert torch.equal(abi_unfused_bwd(dest, dmask, dvm, off1(logit), obs), dls["all"])
    zeros = abi_unfused_bwd(None, None, None, logit, obs)
    assert not bool(zeros.any())
    for lo, hi in per_utterance(B):
        lg, o = logit[lo:hi].double(), obs[lo:hi].to(torch.complex128)
        fw = R.ref_unfused_fwd(lg, o)
        for name, t in (("mask", mask), ("vmask", vmask), ("est", est)):
            note("maskhead_gated_fwd", name, within(t[lo:hi], *fw[name], f"maskhead_gated_fwd {name}"))
        del fw
        for k, (a, b_, c) in grads.items():
            ref, tol = R.ref_unfused_bwd(a[lo:hi].to(torch.complex128) if a is not None else None,
                                         b_[lo:hi].double() if b_ is not None else None,
                                         c[lo:hi].double() if c is not None else None, lg, o)
            note("maskhead_gated_bwd", "d(v)", within(dls[k][lo:hi, ..., 0], ref[..., 0], tol[..., 0], f"d(v) {k}"))
            note("maskhead_gated_bwd", "d(l_f)", within(dls[k][lo:hi, ..., 1:], ref[..., 1:], tol[..., 1:], f"d(l_f) {k}"))
            del ref, tol


def test_unfused_gate_is_the_fused_kernels_gate():
    """A row whose mask logits are all +1e4 has mask = vmask in the unfused forward, bit for bit, and the fused forward's
    samples of that row are the plain inverse transform of the unfused estimate, bit for bit: one gate in both."""
    B, K, N = FUSED_CASES[0]
    d = make_inputs(B, K, N, seed=5, device=DEV)
    _, ws = ws_pair()
    d["logit"][1, 2, :, 1:] = 1e4
    mask, est, vmask = abi_unfused_fwd(d["logit"], d["obs"])
    assert torch.equal(mask[1, 2], vmask[1, 2, :, None].expand(-1, F))
    y, _ = abi_gated_fwd(d["logit"], d["obs"], ws, N)
    y_plain, _ = abi_istft(torch.view_as_complex(est).view(B * K, d["T"], F), ws, N, 1024, 256, True)
    assert torch.equal(y[5], y_plain[5])


# ----------------------------------------------------------------------------------------------------------- gate BCE
def check_bce(logit, ld, vad, gout, entry=""):
    B, K, T = vad.shape
    x = logit.view(B, K, T, ld)[..., 0].double()
    loss, rows = abi_bce_fwd(logit, ld, vad)
    l, e = R.ref_bce_rows(x, vad.double())
    note(entry or "gatebce_fwd", entry and "gatebce_fwd rows" or "rows", within(rows, l, R.finish(e), "gatebce_fwd rows"))
    del l, e
    note(entry or "gatebce_fwd", entry and "gatebce_fwd loss" or "loss", within(loss, *R.ref_bce(x, vad.double()), "gatebce_fwd loss"))
    dl = abi_bce_bwd(logit, ld, vad, gout)
    assert ld == 1 or not bool(dl[..., 1:].any()), "columns 1 .. ld - 1 are exact zeros"
    note(entry or "gatebce_bwd", entry and "gatebce_bwd column 0" or "column 0", within(dl[..., 0], *R.ref_bce_bwd(x, vad.double(), gout), "gatebce_bwd column 0"))


@pytest.mark.parametrize("ld,B,K,T", BCE_CASES)
def test_gate_bce(ld, B, K, T):
    """tssep_gatebce_fwd (every row of the workspace and the mean) and tssep_gatebce_bwd (column 0 within the bound, exact
    zeros behind it) past 2.5 sweeps of the capped grids."""
    g = torch.Generator(device=DEV).manual_seed(ld + T)
    logit = torch.randn(B, K, T, ld, device=DEV, generator=g).mul_(3)
    vad = (torch.rand(B, K, T, device=DEV, generator=g) > 0.5).float()
    vad[0] = torch.rand(K, T, device=DEV, generator=g)                  # (a soft target too: the product x y is rounded)
    gout = torch.rand(B, device=DEV, generator=g) + 0.5
    check_bce(logit, ld, vad, gout)


# -------------------------------------------------------------------------------------------------------- edge values
def edge_values():
    grid = torch.arange(-20 * 64, 20 * 64 + 1, dtype=torch.float64) / 64
    sp = [30.0, 88.0, 100.0, 1e4, 0.0, 2.0 ** -126]
    return torch.cat([grid, torch.tensor(sp + [-v for v in sp], dtype=torch.float64)]).float()


def test_edge_values_through_every_kernel():
    """The edge values in the gate column of distinct frames (rows 0 - 2) and in the mask logits of six frames (row 3);
    row 4's gate is -1e4 (float64 rounds it to 0: exact zeros everywhere) and row 5's cycles through 88, 100 and 1e4
    (float64 rounds it to 1: the ungated kernels' values, bit for bit, and an exactly vanishing d(v))."""
    B, K, N = EDGE
    d = make_inputs(B, K, N, seed=9, device=DEV)
    ws64, ws = ws_pair()
    T = d["T"]
    ev = edge_values().to(DEV)
    n = ev.numel()
    logit = d["logit"]
    logit.view(B * K * T, F + 1)[:n, 0] = ev
    assert n <= 3 * T
    logit[1, 0, 10:16, 1:] = logit[1, 0, 10:16, 1:].reshape(-1).index_copy(0, torch.arange(n, device=DEV), ev).view(6, F)
    logit[1, 1, :, 0] = -1e4
    logit[1, 2, :, 0] = torch.tensor([88.0, 100.0, 1e4], device=DEV).repeat(T)[:T]
    assert float(torch.sigmoid(torch.tensor(-1e4, dtype=torch.float64))) == 0.0
    assert float(torch.sigmoid(torch.tensor(88.0, dtype=torch.float64))) == 1.0
    d["tgt_ties"] = d["tgt"]
    plain = logit[..., 1:].contiguous()
    # fused forward
    y, _ = abi_gated_fwd(logit, d["obs"], ws, N)
    check_fused_fwd(y, logit, d["obs"], ws64, N, "edge values", "mask_istft_gated_fwd y")
    assert not bool(y[4].any())
    y_plain, _ = abi_mask_istft(plain, d["obs"], ws, N)
    assert torch.equal(y[5], y_plain[5])
    # fused backward, dy with and without the fold
    for fold in (False, True):
        dl = run_bwd(d, ws, "dy", fold, "bktf")
        check_fused_bwd(dl, d, ws64, "dy", fold, "edge values", f"mask_istft_gated_bwd{' + BCE fold' if fold else ''}")
        assert not bool(dl[1, 1, :, 1:].any())
        if not fold:
            assert not bool(dl[1, 1].any()) and not bool(dl[1, 2, :, 0].any())
            dl_plain = abi_mask_istft_bwd(d["dy"], plain, d["obs"], ws)
            assert torch.equal(dl[1, 2, :, 1:], dl_plain[1, 2])
    # the unfused pair
    mask, est, vmask = abi_unfused_fwd(logit, d["obs"])
    _, _, dest, dmask, dvm = unfused_inputs(F, B, K, T, seed=10)
    du = abi_unfused_bwd(dest, dmask, dvm, logit, d["obs"])
    for lo, hi in per_utterance(B):
        lg, o = logit[lo:hi].double(), d["obs"][lo:hi].to(torch.complex128)
        fw = R.ref_unfused_fwd(lg, o)
        for name, t in (("mask", mask), ("vmask", vmask), ("est", est)):
            note("edge values", f"maskhead_gated_fwd {name}", within(t[lo:hi], *fw[name], f"edge maskhead_gated_fwd {name}"))
        ref, tol = R.ref_unfused_bwd(dest[lo:hi].to(torch.complex128), dmask[lo:hi].double(), dvm[lo:hi].double(), lg, o)
        note("edge values", "maskhead_gated_bwd", within(du[lo:hi], ref, tol, "edge maskhead_gated_bwd"))
    assert not bool(mask[1, 1].any()) and not bool(vmask[1, 1].any()) and not bool(est[1, 1].any()) and not bool(du[1, 1].any())
    assert bool((vmask[1, 2] == 1).all()) and not bool(du[1, 2, :, 0].any())
    sig = torch.full_like(plain, NAN)
    est_plain = torch.full(plain.shape + (2,), NAN, device=DEV)
    _ok(L().tssep_maskhead_fwd(_p(plain), _p(torch.view_as_real(d["obs"])), _p(sig), _p(est_plain), B, K, T, F, H()._stream()),
        "maskhead_fwd")
    assert torch.equal(mask[1, 2], sig[1, 2]) and torch.equal(est[1, 2], est_plain[1, 2])
    # the gate BCE on the edge gate column against a 0 / 1 vad
    check_bce(logit, F + 1, d["vad"], d["gbce"], entry="edge values")


def test_zz_report():
    """The worst err / tol of every entry point and check of this file (pytest -rP)."""
    for k in sorted(WORST.r):
        print(f"max err/tol  {k}: {WORST.r[k]:.3g}")
    assert all(math.isfinite(v) and v <= 1.0 for v in WORST.r.values())
