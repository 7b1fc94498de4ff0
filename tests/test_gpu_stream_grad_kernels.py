"""tssep_istft_stream_bwd / tssep_mask_istft_stream_bwd on a real MI355X, called directly, every output pre-filled with
NaN.  The calls of a stream run last first, each d_ola_in handed on as the earlier call's d_ola_out:
  * the concatenated dX / dlogit carry the bits of tssep_istft_bwd / tssep_mask_istft_bwd / tssep_mask_istft_gated_bwd over
    all frames (compared after -0 -> +0);
  * with d_ola_out = NULL a call's frames carry the bits of the whole-utterance launch on dy zeroed behind the call's last
    completed sample; NULL equals an all-zero d_ola_out; d_ola_in is the exact copy of hops 0, 1, 2 of g;
  * against the float64 adjoint of tests/stream_grad_reference.py both kernels sit inside the measure of the fused-tail
    backward test (tests/test_gpu_stft_kernels.py) with the SAME worst ratio on the same frames;
  * the guards.
Streams: 7 and 11 pushed hops + rests 0, 1, 37, 255 (even and odd N) by the pushes of stream_grad_reference.PATTERNS
(skip 3, 2, 1, 0; calls of fewer than three frames; calls that complete nothing; the ragged final call), and one call of 70
frames, more than one workgroup's share.  A chained d_ola_out is zero on the hops in front of the utterance's first
sample, so single calls with a RANDOM d_ola_out, every (Tc, skip) in 1 .. 5 x 0 .. 3 (skip > Tc among them), run against
the float64 adjoint as well."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import stream_grad_reference as SG  # noqa: E402

DEV = "cuda"
NAN = float("nan")
E_SHAPE, E_ALIGN, E_UNSUPPORTED, E_NULL = -1, -2, -3, -5
FORMS = ("plain", "masked", "gated")
WORST = {}


def L():
    from tssep_amd import _lib
    return _lib.lib()


def H():
    from tssep_amd import hip_ops
    return hip_ops


def p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nans(*shape):
    return torch.full(shape, NAN, device=DEV, dtype=torch.float32)


def tables():
    from tssep_amd import functional as Fn
    return Fn.windows("hann", 1024, 256, torch.device(DEV), 1024)[1], H().fft_tables(1024, torch.device(DEV))


def whole_bwd(form, dy, frames, obs, T):
    """The whole-utterance entry point of the form: dy [rows, N] -> dX [rows, T, 513, 2] / dlogit [B, K, T, 513 (+ 1)]"""
    ws, tw = tables()
    rows, N = dy.shape
    dy = dy.contiguous()
    if form == "plain":
        d = nans(rows, T, 513, 2)
        rc = L().tssep_istft_bwd(p(dy), rows, N, 1024, 256, 1, p(ws), p(tw), p(d), T, stream())
    else:
        B, K = frames.shape[:2]
        d, ob = nans(*frames.shape), torch.view_as_real(obs.contiguous())
        if form == "masked":
            rc = L().tssep_mask_istft_bwd(p(dy), p(frames), p(ob), B, K, N, 1024, 256, 1, p(ws), p(tw), p(d), T, stream())
        else:
            rc = L().tssep_mask_istft_gated_bwd(p(dy), None, None, None, None, None, p(frames), p(ob), B, K, N, 1024, 256, 1,
                                                p(ws), p(tw), None, 0, p(d), T, stream())
    assert rc == 0, (rc, form)
    return d


def call_bwd(form, dy, d_ola_out, frames, obs, rows, st, last, want_ola=True):
    """One call's backward: frames = logit [B, K, Tc, 513 (+ 1)] of the call (plain: None) -> (d, d_ola_in)"""
    ws, tw = tables()
    Tc, n = st.frames, st.samples
    d_in = nans(rows, 768) if want_ola else None
    dy = None if not n else dy.contiguous()
    if form == "plain":
        d = nans(rows, Tc, 513, 2)
        rc = L().tssep_istft_stream_bwd(p(dy), p(d_ola_out), rows, Tc, 1024, 256, p(ws), p(tw), st.skip, int(last), n, p(d),
                                        p(d_in), stream())
    else:
        fr, ob = frames.contiguous(), torch.view_as_real(obs.contiguous())
        d = nans(*fr.shape)
        rc = L().tssep_mask_istft_stream_bwd(p(dy), p(d_ola_out), p(fr), int(form == "gated"), p(ob), fr.shape[0], fr.shape[1],
                                             Tc, 1024, 256, p(ws), p(tw), st.skip, int(last), n, p(d), p(d_in), stream())
    assert rc == 0, (rc, form, st)
    return d, d_in


def make(form, B, K, T, N, seed):
    g = torch.Generator().manual_seed(seed)
    logit, obs = SG.inputs(B, K, T, form == "gated", seed)
    dy = torch.randn(B * K, N, generator=g) * 10.0 ** (torch.rand(B * K, 1, generator=g) * 2 - 1)
    return (None if form == "plain" else logit.to(DEV)), obs.to(DEV), dy.to(DEV)


def tdim(form):
    return 1 if form == "plain" else 2


def frames_of(d, form, lo, hi):
    return d[:, lo:hi] if form == "plain" else d[:, :, lo:hi]


def run_stream(form, B, K, hops, pushes, rest, seed):
    """Every assertion of the file on one stream -> the worst err / tol against the float64 adjoint."""
    N = hops * 256 + rest
    steps = SG.steps_of(pushes, N)
    T = sum(s.frames for s in steps)
    rows = B * K
    logit, obs, dy = make(form, B, K, T, N, seed)
    whole = whole_bwd(form, dy, logit, obs, T)
    lg_c, ob_c, dy_c = (None if logit is None else logit.cpu()), obs.cpu(), dy.cpu()
    worst = 0.0
    ds, d_ola, t_hi, n_hi = [], None, T, N
    for i in reversed(range(len(steps))):
        st, last = steps[i], i == len(steps) - 1
        t_lo, n_lo = t_hi - st.frames, n_hi - st.samples
        lg = None if logit is None else logit[:, :, t_lo:t_hi]
        ob = obs[:, t_lo:t_hi]
        dyc = dy[:, n_lo:n_hi]
        what = f"{form} B={B} K={K} {hops}+{rest} {pushes} call {i} {st}"
        d, d_in = call_bwd(form, dyc, d_ola, lg, ob, rows, st, last)
        # the float64 adjoint of THIS call (its own carry gradient as input) and the exact copy d_ola_in
        cpu = dict(logit=None if lg is None else lg_c[:, :, t_lo:t_hi], obs=ob_c[:, t_lo:t_hi], rows=rows)
        dv = torch.view_as_complex(d) if form == "plain" else d
        wv = frames_of(whole, form, t_lo, t_hi)
        wv = torch.view_as_complex(wv.contiguous()) if form == "plain" else wv
        r_stream, r_whole = SG.check_call([dv.cpu(), wv.cpu()], d_in.cpu(), dy_c[:, n_lo:n_hi] if st.samples else None,
                                          None if d_ola is None else d_ola.cpu(), st.frames, st.skip, st.samples, what=what,
                                          **cpu)
        assert r_stream == r_whole, (what, r_stream, r_whole)
        worst = max(worst, r_stream)
        # NULL carry: the whole-utterance launch on dy zeroed behind this call's last completed sample, bit for bit; and
        # an all-zero d_ola_out
        d0, d0_in = call_bwd(form, dyc, None, lg, ob, rows, st, last)
        cut = dy.clone()
        cut[:, n_hi:] = 0
        w0 = frames_of(whole_bwd(form, cut, logit, obs, T), form, t_lo, t_hi)
        assert torch.equal(SG.pos_zero(d0), SG.pos_zero(w0)), (what, "NULL carry against the zeroed dy")
        dz, dz_in = call_bwd(form, dyc, torch.zeros(rows, 768, device=DEV), lg, ob, rows, st, last)
        assert torch.equal(dz, d0) and torch.equal(dz_in, d0_in), (what, "NULL against an all-zero d_ola_out")
        # d_ola_in not wanted: the same frames
        dn, none = call_bwd(form, dyc, d_ola, lg, ob, rows, st, last, want_ola=False)
        assert none is None and torch.equal(dn, d), (what, "d_ola_in = NULL")
        ds.insert(0, d)
        d_ola, t_hi, n_hi = d_in, t_lo, n_lo
    assert not bool(d_ola.any()), "the carry in front of a stream is the leading fade: its gradient is zero"
    got = torch.cat(ds, dim=tdim(form))
    assert got.shape == whole.shape
    assert torch.equal(SG.pos_zero(got), SG.pos_zero(whole)), (form, B, K, hops, rest, pushes,
                                                                 float((got - whole).abs().max()))
    return worst


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("B,K", SG.ROWS)
def test_stream_bwd_bits_and_adjoint(form, B, K):
    worst = 0.0
    for hops, pushes, rest in SG.cases():
        worst = max(worst, run_stream(form, B, K, hops, pushes, rest, seed=hops * 1000 + rest + B * 7 + K))
    WORST[form] = max(WORST.get(form, 0.0), worst)
    assert worst <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_a_call_past_one_workgroup(form):
    """Tc = 70 frames in one call: 280 frames of 6 rows, 18 workgroups of 16 frames; a ragged flush behind it."""
    worst = run_stream(form, 2, 3, 70, (70,), 37, seed=70)
    WORST[form + " Tc=70"] = worst
    assert worst <= 1.0


@pytest.mark.parametrize("form", FORMS)
def test_single_calls_with_a_random_carry_gradient(form):
    """A d_ola_out chained from a later call is zero on the hops that lie before the utterance's first sample; a caller may
    differentiate the carry with anything.  Every (Tc, skip) with Tc = 1 .. 5, skip = 0 .. 3 -- skip > Tc among them, where
    the hops Tc .. skip - 1 are d_ola_out's, not zeros -- whole and ragged, with random dy and random d_ola_out: dX / dlogit
    inside the measure against the float64 adjoint, d_ola_in the exact copy."""
    from tssep_amd.train.online import Step
    B, K = 2, 3
    rows = B * K
    worst = 0.0
    for Tc in range(1, 6):
        for skip in range(4):
            hops = max(Tc - skip, 0)
            for n, last in ((hops * 256, False),) + (((hops - 1) * 256 + 37, True),) * (hops > 0):
                logit, obs, dy = make(form, B, K, Tc, max(n, 1), seed=100 * Tc + 10 * skip + last)
                g = torch.Generator().manual_seed(7 * Tc + skip)
                carry = (torch.randn(rows, 768, generator=g) * 3).to(DEV)
                st = Step(Tc, skip, n)
                d, d_in = call_bwd(form, dy[:, :n], carry, logit, obs, rows, st, last)
                dv = torch.view_as_complex(d) if form == "plain" else d
                r = SG.check_call(dv.cpu(), d_in.cpu(), dy[:, :n].cpu() if n else None, carry.cpu(), Tc, skip, n,
                                  None if logit is None else logit.cpu(), obs.cpu(), rows, what=f"{form} single call {st}")
                worst = max(worst, r)
    WORST[form + " random carry"] = worst
    assert worst <= 1.0


def test_guards_refuse_before_any_launch():
    ws, tw = tables()
    dy, dout, din = torch.zeros(2, 256 + 2, device=DEV), torch.zeros(2 * 768 + 2, device=DEV), nans(2 * 768 + 2)
    dX, lg, ob = nans(2, 4, 513, 2), torch.zeros(1, 2, 4, 513, device=DEV), torch.zeros(1, 4, 513, 2, device=DEV)
    dl = nans(1, 2, 4, 513)

    def plain(dy_=dy, yoff=0, do=dout, dooff=0, di=din, dioff=0, Tc=4, size=1024, shift=256, skip=3, last=0, n=256, dX_=dX,
              rows=2):
        return L().tssep_istft_stream_bwd(p(dy_, yoff), p(do, dooff), rows, Tc, size, shift, p(ws), p(tw), skip, last, n, p(dX_),
                                          p(di, dioff), stream())

    def masked(dy_=dy, do=dout, dooff=0, di=din, lg_=lg, ob_=ob, oboff=0, K=2, Tc=4, size=1024, shift=256, skip=3, last=0, n=256,
               dl_=dl, gated=0):
        return L().tssep_mask_istft_stream_bwd(p(dy_), p(do, dooff), p(lg_), gated, p(ob_, oboff), 1, K, Tc, size, shift, p(ws),
                                               p(tw), skip, last, n, p(dl_), p(di), stream())

    for f in (plain, masked):
        assert f(size=512, shift=128) == E_UNSUPPORTED and f(size=2048, shift=512) == E_UNSUPPORTED       # the plan
        assert f(Tc=0) == E_SHAPE and f(n=200) == E_SHAPE and f(n=512) == E_SHAPE and f(skip=4) == E_SHAPE   # shapes
        assert f(last=1, n=0) == E_SHAPE and f(last=1, n=257) == E_SHAPE and f(Tc=2, n=256) == E_SHAPE
        assert f(di=dout) == E_SHAPE                                                                      # overlap
        assert f(dy_=None) == E_NULL
        assert f(do=dout, dooff=4) == E_ALIGN                                                             # alignment
    assert plain(dX_=None) == E_NULL and plain(rows=0) == E_SHAPE
    assert plain(yoff=2) == E_ALIGN and plain(dioff=2) == E_ALIGN
    assert masked(lg_=None) == E_NULL and masked(ob_=None) == E_NULL and masked(dl_=None) == E_NULL and masked(K=0) == E_SHAPE
    assert masked(oboff=4) == E_ALIGN
    torch.cuda.synchronize()
    for t in (dX, dl, din):
        assert bool(torch.isnan(t).all()), "a refused call wrote"


def test_zz_report():
    for k, v in WORST.items():
        print(f"stream backward against the float64 adjoint, worst err / tol  {k}: {v:.3g}")
