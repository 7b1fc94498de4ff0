"""tssep_lstm1_bwd_state / tssep_gru1_bwd_state (the one-direction backward recurrences with the carried state's gradient)
on a real MI355X, against the float64 checkers of tests/state_grad_reference.py (derivations there).

Shapes: N in {1, 8, 9} (8: one workgroup, 9: a ragged second one), T in {1, 2, 7} (T = 1: a step that is first and last
at once), H in {5, 64, 65, 300}, and H = 512 once.  The saved activations come from the forward kernels started at a
random nonzero state; every output is written over NaN.

1. LSTM, bit for bit.  The whole-sequence launch over T = 7 (with c0, dhT, dcT) gives d(gates), dh0, dc0.  The same
   sequence backwards as chunks 1|6, 3|4, 6|1 and 7 x 1, the last chunk first, each chunk with c0 = cell of the frame before
   it and (dhT, dcT) = the (dh0, dc0) the later chunk wrote: its d(gates) and the first chunk's (dh0, dc0) are the whole
   launch's bits.  A wrong dh0, dc0, c0 or dhT anywhere breaks an earlier chunk.
2. LSTM, bounds.  Every element of d(gates), dh0 and dc0 within check_lstm1_backward's bound, random and saturated gates.
3. GRU.  Step by step within check_gru1_backward's bounds with nonzero h0 and dhT; the chunked runs of 1. step by step
   within the same bounds (each chunk against the inputs it was handed) and, concatenated, against the float64 loop over the
   whole sequence within whole_sequence_multiple("stream", H) = 4 times the fp32 torch loop's error -- NOT bit for bit: the
   whole launch forms (parts + dhout) + carry, a chunk boundary hands parts + carry over as one tensor.
4. All-null state arguments give the bits of tssep_lstm1_bwd / tssep_gru1_bwd.
5. Guards decline before anything is launched.

Worst error / bound measured on an MI355X over this file (pytest -rP, test_zz_report): LSTM d(gates) 0.50, dh0 0.034, dc0
0.55; GRU d(gates) 0.37, dh0 0.11; GRU against the float64 loop over the whole sequence, kernel error / fp32 torch error
(allowed 4): d(gates) 0.52, dh0 0.57."""
import pytest
import torch

import gru_reference as G
import state_grad_reference as S
from tssep_amd import _lib, hip_ops as Hop
from test_recurrence_reference import U, whole_sequence_multiple
from test_gpu_recurrence_kernels import DEV, GIB, NAN

pytestmark = pytest.mark.gpu
E_SHAPE, E_ALIGN, E_UNSUPPORTED, E_NULL = -1, -2, -3, -5
EXTRA = 4           # pad columns of hout / dhout beyond Hp
WORST = {}          # (cell, output) -> largest error / bound of this run
F64, F32 = torch.float64, torch.float32
SPLITS = ([1, 6], [3, 4], [6, 1], [1] * 7)
GRID = [(N, T, H) for N in (1, 8, 9) for T in (1, 2, 7) for H in (5, 64, 65, 300)] + [(9, 2, 512)]


@pytest.fixture(autouse=True)
def _device_memory_cap():
    """The GPU is shared: every test here stays under 16 GB of device memory at its peak."""
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    torch.cuda.empty_cache()
    assert peak < 16 * GIB, f"peak device memory {peak / GIB:.1f} GiB"


def nan(*shape):
    return torch.full(shape, NAN, device=DEV)


class Case:
    """One sequence batch of one cell kind: the forward kernel's saved activations from a random state, and the backward's
    inputs.  klass "sat": every pre-activation is +30 or -30."""

    def __init__(self, N, T, H, gru, seed=0, klass="randn"):
        self.N, self.T, self.H, self.gru = N, T, H, gru
        gen = torch.Generator(device=DEV).manual_seed(1000 * seed + 7 * N + 3 * T + H + int(gru))
        rnd = lambda *s: torch.randn(*s, device=DEV, generator=gen)  # noqa: E731
        self.ld = Hop.round_up(H, 4) + EXTRA
        gin = rnd(N, T, H, 4)
        if klass == "sat":
            gin = 30.0 * torch.sign(gin)
        self.h0 = torch.rand(N, H, device=DEV, generator=gen) * 2 - 1
        self.c0 = None if gru else rnd(N, H)
        self.dhT = rnd(N, H)
        self.dcT = None if gru else rnd(N, H)
        self.dhout = nan(N, T, self.ld)
        self.dhout[..., :H] = rnd(N, T, H)
        self.A, self.hout, self.cell = gin.clone(), nan(N, T, self.ld), None
        z = torch.zeros((3 if gru else 4) * H, 4, device=DEV)
        b = torch.zeros((3 if gru else 4) * H, device=DEV)
        if gru:
            self.whh = G.make_gru_whh(H, 1, gen, DEV)[0]
            self.pk = Hop.gru_pack([z, self.whh, b, b], H, 4)
            Hop.gru_fwd(self.A, self.hout, self.ld, 0, self.pk["whh_f"], N, T, H, directions=1, h0=self.h0)
        else:
            self.whh = (torch.rand(4 * H, H, device=DEV, generator=gen) * 2 - 1) * H ** -0.5
            self.pk = Hop.lstm1_pack([z, self.whh, b, b], H, 4)
            self.cell = nan(N, T, H)
            Hop.lstm1_fwd(self.A, self.cell, self.hout, self.ld, self.pk["whh_f"], N, T, H, self.h0, self.c0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(self.A).all())

    def before(self, t0):
        """the state the forward had in front of frame t0: (h, c) or (h,)"""
        if t0 == 0:
            return self.h0, self.c0
        return self.hout[:, t0 - 1, :self.H].contiguous(), None if self.gru else self.cell[:, t0 - 1].contiguous()

    def launch(self, t0, t1, dlast, want=True):
        """one backward launch over the frames t0 .. t1 - 1 with dlast = (dhT, dcT) -> (what it read, d(gates), (dh0, dc0))"""
        N, H, n = self.N, self.H, t1 - t0
        A = self.A[:, t0:t1].contiguous()
        D = A.clone()          # (overwritten in place; a slice of one sequence is contiguous as it is: never the case's own tensor)
        dh = self.dhout[:, t0:t1].contiguous()
        h_in, c_in = self.before(t0)
        dh0 = nan(N, H) if want else None
        if self.gru:
            hout = self.hout[:, t0:t1].contiguous()
            Hop.gru1_bwd(D, hout, dh, self.ld, self.pk["whh_b"], N, n, H, h0=h_in, dhT=dlast[0], dh0=dh0)
            read, out = dict(A=A, hout=hout, dhout=torch.nan_to_num(dh), h0=h_in, dhT=dlast[0]), (dh0,)
        else:
            cell = self.cell[:, t0:t1].contiguous()
            dc0 = nan(N, H) if want else None
            Hop.lstm1_bwd(D, cell, dh, self.ld, self.pk["whh_b"], N, n, H, c0=c_in, dhT=dlast[0], dcT=dlast[1], dh0=dh0, dc0=dc0)
            read, out = dict(A=A, cell=cell, dhout=torch.nan_to_num(dh), c0=c_in, dhT=dlast[0], dcT=dlast[1]), (dh0, dc0)
        torch.cuda.synchronize()
        return read, D, out

    def check(self, read, D, out, what=""):
        """every element of one launch within the derived bounds"""
        if self.gru:
            w = S.check_gru1_backward(read["A"], read["hout"], read["dhout"], D, self.whh, self.H, read["h0"], read["dhT"], out[0])
        else:
            w = S.check_lstm1_backward(read["A"], read["cell"], read["dhout"], D, self.whh, self.H, read["c0"], read["dhT"],
                                       read["dcT"], *out)
        n = D.shape[1]
        print(f"{'gru1' if self.gru else 'lstm1'} bwd_state N={self.N} T={n} H={self.H} {what}: {w}")
        assert w.ok() and w.count == self.N * n * self.H * 4, str(w)
        for name, v in w.ratio.items():
            key = ("gru1" if self.gru else "lstm1", name)
            WORST[key] = max(WORST.get(key, 0.0), v)
        return w

    def chunked(self, split, check=False):
        """the sequence backwards as chunks, the last chunk first -> (d(gates) of all frames, the first chunk's (dh0, dc0))"""
        dlast, parts, t1 = (self.dhT, self.dcT), [], self.T
        for n in reversed(split):
            read, D, out = self.launch(t1 - n, t1, dlast)
            if check:
                self.check(read, D, out, f"chunk {t1 - n}..{t1}")
            parts.insert(0, D)
            dlast = (out[0], None) if self.gru else out
            t1 -= n
        assert t1 == 0
        return torch.cat(parts, 1), out


# ---- 1. the LSTM hand-over is exact --------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H", [(N, H) for N in (1, 8, 9) for H in (5, 64, 65, 300)] + [(9, 512)])
def test_lstm_chunks_reproduce_the_whole_launch_bit_for_bit(N, H):
    c = Case(N, 7, H, False, seed=3)
    _, whole, (dh0, dc0) = c.launch(0, 7, (c.dhT, c.dcT))
    assert all(bool(torch.isfinite(x).all()) for x in (whole, dh0, dc0))
    for split in SPLITS:
        D, out = c.chunked(split)
        assert torch.equal(D, whole), (split, float((D - whole).abs().max()))
        assert torch.equal(out[0], dh0) and torch.equal(out[1], dc0), split
    # and every hand-over matters: without the state's side the chunks differ
    _, plain, _ = c.launch(0, 7, (None, None))
    assert not torch.equal(plain, whole)


# ---- 2. / 3. every element within the derived bounds ---------------------------------------------------------------------
@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("N,T,H", GRID)
def test_step_by_step(N, T, H, gru):
    c = Case(N, T, H, gru, seed=1)
    c.check(*c.launch(0, T, (c.dhT, c.dcT)))


@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
def test_saturated_gates(gru):
    c = Case(9, 7, 300, gru, seed=2, klass="sat")
    c.check(*c.launch(0, 7, (c.dhT, c.dcT)), what="saturated")


@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
def test_outputs_that_are_not_asked_for_are_not_needed(gru):
    """dh0 / dc0 null: d(gates) are the bits of the launch that writes them"""
    c = Case(9, 7, 65, gru, seed=4)
    _, a, _ = c.launch(0, 7, (c.dhT, c.dcT))
    _, b, out = c.launch(0, 7, (c.dhT, c.dcT), want=False)
    assert torch.equal(a, b) and all(o is None for o in out)


@pytest.mark.parametrize("N,H", [(9, 300), (8, 65), (1, 5), (9, 64)])
def test_gru_chunks_against_the_whole_sequence(N, H):
    c = Case(N, 7, H, True, seed=3)
    M = whole_sequence_multiple("stream", H)
    assert M == 4.0
    dh = c.dhout[..., :H].contiguous()
    args = (c.A, c.hout[..., :H].contiguous(), dh, c.whh, H)
    ref, ref0 = S.gru1_backward_loop(*args, F64, c.h0, c.dhT)
    t32, t320 = S.gru1_backward_loop(*args, F32, c.h0, c.dhT)
    _, whole, (whole0,) = c.launch(0, 7, (c.dhT, None))
    runs = [("whole", whole, whole0)] + [("-".join(map(str, s)), *c.chunked(s, check=True)) for s in SPLITS]
    for name, D, out in runs:
        out = out[0] if isinstance(out, tuple) else out
        for what, k, r, t in (("dgates", D, ref, t32), ("dh0", out, ref0, t320)):
            ek, et = float((k.double() - r).abs().max()), float((t.double() - r).abs().max())
            floor = 4 * U * float(r.abs().max())
            print(f"gru1 N={N} H={H} {name} {what}: kernel {ek:.3g}, fp32 torch {et:.3g}, ratio {ek / max(et, 1e-30):.3g} (allowed {M:.3g})")
            WORST[("gru1", "whole " + what)] = max(WORST.get(("gru1", "whole " + what), 0.0), ek / max(et, floor))
            assert ek <= M * et + floor, (name, what, ek, et)


# ---- 4. nulls ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,T,H", [(9, 7, 300), (1, 1, 5), (8, 2, 65)])
def test_all_null_state_arguments_are_the_entry_points_without_a_state(N, T, H):
    L, s = _lib.lib(), Hop._stream()
    p = Hop._p
    for gru in (False, True):
        c = Case(N, T, H, gru, seed=6)
        dh = torch.nan_to_num(c.dhout)
        a, b = c.A.clone(), c.A.clone()
        if gru:
            assert L.tssep_gru1_bwd(p(a), p(c.hout), p(dh), c.ld, p(c.pk["whh_b"]), N, T, H, s) == 0
            assert L.tssep_gru1_bwd_state(p(b), p(c.hout), p(dh), c.ld, p(c.pk["whh_b"]), None, None, None, N, T, H, s) == 0
        else:
            assert L.tssep_lstm1_bwd(p(a), p(c.cell), p(dh), c.ld, p(c.pk["whh_b"]), N, T, H, s) == 0
            assert L.tssep_lstm1_bwd_state(p(b), p(c.cell), p(dh), c.ld, p(c.pk["whh_b"]), None, None, None, None, None,
                                           N, T, H, s) == 0
        torch.cuda.synchronize()
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and not torch.equal(a, c.A)
        # and a launch with a state is logged under the name of one without
        log = Hop.RECURRENCE_LOG = []
        try:
            c.launch(0, T, (c.dhT, c.dcT))
        finally:
            Hop.RECURRENCE_LOG = None
        assert [(e["kernel"], e["direction"], e["sequences"], e["frames"], e["units"]) for e in log] == \
            [("stream1_gru_f32" if gru else "stream1_f32", "bwd", N, T, H)]


# ---- 5. guards -----------------------------------------------------------------------------------------------------------
def test_guards_decline_before_anything_is_launched():
    L = _lib.lib()
    buf = torch.zeros(1 << 16, device=DEV)
    p, odd, s = Hop._p(buf), Hop._p((buf, 1)), Hop._stream()
    N, T, H, ld = 2, 3, 5, 8

    def lstm(gates=p, cell=p, dhout=p, ldo=ld, whh=p, N=N, T=T, H=H):
        return L.tssep_lstm1_bwd_state(gates, cell, dhout, ldo, whh, p, p, p, p, p, N, T, H, s)

    def gru(gates=p, hout=p, dhout=p, ldo=ld, whh=p, N=N, T=T, H=H):
        return L.tssep_gru1_bwd_state(gates, hout, dhout, ldo, whh, p, p, p, N, T, H, s)

    for fn, names in ((lstm, ("gates", "cell", "dhout", "whh")), (gru, ("gates", "hout", "dhout", "whh"))):
        for name in names:
            assert fn(**{name: None}) == E_NULL, (fn.__name__, name)
        for dim in ("N", "T", "H"):
            for v in (0, -1):
                assert fn(**{dim: v}) == E_SHAPE, (fn.__name__, dim, v)
        assert fn(ldo=H - 1) == E_SHAPE
        assert fn(gates=odd) == E_ALIGN and fn(whh=odd) == E_ALIGN
        assert fn(H=513, ldo=516) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert float(buf.abs().max()) == 0.0, "a refused call wrote"


def test_zz_report():
    """the largest error / bound of every output this run saw (pytest -rP)"""
    for (cell, name), v in sorted(WORST.items()):
        print(f"{cell:6s} {name:14s} {v:.3g}")
