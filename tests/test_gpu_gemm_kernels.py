"""The GEMM family (gemm.hip, gemm_bf16x3*.hip: 16 kernels behind gemm_dispatch.h) against float64 references computed on
the device from the same fp32 operands, at the training step's own requests and on both sides of every 2 GB guard.

1. Exact group.  Operand entries are integers in [-3, 3] times 2^e, with one exponent e in [-20, 20] per row of the
   output (M) and one per column (N), never along K.  Such values are bf16-exact, so split2n (gemm_common.h) gives
   lo = 0; every product is an integer of magnitude <= 9 times the element's own power of two, and every partial sum
   is an integer below 9 * 777 216 < 2^24 times it.  Every fp32 partial of every summation order and every split is
   therefore exact, and so is the result: it must equal the float64 product bit for bit.  Epilogues keep that:
     * bias (and the prior C of accumulate): integers in [-64, 64] times the column's 2^eN, with row exponents
       restricted to [-8, 8]: 2^eN (2^eM S + b) then spans at most 24 bits (|S| < 2^15 for K <= 2 400);
     * act = 2: y in {0, +-1/4, +-1/2, +-3/4}, so 1 - y^2 has at most 4 significant bits and S (1 - y^2) at most 19;
     * act = 1: the pre-activation is exact (row exponents in [0, 2], column exponents in [-8, -4], so it spans about
       [-8, 8]) and the Tanh of the store is compared with float64 tanh within TANH_ERR = 3e-7, the absolute error
       gemm_common.h claims for gemm_tanh -- a claim checked here on its own by K = 1 requests whose pre-activations
       are the 2^20 multiples of 2^-15 in [-16, 16).
   Split-K partials are summed in float64 (exact: each partial is exact).  The virtual ones column of b_ones_col is the
   float64 column sum of dY.  Outputs are pre-filled with NaN; every element a request writes must be finite, and a
   remapped store must write exactly M x N elements of its buffer.  Bytes a request must not read (pad columns, rows
   past K) hold 4096.0: read by mistake, they change a sum.
   Cases: every distinct request of one forward + backward of the default model (units 300, projs 320, 4 speakers)
   at batch 768 -- HEADLINE, which test_headline_table_is_the_step_s_requests keeps equal to a live GEMM log -- on
   the library's choice and on every kernel that covers it (tssep_gemm_plan), in precision 1 (split-bf16, the
   default), 0 (exact fp32), 2 (weight gradients without dY_lo * X_hi) and 3 (plain bf16).

2. Arithmetic group.  Random full-mantissa operands (lo != 0), each row scaled by 10^u, u uniform in [-3, 3]: the
   nt requests at their own K with M = 24 576 rows, the weight gradients over R = 24 288 rows at the library's split
   count.  Per output element (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.; Higham and Mary,
   SIAM J. Sci. Comput. 41 (2019) A2815 for the probabilistic term):
     * split product.  x = xh + xl + ex with xh = bf16(x), xl = bf16(x - xh) (x - xh is exact in fp32), so
       |x - xh| <= 2^-8 |x|, |ex| <= 2^-8 |x - xh| <= 2^-16 |x|, |xl| <= 2^-8 (1 + 2^-8) |x|.  The kernels sum
       ah bh + ah bl + al bh; the dropped part al bl + (ah + al) eb + ea (bh + bl) + ea eb is at most
       (3 + 2^-7 + 2^-15) 2^-16 |a| |b| <= C_SPLIT |a| |b|, C_SPLIT = 3.01 * 2^-16.  The bf16 products themselves
       are exact in fp32.  Summed: C_SPLIT (|A| |B|^T)_ij.  (Precision 0 has no split: C_SPLIT = 0.)
     * fp32 accumulation.  The three products of a k go into the same accumulator, so a split of length L makes
       n = 3 L + S additions with the S-way reduction (n = L + S in precision 0); with lambda = LAMBDA = 9 the error
       is at most lambda sqrt(n) U (|A| |B|^T)_ij except with probability 2 n exp(-lambda^2 / 2) < 1e-13 per element.
     * the rounded store U |c|; a bias adds U (|c| + |b|); the Tanh adds TANH_ERR (it is 1-Lipschitz); act = 2
       scales by 1 - y^2 <= 1 and adds 3 U |c| for y^2, 1 - y^2 and the product.
   Dropping the hi x lo product leaves an error of about 2^-9 |a b| per term, a random walk of sqrt(K) terms, against
   the bound's (C_SPLIT + LAMBDA sqrt(3 K) U) K mean|a b|: an estimated 4 to 16 times the bound at K = 2 400 .. 320.  The largest
   err / tol of every kernel is printed (pytest -rP).

3. Guard group.  Every split-bf16 launcher declines a request whose 32-bit buffer offsets could pass 2 GB; the
   dispatcher then takes the next candidate.  For each guard GUARDS derives, from the launcher's own formula, the
   first value past it (a leading dimension, a batch stride or the rows of one split) and the one just below.  Host
   side (no GPU: tssep_gemm_plan is a query): below, the kernel takes the request; past, it declines and the automatic
   choice is the named fallback.  On the GPU, with the exact operands of group 1 and every case under 12 GB: past,
   the automatic choice and every kernel still covering the request are exact; below, the guarded kernel is.  The
   weight-gradient cases force splitk = 1, where one split spans the whole reduction.  Three guards cannot be run
   under 16 GB; their plan-only halves still run:
     * gemm_bf16x3_bigp.hip, aux (130 ldaux 4 B): the aux operand of M >= 1 024 rows spans >= 16.9 GB;
     * gemm_bf16x3_bigp320.hip, aux (98 ldaux 4 B): >= 16.8 GB likewise (and the dispatcher needs M >= 1 024);
     * gemm_bf16x3_stream.hip, C (40 ldc 4 B): C of M >= 1 024 rows spans >= 55 GB."""
import ctypes
import json
import math
import os
import sys
import zlib

import pytest
import torch

from tssep_amd import _lib, hip_ops as H

U = 2.0 ** -24
DEV = "cuda"
NAN = float("nan")
PAD = 4096.0                    # operand bytes a request must not read
TANH_ERR = 3e-7                 # gemm_common.h: gemm_tanh's absolute error
C_SPLIT = 3.01 * 2.0 ** -16     # split-bf16 product error per |a| |b|, derived above
LAMBDA = 9.0
TWO_GB = 1 << 31
ROWS = 32768                    # row block of the references and comparisons

_DEFAULTS = dict(a_kmajor=0, accumulate=0, act=0, b_kmajor=0, b_kshift=0, b_ones_col=0, bias=False, c_K=0, c_T=0, c_cm=0,
                 c_co=0, c_perm_ld=0, c_remap=0, c_sb=0, c_sk=0, c_split_stride=0, c_st=0, has_aux=False, kperiod=0,
                 ldaux=0, ldc=0, perm=False, precision=1, splitk=1)


def _req(M, N, K, lda, ldb, **kw):
    """A pointer-free request: the fields of hip_ops.gemm_descriptor."""
    assert set(kw) <= set(_DEFAULTS), set(kw) - set(_DEFAULTS)
    return dict(_DEFAULTS, M=M, N=N, K=K, lda=lda, ldb=ldb, **kw)


# Every distinct GEMM request of one forward + backward of the default model at batch 768 (tools/sweep_gemm_shapes.py
# requests_of_a_step; kept equal to the live log by test_headline_table_is_the_step_s_requests).
HEADLINE = [
    _req(194304, 2400, 553, 556, 556, bias=True, ldc=2400),
    _req(194304, 513, 600, 600, 600, bias=True, ldc=516),
    _req(777216, 2400, 513, 516, 516, bias=True, ldc=2400),
    _req(777216, 320, 600, 600, 600, act=1, bias=True, ldc=320),
    _req(777216, 2400, 320, 320, 320, bias=True, ldc=2400),
    _req(777216, 320, 600, 600, 600, act=1, bias=True, c_K=4, c_T=253, c_remap=1, c_sb=323840, c_sk=320, c_st=1280),
    _req(194304, 2400, 1280, 1280, 1280, bias=True, ldc=2400),
    _req(194304, 320, 600, 600, 600, bias=True, ldc=320),
    _req(194304, 2052, 320, 320, 320, bias=True, c_K=1, c_T=253, c_cm=513, c_co=129789, c_perm_ld=4, c_remap=1,
         c_sb=519156, c_st=513, perm=True),
    _req(2052, 320, 194304, 2052, 320, a_kmajor=1, b_kmajor=1, c_split_stride=656640, ldc=320, splitk=56),
    _req(194304, 320, 2052, 2052, 2052, ldc=320),
    _req(320, 600, 194304, 320, 600, a_kmajor=1, b_kmajor=1, c_split_stride=192000, ldc=600, splitk=80),
    _req(194304, 600, 320, 320, 320, ldc=600),
    _req(1200, 300, 194304, 2400, 600, a_kmajor=1, b_kmajor=1, b_kshift=-1, c_split_stride=360000, kperiod=253,
         ldc=300, splitk=48),
    _req(1200, 300, 194304, 2400, 600, a_kmajor=1, b_kmajor=1, b_kshift=1, c_split_stride=360000, kperiod=253,
         ldc=300, splitk=48),
    _req(2400, 1281, 194304, 2400, 1280, a_kmajor=1, b_kmajor=1, b_ones_col=1, c_split_stride=3081600, ldc=1284,
         splitk=24),
    _req(194304, 1280, 2400, 2400, 2400, act=2, c_K=1, c_T=253, c_cm=320, c_co=80960, c_remap=1, c_sb=323840, c_st=320,
         has_aux=True, ldaux=1280),
    _req(320, 600, 777216, 320, 600, a_kmajor=1, b_kmajor=1, c_split_stride=192000, ldc=600, splitk=80),
    _req(777216, 600, 320, 320, 320, ldc=600),
    _req(1200, 300, 777216, 2400, 600, a_kmajor=1, b_kmajor=1, b_kshift=-1, c_split_stride=360000, kperiod=253,
         ldc=300, splitk=48),
    _req(1200, 300, 777216, 2400, 600, a_kmajor=1, b_kmajor=1, b_kshift=1, c_split_stride=360000, kperiod=253,
         ldc=300, splitk=48),
    _req(2400, 321, 777216, 2400, 320, a_kmajor=1, b_kmajor=1, b_ones_col=1, c_split_stride=777600, ldc=324, splitk=24),
    _req(777216, 320, 2400, 2400, 2400, act=2, has_aux=True, ldaux=320, ldc=320),
    _req(2400, 514, 777216, 2400, 516, a_kmajor=1, b_kmajor=1, b_ones_col=1, c_split_stride=1238400, ldc=516,
         splitk=24),
    _req(777216, 513, 2400, 2400, 2400, ldc=516),
    _req(513, 600, 194304, 516, 600, a_kmajor=1, b_kmajor=1, c_split_stride=307800, ldc=600, splitk=32),
    _req(194304, 600, 513, 516, 516, ldc=600),
    _req(2400, 554, 194304, 2400, 556, a_kmajor=1, b_kmajor=1, b_ones_col=1, c_split_stride=1334400, ldc=556,
         splitk=24),
]


def _name(d):
    lay = "tn" if d["a_kmajor"] else "nt"
    tags = [t for t, on in (("bias", d["bias"]), ("tanh", d["act"] == 1), ("dtanh", d["act"] == 2),
                            ("acc", d["accumulate"]), ("remap", d["c_remap"]), ("perm", d["perm"]),
                            ("ones", d["b_ones_col"]), (f"shift{d['b_kshift']:+d}", d["kperiod"]),
                            (f"S{d['splitk']}", d["splitk"] > 1)) if on]
    return "-".join([f"{lay}{d['M']}x{d['N']}x{d['K']}"] + tags)


def _key(d):
    return json.dumps(d, sort_keys=True)


def _padded(rows, ld):
    """[rows, ld] of PAD with 16 KB of PAD behind it: a masked 16-byte load past the last row stays in the buffer"""
    return torch.full((rows * ld + 4096,), PAD, device=DEV)[:rows * ld].view(rows, ld)


def _pow2(n, lo, hi, gen):
    return torch.exp2(torch.randint(lo, hi + 1, (n,), device=DEV, generator=gen).float())


class Problem:
    """Operands, epilogue inputs and output buffer of one request `d`.  exact=True: the integer operands of the exact
    group; False: random full-mantissa operands with rows scaled by 10^u (the arithmetic group)."""

    def __init__(self, d, exact=True, seed=0):
        self.d, self.exact = d, exact
        M, N, K = d["M"], d["N"], d["K"]
        assert not (d["b_kmajor"] and not d["a_kmajor"]), "nn requests: not in the step"
        self.tn = bool(d["a_kmajor"])
        self.nr = N - d["b_ones_col"]
        gen = self.gen = torch.Generator(device=DEV).manual_seed(seed)
        if exact:
            if d["act"] == 1:
                em, en = (0, 2), (-8, -4)
            elif d["bias"] or d["accumulate"]:
                em, en = (-8, 8), (-20, 20)
            else:
                em, en = (-20, 20), (-20, 20)
            self.sm, self.sn = _pow2(M, *em, gen), _pow2(self.nr, *en, gen)
        if self.tn:
            rows = K + 64                       # (a time-shifted B reads past row K - 1 by design, masked)
            self.A, self.B = _padded(rows, d["lda"]), _padded(rows, d["ldb"])
            a, b = self.A[:K, :M], self.B[:K, :self.nr]
        else:
            self.A, self.B = _padded(M, d["lda"]), _padded(N, d["ldb"])
            a, b = self.A[:, :K], self.B[:, :K]
        if exact:
            for x, s in ((a, self.sm), (b, self.sn)):
                x.random_(0, 7, generator=gen).sub_(3)
                x.mul_(s[None, :] if self.tn else s[:, None])
        else:
            for x in (a, b):
                x.normal_(generator=gen)
                u = torch.rand(x.shape[0], 1, device=DEV, generator=gen) * 6 - 3
                x.mul_(torch.pow(10.0, u))
        self.bias = self.prior = self.aux = self.perm = None
        if d["bias"]:
            self.bias = self._colvalues(16 if d["act"] == 1 else 64)
        if d["has_aux"]:
            self.aux = _padded(M, d["ldaux"])
            if exact:
                self.aux[:, :N] = (torch.randint(-3, 4, (M, N), device=DEV, generator=gen) * 0.25).float()
            else:
                self.aux[:, :N] = torch.tanh(torch.randn(M, N, device=DEV, generator=gen) * 2)
        if d["perm"]:
            q = -(-N // d["c_cm"])
            assert d["c_perm_ld"] == q
            self.perm = torch.stack([torch.randperm(q, device=DEV, generator=gen) for _ in range(self._utterances())]).int()
        if d["accumulate"]:
            self.prior = torch.randint(-64, 65, (M, N), device=DEV, generator=gen).float() * self.sn
        self.C = torch.empty(self._celems(), device=DEV)

    def _colvalues(self, r):
        v = torch.randint(-r, r + 1, (self.d["N"],), device=DEV, generator=self.gen).float()
        if self.exact:
            v *= self.sn
        else:
            v = torch.randn(self.d["N"], device=DEV, generator=self.gen)
        return v

    def _utterances(self):
        d = self.d
        return -(-d["M"] // (max(d["c_T"], 1) * max(d["c_K"], 1)))

    def _celems(self):
        d = self.d
        if d["splitk"] > 1:
            return d["splitk"] * d["c_split_stride"]
        if d["c_remap"]:
            T, Kc = max(d["c_T"], 1), max(d["c_K"], 1)
            cm = d["c_cm"] or d["N"]
            last = ((d["M"] - 1) // (T * Kc)) * d["c_sb"] + (Kc - 1) * d["c_sk"] + (T - 1) * d["c_st"] + \
                ((d["N"] - 1) // cm) * d["c_co"] + cm
            return max(last, self._utterances() * d["c_sb"]) + 4096
        return d["M"] * d["ldc"]

    def args(self, precision):
        g = _lib.GemmArgs()
        for f, _ in _lib.GemmArgs._fields_:
            if f in self.d:
                setattr(g, f, self.d[f])
        g.A, g.B, g.C = self.A.data_ptr(), self.B.data_ptr(), self.C.data_ptr()
        g.bias = self.bias.data_ptr() if self.bias is not None else None
        g.aux = self.aux.data_ptr() if self.aux is not None else None
        g.c_perm = self.perm.data_ptr() if self.perm is not None else None
        g.precision = precision
        return g

    # ---- float64 references ------------------------------------------------------------------------------------------
    def _b_rows(self, k0, k1):
        """rows k0..k1 of the B operand as the tn kernels read it (time shift applied), float64"""
        d = self.d
        if not d["kperiod"]:
            return self.B[k0:k1, :self.nr].double()
        k = torch.arange(k0, k1, device=DEV)
        ph = k % d["kperiod"] + d["b_kshift"]
        ok = (ph >= 0) & (ph < d["kperiod"])
        src = (k + d["b_kshift"]).clamp(0, self.B.shape[0] - 1)
        return self.B[src, :self.nr].double() * ok[:, None]

    def products(self, absolute=False):
        """-> float64 [M, N] of op(A) op(B) (absolute: |A| |B|), the ones column included; before the epilogue"""
        d = self.d
        M, N, K = d["M"], d["N"], d["K"]
        f = (lambda x: x.abs()) if absolute else (lambda x: x)
        if self.tn:
            out = torch.zeros(M, N, device=DEV, dtype=torch.float64)
            for k0 in range(0, K, ROWS):
                k1 = min(K, k0 + ROWS)
                a = f(self.A[k0:k1, :M].double())
                out[:, :self.nr] += a.t() @ f(self._b_rows(k0, k1))
                if d["b_ones_col"]:
                    out[:, N - 1] += a.sum(0)
            return out
        b = f(self.B[:, :K].double()).t()
        out = torch.empty(M, N, device=DEV, dtype=torch.float64)
        for m0 in range(0, M, ROWS):
            m1 = min(M, m0 + ROWS)
            out[m0:m1] = f(self.A[m0:m1, :K].double()) @ b
        return out

    def epilogue(self, p, m0, m1):
        """float64 rows m0..m1 of the stored value from the products p (act = 1: the pre-activation)"""
        if self.bias is not None:
            p = p + self.bias.double()
        if self.prior is not None:
            p = p + self.prior[m0:m1].double()
        if self.d["act"] == 2:
            y = self.aux[m0:m1, :self.d["N"]].double()
            p = p * (1 - y * y)
        return p

    def exact_reference(self):
        """-> fp32 [M, N] equal to the float64 result (asserted), act = 1: the exact pre-activation"""
        M = self.d["M"]
        ref = torch.empty(M, self.d["N"], device=DEV)
        if self.tn:
            r = self.epilogue(self.products(), 0, M)
            ref.copy_(r)
            assert torch.equal(ref.double(), r), "operands not exact"
            return ref
        b = self.B[:, :self.d["K"]].double().t()
        for m0 in range(0, M, ROWS):
            m1 = min(M, m0 + ROWS)
            r = self.epilogue(self.A[m0:m1, :self.d["K"]].double() @ b, m0, m1)
            ref[m0:m1] = r
            assert torch.equal(ref[m0:m1].double(), r), "operands not exact"
        return ref

    # ---- the kernel's output -------------------------------------------------------------------------------------------
    def reset_output(self):
        self.C.fill_(NAN)
        if self.prior is not None:
            self.C.view(-1)[:self.d["M"] * self.d["ldc"]].view(self.d["M"], -1)[:, :self.d["N"]] = self.prior

    def output_rows(self, m0, m1):
        """float64 rows m0..m1 of what the request's consumer reads: the tensor, the remapped tensor gathered back, or
        the sum of the split-K partials"""
        d = self.d
        M, N = d["M"], d["N"]
        S = d["splitk"]
        if S > 1:
            part = self.C.view(S, -1)[:, :M * d["ldc"]].view(S, M, d["ldc"])[:, m0:m1, :N]
            assert bool(torch.isfinite(part).all()), "a partial is not finite"
            return part.double().sum(0)
        if d["c_remap"]:
            T, Kc = max(d["c_T"], 1), max(d["c_K"], 1)
            cm = d["c_cm"] or N
            m = torch.arange(m0, m1, device=DEV)
            b = m // (T * Kc)
            row = b * d["c_sb"] + (m // T % Kc) * d["c_sk"] + (m % T) * d["c_st"]
            n = torch.arange(N, device=DEV)
            q = n // cm
            if self.perm is not None:
                q = self.perm.long()[b][:, q]
            off = row[:, None] + q * d["c_co"] + n % cm
            return self.C[off].double()
        return self.C[:M * d["ldc"]].view(M, d["ldc"])[m0:m1, :N].double()

    def run(self, kernel, precision):
        g = self.args(precision)
        self.reset_output()
        L = _lib.lib()
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = L.tssep_gemm_f32(ctypes.byref(g), st) if kernel == "auto" else \
            L.tssep_gemm_f32_on(ctypes.byref(g), H.GEMM_KERNELS[kernel], st)
        assert rc == 0, (kernel, precision, rc)
        torch.cuda.synchronize()

    def check_exact(self, ref, what):
        """the output equals the float64 reference bit for bit (act = 1: within TANH_ERR of tanh)"""
        d = self.d
        worst = 0.0
        for m0 in range(0, d["M"], ROWS):
            m1 = min(d["M"], m0 + ROWS)
            got = self.output_rows(m0, m1)
            assert bool(torch.isfinite(got).all()), (what, "unwritten or non-finite rows in", m0, m1)
            want = ref[m0:m1].double()
            if d["act"] == 1:
                err = float((got - torch.tanh(want)).abs().max())
                worst = max(worst, err)
                assert err <= TANH_ERR, (what, m0, err)
            else:
                bad = got != want
                if bool(bad.any()):
                    i = int(bad.flatten().nonzero()[0])
                    r, c = divmod(i, d["N"])
                    raise AssertionError(f"{what}: {int(bad.sum())} elements differ in rows {m0}..{m1}; first at "
                                         f"({m0 + r}, {c}): {float(got[r, c])!r} != {float(want[r, c])!r}")
        if d["c_remap"]:
            written = int((~torch.isnan(self.C)).sum())
            assert written == d["M"] * d["N"], (what, "remapped store wrote", written, "elements")
        return worst


def _stream_kernels(g):
    return [k for k in H.GEMM_KERNELS if k != "auto" and H.gemm_plan(g, k) is not None]


# ======================================================================================== 1. exact group
_RAN = {}          # request key -> kernels run on it (the coverage test reads it)


def _exact_request(d):
    pr = Problem(d, exact=True, seed=zlib.crc32(_name(d).encode()))
    ref = pr.exact_reference()
    ran = set()
    for prec in (1, 0, 2, 3):
        g = pr.args(prec)
        choice = H.gemm_plan(g, "auto")
        names = _stream_kernels(g)
        if prec == 1:
            assert choice is not None and choice in names, (d, choice)
        if prec == 0:
            assert (choice == "f32") == (not d["b_ones_col"]), (choice, d)
        if prec == 2:
            assert (choice is not None) == pr.tn, (choice, d)
        if prec == 3 and not pr.tn:
            assert choice is not None, d
        if choice is None:
            continue
        for k in ["auto"] + [n for n in names if n != choice]:
            pr.run(k, prec)
            worst = pr.check_exact(ref, (_name(d), k if k != "auto" else f"auto={choice}", f"precision {prec}"))
            if d["act"] == 1:
                print(f"{_name(d)} {k} precision {prec}: max |tanh err| {worst:.2e}")
            ran.add(choice if k == "auto" else k)
    _RAN[_key(d)] = ran
    return ran


@pytest.mark.gpu
@pytest.mark.parametrize("d", HEADLINE, ids=[_name(d) for d in HEADLINE])
def test_headline_request_is_exact_on_every_covering_kernel(d):
    _exact_request(d)
    torch.cuda.empty_cache()


def _tanh_sweep_problem():
    """K = 1: pre-activation (m + 8192 n) 2^-15 - 16 for m < 8192, n < 128 -- every multiple of 2^-15 in [-16, 16)"""
    M, N = 8192, 128
    d = _req(M, N, 1, 4, 4, act=1, bias=True, ldc=N)
    pr = Problem(d, exact=True)
    pr.A[:, 0] = torch.arange(M, device=DEV, dtype=torch.float32) * 2.0 ** -15
    pr.B[:, 0] = 1.0
    pr.bias.copy_(torch.arange(N, device=DEV, dtype=torch.float32) * 0.25 - 16)
    return pr


@pytest.mark.gpu
def test_gemm_tanh_error_claim_on_a_dense_sweep():
    """gemm_common.h: |gemm_tanh(x) - tanh(x)| <= 3e-7, through every kernel that takes a K = 1 request"""
    pr = _tanh_sweep_problem()
    ref = pr.exact_reference()
    ran = set()
    for prec in (1, 0):
        g = pr.args(prec)
        choice = H.gemm_plan(g, "auto")
        for k in ["auto"] + [n for n in _stream_kernels(g) if n != choice]:
            pr.run(k, prec)
            worst = pr.check_exact(ref, ("tanh sweep", k, prec))
            print(f"gemm_tanh through {choice if k == 'auto' else k} (precision {prec}): max |err| {worst:.3e}")
            ran.add(choice if k == "auto" else k)
    assert len(ran) >= 3, ran
    _RAN["tanh sweep"] = ran


@pytest.mark.gpu
def test_every_gemm_kernel_ran_in_the_exact_group():
    for d in HEADLINE:
        if _key(d) not in _RAN:          # (a selected subset of the group ran before this test)
            _exact_request(d)
            torch.cuda.empty_cache()
    ran = set().union(*_RAN.values())
    assert ran == set(H.GEMM_KERNELS) - {"auto"}, sorted(set(H.GEMM_KERNELS) - {"auto"} - ran)


@pytest.mark.gpu
def test_headline_table_is_the_step_s_requests():
    """drift guard: HEADLINE is exactly the set of requests one step of the default model makes at batch 768"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import sweep_gemm_shapes as sw
    old = H.GEMM_PRECISION
    H.GEMM_PRECISION = "bf16x3"
    try:
        m = sw.build(300, 320, 4)
        reqs = sw.requests_of_a_step(m, 4, 768)
    finally:
        H.GEMM_PRECISION = old
    del m
    torch.cuda.empty_cache()
    logged = {_key(d) for d, _count in reqs}
    table = {_key(d) for d in HEADLINE}
    assert len(table) == len(HEADLINE)
    assert logged - table == set(), sorted(logged - table)
    assert table - logged == set(), sorted(table - logged)


# ======================================================================================== 2. arithmetic group
def _arith_nt():
    seen, out = set(), []
    for d in HEADLINE:
        if d["a_kmajor"]:
            continue
        key = (d["N"], d["K"], d["bias"], d["act"])
        if key in seen:
            continue
        seen.add(key)
        N, K = d["N"], d["K"]
        out.append(_req(24576, N, K, d["lda"], d["ldb"], bias=d["bias"], act=d["act"], ldc=(N + 3) // 4 * 4,
                        has_aux=d["has_aux"], ldaux=(N + 3) // 4 * 4 if d["has_aux"] else 0))
    return out


R_ARITH = 24288        # 96 utterances of 253 frames: whole utterances (the time shift) and whole K tiles of 16 rows


def _arith_tn():
    seen, out = set(), []
    for d in HEADLINE:
        if not d["a_kmajor"]:
            continue
        key = (d["M"], d["N"], d["b_kshift"], d["b_ones_col"])
        if key in seen:
            continue
        seen.add(key)
        out.append(_req(d["M"], d["N"], R_ARITH, d["lda"], d["ldb"], a_kmajor=1, b_kmajor=1, b_kshift=d["b_kshift"],
                        kperiod=d["kperiod"], b_ones_col=d["b_ones_col"], ldc=d["ldc"]))
    return out


ARITH = _arith_nt() + _arith_tn()


def _with_library_splits(d):
    """weight gradients: the split count the library gives the request (tssep_gemm_wgrad_splits)"""
    if not d["a_kmajor"]:
        return d
    S = int(_lib.lib().tssep_gemm_wgrad_splits(ctypes.byref(_plan_args(d))))
    assert S >= 1, S
    return dict(d, splitk=S, c_split_stride=d["M"] * d["ldc"])


@pytest.mark.gpu
@pytest.mark.parametrize("d0", ARITH, ids=[_name(d) for d in ARITH])
def test_split_bf16_rounding_within_the_derived_bound(d0):
    d = _with_library_splits(d0)
    pr = Problem(d, exact=False, seed=7)
    M, N, K, S = d["M"], d["N"], d["K"], d["splitk"]
    exact = pr.products()
    mag = pr.products(absolute=True)
    L = -(-(-(-K // 16)) // S) * 16 + 32              # the longest split, rounded up to whole K tiles of up to 32
    lines = []
    for prec in (1, 0):
        g = pr.args(prec)
        choice = H.gemm_plan(g, "auto")
        if choice is None:
            assert prec == 0 and d["b_ones_col"], d
            continue
        n = (3 * L if prec else L) + S
        coef = (C_SPLIT if prec else 0.0) + LAMBDA * math.sqrt(n) * U + U
        for k in ["auto"] + [x for x in _stream_kernels(g) if x != choice]:
            pr.run(k, prec)
            worst = 0.0
            for m0 in range(0, M, ROWS):
                m1 = min(M, m0 + ROWS)
                got = pr.output_rows(m0, m1)
                assert bool(torch.isfinite(got).all()), (k, prec, m0)
                c, a = exact[m0:m1], mag[m0:m1]
                tol = coef * a
                if pr.bias is not None:
                    tol = tol + U * (a + pr.bias.double().abs())
                want = pr.epilogue(c, m0, m1)
                if d["act"] == 1:
                    want, tol = torch.tanh(want), tol + TANH_ERR
                elif d["act"] == 2:
                    y = pr.aux[m0:m1, :N].double()
                    tol = tol * (1 - y * y) + 3 * U * a
                r = float(((got - want).abs() / tol).max())
                worst = max(worst, r)
            lines.append(f"{_name(d)} {choice if k == 'auto' else k} precision {prec}: max err/tol {worst:.3f}")
            assert worst <= 1.0, lines[-1]
    print("\n".join(lines))


# ======================================================================================== 3. guard group
def _nt(M, N, K, ldb=None, ldc=None, **kw):
    k4 = (K + 3) // 4 * 4
    return _req(M, N, K, k4, ldb or k4, ldc=N if ldc is None else ldc, **kw)


def _tn(M, N, K, lda, ldb, ldc, **kw):
    return _req(M, N, K, lda, ldb, a_kmajor=1, b_kmajor=1, ldc=ldc, c_split_stride=M * ldc, **kw)


def _rows(T, sb, st):
    return dict(c_remap=1, c_T=T, c_K=1, c_sb=sb, c_st=st)


# kernel, where, request(x), the launcher's byte count at x (declines at >= 2^31), step of x, fallback past it,
# GPU-runnable under 16 GB
GUARDS = [
    ("big", "gemm_bf16x3_big.hip: GN ldb 4 + 4 K",
     lambda x: _nt(65536, 256, 512, ldb=x, accumulate=1), lambda x: 256 * x * 4 + 512 * 4, 4, "tall2", True),
    ("big_p", "gemm_bf16x3_bigp.hip: remapped tensor's last element",
     lambda x: _nt(65536, 256, 128, ldc=0, bias=True, **_rows(256, x, 256)),
     lambda x: 4 * (255 * x + 255 * 256 + 256), 4, "tall2", True),
    ("big_p", "gemm_bf16x3_bigp.hip: 130 ldaux 4",
     lambda x: _nt(65536, 256, 128, act=2, has_aux=True, ldaux=x), lambda x: 130 * x * 4, 4, "tall2", False),
    ("big_p", "gemm_bf16x3_bigp.hip: GN ldb 4 + 4 K",
     lambda x: _nt(65536, 256, 128, ldb=x), lambda x: 256 * x * 4 + 128 * 4, 4, "stream", True),
    ("big_p", "gemm_bf16x3_bigp.hip: (GM + 2) ldc 4",
     lambda x: _nt(1024, 256, 128, ldc=x), lambda x: 258 * x * 4, 4, "pipe", True),
    ("big_p320", "gemm_bf16x3_bigp320.hip: remapped tensor's last element",
     lambda x: _nt(49152, 320, 128, ldc=0, bias=True, **_rows(256, x, 320)),
     lambda x: 4 * (191 * x + 255 * 320 + 320), 4, "nt_w160", True),
    ("big_p320", "gemm_bf16x3_bigp320.hip: (GM + 2) ldc 4",
     lambda x: _nt(1024, 320, 128, ldc=x), lambda x: 194 * x * 4, 4, "pipe", True),
    ("big_p320", "gemm_bf16x3_bigp320.hip: (WTM + 2) ldaux 4",
     lambda x: _nt(49152, 320, 128, act=2, has_aux=True, ldaux=x), lambda x: 98 * x * 4, 4, "nt_w160", False),
    ("big_p320", "gemm_bf16x3_bigp320.hip: GN ldb 4 + 4 K",
     lambda x: _nt(49152, 320, 128, ldb=x), lambda x: 320 * x * 4 + 128 * 4, 4, "stream", True),
    ("nt_w160", "gemm_bf16x3_nt_w160.hip: UN ldb 4 + 4 K",
     lambda x: _nt(49152, 160, 128, ldb=x, act=2, has_aux=True, ldaux=160), lambda x: 160 * x * 4 + 128 * 4, 4,
     "tall2", True),
    ("stream", "gemm_bf16x3_stream.hip: 40 ldc 4",
     lambda x: _nt(32768, 128, 128, ldc=x), lambda x: 40 * x * 4, 4, "pipe", False),
    ("stream", "gemm_bf16x3_stream.hip: SN ldb 4 + 4 K",
     lambda x: _nt(32768, 128, 128, ldb=x), lambda x: 128 * x * 4 + 128 * 4, 4, "pipe", True),
    ("tn_big", "gemm_bf16x3_tn_big.hip: (per + 4) WBK ld 4",
     lambda k: _tn(2400, 514, k, 2400, 516, 516, b_ones_col=1), lambda k: (k // 16 + 4) * 16 * 2400 * 4, 16, "tn", True),
    ("tn_p320", "gemm_bf16x3_tn_p320.hip: (per + 4) QBK ld 4",
     lambda k: _tn(2052, 320, k, 2052, 320, 320), lambda k: (k // 16 + 4) * 16 * 2052 * 4, 16, "tn", True),
    ("tn_h160", "gemm_bf16x3_tn_h160.hip: (per + 4) HBK ld 4",
     lambda k: _tn(320, 601, k, 320, 604, 604), lambda k: (k // 16 + 4) * 16 * 604 * 4, 16, "tn", True),
    ("tn_w160", "gemm_bf16x3_tn_w160.hip: swapped operands, (per + 4) VBK ld 4",
     lambda k: _tn(320, 600, k, 320, 600, 600), lambda k: (k // 16 + 4) * 16 * 600 * 4, 16, "tn", True),
    ("tn_w160", "gemm_bf16x3_tn_w160.hip: (per + 4) VBK ld 4",
     lambda k: _tn(1200, 300, k, 2400, 600, 300, b_kshift=-1, kperiod=253), lambda k: (k // 16 + 4) * 16 * 2400 * 4,
     16, "tn_tall", True),
]


def _first_past(count, step):
    """smallest multiple of `step` at which the launcher's byte count reaches 2^31"""
    lo, hi = 1, 1
    while count(hi * step) < TWO_GB:
        hi *= 2
    while lo < hi:
        mid = (lo + hi) // 2
        if count(mid * step) >= TWO_GB:
            hi = mid
        else:
            lo = mid + 1
    return lo * step


def _plan_args(d):
    g = _lib.GemmArgs()
    for f, _ in _lib.GemmArgs._fields_:
        if f in d:
            setattr(g, f, d[f])
    g.A = g.B = g.C = 0x1000
    g.bias = 0x1000 if d["bias"] else None
    g.aux = 0x1000 if d["has_aux"] else None
    g.c_perm = 0x1000 if d["perm"] else None
    return g


def _sides(case):
    kernel, _where, make, count, step, _fb, _run = case
    x = _first_past(count, step)
    return make(x - step), make(x)


_GIDS = [f"{c[0]}: {c[1].split(': ')[1]}" for c in GUARDS]


@pytest.mark.parametrize("case", GUARDS, ids=_GIDS)
def test_2gb_guard_plans(case):
    """host query: below the guard the kernel takes the request, past it the kernel declines and the automatic choice is
    the named fallback"""
    kernel, _where, _make, _count, _step, fallback, _run = case
    below, past = _sides(case)
    assert H.gemm_plan(_plan_args(below), kernel) == kernel, below
    assert H.gemm_plan(_plan_args(past), kernel) is None, past
    assert H.gemm_plan(_plan_args(past), "auto") == fallback, (H.gemm_plan(_plan_args(past), "auto"), past)


def _gbytes(pr):
    return sum(t.numel() * t.element_size() for t in (pr.A, pr.B, pr.C, pr.aux) if t is not None) / 2 ** 30


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in GUARDS if c[6]], ids=[i for i, c in zip(_GIDS, GUARDS) if c[6]])
def test_2gb_guard_fallback_and_kernel_below_are_exact(case):
    kernel, _where, _make, _count, _step, fallback, _run = case
    below, past = _sides(case)
    for side, d in (("past", past), ("below", below)):
        d = dict(d, splitk=1)
        pr = Problem(d, exact=True, seed=3)
        assert _gbytes(pr) < 12, (side, _gbytes(pr))
        ref = pr.exact_reference()
        g = pr.args(1)
        if side == "past":
            assert H.gemm_plan(g, kernel) is None and H.gemm_plan(g, "auto") == fallback
            names = ["auto"] + [n for n in _stream_kernels(g) if n != fallback]
        else:
            assert H.gemm_plan(g, kernel) == kernel
            names = [kernel]
        for k in names:
            pr.run(k, 1)
            pr.check_exact(ref, (kernel, side, k))
        del pr, ref
        torch.cuda.empty_cache()
