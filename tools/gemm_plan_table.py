"""The GEMM dispatcher's decisions over a fixed corpus of requests, recorded and checked bit for bit (host only, no GPU).

   python tools/gemm_plan_table.py --record tests/golden/gemm_plan.json      (with the library whose behaviour is the reference)
   python tools/gemm_plan_table.py --check tests/golden/gemm_plan.json       (with the library under test)

Which kernel takes a request, and the split count of a weight gradient, are pure functions of the request
(csrc/gemm_rules.h, the candidate table in csrc/gemm_bf16x3.hip), so a change that is meant to preserve behaviour can be
held to a table recorded BEFORE it: build the parent commit elsewhere, name its library in TSSEP_HIP_LIB (as for
tools/step_fingerprint.py) and --record; tests/test_gemm_plan_table.py runs --check against this tree's library.
A change that alters a rule on purpose records again and says so.

Per request the table holds: the kernel tssep_gemm_plan names under `auto` (or the return code), the set of kernel ids
that accept the request when forced, and for weight-gradient requests tssep_gemm_wgrad_splits and
tssep_gemm_wgrad_split_rule of every weight-gradient kernel.  The corpus is built from the constants below; the file
keeps the distinct records once and two characters per request that name its record.

--partial skips the check that every kernel is some request's automatic choice (recordings against the experiment
library with one TSSEP_GEMM_* switch off)."""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.append(ROOT)

R = 253                                                # frames of an utterance (the remapped stores, the time shift)
NT_M = (100, 1024, 2024, 8096, 48576, 194304, 194312, 777216)
NT_N = (50, 160, 256, 257, 300, 320, 513, 600, 780, 1000, 1200, 1280, 2052, 2400, 4104, 5120)
NT_K = (30, 64, 256, 320, 447, 448, 512, 600, 1024, 1280, 1535, 1536, 2400)
NT_STORE = ("plain", "bias_tanh", "tanh_bwd", "remap_wide", "remap_narrow", "accumulate", "tanh_bwd_remap")
NT_PRECISION = (1, 3)
NT_F32_EVERY = 7                                       # every 7th request again in precision 0

WG_K = tuple(b * R for b in (8, 32, 320, 768, 3072))   # the grid of test_wgrad_split_count_and_kernel_are_a_fixed_point_...
WG_M = (320, 513, 640, 1200, 1280, 2052, 2400, 4104)
WG_N = ((300, 0), (301, 1), (321, 1), (320, 0), (514, 1), (554, 1), (557, 1), (601, 1), (600, 0), (1281, 1), (2561, 1),
        (874, 1), (130, 0))                            # (N, ones column)
WG_KSHIFT = (0, -1, -16, -17, -33)                     # 0: not time-shifted
WG_PRECISION = (1, 2)
WG_SPLITK = (1, 3, 8, 24, 56)

CHOICE = "0123456789abcdefg"                           # kernel ids 0 .. 16
RC = {-1: "v", -2: "w", -3: "x", -4: "y", -5: "z"}     # no kernel: the return code
ALPHABET = "".join(chr(c) for c in range(35, 127) if chr(c) != "\\")      # 91 symbols, two per request


def round_up(x, m):
    return (x + m - 1) // m * m


def requests(GemmArgs):
    """-> (is_wgrad, GemmArgs) of the whole corpus, in a fixed order"""
    n = 0
    for M, N, K, store, prec in itertools.product(NT_M, NT_N, NT_K, NT_STORE, NT_PRECISION):
        g = GemmArgs()
        g.A = g.B = 0x1000
        g.C = 0x2000
        g.M, g.N, g.K = M, N, K
        g.lda = g.ldb = round_up(K, 4)
        g.ldc = round_up(N, 4)
        g.precision = prec
        if store == "bias_tanh":
            g.bias, g.act = 0x3000, 1
        if store in ("tanh_bwd", "tanh_bwd_remap"):
            g.aux, g.ldaux, g.act = 0x4000, round_up(N, 4), 2
        if store in ("remap_wide", "remap_narrow", "tanh_bwd_remap"):
            g.c_remap = 2 if store == "remap_narrow" else 1
            g.c_T, g.c_K, g.c_sb, g.c_sk, g.c_st, g.ldc = R, 4, R * 4 * N, N, 4 * N, 0
        if store == "accumulate":
            g.accumulate = 1
        yield False, g
        n += 1
        if n % NT_F32_EVERY == 0:
            g = GemmArgs.from_buffer_copy(g)
            g.precision = 0
            yield False, g
    for K, M, (N, ones), ks, prec, S in itertools.product(WG_K, WG_M, WG_N, WG_KSHIFT, WG_PRECISION, WG_SPLITK):
        if ks and ones:
            continue
        g = GemmArgs()
        g.A = g.B = 0x1000
        g.C = 0x2000
        g.M, g.N, g.K = M, N, K
        g.lda, g.ldb, g.ldc = round_up(M, 4), round_up(N, 4), round_up(N, 4)
        g.a_kmajor = g.b_kmajor = 1
        g.splitk, g.c_split_stride, g.b_ones_col, g.precision = S, M * g.ldc, ones, prec
        if ks:
            g.b_kshift, g.kperiod = ks, R
        yield True, g


def describe(g):
    return {f: getattr(g, f) for f, _ in type(g)._fields_ if getattr(g, f)}


def records():
    """-> [(record string, request description)] with the library _lib names (TSSEP_HIP_LIB or this tree's)"""
    from tssep_amd import _lib
    L = _lib.lib()
    names = []
    while L.tssep_gemm_kernel_name(len(names)) != b"?":
        names.append(L.tssep_gemm_kernel_name(len(names)).decode())
    assert len(names) == len(CHOICE), names
    wgrad_ids = [i for i, n in enumerate(names) if n.startswith("tn")]
    plan, splits, rule = L.tssep_gemm_plan, L.tssep_gemm_wgrad_splits, L.tssep_gemm_wgrad_split_rule
    kid = ctypes.c_int32(0)
    out = []
    for wgrad, g in requests(_lib.GemmArgs):
        p = ctypes.byref(g)
        rc = plan(p, 0, ctypes.byref(kid))
        rec = CHOICE[kid.value] if rc == 0 else RC[rc]
        mask = 0
        for k in range(1, len(names)):
            if plan(p, k, ctypes.byref(kid)) == 0:
                assert kid.value == k, (k, kid.value, describe(g))
                mask |= 1 << k
        rec += "%x" % mask
        if wgrad:
            rec += ":%d:" % splits(p) + ",".join(str(rule(p, k)) for k in wgrad_ids)
        out.append((rec, g))
    return out, names


def encode(recs):
    distinct = sorted({r for r, _ in recs})
    assert len(distinct) <= len(ALPHABET) ** 2, len(distinct)
    at = {r: i for i, r in enumerate(distinct)}
    return distinct, "".join(ALPHABET[at[r] // len(ALPHABET)] + ALPHABET[at[r] % len(ALPHABET)] for r, _ in recs)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--record", metavar="PATH")
    mode.add_argument("--check", metavar="PATH")
    ap.add_argument("--partial", action="store_true")
    args = ap.parse_args(argv)
    recs, names = records()
    n_wgrad = sum(1 for r, _ in recs if ":" in r)
    if args.record:
        assert len(recs) - n_wgrad >= 10000 and n_wgrad >= 2000, (len(recs), n_wgrad)
        chosen = {r[0] for r, _ in recs}
        unreached = [names[i] for i in range(1, len(names)) if CHOICE[i] not in chosen]
        assert args.partial or not unreached, f"never the automatic choice: {unreached}"
        distinct, index = encode(recs)
        with open(args.record, "w") as f:
            json.dump({"kernels": names, "requests": len(recs), "weight_gradients": n_wgrad, "records": distinct,
                       "index": index}, f, separators=(",", ":"))
            f.write("\n")
        print(f"recorded {len(recs)} requests ({n_wgrad} weight gradients), {len(distinct)} distinct records, "
              f"{os.path.getsize(args.record)} bytes; unreached: {unreached}")
        return 0
    with open(args.check) as f:
        want = json.load(f)
    A = len(ALPHABET)
    expected = [want["records"][ALPHABET.index(a) * A + ALPHABET.index(b)]
                for a, b in zip(want["index"][0::2], want["index"][1::2])]
    assert want["kernels"] == names, (want["kernels"], names)
    assert len(expected) == want["requests"] == len(recs), (len(expected), want["requests"], len(recs))
    bad = [(i, e, r, g) for i, (e, (r, g)) in enumerate(zip(expected, recs)) if e != r]
    for i, e, r, g in bad[:20]:
        print(f"request {i}: recorded {e}, now {r}: {describe(g)}")
    print(f"{len(recs)} requests ({n_wgrad} weight gradients): {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
