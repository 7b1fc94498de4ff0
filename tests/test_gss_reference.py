"""The guided cACGMM of DESIGN 4.24 without a GPU: the float64 reference of tests/gss_reference.py recovers the planted
sources, has the properties the definition promises, is moved by every planted defect by more than the GPU tests
allow; and what the Python layers refuse on the arguments alone."""
import re
import subprocess

import numpy as np
import pytest
import torch

import gss_reference as R
from tssep_amd import _lib, hip_ops as H
from tssep_amd.train import enhancer

EPS = 2.0 ** -52
MAIN = (6, 2, 200, 5, "plain")


@pytest.fixture(scope="module")
def fits():
    """seed -> (Y, act, on, gamma after 20 iterations): the scenes of the issue, fitted once"""
    out = {}
    refs = R.yardstick(MAIN, 20)[1]
    for seed in R.SEEDS:
        Y, act, on = R.case_scene(MAIN, seed)
        out[seed] = (Y, act, on, refs[seed])
    return out


# ------------------------------------------------------------------------------------------------ recovery
@pytest.mark.parametrize("seed", R.SEEDS)
def test_reference_recovers_the_sources(fits, seed):
    """argmax_c gamma names the one present speaker (or noise) on >= 0.95 of the tf points with at most one speaker
    present.  Measured here: 0.986, 0.992, 0.995, 0.982 (seeds 0-3); on the overlap frames 80-120 alone 0.993, 0.986,
    0.987, 0.966.  The 0.95 is a condition on the definition, not a tolerance."""
    _, _, on, g = fits[seed]
    whole, overlap = R.recovery(g, on), R.recovery(g[:, 80:120], on[:, 80:120])
    print(f"seed {seed}: recovery {whole:.4f}, overlap frames {overlap:.4f}")
    assert whole >= 0.95
    assert overlap >= 0.95


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("seed", R.SEEDS)
def test_posteriors_sum_to_one_and_respect_the_prior(fits, seed):
    _, act, _, g = fits[seed]
    assert np.abs(g.sum(0) - 1).max() <= 4 * EPS
    assert (g[:-1][act == 0] == 0).all()
    assert (g >= 0).all()


def test_bad_frames_get_zero_and_take_part_in_nothing():
    Y, act, _ = R.case_scene(MAIN, 0)
    Y = Y.copy()
    Y[:, 10] = 0
    Y[2, 50, :] = np.nan
    Y[1, 130, 3] = np.inf
    g = R.guided_cacgmm_reference(Y, act, 5)
    assert (g[:, 10] == 0).all() and (g[:, 50] == 0).all() and (g[:, 130, 3] == 0).all()
    assert np.isfinite(g).all()
    keep = np.setdiff1d(np.arange(Y.shape[1]), [10, 50])
    # the bins without the inf frame: the same bits as a fit that never saw the bad frames
    g2 = R.guided_cacgmm_reference(Y[:, keep], act[:, keep], 5)
    bins = [0, 1, 2, 4]
    assert np.array_equal(g[:, keep][:, :, bins], g2[:, :, bins])


@pytest.mark.parametrize("seed", R.SEEDS)
def test_invariant_to_scale_and_channel_order(seed):
    """A positive rescaling of every frame and a permutation of the channels change gamma by no more than the allowance
    of the GPU tests (MARGIN x the reference's own spread over its summation orders, + 4 * 2^-52): both change
    roundings only."""
    Y, act, _ = R.case_scene(MAIN, seed)
    rng = np.random.default_rng(100 + seed)
    for it in (1, 20):
        g = R.yardstick(MAIN, it)[1][seed]
        scaled = R.guided_cacgmm_reference(Y * rng.uniform(0.1, 10.0, size=(1,) + Y.shape[1:]), act, it)
        permuted = R.guided_cacgmm_reference(Y[rng.permutation(Y.shape[0])], act, it)
        allow = R.allowance(MAIN, it)
        print(it, np.abs(scaled - g).max(), np.abs(permuted - g).max(), allow)
        assert np.abs(scaled - g).max() <= allow
        assert np.abs(permuted - g).max() <= allow


def test_solve_variants_are_the_same_function():
    """L^-1 yh as a product with the explicit inverse, and the Cholesky pivots carried in extended precision, are other
    correct evaluations of the definition: at a well-conditioned shape they stay inside the order allowance; at the
    rank-deficient one they (with the channel reversal and the rescaling) make the yardstick the order cannot give."""
    Y, act, _ = R.case_scene(MAIN, 0)
    for it in (1, 20):
        g = R.yardstick(MAIN, it)[1][0]
        for solve in ("inverse", "extended_pivot"):
            assert np.abs(R.guided_cacgmm_reference(Y, act, it, solve=solve) - g).max() <= R.allowance(MAIN, it)
    assert R.yardstick(R.RANK_DEFICIENT_CASE, 1)[0] == 0
    y1, y20 = R.rounding_yardstick(R.RANK_DEFICIENT_CASE, 1)[0], R.rounding_yardstick(R.RANK_DEFICIENT_CASE, 20)[0]
    print(y1, y20)
    assert 0 < y1 <= 1e-11 and y20 <= 1e-11


def test_one_channel_leaves_the_mixture_weights():
    """D = 1: yh is a phase, B_c = 1 + load and q = 1 / (1 + load) for every class, so log p_tc - log pi_c does not
    depend on c and gamma_tc = a_tc pi_c / sum_c' a_c't pi_c'.  In floating point the identity passes through log and
    exp: |log pi| <= 8 here, its rounding and exp's are a few 2^-53 relative each -> 32 * 2^-52."""
    Y, act, _ = R.case_scene((1, 2, 200, 5, "plain"), 0)
    g1 = R.guided_cacgmm_reference(Y, act, 1)
    a = np.concatenate([act, np.ones((1, act.shape[1]), dtype=act.dtype)])[:, :, None].astype(float)
    start = a / a.sum(0)
    n = start.sum(1)                                                    # [C, F]
    pi = n / n.sum(0)
    want = a * pi[:, None] / (a * pi[:, None]).sum(0)
    assert np.abs(g1 - want).max() <= 32 * EPS


def test_blocks():
    Y, act, _ = R.case_scene(MAIN, 1)
    T = Y.shape[1]
    whole = R.guided_cacgmm_reference(Y, act, 3)
    assert np.array_equal(whole, R.guided_cacgmm_reference(Y, act, 3, blocks=[(0, T, 0, T)]))
    table = H.gss_uniform_blocks(T, 70, 20)
    assert table.tolist() == [[0, 90, 0, 70], [50, 160, 70, 140], [120, 200, 140, 200]]
    g = R.guided_cacgmm_reference(Y, act, 3, blocks=table)
    for sf, ef, so, eo in table.tolist():
        part = R.guided_cacgmm_reference(Y[:, sf:ef], act[:, sf:ef], 3)
        assert np.array_equal(g[:, so:eo], part[:, so - sf:eo - sf])
    assert not np.array_equal(g, whole)


# ------------------------------------------------------------------------------------------------ planted defects
ONE = (6, 2, 63, 5, "plain")
# a defect that cannot show after one iteration: there is no earlier n, and q is 1 in the first B_c
LATE = ("stale_pi", "no_q_weight")


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_exceeds_the_gpu_allowance(defect):
    """Each mistake moves gamma by more than the allowance of tests/test_gpu_gss.py at that file's shapes, one iteration
    (where the mistake can act in the first iteration) and twenty.  Measured here, seed 0: one iteration no_D 0.60,
    plus_ld 0.63, prior_start_only 0.77, q_one 0.78 against 5.2e-14; twenty iterations no_D 1.0, plus_ld 1.0,
    prior_start_only 0.95, stale_pi 7.1e-3, no_q_weight 1.0, q_one 0.99 against 6.5e-12."""
    assert ONE in R.ONE_ITERATION_CASES and MAIN in R.TWENTY_ITERATION_CASES
    for case, it in ((ONE, 1), (MAIN, 20)):
        Y, act, _ = R.case_scene(case, 0)
        moved = np.abs(R.guided_cacgmm_reference(Y, act, it, _defect=defect) - R.yardstick(case, it)[1][0]).max()
        print(defect, it, moved, R.allowance(case, it))
        if it == 1 and defect in LATE:
            assert moved == 0
        else:
            assert moved > 100 * R.allowance(case, it)


def test_yardsticks_are_of_the_size_the_formats_give():
    """The allowance rests on the reference's own spread: it must be rounding-sized, or the GPU test allows anything.
    One iteration: a few hundred 2^-52 at most; twenty: EM amplifies, below 1e-11."""
    for case in R.ONE_ITERATION_CASES:
        assert R.yardstick(case, 1)[0] <= 1024 * EPS, case
    for case in R.TWENTY_ITERATION_CASES:
        assert R.yardstick(case, 20)[0] <= 1e-11, case


# ------------------------------------------------------------------------------------------------ host side
def _args(D=6, K=2, T=20, F=3):
    return torch.zeros(D, T, F, dtype=torch.complex128), torch.ones(K, T, dtype=torch.uint8)


def test_check_accepts_and_returns_the_shape():
    obs, act = _args()
    D, K, T, F, tab = H.guided_cacgmm_check(obs, act)
    assert (D, K, T, F) == (6, 2, 20, 3) and tab.tolist() == [[0, 20, 0, 20]] and tab.dtype == np.int32
    for D in (1, 8):
        for K in (1, 8):
            H.guided_cacgmm_check(*_args(D, K))
    H.guided_cacgmm_check(obs, act.bool(), 1, 1e-3, "uniform", [(0, 12, 0, 10), (8, 20, 10, 20)], torch.float64)


@pytest.mark.parametrize("kw, exc", [
    (dict(D=9), ValueError), (dict(D=0), ValueError), (dict(K=9), ValueError), (dict(K=0), ValueError),
    (dict(load=0.0), ValueError), (dict(load=-1e-6), ValueError), (dict(load=float("inf")), ValueError),
    (dict(load=float("nan")), ValueError), (dict(iterations=0), ValueError), (dict(iterations=1.5), ValueError),
    (dict(weights="frame"), ValueError), (dict(out_dtype=torch.float16), TypeError), (dict(T=0), ValueError),
    (dict(F=0), ValueError),
])
def test_check_refuses(kw, exc):
    shape = {k: kw.pop(k) for k in ("D", "K", "T", "F") if k in kw}
    obs, act = _args(**shape)
    with pytest.raises(exc):
        H.guided_cacgmm_check(obs, act, **kw)


def test_check_refuses_types_and_mismatches():
    obs, act = _args()
    with pytest.raises(TypeError):
        H.guided_cacgmm_check(obs.to(torch.complex64), act)
    with pytest.raises(ValueError):
        H.guided_cacgmm_check(obs[0], act)
    with pytest.raises(ValueError):
        H.guided_cacgmm_check(obs, act[:, :-1])
    with pytest.raises(ValueError):
        H.guided_cacgmm_check(obs, act[0])
    with pytest.raises(ValueError):
        H.guided_cacgmm_check(obs, act * 2)                       # soft or other values: 0 / 1 only
    with pytest.raises(ValueError):
        H.guided_cacgmm_check(obs, act.float() * 0.5)
    with pytest.raises(ValueError):
        H.guided_cacgmm_check(obs.numpy(), act)
    with pytest.raises(NotImplementedError):
        H.guided_cacgmm_check(torch.view_as_complex(torch.zeros(6, 20, 3, 2, dtype=torch.float64, requires_grad=True)),
                              act)


@pytest.mark.parametrize("blocks", [
    [(0, 20, 0, 10)],                                   # does not reach T
    [(0, 20, 0, 10), (0, 20, 11, 20)],                  # a gap
    [(0, 20, 0, 12), (0, 20, 10, 20)],                  # an overlap
    [(0, 20, 10, 20), (0, 20, 0, 10)],                  # out of order
    [(5, 20, 0, 20)],                                   # s_out in front of s_fit
    [(0, 15, 0, 20)],                                   # e_out behind e_fit
    [(0, 21, 0, 20)],                                   # e_fit behind T
    [(-1, 20, 0, 20)],
    [(0, 20, 0, 0), (0, 20, 0, 20)],                    # an empty out range
    [(0, 20, 0)],
    [],
    [(0, 20, 0, 10.5), (0, 20, 10.5, 20)],
])
def test_block_table_refused(blocks):
    with pytest.raises(ValueError):
        H.gss_blocks_check(blocks, 20)
    obs, act = _args()
    with pytest.raises(ValueError):
        H.guided_cacgmm_check(obs, act, blocks=blocks)


def test_uniform_block_table():
    assert H.gss_uniform_blocks(300, 100, 30).tolist() == [[0, 130, 0, 100], [70, 230, 100, 200], [170, 300, 200, 300]]
    assert H.gss_uniform_blocks(250, 100, 0).tolist() == [[0, 100, 0, 100], [100, 200, 100, 200], [200, 250, 200, 250]]
    assert H.gss_uniform_blocks(7, None).tolist() == [[0, 7, 0, 7]]
    assert H.gss_uniform_blocks(7, 100, 1000).tolist() == [[0, 7, 0, 7]]
    for T, block, context in ((300, 100, 30), (1875, 1875, 940), (7500, 1875, 940), (5, 1, 0)):
        tab = H.gss_uniform_blocks(T, block, context)
        assert np.array_equal(H.gss_blocks_check(tab, T), tab)
    for bad in (dict(block=0), dict(block=-5), dict(block=2.5), dict(block=10, context=-1), dict(block=None, context=3)):
        with pytest.raises(ValueError):
            H.gss_uniform_blocks(20, **bad)


def test_gss_is_configurable_and_round_trips():
    cfg = enhancer.GSS.get_config()
    assert cfg["factory"] == "tssep.train.enhancer.GSS"
    assert (cfg["iterations"], cfg["load"], cfg["weights"], cfg["block"], cfg["context"], cfg["pre_wpe"]) == \
        (20, 1e-6, "bin", None, 0, None)
    assert cfg["bf"]["factory"] == "tssep.train.enhancer.ClassicBF_np"
    assert cfg["bf"]["distortion_mask"]["factory"] == "tssep.train.enhancer_distortion_mask.SumCrossTalker"
    g = enhancer.GSS.from_config(cfg)
    assert isinstance(g, enhancer.GSS) and isinstance(g.bf, enhancer.ClassicBF_np)
    assert isinstance(g.bf.distortion_mask, enhancer.enhancer_distortion_mask.SumCrossTalker)
    cfg2 = enhancer.GSS.get_config(dict(iterations=5, weights="uniform", block=1875, context=940,
                                        pre_wpe={"factory": "tssep.train.enhancer.WPE", "taps": 2}))
    g2 = enhancer.GSS.from_config(cfg2)
    assert (g2.iterations, g2.weights, g2.block, g2.context) == (5, "uniform", 1875, 940)
    assert isinstance(g2.pre_wpe, enhancer.WPE) and g2.pre_wpe.taps == 2
    assert enhancer.GSS.get_config(cfg2) == cfg2
    plain = enhancer.GSS()
    assert isinstance(plain.bf.distortion_mask, enhancer.enhancer_distortion_mask.SumCrossTalker)


def test_gss_refuses_on_the_host():
    Y = torch.zeros(6, 20, 3, dtype=torch.complex128)
    dia = [[(0, 10)], [(5, 20)]]
    with pytest.raises(TypeError):
        enhancer.GSS()(Y.to(torch.complex64), dia)
    with pytest.raises(AssertionError):
        enhancer.GSS()(Y[:5], dia)                                       # the chain keeps ClassicBF_np's D >= 6
    with pytest.raises(NotImplementedError):
        enhancer.GSS(bf=enhancer.TorchBF())(Y, dia)
    with pytest.raises(NotImplementedError):
        enhancer.GSS(pre_wpe=enhancer.OnlineWPE())(Y, dia)
    with pytest.raises(ValueError):
        enhancer.GSS(pre_wpe=enhancer.WPE(), bf=enhancer.ClassicBF_np(
            distortion_mask=enhancer.enhancer_distortion_mask.SumCrossTalker(), pre_wpe=enhancer.WPE()))(Y, dia)
    with pytest.raises(ValueError):                                      # masks and filter on different observations
        enhancer.GSS(bf=enhancer.ClassicBF_np(
            distortion_mask=enhancer.enhancer_distortion_mask.SumCrossTalker(), pre_wpe=enhancer.WPE()))(Y, dia)
    # an int32 [*, 3] tensor is a segment table; with T = 3 frames it could be an activity as well: refused, with K or not
    amb = torch.ones(2, 3, dtype=torch.int32)
    for K in (None, 2):
        with pytest.raises(ValueError):
            enhancer.GSS().masks(Y[:, :3], amb, K=K)
    with pytest.raises(ValueError):
        enhancer.GSS().masks(Y, torch.zeros(4, 3, dtype=torch.int32))    # a table comes with K


def test_entry_points_declared_exported_and_wrapped():
    protos = _lib.parse_header()
    names = ("tssep_gss_workspace_bytes", "tssep_gss_fit", "tssep_segments_to_activity")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r" T (tssep_\w+)", out))
    for n in names:
        assert n in protos and n in exported, n
    assert len(protos["tssep_gss_fit"][1]) == 16 and len(protos["tssep_segments_to_activity"][1]) == 6
    for n in ("guided_cacgmm", "guided_cacgmm_check", "segments_to_activity", "gss_blocks_check", "gss_uniform_blocks"):
        assert callable(getattr(H, n)), n
    assert _lib.lib().tssep_abi_version() == 4


def test_workspace_bytes_is_host_only():
    """no GPU here: the size comes back from host arithmetic alone, 0 for what the kernels refuse"""
    L = _lib.lib()
    D, K, T, F = 6, 2, 300, 5
    C, nent, nch = K + 1, D * (D + 1) // 2 + 1, 2
    want = 16 * D * T * F + 8 * F * C * (2 * D * D + 2) + 16 * F * nch * C * nent
    got = L.tssep_gss_workspace_bytes(1, D, K, T, F, T)
    assert want <= got <= want + 16
    assert L.tssep_gss_workspace_bytes(3, D, K, T, F, 160) > 0
    assert L.tssep_gss_workspace_bytes(1, 8, 8, 7500, 513, 7500) > 0
    for bad in ((1, 9, K, T, F, T), (1, 0, K, T, F, T), (1, D, 9, T, F, T), (1, D, 0, T, F, T), (0, D, K, T, F, T),
                (1, D, K, 0, F, T), (1, D, K, T, 0, T), (1, D, K, T, F, 0), (65536, D, K, T, F, T)):
        assert L.tssep_gss_workspace_bytes(*bad) == 0, bad
