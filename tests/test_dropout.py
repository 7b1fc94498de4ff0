"""CPU checks of dropout > 0 on the HIP path: the generator behind the masks (Philox4x32-10, csrc/dropout_philox.h)
against the Random123 known answers and an independent numpy restatement, the host-side mask function, construction of
the two hot-path classes with dropout, the per-rank seed derivation and the toy overlay.  No GPU: the two *_host entry
points of the library run on the host."""
import os

import numpy as np
import pytest
import torch

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
M32 = np.uint64(0xFFFFFFFF)


def H():
    from tssep_amd import hip_ops
    return hip_ops


def np_philox(ctr, key):
    """Philox4x32-10 on uint64 numpy arrays holding 32-bit words: ctr [n, 4], key [n, 2] -> [n, 4]."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k = [key[:, i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & M32, (k[1] + np.uint64(0xBB67AE85)) & M32]
    return np.stack(c, 1)


def np_keep(seed, draw, first, n, p):
    """The mask definition restated: element e -> word e % 4 of Philox(counter = (e / 4, draw), key = seed)."""
    e = np.arange(first, first + n, dtype=np.uint64)
    grp = e >> np.uint64(2)
    u = lambda v: np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)       # noqa: E731
    ctr = np.stack([grp & M32, grp >> np.uint64(32), np.full_like(grp, u(draw) & M32),
                    np.full_like(grp, u(draw) >> np.uint64(32))], 1)
    key = np.stack([np.full_like(grp, u(seed) & M32), np.full_like(grp, u(seed) >> np.uint64(32))], 1)
    words = np_philox(ctr, key)[np.arange(n), (e & np.uint64(3)).astype(np.int64)]
    return (words >= np.uint64(int(p * 2 ** 32))).astype(np.uint8)


KAT = [
    ([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    want = [int(w, 16) for w in want.split()]
    assert H().philox4x32_10_host(ctr, key) == want
    assert np_philox(np.array([ctr], dtype=np.uint64), np.array([key], dtype=np.uint64))[0].tolist() == want


def test_philox_against_numpy_restatement():
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    key = rng.integers(0, 2 ** 32, size=(300, 2), dtype=np.uint64)
    want = np_philox(ctr, key)
    for c, k, w in zip(ctr.tolist(), key.tolist(), want.tolist()):
        assert H().philox4x32_10_host(c, k) == w


@pytest.mark.parametrize("seed,draw,first,n,p", [
    (1234, 0, 0, 4096, 0.3), (1234, 7, 3, 1001, 0.3), (-5, 2 ** 40 + 3, 2 ** 33 + 5, 2050, 0.5),
    (2 ** 63 - 1, 1, 2 ** 33 + 5, 777, 0.1), (0, 0, 1, 1, 0.25)])
def test_keep_host_against_numpy_restatement(seed, draw, first, n, p):
    got = H().dropout_keep_host(seed, draw, first, n, p)
    assert got.dtype == np.uint8 and got.shape == (n,)
    assert np.array_equal(got, np_keep(seed, draw, first, n, p))


def test_keep_host_properties():
    h = H()
    full = h.dropout_keep_host(9, 4, 0, 5000, 0.3)
    for n in (1, 2, 3, 4, 5, 1237):                         # prefix property: element i does not depend on n
        assert np.array_equal(h.dropout_keep_host(9, 4, 0, n, 0.3), full[:n])
    for first in (1, 2, 3, 6, 4093):                        # ... nor on where the window starts
        assert np.array_equal(h.dropout_keep_host(9, 4, first, 300, 0.3), full[first:first + 300])
    assert h.dropout_keep_host(9, 4, 5, 3000, 0.0).all()
    assert not h.dropout_keep_host(9, 4, 5, 3000, 1.0).any()
    assert not np.array_equal(h.dropout_keep_host(9, 5, 0, 5000, 0.3), full)        # another draw
    assert not np.array_equal(h.dropout_keep_host(10, 4, 0, 5000, 0.3), full)       # another seed
    assert h.dropout_keep_host(9, 4, 0, 0, 0.3).shape == (0,)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="invalid shape"):
            h.dropout_keep_host(9, 4, 0, 8, bad)
    with pytest.raises(RuntimeError, match="invalid shape"):
        h.dropout_keep_host(9, 4, -1, 8, 0.3)


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_rate(p):
    """Within five binomial standard deviations of 1 - p over n = 1 024 000 elements (1.5e-3, 2.1e-3, 2.5e-3): a bound
    derived from the distribution, not from what the generator gives."""
    n = 1_024_000
    rate = H().dropout_keep_host(20240, 3, 0, n, p).mean()
    print(f"p={p}: keep rate {rate:.6f}, |rate - (1 - p)| = {abs(rate - (1 - p)):.2e}")
    assert abs(rate - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)


# ---------------------------------------------------------------------------------------------------- construction
ME_KW = dict(idim=12, odim=9, layers=3, units=5, projs=6)


def _names(m):
    return [n for n, _ in m.named_modules()]


def test_rnnp_packed_constructs_with_dropout():
    from tssep_amd.train.rnnp import RNNP_packed
    a, b = RNNP_packed(7, 3, 5, 6, 0.3), RNNP_packed(7, 3, 5, 6, 0)
    assert list(a.state_dict()) == list(b.state_dict()) and _names(a) == _names(b)
    assert isinstance(a.net[2], torch.nn.Dropout) and a.net[2].p == 0.3 and a.net[6].p == 0.3 and a.dropout == 0.3
    assert a.site_p(a.net[2]) == 0.3 and b.site_p(b.net[2]) == 0.0 and a.site_p(None) == 0.0
    a.eval()
    assert a.site_p(a.net[2]) == 0.0
    a.train()
    a.net[2].eval()                                         # per-module switch
    assert a.site_p(a.net[2]) == 0.0 and a.site_p(a.net[6]) == 0.3
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            RNNP_packed(7, 3, 5, 6, bad)
        with pytest.raises(ValueError):
            RNNP_packed(7, 1, 5, 6, bad)                    # (a single layer builds no Dropout member)
    with pytest.raises(NotImplementedError):
        RNNP_packed(7, 3, 5, 6, 0.3, typ="bgru")


@pytest.mark.parametrize("combination,ts_vad", [("mul", 4), ("cat", False)])
def test_mask_estimator_constructs_with_dropout(combination, ts_vad):
    from tssep_amd.train.net import MaskEstimator_v2
    a = MaskEstimator_v2(dropout=0.3, combination=combination, ts_vad=ts_vad, aux_net_output_size=7, **ME_KW)
    b = MaskEstimator_v2(dropout=0, combination=combination, ts_vad=ts_vad, aux_net_output_size=7, **ME_KW)
    assert list(a.state_dict()) == list(b.state_dict()) and _names(a) == _names(b)
    assert [d.p for d in a._dropouts] == [0.3, 0.3] and len(a._dropouts) == len(a._birnns) - 1
    keys = list(a.post_net._modules)
    for site, birnn_key in zip(a._dropout_keys, a._birnn_keys):         # `dropout<l>` sits right behind `birnn<l>`
        assert keys.index(site) == keys.index(birnn_key) + 1
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            MaskEstimator_v2(dropout=bad, combination=combination, ts_vad=ts_vad, aux_net_output_size=7, **ME_KW)


def test_rank_seed_derivation():
    from tssep_amd.train.trainer import rank_dropout_seed
    for seed in (0, 1, 1234, 2 ** 63 - 1, 0x0123456789ABCDEF):
        seeds = [rank_dropout_seed(seed, r) for r in range(8)]
        assert len(set(seeds)) == 8 and seeds[0] == seed
        assert seeds == [rank_dropout_seed(seed, r) for r in range(8)]
        assert all(0 <= s < 2 ** 63 for s in seeds)
    assert rank_dropout_seed(1, 1) != rank_dropout_seed(2, 1)


def test_toy_dropout_overlay_resolves():
    from tssep_amd import configurable
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_dropout.yaml")]
                           + ["eg.trainer.storage_dir=/tmp/unused"])
    assert cfg["eg"]["trainer"]["model"]["mask_estimator"]["dropout"] == 0.1
    assert Experiment.get_config(cfg["eg"])["trainer"]["model"]["mask_estimator"]["dropout"] == 0.1
    from tssep_amd.train.net import MaskEstimator_v2
    assert configurable.resolve(cfg["eg"]["trainer"]["model"]["mask_estimator"]["factory"]) is MaskEstimator_v2
    me = Experiment.from_config(cfg["eg"]).trainer.model.mask_estimator
    assert [d.p for d in me._dropouts] == [0.1] * (me.layers - 1)
    plain = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml")]
                             + ["eg.trainer.storage_dir=/tmp/unused"])
    ref = Experiment.from_config(plain["eg"]).trainer.model
    assert list(Experiment.from_config(cfg["eg"]).trainer.model.state_dict()) == list(ref.state_dict())
