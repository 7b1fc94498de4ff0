"""Learned speaker embeddings, CPU side: the float64 reference checks itself (tests/aux_reference.py), and the drop-in
classes -- Linear, AuxNet, InstanceNorm, InstanceNorm_v2 inside MaskEstimator_v2 -- construct, print, name their
parameters and round-trip their configs like the reference (tssep/train/net.py:19-158, 250-330, 501-600).  No GPU."""
import os

import numpy as np
import pytest
import torch

import aux_reference as R

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")


def _params(idim, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, dtype=dtype) * 0.5 for s in ((idim, idim), (idim,)) * 3]


def _seqs(lens, idim, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, idim, generator=g, dtype=torch.float64) + 0.3 for n in lens]


@pytest.mark.parametrize("norm", [None, "rows"])
def test_reference_padded_auxnet_equals_packed_mean_before_last_layer(norm):
    # (a per-row normalizer turns the reference's all-zero padding rows into 0 / 0 = nan, which its `xs * mask` keeps:
    # with a normalizer the padded form only has a finite answer for sequences of one length -- aux_reference.auxnet_padded)
    p, seqs = _params(7), _seqs([12, 12, 12, 12] if norm else [1, 5, 12, 3], 7)
    normalizer = (lambda x: R.instance_norm(x, -1)) if norm else None
    a, b = R.auxnet_padded(seqs, p, normalizer), R.auxnet_packed(seqs, p, normalizer)
    assert a.shape == (4, 7)
    assert float((a - b).abs().max()) <= 1e-12


def test_reference_normalizers():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 9, 11, generator=g, dtype=torch.float64) * 0.5 + 100
    for dim in (-1, -2):
        y = R.instance_norm(x, dim)
        assert float((y - R.instance_norm_v2(x, dim, dim)).abs().max()) <= 1e-9
        assert float(y.mean(dim).abs().max()) <= 1e-9
        assert float((y.std(dim, unbiased=False) - 1).abs().max()) <= 1e-9
    n = x.shape[-1]
    assert torch.allclose(R.instance_norm(x, -1, unbiased=True) * np.sqrt(n / (n - 1)), R.instance_norm(x, -1), rtol=1e-12)


def test_reference_condition_trial_fold():
    g = torch.Generator().manual_seed(4)
    pre, aux = torch.randn(2, 3, 5, generator=g), torch.randn(2, 4, 5, generator=g)
    xs = R.condition(pre, aux, "mul", trials=2).reshape(2, 2, 4, 3, 5)
    for tr in range(2):
        for k in range(4):
            assert torch.equal(xs[1, tr, k], pre[1] * aux[1, (k + tr) % 4])
    xc = R.condition(pre, aux[..., :2], "cat", trials=1)
    assert xc.shape == (2, 4, 3, 7) and torch.equal(xc[0, 2, 1, 5:], aux[0, 2, :2])


def test_mask_estimator_with_linear_aux_net():
    from tssep_amd.train import net
    me = net.MaskEstimator_v2(idim=12, odim=9, units=5, projs=6, combination="mul", aux_net=net.Linear(7, 9),
                              input_normalizer=net.InstanceNorm(dim=-2, unbiased=True))
    keys = list(me.state_dict())
    assert [k for k in keys if k.startswith("aux_net.")] == ["aux_net.net.weight", "aux_net.net.bias"]
    assert me.aux_net.net.weight.shape == (9, 7)
    # registration order of the reference: pre_net, aux_net, post_net (net.py:554-560, 668)
    assert keys.index("aux_net.net.weight") > keys.index("pre_net.net.1.bias")
    assert keys.index("aux_net.net.weight") < keys.index("post_net.birnn0.net.0.weight_ih_l0")
    text = repr(me)
    assert "(aux_net): Linear(" in text and "(input_normalizer): InstanceNorm(dim=-2, unbiased=True)" in text
    assert list(net.Linear(7, 9, bias=False).state_dict()) == ["net.weight"]


def test_mask_estimator_with_auxnet_and_key_names():
    from tssep_amd.train import net
    plain = net.AuxNet(9)
    assert list(plain.state_dict()) == [f"net.{i}.{n}" for i in (0, 2, 4) for n in ("weight", "bias")]
    normed = net.AuxNet(9, normalizer=net.InstanceNorm())
    assert list(normed.state_dict()) == [f"net.{i}.{n}" for i in (1, 3, 5) for n in ("weight", "bias")]
    assert "(0): InstanceNorm(dim=-1, unbiased=False)" in repr(normed) and "(2): ReLU()" in repr(normed)
    assert repr(net.InstanceNorm_v2()) == "InstanceNorm_v2(mean_dim=-1, norm_dim=-1)"
    me = net.MaskEstimator_v2(idim=12, odim=9, units=5, projs=6, combination="cat", aux_net=normed,
                              aux_net_output_size=9)
    assert me.post_net.birnn0.net[0].input_size == 18
    assert [k for k in me.state_dict() if k.startswith("aux_net.")] == ["aux_net." + k for k in normed.state_dict()]
    with pytest.raises(NotImplementedError):
        net.AuxNet(9, odim=10)


def test_config_round_trip():
    from tssep_amd.train import net
    cfg = net.MaskEstimator_v2.get_config({
        "idim": 12, "odim": 9, "units": 5, "projs": 6, "combination": "cat",
        "aux_net": {"factory": "tssep.train.net.AuxNet", "normalizer": {"factory": "tssep.train.net.InstanceNorm"}},
        "input_normalizer": {"factory": "tssep.train.net.InstanceNorm_v2", "mean_dim": -2, "norm_dim": -2}})
    assert cfg["aux_net"] == {"factory": "tssep.train.net.AuxNet", "idim": 9, "odim": 9,
                              "normalizer": {"factory": "tssep.train.net.InstanceNorm", "dim": -1, "unbiased": False}}
    assert cfg["aux_net_output_size"] == 9                       # net.py:498-499
    me = net.MaskEstimator_v2.from_config(cfg)
    assert isinstance(me.aux_net, net.AuxNet) and isinstance(me.input_normalizer, net.InstanceNorm_v2)
    assert net.MaskEstimator_v2.get_config(cfg) == cfg
    lin = net.MaskEstimator_v2.get_config({"combination": "mul", "idim": 553, "odim": 513,
                                           "aux_net": {"factory": "tssep.train.net.Linear", "idim": 100, "odim": 513},
                                           "aux_normalizer": None})
    assert lin["aux_net"] == {"factory": "tssep.train.net.Linear", "idim": 100, "odim": 513, "bias": True}
    assert isinstance(net.MaskEstimator_v2.from_config(lin).aux_net, net.Linear)
    nrm = net.MaskEstimator_v2.new({"idim": 12, "odim": 9, "units": 5, "projs": 6, "combination": "mul",
                                    "aux_normalizer": {"factory": "tssep.train.net.InstanceNorm_v2"}})
    assert isinstance(nrm.aux_normalizer, net.InstanceNorm_v2) and nrm.aux_net is None


def test_reference_assertions_fire():
    from tssep_amd.train import net
    with pytest.raises(AssertionError):            # net.py:834: aux_net together with aux_normalizer
        net.MaskEstimator_v2(idim=12, odim=9, units=5, projs=6, combination="mul", aux_net=net.Linear(7, 9),
                             aux_normalizer=net.InstanceNorm())
    with pytest.raises(AssertionError):            # net.py:591: cat needs aux_net_output_size == aux_net.odim
        net.MaskEstimator_v2(idim=12, odim=9, units=5, projs=6, combination="cat", aux_net=net.Linear(7, 9),
                             aux_net_output_size=100)


def test_unsupported_dims_raise():
    from tssep_amd.train import net
    for bad in (0, 1, -3):
        with pytest.raises(NotImplementedError):
            net.InstanceNorm(dim=bad)
        with pytest.raises(NotImplementedError):
            net.InstanceNorm_v2(mean_dim=bad, norm_dim=bad)
    with pytest.raises(NotImplementedError):
        net.InstanceNorm_v2(mean_dim=-1, norm_dim=-2)
    with pytest.raises(NotImplementedError, match="PADDED"):
        net.AuxNet(9, normalizer=net.InstanceNorm(dim=-2))
    with pytest.raises(NotImplementedError, match="PADDED"):
        net.AuxNet(9, normalizer=net.InstanceNorm_v2(-2, -2))


@pytest.mark.parametrize("overlay,kind", [("toy_tssep_auxnet.yaml", "linear"), ("toy_tssep_auxnorm.yaml", "norm")])
def test_toy_overlays_resolve(overlay, kind):
    from tssep_amd.train import net, run
    from tssep_amd.train.experiment import Experiment
    for stage in ("toy_tsvad.yaml", "toy_tssep.yaml"):
        cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", stage, overlay)]
                               + ["eg.trainer.storage_dir=/tmp/unused"])
        model = Experiment.from_config(cfg["eg"]).trainer.model
        me = model.mask_estimator
        assert model.reader.aux_size == 100
        if kind == "linear":
            assert isinstance(me.aux_net, net.Linear) and (me.aux_net.idim, me.aux_net.odim) == (100, 513)
            assert me.combination == "mul" and me.aux_normalizer is None
            assert "mask_estimator.aux_net.net.weight" in model.state_dict()
        else:
            assert isinstance(me.aux_normalizer, net.InstanceNorm_v2) and me.aux_net is None
            assert me.combination == "cat" and me.post_net.birnn0.net[0].input_size == 613
