"""tests/estimator_reference.py -- the one restatement of MaskEstimator_v2.forward with every option -- tested without a
GPU, and the case table of tests/test_gpu_estimator_combinations.py.

Anchoring.  In float64 the restatement gives the numbers of the two restatements the suite already pins
(oracle.net.mask_estimator_forward on every me_*.npz configuration, framewise_reference.mask_estimator_forward on the
frame-wise cases: outputs and the gradients behind the conditioning bit for bit, the pre-net's gradients and d(aux) to
1e-13 of the tensor's largest entry -- autograd adds d(pre) over trials and speakers in another order), and in fp32, with their `perm`, it reproduces the reference project's fixtures me_*.npz and ev_me_*.npz
inside the bars tests/test_oracle.py and tests/test_explicit_vad.py hold the oracle to.

The case table.  CASES is a committed list: eight factors (FACTORS), every PAIR of levels of two different factors occurs
in a row (`test_every_accepted_pair_of_levels_is_in_the_table` computes the pairs the constructor accepts and looks each
one up); what the class refuses is shown to raise.  Widths follow the finding of tests/test_gpu_framewise_embeddings.py
(profiles/framewise_ratio_survey.jsonl): units 64, projs 48 (the Tanh fold on) or 46 (off), idim 40, odim 32, B = 2,
K = 3 or 4, T = 9 (stride 4: buckets of 4, 4 and 1 frames), AuxNet enrolments of ragged lengths with a length-1 sequence.

The measure is tests/test_rnnp_layer_reference.py's, imported: per tensor the normwise and element-wise error against
float64, bounded by MARGIN x the fp32 restatement's own (x SPLIT_RATIO for split-bf16 GEMMs).  For every row an
INDEPENDENT fp32 implementation (torch.nn.LSTM + Linear + Tanh under autograd, the same injected dropout masks) must be
inside the fp32 bound -- the margin holds for the reference alone, before any kernel is measured -- and every planted
defect (estimator_reference.DEFECTS) must be rejected under the WIDER bound by every row that exercises it.
"""
import collections
import glob
import itertools
import os

import numpy as np
import pytest
import torch

import estimator_reference as ER
import framewise_reference as FW
from oracle import net as onet
from oracle.rnnp import rnnp
from test_rnnp_layer_reference import (FLOOR, LSTM_ATTRS, MARGIN, SPLIT_RATIO, U, bounds, errors, module_params, modules)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
T_ = torch.as_tensor

FACTORS = collections.OrderedDict(
    combination=("mul", "cat"),
    layout=("spk", "tsvad", "tsvad2"),                 # ts_vad=False | ts_vad=K, one trial | ts_vad=K, two trials
    head=("tf1", "t1", "tf2", "t2", "ev"),             # resolution / nmask, or explicit_vad
    aux=("3d", "3d_norm", "4d_s1", "4d_s4_norm", "linear", "auxnet"),
    dropout=(0, 0.3),                                  # 0.3: in training mode
    fold=(True, False),                                # projs % 4 == 0
    input_norm=(False, True),                          # InstanceNorm(dim=-2)
    shuffle=(True, False),
)
Case = collections.namedtuple("Case", tuple(FACTORS) + ("K", "seed"))
CASES = [Case(*c) for c in (
    ("cat", "spk", "tf1", "3d", 0, True, True, True, 3, 0),
    ("mul", "tsvad", "tf1", "3d_norm", 0.3, True, False, True, 4, 1),
    ("mul", "tsvad2", "tf1", "4d_s1", 0, True, True, False, 3, 2),
    ("cat", "tsvad", "tf1", "4d_s4_norm", 0, False, True, False, 4, 3),
    ("cat", "tsvad", "tf1", "linear", 0, False, True, True, 3, 4),
    ("mul", "tsvad", "tf1", "auxnet", 0.3, False, False, True, 4, 5),
    ("mul", "tsvad", "t1", "3d", 0, True, True, False, 3, 6),
    ("cat", "tsvad2", "t1", "3d_norm", 0.3, False, True, True, 4, 7),
    ("cat", "tsvad2", "t1", "4d_s1", 0, True, False, False, 3, 8),
    ("mul", "tsvad2", "t1", "4d_s4_norm", 0, False, False, True, 4, 9),
    ("mul", "spk", "t1", "linear", 0.3, True, False, False, 3, 10),
    ("mul", "tsvad", "t1", "auxnet", 0, True, False, False, 4, 11),
    ("cat", "spk", "tf2", "3d", 0, True, True, True, 3, 12),
    ("mul", "tsvad2", "tf2", "3d_norm", 0, True, False, False, 4, 13),
    ("mul", "tsvad2", "tf2", "4d_s1", 0.3, False, True, False, 3, 14),
    ("cat", "spk", "tf2", "4d_s4_norm", 0.3, False, False, False, 4, 15),
    ("cat", "tsvad", "tf2", "linear", 0.3, True, False, True, 3, 16),
    ("mul", "tsvad2", "tf2", "auxnet", 0, True, True, True, 4, 17),
    ("cat", "tsvad2", "t2", "3d", 0.3, False, False, True, 3, 18),
    ("cat", "spk", "t2", "3d_norm", 0, True, False, True, 4, 19),
    ("mul", "tsvad", "t2", "4d_s1", 0, True, True, False, 3, 20),
    ("mul", "spk", "t2", "4d_s4_norm", 0.3, True, False, True, 4, 21),
    ("mul", "tsvad2", "t2", "linear", 0, False, True, False, 3, 22),
    ("mul", "spk", "t2", "auxnet", 0, True, False, True, 4, 23),
    ("mul", "tsvad", "ev", "3d", 0.3, True, True, True, 3, 24),
    ("mul", "tsvad", "ev", "3d_norm", 0, True, False, False, 4, 25),
    ("cat", "spk", "ev", "4d_s1", 0, False, False, True, 3, 26),
    ("mul", "spk", "ev", "4d_s4_norm", 0.3, True, False, False, 4, 27),
    ("mul", "tsvad2", "ev", "linear", 0, True, False, False, 3, 28),
    ("cat", "tsvad", "ev", "auxnet", 0.3, True, True, False, 4, 29),
    # two triples on top of the pairs: trial rotation x gate x dropout on frame-wise cat, two masks x trials x dropout
    ("cat", "tsvad2", "ev", "4d_s1", 0.3, True, True, True, 4, 30),
    ("mul", "tsvad2", "tf2", "4d_s4_norm", 0.3, False, False, True, 3, 31),
)]
IDS = [f"{i:02d}-" + "-".join(str(v) for v in c[:8]) for i, c in enumerate(CASES)]

B_, T_FRAMES, IDIM, ODIM, UNITS, LAYERS = 2, 9, 40, 32, 64, 3
E_CAT, LINEAR_IN = 18, 7               # cat: an embedding width that is no multiple of 4; the Linear aux_net's input width
ENROLMENT = (4, 9, 1, 6, 2, 11, 1, 5)  # ragged AuxNet enrolment lengths, taken in turn (length-1 sequences included)


# ---- one case: constructor arguments, inputs, the restatement's arguments ----------------------------------------------
def geometry(c):
    trials = 2 if c.layout == "tsvad2" else 1
    M = 2 if c.head in ("tf2", "t2") else 1
    E = ODIM if c.combination == "mul" else E_CAT
    Ta = {"4d_s1": T_FRAMES, "4d_s4_norm": FW.frames_of(T_FRAMES, 4)}.get(c.aux, 0)
    return dict(trials=trials, M=M, E=E, Ta=Ta, stride=4 if c.aux == "4d_s4_norm" else 1, projs=48 if c.fold else 46,
                ts_vad=False if c.layout == "spk" else c.K, res="t" if c.head in ("t1", "t2") else "tf",
                ev=c.head == "ev")


def module_kwargs(c):
    """the keyword arguments of tssep_amd.train.net.MaskEstimator_v2 for the row"""
    from tssep_amd.train import net
    g = geometry(c)
    aux_net = aux_norm = None
    if c.aux == "linear":
        aux_net = net.Linear(LINEAR_IN, g["E"])
    elif c.aux == "auxnet":
        aux_net = net.AuxNet(g["E"])
    elif c.aux == "3d_norm":
        aux_norm = net.InstanceNorm_v2(-1, -1)
    elif c.aux == "4d_s4_norm":
        aux_norm = net.InstanceNorm(dim=-2)
    return dict(idim=IDIM, odim=ODIM, layers=LAYERS, units=UNITS, projs=g["projs"], dropout=c.dropout, nmask=g["M"],
                aux_net=aux_net, aux_net_output_size=g["E"], combination=c.combination, ts_vad=g["ts_vad"],
                output_resolution=g["res"], random_speaker_order=c.shuffle, num_averaged_permutations=g["trials"],
                input_normalizer=net.InstanceNorm(dim=-2) if c.input_norm else None, aux_normalizer=aux_norm,
                explicit_vad=g["ev"], aux_stride=g["stride"])


def build_module(c):
    from tssep_amd.train import net
    torch.manual_seed(100 + c.seed)
    return net.MaskEstimator_v2(**module_kwargs(c)).train()


def reference_kwargs(c):
    g = geometry(c)
    return dict(odim=ODIM, combination=c.combination, ts_vad=g["ts_vad"], output_resolution=g["res"], nmask=g["M"],
                explicit_vad=g["ev"], num_averaged_permutations=g["trials"], layers=LAYERS,
                input_normalizer=("instance_norm", -2) if c.input_norm else None,
                aux_normalizer={"3d_norm": ("instance_norm_v2", -1), "4d_s4_norm": ("instance_norm", -2)}.get(c.aux),
                aux_net=c.aux if c.aux in ("linear", "auxnet") else None, aux_stride=g["stride"], dropout=c.dropout)


def output_names(c):
    return ("mask", "vad_mask", "vad_logit") if c.head == "ev" else ("mask", "logit")


def shuffle_seed(c):
    return 7000 + c.seed


def make_inputs(c):
    """-> dict: xs [B, T, idim], aux (array, or lists of arrays for AuxNet), perm [B, K] or None, w: one weight array per
    differentiable output (the scalar is sum_o sum(out_o w_o)), keeps: None or the CPU stand-in masks of the sites"""
    from tssep_amd.train.net import MaskEstimator_v2
    g = geometry(c)
    rng = np.random.RandomState(500 + c.seed)
    K, E = c.K, g["E"]
    xs = (rng.randn(B_, T_FRAMES, IDIM) * 1.5 + 0.3).astype(np.float32)
    if c.aux == "auxnet":
        lens = [[ENROLMENT[(c.seed + b * K + k) % len(ENROLMENT)] for k in range(K)] for b in range(B_)]
        lens[0][K - 1] = 1
        aux = [[(rng.randn(n, E) * 0.7 + 0.2).astype(np.float32) for n in lb] for lb in lens]
    elif c.aux == "linear":
        aux = rng.randn(B_, K, LINEAR_IN).astype(np.float32)
    elif g["Ta"]:
        aux = (rng.randn(B_, K, g["Ta"], E) + 0.5).astype(np.float32)
    else:
        aux = (rng.randn(B_, K, E) + 0.5).astype(np.float32)
    shape = (B_, K, g["M"], T_FRAMES, ODIM)
    w = {n: rng.randn(*(shape if n in ("mask", "logit") else shape[:4])).astype(np.float32) for n in output_names(c)}
    perm = None
    if c.shuffle:
        np.random.seed(shuffle_seed(c))                        # what the module's own draw gives behind the same seed
        perm = MaskEstimator_v2.draw_permutations(B_, K)[0]
    keeps = None
    if c.dropout:
        gen = torch.Generator().manual_seed(900 + c.seed)
        rows = B_ * g["trials"] * K * T_FRAMES
        keeps = [torch.rand(rows, g["projs"], generator=gen) >= c.dropout for _ in range(LAYERS - 1)]
    return dict(xs=xs, aux=aux, perm=perm, w=w, keeps=keeps)


class TorchLayers:
    """The RNNP layer by torch.nn.LSTM(bidirectional) + torch.nn.Linear in `dtype` under autograd: ATen's fused LSTM, other
    kernels and summation orders than oracle.rnnp.  The containers are kept; grads() names their gradients."""

    def __init__(self, dtype):
        self.dtype, self.made = dtype, {}

    def __call__(self, x, p, prefix):
        params = [p[prefix + "net.0." + a] for a in LSTM_ATTRS] + [p[prefix + "net.1.weight"], p[prefix + "net.1.bias"]]
        lstm, lin = modules([t.detach() for t in params], dtype=self.dtype)
        self.made[prefix] = (lstm, lin)
        h = x.reshape(-1, x.shape[-2], x.shape[-1])
        y = lin(lstm(h)[0])
        return y.reshape(*x.shape[:-1], y.shape[-1])

    def grads(self):
        out = {}
        for prefix, (lstm, lin) in self.made.items():
            names = ["net.0." + a for a in LSTM_ATTRS] + ["net.1.weight", "net.1.bias"]
            out.update({prefix + n: t.grad for n, t in zip(names, module_params(lstm, lin))})
        return out


def run_reference(c, state, inp, dtype, keeps=None, layer=None, defect=None):
    """The restatement of row `c` on the weights `state` (a state_dict), forward and backward of the weighted sum over
    every differentiable output -> {output name, "embedding", "d <parameter>", "d xs", "d aux" (a tensor aux)}"""
    p = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in state.items()}
    xs = T_(inp["xs"]).to(dtype).requires_grad_()
    if c.aux == "auxnet":
        aux, aux_leaf = [[T_(s).to(dtype) for s in sb] for sb in inp["aux"]], None
    else:
        aux = aux_leaf = T_(inp["aux"]).to(dtype).requires_grad_()
    out = ER.estimator_forward(p, xs, aux, perm=inp["perm"], keeps=keeps if keeps is not None else inp["keeps"],
                               layer=layer or rnnp, defect=defect, **reference_kwargs(c))
    total = sum((out[n] * T_(inp["w"][n]).to(dtype)).sum() for n in output_names(c))
    total.backward()
    res = {n: out[n].detach() for n in output_names(c)}
    res["embedding"] = out["embedding"].detach()
    grads = {k: v.grad for k, v in p.items()}
    if layer is not None and hasattr(layer, "grads"):
        grads.update(layer.grads())
    missing = [k for k, v in grads.items() if v is None]
    assert not missing, missing
    res.update({"d " + k: v for k, v in grads.items()})
    res["d xs"] = xs.grad
    if aux_leaf is not None:
        res["d aux"] = aux_leaf.grad
    return res


def compare(got, r64, r32, split, what, names=None):
    """prints norm, element and ratio per tensor (the format of tests/test_gpu_framewise_embeddings.py)
    -> ({tensor: ratio to the fp32 restatement's own error}, the tensors outside their bound)"""
    ratios, bad = {}, []
    for k in names or r64:
        e, b, own = errors(got[k], r64[k]), bounds(r32[k], r64[k], split), errors(r32[k], r64[k])
        ratios[k] = max(e[0] / max(own[0], U), e[1] / max(own[1], U))
        print(f"{what} {k:46s} norm {e[0]:.3g} (<= {b[0]:.3g}) elem {e[1]:.3g} (<= {b[1]:.3g}) "
              f"ratio to the fp32 restatement {ratios[k]:.3g}")
        if not (e[0] <= b[0] and e[1] <= b[1]):
            bad.append(k)
    return ratios, bad


_REF = {}


def references(i):
    """-> (inputs, state_dict, {float64: ..., float32: ...}) of CASES[i], computed once per process and left unchanged"""
    if i not in _REF:
        c = CASES[i]
        state = {k: v.clone() for k, v in build_module(c).state_dict().items()}
        inp = make_inputs(c)
        _REF[i] = (inp, state, {dt: run_reference(c, state, inp, dt) for dt in (torch.float64, torch.float32)})
    return _REF[i]


# ---- anchoring ---------------------------------------------------------------------------------------------------------
ME_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "me_*.npz")))
EV_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "ev_me_*.npz")))


def _fixture(g, dtype):
    comb, ts_vad, res, nap = [str(s) for s in g["cfg"]]
    kw = dict(combination=comb, ts_vad=False if ts_vad == "False" else int(ts_vad), output_resolution=res,
              num_averaged_permutations=int(nap))
    p = {k[2:]: T_(v).to(dtype).requires_grad_() for k, v in g.items() if k.startswith("p.")}
    return kw, p


def _same_gradients(p, q, what):
    """bit for bit behind the conditioning; the pre-net's gradients sum d(pre) over trials and speakers, which autograd adds
    in the order of the restatement's indexing: to 1e-13 of the largest entry"""
    for k in p:
        if "pre_net." in k:
            assert float((p[k].grad - q[k].grad).abs().max()) <= 1e-13 * float(q[k].grad.abs().max()), (what, k)
        else:
            assert torch.equal(p[k].grad, q[k].grad), (what, k)


@pytest.mark.parametrize("name", ME_CASES)
def test_float64_equals_the_oracle_on_every_fixture_configuration(golden, name):
    g = golden(name)
    assert len(ME_CASES) == 28
    kw, p = _fixture(g, torch.float64)
    _, q = _fixture(g, torch.float64)
    xs, aux, w = T_(g["xs"]).double(), T_(g["aux"]).double(), T_(g["g"]).double()
    mine = ER.estimator_forward(p, xs, aux, odim=9, perm=g["perm"], **kw)
    theirs = onet.mask_estimator_forward(q, xs, aux, odim=9, perm=g["perm"], prefix="", **kw)
    for k in ("logit", "mask", "embedding"):
        assert torch.equal(mine[k], theirs[k]), k
    (mine["mask"] * w).sum().backward()
    (theirs["mask"] * w).sum().backward()
    _same_gradients(p, q, name)


@pytest.mark.parametrize("norm", [None, ("instance_norm", -1), ("instance_norm", -2)])
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("nap", [1, 2])
@pytest.mark.parametrize("combination", ["mul", "cat"])
def test_float64_equals_the_framewise_restatement(combination, nap, stride, norm):
    """the configurations of tests/test_gpu_framewise_embeddings.py case 2 (+ its case 3's normalizers), on a row's weights"""
    c = CASES[2]._replace(combination=combination, layout="tsvad2" if nap > 1 else "spk", aux="4d_s1", K=4, shuffle=True)
    state = build_module(c).state_dict()
    rng = np.random.RandomState(3 + stride)
    E = geometry(c)["E"]
    xs = T_(rng.randn(B_, T_FRAMES, IDIM)).double()
    a0 = T_(rng.randn(B_, 4, FW.frames_of(T_FRAMES, stride), E) + 0.5).double()
    a = [a0.clone().requires_grad_() for _ in (0, 1)]
    perm = np.stack([rng.permutation(4) for _ in range(B_)])
    kw = dict(odim=ODIM, aux_stride=stride, combination=combination, ts_vad=4 if nap > 1 else False,
              num_averaged_permutations=nap, perm=perm)
    p, q = ({k: v.detach().double().requires_grad_() for k, v in state.items()} for _ in (0, 1))
    mine = ER.estimator_forward(p, xs, a[0], aux_normalizer=norm, **kw)
    theirs = FW.mask_estimator_forward(q, xs, a[1], aux_normalizer=None if norm is None else (lambda v: ER.normalize(v, norm)), **kw)
    for k in ("logit", "mask", "embedding"):
        assert torch.equal(mine[k], theirs[k]), k
    w = T_(rng.randn(*mine["mask"].shape))
    (mine["mask"] * w).sum().backward()
    (theirs["mask"] * w).sum().backward()
    _same_gradients(p, q, "parameters")
    assert float((a[0].grad - a[1].grad).abs().max()) <= 1e-13 * float(a[1].grad.abs().max())


@pytest.mark.parametrize("name", ME_CASES)
def test_fp32_reproduces_the_reference_fixture(golden, name):
    """the bars of tests/test_oracle.py::test_mask_estimator_against_reference_fixture"""
    g = golden(name)
    kw, p = _fixture(g, torch.float32)
    out = ER.estimator_forward(p, T_(g["xs"]), T_(g["aux"]), odim=9, perm=g["perm"], **kw)
    np.testing.assert_allclose(out["logit"].detach().numpy(), g["logit"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(out["mask"].detach().numpy(), g["mask"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(out["embedding"].numpy(), g["embedding"])
    (out["mask"] * T_(g["g"])).sum().backward()
    for k, v in p.items():
        np.testing.assert_allclose(v.grad.numpy(), g["dp." + k], rtol=2e-4, atol=2e-6, err_msg=k)


@pytest.mark.parametrize("name", EV_CASES)
def test_fp32_reproduces_the_explicit_vad_fixture(golden, name):
    """the bars of tests/test_explicit_vad.py::test_oracle_composition_against_reference_fixture"""
    g = golden(name)
    assert len(EV_CASES) == 6
    kw, p = _fixture(g, torch.float32)
    out = ER.estimator_forward(p, T_(g["xs"]), T_(g["aux"]), odim=9, perm=g["perm"], explicit_vad=True, **kw)
    assert out["logit"] is None
    for key in ("mask", "vad_mask", "vad_logit"):
        np.testing.assert_allclose(out[key].detach().numpy(), g[key], rtol=1e-5, atol=2e-6, err_msg=key)
    np.testing.assert_allclose(out["embedding"].numpy(), g["embedding"])
    ((out["mask"] * T_(g["g"])).sum() + (out["vad_mask"] * T_(g["gv"])).sum()).backward()
    for k, v in p.items():
        np.testing.assert_allclose(v.grad.numpy(), g["dp." + k], rtol=2e-4, atol=2e-6, err_msg=k)


def test_unbatched_input_is_entry_0_of_the_batch_of_one():
    for i in (0, 14, 26):
        c = CASES[i]
        inp, state, _ = references(i)
        p = {k: v.double() for k, v in state.items()}
        kw = dict(reference_kwargs(c), keeps=None, dropout=0.0)
        perm = None if inp["perm"] is None else inp["perm"][1:2]
        xs, aux = T_(inp["xs"]).double(), T_(inp["aux"]).double()
        one = ER.estimator_forward(p, xs[1], aux[1], perm=None if perm is None else perm[0], **kw)
        batch = ER.estimator_forward(p, xs[1:2], aux[1:2], perm=perm, **kw)
        for n in output_names(c) + ("embedding",):
            assert one[n].shape == batch[n].shape[1:] and torch.equal(one[n], batch[n][0]), (i, n)


# ---- the case table ----------------------------------------------------------------------------------------------------
def _probe(levels):
    """a row with the given levels and, for the other factors, the first level that goes with them"""
    base = dict(combination="mul", layout="tsvad", head="tf1", aux="3d", dropout=0, fold=True, input_norm=False, shuffle=True)
    base.update(levels)
    return Case(K=4, seed=0, **base)


def test_every_accepted_pair_of_levels_is_in_the_table():
    assert 30 <= len(CASES) <= 40 and len(set(c[:8] for c in CASES)) == len(CASES)
    for c in CASES:
        assert all(getattr(c, f) in lv for f, lv in FACTORS.items()) and c.K in (3, 4), c
    have = {((f, getattr(c, f)), (h, getattr(c, h))) for c in CASES for f, h in itertools.combinations(FACTORS, 2)}
    wanted, refused = set(), []
    for f, h in itertools.combinations(FACTORS, 2):
        for x, y in itertools.product(FACTORS[f], FACTORS[h]):
            try:
                build_module(_probe({f: x, h: y}))
            except (AssertionError, NotImplementedError, ValueError) as e:
                refused.append(((f, x), (h, y), type(e).__name__))
                continue
            wanted.add(((f, x), (h, y)))
    print(f"{len(wanted)} accepted pairs of levels, {len(refused)} refused, {len(CASES)} rows")
    assert not refused, refused          # every refusal of the class lies INSIDE one factor (the test below)
    assert len(wanted) == sum(len(FACTORS[f]) * len(FACTORS[h]) for f, h in itertools.combinations(FACTORS, 2))
    assert not wanted - have, sorted(wanted - have)


def test_refused_combinations_raise():
    from tssep_amd.train import net
    kw = dict(idim=IDIM, odim=ODIM, layers=LAYERS, units=UNITS, projs=48, combination="mul")
    with pytest.raises(AssertionError, match="explicit_vad needs output_resolution='tf'"):
        net.MaskEstimator_v2(ts_vad=4, explicit_vad=True, output_resolution="t", **kw)
    with pytest.raises(NotImplementedError, match="explicit_vad=True with nmask=2"):
        net.MaskEstimator_v2(ts_vad=4, explicit_vad=True, nmask=2, **kw)
    with pytest.raises(AssertionError):
        net.MaskEstimator_v2(ts_vad=False, num_averaged_permutations=2, **kw)
    for aux_net in (net.Linear(LINEAR_IN, ODIM), net.AuxNet(ODIM)):
        with pytest.raises(AssertionError, match="Not clear, whether before or after"):
            net.MaskEstimator_v2(aux_net=aux_net, aux_normalizer=net.InstanceNorm(), **kw)
    # (an AuxNet reads [B, K, T_i, idim] as its enrolment sequences: only a tensor-valued aux_net can meet a 4-D embedding)
    me = net.MaskEstimator_v2(aux_net=net.Linear(LINEAR_IN, ODIM), ts_vad=4, **kw)
    with pytest.raises(NotImplementedError, match="on frame-wise embeddings"):           # before anything is launched
        me(torch.zeros(B_, T_FRAMES, IDIM), torch.zeros(B_, 4, T_FRAMES, LINEAR_IN))
    # ... and the restatement refuses the same
    p = {}
    for bad in (dict(explicit_vad=True, output_resolution="t"), dict(explicit_vad=True, nmask=2),
                dict(num_averaged_permutations=2), dict(aux_net="linear", aux_normalizer=("instance_norm", -1))):
        with pytest.raises(AssertionError):
            ER.estimator_forward(p, torch.zeros(B_, T_FRAMES, IDIM), torch.zeros(B_, 4, ODIM), odim=ODIM, **bad)


def test_table_rows_build_what_they_say():
    for i, c in enumerate(CASES):
        me, g, inp = build_module(c), geometry(c), make_inputs(c)
        assert me.training and len(me._dropouts) == LAYERS - 1 and me._birnns[0].hdim == g["projs"]
        assert (g["projs"] % 4 == 0) == c.fold and me.explicit_vad == (c.head == "ev") and me.nmask == g["M"]
        assert (inp["keeps"] is None) == (c.dropout == 0) and (inp["perm"] is None) == (not c.shuffle)
        if c.aux == "auxnet":
            assert 1 in [len(s) for sb in inp["aux"] for s in sb] and len({len(s) for sb in inp["aux"] for s in sb}) > 2
        if c.aux == "4d_s4_norm":
            assert inp["aux"].shape[2] == 3 and T_FRAMES - 2 * 4 == 1            # buckets of 4, 4 and 1
        if inp["perm"] is not None:
            assert any(list(q) != sorted(q) for q in inp["perm"]), (i, inp["perm"])


# ---- the margin holds for the reference alone --------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_margin_covers_an_independent_fp32_implementation(i):
    c = CASES[i]
    inp, state, ref = references(i)
    got = run_reference(c, state, inp, torch.float32, layer=TorchLayers(torch.float32))
    assert set(got) == set(ref[torch.float64])
    ratios, bad = compare(got, ref[torch.float64], ref[torch.float32], False, f"row {i:02d} torch.nn fp32")
    worst = max(ratios, key=ratios.get)
    print(f"row {i:02d} {IDS[i]}: worst ratio {ratios[worst]:.3g} ({worst})")
    assert MARGIN == 8.0 and FLOOR == 2.0 ** -4 and SPLIT_RATIO > 700 and not bad, bad


# ---- teeth -------------------------------------------------------------------------------------------------------------
EXERCISED_BY = {
    "dropout_backward_unscaled": lambda c: c.dropout > 0,
    "dropout_mask_combined_order": lambda c: c.dropout > 0 and c.layout != "spk",
    "gate_outside_trial_mean": lambda c: c.head == "ev" and c.layout == "tsvad2",
    "masks_swapped_in_t": lambda c: c.head == "t2",
    "shuffle_on_time_axis": lambda c: c.aux in ("4d_s1", "4d_s4_norm") and c.shuffle,
    "input_normalizer_constant": lambda c: c.input_norm,
    "aux_normalizer_along_e": lambda c: c.aux == "4d_s4_norm",
    "daux_cat_from_pre_columns": lambda c: c.combination == "cat",
}


@pytest.mark.parametrize("defect", ER.DEFECTS)
def test_planted_defects_are_rejected(defect):
    """the defect planted in the float64 restatement fails the WIDER (split-bf16) bound on EVERY row that exercises it, and
    the fp32 restatement of the same rows is inside the narrower one with the margin to spare"""
    assert set(EXERCISED_BY) == set(ER.DEFECTS)
    rows = [i for i, c in enumerate(CASES) if EXERCISED_BY[defect](c)]
    assert rows, defect
    for i in rows:
        inp, state, ref = references(i)
        r64, r32 = ref[torch.float64], ref[torch.float32]
        bad64 = run_reference(CASES[i], state, inp, torch.float64, defect=defect)
        rejected = [k for k in r64 if not all(e <= b for e, b in zip(errors(bad64[k], r64[k]), bounds(r32[k], r64[k], True)))]
        print(f"{defect}: row {i:02d} rejected in {len(rejected)} tensors, e.g. {rejected[:3]}")
        assert rejected, (defect, i)
        for k in r64:
            e, b = errors(r32[k], r64[k]), bounds(r32[k], r64[k], False)
            assert e[0] * MARGIN <= b[0] * (1 + 1e-12) and e[1] * MARGIN <= b[1] * (1 + 1e-12), (i, k)
