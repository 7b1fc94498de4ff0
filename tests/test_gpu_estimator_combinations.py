"""MaskEstimator_v2 where its options MEET, on a real MI355X, in both GEMM arithmetics: every row of the case table of
tests/test_estimator_reference.py (all pairs of levels of: combination, layout / trials, head, aux kind, dropout, Tanh fold,
input_normalizer, speaker shuffle) against the float64 restatement tests/estimator_reference.py.

Per row: the module built behind torch.manual_seed in training mode, forward and backward of a random-weighted sum over
every differentiable output (mask and logit; mask, vad_mask and vad_logit for explicit_vad), xs and a tensor aux with
requires_grad.  Compared, with the measure and bars of tests/test_rnnp_layer_reference.py taken against the fp32
restatement of the same row (MARGIN = 8, x SPLIT_RATIO for the split-bf16 GEMMs): the outputs, the embedding, every
parameter gradient, d(xs) and d(aux).  Every tensor's figures are printed (pytest -rP); test_zz_report prints the worst
ratio per factor level and arithmetic, which is what DESIGN.md records.

Dropout rows record the {seed, draw} of every site (the pattern of tests/test_gpu_dropout.py), hand the restatement the
host's masks (hip_ops.dropout_keep_host) in logical rows (b, trial, k, t), and count the draws: layers - 1, and the
device's dropout state advanced by exactly as many.

Path assertions keep a row from passing on another path than the one it is in the table for: an act == 2 GEMM request (the
folded Tanh backward) exactly where projs % 4 == 0 and no site is active; Ta > 0 in every cond_* call of a frame-wise row
and Ta == 0 elsewhere; mask_map_* for the nmask = 2 rows and only for them.

Two identities per head kind: an un-batched example gives the bits of the batch of one, and the torch.no_grad() forward
the bits of the grad-enabled one.
"""
import inspect

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_estimator_reference as TR  # noqa: E402
from test_estimator_reference import CASES, FACTORS, IDS, LAYERS  # noqa: E402
from test_gpu_dropout import _record_draws, host_keep  # noqa: E402
from test_rnnp_layer_reference import MARGIN, SPLIT_RATIO  # noqa: E402

T_ = torch.as_tensor
WORST = {}                  # (factor, level, arithmetic) -> (ratio, row, tensor)
_REF = {}                   # row -> {dtype: restatement with the HOST's dropout masks}
DROPOUT_SEED = 4000


@pytest.fixture(params=["f32", "bf16x3"])
def gemm_mode(request):
    from tssep_amd import hip_ops
    old = hip_ops.GEMM_PRECISION
    hip_ops.GEMM_PRECISION = request.param
    yield request.param
    hip_ops.GEMM_PRECISION = old


def _device_inputs(c, inp):
    xs = T_(inp["xs"]).cuda().requires_grad_()
    if c.aux == "auxnet":
        return xs, [[T_(s).cuda() for s in sb] for sb in inp["aux"]], None
    aux = T_(inp["aux"]).cuda().requires_grad_()
    return xs, aux, aux


class _Calls:
    """wraps hip_ops entry points: keeps the bound arguments of every call"""

    def __init__(self, monkeypatch, names):
        from tssep_amd import hip_ops
        self.seen = {n: [] for n in names}
        for n in names:
            monkeypatch.setattr(hip_ops, n, self._wrap(n, getattr(hip_ops, n)))

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        def call(*a, **k):
            self.seen[name].append(sig.bind(*a, **k).arguments)
            return fn(*a, **k)
        return call


def _references(i, c, inp, state, used):
    if not c.dropout:
        return TR.references(i)[2]
    if i not in _REF:
        g = TR.geometry(c)
        rows = TR.B_ * g["trials"] * c.K * TR.T_FRAMES
        keeps = [host_keep(u.cpu(), rows * g["projs"], c.dropout).view(rows, g["projs"]) for u in used]
        assert all(0.5 < float(k.float().mean()) < 0.9 for k in keeps) and not torch.equal(keeps[0], keeps[1])
        _REF[i] = {dt: TR.run_reference(c, state, inp, dt, keeps=keeps) for dt in (torch.float64, torch.float32)}
    return _REF[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_row_against_the_float64_restatement(i, gemm_mode, monkeypatch):
    from tssep_amd import hip_ops as h
    c, g = CASES[i], TR.geometry(CASES[i])
    inp = TR.make_inputs(c)
    me = TR.build_module(c).cuda()
    state = {k: v.detach().cpu().clone() for k, v in me.state_dict().items()}
    xs, aux, aux_leaf = _device_inputs(c, inp)
    calls = _Calls(monkeypatch, ("cond_fwd", "cond_bwd", "cond_aux_bwd", "mask_map_fwd", "mask_map_bwd"))
    h.manual_seed(DROPOUT_SEED + c.seed)
    np.random.seed(TR.shuffle_seed(c))
    h.GEMM_LOG = []
    try:
        with _record_draws() as used:
            out = me(xs, aux)
        after = h.get_state()
        total = sum((getattr(out, n) * T_(inp["w"][n]).cuda()).sum() for n in TR.output_names(c))
        total.backward()
        torch.cuda.synchronize()
    finally:
        log, h.GEMM_LOG = h.GEMM_LOG, None
    # ---- dropout: one draw per active site, the state advanced by as many
    sites = (LAYERS - 1) if c.dropout else 0
    assert len(used) == sites and after == (DROPOUT_SEED + c.seed, sites), (len(used), after)
    assert [u.tolist() for u in used] == [[DROPOUT_SEED + c.seed, d] for d in range(sites)]
    assert h.get_state() == after                                       # the backward draws nothing
    # ---- the path the row is in the table for
    folded = any(d["act"] == 2 for *_, d in log)
    assert folded == bool(c.fold and h.FOLD_TANH and not c.dropout), (folded, c)
    for name in ("cond_fwd", "cond_bwd", "cond_aux_bwd"):
        assert len(calls.seen[name]) == 1, (name, len(calls.seen[name]))       # (d(embedding) is wanted in every row)
        for a in calls.seen[name]:
            assert a.get("Ta", 0) == g["Ta"] and a.get("stride", 1) == g["stride"], (name, a.get("Ta"), a.get("stride"), g)
            assert a["trials"] == g["trials"] and a["K"] == c.K and a["combination"] == c.combination
    two = g["M"] == 2
    assert len(calls.seen["mask_map_fwd"]) == len(calls.seen["mask_map_bwd"]) == int(two), {k: len(v) for k, v in calls.seen.items()}
    # ---- against float64
    ref = _references(i, c, inp, state, used)
    got = {n: getattr(out, n).detach().cpu() for n in TR.output_names(c)}
    got["embedding"] = out.embedding.detach().cpu()
    for k, q in me.named_parameters():
        assert q.grad is not None, k
        got["d " + k] = q.grad.cpu()
    got["d xs"] = xs.grad.cpu()
    if aux_leaf is not None:
        got["d aux"] = aux_leaf.grad.cpu()
    r64, r32 = ref[torch.float64], ref[torch.float32]
    assert set(got) == set(r64), set(got) ^ set(r64)
    for k in got:
        assert got[k].shape == r64[k].shape, (k, got[k].shape, r64[k].shape)
    ratios, bad = TR.compare(got, r64, r32, gemm_mode == "bf16x3", f"row {i:02d} {gemm_mode}")
    worst = max(ratios, key=ratios.get)
    print(f"row {i:02d} {IDS[i]} {gemm_mode}: worst ratio {ratios[worst]:.3g} ({worst})")
    for f in FACTORS:
        key = (f, getattr(c, f), gemm_mode)
        if ratios[worst] > WORST.get(key, (-1.0,))[0]:
            WORST[key] = (ratios[worst], i, worst)
    assert MARGIN == 8.0 and SPLIT_RATIO > 700 and not bad, bad


# one row per head kind: dropout off, a tensor aux
HEAD_ROWS = {"tf1": 0, "t1": 6, "tf2": 12, "t2": 20, "ev": 26}


@pytest.mark.parametrize("head", list(HEAD_ROWS))
def test_unbatched_and_no_grad_give_the_same_bits(head, gemm_mode):
    from tssep_amd import hip_ops as h
    i = HEAD_ROWS[head]
    c = CASES[i]
    assert c.head == head and not c.dropout and c.aux != "auxnet"
    inp = TR.make_inputs(c)
    me = TR.build_module(c).cuda()
    xs, aux = T_(inp["xs"]).cuda(), T_(inp["aux"]).cuda()
    names = TR.output_names(c) + ("embedding",)
    before = h.get_state()

    def run(x, a, grad):
        np.random.seed(TR.shuffle_seed(c))
        if grad:
            return me(x.clone().requires_grad_(), a.clone().requires_grad_())
        with torch.no_grad():
            return me(x, a)

    with_grad, without = run(xs, aux, True), run(xs, aux, False)
    assert getattr(with_grad, names[0]).requires_grad and not getattr(without, names[0]).requires_grad
    for n in names:
        assert torch.equal(getattr(with_grad, n).detach(), getattr(without, n)), (head, n)
    one, batch = run(xs[0], aux[0], False), run(xs[:1], aux[:1], False)
    for n in names:
        a, b = getattr(one, n), getattr(batch, n)
        assert a.shape == b.shape[1:] and torch.equal(a, b[0]), (head, n, a.shape, b.shape)
    assert h.get_state() == before


def test_zz_report():
    """the worst ratio to the fp32 restatement's own error per factor level and arithmetic, over the rows that ran"""
    if not WORST:
        print("no row ran in this process")
    for f, levels in FACTORS.items():
        for lv in levels:
            cells = []
            for mode in ("f32", "bf16x3"):
                r = WORST.get((f, lv, mode))
                cells.append(f"{mode} {r[0]:8.3g} (row {r[1]:02d}, {r[2]})" if r else f"{mode} --")
            print(f"{f:12s} {str(lv):11s} " + "   ".join(cells))
    assert all(np.isfinite(v[0]) for v in WORST.values())
