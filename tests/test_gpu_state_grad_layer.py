"""functional.rnnp_layer(state=..., return_state=True, state_grad=True) on torch.nn.LSTM / torch.nn.GRU + Linear containers
(one direction of time) on a real MI355X, in both GEMM arithmetics, against torch.nn.LSTM / GRU + Linear (+ Tanh) in
float64 on the CPU with a state that requires a gradient and a loss over the output AND the final state
(tests/state_grad_reference.py).  Compared: dx, the six parameter gradients, dh0, dc0, hT, cT, y.

Measure and bound are tests/test_rnnp_layer_reference.py's, unchanged: per tensor the normwise and the element-wise error
against float64, each within MARGIN x the same figure of the fp32 restatement of the same case under GEMM_PRECISION =
"f32", and that x SPLIT_RATIO under "bf16x3".  At toy widths (5 - 12 units) the restatement's figure is the largest over
twelve seeds (state_grad_reference.yardstick, gru_reference.chain_yardstick's measure, for the reason DESIGN 4.20 measured:
one draw's worst error there is one or two roundings on one element).

Shapes: test_causal_reference.LAYER_SHAPES' small ones and (32, 7, 321, 300, 320, 0).  Chunks: T = 23 as (23), (1 x 23),
(5, 1, 17) with the state kept in the graph against the whole-sequence float64 gradients, and detached against the float64
gradients truncated at the same places (tests/test_state_grad_reference.py asserts how far those two are apart).
Direct-sink accumulation over chunks gives the sum.  state_grad=False is the unchanged call, and a returned state nobody
differentiates leaves the launch list unchanged.

Measured on an MI355X (pytest -rP, test_zz_report), the largest error / (the fp32 restatement's error) per tensor over the
file: under "f32" (allowed 8) LSTM y 4.2, x 2.6, w_ih 2.1, w_hh 1.8, b_ih 1.9, b_hh 1.9, w_proj 1.8, b_proj 3.9, h0 1.4,
c0 1.9, hT 1.4, cT 1.3; GRU y 2.1, x 3.2, w_ih 1.7, w_hh 1.8, b_ih 1.9, b_hh 2.1, w_proj 1.8, b_proj 4.0, h0 1.8, hT 1.8;
under "bf16x3" (allowed 8 x 770.6 = 6165) LSTM at most 88 (h0), GRU at most 100 (hT)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

import gru_reference as G  # noqa: E402
import state_grad_reference as S  # noqa: E402
from test_rnnp_layer_reference import assert_within, failures  # noqa: E402
from tssep_amd import functional as Fn, hip_ops as H  # noqa: E402
from tssep_amd.distributed import GradBucket  # noqa: E402
from tssep_amd.train import runtime  # noqa: E402

DEV = "cuda"
F64, F32 = torch.float64, torch.float32
RATIOS = {}          # (mode, cell, tensor) -> the largest error / (the fp32 restatement's error) this run saw (test_zz_report)
TOY_UNITS = 12       # up to here the yardstick over seeds


@pytest.fixture(params=["f32", "bf16x3"])
def mode(request):
    """both GEMM arithmetics, hence both values of fused_colsum(); restored afterwards"""
    with runtime.applied(gemm_precision=request.param):
        assert H.fused_colsum() == (request.param == "bf16x3")
        yield request.param


def is_split():
    return H.GEMM_PRECISION != "f32"


def ident(s):
    return "x".join(map(str, s))


@contextlib.contextmanager
def logged():
    """-> dict(recurrence=[...], wgrads=[(M, N, R) of every weight-gradient product])"""
    seen = dict(recurrence=[], wgrads=[])
    keep = H.wgrad, H.RECURRENCE_LOG

    def wgrad_(dY, ld_dy, X, ld_x, M, N, R, **k):
        seen["wgrads"].append((M, N, R))
        return keep[0](dY, ld_dy, X, ld_x, M, N, R, **k)

    H.wgrad, H.RECURRENCE_LOG = wgrad_, seen["recurrence"]
    try:
        yield seen
    finally:
        H.wgrad, H.RECURRENCE_LOG = keep


def launches(seen):
    return [(e["kernel"], e["direction"], e["sequences"], e["frames"], e["units"]) for e in seen["recurrence"]]


def run(case, N, T, gru, act, combine=0, chunks=None, detach=False, sinks=False, state_loss=True, **kw):
    """The layer on the GPU over `chunks` (None: one call) with the state handed over -> the outputs on the host, keyed as
    state_grad_reference.layer's.  kw: what rnnp_layer is called with in place of state_grad=True."""
    x, params, dy, dlast, state = case
    kw = kw or dict(state_grad=True)
    rnn, lin = S.modules_of(params, gru, device=DEV)
    ps = S.params_of(rnn, lin)
    bucket = GradBucket(ps) if sinks else None
    xg = x.to(DEV).view(N, T, -1).clone().requires_grad_()
    leaves = [s.to(DEV).clone().requires_grad_() for s in state]
    st, ys, t0 = list(leaves), [], 0
    assert not (combine and chunks)
    for n in chunks or [T]:
        y, last = Fn.rnnp_layer(xg[:, t0:t0 + n].reshape(N * n, -1), rnn, lin, N, n, act=act, combine=combine,
                                state=st[0] if gru else tuple(st), return_state=True, **kw)
        ys.append(y if combine else y.view(N, n, -1))
        last = [last] if gru else list(last)
        st = [s.detach() for s in last] if detach else last
        t0 += n
    y = ys[0] if combine else torch.cat(ys, 1).reshape(N * T, -1)
    loss = (y * dy.to(DEV)).sum()
    if state_loss:
        for s, d in zip(last, dlast):
            loss = loss + (s * d.to(DEV)).sum()
    loss.backward()
    if bucket is not None:
        bucket.sync()            # the side stream's weight gradients, BEFORE anything reads the bucket
    torch.cuda.synchronize()
    out = {k: p.grad.detach().cpu() for k, p in zip(S.CNAMES, ps)}
    out.update(y=y.detach().cpu(), x=xg.grad.reshape(N * T, -1).cpu(), h0=leaves[0].grad.cpu(), hT=last[0].detach().cpu())
    if not gru:
        out.update(c0=leaves[1].grad.cpu(), cT=last[1].detach().cpu())
    return out


def held(got, ref, yard, mode_, gru, what):
    """the measure: against the restatement of this case, or (toy widths) the yardstick over seeds"""
    assert set(got) == set(ref[F64]), (sorted(got), sorted(ref[F64]))
    if yard is None:
        rep = assert_within(got, ref[F64], ref[F32], is_split(), what=what)
    else:
        rep = G.yardstick_report(got, ref[F64], yard, is_split())
        for k, v in rep.items():
            print(f"{what} {k:7s} norm {v['norm']:.3g} (<= {v['bound_norm']:.3g}) elem {v['elem']:.3g} (<= {v['bound_elem']:.3g}) "
                  f"ratio to the yardstick {v['ratio']:.3g}")
        bad = failures(rep)
        assert not bad, (what, {k: rep[k] for k in bad})
    for k, v in rep.items():
        key = (mode_, "gru" if gru else "lstm", k)
        RATIOS[key] = max(RATIOS.get(key, 0.0), v["ratio"])


# ---- one call with a state on both sides -------------------------------------------------------------------------------------
@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("shape", S.LAYER_CASES, ids=ident)
def test_layer_with_a_state_in_the_loss_matches_float64(shape, act, gru, mode):
    N, T, I, Hh, hdim, combine = shape
    *case, ref = S.layer_reference(shape, gru, act)
    yard = S.yardstick(shape[:5], gru, act, combine) if Hh <= TOY_UNITS else None
    with logged() as seen:
        got = run(case, N, T, gru, act, combine)
    kernel = "stream1_gru_f32" if gru else "stream1_f32"
    assert launches(seen) == [(kernel, "fwd", N, T, Hh), (kernel, "bwd", N, T, Hh)]
    # the projection's, dW_hh's shifted product, the h0 term over the N frame-0 rows, dW_ih (+ bias)
    assert [w[2] for w in seen["wgrads"]] == [N * T, N * T, N, N * T], seen["wgrads"]
    held(got, ref, yard, mode, gru, f"{ident(shape)} {'gru' if gru else 'lstm'} act={act} {mode}")


# ---- chunks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("chunks,detach", [(S.CHUNKINGS[0], False), (S.CHUNKINGS[1], False), (S.CHUNKINGS[2], False),
                                           (S.CHUNKINGS[1], True), (S.CHUNKINGS[2], True)],
                         ids=["23", "1x23", "5-1-17", "1x23-detached", "5-1-17-detached"])
@pytest.mark.parametrize("name", list(S.CHUNK_CASES))
def test_chunks_with_the_state_handed_over(name, chunks, detach, gru, mode):
    N, T, I, Hh, hdim, scale = S.CHUNK_CASES[name]
    *case, ref = S.chunk_reference(name, gru, chunks, detach)
    yard = S.yardstick((N, T, I, Hh, hdim), gru, 1, 0, chunks, detach, scale) if Hh <= TOY_UNITS else None
    with logged() as seen:
        got = run(case, N, T, gru, 1, chunks=chunks, detach=detach)
    kernel = "stream1_gru_f32" if gru else "stream1_f32"
    assert launches(seen) == [(kernel, "fwd", N, n, Hh) for n in chunks] + [(kernel, "bwd", N, n, Hh) for n in reversed(chunks)]
    held(got, ref, yard, mode, gru, f"{name} {'gru' if gru else 'lstm'} {ident(chunks[:3])}{' detached' if detach else ''} {mode}")


@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
@pytest.mark.parametrize("name", list(S.CHUNK_CASES))
def test_sinks_accumulate_the_sum_over_chunks(name, gru, mode):
    """GradBucket sinks on the side stream (`direct`): every chunk's backward adds into the bucket, the h0 term included"""
    N, T, I, Hh, hdim, scale = S.CHUNK_CASES[name]
    chunks = S.CHUNKINGS[2]
    *case, ref = S.chunk_reference(name, gru, chunks, False)
    yard = S.yardstick((N, T, I, Hh, hdim), gru, 1, 0, chunks, False, scale) if Hh <= TOY_UNITS else None
    assert H.OVERLAP_WGRAD
    got = run(case, N, T, gru, 1, chunks=chunks, sinks=True)
    held(got, ref, yard, mode, gru, f"{name} {'gru' if gru else 'lstm'} sinks over chunks {mode}")


# ---- what does not change ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gru", [False, True], ids=["lstm", "gru"])
def test_without_the_flag_and_without_a_differentiated_state_nothing_changes(gru, mode):
    N, T, I, Hh, hdim, combine = S.LAYER_CASES[2]
    x, params, dy, dlast, _ = S.make_case(N, T, I, Hh, hdim, gru, 0)

    def call(**kw):
        rnn, lin = S.modules_of(params, gru, device=DEV)
        xg = x.to(DEV).clone().requires_grad_()
        with logged() as seen:
            y = Fn.rnnp_layer(xg, rnn, lin, N, T, act=1, **kw)
            last = None
            if kw.get("return_state"):
                y, last = y
            y.backward(dy.to(DEV))
            torch.cuda.synchronize()
        return [y.detach(), xg.grad] + [p.grad for p in S.params_of(rnn, lin)], last, (launches(seen), seen["wgrads"])

    plain, _, log = call()
    off, _, log_off = call(state_grad=False)
    assert log_off == log and all(torch.equal(a, b) for a, b in zip(plain, off))
    kept, last, log_kept = call(return_state=True)
    assert not any(s.requires_grad for s in ([last] if gru else last))
    assert log_kept == log and all(torch.equal(a, b) for a, b in zip(plain, kept))
    # the flag on, the state returned into the graph, and nobody differentiates it: the launches of the plain call, its bits
    unused, last, log_unused = call(return_state=True, state_grad=True)
    assert all(s.requires_grad for s in ([last] if gru else last))
    assert log_unused == log and all(torch.equal(a, b) for a, b in zip(plain, unused))
    assert len(log[1]) == 3 and [w[2] for w in log[1]] == [N * T] * 3      # (no product over the frame-0 rows)
    # the refusal that holds without the flag, on device tensors
    rnn, lin = S.modules_of(params, gru, device=DEV)
    z = torch.zeros(N, Hh, device=DEV)
    with pytest.raises(RuntimeError, match="without gradients"):
        Fn.rnnp_layer(x.to(DEV), rnn, lin, N, T, state=z if gru else (z, z), return_state=True)


def test_zz_report():
    """the largest error / (the fp32 restatement's error) per arithmetic, cell and tensor this run saw (pytest -rP)"""
    for (m, cell, k), v in sorted(RATIOS.items()):
        print(f"{m:7s} {cell:5s} {k:7s} {v:.3g}")
