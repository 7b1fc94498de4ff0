"""Learned speaker embeddings on a real MI355X (csrc/aux.hip, functional._Cond / _InstNorm / _Affine / _AuxMLP,
train/net.py Linear / AuxNet / InstanceNorm / InstanceNorm_v2): every kernel stage against a float64 host reference with
a bound derived from its summation order, the modules and MaskEstimator_v2 against tests/aux_reference.py + the oracle."""
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aux_reference as R  # noqa: E402
from oracle import model as omodel, net as onet  # noqa: E402
from test_gpu_kernels import close  # noqa: E402

U = 2.0 ** -24
EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
T_ = torch.as_tensor


@pytest.fixture(params=["f32", "bf16x3"])
def gemm_mode(request):
    from tssep_amd import hip_ops
    old = hip_ops.GEMM_PRECISION
    hip_ops.GEMM_PRECISION = request.param
    yield request.param
    hip_ops.GEMM_PRECISION = old


def _padded(a, dense=False):
    """float32 [rows, C] array -> (device buffer view [rows, C], ld): rows padded to a multiple of 4 floats (zeros) or,
    dense, packed with ld = C (not 16-byte addressable when C is odd: the kernels' 4-byte path)."""
    rows, C = a.shape
    ld = C if dense else (C + 3) // 4 * 4
    buf = torch.zeros(rows, ld, dtype=torch.float32)
    buf[:, :C] = T_(a)
    buf = buf.cuda()
    return buf, ld


# ------------------------------------------------------------------------------------------------------ d_aux
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("combination", ["mul", "cat"])
@pytest.mark.parametrize("shape", [(1, 3, 1, 5, 9, 4), (2, 3, 2, 67, 513, 7), (2, 4, 2, 300, 513, 100),
                                   (2, 3, 3, 130, 64, 12)])
def test_cond_aux_bwd_stage(shape, combination, dense):
    """d_aux[b,s,c] = sum_tr sum_t dxs[(b,tr,(s-tr) mod K,t), c0+c] (* pre[(b,t), c] for mul) against float64.
    Order of the kernel: a wave adds its frames t0+w, t0+w+4, ... of a 64-frame chunk, trial after trial, into one
    accumulator -- at most trials * min(16, ceil(T/4)) additions -- wave 0 adds the four waves (3), the second launch
    adds the ceil(T/64) chunks (chunks - 1): d = trials * min(16, ceil(T/4)) + 3 + chunks - 1 <= trials * T, and with
    the product's rounding and the first term the componentwise bound is (d + 2) 2^-24 sum|terms|.
    (2,4,2,300,513,E=100): five chunks, odd F, pad columns, a cat window that starts off a 16-byte boundary;
    (…,64,…): F % 4 == 0; dense: leading dimensions that force the 4-byte path.  Two runs are bit-identical.
    Worst error / bound on an MI355X: 0.196 (the 5-frame shape), <= 0.031 for the others."""
    from tssep_amd import hip_ops as H
    B, K, trials, T, F, E = shape
    mul = combination == "mul"
    W, C = (F, F) if mul else (F + E, E)
    rng = np.random.RandomState(5)
    dxs = rng.randn(B * trials * K * T, W).astype(np.float32)
    pre = (rng.randn(B * T, F) + 0.5).astype(np.float32)
    dv, ld = _padded(dxs, dense)
    pv, ldp = _padded(pre, dense)
    args = (dv, ld, pv if mul else None, ldp if mul else 0, B, K, T, F, E, trials, combination)
    got = H.cond_aux_bwd(*args)
    again = H.cond_aux_bwd(*args)
    assert got.shape == (B, K, C) and torch.equal(got, again)
    d5 = T_(dxs).double().view(B, trials, K, T, W)[..., (0 if mul else F):(0 if mul else F) + C]
    p3 = T_(pre).double().view(B, 1, T, F)
    want, mag = torch.zeros(B, K, C, dtype=torch.float64), torch.zeros(B, K, C, dtype=torch.float64)
    for s in range(K):
        for tr in range(trials):
            terms = d5[:, tr, (s - tr) % K] * (p3[:, 0] if mul else 1.0)
            want[:, s] += terms.sum(1)
            mag[:, s] += terms.abs().sum(1)
    d = trials * min(16, -(-T // 4)) + 3 + (-(-T // 64) - 1)
    assert d <= max(trials * T, 4)
    err = (got.cpu().double() - want).abs()
    ratio = float((err / ((d + 2) * U * mag)).max())
    print(f"cond_aux_bwd {shape} {combination} dense={dense}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


# ---------------------------------------------------------------------------------------------- instance norm
def _instnorm_input(R_, n, C, axis, seed):
    """No constant rows; sequence 0 has |mean| / std ~ 200 (the reference docstring's `randn * 0.5 + 100`)."""
    rng = np.random.RandomState(seed)
    x = rng.randn(R_, n, C)
    x[0] = x[0] * 0.5 + 100.0
    if R_ > 1:
        x[1] = x[1] * 5 - 5
    if (C if axis == 0 else n) == 1:
        raise AssertionError("a single value has no variance")
    return x.astype(np.float32)


INSTNORM_CASES = [(0, n, C) for n in (1, 67, 316) for C in (5, 100, 513, 553)] + \
                 [(1, n, C) for n in (67, 316) for C in (5, 100, 513, 553)]


@pytest.mark.parametrize("mode,unbiased", [(0, False), (0, True), (1, False)])
def test_instnorm_fwd_bwd_stage(mode, unbiased):
    """Both modes, both axes, C in {5, 100, 513, 553}, n in {1 (row-wise only), 67, 316}, one sequence with
    |mean| / std ~ 200 (an uncentred variance E[x^2] - mean^2 loses every digit there), against float64.
    Forward, per element, N the reduction length, c = 4 (log2 N + 4):  |y - y64| <= c 2^-24 (|y| + (|x| + |mean|) / std).
    Backward dx = r (dy - a - yhat b), a = mean(dy), b = sum(dy yhat) / dof, computed from the fp32 x, mean, r = 1 / std:
      e_y  = c 2^-24 (|yhat| + (|x| + |mean|) / std)      error of the recomputed yhat (the forward bound)
      rel_r = c 2^-24 (1 + (max|x| + |mean|) / std)       relative error of r: d(ss) <= 2 sum |x - mean| e + c u ss
      |dx - dx64| <= c 2^-24 r (|dy| + mean|dy| + |yhat| sum|dy yhat| / dof)        the three reduction terms
                     + r (e_y |b| + |yhat| sum(|dy| e_y) / dof)                        yhat's error through b
                     + rel_r (|dx64| + 2 r |yhat| |b|)                                 r's error (b carries r twice)
    The kernels accumulate the statistics in double and round once (a chain of fp32 additions put the mean's error at
    1.01 of this bound for one element near zero of a zero-mean row, n = 67, C = 553).  Worst error / bound over all cases on
    an MI355X: forward 0.059, backward 0.028 (mode 0: 0.052 / 0.022, unbiased 0.055 / 0.025; mode 1: 0.059 / 0.028)."""
    from tssep_amd import hip_ops as H
    worst_f = worst_b = 0.0
    for axis, n, C in INSTNORM_CASES:
        R_ = 3
        x = _instnorm_input(R_, n, C, axis, seed=n * 1000 + C)
        dy = np.random.RandomState(C + n).randn(R_, n, C).astype(np.float32)
        xd = T_(x).cuda()
        y, mean, rscale, xinfo = H.instnorm_fwd(xd, axis, mode, unbiased)
        dx = H.instnorm_bwd(T_(dy).cuda(), xinfo, mean, rscale, tuple(xd.shape), axis, mode, unbiased)
        dim = -1 if axis == 0 else -2
        N = C if axis == 0 else n
        x64 = T_(x).double().requires_grad_()
        y64 = R.instance_norm(x64, dim, unbiased) if mode == 0 else R.instance_norm_v2(x64, dim, dim)
        (y64 * T_(dy).double()).sum().backward()
        with torch.no_grad():
            m64 = x64.mean(dim, keepdim=True)
            ss = ((x64 - m64) ** 2).sum(dim, keepdim=True)
            s64 = (ss / (N - 1 if (mode == 0 and unbiased) else N)).sqrt()
            c = 4 * (math.log2(N) + 4)
            e_y = c * U * (y64.abs() + (x64.abs() + m64.abs()) / s64)
            ratio_f = float(((y.cpu().double() - y64).abs() / e_y).max())
            dof = N - 1 if (mode == 0 and unbiased) else N
            g = T_(dy).double()
            r = 1.0 / s64
            b = (g * y64).sum(dim, keepdim=True) / dof
            rel_r = c * U * (1 + (x64.abs().amax(dim, keepdim=True) + m64.abs()) / s64)
            bound = c * U * r * (g.abs() + g.abs().mean(dim, keepdim=True)
                                 + y64.abs() * (g * y64).abs().sum(dim, keepdim=True) / dof) \
                + r * (e_y * b.abs() + y64.abs() * (g.abs() * e_y).sum(dim, keepdim=True) / dof) \
                + rel_r * (x64.grad.abs() + 2 * r * y64.abs() * b.abs())
            ratio_b = float(((dx.cpu().double() - x64.grad).abs() / bound).max())
            close(mean.cpu().view(m64.shape), m64.float(), rtol=1e-5, atol=1e-6, name="mean")
            close(rscale.cpu().view(s64.shape), (1 / s64).float(), rtol=1e-3, atol=0, name="rscale")
        print(f"instnorm mode={mode} unbiased={unbiased} axis={axis} n={n} C={C}: fwd {ratio_f:.3f} bwd {ratio_b:.3f}")
        worst_f, worst_b = max(worst_f, ratio_f), max(worst_b, ratio_b)
        assert ratio_f <= 1.0 and ratio_b <= 1.0, (axis, n, C, ratio_f, ratio_b)
    print(f"instnorm mode={mode} unbiased={unbiased}: worst fwd {worst_f:.3f} bwd {worst_b:.3f}")


# --------------------------------------------------------------------------------------- ReLU and segment mean
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C", [10, 513])
def test_relu_and_segment_mean_stage(C, relu):
    """Lengths [1, 63, 64, 65, 300] (below, at and above the 16- and 64-row phases), C = 10 and 513, fused and unfused.
    ReLU forward / backward are exact.  Mean: wave w, accumulator u add the rows w + 4 u (mod 16) -- ceil(len / 16)
    additions -- the four accumulators (2), the four waves (3), one division: (d + 2) 2^-24 sum|terms| / len with
    d = ceil(len / 16) + 5.  Backward: dout / len is one correctly rounded division, exact up to 2^-24 |dout / len|, and the
    fused mask is exact."""
    from tssep_amd import hip_ops as H
    lengths = [1, 63, 64, 65, 300]
    N, S = sum(lengths), len(lengths)
    rng = np.random.RandomState(C)
    h = rng.randn(N, C).astype(np.float32)
    hv, ld = _padded(h)
    row0 = H.segment_rows(lengths, "cuda")
    assert row0.dtype == torch.int64 and row0.tolist() == [0, 1, 64, 128, 193, 493]
    # ReLU kernels
    yv = H.relu_fwd(hv.clone(), ld, N, C)
    assert torch.equal(yv[:, :C].cpu(), T_(h).clamp(min=0))
    g = rng.randn(N, C).astype(np.float32)
    gv, ldg = _padded(g)
    dxr, ldr = H.relu_bwd(gv, ldg, yv, ld, N, C)
    assert torch.equal(dxr[:, :C].cpu(), T_(g) * (T_(h) > 0))
    # segment mean
    out, ldo = H.segment_mean_fwd(hv, ld, row0, S, C, relu=relu)
    again, _ = H.segment_mean_fwd(hv, ld, row0, S, C, relu=relu)
    assert torch.equal(out, again)
    h64 = T_(h).double().clamp(min=0) if relu else T_(h).double()
    dout = rng.randn(S, C).astype(np.float32)
    dv, ldd = _padded(dout)
    dh, ldh = H.segment_mean_bwd(dv, ldd, hv if relu else None, ld, row0, S, N, C, relu=relu)
    a = 0
    for s, n in enumerate(lengths):
        seg = h64[a:a + n]
        d = -(-n // 16) + 5
        bound = (d + 2) * U * seg.abs().sum(0) / n
        err = (out[s, :C].cpu().double() - seg.mean(0)).abs()
        assert bool((err <= bound).all()), (s, n, float((err / bound.clamp(min=1e-300)).max()))
        want = (T_(dout[s]).double() / n)[None].expand(n, C)
        if relu:
            want = want * (T_(h[a:a + n]) > 0)
        errb = (dh[a:a + n, :C].cpu().double() - want).abs()
        assert bool((errb <= U * want.abs()).all()), (s, n)
        a += n


# ------------------------------------------------------------------------------------------------- modules
def _bars(gemm_mode):
    return 1 if gemm_mode == "f32" else 10


@pytest.mark.parametrize("idim,odim,bias", [(7, 9, True), (100, 513, True), (100, 64, False)])
def test_linear_module_against_reference(idim, odim, bias, gemm_mode):
    from tssep_amd.train import net
    a = _bars(gemm_mode)
    torch.manual_seed(1)
    m = net.Linear(idim, odim, bias=bias).cuda()
    rng = np.random.RandomState(2)
    x = rng.randn(2, 3, idim).astype(np.float32)
    g = rng.randn(2, 3, odim).astype(np.float32)
    y = m([[T_(v).cuda() for v in xb] for xb in x], None, batched=True)      # the reference's lists of lists
    assert y.shape == (2, 3, odim)
    (y * T_(g).cuda()).sum().backward()
    p = [q.detach().cpu().double().requires_grad_() for q in m.net.parameters()]
    y64 = R.linear(T_(x).double(), *p)
    (y64 * T_(g).double()).sum().backward()
    close(y, y64.float(), rtol=1e-3, atol=5e-6 * a, name="y")
    for q, q64, name in zip(m.net.parameters(), p, ("weight", "bias")):
        close(q.grad, q64.grad.float(), rtol=2e-3, atol=5e-6 * a, name="d" + name)


@pytest.mark.parametrize("idim", [9, 100])
@pytest.mark.parametrize("norm", [False, True])
def test_auxnet_module_against_reference(idim, norm, gemm_mode):
    """Ragged enrolment lengths, with and without InstanceNorm(-1): outputs and the gradients of all three layers.
    Without a normalizer the reference is the PADDED form; with one, the packed form (the reference's own padded rows
    turn into nan there, aux_reference.auxnet_padded)."""
    from tssep_amd.train import net
    a = _bars(gemm_mode)
    torch.manual_seed(3)
    m = net.AuxNet(idim, normalizer=net.InstanceNorm(-1) if norm else None).cuda()
    rng = np.random.RandomState(4)
    lens = [[5, 17, 1], [64, 33, 9]]
    seqs = [[(rng.randn(n, idim) * 0.7 + 0.2).astype(np.float32) for n in lb] for lb in lens]
    g = rng.randn(2, 3, idim).astype(np.float32)
    y = m([[T_(s).cuda() for s in sb] for sb in seqs], None, batched=True)
    assert y.shape == (2, 3, idim)
    (y * T_(g).cuda()).sum().backward()
    lin = [q for q in m.net if isinstance(q, torch.nn.Linear)]
    p = [q.detach().cpu().double().requires_grad_() for l in lin for q in (l.weight, l.bias)]
    flat = [T_(s).double() for sb in seqs for s in sb]
    y64 = (R.auxnet_packed(flat, p, lambda v: R.instance_norm(v, -1)) if norm else R.auxnet_padded(flat, p)).view(2, 3, idim)
    (y64 * T_(g).double()).sum().backward()
    close(y, y64.float(), rtol=1e-3, atol=5e-6 * a, name="y")
    got = [q for l in lin for q in (l.weight, l.bias)]
    for i, (q, q64) in enumerate(zip(got, p)):
        close(q.grad, q64.grad.float(), rtol=2e-3, atol=5e-6 * a, name=f"dparam{i}")


# ----------------------------------------------------------------------------------- MaskEstimator_v2 end to end
@pytest.mark.parametrize("nap", [1, 2])
@pytest.mark.parametrize("combination", ["mul", "cat"])
@pytest.mark.parametrize("kind", ["linear", "auxnet", "auxnorm"])
def test_mask_estimator_end_to_end(kind, combination, nap, gemm_mode):
    """idim 12, odim 9, units 5, projs 6, K = 3: masks, embedding and EVERY parameter gradient (aux_net.* included)
    against float64 -- oracle.net.mask_estimator_forward fed with the reference-processed embedding and input
    (aux_reference), so the embedding's gradient chains through the reference aux_net / normalizer.  `linear` also
    carries an input_normalizer; `auxnorm` (no aux_net) checks the gradient of the raw embedding itself."""
    from tssep_amd.train import net
    a = _bars(gemm_mode)
    B, K, T, idim, odim = 2, 3, 7, 12, 9
    mul = combination == "mul"
    rng = np.random.RandomState(11)
    torch.manual_seed(12)
    kw = dict(idim=idim, odim=odim, layers=3, units=5, projs=6, combination=combination,
              ts_vad=K if nap > 1 else False, num_averaged_permutations=nap)
    xs = rng.randn(B, T, idim).astype(np.float32)
    if kind == "linear":
        E = odim if mul else 4
        me = net.MaskEstimator_v2(aux_net=net.Linear(7, E), aux_net_output_size=E,
                                  input_normalizer=net.InstanceNorm(dim=-2), **kw).cuda()
        raw = rng.randn(B, K, 7).astype(np.float32)
        aux_in = T_(raw).cuda()
    elif kind == "auxnet":
        E = odim
        me = net.MaskEstimator_v2(aux_net=net.AuxNet(odim), aux_net_output_size=E, **kw).cuda()
        lens = [[4, 9, 1], [6, 2, 11]]
        raw = [[rng.randn(n, odim).astype(np.float32) for n in lb] for lb in lens]
        aux_in = [[T_(s).cuda() for s in sb] for sb in raw]
    else:
        E = odim if mul else 5
        me = net.MaskEstimator_v2(aux_net_output_size=E, aux_normalizer=net.InstanceNorm_v2(), **kw).cuda()
        raw = (rng.randn(B, K, E) + 1.0).astype(np.float32)
        aux_in = T_(raw).cuda().requires_grad_()
    p = {k: v.detach().cpu().double().requires_grad_() for k, v in me.state_dict().items()}
    x64 = T_(xs).double()
    raw64 = None
    if kind == "linear":
        emb = R.linear(T_(raw).double(), p["aux_net.net.weight"], p["aux_net.net.bias"])
        x64 = R.instance_norm(x64, -2)
    elif kind == "auxnet":
        emb = R.auxnet_padded([T_(s).double() for sb in raw for s in sb],
                              [p[f"aux_net.net.{i}.{n}"] for i in (0, 2, 4) for n in ("weight", "bias")]).view(B, K, E)
    else:
        raw64 = T_(raw).double().requires_grad_()
        emb = R.instance_norm_v2(raw64)
    np.random.seed(21)
    o = onet.mask_estimator_forward(p, x64, emb, odim=odim, combination=combination, ts_vad=kw["ts_vad"],
                                    num_averaged_permutations=nap, prefix="")
    gm = rng.randn(*o["mask"].shape).astype(np.float32)
    (o["mask"] * T_(gm).double()).sum().backward()
    np.random.seed(21)
    out = me(T_(xs).cuda(), aux_in)
    close(out.mask, o["mask"].float(), rtol=1e-3, atol=2e-6 * a, name="mask")
    close(out.logit, o["logit"].float(), rtol=1e-3, atol=5e-6 * a, name="logit")
    close(out.embedding, o["embedding"].float(), rtol=1e-3, atol=5e-6 * a, name="embedding")
    (out.mask * T_(gm).cuda()).sum().backward()
    names = [k for k, _ in me.named_parameters()]
    assert (kind == "auxnorm") == (not any(k.startswith("aux_net.") for k in names))
    for k, q in me.named_parameters():
        assert q.grad is not None, k
        close(q.grad, p[k].grad.float(), rtol=2e-3, atol=5e-6 * a, name="d" + k)
    if raw64 is not None:
        close(aux_in.grad, raw64.grad.float(), rtol=2e-3, atol=5e-6 * a, name="d aux")


# ---------------------------------------------------------------------------------------- Model step, toy overlay
def _toy_model(units=12, projs=16, K=4, input_norm=False, seed=0):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net
    torch.manual_seed(seed)
    return model.Model(
        fe=fe.ConcaternatedSTFTFeatures(
            fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=units, projs=projs, combination="mul",
                                            aux_net=net.Linear(100, 513), aux_net_output_size=513, ts_vad=K,
                                            output_resolution="tf",
                                            input_normalizer=net.InstanceNorm(dim=-2) if input_norm else None),
        enhancer=enhancer.Masking(), loss=loss.LogMAE())


def _toy_batch(B, K, N, seed):
    rng = np.random.RandomState(seed)
    tgt = (rng.randn(B, K, N) * 0.1).astype(np.float32)
    obs = tgt.sum(1, keepdims=True) + 0.05 * rng.rand(B, 1, N).astype(np.float32)
    return T_(obs), T_(rng.rand(B, K, 100).astype(np.float32)), T_(tgt)


def test_model_step_with_linear_aux_net_against_oracle(gemm_mode):
    """The toy overlay's model (aux_net: Linear 100 -> 513, mul) through Model.forward + review + backward against the CPU
    oracle fed with the reference-processed embedding (bars of test_model_end_to_end_against_oracle); the gradient of
    aux_net.* chains through the oracle.  The step is bitwise reproducible."""
    B, K, N = 2, 4, 6000
    obs, aux, tgt = _toy_batch(B, K, N, 0)
    m = _toy_model().cuda()
    p = {"mask_estimator." + k: v.detach().cpu().clone().requires_grad_() for k, v in m.mask_estimator.state_dict().items()}
    emb = R.linear(aux, p["mask_estimator.aux_net.net.weight"], p["mask_estimator.aux_net.net.bias"])
    cfg = dict(odim=513, combination="mul", ts_vad=K, output_resolution="tf")
    np.random.seed(3)
    o = omodel.forward_loss(p, obs, emb, tgt, cfg=cfg, loss="LogMAE", fast=True)
    o["loss"].sum().backward()

    def step():
        m.zero_grad(set_to_none=True)
        ex = dict(observation=obs.cuda(), auxInput=aux.cuda(), reference_channel=0,
                  speaker_reverberation_early_ch0=tgt.cuda(), dataset=["v"] * B)
        np.random.seed(3)
        out = m(ex)
        summary = m.review(ex, out)
        summary["loss"].backward()
        torch.cuda.synchronize()
        return out, summary["loss"].detach().clone(), {k: v.grad.clone() for k, v in m.mask_estimator.named_parameters()}

    out, loss1, g1 = step()
    close(out.logit, o["logit"], rtol=1e-3, atol=2e-5, name="logit")
    close(out.mask, o["mask"], rtol=1e-3, atol=1e-5, name="mask")
    close(loss1, o["loss"].sum(), rtol=1e-4, atol=1e-6, name="loss")
    assert "aux_net.net.weight" in g1
    for k, v in g1.items():
        ref = p["mask_estimator." + k].grad
        close(v, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()) + 1e-9, name="d" + k)
    _, loss2, g2 = step()
    assert torch.equal(loss1, loss2) and all(torch.equal(g1[k], g2[k]) for k in g1)


def test_trainer_graph_step_bit_identical_with_linear_aux_net(tmp_path):
    """aux_net: Linear plus an input_normalizer are tensor-in, fixed-shape work: GraphedStep captures them, and 8
    iterations through graphs give the losses and parameters of the eager trainer bit for bit (graph_replays >= 5)."""
    from tssep_amd.train import runtime
    from tssep_amd.train.optimizer import Adam
    from tssep_amd.train.trainer import Trainer
    data = []
    for i in range(4):
        obs, aux, tgt = _toy_batch(2, 4, 5000, 40 + i)
        data.append(dict(observation=obs.cuda(), auxInput=aux.cuda(), speaker_reverberation_early_ch0=tgt.cuda(),
                         reference_channel=0, dataset=["tg"] * 2))

    class Dataset(list):
        def __iter__(self):
            return (dict(ex) for ex in list.__iter__(self))

    runs = {}
    for mode in ("off", "on"):
        with runtime.applied(graph_step=mode):
            np.random.seed(77)
            tr = Trainer(_toy_model(units=24, projs=24, input_norm=True, seed=21), tmp_path / mode,
                         Adam(gradient_clipping=10.0, lr=1e-3), summary_trigger=(1, "iteration"),
                         checkpoint_trigger=(1000, "iteration"), stop_trigger=(8, "iteration"), virtual_minibatch_size=2)
            hist = tr.train(Dataset(data), device=0)
            torch.cuda.synchronize()
            hist_file = json.loads((tmp_path / mode / "log" / "history.json").read_text())
            names = [n for n, _ in tr.model.named_parameters()]
            runs[mode] = ([l for _, l in hist], tr.optimizer.flat_param.clone(), hist_file, names)
    l_off, p_off, h_off, names = runs["off"]
    l_on, p_on, h_on, _ = runs["on"]
    assert "mask_estimator.aux_net.net.weight" in names
    assert len(l_off) == 8 and all(np.isfinite(l_off)) and len(set(l_off)) > 4
    assert "graph_replays" not in h_off and h_on["graph_replays"] >= 5, h_on
    assert l_on == l_off, [(i, x, y) for i, (x, y) in enumerate(zip(l_on, l_off)) if x != y]
    assert torch.equal(p_on, p_off), float((p_on - p_off).abs().max())
    # the new parameters live in the flat bucket like every other parameter, and they moved
    m0 = _toy_model(units=24, projs=24, input_norm=True, seed=21)
    total = sum(q.numel() for q in m0.parameters())
    assert p_off.numel() >= total
    w = tr.model.mask_estimator.aux_net.net.weight
    assert getattr(w, "_tssep_grad_sinks", None), "aux_net.net.weight is outside the flat gradient bucket"
    assert not torch.equal(w.detach().cpu(), m0.mask_estimator.aux_net.net.weight)


@pytest.mark.parametrize("overlay", ["toy_tssep_auxnet.yaml", "toy_tssep_auxnorm.yaml"])
def test_toy_experiment_with_the_overlays(overlay, tmp_path):
    """Both overlays through the existing toy runner (a TS-VAD checkpoint of the same overlay, then run_tssep)."""
    from tssep_amd.exp import run_tssep
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tsvad.yaml", overlay)]
                           + [f"eg.trainer.storage_dir={tmp_path / 'v'}"])
    ck = tmp_path / "vad.pth"
    torch.save({"model": Experiment.from_config(cfg["eg"]).trainer.model.state_dict()}, ck)
    fast = ["eg.trainer.stop_trigger=[3,iteration]", "eg.trainer.checkpoint_trigger=[3,iteration]",
            "eg.trainer.summary_trigger=[1,iteration]"]
    sep_dir = run_tssep.main(configs=tuple(os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", overlay)),
                             storage_dir=tmp_path / "tssep", checkpoint=ck, overrides=fast)
    hist = json.loads((sep_dir / "log" / "history.json").read_text())
    assert hist["iteration"] == 3 and len(hist["loss"]) == 3 and all(np.isfinite(l) for _, l in hist["loss"])
    sd = torch.load(sep_dir / "checkpoints" / "ckpt_latest.pth", map_location="cpu")
    has_aux = any(k.startswith("mask_estimator.aux_net.") for k in sd["model"])
    assert has_aux == (overlay == "toy_tssep_auxnet.yaml")


# ------------------------------------------------------------------------------ nothing changed for existing users
def test_default_model_makes_none_of_the_new_calls(monkeypatch):
    """Every new hip_ops wrapper raises; a forward + backward of the default toy model (no aux_net, no normalizers, a
    fixed embedding) still runs: its launches are what they were."""
    from tssep_amd import hip_ops as H
    from tssep_amd.train import net

    def refuse(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called on the default path")
        return f
    for name in ("cond_aux_bwd", "instnorm_fwd", "instnorm_bwd", "relu_fwd", "relu_bwd", "segment_rows",
                 "segment_mean_fwd", "segment_mean_bwd"):
        assert callable(getattr(H, name))
        monkeypatch.setattr(H, name, refuse(name))
    torch.manual_seed(0)
    for comb in ("mul", "cat"):
        me = net.MaskEstimator_v2(idim=553, odim=513, units=40, projs=42, combination=comb,
                                  aux_net_output_size=513 if comb == "mul" else 100, ts_vad=8,
                                  num_averaged_permutations=2).cuda()
        xs = torch.randn(1, 20, 553, device="cuda")
        aux = torch.rand(1, 8, 513 if comb == "mul" else 100, device="cuda")
        out = me(xs, aux)
        out.mask.sum().backward()
        assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in me.parameters())
