"""explicit_vad on a real MI355X: the gated kernels (stft.hip, maskhead.hip, elementwise.hip) against float64 torch, the
gated fused tail against the materialised chain, MaskEstimator_v2(explicit_vad=True) against fixtures of the reference
class, the model end to end against the oracle composition, reproducibility, hipGraph replay and the VAD2Sep start."""
import glob
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import features as ofeat, loss as oloss, net as onet, stft as ostft  # noqa: E402
from test_gpu_kernels import close  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EV_CASES = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "ev_me_*.npz")))
T_ = torch.as_tensor
F = 513


@pytest.fixture(params=["f32", "bf16x3"])
def gemm_mode(request):
    from tssep_amd import hip_ops
    old = hip_ops.GEMM_PRECISION
    hip_ops.GEMM_PRECISION = request.param
    yield request.param
    hip_ops.GEMM_PRECISION = old


def _inputs(B, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    T = ostft.num_frames(N)
    logit = (torch.randn(B, K, T, F + 1, generator=g) * 2).cuda()
    obs = torch.complex(torch.randn(B, T, F, generator=g), torch.randn(B, T, F, generator=g)).cuda()
    tgt = (torch.randn(B, K, N, generator=g) * 0.5).cuda()
    vad = (torch.rand(B, K, T, generator=g) > 0.5).float().cuda()
    return logit, obs, tgt, vad, T


def _ref_tail(logit, obs, N):
    """float64 torch: mask = sigmoid(l) sigmoid(v), est = obs mask, y = istft(est) (oracle.stft.istft)."""
    l64 = _d(logit).requires_grad_()
    gate = torch.sigmoid(l64[..., 0])
    mask = torch.sigmoid(l64[..., 1:]) * gate[..., None]
    est = obs.detach().cpu().to(torch.complex128)[:, None] * mask
    y = ostft.istft(est, size=1024, shift=256, window="hann", num_samples=N)
    return l64, mask, gate, est, y


def _d(t):
    """the float64 reference runs on the host (the oracle's STFT is CPU code)"""
    return t.detach().cpu().double()


def _tail_scale(t):
    return float(t.detach().abs().max())


# (small; T = 253 with B K = 64 frames rows -- more frames than one grid wave of the backward; T = 1878, 30 s)
SIZES = [(1, 2, 6000), (8, 8, 64000), (1, 2, 480000)]


@pytest.mark.parametrize("B,K,N", SIZES)
def test_gated_fused_tail_against_float64(B, K, N):
    from tssep_amd import functional as Fn, hip_ops as H
    logit, obs, tgt, vad, T = _inputs(B, K, N, seed=B * 1000 + K)
    _, wsyn = Fn.windows("hann", 1024, 256, logit.device)
    l64, mask, gate, est, y64 = _ref_tail(logit, obs, N)
    y, part = H.mask_istft_fwd(logit, obs, wsyn, N, tgt=tgt)
    close(y, y64, rtol=1e-4, atol=2e-6 * _tail_scale(y64), name="y")
    sums64 = (y64.detach() - _d(tgt)).abs().sum(-1)
    close(part.view(B, K, -1).sum(-1), sums64, rtol=1e-4, atol=1e-6, name="|y - tgt| sums")
    # plain backward: dy given
    dy = torch.randn(B, K, N, generator=torch.Generator().manual_seed(5)).cuda()
    (dl64,) = torch.autograd.grad(y64, l64, _d(dy), retain_graph=True)
    dl = H.mask_istft_bwd(dy, logit, obs, wsyn)
    sc = _tail_scale(dl64)
    close(dl[..., 1:], dl64[..., 1:], rtol=1e-3, atol=1e-5 * sc, name="d(mask logits)")
    close(dl[..., 0], dl64[..., 0], rtol=1e-3, atol=1e-5 * _tail_scale(dl64[..., 0]), name="d(vad logit)")
    # the loss-folded backward: LogMAE (gout) + the gate column's BCE (gbce), bt_major store through iperm
    gout = torch.rand(B).cuda() + 0.5
    gbce = torch.rand(B).cuda() + 0.5
    yl = y.detach().clone()
    loss64 = (torch.log10((_d(yl) - _d(tgt)).abs().mean(-1).sum(-1)) * _d(gout)).sum()
    # sign(est - tgt) is taken at the float32 estimate, as the kernel does: the float64 chain reads y's float32 value
    ysub = y64 + (_d(yl) - y64).detach()
    bce = torch.nn.functional.binary_cross_entropy_with_logits(l64[..., 0], _d(vad), reduction="none").mean((-1, -2))
    loss64 = (torch.log10((ysub - _d(tgt)).abs().mean(-1).sum(-1)) * _d(gout)).sum() + (bce * _d(gbce)).sum()
    (dl64,) = torch.autograd.grad(loss64, l64)
    _, sums = H.logmae_fwd(yl, tgt)
    perm = torch.stack([torch.randperm(K, generator=torch.Generator().manual_seed(b)) for b in range(B)]).int().cuda()
    iperm = torch.argsort(perm, dim=-1).int()
    d = H.mask_istft_bwd(None, logit, obs, wsyn, loss=(yl, tgt, sums, gout), vad=(vad, gbce), iperm=iperm,
                         bt_major=True)
    assert tuple(d.shape) == (B * T, K * (F + 1))
    d = d.view(B, T, K, F + 1)
    got = torch.stack([d[b][:, iperm[b].long()] for b in range(B)]).permute(0, 2, 1, 3)     # -> [B, K, T, F + 1]
    close(got[..., 1:], dl64[..., 1:], rtol=1e-3, atol=1e-5 * _tail_scale(dl64[..., 1:]), name="folded d(mask logits)")
    close(got[..., 0], dl64[..., 0], rtol=1e-3, atol=1e-5 * _tail_scale(dl64[..., 0]), name="folded d(vad logit)")
    # the same fold into the [B, K, T, F + 1] layout equals the bt_major one bit for bit
    d2 = H.mask_istft_bwd(None, logit, obs, wsyn, loss=(yl, tgt, sums, gout), vad=(vad, gbce))
    assert torch.equal(d2, got)
    # deterministic: the in-wave reduction of d(v) is a fixed order
    assert torch.equal(H.mask_istft_bwd(dy, logit, obs, wsyn), dl)


@pytest.mark.parametrize("B,K,N", SIZES[:2])
def test_gated_mask_head_and_gate_bce_against_float64(B, K, N):
    from tssep_amd import hip_ops as H
    logit, obs, tgt, vad, T = _inputs(B, K, N, seed=7 + B)
    l64, mask64, gate64, est64, _ = _ref_tail(logit, obs, N)
    mask, est, vmask = H.maskhead_gated_fwd(logit, obs)
    close(mask, mask64, rtol=1e-5, atol=1e-6, name="mask")
    close(vmask, gate64, rtol=1e-5, atol=1e-6, name="vad_mask")
    close(torch.view_as_real(est), torch.view_as_real(est64), rtol=1e-5, atol=1e-5, name="est")
    gen = torch.Generator().manual_seed(11)
    dest = torch.complex(torch.randn(B, K, T, F, generator=gen), torch.randn(B, K, T, F, generator=gen)).cuda()
    dmask = torch.randn(B, K, T, F, generator=gen).cuda()
    dvm = torch.randn(B, K, T, generator=gen).cuda()
    s = (torch.view_as_real(est64) * torch.view_as_real(dest.cpu().to(torch.complex128))).sum() + \
        (mask64 * _d(dmask)).sum() + (gate64 * _d(dvm)).sum()
    (dl64,) = torch.autograd.grad(s, l64)
    dl = H.maskhead_gated_bwd(dest, dmask, dvm, logit, obs)
    close(dl[..., 1:], dl64[..., 1:], rtol=1e-4, atol=1e-6 * _tail_scale(dl64), name="d(mask logits)")
    close(dl[..., 0], dl64[..., 0], rtol=1e-4, atol=1e-6 * _tail_scale(dl64[..., 0]), name="d(vad logit)")
    # gate BCE on the strided column
    l64b = _d(logit).requires_grad_()
    bce64 = torch.nn.functional.binary_cross_entropy_with_logits(l64b[..., 0], _d(vad), reduction="none").mean((-1, -2))
    close(H.gatebce_fwd(logit, vad), bce64, rtol=1e-5, atol=1e-6, name="bce")
    gout = torch.rand(B).cuda() + 0.5
    (dbce64,) = torch.autograd.grad((bce64 * _d(gout)).sum(), l64b)
    close(H.gatebce_bwd(logit, vad, gout), dbce64, rtol=1e-5, atol=1e-9, name="d bce")


def _model(K=4, units=12, projs=10, loss_name="joint", ts_vad=4, random_speaker_order=True, seed=4):
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss, model, net
    torch.manual_seed(seed)
    lo = loss.SignalAndVADSigmoidBCE(signal_loss=loss.LogMAE()) if loss_name == "joint" else loss.LogMAE()
    return model.Model(
        fe=fe.ConcaternatedSTFTFeatures(
            fe.TorchMFCC(size=1024, shift=256, window="hann", output_size=40),
            fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), size=1024, shift=256, window="hann"),
        reader=DummyReader(),
        mask_estimator=net.MaskEstimator_v2(idim=553, odim=513, units=units, projs=projs, combination="mul",
                                            aux_net_output_size=513, ts_vad=ts_vad, output_resolution="tf",
                                            random_speaker_order=random_speaker_order, explicit_vad=True),
        enhancer=enhancer.Masking(), loss=lo).cuda()


def _batch(B, K, N, seed):
    rng = np.random.RandomState(seed)
    tgt = 0.1 * rng.randn(B, K, N).astype(np.float32)
    vad = np.zeros((B, K, N), dtype=np.float32)
    for k in range(K):
        vad[:, k, k * N // (K + 1):(k + 2) * N // (K + 1)] = 1
    tgt *= vad
    T = ostft.num_frames(N)
    Vad = T_(vad)[..., ::256][..., :T]
    Vad = torch.nn.functional.pad(Vad, (0, T - Vad.shape[-1]))
    obs = tgt.sum(1, keepdims=True) + 0.05 * rng.rand(B, 1, N).astype(np.float32)
    aux = rng.rand(B, K, 513).astype(np.float32)
    return dict(observation=T_(obs).cuda(), auxInput=T_(aux).cuda(), reference_channel=0,
                speaker_reverberation_early_ch0=T_(tgt).cuda(), Vad=Vad.cuda(), dataset=["e"] * B)


def test_fused_gated_tail_equals_materialised_chain():
    """Model.review on an untouched explicit_vad ForwardOutput runs the gated fused tail with the BCE folded into its
    backward; touching out.mask first takes the unfused gated mask head -> istft -> LogMAE + gate BCE.  Same loss, same
    time estimate, same gradients."""
    m = _model(random_speaker_order=False)
    B, K, N = 2, 4, 7000
    ex0 = _batch(B, K, N, seed=3)
    res = {}
    for mode in ("fused", "materialised"):
        m.zero_grad()
        ex = dict(ex0)
        out = m(ex)
        assert out.logit is None and tuple(out.vad_logit.shape) == (B, K, 1, ex["Observation"].shape[-2])
        if mode == "materialised":
            assert tuple(out.mask.shape) == (B, K, 1, ex["Observation"].shape[-2], 513)
            assert tuple(out.vad_mask.shape) == (B, K, 1, ex["Observation"].shape[-2])
        s_ = m.review(ex, out)
        s_["loss"].backward()
        if mode == "fused":
            assert not out.materialised and getattr(out, "_gate_bce", None) is not None
        res[mode] = (s_["loss"].detach(), out.time_estimate.detach(),
                     {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
    (lf, tf_, gf), (lm, tm, gm) = res["fused"], res["materialised"]
    close(lf, lm, rtol=1e-5, atol=1e-6, name="loss")
    close(tf_, tm, rtol=1e-4, atol=1e-6, name="time_estimate")
    assert set(gf) == set(gm) and len(gf) > 10
    for k in gf:
        close(gf[k], gm[k], rtol=1e-3, atol=1e-4 * float(gm[k].abs().max()) + 1e-9, name="d" + k)


@pytest.mark.parametrize("name", EV_CASES)
def test_mask_estimator_against_reference_fixture(golden, name, gemm_mode):
    from tssep_amd.train.net import MaskEstimator_v2
    a = 1 if gemm_mode == "f32" else 10
    g = golden(name)
    comb, ts_vad, res, nap = [str(s) for s in g["cfg"]]
    ts_vad = False if ts_vad == "False" else int(ts_vad)
    E = g["aux"].shape[-1]
    me = MaskEstimator_v2(idim=12, odim=9, layers=3, units=5, projs=6, combination=comb, aux_net_output_size=E,
                          ts_vad=ts_vad, output_resolution=res, num_averaged_permutations=int(nap), explicit_vad=True)
    sd = {k[2:]: T_(v) for k, v in g.items() if k.startswith("p.")}
    me.load_state_dict(sd, strict=True)
    me.cuda()
    np.random.seed(int(g["seed"]))             # the stream the reference forward consumed
    aux = T_(g["aux"]).cuda()
    out = me(T_(g["xs"]).cuda(), [[x for x in ab] for ab in aux])
    assert out.logit is None
    close(out.vad_logit, g["vad_logit"], rtol=1e-3, atol=5e-6 * a, name="vad_logit")
    close(out.vad_mask, g["vad_mask"], rtol=1e-3, atol=2e-6 * a, name="vad_mask")
    close(out.mask, g["mask"], rtol=1e-3, atol=2e-6 * a, name="mask")
    close(out.embedding, g["embedding"], name="embedding")
    ((out.mask * T_(g["g"]).cuda()).sum() + (out.vad_mask * T_(g["gv"]).cuda()).sum()).backward()
    for k, p in me.named_parameters():
        close(p.grad, g["dp." + k], rtol=2e-3, atol=5e-6 * a, name="d" + k)


def _oracle_joint(p, obs, aux, tgt, Vad, K, perm):
    """STFT -> features -> oracle mask estimator with F + 1 columns -> gate -> masking -> istft -> LogMAE + BCE."""
    X = ostft.stft(obs, size=1024, shift=256, window="hann")
    fb, dct = ofeat.mfcc_tables(1024)
    inp = ofeat.concat_features(X[..., 0, :, :], fb, dct).to(torch.float32)
    out = onet.mask_estimator_forward(p, inp, aux, odim=514, combination="mul", ts_vad=K, output_resolution="tf",
                                      perm=perm, fast=True)
    logit = out["logit"]
    v = logit[..., 0]
    mask = torch.sigmoid(logit[..., 1:]) * torch.sigmoid(v)[..., None]
    est = oloss.masking(mask, X, 0)
    y = ostft.istft(est, size=1024, shift=256, window="hann", num_samples=obs.shape[-1])
    loss = oloss.vad_sigmoid_bce(torch.squeeze(v[..., None], dim=-3), Vad) + oloss.log_mae(y, tgt)
    return dict(mask=mask, vad_logit=v, time_estimate=y, loss=loss)


def test_model_end_to_end_against_oracle(gemm_mode):
    m = _model(units=12, projs=16)
    B, K, N = 2, 4, 6000
    ex0 = _batch(B, K, N, seed=0)
    p = {"mask_estimator." + k: v.detach().cpu().clone().requires_grad_()
         for k, v in m.mask_estimator.state_dict().items()}
    np.random.seed(3)
    perm = np.stack([np.random.permutation(K) for _ in range(B)])
    o = _oracle_joint(p, ex0["observation"].cpu(), ex0["auxInput"].cpu(), ex0["speaker_reverberation_early_ch0"].cpu(),
                      ex0["Vad"].cpu(), K, perm)
    o["loss"].sum().backward()
    ex = dict(ex0)
    np.random.seed(3)
    out = m(ex)
    summary = m.review(ex, out)
    close(out.time_estimate, o["time_estimate"], rtol=1e-3, atol=1e-5, name="time_estimate")
    close(summary["loss"], o["loss"].sum(), rtol=1e-4, atol=1e-6, name="loss")
    summary["loss"].backward()
    close(out.vad_logit, o["vad_logit"], rtol=1e-3, atol=2e-5, name="vad_logit")
    close(out.mask, o["mask"], rtol=1e-3, atol=1e-5, name="mask")
    for k, v in m.mask_estimator.named_parameters():
        ref = p["mask_estimator." + k].grad
        close(v.grad, ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max()) + 1e-9, name="d" + k)


def test_step_is_bitwise_reproducible():
    from tssep_amd import hip_ops
    m = _model(units=24, projs=24)
    ex0 = _batch(3, 4, 20000, seed=9)
    runs = []
    for _ in range(2):
        m.zero_grad()
        np.random.seed(11)
        ex = dict(ex0)
        out = m(ex)
        m.review(ex, out)["loss"].backward()
        torch.cuda.synchronize()
        hip_ops.check_cluster_errors()
        runs.append((out.time_estimate.detach().clone(), [p.grad.clone() for p in m.parameters() if p.grad is not None]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))


def test_trainer_graph_step_is_bit_identical_to_the_eager_trainer(tmp_path):
    from tssep_amd.train import runtime
    from tssep_amd.train.optimizer import Adam
    from tssep_amd.train.trainer import Trainer
    data = [_batch(2, 4, 5000 if i % 2 else 7300, seed=31 + i) for i in range(4)]
    for ex in data:
        ex["dataset"] = ["tg"] * 2

    class Dataset(list):
        def __iter__(self):
            return (dict(ex) for ex in list.__iter__(self))

    runs = {}
    for mode in ("off", "on"):
        with runtime.applied(graph_step=mode):
            np.random.seed(77)
            tr = Trainer(_model(units=24, projs=24, seed=21), tmp_path / mode, Adam(gradient_clipping=10.0, lr=1e-3),
                         summary_trigger=(1, "iteration"), checkpoint_trigger=(1000, "iteration"),
                         stop_trigger=(8, "iteration"), virtual_minibatch_size=2)
            hist = tr.train(Dataset(data), device=0)
            torch.cuda.synchronize()
            h = json.loads((tmp_path / mode / "log" / "history.json").read_text())
            runs[mode] = ([l for _, l in hist], tr.optimizer.flat_param.clone(), h)
    l_off, p_off, _ = runs["off"]
    l_on, p_on, h_on = runs["on"]
    assert len(l_off) == 8 and all(np.isfinite(l_off))
    assert h_on.get("graph_replays", 0) >= 5, h_on
    assert l_on == l_off, [(i, a, b) for i, (a, b) in enumerate(zip(l_on, l_off)) if a != b]
    assert torch.equal(p_on, p_off), float((p_on - p_off).abs().max())


def test_vad2sep_initial_gate_equals_tsvad_logit(tmp_path):
    """InitCheckPointVAD2Sep from a TS-VAD model ('t' resolution): at initialisation the explicit_vad model's gate -- and
    every mask logit -- equal the TS-VAD logit (the head's rows are repeated F + 1 times per speaker)."""
    from tssep_amd.train import net
    from tssep_amd.train.init_ckpt import InitCheckPointVAD2Sep
    K = 4
    kw = dict(idim=553, odim=513, units=12, projs=16, combination="mul", aux_net_output_size=513, ts_vad=K,
              random_speaker_order=False)
    torch.manual_seed(5)
    vadm = net.MaskEstimator_v2(output_resolution="t", **kw)
    sepm = net.MaskEstimator_v2(output_resolution="tf", explicit_vad=True, **kw)
    hv, hs = torch.nn.Module(), torch.nn.Module()
    hv.mask_estimator, hs.mask_estimator = vadm, sepm
    ck = tmp_path / "vad.pth"
    torch.save({"model": hv.state_dict()}, ck)

    class EG:
        class trainer:
            model = hs
    InitCheckPointVAD2Sep(init_ckpt=str(ck)).load_model_state_dict(EG, ck)
    vadm.cuda(), sepm.cuda()
    xs = torch.rand(2, 30, 553).cuda()
    aux = torch.rand(2, K, 513).cuda()
    with torch.no_grad():
        lv = vadm(xs, aux).logit[..., 0, :, 0]                  # [B, K, T] ('t': repeated over frequency)
        lg, _ = sepm.logits(xs, aux)                            # [B, K, T, 514]
        out = sepm(xs, aux)
    close(out.vad_logit[..., 0, :], lv, rtol=1e-4, atol=1e-5, name="gate")
    close(lg[..., 1:], lv[..., None].expand_as(lg[..., 1:]), rtol=1e-4, atol=1e-5, name="mask logits")


def test_toy_tsvad_to_explicit_vad_tssep_chain(tmp_path):
    """The toy TS-VAD -> explicit-VAD TS-SEP chain (tssep_amd/exp, toy_tssep_explicit_vad.yaml): a TS-VAD checkpoint
    initialises the explicit_vad model, which trains a few iterations with finite joint losses."""
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")

    def toy(*yamls, overrides=()):
        cfg = run.build_config([os.path.join(exp, y) for y in yamls] + list(overrides))
        return Experiment.from_config(cfg["eg"])
    vad = toy("toy_common.yaml", "toy_tsvad.yaml", overrides=[f"eg.trainer.storage_dir={tmp_path / 'v'}"])
    ck = tmp_path / "vad.pth"
    torch.save({"model": vad.trainer.model.state_dict()}, ck)
    sep = toy("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_explicit_vad.yaml",
              overrides=[f"eg.trainer.storage_dir={tmp_path / 's'}", f"eg.init_ckpt.init_ckpt={ck}",
                         "eg.trainer.stop_trigger=[3,iteration]"])
    sep.init_ckpt(sep)
    m = sep.trainer.model.cuda()
    ds = m.prepare_train_dataset(torch.device("cuda"), batch_size=1, prefetch=False)
    losses = []
    for i, ex in enumerate(ds):
        if i == 3:
            break
        m.zero_grad()
        out = m(ex)
        summary = m.review(ex, out)
        summary["loss"].backward()
        losses.append(float(summary["loss"]))
    assert len(losses) == 3 and all(np.isfinite(losses)), losses
