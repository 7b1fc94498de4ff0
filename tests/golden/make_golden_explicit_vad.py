"""Fixtures of the explicit_vad feature, generated from the REFERENCE classes (stubbed imports of make_golden.py):

* ``ev_me_{combination}_{ts_vad}_{trials}.npz``: MaskEstimator_v2(explicit_vad=True) (net.py:521-535, 630, 969-979) --
  parameters, inputs, the speaker permutations the forward drew, mask / vad_mask / vad_logit and the parameter
  gradients of sum(mask g) + sum(vad_mask gv).  (Not ``me_*``: that prefix is the grid of the ungated estimator.)
* ``ev_loss.npz``: SignalAndVADSigmoidBCE(signal_loss=LogMAE()) (loss.py:348-395) through its from_ex_out.

Run from the repository root with the reference checkout at the path make_golden.py names:
    python tests/golden/make_golden_explicit_vad.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import _stub_imports, npz  # noqa: E402

CASES = [("mul", 4, 1), ("mul", 4, 2), ("mul", False, 1), ("cat", 4, 1), ("cat", 4, 2), ("cat", False, 1)]
B, T, D, F, E_cat = 2, 7, 12, 9, 4


def main():
    _stub_imports()
    from tssep.train import net, loss

    for case, (comb, ts_vad, nap) in enumerate(CASES):
        K = ts_vad if ts_vad else 3
        E = F if comb == "mul" else E_cat
        np.random.seed(300 + case)
        torch.manual_seed(300 + case)
        me = net.MaskEstimator_v2(
            idim=D, odim=F, layers=3, units=5, projs=6, dropout=0, nmask=1, pre_net="RNNP", aux_net=None,
            aux_net_output_size=E, combination=comb, ts_vad=ts_vad, output_resolution="tf",
            random_speaker_order=True, num_averaged_permutations=nap, explicit_vad=True)
        xs = torch.randn(B, T, D)
        aux = torch.rand(B, K, E)
        g = torch.randn(B, K, 1, T, F)
        gv = torch.randn(B, K, 1, T)
        rng_state = np.random.get_state()
        out = me(xs, [[a for a in ab] for ab in aux])
        assert out.logit is None
        np.random.set_state(rng_state)
        perm = np.stack([np.random.permutation(K) for _ in range(B)])
        me.zero_grad()
        ((out.mask * g).sum() + (out.vad_mask * gv).sum()).backward()
        arrs = {"p." + k: v for k, v in me.state_dict().items()}
        arrs.update({"dp." + k: v.grad for k, v in me.named_parameters()})
        arrs.update(xs=xs, aux=aux, g=g, gv=gv, perm=perm, mask=out.mask, vad_mask=out.vad_mask,
                    vad_logit=out.vad_logit, embedding=out.embedding, seed=np.array(300 + case),
                    cfg=np.array([comb, str(ts_vad), "tf", str(nap)]))
        npz(f"ev_me_{comb}_{ts_vad}_{nap}", **arrs)

    # SignalAndVADSigmoidBCE(signal_loss=LogMAE()) through from_ex_out (loss.py:368-395)
    torch.manual_seed(7)
    K, N = 3, 400
    vad_logit = torch.randn(B, K, 1, T) * 3
    Vad = (torch.rand(B, K, T) > 0.5).float()
    e, t = torch.randn(B, K, N), torch.randn(B, K, N)
    lo = loss.SignalAndVADSigmoidBCE(signal_loss=loss.LogMAE(pit=False))
    out = types.SimpleNamespace(vad_logit=vad_logit, time_estimate=e)
    ex = {"Vad": Vad, "speaker_reverberation_early_ch0": t}
    value = lo.from_ex_out(ex, out, None, None)
    npz("ev_loss", vad_logit=vad_logit, Vad=Vad, e=e, t=t, loss=value,
        signal=loss.LogMAE(pit=False)(e, t), targets=np.array(lo.targets()),
        targets_lower=np.array(lo.targets(lower=True)))


if __name__ == "__main__":
    main()
