"""CPU checks of pit=True on the loss modules: what constructs, what is refused (and where), the targets, the routing
switch Model.review reads, and the toy overlay."""
import os

import pytest
import torch

from tssep_amd.train import loss

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")


@pytest.mark.parametrize("cls,power,log", [(loss.LogMAE, 1, True), (loss.MAE, 1, False), (loss.MSE, 2, False)])
def test_time_domain_losses_take_pit(cls, power, log):
    for pit in (False, True):
        lo = cls(pit=pit)
        assert lo.pit is pit and (lo.power, lo.log) == (power, log) and isinstance(lo, loss.TimeDomain)
        assert lo.permutation is None
        assert lo.targets() == ("speaker_reverberation_early_ch0",)
        assert lo.targets(lower=True) == ("speaker_reverberation_early_ch0",)
        assert lo.targets(upper=True) == ("Speaker_reverberation_early_ch0",)
        assert cls(target="x", pit=pit).targets() == ("x",)
        # the fused tail forms the loss only for an L1 loss on the targets' own order
        assert lo.fused_tail is (power == 1 and not pit)
    assert cls().pit is False and cls().name == cls.__name__


def test_vad_losses_refuse_pit():
    with pytest.raises(NotImplementedError, match="pit"):
        loss.VADSigmoidBCE(pit=True)
    with pytest.raises(NotImplementedError, match="pit"):
        loss.SignalAndVADSigmoidBCE(signal_loss=loss.LogMAE(), pit=True)
    for cls in (loss.LogMAE, loss.MAE, loss.MSE):
        with pytest.raises(NotImplementedError, match="permutation"):       # the VAD term would not follow it
            loss.SignalAndVADSigmoidBCE(signal_loss=cls(pit=True))
    lo = loss.SignalAndVADSigmoidBCE(signal_loss=loss.MSE(target="x"))
    assert lo.targets() == ("Vad", "x") and not lo.signal_loss.fused_tail
    assert loss.VADSigmoidBCE().targets() == ("Vad",) and loss.VADSigmoidBCE().pit is False


def test_more_than_eight_speakers_are_refused_before_any_launch():
    """K = 9 raises in Python, on CPU tensors: no kernel, no library call."""
    e = torch.zeros(2, 9, 16)
    for lo in (loss.LogMAE(pit=True), loss.MAE(pit=True), loss.MSE(pit=True), loss.MSE()):
        with pytest.raises(NotImplementedError, match="8"):
            lo(e, e)
        with pytest.raises(NotImplementedError, match="8"):
            lo(e[0], e[0])
    with pytest.raises(AssertionError):
        loss.MSE(pit=True)(torch.zeros(2, 3, 16), torch.zeros(2, 3, 15))


def test_toy_overlay_resolves(tmp_path):
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_pit.yaml")]
                           + [f"eg.trainer.storage_dir={tmp_path}"])
    m = Experiment.from_config(cfg["eg"]).trainer.model
    assert isinstance(m.loss, loss.LogMAE) and m.loss.pit is True and not m.loss.fused_tail
    assert m.loss.targets() == ("speaker_reverberation_early_ch0",)
    plain = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml")]
                             + [f"eg.trainer.storage_dir={tmp_path}"])
    lo = Experiment.from_config(plain["eg"]).trainer.model.loss
    assert lo.pit is False and lo.fused_tail
