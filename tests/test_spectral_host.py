"""CPU checks of FreqMSE / STFTDomain on the loss modules: the constructor and its defaults, the targets, the config
round trip, the toy overlay, what is refused before any launch, and the host-only size queries of the kernels."""
import os

import pytest
import torch

from tssep_amd import _lib, configurable
from tssep_amd.train import loss

EXP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")


def test_constructor_targets_and_name():
    lo = loss.FreqMSE()
    assert isinstance(lo, loss.STFTDomain) and not isinstance(lo, loss.TimeDomain)
    assert (lo.target, lo.pit, lo.name, lo.permutation) == ("Speaker_reverberation_early", False, "FreqMSE", None)
    assert lo.targets() == ("Speaker_reverberation_early",)
    assert lo.targets(lower=True) == ("speaker_reverberation_early",)
    assert lo.targets(upper=True) == ("Speaker_reverberation_early",)
    lo = loss.FreqMSE(target="Speaker_reverberation_early_ch0", pit=True)
    assert lo.pit is True and lo.targets(lower=True) == ("speaker_reverberation_early_ch0",)
    assert loss.FreqMSE(target="x").targets(upper=True) == ("X",)


def test_config_round_trip_and_resolve():
    assert configurable.resolve("tssep.train.loss.FreqMSE") is loss.FreqMSE
    assert configurable.factory_path(loss.FreqMSE) == "tssep.train.loss.FreqMSE"
    cfg = loss.FreqMSE.get_config({"pit": True})
    assert cfg == {"factory": "tssep.train.loss.FreqMSE", "target": "Speaker_reverberation_early", "pit": True}
    lo = loss.FreqMSE.from_config(cfg)
    assert isinstance(lo, loss.FreqMSE) and lo.pit is True
    assert loss.FreqMSE.get_config() == dict(cfg, pit=False)


def test_toy_overlay_resolves(tmp_path):
    from tssep_amd.train import run
    from tssep_amd.train.experiment import Experiment
    cfg = run.build_config([os.path.join(EXP, y) for y in ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_freqmse.yaml")]
                           + [f"eg.trainer.storage_dir={tmp_path}"])
    m = Experiment.from_config(cfg["eg"]).trainer.model
    assert isinstance(m.loss, loss.FreqMSE) and m.loss.pit is False
    assert m.loss.targets() == ("Speaker_reverberation_early_ch0",)
    assert m.loss.targets(lower=True) == ("speaker_reverberation_early_ch0",)


def test_joint_loss_still_refuses_a_spectral_signal_loss():
    with pytest.raises(TypeError, match="time-domain"):
        loss.SignalAndVADSigmoidBCE(signal_loss=loss.FreqMSE())


@pytest.mark.parametrize("pit", [False, True])
def test_refusals_on_cpu_tensors_before_any_launch(pit):
    lo = loss.FreqMSE(pit=pit)
    e = torch.zeros(2, 9, 3, 5, dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match="8"):                # K = 9
        lo(e, e)
    with pytest.raises(NotImplementedError, match="8"):
        lo(e[0], e[0])
    with pytest.raises(AssertionError):                                # shapes must match exactly
        lo(torch.zeros(2, 3, 4, 5, dtype=torch.complex64), torch.zeros(2, 3, 4, 6, dtype=torch.complex64))

    class Out:
        stft_estimate = torch.zeros(2, 3, 4, 5, dtype=torch.complex64)
    with pytest.raises(AssertionError):                                # a lower-case target names a signal, not a spectrum
        loss.FreqMSE(target="speaker_reverberation_early_ch0", pit=pit).from_ex_out(
            {"speaker_reverberation_early_ch0": torch.zeros(2, 3, 100)}, Out(), None, None)


def test_functional_refuses_nine_speakers_before_any_launch():
    from tssep_amd import functional as Fn
    e = torch.zeros(1, 9, 2, 3, dtype=torch.complex64)
    with pytest.raises(NotImplementedError, match="8"):
        Fn.spec_mse(e, e, pit=True)
    with pytest.raises(NotImplementedError, match="8"):
        Fn.mask_spec_mse(torch.zeros(1, 9, 2, 3), torch.zeros(1, 2, 3, dtype=torch.complex64), e)


def test_size_queries_are_host_only():
    L = _lib.lib()
    assert L.tssep_specmse_chunks(0) == 0 and L.tssep_specmse_chunks(1) == 1
    ct = 2 ** 20 // L.tssep_specmse_chunks(2 ** 20)                    # frames per chunk
    assert ct >= 1
    for T in (1, ct, ct + 1, 253, 1878):
        assert L.tssep_specmse_chunks(T) == -(-T // ct)
    for B, K, T, F in ((1, 1, 1, 1), (2, 3, 9, 513), (8, 8, 253, 513), (768, 8, 253, 513), (3, 8, 2, 5)):
        n = L.tssep_specmse_workspace_bytes(B, K, T, F)
        assert n % 16 == 0 and n >= 4 * B * L.tssep_specmse_chunks(T) * K * K > 0
    for shape in ((1, 9, 4, 5), (0, 2, 4, 5), (1, 0, 4, 5), (1, 2, 0, 5), (1, 2, 4, 0)):
        assert L.tssep_specmse_workspace_bytes(*shape) == 0, shape
