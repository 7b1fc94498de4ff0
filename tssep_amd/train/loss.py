"""Losses -- drop-ins for tssep/train/loss.py on the HIP kernels: ``LogMAE`` (:219-247) and
``VADSigmoidBCE`` (:272-345) with their ``from_ex_out`` glue (:89-99, :118-146), ``MAE`` (:194-216) and the joint
TS-SEP loss ``SignalAndVADSigmoidBCE`` (:348-424) of an ``explicit_vad`` mask estimator.
MSE / FreqMSE are not selected by any shipped config."""
import torch

from .. import functional as Fn
from ..configurable import Configurable


class ABC(Configurable, torch.nn.Module):
    def __init__(self, target: str = "speaker_reverberation_early_ch0", pit: bool = False):
        super().__init__()
        if pit:
            raise NotImplementedError("pit=True (every shipped config uses pit: false)")
        self.target, self.pit = target, pit

    def _upper(self, s):
        return s[0].upper() + s[1:]

    def targets(self, lower=False, upper=False):         # loss.py:30-40
        if lower:
            assert not upper
            return tuple(t.lower() for t in self.targets())
        if upper:
            return tuple(self._upper(t) for t in self.targets())
        return (self.target,)

    @property
    def name(self):
        return self.__class__.__name__

    def forward(self, estimate, target):
        assert estimate.shape == target.shape, (estimate.shape, target.shape)
        return self.loss_fn(estimate, target)

    def update_summary(self, summary, ex, out, model):
        pass


class TimeDomain(ABC):
    def from_ex_out(self, ex, out, model, summary):      # loss.py:90-99
        return self(out.time_estimate, ex[self.target])


class LogMAE(TimeDomain):
    def loss_fn(self, estimate, target):
        """log10(sum_k mean_n |e - t|) -> [B]  (loss.py:244-247)"""
        if estimate.dim() == 2:
            return Fn.log_mae(estimate[None], target[None])[0]
        return Fn.log_mae(estimate, target)


class MAE(TimeDomain):
    def loss_fn(self, estimate, target):
        """sum_k mean_n |e - t| -> [B]  (loss.py:194-216)"""
        if estimate.dim() == 2:
            return Fn.mae(estimate[None], target[None])[0]
        return Fn.mae(estimate, target)


class LogitsSTFTDomain(ABC):
    def from_ex_out(self, ex, out, model, summary):      # loss.py:122-146
        if out.logit is None:
            raise ValueError(
                f"{self.name} reads out.logit, which an explicit_vad mask estimator does not produce (net.py:969-979); "
                "train it with SignalAndVADSigmoidBCE(signal_loss=...), whose VAD term reads out.vad_logit")
        if out.logit.shape[-3] != 1:
            raise ValueError(f"{self.name} on a logit with {out.logit.shape[-3]} masks per speaker {tuple(out.logit.shape)}: "
                             "the squeeze of the mask axis (loss.py:122-146) is a no-op then; use nmask=1")
        estimate = torch.squeeze(out.logit, dim=-3)
        assert self.target[0].isupper(), self.target
        if self.target not in ex:
            if self.target == "Vad":
                from ..util.utils import stft_vad
                ex[self.target] = stft_vad(ex[self.target.lower()], model.fe.window_length,
                                           model.fe.shift, model.fe.fading)
            else:
                raise NotImplementedError(self.target)
        return self(estimate, ex[self.target])

    def update_summary(self, summary, ex, out, model):   # loss.py:148-169: the mask image framed by the target activity
        import einops
        target_vad = einops.repeat(self.prepare_target(torch.as_tensor(ex[self.target])).to(out.mask.device, torch.float32),
                                   "... spk time -> ... spk mask time freq", freq=40, mask=out.mask.shape[-3])
        masks = torch.concat([target_vad, out.mask.detach(), target_vad], dim=-1)
        summary.add_mask_image(f"{model.enhancer.name}_mask", masks,
                               rearrange="... spk mask time freq -> ... time (spk mask freq)", batch_first=True)


class VADSigmoidBCE(LogitsSTFTDomain):
    def __init__(self, target: str = "Vad", pit: bool = False, magnitude_threshold: float = 0.05):
        super().__init__(target=target, pit=pit)
        assert 0 < magnitude_threshold < 1, magnitude_threshold
        self.magnitude_threshold = magnitude_threshold

    def prepare_target(self, target, dtype=None):
        if self.target in ["vad", "Vad"]:
            return target
        raise NotImplementedError("STFT-magnitude VAD targets (loss.py:316-327) are off the hot path")

    def forward(self, estimate, target):                 # loss.py:329-345
        if not isinstance(target, torch.Tensor):
            target = torch.stack(target)
        if self.target not in ["vad", "Vad"]:
            raise NotImplementedError(self.target)
        target = target.to(device=estimate.device, dtype=torch.float32)
        if estimate.dim() == 3:
            return Fn.vad_bce(estimate[None], target[None])[0]
        return Fn.vad_bce(estimate, target)


class SignalAndVADSigmoidBCE(VADSigmoidBCE):
    """loss[b] = mean_{k,t} BCEWithLogits(vad_logit, Vad) + signal_loss[b]  (loss.py:348-395); needs
    ``MaskEstimator_v2(explicit_vad=True)``.  On the fused training step the BCE is computed beside the gated tail
    (``Model.review``) and its gradient is folded into the tail's d(vad_logit) store; anywhere else it runs on the gate
    column of the head's logit rows (``functional.gate_bce``)."""

    def __init__(self, signal_loss: TimeDomain, target: str = "Vad", pit: bool = False,
                 magnitude_threshold: float = 0.05):
        super().__init__(target=target, pit=pit, magnitude_threshold=magnitude_threshold)
        if target != "Vad":
            raise NotImplementedError(f"target {target!r}: only the frame-level 'Vad' target (loss.py:384-393)")
        if not isinstance(signal_loss, TimeDomain):
            raise TypeError(f"signal_loss must be a time-domain loss (LogMAE, MAE), got {type(signal_loss).__name__}")
        self.signal_loss = signal_loss

    def targets(self, lower=False, upper=False):          # loss.py:363-366
        return super().targets(lower=lower, upper=upper) + self.signal_loss.targets(lower=lower, upper=upper)

    def frame_vad(self, ex, model):
        """ex['Vad'] as a float32 tensor on the logits' device: from the sample activity ``vad`` when absent
        (loss.py:381-391, util/utils.stft_vad) -- stored back, so that every user sees the same tensor."""
        v = ex.get(self.target)
        if v is None:
            if ex.get(self.target.lower()) is None:
                return None
            from ..util.utils import stft_vad
            v = stft_vad(ex[self.target.lower()], model.fe.window_length, model.fe.shift, model.fe.fading)
        if not isinstance(v, torch.Tensor):
            v = torch.stack(list(v)) if isinstance(v, (list, tuple)) else torch.as_tensor(v)
        dev = next(model.parameters()).device
        if v.device != dev or v.dtype != torch.float32:
            v = v.to(device=dev, dtype=torch.float32)
        ex[self.target] = v
        return v

    def from_ex_out(self, ex, out, model, summary):       # loss.py:368-395
        signal_loss = self.signal_loss.from_ex_out(ex, out, model, summary)
        fused = getattr(out, "_gate_bce", None)
        if fused is not None and fused[1] is ex.get(self.target):
            return fused[0] + signal_loss
        target = self.frame_vad(ex, model)
        gated = getattr(out, "_gated", None)
        if gated is not None:
            if target.dim() == 2:
                target = target[None]
            bce = Fn.gate_bce(gated, target)
            if out.vad_logit.dim() == 2:                 # (an unbatched example)
                bce = bce[0]
        else:
            # any other producer of vad_logit [..., K, 1, T]: the VADSigmoidBCE of loss.py:379 on it
            bce = self(torch.squeeze(out.vad_logit[..., None], dim=-3).contiguous(), target)
        return bce + signal_loss

    def update_summary(self, summary, ex, out, model):    # loss.py:397-424
        import einops
        target_vad = einops.repeat(self.prepare_target(torch.as_tensor(ex[self.target])).to(out.mask.device, torch.float32),
                                   "... spk time -> ... spk mask time freq", freq=40, mask=out.mask.shape[-3])
        estimate_vad = einops.repeat(out.vad_mask.detach(), "... spk mask time -> ... spk mask time freq", freq=40)
        masks = torch.concat([target_vad, estimate_vad, out.mask.detach(), estimate_vad, target_vad], dim=-1)
        summary.add_mask_image(f"{model.enhancer.name}_mask", masks,
                               rearrange="... spk mask time freq -> ... time (spk mask freq)", batch_first=True)
