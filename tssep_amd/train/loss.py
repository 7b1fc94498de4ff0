"""Losses -- drop-ins for tssep/train/loss.py on the HIP kernels: ``LogMAE`` (:219-247) and
``VADSigmoidBCE`` (:272-345) with their ``from_ex_out`` glue (:89-99, :118-146), ``MAE`` (:194-216), ``MSE`` (:183-190)
and the joint TS-SEP loss ``SignalAndVADSigmoidBCE`` (:348-424) of an ``explicit_vad`` mask estimator.

``pit=True`` on the time-domain losses (LogMAE, MAE, MSE): the loss of the best speaker permutation per utterance
(pt.ops.losses.pit_loss).  Each of them is f(sum_k C[k, perm(k)]) with f monotone on the pairwise costs
C[i, j] = mean_n |e_i - t_j|^p, so the best permutation is the best assignment on C: one pass over both signals yields
C, the assignment is found on the device (K <= 8), and ``.permutation`` keeps the last call's choice.

The VAD losses take two kinds of target.  ``'Vad'``: the frame activity, given by the reader or derived from the sample
activity ``vad`` (util.utils.stft_vad, host code as in the reference; stft_vad_device is its one-kernel form).  An upper-case signal name such as
``'Speaker_reverberation_early_ch0'`` (loss.py:312-327): a frame is active where the sum of its STFT magnitudes exceeds
``magnitude_threshold`` times the row's largest.  That activity is built on the device too -- from the spectrum ``ex[target]``
when the caller supplies one, otherwise from the signal ``ex[target.lower()]`` by a frame kernel that never writes the
spectrum (STFT.frame_activity) -- and is kept in ``ex`` under a private key; ``ex[target]`` always stays a spectrum.

``FreqMSE`` (:250-269, on ``STFTDomain``, :102-115) compares spectra: sum_k sum_t mean_f |E - S|^2 per utterance, with pit
the best speaker permutation on the K x K costs.  On the training step of a Masking enhancer Model.review forms it from
the logits, the Observation and the target spectrum in one pass each way -- no mask, no estimate, no inverse STFT
(functional.mask_spec_mse); anywhere else it reads ``out.stft_estimate`` (functional.spec_mse; complex128 from TorchBF).

``SDR`` has no counterpart in the reference: the negated mean over speakers of the SI-SDR or SDR in dB, on float64
dot-product sums from one pass over estimate and target, with pit and a soft threshold; usable as
``signal_loss`` of the joint loss, and ``.values`` keeps the last call's dB per speaker.
Not built: FreqMSE as ``signal_loss`` of the joint loss, pit for the VAD losses, K > 8."""
import numpy as np
import torch

from .. import functional as Fn
from ..configurable import Configurable


class ABC(Configurable, torch.nn.Module):
    def __init__(self, target: str = "speaker_reverberation_early_ch0", pit: bool = False):
        super().__init__()
        self.target, self.pit = target, bool(pit)

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
    """estimate, target [B, K, N] (or [K, N]: one utterance, the result squeezed back) -> [B].
    pit=True: the minimum over the speaker permutations, found per utterance; ``permutation`` then holds the last call's
    detached int32 [B, K] (or [K]) tensor, permutation[b, i] = the target row matched to estimate row i, so that
    evaluation code can reorder estimates (``target[b, permutation[b]]`` lines up with ``estimate[b]``).  It stays on the
    device -- no host sync, a captured step recomputes it on every replay -- and is None while pit is false."""
    power, log = 1, False              # the pairwise cost mean_n |e - t|^power; log10 of the matched sum
    permutation = None

    @property
    def fused_tail(self):
        """Whether the fused tail of Model.review may form this loss's |e - t| sums and gradient itself: the L1 losses
        with the targets in their own order only."""
        return self.power == 1 and not self.pit

    def from_ex_out(self, ex, out, model, summary):      # loss.py:90-99
        return self(out.time_estimate, ex[self.target])

    def _pit(self, estimate, target):
        batched = estimate.dim() == 3
        loss, perm = Fn.pair_loss(estimate if batched else estimate[None], target if batched else target[None],
                                  self.power, self.log, True)
        self.permutation = perm.detach() if batched else perm.detach()[0]
        return loss if batched else loss[0]


class LogMAE(TimeDomain):
    log = True

    def loss_fn(self, estimate, target):
        """log10(sum_k mean_n |e - t|) -> [B]  (loss.py:244-247)"""
        if self.pit:
            return self._pit(estimate, target)
        if estimate.dim() == 2:
            return Fn.log_mae(estimate[None], target[None])[0]
        return Fn.log_mae(estimate, target)


class MAE(TimeDomain):
    def loss_fn(self, estimate, target):
        """sum_k mean_n |e - t| -> [B]  (loss.py:194-216)"""
        if self.pit:
            return self._pit(estimate, target)
        if estimate.dim() == 2:
            return Fn.mae(estimate[None], target[None])[0]
        return Fn.mae(estimate, target)


class MSE(TimeDomain):
    power = 2

    def loss_fn(self, estimate, target):
        """sum_k mean_n (e - t)^2  (loss.py:183-190: 0.1673 in its doctest, not the mean over all elements).  Batched
        input gives one value per utterance, [B] -- this project's convention, the same as MAE."""
        if self.pit:
            return self._pit(estimate, target)
        if estimate.dim() == 2:
            return Fn.mse(estimate[None], target[None])[0]
        return Fn.mse(estimate, target)


class SDR(TimeDomain):
    """The negated mean over speakers of the SI-SDR (``scale_invariant=True``) or SDR in dB -- this project's own loss,
    the reference has none.  Per estimate row e and matched target row t, sums over the samples:
    a = sum e^2, b = sum t^2, c = sum e t;  scale-invariant: alpha = c / (b + eps), s = alpha c, n = a - s;  plain: s = b,
    n = max(a - 2 c + b, 0);  value = 10 log10((s + eps) / (n + tau s + eps)), tau = 10^(-sdr_max / 10) (``sdr_max=None``:
    0) the soft threshold that keeps a value below ``sdr_max``.  ``eps`` is an absolute energy (a sum, not a mean).
    ``pit=True`` takes the best assignment on the K x K values; ``.permutation`` as on the other time-domain losses.
    ``.values`` keeps the last call's detached dB per speaker, [B, K] (or [K]), on the device."""
    values = None

    def __init__(self, target: str = "speaker_reverberation_early_ch0", pit: bool = False, scale_invariant: bool = True,
                 sdr_max=None, eps: float = 1e-8):
        super().__init__(target=target, pit=pit)
        if not (isinstance(eps, (int, float)) and np.isfinite(eps) and eps > 0):
            raise ValueError(f"eps must be a positive finite energy, got {eps!r}")
        if sdr_max is not None and not (isinstance(sdr_max, (int, float)) and np.isfinite(sdr_max)):
            raise ValueError(f"sdr_max must be None or a finite level in dB, got {sdr_max!r}")
        self.scale_invariant = bool(scale_invariant)
        self.sdr_max = None if sdr_max is None else float(sdr_max)
        self.eps = float(eps)

    @property
    def fused_tail(self):
        return False

    def loss_fn(self, estimate, target):
        """-(1/K) sum_k value[k, perm(k)] -> [B]"""
        Fn.H._check_pit_k(estimate.shape[-2])
        loss, perm, values = Fn.sdr_loss(estimate, target, self.scale_invariant, self.sdr_max, self.eps, self.pit)
        self.permutation = perm.detach() if self.pit else None
        self.values = values.detach()
        return loss


class STFTDomain(ABC):
    """estimate, target [B, K, T, F] complex (or [K, T, F]: one utterance, the result squeezed back) -> [B].
    pit=True permutes SPEAKERS, per utterance, and ``permutation`` is kept as on TimeDomain.  (The reference's
    ``pit_loss(axis=-2)`` would permute the frames of a [K, T, F] estimate; that reading is not reproduced.)"""
    permutation = None

    def target_spectrum(self, ex, model):
        """ex[target], computed from the signal ``ex[target.lower()]`` when absent (loss.py:111-114) and stored back.
        The reference writes ``self.fe`` there, which no loss has: ``model.fe`` is used, as in LogitsSTFTDomain."""
        assert self.target[0].isupper(), self.target
        if self.target not in ex:
            ex[self.target] = model.fe.stft(ex[self.target.lower()])
        return ex[self.target]

    def from_ex_out(self, ex, out, model, summary):      # loss.py:103-115
        target = self.target_spectrum(ex, model)
        fused = getattr(out, "_spec_loss", None)         # Model.review's fused tail: (loss, permutation, the target it used)
        if fused is not None and fused[2] is target:
            self.permutation = fused[1]
            return fused[0]
        return self(out.stft_estimate, target)


class FreqMSE(STFTDomain):
    def __init__(self, target: str = "Speaker_reverberation_early", pit: bool = False):
        super().__init__(target=target, pit=pit)

    def loss_fn(self, estimate, target):
        """sum_k sum_t mean_f |e - t|^2 -> [B]  (loss.py:258-269: its doctest's 0.1673 is MSE's, the mean over the last
        axis and the sum over the others; the batch axis is kept, this project's convention).  With pit the minimum over
        the speaker permutations."""
        batched = estimate.dim() == 4
        assert estimate.dim() in (3, 4), estimate.shape
        if not isinstance(target, torch.Tensor):
            target = torch.stack(list(target))
        e, t = (estimate, target) if batched else (estimate[None], target[None])
        Fn.H._check_pit_k(e.shape[1])
        if t.dtype != torch.complex64:
            t = t.to(torch.complex64)
        loss, perm = Fn.spec_mse(e, t.to(e.device), self.pit)
        self.permutation = (perm.detach() if batched else perm.detach()[0]) if self.pit else None
        return loss if batched else loss[0]


_ACTIVITY_KEY = "_tssep_amd_frame_activity:"      # ex[_ACTIVITY_KEY + target] = (the tensor it came from, the activity)


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
        if self.target != "Vad":
            return self._bce(estimate, self.frame_activity(ex, model))
        if self.target not in ex:
            from ..util.utils import stft_vad
            ex[self.target] = stft_vad(ex[self.target.lower()], model.fe.window_length,
                                       model.fe.shift, model.fe.fading)
        return self(estimate, ex[self.target])

    def frame_activity(self, ex, model):
        """The frame activity [..., K, T] (float32 of 0 / 1, on the model's device) of a magnitude target
        (loss.py:143-146 + 312-327): from the caller's spectrum ``ex[target]`` when there is one, otherwise from the signal
        ``ex[target.lower()]`` without its spectrum (STFT.frame_activity).  Cached in ``ex`` under a private key, next to the
        tensor it was derived from; ``ex[target]`` is left as it is -- other code reads that key as a spectrum."""
        assert self.target[0].isupper() and self.target != "Vad", self.target
        spectrum = self.target in ex
        src = ex[self.target] if spectrum else ex[self.target.lower()]
        cached = ex.get(_ACTIVITY_KEY + self.target)
        if cached is not None and cached[0] is src:
            return cached[1]
        if not isinstance(src, torch.Tensor):
            src = torch.stack(list(src)) if isinstance(src, (list, tuple)) else torch.as_tensor(src)
        dev = next(model.parameters()).device
        x = src.to(dev)
        act = model.fe.stft_activity(x, self.magnitude_threshold) if spectrum \
            else model.fe.frame_activity(x, self.magnitude_threshold)
        ex[_ACTIVITY_KEY + self.target] = (ex[self.target] if spectrum else ex[self.target.lower()], act)
        return act

    def _target_activity(self, ex, model):
        """What the summaries draw: the activity the loss was computed on."""
        if self.target == "Vad":
            return torch.as_tensor(ex[self.target])
        return self.frame_activity(ex, model)

    def update_summary(self, summary, ex, out, model):   # loss.py:148-169: the mask image framed by the target activity
        import einops
        target_vad = einops.repeat(self._target_activity(ex, model).to(out.mask.device, torch.float32),
                                   "... spk time -> ... spk mask time freq", freq=40, mask=out.mask.shape[-3])
        masks = torch.concat([target_vad, out.mask.detach(), target_vad], dim=-1)
        summary.add_mask_image(f"{model.enhancer.name}_mask", masks,
                               rearrange="... spk mask time freq -> ... time (spk mask freq)", batch_first=True)


class VADSigmoidBCE(LogitsSTFTDomain):
    def __init__(self, target: str = "Vad", pit: bool = False, magnitude_threshold: float = 0.05):
        if pit:
            raise NotImplementedError("pit=True on a VAD loss (only the time-domain losses LogMAE, MAE, MSE take it)")
        super().__init__(target=target, pit=pit)
        assert 0 < magnitude_threshold < 1, magnitude_threshold
        self.magnitude_threshold = magnitude_threshold

    def prepare_target(self, target, dtype=None):        # loss.py:312-327
        """A spectrum [..., T, F] (complex or real) -> the activity [..., T] in ``dtype`` (default: the spectrum's real
        dtype): sum_f |X| / max_t sum_f |X| > magnitude_threshold.  A CUDA tensor goes through the kernels
        (STFT.stft_activity); numpy arrays and CPU tensors -- summaries, tests -- take the reference's formula as it
        stands."""
        if self.target in ["vad", "Vad"]:
            return target
        if dtype is None:
            dtype = target.real.dtype
        if isinstance(target, torch.Tensor):
            if target.is_cuda:
                from .feature_extractor import STFT
                return STFT.stft_activity(target, self.magnitude_threshold).type(dtype)
            target = abs(target).sum(axis=-1)
            target = target / torch.amax(target, dim=-1, keepdim=True)
            return (target > self.magnitude_threshold).type(dtype)
        target = np.abs(target).sum(axis=-1)
        with np.errstate(invalid="ignore"):               # (a silent row: 0 / 0 = NaN compares false, as in torch)
            target = target / np.amax(target, axis=-1, keepdims=True)
            return (target > self.magnitude_threshold).astype(dtype)

    def _bce(self, estimate, activity):
        """estimate [..., K, T, F] (the mean over F is the kernel's), activity [..., K, T] -> mean_{k,t} BCE"""
        assert estimate.shape[:-1] == activity.shape, (estimate.shape, activity.shape)
        activity = activity.to(device=estimate.device, dtype=torch.float32)
        if estimate.dim() == 3:
            return Fn.vad_bce(estimate[None], activity[None])[0]
        return Fn.vad_bce(estimate, activity)

    def forward(self, estimate, target):                 # loss.py:329-345
        if not isinstance(target, torch.Tensor):
            target = torch.stack(target)
        if self.target not in ["vad", "Vad"]:
            assert estimate.shape == target.shape, (estimate.shape, target.shape)
            assert estimate.ndim > 2, estimate.shape
            target = self.prepare_target(target.to(estimate.device), dtype=torch.float32)
        return self._bce(estimate, target)


class SignalAndVADSigmoidBCE(VADSigmoidBCE):
    """loss[b] = mean_{k,t} BCEWithLogits(vad_logit, Vad) + signal_loss[b]  (loss.py:348-395); needs
    ``MaskEstimator_v2(explicit_vad=True)``.  On the fused training step the BCE is computed beside the gated tail
    (``Model.review``) and its gradient is folded into the tail's d(vad_logit) store; anywhere else it runs on the gate
    column of the head's logit rows (``functional.gate_bce``)."""

    def __init__(self, signal_loss: TimeDomain, target: str = "Vad", pit: bool = False,
                 magnitude_threshold: float = 0.05):
        super().__init__(target=target, pit=pit, magnitude_threshold=magnitude_threshold)
        if not target[:1].isupper():
            raise NotImplementedError(f"target {target!r}: the frame-level 'Vad' or an upper-case signal name, whose STFT "
                                      "magnitudes give the activity (loss.py:380-393 asserts the upper case)")
        if not isinstance(signal_loss, TimeDomain):
            raise TypeError(f"signal_loss must be a time-domain loss (LogMAE, MAE, MSE), got {type(signal_loss).__name__}")
        if signal_loss.pit:
            raise NotImplementedError("signal_loss with pit=True: the VAD term compares vad_logit with Vad row by row and "
                                      "would not follow the signal loss's permutation")
        self.signal_loss = signal_loss

    def targets(self, lower=False, upper=False):          # loss.py:363-366
        return super().targets(lower=lower, upper=upper) + self.signal_loss.targets(lower=lower, upper=upper)

    def frame_vad(self, ex, model):
        """ex['Vad'] as a float32 tensor on the logits' device: from the sample activity ``vad`` when absent
        (loss.py:381-391, util/utils.stft_vad) -- stored back, so that every user sees the same tensor.  A magnitude
        target: the cached ``frame_activity`` (the same tensor on every call for the same ``ex``)."""
        if self.target != "Vad":
            if ex.get(self.target) is None and ex.get(self.target.lower()) is None:
                return None
            return self.frame_activity(ex, model)
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
        target = self.frame_vad(ex, model)
        if fused is not None and fused[1] is target:
            return fused[0] + signal_loss
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
        target_vad = einops.repeat(self._target_activity(ex, model).to(out.mask.device, torch.float32),
                                   "... spk time -> ... spk mask time freq", freq=40, mask=out.mask.shape[-3])
        estimate_vad = einops.repeat(out.vad_mask.detach(), "... spk mask time -> ... spk mask time freq", freq=40)
        masks = torch.concat([target_vad, estimate_vad, out.mask.detach(), estimate_vad, target_vad], dim=-1)
        summary.add_mask_image(f"{model.enhancer.name}_mask", masks,
                               rearrange="... spk mask time freq -> ... time (spk mask freq)", batch_first=True)
