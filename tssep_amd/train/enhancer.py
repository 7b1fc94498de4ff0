"""Enhancers -- drop-in for tssep/train/enhancer.py:21-590: the training-time classes (Dummy,
Nothing, Masking), the eval-time mask-based MVDR beamformer TorchBF and the
segment-wise ClassicBF_np('mvdr_souden') with its WPE / ChannelWiseWPE dereverberation stages."""
import numpy as np
import torch

from .. import functional as Fn, hip_ops as H
from ..configurable import Configurable
from . import enhancer_distortion_mask


class ABC(Configurable):
    @property
    def name(self):
        return self.__class__.__name__


def _observation(masks, ex):
    """reference-channel selection shared by Nothing / Masking (enhancer.py:50-69,79-95)."""
    reference_channel = ex["reference_channel"]
    Observation = ex["Observation"]
    batched = {4: False, 5: True}[len(masks.shape)]
    if reference_channel is None:
        assert len(Observation.shape) == (3 if batched else 2), Observation.shape
    else:
        assert len(Observation.shape) == (4 if batched else 3), Observation.shape
        Observation = Observation[..., reference_channel, :, :]
    if isinstance(Observation, np.ndarray):
        Observation = torch.tensor(Observation, device=masks.device)
    return Observation, batched


class Dummy(ABC):
    def __call__(self, masks: torch.Tensor, ex, model):
        return None


class Nothing(ABC):
    def __call__(self, masks: torch.Tensor, ex, model):
        """the observation of the reference channel, with a speaker axis (enhancer.py:44-70)"""
        Observation, _ = _observation(masks, ex)
        return Observation[..., None, :, :]


class Masking(ABC):
    def __call__(self, masks: torch.Tensor, ex, model):
        """masks [B,K,1,T,F] -> complex [B,K,T,F] = Obs[ref] * mask (enhancer.py:98-100).
        Standalone form (mask tensor in).  ``Model.forward`` does not come through here for the
        Masking enhancer: it fuses sigmoid + product into one mask-head kernel."""
        if masks.shape[-3] != 1:
            raise ValueError(f"Masking takes one mask per speaker, got {masks.shape[-3]} (masks {tuple(masks.shape)}): the "
                             "squeeze of the mask axis is a no-op then and the product with the observation does not "
                             "broadcast (enhancer.py:98-100); train such an estimator through TorchBF")
        Observation, batched = _observation(masks, ex)
        m = torch.squeeze(masks, dim=-3)
        if not batched:
            m, Observation = m[None], Observation[None]
        est = _MaskMul.apply(m.contiguous(), Observation.contiguous())
        return est if batched else est[0]


class _MaskMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mask, obs):
        ctx.save_for_backward(obs)
        return H.mask_mul_fwd(mask, obs)

    @staticmethod
    def backward(ctx, dest):
        (obs,) = ctx.saved_tensors
        return H.mask_mul_bwd(dest, obs), None


def trace(input, axis1=-2, axis2=-1):
    """batched trace (enhancer.py:103-137)"""
    assert input.shape[axis1] == input.shape[axis2], input.shape
    return torch.diagonal(input, dim1=axis1, dim2=axis2).sum(-1)


class TorchBF(ABC):
    """Mask-based MVDR (Souden) beamformer in complex128 -- enhancer.py:140-265, same constructor
    arguments, same call signature, same checks.  One fused pipeline of three HIP kernels
    (statistics, per-bin solve, filtering; csrc/mvdr.hip).  The reference's class is plain differentiable
    torch, so a config with this enhancer and a time-domain loss trains the mask estimator through the beamformer
    there; here that takes ``differentiable=True`` (THIS PROJECT'S keyword, not a key of the reference's config):
    the call then goes through functional.mvdr_souden, whose backward is three more HIP stages and yields the
    gradient of the masks (never of the Observation: one that requires grad raises NotImplementedError).  With the
    default False the class is the evaluation-time enhancer it always was and refuses masks that require grad.
    Eager only either way: the singular check of the solve is a host sync, a hipGraph capture cannot hold it."""

    def __init__(self, bf="mvdr_souden", masking=False, masking_eps=0.0, eps=None, differentiable=False):
        super().__init__()
        self.differentiable = differentiable
        assert bf == "mvdr_souden", (bf, "Only mvdr_souden is implemented")
        self.bf = bf
        self.eps = eps
        self.masking = masking
        self.masking_eps = masking_eps

    def __call__(self, masks, ex, model):
        """masks [(B,) K, M, T, F] with M = 2 (target, interference) or 1 (interference = 1 - m);
        ex['Observation'] [(B,) D, T, F] complex128 -> [(B,) K, T, F] complex128."""
        batched = {4: False, 5: True}[len(masks.shape)]
        reference_channel = ex["reference_channel"]
        Observation = ex["Observation"]
        assert len(Observation.shape) == (4 if batched else 3), Observation.shape
        assert Observation.dtype == torch.complex128, Observation.dtype
        if masks.shape[-3] not in (1, 2):
            raise ValueError(masks.shape)
        if Observation.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("TorchBF: the Observation requires grad, but the MVDR backward has a gradient "
                                      "for the masks only (detach the Observation)")
        train = masks.requires_grad and torch.is_grad_enabled()
        if train and not self.differentiable:
            raise NotImplementedError("TorchBF is an evaluation-time enhancer by default: call it under "
                                      "torch.no_grad(), or construct it with differentiable=True to train "
                                      "through it (no backward kernel is run without that keyword)")
        Observation = Observation.to(masks.device)
        if not batched:
            masks, Observation = masks[None], Observation[None]
        if train:
            enh = Fn.mvdr_souden(masks, Observation, reference_channel, eps=self.eps, masking=self.masking,
                                 masking_eps=self.masking_eps)
        else:
            enh = H.mvdr_souden(masks.detach(), Observation, reference_channel, eps=self.eps,
                                masking=self.masking, masking_eps=self.masking_eps)
        return enh if batched else enh[0]


class OnlineMVDR(ABC):
    """Frame-recursive mask-based MVDR -- THIS PROJECT'S enhancer, the reference has no online mode: the
    PSDs of TorchBF grow (or forget, ``forgetting`` < 1) frame by frame, and frame t is filtered with the Souden filter of
    the statistics up to and including t, the interference PSD loaded with ``diag_load`` times the mean channel power.
    One HIP kernel (hip_ops.online_mvdr, csrc/mvdr.hip).  Called on a whole utterance like TorchBF it runs the recursion
    over all T frames in one launch -- what ``Model.online`` streams, chunk by chunk, bit for bit; with forgetting=1 and
    diag_load=0 its last frame is TorchBF's.  Evaluation only (there is no backward), one mask per speaker.  Neither
    default is tuned.
    ``pre_wpe`` (an `OnlineWPE` below; default None: nothing changes) dereverberates every frame before it is
    beamformed, the online counterpart of ClassicBF_np's pre_wpe: the masks still belong to the raw reference channel,
    the PSDs and the filtering read the dereverberated frames, and the carried state becomes the pair
    (the OnlineWPE's state, the PSDs)."""

    def __init__(self, forgetting=1.0, diag_load=1e-6, eps=None, masking=False, masking_eps=0.0, pre_wpe=None):
        super().__init__()
        self.forgetting = forgetting
        self.diag_load = diag_load
        self.eps = eps
        self.masking = masking
        self.masking_eps = masking_eps
        self.pre_wpe = pre_wpe

    def _kwargs(self):
        return dict(forgetting=self.forgetting, diag_load=self.diag_load, eps=self.eps, masking=self.masking,
                    masking_eps=self.masking_eps)

    def _check_pre_wpe(self):
        if self.pre_wpe is not None and not isinstance(self.pre_wpe, OnlineWPE):
            raise NotImplementedError(f"pre_wpe={self.pre_wpe!r}: a stream is dereverberated by this module's OnlineWPE "
                                      "(WPE / ChannelWiseWPE iterate over whole segments)")

    def chunk(self, masks, Y, state, reference_channel, with_observation=False):
        """The next frames of a stream: masks [B,K,(1,)Tc,F], Y [B,D,Tc,F] -> (enh [B,K,Tc,F] complex128, state).
        with_observation: -> (enh, state, the frames that were beamformed: Y, or pre_wpe's output)."""
        self._check_pre_wpe()
        if self.pre_wpe is None:
            enh, state = H.online_mvdr(masks, Y, state, reference_channel, **self._kwargs())
            return (enh, state, Y) if with_observation else (enh, state)
        if state is not None and not (isinstance(state, tuple) and len(state) == 2):
            raise ValueError("OnlineMVDR(pre_wpe=...): the state of a stream is the pair (OnlineWPE's state, PSDs) an "
                             f"earlier call returned, got {type(state).__name__}")
        wpe_state, psd = (None, None) if state is None else state
        H.online_mvdr_check(masks, Y, psd, reference_channel, self.forgetting, self.diag_load)
        X, wpe_state = self.pre_wpe.chunk(Y, wpe_state)
        enh, psd = H.online_mvdr(masks, X, psd, reference_channel, **self._kwargs())
        return (enh, (wpe_state, psd), X) if with_observation else (enh, (wpe_state, psd))

    def __call__(self, masks, ex, model):
        """masks [(B,) K, 1, T, F]; ex['Observation'] [(B,) D, T, F] complex64 | complex128 -> [(B,) K, T, F] complex128."""
        batched = {4: False, 5: True}[len(masks.shape)]
        Observation = ex["Observation"]
        assert len(Observation.shape) == (4 if batched else 3), Observation.shape
        if (masks.requires_grad or Observation.requires_grad) and torch.is_grad_enabled():
            raise NotImplementedError("OnlineMVDR is an evaluation-time enhancer: call it under torch.no_grad() (the "
                                      "recursion has no backward; train through Masking or TorchBF(differentiable=True))")
        if not batched:
            masks, Observation = masks[None], Observation[None]
        H.online_mvdr_check(masks, Observation, None, ex["reference_channel"], self.forgetting, self.diag_load)
        self._check_pre_wpe()
        if self.pre_wpe is not None:
            H.online_wpe_check(Observation, None, **self.pre_wpe._kwargs())
        enh, _ = self.chunk(masks.detach(), Observation.detach().to(masks.device), None, ex["reference_channel"])
        return enh if batched else enh[0]


class OnlineWPE(ABC):
    """Frame-recursive WPE dereverberation -- THIS PROJECT'S class, the reference has no online mode: the
    recursive least squares form of WPE above.  Per bin one rank-one update of the inverse correlation matrix of the
    delayed frames per frame, weighted by the inverse of the frame's power (the mean over the channels and the last
    ``power_context`` + 1 frames, floored at 1e-10 of the largest seen), forgotten with ``forgetting``; frame t is
    filtered with the taps of the frames before it.  One HIP kernel (hip_ops.online_wpe, csrc/wpe.hip).  ``chunk`` takes
    the next frames of a stream and the carried state; called on a whole utterance like WPE -- Observation [D, T, F]
    complex128, numpy in gives numpy out -- it runs the recursion over all T frames in one launch, bit for bit what the
    chunks give.  Evaluation only (there is no backward).  No default is tuned: taps and delay are WPE's, forgetting and
    load are placeholders that were not searched on data."""

    def __init__(self, taps=10, delay=2, forgetting=0.99, load=1.0, power_context=0):
        super().__init__()
        self.taps = taps
        self.delay = delay
        self.forgetting = forgetting
        self.load = load
        self.power_context = power_context

    def _kwargs(self):
        return dict(taps=self.taps, delay=self.delay, forgetting=self.forgetting, load=self.load,
                    power_context=self.power_context)

    def chunk(self, Y, state=None):
        """The next frames of a stream: Y [B,D,Tc,F] complex64 | complex128 -> (X [B,D,Tc,F] complex128, state)."""
        return H.online_wpe(Y, state, **self._kwargs())

    def __call__(self, Observation, inplace=False):
        if isinstance(Observation, np.ndarray):
            obs, numpy_out = torch.from_numpy(np.ascontiguousarray(Observation)), True
        elif isinstance(Observation, torch.Tensor):
            obs, numpy_out = Observation, False
        else:
            raise NotImplementedError(type(Observation), Observation)
        if obs.dtype != torch.complex128:
            raise TypeError(f"{self.name}: Observation is {obs.dtype}, complex128 is required (as for WPE; `chunk` takes "
                            "the complex64 frames of a stream too)")
        assert obs.dim() == 3, obs.shape
        H.online_wpe_check(obs[None], None, **self._kwargs())      # every refusal before anything touches the device
        obs = obs.detach()
        out, _ = self.chunk((obs if obs.is_cuda else obs.to("cuda"))[None])
        return out[0].cpu().numpy() if numpy_out else out[0]


def normalized_intervals(ai, T):
    """One speaker's activity -> [(s, e), ...], sorted, disjoint, non-empty, inside [0, T].
    ai: anything with ``.normalized_intervals`` (paderbox's ArrayInterval), a 0/1 array of length T,
    or a list of (s, e).  Empty intervals are dropped; overlapping, unsorted or out-of-range ones
    raise ValueError."""
    if hasattr(ai, "normalized_intervals"):
        pairs = ai.normalized_intervals
    else:
        arr = np.asarray(ai.detach().cpu() if isinstance(ai, torch.Tensor) else ai)
        if arr.ndim == 1 and arr.shape[0] == T:
            if not np.isin(arr, (0, 1)).all():
                raise ValueError("an activity array holds only 0 and 1")
            edges = np.flatnonzero(np.diff(np.concatenate([[0], arr.astype(np.int8), [0]])))
            pairs = edges.reshape(-1, 2)
        elif arr.size == 0:
            pairs = []
        elif arr.ndim == 2 and arr.shape[1] == 2:
            pairs = arr
        else:
            raise ValueError(f"expected .normalized_intervals, a 0/1 array of length {T} or a list of "
                             f"(start, end); got shape {arr.shape}")
    out, last = [], 0
    for s, e in pairs:
        if int(s) != s or int(e) != e:
            raise ValueError(f"interval ({s}, {e}) is not integral")
        s, e = int(s), int(e)
        if s < 0 or e > T or e < s:
            raise ValueError(f"interval ({s}, {e}) is not inside [0, {T}]")
        if s < last:
            raise ValueError(f"interval ({s}, {e}) overlaps or precedes the one ending at {last}: "
                             f"intervals must be sorted and disjoint")
        if e > s:
            out.append((s, e))
            last = e
    return out


def _table_intervals(rows, K, T):
    """host rows (k, s, e) of a segment table -> per speaker [(s, e), ...]; a row outside [0, K) x [0, T] or an empty
    one raises ValueError"""
    out = [[] for _ in range(K)]
    for k, s, e in rows:
        if not (0 <= k < K and 0 <= s < e <= T):
            raise ValueError(f"segment table row ({k}, {s}, {e}) lies outside speakers [0, {K}) x frames [0, {T}] or is "
                             f"empty")
        out[k].append((s, e))
    return out


class WPE(ABC):
    """WPE dereverberation -- enhancer.py:292-348, same constructor and call.  The reference hands the array to
    nara_wpe's wpe_v8 on the host; here it is one pipeline of HIP kernels (hip_ops.wpe, csrc/wpe.hip; the definition
    is DESIGN 4.5).  Observation [D, T, F] complex128: a torch tensor gives a device tensor, a numpy array a numpy
    array.  `inplace` is accepted and ignored: a new array is returned."""

    def __init__(self, taps=10, delay=2, iterations=3, psd_context=0, statistics_mode="full"):
        super().__init__()
        self.taps = taps
        self.delay = delay
        self.iterations = iterations
        self.psd_context = psd_context
        self.statistics_mode = statistics_mode

    def _kwargs(self):
        if self.psd_context != 0:
            raise NotImplementedError(f"psd_context={self.psd_context!r}: only 0 is built (the edge normalisation of "
                                      f"nara_wpe's window mean could not be checked against nara_wpe)")
        return dict(taps=self.taps, delay=self.delay, iterations=self.iterations,
                    statistics_mode=self.statistics_mode)

    def _layout(self, obs):
        return obs, (lambda out: out)

    def __call__(self, Observation, inplace=False):
        kw = self._kwargs()
        if isinstance(Observation, np.ndarray):
            obs, numpy_out = torch.from_numpy(np.ascontiguousarray(Observation)), True
        elif isinstance(Observation, torch.Tensor):
            obs, numpy_out = Observation.detach(), False
        else:
            raise NotImplementedError(type(Observation), Observation)
        if obs.dtype != torch.complex128:
            raise TypeError(f"{self.name}: Observation is {obs.dtype}, complex128 is required (the correlation matrices "
                            f"reach condition numbers of 1e11 on reverberant data)")
        assert obs.dim() == 3, obs.shape
        obs, back = self._layout(obs)
        checked = H.wpe_validate(obs, None, **kw)             # every refusal before anything touches the device
        out = back(H.wpe(obs.contiguous() if obs.is_cuda else obs.contiguous().to("cuda"), _rows=checked, **kw))
        return out.cpu().numpy() if numpy_out else out

    def rows(self, obs, rows):
        """The segment-wise form: every row (s, e) as if obs[:, s:e] were the whole array -> (obs_seg, row0)."""
        return H.wpe(obs, rows, **self._kwargs())


class ChannelWiseWPE(WPE):
    """WPE on every channel alone -- enhancer.py:351-367: the D = 1 kernels on '1 t (d f)'."""

    def _layout(self, obs):
        D, T, F = obs.shape
        return (obs.permute(1, 0, 2).reshape(1, T, D * F),
                lambda out: out.reshape(T, D, F).permute(1, 0, 2).contiguous())

    def rows(self, obs, rows):
        D, T, F = obs.shape
        seg, row0 = H.wpe(obs.permute(1, 0, 2).reshape(1, T, D * F).contiguous(), rows, **self._kwargs())
        return seg.reshape(-1, D, F).permute(1, 0, 2).contiguous(), row0


class ClassicBF_np(ABC):
    """Segment-wise mask-based MVDR (Souden) -- enhancer.py:370-590, same constructor, same call
    signature, same checks; `_np` is the reference's name (it runs numpy on pb_bss there), here it
    is one pipeline of HIP kernels over a segment table (hip_ops.segment_mvdr, csrc/mvdr.hip): for
    every activity interval of a speaker the PSDs of that interval only (_get_psd, real part), the
    distortion mask from the other speakers' masks, one beamformer, zeros outside the intervals.
    pre_wpe dereverberates the whole observation first, segment_wpe every interval's slice on its own (WPE above).
    The weights are TorchBF's phi[:, 0] / max(Re tr phi, tiny); pb_bss's least-squares fallback for
    singular systems is not reproduced: those raise torch.linalg.LinAlgError."""

    @classmethod
    def finalize_dogmatic_config(cls, config):
        config["distortion_mask"] = {"factory": enhancer_distortion_mask.SumCrossTalker}

    def __init__(self, bf="mvdr_souden", masking=False, masking_eps=0, distortion_mask=None,
                 pre_wpe=None, segment_wpe=None, mask_power=1):
        super().__init__()
        self.bf = bf
        self.masking = masking
        self.masking_eps = masking_eps
        self.distortion_mask = distortion_mask
        self.mask_power = mask_power
        self.pre_wpe = pre_wpe
        self.segment_wpe = segment_wpe

    def __repr__(self):
        return f"{self.__class__.__name__}()"

    def _kernel_mode(self):
        dm = self.distortion_mask
        if isinstance(dm, (enhancer_distortion_mask.SumCrossTalker, enhancer_distortion_mask.OneMinus)):
            return dm.kernel_mode, float(dm.eps)
        raise NotImplementedError(f"distortion_mask {dm!r}: the kernels build SumCrossTalker and OneMinus only")

    def __call__(self, masks, Observation, dia, segment_bf=True, numpy_out=False):
        """masks [K, M=1, T, F], Observation [D, T, F] complex128, dia: one activity per speaker
        (see normalized_intervals), a segment table int32 [S, 3] of rows (k, s, e) (segmenter.ActivitySegmenter; with
        numpy_out=True and no segment_wpe it goes to the kernels as it is, without a host read of its own) or None.
        numpy_out=True: the dense [K, T, F] device tensor; False: per speaker a dict {(s, e): [e - s, F]} of views."""
        if self.bf != "mvdr_souden":
            raise NotImplementedError(f"bf={self.bf!r}: only 'mvdr_souden' is implemented")
        for name in ("pre_wpe", "segment_wpe"):
            w = getattr(self, name)
            if w is not None and not isinstance(w, WPE):
                raise NotImplementedError(f"{name}={w!r}: only this module's WPE / ChannelWiseWPE are built")
        if not isinstance(masks, torch.Tensor):
            masks = torch.as_tensor(np.asarray(masks))
        if not isinstance(Observation, torch.Tensor):
            Observation = torch.as_tensor(np.asarray(Observation))
        mics = Observation.shape[0]
        assert mics >= 6, Observation.shape      # all channels loaded? (training usually loads one or two)
        K, M, T, F = masks.shape
        if M != 1:
            assert M == 2, masks.shape
            raise NotImplementedError(masks.shape)
        assert self.mask_power > 0, self.mask_power
        mode, dist_eps = self._kernel_mode()
        if mode == "one_minus":
            assert K == 1, masks.shape
        device_table = None
        if dia is None:
            assert segment_bf is False, segment_bf
            assert self.segment_wpe is None, self.segment_wpe
            assert numpy_out is True, numpy_out
            intervals = [[(0, T)]] * K
        elif isinstance(dia, torch.Tensor) and dia.dtype == torch.int32 and dia.dim() == 2 and dia.shape[1] == 3:
            # a segment table (segmenter.ActivitySegmenter): rows (k, s, e) with k < K inside [0, T]
            if not segment_bf:
                raise NotImplementedError("segment_bf=False with a diarization (the reference raises there too)")
            if numpy_out and self.segment_wpe is None:
                device_table, intervals = dia, None          # as it is: checked in the read of the singular check
            else:
                intervals = _table_intervals(dia.cpu().tolist(), K, T)      # these paths need host numbers anyway
        else:
            assert isinstance(dia, (tuple, list)), ("Expect list of ArrayInterval", type(dia), dia)
            assert len(dia) == K, (len(dia), K)
            if not segment_bf:
                raise NotImplementedError("segment_bf=False with a diarization (the reference raises there too)")
            intervals = [normalized_intervals(ai, T) for ai in dia]
        device = masks.device if masks.is_cuda else torch.device("cuda")
        if device_table is not None:
            table = device_table.to(device)
        else:
            table = [(k, s, e) for k, iv in enumerate(intervals) for s, e in iv]
        if len(table) == 0:
            out = torch.zeros(K, T, F, dtype=torch.complex128, device=device)
        else:
            Observation = Observation.to(device)
            if self.pre_wpe is not None:
                Observation = self.pre_wpe(Observation)
            packed = {}
            if self.segment_wpe is not None:
                # one table of all rows: the launches do not grow with the number of segments
                packed["obs_seg"], packed["row0"] = self.segment_wpe.rows(Observation, [(s, e) for _, s, e in table])
            out = H.segment_mvdr(masks.detach().to(device), Observation, table, mode=mode,
                                 distortion_eps=dist_eps, mask_power=self.mask_power, masking=self.masking,
                                 masking_eps=self.masking_eps, psd_real=True, check_table=device_table is not None,
                                 **packed)
        if numpy_out:
            return out
        return [{(s, e): out[k, s:e] for s, e in iv} for k, iv in enumerate(intervals)]


ClassicBF = ClassicBF_np


class GSS(ABC):
    """Guided source separation -- THIS PROJECT'S class, the reference has none: what turns the speaker
    activities of a TS-VAD model into audio.  Per frequency bin a complex angular central Gaussian mixture model with
    one class per speaker and one for noise is fitted by ``iterations`` EM steps, the activities as hard priors on the
    class affiliations (a speaker who is silent in a frame cannot own it; noise is always allowed); the posteriors are
    the masks of the segment-wise MVDR.  One pipeline of HIP kernels (hip_ops.guided_cacgmm, csrc/gss.hip), float64.
    ``block`` / ``context``: the model is fitted on windows of block + 2 context frames and read in their middle
    (nobody moves inside a window); None: one fit over the recording.  ``weights``: 'bin' (mixture weights per bin) or
    'uniform'.  ``load``: the diagonal loading of every B_c, relative to its mean eigenvalue 1.  No default is tuned.
    ``masks`` returns the posteriors [K+1, 1, T, F] (class K: noise); calling the object runs the chain
    pre_wpe (once) -> masks -> ``bf`` (default ClassicBF_np with SumCrossTalker), the noise class as a (K+1)-th speaker
    without rows, so that the distortion mask of a speaker sums every other class, noise included.  Dereverberation
    belongs to this class's ``pre_wpe``: a ``bf`` with a pre_wpe of its own is refused, the masks and the filter would
    see different observations."""

    @classmethod
    def finalize_dogmatic_config(cls, config):
        config["bf"] = {"factory": ClassicBF_np}

    def __init__(self, iterations=20, load=1e-6, weights="bin", block=None, context=0, pre_wpe=None, bf=None):
        super().__init__()
        self.iterations = iterations
        self.load = load
        self.weights = weights
        self.block = block
        self.context = context
        self.pre_wpe = pre_wpe
        self.bf = bf if bf is not None else ClassicBF_np(distortion_mask=enhancer_distortion_mask.SumCrossTalker())

    def _observation(self, Observation):
        if not isinstance(Observation, torch.Tensor):
            Observation = torch.as_tensor(np.ascontiguousarray(Observation))
        if Observation.dtype != torch.complex128:
            raise TypeError(f"{self.name}: Observation is {Observation.dtype}, complex128 is required")
        assert Observation.dim() == 3, Observation.shape
        return Observation.detach()

    def _activity(self, dia, T, K, device):
        """dia -> (activity [K, T] on `device`, what the beamformer takes as dia for K + 1 'speakers')"""
        if isinstance(dia, torch.Tensor) and dia.dtype == torch.int32 and dia.dim() == 2 and dia.shape[1] == 3:
            if T == 3:
                raise ValueError(f"{self.name}: an int32 [*, 3] tensor with T = 3 frames is a segment table or an activity: "
                                 "pass the activity as uint8 or bool, or the table's speakers as lists of intervals")
            if K is None:
                raise ValueError(f"{self.name}: a segment table comes with K, the number of speakers")
            table = dia.to(device)
            return H.segments_to_activity(table, K, T), table          # stays on the device
        if isinstance(dia, (torch.Tensor, np.ndarray)):
            act = torch.as_tensor(dia)
            if act.dim() != 2 or act.shape[1] != T:
                raise ValueError(f"{self.name}: an activity array is [K, {T}], got {tuple(act.shape)}")
            rows = list(act.detach().cpu().numpy())
        else:
            assert isinstance(dia, (tuple, list)), ("Expect list of ArrayInterval", type(dia), dia)
            rows = dia
        if K is not None and len(rows) != K:
            raise ValueError(f"{self.name}: {len(rows)} activities for K = {K} speakers")
        intervals = [normalized_intervals(ai, T) for ai in rows]
        host = np.zeros((len(intervals), T), dtype=np.uint8)
        for k, iv in enumerate(intervals):
            for s, e in iv:
                host[k, s:e] = 1
        return torch.from_numpy(host).to(device), intervals + [[]]      # the noise class has no rows

    def _masks(self, obs, act):
        blocks = H.gss_uniform_blocks(obs.shape[1], self.block, self.context)
        return H.guided_cacgmm(obs, act, self.iterations, self.load, self.weights, blocks)[:, None]

    def masks(self, Observation, dia, K=None):
        """Observation [D, T, F] complex128 (D >= 1), dia: one activity per speaker (see normalized_intervals), a 0/1
        array [K, T], or a segment table int32 [S, 3] together with K (that route stays on the device; an int32 [*, 3]
        tensor is always read as a table, and refused as ambiguous when T = 3) -> float32 [K+1, 1, T, F] on the device."""
        obs = self._observation(Observation)
        device = obs.device if obs.is_cuda else torch.device("cuda")
        act, _ = self._activity(dia, obs.shape[1], K, device)
        H.guided_cacgmm_check(obs, act, self.iterations, self.load, self.weights)      # before obs moves
        return self._masks(obs.to(device), act)

    def __call__(self, Observation, dia, numpy_out=False, K=None):
        """The whole chain; the output is ClassicBF_np's for the K speakers: numpy_out=True the dense [K, T, F] device
        tensor, False per speaker a dict {(s, e): [e - s, F]} of views (not with a segment table: its rows stay on
        the device)."""
        if not isinstance(self.bf, ClassicBF_np):
            raise NotImplementedError(f"bf={self.bf!r}: the masks go to this module's ClassicBF_np")
        if self.pre_wpe is not None and not isinstance(self.pre_wpe, WPE):
            raise NotImplementedError(f"pre_wpe={self.pre_wpe!r}: only this module's WPE / ChannelWiseWPE are built")
        if self.bf.pre_wpe is not None:
            raise ValueError(f"{self.name}: bf.pre_wpe is set: the masks would be fitted on another observation than the "
                             f"beamformer filters (or, with pre_wpe here as well, it would be dereverberated twice); give "
                             f"pre_wpe to {self.name} alone")
        obs = self._observation(Observation)
        assert obs.shape[0] >= 6, obs.shape      # all channels loaded? (ClassicBF_np's own check)
        device = obs.device if obs.is_cuda else torch.device("cuda")
        act, bf_dia = self._activity(dia, obs.shape[1], K, device)
        H.guided_cacgmm_check(obs, act, self.iterations, self.load, self.weights)
        if isinstance(bf_dia, torch.Tensor) and not numpy_out:
            raise NotImplementedError(f"{self.name}: a segment table gives the dense output (numpy_out=True)")
        obs = obs.to(device)
        if self.pre_wpe is not None:
            obs = self.pre_wpe(obs)
        out = self.bf(self._masks(obs, act), obs, bf_dia, numpy_out=numpy_out)
        return out[:act.shape[0]]
