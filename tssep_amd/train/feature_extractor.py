"""STFT feature extractors -- drop-ins for tssep/train/feature_extractor.py (and the
padertorch ``STFT`` base it star-imports, feature_extractor.py:8) on the HIP kernels.

Implemented: ``STFT`` (base: stft / istft / __call__), ``Log1pMaxNormAbsSTFT`` (:183-263),
``ConcaternatedSTFTFeatures`` (:290-367), ``TorchMFCC`` (feature_extractor_torchaudio.py), ``AbsSTFT`` / ``Log1pAbsSTFT``
(padertorch's), ``MVNLog1pAbsSTFT`` (:112-168), ``NoFeatureSTFT`` (:171-180).  Not built: the two IPD classes, KaldiTorch*.
Inputs must be CUDA tensors: there is no CPU path in this package.
"""
import math

import numpy as np
import torch

from .. import functional as Fn
from .. import hip_ops as H
from ..configurable import Configurable


def _cuda_f32(x):
    if isinstance(x, np.ndarray):
        x = torch.as_tensor(x)
    if not x.is_cuda:
        raise RuntimeError("tssep_amd runs on the GPU only: move the input to cuda first "
                           "(no CPU fallback)")
    return x.to(torch.float32)


class STFT(Configurable):
    """padertorch.contrib.cb.feature_extractor.STFT on paderbox.transform.module_stft (star-imported at
    feature_extractor.py:8): every option the reference's configs may set (init_cfg_common.yaml:33-43) --
    ``window_length <= size`` (the transform is zero-padded), ``pad`` (False: only full frames), ``fading`` in
    {True / 'full', 'half', False / None}.  The FFT plan is 1024 / 256 (any other: TSSEP_E_UNSUPPORTED from
    the library, naming the plan)."""

    def __init__(self, size=1024, shift=256, window_length=None, pad=True, fading=True,
                 output_size=None, window="blackman"):
        if window_length is None:
            window_length = size
        if not 0 < window_length <= size:
            raise ValueError(f"window_length = {window_length} must lie in (0, size = {size}]")
        if fading not in (None, False, True, "full", "half"):
            raise ValueError(f"fading = {fading!r}: None, False, True, 'full' or 'half' (paderbox stft)")
        self.size, self.shift, self.window_length = size, shift, window_length
        self.pad, self.fading, self.window = pad, fading, window
        self.output_size = self._get_output_size(output_size)

    @property
    def frequencies(self):
        return self.size // 2 + 1

    def _get_output_size(self, output_size):
        if output_size is None:
            return self.frequencies
        return output_size

    def _windows(self, device):
        return Fn.windows(self.window, self.size, self.shift, device, self.window_length)

    def _fade(self):
        """(zeros in front, zeros behind) that `fading` adds to a signal (paderbox stft): 'full' = window_length -
        shift on both sides, 'half' = half of that (the odd sample behind)."""
        if self.fading in (None, False):
            return 0, 0
        p = self.window_length - self.shift
        if self.fading == "half":
            return p // 2, p - p // 2
        return p, p

    def _plain(self):
        """The configuration the fused kernels are built for: the 1024 / 256 plan, full fading, a full-size window."""
        return self.window_length == self.size and self.fading in (True, "full") and self._check_plan() == 1

    def _check_plan(self):
        """1: the plan specialised to the shipped configs (1024 / 256: fused mask head + inverse STFT); 2: the general plan
        (stft_generic.hip: even sizes with size / 2 = 2^a 3^b 5^c <= 2048, shift <= min(size, 512) -- 512 / 128, TorchMFCC's
        own default 400 / 200, ...); anything else raises, naming the plan."""
        from .. import _lib
        plan = int(_lib.lib().tssep_stft_plan(int(self.size), int(self.shift)))
        if not plan:
            raise RuntimeError(f"unsupported FFT plan size={self.size}, shift={self.shift}: libtssep_hip.so builds even sizes "
                               "with size / 2 = 2^a 3^b 5^c <= 2048 and shift <= min(size, 512) whose two LDS lines per "
                               "wave fit the device (TSSEP_E_UNSUPPORTED)")
        return plan

    FEATURE_MAX_BINS = 1032      # MAXF of csrc/feat.hip: the feature kernels keep one LDS line of F bins per wave

    def _check_feature_bins(self):
        """The feature kernels (tssep_feat_fwd) take at most FEATURE_MAX_BINS frequency bins (size <= 2062): say so up
        front instead of TSSEP_E_SHAPE out of the kernel launch after the STFT plan was accepted."""
        F = self.size // 2 + 1
        if F > self.FEATURE_MAX_BINS:
            raise RuntimeError(f"{type(self).__name__}: size={self.size} gives {F} frequency bins; the feature kernels of "
                               f"libtssep_hip.so take at most {self.FEATURE_MAX_BINS} (size <= {2 * (self.FEATURE_MAX_BINS - 1)}); "
                               "the STFT / iSTFT themselves support this plan")

    def frames(self, num_samples):
        lead, tail = self._fade()
        n = num_samples + lead + tail
        if self.pad:
            return max(-(-(n - self.window_length) // self.shift), 0) + 1
        if n < self.window_length:
            raise ValueError(f"pad=False: {num_samples} samples (+ fading) are shorter than one window")
        return (n - self.window_length) // self.shift + 1

    def stft(self, signal):
        """[..., N] -> complex64 [..., T, F]  (fe.stft, model.py:503-504)"""
        self._check_plan()
        x = _cuda_f32(signal)
        w, _ = self._windows(x.device)
        x2 = x.reshape(-1, x.shape[-1])
        T = self.frames(x.shape[-1])
        if self._plain():
            X = H.stft_fwd(x2, w, self.size, self.shift, True, T=T)
        else:
            # the kernel knows "size - shift zeros in front" or none: any other fade is laid out here (zero padding is
            # layout, the transform stays the library's); frames reaching past the signal read zeros (pad=True) or
            # do not exist (pad=False: T is smaller)
            lead, tail = self._fade()
            if lead or tail:
                x2 = torch.nn.functional.pad(x2, (lead, tail))
            X = H.stft_fwd(x2, w, self.size, self.shift, False, T=T)
        return X.reshape(*x.shape[:-1], X.shape[-2], X.shape[-1])

    def frame_activity(self, signal, threshold):
        """[..., N] -> float32 [..., T] of 0 / 1: VADSigmoidBCE.prepare_target (loss.py:316-321) of ``self.stft(signal)`` --
        sum_f |X| per frame, divided by its maximum over the row's frames, compared with ``threshold`` -- without the
        spectrum: the frame kernel sums the magnitudes of the bins it formed (hip_ops.stft_framemag).  Options as in
        ``stft``."""
        self._check_plan()
        x = _cuda_f32(signal)
        w, _ = self._windows(x.device)
        x2 = x.reshape(-1, x.shape[-1])
        T = self.frames(x.shape[-1])
        if self._plain():
            a = H.stft_framemag(x2, w, self.size, self.shift, True, T=T)
        else:
            lead, tail = self._fade()          # (zero padding is layout, as in `stft`)
            if lead or tail:
                x2 = torch.nn.functional.pad(x2, (lead, tail))
            a = H.stft_framemag(x2, w, self.size, self.shift, False, T=T)
        return H.vad_from_mag(a, threshold).reshape(*x.shape[:-1], T)

    @staticmethod
    def stft_activity(X, threshold):
        """A spectrum [..., T, F] (complex, or real: loss.py's doctest) on the device -> float32 [..., T] of 0 / 1, the
        activity ``frame_activity`` derives from the signal."""
        if X.dtype == torch.complex128:
            X = X.to(torch.complex64)
        elif not X.is_complex():
            X = X.to(torch.float32)
        if not X.is_cuda:
            raise RuntimeError("tssep_amd runs on the GPU only: move the spectrum to cuda first (no CPU fallback)")
        T, F = X.shape[-2:]
        a = H.framemag(X.reshape(-1, T, F))
        return H.vad_from_mag(a, threshold).reshape(X.shape[:-1])

    def _num_samples(self, T, num_samples):
        lead, tail = self._fade()
        full = (T - 1) * self.shift + self.window_length - lead - tail
        return full if num_samples is None else min(num_samples, full)

    def istft(self, signal, num_samples=None):
        """complex [..., T, F] -> [..., N]  (fe.istft, model.py:661-664); differentiable.  The transform runs in float32:
        a complex128 estimate (TorchBF's) is cast to complex64 in front of it, one torch cast each way."""
        self._check_plan()
        if signal.dtype == torch.complex128:
            signal = signal.to(torch.complex64)
        if self.window_length % self.shift:
            raise ValueError("istft: window_length must be a multiple of shift (paderbox's biorthogonal window)")
        T = signal.shape[-2]
        N = self._num_samples(T, num_samples)
        _, wsyn = self._windows(signal.device)
        lead, _ = self._fade()
        lead0 = self.size - self.shift                 # what the kernel drops in front
        if lead == lead0:
            return Fn.istft(signal, wsyn, N, self.size, self.shift, True)
        # another fade: k empty frames in front move the overlap-add by k hops, d more samples are computed and cut
        # (layout only; autograd takes pad and slice back)
        k = -(-(lead0 - lead) // self.shift)
        d = lead - lead0 + k * self.shift
        Xp = torch.nn.functional.pad(torch.view_as_real(signal), (0, 0, 0, 0, k, 0))
        y = Fn.istft(torch.view_as_complex(Xp), wsyn, N + d, self.size, self.shift, True)
        return y[..., d:]

    def masked_istft(self, logit, observation, num_samples=None, target=None, vad=None):
        """istft(sigmoid(logit) * observation) as one fused kernel each way (functional.mask_istft):
        logit [B,K,T,F], observation complex [B,T,F] -> [B,K,N]; ``target`` [B,K,N] (optional) lets the
        forward accumulate the |estimate - target| sums a LogMAE / MAE loss needs.
        explicit_vad rows (logit [B,K,T,F+1], the VAD logit at column 0) -> (time estimate, the gate column's BCE against
        ``vad`` [B,K,T] or None)."""
        gated = logit.shape[-1] == observation.shape[-1] + 1
        if self._plain():
            _, wsyn = self._windows(logit.device)
            est, bce = Fn.mask_istft(logit, observation, wsyn, self._num_samples(logit.shape[-2], num_samples), self.size,
                                     self.shift, True, tgt=target, vad=vad if gated else None)
        else:                         # the fused tail is built for the shipped STFT; any other: mask head, then istft
            est = (Fn.mask_head_gated if gated else Fn.mask_head)(logit, observation)[1]
            est = self.istft(est, num_samples=num_samples)
            bce = Fn.gate_bce(logit, vad) if gated and vad is not None else None
        return (est, bce) if gated else est

    # ---- a live signal in pushes: the caller carries the state between the calls -------------------------
    causal = False        # the feature statistics span the whole utterance (the classes below take causal=True)

    def _check_stream(self):
        """The stream kernels are built for the plain 1024 / 256 STFT: say what is missing for any other."""
        missing = []
        if (self.size, self.shift) != (1024, 256):
            missing.append(f"size / shift = {self.size} / {self.shift} (a stream kernel for that FFT plan)")
        if self.window_length != self.size:
            missing.append(f"window_length = {self.window_length} < size (a stream kernel for a zero-padded window)")
        if self.fading not in (True, "full"):
            missing.append(f"fading = {self.fading!r} (the carried state is the full fade)")
        if not self.pad:
            missing.append("pad = False (flush pads the last frame)")
        if missing:
            raise NotImplementedError("the online STFT / inverse STFT are built for size 1024, shift 256, a full-size "
                                      "window, fading 'full' and pad=True; not built: " + "; ".join(missing))

    def stft_chunk(self, x_new, tail=None):
        """The frames a push completes: x_new [..., Tc * shift], tail [rows, size - shift] the state of the push before
        (None: a fresh stream) -> (complex64 [..., Tc, F] = the frames ``stft`` gives at those indices, bit for bit; the
        new tail).  The utterance's last 3 or 4 frames come from pushing zeros (the trailing fade): OnlineSeparator.flush."""
        self._check_stream()
        x = _cuda_f32(x_new)
        if x.shape[-1] == 0 or x.shape[-1] % self.shift:
            raise ValueError(f"stft_chunk: a push holds a positive multiple of shift = {self.shift} samples, not {x.shape[-1]}")
        w, _ = self._windows(x.device)
        X, tail = H.stft_stream_fwd(x.reshape(-1, x.shape[-1]), tail, w, self.size, self.shift)
        return X.reshape(*x.shape[:-1], X.shape[-2], X.shape[-1]), tail

    def istft_chunk(self, signal, ola=None, skip=0, num_samples=None, differentiable=False):
        """The samples the stream's next frames complete: complex64 [..., Tc, F], ola the carry of the call before (None:
        a fresh stream), skip = max(0, 3 - frames of the earlier calls) -> ([..., (Tc - skip) * shift] -- the first
        ``num_samples`` of them in the utterance's final call --, the new carry).  differentiable=True: the call is a node
        of the graph with a gradient for ``signal`` and ``ola``; without it forward only."""
        self._check_stream()
        X = signal.to(torch.complex64) if signal.dtype == torch.complex128 else signal
        _, wsyn = self._windows(X.device)
        if differentiable:
            y, ola = Fn.istft_stream(X.reshape(-1, X.shape[-2], X.shape[-1]), wsyn, ola, skip, num_samples, self.size,
                                     self.shift)
        else:
            y, ola = H.istft_stream_fwd(X.reshape(-1, X.shape[-2], X.shape[-1]), wsyn, ola, skip, num_samples, self.size,
                                        self.shift)
        return y.reshape(*X.shape[:-2], y.shape[-1]), ola

    def masked_istft_chunk(self, logit, observation, ola=None, skip=0, num_samples=None, differentiable=False):
        """``masked_istft`` on the stream's next frames (plain or explicit_vad rows): logit [B,K,Tc,F(+1)], observation
        complex64 [B,Tc,F] -> ([B,K,n], the new carry); arguments as ``istft_chunk``.  Neither mask nor masked spectrum is
        written.  differentiable=True: a node of the graph with a gradient for ``logit`` and ``ola``, none for the
        observation."""
        self._check_stream()
        _, wsyn = self._windows(logit.device)
        if differentiable:
            return Fn.mask_istft_stream(logit, observation, wsyn, ola, skip, num_samples, self.size, self.shift)
        return H.mask_istft_stream_fwd(logit, observation, wsyn, ola, skip, num_samples, self.size, self.shift)

    def stft_to_feature(self, stft_signals):
        raise NotImplementedError(type(self))

    def __call__(self, signal):
        return self.stft_to_feature(self.stft(signal))

    def sample_index_to_frame_index(self, sample_index):
        """paderbox STFT.sample_index_to_frame_index (feature_extractor.py:208,306)."""
        from ..util.utils import sample_index_to_stft_frame_index
        return sample_index_to_stft_frame_index(sample_index, self.window_length, self.shift, self.fading)


class Log1pMaxNormAbsSTFT(STFT):
    def __init__(self, size=1024, shift=256, window_length=None, pad=True, fading=True,
                 output_size=None, window="blackman", statistics_axis="tf", causal=False):
        super().__init__(size=size, shift=shift, window_length=window_length, pad=pad,
                         fading=fading, output_size=output_size, window=window)
        if statistics_axis not in H.STAT_AXES:
            raise ValueError(f"statistics_axis = {statistics_axis!r}: 'tf', 't' or 'f' (feature_extractor.py:239-242)")
        if causal and statistics_axis == "t":
            raise NotImplementedError("Log1pMaxNormAbsSTFT(causal=True, statistics_axis='t'): a running maximum per "
                                      "(utterance, frequency) is not built ('tf': the running maximum of the utterance; "
                                      "'f' is causal as it is)")
        self.statistics_axis = statistics_axis
        self.causal = bool(causal)           # this project's own keyword
        self._check_feature_bins()

    def stft_to_feature(self, stft_signals, state=None, return_state=False):
        """causal=True: norm[b,t] = max over t' <= t and f of |X| (0 so far: the feature is 0).  ``state`` [rows, 2] is the
        state a chunk's predecessor returned (None: the utterance starts here); return_state: -> (feature, state)."""
        X = stft_signals
        lead = X.shape[:-2]
        X3 = X.reshape(-1, X.shape[-2], X.shape[-1]).contiguous()
        if self.causal and self.statistics_axis == "tf":
            out, _, state = H.feat_causal_fwd(X3, None, None, 0, state=state)
        else:
            if not self.causal:              # ('f' is causal as it is: a state passes through untouched)
                _no_state(self, state)
            out, _ = H.feat_fwd(X3, None, None, 0, statistics_axis=self.statistics_axis)
        out = out.reshape(*lead, X.shape[-2], X.shape[-1])
        return (out, state) if return_state else out


def _no_state(fe, state):
    if state is not None:
        raise ValueError(f"{type(fe).__name__}: a carried state belongs to causal statistics (causal=True); these span "
                         "the whole utterance")


def _spectrum3(X):
    """[..., T, F] (a 2-D spectrum is one utterance) on the device -> (complex64 [rows, T, F], the leading dimensions)."""
    if isinstance(X, np.ndarray):
        X = torch.as_tensor(X)
    if not X.is_cuda:
        raise RuntimeError("tssep_amd runs on the GPU only: move the spectrum to cuda first (no CPU fallback)")
    if X.dim() < 2:
        raise ValueError(f"stft_to_feature: a spectrum [..., T, F], got {tuple(X.shape)}")
    if X.dtype != torch.complex64:
        X = X.to(torch.complex64)
    return X.reshape(-1, X.shape[-2], X.shape[-1]).contiguous(), X.shape[:-2]


class AbsSTFT(STFT):
    """padertorch.contrib.cb.feature_extractor.AbsSTFT (star-imported at feature_extractor.py:8): |X|.  No statistics, so
    ``causal=True`` (this project's own keyword) changes nothing: a state passes through untouched."""
    _kind = "abs"

    def __init__(self, size=1024, shift=256, window_length=None, pad=True, fading=True,
                 output_size=None, window="blackman", causal=False):
        super().__init__(size=size, shift=shift, window_length=window_length, pad=pad,
                         fading=fading, output_size=output_size, window=window)
        self.causal = bool(causal)
        self._check_feature_bins()

    def _check_feature_bins(self):
        F = self.size // 2 + 1
        if F > H.SPECFEAT_MAX_BINS:
            raise RuntimeError(f"{type(self).__name__}: size={self.size} gives {F} frequency bins; the spectral feature "
                               f"kernels of libtssep_hip.so take at most {H.SPECFEAT_MAX_BINS} (size <= "
                               f"{2 * (H.SPECFEAT_MAX_BINS - 1)}); the STFT / iSTFT themselves support this plan")

    def _feature(self, X3, state, out=None, col0=0):
        """[rows, T, F] -> (view [rows, T, F] -- of ``out`` from column ``col0`` when given --, the state)"""
        if not self.causal:
            _no_state(self, state)
        return H.specfeat_fwd(X3, self._kind, out=out, col0=col0), state

    def stft_to_feature(self, stft_signals, state=None, return_state=False):
        X3, lead = _spectrum3(stft_signals)
        out, state = self._feature(X3, state)
        out = out.reshape(*lead, X3.shape[-2], X3.shape[-1])
        return (out, state) if return_state else out


class Log1pAbsSTFT(AbsSTFT):
    """padertorch's Log1pAbsSTFT: log1p(|X|) (the doctest at feature_extractor.py:117-119)."""
    _kind = "log1p"


class MVNLog1pAbsSTFT(Log1pAbsSTFT):
    """feature_extractor.py:112-168: log1p(|X|) minus its mean over the utterance's frames, one mean per frequency.
    ``causal=True`` (this project's own): the mean of the frames so far -- a running sum S and a weight n per
    utterance, ``S = a S + L, n = a n + 1, out = L - S / n`` with ``a = forgetting`` in (0, 1] (1: every frame counts
    alike; < 1: a frame's weight decays by a per hop, the stream forgets).  ``state`` float64 [rows, F + 1] is what a
    chunk's predecessor returned (None: the utterance starts here)."""
    _kind = "mvn"

    def __init__(self, size=1024, shift=256, window_length=None, pad=True, fading=True,
                 output_size=None, window="blackman", norm_means: bool = True, norm_vars: bool = False,
                 eps: float = 1.0e-20, causal=False, forgetting=1.0):
        super().__init__(size=size, shift=shift, window_length=window_length, pad=pad, fading=fading,
                         output_size=output_size, window=window, causal=causal)
        self.norm_means, self.norm_vars, self.eps = norm_means, norm_vars, eps
        if not 0.0 < float(forgetting) <= 1.0:
            raise ValueError(f"MVNLog1pAbsSTFT: forgetting = {forgetting} lies outside (0, 1]")
        if float(forgetting) != 1.0 and not self.causal:
            raise ValueError(f"MVNLog1pAbsSTFT: forgetting = {forgetting} belongs to the running mean (causal=True); the "
                             "mean of causal=False spans the whole utterance")
        self.forgetting = float(forgetting)

    def _feature(self, X3, state, out=None, col0=0):
        if not self.norm_means:
            raise NotImplementedError()              # (feature_extractor.py:165-166)
        if self.norm_vars:
            raise NotImplementedError()              # (:163-164)
        if self.causal:
            return H.specfeat_causal_fwd(X3, state, self.forgetting, out=out, col0=col0)
        return super()._feature(X3, state, out, col0)


class NoFeatureSTFT(STFT):
    """feature_extractor.py:171-180: no spectral feature at all (host only: a slice).  ``causal`` is accepted because
    ConcaternatedSTFTFeatures copies the key into its parts; there is nothing it could change."""

    def __init__(self, size=1024, shift=256, window_length=None, pad=True, fading=True,
                 output_size=None, window="blackman", causal=False):
        super().__init__(size=size, shift=shift, window_length=window_length, pad=pad,
                         fading=fading, output_size=output_size, window=window)
        self.causal = bool(causal)

    def stft_to_feature(self, stft_signals, state=None, return_state=False):
        out = stft_signals[..., :0]
        return (out, state) if return_state else out

    def _get_output_size(self, output_size):
        if output_size is None:
            return 0
        assert output_size == 0, (output_size, self.frequencies)
        return output_size


class TorchMFCC(STFT, torch.nn.Module):
    """feature_extractor_torchaudio.py:11-106; filterbank / DCT tables restated from
    torchaudio 2.0.2 (absent here; parity unpinned, see oracle/features.py)."""

    def __init__(self, size=400, shift=200, window_length=None, pad=True, fading=True,
                 output_size=None, window="hann", sample_rate: int = 16000, n_mfcc: int = 40,
                 dct_norm: str = "ortho", log_mels: bool = False, f_min: float = 40,
                 f_max: float = -400, n_mels: int = 40, mel_norm: str = None,
                 mel_scale: str = "htk", causal: bool = False):
        torch.nn.Module.__init__(self)
        self.n_mfcc = n_mfcc
        self.causal = bool(causal)           # this project's own keyword
        STFT.__init__(self, size=size, shift=shift, window_length=window_length, pad=pad,
                      fading=fading, output_size=output_size, window=window)
        # every option of feature_extractor_torchaudio.py:22-39 (round 5; the shipped configs use the defaults): the mel scale
        # ('htk' | 'slaney'), its area normalisation (None | 'slaney'), the DCT normalisation ('ortho' | None) are TABLES
        # handed to tssep_feat_fwd, `log_mels` is an argument of the kernel -- restated from torchaudio 2.0.2 (absent here:
        # parity unpinned like the defaults, oracle/features.py)
        if mel_scale not in ("htk", "slaney"):
            raise ValueError('mel_scale should be one of "htk" or "slaney"')        # (torchaudio's message)
        if mel_norm is not None and mel_norm != "slaney":
            raise ValueError('norm must be one of None or "slaney"')
        if dct_norm is not None and dct_norm != "ortho":
            raise ValueError("norm must be either 'ortho' or None")
        self.sample_rate, self.f_min = sample_rate, f_min
        if f_max and f_max < 0:
            f_max = sample_rate + f_max                       # :57-58
        self.f_max, self.n_mels = f_max, n_mels
        self.dct_norm, self.mel_norm, self.top_db, self.log_mels = dct_norm, mel_norm, 80, log_mels
        # module tree of the reference (feature_extractor_torchaudio.py:69-85): a parameter-free
        # ``amplitude_to_DB``, ``mel_scale`` holding the persistent buffer ``fb`` and the buffer
        # ``dct_mat`` -> checkpoint keys ``<fe>.dct_mat`` and ``<fe>.mel_scale.fb``, so a checkpoint the
        # reference wrote loads with strict=True (init_cfg_tssep.yaml:22)
        self.amplitude_to_DB = _AmplitudeToDB("power", self.top_db)
        self.mel_scale = _MelScale(n_mels, sample_rate, f_min, f_max, size // 2 + 1, mel_norm, mel_scale)
        self.register_buffer("dct_mat", _create_dct(n_mfcc, n_mels, dct_norm))

    @property
    def fb(self):
        return self.mel_scale.fb

    def _get_output_size(self, output_size):
        return self.n_mfcc if output_size is None else output_size

    def stft_to_feature(self, stft_signals, state=None, return_state=False):
        """causal=True: floor[b,t] = max over t' <= t and m of dB - top_db, per utterance (``state`` / return_state as in
        Log1pMaxNormAbsSTFT)."""
        X = stft_signals
        if X.dim() == 2:        # un-batched example: the dB floor is per utterance (torchaudio 2-D case)
            out = self.stft_to_feature(X[None], state, return_state)
            return (out[0][0], out[1]) if return_state else out[0]
        assert X.dim() == 3, X.shape
        self._check_feature_bins()
        if self.causal:
            out, _, state = H.feat_causal_fwd(X, self.fb, self.dct_mat, self.n_mfcc, self._db_arg, state=state)
        else:
            _no_state(self, state)
            out, _ = H.feat_fwd(X, self.fb, self.dct_mat, self.n_mfcc, self._db_arg)
        out = out[..., :self.n_mfcc]
        return (out, state) if return_state else out

    @property
    def _db_arg(self):
        """top_db for tssep_feat_fwd; negative = `log_mels` (log(mel + 1e-6), no floor: include/tssep_hip.h)."""
        return -1.0 if self.log_mels else float(self.top_db)


class _MelScale(torch.nn.Module):
    """Holder of the mel filterbank under torchaudio's key (``MelScale.fb``, a persistent buffer
    [n_freqs, n_mels]); the filtering itself runs inside tssep_feat_fwd."""

    def __init__(self, n_mels, sample_rate, f_min, f_max, n_stft, norm=None, mel_scale="htk"):
        super().__init__()
        self.n_mels, self.sample_rate, self.f_min, self.f_max = n_mels, sample_rate, f_min, f_max
        self.norm, self.mel_scale = norm, mel_scale
        self.register_buffer("fb", _melscale_fbanks(n_stft, f_min, f_max, n_mels, sample_rate, norm, mel_scale))


class _AmplitudeToDB(torch.nn.Module):
    """Parameter- and buffer-free, like torchaudio's; keeps the attribute name of the reference."""

    def __init__(self, stype, top_db):
        super().__init__()
        self.stype, self.top_db = stype, top_db


def _hz_to_mel(freq, mel_scale="htk"):
    """torchaudio.functional._hz_to_mel (2.0.2): HTK 2595 log10(1 + f / 700); Slaney: linear below 1 kHz
    (200 / 3 Hz per mel), logarithmic above (step log(6.4) / 27)."""
    if mel_scale == "htk":
        return 2595.0 * math.log10(1.0 + freq / 700.0)
    f_sp = 200.0 / 3
    mels = freq / f_sp
    min_log_hz = 1000.0
    if freq >= min_log_hz:
        mels = min_log_hz / f_sp + math.log(freq / min_log_hz) / (math.log(6.4) / 27.0)
    return mels


def _mel_to_hz(mels, mel_scale="htk"):
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (mels / 2595.0) - 1.0)
    f_sp = 200.0 / 3
    freqs = f_sp * mels
    min_log_mel = 1000.0 / f_sp
    log_t = mels >= min_log_mel
    freqs[log_t] = 1000.0 * torch.exp((math.log(6.4) / 27.0) * (mels[log_t] - min_log_mel))
    return freqs


def _melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate, norm=None, mel_scale="htk"):
    """torchaudio.functional.melscale_fbanks (2.0.2) -> [n_freqs, n_mels]; norm='slaney': every triangle divided by the
    width of its mel band (area normalisation)."""
    all_freqs = torch.linspace(0, sample_rate // 2, n_freqs)
    m_pts = torch.linspace(_hz_to_mel(f_min, mel_scale), _hz_to_mel(f_max, mel_scale), n_mels + 2)
    f_pts = _mel_to_hz(m_pts, mel_scale)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts.unsqueeze(0) - all_freqs.unsqueeze(1)
    down = (-1.0 * slopes[:, :-2]) / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    fb = torch.clamp(torch.min(down, up), min=0.0)
    if norm == "slaney":
        fb = fb * (2.0 / (f_pts[2:n_mels + 2] - f_pts[:n_mels])).unsqueeze(0)
    return fb.contiguous()


def _create_dct(n_mfcc, n_mels, norm="ortho"):
    """torchaudio.functional.create_dct -> [n_mels, n_mfcc] (norm None: the DCT-II scaled by 2)."""
    n = torch.arange(float(n_mels))
    k = torch.arange(float(n_mfcc)).unsqueeze(1)
    dct = torch.cos(math.pi / float(n_mels) * (n + 0.5) * k)
    if norm is None:
        dct *= 2.0
    else:
        dct[0] *= 1.0 / math.sqrt(2.0)
        dct *= math.sqrt(2.0 / float(n_mels))
    return dct.t().contiguous()


class ConcaternatedSTFTFeatures(STFT, torch.nn.Module):
    @classmethod
    def finalize_dogmatic_config(cls, config):               # feature_extractor.py:308-321
        for fe in ["fe1", "fe2"]:
            if isinstance(config.get(fe), dict):
                for k in ("size", "shift", "pad", "fading", "window", "causal"):
                    if k in config:
                        config[fe][k] = config[k]
                if config.get("window_length") is not None:
                    config[fe]["window_length"] = config["window_length"]

    def __init__(self, fe1, fe2, output_size=None, size=1024, shift=256, window="blackman",
                 window_length=None, pad=True, fading=True, causal=False):
        torch.nn.Module.__init__(self)
        self._tmp = [fe1, fe2]
        STFT.__init__(self, size=size, shift=shift, window_length=window_length, pad=pad,
                      fading=fading, output_size=output_size, window=window)
        self.fe1, self.fe2 = fe1, fe2
        # causal (this project's own keyword) reaches the parts through finalize_dogmatic_config; what the
        # object IS follows from the parts it holds
        self.causal = bool(getattr(fe1, "causal", False) and getattr(fe2, "causal", False))
        if causal and not self.causal:
            raise ValueError("ConcaternatedSTFTFeatures(causal=True) needs causal parts: build fe1 and fe2 with causal=True "
                             "(from a config the key is propagated to them)")

    def _get_output_size(self, output_size):
        fe1, fe2 = self._tmp
        if output_size is None:
            return fe1._get_output_size(None) + fe2._get_output_size(None)
        return output_size

    def stft_to_feature(self, stft_signals, state=None, return_state=False):
        """Both parts causal: ``state`` [B, 2] / return_state as in the parts (one state serves both: the running max |X|
        and the running max dB)."""
        X = stft_signals
        if X.dim() == 2:
            out = self.stft_to_feature(X[None], state, return_state)
            return (out[0][0], out[1]) if return_state else out[0]
        fused = isinstance(self.fe1, TorchMFCC) and isinstance(self.fe2, Log1pMaxNormAbsSTFT) and X.dim() == 3
        if fused and self.causal and self.fe2.statistics_axis == "tf":
            out, _, state = H.feat_causal_fwd(X, self.fe1.fb, self.fe1.dct_mat, self.fe1.n_mfcc, self.fe1._db_arg,
                                              state=state)
            return (out, state) if return_state else out
        # TorchMFCC beside a feature of csrc/specfeat.hip (AbsSTFT and its subclasses), both causal or neither: feat_fwd
        # lays out the final [B, T, ld] buffer and writes the MFCC columns (and a log1p block it cannot skip), then the
        # spectral kernel writes columns [n_mfcc, n_mfcc + F) over that block in place -- no concat, no third buffer.
        # Causal: the carried state is the pair (TorchMFCC's, the spectral part's).
        placed = isinstance(self.fe1, TorchMFCC) and isinstance(self.fe2, AbsSTFT) and X.dim() == 3 \
            and self.fe1.causal == self.fe2.causal
        if placed:
            self.fe1._check_feature_bins()
            X3, _ = _spectrum3(X)
            if self.causal:
                if state is None:
                    state = (None, None)
                if not isinstance(state, (tuple, list)) or len(state) != 2:
                    got = f"{state.dtype} {tuple(state.shape)}" if isinstance(state, torch.Tensor) else type(state).__name__
                    raise ValueError(f"ConcaternatedSTFTFeatures(TorchMFCC, {type(self.fe2).__name__}): the carried state is "
                                     f"the pair (state of fe1, state of fe2) an earlier call returned, got {got}")
                out, _, s1 = H.feat_causal_fwd(X3, self.fe1.fb, self.fe1.dct_mat, self.fe1.n_mfcc, self.fe1._db_arg,
                                               state=state[0])
                _, s2 = self.fe2._feature(X3, state[1], out=out, col0=self.fe1.n_mfcc)
                return (out, (s1, s2)) if return_state else out
            _no_state(self, state)
            out, _ = H.feat_fwd(X3, self.fe1.fb, self.fe1.dct_mat, self.fe1.n_mfcc, self.fe1._db_arg)
            self.fe2._feature(X3, None, out=out, col0=self.fe1.n_mfcc)
            return (out, None) if return_state else out
        if self.causal:
            # (causal parts the fused kernel does not cover -- 'f' statistics: each part with the state, whose columns are
            # disjoint: the MFCC's dB maximum, the log1p's |X| maximum)
            o1, s1 = self.fe1.stft_to_feature(X, state, True)
            o2, s2 = self.fe2.stft_to_feature(X, state, True)
            if s2 is not None and s1 is not None:
                s1 = torch.stack([s2[:, 0], s1[:, 1]], dim=1)
            out = torch.concat([o1, o2], dim=-1)
            return (out, s1) if return_state else out
        _no_state(self, state)
        if fused and not self.fe1.causal and not self.fe2.causal:
            # one fused pass pair writes [mfcc | log1p] side by side (feature_extractor.py:352-360)
            out, _ = H.feat_fwd(X, self.fe1.fb, self.fe1.dct_mat, self.fe1.n_mfcc, self.fe1._db_arg,
                                statistics_axis=self.fe2.statistics_axis)
        else:
            out = torch.concat([self.fe1.stft_to_feature(X), self.fe2.stft_to_feature(X)], dim=-1)
        return (out, None) if return_state else out
