"""Online separation: audio chunks in, separated audio chunks out (this project's own).

``Model.online(aux)`` -> ``OnlineSeparator``.  A push of ``Tc * shift`` samples runs, without gradients,

    streaming STFT (carried: the last size - shift samples)  ->  causal features (carried: two running maxima)
    ->  MaskEstimator_v2's chunk trunk (carried: every layer's (h, c))  ->  fused mask head + streaming inverse STFT
    (carried: the partial sums of the three pending hops)

and returns the samples those frames complete.  With the enhancer `OnlineMVDR` a push holds D channels:
all of them go through the streaming STFT, features and trunk read the reference channel, and the tail is sigmoid ->
frame-recursive MVDR (carried: the two PSDs per speaker and bin, a fifth state) -> streaming inverse STFT.  With
`OnlineMVDR(pre_wpe=OnlineWPE(...))` the frames are dereverberated by the recursive WPE between the STFT and
the beamformer -- the masks still come from the raw reference channel -- and the fifth state is the pair (the WPE's
inverse correlation matrices, taps and frame ring; the PSDs).  The algorithmic latency is size - shift samples (48 ms at
16 kHz); the dereverberation adds none, its taps reach back only.  The frame / hop bookkeeping is `schedule`, a pure
function.
"""
from collections import namedtuple

import torch

Step = namedtuple("Step", "frames skip samples")


def _step(frames_before, frames, shift):
    """A call of `frames` frames behind `frames_before`: (hops of the call that lie before the utterance's first sample,
    samples it completes).  Hop h of the utterance sums frames h .. h + 3: frame t completes hop t - 3."""
    skip = max(0, 3 - frames_before)
    return skip, max(frames - skip, 0) * shift


def schedule(pushes, N, shift=256, size=1024):
    """The calls of a stream over an utterance of N samples: `pushes` = frames (hops of `shift` samples) per push, in
    order; the rest of the utterance -- fewer than `shift` samples -- goes to flush.  -> [Step(frames, skip, samples)] per
    push and, last, for the flush: a push of Tc frames yields exactly Tc frames; the first three frames of a stream
    complete no hop; flush transforms the frames the trailing fade and the padding still owe -- (size - shift) / shift of
    them, one more for a ragged rest -- and ends the output at sample N.  sum(samples) == N."""
    if size % shift:
        raise ValueError(f"size = {size} must be a multiple of shift = {shift}")
    pushes = [int(p) for p in pushes]
    if any(p < 1 for p in pushes):
        raise ValueError(f"a push holds at least one frame: {pushes}")
    pushed = sum(pushes)
    rest = N - pushed * shift
    if not 0 <= rest < shift:
        raise ValueError(f"{pushed} pushed hops of {shift} leave {rest} of {N} samples: flush takes 0 .. {shift - 1}")
    if N < 1:
        raise ValueError("an utterance holds at least one sample")
    total = -(-N // shift) + (size - shift) // shift            # fe.frames(N): full fading, pad=True
    steps, seen, out = [], 0, 0
    for p in pushes:
        skip, m = _step(seen, p, shift)
        steps.append(Step(p, skip, m))
        seen, out = seen + p, out + m
    skip, _ = _step(seen, total - seen, shift)
    steps.append(Step(total - seen, skip, N - out))
    return steps


def check_online(model, aux=None):
    """What `Model.online` refuses, from the arguments alone: nothing is launched."""
    from . import enhancer as _enh
    me, fe = model.mask_estimator, model.fe
    if getattr(me, "rnn_typ", None) != "lstm":
        raise ValueError(f"online separation needs a causal trunk, rnn_typ='lstm': {getattr(me, 'rnn_typ', None)!r} reads "
                         "the future of every frame")
    if not getattr(fe, "causal", False):
        raise ValueError(f"online separation needs causal features: {type(fe).__name__} normalises with utterance-wide "
                         "statistics (the maximum of |X| over the utterance, the dB floor of the batch); build it with "
                         "causal=True and train with it")
    if getattr(me, "nmask", 1) != 1:
        raise NotImplementedError(f"online separation with nmask = {me.nmask}: the streaming tail takes one mask per speaker")
    if not isinstance(model.enhancer, (_enh.Masking, _enh.OnlineMVDR)):
        raise NotImplementedError(f"online separation with the enhancer {type(model.enhancer).__name__}: only Masking has a "
                                  "streaming tail (multi-channel / beamforming enhancers are not built)")
    if getattr(me, "output_resolution", "tf") != "tf":
        raise NotImplementedError(f"online separation with output_resolution = {me.output_resolution!r}: the streaming "
                                  "tail reads a logit per bin")
    if not hasattr(fe, "_check_stream"):
        raise NotImplementedError(f"online separation with {type(fe).__name__}: no STFT to stream")
    fe._check_stream()
    me._check_chunkable(aux)


class OnlineSeparator:
    """``push(x)``: x [B, n] or [n] float32 on the device, n a positive multiple of shift -> [B, K, m] (un-batched:
    [K, m]), the samples this push completes: (Tc - 3) * shift for the first (none while fewer than four frames
    exist), Tc * shift afterwards.  ``flush(x_last=None)``: the ragged rest (fewer than shift samples) -> the remaining
    samples; the concatenation has exactly the utterance's length and `push` raises afterwards.  ``last``: the last
    call's `Output` (masks, VAD), formed when read.  record=True keeps every call's ``Observation`` and ``Input`` (and
    with OnlineMVDR ``logit``, ``mask``, ``Estimate``; with its pre_wpe also ``Dereverberated``, the frames it beamformed).
    With the enhancer `OnlineMVDR` x is [B, D, n] (un-batched: [D, n]), ``reference_channel`` names the channel the
    features are taken from and the beamformer is steered to (Masking ignores it)."""

    def __init__(self, model, aux, record=False, reference_channel=0, grad=False, detach=True):
        from . import enhancer as _enh
        check_online(model, aux)
        if grad and isinstance(model.enhancer, _enh.OnlineMVDR):
            raise NotImplementedError("Model.online(grad=True) with the enhancer OnlineMVDR: the frame-recursive beamformer "
                                      "is evaluation-time and has no backward; train the stream with Masking")
        self.grad, self.detach = bool(grad), bool(detach)
        self.model, self.fe, self.me = model, model.fe, model.mask_estimator
        self._aux = aux
        self._tail = self._feat = self._trunk = self._ola = None       # the four carried states
        self._bf = model.enhancer if isinstance(model.enhancer, _enh.OnlineMVDR) else None
        self._psd = None                    # the beamformer's fifth: Phi_s, Phi_n (with pre_wpe: the pair of both states)
        self._ref = int(reference_channel)
        if self._bf is not None and not 0 <= self._ref < 8:
            raise ValueError(f"reference_channel = {reference_channel}: the beamformer takes at most 8 channels")
        self._lead = None                                              # the axes of a push in front of the samples
        self.frames = self.samples_in = self.samples_out = 0
        self.closed = False
        self._res = self._un = None
        self.record = [] if record else None

    def _run_bf(self, x, frames, num_samples=None):
        """x [B, D, n]: STFT of all channels (rows B * D), features and trunk on the reference channel, then
        sigmoid -> online MVDR -> streaming inverse STFT."""
        fe = self.fe
        if not self._ref < x.shape[1]:
            raise ValueError(f"reference_channel = {self._ref} of {x.shape[1]} channels")
        with torch.no_grad():
            X, self._tail = fe.stft_chunk(x, self._tail)                                     # [B, D, Tc, F]
            feat, self._feat = fe.stft_to_feature(X[:, self._ref].contiguous(), self._feat, True)
            aux = None if self._trunk is not None else ([self._aux] if self._un else self._aux)
            res, _, self._trunk = self.me._chunk_logits(feat.to(torch.float32), aux, self._trunk)
            mask = self.me._output(res).mask                                                 # [B, K, 1, Tc, F]
            enh, self._psd, Xd = self._bf.chunk(mask, X, self._psd, self._ref, with_observation=True)
            skip, _ = _step(self.frames, frames, fe.shift)
            y, self._ola = fe.istft_chunk(enh, self._ola, skip, num_samples)
        self._res = res
        if self.record is not None:
            self.record.append({"Observation": X, "Input": feat, "logit": res[0], "mask": mask, "Estimate": enh})
            if self._bf.pre_wpe is not None:
                self.record[-1]["Dereverberated"] = Xd
        self.frames += frames
        self.samples_out += y.shape[-1]
        return y

    def _run(self, x, frames, num_samples=None):
        self._lead = tuple(x.shape[:-1])
        if self._bf is not None:
            return self._run_bf(x, frames, num_samples)
        if self.grad:
            return self._run_grad(x, frames, num_samples)
        fe = self.fe
        with torch.no_grad():
            X, self._tail = fe.stft_chunk(x, self._tail)                                     # [B, Tc, F]
            feat, self._feat = fe.stft_to_feature(X, self._feat, True)
            # (an un-batched stream is a batch of one: its aux is one entry, as in forward_chunk)
            aux = None if self._trunk is not None else ([self._aux] if self._un else self._aux)
            res, _, self._trunk = self.me._chunk_logits(feat.to(torch.float32), aux, self._trunk)
            skip, _ = _step(self.frames, frames, fe.shift)
            # the head's rows as they are ([B,K,Tc,F], explicit_vad: [B,K,Tc,F+1]) into the fused tail: no mask, no masked
            # spectrum
            y, self._ola = fe.masked_istft_chunk(res[0], X, self._ola, skip, num_samples)
        self._res = res
        if self.record is not None:
            self.record.append({"Observation": X, "Input": feat, "logit": res[0]})
        self.frames += frames
        self.samples_out += y.shape[-1]
        return y

    def _run_grad(self, x, frames, num_samples=None):
        """`_run` as a training step: STFT and features are data, without gradients; the trunk runs through
        `_chunk_logits(grad=True)` and the tail through the differentiable chunk, so y is in the graph.  detach: the layer
        states, the embedding and the overlap-add carry are cut after the call (truncated BPTT)."""
        fe = self.fe
        with torch.no_grad():
            X, self._tail = fe.stft_chunk(x, self._tail)                                     # [B, Tc, F]
            feat, self._feat = fe.stft_to_feature(X, self._feat, True)
        aux = None if self._trunk is not None else ([self._aux] if self._un else self._aux)
        res, _, self._trunk = self.me._chunk_logits(feat.to(torch.float32), aux, self._trunk, grad=True, detach=self.detach)
        skip, _ = _step(self.frames, frames, fe.shift)
        y, ola = fe.masked_istft_chunk(res[0], X, self._ola, skip, num_samples, differentiable=True)
        self._ola = ola.detach() if self.detach else ola
        self._res = res
        if self.record is not None:
            self.record.append({"Observation": X, "Input": feat, "logit": res[0]})
        self.frames += frames
        self.samples_out += y.shape[-1]
        return y

    def _batched(self, x):
        nd = 1 if self._bf is None else 2
        if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or x.dim() not in (nd, nd + 1):
            raise ValueError("push / flush take a float32 tensor [B, n] or [n] on the device" if nd == 1 else
                             "push / flush take a float32 tensor [B, D, n] or [D, n] on the device (OnlineMVDR)")
        un = x.dim() == nd
        if self._un is None:
            self._un = un
        elif un != self._un:
            raise ValueError("a stream is batched or un-batched from its first call on")
        return x[None] if un else x

    def push(self, x):
        if self.closed:
            raise RuntimeError("push after flush: the stream is closed (Model.online(aux) opens another)")
        x = self._batched(x)
        n, shift = x.shape[-1], self.fe.shift
        if n < shift or n % shift:
            raise ValueError(f"push takes a positive multiple of shift = {shift} samples, not {n} (flush takes the rest)")
        y = self._run(x, n // shift)
        self.samples_in += n
        return y[0] if self._un else y

    def flush(self, x_last=None):
        if self.closed:
            raise RuntimeError("flush after flush: the stream is closed")
        fe = self.fe
        r = 0
        if x_last is not None:
            x_last = self._batched(x_last)
            r = x_last.shape[-1]
            if r >= fe.shift:
                raise ValueError(f"flush takes the rest of the utterance, fewer than shift = {fe.shift} samples, not {r}")
        N = self.samples_in + r
        if N < 1:
            raise ValueError("flush of an empty stream: nothing was pushed")
        if self._tail is None and not r:
            raise ValueError("flush without samples on a stream that never saw any")
        owed = fe.frames(N) - self.frames                    # the trailing fade and the padding: 3 frames, or 4
        lead = tuple(x_last.shape[:-1]) if r else self._lead
        device = x_last.device if r else self._tail.device
        x = torch.zeros(*lead, owed * fe.shift, device=device, dtype=torch.float32)
        if r:
            x[..., :r] = x_last
        y = self._run(x, owed, num_samples=N - self.samples_out)
        self.samples_in, self.closed = N, True
        return y[0] if self._un else y

    @property
    def last(self):
        """The `Output` of the last call's frames (mask, logit or vad_mask / vad_logit, embedding)."""
        if self._res is None:
            return None
        with torch.no_grad():
            return self.me._output(self._res)


def stream_loss_step(model, ex_audio, targets, aux, loss, pushes, detach=True):
    """One batch as a stream: ex_audio [B, N] is pushed through ``model.online(aux, grad=True,
    detach=detach)`` in `pushes` (frames per push; the rest, fewer than shift samples, goes to flush) and every call's
    samples meet their part of targets [B, K, N] in ``loss(y_chunk, target_chunk) -> [B]`` -- a TimeDomain loss module
    or any callable.  Calls that complete no sample are skipped.  detach=True: ``backward()`` of the call's mean loss
    after every call (truncated BPTT, memory bounded by one chunk); detach=False: one ``backward()`` of the sum after
    flush, the whole utterance's gradient.  -> the per-call losses [B], detached, in order.  The gradients accumulate in
    the parameters' ``.grad``: no optimizer step and no zero_grad inside."""
    N, shift = ex_audio.shape[-1], model.fe.shift
    schedule(pushes, N, shift, model.fe.size)                  # (raises on pushes that do not fit the utterance)
    stream = model.online(aux, grad=True, detach=detach)
    losses, total, pos, at = [], None, 0, 0
    calls = [int(p) * shift for p in pushes] + [None]
    for n in calls:
        if n is None:
            y = stream.flush(ex_audio[..., at:] if at < N else None)
        else:
            y = stream.push(ex_audio[..., at:at + n])
            at += n
        m = y.shape[-1]
        if not m:
            continue
        per = loss(y, targets[..., pos:pos + m].contiguous())
        pos += m
        losses.append(per.detach())
        if detach:
            per.mean().backward()
        else:
            total = per.mean() if total is None else total + per.mean()
    if total is not None:
        total.backward()
    return losses
