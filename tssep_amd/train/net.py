"""MaskEstimator_v2 -- drop-in for tssep/train/net.py:333-986 on the HIP kernels.

Constructor signature, module tree and parameter registration order follow the reference
(net.py:501-669) so ``state_dict`` keys, default-init random streams and ``config.yaml`` are
interchangeable.  The einops layout changes of the reference (speaker combination, final
rearrange, trial mean, speaker un-permutation) are not separate copies here: they are folded
into the producing GEMM's store or one fused map kernel.
"""
import collections
import contextlib
import dataclasses

import numpy as np
import torch

from .. import functional as Fn
from ..configurable import Configurable, resolve
from .rnnp import RNNP_packed


def _signature_repr(module):
    import inspect
    sig = inspect.signature(module.__class__)
    return ", ".join(f"{p.name}={getattr(module, p.name)!r}" for p in sig.parameters.values())


class InstanceNorm(torch.nn.Module):                   # net.py:250-285
    """(x - mean) / std along ``dim``: -1 (one statistic per row) or -2 (the time axis, one per column)."""

    def __init__(self, dim=-1, unbiased=False):
        super().__init__()
        if dim not in Fn.H.INSTNORM_AXES:
            raise NotImplementedError(f"InstanceNorm(dim={dim}): the kernels cover dim -1 and -2")
        self.dim = dim
        self.unbiased = unbiased

    def extra_repr(self):
        return _signature_repr(self)

    def forward(self, x):
        return Fn.instance_norm(x, Fn.H.INSTNORM_AXES[self.dim], 0, self.unbiased)


class InstanceNorm_v2(torch.nn.Module):                # net.py:288-330
    """(x - mean) / (||x - mean|| / sqrt(n)) along one dim (-1 or -2)."""

    def __init__(self, mean_dim=-1, norm_dim=-1):
        super().__init__()
        if mean_dim != norm_dim:
            raise NotImplementedError(f"InstanceNorm_v2(mean_dim={mean_dim}, norm_dim={norm_dim}): "
                                      "one kernel pass takes both statistics along the same dim")
        if mean_dim not in Fn.H.INSTNORM_AXES:
            raise NotImplementedError(f"InstanceNorm_v2(mean_dim={mean_dim}): the kernels cover dim -1 and -2")
        self.mean_dim = mean_dim
        self.norm_dim = norm_dim

    def extra_repr(self):
        return _signature_repr(self)

    def forward(self, x):
        return Fn.instance_norm(x, Fn.H.INSTNORM_AXES[self.mean_dim], 1)


def _stack_aux(aux):
    """(lists of) lists of [E] tensors -> one tensor (net.py:38-42, 840-851)."""
    if isinstance(aux, (tuple, list)):
        return torch.stack([torch.stack(list(a), 0) if isinstance(a, (tuple, list)) else a for a in aux], 0)
    return aux


def _aux_ndim(aux):
    """dimensions of what _stack_aux would return, without building it"""
    n = 0
    while isinstance(aux, (tuple, list)):
        aux, n = aux[0], n + 1
    return n + aux.dim()


class Linear(Configurable, torch.nn.Module):           # net.py:19-43: how i-vectors enter a `mul` model
    def __init__(self, idim, odim, bias=True):
        super().__init__()
        self.idim = idim
        self.odim = odim
        self.bias = bias
        self.net = torch.nn.Linear(idim, odim, bias=bias)

    def forward(self, AuxInput, Input=None, batched=False):
        return Fn.affine(_stack_aux(AuxInput), self.net.weight, self.net.bias)


class AuxNet(Configurable, torch.nn.Module):           # net.py:46-158
    """SpeakerBeam-style auxiliary network: three Linear layers over the enrolment frames of every speaker and the mean
    over time.  The reference pads the sequences and takes a length-aware mean; padding rows never reach its result, so
    the sequences are PACKED here (concatenated, one device prefix of their lengths) and nothing is padded."""

    @classmethod
    def finalize_dogmatic_config(cls, config):
        if config.get("odim") is None:
            config["odim"] = config.get("idim")

    def __init__(self, idim, odim=None, normalizer: "InstanceNorm" = None):
        super().__init__()
        if odim is None:
            odim = idim
        elif idim != odim:
            raise NotImplementedError(odim, idim)
        if normalizer is not None:
            if not isinstance(normalizer, (InstanceNorm, InstanceNorm_v2)):
                raise NotImplementedError(f"AuxNet normalizer {type(normalizer).__name__}")
            if getattr(normalizer, "dim", getattr(normalizer, "mean_dim", None)) != -1:
                raise NotImplementedError(
                    "AuxNet normalizer along the time axis: the reference takes its statistics over the PADDED "
                    "sequences (zeros behind the shorter ones included); only dim=-1 is the same on packed rows")
        self.idim, self.odim = idim, odim
        self.net = Sequential(*[e for e in [normalizer] if e is not None],
                              torch.nn.Linear(idim, idim), torch.nn.ReLU(),
                              torch.nn.Linear(idim, idim), torch.nn.ReLU(),
                              torch.nn.Linear(idim, idim))

    def forward(self, AuxInput, Input=None, batched=False):
        h = AuxInput
        if batched:
            assert len({len(a) for a in AuxInput}) == 1, [len(a) for a in AuxInput]
            h = [e for a in AuxInput for e in a]
        lengths = [int(e.shape[0]) for e in h]
        x = torch.cat([e.reshape(-1, self.idim) for e in h], 0)
        row0 = Fn.H.segment_rows(lengths, x.device)           # built on the host from the lengths, one copy
        mods = list(self.net)
        if not isinstance(mods[0], torch.nn.Linear):
            x = mods[0](x).detach()
        y = Fn.aux_mlp(x, row0, len(lengths), [m for m in mods if isinstance(m, torch.nn.Linear)])
        if batched:
            y = y.reshape(len(AuxInput), -1, y.shape[-1])
        return y


@dataclasses.dataclass
class Output:                      # net.py:240-247
    mask: torch.Tensor
    logit: torch.Tensor
    embedding: torch.Tensor = None
    vad_mask: torch.Tensor = None
    vad_logit: torch.Tensor = None


@dataclasses.dataclass
class ChunkState:
    """What MaskEstimator_v2.forward_chunk / train_chunk carries from one chunk to the next (opaque to its callers)."""
    layers: list             # per recurrent layer, pre-net first: (h, c), each [1, N, units]
    perm: torch.Tensor       # speaker permutation and its inverse, device int32 [B, K] (None: speakers in their order)
    iperm: torch.Tensor
    embedding: torch.Tensor  # [B, K, E], as the conditioning reads it
    K: int
    frames: int              # consumed so far


class Sequential(torch.nn.Sequential):        # net.py:190-237 (container role only)
    pass


class _Marker(torch.nn.Module):
    """Parameter-free stand-in for the einops layers of the reference post-net (keeps the
    ``post_net`` key numbering: rearrange2, linear2, rearrange3 ...)."""

    def __init__(self, pattern):
        super().__init__()
        self.pattern = pattern

    def extra_repr(self):
        return repr(self.pattern)


class MaskEstimator_v2(Configurable, torch.nn.Module):
    @classmethod
    def finalize_dogmatic_config(cls, config):        # net.py:342-499
        aux_net = config.get("aux_net")
        if aux_net is None:
            if config.get("combination", "cat") == "cat" and config.get("aux_net_output_size") is None:
                config["aux_net_output_size"] = 100            # i-vectors (net.py:488-490)
        elif isinstance(aux_net, dict):                        # net.py:491-499
            if issubclass(resolve(aux_net["factory"]), AuxNet):
                aux_net["idim"] = config.get("odim") or config.get("idim")
                if aux_net.get("odim") is None:
                    aux_net["odim"] = aux_net["idim"]
            if config.get("combination", "cat") == "cat" and "odim" in aux_net:
                config["aux_net_output_size"] = aux_net["odim"]

    def __init__(self, *, idim=80, odim=None, layers=3, units=300, projs=320, dropout=0, nmask=1,
                 pre_net="RNNP", aux_net=None, aux_net_output_size=None, combination: str = "cat",
                 ts_vad=False, output_resolution: str = "tf", random_speaker_order=True,
                 num_averaged_permutations=1, input_normalizer=None, aux_normalizer=None,
                 explicit_vad=False, aux_stride=1, rnn_typ="blstm"):
        super().__init__()
        if rnn_typ not in ("blstm", "lstm"):
            raise ValueError(f"rnn_typ={rnn_typ!r}: 'blstm' | 'lstm'")
        self.rnn_typ = rnn_typ                    # this project's keyword: 'lstm' = every recurrent layer causal (forward_chunk)
        if not isinstance(aux_stride, int) or isinstance(aux_stride, bool) or aux_stride < 1:
            raise ValueError(f"aux_stride={aux_stride!r}: a positive number of frames per row of a frame-wise embedding")
        self.aux_stride = aux_stride              # this project's keyword (frame-wise embeddings at their own frame rate)
        if odim is None:
            odim = idim
        for name, norm in (("input_normalizer", input_normalizer), ("aux_normalizer", aux_normalizer)):
            if norm is not None and not isinstance(norm, (InstanceNorm, InstanceNorm_v2)):
                raise NotImplementedError(f"{name}: {type(norm).__name__} (InstanceNorm / InstanceNorm_v2 are built)")
        if aux_net is not None and not isinstance(aux_net, (Linear, AuxNet)):
            raise NotImplementedError(f"aux_net: {type(aux_net).__name__} (Linear / AuxNet are built)")
        assert aux_net is None or aux_normalizer is None, (aux_normalizer, "Not clear, whether before or after")   # net.py:834
        if explicit_vad and output_resolution == "t":
            raise AssertionError("explicit_vad needs output_resolution='tf' (net.py:643)")
        if not isinstance(nmask, int) or isinstance(nmask, bool) or nmask < 1:
            raise ValueError(f"nmask={nmask!r}: a positive number of masks per speaker")
        if explicit_vad and nmask != 1:
            raise NotImplementedError(f"explicit_vad=True with nmask={nmask}: the gate column is built for one mask per speaker, "
                                      "and the reference's SignalAndVADSigmoidBCE cannot consume more (net.py:969-979)")
        self.odim, self.nmask = odim, nmask
        self.output_resolution = output_resolution
        self.random_speaker_order = random_speaker_order
        self.num_averaged_permutations = num_averaged_permutations
        self.ts_vad = ts_vad
        self.input_normalizer, self.aux_normalizer = input_normalizer, aux_normalizer
        self.explicit_vad = bool(explicit_vad)
        self.layers, self.projs = layers, projs
        if not self.ts_vad:
            assert self.num_averaged_permutations == 1, (self.ts_vad, self.num_averaged_permutations)
        if pre_net == "RNNP":
            self.pre_net = RNNP_packed(idim=idim, elayers=1, cdim=units, hdim=odim, dropout=dropout,
                                       typ=rnn_typ)
        elif pre_net in [None, False]:
            raise NotImplementedError("pre_net=None (every shipped config uses 'RNNP')")
        else:
            raise ValueError(pre_net)
        self.aux_net = aux_net
        self.combination = combination

        data = collections.OrderedDict()
        counter = [0]

        def put(key, value):                       # SequentialDict of net.py:562-578
            for counter[0] in range(counter[0], 100):
                k = f"{key}{counter[0]}"
                if k not in data:
                    data[k] = value
                    return
            raise RuntimeError(key)

        ts_factor = 1
        if combination == "cat":
            if aux_net is None:
                assert aux_net_output_size is not None, (combination, aux_net_output_size)
            else:                                                # net.py:590-595
                assert aux_net_output_size == aux_net.odim, (combination, aux_net_output_size, aux_net)
            first_birnn_idim = odim + aux_net_output_size
        elif combination in ["mul"]:
            first_birnn_idim = odim
        elif combination == "film":
            raise NotImplementedError(combination)          # net.py:875-878
        else:
            raise ValueError(combination)
        for l in range(layers):
            if l == layers - 1 and ts_vad is not False:
                assert 2 < ts_vad < 20, ts_vad               # net.py:607
                put("rearrange", _Marker("... spk time feature -> ... 1 time (spk feature)"))
                ts_factor = ts_vad
            put("birnn", RNNP_packed(idim=(first_birnn_idim if l == 0 else projs) * ts_factor,
                                     elayers=1, cdim=units, hdim=projs, dropout=dropout, typ=rnn_typ))
            if l < layers - 1:
                put("dropout", torch.nn.Dropout(p=dropout))
                put("activation", torch.nn.Tanh())
        if output_resolution == "tf":
            final_out_features = (odim + int(self.explicit_vad)) * nmask * ts_factor    # net.py:630
        elif output_resolution == "t":
            final_out_features = nmask * ts_factor
        else:
            raise ValueError(output_resolution)
        put("linear", torch.nn.Linear(in_features=projs, out_features=final_out_features))
        put("rearrange", _Marker("final einops rearrange / reduce-repeat (net.py:631-659)"))
        self.post_net = Sequential(data)
        self.final_activation = torch.nn.Sigmoid()
        self._birnn_keys = [k for k in data if k.startswith("birnn")]
        self._dropout_keys = [k for k in data if k.startswith("dropout")]      # the one behind birnn l, l < layers - 1
        self._linear_key = [k for k in data if k.startswith("linear")][0]
        if ts_vad is not False and layers < 2:
            raise NotImplementedError("ts_vad with a single post-net layer")

    @property
    def _birnns(self):
        return [self.post_net._modules[k] for k in self._birnn_keys]

    @property
    def _dropouts(self):
        return [self.post_net._modules[k] for k in self._dropout_keys]

    @property
    def _linear(self):
        return self.post_net._modules[self._linear_key]

    def extra_repr(self) -> str:
        return f"combination={self.combination!r},"

    # hook for hipGraph replay (tssep_amd.train.graph.GraphedStep): a callable (B, K, device) ->
    # (perm, iperm) device int32 [B, K] that replaces the host draw + H2D copy below
    permutation_source = None

    @staticmethod
    def draw_permutations(B, K):
        """One np.random.permutation(K) per batch entry, in batch order, from the GLOBAL numpy RNG
        (net.py:824-826) -> int32 [2, B, K]: the permutations and their inverses (net.py:827-831)."""
        perm = np.stack([np.random.permutation(K) for _ in range(B)])
        return np.stack([perm, np.argsort(perm, axis=-1)]).astype(np.int32)

    def _speaker_permutations(self, B, K, dev):
        if self.permutation_source is not None:
            return self.permutation_source(B, K, dev)
        # kernels want: output index of the speaker at shuffled position s == perm[b][s]
        both = torch.as_tensor(self.draw_permutations(B, K)).to(dev)              # one H2D copy
        return both[0], both[1]

    # ----------------------------------------------------------------------------------
    def logits(self, xs, aux):
        """-> (logit [B,K,T,F], embedding [B,K,1,E]; a frame-wise aux [B,K,Ta,E] comes back as it entered the conditioning,
        net.py:866-867: frame t is conditioned on row t // aux_stride).  explicit_vad: logit [B,K,T,F+1], the VAD logit at column 0 of
        every row and the mask logits behind it (net.py:969-979 slices them apart).  nmask > 1: (logit [B,K,M,T,F], mask
        [B,K,M,T,F], embedding) -- the fused two-mask tail computes the sigmoid in the pass that lays the logit out."""
        if xs.dim() == 2:
            return tuple(r[0] for r in self.logits(xs[None], [aux]))
        assert xs.dim() == 3, xs.shape
        aux, perm_d, iperm_d, K = self._embedding(aux, xs.shape[0], xs.shape[1], xs.device)
        return self._trunk(xs, aux, perm_d, iperm_d, K)

    def _embedding(self, aux, B, T, dev):
        """aux as the caller gave it -> (the embedding the conditioning reads, [B,K,E] or frame-wise [B,K,Ta,E]; perm,
        iperm device int32 [B,K] or None; K): the speaker permutation (net.py:823-831), aux_net / aux_normalizer."""
        ragged = isinstance(self.aux_net, AuxNet)       # enrolment sequences [T_i, idim]: lists, shuffled on the host
        if ragged:
            aux = [list(a) for a in aux]
        else:
            aux = _stack_aux(aux)
        K = len(aux[0]) if ragged else aux.shape[1]
        if not ragged and aux.dim() == 4:               # an embedding per speaker AND frame (net.py:866-867)
            if aux.shape[0] != B:
                raise ValueError(f"frame-wise embeddings {tuple(aux.shape)} for a batch of {B}")
            if self.aux_net is not None:
                raise NotImplementedError(f"aux_net={type(self.aux_net).__name__} on frame-wise embeddings "
                                          f"{tuple(aux.shape)}: aux_net maps one enrolment to one embedding per speaker")
            Fn.H.cond_frames(T, aux.shape[2], self.aux_stride)       # ValueError, before anything is launched
        elif not ragged and aux.dim() != 3:
            raise ValueError(f"aux {tuple(aux.shape)}: [B, K, E] or frame-wise [B, K, Ta, E]")
        elif self.aux_stride != 1:
            raise ValueError(f"aux_stride={self.aux_stride} with one embedding per speaker and utterance "
                             f"({'enrolment lists' if ragged else tuple(aux.shape)}): it is the frame rate of a frame-wise aux [B, K, Ta, E]")
        perm_d = iperm_d = None
        if self.random_speaker_order:                   # the RAW aux entries are shuffled (net.py:823-831)
            perm_d, iperm_d = self._speaker_permutations(B, K, dev)
            if ragged:
                perm_h = perm_d.tolist()
                aux = [[a[i] for i in q] for a, q in zip(aux, perm_h)]
            else:
                # shuffled aux[b, s] = aux[b, perm[b, s]]: one gather for the whole batch
                idx = perm_d.long().reshape(B, K, *([1] * (aux.dim() - 2))).expand(-1, -1, *aux.shape[2:])
                aux = torch.gather(aux, 1, idx)
        if self.aux_net is not None:                    # net.py:833-838
            aux = self.aux_net(aux, None, batched=True)
        else:
            aux = aux.to(torch.float32)
            if self.aux_normalizer is not None:         # net.py:852-853
                aux = self.aux_normalizer(aux)
        return aux.contiguous(), perm_d, iperm_d, K

    def _trunk(self, xs, aux, perm_d, iperm_d, K, prev=None, states=None, state_grad=False):
        """xs [B,T,idim] and what _embedding returned -> `logits`' result.  prev / states: the per-layer (h, c) lists of
        RNNP_packed.forward_rows, pre-net first (forward_chunk: without gradients; train_chunk: state_grad, with them)."""
        B, T = xs.shape[0], xs.shape[1]
        framewise = aux.dim() == 4
        carry = prev is not None or states is not None

        def st(i):      # keywords of layer i's forward_rows: its own slice of the state lists
            if not carry:
                return {}
            return dict(prev_state=None if prev is None else prev[i:i + 1], states=states,
                        **(dict(state_grad=True) if state_grad else {}))
        if self.input_normalizer is not None:           # net.py:858-859
            xs = self.input_normalizer(xs)
        if self.ts_vad is not False:
            assert K == self.ts_vad, (K, self.ts_vad)
        trials = self.num_averaged_permutations
        F = self.odim + int(self.explicit_vad)         # the head's columns per speaker
        pre = self.pre_net.forward_rows(xs.reshape(B * T, xs.shape[-1]), B, T, **st(0))       # [B*T, odim]
        h = Fn.condition(pre, aux, B, K, T, trials, self.combination, self.aux_stride)     # rows (b,tr,k,t)
        nb = len(self._birnns)
        # the Tanh between two post-net modules runs forward in the producer's projection store and backward in
        # the consumer's d(input) GEMM store (functional.rnnp_layer): `fold` = both ends agree on it.  A Tanh behind an
        # ACTIVE dropout site (the `dropout<l>` container in training mode, p > 0) is one masked pass of its own instead
        prev_tanh = 0
        dropouts = self._dropouts
        for l, birnn in enumerate(self._birnns):
            last = l == nb - 1
            site = None if last else dropouts[l]
            fold = (not last) and birnn.hdim % 4 == 0 and Fn.H.FOLD_TANH and not birnn.site_p(site)
            if last and self.ts_vad is not False:
                h = birnn.forward_rows(h, B * trials, T, in_tanh=prev_tanh, **st(l + 1))        # combined input
            else:
                nxt_combined = (l == nb - 2) and self.ts_vad is not False
                h = birnn.forward_rows(h, B * trials * K, T, final_act=0 if last else 1,
                                       combine=K if nxt_combined else 0, in_tanh=prev_tanh, next_folds=fold,
                                       final_dropout=site, **st(l + 1))
                prev_tanh = (K if nxt_combined else 1) if fold else 0
        Fr = F if self.output_resolution == "tf" else 1
        if self.nmask > 1:
            logit, mask = Fn.head_masks(h, self._linear, perm_d, iperm_d, B, K, self.nmask, T, F, trials, Fr,
                                        spk_rows=self.ts_vad is False)
            return logit, mask, aux if framewise else aux.unsqueeze(-2)
        logit = Fn.head(h, self._linear, perm_d, iperm_d, B, K, T, F, trials, Fr,
                        spk_rows=self.ts_vad is False)
        return logit, aux if framewise else aux.unsqueeze(-2)

    def forward(self, xs, aux=None) -> Output:
        return self._output(self.logits(xs, aux))

    def forward_chunk(self, xs, aux, state=None):
        """Online inference of a causal model (rnn_typ='lstm'), without gradients: xs [B, Tc, idim] or [Tc, idim] are the
        NEXT Tc >= 1 feature frames of the utterance(s), `state` what the previous call returned (None: the utterance
        starts here) -> (Output for exactly these frames, the new state).  The state is opaque: the (h, c) of every
        recurrent layer, the speaker permutation (drawn ONCE, at the first chunk, when random_speaker_order) and the
        embedding (computed ONCE, aux_net / aux_normalizer included; `aux` is not read again), and the frames consumed.
        Chunks of any lengths give what `forward` gives on their concatenation within the layers' error bounds: the
        recurrence continues from the very bits it stopped at; a GEMM over another number of rows may round differently."""
        res, unbatched, state = self._chunk_logits(xs, aux, state)
        with torch.no_grad():
            out = self._output(tuple(r[0] for r in res) if unbatched else res)
        return out, state

    def train_chunk(self, xs, aux, state=None, detach=True):
        """forward_chunk's contract WITH gradients: training a causal model (rnn_typ='lstm') on consecutive chunks of a
        recording -> (Output for exactly these frames, the new state).  The speaker permutation is drawn once and the
        embedding computed once, in the first chunk (state=None); later calls do not read `aux`.
        detach=True -- truncated BPTT: the layer states in the returned state are cut from the graph, so a loss on the next
        chunk stops at its first frame; call backward() after every chunk.  The embedding kept in the state is detached
        too: aux_net / aux_normalizer receive a gradient from the FIRST chunk's loss only, a later chunk trains the trunk.
        detach=False -- full BPTT over chunks: states and embedding stay in the graph; a loss on a later chunk reaches the
        earlier chunks' frames and parameters and aux_net from every chunk, and the chunked gradient is the whole
        utterance's within the layers' error bounds.  Hand such a state to a later call only while the
        graph behind it is alive (backward once, after the last chunk, or with retain_graph).
        Refuses what forward_chunk refuses."""
        res, unbatched, state = self._chunk_logits(xs, aux, state, grad=True, detach=detach)
        return self._output(tuple(r[0] for r in res) if unbatched else res), state

    def _check_chunkable(self, aux=None):
        """What forward_chunk refuses, from the arguments alone (nothing is launched)."""
        if self.rnn_typ != "lstm":
            raise ValueError(f"forward_chunk needs rnn_typ='lstm': {self.rnn_typ!r} reads the future of every frame")
        if self.input_normalizer is not None:
            raise NotImplementedError("forward_chunk with input_normalizer: its statistics span the utterance")
        if aux is not None and not isinstance(self.aux_net, AuxNet) and _aux_ndim(aux) == 4:
            raise NotImplementedError("forward_chunk with a frame-wise aux [B, K, Ta, E]: an embedding per frame "
                                      "would have to arrive with the frames (not built)")

    def _chunk_logits(self, xs, aux, state=None, grad=False, detach=True):
        """forward_chunk in front of the Output: -> (what `logits` returns for these frames -- batched, the head's rows as
        they are --, whether xs came un-batched, the new state).  The online separator feeds the rows to the fused tail.
        grad (train_chunk): under the caller's gradient mode, the layer states through functional.rnnp_layer's state_grad;
        detach: what the new state keeps of the graph."""
        self._check_chunkable()
        unbatched = xs.dim() == 2
        if unbatched:
            xs, aux = xs[None], ([aux] if state is None else aux)
        if xs.dim() != 3 or xs.shape[1] < 1:
            raise ValueError(f"xs {tuple(xs.shape)}: [B, Tc, idim] or [Tc, idim] with Tc >= 1")
        B, T = xs.shape[0], xs.shape[1]
        with contextlib.nullcontext() if grad else torch.no_grad():
            if state is None:
                self._check_chunkable(aux)
                emb, perm_d, iperm_d, K = self._embedding(aux, B, T, xs.device)
                state = ChunkState(layers=None, perm=perm_d, iperm=iperm_d, embedding=emb, K=K, frames=0)
            elif not isinstance(state, ChunkState):
                raise TypeError(f"state: what forward_chunk returned, not {type(state).__name__}")
            layers = []
            res = self._trunk(xs, state.embedding, state.perm, state.iperm, state.K, prev=state.layers, states=layers,
                              state_grad=grad)
        emb = state.embedding
        if grad and detach:
            layers, emb = [tuple(s.detach() for s in hc) for hc in layers], emb.detach()
        return res, unbatched, ChunkState(layers=layers, perm=state.perm, iperm=state.iperm, embedding=emb,
                                          K=state.K, frames=state.frames + T)

    def _output(self, res) -> Output:
        if self.nmask > 1:                         # [..., K, M, T, F] as they are (net.py:631-659, 983)
            logit, mask, emb = res
            return Output(mask=mask, logit=logit, embedding=emb)
        logit, emb = res
        u = -3
        if self.explicit_vad:                      # net.py:969-979
            lg = logit if logit.dim() == 4 else logit[None]
            mask, vad_mask = Fn.sigmoid_gated(lg)
            vad_logit = lg[..., 0]
            if logit.dim() == 3:
                mask, vad_mask, vad_logit = mask[0], vad_mask[0], vad_logit[0]
            return Output(mask=mask.unsqueeze(u), logit=None, embedding=emb, vad_mask=vad_mask.unsqueeze(-2),
                          vad_logit=vad_logit.unsqueeze(-2))
        mask = Fn.sigmoid(logit) if logit.dim() == 4 else Fn.sigmoid(logit[None])[0]      # (un-batched xs: [K, T, F])
        return Output(mask=mask.unsqueeze(u), logit=logit.unsqueeze(u), embedding=emb)
