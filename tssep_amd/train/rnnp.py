"""RNNP_packed -- drop-in for tssep/train/rnnp.py:11-173 on the HIP kernels.

Same constructor, attribute names and ``state_dict`` keys (``net.0.weight_ih_l0`` ...): the
``torch.nn.LSTM`` / ``Linear`` / ``Tanh`` members are kept as PARAMETER CONTAINERS so that
initialisation order (torch.manual_seed parity) and checkpoints are interchangeable; their
``forward`` is never called -- the math runs in libtssep_hip.so.

``typ='lstm'`` (rnnp.py:80-96: ``torch.nn.LSTM(bidirectional=False)`` + ``Linear(cdim, hdim)``) is the causal layer.  With
``return_states=True`` its ``forward(xs, prev_state=None)`` returns ``(h, states)``, one ``(h_n, c_n)`` [1, N, cdim] per
layer, and accepts that list back as ``prev_state`` -- the meaning the reference's parameters sketch and then assert away
(rnnp.py:121).  The state is carried without gradients -- unless ``forward(xs, prev_state, state_grad=True)``: then
``prev_state`` is accepted with gradients enabled and the returned states are part of the graph, for truncated BPTT (hand
the detached states on) or full BPTT over chunks (hand them on as they are); functional.rnnp_layer, DESIGN 4.21.

``dropout``: the ``torch.nn.Dropout`` members sit in front of a Tanh (rnnp.py:98-100).  One that is in training mode with
p > 0 makes that Tanh a dropout site of the HIP path (functional._RNNP); its own ``.training`` / ``.p`` are read at every
forward, so ``model.eval()`` and per-module switches behave as in the reference.
"""
import torch

from .. import functional as Fn


class RNNP_packed(torch.nn.Module):
    def __init__(self, idim, elayers, cdim, hdim, dropout, typ="blstm", return_states=False):
        super().__init__()
        if typ in ("bgru", "gru"):
            raise NotImplementedError(f"typ={typ!r}: only 'blstm' and 'lstm' are on the hot path (rnnp.py:40)")
        if typ not in ("blstm", "lstm"):
            raise ValueError(f"typ={typ!r}: 'blstm' | 'lstm'")
        if dropout < 0 or dropout > 1:      # (torch.nn.Dropout's own check; a single layer builds no Dropout member)
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout}")
        bidir = typ[0] == "b"
        if return_states and bidir:      # (a state of the reverse direction is the utterance's END: nothing to carry)
            raise NotImplementedError("return_states on a 'blstm' layer: a carried state needs typ='lstm'")
        net = []
        for i in range(elayers):
            inputdim = idim if i == 0 else hdim
            net.append(torch.nn.LSTM(inputdim, cdim, num_layers=1, bidirectional=bidir,
                                     batch_first=True))
            net.append(torch.nn.Linear(2 * cdim if bidir else cdim, hdim))
            if i < elayers - 1:
                net.append(torch.nn.Dropout(p=dropout))
                net.append(torch.nn.Tanh())
        self.net = torch.nn.ModuleList(net)
        self.elayers, self.cdim, self.typ, self.bidir = elayers, cdim, typ, bidir
        self.dropout, self.return_states = dropout, return_states
        self.hdim = hdim

    @staticmethod
    def site_p(site):
        """p of an ACTIVE dropout site (a torch.nn.Dropout in training mode with p > 0), else 0."""
        return float(site.p) if site is not None and site.training and site.p > 0 else 0.0

    def forward_rows(self, rows, N, T, final_act=0, combine=0, in_tanh=0, next_folds=False, final_dropout=None,
                     prev_state=None, states=None, state_grad=False):
        """rows: [N*T, I] (rows (n,t)) -> [N*T, hdim]; ``final_act``/``combine`` fuse the Tanh
        that follows this module in the post-net and the speaker-combination rearrange.  ``in_tanh``: the
        rows are the output of such a fused Tanh of the module in front (K > 1: in its speaker-combined
        layout) -- its backward is folded into this module's first d(input) GEMM; ``next_folds``: the module
        behind does the same for this module's final Tanh (functional.rnnp_layer).  ``final_dropout``: the
        ``torch.nn.Dropout`` container in front of that final Tanh (post-net, net.py:623-625), if there is one; a Tanh
        behind an active site is not folded, so the caller passes ``next_folds`` False and the module behind ``in_tanh`` 0.
        ``states``: a list that receives one ``(h_n, c_n)`` [1, N, cdim] per layer; ``prev_state``: such a list, the state
        every layer starts from (typ='lstm', without gradients: functional.rnnp_layer).  ``state_grad``: with gradients
        -- ``prev_state`` may require one, and what ``states`` receives is part of the graph."""
        h = rows
        stateful = states is not None or prev_state is not None
        if stateful and self.bidir:
            raise NotImplementedError("a carried state needs typ='lstm' ('blstm' reads the whole utterance)")
        if prev_state is not None and torch.is_grad_enabled() and not state_grad:
            raise RuntimeError("prev_state carries the recurrent state without gradients only: call the module under "
                               "torch.no_grad() (the states it returns never carry a gradient either)")
        if prev_state is not None and len(prev_state) != self.elayers:
            raise ValueError(f"prev_state: one (h, c) per layer, {self.elayers} -- got {len(prev_state)}")
        p_prev = 0.0
        for i in range(self.elayers):
            lstm, lin = self.net[4 * i], self.net[4 * i + 1]
            last = i == self.elayers - 1
            p_site = self.site_p(final_dropout if final_act == 1 else None) if last else self.site_p(self.net[4 * i + 2])
            fold_ok = self.hdim % 4 == 0 and Fn.H.FOLD_TANH
            h = Fn.rnnp_layer(h, lstm, lin, N, T, act=(final_act if last else 1),
                              combine=(combine if last else 0),
                              in_tanh=(in_tanh if i == 0 else (1 if fold_ok and not p_prev else 0)),
                              dz_given=((next_folds and final_act == 1) if last else fold_ok) and not p_site,
                              dropout_p=p_site,
                              **(dict(state=None if prev_state is None else prev_state[i], return_state=True) if stateful else {}),
                              **(dict(state_grad=True) if state_grad else {}))
            if stateful:
                h, (hT, cT) = h
                if states is not None:
                    states.append((hT.unsqueeze(0), cT.unsqueeze(0)))
            p_prev = p_site
        return h

    def forward(self, xs_pack, prev_state=None, state_grad=False):
        if prev_state is not None and not self.return_states:
            raise ValueError("prev_state needs return_states=True (and typ='lstm')")
        if isinstance(xs_pack, torch.nn.utils.rnn.PackedSequence):
            raise NotImplementedError("PackedSequence (unimplemented in the reference too, rnnp.py:124-129)")
        shape = xs_pack.shape
        if len(shape) == 4:
            N, T = shape[0] * shape[1], shape[2]
        elif len(shape) == 3:
            N, T = shape[0], shape[1]
        elif len(shape) == 2:
            N, T = 1, shape[0]
        else:
            raise KeyError(len(shape))
        states = [] if self.return_states else None
        y = self.forward_rows(xs_pack.reshape(N * T, shape[-1]), N, T, prev_state=prev_state, states=states,
                              **(dict(state_grad=True) if state_grad else {}))
        y = y.reshape(*shape[:-1], y.shape[-1])
        return (y, states) if self.return_states else y
