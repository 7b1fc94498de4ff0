"""torch.autograd.Function wrappers around the HIP kernels (hip_ops).

Each Function mirrors one ATen-level operator group of the reference hot path (SURVEY.md
section 2.2) with an explicit backward; autograd is only the glue that chains them.
"""
import collections
import contextlib

import numpy as np
import torch

from . import hip_ops as H


# ---- hand-offs between neighbouring Functions of the tail --------------------------------------------------
# head (final Linear) -> fused mask / iSTFT -> LogMAE are three autograd Functions (three reference modules:
# net.py:629-666, enhancer.py:98-100 + model.py:661-664, loss.py:244-247), but on the training step the
# backward of the middle one can take the loss's arguments instead of a [B,K,N] gradient and write d(logit)
# where the Linear's backward reads it.  A producer that folds its work into its neighbour returns _dummy_grad
# (zeros without memory) and leaves the real arguments on a link object both Functions hold; a consumer that
# receives anything but that pristine dummy (another loss used the same tensor, autograd summed gradients)
# falls back to the unfused kernels for the linked part and adds it -- correct either way.
_ZERO = {}


def _dummy_grad(like, shape=None):
    z = _ZERO.get(like.device)
    if z is None:
        z = _ZERO[like.device] = torch.zeros(1, device=like.device, dtype=torch.float32)
    return z.expand(tuple(like.shape if shape is None else shape))


def _is_dummy(g):
    z = _ZERO.get(g.device)
    return z is not None and g.data_ptr() == z.data_ptr() and all(st == 0 for st in g.stride())


class _Link:
    """payload: set by the producer's backward, taken (and cleared) by the consumer's."""

    def __init__(self, **kw):
        self.payload = None
        self.__dict__.update(kw)

    def take(self):
        p, self.payload = self.payload, None
        return p

    def observed(self):
        """True when somebody watches the gradient of the tensor this link hangs on (``register_hook``,
        ``retain_grad``): a fold that never forms that gradient must not be taken then."""
        ref = getattr(self, "out", None)
        t = ref() if ref is not None else None
        return t is not None and (bool(getattr(t, "_backward_hooks", None)) or bool(getattr(t, "retains_grad", False)))


# --------------------------------------------------- weight gradients of y = x W^T + b: one emitter, one fork
def _notify_grads(params):
    """The gradients of `params` are queued completely (directly into the flat bucket): a bucket with per-layer
    segments may all-reduce the layer now (distributed.GradBucket.notify; a no-op unless armed)."""
    b = getattr(params[0], "_tssep_bucket", None)
    b = b() if b is not None else None
    if b is not None and b._armed:
        b.notify(params)


def _grad_sink(p):
    """Flat-bucket view a parameter's gradient may be accumulated into directly (set by
    tssep_amd.distributed.GradBucket), or None -> return the gradient through autograd."""
    sinks = getattr(p, "_tssep_grad_sinks", None)
    if not sinks or p.grad is None or p.grad.data_ptr() != sinks[0].data_ptr():
        return None
    return sinks[H.ACTIVE_SINK % len(sinks)]


def _is_direct(sinks, honours_overlap_wgrad):
    """Whether a layer accumulates its weight gradients straight into the flat bucket: every parameter offers a sink,
    and -- for a layer that honours the switch -- runtime.overlap_wgrad is on."""
    return all(s is not None for s in sinks) and bool(H.OVERLAP_WGRAD or not honours_overlap_wgrad)


@contextlib.contextmanager
def _wgrad_branch(dev, R, reads, direct):
    """direct: the body runs on the weight-gradient stream of the current stream (H.side_stream: the compute stream itself
    for layers past SIDE_STREAM_MAX_SEQS), which first waits for the compute stream; `reads` are the tensors the body reads.
    Not direct: the body runs where it stands, and nothing of torch.cuda is touched."""
    if direct:
        main, side = torch.cuda.current_stream(), H.side_stream(dev, R)
        side.wait_stream(main)
        for t in reads:
            t.record_stream(side)
    with torch.cuda.stream(side) if direct else contextlib.nullcontext():
        yield


def _linear_wgrads(dv, ld_d, xv, ld_x, Nout, P, R, sinks, fused, bias=True):
    """dW [Nout, P] = dv^T xv and db [Nout] = the column sums of dv, for y = x W^T + b over R rows: the one place that
    issues this work.  sinks = (sw, sb): accumulated there, -> (None, None); sinks = None: -> (dw, db) in new tensors.
    fused: db rides on the weight-gradient GEMM as a virtual ones column of xv -- one pass over dv instead of two, and
    N = 600 -> 601 costs no extra tile (H.fused_colsum() says whether the GEMM arithmetic has it).  bias=False: a layer
    without bias (sb is None; db comes back None)."""
    acc = sinks is not None
    fused = fused and bias
    part, S = H.wgrad(dv, ld_d, xv, ld_x, Nout, P, R, with_colsum=fused)
    new = lambda *shape: torch.empty(*shape, device=dv.device, dtype=torch.float32)  # noqa: E731
    dw, db = sinks if acc else (new(Nout, P), new(Nout) if fused else None)
    if fused:
        H.reduce_splits_bias(part, S, Nout, P, H.round_up(P + 1, 4), dw, db, accumulate=acc)
    else:
        H.reduce_splits(part, S, Nout * P, dw, accumulate=acc)
        if bias:
            db = H.colsum(dv, ld_d, R, Nout, out=db, accumulate=acc)
    return (None, None) if acc else (dw, db)


# ---- derived weight layouts: ONE builder per tag (hip_ops.derived keeps the first it sees and prepare_derived replays it;
# a build reads the parameters, never a step's tensors).  D directions of time -- 2: BLSTM, 1: typ = 'lstm', the causal
# route -- are 4 D LSTM tensors and D column blocks of the projection; memo and builder live on the parameter object, and a
# parameter belongs to one LSTM, so both kinds share the tags.  A torch.nn.GRU container (rnnp.py:87) has the
# same 4 D tensors with three gate rows per unit; its pack (four slots per unit, gru.hip) has a tag of its own.  The cell
# kind is decided ONCE, by rnnp_layer from the container's class, and travels as the flag `gru`.
def _lstm_pack_of(lstm_params, Hh, I, gru=False):
    lstm_params = list(lstm_params)
    if gru:
        return H.derived("gru_pack", lstm_params, lambda: H.gru_pack(lstm_params, Hh, I))
    # (the library has an entry point per direction count; looked up when the build runs)
    return H.derived("lstm_pack", lstm_params,
                     lambda: (H.lstm1_pack if len(lstm_params) == 4 else H.lstm_pack)(lstm_params, Hh, I))


def _proj_layout_of(w_proj, Hh, Hp):
    """projection weight [hdim, D*Hh] in the (possibly padded) [hdim, D*Hp] column layout of hout"""
    def build():
        w = w_proj.detach()
        if Hp == Hh and w.is_contiguous() and w.data_ptr() % 16 == 0:
            return w
        D = w.shape[1] // Hh
        out = torch.zeros(w.shape[0], D * Hp, device=w.device, dtype=torch.float32)
        for d in range(D):
            out[:, d * Hp:d * Hp + Hh] = w[:, d * Hh:(d + 1) * Hh]
        return out
    return H.derived("proj_layout", [w_proj], build)


def _proj_T_of(w_proj, Hh, Hp):
    return H.derived("proj_T", [w_proj], lambda: H.transposed(_proj_layout_of(w_proj, Hh, Hp), w_proj.shape[0],
                                                              w_proj.shape[1] // Hh * Hp))


def _wih_T_of(lstm_params, Hh, I, gru=False):
    G = len(lstm_params) * Hh      # 4 D Hh gate rows (a GRU's four slots per unit likewise)

    def build():
        pk = _lstm_pack_of(lstm_params, Hh, I, gru)
        return H.transposed(pk["wih_p"].view(G, pk["ld_i"]), G, I)
    return H.derived("wih_T", list(lstm_params[0::4]), build)


# ------------------------------------------------------------------------------ RNNP
_RNNPMeta = collections.namedtuple("_RNNPMeta", "N T I D Hh Hp hdim ld_x ld_y act combine gru")


def _rnnp_forward(x, lstm_params, w_proj, b_proj, N, T, act, combine, dropout_p, state=None, want_state=False, gru=False):
    """The forward stages of one layer over D = len(lstm_params) // 4 directions of time: input GEMM with bias into gates
    [R, 4 D Hh], the recurrence (D = 1: from `state` = (h0, c0) [N, Hh] when given), the projection [hdim, D Hh] with
    act / combine / the dropout site.  Run inside _RNNP, and as they are under no_grad with a carried state (rnnp_layer).
    gru: the 4 D tensors are a torch.nn.GRU's (three gate rows per unit) -- the same stages on the four slots (r, z, n, q)
    per unit; no `cell` is allocated, the backward recurrence reads hout in its place, and the state is h alone: `state` =
    (h0,), the last state (hT,).
    -> (y, saved tensors, (drop, used), meta, the backward's (plan, W_hh layout), the last state -- (hT, cT), a GRU's (hT,)
    -- or None)"""
    D = len(lstm_params) // 4
    w_ih, w_hh = lstm_params[0], lstm_params[1::4]
    dev = x.device
    Hh, I, hdim = w_hh[0].shape[1], w_ih.shape[1], w_proj.shape[0]
    assert w_proj.shape[1] == D * Hh, (tuple(w_proj.shape), D, Hh)
    xv, ld_x = H.rows_view(x)
    R, G = N * T, 4 * D * Hh
    assert xv.shape[0] == R and xv.shape[1] >= I, (xv.shape, R, I)
    assert w_ih.shape[0] == (3 if gru else 4) * Hh, (tuple(w_ih.shape), Hh, gru)
    pk = _lstm_pack_of(lstm_params, Hh, I, gru)
    gates = torch.empty(R, G, device=dev, dtype=torch.float32)
    H.gemm(xv, ld_x, pk["wih_p"], pk["ld_i"], gates, G, R, G, I, bias=pk["bias_p"])
    Hp = H.round_up(Hh, 4)
    cell = None if gru else torch.empty(N, T, D, Hh, device=dev, dtype=torch.float32)
    hout = (torch.zeros if Hp != Hh else torch.empty)(R, D * Hp, device=dev, dtype=torch.float32)
    h0 = c0 = hT = cT = None
    if state is not None:
        h0 = H._f32(state[0]).reshape(N, Hh).contiguous()
        if not gru:
            c0 = H._f32(state[1]).reshape(N, Hh).contiguous()
    if want_state:
        hT = torch.empty(N, Hh, device=dev, dtype=torch.float32)
        if not gru:
            cT = torch.empty(N, Hh, device=dev, dtype=torch.float32)
    # the plan and BOTH directions' W_hh layouts are fetched here, once: the backward launches from what ctx keeps (a
    # step captured without prepare_derived builds a layout at every ask)
    plan = H.recurrence_plan(N, T, Hh, H.n_cus(dev), directions=D, **(dict(cell="gru") if gru else {}))
    whh = H.recurrence_packs(plan, w_hh[0], w_hh[-1], Hh, pk, memo=True)
    H.recurrence_launch(plan["fwd"], "fwd", gates, cell, hout, D * Hp, Hp, whh["fwd"], N, T, Hh, state=(h0, c0, hT, cT))
    wp = _proj_layout_of(w_proj, Hh, Hp)
    drop = float(dropout_p) if dropout_p else 0.0
    store_act = 0 if drop else act
    if combine:
        K = combine
        y = torch.empty(N // K * T, K * hdim, device=dev, dtype=torch.float32)
        H.gemm(hout, D * Hp, wp, D * Hp, y, 0, R, hdim, D * Hp, bias=b_proj.detach(), act=store_act,
               remap=dict(T=T, K=K, sb=T * K * hdim, sk=hdim, st=K * hdim))
        ld_y = K * hdim
    else:
        y, ld_y = H.padded(R, hdim, dev, zero=True)
        H.gemm(hout, D * Hp, wp, D * Hp, y, ld_y, R, hdim, D * Hp, bias=b_proj.detach(), act=store_act)
    used = None
    if drop:
        used = H.dropout_draw(dev)
        H.dropout_tanh_fwd(y, y, R, hdim, ld_y, combine if combine else 1, T, bool(combine), drop, used)
    meta = _RNNPMeta(N, T, I, D, Hh, Hp, hdim, ld_x, ld_y, act, combine, gru)
    return (y, (xv, gates, cell, hout, y, wp), (drop, used), meta, (plan["bwd"], whh["bwd"]),
            ((hT,) if gru else (hT, cT)) if want_state else None)


class _RNNP(torch.autograd.Function):
    """One RNNP_packed layer (tssep/train/rnnp.py:80-96,146-168): LSTM in both directions of time (BLSTM), or in ONE
    (typ='lstm') + Linear (+ tanh).  params: the 4 D LSTM tensors (w_ih, w_hh, b_ih, b_hh forward, then reverse), w_proj
    [hdim, D Hh], b_proj.

    x: [R, ld_x] buffer view, rows (n, t) for N sequences of T frames, I valid columns.
    Output: [R, hdim] rows (padded leading dimension), or the speaker-combined layout
    [B, T, K*hdim] when ``combine=K`` (net.py:608-611 fused into the projection's store).
    ``dropout_p`` > 0: the Tanh behind this layer is an ACTIVE dropout site (rnnp.py:98-100, net.py:623-625) -- the
    projection stores plainly (act = 0) and one pass over y applies mask, 1 / (1 - p) and Tanh in place; the backward
    regenerates the mask from the {seed, draw} pair the forward drew (hip_ops.dropout_draw).
    ``want_state`` (D = 1): the state after the last frame leaves as two more outputs.  Zero initial state: a carried state
    exists without gradients only (rnnp_layer) -- unless ``state_grad``: then h0 / c0 [N, Hh] (None: zeros) are
    differentiable inputs and the last state leaves as differentiable outputs.  Gradients are not
    materialised there: a final state nobody differentiates arrives as None and reaches the recurrence as a null pointer,
    so such a layer makes the launches of one without a state.
    The 4 D tensors of a torch.nn.GRU (three gate rows per unit) run the GRU recurrence (gru.hip) through the same stages;
    its state is one more output, h.  ``gru``: rnnp_layer's flag, the container's class."""

    @staticmethod
    def forward(ctx, x, N, T, act, combine, in_tanh, in_link, out_link, dropout_p, want_state, gru, state_grad, h0, c0,
                *params):
        assert not dropout_p or (act == 1 and out_link is None), "dropout_p: a site is the Tanh behind the layer, never folded"
        assert state_grad or (h0 is None and c0 is None), "a state is an input under state_grad only"
        state, ctx.state_shapes = None, (None, None)
        if h0 is not None:
            Hh = params[1].shape[1]
            ctx.state_shapes = (h0.shape, None if gru else c0.shape)
            h0 = H._f32(h0).reshape(N, Hh).contiguous()
            c0 = None if gru else H._f32(c0).reshape(N, Hh).contiguous()
            state = (h0,) if gru else (h0, c0)
        y, saved, ctx.drop, ctx.meta, ctx.recurrence, last = _rnnp_forward(x, params[:-2], *params[-2:], N, T, act, combine,
                                                                           dropout_p, state=state, want_state=want_state,
                                                                           gru=gru)
        ctx.save_for_backward(*saved, h0, c0)
        ctx.state_grad = bool(state_grad)
        ctx.params = params
        # Tanh-backward fold (see rnnp_layer): in_link = the link my producer hung on x, out_link = the one my
        # consumer may answer on.  Both are decided again in backward, when it is known who else uses the tensors.
        ctx.fold = (int(in_tanh) if in_link is not None else 0, in_link, out_link)
        assert out_link is None or act == 1, "out_link: only behind the fused Tanh"
        ctx.x_shape = x.shape
        y = y if combine else y[:, :ctx.meta.hdim]
        if state_grad:
            ctx.set_materialize_grads(False)
        if not want_state:
            return y
        if not state_grad:
            ctx.mark_non_differentiable(*last)      # (the last frame's state leaves without a gradient: no truncated BPTT)
        return (y, *last)

    @staticmethod
    def backward(ctx, dy, *dlast):
        xv, gates, cell, hout, y, _, h0, c0 = ctx.saved_tensors
        m, params = ctx.meta, ctx.params
        in_tanh, in_link, out_link = ctx.fold
        bstate = None
        if ctx.state_grad:
            if dy is None:      # (the loss reads the final state alone)
                dy = torch.zeros_like(y if m.combine else y[:, :m.hdim])
            new = lambda: torch.empty(m.N, m.Hh, device=gates.device, dtype=torch.float32)  # noqa: E731
            dlast = [None if g is None else H._f32(g).reshape(m.N, m.Hh).contiguous() for g in dlast] + [None, None]
            dh0 = new() if h0 is not None and ctx.needs_input_grad[12] else None
            dc0 = new() if c0 is not None and ctx.needs_input_grad[13] else None
            bstate = (h0, dlast[0], dh0) if m.gru else (c0, dlast[0], dlast[1], dh0, dc0)
        dz, ld_dz = H.rows_view(_rnnp_dz(dy, y, m, ctx.drop, out_link.take() if out_link is not None else None))
        sinks = [_grad_sink(p) for p in params]
        direct = _is_direct(sinks, True)
        d_w_proj, d_b_proj = _rnnp_proj_wgrads(dz, ld_dz, hout, m, sinks[-2:], direct)
        # the critical path: gates <- d(pre-activations); a GRU's backward recurrence reads hout (h_prev) where the LSTM's reads cell
        _rnnp_bptt(dz, ld_dz, gates, hout if m.gru else cell, params[-2], m, ctx.recurrence, bstate)
        lstm_grads = _rnnp_lstm_wgrads(gates, hout, xv, m, sinks[:-2], direct, h0)
        if direct:
            _notify_grads(params)                    # (4 D + 2 tensors: every direction's LSTM weights + the projection)
        dx = _rnnp_dx(gates, xv, params[:-2], m, ctx.x_shape, in_link, in_tanh) if ctx.needs_input_grad[0] else None
        dstate = (None, None)
        if bstate is not None:
            dstate = tuple(None if g is None else g.reshape(shape)
                           for g, shape in zip((bstate[-1], None) if m.gru else bstate[-2:], ctx.state_shapes))
        return (dx,) + (None,) * 11 + dstate + (*lstm_grads, d_w_proj, d_b_proj)


def _rnnp_dz(dy, y, m, drop, folded):
    """stage 1 -> d(pre-activation) of the projection, rows (n,t) x hdim.  folded: what the consumer left on the link."""
    R, hdim, T, K, combined = m.N * m.T, m.hdim, m.T, m.combine or 1, bool(m.combine)

    def tanh_args():      # (d(y), y) as the Tanh backward kernels read them -- combined as they are, dense rows otherwise -- + geometry
        pair = (dy.contiguous(), y) if combined else (dy.reshape(-1, hdim).contiguous(), y[:, :hdim].contiguous())
        return (*pair, R, hdim, K, T, combined)
    if folded is not None:
        # the consumer's d(input) GEMM already applied 1 - y^2 and wrote dense rows (n,t) x hdim; `dy` is the
        # dummy it returned -- unless y has ANOTHER consumer (auxiliary loss): autograd then summed that
        # consumer's plain d(y) onto the dummy's zeros, and it goes through the Tanh backward here
        dz = folded.view(R, hdim)
        if not _is_dummy(dy):
            dz = dz + H.tanh_bwd(*tanh_args())
        return dz
    if m.act:
        p, used = drop
        return H.dropout_tanh_bwd(*tanh_args(), p, used) if p else H.tanh_bwd(*tanh_args())
    if combined:   # layout change only: reuse tanh_bwd's gather with y = 0
        return H.tanh_bwd(dy.contiguous(), torch.zeros_like(dy), R, hdim, K, T, True)
    # (a strided [R, hdim] view of a padded buffer -- what the conditioning's backward hands the pre-net --
    # goes to the GEMMs as it is: rows_view only copies what is not 16-byte-row addressable)
    return dy if dy.dim() == 2 else dy.reshape(-1, hdim)


def _rnnp_proj_wgrads(dz, ld_dz, hout, m, sinks, direct):
    """stage 2 -> (d_w_proj [hdim, D Hh], d_b_proj), or (None, None) when they went into `sinks` (side stream)"""
    R, Hh, Hp, ld_h = m.N * m.T, m.Hh, m.Hp, m.D * m.Hp
    aligned = Hp == Hh           # hout's column layout is w_proj's: the emitter writes the sinks itself, fused where it can
    with _wgrad_branch(dz.device, R, (dz, hout), direct):
        to_sinks = direct and aligned
        d_w, d_b = _linear_wgrads(dz, ld_dz, hout, ld_h, m.hdim, ld_h, R, sinks if to_sinks else None,
                                  to_sinks and H.fused_colsum())
        if not aligned:
            d_w = _proj_unlayout(d_w, Hh, Hp)
            if direct:
                sinks[0].add_(d_w)
                sinks[1].add_(d_b)
                d_w = d_b = None
    return d_w, d_b


def _rnnp_bptt(dz, ld_dz, gates, cell, w_proj, m, recurrence, state=None):
    """stage 3: dhout = dz W_proj, then the recurrence backwards in time: `gates` <- d(pre-activations).  state (D = 1):
    the carried state's side, (c0, dhT, dcT, dh0, dc0) -- a GRU's (h0, dhT, dh0) -- as hip_ops.recurrence_launch takes it"""
    R, Hp, ld_h = m.N * m.T, m.Hp, m.D * m.Hp
    dhout = torch.empty(R, ld_h, device=dz.device, dtype=torch.float32)
    wpT, ld_t = _proj_T_of(w_proj, m.Hh, Hp)
    H.gemm(dz, ld_dz, wpT, ld_t, dhout, ld_h, R, ld_h, m.hdim)
    H.recurrence_launch(recurrence[0], "bwd", gates, cell, dhout, ld_h, Hp, recurrence[1], m.N, m.T, m.Hh,
                        **({} if state is None else dict(state=state)))


def _rnnp_lstm_wgrads(gates, hout, xv, m, sinks, direct, h0=None):
    """stage 4 -> the 4 D LSTM gradients in parameter order from dgates (in `gates`), or 4 D None when they went into
    `sinks` (side stream).  A GRU (m.gru): the same products over the four slots, unpacked to torch's three gate rows --
    dW_ih and db_ih from the slots (r, z, n), dW_hh and db_hh from (r, z, q): the two biases have gradients of their own.
    h0 [N, Hh] (D = 1): the state the forward started from -- the frame-shifted product pairs frame 0 with zero, so dW_hh
    takes sum_n dgates[n, 0]^T h0[n] from one more product over the N frame-0 rows of `gates` (row stride T G), added to
    the packed dW_hh in a fixed order ahead of the unpack: both sink modes and a GRU's slots (r, z, q) see it alike."""
    R, T, I, D, Hh, Hp, G = m.N * m.T, m.T, m.I, m.D, m.Hh, m.Hp, 4 * m.D * m.Hh
    with _wgrad_branch(gates.device, R, (gates, hout, xv) + (() if h0 is None else (h0,)), direct):
        dwhh = torch.empty(D, 4 * Hh * Hh, device=gates.device, dtype=torch.float32)
        for d in range(D):   # dgates_t paired with h_{t-1} (forward dir) / h_{t+1} (reverse)
            part, S = H.wgrad((gates, d * 4 * Hh), G, (hout, d * Hp), D * Hp, 4 * Hh, Hh, R,
                              b_kshift=(-1 if d == 0 else 1), kperiod=T)
            H.reduce_splits(part, S, 4 * Hh * Hh, dwhh[d])
        if h0 is not None:
            h0v, ld_h0 = H.rows_view(h0)
            part, S = H.wgrad(gates, T * G, h0v, ld_h0, 4 * Hh, Hh, m.N)
            H.reduce_splits(part, S, 4 * Hh * Hh, dwhh[0], accumulate=True)
        # dW_ih and (split-bf16 GEMM) the bias gradient in ONE pass over dgates: a virtual ones
        # column of x makes column I of the partials the column sums
        fused = H.fused_colsum()
        part, S = H.wgrad(gates, G, xv, m.ld_x, G, I, R, with_colsum=fused)
        ldp = H.round_up(I + 1, 4) if fused else I
        bias_src = ((part, I), ldp, S, G * ldp) if fused else (H.colsum(gates, G, R, G), 1, 1, 0)
        # (source, columns, index of the forward direction's destination: the reverse one's is 4 further)
        unpacks = [((dwhh, Hh, 1, 0), Hh, 1), ((part, ldp, S, G * ldp), I, 0), (bias_src, 1, 2)]
        if direct or m.gru:
            unpacks.append((bias_src, 1, 3))      # b_ih and b_hh receive the same gradient (LSTM; a GRU's differ in the n rows)
        rows = (3 if m.gru else 4) * Hh
        if direct:
            dst = sinks
        else:
            new = lambda *shape: torch.empty(*shape, device=gates.device, dtype=torch.float32)  # noqa: E731
            dst = [t for _ in range(D) for t in (new(rows, I), new(rows, Hh), new(rows), new(rows) if m.gru else None)]
        unpack = H.lstm1_unpack if D == 1 else H.lstm_unpack      # (the library's entry point per direction count)
        for src, ncols, i in unpacks:
            if m.gru:      # (the hidden side -- W_hh, b_hh: indices 1 and 3 -- reads slot q for the n rows)
                H.gru_unpack(*src, Hh, ncols, H.GRU_HH if i % 2 else H.GRU_IH, *dst[i::4], accumulate=direct)
            else:
                unpack(*src, Hh, ncols, *dst[i::4], accumulate=direct)
    if direct:
        return (None,) * (4 * D)
    for d in range(D):
        if not m.gru:
            dst[4 * d + 3] = dst[4 * d + 2].clone()
    return tuple(dst)


def _rnnp_dx(gates, xv, lstm_params, m, x_shape, in_link, Kc):
    """stage 5 -> d(input).  Kc > 0: my input is a Tanh output whose backward rides on this GEMM's store; the result
    travels on in_link and x receives a dummy (its true gradient is never formed -- hence not when it is watched)"""
    R, T, I, G, dev = m.N * m.T, m.T, m.I, 4 * m.D * m.Hh, gates.device
    wihT, ld_t = _wih_T_of(lstm_params, m.Hh, I, m.gru)
    if not Kc or in_link.observed():
        dxb, ld_dx = H.padded(R, I, dev, zero=True)
        H.gemm(gates, G, wihT, ld_t, dxb, ld_dx, R, I, G)
        return dxb[:, :I].reshape(x_shape)
    assert I % 4 == 0 and I % Kc == 0 and m.ld_x == I, (I, Kc, m.ld_x)
    dxb = torch.empty(R, I, device=dev, dtype=torch.float32)
    hd = I // Kc      # Kc > 1: rows (b,t) x (k, hdim) -> rows (b,k,t) x hdim (inverse of net.py:608-611)
    remap = dict(T=T, K=1, sb=Kc * T * hd, sk=0, st=hd, cm=hd, co=T * hd) if Kc > 1 else None
    H.gemm(gates, G, wihT, ld_t, dxb, 0 if remap else I, R, I, G, act=2, aux=(xv, m.ld_x), remap=remap)
    # (accumulated, like head_link below: the activation may feed TWO folded consumers -- ADVICE r4)
    in_link.payload = dxb if in_link.payload is None else in_link.payload + dxb.view_as(in_link.payload)
    return _dummy_grad(xv, x_shape)


def _proj_unlayout(dwp, Hh, Hp):
    """the D column blocks of w_proj out of hout's padded layout (the pad columns of hout are zero: nothing of them
    reaches dW_proj)"""
    if Hp == Hh:
        return dwp
    return torch.cat([dwp[:, d * Hp:d * Hp + Hh] for d in range(dwp.shape[1] // Hp)], dim=1).contiguous()


def rnnp_layer(x, lstm, linear, N, T, act=0, combine=0, in_tanh=0, dz_given=False, dropout_p=0.0, state=None,
               return_state=False, state_grad=False):
    """x rows (n,t); lstm = torch.nn.LSTM parameter container, linear = nn.Linear container.
    lstm a torch.nn.GRU container: the same layer on the GRU recurrence (gru.hip); its state is ONE tensor, h -- `state`
    = h0 [N, H], and the result with return_state is (output, hT).
    lstm.bidirectional False: the causal route -- the same _RNNP over one direction of time.  There, and only without
    gradients, state = (h0, c0) [N, H] starts the recurrence from a carried state and / or return_state asks for the last
    frame's: the result is then (output, (hT, cT)).
    state_grad (one direction): the state is part of the graph -- `state` is accepted with gradients enabled, its tensors
    may require a gradient, and the returned state carries one back: truncated BPTT hands `[s.detach() for s in state]`
    to the next chunk, full BPTT over chunks the state itself.  Without the flag nothing changes.
    The Tanh between two layers (net.py:623-625) runs forward in the producer's projection epilogue (act = 1);
    its BACKWARD may run in the store of the consumer's d(input) GEMM: the producer is called with dz_given and
    hangs a _Link on its output, the consumer with in_tanh (1: same row layout; K > 1: its input is the
    producer's speaker-combined tensor [B T, K hdim] and the gradient is stored back as rows (b,k,t) x hdim).
    In backward the consumer leaves d(pre-activation) on the link and returns a dummy for its input; the
    producer adds the Tanh backward of whatever ELSE arrived for its output (a second consumer), and when the
    output is watched (hook / retain_grad) or the consumer never ran, nothing is folded and `tssep_tanh_bwd`
    runs as without the fold -- correct either way.
    dropout_p > 0 (with act = 1): that Tanh is an active dropout site, y = keep ? tanh(z / (1 - p)) : 0 (_RNNP); such a
    site is never folded -- the caller passes in_tanh = 0 to the consumer, and dz_given is ignored here."""
    import weakref
    if lstm.bidirectional and (state is not None or return_state or state_grad):
        raise NotImplementedError("rnnp_layer: a state on a bidirectional layer (it reads the whole utterance)")
    gru = isinstance(lstm, torch.nn.GRU)
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    lstm_params = [getattr(lstm, n) for n in names]
    if lstm.bidirectional:
        lstm_params += [getattr(lstm, n + "_reverse") for n in names]
    dropout_p = float(dropout_p) if (dropout_p and act == 1) else 0.0
    state_grad = bool(state_grad) and torch.is_grad_enabled()      # (without gradients: the path a carried state always had)
    if state is not None and state_grad:
        if gru and not torch.is_tensor(state):
            raise ValueError("state: h0 (a GRU carries one tensor)")
        if not gru and len(state) != 2:
            raise ValueError("state: (h0, c0)")
    elif state is not None:
        if torch.is_grad_enabled():
            raise RuntimeError("rnnp_layer: a carried state (state=(h0, c0)) exists without gradients only -- call it under "
                               "torch.no_grad() (a gradient through the state, truncated BPTT, is not implemented)")
        if gru and not torch.is_tensor(state):
            raise ValueError("state: h0 (a GRU carries one tensor)")
        if not gru and len(state) != 2:
            raise ValueError("state: (h0, c0)")
        y, _, _, m, _, last = _rnnp_forward(x, lstm_params, linear.weight, linear.bias, N, T, act, combine, dropout_p,
                                            state=(state,) if gru else state, want_state=True, gru=gru)
        return (y if combine else y[:, :m.hdim]), (last[0] if gru else last)
    in_link = getattr(x, "_tssep_tanh_link", None) if in_tanh else None
    if in_link is not None and not (x.requires_grad and torch.is_grad_enabled()):
        in_link = None
    out_link = _Link() if (dz_given and act == 1 and not dropout_p and torch.is_grad_enabled()) else None
    h0, c0 = (None, None) if state is None else (state, None) if gru else state
    out = _RNNP.apply(x, N, T, act, combine, in_tanh, in_link, out_link, dropout_p, bool(return_state), gru, state_grad,
                      h0, c0, *lstm_params, linear.weight, linear.bias)
    last = None
    if return_state:
        out, last = out[0], (out[1] if gru else (out[1], out[2]))
    if out_link is not None and out.requires_grad:
        out_link.out = weakref.ref(out)
        out._tssep_tanh_link = out_link
    return (out, last) if return_state else out


# ---------------------------------------------------------------------- conditioning
class _Cond(torch.autograd.Function):
    """tssep/train/net.py:862-896 (+ trial fold :913-924).  pre rows (b,t) -> rows (b,tr,k,t).
    aux [B, K, E] (one embedding per speaker and utterance), or frame-wise [B, K, Ta, E]: frame t reads row t // stride
    (net.py:866-867 at stride 1), through the *_t entry points; a 3-D aux makes the calls it always made.
    An embedding that requires a gradient (aux_net, a trainable normalised embedding) gets it from one more launch over
    dxs (hip_ops.cond_aux_bwd); a fixed embedding makes exactly the calls it always made."""

    @staticmethod
    def forward(ctx, pre, aux, B, K, T, trials, combination, stride):
        F = pre.shape[-1]
        Ta = aux.shape[-2] if aux.dim() == 4 else 0
        pv, ld_pre = H.rows_view(pre)
        xs, ld, info = H.cond_fwd(pv, ld_pre, aux.detach(), B, K, T, F, trials, combination, Ta, stride)
        W = F if combination == "mul" else F + aux.shape[-1]
        ctx.info = info
        ctx.meta = (B, K, T, F, trials, combination, ld, Ta, stride)
        ctx.aux_grad = None
        if aux.requires_grad:
            ctx.aux_grad = (tuple(aux.shape), (pv, ld_pre) if combination == "mul" else None)
        return xs[:, :W]

    @staticmethod
    def backward(ctx, dxs):
        B, K, T, F, trials, combination, ld, Ta, stride = ctx.meta
        dv, ld_d = H.rows_view(dxs)
        dpre, ldp = H.cond_bwd(dv, ld_d, ctx.info, B, K, T, F, trials, combination, Ta, stride)
        d_aux = None
        if ctx.aux_grad is not None and ctx.needs_input_grad[1]:
            shape, pre = ctx.aux_grad
            pv, ld_pre = pre if pre is not None else (None, 0)
            d_aux = H.cond_aux_bwd(dv, ld_d, pv, ld_pre, B, K, T, F, shape[-1], trials, combination, Ta,
                                   stride).view(shape)
        return dpre[:, :F], d_aux, None, None, None, None, None, None


def condition(pre, aux, B, K, T, trials, combination, stride=1):
    return _Cond.apply(pre, aux, B, K, T, trials, combination, stride)


# ------------------------------------------------------------------------ final linear
# geo: what the map kernels take behind (perm, iperm) -- (B, trials, K, [M,] T, F, Fr, spk_rows)
_HeadMeta = collections.namedtuple("_HeadMeta", "geo ld_x P R Nout")


def _head_grads(ctx, draw):
    """d(raw) [R, Nout] of the final Linear -> (dx, dw, db): the weight gradient and the bias column sums (straight into
    the optimizer's bucket on the side stream where that is set up: dw = db = None then) and the d(input) GEMM.  Shared
    by _Head and _HeadMasks; ctx carries saved_tensors (xv, ...), params, meta (_HeadMeta) and x_shape."""
    xv, m = ctx.saved_tensors[0], ctx.meta
    weight, bias = ctx.params
    dv, ld_d = H.rows_view(draw)
    sinks = (_grad_sink(weight), _grad_sink(bias))
    direct = _is_direct(sinks, True)
    with _wgrad_branch(draw.device, m.R, (dv, xv), direct):
        dw, db = _linear_wgrads(dv, ld_d, xv, m.ld_x, m.Nout, m.P, m.R, sinks if direct else None,
                                direct and H.fused_colsum())
    if direct:
        _notify_grads(ctx.params)
    dxb, ld_dx = H.padded(m.R, m.P, draw.device, zero=True)
    wvT, ld_t = H.derived("head_T", [weight], lambda: H.transposed(H.rows_view(weight.detach())[0], m.Nout, m.P))
    H.gemm(dv, ld_d, wvT, ld_t, dxb, ld_dx, m.R, m.P, m.Nout)
    return dxb[:, :m.P].reshape(ctx.x_shape), dw, db


class _Head(torch.autograd.Function):
    """post_net.linear + final einops + trial mean + speaker un-permutation
    (tssep/train/net.py:629-666, 928-967): x rows -> logit [B,K,T,F]."""

    @staticmethod
    def forward(ctx, x, weight, bias, perm, iperm, B, K, T, F, trials, Fr, spk_rows, link=None):
        dev = x.device
        ctx.link = link
        xv, ld_x = H.rows_view(x)
        P = weight.shape[1]
        wv, ld_w = H.rows_view(weight.detach())
        R = xv.shape[0]
        Nout = weight.shape[0]
        fast = (not spk_rows) and trials == 1 and Fr == F
        if fast:      # store straight into [B, perm[k], T, F] from the GEMM epilogue
            out = torch.empty(B, K, T, F, device=dev, dtype=torch.float32)
            H.gemm(xv, ld_x, wv, ld_w, out, 0, R, Nout, P, bias=bias.detach(),
                   remap=dict(T=T, K=1, sb=K * T * F, sk=0, st=F, cm=F, co=T * F, perm=perm,
                              perm_ld=K))
        else:
            raw = torch.empty(R, Nout, device=dev, dtype=torch.float32)
            H.gemm(xv, ld_x, wv, ld_w, raw, Nout, R, Nout, P, bias=bias.detach())
            out = H.logit_map_fwd(raw, perm, iperm, B, trials, K, T, F, Fr, spk_rows)
        ctx.save_for_backward(xv, wv)
        ctx.params = (weight, bias)
        ctx.aux = (perm, iperm)
        ctx.meta = _HeadMeta((B, trials, K, T, F, Fr, spk_rows), ld_x, P, R, Nout)
        ctx.x_shape = x.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        m = ctx.meta
        draw = ctx.link.take() if ctx.link is not None else None
        if draw is None:
            draw = H.logit_map_bwd(dout, *ctx.aux, *m.geo).view(m.R, m.Nout)
        elif not _is_dummy(dout):      # the fused tail wrote its part already laid out; someone else used logit too
            draw = draw + H.logit_map_bwd(dout, *ctx.aux, *m.geo).view(m.R, m.Nout)
        dx, dw, db = _head_grads(ctx, draw)
        return dx, dw, db, None, None, None, None, None, None, None, None, None, None


class _HeadMasks(torch.autograd.Function):
    """post_net.linear with nmask = M > 1 masks per speaker + final einops + trial mean + un-permutation + sigmoid
    (tssep/train/net.py:629-666, 928-967, 983): x rows -> (logit, mask), both [B,K,M,T,F].  The raw GEMM, then ONE fused
    map kernel each way (hip_ops.mask_map_fwd / _bwd)."""

    @staticmethod
    def forward(ctx, x, weight, bias, perm, iperm, B, K, M, T, F, trials, Fr, spk_rows):
        xv, ld_x = H.rows_view(x)
        P = weight.shape[1]
        wv, ld_w = H.rows_view(weight.detach())
        R, Nout = xv.shape[0], weight.shape[0]
        assert Nout == (1 if spk_rows else K) * M * Fr and R == B * trials * T * (K if spk_rows else 1), \
            (R, Nout, (B, K, M, T, F, trials, Fr, spk_rows))
        raw = torch.empty(R, Nout, device=x.device, dtype=torch.float32)
        H.gemm(xv, ld_x, wv, ld_w, raw, Nout, R, Nout, P, bias=bias.detach())
        logit, mask = H.mask_map_fwd(raw, perm, iperm, B, trials, K, M, T, F, Fr, spk_rows)
        ctx.save_for_backward(xv, wv, mask)
        ctx.params = (weight, bias)
        ctx.aux = (perm, iperm)
        ctx.meta = _HeadMeta((B, trials, K, M, T, F, Fr, spk_rows), ld_x, P, R, Nout)
        ctx.x_shape = x.shape
        ctx.set_materialize_grads(False)          # d(logit) is None when nobody else used the logit
        return logit, mask

    @staticmethod
    def backward(ctx, dlogit, dmask):
        m, mask = ctx.meta, ctx.saved_tensors[2]
        if dmask is None:                         # only the logit was used: the same kernel with d(mask) = 0
            dmask = torch.zeros_like(mask)
        draw = H.mask_map_bwd(dmask, mask, dlogit, *ctx.aux, *m.geo).view(m.R, m.Nout)
        dx, dw, db = _head_grads(ctx, draw)
        return (dx, dw, db) + (None,) * 10


def head_masks(x, linear, perm, iperm, B, K, M, T, F, trials, Fr, spk_rows):
    """nmask = M > 1 -> (logit, mask) [B,K,M,T,F]"""
    return _HeadMasks.apply(x, linear.weight, linear.bias, perm, iperm, B, K, M, T, F, trials, Fr, spk_rows)


def head(x, linear, perm, iperm, B, K, T, F, trials, Fr, spk_rows):
    link = None
    if H.FOLD_TAIL and (not spk_rows) and trials == 1 and Fr == F and x.requires_grad:
        link = _Link(iperm=iperm, shape=(B, K, T, F))       # the layout the fused tail may write d(logit) in
    out = _Head.apply(x, linear.weight, linear.bias, perm, iperm, B, K, T, F, trials, Fr, spk_rows, link)
    if link is not None:
        out._tssep_head_link = link
    return out


# --------------------------------------------------------------------------- mask head
class _MaskHead(torch.autograd.Function):
    """sigmoid + Masking (tssep/train/net.py:981-986, tssep/train/enhancer.py:98-100)."""

    @staticmethod
    def forward(ctx, logit, obs):
        mask, est = H.maskhead_fwd(logit, obs)
        ctx.save_for_backward(mask, obs)
        return mask, est

    @staticmethod
    def backward(ctx, dmask, dest):
        mask, obs = ctx.saved_tensors
        if dest is None:
            dest = torch.zeros(mask.shape, device=mask.device, dtype=torch.complex64)
        return H.maskhead_bwd(dest, dmask, mask, obs), None


def mask_head(logit, obs):
    """logit [B,K,T,F], obs complex [B,T,F] -> (mask, stft_estimate)."""
    return _MaskHead.apply(logit, obs)


def sigmoid(logit):
    """mask only (no observation available): the mask head with obs = 0, its estimate discarded."""
    B, K, T, F = logit.shape
    return _MaskHead.apply(logit, torch.zeros(B, T, F, device=logit.device, dtype=torch.complex64))[0]


class _MVDRSouden(torch.autograd.Function):
    """TorchBF.__call__ (enhancer.py:215-265) with a backward: hip_ops.mvdr_souden keeps its workspace (reduced
    statistics, wconj), hip_ops.mvdr_souden_bwd turns d(loss)/d(enh) into d(loss)/d(masks).  The observation gets no
    gradient.  The singular check of the forward is a host sync: eager only."""

    @staticmethod
    def forward(ctx, masks, obs, reference_channel, eps, masking, masking_eps):
        enh, state = H.mvdr_souden(masks.detach(), obs.detach(), reference_channel, eps=eps, masking=masking,
                                   masking_eps=masking_eps, return_state=True)
        # through save_for_backward: autograd then notices an in-place change of any of them before the backward
        ctx.save_for_backward(state.pop("masks"), state.pop("obs_r"), state.pop("ws"))
        ctx.scalars, ctx.mask_dtype = state, masks.dtype
        return enh

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, genh):
        masks, obs_r, ws = ctx.saved_tensors
        dmask = H.mvdr_souden_bwd(genh.to(torch.complex128), dict(ctx.scalars, masks=masks, obs_r=obs_r, ws=ws))
        return dmask.to(ctx.mask_dtype), None, None, None, None, None


def mvdr_souden(masks, obs, reference_channel, eps=None, masking=False, masking_eps=0.0):
    """masks [B,K,M,T,F] fp32|fp64, obs [B,D,T,F] complex128 -> enh [B,K,T,F] complex128, differentiable in masks."""
    if obs.requires_grad:
        raise NotImplementedError("mvdr_souden: the Observation requires grad, but the MVDR backward has a gradient for "
                                  "the masks only (detach the Observation)")
    return _MVDRSouden.apply(masks, obs, reference_channel, eps, masking, masking_eps)


# ------------------------------------------------------------------------- STFT family
_WINDOWS = {}


def windows(window, size, shift, device, window_length=None):
    """(analysis window, biorthogonal synthesis window), both [size] fp32 on `device`.  window_length < size
    (paderbox stft / istft: the window covers the first window_length samples of a frame, the transform is
    zero-padded to size): both windows are zero beyond window_length, so the kernels -- which always move `size`
    samples per frame -- compute exactly irfft(X)[..., :window_length] * w_syn."""
    from scipy.signal import get_window
    wl = size if window_length is None else int(window_length)
    key = (window, size, shift, str(device), wl)
    if key not in _WINDOWS:
        w = get_window(window, wl, fftbins=True).astype(np.float64)
        denom = np.zeros(wl)
        for i in range(-(wl // shift) - 1, wl // shift + 2):
            off = i * shift
            lo, hi = max(0, off), min(wl, wl + off)
            if lo < hi:
                denom[lo:hi] += (w ** 2)[lo - off:hi - off]
        wa, ws = np.zeros(size), np.zeros(size)
        wa[:wl] = w
        ws[:wl] = w / denom
        _WINDOWS[key] = (torch.as_tensor(wa, dtype=torch.float32).to(device),
                         torch.as_tensor(ws, dtype=torch.float32).to(device))
    return _WINDOWS[key]


class _ISTFT(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, wsyn, N, size, shift, fading):
        lead = X.shape[:-2]
        T = X.shape[-2]
        y, _ = H.istft_fwd(X.reshape(-1, T, X.shape[-1]), wsyn, N, size, shift, fading)
        ctx.save_for_backward(wsyn)
        ctx.meta = (lead, T, N, size, shift, fading)
        return y.reshape(*lead, N)

    @staticmethod
    def backward(ctx, dy):
        (wsyn,) = ctx.saved_tensors
        lead, T, N, size, shift, fading = ctx.meta
        dX = H.istft_bwd(dy.reshape(-1, N), wsyn, T, size, shift, fading)
        return dX.reshape(*lead, T, size // 2 + 1), None, None, None, None, None


def istft(X, wsyn, N, size=1024, shift=256, fading=True):
    return _ISTFT.apply(X, wsyn, N, size, shift, fading)


class _MaskISTFT(torch.autograd.Function):
    """sigmoid (net.py:983) -> Masking (enhancer.py:98-100) -> fe.istft (model.py:661-664) as ONE kernel
    each way; with ``tgt`` the forward also leaves the per-chunk sums of |estimate - tgt| on the result
    (``_tssep_absdiff``), which ``log_mae`` / ``mae`` consume instead of re-reading both signals.
    Gated rows (explicit_vad; hip_ops._tail_rows decides) take the same path; with ``vad`` the forward also returns
    SignalAndVADSigmoidBCE's BCE term of the gate column ([B]), and its gradient is folded into the tail's d(v) store: the
    BCE needs no pass of its own."""

    @staticmethod
    def forward(ctx, logit, obs, wsyn, N, size, shift, fading, tgt, vad, head_link=None, loss_link=None):
        y, part = H.mask_istft_fwd(logit, obs, wsyn, N, size, shift, fading, tgt)
        outs = [y]
        if part is not None:
            outs.append(part)
            ctx.mark_non_differentiable(part)
        if vad is not None:
            outs.append(H.gatebce_fwd(logit, vad))
        ctx.save_for_backward(logit, obs, wsyn, vad)
        ctx.meta = (size, shift, fading)
        ctx.links = (head_link, loss_link)
        return tuple(outs)

    @staticmethod
    def backward(ctx, dy, *rest):
        logit, obs, wsyn, vad = ctx.saved_tensors
        head_link, loss_link = ctx.links
        vadarg = (vad, rest[-1]) if vad is not None else None          # (Vad, d(loss) / d(bce))
        loss = loss_link.take() if loss_link is not None else None      # (est, tgt, sums, gout) of LogMAE / MAE
        if loss is not None and not _is_dummy(dy):      # someone else used the estimate too: the loss's part, unfused
            dy = dy + H.logmae_bwd(loss[0].contiguous(), loss[1].contiguous(), loss[2], loss[3])
            loss = None
        to_head = head_link is not None and tuple(head_link.shape) == tuple(logit.shape)
        d = H.mask_istft_bwd(dy, logit, obs, wsyn, *ctx.meta, loss=loss, vad=vadarg,
                             iperm=head_link.iperm if to_head else None, bt_major=to_head)
        if to_head:                                     # written where the Linear's backward reads it
            head_link.payload = d if head_link.payload is None else head_link.payload + d
            d = _dummy_grad(logit)
        return (d,) + (None,) * 10


def mask_istft(logit, obs, wsyn, N, size=1024, shift=256, fading=True, tgt=None, vad=None):
    """logit [B,K,T,F], obs complex [B,T,F] -> (time_estimate [B,K,N], None), differentiable w.r.t. logit.
    explicit_vad: logit [B,K,T,F+1] (VAD logit at column 0); with vad [B,K,T] the gate column's BCE against it ([B]) is
    returned as well, its backward folded into the tail's."""
    B, K, T = logit.shape[:3]
    assert vad is None or logit.shape[-1] == obs.shape[-1] + 1, "mask_istft: vad= needs gated logit rows"
    if tgt is not None and tuple(tgt.shape) != (B, K, N):
        tgt = None
    if vad is not None and tuple(vad.shape) != (B, K, T):
        vad = None
    fold = H.FOLD_TAIL and logit.requires_grad
    loss_link = _Link() if fold and tgt is not None and H.FOLD_TAIL != 3 else None
    head_link = getattr(logit, "_tssep_head_link", None) if fold and H.FOLD_TAIL != 2 else None
    out = _MaskISTFT.apply(logit, obs, wsyn, N, size, shift, fading, tgt, vad, head_link, loss_link)
    y = out[0]
    if tgt is not None:
        y._tssep_absdiff = (out[1], tgt.data_ptr(), tuple(tgt.shape))
        y._tssep_loss_link = loss_link
    return y, (out[-1] if vad is not None else None)


# ---------------------------------------------------------------- training on a stream
# One call of a streaming tail as a node of the graph: inputs (logit | X, ola_in), outputs (y, ola_out).  The gradients
# are not materialised: a y nobody used is zeros inside the wrapper, an ola_out nobody differentiates reaches the kernel as
# NULL -- the stream is cut behind this call -- and d_ola_in is asked for only when ola_in wants one.
class _MaskISTFTStream(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, ola_in, obs, wsyn, skip, N, size, shift):
        ctx.set_materialize_grads(False)
        y, ola_out = H.mask_istft_stream_fwd(logit, obs, wsyn, ola_in, skip, N, size, shift)
        ctx.save_for_backward(logit, obs, wsyn)
        ctx.meta = (skip, N, size, shift)
        return y, ola_out

    @staticmethod
    def backward(ctx, dy, d_ola_out):
        if dy is None and d_ola_out is None:        # nobody used either output: no gradient, no launch
            return (None,) * 8
        logit, obs, wsyn = ctx.saved_tensors
        dlogit, d_ola_in = H.mask_istft_stream_bwd(dy, d_ola_out, logit, obs, wsyn, *ctx.meta,
                                                   want_ola=ctx.needs_input_grad[1])
        return (dlogit if ctx.needs_input_grad[0] else None, d_ola_in) + (None,) * 6


class _ISTFTStream(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, ola_in, wsyn, skip, N, size, shift):
        ctx.set_materialize_grads(False)
        y, ola_out = H.istft_stream_fwd(X, wsyn, ola_in, skip, N, size, shift)
        ctx.save_for_backward(wsyn)
        ctx.meta = (X.shape[0], X.shape[1], skip, N, size, shift, X.device)
        return y, ola_out

    @staticmethod
    def backward(ctx, dy, d_ola_out):
        (wsyn,) = ctx.saved_tensors
        rows, Tc, skip, N, size, shift, device = ctx.meta
        if dy is None and d_ola_out is None:
            return (None,) * 7
        dX, d_ola_in = H.istft_stream_bwd(dy, d_ola_out, wsyn, Tc, skip, N, size, shift, want_ola=ctx.needs_input_grad[1])
        return (dX if ctx.needs_input_grad[0] else None, d_ola_in) + (None,) * 5


def mask_istft_stream(logit, obs, wsyn, ola, skip, N=None, size=1024, shift=256):
    """hip_ops.mask_istft_stream_fwd, differentiable w.r.t. logit and the carry `ola` -> (y [B,K,n], the carry behind)."""
    return _MaskISTFTStream.apply(logit, ola, obs, wsyn, skip, N, size, shift)


def istft_stream(X, wsyn, ola, skip, N=None, size=1024, shift=256):
    """hip_ops.istft_stream_fwd, differentiable w.r.t. X [rows, Tc, F] and the carry `ola` -> (y [rows, n], the carry)."""
    return _ISTFTStream.apply(X, ola, wsyn, skip, N, size, shift)


# ---------------------------------------------------------------- explicit_vad (gated mask head)
# MaskEstimator_v2(explicit_vad=True) (net.py:630, 969-979): the head writes rows of F + 1 logits per (b, k, t), the
# VAD logit v at column 0 and the mask logits l_f behind it; mask = sigmoid(l_f) sigmoid(v).  The Functions below keep
# that [B,K,T,F+1] tensor whole -- the gated kernels read the gate where the GEMM wrote it and write d(v) where the
# Linear's backward reads it -- so neither the gate nor its gradient is ever sliced out or scattered back.
class _MaskHeadGated(torch.autograd.Function):
    """sigmoid + gate + Masking: logit [B,K,T,F+1], obs [B,T,F] -> (mask [B,K,T,F], est, vad_mask [B,K,T])."""

    @staticmethod
    def forward(ctx, logit, obs):
        mask, est, vmask = H.maskhead_gated_fwd(logit, obs)
        ctx.save_for_backward(logit, obs)
        return mask, est, vmask

    @staticmethod
    def backward(ctx, dmask, dest, dvmask):
        logit, obs = ctx.saved_tensors
        return H.maskhead_gated_bwd(dest, dmask, dvmask, logit, obs), None


def mask_head_gated(logit, obs):
    return _MaskHeadGated.apply(logit, obs)


class _SigmoidGated(torch.autograd.Function):
    """mask and vad_mask only (no observation available).  Not routed through _MaskHeadGated as `sigmoid` is through
    _MaskHead: these launches pass est == NULL (no estimate is written or read back), that Function's do not."""

    @staticmethod
    def forward(ctx, logit):
        B, K, T, F1 = logit.shape
        obs = torch.zeros(B, T, F1 - 1, device=logit.device, dtype=torch.complex64)
        mask, _, vmask = H.maskhead_gated_fwd(logit, obs, with_est=False)
        ctx.save_for_backward(logit, obs)
        return mask, vmask

    @staticmethod
    def backward(ctx, dmask, dvmask):
        logit, obs = ctx.saved_tensors
        return H.maskhead_gated_bwd(None, dmask, dvmask, logit, obs)


def sigmoid_gated(logit):
    """logit [B,K,T,F+1] -> (mask [B,K,T,F] = sigmoid(l) sigmoid(v), vad_mask [B,K,T] = sigmoid(v))."""
    return _SigmoidGated.apply(logit)


class _GateBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, vad):
        ctx.save_for_backward(logit, vad)
        return H.gatebce_fwd(logit, vad)

    @staticmethod
    def backward(ctx, g):
        logit, vad = ctx.saved_tensors
        return H.gatebce_bwd(logit, vad, g), None


def gate_bce(logit, vad):
    """mean_{k,t} BCEWithLogits(logit[..., 0], vad) -> [B]: SignalAndVADSigmoidBCE's VAD term on the gate column of
    logit [B,K,T,F+1] (vad [B,K,T])."""
    return _GateBCE.apply(logit, vad.to(device=logit.device, dtype=torch.float32))


# ------------------------------------------------------------------------------ losses
def _fused_absdiff(est, tgt):
    """Partial sums the fused mask-head + iSTFT forward left on `est` for exactly this target."""
    info = getattr(est, "_tssep_absdiff", None)
    if info is not None and info[1] == tgt.data_ptr() and info[2] == tuple(tgt.shape):
        return info[0]
    return None


def _loss_link(est, part):
    """The hand-off to the fused tail that produced `est` (and `part` for this very target), if any."""
    return getattr(est, "_tssep_loss_link", None) if part is not None else None


class _AbsErrorLoss(torch.autograd.Function):
    """log = True: LogMAE, log10(sum_k mean_n |e - t|) (loss.py:244-247); False: MAE, the logarithm's argument
    (loss.py:214-216) -- one forward kernel computes both, and the backward differs in `sums` being None."""

    @staticmethod
    def forward(ctx, est, tgt, log, part=None, link=None):
        loss, sums = H.logmae_finalize(part, *est.shape) if part is not None else H.logmae_fwd(est, tgt)
        ctx.save_for_backward(est, tgt, sums)
        ctx.log, ctx.link = log, link
        return loss if log else sums

    @staticmethod
    def backward(ctx, g):
        est, tgt, sums = ctx.saved_tensors
        if not ctx.log:
            sums = None
        if ctx.link is not None and ctx.link.payload is None:     # the tail's backward forms this gradient itself
            ctx.link.payload = (est, tgt, sums, g)
            return _dummy_grad(est), None, None, None, None
        return H.logmae_bwd(est.contiguous(), tgt.contiguous(), sums, g), None, None, None, None


class _PairLoss(torch.autograd.Function):
    """f(sum_k C[k, perm(k)]) on the pairwise costs C[i, j] = mean_n |e_i - t_j|^p, f = log10 or the identity:
    pit=True: perm = the best assignment per utterance (= the best permutation of pt.ops.losses.pit_loss, f being
    monotone), found on the device; pit=False: the identity, on the diagonal-only pass.  One pass over est and tgt
    either way.  -> (loss [B], perm int32 [B,K]); the permutation is a constant of the backward."""

    @staticmethod
    def forward(ctx, est, tgt, p, log, pit):
        est, tgt = est.contiguous(), tgt.contiguous()
        part = H.pair_cost_fwd(est, tgt, p, diag_only=not pit)
        _, perm, sums, loss = H.pit_assign(part, est.shape[-1], pit=pit, log=log, want_cost=False)
        ctx.save_for_backward(est, tgt, perm, sums)
        ctx.meta = (p, log, pit)
        ctx.mark_non_differentiable(perm)
        return loss, perm

    @staticmethod
    def backward(ctx, g, _gperm):
        est, tgt, perm, sums = ctx.saved_tensors
        p, log, pit = ctx.meta
        return H.pair_loss_bwd(est, tgt, perm if pit else None, sums if log else None, g, p), None, None, None, None


def pair_loss(est, tgt, p=1, log=False, pit=True):
    """est, tgt [B,K,N] (K <= 8) -> (loss [B], perm int32 [B,K]); perm[b, i] = the target row matched to estimate row i."""
    H._check_pit_k(est.shape[-2])
    return _PairLoss.apply(est, tgt, int(p), bool(log), bool(pit))


def log_mae(est, tgt, pit=False):
    if pit:
        return pair_loss(est, tgt, 1, True, True)[0]
    part = _fused_absdiff(est, tgt)
    return _AbsErrorLoss.apply(est, tgt, True, part, _loss_link(est, part))


def mae(est, tgt, pit=False):
    if pit:
        return pair_loss(est, tgt, 1, False, True)[0]
    part = _fused_absdiff(est, tgt)
    return _AbsErrorLoss.apply(est, tgt, False, part, _loss_link(est, part))


def mse(est, tgt, pit=False):
    """sum_k mean_n (e - t)^2 -> [B] (loss.py:183-190), with pit the minimum over the speaker permutations."""
    return pair_loss(est, tgt, 2, False, pit)[0]


class _SDRLoss(torch.autograd.Function):
    """-(1/K) sum_i value[i, perm(i)], value the SDR or SI-SDR in dB: one pass over est and tgt leaves the
    float64 statistics, a small launch maps them to the K x K costs, tssep_pit_assign matches (pit=False: the identity
    on the diagonal-only pass), and the backward is linear in est and tgt with two coefficients per row.
    -> (loss [B], perm int32 [B,K], values dB [B,K]); perm and values are constants of the backward."""

    @staticmethod
    def forward(ctx, est, tgt, scale_invariant, sdr_max, eps, pit):
        est, tgt = est.contiguous(), tgt.contiguous()
        loss, perm, values, stat = H.sdr_forward(est, tgt, scale_invariant, sdr_max, eps, pit)
        ctx.save_for_backward(est, tgt, perm, stat)
        ctx.meta = (scale_invariant, sdr_max, eps, pit)
        ctx.mark_non_differentiable(perm, values)
        return loss, perm, values

    @staticmethod
    def backward(ctx, g, _gperm, _gvalues):
        est, tgt, perm, stat = ctx.saved_tensors
        scale_invariant, sdr_max, eps, pit = ctx.meta
        return H.sdr_bwd(est, tgt, perm if pit else None, stat, g, scale_invariant, sdr_max, eps), None, None, None, \
            None, None


def sdr_loss(est, tgt, scale_invariant=True, sdr_max=None, eps=1e-8, pit=False):
    """est, tgt [B,K,N] or [K,N] (K <= 8) -> (loss [B] = the negated mean over speakers of the matched SDR / SI-SDR in dB,
    perm int32 [B,K], values dB [B,K]); a [K,N] input gives the same without the batch axis.  Differentiable in est."""
    H._check_pit_k(est.shape[-2])
    if est.dim() == 2:
        loss, perm, values = _SDRLoss.apply(est[None], tgt[None], bool(scale_invariant), sdr_max, float(eps), bool(pit))
        return loss[0], perm[0], values[0]
    return _SDRLoss.apply(est, tgt, bool(scale_invariant), sdr_max, float(eps), bool(pit))


class _SpecMSE(torch.autograd.Function):
    """FreqMSE on an estimate in memory: sum_k C[k, perm(k)] on C[i, j] = sum_t mean_f |E_i - S_j|^2, est [B,K,T,F]
    complex64 | complex128, tgt complex64; pit as _PairLoss (the same assignment kernel).  -> (loss [B], perm)."""

    @staticmethod
    def forward(ctx, est, tgt, pit):
        est, tgt = est.contiguous(), tgt.contiguous()
        part = H.specmse_fwd(est, tgt, diag_only=not pit)
        _, perm, _, loss = H.pit_assign(part, est.shape[-1], pit=pit, log=False, want_cost=False)
        ctx.save_for_backward(est, tgt, perm)
        ctx.pit = pit
        ctx.mark_non_differentiable(perm)
        return loss, perm

    @staticmethod
    def backward(ctx, g, _gperm):
        est, tgt, perm = ctx.saved_tensors
        return H.specmse_bwd(est, tgt, perm if ctx.pit else None, g), None, None


def spec_mse(est, tgt, pit=False):
    """est, tgt [B,K,T,F] complex (K <= 8) -> (loss [B], perm int32 [B,K]), differentiable in est."""
    H._check_pit_k(est.shape[-3])
    return _SpecMSE.apply(est, tgt, bool(pit))


class _MaskSpecMSE(torch.autograd.Function):
    """sigmoid (net.py:983) -> Masking (enhancer.py:98-100) -> FreqMSE as ONE kernel each way: logit, Observation and
    target are read once, mask and estimate never written, no inverse STFT.  The head link as in _MaskISTFT: d(logit)
    is stored where the final Linear's backward reads it."""

    @staticmethod
    def forward(ctx, logit, obs, tgt, pit, head_link=None):
        logit, obs, tgt = logit.contiguous(), obs.contiguous(), tgt.contiguous()
        part = H.mask_specmse_fwd(logit, obs, tgt, diag_only=not pit)
        _, perm, _, loss = H.pit_assign(part, logit.shape[-1], pit=pit, log=False, want_cost=False)
        ctx.save_for_backward(logit, obs, tgt, perm)
        ctx.pit, ctx.link = pit, head_link
        ctx.mark_non_differentiable(perm)
        return loss, perm

    @staticmethod
    def backward(ctx, g, _gperm):
        logit, obs, tgt, perm = ctx.saved_tensors
        head_link = ctx.link
        to_head = head_link is not None and tuple(head_link.shape) == tuple(logit.shape)
        d = H.mask_specmse_bwd(logit, obs, tgt, perm if ctx.pit else None, g,
                               iperm=head_link.iperm if to_head else None, bt_major=to_head)
        if to_head:                                     # written where the Linear's backward reads it
            head_link.payload = d if head_link.payload is None else head_link.payload + d
            d = _dummy_grad(logit)
        return d, None, None, None, None


def mask_spec_mse(logit, obs, tgt, pit=False):
    """logit [B,K,T,F], obs complex64 [B,T,F], tgt complex64 [B,K,T,F] (K <= 8) -> (loss [B], perm int32 [B,K]) of
    FreqMSE on sigmoid(logit) * obs, differentiable in logit only."""
    H._check_pit_k(logit.shape[-3])
    fold = H.FOLD_TAIL and logit.requires_grad
    head_link = getattr(logit, "_tssep_head_link", None) if fold and H.FOLD_TAIL != 2 else None
    return _MaskSpecMSE.apply(logit, obs, tgt, bool(pit), head_link)


class _VadBCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, vad):
        loss, xmean = H.vadbce_fwd(logit, vad)
        ctx.save_for_backward(xmean, vad)
        ctx.F = logit.shape[-1]
        return loss

    @staticmethod
    def backward(ctx, g):
        xmean, vad = ctx.saved_tensors
        return H.vadbce_bwd(xmean, vad, g, ctx.F), None


def vad_bce(logit, vad):
    return _VadBCE.apply(logit, vad)


# ---------------------------------------------------------- learned speaker embeddings (net.py:19-158, 250-330)
class _InstNorm(torch.autograd.Function):
    """InstanceNorm (mode 0) / InstanceNorm_v2 (mode 1) over the last (axis 0) or the time (axis 1) dimension."""

    @staticmethod
    def forward(ctx, x, axis, mode, unbiased):
        y, mean, rscale, xinfo = H.instnorm_fwd(x, axis, mode, unbiased)
        ctx.save_for_backward(xinfo[0], mean, rscale)
        ctx.meta = (xinfo[1], tuple(x.shape), axis, mode, unbiased)
        return y

    @staticmethod
    def backward(ctx, dy):
        xv, mean, rscale = ctx.saved_tensors
        ld, shape, axis, mode, unbiased = ctx.meta
        return H.instnorm_bwd(dy, (xv, ld), mean, rscale, shape, axis, mode, unbiased), None, None, None


def instance_norm(x, axis, mode, unbiased=False):
    return _InstNorm.apply(x.to(torch.float32), axis, mode, bool(unbiased))


def _affine_wgrads(dv, ld_d, xv, ld_x, R, weight, bias):
    """dW and db of one affine layer (bias may be None): straight into the flat gradient bucket when the parameters live
    there (-> None, None), through autograd otherwise."""
    Nout, P = weight.shape
    params = [weight] if bias is None else [weight, bias]
    sinks = [_grad_sink(p) for p in params]
    # honours_overlap_wgrad=False, fused=False, no fork: what these layers launch today; changing it is another PR
    direct = _is_direct(sinks, False)
    grads = _linear_wgrads(dv, ld_d, xv, ld_x, Nout, P, R, (sinks + [None])[:2] if direct else None, False,
                           bias=bias is not None)
    if direct:
        _notify_grads(params)
    return grads


def _affine_fwd(xv, ld_x, R, weight, bias):
    """-> (y, ld_y): rows of x W^T + b in a padded buffer."""
    Nout, P = weight.shape
    wv, ld_w = H.rows_view(weight.detach())
    y, ld_y = H.padded(R, Nout, xv.device, zero=True)
    H.gemm(xv, ld_x, wv, ld_w, y, ld_y, R, Nout, P, bias=bias.detach() if bias is not None else None)
    return y, ld_y


def _affine_dgrad(dv, ld_d, R, weight):
    """-> (dx, ld): dv W in a padded buffer."""
    Nout, P = weight.shape
    wT, ld_t = H.derived("affine_T", [weight], lambda: H.transposed(H.rows_view(weight.detach())[0], Nout, P))
    dx, ld_dx = H.padded(R, P, dv.device, zero=True)
    H.gemm(dv, ld_d, wT, ld_t, dx, ld_dx, R, P, Nout)
    return dx, ld_dx


_AffineMeta = collections.namedtuple("_AffineMeta", "R ld_x x_shape")
_AuxMLPMeta = collections.namedtuple("_AuxMLPMeta", "N S C ld_x ld1 ld2 ldm")


class _Affine(torch.autograd.Function):
    """net.Linear (net.py:19-43): y = x W^T + b over the rows of x [..., idim]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xv, ld_x = H.rows_view(x)
        R = xv.shape[0]
        y, ld_y = _affine_fwd(xv, ld_x, R, weight, bias)
        ctx.save_for_backward(xv)
        ctx.params = (weight, bias)
        ctx.meta = _AffineMeta(R, ld_x, tuple(x.shape))
        return y[:, :weight.shape[0]].reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        (xv,) = ctx.saved_tensors
        weight, bias = ctx.params
        m = ctx.meta
        dv, ld_d = H.rows_view(dy)
        dw, db = _affine_wgrads(dv, ld_d, xv, m.ld_x, m.R, weight, bias)
        dx = None
        if ctx.needs_input_grad[0]:
            dxb, _ = _affine_dgrad(dv, ld_d, m.R, weight)
            dx = dxb[:, :weight.shape[1]].reshape(m.x_shape)
        return dx, dw, db


def affine(x, weight, bias=None):
    return _Affine.apply(x.to(torch.float32), weight, bias)


class _AuxMLP(torch.autograd.Function):
    """AuxNet (net.py:118-149) on PACKED enrolment rows x [N, idim] (all sequences concatenated, row0 [S+1] their
    device prefix): Linear, ReLU, Linear, ReLU, length-aware mean, and the last (affine) Linear AFTER the mean --
    mean(h) W3^T + b3 on [S, idim] equals the reference's mean(h W3^T + b3) and saves a third of the MLP's FLOPs.  The
    second ReLU is fused into the mean's read.  No gradient goes to the enrolment input."""

    @staticmethod
    def forward(ctx, x, row0, S, w1, b1, w2, b2, w3, b3):
        xv, ld_x = H.rows_view(x)
        N, C = xv.shape[0], w1.shape[0]
        h1, ld1 = _affine_fwd(xv, ld_x, N, w1, b1)
        H.relu_fwd(h1, ld1, N, C)
        z2, ld2 = _affine_fwd(h1, ld1, N, w2, b2)
        m, ldm = H.segment_mean_fwd(z2, ld2, row0, S, C, relu=True)
        y, ld_y = _affine_fwd(m, ldm, S, w3, b3)
        ctx.save_for_backward(xv, h1, z2, m, row0)
        ctx.params = (w1, b1, w2, b2, w3, b3)
        ctx.meta = _AuxMLPMeta(N, S, C, ld_x, ld1, ld2, ldm)
        return y[:, :w3.shape[0]]

    @staticmethod
    def backward(ctx, dy):
        xv, h1, z2, m, row0 = ctx.saved_tensors
        w1, b1, w2, b2, w3, b3 = ctx.params
        g = ctx.meta
        dv, ld_d = H.rows_view(dy)
        dw3, db3 = _affine_wgrads(dv, ld_d, m, g.ldm, g.S, w3, b3)
        dm, ld_dm = _affine_dgrad(dv, ld_d, g.S, w3)
        dz2, ld_dz2 = H.segment_mean_bwd(dm, ld_dm, z2, g.ld2, row0, g.S, g.N, g.C, relu=True)
        dw2, db2 = _affine_wgrads(dz2, ld_dz2, h1, g.ld1, g.N, w2, b2)
        dh1, ld_dh1 = _affine_dgrad(dz2, ld_dz2, g.N, w2)
        dz1, ld_dz1 = H.relu_bwd(dh1, ld_dh1, h1, g.ld1, g.N, g.C)
        dw1, db1 = _affine_wgrads(dz1, ld_dz1, xv, g.ld_x, g.N, w1, b1)
        return None, None, None, dw1, db1, dw2, db2, dw3, db3


def aux_mlp(x, row0, S, linears):
    """x packed [N, idim] -> [S, odim]; linears: the three torch.nn.Linear containers of AuxNet.net."""
    l1, l2, l3 = linears
    return _AuxMLP.apply(x.to(torch.float32), row0, S, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
