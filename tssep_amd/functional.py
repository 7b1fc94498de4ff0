"""torch.autograd.Function wrappers around the HIP kernels (hip_ops).

Each Function mirrors one ATen-level operator group of the reference hot path (SURVEY.md
section 2.2) with an explicit backward; autograd is only the glue that chains them.
"""
import numpy as np
import torch

from . import hip_ops as H


def _pad4(n):
    return H.round_up(n, 4)


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


# ------------------------------------------------------------------------------ RNNP
class _RNNP(torch.autograd.Function):
    """One RNNP_packed layer (tssep/train/rnnp.py:88-96,146-168): BLSTM + Linear (+ tanh).

    x: [R, ld_x] buffer view, rows (n, t) for N sequences of T frames, I valid columns.
    Output: [R, hdim] rows (padded leading dimension), or the speaker-combined layout
    [B, T, K*hdim] when ``combine=K`` (net.py:608-611 fused into the projection's store).
    ``dropout_p`` > 0: the Tanh behind this layer is an ACTIVE dropout site (rnnp.py:98-100, net.py:623-625) -- the
    projection stores plainly (act = 0) and one pass over y applies mask, 1 / (1 - p) and Tanh in place; the backward
    regenerates the mask from the {seed, draw} pair the forward drew (hip_ops.dropout_draw)."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r, w_proj, b_proj,
                N, T, act, combine, in_tanh=0, in_link=None, out_link=None, dropout_p=0.0):
        dev = x.device
        Hh = w_hh.shape[1]
        I = w_ih.shape[1]
        hdim = w_proj.shape[0]
        xv, ld_x = H.rows_view(x)
        R = N * T
        assert xv.shape[0] == R and xv.shape[1] >= I, (xv.shape, R, I)
        lstm_params = [w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r]
        pk = H.derived("lstm_pack", lstm_params, lambda: H.lstm_pack(lstm_params, Hh, I))
        gates = torch.empty(R, 8 * Hh, device=dev, dtype=torch.float32)
        H.gemm(xv, ld_x, pk["wih_p"], pk["ld_i"], gates, 8 * Hh, R, 8 * Hh, I, bias=pk["bias_p"])
        Hp = _pad4(Hh)
        cell = torch.empty(N, T, 2, Hh, device=dev, dtype=torch.float32)
        hout = (torch.zeros if Hp != Hh else torch.empty)(R, 2 * Hp, device=dev, dtype=torch.float32)
        # the plan and BOTH directions' W_hh layouts are fetched here, once: the backward launches from what ctx keeps (a
        # step captured without prepare_derived builds a layout at every ask)
        plan = H.recurrence_plan(N, T, Hh, H.n_cus(dev))
        whh = H.recurrence_packs(plan, w_hh, w_hh_r, Hh, pk, memo=True)
        H.recurrence_launch(plan["fwd"], "fwd", gates, cell, hout, 2 * Hp, Hp, whh["fwd"], N, T, Hh)
        # projection weight in the (possibly padded) [hdim, 2*Hp] column layout of hout
        wp = H.derived("proj_layout", [w_proj], lambda: _proj_layout(w_proj, Hh, Hp))
        drop = float(dropout_p) if dropout_p else 0.0
        assert not drop or (act == 1 and out_link is None), "dropout_p: a site is the Tanh behind the layer, never folded"
        store_act = 0 if drop else act
        if combine:
            K = combine
            B = N // K
            y = torch.empty(B * T, K * hdim, device=dev, dtype=torch.float32)
            H.gemm(hout, 2 * Hp, wp, 2 * Hp, y, 0, R, hdim, 2 * Hp, bias=b_proj.detach(), act=store_act,
                   remap=dict(T=T, K=K, sb=T * K * hdim, sk=hdim, st=K * hdim))
            ld_y = K * hdim
        else:
            y, ld_y = H.padded(R, hdim, dev, zero=True)
            H.gemm(hout, 2 * Hp, wp, 2 * Hp, y, ld_y, R, hdim, 2 * Hp, bias=b_proj.detach(), act=store_act)
        used = None
        if drop:
            used = H.dropout_draw(dev)
            H.dropout_tanh_fwd(y, y, R, hdim, ld_y, combine if combine else 1, T, bool(combine), drop, used)
        ctx.drop = (drop, used)
        ctx.save_for_backward(xv, gates, cell, hout, y, wp)
        ctx.params = (w_ih, w_hh, b_ih, b_hh, w_ih_r, w_hh_r, b_ih_r, b_hh_r, w_proj, b_proj)
        ctx.recurrence = (plan["bwd"], whh["bwd"])
        ctx.meta = (N, T, I, Hh, Hp, hdim, ld_x, ld_y, act, combine)
        # Tanh-backward fold (see rnnp_layer): in_link = the link my producer hung on x, out_link = the one my
        # consumer may answer on.  Both are decided again in backward, when it is known who else uses the tensors.
        ctx.fold = (int(in_tanh) if in_link is not None else 0, in_link, out_link)
        assert out_link is None or act == 1, "out_link: only behind the fused Tanh"
        ctx.x_shape = x.shape
        return y if combine else y[:, :hdim]

    @staticmethod
    def backward(ctx, dy):
        xv, gates, cell, hout, y, wp = ctx.saved_tensors
        N, T, I, Hh, Hp, hdim, ld_x, ld_y, act, combine = ctx.meta
        dev = dy.device
        R = N * T
        K = combine if combine else 1
        # d(pre-activation) of the projection, rows (n,t) x hdim, contiguous
        in_tanh, in_link, out_link = ctx.fold
        folded = out_link.take() if out_link is not None else None
        if folded is not None:
            # the consumer's d(input) GEMM already applied 1 - y^2 and wrote dense rows (n,t) x hdim; `dy` is the
            # dummy it returned -- unless y has ANOTHER consumer (auxiliary loss): autograd then summed that
            # consumer's plain d(y) onto the dummy's zeros, and it goes through the Tanh backward here
            dz = folded.view(R, hdim)
            if not _is_dummy(dy):
                dyc = dy.contiguous() if combine else _dense_rows(dy, hdim)
                yc = y if combine else _dense_rows(y[:, :hdim], hdim)
                dz = dz + H.tanh_bwd(dyc, yc, R, hdim, K, T, bool(combine))
        elif act:
            dyc = dy.contiguous() if combine else _dense_rows(dy, hdim)
            yc = y if combine else _dense_rows(y[:, :hdim], hdim)
            drop, used = ctx.drop
            if drop:
                dz = H.dropout_tanh_bwd(dyc, yc, R, hdim, K, T, bool(combine), drop, used)
            else:
                dz = H.tanh_bwd(dyc, yc, R, hdim, K, T, bool(combine))
        else:
            if combine:   # layout change only: reuse tanh_bwd's gather with y = 0
                dz = H.tanh_bwd(dy.contiguous(), torch.zeros_like(dy), R, hdim, K, T, True)
            else:
                # (a strided [R, hdim] view of a padded buffer -- what the conditioning's backward hands the pre-net --
                # goes to the GEMMs as it is: rows_view only copies what is not 16-byte-row addressable)
                dz = dy if dy.dim() == 2 else dy.reshape(-1, hdim)
        dz, ld_dz = H.rows_view(dz)
        G = 8 * Hh
        params = ctx.params
        sinks = [_grad_sink(p) for p in params]
        direct = all(s_ is not None for s_ in sinks) and H.OVERLAP_WGRAD
        main = torch.cuda.current_stream()
        side = H.side_stream(dev, R) if direct else main

        # ---- projection weight / bias gradients (side stream when direct)
        def proj_wgrads():
            if direct and Hp == Hh and H.fused_colsum():
                # the bias gradient (column sums of dz) rides on the weight-gradient GEMM as a virtual ones
                # column of hout: one pass over dz instead of two, and N = 600 -> 601 costs no extra tile
                part, S = H.wgrad(dz, ld_dz, hout, 2 * Hp, hdim, 2 * Hp, R, with_colsum=True)
                H.reduce_splits_bias(part, S, hdim, 2 * Hp, H.round_up(2 * Hp + 1, 4), sinks[8], sinks[9],
                                     accumulate=True)
                return None, None
            part, S = H.wgrad(dz, ld_dz, hout, 2 * Hp, hdim, 2 * Hp, R)
            if direct and Hp == Hh:
                H.reduce_splits(part, S, hdim * 2 * Hp, sinks[8], accumulate=True)
                H.colsum(dz, ld_dz, R, hdim, out=sinks[9], accumulate=True)
                return None, None
            dwp = torch.empty(hdim, 2 * Hp, device=dev, dtype=torch.float32)
            H.reduce_splits(part, S, hdim * 2 * Hp, dwp)
            d_w = _proj_unlayout(dwp, Hh, Hp)
            d_b = H.colsum(dz, ld_dz, R, hdim)
            if direct:
                sinks[8].add_(d_w)
                sinks[9].add_(d_b)
                return None, None
            return d_w, d_b

        if direct:
            side.wait_stream(main)
            for t_ in (dz, hout):
                t_.record_stream(side)
            with torch.cuda.stream(side):
                d_w_proj, d_b_proj = proj_wgrads()
        else:
            d_w_proj, d_b_proj = proj_wgrads()
        # ---- critical path: dhout, BPTT (gates <- d pre-activations)
        dhout = torch.empty(R, 2 * Hp, device=dev, dtype=torch.float32)
        w_proj = params[8]      # (the builds read the parameters, not this step's tensors: hip_ops.prepare_derived)
        wpT, ld_t = H.derived("proj_T", [w_proj], lambda: H.transposed(
            H.derived("proj_layout", [w_proj], lambda: _proj_layout(w_proj, Hh, Hp)), hdim, 2 * Hp))
        H.gemm(dz, ld_dz, wpT, ld_t, dhout, 2 * Hp, R, 2 * Hp, hdim)
        planned, whh_bwd = ctx.recurrence
        H.recurrence_launch(planned, "bwd", gates, cell, dhout, 2 * Hp, Hp, whh_bwd, N, T, Hh)

        # ---- LSTM weight / bias gradients from dgates (side stream when direct)
        def lstm_wgrads():
            dwhh = torch.empty(2, 4 * Hh * Hh, device=dev, dtype=torch.float32)
            for d in range(2):   # dgates_t paired with h_{t-1} (forward dir) / h_{t+1} (reverse)
                part, S = H.wgrad((gates, d * 4 * Hh), G, (hout, d * Hp), 2 * Hp, 4 * Hh, Hh, R,
                                  b_kshift=(-1 if d == 0 else 1), kperiod=T)
                H.reduce_splits(part, S, 4 * Hh * Hh, dwhh[d])
            # dW_ih and (split-bf16 GEMM) the bias gradient in ONE pass over dgates: a virtual ones
            # column of x makes column I of the partials the column sums
            fused = H.fused_colsum()
            part, S = H.wgrad(gates, G, xv, ld_x, G, I, R, with_colsum=fused)
            ldp = H.round_up(I + 1, 4) if fused else I
            if fused:
                cs, cs_ld, cs_S, cs_stride = (part, I), ldp, S, G * ldp
            else:
                cs, cs_ld, cs_S, cs_stride = H.colsum(gates, G, R, G), 1, 1, 0
            if direct:
                H.lstm_unpack(dwhh, Hh, 1, 0, Hh, Hh, sinks[1], sinks[5], accumulate=True)
                H.lstm_unpack(part, ldp, S, G * ldp, Hh, I, sinks[0], sinks[4], accumulate=True)
                for a_, b_ in ((2, 6), (3, 7)):      # b_ih and b_hh receive the same gradient
                    H.lstm_unpack(cs, cs_ld, cs_S, cs_stride, Hh, 1, sinks[a_], sinks[b_], accumulate=True)
                return (None,) * 8
            new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
            d_whh, d_whh_r = new(4 * Hh, Hh), new(4 * Hh, Hh)
            H.lstm_unpack(dwhh, Hh, 1, 0, Hh, Hh, d_whh, d_whh_r)
            d_wih, d_wih_r = new(4 * Hh, I), new(4 * Hh, I)
            H.lstm_unpack(part, ldp, S, G * ldp, Hh, I, d_wih, d_wih_r)
            d_b, d_b_r = new(4 * Hh), new(4 * Hh)
            H.lstm_unpack(cs, cs_ld, cs_S, cs_stride, Hh, 1, d_b, d_b_r)
            return d_wih, d_whh, d_b, d_b.clone(), d_wih_r, d_whh_r, d_b_r, d_b_r.clone()

        if direct:
            side.wait_stream(main)
            for t_ in (gates, hout, xv):
                t_.record_stream(side)
            with torch.cuda.stream(side):
                lstm_grads = lstm_wgrads()
            _notify_grads(params)                    # (10 tensors: both directions' LSTM weights + the projection)
        else:
            lstm_grads = lstm_wgrads()
        dx = None
        if ctx.needs_input_grad[0]:
            lstm_params = list(params[:8])

            def wih_t():
                pk_ = H.derived("lstm_pack", lstm_params, lambda: H.lstm_pack(lstm_params, Hh, I))
                return H.transposed(pk_["wih_p"].view(G, pk_["ld_i"]), G, I)
            wihT, ld_t = H.derived("wih_T", [params[0], params[4]], wih_t)
            if in_tanh and not in_link.observed():
                # my input is a Tanh output: its backward rides on this GEMM's store and the result travels on
                # the link; x receives a dummy (its true gradient is never formed -- hence not when it is watched)
                Kc = in_tanh
                assert I % 4 == 0 and I % Kc == 0 and ld_x == I, (I, Kc, ld_x)
                dxb = torch.empty(R, I, device=dev, dtype=torch.float32)
                remap = None
                if Kc > 1:    # rows (b,t) x (k, hdim) -> rows (b,k,t) x hdim (inverse of net.py:608-611)
                    hd = I // Kc
                    remap = dict(T=T, K=1, sb=Kc * T * hd, sk=0, st=hd, cm=hd, co=T * hd)
                H.gemm(gates, G, wihT, ld_t, dxb, 0 if remap else I, R, I, G, act=2, aux=(xv, ld_x), remap=remap)
                # (accumulated, like head_link below: the activation may feed TWO folded consumers -- ADVICE r4)
                in_link.payload = dxb if in_link.payload is None else in_link.payload + dxb.view_as(in_link.payload)
                dx = _dummy_grad(xv, ctx.x_shape)
            else:
                dxb, ld_dx = H.padded(R, I, dev, zero=True)
                H.gemm(gates, G, wihT, ld_t, dxb, ld_dx, R, I, G)
                dx = dxb[:, :I]
                if tuple(ctx.x_shape) != tuple(dx.shape):
                    dx = dx.reshape(ctx.x_shape)
        return (dx, *lstm_grads, d_w_proj, d_b_proj, None, None, None, None, None, None, None, None)


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


def _dense_rows(t, cols):
    t = t if t.dim() == 2 else t.reshape(-1, cols)
    return t.contiguous()


def _proj_layout(w_proj, Hh, Hp):
    w = w_proj.detach()
    if Hp == Hh and w.is_contiguous() and w.data_ptr() % 16 == 0:
        return w
    out = torch.zeros(w.shape[0], 2 * Hp, device=w.device, dtype=torch.float32)
    out[:, :Hh] = w[:, :Hh]
    out[:, Hp:Hp + Hh] = w[:, Hh:]
    return out


def _proj_unlayout(dwp, Hh, Hp):
    if Hp == Hh:
        return dwp
    return torch.cat([dwp[:, :Hh], dwp[:, Hp:Hp + Hh]], dim=1).contiguous()


def rnnp_layer(x, lstm, linear, N, T, act=0, combine=0, in_tanh=0, dz_given=False, dropout_p=0.0):
    """x rows (n,t); lstm = torch.nn.LSTM parameter container, linear = nn.Linear container.
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
    in_link = getattr(x, "_tssep_tanh_link", None) if in_tanh else None
    if in_link is not None and not (x.requires_grad and torch.is_grad_enabled()):
        in_link = None
    dropout_p = float(dropout_p) if (dropout_p and act == 1) else 0.0
    out_link = _Link() if (dz_given and act == 1 and not dropout_p and torch.is_grad_enabled()) else None
    out = _RNNP.apply(x, lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0,
                      lstm.weight_ih_l0_reverse, lstm.weight_hh_l0_reverse,
                      lstm.bias_ih_l0_reverse, lstm.bias_hh_l0_reverse,
                      linear.weight, linear.bias, N, T, act, combine, in_tanh, in_link, out_link, dropout_p)
    if out_link is not None and out.requires_grad:
        out_link.out = weakref.ref(out)
        out._tssep_tanh_link = out_link
    return out


# ---------------------------------------------------------------------- conditioning
class _Cond(torch.autograd.Function):
    """tssep/train/net.py:862-896 (+ trial fold :913-924).  pre rows (b,t) -> rows (b,tr,k,t).
    An embedding that requires a gradient (aux_net, a trainable normalised embedding) gets it from one more launch over
    dxs (hip_ops.cond_aux_bwd); a fixed embedding makes exactly the calls it always made."""

    @staticmethod
    def forward(ctx, pre, aux, B, K, T, trials, combination):
        F = pre.shape[-1]
        pv, ld_pre = H.rows_view(pre)
        xs, ld, info = H.cond_fwd(pv, ld_pre, aux.detach(), B, K, T, F, trials, combination)
        W = F if combination == "mul" else F + aux.shape[-1]
        ctx.info = info
        ctx.meta = (B, K, T, F, trials, combination, ld)
        ctx.aux_grad = None
        if aux.requires_grad:
            ctx.aux_grad = (tuple(aux.shape), (pv, ld_pre) if combination == "mul" else None)
        return xs[:, :W]

    @staticmethod
    def backward(ctx, dxs):
        B, K, T, F, trials, combination, ld = ctx.meta
        dv, ld_d = H.rows_view(dxs)
        dpre, ldp = H.cond_bwd(dv, ld_d, ctx.info, B, K, T, F, trials, combination)
        d_aux = None
        if ctx.aux_grad is not None and ctx.needs_input_grad[1]:
            shape, pre = ctx.aux_grad
            pv, ld_pre = pre if pre is not None else (None, 0)
            d_aux = H.cond_aux_bwd(dv, ld_d, pv, ld_pre, B, K, T, F, shape[-1], trials, combination).view(shape)
        return dpre[:, :F], d_aux, None, None, None, None, None


def condition(pre, aux, B, K, T, trials, combination):
    return _Cond.apply(pre, aux, B, K, T, trials, combination)


# ------------------------------------------------------------------------ final linear
def _head_grads(ctx, draw):
    """d(raw) [R, Nout] of the final Linear -> (dx, dw, db): the weight gradient and the bias column sums (straight into
    the optimizer's bucket on the side stream where that is set up: dw = db = None then) and the d(input) GEMM.  Shared
    by _Head and _HeadMasks; ctx carries saved_tensors (xv, wv), params, meta and x_shape."""
    xv, wv = ctx.saved_tensors[:2]
    ld_x, ld_w, P, R, Nout = ctx.meta[-5:]
    dev = draw.device
    dv, ld_d = H.rows_view(draw)
    sw, sb = _grad_sink(ctx.params[0]), _grad_sink(ctx.params[1])
    direct = sw is not None and sb is not None and H.OVERLAP_WGRAD
    if direct:
        main, side = torch.cuda.current_stream(), H.side_stream(dev, R)
        side.wait_stream(main)
        for t_ in (dv, xv):
            t_.record_stream(side)
        with torch.cuda.stream(side):
            if H.fused_colsum():
                part, S = H.wgrad(dv, ld_d, xv, ld_x, Nout, P, R, with_colsum=True)
                H.reduce_splits_bias(part, S, Nout, P, H.round_up(P + 1, 4), sw, sb, accumulate=True)
            else:
                part, S = H.wgrad(dv, ld_d, xv, ld_x, Nout, P, R)
                H.reduce_splits(part, S, Nout * P, sw, accumulate=True)
                H.colsum(dv, ld_d, R, Nout, out=sb, accumulate=True)
        dw = db = None
        _notify_grads(ctx.params)
    else:
        part, S = H.wgrad(dv, ld_d, xv, ld_x, Nout, P, R)
        dw = torch.empty(Nout, P, device=dev, dtype=torch.float32)
        H.reduce_splits(part, S, Nout * P, dw)
        db = H.colsum(dv, ld_d, R, Nout)
    dxb, ld_dx = H.padded(R, P, dev, zero=True)
    weight = ctx.params[0]
    wvT, ld_t = H.derived("head_T", [weight], lambda: H.transposed(H.rows_view(weight.detach())[0], Nout, P))
    H.gemm(dv, ld_d, wvT, ld_t, dxb, ld_dx, R, P, Nout)
    dx = dxb[:, :P]
    if tuple(ctx.x_shape) != tuple(dx.shape):
        dx = dx.reshape(ctx.x_shape)
    return dx, dw, db


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
        ctx.meta = (B, K, T, F, trials, Fr, spk_rows, ld_x, ld_w, P, R, Nout)
        ctx.x_shape = x.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        perm, iperm = ctx.aux
        B, K, T, F, trials, Fr, spk_rows, _, _, _, R, Nout = ctx.meta
        draw = ctx.link.take() if ctx.link is not None else None
        if draw is None:
            draw = H.logit_map_bwd(dout, perm, iperm, B, trials, K, T, F, Fr, spk_rows).view(R, Nout)
        elif not _is_dummy(dout):      # the fused tail wrote its part already laid out; someone else used logit too
            draw = draw + H.logit_map_bwd(dout, perm, iperm, B, trials, K, T, F, Fr, spk_rows).view(R, Nout)
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
        ctx.meta = (B, K, M, T, F, trials, Fr, spk_rows, ld_x, ld_w, P, R, Nout)
        ctx.x_shape = x.shape
        ctx.set_materialize_grads(False)          # d(logit) is None when nobody else used the logit
        return logit, mask

    @staticmethod
    def backward(ctx, dlogit, dmask):
        perm, iperm = ctx.aux
        B, K, M, T, F, trials, Fr, spk_rows, _, _, _, R, Nout = ctx.meta
        mask = ctx.saved_tensors[2]
        if dmask is None:                         # only the logit was used: the same kernel with d(mask) = 0
            dmask = torch.zeros_like(mask)
        draw = H.mask_map_bwd(dmask, mask, dlogit, perm, iperm, B, trials, K, M, T, F, Fr, spk_rows).view(R, Nout)
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
    """dW = dv^T xv and db = column sums of dv for y = x W^T + b: straight into the flat gradient bucket when the
    parameters live there (-> None, None), through autograd otherwise."""
    Nout, P = weight.shape
    sw = _grad_sink(weight)
    sb = _grad_sink(bias) if bias is not None else None
    direct = sw is not None and (bias is None or sb is not None)
    part, S = H.wgrad(dv, ld_d, xv, ld_x, Nout, P, R)
    if direct:
        H.reduce_splits(part, S, Nout * P, sw, accumulate=True)
        if bias is not None:
            H.colsum(dv, ld_d, R, Nout, out=sb, accumulate=True)
        _notify_grads([weight] + ([bias] if bias is not None else []))
        return None, None
    dw = torch.empty(Nout, P, device=dv.device, dtype=torch.float32)
    H.reduce_splits(part, S, Nout * P, dw)
    return dw, (H.colsum(dv, ld_d, R, Nout) if bias is not None else None)


def _affine_fwd(xv, ld_x, R, weight, bias, out=None):
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


class _Affine(torch.autograd.Function):
    """net.Linear (net.py:19-43): y = x W^T + b over the rows of x [..., idim]."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        xv, ld_x = H.rows_view(x)
        R = xv.shape[0]
        y, ld_y = _affine_fwd(xv, ld_x, R, weight, bias)
        ctx.save_for_backward(xv)
        ctx.params = (weight, bias)
        ctx.meta = (R, ld_x, tuple(x.shape))
        return y[:, :weight.shape[0]].reshape(*x.shape[:-1], weight.shape[0])

    @staticmethod
    def backward(ctx, dy):
        (xv,) = ctx.saved_tensors
        weight, bias = ctx.params
        R, ld_x, x_shape = ctx.meta
        dv, ld_d = H.rows_view(dy)
        dw, db = _affine_wgrads(dv, ld_d, xv, ld_x, R, weight, bias)
        dx = None
        if ctx.needs_input_grad[0]:
            dxb, _ = _affine_dgrad(dv, ld_d, R, weight)
            dx = dxb[:, :weight.shape[1]].reshape(x_shape)
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
        ctx.meta = (N, S, C, ld_x, ld1, ld2, ldm)
        return y[:, :w3.shape[0]]

    @staticmethod
    def backward(ctx, dy):
        xv, h1, z2, m, row0 = ctx.saved_tensors
        w1, b1, w2, b2, w3, b3 = ctx.params
        N, S, C, ld_x, ld1, ld2, ldm = ctx.meta
        dv, ld_d = H.rows_view(dy)
        dw3, db3 = _affine_wgrads(dv, ld_d, m, ldm, S, w3, b3)
        dm, ld_dm = _affine_dgrad(dv, ld_d, S, w3)
        dz2, ld_dz2 = H.segment_mean_bwd(dm, ld_dm, z2, ld2, row0, S, N, C, relu=True)
        dw2, db2 = _affine_wgrads(dz2, ld_dz2, h1, ld1, N, w2, b2)
        dh1, ld_dh1 = _affine_dgrad(dz2, ld_dz2, N, w2)
        dz1, ld_dz1 = H.relu_bwd(dh1, ld_dh1, h1, ld1, N, C)
        dw1, db1 = _affine_wgrads(dz1, ld_dz1, xv, ld_x, N, w1, b1)
        return None, None, None, dw1, db1, dw2, db2, dw3, db3


def aux_mlp(x, row0, S, linears):
    """x packed [N, idim] -> [S, odim]; linears: the three torch.nn.Linear containers of AuxNet.net."""
    l1, l2, l3 = linears
    return _AuxMLP.apply(x.to(torch.float32), row0, S, l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias)
