"""Float64 references and per-element bounds for the gradient through a carried recurrent state (tssep_lstm1_bwd_state,
tssep_gru1_bwd_state, functional.rnnp_layer(state_grad=True)); a helper, no tests of its own (tests/
test_state_grad_reference.py runs it on the CPU, the tests/test_gpu_state_grad_*.py files on the kernels' outputs).  Built
from the pieces of tests/test_recurrence_reference.py and tests/gru_reference.py for fam = "stream", ONE direction of time.

Tensors: gates [N, T, H, 4] (LSTM: i, f, g, o; GRU: the slots r, z, n, q), cell / h [N, T, H], dh_in [N, T, H] =
d(loss) / d(hout); the state side is [N, H]: h0 / c0 the state the forward started from, dhT / dcT the gradient arriving
for the final state, dh0 / dc0 the gradient of the initial one.  None is zeros everywhere.

Bounds, in units of U = 2^-24, every step from the kernel's OWN d(gates) of the later step, as in those files:

LSTM.  dh[t] = dhout[t] + W^T D[t+1] for t < T-1: one fmaf chain of 4H terms joined from four partials and one addition,
  k_4H S + U |dh| with k_4H = dot_factor("stream", 4H, backward=True), S = sum |D| |W| -- check_backward's term.  At
  t = T-1 the four partials are (dhT, 0, 0, 0): their sum is dhT EXACTLY, and dh = fl(dhT + dhout[T-1]) costs one more
  rounding of dh, U |dh| -- the same formula with S = 0.  The carried dc is followed by the float64 scan of
  check_backward with its error alongside; it starts from dcT, an exact input (error 0), in place of 0.  The forget
  gate's gradient at frame 0 multiplies by c0, an exact input, where it multiplied by 0.  d(gates): check_backward's
  coefficients and its 5 U |ref|.
  dh0 is a carried dh that no dhout joins: W^T D[0], k_4H S + U |dh0| (the U for the reference's own rounding).
  dc0 is a carried dc: fl(dc[0] f[0]), the scan's error after one more step, f E + U |dc0|.
GRU.  dh[t] = (W^T Dg[t+1] + dhout[t]) + fl(dh[t+1] z[t+1]): gru_reference.check_backward's base k_3H S + U |base| and its
  scan E = e_base + z E_later + U |carried| + 2 U |dh|.  At t = T-1 the carry's place holds dhT, exact: dh = fl(dhout +
  dhT), inside the same 2 U |dh|.  h_prev of frame 0 is h0, exact, in the coefficient of da_z.
  dh0 = fl(W^T Dg[0] + fl(dh[0] z[0])): k_3H S + U |W^T Dg[0]| for the matrix part, z E + U |carried| for the lane-local
  carry, U |dh0| for the addition that joins them and U |dh0| for the reference's rounding.
  The hand-over is not exact: inside one launch dhout[t] is added BETWEEN the matrix part and the carry, and dh0 hands
  their sum over as one tensor, so a chunked backward differs from the whole launch by one rounding of dh per boundary.

The layer: `layer` restates one RNNP layer (input product, time loop, projection, optional Tanh) with a state that takes
part in the loss, loss = sum(y dy) + sum(hT dhT) + sum(cT dcT), every gradient as the explicit sum it is; `torch_layer`
is the same by torch.nn.LSTM / torch.nn.GRU + Linear under autograd.  Both run whole or as chunks with the state handed
over, kept in the graph or detached (truncated BPTT)."""
import torch

import gru_reference as G
from test_causal_reference import CNAMES, LAYER_SHAPES, causal_module_params, causal_modules, lstm1_loop, make_causal_params
from test_recurrence_reference import TINY, U, Worst, _w_bwd, dot_factor, tanh_err
from test_rnnp_layer_reference import combine_rows, uncombine_rows

FAM = "stream"
LSTM_DEFECTS = ("c0_missing", "dcT_dropped", "dhT_dropped", "dhT_twice", "dc0_before_f")
GRU_DEFECTS = ("dhT_dropped", "dhT_twice", "hprev_zero", "dh0_without_carry")
LAYER_DEFECTS = ("dwhh_h0_missing",)
# The factor on W_hh of the chunked cases.  Measured on the CPU (float64 truncated against full dW_hh, normwise, over the
# GPU test's bound under split-bf16 GEMMs = 8 x 770.6 x the fp32 restatement's error), LSTM / GRU: wide at 1: 35 / 68, 2:
# 65 / 74, 3: 92 / 82, 4: 101 / 80, 6: 31 / 15 (the fp32 error itself grows), 8: 2.4 / 2.3; toy at 1: 162 / 309.  Under
# fp32 GEMMs the bound is 770.6 times narrower and the distance 770.6 times those figures.
WHH_SCALE_TOY, WHH_SCALE_WIDE = 1.0, 3.0


def _z(v, like):
    return torch.zeros_like(like) if v is None else v.to(like.dtype)


# ---- plain time loops, one direction, with the state's side --------------------------------------------------------------
def lstm1_backward_loop(A, cell, dh_in, whh, H, dtype, c0=None, dhT=None, dcT=None, defect=None):
    """-> (D [n, T, H, 4], dh0, dc0 [n, H]) from the saved A [n, T, H, 4], cell [n, T, H] and dh_in [n, T, H]"""
    a, c, dh_in = A.to(dtype), cell.to(dtype), dh_in.to(dtype)
    n, T = a.shape[:2]
    wb = _w_bwd([whh], H, dtype)[0]
    zero = torch.zeros(n, H, dtype=dtype, device=a.device)
    c0, dhT, dcT = _z(c0, zero), _z(dhT, zero), _z(dcT, zero)
    D = torch.empty_like(a)
    rec = {"dhT_dropped": zero, "dhT_twice": 2 * dhT}.get(defect, dhT)
    dcc = zero if defect == "dcT_dropped" else dcT
    dc = zero
    for t in range(T - 1, -1, -1):
        cp = c[:, t - 1] if t else (zero if defect == "c0_missing" else c0)
        dh = rec + dh_in[:, t]
        i, f, g, o = a[:, t].unbind(-1)
        tc = torch.tanh(c[:, t])
        dc = dh * o * (1 - tc * tc) + dcc
        dcc = dc * f
        d = torch.stack([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
        D[:, t] = d
        rec = d.reshape(n, 4 * H) @ wb
    return D, rec, (dc if defect == "dc0_before_f" else dcc)


def gru1_backward_loop(A, h, dh_in, whh, H, dtype, h0=None, dhT=None, defect=None):
    """-> (Dg [n, T, H, 4], dh0 [n, H]) from the saved A = (r, z, n, q), h [n, T, H] and dh_in [n, T, H]"""
    a, h, dh_in = A.to(dtype), h.to(dtype), dh_in.to(dtype)
    n, T = a.shape[:2]
    wb = G._w_bwd([whh], H, dtype)[0]
    zero = torch.zeros(n, H, dtype=dtype, device=a.device)
    h0, dhT = _z(h0, zero), _z(dhT, zero)
    Dg = torch.empty_like(a)
    rec = zero
    carry = {"dhT_dropped": zero, "dhT_twice": 2 * dhT}.get(defect, dhT)
    for t in range(T - 1, -1, -1):
        hp = h[:, t - 1] if t else (zero if defect == "hprev_zero" else h0)
        dh = rec + dh_in[:, t] + carry
        r, z, nn, q = a[:, t].unbind(-1)
        dan = dh * (1 - z) * (1 - nn * nn)
        carry = dh * z
        dg = torch.stack([dan * q * r * (1 - r), dh * (hp - nn) * z * (1 - z), dan, dan * r], -1)
        Dg[:, t] = dg
        rec = dg.reshape(n, 4 * H) @ wb
    return Dg, (rec if defect == "dh0_without_carry" else rec + carry)


# ---- the bounds ----------------------------------------------------------------------------------------------------------
def _products(Dk, wb, tail):
    """Dk [n, T, H, 4] in float64 -> (W^T Dk[t] and sum |W| |Dk[t]| as the EARLIER step reads them: index t holds the later
    step's product, the last index `tail` and 0; the product of frame 0 and its sum)"""
    n, T = Dk.shape[:2]
    rows = Dk.reshape(n, T, -1)
    rec, S = rows @ wb, rows.abs() @ wb.abs()
    later = torch.cat([rec[:, 1:], tail.unsqueeze(1)], 1)
    Sl = torch.cat([S[:, 1:], torch.zeros_like(S[:, :1])], 1)
    return later, Sl, rec[:, 0], S[:, 0]


def check_lstm1_backward(A, cell, dhout, D, whh, H, c0=None, dhT=None, dcT=None, dh0=None, dc0=None, worst=None):
    """A [N, T, H, 4], cell [N, T, H], dhout [N, T, >= H] and the state's inputs: what the launch read; D, dh0, dc0: what it
    wrote (dh0 / dc0 None: not asked for).  Every element against the float64 step from the kernel's own later D."""
    worst = worst or Worst()
    a, c = A.double(), cell.double()
    n, T = a.shape[:2]
    zero = torch.zeros(n, H, dtype=torch.float64, device=a.device)
    c0, dhT, dcT = _z(c0, zero), _z(dhT, zero), _z(dcT, zero)
    i, f, g, o = a.unbind(-1)
    cp = torch.cat([c0.unsqueeze(1), c[:, :-1]], 1)
    kf = dot_factor(FAM, 4 * H, backward=True)
    rec, S, rec0, S0 = _products(D.double(), _w_bwd([whh], H, torch.float64)[0], dhT)
    dh = dhout[..., :H].double() + rec
    edh = kf * S + U * dh.abs()
    tc = torch.tanh(c)
    etc = tanh_err(c, tc, False)
    omt = 1 - tc * tc
    p = dh * o * omt
    ep = edh * o * omt + dh.abs() * o * (2 * tc.abs() * etc + etc * etc + U) + 3 * U * p.abs()
    dc, E = torch.empty_like(p), torch.empty_like(p)
    carried, Ec = dcT, torch.zeros_like(dcT)
    for t in range(T - 1, -1, -1):
        dcn = p[:, t] + carried
        En = ep[:, t] + Ec + U * dcn.abs()
        dc[:, t], E[:, t] = dcn, En
        carried = f[:, t] * dcn
        Ec = f[:, t] * En + U * carried.abs()
    ref = torch.stack([dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)], -1)
    err = torch.stack([E * (g * i * (1 - i)).abs(), E * (cp * f * (1 - f)).abs(), E * i * (1 - g * g) + U * (dc * i).abs(),
                       edh * (tc * o * (1 - o)).abs() + dh.abs() * etc * o * (1 - o)], -1)
    worst.add("dgates", D, ref, err + 5 * U * ref.abs() + TINY)
    if dh0 is not None:
        worst.add("dh0", dh0, rec0, kf * S0 + U * rec0.abs() + TINY)
    if dc0 is not None:
        worst.add("dc0", dc0, carried, Ec + U * carried.abs() + TINY)
    worst.count += ref.numel()
    return worst


def check_gru1_backward(A, hout, dhout, Dg, whh, H, h0=None, dhT=None, dh0=None, worst=None):
    """A [N, T, H, 4] = (r, z, n, q), hout, dhout [N, T, >= H], h0, dhT: what the launch read; Dg, dh0: what it wrote"""
    worst = worst or Worst()
    a = A.double()
    n, T = a.shape[:2]
    zero = torch.zeros(n, H, dtype=torch.float64, device=a.device)
    h0, dhT = _z(h0, zero), _z(dhT, zero)
    r, z, nn, q = a.unbind(-1)
    hp = torch.cat([h0.unsqueeze(1), hout[:, :-1, :H].double()], 1)
    kf = dot_factor(FAM, 3 * H, backward=True)
    rec, S, rec0, S0 = _products(Dg.double(), G._w_bwd([whh], H, torch.float64)[0], zero)
    base = dhout[..., :H].double() + rec
    ebase = kf * S + U * base.abs()
    dh, E = torch.empty_like(base), torch.empty_like(base)
    carried, Ec = dhT, torch.zeros_like(dhT)
    for t in range(T - 1, -1, -1):
        dhn = base[:, t] + carried
        En = ebase[:, t] + Ec + 2 * U * dhn.abs()
        dh[:, t], E[:, t] = dhn, En
        carried = z[:, t] * dhn
        Ec = z[:, t] * En + U * carried.abs()
    cn = (1 - z) * (1 - nn * nn)
    coef = torch.stack([cn * q * r * (1 - r), (hp - nn) * z * (1 - z), cn, cn * r], -1)
    ref = dh.unsqueeze(-1) * coef
    rest = torch.stack([(q * r * (1 - r)).abs(), torch.zeros_like(r), torch.ones_like(r), r], -1)
    e_omn = 2 * U * (dh * (1 - z)).abs().unsqueeze(-1) * rest
    worst.add("dgates", Dg, ref, E.unsqueeze(-1) * coef.abs() + e_omn + 8 * U * ref.abs() + TINY)
    if dh0 is not None:
        ref0 = rec0 + carried
        worst.add("dh0", dh0, ref0, kf * S0 + U * rec0.abs() + Ec + 2 * U * ref0.abs() + TINY)
    worst.count += ref.numel()
    return worst


# ---- one RNNP layer with a state in the loss -------------------------------------------------------------------------------
def make_state(N, H, gru, seed, scale=1.0):
    """-> (the state (h0, c0) or (h0,), the weights (dhT, dcT) or (dhT,) of the final state in the loss): fp32, fixed seed.
    h0 lies in (-1, 1) as an h does; c0 is a cell state of a few frames."""
    gen = torch.Generator().manual_seed(4000 + seed)
    k = 1 if gru else 2
    state = [torch.rand(N, H, generator=gen) * 2 - 1] + [torch.randn(N, H, generator=gen)] * (k - 1)
    return tuple(state), tuple(torch.randn(N, H, generator=gen) * scale for _ in range(k))


def make_case(N, T, I, H, hdim, gru, seed, combine=0, whh_scale=1.0):
    """-> x rows (n, t), the six parameters, dy, dlast, state: fp32 values, fixed seed.  whh_scale multiplies W_hh."""
    gen = torch.Generator().manual_seed(5000 + seed)
    params = G.make_layer_params(I, H, hdim, 1, gen) if gru else make_causal_params(I, H, hdim, gen)
    params[1] = params[1] * whh_scale
    K = combine or 1
    x, dy = torch.randn(N * T, I, generator=gen), torch.randn(N // K * T, K * hdim, generator=gen)
    state, dlast = make_state(N, H, gru, seed)
    return x, params, dy, dlast, state


def _forward(x3, p, H, gru, state, act):
    """x3 [N, n, I] in the dtype of p -> the saved tensors of one chunk"""
    N, n = x3.shape[:2]
    dtype = x3.dtype
    zero = torch.zeros(N, H, dtype=dtype)
    state = tuple(_z(s, zero) for s in (state or (None,) * (1 if gru else 2)))
    x = x3.reshape(N * n, -1)
    if gru:
        wih_p, bias_p = G.pack_reference(p[:4], H)
        gin = (x @ wih_p.t() + bias_p).view(N, n, 1, H, 4)
        A, h = G.gru_forward_loop(gin, [p[1]], H, dtype, h0=state[0])
        A, h, c, last = A[:, :, 0], h[:, :, 0], None, (h[:, -1, 0],)
    else:
        wih_p = None
        gin = (x @ p[0].t() + (p[2] + p[3])).view(N, n, 4, H).transpose(2, 3)
        A, c, h, last = lstm1_loop(gin, p[1], H, dtype, state)
    zz = h.reshape(N * n, H) @ p[4].t() + p[5]
    return dict(x=x, A=A, c=c, h=h, y_rows=torch.tanh(zz) if act else zz, last=last, state=state, wih_p=wih_p, N=N, n=n)


def _backward(fw, p, H, gru, act, dy_rows, dlast, defect=None):
    """-> ({"x", the six names}, the gradient of the chunk's initial state)"""
    N, n, x = fw["N"], fw["n"], fw["x"]
    dtype = x.dtype
    dz = dy_rows * (1 - fw["y_rows"] ** 2) if act else dy_rows
    out = {"b_proj": dz.sum(0), "w_proj": dz.t() @ fw["h"].reshape(N * n, H)}
    dh_in = (dz @ p[4]).view(N, n, H)
    h0 = torch.zeros_like(fw["state"][0]) if defect == "dwhh_h0_missing" else fw["state"][0]
    hp = torch.cat([h0.unsqueeze(1), fw["h"][:, :-1]], 1).reshape(N * n, H)
    kdef = defect if defect not in LAYER_DEFECTS else None
    if gru:
        Dg, dh0 = gru1_backward_loop(fw["A"], fw["h"], dh_in, p[1], H, dtype, fw["state"][0], dlast[0], kdef)
        rows = Dg.reshape(N * n, 4 * H)
        out["x"] = rows @ fw["wih_p"]
        col = rows.sum(0).unsqueeze(-1)
        out["w_ih"], out["w_hh"] = G.unpack_reference(rows.t() @ x, H, "ih")[0], G.unpack_reference(rows.t() @ hp, H, "hh")[0]
        out["b_ih"], out["b_hh"] = G.unpack_reference(col, H, "ih")[0].view(-1), G.unpack_reference(col, H, "hh")[0].view(-1)
        return out, (dh0,)
    D, dh0, dc0 = lstm1_backward_loop(fw["A"], fw["c"], dh_in, p[1], H, dtype, fw["state"][1], dlast[0], dlast[1], kdef)
    rows = D.transpose(2, 3).reshape(N * n, 4 * H)
    out["x"] = rows @ p[0]
    out["w_ih"], out["w_hh"] = rows.t() @ x, rows.t() @ hp
    out["b_ih"] = out["b_hh"] = rows.sum(0)
    return out, (dh0, dc0)


def _result(grads, dstate, y, last, gru):
    out = dict(grads)
    out.update(y=y, h0=dstate[0], hT=last[0])
    if not gru:
        out.update(c0=dstate[1], cT=last[1])
    return out


def layer(x, params, dy, dlast, state, N, T, dtype, gru=False, act=0, combine=0, chunks=None, detach=False, defect=None):
    """The restated layer in `dtype` -> {"y", "x", the six parameter names, "h0" (, "c0"): the gradient of the initial
    state, "hT" (, "cT"): the final state}.  x rows (n, t) [N T, I]; dy in the output's layout; dlast the weights of the
    final state in the loss; state the initial state or None.  chunks: frame counts that sum to T -- the layer runs chunk
    after chunk from the state the one before ended in, and backwards from the last: each chunk's (dh0, dc0) is the
    earlier chunk's (dhT, dcT), or zeros when detach (truncated BPTT: the loss reads every chunk's output and the LAST
    chunk's final state)."""
    p = [t.to(dtype) for t in params]
    H = p[1].shape[1]
    x3 = x.to(dtype).view(N, T, -1)
    dy = dy.to(dtype)
    dy3 = (uncombine_rows(dy, N, T, combine) if combine else dy).reshape(N, T, -1)
    st = None if state is None else tuple(s.to(dtype) for s in state)
    chunks = list(chunks or [T])
    assert sum(chunks) == T, (chunks, T)
    fws, t0 = [], 0
    for n in chunks:
        fws.append(_forward(x3[:, t0:t0 + n], p, H, gru, st, act))
        st = fws[-1]["last"]
        t0 += n
    dlast = tuple(d.to(dtype) for d in dlast)
    total, dxs, t1 = None, [], T
    for fw in reversed(fws):
        n = fw["n"]
        g, dstate = _backward(fw, p, H, gru, act, dy3[:, t1 - n:t1].reshape(N * n, -1), dlast, defect)
        dxs.insert(0, g.pop("x").view(N, n, -1))
        total = g if total is None else {k: total[k] + v for k, v in g.items()}
        dlast = tuple(torch.zeros_like(d) for d in dstate) if detach else dstate
        t1 -= n
    total["x"] = torch.cat(dxs, 1).reshape(N * T, -1)
    y = torch.cat([fw["y_rows"].view(N, fw["n"], -1) for fw in fws], 1).reshape(N * T, -1)
    return _result(total, dstate, combine_rows(y, N, T, combine) if combine else y, fws[-1]["last"], gru)


def modules_of(params, gru, device="cpu", dtype=torch.float32):
    return G.gru_modules(params, device=device, dtype=dtype) if gru else causal_modules(params, device=device, dtype=dtype)


def params_of(rnn, lin):
    return G.module_params(rnn, lin) if isinstance(rnn, torch.nn.GRU) else causal_module_params(rnn, lin)


def torch_layer(x, params, dy, dlast, state, N, T, dtype, gru=False, act=0, combine=0, chunks=None, detach=False):
    """`layer` by torch.nn.LSTM / torch.nn.GRU + Linear (+ Tanh) under autograd; the state requires a gradient"""
    rnn, lin = modules_of(params, gru, dtype=dtype)
    xr = x.to(dtype).view(N, T, -1).clone().requires_grad_()
    H = params[1].shape[1]
    if state is None:
        state = tuple(torch.zeros(N, H) for _ in range(1 if gru else 2))
    leaves = [s.to(dtype).clone().requires_grad_() for s in state]
    st, zs, t0 = [s.unsqueeze(0) for s in leaves], [], 0
    for n in chunks or [T]:
        h, last = rnn(xr[:, t0:t0 + n], st[0] if gru else tuple(st))
        zs.append(lin(h))
        st = [s.detach() if detach else s for s in ((last,) if gru else last)]
        t0 += n
    last = (last,) if gru else last
    z = torch.cat(zs, 1).reshape(N * T, -1)
    y = torch.tanh(z) if act else z
    y = combine_rows(y, N, T, combine) if combine else y
    loss = (y * dy.to(dtype)).sum()
    for s, d in zip(last, dlast):
        loss = loss + (s[0] * d.to(dtype)).sum()
    loss.backward()
    grads = {k: t.grad for k, t in zip(CNAMES, params_of(rnn, lin))}
    grads["x"] = xr.grad.reshape(N * T, -1)
    return _result(grads, [s.grad for s in leaves], y.detach(), [s[0].detach() for s in last], gru)


# ---- the cases of the GPU layer file, each reference computed once and left unchanged -------------------------------------------
LAYER_CASES = list(LAYER_SHAPES[:4])      # (N, T, I, H, hdim, combine): the small ones and (32, 7, 321, 300, 320, 0)
# name -> (N, T, I, H, hdim, the factor on W_hh): T = 23 run as (23), (1 x 23), (5, 1, 17).  The factor makes the state
# matter: with it the truncated gradient is far from the full one (tests/test_state_grad_reference.py asserts how far)
CHUNK_CASES = {"toy": (3, 23, 7, 5, 6, WHH_SCALE_TOY), "wide": (8, 23, 321, 300, 320, WHH_SCALE_WIDE)}
CHUNKINGS = ([23], [1] * 23, [5, 1, 17])
F64, F32 = torch.float64, torch.float32
_CACHE = {}


def layer_reference(shape, gru, act, seed=0):
    """-> x, params, dy, dlast, state, {float64: torch autograd, float32: the restatement} of one whole-sequence call"""
    key = ("layer", tuple(shape), gru, act, seed)
    if key not in _CACHE:
        N, T, I, H, hdim, combine = shape
        c = make_case(N, T, I, H, hdim, gru, seed, combine)
        with torch.no_grad():
            r32 = layer(*c, N, T, F32, gru, act, combine)
        _CACHE[key] = (*c, {F64: torch_layer(*c, N, T, F64, gru, act, combine), F32: r32})
    return _CACHE[key]


def chunk_reference(name, gru, chunks=(5, 1, 17), detach=False, act=1):
    """-> x, params, dy, dlast, state, {float64: torch autograd over `chunks`, float32: the restatement over `chunks`}, the
    state kept in the graph (the gradient is then the whole sequence's, whatever the chunking) or detached"""
    key = ("chunks", name, gru, tuple(chunks), detach, act)
    if key not in _CACHE:
        N, T, I, H, hdim, scale = CHUNK_CASES[name]
        c = make_case(N, T, I, H, hdim, gru, 1, whh_scale=scale)
        with torch.no_grad():
            r32 = layer(*c, N, T, F32, gru, act, chunks=chunks, detach=detach)
        _CACHE[key] = (*c, {F64: torch_layer(*c, N, T, F64, gru, act, chunks=chunks, detach=detach), F32: r32})
    return _CACHE[key]


TOY_SEEDS = tuple(range(12))


def yardstick(dims, gru, act, combine=0, chunks=None, detach=False, whh_scale=1.0, seeds=TOY_SEEDS):
    """-> {tensor: (normwise, element-wise)}: the fp32 restatement's own error against float64 at these sizes, the LARGEST
    over `seeds` -- gru_reference.chain_yardstick's measure, for its reason: at 5 units the worst error of one draw is one
    or two roundings on one element and moves by an order of magnitude from seed to seed.  CPU only; cached."""
    from test_rnnp_layer_reference import errors
    key = ("yard", tuple(dims), gru, act, combine, tuple(chunks or ()), detach, whh_scale)
    if key not in _CACHE:
        N, T = dims[:2]
        worst = {}
        for seed in seeds:
            c = make_case(*dims, gru, seed, combine, whh_scale)
            with torch.no_grad():
                r32 = layer(*c, N, T, F32, gru, act, combine, chunks, detach)
                r64 = layer(*c, N, T, F64, gru, act, combine, chunks, detach)
            for k in r64:
                worst[k] = tuple(max(a, b) for a, b in zip(worst.get(k, (0.0, 0.0)), errors(r32[k], r64[k])))
        _CACHE[key] = worst
    return _CACHE[key]
