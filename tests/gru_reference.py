"""Float64 references and per-element bounds of the GRU recurrence kernels (tssep_amd/csrc/gru.hip), in the manner of
tests/test_recurrence_reference.py for fam = "stream"; a helper, no tests of its own (tests/test_gru_reference.py runs it on
the CPU, tests/test_gpu_gru_kernels.py on the kernels' outputs).

Tensors (include/tssep_hip.h): gates [N, T, D, H, 4] with the four SLOTS (r, z, n, q) per unit -- read as the input GEMM's
(a_r, a_z, a_n, b_hn), written as (r, z, n, q), q = W_hn h + b_hn --; hout / dhout [N, T, ldo] with direction d in columns
d * dstride .. + H; W_hh in torch's layout [3H, H] (rows r, z, n) per direction; D = 1 | 2 directions of time, the second
running backwards.

Bounds, in units of U = 2^-24, every step from the kernel's OWN previous h (forward) / own next d(gates) (backward):

forward.  A recurrent sum is one fmaf chain of H terms per slot (v_mfma_f32_4x4x1 accumulates in fp32, one rounding per
  term) joined with the input's value by one addition: |error| <= k_H S + U |a|, S = sum |h_prev| |W|, k_H =
  dot_factor("stream", H) -- the project's factor for one chain of H terms.  Slot 2 (n) has no recurrent part: the kernel
  adds 0, a_n is EXACT.  r, z: the argument error through the sigmoid (first derivative, |f''| / 2 for the square) plus
  sigmoid_err, OCML's expf then one addition and one division.  q = a_3.  n = tanhf(fmaf(r, q, a_n)): the argument
  carries e_r |q| + r e_q + e_r e_q and ONE rounding U |arg|; then through tanh plus tanh_err (OCML tanhf).
  h' = fmaf(z, h_prev, fl(fl(1 - z) n)): h_prev is exact (the kernel's own); w = fl(1 - z) errs by e_z + U (1 - z);
  p = fl(w n) by |n| e_w + (1 - z) e_n + e_w e_n + U |p|; h' by e_z |h_prev| + e_p + U |h'|.  One more U |h'| of slack
  for the reference's own rounding to fp32 inputs (as the LSTM checker's 2 U |h|).
backward.  dh = dhout + the four partial sums of W^T d(gates of the later step) + fl(dh_later z_later): the matrix part
  errs by k_3H S' (3H non-zero terms: the slot-2 block of the matrix is zero and contributes nothing), the additions by
  U |.| each; the lane-local carry is followed by a float64 scan with its error alongside, E = e_base + z_later E_later +
  U |carried| + 2 U |dh|, as the LSTM checker follows dc.  Every output is dh times a coefficient formed from EXACT inputs
  (the saved r, z, n, q and hout, fp32) by at most eight roundings, each relative to a partial result that is a factor of
  the output (1 - z, 1 - r, h_prev - n are single subtractions): E |coefficient| + 8 U |reference|.  The one factor that
  is not a single operation is 1 - n^2: the kernel forms it with one fmaf (one relative rounding), an fp32 loop that
  rounds n^2 first errs by up to U n^2 + U (1 - n^2) <= 2 U ABSOLUTE, which is not small beside 1 - n^2 where tanh
  saturates; the bound takes the absolute form for both (as the LSTM checker's U |dc i| for 1 - g^2): the three outputs
  that carry the factor, da_r, da_n, da_q, add 2 U |dh (1 - z)| times the rest of their coefficient.
"""
import torch

from test_recurrence_reference import (SIG_D2, TANH_D2, TINY, U, Worst, _through, dot_factor, sigmoid_err, tanh_err)

FAM = "stream"
ROWS = 16384


def hh_blocks(whh, H, dtype):
    """torch's W_hh [3H, H] of one direction -> [4 slots, H(unit), H(k)]: rows (W_hr, W_hz, 0, W_hn)"""
    w = whh.to(dtype).view(3, H, H)
    return torch.stack([w[0], w[1], torch.zeros_like(w[0]), w[2]])


def _w_fwd(whh, H, dtype):
    """[D, H(k), 4H(unit * 4 + slot)]"""
    return torch.stack([hh_blocks(w, H, dtype).permute(2, 1, 0).reshape(H, 4 * H) for w in whh])


def _w_bwd(whh, H, dtype):
    """[D, 4H(unit * 4 + slot), H(k)]: d(h_prev)[k] = sum over (unit, slot) of d(gates) W_slot[unit, k]"""
    return torch.stack([hh_blocks(w, H, dtype).permute(1, 0, 2).reshape(4 * H, H) for w in whh])


def dirs(h, H, dstride, D):
    """hout / dhout [n, T, ldo] -> [n, T, D, H]"""
    return torch.stack([h[..., d * dstride:d * dstride + H] for d in range(D)], 2)


def packed(h4, ldo, dstride, fill=0.0):
    """[n, T, D, H] -> hout layout [n, T, ldo]"""
    n, T, D, H = h4.shape
    out = torch.full((n, T, ldo), fill, dtype=h4.dtype, device=h4.device)
    for d in range(D):
        out[..., d * dstride:d * dstride + H] = h4[:, :, d]
    return out


def shift(x, first=None):
    """x [n, T, D, ...] -> the previous step's x in each direction's time order (direction 1 runs backwards); the first
    step of direction 0 reads `first` [n, ...] when given, zeros otherwise"""
    out = torch.zeros_like(x)
    out[:, 1:, 0] = x[:, :-1, 0]
    if first is not None:
        out[:, 0, 0] = first
    if x.shape[2] == 2:
        out[:, :-1, 1] = x[:, 1:, 1]
    return out


def _later(x):
    """x [n, T, D, ...] -> the LATER step's x in each direction's time order, zeros behind the last step"""
    out = torch.zeros_like(x)
    out[:, :-1, 0] = x[:, 1:, 0]
    if x.shape[2] == 2:
        out[:, 1:, 1] = x[:, :-1, 1]
    return out


def _blocks(N, T, D):
    nb = max(1, ROWS // (D * T))
    return [(n0, min(N, n0 + nb)) for n0 in range(0, N, nb)]


# ---- the bounds --------------------------------------------------------------------------------------------------------
def check_forward(gin, A, hout, whh, H, dstride, h0=None, worst=None):
    """gin: the pre-activations the launch read [N, T, D, H, 4]; A, hout: what it wrote; h0 [N, H] (D = 1) the initial
    state.  Every element of every step against the float64 step from the kernel's own previous h."""
    worst = worst or Worst()
    N, T, D = A.shape[:3]
    wk = _w_fwd(whh, H, torch.float64)
    kf = dot_factor(FAM, H)
    for n0, n1 in _blocks(N, T, D):
        n = n1 - n0
        g = gin[n0:n1].double()
        hk = dirs(hout[n0:n1], H, dstride, D)
        hp = shift(hk.double(), None if h0 is None else h0[n0:n1].double())
        hp2 = hp.permute(2, 0, 1, 3).reshape(D, n * T, H)
        rec = torch.bmm(hp2, wk).view(D, n, T, H, 4).permute(1, 2, 0, 3, 4)
        S = torch.bmm(hp2.abs(), wk.abs()).view(D, n, T, H, 4).permute(1, 2, 0, 3, 4)
        a = g + rec
        ea = kf * S + U * a.abs()
        ea[..., 2] = 0.0                                   # acc = 0 exactly: a_n is the input's value
        r, z = torch.sigmoid(a[..., 0]), torch.sigmoid(a[..., 1])
        er = _through(ea[..., 0], r * (1 - r), SIG_D2, sigmoid_err(a[..., 0], r, False))
        ez = _through(ea[..., 1], z * (1 - z), SIG_D2, sigmoid_err(a[..., 1], z, False))
        q, eq = a[..., 3], ea[..., 3]
        arg = a[..., 2] + r * q
        earg = er * q.abs() + r * eq + er * eq + U * arg.abs()
        nn = torch.tanh(arg)
        en = _through(earg, 1 - nn * nn, TANH_D2, tanh_err(arg, nn, False))
        ref = torch.stack([r, z, nn, q], -1)
        worst.add("act", A[n0:n1], ref, torch.stack([er, ez, en, eq], -1) + U * ref.abs())
        ew = ez + U * (1 - z)
        p = (1 - z) * nn
        ep = nn.abs() * ew + (1 - z) * en + ew * en + U * p.abs()
        h = p + z * hp
        worst.add("h", hk, h, ez * hp.abs() + ep + 2 * U * h.abs() + TINY)
        worst.count += h.numel()
    return worst


def check_backward(A, hout, dhout, Dg, whh, H, dstride, worst=None):
    """A [N, T, D, H, 4] (r, z, n, q), hout, dhout: what the launch read; Dg: the d(pre-activations) it wrote.  The matrix
    part of dh from the kernel's own Dg of the later step, the carried dh z by a float64 scan with its error alongside."""
    worst = worst or Worst()
    N, T, D = Dg.shape[:3]
    wb = _w_bwd(whh, H, torch.float64)
    kf = dot_factor(FAM, 3 * H, backward=True)
    for n0, n1 in _blocks(N, T, D):
        n = n1 - n0
        r, z, nn, q = A[n0:n1].double().unbind(-1)
        hp = shift(dirs(hout[n0:n1], H, dstride, D).double())
        Dk = Dg[n0:n1]
        Dn = _later(Dk.double()).permute(2, 0, 1, 3, 4).reshape(D, n * T, 4 * H)
        rec = torch.bmm(Dn, wb).view(D, n, T, H).permute(1, 2, 0, 3)
        S = torch.bmm(Dn.abs(), wb.abs()).view(D, n, T, H).permute(1, 2, 0, 3)
        base = dirs(dhout[n0:n1], H, dstride, D).double() + rec
        ebase = kf * S + U * base.abs()
        zl = _later(z)
        dh, E = torch.empty_like(base), torch.empty_like(base)
        for d, order in ((0, range(T - 1, -1, -1)), (1, range(T)))[:D]:
            dhn = torch.zeros_like(base[:, 0, d])
            En = torch.zeros_like(dhn)
            for t in order:
                carried = zl[:, t, d] * dhn
                dhn = base[:, t, d] + carried
                En = ebase[:, t, d] + zl[:, t, d] * En + U * carried.abs() + 2 * U * dhn.abs()
                dh[:, t, d], E[:, t, d] = dhn, En
        cn = (1 - z) * (1 - nn * nn)
        coef = torch.stack([cn * q * r * (1 - r), (hp - nn) * z * (1 - z), cn, cn * r], -1)
        ref = dh.unsqueeze(-1) * coef
        rest = torch.stack([(q * r * (1 - r)).abs(), torch.zeros_like(r), torch.ones_like(r), r], -1)
        e_omn = 2 * U * (dh * (1 - z)).abs().unsqueeze(-1) * rest
        worst.add("dgates", Dk, ref, E.unsqueeze(-1) * coef.abs() + e_omn + 8 * U * ref.abs() + TINY)
        worst.count += ref.numel()
    return worst


# ---- plain time loops (torch.nn.GRU's formula on the four slots) ---------------------------------------------------------
def gru_forward_loop(gin, whh, H, dtype, h0=None, defect=None):
    """-> A [n, T, D, H, 4] = (r, z, n, q), h [n, T, D, H] of the recurrence in `dtype`.  defect: "bhn_outside" (b_hn, the
    input's slot 3, added outside the r product) | "z_swapped" (z and 1 - z exchanged)."""
    g = gin.to(dtype)
    n, T, D = g.shape[:3]
    wk = _w_fwd(whh, H, dtype)
    A, Hh = torch.empty_like(g), torch.empty_like(g[..., 0])
    h = torch.zeros(n, D, H, dtype=dtype, device=g.device)
    if h0 is not None:
        h[:, 0] = h0.to(dtype)
    for s in range(T):
        ts = (s, T - 1 - s)[:D]
        rec = torch.bmm(h.transpose(0, 1), wk).view(D, n, H, 4).transpose(0, 1)
        gx = torch.stack([g[:, ts[d], d] for d in range(D)], 1)
        a = gx + rec
        r, z, q = torch.sigmoid(a[..., 0]), torch.sigmoid(a[..., 1]), a[..., 3]
        if defect == "bhn_outside":
            nn = torch.tanh(a[..., 2] + r * rec[..., 3] + gx[..., 3])
        else:
            nn = torch.tanh(a[..., 2] + r * q)
        h = (z * nn + (1 - z) * h) if defect == "z_swapped" else ((1 - z) * nn + z * h)
        act = torch.stack([r, z, nn, q], -1)
        for d in range(D):
            A[:, ts[d], d], Hh[:, ts[d], d] = act[:, d], h[:, d]
    return A, Hh


def gru_backward_loop(A, h, dh_in, whh, H, dtype, defect=None):
    """-> Dg [n, T, D, H, 4] = (da_r, da_z, da_n, da_q) from the saved A, h [n, T, D, H] and dh_in [n, T, D, H]; zero
    initial state.  defect: "daq_without_r" | "hprev_first_frame" (h_prev of a direction's first step read from that
    frame's own h instead of the zero state)."""
    a, h, dh_in = A.to(dtype), h.to(dtype), dh_in.to(dtype)
    n, T, D = a.shape[:3]
    wb = _w_bwd(whh, H, dtype)
    Dg = torch.empty_like(a)
    Dn = torch.zeros(D, n, 4 * H, dtype=dtype, device=a.device)
    carry = torch.zeros(n, D, H, dtype=dtype, device=a.device)
    zero = torch.zeros(n, H, dtype=dtype, device=a.device)
    for s in range(T):
        ts = (T - 1 - s, s)[:D]
        prev = (ts[0] - 1, s + 1)[:D]
        first = s + 1 == T                              # this direction's first step of the forward pass
        at = torch.stack([a[:, ts[d], d] for d in range(D)], 1)
        if first:
            hp = torch.stack([h[:, ts[d], d] if defect == "hprev_first_frame" else zero for d in range(D)], 1)
        else:
            hp = torch.stack([h[:, prev[d], d] for d in range(D)], 1)
        dh = torch.stack([dh_in[:, ts[d], d] for d in range(D)], 1) + torch.bmm(Dn, wb).transpose(0, 1) + carry
        r, z, nn, q = at.unbind(-1)
        dn = dh * (1 - z)
        dz = dh * (hp - nn)
        dan = dn * (1 - nn * nn)
        carry = dh * z
        dg = torch.stack([dan * q * r * (1 - r), dz * z * (1 - z), dan, dan if defect == "daq_without_r" else dan * r], -1)
        for d in range(D):
            Dg[:, ts[d], d] = dg[:, d]
        Dn = dg.transpose(0, 1).reshape(D, n, 4 * H)
    return Dg


# ---- the packed layer in torch: pack, the four-slot GEMMs, unpack ----------------------------------------------------------
def pack_reference(params, H):
    """params: D x (w_ih [3H, I], w_hh [3H, H], b_ih, b_hh), torch.nn.GRU's -> (wih_p [D 4H, I], bias_p [D 4H]), rows
    [dir][unit][slot], in the parameters' dtype (b_ir + b_hr and b_iz + b_hz are ONE addition: bit-equal in fp32)"""
    wih, bias = [], []
    for d in range(len(params) // 4):
        w_ih, _, b_ih, b_hh = params[4 * d:4 * d + 4]
        w3, bi, bh = w_ih.view(3, H, -1), b_ih.view(3, H), b_hh.view(3, H)
        wih.append(torch.stack([w3[0], w3[1], w3[2], torch.zeros_like(w3[0])], 1).reshape(4 * H, -1))
        bias.append(torch.stack([bi[0] + bh[0], bi[1] + bh[1], bi[2], bh[2]], 1).reshape(4 * H))
    return torch.cat(wih), torch.cat(bias)


def unpack_reference(src, H, which, defect=None):
    """src [D 4H, ncols] packed rows -> D tensors [3H, ncols] in torch's rows (r, z, n).  which: "ih" reads the slots
    (0, 1, 2), "hh" (0, 1, 3).  defect "hh_from_slot_2": the hidden side's n rows taken from slot 2."""
    slots = [0, 1, 2] if (which == "ih" or defect == "hh_from_slot_2") else [0, 1, 3]
    s = src.view(-1, H, 4, src.shape[-1])
    return [s[d][:, slots].permute(1, 0, 2).reshape(3 * H, -1) for d in range(s.shape[0])]


def layer_gradients(x, params, dh_in, H, defect=None, dtype=torch.float64):
    """One GRU layer as the HIP path composes it, in `dtype`: x [n, T, I], params as pack_reference's, dh_in [n, T, D, H]
    = d(loss) / d(h) -> (h [n, T, D, H], dx, [dW_ih, dW_hh, db_ih, db_hh] per direction)."""
    n, T, I = x.shape
    D = len(params) // 4
    ps = [p.to(dtype) for p in params]
    whh = ps[1::4]
    wih_p, bias_p = pack_reference(ps, H)
    gin = (x.to(dtype).reshape(n * T, I) @ wih_p.t() + bias_p).view(n, T, D, H, 4)
    A, h = gru_forward_loop(gin, whh, H, dtype)
    Dg = gru_backward_loop(A, h, dh_in, whh, H, dtype)
    rows = Dg.reshape(n * T, D * 4 * H)
    dx = (rows @ wih_p).view(n, T, I)
    dwih = unpack_reference(rows.t() @ x.to(dtype).reshape(n * T, I), H, "ih")
    dbih = unpack_reference(rows.sum(0).unsqueeze(-1), H, "ih")
    dbhh = unpack_reference(rows.sum(0).unsqueeze(-1), H, "hh", defect)
    hp = shift(h)
    grads = []
    for d in range(D):
        dwhh_p = Dg[:, :, d].reshape(n * T, 4 * H).t() @ hp[:, :, d].reshape(n * T, H)
        grads += [dwih[d], unpack_reference(dwhh_p, H, "hh")[0], dbih[d].view(-1), dbhh[d].view(-1)]
    return h, dx, grads


def make_gru_whh(H, D, gen, device):
    b = H ** -0.5
    return [(torch.rand(3 * H, H, generator=gen, device=device) * 2 - 1) * b for _ in range(D)]


# ---- one RNNP layer on GRU containers: GRU + projection (+ Tanh), restated and by torch ------------------------------------
GRU_ATTRS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def layer_names(D):
    """the names of a layer's parameters in order: 4 per direction, then the projection"""
    base = ("w_ih", "w_hh", "b_ih", "b_hh")
    return base + tuple(n + "_r" for n in base)[:4 * (D - 1)] + ("w_proj", "b_proj")


def make_layer_params(I, H, hdim, D, gen, device="cpu"):
    """the 4 D + 2 tensors with torch.nn.GRU's / Linear's initial ranges"""
    def uni(bound, *shape):
        return (torch.rand(*shape, generator=gen, device=device) * 2 - 1) * bound
    b, bp = H ** -0.5, (D * H) ** -0.5
    gru = [t for _ in range(D) for t in (uni(b, 3 * H, I), uni(b, 3 * H, H), uni(b, 3 * H), uni(b, 3 * H))]
    return gru + [uni(bp, hdim, D * H), uni(bp, hdim)]


def make_layer_case(N, T, I, H, hdim, D, seed, combine=0):
    """-> x rows (n, t) [N T, I], the parameters, dy in the output's layout: fp32 values, fixed seed"""
    gen = torch.Generator().manual_seed(3000 + seed)
    params = make_layer_params(I, H, hdim, D, gen)
    x = torch.randn(N * T, I, generator=gen)
    K = combine or 1
    return x, params, torch.randn(N // K * T, K * hdim, generator=gen)


def gru_modules(params, device="cpu", dtype=torch.float32):
    """the tensors in torch.nn.GRU / Linear containers"""
    D = (len(params) - 2) // 4
    I, H, hdim = params[0].shape[1], params[1].shape[1], params[-2].shape[0]
    gru, lin = torch.nn.GRU(I, H, bidirectional=D == 2, batch_first=True), torch.nn.Linear(D * H, hdim)
    with torch.no_grad():
        for p, t in zip(module_params(gru, lin), params):
            p.copy_(t)
    return gru.to(device=device, dtype=dtype), lin.to(device=device, dtype=dtype)


def module_params(gru, lin):
    sfx = ("", "_reverse")[:2 if gru.bidirectional else 1]
    return [getattr(gru, a + s) for s in sfx for a in GRU_ATTRS] + [lin.weight, lin.bias]


def _combine_rows(y, N, T, K):
    hd = y.shape[-1]
    return y.reshape(N // K, K, T, hd).permute(0, 2, 1, 3).reshape(N // K * T, K * hd)


def _uncombine_rows(yc, N, T, K):
    hd = yc.shape[-1] // K
    return yc.reshape(N // K, T, K, hd).permute(0, 2, 1, 3).reshape(N * T, hd)


def torch_layer(x, params, dy, N, T, dtype, act=0, combine=0):
    """the layer by torch.nn.GRU + Linear (+ Tanh) under autograd -> {"y", "x", the parameter names}"""
    gru, lin = gru_modules(params, dtype=dtype)
    xr = x.to(dtype).view(N, T, -1).clone().requires_grad_()
    z = lin(gru(xr)[0]).reshape(N * T, -1)
    y = torch.tanh(z) if act else z
    y = _combine_rows(y, N, T, combine) if combine else y
    (y * dy.to(dtype)).sum().backward()
    out = {k: t.grad for k, t in zip(layer_names(len(params) // 4), module_params(gru, lin))}
    out.update(y=y.detach(), x=xr.grad.reshape(N * T, -1))
    return out


def layer_forward(x, params, N, T, dtype, act=0, combine=0, h0=None):
    """the restatement: the four-slot input product, the time loop, the projection, in `dtype` ("same formulas, torch,
    natural summation order")"""
    D = len(params) // 4
    p = [t.to(dtype) for t in params]
    H = p[1].shape[1]
    x = x.to(dtype).reshape(N * T, -1)
    wih_p, bias_p = pack_reference(p[:4 * D], H)
    gin = (x @ wih_p.t() + bias_p).view(N, T, D, H, 4)
    A, h = gru_forward_loop(gin, p[1:4 * D:4], H, dtype, h0=h0)
    z = h.reshape(N * T, D * H) @ p[-2].t() + p[-1]
    y_rows = torch.tanh(z) if act else z
    y = _combine_rows(y_rows, N, T, combine) if combine else y_rows
    return dict(x=x, A=A, h=h, y_rows=y_rows, y=y, N=N, T=T, H=H, D=D, act=act, combine=combine, p=p, wih_p=wih_p)


def layer_backward(fw, dy):
    """-> {"x": dx rows (n, t), the parameter names}: every gradient as the explicit sum it is"""
    N, T, H, D, p = fw["N"], fw["T"], fw["H"], fw["D"], fw["p"]
    dtype = fw["x"].dtype
    dy = dy.to(dtype)
    dy = _uncombine_rows(dy, N, T, fw["combine"]) if fw["combine"] else dy.reshape(N * T, -1)
    dz = dy * (1 - fw["y_rows"] ** 2) if fw["act"] else dy
    hcat = fw["h"].reshape(N * T, D * H)
    out = {"b_proj": dz.sum(0), "w_proj": dz.t() @ hcat}
    Dg = gru_backward_loop(fw["A"], fw["h"], (dz @ p[-2]).view(N, T, D, H), p[1:4 * D:4], H, dtype)
    rows = Dg.reshape(N * T, D * 4 * H)
    out["x"] = rows @ fw["wih_p"]
    dwih = unpack_reference(rows.t() @ fw["x"], H, "ih")
    col = rows.sum(0).unsqueeze(-1)
    dbih, dbhh = unpack_reference(col, H, "ih"), unpack_reference(col, H, "hh")
    hp = shift(fw["h"])
    for d, sfx in ((0, ""), (1, "_r"))[:D]:
        dwhh_p = Dg[:, :, d].reshape(N * T, 4 * H).t() @ hp[:, :, d].reshape(N * T, H)
        out["w_ih" + sfx], out["w_hh" + sfx] = dwih[d], unpack_reference(dwhh_p, H, "hh")[0]
        out["b_ih" + sfx], out["b_hh" + sfx] = dbih[d].view(-1), dbhh[d].view(-1)
    return out


def layer(x, params, dy, N, T, dtype, act=0, combine=0):
    """-> the restated layer's outputs {"y", "x", the parameter names} in `dtype`"""
    fw = layer_forward(x, params, N, T, dtype, act, combine)
    out = layer_backward(fw, dy)
    out["y"] = fw["y"]
    return out


def two_layers(x, p0, p1, dy, N, T, K, dtype, by_torch=False):
    """Layer 0 (act = 1, combine = K or 0) feeding layer 1 (act = 0, N / K sequences): the chain through tanh.
    -> {"y", "h", "dh", "x", "0.<name>", "1.<name>"}; by_torch: torch.nn.GRU + Linear + Tanh under autograd"""
    Kc = K or 1
    D = len(p0) // 4
    if by_torch:
        (g0, l0), (g1, l1) = gru_modules(p0, dtype=dtype), gru_modules(p1, dtype=dtype)
        xr = x.to(dtype).view(N, T, -1).clone().requires_grad_()
        h = torch.tanh(l0(g0(xr)[0]).reshape(N * T, -1))
        h = _combine_rows(h, N, T, K) if K else h
        h.retain_grad()
        y = l1(g1(h.view(N // Kc, T, -1))[0]).reshape(N // Kc * T, -1)
        (y * dy.to(dtype)).sum().backward()
        out = {"y": y.detach(), "h": h.detach(), "dh": h.grad, "x": xr.grad.reshape(N * T, -1)}
        out.update({"0." + k: t.grad for k, t in zip(layer_names(D), module_params(g0, l0))})
        out.update({"1." + k: t.grad for k, t in zip(layer_names(D), module_params(g1, l1))})
        return out
    f0 = layer_forward(x, p0, N, T, dtype, 1, K)
    f1 = layer_forward(f0["y"], p1, N // Kc, T, dtype, 0, 0)
    b1 = layer_backward(f1, dy)
    b0 = layer_backward(f0, b1["x"])
    out = {"y": f1["y"], "h": f0["y"], "dh": b1["x"], "x": b0["x"]}
    out.update({"0." + k: b0[k] for k in layer_names(D)})
    out.update({"1." + k: b1[k] for k in layer_names(D)})
    return out


def chunked_forward(x, params, N, T, chunks, dtype, act=0):
    """The one-direction layer's forward over consecutive chunks of frames, each started from the h the previous one ended
    in -> (y rows (n, t) [N T, hdim], the final h [N, H])."""
    x3 = x.to(dtype).view(N, T, -1)
    ys, h0, t0 = [], None, 0
    for n in chunks:
        fw = layer_forward(x3[:, t0:t0 + n], params, N, n, dtype, act, h0=h0)
        ys.append(fw["y"].view(N, n, -1))
        h0 = fw["h"][:, -1, 0]
        t0 += n
    return torch.cat(ys, 1).reshape(N * T, -1), h0


# ---- the two-layer chain: cases, and a yardstick over seeds for the toy width ---------------------------------------------------
CHAIN_SEED = 77
YARDSTICK_SEEDS = (77, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10)


def chain_case(N, T, I, H, hdim, K, D, seed=CHAIN_SEED):
    """-> x rows (n, t), the parameters of layer 0 and of layer 1 (whose input is layer 0's output, K-combined), dy"""
    gen = torch.Generator().manual_seed(seed)
    p0, p1 = make_layer_params(I, H, hdim, D, gen), make_layer_params((K or 1) * hdim, H, hdim, D, gen)
    x = torch.randn(N * T, I, generator=gen)
    return x, p0, p1, torch.randn(N // (K or 1) * T, hdim, generator=gen)


def chain_yardstick(N, T, I, H, hdim, K, D, seeds=YARDSTICK_SEEDS):
    """-> {tensor: (normwise, element-wise)}: the fp32 restatement's own error against float64 at this shape, the LARGEST
    over `seeds` (other weights and data, the same sizes).  At 5 units a tensor has 25 - 75 elements and its worst error is
    one or two roundings on one element, often one whose value nearly cancels: the figure of ONE draw moves by an order of
    magnitude from seed to seed (tests/test_gru_reference.py measures it) and by a factor of 4 with the host CPU's
    summation order alone, so one draw is no measure of what an fp32 implementation needs at this size; the largest of
    twelve is.  Everything here runs on the CPU; nothing comes from a kernel."""
    from test_rnnp_layer_reference import errors
    worst = {}
    for seed in seeds:
        x, p0, p1, dy = chain_case(N, T, I, H, hdim, K, D, seed)
        with torch.no_grad():
            r32 = two_layers(x, p0, p1, dy, N, T, K, torch.float32)
        r64 = two_layers(x, p0, p1, dy, N, T, K, torch.float64, by_torch=True)
        for k in r64:
            e = errors(r32[k], r64[k])
            worst[k] = tuple(max(a, b) for a, b in zip(worst.get(k, (0.0, 0.0)), e))
    return worst


def yardstick_report(got, ref64, yard, split, names=None):
    """tests/test_rnnp_layer_reference.py's `report` with the yardstick given: the bound of either figure is MARGIN x the
    yardstick's (never below U), x SPLIT_RATIO under split-bf16 GEMMs"""
    from test_rnnp_layer_reference import MARGIN, SPLIT_RATIO, U, errors
    s = MARGIN * (SPLIT_RATIO if split else 1.0)
    out = {}
    for k in names or ref64.keys():
        e, y = errors(got[k], ref64[k]), yard[k]
        out[k] = dict(norm=e[0], elem=e[1], bound_norm=s * max(y[0], U), bound_elem=s * max(y[1], U),
                      ratio=max(e[0] / max(y[0], U), e[1] / max(y[1], U)))
    return out
