"""The float64 reference and element-wise bounds of the fused two-mask tail (tssep_mask_map_fwd / _bwd, tested on the
device in tests/test_gpu_two_mask_kernels.py), and the host behaviour of nmask > 1 -- all without a GPU.  The references
below run on the device of their inputs; here they run on the CPU.  Nothing in the reference part is compared with the
code under test: the restatement is anchored against oracle.net.mask_estimator_forward(nmask = 2 | 3) and float64
autograd, the fp32 rounding of its own outputs and an operation-by-operation fp32 emulation of the kernels' arithmetic
must lie inside the bounds, and its outputs with eight defects planted must fall outside them.

The tail (M = nmask masks per speaker, K speakers, `trials` averaged permutations, Fr = F for 'tf' and 1 for 't'):

    raw     the final Linear's output.  ts_vad: rows (b, trial, t), columns (spk mask freq); else rows (b, spk, t),
            columns (mask freq) (net.py:631-659).  Either way runs of Fr floats numbered (b, tr, t, k, m) / (b, k, t, m).
    logit   [B, K, M, T, F]: trial tr holds speaker (k + tr) % K at position k; mean over the trials (net.py:928-951);
            speaker s goes to output row perm[b, s], i.e. row j shows speaker iperm[b, j] (net.py:957-967); 't': the value
            repeated over f.
    mask    sigmoid(logit) (net.py:983)
    draw    (raw layout) the adjoint: term = dmask s (1 - s) [+ dlogit] per element, summed over f for 't', gathered back
            and divided by trials.

Bounds, U = 2^-24, first order; `finish` multiplies by SECOND = 1 + 2^-8 for the products of two relative errors and adds
TINY = 2^-126 for a result below the normal range (both from test_gated_reference.py).
  * logit: the bound of test_gpu_streaming_kernels.py::test_logit_map, (trials - 1) U mean_tr |raw|; exact (tolerance 0)
    at trials == 1.  For a power of two of trials the kernel adds the trials in order onto 0 in fp32 (the first addition
    is exact) and multiplies by fl(1 / trials), an exact scaling: trials - 1 rounded additions, each at most U times a
    partial sum <= sum_tr |raw|, scaled by 1 / trials.  For any other count fl(1 / trials) and the product with it would
    be two more roundings, which that bound has no room for (an fp32 emulation of `* fl(1 / 3)` left it in 247 of the
    78 948 logits of this file's trials = 3 settings, by up to 1.271 x), so the kernels carry the sum and the division in
    double and round once: U |mean| <= U mean |raw|, inside the bound for trials >= 2.  tssep_logit_map_fwd shares the
    device function, so the two stay bit-identical at M = 1.
  * mask = sigmoidf_mask(x) at the fp32 logit x THE KERNEL produced: mask_err(x, sigmoid(x)) = U s (8 + 2 |x|) + TINY
    (v_exp_f32 and v_rcp_f32 at 1 ulp each, the product with log2 e, the addition; test_gated_reference.py).  Taken
    at the kernel's own x, so the logit's error is not counted a second time.
  * draw, 'tf'.  The kernel reads the saved fp32 mask s^ with |s^ - s| <= e(l) = mask_err(l, s) and computes
    fl(fl(dm s^) fl(1 - s^)): |s^ (1 - s^) - s (1 - s)| <= e(l) |1 - s - s^| <= e(l), and two products, the
    subtraction and the first-order slack of the three make 4 U s (1 - s): |dm| (e(l) + 4 U s (1 - s)).  Every further
    operation costs U of its result: the dlogit addition, and for trials > 1 the product with fl(1 / trials) -- and the
    division that forms fl(1 / trials), which is an operation of its own exactly when trials is no power of two (it is
    exact otherwise).  Then finish.
  * draw, 't': the sum S over f of the same terms in logit_map_bwd_t_kernel's fixed order -- lane l adds its bins l,
    l + 64, ..., then six shuffle steps -- so a term passes through at most chain(F) = ceil(F / 64) + 6 + 1 roundings
    (test_gated_reference.py, the d(v) sum): chain(F) U sum_f |term_f|, plus the terms' own bounds summed, plus the
    1 / trials operations on S as above.

The planted defects are caught at the sizes of the GPU file (B = 2, T = 3, K = 3, M = 2, F = 5 among them) because of how
make_inputs draws: utterance b's permutation is the rotation by 1 + b, so perm != iperm in utterance 0 for K >= 3; raw is
3 randn, so |logit| ~ 3, a bf16 rounding moves it by 2^-9 relative (against at most 2 U) and the sigmoid of a mean is
far from the mean of the sigmoids; the rows of dmask and dlogit are scaled by 10^u with u in [-3, 3], independently, so
neighbouring masks' gradients differ by decades and dlogit dominates many rows."""
import einops
import pytest
import torch

from oracle import net as onet
from test_gated_reference import SECOND, TINY, U, chain, mask_err


def finish(tol):
    return tol * SECOND + TINY


# ------------------------------------------------------------------------------------------------------------ layouts
def raw_to_trials(raw, B, trials, K, M, T, Fr, spk_rows, columns="k m f"):
    """raw (flat) -> [B, trials, K (speaker), M, T, Fr]: the final einops rearrange and the trial convention.  `columns`
    is the order the ts_vad columns are read in ('k m f' is right); without ts_vad the same string without its k."""
    if spk_rows:
        cols = columns.replace("k", "").strip()
        pos = einops.rearrange(raw.reshape(B * K * T, M * Fr), f"(b k t) ({cols}) -> b 1 k m t f", b=B, k=K, t=T, m=M, f=Fr)
    else:
        pos = einops.rearrange(raw.reshape(B * trials * T, K * M * Fr), f"(b r t) ({columns}) -> b r k m t f",
                               b=B, r=trials, t=T, k=K, m=M, f=Fr)
    # trial r holds speaker (k + r) % K at position k: speaker s sits at position (s - r) % K
    return torch.stack([torch.roll(pos[:, r], r, dims=1) for r in range(pos.shape[1])], 1)


def unpermute(x, iperm):
    """[B, K (speaker), ...] -> [B, K (output row), ...]: row j shows speaker iperm[b, j]"""
    if iperm is None:
        return x
    return torch.take_along_dim(x, iperm.long().reshape(iperm.shape + (1,) * (x.dim() - 2)), 1)


def ref_fwd(raw, iperm, B, trials, K, M, T, F, Fr, spk_rows, defect=None):
    """raw float64 (flat) -> logit, mask [B, K, M, T, F] float64"""
    columns = {"freq_mask": "k f m", "mask_spk_freq": "m k f"}.get(defect, "k m f")
    spk = raw_to_trials(raw, B, trials, K, M, T, Fr, spk_rows, columns)
    logit = unpermute(spk.mean(1), iperm).expand(B, K, M, T, F)
    if defect == "bf16_logit":
        logit = logit.float().bfloat16().double()
    mask = torch.sigmoid(logit)
    if defect == "sigmoid_before_mean":
        mask = unpermute(torch.sigmoid(spk).mean(1), iperm).expand(B, K, M, T, F)
    return logit, mask


def to_raw(x, perm, B, trials, K, M, T, Fr, spk_rows):
    """[B, K (output row), M, T, Fr] -> the raw layout [B, trials, ...] (flat), a pure gather: every raw run receives the
    output run of its speaker.  The adjoint of the forward map is this over trials."""
    spk = unpermute(x, perm)                              # speaker s reads output row perm[b, s]
    pos = torch.stack([torch.roll(spk, -r, dims=1) for r in range(trials)], 1)            # position k: speaker (k + r) % K
    if spk_rows:
        return einops.rearrange(pos, "b 1 k m t f -> (b k t m f)")
    return einops.rearrange(pos, "b r k m t f -> (b r t k m f)")


def scale_ops(trials):
    """roundings of `* fl(1 / trials)`: the product, and the division when 1 / trials is no fp32 number"""
    if trials == 1:
        return 0
    return 1 if trials & (trials - 1) == 0 else 2


def logit_tol(raw, iperm, B, trials, K, M, T, F, Fr, spk_rows):
    if trials == 1:
        return torch.zeros(B, K, M, T, F, dtype=torch.float64, device=raw.device)
    mag, _ = ref_fwd(raw.abs(), iperm, B, trials, K, M, T, F, Fr, spk_rows)
    return (trials - 1) * U * mag


def mask_tol(x32):
    """the bound of the kernel's mask at the fp32 logit x32 it produced -> (sigmoid(x) float64, tol)"""
    x = x32.double()
    s = torch.sigmoid(x)
    return s, mask_err(x, s)


def ref_bwd(dm, l32, dl, perm, B, trials, K, M, T, F, Fr, spk_rows, defect=None):
    """dm, dl (or None) [B, K, M, T, F] float64 of the fp32 inputs, l32 the fp32 logit whose sigmoid the kernel saved ->
    (draw (flat, raw layout) float64, tol)"""
    l = l32.double()
    s = torch.sigmoid(l)
    mm = s * (1 - s)
    term = dm * mm
    e = dm.abs() * (mask_err(l, s) + 4 * U * mm)
    if dl is not None and defect != "dlogit_dropped":
        term = term + dl
        e = e + U * term.abs()
    if Fr == 1 and F != 1:
        e = e.sum(-1, keepdim=True) + chain(F) * U * term.abs().sum(-1, keepdim=True)
        term = term.sum(-1, keepdim=True)
    draw = to_raw(term, perm, B, trials, K, M, T, Fr, spk_rows) / trials
    tol = to_raw(e, perm, B, trials, K, M, T, Fr, spk_rows) / trials + scale_ops(trials) * U * draw.abs()
    if defect == "no_inv_trials":
        draw = draw * trials
    if defect == "grad_mask1_in_mask0":
        d = draw.view(-1, M, Fr).clone()
        d[:, 0] = d[:, 1]
        draw = d.reshape(-1)
    return draw, finish(tol)


# ----------------------------------------------------------------------------------- fp32 emulation of the arithmetic
def emulate_fwd_logit(raw32, iperm, B, trials, K, M, T, F, Fr, spk_rows):
    """the kernel's logit, operation by operation.  A power of two of trials: fp32, acc = 0; acc += raw (trial order);
    * fl(1 / trials).  Any other count: the same sum and the division in double, rounded to fp32 once."""
    spk = raw_to_trials(raw32, B, trials, K, M, T, Fr, spk_rows)
    exact = bool(trials & (trials - 1))
    acc = torch.zeros_like(spk[:, 0], dtype=torch.float64 if exact else torch.float32)
    for r in range(spk.shape[1]):
        acc = acc + spk[:, r]
    if exact:
        acc = (acc / float(trials)).float()
    elif trials > 1:
        acc = acc * torch.tensor(1.0, dtype=torch.float32, device=acc.device).div(float(trials))
    return unpermute(acc, iperm).expand(B, K, M, T, F)


def emulate_bwd(dm32, s32, dl32, perm, B, trials, K, M, T, F, Fr, spk_rows):
    """the kernel's draw in fp32: fl(fl(dm s) fl(1 - s)) [+ dl]; 't': lane l adds f = l, l + 64, ..., then the xor
    shuffle tree; * fl(1 / trials)"""
    g = (dm32 * s32) * (1.0 - s32)
    if dl32 is not None:
        g = g + dl32
    if Fr == 1 and F != 1:
        pad = (-F) % 64
        lanes = torch.nn.functional.pad(g, (0, pad)).reshape(*g.shape[:-1], -1, 64)
        acc = torch.zeros_like(lanes[..., 0, :])
        for i in range(lanes.shape[-2]):
            acc = acc + lanes[..., i, :]
        idx = torch.arange(64, device=g.device)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., idx ^ o]
        g = acc[..., :1]
    if trials > 1:
        g = g * torch.tensor(1.0, dtype=torch.float32, device=g.device).div(float(trials))
    return to_raw(g, perm, B, trials, K, M, T, Fr, spk_rows)


# ------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(B, K, M, T, F, Fr, trials, spk_rows, perm=True, seed=0, device="cpu"):
    """fp32 inputs as the kernels take them, drawn on the CPU (the same values on every device): raw 3 randn; dmask and
    dlogit randn with every (b, k, m, t) row scaled by 10^u, u in [-3, 3], independently; utterance b's permutation is
    the rotation by 1 + b."""
    g = torch.Generator().manual_seed(1000 + seed)
    n = B * K * M * T
    d = dict(B=B, K=K, M=M, T=T, F=F, Fr=Fr, trials=trials, spk_rows=int(spk_rows))
    d["raw"] = torch.randn(n * trials * Fr, generator=g).mul_(3).to(device)
    for name in ("dmask", "dlogit"):
        scale = 10.0 ** (torch.rand(B, K, M, T, 1, generator=g) * 6 - 3)
        d[name] = (torch.randn(B, K, M, T, F, generator=g) * scale).to(device)
    if perm:
        pm = (torch.arange(K)[None] + 1 + torch.arange(B)[:, None]) % K
        d["perm"], d["iperm"] = pm.int().to(device), torch.argsort(pm, dim=1).int().to(device)
    else:
        d["perm"] = d["iperm"] = None
    return d


def geometry(d):
    return tuple(d[k] for k in ("B", "trials", "K", "M", "T", "F", "Fr", "spk_rows"))


def outside(got32, ref, tol):
    """elements of the fp32 tensor outside the bound (NaN counts)"""
    return int((~((got32.double() - ref).abs() <= tol)).sum())


# the settings of the GPU file: (K, M, F, Fr == F, trials, spk_rows, perm, dlogit) -- the whole grid, plus two at F = 513
def gpu_settings():
    out = [(K, M, F, tf, trials, spk_rows, perm, dl)
           for K in (3, 4) for M in (1, 2, 3) for F in (5, 65) for tf in (True, False)
           for spk_rows, trials in ((1, 1), (0, 1), (0, 2), (0, K)) for perm in (False, True) for dl in (False, True)]
    out.append((3, 2, 513, True, 2, 0, True, True))
    out.append((3, 2, 513, False, 3, 0, True, False))
    return out


SETTINGS = gpu_settings()
GROUPS = sorted({s[:3] for s in SETTINGS})


def group_id(g):
    return "K%d-M%d-F%d" % g


def settings_of(group):
    return [s for s in SETTINGS if s[:3] == group]


def setting_id(s):
    K, M, F, tf, trials, spk_rows, perm, dl = s
    return f"K{K}-M{M}-F{F}-{'tf' if tf else 't'}-trials{trials}-{'rows' if spk_rows else 'cols'}-perm{int(perm)}-dl{int(dl)}"


def case_of(s, B=2, T=3, device="cpu", seed=None):
    K, M, F, tf, trials, spk_rows, perm, dl = s
    d = make_inputs(B, K, M, T, F, F if tf else 1, trials, spk_rows, perm, seed=SETTINGS.index(s) if seed is None else seed,
                    device=device)
    if not dl:
        d["dlogit"] = None
    return d


def test_the_settings_cover_the_grid():
    assert len(SETTINGS) == 2 * 3 * 2 * 2 * 4 * 2 * 2 + 2 and len(set(SETTINGS)) == len(SETTINGS)
    assert {s[4] for s in SETTINGS if s[5]} == {1} and {s[4] for s in SETTINGS if not s[5] and s[0] == 4} == {1, 2, 4}
    assert any(s[2] == 513 and s[3] for s in SETTINGS) and any(s[2] == 513 and not s[3] for s in SETTINGS)


# --------------------------------------------------------------------------------------------------------------- anchors
class _Spy(torch.overrides.TorchFunctionMode):
    """records the left operand of the matmul whose right operand is a view of `weight`: the final Linear's input"""

    def __init__(self, weight):
        super().__init__()
        self.weight, self.h = weight, None

    def __torch_function__(self, func, types, args=(), kwargs=None):
        if getattr(func, "__name__", "") in ("matmul", "__matmul__") and len(args) == 2 \
                and isinstance(args[1], torch.Tensor) and args[1].data_ptr() == self.weight.data_ptr():
            self.h = args[0]
        return func(*args, **(kwargs or {}))


def _oracle_params(K, ts_vad, res, nmask, trials, seed):
    g = torch.Generator().manual_seed(seed)
    idim, odim, units, projs = 7, 5, 4, 6
    shapes = {}

    def rnnp(prefix, i, h):
        for sfx in ("", "_reverse"):
            shapes[f"{prefix}net.0.weight_ih_l0{sfx}"] = (4 * units, i)
            shapes[f"{prefix}net.0.weight_hh_l0{sfx}"] = (4 * units, units)
            shapes[f"{prefix}net.0.bias_ih_l0{sfx}"] = (4 * units,)
            shapes[f"{prefix}net.0.bias_hh_l0{sfx}"] = (4 * units,)
        shapes[f"{prefix}net.1.weight"] = (h, 2 * units)
        shapes[f"{prefix}net.1.bias"] = (h,)
    rnnp("mask_estimator.pre_net.", idim, odim)
    for l in range(3):
        factor = K if (l == 2 and ts_vad) else 1
        rnnp(f"mask_estimator.post_net.birnn{l}.", (odim if l == 0 else projs) * factor, projs)
    nout = (odim if res == "tf" else 1) * nmask * (K if ts_vad else 1)
    shapes["mask_estimator.post_net.linear2.weight"] = (nout, projs)
    shapes["mask_estimator.post_net.linear2.bias"] = (nout,)
    p = {k: torch.randn(*s, generator=g, dtype=torch.float64) * 0.5 for k, s in shapes.items()}
    p["mask_estimator.post_net.linear2.weight"] *= 6             # |logit| of a few units
    return p, idim, odim


# (num_averaged_permutations > 1 needs ts_vad, net.py:547)
@pytest.mark.parametrize("ts_vad,res,trials,nmask", [(v, r, t, n) for v in (False, True) for r in ("tf", "t") for t in (1, 2)
                                                     for n in (2, 3) if v or t == 1])
def test_restatement_matches_the_oracle(ts_vad, res, trials, nmask):
    """Linear, rearrange, trial mean, un-permutation, sigmoid as restated here == oracle.net.mask_estimator_forward on the
    same final-Linear input (caught inside the oracle's own run), for ts_vad off / on, 'tf' / 't', trials 1 / 2."""
    B, K, T = 2, 3, 4
    p, idim, odim = _oracle_params(K, ts_vad, res, nmask, trials, seed=7)
    g = torch.Generator().manual_seed(8)
    xs = torch.randn(B, T, idim, generator=g, dtype=torch.float64)
    aux = torch.rand(B, K, odim, generator=g, dtype=torch.float64)
    d = make_inputs(B, K, nmask, T, odim, odim if res == "tf" else 1, trials, not ts_vad)
    w = p["mask_estimator.post_net.linear2.weight"]
    with _Spy(w) as spy:
        o = onet.mask_estimator_forward(p, xs, aux, odim=odim, nmask=nmask, combination="mul", ts_vad=K if ts_vad else False,
                                        output_resolution=res, num_averaged_permutations=trials, perm=d["perm"].numpy())
    assert spy.h is not None
    raw = spy.h @ w.t() + p["mask_estimator.post_net.linear2.bias"]               # the Linear
    logit, mask = ref_fwd(raw.reshape(-1), d["iperm"], B, trials, K, nmask, T, odim, d["Fr"], d["spk_rows"])
    assert tuple(o["logit"].shape) == (B, K, nmask, T, odim) == tuple(logit.shape)
    assert float(o["logit"].abs().max()) > 1
    assert float((logit - o["logit"]).abs().max()) <= 1e-13 * float(o["logit"].abs().max())
    assert float((mask - o["mask"]).abs().max()) <= 1e-14


@pytest.mark.parametrize("group", [g for g in GROUPS if g[2] == 5], ids=group_id)
def test_backward_reference_matches_autograd(group):
    """ref_bwd == float64 autograd of ref_fwd under sum(mask dmask) + sum(logit dlogit)"""
    for s in settings_of(group):
        _backward_matches_autograd(case_of(s))


def _backward_matches_autograd(d):
    geo = geometry(d)
    B, trials, K, M, T, F, Fr, spk_rows = geo
    raw = d["raw"].double().requires_grad_()
    logit, mask = ref_fwd(raw, d["iperm"], *geo)
    loss = (mask * d["dmask"].double()).sum()
    if d["dlogit"] is not None:
        loss = loss + (logit * d["dlogit"].double()).sum()
    (want,) = torch.autograd.grad(loss, raw)
    # (l32 = the float64 logit itself here: the formula, not its rounding)
    got, _ = ref_bwd(d["dmask"].double(), logit.detach(), None if d["dlogit"] is None else d["dlogit"].double(), d["perm"],
                     *geo)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


# ------------------------------------------------------------------------------------------- roundings inside the bounds
def references(d, defect=None):
    """{name: (ref, tol)} of a case, with the fp32 logit taken as the rounding of the reference's own"""
    geo = geometry(d)
    fwd_defect = defect if defect in ("freq_mask", "mask_spk_freq", "bf16_logit", "sigmoid_before_mean") else None
    iperm = d["perm"] if defect == "perm_for_iperm" else d["iperm"]
    logit, mask = ref_fwd(d["raw"].double(), iperm, *geo, defect=fwd_defect)
    clean, _ = ref_fwd(d["raw"].double(), d["iperm"], *geo)
    l32 = clean.float()
    s, e = mask_tol(l32)
    if defect is not None:                      # a defective forward is measured against the clean logit's sigmoid bound
        out = {"logit": (logit, None), "mask": (mask, None)}
    else:
        out = {"logit": (logit, logit_tol(d["raw"].double(), d["iperm"], *geo)), "mask": (s, e)}
    dl = None if d["dlogit"] is None else d["dlogit"].double()
    bwd_defect = defect if defect in ("dlogit_dropped", "no_inv_trials", "grad_mask1_in_mask0") else None
    out["draw"] = ref_bwd(d["dmask"].double(), l32, dl, d["perm"], *geo, defect=bwd_defect)
    out["l32"] = l32
    return out


@pytest.mark.parametrize("group", GROUPS, ids=group_id)
def test_clean_rounding_and_fp32_emulation_are_inside_every_bound(group):
    """The fp32 rounding of each reference output, and the kernels' arithmetic carried out operation by operation in
    the kernels' precision (the logit mean; the backward from the fp32 rounding of the float64 mask), lie inside the bounds everywhere."""
    for s in settings_of(group):
        _rounding_inside(s)


def _rounding_inside(s):
    d = case_of(s)
    geo = geometry(d)
    r = references(d)
    counts = {}
    for name in ("logit", "mask", "draw"):
        ref, tol = r[name]
        counts["rounded " + name] = outside(ref.float(), ref, tol)
    lg, tol = r["logit"]
    emu = emulate_fwd_logit(d["raw"], d["iperm"], *geo)
    counts["emulated logit"] = outside(emu, lg, tol)
    worst = float(((emu.double() - lg).abs() / tol.clamp(min=TINY)).max()) if geo[1] > 1 else 0.0
    s64, _ = mask_tol(emu)
    draw, dtol = ref_bwd(d["dmask"].double(), emu, None if d["dlogit"] is None else d["dlogit"].double(), d["perm"], *geo)
    emu_d = emulate_bwd(d["dmask"], s64.float(), d["dlogit"], d["perm"], *geo)
    counts["emulated draw"] = outside(emu_d, draw, dtol)
    worst_d = float(((emu_d.double() - draw).abs() / dtol).max())
    print(f"{setting_id(s)}: emulated logit {worst:.3f} of its bound, emulated draw {worst_d:.3f} of its bound")
    assert not any(counts.values()), counts


DEFECTS = {
    # name: (what must leave the bound, a filter on the settings it is planted in)
    "freq_mask": ("logit", lambda s: s[1] >= 2 and s[3]),
    "mask_spk_freq": ("logit", lambda s: s[1] >= 2 and not s[5]),
    "perm_for_iperm": ("logit", lambda s: s[6]),
    "sigmoid_before_mean": ("mask", lambda s: s[4] > 1),
    "grad_mask1_in_mask0": ("draw", lambda s: s[1] >= 2),
    "no_inv_trials": ("draw", lambda s: s[4] > 1),
    "dlogit_dropped": ("draw", lambda s: s[7]),
    "bf16_logit": ("logit", lambda s: True),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_planted_defect_falls_outside_the_bounds(defect):
    """Each defect, applied to the reference's own output and rounded to fp32, leaves the bounds of the clean one -- at
    EVERY setting of the GPU file the defect can show in, F = 5 included."""
    what, applies = DEFECTS[defect]
    cases = [s for s in SETTINGS if applies(s)]
    assert any(s[:3] == (3, 2, 5) for s in cases) or any(s[:3] == (3, 1, 5) for s in cases)
    fewest = None
    for s in cases:
        d = case_of(s)
        clean, bad = references(d), references(d, defect)
        ref, tol = clean[what]
        assert outside(ref.float(), ref, tol) == 0
        n = outside(bad[what][0].float(), ref, tol)
        assert n > 0, setting_id(s)
        if defect == "bf16_logit":                            # ... and its sigmoid leaves the mask's bound
            assert outside(bad["mask"][0].float(), *clean["mask"]) > 0, setting_id(s)
        if fewest is None or n / ref.numel() < fewest[0]:
            fewest = (n / ref.numel(), n, ref.numel(), setting_id(s))
    print(f"planted {defect}: {len(cases)} settings; fewest elements of {what} outside the bound: {fewest[1]} of {fewest[2]} "
          f"at {fewest[3]}")


# ------------------------------------------------------------------------------------------------------- host behaviour
KW = dict(idim=12, odim=9, layers=3, units=5, projs=6, combination="mul")


def test_two_mask_estimator_constructs():
    from tssep_amd.train.net import MaskEstimator_v2
    for ts_vad, factor in ((4, 4), (False, 1)):
        tf = MaskEstimator_v2(ts_vad=ts_vad, nmask=2, **KW)
        assert tf.nmask == 2 and tf._linear.out_features == 9 * 2 * factor           # odim nmask ts_factor
        t = MaskEstimator_v2(ts_vad=ts_vad, nmask=2, output_resolution="t", **KW)
        assert t._linear.out_features == 2 * factor
        one = MaskEstimator_v2(ts_vad=ts_vad, **KW)
        assert list(tf.state_dict()) == list(one.state_dict()) == list(t.state_dict())
        assert MaskEstimator_v2(ts_vad=ts_vad, nmask=3, **KW)._linear.out_features == 27 * factor


def test_one_mask_estimator_is_unchanged():
    from tssep_amd.train.net import MaskEstimator_v2
    a, b = MaskEstimator_v2(ts_vad=4, **KW), MaskEstimator_v2(ts_vad=4, nmask=1, **KW)
    assert repr(a) == repr(b) and a.nmask == 1
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
    assert a._linear.out_features == 36
    two = MaskEstimator_v2(ts_vad=4, nmask=2, **KW)
    assert [type(m).__name__ for m in two.modules()] == [type(m).__name__ for m in a.modules()]


def test_refusals():
    from tssep_amd.data import DummyReader
    from tssep_amd.train import enhancer, feature_extractor as fe, loss
    from tssep_amd.train.model import Model
    from tssep_amd.train.net import MaskEstimator_v2
    with pytest.raises(NotImplementedError, match="explicit_vad"):
        MaskEstimator_v2(ts_vad=4, nmask=2, explicit_vad=True, **KW)
    with pytest.raises(ValueError, match="nmask"):
        MaskEstimator_v2(ts_vad=4, nmask=0, **KW)
    two = MaskEstimator_v2(ts_vad=4, nmask=2, **KW)
    front = dict(fe=fe.Log1pMaxNormAbsSTFT(size=1024, shift=256, window="hann"), reader=DummyReader())
    with pytest.raises(ValueError, match="Masking"):
        Model(mask_estimator=two, enhancer=enhancer.Masking(), loss=loss.LogMAE(), **front)
    with pytest.raises(ValueError, match="VADSigmoidBCE"):
        Model(mask_estimator=two, enhancer=enhancer.TorchBF(), loss=loss.VADSigmoidBCE(), **front)
    Model(mask_estimator=two, enhancer=enhancer.TorchBF(differentiable=True), loss=loss.LogMAE(), **front)
    # the enhancer and the loss refuse a two-mask tensor themselves, whoever calls them
    masks = torch.zeros(1, 3, 2, 4, 9)
    with pytest.raises(ValueError, match="one mask per speaker"):
        enhancer.Masking()(masks, {"reference_channel": 0, "Observation": torch.zeros(1, 1, 4, 9, dtype=torch.complex64)}, None)
    with pytest.raises(ValueError, match="masks per speaker"):
        loss.VADSigmoidBCE().from_ex_out({"Vad": torch.zeros(1, 3, 4)}, Model.ForwardOutput(logit=masks), None, None)
    with pytest.raises(NotImplementedError):
        enhancer.ClassicBF_np(distortion_mask=None)(torch.zeros(3, 2, 4, 9), torch.zeros(6, 4, 9, dtype=torch.complex128), None,
                                                    segment_bf=False, numpy_out=True)


def test_default_model_config_keeps_one_mask():
    from tssep_amd.train.model import Model
    cfg = {}
    Model.finalize_dogmatic_config(cfg)
    assert cfg["mask_estimator"]["nmask"] == 1


def test_toy_overlay_resolves():
    import os
    from tssep_amd.train import enhancer, loss, run
    from tssep_amd.train.experiment import Experiment
    exp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tssep_amd", "exp")
    cfg = run.build_config([os.path.join(exp, y) for y in ("toy_common.yaml", "toy_tssep.yaml", "toy_tssep_two_mask.yaml")]
                           + ["eg.trainer.storage_dir=/tmp/unused"])
    eg = Experiment.from_config(cfg["eg"])
    m = eg.trainer.model
    assert m.mask_estimator.nmask == 2 and isinstance(m.enhancer, enhancer.TorchBF) and m.enhancer.differentiable
    assert isinstance(m.loss, loss.LogMAE) and eg.init_ckpt.init_ckpt is None
    K = m.mask_estimator.ts_vad
    assert m.mask_estimator._linear.out_features == K * 2 * 513


def test_kernel_plan_lists_the_tail():
    from tssep_amd.train import runtime
    assert runtime.summarise_plan([], [])["tail"] == []
    assert runtime.summarise_plan([], [], [dict(kernel="mask_map_fwd", M=2)])["tail"] == [dict(kernel="mask_map_fwd", M=2)]
