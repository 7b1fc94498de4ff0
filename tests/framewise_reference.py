"""Speaker conditioning on FRAME-WISE embeddings restated in plain torch (float64: the reference; float32: the
yardstick), with the bound of every stage, and MaskEstimator_v2.forward with a time axis on the embedding.  Used by
tests/test_framewise_reference.py (CPU) and the two GPU files tests/test_gpu_framewise_*.py; nothing here touches the
code under test, and everything runs on the device of its inputs.

Definitions (tssep/train/net.py:862-894 at stride 1, + the trial fold :913-924).  aux [B, K, Ta, E], Ta = ceil(T / stride);
xs rows are (b, trial, k, t); trial tr holds speaker spk = (k + tr) % K at position k; frame t reads row ta = t // stride:

    mul   xs[b, tr, k, t, :] = pre[b, t, :] * aux[b, spk, ta, :]                                  (E == F)
    cat   xs[b, tr, k, t, :] = [pre[b, t, :] | aux[b, spk, ta, :]]
    d(pre)[b, t, :]     = sum_tr sum_k dxs[b, tr, k, t, :F] (* aux[b, spk, ta, :] for mul)
    d(aux)[b, s, ta, :] = sum_tr sum_{t in bucket ta} dxs[b, tr, (s - tr) % K, t, cols] (* pre[b, t, :] for mul)

bucket ta = frames [ta stride, min((ta + 1) stride, T)): the last one may be shorter, stride >= T gives one bucket.

Bounds (U = 2^-24, as in tests/test_gpu_gemm_kernels.py):
    forward mul   exact: the float64 product of two fp32 numbers is exact, so the kernel must give it rounded to fp32
    forward cat   exact (copies)
    d(pre) mul    n U sum|d a|, n = trials K   (n products, each rounded or fused, and n - 1 additions in any order)
    d(pre) cat    (n - 1) U sum|d|             (n - 1 additions)
    d(aux)        m U sum|terms|, m = trials (frames of the bucket)   (m terms: at most m - 1 additions, one rounding of
                  each product; any fixed order of the additions is inside it)

`defect` plants what an implementation of the time axis could get wrong:
    "drop_last_bucket"   the last, partial bucket is left out of d(aux)
    "mod_ta"             t % Ta instead of t // stride
    "rotate_time"        the trial rotation applied to the time index: aux[b, k, (ta + tr) % Ta]
    "no_clamp"           the bucket's end not clamped to T (stride >= T and every last partial bucket): d(aux) adds the
                         frames behind row T - 1 of the flat (b, tr, k, t) rows, i.e. the next block's first frames
"""
import numpy as np
import torch

from oracle.rnnp import rnnp

U = 2.0 ** -24
DEFECTS = ("drop_last_bucket", "mod_ta", "rotate_time", "no_clamp")


def gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def frames_of(T, stride):
    """Ta = ceil(T / stride)"""
    return -(-T // stride)


def inputs(B, K, trials, T, F, E, mul, stride, seed, device="cpu"):
    """-> pre [B, T, F], aux [B, K, Ta, C], dxs [B, trials, K, T, W] fp32 (C = W = F for mul; C = E, W = F + E for cat)"""
    g = gen(seed, device)
    Ta = frames_of(T, stride)
    pre = torch.randn(B, T, F, device=device, generator=g) + 0.5
    aux = torch.randn(B, K, Ta, F if mul else E, device=device, generator=g) + 0.25
    dxs = torch.randn(B, trials, K, T, F if mul else F + E, device=device, generator=g)
    return pre, aux, dxs


def targets(K, T, Ta, trials, stride, defect=None, device="cpu"):
    """-> (spk, ta) int64 [trials, K, T]: the embedding row (spk, ta) that row (tr, k, t) of xs is conditioned on"""
    tr = torch.arange(trials, device=device)[:, None, None]
    k = torch.arange(K, device=device)[None, :, None]
    t = torch.arange(T, device=device)[None, None, :]
    ta = t % Ta if defect == "mod_ta" else t // stride
    if defect == "rotate_time":
        return (k + 0 * tr + 0 * t), (ta + tr + 0 * k) % Ta
    return (k + tr + 0 * t) % K, ta + 0 * (k + tr)


def gathered(aux, T, trials, stride, defect=None):
    """aux [B, K, Ta, E] -> [B, trials, K, T, E]: the embedding row of every row (b, tr, k, t) of xs"""
    spk, ta = targets(aux.shape[1], T, aux.shape[2], trials, stride, defect, aux.device)
    return aux[:, spk, ta]


def cond_fwd(pre, aux, mul, trials, stride, dtype=torch.float64, defect=None):
    """-> xs [B, trials, K, T, W] in `dtype`"""
    B, T, F = pre.shape
    a = gathered(aux.to(dtype), T, trials, stride, defect)
    p = pre.to(dtype)[:, None, None].expand(B, trials, aux.shape[1], T, F)
    return p * a if mul else torch.cat([p, a], -1)


def cond_dpre(dxs, aux, mul, stride, dtype=torch.float64, defect=None):
    """dxs [B, trials, K, T, W] -> (d(pre) [B, T, F] in `dtype`, its bound in float64)"""
    B, trials, K, T, W = dxs.shape
    n = trials * K
    if mul:
        terms = dxs.to(dtype) * gathered(aux.to(dtype), T, trials, stride, defect)
        return terms.sum((1, 2)), n * U * terms.double().abs().sum((1, 2))
    F = W - aux.shape[-1]
    terms = dxs.to(dtype)[..., :F]
    return terms.sum((1, 2)), (n - 1) * U * terms.double().abs().sum((1, 2))


def cond_daux(dxs, pre, E, stride, dtype=torch.float64, defect=None):
    """dxs [B, trials, K, T, W], pre [B, T, F] (mul) or None (cat, the last E columns of dxs count)
    -> (d(aux) [B, K, Ta, C] in `dtype`, its bound in float64): the adjoint of `gathered`, summed bucket by bucket"""
    B, trials, K, T, W = dxs.shape
    mul = pre is not None
    C = W if mul else E
    Ta = frames_of(T, stride)
    dev = dxs.device
    d = dxs.to(dtype)[..., W - C:]
    terms = d * pre.to(dtype)[:, None, None] if mul else d                       # [B, trials, K, T, C]
    spk, ta = targets(K, T, Ta, trials, stride, defect, dev)
    row = (spk * Ta + ta).reshape(-1)
    used = terms
    if defect == "drop_last_bucket" and T % stride:
        used = terms * (ta != Ta - 1).to(dtype)[None, ..., None]
    out = terms.new_zeros(B, K * Ta, C).index_add_(1, row, used.reshape(B, -1, C))
    if defect == "no_clamp" and Ta * stride > T:
        # the last bucket runs on behind frame T - 1 of the flat rows (b, tr, k, t): the next block's first frames, and
        # zeros behind the last block
        X = Ta * stride - T
        flat = torch.cat([terms.reshape(-1, C), terms.new_zeros(X, C)], 0)
        rows = (torch.arange(B * trials * K, device=dev) * T + T)[:, None] + torch.arange(X, device=dev)
        extra = flat[rows].reshape(B, trials * K, X, C).sum(2)
        out.index_add_(1, (spk[:, :, 0] * Ta + Ta - 1).reshape(-1), extra)
    mag = torch.zeros(B, K * Ta, C, dtype=torch.float64, device=dev).index_add_(
        1, (lambda st: (st[0] * Ta + st[1]).reshape(-1))(targets(K, T, Ta, trials, stride, None, dev)),
        terms.double().abs().reshape(B, -1, C))
    width = torch.clamp(T - torch.arange(Ta, device=dev) * stride, max=stride).double()       # frames of every bucket
    bound = (trials * width)[None, None, :, None] * U * mag.view(B, K, Ta, C)
    return out.view(B, K, Ta, C), bound


def outside(got, ref, tol):
    """number of elements of the fp32 `got` further than `tol` from the float64 `ref` (a NaN counts)"""
    return int((~((got.double() - ref).abs() <= tol)).sum())


def worst(got, ref, tol):
    """max err / bound over the elements with a positive bound; every element must be inside"""
    err = (got.double() - ref).abs()
    assert bool((err <= tol).all()), (int((~(err <= tol)).sum()), got.numel(), float((err - tol).max()))
    pos = tol > 0
    return float((err[pos] / tol[pos]).max()) if bool(pos.any()) else 0.0


# ------------------------------------------------------------------------------------------------ MaskEstimator_v2.forward
def mask_estimator_forward(p, xs, aux, *, odim, aux_stride=1, combination="mul", ts_vad=False, output_resolution="tf",
                           num_averaged_permutations=1, layers=3, prefix="", perm=None, aux_normalizer=None):
    """oracle.net.mask_estimator_forward (nmask = 1) with the time axis of net.py:866-867: aux [B, K, Ta, E] is
    conditioned frame by frame, frame t on row t // aux_stride; a 3-D aux [B, K, E] takes the `unsqueeze` branch.  perm
    [B, K]: the speaker shuffle of the RAW aux (net.py:823-831), None = no shuffle; aux_normalizer: a callable on the
    shuffled aux (net.py:852-853).  -> dict(mask, logit [B, K, 1, T, F], embedding: aux as it entered the conditioning)."""
    assert xs.dim() == 3 and aux.dim() in (3, 4), (xs.shape, aux.shape)
    B, K = aux.shape[:2]
    T = xs.shape[1]
    if perm is not None:
        perm = np.asarray(perm)
        iperm = np.argsort(perm, axis=-1)
        aux = torch.stack([a[torch.as_tensor(q)] for a, q in zip(aux, perm)], 0)
    if aux_normalizer is not None:
        aux = aux_normalizer(aux)
    emb = aux
    xs = rnnp(xs, p, prefix + "pre_net.")
    if aux.dim() == 3:
        emb = aux4 = aux.unsqueeze(-2)
    else:
        assert aux.shape[2] == frames_of(T, aux_stride), (aux.shape, T, aux_stride)
        aux4 = aux[:, :, torch.arange(T) // aux_stride]
    if combination == "mul":
        xs = xs[..., None, :, :] * aux4
    elif combination == "cat":
        xs = torch.concat([xs[:, None].expand(B, K, T, xs.shape[-1]), aux4.expand(B, K, T, aux4.shape[-1])], dim=-1)
    else:
        raise NotImplementedError(combination)
    trials = num_averaged_permutations
    if trials > 1:
        idx = ((np.arange(K)[:, None] + np.arange(K)[None, :]) % K)[:trials].ravel()
        xs = xs[:, idx].reshape(B, trials, K, *xs.shape[-2:]).reshape(B * trials, K, *xs.shape[-2:])
    for l in range(layers):
        if l == layers - 1 and ts_vad is not False:
            n, k, t, f = xs.shape
            xs = xs.permute(0, 2, 1, 3).reshape(n, 1, t, k * f)
        xs = rnnp(xs, p, prefix + f"post_net.birnn{l}.")
        if l < layers - 1:
            xs = torch.tanh(xs)
    xs = xs @ p[prefix + f"post_net.linear{layers - 1}.weight"].t() + p[prefix + f"post_net.linear{layers - 1}.bias"]
    n, _, t, _ = xs.shape
    if output_resolution == "tf":
        if ts_vad is False:
            logit = xs.reshape(n, xs.shape[1], t, 1, odim).permute(0, 1, 3, 2, 4)
        else:
            logit = xs.reshape(n, t, ts_vad, 1, odim).permute(0, 2, 3, 1, 4)
    elif output_resolution == "t":
        if ts_vad is False:
            logit = xs.permute(0, 1, 3, 2)[..., None].expand(n, xs.shape[1], 1, t, odim)
        else:
            logit = xs.reshape(n, t, ts_vad, 1).permute(0, 2, 3, 1)[..., None].expand(n, ts_vad, 1, t, odim)
    else:
        raise ValueError(output_resolution)
    if trials > 1:
        logit = logit.reshape(B, trials * K, *logit.shape[2:])
        logit = logit[:, np.argsort(idx.ravel())]
        logit = logit.reshape(B, K, trials, *logit.shape[2:]).mean(dim=2)
    if perm is not None:
        logit = logit[np.arange(B)[:, None], iperm]
    return dict(mask=torch.sigmoid(logit), logit=logit, embedding=emb)
