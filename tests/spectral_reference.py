"""Float64 references and element-wise bounds of the FreqMSE kernels (tssep_amd/csrc/specloss.hip), shared by
tests/test_spectral_reference.py (CPU: the references themselves), tests/test_gpu_spectral_kernels.py and
tests/test_gpu_spectral.py.  Everything runs on the device of its inputs.

    cost[b,i,j] = sum_t (1/F) sum_f |E[b,i,t,f] - S[b,j,t,f]|^2        E = sigmoid(logit) Y (fused) or given (generic)
    loss[b]     = sum_k cost[b,k,p(k)],  p = identity or the best of the K! speaker permutations
    d loss / d E     = gout[b] (2/F) (E - t)            t = S[b, p(k)]
    d loss / d logit = gout[b] (2/F) Re(conj(d) Y) m (1 - m),   m = sigmoid(l), d = m Y - t

Bounds, U = 2^-24, first order; every tolerance is multiplied by SECOND = 1 + 2^-8 at the end and gets + TINY (``finish`` of
test_gated_reference.py, whose U, TINY, SECOND and device-sigmoid bound ``mask_err`` are imported, not restated).
The kernel's order of operations (contraction is off except where fmaf is written):
  * estimate component, fused: e_c^ = fl(m^ Y_c), |m^ - m| <= e_m = mask_err(l, m):  e_E,c = |Y_c| (e_m + U m).
    generic: the estimate is an input, e_E,c = 0 (complex128: its difference with the target is formed in double and
    rounded to float32 once -- the same single U |d_c| as the float32 subtraction).
  * d_c^ = fl(e_c^ - t_c):  e_d,c = e_E,c + U |d_c|.
  * a term q = |d|^2 enters its accumulator as acc = fmaf(d_re, d_re, acc); acc = fmaf(d_im, d_im, acc): propagated
    2 |d_re| e_d,re + 2 |d_im| e_d,im; the issue's 3 U q for the squares is kept although the fused squares round only
    with the sum (slack, not need).
  * the sum: a term passes through at most chain(F, T, ct) roundings -- a lane's running sum takes two fused adds per
    position, ceil(ct F / 256) positions of a chunk of ct frames; six steps of the shuffle tree; two adds over the four
    waves; the chunk sum of tssep_pit_assign, ceil(T / ct) adds; the division by F -- chain U sum q (all terms >= 0).
  * loss: the K matched costs are added in ascending k in float32: + K U sum_k cost.
  * backward, fused: dm^ = fl(fl(d_re^ Y_re) + fl(d_im^ Y_im)):  e(dm) = |Y_re| e_d,re + |Y_im| e_d,im + 3 U (|d_re Y_re| +
    |d_im Y_im|).  mm^ = fl(m^ fl(1 - m^)): |mm^ - mm| <= e_m + 2 U mm (|d mm / d m| <= 1; a 1 - m^ that rounds to 0 is
    covered by e_m, which is absolute).  coef^ = fl(2 gout / F): U.  out = fl(fl(coef^ dm^) mm^):
    |coef| (e(dm) mm + |dm| (e_m + 4 U mm)) + 2 U |dlogit|.
  * backward, generic complex64: fl(coef^ fl(E_c - t_c)): 4 U |dest_c|; complex128: double throughout, 8 x 2^-53 |dest_c|.
The reference permutation is found by brute force over itertools.permutations; ``gap`` is the distance from the best to
the second-best sum, and a pit comparison is made only where gap >= 100 x the forward bound (asserted, never assumed)."""
import itertools

import torch

from test_gated_reference import SECOND, TINY, U, bt_load, bt_store, finish, mask_err, outside, row_scale  # noqa: F401

U64 = 2.0 ** -53
SHAPES = [(1, 1, 1, 1), (2, 3, 9, 513), (2, 8, 5, 64), (1, 2, 3, 65), (3, 8, 2, 5)]
DEFECTS = ["mean_over_tf", "no_factor_2", "last_bin_dropped", "no_conj", "obs_of_utterance_0", "target_of_speaker_0",
           "bwd_ignores_perm", "bwd_inverse_perm", "iperm_for_perm"]


def chain(Fb, T, ct):
    """roundings a term of a cost passes through, at most (ct: the kernel's frames per chunk)"""
    return 2 * -(-(ct * Fb) // 256) + 6 + 2 + -(-T // ct) + 1


# ------------------------------------------------------------------------------------------------------------- inputs
def make_inputs(B, K, T, Fb, seed, device="cpu"):
    """fp32 / complex64 inputs as the kernels take them, drawn on the CPU (the same values on every device).  The
    Observation of utterance b is scaled by 10^u, u in [-3, 3] (utterances up to 1e6 apart), the target is a masked
    Observation of the speakers in another order plus noise -- so that a best permutation exists and E - S cancels --
    scaled per speaker by 10^u, u in [-1/2, 1/2].  perm: rotation by 1 + b (no involution at b = 0 for K >= 3); iperm:
    the inverse of the head's order K - 1 - k + b, a third arrangement.  One row of logits at +30, one at -30 (the sigmoid
    saturates), one whole frame with E == S in float32 (the fused estimate's own rounding), a few hundred single ties."""
    g = torch.Generator().manual_seed(seed)
    d = dict(B=B, K=K, T=T, F=Fb)
    logit = torch.randn(B, K, T, Fb, generator=g).mul_(3)
    logit[0, 0, 0] = 30.0
    logit[B - 1, K - 1, T - 1] = -30.0
    scale = row_scale(B, g, "cpu")
    obs = torch.randn(B, T, Fb, generator=g, dtype=torch.complex64) * scale[:, None, None]
    rot = (torch.arange(K)[None] + 1 + torch.arange(B)[:, None]) % K
    other = torch.sigmoid(logit + 0.5 * torch.randn(B, K, T, Fb, generator=g))
    other = other[torch.arange(B)[:, None], rot]                       # target j looks like estimate rot[b, j]
    spk = 10.0 ** (torch.rand(B, K, generator=g) - 0.5)
    tgt = obs[:, None] * other * spk[:, :, None, None]
    tgt = tgt + 0.1 * scale[:, None, None, None] * torch.randn(B, K, T, Fb, generator=g, dtype=torch.complex64)
    tgt = tgt.to(torch.complex64)
    # the exact tie over one whole frame: sigmoidf_mask(30) is exactly 1 (1 + 2^-43 rounds to 1), so E[0, 0, 0] = Y[0, 0]
    # bit for bit in the fused kernels too; planted under the identity pairing and under perm
    tgt[0, 0, 0] = obs[0, 0]
    tgt[0, rot[0, 0], 0] = obs[0, 0]
    est = (obs[:, None] * torch.sigmoid(logit)).to(torch.complex64)    # a generic estimate: any complex64 tensor
    est[0, 0, 0] = obs[0, 0]
    idx = torch.randint(0, est.numel(), (min(300, est.numel()),), generator=g)
    est.view(-1)[idx] = tgt.view(-1)[idx]                              # (and single ties of the identity pairing)
    est128 = est.to(torch.complex128) * (1 + 1e-9 * torch.randn(B, K, T, Fb, generator=g, dtype=torch.float64))
    est128[0, 0, 0] = obs[0, 0].to(torch.complex128)
    d.update(logit=logit, obs=obs, tgt=tgt, est=est, est128=est128)
    d["gout"] = torch.rand(B, generator=g) + 0.5
    d["perm"] = rot.int()
    head = (K - 1 - torch.arange(K)[None] + torch.arange(B)[:, None]) % K
    d["iperm"] = torch.argsort(head, dim=1).int()
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


# --------------------------------------------------------------------------------------------------------- references
def ref_estimate(lg, obs, defect=None):
    """lg [B,K,T,F] float64 of the fp32 logits, obs [B,T,F] complex128 -> E complex128, e_E [B,K,T,F,2] (per component)"""
    if defect == "obs_of_utterance_0":
        obs = obs[:1].expand_as(obs)
    m = torch.sigmoid(lg)
    o = obs[:, None]
    e = (mask_err(lg, m) + U * m)[..., None] * torch.view_as_real(o).abs()
    return o * m, e


def ref_costs(E, S, e_E=None, ct=4, diag_only=False, defect=None):
    """E, S [B,K,T,F] complex128 -> cost [B,K,K] float64 and its bound (diag_only: i != j is exactly 0)"""
    B, K, T, Fb = E.shape
    if defect == "target_of_speaker_0":
        S = S[:, :1].expand_as(S)
    d = torch.view_as_real(E[:, :, None] - S[:, None])                  # [B, i, j, T, F, 2]
    e_d = U * d.abs() + (0 if e_E is None else e_E[:, :, None])
    q = (d * d).sum(-1)
    t_q = (2 * d.abs() * e_d).sum(-1) + 3 * U * q
    if defect == "last_bin_dropped":
        q = q[..., :-1]
    div = Fb * (T if defect == "mean_over_tf" else 1)
    cost = q.sum((-1, -2)) / div
    tol = (t_q.sum((-1, -2)) + chain(Fb, T, ct) * U * q.sum((-1, -2))) / Fb
    if diag_only:
        eye = torch.eye(K, dtype=torch.bool, device=E.device)
        cost, tol = cost * eye, tol * eye
    return cost, finish(tol)


def all_perms(K, device):
    return torch.tensor(list(itertools.permutations(range(K))), dtype=torch.long, device=device)


def ref_loss(cost, tol, pit):
    """-> loss [B], its bound, perm int32 [B,K] (brute force over itertools.permutations), gap [B] (second best - best;
    inf where there is one permutation)"""
    B, K, _ = cost.shape
    P = all_perms(K, cost.device) if pit else torch.arange(K, device=cost.device)[None]
    rows = torch.arange(K, device=cost.device)
    sums = cost[:, rows, P].sum(-1)                                     # [B, nperm]
    tols = tol[:, rows, P].sum(-1) + K * U * cost[:, rows, P].abs().sum(-1)
    best = sums.argmin(-1)
    bi = torch.arange(B, device=cost.device)
    srt = sums.sort(-1).values
    gap = srt[:, 1] - srt[:, 0] if sums.shape[1] > 1 else torch.full((B,), float("inf"), device=cost.device)
    return sums[bi, best], finish(tols[bi, best]), P[best].int(), gap


def _gather_target(S, perm):
    B = S.shape[0]
    return S if perm is None else S[torch.arange(B, device=S.device)[:, None], perm.long()]


def _bwd_perm(perm, iperm, defect):
    if defect == "bwd_ignores_perm":
        return None
    if defect == "bwd_inverse_perm":
        return torch.argsort(perm.long(), dim=1)
    if defect == "iperm_for_perm":
        return iperm
    return perm


def ref_mask_bwd(lg, obs, S, perm, gout, iperm=None, defect=None, unfused=False):
    """-> d(logit) [B,K,T,F] float64 and its bound; perm None: identity; gout [B] fp32.
    unfused: the bound of the chain tssep_specmse_bwd -> tssep_maskhead_bwd on the mask head's own complex64 estimate
    (the same e_E): dest_c = fl(coef^ d_c^) carries 2 U |dest_c| before the dot product with Y, which the fused kernel
    applies to the finished dm instead: + 2 U |coef| (|d_re Y_re| + |d_im Y_im|) mm."""
    B, K, T, Fb = lg.shape
    E, e_E = ref_estimate(lg, obs, defect)
    if defect == "obs_of_utterance_0":
        obs = obs[:1].expand_as(obs)
    t = _gather_target(S[:, :1].expand_as(S) if defect == "target_of_speaker_0" else S, _bwd_perm(perm, iperm, defect))
    m = torch.sigmoid(lg)
    e_m = mask_err(lg, m)
    mm = m * (1 - m)
    y = torch.view_as_real(obs[:, None]).expand(B, K, T, Fb, 2)
    d = torch.view_as_real(E - t)
    e_d = e_E + U * d.abs()
    prod = d * y
    dm = prod[..., 0] - prod[..., 1] if defect == "no_conj" else prod.sum(-1)
    e_dm = (y.abs() * e_d).sum(-1) + 3 * U * prod.abs().sum(-1)
    coef = ((1.0 if defect == "no_factor_2" else 2.0) * gout.double() / (Fb * (T if defect == "mean_over_tf" else 1)))
    coef = coef[:, None, None, None]
    out = coef * dm * mm
    if defect == "last_bin_dropped":
        out = out.clone()
        out[..., -1] = 0
    c = (2.0 * gout.double() / Fb).abs()[:, None, None, None]
    tol = c * (e_dm * mm + dm.abs() * (e_m + 4 * U * mm)) + 2 * U * (c * dm * mm).abs()
    if unfused:
        tol = tol + 2 * U * c * prod.abs().sum(-1) * mm
    return out, finish(tol)


def ref_spec_bwd(E, S, perm, gout, f64, iperm=None, defect=None):
    """-> d(loss)/d(E) as reals [B,K,T,F,2] float64 and its bound (f64: the complex128 entry point)"""
    B, K, T, Fb = E.shape
    t = _gather_target(S[:, :1].expand_as(S) if defect == "target_of_speaker_0" else S, _bwd_perm(perm, iperm, defect))
    coef = ((1.0 if defect == "no_factor_2" else 2.0) * gout.double() / (Fb * (T if defect == "mean_over_tf" else 1)))
    out = torch.view_as_real(E - t) * coef[:, None, None, None, None]
    if defect == "last_bin_dropped":
        out = out.clone()
        out[..., -1, :] = 0
    clean = torch.view_as_real(E - _gather_target(S, perm)) * (2.0 * gout.double() / Fb)[:, None, None, None, None]
    return out, (8 * U64 if f64 else 4 * U) * clean.abs() * SECOND + (1e-300 if f64 else TINY)


def within(got, ref, tol, what):
    """every element of `got` within tol of ref (NaN fails); prints the worst ratio"""
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    ratio = float((err / tol).max()) if err.numel() else 0.0
    print(f"{what}: worst |err| / bound = {ratio:.3g}, outside {int(bad.sum())} of {err.numel()}")
    assert not bool(bad.any()), (what, ratio, int(bad.sum()))
