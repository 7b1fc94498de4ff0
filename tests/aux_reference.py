"""float64 torch restatement of the reference's learned-embedding path (tssep/train/net.py:19-158, 250-330, 862-924),
written for this repository's tests: InstanceNorm, InstanceNorm_v2, Linear, AuxNet with REAL padding and the
length-aware mean, and the conditioning with its trial fold.  Everything is differentiable torch."""
import numpy as np
import torch


def instance_norm(x, dim=-1, unbiased=False):                       # net.py:281-285
    std, mean = torch.std_mean(x, dim=dim, unbiased=unbiased, keepdim=True)
    return (x - mean) / std


def instance_norm_v2(x, mean_dim=-1, norm_dim=-1):                  # net.py:322-330
    x = x - torch.mean(x, dim=mean_dim, keepdim=True)
    norm = torch.linalg.norm(x, dim=norm_dim, keepdim=True) / np.sqrt(x.shape[norm_dim])
    return x / norm


def linear(x, weight, bias=None):                                   # net.py:38-43
    y = x @ weight.t()
    return y if bias is None else y + bias


def _mlp_head(h, p):
    h = torch.relu(linear(h, p[0], p[1]))
    return torch.relu(linear(h, p[2], p[3]))


def auxnet_padded(seqs, p, normalizer=None):
    """net.py:142-149: pad_sequence, the whole net on the padded tensor, mean over the valid frames of every sequence.
    seqs: list of [T_i, idim]; p: (w1, b1, w2, b2, w3, b3); normalizer: callable on the padded tensor or None.
    With a per-row normalizer the all-zero padding rows become 0 / 0 = nan and `h * mask` keeps them (nan * 0): for
    ragged lengths the reference's own result is nan for every sequence but the longest.  The packed form below is what
    the valid rows define; the two agree whenever the padded one is finite."""
    lens = [len(s) for s in seqs]
    h = torch.nn.utils.rnn.pad_sequence(list(seqs), batch_first=True)
    if normalizer is not None:
        h = normalizer(h)
    h = linear(_mlp_head(h, p), p[4], p[5])
    mask = (torch.arange(h.shape[1])[None, :] < torch.as_tensor(lens)[:, None]).to(h.dtype)
    return (h * mask[..., None]).sum(1) / torch.as_tensor(lens, dtype=h.dtype)[:, None]


def auxnet_packed(seqs, p, normalizer=None):
    """The form the kernels compute: packed rows, mean BEFORE the (affine) last layer."""
    x = torch.cat(list(seqs), 0)
    if normalizer is not None:
        x = normalizer(x)
    h = _mlp_head(x, p)
    bounds = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    m = torch.stack([h[a:b].mean(0) for a, b in zip(bounds[:-1], bounds[1:])], 0)
    return linear(m, p[4], p[5])


def condition(pre, aux, combination, trials=1):
    """net.py:871-924: pre [B,T,F], aux [B,K,E] -> xs [B*trials, K, T, W]; trial tr holds speaker (k+tr) % K at k."""
    B, T, F = pre.shape
    K = aux.shape[1]
    if combination == "mul":
        xs = pre[:, None] * aux[:, :, None]
    else:
        xs = torch.cat([pre[:, None].expand(B, K, T, F), aux[:, :, None].expand(B, K, T, aux.shape[-1])], -1)
    idx = ((np.arange(K)[:, None] + np.arange(K)[None, :]) % K)[:trials].ravel()
    return xs[:, idx].reshape(B * trials, K, T, xs.shape[-1])
