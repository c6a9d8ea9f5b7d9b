"""Torch statements of attention with a row log-sum-exp and of the N-way merge of attention states — what svg_cross_attention_lse and
svg_merge_attention_states compute, in whatever dtype the inputs have (float64 in the tests that use them as a reference).
ref: flashinfer's run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188."""
import math

import torch


def attention_lse(q, k, v, sm_scale=None, return_lse=True):
    """softmax(q k^T * sm_scale) v and lse = log sum_j exp(sm_scale * q.k_j) over the keys given; no key: zeros and -inf"""
    scale = 1.0 / math.sqrt(q.shape[-1]) if sm_scale is None else sm_scale
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if k.shape[-2] == 0:
        o = torch.zeros(q.shape[:-1] + (v.shape[-1],), dtype=q.dtype)
        lse = torch.full(q.shape[:-1], float("-inf"), dtype=q.dtype)
    else:
        lse = torch.logsumexp(s, dim=-1)
        o = torch.matmul(torch.exp(s - lse[..., None]), v)
    return (o, lse) if return_lse else o


def merge_states(o_parts, lse_parts, return_lse=False):
    """m = max_i lse_i, w_i = exp(lse_i - m), o = sum_i w_i o_i / sum_i w_i, lse = m + log sum_i w_i; -inf parts contribute nothing, all
    -inf: zeros and -inf.  Computed in the dtype of lse_parts[0] promoted with o's."""
    dt = torch.promote_types(o_parts[0].dtype, lse_parts[0].dtype)
    L = torch.stack([l.to(dt) for l in lse_parts])                     # [n, ...]
    O = torch.stack([o.to(dt) for o in o_parts])                       # [n, ..., D]
    m = L.max(dim=0).values
    m_safe = torch.where(torch.isinf(m) & (m < 0), torch.zeros_like(m), m)
    w = torch.exp(L - m_safe)                                          # exp(-inf) = 0
    sw = w.sum(0)
    contrib = torch.where(w[..., None] > 0, w[..., None] * O, torch.zeros_like(O))   # a part without weight is not looked at
    o = contrib.sum(0) / torch.where(sw > 0, sw, torch.ones_like(sw))[..., None]
    lse = torch.where(sw > 0, m_safe + torch.log(sw), torch.full_like(sw, float("-inf")))
    return (o, lse) if return_lse else o
