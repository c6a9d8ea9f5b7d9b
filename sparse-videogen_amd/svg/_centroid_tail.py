"""The allocating wrappers of the centroid-tail entries (include/svg_attn_centroid_tail.h: svg_cluster_means,
svg_centroid_tail_attention_lse), reachable as svg._native.cluster_means / centroid_tail_attention.  A module of its own, like
svg/_kmeans_e4m3.py: every allocation goes through svg._native.empty, so the wrappers run poisoned under _native.poison_allocations
(tests/test_gpu_centroid_tail.py checks what they write and what they leave)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native

MAX_KC = 4032   # the variable-block limit on key clusters (csrc/varblock_policy.h kVbMaxKB)


def _refuse(what: str, ok: bool, msg: str) -> None:
    if not ok:
        raise ValueError(f"{what}: {msg}")


def cluster_means(x: torch.Tensor, sorted_idx: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
    """means [B, K, D] of x's dtype: row c of batch b is the mean of the counts[b, c] rows of x[b] that sorted_idx[b] lists for cluster c,
    summed in fp32 and rounded once; an empty cluster gives zeros (svg_cluster_means).
    x: [B, N, D] or [cfg, H, N, D] (B = cfg * H), bf16 / fp16, D 64 / 128 — read once and IN PLACE where it is a view whose last dimension is
    contiguous with strides that are multiples of 8 (the token-major view of a projection output); anything else is copied.
    sorted_idx int32 [B, N], counts int32 [B, K]: what the k-means loop returns."""
    what = "cluster_means"
    _refuse(what, x.dim() in (3, 4), f"x is [B, N, D] or [cfg, H, N, D], got {tuple(x.shape)}")
    N, D = x.shape[-2], x.shape[-1]
    B = x.numel() // max(N * D, 1)
    _refuse(what, x.dtype in (torch.bfloat16, torch.float16) and D in (64, 128), f"bf16 / fp16 and head_dim 64 / 128, got {x.dtype}, D = {D}")
    _refuse(what, sorted_idx.dtype == torch.int32 and counts.dtype == torch.int32, f"int32 sorted_idx and counts, got {sorted_idx.dtype}, {counts.dtype}")
    _refuse(what, sorted_idx.numel() == B * N and sorted_idx.shape[-1] == N, f"sorted_idx is [B, N] = [{B}, {N}], got {tuple(sorted_idx.shape)}")
    _refuse(what, counts.dim() >= 2 and counts.numel() // counts.shape[-1] == B, f"counts is [B, K] with B = {B}, got {tuple(counts.shape)}")
    K = counts.shape[-1]
    lib = _native.load()
    _native._dev(sorted_idx, counts)
    _native._gpu(x)
    x4 = x if x.dim() == 4 else x.unsqueeze(0)
    st = x4.stride()
    if not (st[3] == 1 and st[2] >= D and all(s % 8 == 0 and s >= 0 for s in st[:3]) and st[2] < (1 << 23) and x4.data_ptr() % 16 == 0):
        x4 = x4.contiguous()
        st = x4.stride()
    means = _native.empty((B, K, D), dtype=x.dtype, device=x.device)
    strides = None if x4.is_contiguous() else C.byref(_native.TensorStrides(st[0], st[1], st[2]))
    _native._check(lib.svg_cluster_means(x4.data_ptr(), strides, x4.shape[1], sorted_idx.data_ptr(), counts.data_ptr(), means.data_ptr(), B, N, K,
                                         D, _native._dtype_code(x), _native._stream()), "svg_cluster_means")
    return means


def centroid_tail_attention(q: torch.Tensor, kbar: torch.Tensor, vbar: torch.Tensor, block_map: torch.Tensor, q_sizes: torch.Tensor,
                            k_sizes: torch.Tensor, q_row_idx: Optional[torch.Tensor] = None, sm_scale: Optional[float] = None):
    """The attention state of every query row over the key clusters its block-row's map row does NOT select, each cluster one pseudo key
    (kbar_c, vbar_c) of weight k_sizes[c] (svg_centroid_tail_attention_lse) -> (o, lse): o contiguous of q's shape and dtype, lse fp32 of
    shape q.shape[:-1], natural logarithm, both in the caller's row order — a part for merge_attention_states beside
    varblock_attention(..., return_lse=True) under the same map.
    q: [H, Sq, 128] or [cfg, Hh, Sq, 128] (H = cfg * Hh), bf16 / fp16, read in place where the attention layout can describe it;
    kbar, vbar [H, KC, 128] (cluster_means); block_map bool / uint8 [H, QB, C] with C >= KC — only columns [0, KC) are read; q_sizes int32
    [H, QB]; k_sizes int32 [H, KC]; q_row_idx int32 [H, Sq] or None.
    A row whose clusters are all selected or empty: o = 0, lse = -inf.  A row no block-row covers is NOT written (the caller's
    q_sizes cover every row where k-means made them)."""
    what = "centroid_tail_attention"
    _refuse(what, q.dim() in (3, 4), f"q is [H, Sq, D] or [cfg, H, Sq, D], got {tuple(q.shape)}")
    Sq, D = q.shape[-2], q.shape[-1]
    H = q.numel() // max(Sq * D, 1)
    _refuse(what, D == 128 and q.dtype in (torch.bfloat16, torch.float16), f"head_dim 128, bf16 / fp16; got D = {D}, {q.dtype}")
    _refuse(what, kbar.dim() == 3 and kbar.shape[0] == H and kbar.shape[2] == D and vbar.shape == kbar.shape,
            f"kbar, vbar are [H, KC, D] = [{H}, KC, {D}], got {tuple(kbar.shape)}, {tuple(vbar.shape)}")
    _refuse(what, kbar.dtype == q.dtype and vbar.dtype == q.dtype, f"kbar, vbar of q's dtype {q.dtype}, got {kbar.dtype}, {vbar.dtype}")
    KC = kbar.shape[1]
    _refuse(what, 1 <= KC <= MAX_KC, f"1 to {MAX_KC} key clusters, got {KC}")
    _refuse(what, q_sizes.dim() == 2 and q_sizes.shape[0] == H and q_sizes.dtype == torch.int32, f"q_sizes is int32 [H, QB], got {tuple(q_sizes.shape)} {q_sizes.dtype}")
    QB = q_sizes.shape[1]
    _refuse(what, k_sizes.shape == (H, KC) and k_sizes.dtype == torch.int32, f"k_sizes is int32 [H, KC] = [{H}, {KC}], got {tuple(k_sizes.shape)} {k_sizes.dtype}")
    _refuse(what, block_map.dim() == 3 and block_map.shape[:2] == (H, QB) and block_map.shape[2] >= KC and block_map.dtype in (torch.bool, torch.uint8),
            f"block_map is bool / uint8 [H, QB, >= KC] = [{H}, {QB}, >= {KC}], got {tuple(block_map.shape)} {block_map.dtype}")
    if q_row_idx is not None:
        _refuse(what, q_row_idx.shape == (H, Sq) and q_row_idx.dtype == torch.int32, f"q_row_idx is int32 [H, Sq], got {tuple(q_row_idx.shape)} {q_row_idx.dtype}")
    lib = _native.load()
    _native._dev(kbar, vbar, block_map, q_sizes, k_sizes, q_row_idx)
    _native._gpu(q)
    q4 = _native._view4(q)
    lay = None
    if not q.is_contiguous():
        if _native._strided_ok(q4):
            lay = C.byref(_native.attn_layout(q4, q4, q4, q4))
        else:
            q4 = q4.contiguous()
    o = _native.empty(q.shape, dtype=q.dtype, device=q.device)
    lse = _native.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    ws = _native.empty(int(lib.svg_centroid_tail_workspace_bytes(H, QB, KC)), dtype=torch.uint8, device=q.device)
    _native._check(lib.svg_centroid_tail_attention_lse(q4.data_ptr(), kbar.data_ptr(), vbar.data_ptr(), o.data_ptr(), lse.data_ptr(), H, Sq, KC, D,
                                                       _native._dtype_code(q), _native._sm_scale(sm_scale, D), block_map.data_ptr(),
                                                       block_map.shape[2], q_sizes.data_ptr(), k_sizes.data_ptr(), QB, _native._ptr(q_row_idx),
                                                       ws.data_ptr(), ws.numel(), lay, _native._stream()), "svg_centroid_tail_attention_lse")
    return o, lse
