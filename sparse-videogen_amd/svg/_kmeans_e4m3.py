"""The allocating wrappers of the e4m3 k-means entries (include/svg_attn_kmeans_e4m3.h: svg_kmeans_centre, svg_kmeans_assign_e4m3,
svg_kmeans_loop_e4m3), reachable as svg._native.kmeans_centre / kmeans_assign_e4m3 / kmeans_loop_e4m3.  A module of its own, like
svg/_kmeans_stepped.py: every allocation goes through svg._native.empty / empty_like, so the wrappers run poisoned under
_native.poison_allocations (tests/test_gpu_kmeans_e4m3.py checks every output for unwritten words)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native


def kmeans_centre(centroids: torch.Tensor) -> torch.Tensor:
    """mu float32 [B, 128]: the channel mean of centroids [B, K, 128] in fp32 (svg_kmeans_centre)"""
    lib = _native.load()
    _native._dev(centroids)
    B, K, D = centroids.shape
    mu = _native.empty((B, D), dtype=torch.float32, device=centroids.device)
    _native._check(lib.svg_kmeans_centre(centroids.data_ptr(), mu.data_ptr(), B, K, D, _native._dtype_code(centroids), _native._stream()),
                   "svg_kmeans_centre")
    return mu


def kmeans_assign_e4m3(x: torch.Tensor, centroids: torch.Tensor, mu: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels int32 [B, N]: the arg-max (lowest index on ties) of the e4m3 scores of include/svg_attn_kmeans_e4m3.h around the centre mu
    float32 [B, 128] (None: zeros); head_dim 128 only (svg_kmeans_assign_e4m3)"""
    lib = _native.load()
    _native._dev(x, centroids, mu)
    B, N, D = x.shape
    K = centroids.shape[1]
    assert centroids.shape == (B, K, D) and centroids.dtype == x.dtype
    if mu is not None:
        _native._f32_vector("kmeans_assign_e4m3(mu)", mu, B * D)
    labels = _native.empty((B, N), dtype=torch.int32, device=x.device)
    ws = _native.empty(lib.svg_kmeans_assign_e4m3_workspace_bytes(B, N, K, D), dtype=torch.uint8, device=x.device)
    _native._check(lib.svg_kmeans_assign_e4m3(x.data_ptr(), centroids.data_ptr(), _native._ptr(mu), labels.data_ptr(), B, N, K, D,
                                              _native._dtype_code(x), ws.data_ptr(), ws.numel(), _native._stream()), "svg_kmeans_assign_e4m3")
    return labels


def kmeans_loop_e4m3(x: torch.Tensor, c_init: torch.Tensor, max_iters: int, tol: float, fp8_iters: int, work=None,
                     group: Optional[int] = None):
    """kmeans_loop whose first fp8_iters iterations assign with the e4m3 scores (svg_kmeans_loop_e4m3; fp8_iters = 0: the bits of
    kmeans_loop) -> (labels int32 [B, N], centroids [B, K, D], counts int32 [B, K], n_iters int32 [] or [B // group] on the device,
    sorted_idx int32 [B, N]).  x: contiguous, or batches further apart with contiguous rows (read in place); head_dim 128 only."""
    lib = _native.load()
    _native._dev(c_init)
    _native._gpu(x)
    B, N, D = x.shape
    K = c_init.shape[1]
    assert c_init.shape == (B, K, D) and c_init.dtype == x.dtype
    g = B if group is None else int(group)
    assert g >= 1 and B % g == 0, f"kmeans_loop_e4m3: group = {group} must divide B = {B}"
    if not (x.stride(2) == 1 and x.stride(1) == D and x.stride(0) >= N * D and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0):
        x = x.contiguous()
    key = _native.WorkspaceCache.key("kmeans_e4m3", B, N, K, D, x.dtype, g, device=x.device)
    w = None if work is None else work.get(key)
    if w is None:
        nb = lib.svg_kmeans_loop_e4m3_workspace_bytes(B, N, K, D, g)
        w = dict(ca=_native.empty_like(c_init), cb=_native.empty_like(c_init), ws=_native.empty(nb, dtype=torch.uint8, device=x.device))
        if work is not None:
            work[key] = w
    labels = _native.empty((B, N), dtype=torch.int32, device=x.device)
    sorted_idx = _native.empty((B, N), dtype=torch.int32, device=x.device)
    counts = _native.empty((B, K), dtype=torch.int32, device=x.device)
    cent = _native.empty_like(c_init)
    n_it = _native.empty(() if group is None else (B // g,), dtype=torch.int32, device=x.device)
    _native._check(lib.svg_kmeans_loop_e4m3(x.data_ptr(), int(x.stride(0)), c_init.data_ptr(), w["ca"].data_ptr(), w["cb"].data_ptr(),
                                    labels.data_ptr(), counts.data_ptr(), sorted_idx.data_ptr(), cent.data_ptr(), n_it.data_ptr(), B, N, K, D,
                                    _native._dtype_code(x), g, int(max_iters), float(tol), int(fp8_iters), w["ws"].data_ptr(), w["ws"].numel(),
                                    _native._stream()), "svg_kmeans_loop_e4m3")
    return labels, cent, counts, n_it, sorted_idx
