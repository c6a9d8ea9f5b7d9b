"""The allocating wrappers of the cosine / dot-product k-means entries (include/svg_attn_kmeans_metric.h: svg_kmeans_assign_metric,
svg_kmeans_update_metric, svg_kmeans_loop_metric), reachable as svg._native.kmeans_assign_metric / kmeans_update_metric /
kmeans_loop_metric.  A module of its own, like svg/_kmeans_e4m3.py: every output and workspace comes from svg._native.empty / empty_like,
so the wrappers run poisoned under _native.poison_allocations (tests/test_gpu_kmeans_metric.py takes its _native from
poisoned.load_native())."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native

METRICS = {"cosine": _native.KMEANS_COSINE, "dot": _native.KMEANS_DOT}


def _code(metric) -> int:
    if metric not in METRICS:
        raise ValueError(f"metric is 'cosine' or 'dot', got {metric!r} (the Euclidean metric keeps its own entries: kmeans_assign, ...)")
    return METRICS[metric]


def kmeans_assign_metric(x: torch.Tensor, centroids: torch.Tensor, metric: str = "cosine") -> torch.Tensor:
    """labels int32 [B, N] = arg-max_k <x_n, c_k>, lowest index on ties (svg_kmeans_assign_metric).  The raw x for both metrics: a row's
    norm does not change its arg-max."""
    lib = _native.load()
    _native._dev(x, centroids)
    B, N, D = x.shape
    K = centroids.shape[1]
    assert centroids.shape == (B, K, D) and centroids.dtype == x.dtype
    labels = _native.empty((B, N), dtype=torch.int32, device=x.device)
    ws = _native.empty(lib.svg_kmeans_workspace_bytes(B, N, K, D), dtype=torch.uint8, device=x.device)
    _native._check(lib.svg_kmeans_assign_metric(x.data_ptr(), centroids.data_ptr(), labels.data_ptr(), B, N, K, D, _native._dtype_code(x),
                                                _code(metric), ws.data_ptr(), ws.numel(), _native._stream()), "svg_kmeans_assign_metric")
    return labels


def kmeans_update_metric(x: torch.Tensor, labels: torch.Tensor, centroids_in: torch.Tensor, metric: str = "cosine"):
    """The update on given labels (svg_kmeans_update_metric) -> (unit centroids [B, K, D] of x.dtype, counts int32 [B, K], sorted_idx int32
    [B, N], shift float32 [B]).  'cosine' weights every row by 1 / |x|, 'dot' sums the rows as they are; an empty cluster returns its
    normalised centroids_in."""
    lib = _native.load()
    _native._dev(x, labels, centroids_in)
    B, N, D = x.shape
    K = centroids_in.shape[1]
    assert labels.dtype == torch.int32 and labels.shape == (B, N)
    assert centroids_in.shape == (B, K, D) and centroids_in.dtype == x.dtype
    cent = _native.empty_like(centroids_in)
    counts = _native.empty((B, K), dtype=torch.int32, device=x.device)
    sorted_idx = _native.empty((B, N), dtype=torch.int32, device=x.device)
    shift = _native.empty((B,), dtype=torch.float32, device=x.device)
    ws = _native.empty(lib.svg_kmeans_workspace_bytes(B, N, K, D), dtype=torch.uint8, device=x.device)
    _native._check(lib.svg_kmeans_update_metric(x.data_ptr(), labels.data_ptr(), centroids_in.data_ptr(), cent.data_ptr(), counts.data_ptr(),
                                                sorted_idx.data_ptr(), shift.data_ptr(), B, N, K, D, _native._dtype_code(x), _code(metric),
                                                ws.data_ptr(), ws.numel(), _native._stream()), "svg_kmeans_update_metric")
    return cent, counts, sorted_idx, shift


def kmeans_loop_metric(x: torch.Tensor, c_init: torch.Tensor, max_iters: int, tol: float, metric: str = "cosine", work=None,
                       group: Optional[int] = None):
    """The Lloyd loop of kmeans_loop under the cosine or the dot-product metric, one library call without host synchronisation
    (svg_kmeans_loop_metric) -> (labels int32 [B, N], centroids [B, K, D], counts int32 [B, K], n_iters int32 [] or [B // group] on the
    device, sorted_idx int32 [B, N]).  x: contiguous, or batches further apart with contiguous rows (read in place).  c_init is not
    written: 'cosine' normalises it into the workspace."""
    lib = _native.load()
    _native._dev(c_init)
    _native._gpu(x)
    B, N, D = x.shape
    K = c_init.shape[1]
    assert c_init.shape == (B, K, D) and c_init.dtype == x.dtype
    g = B if group is None else int(group)
    assert g >= 1 and B % g == 0, f"kmeans_loop_metric: group = {group} must divide B = {B}"
    if not (x.stride(2) == 1 and x.stride(1) == D and x.stride(0) >= N * D and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0):
        x = x.contiguous()
    key = _native.WorkspaceCache.key("kmeans_metric", B, N, K, D, x.dtype, g, device=x.device)
    w = None if work is None else work.get(key)
    if w is None:
        nb = lib.svg_kmeans_loop_metric_workspace_bytes(B, N, K, D, g)
        w = dict(ca=_native.empty_like(c_init), cb=_native.empty_like(c_init), ws=_native.empty(nb, dtype=torch.uint8, device=x.device))
        if work is not None:
            work[key] = w
    labels = _native.empty((B, N), dtype=torch.int32, device=x.device)
    sorted_idx = _native.empty((B, N), dtype=torch.int32, device=x.device)
    counts = _native.empty((B, K), dtype=torch.int32, device=x.device)
    cent = _native.empty_like(c_init)
    n_it = _native.empty(() if group is None else (B // g,), dtype=torch.int32, device=x.device)
    _native._check(lib.svg_kmeans_loop_metric(x.data_ptr(), int(x.stride(0)), c_init.data_ptr(), w["ca"].data_ptr(), w["cb"].data_ptr(),
                                              labels.data_ptr(), counts.data_ptr(), sorted_idx.data_ptr(), cent.data_ptr(), n_it.data_ptr(), B, N,
                                              K, D, _native._dtype_code(x), _code(metric), g, int(max_iters), float(tol), w["ws"].data_ptr(),
                                              w["ws"].numel(), _native._stream()), "svg_kmeans_loop_metric")
    return labels, cent, counts, n_it, sorted_idx
