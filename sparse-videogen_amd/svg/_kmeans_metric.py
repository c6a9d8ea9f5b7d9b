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
    _native.load()
    _native._dev(x, centroids)
    (B, N, D), K = x.shape, centroids.shape[1]
    assert centroids.shape == (B, K, D) and centroids.dtype == x.dtype
    return _native._kmeans_assign_call("svg_kmeans_assign_metric", x, centroids, _code(metric))


def kmeans_update_metric(x: torch.Tensor, labels: torch.Tensor, centroids_in: torch.Tensor, metric: str = "cosine"):
    """The update on given labels (svg_kmeans_update_metric) -> (unit centroids [B, K, D] of x.dtype, counts int32 [B, K], sorted_idx int32
    [B, N], shift float32 [B]).  'cosine' weights every row by 1 / |x|, 'dot' sums the rows as they are; an empty cluster returns its
    normalised centroids_in."""
    _native.load()
    _native._dev(x, labels, centroids_in)
    return _native._kmeans_update_call("svg_kmeans_update_metric", x, labels, centroids_in, _code(metric))


def kmeans_loop_metric(x: torch.Tensor, c_init: torch.Tensor, max_iters: int, tol: float, metric: str = "cosine", work=None,
                       group: Optional[int] = None):
    """The Lloyd loop of kmeans_loop under the cosine or the dot-product metric, one library call without host synchronisation
    (svg_kmeans_loop_metric) -> (labels int32 [B, N], centroids [B, K, D], counts int32 [B, K], n_iters int32 [] or [B // group] on the
    device, sorted_idx int32 [B, N]).  x: contiguous, or batches further apart with contiguous rows (read in place).  c_init is not
    written: 'cosine' normalises it into the workspace."""
    _native.load()
    code = _code(metric)
    return _native._kmeans_strided_loop("kmeans_loop_metric", "kmeans_metric", x, c_init, work, group,
                                        lambda g: (code, g, int(max_iters), float(tol)))
