"""Batched k-means by direction — the reference's batch_kmeans_Cosine, batch_kmeans_Dot, triton_centroid_update_cosine and
triton_centroid_update_sorted_cosine (its svg/kmeans_utils.py:143-190, 328-372, 740-822) under their names and signatures, backed by the
HIP kernels of libsvgattn (include/svg_attn_kmeans_metric.h; csrc/kmeans.hip, csrc/kmeans_metric.hip).  No Triton, no eager fall-back.

They live in this module and not in svg.kmeans_utils: tests/test_api_surface_cpu.py pins those four names as absent from that module, and
existing tests are not changed by a feature.  `from svg.kmeans_metric import batch_kmeans_Cosine` is the import line.

Both loops run wholly inside the library (svg_kmeans_loop_metric), like batch_kmeans_Euclid(check_every=0): no F.normalize(x) tensor, no
[B, N, K] similarity tensor, no read-back per iteration."""
from __future__ import annotations

import torch

from . import _native
from .timer import time_logging_decorator

_LOOP_WORK = _native._KMEANS_WS   # the scratch cache of the library loops, per (shape, device, stream)


def _batch_kmeans_metric(metric, x, n_clusters, max_iters, tol, init_centroids, return_sorted_indices, group):
    assert x.is_cuda, f"batch_kmeans_{metric.capitalize()} requires GPU tensors"
    assert max_iters >= 1, "max_iters must be >= 1 (the reference raises NameError for 0)"
    B, N, D = x.shape
    if init_centroids is None:
        # ref :763 / :799 — random points of x as initial centres (the cosine loop normalises them on the device, as it does given ones)
        indices = torch.randint(0, N, (B, n_clusters), device=x.device)
        c_in = torch.gather(x, dim=1, index=indices[..., None].expand(-1, -1, D)).contiguous()
    else:
        c_in = init_centroids.reshape(B, n_clusters, D).to(x.dtype).contiguous()
    labels, cent, counts, n_it, sorted_idx = _native.kmeans_loop_metric(x, c_in, max_iters, tol, metric, work=_LOOP_WORK, group=group)
    out = (labels.to(torch.int64), cent, counts, n_it.to(torch.int64))
    return out + (sorted_idx,) if return_sorted_indices else out


@time_logging_decorator("Level 4 - batch kmeans cosine")
def batch_kmeans_Cosine(x, n_clusters, max_iters=100, tol=1e-4, init_centroids=None, verbose=False, *, return_sorted_indices=False,
                        group=None):
    """ref: batch_kmeans_Cosine, svg/kmeans_utils.py:740-787 — spherical k-means: points go to the centroid of the largest cosine, a
    centroid is the normalised mean of its points' unit vectors.

    x: [B, N, D] bf16/fp16 GPU tensor; a strided batch view (row stride D) is read in place.  Returns (cluster_ids int64 [B, N], unit
    centroids [B, K, D], cluster_sizes int32 [B, K], n_iters) and the stable sorted indices int32 [B, N] on request.  The loop, its
    stopping rule (the reference's `center_shift < tol`, :779) and `group` are those of batch_kmeans_Euclid(check_every=0): the whole
    loop runs inside the library (svg_kmeans_loop_metric) without a host read-back, so n_iters is an int64 GPU tensor (0-dim, or
    [B // group]) and `verbose=True` is accepted but prints nothing per iteration — there is no shift on the host to print.

    Departures from the reference's bits, on purpose: the assignment reads the raw x (a row's norm does not change its arg-max; the
    reference's F.normalize(x) is never materialised), the update accumulates x_n / max(|x_n|, 1e-12) in fp32 WITHOUT rounding the
    normalised row to 16 bits first, and every sum has a fixed order (bit-reproducible; the reference adds with atomics).  A zero row
    gets label 0."""
    return _batch_kmeans_metric("cosine", x, n_clusters, max_iters, tol, init_centroids, return_sorted_indices, group)


@time_logging_decorator("Level 4 - batch kmeans dot")
def batch_kmeans_Dot(x, n_clusters, max_iters=100, tol=1e-4, init_centroids=None, verbose=False, *, return_sorted_indices=False, group=None):
    """ref: batch_kmeans_Dot, svg/kmeans_utils.py:790-822 — points go to the centroid of the largest dot product, a centroid is the
    normalised mean of its points as they are (long rows pull harder); the initial centroids are used as given (:804), every later
    iteration runs on unit centroids.  Arguments, results and the loop as batch_kmeans_Cosine (verbose prints nothing: no host read-back)."""
    return _batch_kmeans_metric("dot", x, n_clusters, max_iters, tol, init_centroids, return_sorted_indices, group)


def triton_centroid_update_sorted_cosine(x_norm, cluster_ids, old_centroids, *, BLOCK_N: int = 256):
    """-> unit centroids [B, K, D] of x_norm.dtype (ref :328-372): the fp32 mean of each cluster's rows AS GIVEN (the caller has
    normalised them, or wants the dot-product update), rounded to the dtype, then normalised; an empty cluster returns its normalised
    old centroid.  svg_kmeans_update_metric with the dot metric: sums in a fixed order, bit-reproducible, unlike the reference's atomics."""
    assert x_norm.is_cuda and cluster_ids.is_cuda, "Inputs must be on CUDA"
    return _native.kmeans_update_metric(x_norm.contiguous(), cluster_ids.to(torch.int32).contiguous(),
                                        old_centroids.to(x_norm.dtype).contiguous(), "dot")[0]


def triton_centroid_update_cosine(x_norm, cluster_ids, old_centroids):
    """ref :143-190 (the unsorted, one-atomic-per-token kernel): the same result as the sorted form"""
    return triton_centroid_update_sorted_cosine(x_norm, cluster_ids, old_centroids)
