"""The allocating side of the Lloyd loop in steps (include/svg_attn_kmeans_stepped.h; the bindings on the caller's buffers are
svg._native.kmeans_stepped_*).  A module of its own, like svg/_adaptive_band.py: every allocation goes through svg._native.empty / empty_like,
so the side runs poisoned under _native.poison_allocations (tests/test_gpu_kmeans_stepped.py checks every output for unwritten words)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native


class KmeansSteppedSide:
    """One Lloyd loop in steps: `iterate(it)` runs iteration `it` and writes this side's group maxima into `maxima` (float32 [G], G = 1
    without a group — usually a slice of the tensor a driver reduces in one piece: svg.kmeans_utils.lloyd_stepped), `commit(it)` applies the
    stopping rule to whatever `maxima` holds by then, `finish()` -> (labels int32 [B, N], centroids [B, K, D], counts int32 [B, K], n_iters
    int32 [] or [G], sorted_idx int32 [B, N]) — with `maxima` untouched the bits of _native.kmeans_loop(x, None, c_init, max_iters, tol,
    group=group).  x: contiguous, or a view kmeans_loop reads in place (batches further apart than N * D); anything else is copied.
    Outputs, work buffers and workspace are allocated here, per side; every entry launches on the stream that is current when it is
    called."""

    def __init__(self, x: torch.Tensor, c_init: torch.Tensor, tol: float, group: Optional[int] = None, maxima: Optional[torch.Tensor] = None):
        B, N, D = x.shape
        K = c_init.shape[1]
        assert c_init.shape == (B, K, D) and c_init.dtype == x.dtype and c_init.is_contiguous()
        self.grouped = group is not None
        group = B if group is None else int(group)
        assert group >= 1 and B % group == 0, f"KmeansSteppedSide: group = {group} must divide B = {B}"
        G = B // group
        in_place = x.stride(2) == 1 and x.stride(1) == D and x.stride(0) >= N * D and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0
        self.x = x if in_place else x.contiguous()
        self.c_init, self.tol, self.group, self.G = c_init, float(tol), group, G
        self.maxima = _native.empty((G,), dtype=torch.float32, device=x.device) if maxima is None else maxima
        self.ca, self.cb = _native.empty_like(c_init), _native.empty_like(c_init)
        self.ws = _native.empty(_native.kmeans_stepped_workspace_bytes(B, N, K, D, group), dtype=torch.uint8, device=x.device)
        self.labels = _native.empty((B, N), dtype=torch.int32, device=x.device)
        self.sorted_idx = _native.empty((B, N), dtype=torch.int32, device=x.device)
        self.counts = _native.empty((B, K), dtype=torch.int32, device=x.device)

    def iterate(self, it: int) -> torch.Tensor:
        _native.kmeans_stepped_iterate(self.x, self.c_init, self.ca, self.cb, it, self.maxima, self.group, self.ws)
        return self.maxima

    def commit(self, it: int) -> None:
        _native.kmeans_stepped_commit(self.maxima, self.labels, self.counts, self.sorted_idx, it, self.tol, self.group, self.ws)

    def finish(self):
        cent = _native.empty_like(self.c_init)
        n_it = _native.empty((self.G,) if self.grouped else (), dtype=torch.int32, device=self.x.device)
        _native.kmeans_stepped_finish(self.c_init, self.ca, self.cb, cent, n_it, self.group, self.ws)
        return self.labels, cent, self.counts, n_it, self.sorted_idx
