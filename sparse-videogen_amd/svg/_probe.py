"""The quality probe's native op (include/svg_attn_sample_rows.h): dense attention of a few sampled query rows — fp32 rows and their row
log-sum-exp — streamed in one pass over K and V.  svg/models/_core.py sparse_quality sets a sparse layer-call against it.  Its K-only half,
sample_dense_lse (include/svg_attn_adaptive_top_p.h), feeds the controller of the adaptive top-p.

The allocating wrapper lives here, not in svg/_native.py: that module's public functions are the table of tests/test_gpu_poison.py.  Outputs
and workspace come from _native.empty like every allocation of the package."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native

MAX_ROWS = 64   # svg_sample_dense_rows: sampled rows of one call


def check_rows(rows: torch.Tensor, S: int) -> None:
    """ValueError unless rows is an int64 tensor of 1..MAX_ROWS rows of [0, S).  The values are read on CPU tensors only: the kernel cannot
    check a device tensor's rows, they are the caller's (include/svg_attn_sample_rows.h)."""
    if rows.dtype != torch.int64 or rows.dim() != 1:
        raise ValueError(f"sample_dense_rows: rows is an int64 vector, got {rows.dtype} {tuple(rows.shape)}")
    if not 1 <= rows.numel() <= MAX_ROWS:
        raise ValueError(f"sample_dense_rows: 1 to {MAX_ROWS} sampled rows, got {rows.numel()}")
    if not rows.is_cuda and (int(rows.min()) < 0 or int(rows.max()) >= S):
        raise ValueError(f"sample_dense_rows: rows outside [0, {S}): min {int(rows.min())}, max {int(rows.max())}")


def sample_dense_rows(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, rows: torch.Tensor, valid_len: Optional[int] = None,
                      sm_scale: Optional[float] = None):
    """q, k, v [cfg, H, S, D] views (bf16 / fp16, head_dim 64 / 128; token-major views are read in place, what the layout cannot describe is
    copied: _native._layout_plan); rows int64 [R], R <= 64, CPU (checked against [0, S), then uploaded) or device (the caller's fault) -> (o32 [cfg, H, R, D]
    fp32, lse [cfg, H, R] fp32): dense attention of the sampled rows over the keys dense_attention(valid_len=) gives them, natural-log lse.
    Duplicate rows are allowed, the order is kept."""
    if q.dim() != 4 or k.shape != q.shape or v.shape != q.shape:
        raise ValueError(f"sample_dense_rows: q, k, v are [cfg, H, S, D] of one shape, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    cfg, H, S, D = q.shape
    check_rows(rows, S)
    _native._gpu(q, k, v)
    lib = _native.load()
    rows = rows.to(q.device, non_blocking=True).contiguous()
    BH, R = cfg * H, rows.numel()
    o32 = _native.empty((cfg, H, R, D), dtype=torch.float32, device=q.device)
    lse = _native.empty((cfg, H, R), dtype=torch.float32, device=q.device)
    ws = _native.empty(lib.svg_sample_dense_rows_workspace_bytes(BH, R, D, S), dtype=torch.uint8, device=q.device)
    scale = _native._sm_scale(sm_scale, D)
    vl = 0 if valid_len is None else int(valid_len)
    p = _native._layout_plan(q, k, v, o=_native._NO_O)
    rc = lib.svg_sample_dense_rows(p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), rows.data_ptr(), R, BH, S, D, _native._dtype_code(q), scale, vl,
                                   o32.data_ptr(), lse.data_ptr(), ws.data_ptr(), ws.numel(), p.lay, _native._stream())
    _native._check(rc, "svg_sample_dense_rows")
    return o32, lse



# the K-only half of the probe (include/svg_attn_adaptive_top_p.h) lives in svg/_adaptive.py, beside what it feeds; it is reached from here too
from ._adaptive import sample_dense_lse  # noqa: E402,F401
