"""The native ops of SVG2's adaptive top-p that allocate (include/svg_attn_adaptive_top_p.h): sample_dense_lse, the K-only half of the quality
probe (svg/_probe.py re-exports it).  The controller around them is svg/models/_core.py AdaptiveTopP / TopPStore / adaptive_step; the
non-allocating bindings (identify_dynamic_map_per_head, top_p_update) are in svg/_native.py.  Outputs and workspace come from _native.empty
like every allocation of the package."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native


def sample_dense_lse(q: torch.Tensor, k: torch.Tensor, rows: torch.Tensor, valid_len: Optional[int] = None, sm_scale: Optional[float] = None):
    """The K-only half of sample_dense_rows (svg_sample_dense_lse, include/svg_attn_adaptive_top_p.h): q, k [cfg, H, S, D] views, rows as
    there -> lse [cfg, H, R] fp32 alone, the bits sample_dense_rows gives on the same call.  V is not read: the controller of the adaptive
    top-p needs the row log-sum-exp only (svg/models/_core.py AdaptiveTopP)."""
    from . import _probe   # (imports this module at its end)

    if q.dim() != 4 or k.shape != q.shape:
        raise ValueError(f"sample_dense_lse: q, k are [cfg, H, S, D] of one shape, got {tuple(q.shape)}, {tuple(k.shape)}")
    cfg, H, S, D = q.shape
    _probe.check_rows(rows, S)
    _native._gpu(q, k)
    lib = _native.load()
    rows = rows.to(q.device, non_blocking=True).contiguous()
    BH, R = cfg * H, rows.numel()
    lse = _native.empty((cfg, H, R), dtype=torch.float32, device=q.device)
    ws = _native.empty(lib.svg_sample_dense_lse_workspace_bytes(BH, R, S), dtype=torch.uint8, device=q.device)
    scale = _native._sm_scale(sm_scale, D)
    vl = 0 if valid_len is None else int(valid_len)
    p = _native._layout_plan(q, k, k, o=_native._NO_O)   # (no V: the layout's v member takes k's strides)
    rc = lib.svg_sample_dense_lse(p.q.data_ptr(), p.k.data_ptr(), rows.data_ptr(), R, BH, S, D, _native._dtype_code(q), scale, vl, lse.data_ptr(),
                                  ws.data_ptr(), ws.numel(), p.lay, _native._stream())
    _native._check(rc, "svg_sample_dense_lse")
    return lse
