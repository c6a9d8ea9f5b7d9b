"""The native ops of SVG1's adaptive band width that allocate (include/svg_attn_adaptive_band.h): band attention that reads one band per head
from a device vector, and its device-switch form.  The controller around them is svg/models/_core.py AdaptiveBand / BandStore /
adaptive_band_step; the non-allocating binding (band_width_update) is in svg/_native.py.  Outputs come from _native.empty / _layout_plan like
every allocation of the package."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native


def _checked(what: str, q, k, v, band, head_perm_flag, out):
    if q.shape[-1] != 128 or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{what}: head_dim 128, bf16 / fp16 (the row log-sum-exp form of the default schedule); got D = {q.shape[-1]}, {q.dtype}")
    _native._dev(head_perm_flag, band)
    _native._gpu(q, k, v, out)
    assert q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype
    S, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (S * D)
    _native._i32_vector(f"{what}(band)", band, BH)
    return BH, S, D


def band_attention_per_head(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: _native.BandMask, band: torch.Tensor,
                            sm_scale: Optional[float] = None, head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0,
                            num_frame: int = 1, frame_size: int = 1, out: Optional[torch.Tensor] = None, token_major_out: bool = False,
                            return_lse: bool = True, work_queue: bool = False):
    """band_attention(return_lse=True) with one band per head: band is a device int32 tensor of BH elements, and head h runs `mask` with its
    band replaced by min(max(band[h], 1), S + 1) — the bits of that call (svg_band_attention_per_head_lse: head_dim 128, bf16 / fp16; anything
    else raises ValueError).  The band is read on the device and never written.  -> (o, lse), or o alone with return_lse=False (the same
    launch).  work_queue=True: the same bits from resident workgroups on the work queue (svg_band_attention_per_head_queue_lse,
    include/svg_attn_band_per_head_queue.h)."""
    BH, S, D = _checked("band_attention_per_head", q, k, v, band, head_perm_flag, out)
    _native.load()
    perm = _native._perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
    lse = _native.empty(q.shape[:-1], dtype=torch.float32, device=q.device)   # (contiguous [BH, S] whatever the layout of q / o)
    p = _native._layout_plan(q, k, v, out=out, token_major_out=token_major_out)
    name = "svg_band_attention_per_head_queue_lse" if work_queue else "svg_band_attention_per_head_lse"
    _native._call_lse(name, False, p, lse, BH, S, D, _native._dtype_code(q), _native._sm_scale(sm_scale, D), C.byref(mask), band.data_ptr(), perm)
    return (p.result(), lse) if return_lse else p.result()


def band_attention_switch_per_head(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: _native.BandMask, alt_mask: _native.BandMask,
                                   use_alt_flag: torch.Tensor, band: torch.Tensor, sm_scale: Optional[float] = None,
                                   head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0, num_frame: int = 1, frame_size: int = 1,
                                   out: Optional[torch.Tensor] = None, token_major_out: bool = False, return_lse: bool = True,
                                   work_queue: bool = False):
    """band_attention_switch(return_lse=True) with one band per head: `use_alt_flag` (int32 [1] on the GPU) != 0 runs `alt_mask` as it is,
    without the head placement, and ignores `band`; otherwise band_attention_per_head (svg_band_attention_switch_per_head_lse).  work_queue=True: the same bits from
    resident workgroups on the work queue (svg_band_attention_switch_per_head_queue_lse)."""
    BH, S, D = _checked("band_attention_switch_per_head", q, k, v, band, head_perm_flag, out)
    _native._dev(use_alt_flag)
    assert use_alt_flag.dtype == torch.int32 and use_alt_flag.numel() >= 1
    _native.load()
    perm = _native._perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
    lse = _native.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    p = _native._layout_plan(q, k, v, out=out, token_major_out=token_major_out)
    name = "svg_band_attention_switch_per_head_queue_lse" if work_queue else "svg_band_attention_switch_per_head_lse"
    _native._call_lse(name, False, p, lse, BH, S, D, _native._dtype_code(q), _native._sm_scale(sm_scale, D), C.byref(mask), C.byref(alt_mask),
                      use_alt_flag.data_ptr(), band.data_ptr(), perm)
    return (p.result(), lse) if return_lse else p.result()
