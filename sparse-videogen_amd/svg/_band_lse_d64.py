"""Band (SVG1) attention at head_dim 64 with the row log-sum-exp, and with fp32 rows (include/svg_attn_band_lse_d64.h): the allocating
wrappers of the four entries _native binds from BAND_LSE_D64_ENTRIES, reachable as _native.band_attention_lse_d64 and
_native.band_attention_switch_lse_d64.  _native.band_attention / band_attention_switch keep refusing return_lse at head_dim 64; these are
what a CogVideoX layer-call takes instead (svg/models/_core.py).  Outputs come from _native.empty / _layout_plan like every allocation of
the package."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native


def _plan(what: str, q, k, v, head_perm_flag, vid0, num_frame, frame_size, out_dtype, token_major_out, out):
    """refusals before anything is loaded, then (fp32 rows?, BH, S, D, perm, lse, layout plan)"""
    if q.shape[-1] != 64 or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{what}: head_dim 64, bf16 / fp16 (head_dim 128: band_attention(return_lse=True)); got D = {q.shape[-1]}, {q.dtype}")
    f32 = _native._want_f32_parts(what, out_dtype, True, out, token_major_out)
    _native._dev(head_perm_flag)
    _native._gpu(q, k, v, out)
    assert q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype
    S, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (S * D)
    _native.load()
    perm = _native._perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
    lse = _native.empty(q.shape[:-1], dtype=torch.float32, device=q.device)   # (contiguous [BH, S] whatever the layout of q / o)
    p = _native._layout_plan(q, k, v, o=_native._O32 if f32 else _native._O16, out=out, token_major_out=token_major_out)
    return f32, BH, S, D, perm, lse, p


def band_attention_lse_d64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: _native.BandMask, *, sm_scale: Optional[float] = None,
                           head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0, num_frame: int = 1, frame_size: int = 1,
                           out_dtype: Optional[torch.dtype] = None, token_major_out: bool = False, out: Optional[torch.Tensor] = None):
    """q, k, v: [B, H, S, 64] (or [BH, S, 64]) bf16 / fp16 GPU tensors -> (o, lse): o the bits of band_attention on the same arguments, lse
    the row log-sum-exp of the scaled scores over the keys the mask gives the row (natural log; -inf, with a zero row of o, where it gives
    none), contiguous fp32 of shape q.shape[:-1] in the row order of o — a part for merge_attention_states (svg_band_attention_lse_d64).
    Strided views, token_major_out, out: as band_attention.  out_dtype=torch.float32 (without out / token_major_out): (o32, lse) with o32
    the rows before their rounding, contiguous fp32 of q's shape (svg_band_attention_lse_d64_f32); o32.to(q.dtype) is o.  Anything but
    head_dim 64 at bf16 / fp16 raises ValueError."""
    f32, BH, S, D, perm, lse, p = _plan("band_attention_lse_d64", q, k, v, head_perm_flag, vid0, num_frame, frame_size, out_dtype,
                                        token_major_out, out)
    _native._call_lse("svg_band_attention_lse_d64", f32, p, lse, BH, S, D, _native._dtype_code(q), _native._sm_scale(sm_scale, D),
                      C.byref(mask), perm)
    return p.result(), lse


def band_attention_switch_lse_d64(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: _native.BandMask, alt_mask: _native.BandMask,
                                  use_alt_flag: torch.Tensor, *, sm_scale: Optional[float] = None,
                                  head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0, num_frame: int = 1, frame_size: int = 1,
                                  out_dtype: Optional[torch.dtype] = None, token_major_out: bool = False,
                                  out: Optional[torch.Tensor] = None):
    """band_attention_lse_d64 with the device switch of band_attention_switch: `use_alt_flag` (int32 [1] on the GPU) != 0 selects `alt_mask`
    without the head placement, otherwise `mask` with it; o, lse and o32 are in the row order the selected mask runs in
    (svg_band_attention_switch_lse_d64[_f32]).  No host read of the flag."""
    f32, BH, S, D, perm, lse, p = _plan("band_attention_switch_lse_d64", q, k, v, head_perm_flag, vid0, num_frame, frame_size, out_dtype,
                                        token_major_out, out)   # (the refusals first)
    _native._dev(use_alt_flag)
    assert use_alt_flag.dtype == torch.int32 and use_alt_flag.numel() >= 1
    _native._call_lse("svg_band_attention_switch_lse_d64", f32, p, lse, BH, S, D, _native._dtype_code(q), _native._sm_scale(sm_scale, D),
                      C.byref(mask), perm, C.byref(alt_mask), use_alt_flag.data_ptr())
    return p.result(), lse
