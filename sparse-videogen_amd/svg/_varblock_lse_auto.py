"""Variable-block (SVG2) attention with the row log-sum-exp, and with fp32 rows, from the body the plain variant -1 call runs
(include/svg_attn_varblock_lse_auto.h): the allocating wrapper of the two entries _native binds from VARBLOCK_LSE_AUTO_ENTRIES, reachable
as _native.varblock_attention_lse_auto and through _native.varblock_attention(return_lse=True, body="auto").
_native.varblock_attention(return_lse=True) without `body` keeps running the two-phase 16x16x32 body whatever the shape, and keeps
refusing head_dim 64; this is what a layer-call below Sq = 160 block-rows, or at head_dim 64, takes instead (svg/models/_core.py).
Outputs come from _native.empty / _layout_plan like every allocation of the package."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native


def varblock_attention_lse_auto(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map: torch.Tensor, q_sizes: torch.Tensor,
                                k_sizes: torch.Tensor, *, sm_scale: Optional[float] = None, q_row_idx: Optional[torch.Tensor] = None,
                                kv_row_idx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                                token_major_out: bool = False, rows_covered: bool = False, out_dtype: Optional[torch.dtype] = None):
    """The arguments of varblock_attention -> (o, lse): o the bits of varblock_attention(variant=-1) on the same arguments, lse the row
    log-sum-exp of the scaled scores over the keys the block map gives the row (natural log), contiguous fp32 of shape q.shape[:-1] (per
    q head) in the caller's row order; -inf, with a zero row of o, for a row that sees no key and, without rows_covered, for a row no
    block-row covers.  head_dim 128 and 64, bf16 / fp16; anything else raises ValueError before the library is loaded.
    Strided views / token_major_out: as varblock_attention — where the two-phase bodies run (Sq >= 160 QB); below, copies and a
    head-major output.  out_dtype=torch.float32 (without token_major_out): (o32, lse) with o32 the rows before their rounding,
    contiguous fp32 of q's shape (svg_varblock_attention_lse_auto_f32), zero-filled first unless rows_covered; o32.to(q.dtype) is o."""
    what = "varblock_attention_lse_auto"
    if q.shape[-1] not in (64, 128) or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{what}: head_dim 128 or 64, bf16 / fp16; got D = {q.shape[-1]}, {q.dtype}")
    f32 = _native._want_f32_parts(what, out_dtype, True, None, token_major_out)
    _native._dev(block_map, q_sizes, k_sizes, q_row_idx, kv_row_idx)
    _native._gpu(q, k, v)
    lib = _native.load()
    Sq, D, Skv = q.shape[-2], q.shape[-1], k.shape[-2]
    Hq, Hkv = q.numel() // (Sq * D), k.numel() // (Skv * D)
    QB, KB = q_sizes.shape[-1], k_sizes.shape[-1]
    assert block_map.shape == (Hkv, QB, KB) and block_map.dtype in (torch.bool, torch.uint8)
    assert q_sizes.dtype == torch.int32 and k_sizes.dtype == torch.int32
    assert q_row_idx is None or (q_row_idx.dtype == torch.int32 and q_row_idx.shape == (Hq, Sq))
    assert kv_row_idx is None or (kv_row_idx.dtype == torch.int32 and kv_row_idx.shape == (Hkv, Skv))
    need = int(lib.svg_varblock_workspace_bytes(Hq, Hkv, QB, KB, Sq))
    ws = _native.empty(need, dtype=torch.uint8, device=q.device) if workspace is None else workspace
    _native._dev(ws)
    assert ws.dtype == torch.uint8 and ws.numel() >= need
    # (contiguous [Hq, Sq] whatever the layout of q / o; rows the kernel does not write: -inf where o holds zeros)
    lse = _native.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    if not rows_covered:
        lse.fill_(float("-inf"))
    p = _native._layout_plan(q, k, v, o=_native._O32 if f32 else _native._O16, token_major_out=token_major_out, zero_o=not rows_covered,
                             views=Sq >= 160 * QB)   # (the lock-step body takes contiguous tensors only)
    _native._call_lse("svg_varblock_attention_lse_auto", f32, p, lse, Hq, Hkv, Sq, Skv, D, _native._dtype_code(q),
                      _native._sm_scale(sm_scale, D), block_map.data_ptr(), q_sizes.data_ptr(), k_sizes.data_ptr(), QB, KB,
                      _native._ptr(q_row_idx), _native._ptr(kv_row_idx), ws.data_ptr(), ws.numel())
    return p.o, lse
