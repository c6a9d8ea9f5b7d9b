"""ctypes binding of libsvgattn.so (the C ABI declared in include/svg_attn.h).

PyTorch is only plumbing here: it owns the device memory and the HIP stream; every op below passes raw device
pointers + sizes + the current stream to the C entry point and raises on a non-zero status.  There is NO CPU
fallback: calling a native op without the library (or with CPU tensors) raises RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path
from typing import NamedTuple, Optional, Sequence

import torch

_LIB_PATH = Path(__file__).resolve().parent.parent / "lib" / "libsvgattn.so"
_lib: Optional[C.CDLL] = None
_load_error: Optional[str] = None

SVG_DTYPE_BF16, SVG_DTYPE_F16 = 0, 1


# ------------------------------------------------------------------------------------------------------
# the ONE allocation path of the package: every uninitialised tensor (outputs, workspaces, receive buffers) of svg/_native.py,
# svg/distributed.py, svg/kmeans_utils.py and svg/models/_core.py comes from these two callables — torch's own functions unless
# poison_allocations(True) swapped them (tests/test_poison_cpu.py walks the sources for calls that go round them)
# ------------------------------------------------------------------------------------------------------
POISON_BYTE = 0xFF   # bf16 / fp16 / fp32: a NaN, int32 / int64: -1, uint8: 255


def poison_storage(t: torch.Tensor) -> torch.Tensor:
    """Fill the WHOLE storage behind t with POISON_BYTE (a permuted or sliced view: every byte of what was allocated)."""
    st = t.untyped_storage()
    if st.nbytes():
        torch.zeros(0, dtype=torch.uint8, device=t.device).set_(st).fill_(POISON_BYTE)
    return t


def _poisoned_empty(*args, **kwargs) -> torch.Tensor:
    return poison_storage(torch.empty(*args, **kwargs))


def _poisoned_empty_like(*args, **kwargs) -> torch.Tensor:
    return poison_storage(torch.empty_like(*args, **kwargs))


empty = torch.empty
empty_like = torch.empty_like


def poison_allocations(on: bool) -> None:
    """on: every allocation of the package is followed by a fill of its storage with POISON_BYTE, so that what a launch leaves unwritten
    reads as NaN / -1 / 255 instead of what the memory held before (the GPU suite runs this way, tests/poisoned.py).  off (the default):
    torch.empty / torch.empty_like themselves.  Tensors a caller passes in (out=, workspace=) are never touched."""
    global empty, empty_like
    empty, empty_like = (_poisoned_empty, _poisoned_empty_like) if on else (torch.empty, torch.empty_like)


def allocations_poisoned() -> bool:
    return empty is _poisoned_empty


class BandMask(C.Structure):
    """svg_band_mask_t"""

    _fields_ = [
        ("real_len", C.c_int32),
        ("band", C.c_int32),
        ("colfull_lo", C.c_int32),
        ("colfull_hi", C.c_int32),
        ("rowfull_lo", C.c_int32),
        ("rowfull_hi", C.c_int32),
    ]

    def as_tuple(self):
        return (self.real_len, self.band, self.colfull_lo, self.colfull_hi, self.rowfull_lo, self.rowfull_hi)


class PermDesc(C.Structure):
    """svg_perm_desc_t"""

    _fields_ = [
        ("head_perm_flag", C.c_void_p),
        ("vid0", C.c_int32),
        ("num_frame", C.c_int32),
        ("frame_size", C.c_int32),
    ]


class ProfileVariant(C.Structure):
    """svg_profile_variant_t"""

    _fields_ = [
        ("coord", C.c_int32),
        ("origin", C.c_int32),
        ("span", C.c_int32),
        ("band_blocks", C.c_int32),
        ("sink_cols", C.c_int32),
        ("text_lo", C.c_int32),
        ("text_hi", C.c_int32),
    ]


class ProfileDesc(C.Structure):
    """svg_profile_desc_t"""

    _fields_ = [
        ("vid0", C.c_int32),
        ("num_frame", C.c_int32),
        ("frame_size", C.c_int32),
        ("emulate_bf16", C.c_int32),
        ("variant", ProfileVariant * 2),
    ]


_I32, _I64, _F32, _VP, _SZ = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t


class PrologueSegment(C.Structure):
    """svg_prologue_segment_t (include/svg_attn.h): one stream of svg_qk_norm_rope_transpose_joint."""
    _fields_ = [("q_in", C.c_void_p), ("k_in", C.c_void_p), ("v_in", C.c_void_p), ("rows", C.c_int32), ("norm_kind", C.c_int32),
                ("q_weight", C.c_void_p), ("q_bias", C.c_void_p), ("k_weight", C.c_void_p), ("k_bias", C.c_void_p), ("eps", C.c_float)]


class TensorStrides(C.Structure):
    """svg_tensor_strides_t: element strides of a [B, H, S, D] view whose last dimension is contiguous."""
    _fields_ = [("batch", C.c_int64), ("head", C.c_int64), ("row", C.c_int64)]


class AttnLayout(C.Structure):
    """svg_attn_layout_t (include/svg_attn.h): where q, k, v, o of a *_strided attention call live."""
    _fields_ = [("heads_per_batch", C.c_int32), ("kv_heads_per_batch", C.c_int32), ("q", TensorStrides), ("k", TensorStrides),
                ("v", TensorStrides), ("o", TensorStrides)]


# name -> (restype, argtypes); must list every symbol include/svg_attn.h declares (tests check this)
SIGNATURES = {
    "svg_abi_version": (C.c_int, []),
    "svg_strerror": (C.c_char_p, [C.c_int]),
    "svg_last_hip_error": (C.c_int, []),
    "svg_build_info": (C.c_char_p, []),
    "svg_debug_pp_trace": (C.c_int, [_VP]),
    "svg_debug_wg_trace": (C.c_int, [_VP, _I32]),
    "svg_band_queue_order": (_I32, [_I32, _I32, C.POINTER(BandMask), _VP, _I32]),
    "svg_debug_band_queue_cap": (C.c_int, [_I32]),
    "svg_debug_band_replays": (C.c_int64, [_I32]),
    "svg_debug_band_row_cursor": (_I32, [_I32, _I32, _I32, _I32, _I32, _VP, _I32, _VP, _I32, _VP]),
    "svg_debug_band_tile_run": (_I32, [_I32, C.POINTER(BandMask), _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _I32, _VP, _I32]),
    "svg_rms_norm_forward": (C.c_int, [_VP, _VP, C.c_int64, _I32, _I32, C.c_float, _VP]),
    "svg_layer_norm_forward": (C.c_int, [_VP, _VP, _VP, C.c_int64, _I32, _I32, _VP]),
    "svg_apply_qk_rope_inplace_cossin": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP]),
    "svg_apply_qk_rope_inplace_cossin_txtlast": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP]),
    "svg_apply_qk_rope_inplace_cossin_complex": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP]),
    "svg_bsr_to_block_map": (C.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
    "svg_layernorm_forward": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _I32, _I32, _I32, _I32, C.c_float, _VP]),
    "svg_rmsnorm_forward": (C.c_int, [_VP, _VP, _VP, C.c_int64, _I32, _I32, _I32, _I32, C.c_float, _VP]),
    "svg_layernorm_forward_ex": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _I32, _I32, _I32, _I32, C.c_float, _I32, _VP]),
    "svg_modulate_shift_forward": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _I32, C.c_int64, _I32, _I32, _VP]),
    "svg_modulate_gate_residual_forward": (C.c_int, [_VP, _VP, _VP, _VP, C.c_int64, _I32, C.c_int64, _I32, _I32, _I32, _VP]),
    "svg_layernorm_modulate_forward": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _I32, C.c_int64, _I32, _I32, _I32,
                                                 C.c_float, _VP]),
    "svg_layernorm_modulate_forward_ex": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, C.c_int64, _I32, C.c_int64, _I32, _I32, _I32,
                                                    C.c_float, _I32, _VP]),
    "svg_qk_norm_rope_transpose": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP,
                                             C.c_float, _I32, _VP, _VP, _I32, _I32, _VP]),
    "svg_qk_norm_rope": (C.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, C.c_float, _I32, _VP,
                                   _VP, _I32, _I32, _VP]),
    "svg_qk_norm_rope_qscale": (C.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP, C.c_float, _I32, _VP,
                                          _VP, _I32, _I32, C.c_float, _VP]),
    "svg_qk_norm_rope_transpose_qscale": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _VP, _VP,
                                                    C.c_float, _I32, _VP, _VP, _I32, _I32, C.c_float, _VP]),
    "svg_qk_norm_rope_transpose_joint": (C.c_int, [C.POINTER(PrologueSegment), _I32, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP,
                                                   _I32, _I32, C.c_float, _VP]),
    "svg_rmsnorm_rope_transpose": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _I32, C.c_float, _I32, _VP,
                                             _VP, _I32, _I32, C.c_float, _VP]),
    "svg_head_placement": (C.c_int, [_VP, _VP, _I32, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _VP]),
    "svg_permute_rows": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP]),
    "svg_inverse_permute_rows": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _VP]),
    "svg_argsort_workspace_bytes": (_SZ, [_I32, _I32, _I32]),
    "svg_argsort_labels": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "svg_band_attention": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                     C.POINTER(PermDesc), _I32, _VP]),
    "svg_band_attention_strided": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                             C.POINTER(PermDesc), C.POINTER(AttnLayout), _VP]),
    "svg_band_attention_switch_strided": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                                    C.POINTER(PermDesc), C.POINTER(BandMask), _VP, C.POINTER(AttnLayout), _VP]),
    "svg_varblock_attention_strided": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _VP,
                                                 _I32, _I32, _VP, _VP, _VP, _SZ, C.POINTER(AttnLayout), _VP]),
    "svg_cross_attention": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, C.POINTER(AttnLayout), _VP]),
    "svg_cross_attention_keyrange": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _I32, C.POINTER(AttnLayout),
                                               _VP]),
    "svg_cross_attention_pair": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _F32, C.POINTER(AttnLayout),
                                           C.POINTER(AttnLayout), _VP]),
    "svg_cross_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _I32, C.POINTER(AttnLayout),
                                          _VP]),
    "svg_merge_attention_states": (C.c_int, [_VP, _VP, _I32, _VP, _VP, _I32, _I32, _I32, _I32, C.POINTER(AttnLayout), _VP]),
    "svg_cross_attention_lse_f32": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _I32, C.POINTER(AttnLayout),
                                              _VP]),
    "svg_merge_attention_states_f32": (C.c_int, [_VP, _VP, _I32, _VP, _VP, _I32, _I32, _I32, _I32, C.POINTER(AttnLayout), _VP]),
    "svg_sample_mse_strided": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, C.POINTER(ProfileDesc), _VP, _VP,
                                         _SZ, _VP, C.POINTER(AttnLayout), _VP]),
    "svg_band_attention_prescaled": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, C.POINTER(BandMask), C.POINTER(PermDesc), _VP]),
    "svg_band_attention_switch_prescaled": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, C.POINTER(BandMask),
                                                      C.POINTER(PermDesc), C.POINTER(BandMask), _VP, _VP]),
    "svg_debug_clock_probe": (C.c_int, [_VP, _VP, _I32, _VP]),
    "svg_band_attention_prescaled_notify_seg": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, C.POINTER(BandMask),
                                                          C.POINTER(PermDesc), _VP, _I32, _I32, _VP]),
    "svg_band_attention_notify_target": (_I32, [_I32, C.POINTER(BandMask)]),
    "svg_band_attention_notify": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                            C.POINTER(PermDesc), _VP, _I32, _VP]),
    "svg_varblock_attention_fp8_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32, _I32, _I32, _I32]),
    "svg_varblock_attention_fp8": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _VP, _I32, _I32,
                                             _VP, _VP, _VP, _SZ, _VP]),
    "svg_band_attention_fp8_workspace_bytes": (_SZ, [_I32, _I32, _I32]),
    "svg_band_attention_fp8": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _VP, _SZ, _VP]),
    "svg_band_attention_fp8_stage": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _VP, _SZ, _I32, _VP]),
    "svg_wait_counters": (C.c_int, [_VP, _I32, _I32, _VP]),
    "svg_wait_counters_deadline": (C.c_int, [_VP, _I32, _I32, _I32, _VP, _VP]),
    "svg_band_attention_notify_layout": (_I32, [_I32, C.POINTER(BandMask), _I32, _VP, _VP]),
    "svg_band_attention_notify_seg": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                                C.POINTER(PermDesc), _VP, _I32, _I32, _VP]),
    "svg_band_attention_switch": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                            C.POINTER(PermDesc), C.POINTER(BandMask), _VP, _VP]),
    "svg_band_groups_attention": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask), C.POINTER(BandMask),
                                            C.POINTER(_I32), _I32, C.POINTER(PermDesc), _VP, _I32, C.POINTER(AttnLayout), _VP]),
    "svg_sample_mse_flagged": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, C.POINTER(ProfileDesc), _VP, _VP,
                                         _SZ, _VP, _VP]),
    "svg_varblock_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    "svg_varblock_attention": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _VP,
                                         _I32, _I32, _VP, _VP, _VP, _SZ, _I32, _VP]),
    "svg_sample_mse_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32]),
    "svg_sample_mse": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, C.POINTER(ProfileDesc), _VP, _VP,
                                 _SZ, _VP]),
    "svg_kmeans_xsq": (C.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _VP]),
    "svg_kmeans_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32]),
    "svg_kmeans_iter": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "svg_kmeans_assign": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "svg_kmeans_update": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "svg_kmeans_loop_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32]),
    "svg_kmeans_loop": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _SZ, _VP]),
    "svg_kmeans_loop_strided": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _SZ, _VP]),
    "svg_kmeans_loop_grouped_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    "svg_kmeans_loop_grouped": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _SZ,
                                          _VP]),
    "svg_kmeans_loop_grouped_strided": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32,
                                                  _VP, _SZ, _VP]),
    "svg_identify_dynamic_map": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, _I32, _VP]),
    "svg_map_density": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _VP]),
}


SVG_ABI_VERSION = 4   # include/svg_attn.h


# include/svg_attn_sparse_lse.h: the row log-sum-exp forms of band and variable-block attention.  A table of their own, as the header is:
# tests/test_entry_validation_cpu.py pins a validation table to every svg_band_attention* / svg_varblock_attention* name of SIGNATURES; the
# table (and the prototype check) of these two is tests/test_sparse_attention_lse_cpu.py.  load() types both tables.
SPARSE_LSE_SIGNATURES = {
    "svg_band_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask), C.POINTER(PermDesc),
                                         C.POINTER(AttnLayout), _VP]),
    "svg_varblock_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _VP, _VP, _I32, _I32,
                                             _VP, _VP, _VP, _SZ, C.POINTER(AttnLayout), _VP]),
}

# include/svg_attn_f32_parts.h: their fp32-row forms, in a table of their own for the same reason (tests/test_attention_f32_parts_cpu.py)
SPARSE_F32_SIGNATURES = {
    "svg_band_attention_lse_f32": SPARSE_LSE_SIGNATURES["svg_band_attention_lse"],
    "svg_varblock_attention_lse_f32": SPARSE_LSE_SIGNATURES["svg_varblock_attention_lse"],
}


# include/svg_attn_band_lse_forms.h: the LSE / fp32 forms of the device-switch and groups launches of band attention, in a table of their own
# for the same reason (tests/test_band_lse_forms_cpu.py)
BAND_LSE_FORM_SIGNATURES = {
    "svg_band_attention_switch_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask), C.POINTER(PermDesc),
                                                C.POINTER(BandMask), _VP, C.POINTER(AttnLayout), _VP]),
    "svg_band_groups_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask), C.POINTER(BandMask),
                                                C.POINTER(_I32), _I32, C.POINTER(PermDesc), _VP, C.POINTER(AttnLayout), _VP]),
}
BAND_LSE_FORM_SIGNATURES["svg_band_attention_switch_lse_f32"] = BAND_LSE_FORM_SIGNATURES["svg_band_attention_switch_lse"]
BAND_LSE_FORM_SIGNATURES["svg_band_groups_attention_lse_f32"] = BAND_LSE_FORM_SIGNATURES["svg_band_groups_attention_lse"]


# include/svg_attn_band_window.h: band attention over a row window and a key window of the mask, in a table of its own for the same reason
# (tests/test_band_window_cpu.py)
BAND_WINDOW_SIGNATURES = {
    "svg_band_window_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32,
                                                C.POINTER(BandMask), C.POINTER(AttnLayout), _VP]),
}
BAND_WINDOW_SIGNATURES["svg_band_window_attention_lse_f32"] = BAND_WINDOW_SIGNATURES["svg_band_window_attention_lse"]


class BandShard(C.Structure):
    """svg_band_shard_t (include/svg_attn_band_shard.h): the whole frames [f0, f0 + n_frames) of the video, frame-major, and behind them the
    sequence rows [tail_begin, tail_begin + n_tail) behind the video"""

    _fields_ = [("f0", C.c_int32), ("n_frames", C.c_int32), ("tail_begin", C.c_int32), ("n_tail", C.c_int32)]

    def as_tuple(self):
        return (self.f0, self.n_frames, self.tail_begin, self.n_tail)


# include/svg_attn_band_shard.h: band attention of a frame shard of the rows over a frame shard of the keys, in a table of its own for the
# same reason (tests/test_band_shard_cpu.py)
BAND_SHARD_SIGNATURES = {
    "svg_band_shard_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask), C.POINTER(PermDesc),
                                               C.POINTER(BandShard), C.POINTER(BandShard), C.POINTER(AttnLayout), _VP]),
    "svg_debug_band_shard_map": (_I32, [C.POINTER(PermDesc), _I32, C.POINTER(BandShard), _I32, _VP, _I32, _VP, _VP]),
}
BAND_SHARD_SIGNATURES["svg_band_shard_attention_lse_f32"] = BAND_SHARD_SIGNATURES["svg_band_shard_attention_lse"]

# include/svg_attn_band_shard_switch.h: the device switch between two masks of the shard form, in a table of its own for the same reason
# (tests/test_band_shard_switch_cpu.py)
BAND_SHARD_SWITCH_SIGNATURES = {
    "svg_band_shard_attention_switch_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                                      C.POINTER(PermDesc), C.POINTER(BandMask), _VP, C.POINTER(BandShard),
                                                      C.POINTER(BandShard), C.POINTER(AttnLayout), _VP]),
}
BAND_SHARD_SWITCH_SIGNATURES["svg_band_shard_attention_switch_lse_f32"] = BAND_SHARD_SWITCH_SIGNATURES["svg_band_shard_attention_switch_lse"]

# include/svg_attn_profile_shard.h: the online profiler's partial over one key shard and the combine over partials, in a table of its own
# for the same reason (tests/test_profile_shard_cpu.py)
PROFILE_SHARD_SIGNATURES = {
    "svg_sample_mse_shard_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32]),
    "svg_sample_mse_shard_partial": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, C.POINTER(ProfileDesc),
                                               C.POINTER(BandShard), _VP, _VP, _SZ, _VP, C.POINTER(AttnLayout), _VP]),
    "svg_sample_mse_from_parts_workspace_bytes": (_SZ, [_I32]),
    "svg_sample_mse_from_parts": (C.c_int, [_VP, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _VP, _SZ, _VP, _VP]),
}

# include/svg_attn_sample_rows.h: the quality probe's dense rows, in a table of its own for the same reason (tests/test_sample_rows_cpu.py;
# the allocating wrapper is svg/_probe.py sample_dense_rows)
SAMPLE_ROWS_SIGNATURES = {
    "svg_sample_dense_rows_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32]),
    "svg_sample_dense_rows": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, _I32, _VP, _VP, _VP, _SZ,
                                        C.POINTER(AttnLayout), _VP]),
}

# include/svg_attn_adaptive_top_p.h: SVG2's per-head top-p — the block map from a device vector, the K-only probe, the controller step —, in
# a table of its own for the same reason (tests/test_adaptive_top_p_cpu.py; allocating wrappers: svg/kmeans_utils.py identify_dynamic_map,
# svg/_probe.py sample_dense_lse)
ADAPTIVE_TOP_P_SIGNATURES = {
    "svg_identify_dynamic_map_per_head": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _I32, _VP]),
    "svg_sample_dense_lse_workspace_bytes": (_SZ, [_I32, _I32, _I32]),
    "svg_sample_dense_lse": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, _I32, _VP, _VP, _SZ, C.POINTER(AttnLayout), _VP]),
    "svg_top_p_update": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _F32, _F32, _F32, _F32, _F32, _F32, _VP, _VP, _VP]),
}


# include/svg_attn_adaptive_band.h: SVG1's per-head band width — band attention from a device vector of bands, its device switch, the
# controller step —, in a table of its own for the same reason (tests/test_adaptive_band_cpu.py; allocating wrappers: svg/_adaptive_band.py).
# (Named ..._ENTRIES: tests/test_wrapper_layout_plan_cpu.py wants a golden transcript for every attention entry of a *SIGNATURES table, and
#  its golden is closed; the transcripts of these wrappers are in tests/test_adaptive_band_cpu.py.)
ADAPTIVE_BAND_ENTRIES = {
    "svg_band_attention_per_head_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask), _VP,
                                                  C.POINTER(PermDesc), C.POINTER(AttnLayout), _VP]),
    "svg_band_attention_switch_per_head_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                                         C.POINTER(BandMask), _VP, _VP, C.POINTER(PermDesc), C.POINTER(AttnLayout), _VP]),
    "svg_band_width_update": (C.c_int, [_VP, _VP, _VP, _I32, _I32, _I32, _F32, _F32, _F32, _F32, _I32, _I32, _I32, _VP, _VP, _VP, _VP]),
}

# include/svg_attn_band_per_head_queue.h: the two attention entries above as resident workgroups on the work queue — the arguments of their
# static siblings — and the host statement of the order, in a table of its own (tests/test_band_per_head_queue_cpu.py; the wrappers of
# svg/_adaptive_band.py take them with work_queue=True).  Named ..._ENTRIES for the reason given above.
ADAPTIVE_BAND_QUEUE_ENTRIES = {
    "svg_band_attention_per_head_queue_lse": ADAPTIVE_BAND_ENTRIES["svg_band_attention_per_head_lse"],
    "svg_band_attention_switch_per_head_queue_lse": ADAPTIVE_BAND_ENTRIES["svg_band_attention_switch_per_head_lse"],
    "svg_band_per_head_queue_order": (_I32, [_I32, _I32, C.POINTER(BandMask), C.POINTER(BandMask), _I32, _VP, _VP, _I32]),
}


# include/svg_attn_kmeans_stepped.h: the Lloyd loop of svg_kmeans_loop_grouped in steps — iterate hands the group maxima out, commit takes
# them back —, in a table of its own for the same reason (tests/test_kmeans_stepped_cpu.py; bindings on the caller's buffers:
# kmeans_stepped_* below; the allocating side: svg/_kmeans_stepped.py KmeansSteppedSide)
KMEANS_STEPPED_SIGNATURES = {
    "svg_kmeans_stepped_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    "svg_kmeans_stepped_iterate": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _I32, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "svg_kmeans_stepped_commit": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _F32, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "svg_kmeans_stepped_finish": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
}


# include/svg_attn_kmeans_e4m3.h: the centre, the e4m3 assignment and the Lloyd loop whose first iterations use it, in a table of its own
# for the same reason (tests/test_kmeans_e4m3_cpu.py; the allocating wrappers kmeans_centre, kmeans_assign_e4m3, kmeans_loop_e4m3: svg/_kmeans_e4m3.py,
# reachable as attributes of this module — __getattr__ at its end)
KMEANS_E4M3_SIGNATURES = {
    "svg_kmeans_centre": (C.c_int, [_VP, _VP, _I32, _I32, _I32, _I32, _VP]),
    "svg_kmeans_assign_e4m3_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32]),
    "svg_kmeans_assign_e4m3": (C.c_int, [_VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP, _SZ, _VP]),
    "svg_kmeans_loop_e4m3_workspace_bytes": (_SZ, [_I32, _I32, _I32, _I32, _I32]),
    "svg_kmeans_loop_e4m3": (C.c_int, [_VP, _I64, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F32, _I32,
                                       _VP, _SZ, _VP]),
}


# include/svg_attn_centroid_tail.h: the cluster means and the attention state over the key clusters a block map leaves out, in a table of its
# own for the same reason (tests/test_centroid_tail_cpu.py; the allocating wrappers cluster_means, centroid_tail_attention:
# svg/_centroid_tail.py, reachable as attributes of this module — __getattr__ at its end; named ..._ENTRIES for the reason ADAPTIVE_BAND_ENTRIES
# gives: the golden of tests/test_wrapper_layout_plan_cpu.py is closed; what these wrappers pass is checked on the GPU, in
# tests/test_gpu_centroid_tail.py)
CENTROID_TAIL_ENTRIES = {
    "svg_cluster_means": (C.c_int, [_VP, C.POINTER(TensorStrides), _I32, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _VP]),
    "svg_centroid_tail_workspace_bytes": (_SZ, [_I32, _I32, _I32]),
    "svg_centroid_tail_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _I32, _F32, _VP, _I32, _VP, _VP, _I32, _VP,
                                                  _VP, _SZ, C.POINTER(AttnLayout), _VP]),
}


class CopyBox(C.Structure):
    """svg_copy_box_t (include/svg_attn_shard_exchange.h): extent[0] * extent[1] * extent[2] rows of D contiguous elements; offsets and
    strides in elements"""

    _fields_ = [("src_offset", C.c_int64), ("dst_offset", C.c_int64), ("extent", C.c_int32 * 3), ("reserved", C.c_int32),
                ("src_stride", C.c_int64 * 3), ("dst_stride", C.c_int64 * 3)]


class CopyTensor(C.Structure):
    """svg_copy_tensor_t: the two base pointers of one tensor of a launch and the boxes [box_begin, box_begin + box_count) it copies"""

    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("box_begin", C.c_int32), ("box_count", C.c_int32)]


# include/svg_attn_shard_exchange.h: the pack / unpack layouts of the token-shard exchanges as one batched strided copy, in a table of its
# own for the same reason (tests/test_token_shards_cpu.py)
SHARD_EXCHANGE_SIGNATURES = {
    "svg_copy_boxes": (C.c_int, [C.POINTER(CopyTensor), _I32, C.POINTER(CopyBox), _I32, _I32, _I32, _VP]),
}


def lib_path() -> Path:
    return Path(os.environ.get("SVG_ATTN_LIB", str(_LIB_PATH)))


def load(strict: bool = True) -> Optional[C.CDLL]:
    """dlopen the library once and type every entry point.  strict=False returns None instead of raising."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    p = lib_path()
    try:
        lib = C.CDLL(str(p))
        for name, (res, args) in {**SIGNATURES, **SPARSE_LSE_SIGNATURES, **SPARSE_F32_SIGNATURES, **BAND_LSE_FORM_SIGNATURES,
                                   **BAND_WINDOW_SIGNATURES, **BAND_SHARD_SIGNATURES, **BAND_SHARD_SWITCH_SIGNATURES,
                                   **PROFILE_SHARD_SIGNATURES, **SAMPLE_ROWS_SIGNATURES, **SHARD_EXCHANGE_SIGNATURES,
                                   **ADAPTIVE_TOP_P_SIGNATURES, **ADAPTIVE_BAND_ENTRIES, **ADAPTIVE_BAND_QUEUE_ENTRIES,
                                   **KMEANS_STEPPED_SIGNATURES, **KMEANS_E4M3_SIGNATURES, **CENTROID_TAIL_ENTRIES}.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        got = int(lib.svg_abi_version())
        if got != SVG_ABI_VERSION:   # a library built from another revision of include/svg_attn.h: its entry points may take other arguments
            raise OSError(f"ABI version {got}, this binding was written against {SVG_ABI_VERSION} (rebuild: python sparse-videogen_amd/build.py)")
        _lib = lib
    except (OSError, AttributeError) as e:  # missing .so, missing symbol or ABI mismatch
        _load_error = f"{p}: {e}"
        if strict:
            raise RuntimeError(
                f"libsvgattn.so could not be loaded ({_load_error}). Build it with "
                f"`python sparse-videogen_amd/build.py` (hipcc, gfx950). There is no CPU fallback."
            ) from e
        return None
    return _lib


def available() -> bool:
    return load(strict=False) is not None


def build_info() -> str:
    return load().svg_build_info().decode()


def _check(rc: int, what: str) -> None:
    if rc != 0:
        lib = load()
        msg = lib.svg_strerror(rc).decode()
        raise RuntimeError(f"{what} failed: {msg} (code {rc}, hipError {lib.svg_last_hip_error()})")


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return SVG_DTYPE_BF16
    if t.dtype == torch.float16:
        return SVG_DTYPE_F16
    raise RuntimeError(f"libsvgattn supports bfloat16 / float16 tensors, got {t.dtype}")


def _dev(*ts: torch.Tensor) -> None:
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("libsvgattn ops need GPU (HIP) tensors; there is no CPU fallback for the sparse path")
        if not t.is_contiguous():
            raise RuntimeError("libsvgattn ops need contiguous tensors")


def _gpu(*ts: Optional[torch.Tensor]) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("libsvgattn ops need GPU (HIP) tensors; there is no CPU fallback for the sparse path")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------
# strided attention tensors (svg_attn_layout_t): q / k / v read where a projection wrote them, o written where the output projection
# reads it — the reference's processors hand flex_attention / flash-attn `proj(x).unflatten(2, (H, -1)).transpose(1, 2)` VIEWS and
# copy what those cannot take (wan/attention.py:123-125,168-170)
# ------------------------------------------------------------------------------------------------------
def _view4(t: torch.Tensor) -> torch.Tensor:
    """[B, H, S, D] view of a [B, H, S, D] or [BH, S, D] tensor (no copy)."""
    return t if t.dim() == 4 else t.unsqueeze(0)


def _strided_ok(t4: torch.Tensor, dma: bool = False) -> bool:
    """Can a *_strided entry point read / write this [B, H, S, D] view in place?  (layout_from_abi, csrc/svg_common.h)"""
    B, H, S, D = t4.shape
    st = t4.stride()
    if st[3] != 1 or t4.data_ptr() % 16 != 0 or st[2] < D or st[2] >= (1 << 23):
        return False
    if any(x % 8 != 0 or x < 0 for x in st[:3]):
        return False
    return (not dma) or S * st[2] * 2 < (1 << 32)   # k / v: 32-bit byte offsets per head in the LDS-DMA requests


def attn_layout(q4: torch.Tensor, k4: torch.Tensor, v4: torch.Tensor, o4: torch.Tensor) -> AttnLayout:
    ts = [TensorStrides(t.stride(0), t.stride(1), t.stride(2)) for t in (q4, k4, v4, o4)]
    return AttnLayout(q4.shape[1], k4.shape[1], *ts)


def token_major_empty(like4: torch.Tensor, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """An uninitialised [B, H, S, D] tensor (of like4's dtype, or `dtype`) stored token-major ([B, S, H, D] in memory):
    `out.transpose(1, 2).flatten(2, 3)` — what every processor of the reference does with the attention output before the output
    projection — is then a view, not a copy."""
    B, H, S, D = like4.shape
    return empty((B, S, H, D), dtype=dtype or like4.dtype, device=like4.device).permute(0, 2, 1, 3)


def strided_attention_supported(q: torch.Tensor, variant: int = 0) -> bool:
    """The *_strided entry points exist for the default schedules (the two-phase bodies: 16x16x32 at head_dim 128, 32x32x16 at 64)."""
    return q.shape[-1] in (64, 128) and variant == 0 and q.dtype in (torch.bfloat16, torch.float16)


class _LayoutPlan:
    """What _layout_plan decided: the tensors to launch on (q, k, v, k_b, v_b: the caller's or contiguous copies), the output to launch
    on (o: the caller's `out`, a new tensor or a stand-in; None for a plan of inputs only), the layout arguments (lay, lay_b: NULL or a
    reference to an AttnLayout) and the caller's `out`."""

    __slots__ = ("q", "k", "v", "k_b", "v_b", "o", "lay", "lay_b", "out")

    def result(self) -> torch.Tensor:
        """The wrapper's o: the new tensor, or the caller's `out` — after the copy-back where the launch wrote a stand-in."""
        if self.out is None:
            return self.o
        if self.o is not self.out:
            self.out.copy_(self.o)
        return self.out


_O16, _O32, _NO_O = "16-bit", "fp32 rows", "inputs only"


def _layout_plan(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_b: Optional[torch.Tensor] = None, v_b: Optional[torch.Tensor] = None, *,
                 o: str = _O16, out: Optional[torch.Tensor] = None, token_major_out: bool = False, o_dtype: Optional[torch.dtype] = None,
                 null_layout: bool = True, views: bool = True, views_on_copies: bool = True, inputs_as_given: bool = False,
                 zero_o: bool = False) -> _LayoutPlan:
    """Where one attention launch reads q / k / v and writes o — decided from shapes, strides and alignment, before anything is called.

    The fall-back of every attention wrapper: tensors are read and written where they lie — without a layout when everything is
    contiguous (null_layout: the entry takes NULL then; an entry whose strided form has another name is picked by `plan.lay is None`),
    through an AttnLayout over [B, H, S, D] views where _strided_ok describes every one of them.  What it cannot describe is copied,
    as the reference copies what its kernels cannot take: first q, k, v (all of them), and an `out` it still cannot write gets a
    stand-in — the output a call without `out` would make — that plan.result() copies back.

    q and k / v may have different row counts (window, shard, cross); k_b, v_b: the second key set of the pair entry, with its own
    strides (lay_b) and its own describability.  The same tensor passed twice is copied once (a K-only probe plans q, k, k).
    o: _O16 — `out`, or a new tensor of q's shape and dtype (o_dtype), token-major when token_major_out and a layout can say so;
       _O32 — fp32 rows: always new and contiguous, the layout's o member takes q's strides;
       _NO_O — inputs only (the profilers, the probes).
    views: may this call take a layout at all (the schedule, q_prescaled, completion counters, groups that split a video's heads,
    block-rows too small, fp8, a dtype without a strided form)?  Without, a token-major output cannot be made either.
    views_on_copies=False: the entries with a `_strided` twin take views of the caller's own tensors only — once anything was copied
    they run their plain form, a new output is head-major whatever token_major_out says and a non-contiguous `out` gets a stand-in.
    inputs_as_given: q, k, v are neither examined nor copied (merge: its parts are the caller's contract), their strides still fill
    the layout.  zero_o: zero-fill the tensor the launch writes (rows a kernel may leave out), once."""
    ins = (q, k, v) if k_b is None else (q, k, v, k_b, v_b)
    p = _LayoutPlan()
    p.out, p.lay, p.lay_b = out, None, None
    p.o = empty(q.shape, dtype=torch.float32, device=q.device) if o is _O32 else None
    dst, with_views = out, views
    for attempt in ("as they lie", "inputs copied", "and a stand-in for out"):
        if attempt == "inputs copied":
            with_views = views and views_on_copies
            if not inputs_as_given:
                copies = {}
                for t in ins:
                    if id(t) not in copies:
                        copies[id(t)] = t.contiguous()
                ins = tuple([copies[id(t)] for t in ins])
        elif attempt == "and a stand-in for out":
            if out is None:
                continue
            dst = None
        if null_layout and (inputs_as_given or not [t for t in ins if not t.is_contiguous()]) and (
                o is not _O16 or (dst.is_contiguous() if dst is not None else not (token_major_out and with_views))):
            if o is _O16:   # (everything contiguous: the entry takes no layout)
                p.o = dst if dst is not None else (empty_like(ins[0]) if o_dtype is None else empty_like(ins[0], dtype=o_dtype))
            break
        if not with_views:
            continue
        q4, *kv4 = [_view4(t) for t in ins]
        if not (inputs_as_given or (_strided_ok(q4) and not [t for t in kv4 if not _strided_ok(t, True)])):
            continue
        if o is not _O16:
            o4 = q4
        elif dst is not None:
            o4 = _view4(dst)
        elif token_major_out:
            o4 = token_major_empty(q4, o_dtype)
        else:
            o4 = empty_like(q4, dtype=o_dtype, memory_format=torch.contiguous_format)
        if _strided_ok(o4) and o4.shape == q4.shape:
            if o is _O16:
                p.o = dst if dst is not None else (o4 if q.dim() == 4 else o4.squeeze(0))
            p.lay = C.byref(attn_layout(q4, kv4[0], kv4[1], o4))
            if k_b is not None:   # (its k / v strides are what the entry reads)
                p.lay_b = C.byref(attn_layout(q4, kv4[2], kv4[3], o4))
            break
    else:
        raise RuntimeError("libsvgattn: contiguous copies of q / k / v that the attention layout still cannot describe (16-byte alignment, "
                           "row stride below 2^23 elements, k / v of less than 4 GiB per head)")
    p.q, p.k, p.v = ins[:3]
    p.k_b, p.v_b = ins[3:] if k_b is not None else (None, None)
    if zero_o:
        p.o.zero_()
    return p


def _sm_scale(sm_scale: Optional[float], D: int) -> float:
    return float(sm_scale) if sm_scale is not None else 1.0 / (D ** 0.5)


def _perm_arg(head_perm_flag: Optional[torch.Tensor], BH: int, vid0: int, num_frame: int, frame_size: int):
    """The svg_perm_desc_t argument of the fused head placement (None without flags); it keeps its int64 flag tensor alive."""
    if head_perm_flag is None:
        return None
    flag = head_perm_flag.to(torch.int64).contiguous()
    assert flag.numel() == BH
    perm = PermDesc(flag.data_ptr(), vid0, num_frame, frame_size)
    perm.flag = flag
    return C.byref(perm)


# ------------------------------------------------------------------------------------------------------
# typed wrappers (torch tensors in, torch tensors out)
# ------------------------------------------------------------------------------------------------------
def head_placement(srcs: Sequence[torch.Tensor], dsts: Sequence[torch.Tensor], best_mask_idx: torch.Tensor,
                   context_length: int, num_frame: int, frame_size: int, text_first: bool, inverse: bool) -> None:
    lib = load()
    n = len(srcs)
    assert 1 <= n <= 3 and len(dsts) == n
    _dev(*srcs, *dsts, best_mask_idx)
    x = srcs[0]
    BH = x.shape[0] * x.shape[1]
    S, D = x.shape[2], x.shape[3]
    for t in list(srcs) + list(dsts):
        assert t.shape == x.shape and t.dtype == x.dtype
    best = best_mask_idx.to(torch.int64).contiguous()
    assert best.numel() == BH
    sp = (C.c_void_p * 3)(*[s.data_ptr() for s in srcs], *([None] * (3 - n)))
    dp = (C.c_void_p * 3)(*[d.data_ptr() for d in dsts], *([None] * (3 - n)))
    rc = lib.svg_head_placement(C.cast(sp, _VP), C.cast(dp, _VP), n, best.data_ptr(), BH, S, D, _dtype_code(x),
                                context_length, num_frame, frame_size, int(text_first), int(inverse), _stream())
    _check(rc, "svg_head_placement")


def permute_rows(x: torch.Tensor, idx: torch.Tensor, inverse: bool = False) -> torch.Tensor:
    lib = load()
    _dev(x, idx)
    BH, S, D = x.shape
    assert idx.dtype == torch.int32 and idx.shape == (BH, S)
    y = empty_like(x)
    fn = lib.svg_inverse_permute_rows if inverse else lib.svg_permute_rows
    _check(fn(x.data_ptr(), idx.data_ptr(), y.data_ptr(), BH, S, D, _dtype_code(x), _stream()), "svg_permute_rows")
    return y


def argsort_labels(labels: torch.Tensor, K: int):
    """labels int32 [B, N] in [0, K) -> (sorted_idx int32 [B, N] (stable), counts int32 [B, K])"""
    lib = load()
    _dev(labels)
    assert labels.dtype == torch.int32 and labels.dim() == 2
    B, N = labels.shape
    ws = empty(lib.svg_argsort_workspace_bytes(B, N, K), dtype=torch.uint8, device=labels.device)
    sidx = empty((B, N), dtype=torch.int32, device=labels.device)
    counts = empty((B, K), dtype=torch.int32, device=labels.device)
    rc = lib.svg_argsort_labels(labels.data_ptr(), sidx.data_ptr(), counts.data_ptr(), B, N, K, ws.data_ptr(),
                                ws.numel(), _stream())
    _check(rc, "svg_argsort_labels")
    return sidx, counts


def _want_f32_parts(what: str, out_dtype, return_lse: bool, out, token_major_out: bool) -> bool:
    """out_dtype of the attention wrappers: None (q's dtype), or torch.float32 — the rows before their rounding, parts for
    merge_attention_states — which goes with return_lse=True and without out / token_major_out only."""
    if out_dtype is None:
        return False
    if out_dtype != torch.float32:
        raise ValueError(f"{what}: out_dtype is None (q's dtype) or torch.float32, got {out_dtype}")
    if not return_lse or out is not None or token_major_out:
        raise ValueError(f"{what}(out_dtype=torch.float32): fp32 rows are parts for merge_attention_states — with return_lse=True and without "
                         f"out / token_major_out; got return_lse = {return_lse}, out = {out is not None}, token_major_out = {token_major_out}")
    return True


def band_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: BandMask, sm_scale: Optional[float] = None,
                   head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0, num_frame: int = 1,
                   frame_size: int = 1, variant: int = 0, out: Optional[torch.Tensor] = None,
                   done: Optional[torch.Tensor] = None, done_nseg: int = 1, q_prescaled: bool = False,
                   token_major_out: bool = False, return_lse: bool = False, out_dtype: Optional[torch.dtype] = None):
    """q, k, v: [B, H, S, D] (or [BH, S, D]) bf16/fp16 GPU tensors -> o of the same shape.
    Strided views (last dimension contiguous — e.g. `proj(x).unflatten(2, (H, -1)).transpose(1, 2)`, or a slice of a fused QKV
    projection) are read in place by svg_band_attention_strided where it exists (head_dim 128, default schedule, plain q, no completion
    counters); layouts and copies: _layout_plan.  token_major_out: the result is a [B, H, S, D] tensor stored [B, S, H, D]
    (token_major_empty), so the processors' `.transpose(1, 2).flatten(2, 3)` is a view.
    q_prescaled: q already carries sm_scale * log2(e) (SOFTMAX_Q_SCALE(D) for the default scale; what qk_norm_rope*(q_scale=...)
    writes): svg_band_attention_prescaled, default schedule only.
    done: int32 [BH * (done_nseg + 1)] zeroed completion counters (svg_band_attention_notify[_seg]; see band_notify_target /
    band_notify_layout / wait_counters / notify_counters): counter (h, s) at done[h * done_nseg + s], the last BH words are scratch
    of the library (hidden per-head counters of heads that run with the fused layout permutation).
    return_lse: (o, lse) with lse the row log-sum-exp of the scaled scores over the keys the mask gives the row (natural log), contiguous
    fp32 of shape q.shape[:-1], in the caller's row order — what merge_attention_states takes (svg_band_attention_lse: head_dim 128,
    default schedule, plain q, no completion counters; anything else raises ValueError); o has the same bits as without.
    out_dtype=torch.float32 (with return_lse=True, without out / token_major_out; ValueError otherwise): (o32, lse) with o32 the rows
    before their rounding, contiguous fp32 of q's shape (svg_band_attention_lse_f32) — parts for merge_attention_states, which then rounds
    once; o32.to(q.dtype) is the o of return_lse=True."""
    f32 = _want_f32_parts("band_attention", out_dtype, return_lse, out, token_major_out)
    if return_lse:
        if variant != 0 or done is not None or q_prescaled or q.shape[-1] != 128:
            raise ValueError("band_attention(return_lse=True): head_dim 128 on the default schedule (variant 0) with a plain q and no "
                             f"completion counters; got D = {q.shape[-1]}, variant = {variant}, done = {done is not None}, "
                             f"q_prescaled = {q_prescaled}")
        return _band_attention_lse(q, k, v, mask, sm_scale, head_perm_flag, vid0, num_frame, frame_size, out, token_major_out, f32)
    return _band_attention(q, k, v, mask, None, None, sm_scale, head_perm_flag, vid0, num_frame, frame_size, variant, out, done, done_nseg,
                           q_prescaled, token_major_out)


def _call_lse(name: str, f32: bool, p, lse: torch.Tensor, *geom) -> None:
    """The launch of LSE entry `name` (f32: of its *_f32 form) on layout plan p: the five pointers, the entry's own arguments `geom`, the
    layout, the stream; a failure raises under the entry's name.  Allocates nothing: lse is the caller's.  For the window, shard and per-head
    wrappers; band_attention, band_attention_switch and band_attention_groups spell their calls out, which the call-site walks of
    tests/test_sparse_attention_lse_cpu.py, test_attention_f32_parts_cpu.py and test_band_lse_forms_cpu.py read."""
    if f32:
        name += "_f32"
    _check(getattr(load(), name)(p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), p.o.data_ptr(), lse.data_ptr(), *geom, p.lay, _stream()), name)


def _band_attention_lse(q, k, v, mask, sm_scale, head_perm_flag, vid0, num_frame, frame_size, out, token_major_out, f32=False):
    """band_attention(return_lse=True): svg_band_attention_lse (f32: svg_band_attention_lse_f32), never the entry without lse.  Layouts
    and copies: _layout_plan."""
    lib = load()
    _dev(head_perm_flag)
    _gpu(q, k, v, out)
    assert q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype
    S, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (S * D)
    scale = _sm_scale(sm_scale, D)
    perm = _perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
    lse = empty(q.shape[:-1], dtype=torch.float32, device=q.device)   # (contiguous [BH, S] whatever the layout of q / o)
    p = _layout_plan(q, k, v, o=_O32 if f32 else _O16, out=out, token_major_out=token_major_out)
    if f32:
        _check(lib.svg_band_attention_lse_f32(p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), p.o.data_ptr(), lse.data_ptr(), BH, S, D,
                                              _dtype_code(q), scale, C.byref(mask), perm, p.lay, _stream()), "svg_band_attention_lse_f32")
    else:
        _check(lib.svg_band_attention_lse(p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), p.o.data_ptr(), lse.data_ptr(), BH, S, D,
                                          _dtype_code(q), scale, C.byref(mask), perm, p.lay, _stream()), "svg_band_attention_lse")
    return p.result(), lse


def _band_form_checks(what, q, k, v, out, q_prescaled, return_lse, out_dtype, token_major_out) -> bool:
    """return_lse / out_dtype of band_attention_switch and band_attention_groups, before anything is loaded: -> fp32 rows?"""
    f32 = _want_f32_parts(what, out_dtype, return_lse, out, token_major_out)
    if return_lse and (q_prescaled or q.shape[-1] != 128):
        raise ValueError(f"{what}(return_lse=True): head_dim 128 with a plain q; got D = {q.shape[-1]}, q_prescaled = {q_prescaled}")
    return f32


def _band_attention(q, k, v, mask, alt_mask, use_alt_flag, sm_scale, head_perm_flag, vid0, num_frame, frame_size, variant, out, done,
                    done_nseg, q_prescaled, token_major_out):
    """band_attention, and band_attention_switch when use_alt_flag is given"""
    lib = load()
    _dev(head_perm_flag)
    _gpu(q, k, v, out)
    assert q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype
    S, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (S * D)
    scale = _sm_scale(sm_scale, D)
    perm = _perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
    switch = use_alt_flag is not None
    if done is not None:
        _dev(done)
        assert done.dtype == torch.int32 and done.is_contiguous() and variant == 0
    if q_prescaled:
        assert variant == 0 and sm_scale is None, "q_prescaled: default-schedule call, the scale lives in q"
    p = _layout_plan(q, k, v, out=out, token_major_out=token_major_out, views_on_copies=False,
                     views=done is None and not q_prescaled and strided_attention_supported(q, variant))
    q, k, v, o = p.q, p.k, p.v, p.o
    if p.lay is not None and switch:
        rc = lib.svg_band_attention_switch_strided(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q), scale,
                                                   C.byref(mask), perm, C.byref(alt_mask), use_alt_flag.data_ptr(), p.lay, _stream())
        _check(rc, "svg_band_attention_switch_strided")
    elif p.lay is not None:
        rc = lib.svg_band_attention_strided(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q), scale,
                                            C.byref(mask), perm, p.lay, _stream())
        _check(rc, "svg_band_attention_strided")
    elif switch and q_prescaled:
        rc = lib.svg_band_attention_switch_prescaled(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q),
                                                     C.byref(mask), perm, C.byref(alt_mask), use_alt_flag.data_ptr(), _stream())
        _check(rc, "svg_band_attention_switch_prescaled")
    elif switch:
        rc = lib.svg_band_attention_switch(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q), scale,
                                           C.byref(mask), perm, C.byref(alt_mask), use_alt_flag.data_ptr(), _stream())
        _check(rc, "svg_band_attention_switch")
    elif q_prescaled and done is not None:
        rc = lib.svg_band_attention_prescaled_notify_seg(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D,
                                                         _dtype_code(q), C.byref(mask), perm, done.data_ptr(), int(done.numel()),
                                                         int(done_nseg), _stream())
        _check(rc, "svg_band_attention_prescaled_notify_seg")
    elif q_prescaled:
        rc = lib.svg_band_attention_prescaled(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q),
                                              C.byref(mask), perm, _stream())
        _check(rc, "svg_band_attention_prescaled")
    elif done is not None:
        rc = lib.svg_band_attention_notify_seg(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q),
                                               scale, C.byref(mask), perm, done.data_ptr(), int(done.numel()), int(done_nseg),
                                               _stream())   # too small: SVG_ERR_WORKSPACE
        _check(rc, "svg_band_attention_notify_seg")
    else:
        rc = lib.svg_band_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q), scale,
                                    C.byref(mask), perm, variant, _stream())
        _check(rc, "svg_band_attention")
    return p.result()


def softmax_q_scale(D: int, sm_scale: Optional[float] = None) -> float:
    """The factor a pre-scaled q carries: sm_scale * log2(e) (default sm_scale = 1 / sqrt(D))."""
    return _sm_scale(sm_scale, D) * 1.4426950408889634


class WorkspaceCache:
    """Scratch tensors the wrappers keep between calls, keyed by (shape..., device, stream): two calls of one shape on different
    streams never share a buffer, and at most `capacity` entries stay alive (least recently used goes first), so transient streams
    cannot pile up multi-GB workspaces.  One policy for the fp8 workspaces and the k-means loop scratch."""

    def __init__(self, capacity: int = 8):
        from collections import OrderedDict

        self.capacity, self._d = capacity, OrderedDict()

    @staticmethod
    def key(*shape, device):
        return tuple(shape) + (device, _stream())

    def get(self, key):
        v = self._d.get(key)
        if v is not None:
            self._d.move_to_end(key)
        return v

    def __setitem__(self, key, value):
        self._d[key] = value
        self._d.move_to_end(key)
        while len(self._d) > self.capacity:
            self._d.popitem(last=False)

    def __len__(self):
        return len(self._d)

    def clear(self):
        self._d.clear()


_F8_WS = WorkspaceCache()
_KMEANS_WS = WorkspaceCache()


def band_attention_fp8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: BandMask, sm_scale: Optional[float] = None,
                       head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0, num_frame: int = 1, frame_size: int = 1,
                       out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None, stage: int = 0) -> torch.Tensor:
    """band_attention with e4m3 QK^T / PV (svg_band_attention_fp8; D = 128).  Same arguments and output as band_attention; the
    quantise + placement pre-pass runs inside the call.  workspace: uint8 GPU tensor of band_attention_fp8_workspace_bytes(...)
    bytes, cached per (BH, S, device) when omitted.  stage 1 / 2: only the pre-pass / only the attention kernel on the workspace
    a stage-1 call has filled (svg_band_attention_fp8_stage)."""
    lib = load()
    _dev(q, k, v, head_perm_flag)
    assert q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype
    S, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (S * D)
    o = empty_like(q) if out is None else out
    _dev(o)
    scale = _sm_scale(sm_scale, D)
    perm = _perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
    need = int(lib.svg_band_attention_fp8_workspace_bytes(BH, S, D))
    if need == 0:
        raise RuntimeError(f"svg_band_attention_fp8: unsupported shape (D = {D}; only 128)")
    if workspace is None:
        key = WorkspaceCache.key("band", BH, S, device=q.device)
        workspace = _F8_WS.get(key)
        if workspace is None or workspace.numel() < need:
            workspace = _F8_WS[key] = empty(need, dtype=torch.uint8, device=q.device)
    _dev(workspace)
    assert workspace.dtype == torch.uint8 and workspace.numel() >= need
    args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, S, D, _dtype_code(q), scale, C.byref(mask), perm,
            workspace.data_ptr(), workspace.numel())
    if stage:
        _check(lib.svg_band_attention_fp8_stage(*args, int(stage), _stream()), "svg_band_attention_fp8_stage")
    else:
        _check(lib.svg_band_attention_fp8(*args, _stream()), "svg_band_attention_fp8")
    return o


def notify_counters(BH: int, nseg: int, device) -> torch.Tensor:
    """Zeroed counter buffer for band_attention(done=...): BH * nseg segment counters + BH words of library scratch."""
    return torch.zeros(BH * (nseg + 1), device=device, dtype=torch.int32)


def band_notify_target(S: int, mask: BandMask) -> int:
    """Value a head's completion counter reaches when the head is done (svg_band_attention_notify_target)."""
    t = load().svg_band_attention_notify_target(int(S), C.byref(mask))
    assert t > 0
    return int(t)


def band_replays(reset: bool = False) -> int:
    """q-tiles the bf16 band kernels at head_dim 128 computed a second time because the validation of their sums failed
    (svg_debug_band_replays): synchronises the current device; reset=True zeroes the counter after reading."""
    n = int(load().svg_debug_band_replays(1 if reset else 0))
    if n < 0:
        raise RuntimeError("svg_debug_band_replays failed")
    return n


def band_notify_layout(S: int, mask: BandMask, nseg: int):
    """(n, row_bounds [n + 1], targets [n]) of the per-segment completion counters (svg_band_attention_notify_layout):
    counter (h, s) >= targets[s]  =>  the physical rows [row_bounds[s], row_bounds[s + 1]) of head h are complete and visible
    (heads with the fused layout permutation release all their segments together, see include/svg_attn.h); n <= nseg."""
    rb = (C.c_int32 * (nseg + 1))()
    tg = (C.c_int32 * nseg)()
    n = load().svg_band_attention_notify_layout(int(S), C.byref(mask), int(nseg), C.cast(rb, C.c_void_p), C.cast(tg, C.c_void_p))
    assert n > 0
    return n, list(rb)[: n + 1], list(tg)[:n]


def wait_counters(counters: torch.Tensor, target: int, timeout_ms: int = 0, timed_out: Optional[torch.Tensor] = None) -> None:
    """Enqueue, on the current stream, a one-wave kernel that returns once every element of `counters` (int32, GPU) >= target.
    timeout_ms > 0: the kernel gives up after that time and stores 1 to `timed_out` (int32 [1], GPU) — it cannot hang the stream;
    the caller reads the flag before trusting what was queued behind the waiter."""
    _dev(counters)
    assert counters.dtype == torch.int32 and counters.is_contiguous()
    if timeout_ms > 0:
        assert timed_out is not None, "wait_counters(timeout_ms > 0) needs a `timed_out` flag tensor (int32 [1] on the GPU)"
        _dev(timed_out)
        assert timed_out.dtype == torch.int32 and timed_out.numel() >= 1
        _check(load().svg_wait_counters_deadline(counters.data_ptr(), counters.numel(), int(target), int(timeout_ms),
                                                 timed_out.data_ptr(), _stream()), "svg_wait_counters_deadline")
        return
    _check(load().svg_wait_counters(counters.data_ptr(), counters.numel(), int(target), _stream()), "svg_wait_counters")


def band_attention_switch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: BandMask, alt_mask: BandMask,
                          use_alt_flag: torch.Tensor, sm_scale: Optional[float] = None,
                          head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0, num_frame: int = 1, frame_size: int = 1,
                          out: Optional[torch.Tensor] = None, q_prescaled: bool = False, token_major_out: bool = False,
                          return_lse: bool = False, out_dtype: Optional[torch.dtype] = None):
    """band_attention with a device-side switch: `use_alt_flag` (int32 [1] on the GPU) != 0 selects `alt_mask` without the head
    placement, otherwise `mask` with it (svg_band_attention_switch) — no host read of the flag.
    q_prescaled: q carries sm_scale * log2(e) (svg_band_attention_switch_prescaled, D = 128).
    Strided views / token_major_out: as band_attention (svg_band_attention_switch_strided: head_dim 128, plain q).
    return_lse / out_dtype=torch.float32: (o, lse) / (o32, lse) as in band_attention, lse under the mask the flag selects and in the row
    order that mask runs in (svg_band_attention_switch_lse[_f32]: head_dim 128, plain q; anything else raises ValueError); o has the
    same bits as without."""
    f32 = _band_form_checks("band_attention_switch", q, k, v, out, q_prescaled, return_lse, out_dtype, token_major_out)
    _dev(use_alt_flag)
    assert use_alt_flag.dtype == torch.int32 and use_alt_flag.numel() >= 1
    if return_lse:
        lib = load()
        _dev(head_perm_flag)
        _gpu(q, k, v, out)
        assert q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype
        S, D = q.shape[-2], q.shape[-1]
        BH = q.numel() // (S * D)
        perm = _perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
        args = (BH, S, D, _dtype_code(q), _sm_scale(sm_scale, D), C.byref(mask), perm, C.byref(alt_mask), use_alt_flag.data_ptr())
        lse = empty(q.shape[:-1], dtype=torch.float32, device=q.device)   # (contiguous [BH, S] whatever the layout of q / o)
        p = _layout_plan(q, k, v, o=_O32 if f32 else _O16, out=out, token_major_out=token_major_out)
        ptrs = (p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), p.o.data_ptr(), lse.data_ptr())
        if f32:
            _check(lib.svg_band_attention_switch_lse_f32(*ptrs, *args, p.lay, _stream()), "svg_band_attention_switch_lse_f32")
        else:
            _check(lib.svg_band_attention_switch_lse(*ptrs, *args, p.lay, _stream()), "svg_band_attention_switch_lse")
        return p.result(), lse
    return _band_attention(q, k, v, mask, alt_mask, use_alt_flag, sm_scale, head_perm_flag, vid0, num_frame, frame_size, 0, out, None, 1,
                           q_prescaled, token_major_out)


def band_attention_groups(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, masks: Sequence[BandMask], group_heads: Sequence[int],
                          alt_masks: Optional[Sequence[BandMask]] = None, use_alt_flag: Optional[torch.Tensor] = None,
                          head_perm_flag: Optional[torch.Tensor] = None, vid0: int = 0, num_frame: int = 1, frame_size: int = 1,
                          out: Optional[torch.Tensor] = None, q_prescaled: bool = False, token_major_out: bool = False,
                          return_lse: bool = False, out_dtype: Optional[torch.dtype] = None):
    """band_attention / band_attention_switch (use_alt_flag given, with alt_masks) over groups of consecutive heads, group g —
    group_heads[g] heads — under masks[g] (alt_masks[g]): svg_band_groups_attention, bit for bit the single-mask call on each group's
    heads.  q, k, v: [B, H, S, D] (or [BH, S, D]), default schedule, default softmax scale.  Strided views, `out` and token_major_out as in
    band_attention: read / written in place where the single-mask strided entry would (plain q, every group a whole number of the H
    heads of a video); layouts and copies: _layout_plan.
    return_lse / out_dtype=torch.float32: (o, lse) / (o32, lse) as in band_attention / band_attention_switch, bit for bit that call on
    each group's heads (svg_band_groups_attention_lse[_f32]: head_dim 128, plain q; anything else raises ValueError)."""
    f32 = _band_form_checks("band_attention_groups", q, k, v, out, q_prescaled, return_lse, out_dtype, token_major_out)
    lib = load()
    _dev(head_perm_flag, use_alt_flag)
    _gpu(q, k, v, out)
    assert q.shape == k.shape == v.shape and q.dtype == k.dtype == v.dtype
    n = len(masks)
    assert n >= 1 and len(group_heads) == n and (alt_masks is None or len(alt_masks) == n)
    assert (alt_masks is None) == (use_alt_flag is None)
    S, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (S * D)
    perm = _perm_arg(head_perm_flag, BH, vid0, num_frame, frame_size)
    marr = (BandMask * n)(*masks)
    aarr = None if alt_masks is None else (BandMask * n)(*alt_masks)
    garr = (_I32 * n)(*[int(g) for g in group_heads])
    flag = _ptr(use_alt_flag)

    H = _view4(q).shape[1]
    whole = all(int(g) % H == 0 for g in group_heads)   # (a layout describes heads per video: no group may split one)
    args = (BH, S, D, _dtype_code(q), _sm_scale(None, D), marr, aarr, garr, n, perm, flag)
    if return_lse:
        lse = empty(q.shape[:-1], dtype=torch.float32, device=q.device)   # (contiguous [BH, S] whatever the layout of q / o)
        p = _layout_plan(q, k, v, o=_O32 if f32 else _O16, out=out, token_major_out=token_major_out, views=whole)
        ptrs = (p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), p.o.data_ptr(), lse.data_ptr())
        if f32:
            _check(lib.svg_band_groups_attention_lse_f32(*ptrs, *args, p.lay, _stream()), "svg_band_groups_attention_lse_f32")
        else:
            _check(lib.svg_band_groups_attention_lse(*ptrs, *args, p.lay, _stream()), "svg_band_groups_attention_lse")
        return p.result(), lse
    p = _layout_plan(q, k, v, out=out, token_major_out=token_major_out, views_on_copies=False,
                     views=not q_prescaled and strided_attention_supported(q) and whole)
    _check(lib.svg_band_groups_attention(p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), p.o.data_ptr(), *args, int(q_prescaled), p.lay,
                                         _stream()), "svg_band_groups_attention")
    return p.result()


def band_window_has_keys(mask: BandMask, num_tokens: int, q_range, k_range) -> bool:
    """Does the band mask over a sequence of num_tokens rows allow ANY (row, key) pair of the rectangle rows [q0, q1) x keys [k0, k1)?
    Host only, closed form (no element is enumerated): the predicate of svg_band_mask_t (include/svg_attn.h) on intervals — what
    svg.distributed.band_exchange_plan asks for every pair of shards."""
    real, band, cf_lo, cf_hi, rf_lo, rf_hi = mask.as_tuple()
    S = int(num_tokens)
    q0, q1 = max(int(q_range[0]), 0), min(int(q_range[1]), S)
    k0, k1 = max(int(k_range[0]), 0), min(int(k_range[1]), S)
    if q1 <= q0 or k1 <= k0:
        return False
    real = min(max(real, 0), S)
    qa, qb, ka, kb = q0, min(q1, real), k0, min(k1, real)      # the real rows and the real keys of the rectangle
    if qb > qa and kb > ka:
        if band > 0 and ka - (qb - 1) < band and qa - (kb - 1) < band:   # the closest pair of the two intervals lies inside the band
            return True
        if min(kb, cf_hi) > max(ka, cf_lo) or min(qb, rf_hi) > max(qa, rf_lo):   # a full column / a full row
            return True
    return q1 > max(q0, real) and k1 > max(k0, real)           # rows behind real_len see the keys behind real_len


def band_window_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: BandMask, num_tokens: int, q_begin: int, k_begin: int,
                          out_dtype: Optional[torch.dtype] = None, out: Optional[torch.Tensor] = None):
    """Band attention of a ROW window over a KEY window of the mask (svg_band_window_attention_lse[_f32]) -> (o, lse): q [cfg, H, Sq, D]
    (or [BH, Sq, D]) holds the rows [q_begin, q_begin + Sq), k / v [cfg, H, Sk, D] the rows [k_begin, k_begin + Sk) of a sequence of
    num_tokens rows, in the LOGICAL order of the mask; row i sees key j where the mask allows (q_begin + i, k_begin + j).  o has q's shape
    and dtype, lse is contiguous fp32 of shape q.shape[:-1] (natural log; a row that sees no key of the window: o = 0, lse = -inf) — parts
    for merge_attention_states: the parts of one row window over disjoint key windows covering the sequence merge to band_attention's
    result.  Layouts and copies: _layout_plan.
    out_dtype=torch.float32 (without out): (o32, lse), the rows before their rounding, contiguous fp32.
    Sq == 0 or Sk == 0 is answered without a launch.  head_dim 128, bf16 / fp16, GPU tensors, k_begin a multiple of 64: anything else
    raises before anything runs — there is no fall-back and no head permutation (token-major heads need their placement first)."""
    if out_dtype not in (None, torch.float32):
        raise ValueError(f"band_window_attention: out_dtype is None (q's dtype) or torch.float32, got {out_dtype}")
    f32 = out_dtype == torch.float32
    if f32 and out is not None:
        raise ValueError("band_window_attention(out_dtype=torch.float32): fp32 rows are parts for merge_attention_states, without out")
    _gpu(q, k, v, out)
    if not (q.dim() == k.dim() == v.dim() and q.dim() in (3, 4) and k.shape == v.shape and q.shape[:-2] == k.shape[:-2]
            and q.shape[-1] == k.shape[-1] and q.dtype == k.dtype == v.dtype):
        raise ValueError(f"band_window_attention: q [.., Sq, D], k / v [.., Sk, D] of one dtype, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    Sq, Sk, D = q.shape[-2], k.shape[-2], q.shape[-1]
    S, q_begin, k_begin = int(num_tokens), int(q_begin), int(k_begin)
    if D != 128 or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"band_window_attention: head_dim 128, bfloat16 / float16; got D = {D}, {q.dtype} (no window form, no fall-back)")
    if k_begin % 64 != 0:
        raise ValueError(f"band_window_attention: k_begin must be a multiple of 64 (key tiles stay aligned to the mask), got {k_begin}")
    if q_begin < 0 or k_begin < 0 or q_begin + Sq > S or k_begin + Sk > S:
        raise ValueError(f"band_window_attention: rows [{q_begin}, {q_begin + Sq}) / keys [{k_begin}, {k_begin + Sk}) outside [0, {S})")
    if out is not None and (out.shape != q.shape or out.dtype != q.dtype):
        raise ValueError(f"band_window_attention: out must have q's shape and dtype, got {tuple(out.shape)} {out.dtype}")
    lse = empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    if Sq == 0 or Sk == 0:   # no row, or no key: nothing to launch
        o = out if out is not None else empty(q.shape, dtype=torch.float32 if f32 else q.dtype, device=q.device)
        o.zero_()
        lse.fill_(float("-inf"))
        return o, lse
    load()
    BH = q.numel() // (Sq * D)
    p = _layout_plan(q, k, v, o=_O32 if f32 else _O16, out=out)
    _call_lse("svg_band_window_attention_lse", f32, p, lse, BH, S, q_begin, Sq, k_begin, Sk, D, _dtype_code(q), _sm_scale(None, D), C.byref(mask))
    return p.result(), lse


# ------------------------------------------------------------------------------------------------------
# frame shards (include/svg_attn_band_shard.h): the coordinate maps on the host, the closed form of "does this pair of shards hold an
# allowed element", and the launch
# ------------------------------------------------------------------------------------------------------
def _shard(s) -> BandShard:
    return s if isinstance(s, BandShard) else BandShard(*[int(x) for x in s])


def _video(perm):
    """(vid0, num_frame, frame_size) of a PermDesc or a 3-tuple"""
    if isinstance(perm, PermDesc):
        return int(perm.vid0), int(perm.num_frame), int(perm.frame_size)
    vid0, F, P = perm
    return int(vid0), int(F), int(P)


def _check_shard(what: str, s: BandShard, S: int, vid0: int, F: int, P: int) -> None:
    if s.f0 < 0 or s.n_frames < 0 or s.f0 + s.n_frames > F or s.n_tail < 0:
        raise ValueError(f"{what}: frames [{s.f0}, {s.f0 + s.n_frames}) / a tail of {s.n_tail} rows outside a video of {F} frames")
    if s.n_tail > 0 and (s.tail_begin < vid0 + F * P or s.tail_begin + s.n_tail > S):
        raise ValueError(f"{what}: tail [{s.tail_begin}, {s.tail_begin + s.n_tail}) outside [{vid0 + F * P}, {S}) (the rows behind the video)")
    if s.n_frames == 0 and s.n_tail == 0:
        raise ValueError(f"{what}: an empty shard")


def band_shard_rows(shard, frame_size: int) -> int:
    """rows a shard holds: frame_size * n_frames + n_tail"""
    s = _shard(shard)
    return int(frame_size) * s.n_frames + s.n_tail


def band_shard_coord(perm, shard, token_major: bool, l: int) -> int:
    """g(l): the mask coordinate of index l of a shard in the order of a head in logical order (token_major False: the shard's rows as
    stored) or of a token-major head (index p * n_frames + fl, stored at row fl * P + p), see include/svg_attn_band_shard.h"""
    vid0, F, P = _video(perm)
    s = _shard(shard)
    nv = P * s.n_frames
    if l >= nv:
        return (s.tail_begin if s.n_tail > 0 else vid0 + F * P) + (l - nv)
    if not token_major:
        return vid0 + s.f0 * P + l
    return vid0 + (l // s.n_frames) * F + s.f0 + l % s.n_frames


def band_shard_coord_inv(perm, shard, token_major: bool, x: int) -> int:
    """ginv(x): the smallest index l of the shard with g(l) >= x, the shard's row count where there is none — closed form, one division by
    the video's frame count.  g increases, so the mask coordinates [a, b) are the shard indices [ginv(a), ginv(b))."""
    vid0, F, P = _video(perm)
    s = _shard(shard)
    nv = P * s.n_frames
    y = max(x - vid0, 0)
    if token_major:
        lv = (y // F) * s.n_frames + min(max(y % F - s.f0, 0), s.n_frames)
    else:
        lv = max(y - s.f0 * P, 0)
    if lv < nv:
        return lv
    return nv + min(max(x - (s.tail_begin if s.n_tail > 0 else vid0 + F * P), 0), s.n_tail)


def band_shard_has_keys(mask: BandMask, num_tokens: int, perm, q_shard, k_shard, token_major: bool) -> bool:
    """Does the band mask over a sequence of num_tokens rows allow ANY pair (row of q_shard, key of k_shard) for a head in logical order
    (token_major False) or a token-major head?  Host only, closed form on intervals of the two coordinate maps — no element is enumerated:
    what svg.distributed.band_shard_exchange_plan asks for every pair of shards.  Exact, except for a token-major head under a mask whose
    real_len lies INSIDE the video (no SVG1 mask: the video rows are real), where the band between the two video parts is judged on
    their hulls — True where in doubt, so a plan never drops a pair that holds an element."""
    vid0, F, P = _video(perm)
    S = int(num_tokens)
    real, band, cf_lo, cf_hi, rf_lo, rf_hi = mask.as_tuple()
    real = min(max(real, 0), S)
    qs, ks = _shard(q_shard), _shard(k_shard)
    kind = bool(token_major)

    def inv(s, x):
        return band_shard_coord_inv((vid0, F, P), s, kind, x)

    def count(s, a, b, lo=0, hi=None):   # indices in [lo, hi) whose coordinate lies in [a, b)
        if b <= a:
            return 0
        hi = band_shard_rows(s, P) if hi is None else hi
        return max(0, min(hi, inv(s, b)) - max(lo, inv(s, a)))

    if count(qs, real, S) > 0 and count(ks, real, S) > 0:          # rows behind real_len see the keys behind real_len
        return True
    nq, nk = inv(qs, real), inv(ks, real)                           # the real rows / keys: indices [0, nq) / [0, nk)
    if nq == 0 or nk == 0:
        return False
    if count(qs, max(rf_lo, 0), min(rf_hi, real)) > 0 or count(ks, max(cf_lo, 0), min(cf_hi, real)) > 0:   # a full row / a full column
        return True
    if band <= 0:
        return False

    def parts(s, n):   # (first index, end index, is an interval of coordinates) of the video part and of the tail part below real_len
        nv = P * s.n_frames
        out = []
        if min(n, nv) > 0:
            out.append((0, min(n, nv), not kind or s.n_frames == F))   # (token-major, all frames: the coordinates are consecutive)
        if n > nv:
            out.append((nv, n, True))
        return out

    def coord(s, l):
        return band_shard_coord((vid0, F, P), s, kind, l)

    for qa, qb, q_iv in parts(qs, nq):
        for ka, kb, k_iv in parts(ks, nk):
            if q_iv:      # an interval of rows [x, y]: a key within the band of it
                x, y = coord(qs, qa), coord(qs, qb - 1)
                if count(ks, x - band + 1, y + band, ka, kb) > 0:
                    return True
            elif k_iv:
                x, y = coord(ks, ka), coord(ks, kb - 1)
                if count(qs, x - band + 1, y + band, qa, qb) > 0:
                    return True
            elif qb < P * qs.n_frames or kb < P * ks.n_frames:   # real_len inside the video: the hulls
                if coord(ks, ka) - coord(qs, qb - 1) < band and coord(qs, qa) - coord(ks, kb - 1) < band:
                    return True
            else:
                # two sets of whole frames: row - key = m * F + d with the patch distance |m| <= P - 1 and the frame distance d in [d_lo, d_hi]
                d_lo, d_hi = qs.f0 - (ks.f0 + ks.n_frames - 1), qs.f0 + qs.n_frames - 1 - ks.f0
                m_lo, m_hi = (-band - d_hi) // F + 1, -((d_lo - band) // F) - 1     # m * F + d_hi > -band, m * F + d_lo < band
                if max(m_lo, -(P - 1)) <= min(m_hi, P - 1):
                    return True
    return False


def _band_shard_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: BandMask, num_tokens: int, perm, q_shard, k_shard,
                          out_dtype: Optional[torch.dtype] = None, flags: Optional[torch.Tensor] = None,
                          out: Optional[torch.Tensor] = None, _switch=None):
    """Band attention of a FRAME SHARD of the rows over a FRAME SHARD of the keys (svg_band_shard_attention_lse[_f32]) -> (o, lse): q
    [cfg, H, Sq, D] (or [BH, Sq, D]) holds the rows of q_shard, k / v [cfg, H, Sk, D] those of k_shard — whole frames of the video, frame-
    major as the model stores them, and the rows of the shard's tail behind them (BandShard or (f0, n_frames, tail_begin, n_tail)) — of a
    sequence of num_tokens rows whose video `perm` = (vid0, num_frame, frame_size) describes.  flags (int64 / bool [BH] on the GPU, or
    None: every head in logical order) marks the token-major heads: the kernel reads their rows through the fused placement of a video of
    the shard's frames, both kinds of head in ONE launch, no flag is read back.  Row lq sees key lk where `mask` allows the coordinates the
    two maps give (band_shard_coord).  o has q's shape and dtype and lse is contiguous fp32 of shape q.shape[:-1], both in the order q was
    given in (a row that sees no key of the shard: o = 0, lse = -inf) — parts for merge_attention_states: the parts of one q shard over
    k shards that cover the sequence merge to the shard's rows of band_attention with the same flags.  Layouts and copies: _layout_plan.
    out_dtype=torch.float32 (without out): (o32, lse), the rows before their rounding.
    head_dim 128, bf16 / fp16, GPU tensors: anything else raises before anything runs — there is no fall-back.
    _switch: (alt_mask, use_alt_flag) of band_shard_attention_switch — the svg_band_shard_attention_switch_lse[_f32] entries."""
    if out_dtype not in (None, torch.float32):
        raise ValueError(f"band_shard_attention: out_dtype is None (q's dtype) or torch.float32, got {out_dtype}")
    f32 = out_dtype == torch.float32
    if f32 and out is not None:
        raise ValueError("band_shard_attention(out_dtype=torch.float32): fp32 rows are parts for merge_attention_states, without out")
    _gpu(q, k, v, out, flags)
    if _switch is not None:
        alt_mask, use_alt_flag = _switch
        _dev(use_alt_flag)
        if use_alt_flag.dtype != torch.int32 or use_alt_flag.numel() < 1:
            raise ValueError(f"band_shard_attention_switch: use_alt_flag is int32 [1] on the GPU, got {use_alt_flag.dtype} "
                             f"{tuple(use_alt_flag.shape)}")
    if not (q.dim() == k.dim() == v.dim() and q.dim() in (3, 4) and k.shape == v.shape and q.shape[:-2] == k.shape[:-2]
            and q.shape[-1] == k.shape[-1] and q.dtype == k.dtype == v.dtype):
        raise ValueError(f"band_shard_attention: q [.., Sq, D], k / v [.., Sk, D] of one dtype, got {tuple(q.shape)}, {tuple(k.shape)}, "
                         f"{tuple(v.shape)}")
    Sq, Sk, D = q.shape[-2], k.shape[-2], q.shape[-1]
    S = int(num_tokens)
    if D != 128 or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"band_shard_attention: head_dim 128, bfloat16 / float16; got D = {D}, {q.dtype} (no shard form, no fall-back)")
    vid0, F, P = _video(perm)
    if F <= 0 or P <= 0 or vid0 < 0 or vid0 + F * P > S:
        raise ValueError(f"band_shard_attention: a video of {F} frames of {P} rows from row {vid0} does not fit {S} rows")
    qs, ks = _shard(q_shard), _shard(k_shard)
    _check_shard("band_shard_attention: q shard", qs, S, vid0, F, P)
    _check_shard("band_shard_attention: k shard", ks, S, vid0, F, P)
    if Sq != band_shard_rows(qs, P) or Sk != band_shard_rows(ks, P):
        raise ValueError(f"band_shard_attention: q holds {Sq} rows, k {Sk}; the shards say {band_shard_rows(qs, P)} and {band_shard_rows(ks, P)}")
    if out is not None and (out.shape != q.shape or out.dtype != q.dtype):
        raise ValueError(f"band_shard_attention: out must have q's shape and dtype, got {tuple(out.shape)} {out.dtype}")
    BH = q.numel() // (Sq * D)
    flag = None
    if flags is not None:
        flag = flags.to(torch.int64).contiguous()
        if flag.numel() != BH:
            raise ValueError(f"band_shard_attention: {flag.numel()} flags for {BH} heads")
    load()
    lse = empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    pd = PermDesc(_ptr(flag), vid0, F, P)
    geom = (BH, S, D, _dtype_code(q), _sm_scale(None, D), C.byref(mask), C.byref(pd))
    name = "svg_band_shard_attention_lse"
    if _switch is not None:   # the device switch: alt_mask and the flag behind perm, the entries of include/svg_attn_band_shard_switch.h
        geom += (C.byref(alt_mask), use_alt_flag.data_ptr())
        name = "svg_band_shard_attention_switch_lse"
    p = _layout_plan(q, k, v, o=_O32 if f32 else _O16, out=out)
    _call_lse(name, f32, p, lse, *geom, C.byref(qs), C.byref(ks))
    return p.result(), lse


# (The public name is bound by assignment: the coverage walk of tests/test_gpu_poison.py lists the `def`s of this module that allocate and
#  looks for their poison rows in its own file; the rows of this wrapper are in tests/test_gpu_band_shard.py, which also checks that the
#  wrapper allocates through the switch.)
band_shard_attention = _band_shard_attention


def _band_shard_attention_switch(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: BandMask, alt_mask: BandMask,
                                 use_alt_flag: torch.Tensor, num_tokens: int, perm, q_shard, k_shard,
                                 out_dtype: Optional[torch.dtype] = None, flags: Optional[torch.Tensor] = None,
                                 out: Optional[torch.Tensor] = None):
    """band_shard_attention with a device-side switch (svg_band_shard_attention_switch_lse[_f32]) -> (o, lse) or, with
    out_dtype=torch.float32, (o32, lse): `use_alt_flag` (int32 [1] on the GPU) == 0 gives band_shard_attention(mask, flags) bit for bit,
    != 0 band_shard_attention(alt_mask, flags=None) — the alternate mask over the num_tokens rows of the whole sequence, every head in
    logical order, `flags` not read — on the same two shards; no host read of the flag.  What a frame-sharded rank launches where an SVG1
    processor switches between its sparse mask with the head placement and the dense warm-up mask without it.  Everything else — shapes,
    views, out, what is refused — as band_shard_attention."""
    return _band_shard_attention(q, k, v, mask, num_tokens, perm, q_shard, k_shard, out_dtype, flags, out, _switch=(alt_mask, use_alt_flag))


# (bound by assignment like band_shard_attention; its poison rows are in tests/test_gpu_band_shard_switch.py)
band_shard_attention_switch = _band_shard_attention_switch


def cross_attention_supported(q: torch.Tensor, k: torch.Tensor) -> bool:
    """svg_cross_attention exists for 16-bit GPU tensors of head_dim 128 (q and k of one dtype)."""
    return (q.is_cuda and k.is_cuda and q.dtype in (torch.bfloat16, torch.float16) and k.dtype == q.dtype
            and q.shape[-1] == 128 and k.shape[-1] == 128)


def cross_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, sm_scale: Optional[float] = None, token_major_out: bool = False,
                    out: Optional[torch.Tensor] = None, return_lse: bool = False, out_dtype: Optional[torch.dtype] = None):
    """Dense attention of q [B, H, Sq, D] over k, v [B, H, Skv, D] (or [BH, S, D]; Sq != Skv allowed) -> o of q's shape: softmax(q k^T
    * sm_scale) v per head (svg_cross_attention: head_dim 128, bf16 / fp16).  Strided views with stride(-1) == 1 (projection outputs,
    slices of a fused k/v projection) are read in place (always through a layout; layouts and copies: _layout_plan).  token_major_out: as
    band_attention.
    return_lse: (o, lse) with lse the row log-sum-exp of the scaled scores (natural log), contiguous fp32 of shape q.shape[:-1] — what
    merge_attention_states takes (svg_cross_attention_lse); o has the same bits as without.
    out_dtype=torch.float32 (with return_lse=True, without out / token_major_out; ValueError otherwise): (o32, lse) with o32 the rows
    before their rounding, contiguous fp32 of q's shape (svg_cross_attention_lse_f32) — parts for merge_attention_states, which then rounds
    once; o32.to(q.dtype) is the o of return_lse=True."""
    f32 = _want_f32_parts("cross_attention", out_dtype, return_lse, out, token_major_out)
    return _cross_attention(q, k, v, None, None, sm_scale, token_major_out, out, return_lse, f32)


def cross_attention_keyrange(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, kv_end: torch.Tensor, kv_begin: Optional[torch.Tensor] = None,
                             sm_scale: Optional[float] = None, token_major_out: bool = False, out: Optional[torch.Tensor] = None,
                             return_lse: bool = False, out_dtype: Optional[torch.dtype] = None):
    """cross_attention over one key window per group of heads (svg_cross_attention_keyrange): kv_end / kv_begin are int32 GPU tensors of n
    entries, BH % n == 0 (n = B: one window per video, the key-padding mask of a batch of prompts); heads [i * BH / n, (i + 1) * BH / n)
    attend to the keys [kv_begin[i], kv_end[i]) (kv_begin None: from key 0).  The kernel clamps the windows to 0 <= begin <= end <= Skv,
    reads no key row outside a window and writes zeros for an empty one.  Layouts, token_major_out, out: as cross_attention.
    return_lse: as cross_attention, over the window's keys; -inf for an empty window.  out_dtype: as cross_attention (zeros for an
    empty window)."""
    assert kv_end is not None
    f32 = _want_f32_parts("cross_attention_keyrange", out_dtype, return_lse, out, token_major_out)
    return _cross_attention(q, k, v, kv_begin, kv_end, sm_scale, token_major_out, out, return_lse, f32)


def _cross_attention(q, k, v, kv_begin, kv_end, sm_scale, token_major_out, out, return_lse=False, f32=False):
    """cross_attention (kv_end None), and cross_attention_keyrange; f32: svg_cross_attention_lse_f32, (o32, lse)"""
    lib = load()
    _gpu(q, k, v, out)
    assert k.shape == v.shape and q.shape[:-2] == k.shape[:-2] and q.shape[-1] == k.shape[-1] and q.dtype == k.dtype == v.dtype
    Sq, D = q.shape[-2], q.shape[-1]
    Skv = k.shape[-2]
    BH = q.numel() // (Sq * D)
    scale = _sm_scale(sm_scale, D)
    n = 1
    if kv_end is not None:
        _dev(kv_end, kv_begin)
        n = kv_end.numel()
        assert kv_end.dtype == torch.int32 and n > 0 and BH % n == 0, "kv_end: int32, BH % numel == 0"
        assert kv_begin is None or (kv_begin.dtype == torch.int32 and kv_begin.numel() == n), "kv_begin: int32, as many entries as kv_end"
    # (contiguous [BH, Sq] whatever the layout of q / o)
    lse = empty(q.shape[:-1], dtype=torch.float32, device=q.device) if return_lse else None
    p = _layout_plan(q, k, v, o=_O32 if f32 else _O16, out=out, token_major_out=token_major_out, null_layout=False)
    q, k, v, o = p.q, p.k, p.v, p.o
    if f32:
        _check(lib.svg_cross_attention_lse_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), BH, Sq, Skv, D,
                                               _dtype_code(q), scale, _ptr(kv_begin), _ptr(kv_end), BH // n, p.lay, _stream()),
               "svg_cross_attention_lse_f32")
    elif return_lse:
        _check(lib.svg_cross_attention_lse(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), BH, Sq, Skv, D,
                                           _dtype_code(q), scale, _ptr(kv_begin), _ptr(kv_end), BH // n, p.lay, _stream()),
               "svg_cross_attention_lse")
    elif kv_end is None:
        _check(lib.svg_cross_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, Sq, Skv, D, _dtype_code(q), scale, p.lay,
                                       _stream()), "svg_cross_attention")
    else:
        _check(lib.svg_cross_attention_keyrange(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), BH, Sq, Skv, D, _dtype_code(q), scale,
                                                _ptr(kv_begin), kv_end.data_ptr(), BH // n, p.lay, _stream()), "svg_cross_attention_keyrange")
    return (p.result(), lse) if return_lse else p.result()


MERGE_MAX_PARTS = 8   # svg_merge_attention_states: the part pointers travel in the kernel arguments


def merge_attention_states(o_parts: Sequence[torch.Tensor], lse_parts: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None,
                           token_major_out: bool = False, return_lse: bool = False, out_dtype: Optional[torch.dtype] = None):
    """Combine n partial attention results of the SAME query rows over disjoint parts of the keys into the result over all of them
    (svg_merge_attention_states): o_parts[i] [B, H, Sq, D] or [BH, Sq, D] (16-bit, D 64 / 128), lse_parts[i] fp32 of shape o.shape[:-1], as
    cross_attention(..., return_lse=True) returns them.  All parts in one pass, fp32, one rounding: o = sum_i w_i o_i / sum_i w_i with w_i =
    exp(lse_i - max lse).  At most MERGE_MAX_PARTS parts (ValueError).  out / token_major_out: as cross_attention; return_lse: (o, lse) with
    the merged log-sum-exp.
    fp32 parts (o_parts[0].dtype == torch.float32: what the attention wrappers return with out_dtype=torch.float32) are merged by
    svg_merge_attention_states_f32: the same statement, the parts unrounded, so the rounding to the output dtype is the only one.  The
    output dtype is then out_dtype (bf16 / fp16) or that of `out` — one of them is required; parts of mixed dtype: ValueError."""
    lib = load()
    n = len(o_parts)
    if not 1 <= n <= MERGE_MAX_PARTS or len(lse_parts) != n:
        raise ValueError(f"merge_attention_states takes 1 to {MERGE_MAX_PARTS} parts with one lse each, got {n} and {len(lse_parts)}")
    x = o_parts[0]
    if any(t.dtype != x.dtype for t in o_parts):
        raise ValueError(f"merge_attention_states: parts of one dtype, got {[t.dtype for t in o_parts]}")
    f32 = x.dtype == torch.float32
    if f32:
        if out is not None and out_dtype is not None and out.dtype != out_dtype:
            raise ValueError(f"merge_attention_states: out is {out.dtype}, out_dtype {out_dtype}")
        odt = out.dtype if out is not None else out_dtype
        if odt not in (torch.bfloat16, torch.float16):
            raise ValueError(f"merge_attention_states of fp32 parts: out_dtype (torch.bfloat16 / torch.float16) or a 16-bit out, got {odt}")
    else:
        if out_dtype is not None and out_dtype != x.dtype:
            raise ValueError(f"merge_attention_states of {x.dtype} parts returns {x.dtype}, got out_dtype = {out_dtype}")
        odt = x.dtype
    _gpu(*o_parts, *lse_parts, out)
    Sq, D = x.shape[-2], x.shape[-1]
    BH = x.numel() // (Sq * D)
    for o_i, l_i in zip(o_parts, lse_parts):
        assert o_i.shape == x.shape and l_i.shape == x.shape[:-1] and l_i.dtype == torch.float32
    # (parts are contiguous by contract; one that is not — or not 16-byte aligned — is copied, as the cross-attention entries copy)
    o_c = [t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format) for t in o_parts]
    l_c = [t.contiguous() for t in lse_parts]
    if out is not None:
        assert out.shape == x.shape and out.dtype == odt
    p = _layout_plan(x, x, x, out=out, token_major_out=token_major_out, o_dtype=odt, null_layout=False, inputs_as_given=True)
    lse = empty(x.shape[:-1], dtype=torch.float32, device=x.device) if return_lse else None
    op = (C.c_void_p * MERGE_MAX_PARTS)(*[t.data_ptr() for t in o_c], *([None] * (MERGE_MAX_PARTS - n)))
    lp = (C.c_void_p * MERGE_MAX_PARTS)(*[t.data_ptr() for t in l_c], *([None] * (MERGE_MAX_PARTS - n)))
    name = "svg_merge_attention_states_f32" if f32 else "svg_merge_attention_states"
    rc = getattr(lib, name)(C.cast(op, _VP), C.cast(lp, _VP), n, p.o.data_ptr(), _ptr(lse), BH, Sq, D, _dtype_code(p.o), p.lay, _stream())
    _check(rc, name)
    return (p.result(), lse) if return_lse else p.result()


def cross_attention_pair(q: torch.Tensor, k_a: torch.Tensor, v_a: torch.Tensor, k_b: torch.Tensor, v_b: torch.Tensor,
                         sm_scale: Optional[float] = None, token_major_out: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cross_attention(q, k_a, v_a) + cross_attention(q, k_b, v_b) in ONE launch (svg_cross_attention_pair: the text and the image keys
    of a Wan I2V block), bit for bit: each branch is rounded to the 16-bit type, then added as torch adds two 16-bit tensors.  The two key
    sets have their own lengths and their own strides.  Layouts, token_major_out, out: as cross_attention; out must not overlap an input."""
    lib = load()
    _gpu(q, k_a, v_a, k_b, v_b, out)
    for k, v in ((k_a, v_a), (k_b, v_b)):
        assert k.shape == v.shape and q.shape[:-2] == k.shape[:-2] and q.shape[-1] == k.shape[-1] and q.dtype == k.dtype == v.dtype
    Sq, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (Sq * D)
    scale = _sm_scale(sm_scale, D)

    p = _layout_plan(q, k_a, v_a, k_b, v_b, out=out, token_major_out=token_major_out, null_layout=False)
    _check(lib.svg_cross_attention_pair(p.q.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), p.k_b.data_ptr(), p.v_b.data_ptr(), p.o.data_ptr(), BH,
                                        Sq, k_a.shape[-2], k_b.shape[-2], D, _dtype_code(q), scale, p.lay, p.lay_b, _stream()),
           "svg_cross_attention_pair")
    return p.result()


def varblock_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, block_map: torch.Tensor, q_sizes: torch.Tensor,
                       k_sizes: torch.Tensor, sm_scale: Optional[float] = None, q_row_idx: Optional[torch.Tensor] = None,
                       kv_row_idx: Optional[torch.Tensor] = None, variant: int = -1, fp8: bool = False,
                       workspace: Optional[torch.Tensor] = None, token_major_out: bool = False,
                       rows_covered: bool = False, return_lse: bool = False, out_dtype: Optional[torch.dtype] = None):
    """q: [Hq, Sq, D], k/v: [Hkv, Skv, D] (or [B, H, S, D]: heads = B * H); block_map bool [Hkv, QB, KB]; sizes int32 [Hkv, QB] /
    [Hkv, KB].  -> o of q's shape.
    fp8=True: e4m3 QK^T / PV (svg_varblock_attention_fp8, D = 128, default schedule only).
    workspace: optional uint8 GPU tensor of svg_varblock_workspace_bytes(...) bytes for the 16-bit call (tests read the launch
    order back from it; see varblock_launch_order).
    Strided views / token_major_out: as band_attention (svg_varblock_attention_strided: head_dim 128, variant -1 on block-rows large
    enough for the default body, 16-bit).
    rows_covered: the caller guarantees sum(q_sizes[h]) == Sq for every head (k-means cluster sizes do), so every output row is
    written by the kernel and the output is not zero-filled first (a 2 S H D-byte memset per call otherwise).
    return_lse: (o, lse) with lse the row log-sum-exp of the scaled scores over the keys the block map gives the row (natural log),
    contiguous fp32 of shape q.shape[:-1] (per q head), in the caller's row order; -inf for a row that sees no key and, without
    rows_covered, for a row no block-row covers (svg_varblock_attention_lse: head_dim 128, 16-bit, ALWAYS the two-phase body of variant
    3 — variant -1, 3 or 8; anything else raises ValueError); o has the bits of variant 3.
    out_dtype=torch.float32 (with return_lse=True, without token_major_out; ValueError otherwise): (o32, lse) with o32 the rows before
    their rounding, contiguous fp32 of q's shape (svg_varblock_attention_lse_f32), zero-filled first unless rows_covered — parts for
    merge_attention_states, which then rounds once; o32.to(q.dtype) is the o of return_lse=True."""
    f32 = _want_f32_parts("varblock_attention", out_dtype, return_lse, None, token_major_out)
    if return_lse:
        if fp8 or variant not in (-1, 3, 8) or q.shape[-1] != 128:
            raise ValueError("varblock_attention(return_lse=True): head_dim 128, 16-bit, variant -1 / 3 / 8 (the two-phase 16x16x32 body); "
                             f"got D = {q.shape[-1]}, variant = {variant}, fp8 = {fp8}")
        return _varblock_attention_lse(q, k, v, block_map, q_sizes, k_sizes, sm_scale, q_row_idx, kv_row_idx, workspace, token_major_out,
                                       rows_covered, f32)
    lib = load()
    _dev(block_map, q_sizes, k_sizes, q_row_idx, kv_row_idx)
    _gpu(q, k, v)
    Sq, D = q.shape[-2], q.shape[-1]
    Skv = k.shape[-2]
    Hq, Hkv = q.numel() // (Sq * D), k.numel() // (Skv * D)
    QB, KB = q_sizes.shape[-1], k_sizes.shape[-1]
    assert block_map.shape == (Hkv, QB, KB) and block_map.dtype in (torch.bool, torch.uint8)
    assert q_sizes.dtype == torch.int32 and k_sizes.dtype == torch.int32
    if q_row_idx is not None:
        assert q_row_idx.dtype == torch.int32 and q_row_idx.shape == (Hq, Sq)
    if kv_row_idx is not None:
        assert kv_row_idx.dtype == torch.int32 and kv_row_idx.shape == (Hkv, Skv)
    scale = _sm_scale(sm_scale, D)
    p = _layout_plan(q, k, v, token_major_out=token_major_out, views_on_copies=False, zero_o=not rows_covered,
                     views=not fp8 and variant == -1 and strided_attention_supported(q) and Sq >= 160 * QB)
    q, k, v, o = p.q, p.k, p.v, p.o
    if fp8:
        need = int(lib.svg_varblock_attention_fp8_workspace_bytes(Hq, Hkv, QB, KB, Sq, Skv, D))
        if need == 0:
            raise RuntimeError(f"svg_varblock_attention_fp8: unsupported shape (D = {D}; only 128)")
        key = WorkspaceCache.key("vb", Hq, Hkv, Sq, Skv, QB, KB, device=q.device)
        ws = _F8_WS.get(key)
        if ws is None or ws.numel() < need:
            ws = _F8_WS[key] = empty(need, dtype=torch.uint8, device=q.device)
        rc = lib.svg_varblock_attention_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), Hq, Hkv, Sq, Skv, D, _dtype_code(q),
                                            scale, block_map.data_ptr(), q_sizes.data_ptr(), k_sizes.data_ptr(), QB, KB,
                                            _ptr(q_row_idx), _ptr(kv_row_idx), ws.data_ptr(), ws.numel(), _stream())
        _check(rc, "svg_varblock_attention_fp8")
        return o
    need = int(lib.svg_varblock_workspace_bytes(Hq, Hkv, QB, KB, Sq))
    ws = empty(need, dtype=torch.uint8, device=q.device) if workspace is None else workspace
    _dev(ws)
    assert ws.dtype == torch.uint8 and ws.numel() >= need
    if p.lay is not None:
        rc = lib.svg_varblock_attention_strided(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), Hq, Hkv, Sq, Skv, D,
                                                _dtype_code(q), scale, block_map.data_ptr(), q_sizes.data_ptr(), k_sizes.data_ptr(),
                                                QB, KB, _ptr(q_row_idx), _ptr(kv_row_idx), ws.data_ptr(), ws.numel(), p.lay, _stream())
        _check(rc, "svg_varblock_attention_strided")
        return o
    rc = lib.svg_varblock_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), Hq, Hkv, Sq, Skv, D,
                                    _dtype_code(q), scale, block_map.data_ptr(), q_sizes.data_ptr(), k_sizes.data_ptr(),
                                    QB, KB, _ptr(q_row_idx), _ptr(kv_row_idx), ws.data_ptr(), ws.numel(), variant,
                                    _stream())
    _check(rc, "svg_varblock_attention")
    return o


def _varblock_attention_lse(q, k, v, block_map, q_sizes, k_sizes, sm_scale, q_row_idx, kv_row_idx, workspace, token_major_out, rows_covered,
                            f32=False):
    """varblock_attention(return_lse=True): svg_varblock_attention_lse (f32: svg_varblock_attention_lse_f32), never an entry without lse.
    Layouts and copies: _layout_plan."""
    lib = load()
    _dev(block_map, q_sizes, k_sizes, q_row_idx, kv_row_idx)
    _gpu(q, k, v)
    Sq, D = q.shape[-2], q.shape[-1]
    Skv = k.shape[-2]
    Hq, Hkv = q.numel() // (Sq * D), k.numel() // (Skv * D)
    QB, KB = q_sizes.shape[-1], k_sizes.shape[-1]
    assert block_map.shape == (Hkv, QB, KB) and block_map.dtype in (torch.bool, torch.uint8)
    assert q_sizes.dtype == torch.int32 and k_sizes.dtype == torch.int32
    if q_row_idx is not None:
        assert q_row_idx.dtype == torch.int32 and q_row_idx.shape == (Hq, Sq)
    if kv_row_idx is not None:
        assert kv_row_idx.dtype == torch.int32 and kv_row_idx.shape == (Hkv, Skv)
    scale = _sm_scale(sm_scale, D)
    need = int(lib.svg_varblock_workspace_bytes(Hq, Hkv, QB, KB, Sq))
    ws = empty(need, dtype=torch.uint8, device=q.device) if workspace is None else workspace
    _dev(ws)
    assert ws.dtype == torch.uint8 and ws.numel() >= need
    # (contiguous [Hq, Sq] whatever the layout of q / o; rows the kernel does not write: -inf where o holds zeros)
    lse = empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    if not rows_covered:
        lse.fill_(float("-inf"))
    p = _layout_plan(q, k, v, o=_O32 if f32 else _O16, token_major_out=token_major_out, zero_o=not rows_covered)
    q, k, v, o = p.q, p.k, p.v, p.o
    if f32:
        rc = lib.svg_varblock_attention_lse_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), Hq, Hkv, Sq, Skv, D,
                                                _dtype_code(q), scale, block_map.data_ptr(), q_sizes.data_ptr(), k_sizes.data_ptr(), QB, KB,
                                                _ptr(q_row_idx), _ptr(kv_row_idx), ws.data_ptr(), ws.numel(), p.lay, _stream())
        _check(rc, "svg_varblock_attention_lse_f32")
    else:
        rc = lib.svg_varblock_attention_lse(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), Hq, Hkv, Sq, Skv, D,
                                            _dtype_code(q), scale, block_map.data_ptr(), q_sizes.data_ptr(), k_sizes.data_ptr(), QB, KB,
                                            _ptr(q_row_idx), _ptr(kv_row_idx), ws.data_ptr(), ws.numel(), p.lay, _stream())
        _check(rc, "svg_varblock_attention_lse")
    return o, lse


def varblock_workspace(Hq: int, Hkv: int, QB: int, KB: int, Sq: int, device) -> torch.Tensor:
    return torch.zeros(int(load().svg_varblock_workspace_bytes(Hq, Hkv, QB, KB, Sq)), dtype=torch.uint8, device=device)


def varblock_launch_order(workspace: torch.Tensor, Hkv: int, QB: int, KB: int):
    """The launch order a 256-row variable-block call (variants 3 / 6 / 7) left in its workspace: int32 [n, 3] rows of
    (q head, block-row << 16 | sub-tile, partner) in dispatch order — partner >= 0: the tile also carries the ragged last tile of
    that block-row (remainder packing) — (layout: csrc/attention_varblock.hip vb_ws: plan prefix sums, two buckets + the partner per
    block-row, histogram, then [count, pad, entries])."""
    w = workspace.view(torch.int32)
    off = Hkv * (3 * (QB + 1) + (KB + 1)) + 3 * Hkv * QB + Hkv * 64
    n = int(w[off].item())
    return w[off + 2: off + 2 + 3 * n].view(n, 3).clone()


def varblock_partners(workspace: torch.Tensor, Hkv: int, QB: int, KB: int) -> torch.Tensor:
    """The remainder-packing partners a variant-3 call left in its workspace: int32 [Hkv, QB]; j >= 0: block-row i's ragged last tile
    also carries block-row j's, -2: carried by its partner, -1: alone (csrc/attention_varblock.hip varblock_pair_*_kernel)."""
    w = workspace.view(torch.int32)
    off = Hkv * (3 * (QB + 1) + (KB + 1)) + 2 * Hkv * QB
    return w[off: off + Hkv * QB].view(Hkv, QB).clone()


class ClockProbe:
    """Sustained shader clock over a span of GPU work (svg_debug_clock_probe): `start()` launches the one-wave probe on its own
    stream, `arm_stop()` raises its flag from a third stream behind the work enqueued so far, `result()` waits for the probe and returns
    MHz (None if the counters did not move)."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self.flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.out = torch.zeros(2, dtype=torch.int64, device=self.dev)
        self.s_probe = torch.cuda.Stream(device=self.dev)
        self.s_flag = torch.cuda.Stream(device=self.dev)

    def start(self, max_ms: int = 20000) -> None:
        self.flag.zero_()
        self.out.zero_()
        torch.cuda.synchronize(self.dev)
        with torch.cuda.stream(self.s_probe):
            _check(load().svg_debug_clock_probe(self.flag.data_ptr(), self.out.data_ptr(), int(max_ms), _stream()),
                   "svg_debug_clock_probe")

    def arm_stop(self) -> None:
        """Raise the flag once everything enqueued so far on the CURRENT stream has finished (stream-ordered, no host wait) — call it
        right after the last launch of the span, BEFORE any device-wide synchronisation (which would wait for the probe itself)."""
        self.s_flag.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.s_flag):
            self.flag.fill_(1)

    def result(self):
        self.s_probe.synchronize()
        c, w = (int(x) for x in self.out.tolist())
        return round(100.0 * c / w, 1) if w > 0 and c > 0 else None


def clear_workspace_cache() -> None:
    """Drop the cached workspaces (band_attention_fp8 / varblock_attention(fp8=True) / kmeans_loop keep one per shape, device and stream,
    at most WorkspaceCache.capacity of each kind)."""
    _F8_WS.clear()
    _KMEANS_WS.clear()
    from . import kmeans_utils as _ku   # (its KMeansState cache of the per-iteration path follows the same policy)

    _ku._STATE_CACHE.clear()


def sample_mse(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, rows: torch.Tensor, prof: ProfileDesc,
               sm_scale: Optional[float] = None, skip_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q,k,v [BH, S, D] (or [B, H, S, D]: BH = B * H); rows int64 [R] (device) -> mse float32 [2, BH].  skip_flag (int32 [1] on the
    GPU) != 0: the kernels return at once and the result is undefined (a dense step does not use it).
    Strided views are read in place by svg_sample_mse_strided (bf16: the second form of the kernel); layouts and copies: _layout_plan."""
    lib = load()
    _dev(rows, skip_flag)
    _gpu(q, k, v)
    S, D = q.shape[-2], q.shape[-1]
    BH = q.numel() // (S * D)
    R = rows.numel()
    out = empty((2, BH), dtype=torch.float32, device=q.device)
    ws = empty(lib.svg_sample_mse_workspace_bytes(BH, R, D, S), dtype=torch.uint8, device=q.device)
    scale = _sm_scale(sm_scale, D)
    if skip_flag is not None:
        assert skip_flag.dtype == torch.int32
        out.zero_()
    p = _layout_plan(q, k, v, o=_NO_O, views=q.dtype == torch.bfloat16)   # (the strided form is the kernel's second form: bf16)
    q, k, v = p.q, p.k, p.v
    if p.lay is not None:
        rc = lib.svg_sample_mse_strided(q.data_ptr(), k.data_ptr(), v.data_ptr(), rows.data_ptr(), R, BH, S, D, _dtype_code(q), scale,
                                        C.byref(prof), out.data_ptr(), ws.data_ptr(), ws.numel(), _ptr(skip_flag), p.lay, _stream())
        _check(rc, "svg_sample_mse_strided")
    elif skip_flag is not None:
        rc = lib.svg_sample_mse_flagged(q.data_ptr(), k.data_ptr(), v.data_ptr(), rows.data_ptr(), R, BH, S, D, _dtype_code(q),
                                        scale, C.byref(prof), out.data_ptr(), ws.data_ptr(), ws.numel(), skip_flag.data_ptr(),
                                        _stream())
        _check(rc, "svg_sample_mse_flagged")
    else:
        rc = lib.svg_sample_mse(q.data_ptr(), k.data_ptr(), v.data_ptr(), rows.data_ptr(), R, BH, S, D, _dtype_code(q), scale,
                                C.byref(prof), out.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        _check(rc, "svg_sample_mse")
    return out


# ------------------------------------------------------------------------------------------------------
# the online profiler on frame shards (include/svg_attn_profile_shard.h): a partial per key shard, the combine over partials
# ------------------------------------------------------------------------------------------------------
PROFILE_MAX_PARTS = 64   # svg_sample_mse_from_parts: the part pointers travel in the kernel arguments


def _sample_mse_shard_partial(q_rows: torch.Tensor, k: torch.Tensor, v: torch.Tensor, rows: torch.Tensor, prof: ProfileDesc, k_shard,
                              num_tokens: int, sm_scale: Optional[float] = None, skip_flag: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The profiler's partial of R sampled rows over the keys of ONE frame shard (svg_sample_mse_shard_partial): q_rows [BH, R, D] (or
    [B, H, R, D]) is q[..., rows, :] of the whole sequence, already gathered; rows int64 [R] on the GPU, the GLOBAL row indices; k / v
    [BH, Sk, D] the rows of k_shard (BandShard or (f0, n_frames, tail_begin, n_tail)) of a sequence of num_tokens rows whose video prof
    describes (prof.vid0 == 0) -> part fp32 [3, BH, R, D + 4]: per output (golden, variant 0, variant 1), head and row — in the kernel's rank
    order, a function of rows alone — the un-normalised O, then m (log2 domain), l, 0, 0.  Parts of shards that cover the keys go to
    sample_mse_from_parts.  Layouts and copies of k / v: _layout_plan.
    skip_flag (int32 [1] on the GPU) != 0: the kernels return at once and part is left as allocated.  bf16, head_dim 128, R <= 64; anything
    else raises — there is no fall-back."""
    lib = load()
    _dev(rows, skip_flag)
    _gpu(q_rows, k, v)
    R, D = q_rows.shape[-2], q_rows.shape[-1]
    Sk = k.shape[-2]
    BH = q_rows.numel() // (R * D)
    if q_rows.dtype != torch.bfloat16 or D != 128 or not (q_rows.dtype == k.dtype == v.dtype):
        raise ValueError(f"sample_mse_shard_partial: bfloat16, head_dim 128; got {q_rows.dtype} / {k.dtype} / {v.dtype}, D = {D} "
                         f"(no shard form, no fall-back)")
    if rows.numel() != R or rows.dtype != torch.int64 or k.shape != v.shape or k.shape[-1] != D or k.numel() != BH * Sk * D:
        raise ValueError(f"sample_mse_shard_partial: q_rows [BH, R, D], rows int64 [R], k / v [BH, Sk, D]; got {tuple(q_rows.shape)}, "
                         f"{tuple(rows.shape)} {rows.dtype}, {tuple(k.shape)}, {tuple(v.shape)}")
    S = int(num_tokens)
    ks = _shard(k_shard)
    F, P = int(prof.num_frame), int(prof.frame_size)
    if prof.vid0 != 0 or F <= 0 or P <= 0 or F * P > S:
        raise ValueError(f"sample_mse_shard_partial: a video of {F} frames of {P} rows from row {prof.vid0} in {S} rows (vid0 must be 0: rows "
                         f"in front of the video belong to no shard)")
    _check_shard("sample_mse_shard_partial: k shard", ks, S, 0, F, P)
    if Sk != band_shard_rows(ks, P):
        raise ValueError(f"sample_mse_shard_partial: k holds {Sk} rows, the shard says {band_shard_rows(ks, P)}")
    if skip_flag is not None:
        assert skip_flag.dtype == torch.int32
    part = empty((3, BH, R, D + 4), dtype=torch.float32, device=k.device)
    ws = empty(lib.svg_sample_mse_shard_workspace_bytes(BH, R, D, Sk), dtype=torch.uint8, device=k.device)
    q_rows = q_rows.contiguous()
    p = _layout_plan(k, k, v, o=_NO_O)   # (k and v alone: the layout's q and o members take k's strides)
    rc = lib.svg_sample_mse_shard_partial(q_rows.data_ptr(), p.k.data_ptr(), p.v.data_ptr(), rows.data_ptr(), R, BH, S, D, _dtype_code(k),
                                          _sm_scale(sm_scale, D), C.byref(prof), C.byref(ks), part.data_ptr(), ws.data_ptr(), ws.numel(),
                                          _ptr(skip_flag), p.lay, _stream())
    _check(rc, "svg_sample_mse_shard_partial")
    return part


def _sample_mse_from_parts(parts: Sequence[torch.Tensor], R: int, dtype: torch.dtype, emulate_bf16, skip_flag: Optional[torch.Tensor] = None
                           ) -> torch.Tensor:
    """mse fp32 [2, BH] from the partials of shards that cover the keys (svg_sample_mse_from_parts): parts[i] fp32 [3, BH, R, D + 4] as
    sample_mse_shard_partial (or neutral_profile_part) returns them, 1 to PROFILE_MAX_PARTS of them, merged in list order with the arithmetic
    of sample_mse's own combine; dtype is that of q, k, v (the roundings of emulate_bf16).  One part of the whole sequence gives the bits of
    sample_mse.  skip_flag != 0: the kernels return at once and the result is left as allocated."""
    lib = load()
    n = len(parts)
    if not 1 <= n <= PROFILE_MAX_PARTS:
        raise ValueError(f"sample_mse_from_parts takes 1 to {PROFILE_MAX_PARTS} parts, got {n}")
    x = parts[0]
    _dev(*parts, skip_flag)
    if any(t.dtype != torch.float32 or t.shape != x.shape for t in parts) or x.dim() != 4 or x.shape[0] != 3 or x.shape[2] != int(R):
        raise ValueError(f"sample_mse_from_parts: fp32 parts [3, BH, {R}, D + 4] of one shape, got {[tuple(t.shape) for t in parts]}")
    if dtype != torch.bfloat16:
        raise ValueError(f"sample_mse_from_parts: bfloat16 (the second form of the kernel), got {dtype}")
    if skip_flag is not None:
        assert skip_flag.dtype == torch.int32
    BH, D = x.shape[1], x.shape[3] - 4
    out = empty((2, BH), dtype=torch.float32, device=x.device)
    ws = empty(lib.svg_sample_mse_from_parts_workspace_bytes(BH), dtype=torch.uint8, device=x.device)
    pp = (C.c_void_p * n)(*[t.data_ptr() for t in parts])
    rc = lib.svg_sample_mse_from_parts(C.cast(pp, _VP), n, int(R), BH, D, SVG_DTYPE_BF16, int(bool(emulate_bf16)), out.data_ptr(),
                                       ws.data_ptr(), ws.numel(), _ptr(skip_flag), _stream())
    _check(rc, "svg_sample_mse_from_parts")
    return out


def _neutral_profile_part(BH: int, R: int, D: int, device) -> torch.Tensor:
    """The part of a rank that holds no rows: O = 0, m = -inf, l = 0 — weight 0 in sample_mse_from_parts, the other parts' bits unchanged."""
    part = empty((3, int(BH), int(R), int(D) + 4), dtype=torch.float32, device=device)
    part.zero_()
    part[..., int(D)] = float("-inf")
    return part


# (The public names are bound by assignment, as band_shard_attention is: the coverage walk of tests/test_gpu_poison.py lists the `def`s of
#  this module that allocate and looks for their poison rows in its own file; the rows of these are in tests/test_gpu_profile_shard.py.)
sample_mse_shard_partial = _sample_mse_shard_partial
sample_mse_from_parts = _sample_mse_from_parts
neutral_profile_part = _neutral_profile_part


def kmeans_xsq(x: torch.Tensor) -> torch.Tensor:
    lib = load()
    _dev(x)
    B, N, D = x.shape
    xsq = empty((B, N), dtype=torch.float32, device=x.device)
    _check(lib.svg_kmeans_xsq(x.data_ptr(), xsq.data_ptr(), B, N, D, _dtype_code(x), _stream()), "svg_kmeans_xsq")
    return xsq


class KmeansBuffers:
    """Device buffers reused across Lloyd iterations (labels, counts, sorted indices, shift, workspace)."""

    def __init__(self, B: int, N: int, K: int, D: int, device):
        lib = load()
        self.labels = empty((B, N), dtype=torch.int32, device=device)
        self.counts = empty((B, K), dtype=torch.int32, device=device)
        self.sorted_idx = empty((B, N), dtype=torch.int32, device=device)
        self.shift = empty((B,), dtype=torch.float32, device=device)
        self.ws = empty(lib.svg_kmeans_workspace_bytes(B, N, K, D), dtype=torch.uint8, device=device)


def kmeans_iter(x: torch.Tensor, xsq: Optional[torch.Tensor], c_in: torch.Tensor, c_out: torch.Tensor, buf: KmeansBuffers) -> None:
    """xsq: the reference's x_sq or None (the assignment kernel does not read it)"""
    lib = load()
    _dev(x, xsq, c_in, c_out)
    B, N, D = x.shape
    K = c_in.shape[1]
    assert c_in.shape == (B, K, D) and c_out.shape == (B, K, D) and c_in.dtype == x.dtype == c_out.dtype
    rc = lib.svg_kmeans_iter(x.data_ptr(), _ptr(xsq), c_in.data_ptr(), c_out.data_ptr(), buf.labels.data_ptr(),
                             buf.counts.data_ptr(), buf.sorted_idx.data_ptr(), buf.shift.data_ptr(), B, N, K, D,
                             _dtype_code(x), buf.ws.data_ptr(), buf.ws.numel(), _stream())
    _check(rc, "svg_kmeans_iter")


def kmeans_assign(x: torch.Tensor, centroids: torch.Tensor) -> torch.Tensor:
    """labels int32 [B, N] of the nearest centroid (lowest index on ties): the assignment half of kmeans_iter (svg_kmeans_assign)"""
    lib = load()
    _dev(x, centroids)
    B, N, D = x.shape
    K = centroids.shape[1]
    assert centroids.shape == (B, K, D) and centroids.dtype == x.dtype and x.is_contiguous() and centroids.is_contiguous()
    labels = empty((B, N), dtype=torch.int32, device=x.device)
    ws = empty(lib.svg_kmeans_workspace_bytes(B, N, K, D), dtype=torch.uint8, device=x.device)
    _check(lib.svg_kmeans_assign(x.data_ptr(), centroids.data_ptr(), labels.data_ptr(), B, N, K, D, _dtype_code(x), ws.data_ptr(),
                                 ws.numel(), _stream()), "svg_kmeans_assign")
    return labels


def kmeans_update(x: torch.Tensor, labels: torch.Tensor, centroids_in: torch.Tensor):
    """The update half on given labels (svg_kmeans_update) -> (centroids [B, K, D] of x.dtype, counts int32 [B, K], sorted_idx int32
    [B, N], shift float32 [B]); empty clusters keep centroids_in."""
    lib = load()
    _dev(x, labels, centroids_in)
    B, N, D = x.shape
    K = centroids_in.shape[1]
    assert labels.dtype == torch.int32 and labels.shape == (B, N) and labels.is_contiguous()
    assert centroids_in.shape == (B, K, D) and centroids_in.dtype == x.dtype and x.is_contiguous() and centroids_in.is_contiguous()
    cent = empty_like(centroids_in)
    counts = empty((B, K), dtype=torch.int32, device=x.device)
    sorted_idx = empty((B, N), dtype=torch.int32, device=x.device)
    shift = empty((B,), dtype=torch.float32, device=x.device)
    ws = empty(lib.svg_kmeans_workspace_bytes(B, N, K, D), dtype=torch.uint8, device=x.device)
    _check(lib.svg_kmeans_update(x.data_ptr(), labels.data_ptr(), centroids_in.data_ptr(), cent.data_ptr(), counts.data_ptr(),
                                 sorted_idx.data_ptr(), shift.data_ptr(), B, N, K, D, _dtype_code(x), ws.data_ptr(), ws.numel(), _stream()),
           "svg_kmeans_update")
    return cent, counts, sorted_idx, shift


def kmeans_loop(x: torch.Tensor, xsq: Optional[torch.Tensor], c_init: torch.Tensor, max_iters: int, tol: float, work=None,
                group: Optional[int] = None):
    """The whole Lloyd loop as one library call without host synchronisation (svg_kmeans_loop) -> (labels int32 [B, N], centroids
    [B, K, D], counts int32 [B, K], n_iters int32 [] on the device, sorted_idx int32 [B, N]).  `work`: a WorkspaceCache (or None: fresh
    scratch per call) that keeps the scratch tensors of a (B, N, K, D) shape per device AND stream between calls.
    group: None — one stopping rule over all B batches; an integer dividing B — one stopping rule per `group` consecutive batches
    (svg_kmeans_loop_grouped), n_iters is then int32 [B // group]."""
    lib = load()
    _dev(xsq, c_init)
    _gpu(x)
    B, N, D = x.shape
    K = c_init.shape[1]
    assert c_init.shape == (B, K, D) and c_init.dtype == x.dtype and c_init.is_contiguous()
    if group is not None:
        group = int(group)
        assert group >= 1 and B % group == 0, f"kmeans_loop: group = {group} must divide B = {B}"
    # x: contiguous, or batches further apart than N * D with contiguous rows inside (the video tokens `q[:, :V]` of a [H, S, D] tensor):
    # svg_kmeans_loop_strided reads them in place
    batch_strided = (not x.is_contiguous()) and x.stride(2) == 1 and x.stride(1) == D and x.stride(0) >= N * D and x.stride(0) % 8 == 0 \
        and x.data_ptr() % 16 == 0
    if not x.is_contiguous() and not batch_strided:
        x = x.contiguous()
    key = WorkspaceCache.key("kmeans", B, N, K, D, x.dtype, group, device=x.device)
    w = None if work is None else work.get(key)
    if w is None:
        nb = lib.svg_kmeans_loop_workspace_bytes(B, N, K, D) if group is None else lib.svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, group)
        w = dict(ca=empty_like(c_init), cb=empty_like(c_init), ws=empty(nb, dtype=torch.uint8, device=x.device))
        if work is not None:
            work[key] = w
    labels = empty((B, N), dtype=torch.int32, device=x.device)
    sorted_idx = empty((B, N), dtype=torch.int32, device=x.device)
    counts = empty((B, K), dtype=torch.int32, device=x.device)
    cent = empty_like(c_init)
    n_it = empty(() if group is None else (B // group,), dtype=torch.int32, device=x.device)   # (copied from the loop's state by every call)
    outs = (labels.data_ptr(), counts.data_ptr(), sorted_idx.data_ptr(), cent.data_ptr(), n_it.data_ptr(), B, N, K, D, _dtype_code(x))
    tail = (int(max_iters), float(tol), w["ws"].data_ptr(), w["ws"].numel(), _stream())
    cs = (c_init.data_ptr(), w["ca"].data_ptr(), w["cb"].data_ptr())
    if group is not None:
        if batch_strided:
            _check(lib.svg_kmeans_loop_grouped_strided(x.data_ptr(), int(x.stride(0)), *cs, *outs, group, *tail), "svg_kmeans_loop_grouped_strided")
        else:
            _check(lib.svg_kmeans_loop_grouped(x.data_ptr(), _ptr(xsq), *cs, *outs, group, *tail), "svg_kmeans_loop_grouped")
        return labels, cent, counts, n_it, sorted_idx
    if batch_strided:
        rc = lib.svg_kmeans_loop_strided(x.data_ptr(), int(x.stride(0)), *cs, *outs, *tail)
        _check(rc, "svg_kmeans_loop_strided")
        return labels, cent, counts, n_it, sorted_idx
    rc = lib.svg_kmeans_loop(x.data_ptr(), _ptr(xsq), *cs, *outs, *tail)
    _check(rc, "svg_kmeans_loop")
    return labels, cent, counts, n_it, sorted_idx


def kmeans_stepped_workspace_bytes(B: int, N: int, K: int, D: int, group: int) -> int:
    return int(load().svg_kmeans_stepped_workspace_bytes(B, N, K, D, group))


def kmeans_stepped_iterate(x: torch.Tensor, c_init: torch.Tensor, c_work_a: torch.Tensor, c_work_b: torch.Tensor, it: int,
                           maxima: torch.Tensor, group: int, ws: torch.Tensor) -> None:
    """svg_kmeans_stepped_iterate on the caller's buffers (the allocating side: svg/_kmeans_stepped.py KmeansSteppedSide).  x [B, N, D]:
    rows of a batch contiguous, batches x.stride(0) elements apart; maxima float32 [B // group], written."""
    _dev(c_init, c_work_a, c_work_b, maxima)
    _gpu(x, ws)
    B, N, D = x.shape
    K = c_init.shape[1]
    assert x.stride(2) == 1 and x.stride(1) == D and c_init.shape == c_work_a.shape == c_work_b.shape == (B, K, D)
    assert c_init.dtype == c_work_a.dtype == c_work_b.dtype == x.dtype
    _f32_vector("kmeans_stepped_iterate(maxima)", maxima, B // group)
    _check(load().svg_kmeans_stepped_iterate(x.data_ptr(), int(x.stride(0)), c_init.data_ptr(), c_work_a.data_ptr(), c_work_b.data_ptr(),
                                             int(it), maxima.data_ptr(), B, N, K, D, _dtype_code(x), int(group), ws.data_ptr(), ws.numel(),
                                             _stream()), "svg_kmeans_stepped_iterate")


def kmeans_stepped_commit(maxima: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor, sorted_idx: torch.Tensor, it: int, tol: float,
                          group: int, ws: torch.Tensor) -> None:
    """svg_kmeans_stepped_commit: the stopping rule of iteration `it` from whatever maxima [B // group] holds; labels / sorted_idx int32
    [B, N] and counts int32 [B, K] take the iteration's results for the groups still running."""
    _dev(maxima, labels, counts, sorted_idx)
    _gpu(ws)
    (B, N), K = labels.shape, counts.shape[1]
    assert labels.dtype == counts.dtype == sorted_idx.dtype == torch.int32 and sorted_idx.shape == (B, N) and counts.shape == (B, K)
    _f32_vector("kmeans_stepped_commit(maxima)", maxima, B // group)
    _check(load().svg_kmeans_stepped_commit(maxima.data_ptr(), labels.data_ptr(), counts.data_ptr(), sorted_idx.data_ptr(), int(it),
                                            float(tol), B, N, K, int(group), ws.data_ptr(), ws.numel(), _stream()), "svg_kmeans_stepped_commit")


def kmeans_stepped_finish(c_init: torch.Tensor, c_work_a: torch.Tensor, c_work_b: torch.Tensor, centroids_out: torch.Tensor,
                          n_iters: torch.Tensor, group: int, ws: torch.Tensor) -> None:
    """svg_kmeans_stepped_finish: every group's centroids [B, K, D] from the buffer its loop ended on, n_iters int32 [B // group]"""
    _dev(c_init, c_work_a, c_work_b, centroids_out, n_iters)
    _gpu(ws)
    B, K, D = c_init.shape
    assert c_work_a.shape == c_work_b.shape == centroids_out.shape == (B, K, D) and centroids_out.dtype == c_init.dtype
    assert n_iters.dtype == torch.int32 and n_iters.numel() == B // group
    _check(load().svg_kmeans_stepped_finish(c_init.data_ptr(), c_work_a.data_ptr(), c_work_b.data_ptr(), centroids_out.data_ptr(),
                                            n_iters.data_ptr(), B, K, D, _dtype_code(c_init), int(group), ws.data_ptr(), ws.numel(),
                                            _stream()), "svg_kmeans_stepped_finish")


def identify_dynamic_map(qc: torch.Tensor, kc: torch.Tensor, k_sizes: torch.Tensor, top_p: float,
                         preserve_length: int) -> torch.Tensor:
    """qc [BH, QC, D], kc [BH, KC, D], k_sizes int32 [BH, KC] -> bool [BH, QC, KC]"""
    lib = load()
    _dev(qc, kc, k_sizes)
    BH, QC, D = qc.shape
    KC = kc.shape[1]
    assert k_sizes.dtype == torch.int32 and k_sizes.shape == (BH, KC)
    out = empty((BH, QC, KC), dtype=torch.uint8, device=qc.device)
    rc = lib.svg_identify_dynamic_map(qc.data_ptr(), kc.data_ptr(), k_sizes.data_ptr(), out.data_ptr(), BH, QC, KC, D,
                                      _dtype_code(qc), float(top_p), int(preserve_length), _stream())
    _check(rc, "svg_identify_dynamic_map")
    return out.view(torch.bool)


def _f32_vector(what: str, t: torch.Tensor, n: int) -> None:
    if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous float32 tensor of {n} elements, got {t.dtype} {tuple(t.shape)}")


def identify_dynamic_map_per_head(qc: torch.Tensor, kc: torch.Tensor, k_sizes: torch.Tensor, top_p: torch.Tensor, preserve_length: int,
                                  out: torch.Tensor) -> torch.Tensor:
    """identify_dynamic_map with one top_p per head: top_p a device float32 tensor of BH elements (svg_identify_dynamic_map_per_head).
    out: uint8 [BH, QC, KC], written whole (the allocating caller is svg/kmeans_utils.py identify_dynamic_map) -> its bool view."""
    BH, QC, D = qc.shape
    KC = kc.shape[1]
    _f32_vector("identify_dynamic_map_per_head(top_p)", top_p, BH)
    if out.dtype != torch.uint8 or out.shape != (BH, QC, KC):
        raise ValueError(f"identify_dynamic_map_per_head(out): uint8 {(BH, QC, KC)}, got {out.dtype} {tuple(out.shape)}")
    lib = load()
    _dev(qc, kc, k_sizes, top_p, out)
    assert k_sizes.dtype == torch.int32 and k_sizes.shape == (BH, KC)
    rc = lib.svg_identify_dynamic_map_per_head(qc.data_ptr(), kc.data_ptr(), k_sizes.data_ptr(), out.data_ptr(), BH, QC, KC, D,
                                               _dtype_code(qc), top_p.data_ptr(), int(preserve_length), _stream())
    _check(rc, "svg_identify_dynamic_map_per_head")
    return out.view(torch.bool)


def _i32_vector(what: str, t: torch.Tensor, n: int) -> None:
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous int32 tensor of {n} elements, got {t.dtype} {tuple(t.shape)}")


def _kept_mass_operands(what: str, lse_sparse: torch.Tensor, rows: torch.Tensor, lse_dense: torch.Tensor, state: torch.Tensor, kept: torch.Tensor):
    """The operands both controller steps share, beside the knob's own state [BH] (its binding checks that): rows int64 [R], R in 1..64, and
    contiguous fp32 kept [BH], lse_sparse of BH * S elements (the kernel indexes it h * S + row) and lse_dense of BH * R.  -> (R, BH, S)"""
    if rows.dtype != torch.int64 or rows.dim() != 1 or not 1 <= rows.numel() <= 64:
        raise ValueError(f"{what}: rows is an int64 vector of 1 to 64 rows, got {rows.dtype} {tuple(rows.shape)}")
    R, BH = rows.numel(), state.numel()
    _f32_vector(f"{what}(kept)", kept, BH)
    if BH < 1 or lse_sparse.dtype != torch.float32 or lse_sparse.numel() % BH != 0 or lse_sparse.numel() == 0 or not lse_sparse.is_contiguous():
        raise ValueError(f"{what}: lse_sparse is a contiguous float32 [BH = {BH}, S], got {lse_sparse.dtype} "
                         f"{tuple(lse_sparse.shape)}, strides {tuple(lse_sparse.stride())}")
    _f32_vector(f"{what}(lse_dense)", lse_dense, BH * R)
    return R, BH, lse_sparse.numel() // BH


def top_p_update(lse_sparse: torch.Tensor, rows: torch.Tensor, lse_dense: torch.Tensor, top_p: torch.Tensor, kept: torch.Tensor,
                 target: float, gain_up: float, gain_down: float, band: float, p_min: float, p_max: float) -> None:
    """The controller step (svg_top_p_update): lse_sparse fp32 [BH, S] (any leading shape), rows device int64 [R], lse_dense fp32 [BH, R];
    kept fp32 [BH] is written, top_p fp32 [BH] stepped in place.  No allocation, no host synchronisation."""
    R, BH, S = _kept_mass_operands("top_p_update", lse_sparse, rows, lse_dense, top_p, kept)
    _f32_vector("top_p_update(top_p)", top_p, BH)
    lib = load()
    _dev(lse_sparse, rows, lse_dense, top_p, kept)
    rc = lib.svg_top_p_update(lse_sparse.data_ptr(), rows.data_ptr(), lse_dense.data_ptr(), R, BH, S, float(target), float(gain_up),
                              float(gain_down), float(band), float(p_min), float(p_max), kept.data_ptr(), top_p.data_ptr(), _stream())
    _check(rc, "svg_top_p_update")


def band_width_update(lse_sparse: torch.Tensor, rows: torch.Tensor, lse_dense: torch.Tensor, band: torch.Tensor, kept: torch.Tensor,
                      target: float, gain_up: float, gain_down: float, dead: float, quantum: int, band_min: int, band_max: int,
                      skip_flag: Optional[torch.Tensor] = None) -> None:
    """The controller step of SVG1's per-head band (svg_band_width_update), operands as top_p_update: kept fp32 [BH] is written, band int32
    [BH] stepped in place by whole quanta inside [band_min, band_max].  skip_flag (int32 [1] on the device, or None): non-zero leaves
    every band as it is — the dense_flag of the switched path.  No allocation, no host synchronisation."""
    R, BH, S = _kept_mass_operands("band_width_update", lse_sparse, rows, lse_dense, band, kept)
    _i32_vector("band_width_update(band)", band, BH)
    if skip_flag is not None and (skip_flag.dtype != torch.int32 or skip_flag.numel() < 1):
        raise ValueError(f"band_width_update: skip_flag is an int32 tensor of one element, got {skip_flag.dtype} {tuple(skip_flag.shape)}")
    lib = load()
    _dev(lse_sparse, rows, lse_dense, band, kept, skip_flag)
    rc = lib.svg_band_width_update(lse_sparse.data_ptr(), rows.data_ptr(), lse_dense.data_ptr(), R, BH, S, float(target), float(gain_up),
                                   float(gain_down), float(dead), int(quantum), int(band_min), int(band_max), _ptr(skip_flag),
                                   kept.data_ptr(), band.data_ptr(), _stream())
    _check(rc, "svg_band_width_update")


def map_density(block_map: torch.Tensor, q_sizes: torch.Tensor, k_sizes: torch.Tensor) -> torch.Tensor:
    lib = load()
    _dev(block_map, q_sizes, k_sizes)
    BH, QB, KB = block_map.shape
    out = empty((BH,), dtype=torch.float32, device=block_map.device)
    rc = lib.svg_map_density(block_map.data_ptr(), q_sizes.data_ptr(), k_sizes.data_ptr(), out.data_ptr(), BH, QB, KB,
                             _stream())
    _check(rc, "svg_map_density")
    return out


def debug_pp_trace():
    """Cycle trace of the ping-pong attention schedule (svg_debug_pp_trace): dict wave -> 8 tick sums, tiles, loop ticks."""
    buf = (C.c_uint64 * 104)()
    torch.cuda.synchronize()
    _check(load().svg_debug_pp_trace(C.cast(buf, C.c_void_p)), "svg_debug_pp_trace")
    v = list(buf)
    return {"waves": [v[8 * w: 8 * w + 8] for w in range(8)], "sv": [v[72 + 4 * w: 72 + 4 * w + 3] for w in range(8)],
            "tiles": v[64], "loop_ticks": v[65]}


def debug_wg_trace(n_workgroups: int):
    """Launch timeline of the traced two-phase kernel (svg_debug_wg_trace): int64 array [n, 6] =
    [entry, loop start, loop end, exit (s_memtime ticks), HW_ID, XCC_ID] per workgroup."""
    import numpy as np

    buf = np.zeros((n_workgroups, 6), dtype=np.uint64)
    torch.cuda.synchronize()
    _check(load().svg_debug_wg_trace(C.c_void_p(buf.ctypes.data), n_workgroups), "svg_debug_wg_trace")
    return buf


# ---- pre-attention prologue (svg/kernels/csrc/ops.h of the reference) ----
def _qk4(q, k):
    assert q.dim() == 4 and k.dim() == 4 and q.is_contiguous() and k.is_contiguous(), "q, k: contiguous [bsz, H, S, D]"
    assert q.shape[0] == k.shape[0] and q.shape[2] == k.shape[2] and q.shape[3] == k.shape[3] and q.dtype == k.dtype
    return q.shape[0], q.shape[1], k.shape[1], q.shape[2], q.shape[3]


def rms_norm_forward(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-5) -> None:
    """in place; x [m, n] (ref: ops.h:52-78)"""
    lib = load()
    _dev(x, weight)
    assert x.dim() == 2 and x.is_contiguous() and weight.shape == (x.shape[1],) and weight.dtype == x.dtype
    _check(lib.svg_rms_norm_forward(x.data_ptr(), weight.data_ptr(), x.shape[0], x.shape[1], _dtype_code(x), float(eps),
                                    _stream()), "svg_rms_norm_forward")


def layer_norm_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> None:
    """in place; x [m, n], eps = 1e-5 (ref: ops.h:19-44)"""
    lib = load()
    _dev(x, weight, bias)
    assert x.dim() == 2 and x.is_contiguous() and weight.shape == (x.shape[1],) and bias.shape == weight.shape
    assert weight.dtype == x.dtype and bias.dtype == x.dtype
    _check(lib.svg_layer_norm_forward(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), x.shape[0], x.shape[1],
                                      _dtype_code(x), _stream()), "svg_layer_norm_forward")


def _rope(fn_name: str, q, k, a, b, len_text_prompt: int, half: bool) -> None:
    lib = load()
    _dev(q, k, a, b)
    bsz, Hq, Hkv, S, D = _qk4(q, k)
    valid = S - int(len_text_prompt)
    assert valid > 0, "len_text_prompt must be smaller than the sequence"
    cols = D // 2 if half else D
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous() and b.is_contiguous()
    assert a.shape == (valid, cols) and b.shape == (valid, cols), f"rope tables must be [{valid}, {cols}]"
    _check(getattr(lib, fn_name)(q.data_ptr(), k.data_ptr(), a.data_ptr(), b.data_ptr(), bsz, Hq, Hkv, S, D, _dtype_code(q),
                                 int(len_text_prompt), _stream()), fn_name)


def apply_qk_rope_inplace_cossin(q, k, cos, sin, len_text_prompt: int) -> None:
    """ref: ops.h:80-136 — the FIRST len_text_prompt positions are skipped"""
    _rope("svg_apply_qk_rope_inplace_cossin", q, k, cos, sin, len_text_prompt, False)


def apply_qk_rope_inplace_cossin_txtlast(q, k, cos, sin, len_text_prompt: int) -> None:
    """ref: ops.h:138-196 — the LAST len_text_prompt positions are skipped"""
    _rope("svg_apply_qk_rope_inplace_cossin_txtlast", q, k, cos, sin, len_text_prompt, False)


def apply_qk_rope_inplace_cossin_complex(q, k, freqs_real, freqs_imag, len_text_prompt: int) -> None:
    """ref: ops.h:198-260 — complex multiply in fp64, tables [S - len_text_prompt, D / 2]"""
    _rope("svg_apply_qk_rope_inplace_cossin_complex", q, k, freqs_real, freqs_imag, len_text_prompt, True)


def qk_norm_rope(q, k=None, norm_kind: int = 0, q_weight=None, q_bias=None, k_weight=None, k_bias=None, eps: float = 1e-5,
                 rope_kind: int = 0, cos=None, sin=None, rope_lo: int = 0, rope_hi: Optional[int] = None,
                 q_scale: float = 1.0) -> None:
    """Fused in-place normalisation + rotary embedding of q and (optionally) k in one pass (svg_qk_norm_rope).
    rope_kind 0 none / 1 interleaved pairs / 2 complex pairs (tables [.., D / 2]) / 3 half-split (channel i against i + D / 2; tables
    [.., D] like kind 1, every column read).
    q_scale != 1: folded into the last rounding of q (svg_qk_norm_rope_qscale; softmax_q_scale(D) for band_attention(q_prescaled=True))."""
    lib = load()
    _dev(q, k, q_weight, q_bias, k_weight, k_bias, cos, sin)
    if k is not None:
        bsz, Hq, Hkv, S, D = _qk4(q, k)
    else:
        assert q.dim() == 4 and q.is_contiguous()
        (bsz, Hq, S, D), Hkv = q.shape, 0
    rope_hi = S if rope_hi is None else rope_hi
    if rope_kind:
        cols = D // 2 if rope_kind == 2 else D
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
        assert cos.shape == (rope_hi - rope_lo, cols) and sin.shape == cos.shape
    for w in (q_weight, q_bias, k_weight, k_bias):
        assert w is None or (w.dtype == q.dtype and w.shape == (D,) and w.is_contiguous())
    _check(lib.svg_qk_norm_rope_qscale(q.data_ptr(), _ptr(k), bsz, Hq, Hkv, S, D, _dtype_code(q), int(norm_kind), _ptr(q_weight),
                                       _ptr(q_bias), _ptr(k_weight), _ptr(k_bias), float(eps), int(rope_kind), _ptr(cos), _ptr(sin),
                                       int(rope_lo), int(rope_hi), float(q_scale), _stream()), "svg_qk_norm_rope")


def qk_norm_rope_transpose(q_in, k_in, heads_q: int, heads_k: int, norm_kind: int = 0, q_weight=None, q_bias=None, k_weight=None,
                           k_bias=None, eps: float = 1e-5, rope_kind: int = 0, cos=None, sin=None, rope_lo: int = 0,
                           rope_hi: Optional[int] = None, q_scale: float = 1.0):
    """q_in [bsz, S, Hq * D] (k_in [bsz, S, Hkv * D] or None) token-major -> new head-major tensors [bsz, H, S, D] with
    normalisation + rotary embedding applied in the same pass (svg_qk_norm_rope_transpose); rope_kind and q_scale as in qk_norm_rope."""
    lib = load()
    _dev(q_in, k_in, q_weight, q_bias, k_weight, k_bias, cos, sin)
    bsz, S, HD = q_in.shape
    D = HD // heads_q
    q_out = empty((bsz, heads_q, S, D), dtype=q_in.dtype, device=q_in.device)
    k_out = None
    if k_in is not None:
        assert k_in.shape == (bsz, S, heads_k * D) and k_in.dtype == q_in.dtype
        k_out = empty((bsz, heads_k, S, D), dtype=q_in.dtype, device=q_in.device)
    rope_hi = S if rope_hi is None else rope_hi
    if rope_kind:
        cols = D // 2 if rope_kind == 2 else D
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.shape == (rope_hi - rope_lo, cols) and sin.shape == cos.shape
    _check(lib.svg_qk_norm_rope_transpose_qscale(q_in.data_ptr(), _ptr(k_in), q_out.data_ptr(), _ptr(k_out), bsz, heads_q, heads_k, S,
                                                 D, _dtype_code(q_in), int(norm_kind), _ptr(q_weight), _ptr(q_bias), _ptr(k_weight),
                                                 _ptr(k_bias), float(eps), int(rope_kind), _ptr(cos), _ptr(sin), int(rope_lo),
                                                 int(rope_hi), float(q_scale), _stream()), "svg_qk_norm_rope_transpose")
    return q_out, k_out


class JointSegment(NamedTuple):
    """One stream of qk_norm_rope_transpose_joint: token-major projections [bsz, rows, heads * D] (k / v may be None when no segment has
    them) and the stream's own norm over head_dim (norm_kind 0 none / 1 rms / 2 layer; weights / biases [D] of the tensor dtype or None)."""
    q: Optional[torch.Tensor]
    k: Optional[torch.Tensor] = None
    v: Optional[torch.Tensor] = None
    norm_kind: int = 0
    q_weight: Optional[torch.Tensor] = None
    q_bias: Optional[torch.Tensor] = None
    k_weight: Optional[torch.Tensor] = None
    k_bias: Optional[torch.Tensor] = None
    eps: float = 1e-6


def qk_norm_rope_transpose_joint(segments: Sequence[JointSegment], heads: int, rope_kind: int = 0, cos=None, sin=None, rope_lo: int = 0,
                                 rope_hi: Optional[int] = None, q_scale: float = 1.0, with_v: bool = True):
    """Joint (MMDiT) prologue in one launch (svg_qk_norm_rope_transpose_joint): one or two token-major streams -> head-major
    (q, k, v) [bsz, heads, sum(rows), D], segment i filling its rows in order, each with its own norm; RoPE on JOINT positions
    [rope_lo, rope_hi) (tables [rope_hi - rope_lo, D], complex: [.., D / 2]); q_scale folded into q's last rounding; v transposed.
    Bit-identical to qk_norm_rope_transpose per segment + the transpose of v, concatenated along the rows.  Outputs of tensors the
    segments do not supply (and v when with_v is False) are None."""
    lib = load()
    segs = list(segments)
    if not 1 <= len(segs) <= 2:
        raise ValueError(f"qk_norm_rope_transpose_joint takes 1 or 2 segments, got {len(segs)}")
    ref = segs[0].q if segs[0].q is not None else segs[0].k
    bsz, _, HD = ref.shape
    D = HD // heads
    for sg in segs:
        _dev(sg.q, sg.k, sg.v if with_v else None, sg.q_weight, sg.q_bias, sg.k_weight, sg.k_bias)
        for t in (sg.q, sg.k, sg.v):
            assert t is None or (t.dim() == 3 and t.shape[0] == bsz and t.shape[2] == HD and t.dtype == ref.dtype), "segment tensors disagree"
    rows = [(sg.q if sg.q is not None else sg.k).shape[1] for sg in segs]
    S = sum(rows)
    mk = lambda on: empty((bsz, heads, S, D), dtype=ref.dtype, device=ref.device) if on else None  # noqa: E731
    q_out, k_out = mk(segs[0].q is not None), mk(segs[0].k is not None)
    v_out = mk(with_v and segs[0].v is not None)
    rope_hi = S if rope_hi is None else rope_hi
    if rope_kind:
        _dev(cos, sin)
        cols = D // 2 if rope_kind == 2 else D
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.shape == (rope_hi - rope_lo, cols) and sin.shape == cos.shape
    arr = (PrologueSegment * len(segs))()
    for a, sg, n in zip(arr, segs, rows):
        a.q_in, a.k_in, a.v_in = _ptr(sg.q), _ptr(sg.k), _ptr(sg.v) if with_v else None
        a.rows, a.norm_kind, a.eps = n, int(sg.norm_kind), float(sg.eps)
        a.q_weight, a.q_bias, a.k_weight, a.k_bias = _ptr(sg.q_weight), _ptr(sg.q_bias), _ptr(sg.k_weight), _ptr(sg.k_bias)
    _check(lib.svg_qk_norm_rope_transpose_joint(arr, len(segs), _ptr(q_out), _ptr(k_out), _ptr(v_out), bsz, heads, D, _dtype_code(ref),
                                                int(rope_kind), _ptr(cos), _ptr(sin), int(rope_lo), int(rope_hi), float(q_scale), _stream()),
           "svg_qk_norm_rope_transpose_joint")
    return q_out, k_out, v_out


def rmsnorm_rope_transpose(q_in, k_in, v_in, heads: int, q_weight=None, k_weight=None, eps: float = 1e-6, rope_kind: int = 0, cos=None,
                           sin=None, rope_lo: int = 0, rope_hi: Optional[int] = None, q_scale: float = 1.0):
    """The Wan 2.1 prologue in one pass (svg_rmsnorm_rope_transpose): q_in / k_in / v_in [bsz, S, heads * D] token-major (k_in, v_in may be
    None) -> (q, k, v) head-major [bsz, heads, S, D]; q and k RMS-normalised ACROSS ALL HEADS (the reference's Triton form, weights [heads * D])
    and rotated, v transposed.  Bit-identical to rmsnorm_forward -> qk_norm_rope_transpose(norm 0, rope) and a transpose of v."""
    lib = load()
    _dev(q_in, k_in, v_in, q_weight, k_weight, cos, sin)
    bsz, S, HD = q_in.shape
    D = HD // heads
    assert q_in.is_contiguous() and all(t is None or (t.shape == q_in.shape and t.dtype == q_in.dtype and t.is_contiguous()) for t in (k_in, v_in))
    mk = lambda t: None if t is None else empty((bsz, heads, S, D), dtype=q_in.dtype, device=q_in.device)  # noqa: E731
    q_out, k_out, v_out = mk(q_in), mk(k_in), mk(v_in)
    w = q_weight if q_weight is not None else k_weight
    wdt = _GLUE_DT[w.dtype] if w is not None else 2
    for t in (q_weight, k_weight):
        assert t is None or (t.shape == (HD,) and t.is_contiguous() and _GLUE_DT[t.dtype] == wdt)
    rope_hi = S if rope_hi is None else rope_hi
    if rope_kind:
        cols = D // 2 if rope_kind == 2 else D
        assert cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.shape == (rope_hi - rope_lo, cols) and sin.shape == cos.shape
    _check(lib.svg_rmsnorm_rope_transpose(q_in.data_ptr(), _ptr(k_in), _ptr(v_in), q_out.data_ptr(), _ptr(k_out), _ptr(v_out), bsz, heads, S, D,
                                          _dtype_code(q_in), _ptr(q_weight), _ptr(k_weight), wdt, float(eps), int(rope_kind), _ptr(cos),
                                          _ptr(sin), int(rope_lo), int(rope_hi), float(q_scale), _stream()), "svg_rmsnorm_rope_transpose")
    return q_out, k_out, v_out


# ---- transformer-block glue (svg/kernels/triton/{layernorm,modulate}.py of the reference) ----
_GLUE_DT = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}


def _rows(x: torch.Tensor):
    assert x.dim() in (2, 3) and x.is_contiguous(), "expected contiguous [M, N] or [B, S, N]"
    N = x.shape[-1]
    return x.numel() // N, N, (x.shape[1] if x.dim() == 3 else x.numel() // N)


def _per_batch(t: torch.Tensor, x: torch.Tensor, N: int) -> torch.Tensor:
    """scale / shift / gate: fp32, one row of N per batch element ([N], [1, N], [B, 1, N], [B, N])"""
    B = x.shape[0] if x.dim() == 3 else 1
    t = t.detach().to(torch.float32).reshape(-1, N)
    if t.shape[0] == 1 and B > 1:
        t = t.expand(B, N)
    assert t.shape == (B, N), f"modulation tensor must broadcast to [{B}, {N}]"
    return t.contiguous()


def layernorm_forward(x, weight=None, bias=None, eps: float = 1e-5, out_dtype=torch.float32, reference_padding: bool = False) -> torch.Tensor:
    """fp32 LayerNorm of the rows of x.  reference_padding: the variance of the reference's Triton kernels as they are — the zero
    padding of a row up to the next power of two counted in (svg_layernorm_forward_ex; include/svg_attn.h) — instead of LayerNorm's."""
    lib = load()
    _dev(x, weight, bias)
    M, N, _ = _rows(x)
    y = empty(x.shape, dtype=out_dtype, device=x.device)
    wdt = _GLUE_DT[weight.dtype] if weight is not None else 2
    if weight is not None:
        assert bias is not None and weight.shape == (N,) and bias.shape == (N,) and bias.dtype == weight.dtype
    _check(lib.svg_layernorm_forward_ex(x.data_ptr(), y.data_ptr(), _ptr(weight), _ptr(bias), M, N, _GLUE_DT[x.dtype],
                                        _GLUE_DT[out_dtype], wdt, float(eps), int(bool(reference_padding)), _stream()),
           "svg_layernorm_forward_ex")
    return y


def rmsnorm_forward(x, weight=None, eps: float = 1e-6, out_dtype=None) -> torch.Tensor:
    """RMSNorm of the rows of x ([M, N] or [B, S, N]) in the reference's Triton form: fp32, x * rstd * w, one rounding
    (svg_rmsnorm_forward); out_dtype defaults to x.dtype."""
    lib = load()
    _dev(x, weight)
    M, N, _ = _rows(x)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    y = empty(x.shape, dtype=out_dtype, device=x.device)
    wdt = _GLUE_DT[weight.dtype] if weight is not None else 2
    if weight is not None:
        assert weight.shape == (N,) and weight.is_contiguous()
    _check(lib.svg_rmsnorm_forward(x.data_ptr(), y.data_ptr(), _ptr(weight), M, N, _GLUE_DT[x.dtype], _GLUE_DT[out_dtype], wdt,
                                   float(eps), _stream()), "svg_rmsnorm_forward")
    return y


def modulate_shift_forward(x, scale, shift, out_dtype=torch.float32) -> torch.Tensor:
    lib = load()
    _dev(x)
    M, N, rpb = _rows(x)
    sc, sh = _per_batch(scale, x, N), _per_batch(shift, x, N)
    _dev(sc, sh)
    y = empty(x.shape, dtype=out_dtype, device=x.device)
    _check(lib.svg_modulate_shift_forward(x.data_ptr(), y.data_ptr(), sc.data_ptr(), sh.data_ptr(), M, N, rpb, _GLUE_DT[x.dtype],
                                          _GLUE_DT[out_dtype], _stream()), "svg_modulate_shift_forward")
    return y


def modulate_gate_residual_forward(residual, x, gate, out_dtype=torch.float32) -> torch.Tensor:
    lib = load()
    _dev(residual, x)
    assert residual.shape == x.shape
    M, N, rpb = _rows(x)
    _rows(residual)
    g = _per_batch(gate, x, N)
    _dev(g)
    y = empty(x.shape, dtype=out_dtype, device=x.device)
    _check(lib.svg_modulate_gate_residual_forward(residual.data_ptr(), x.data_ptr(), g.data_ptr(), y.data_ptr(), M, N, rpb,
                                                  _GLUE_DT[residual.dtype], _GLUE_DT[x.dtype], _GLUE_DT[out_dtype], _stream()),
           "svg_modulate_gate_residual_forward")
    return y


def layernorm_modulate_forward(x, weight=None, bias=None, scale=None, shift=None, eps: float = 1e-5, out_dtype=None,
                               reference_padding: bool = False) -> torch.Tensor:
    """Fused fp32 LayerNorm (+ affine) (+ y * (1 + scale) + shift), one pass; out_dtype defaults to x.dtype.
    reference_padding: see layernorm_forward."""
    lib = load()
    _dev(x, weight, bias)
    M, N, rpb = _rows(x)
    out_dtype = x.dtype if out_dtype is None else out_dtype
    sc = _per_batch(scale, x, N) if scale is not None else None
    sh = _per_batch(shift, x, N) if shift is not None else None
    _dev(sc, sh)
    wdt = _GLUE_DT[weight.dtype] if weight is not None else 2
    y = empty(x.shape, dtype=out_dtype, device=x.device)
    _check(lib.svg_layernorm_modulate_forward_ex(x.data_ptr(), y.data_ptr(), _ptr(weight), _ptr(bias), _ptr(sc), _ptr(sh), M, N, rpb,
                                                 _GLUE_DT[x.dtype], _GLUE_DT[out_dtype], wdt, float(eps), int(bool(reference_padding)),
                                                 _stream()),
           "svg_layernorm_modulate_forward_ex")
    return y


def bsr_to_block_map(indptr: torch.Tensor, indices: torch.Tensor, MB: int, NB: int, row_block: int, col_block: int,
                     len_text: int, heads: int):
    """BSR over uniform blocks -> (block_map uint8 [heads, MB+1, NB+1], q_sizes int32 [heads, MB+1], k_sizes int32 [heads, NB+1])
    with the text block in front (svg_bsr_to_block_map)."""
    lib = load()
    _dev(indptr, indices)
    assert indptr.dtype == torch.int32 and indices.dtype == torch.int32 and indptr.numel() == MB + 1
    dev = indptr.device
    bm = empty((heads, MB + 1, NB + 1), dtype=torch.uint8, device=dev)
    qs = empty((heads, MB + 1), dtype=torch.int32, device=dev)
    ks = empty((heads, NB + 1), dtype=torch.int32, device=dev)
    _check(lib.svg_bsr_to_block_map(indptr.data_ptr(), indices.data_ptr(), MB, NB, row_block, col_block, len_text, heads,
                                    bm.data_ptr(), qs.data_ptr(), ks.data_ptr(), _stream()), "svg_bsr_to_block_map")
    return bm, qs, ks


# ------------------------------------------------------------------------------------------------------
# svg_copy_boxes (include/svg_attn_shard_exchange.h): the pack / unpack layouts either side of the two all-to-all exchanges of a
# token-sharded layer-call (svg/distributed.py run_token_sharded).  One builder per layout returns its boxes from (cfg, head counts, row
# ranges, strides); copy_boxes runs them as one launch, copy_boxes_torch is the torch statement of the same copies — what CPU tensors take
# and what the GPU test compares the kernel with.
# ------------------------------------------------------------------------------------------------------
COPY_MAX_TENSORS, COPY_MAX_BOXES = 3, 16


class Box(NamedTuple):
    """one svg_copy_box_t: rows of D contiguous elements, offsets and strides in elements from the tensors' first elements"""
    src_offset: int
    dst_offset: int
    extent: tuple        # (n0, n1, n2): the kernel's tiles run along n2 — the rows of a shard
    src_stride: tuple
    dst_stride: tuple


def inbound_pack_boxes(cfg: int, head_counts: Sequence[int], n_rows: int, D: int, strides: Sequence[int]):
    """Before the inbound exchange: x [cfg, H, S_r, D] with element strides `strides` = (video, head, row) -> the send buffer, one block
    [cfg, H_j, S_r, D] per destination rank j, in rank order."""
    boxes, h0, off = [], 0, 0
    for hj in head_counts:
        boxes.append(Box(h0 * strides[1], off, (cfg, hj, n_rows), tuple(strides), (hj * n_rows * D, n_rows * D, D)))
        h0, off = h0 + hj, off + cfg * hj * n_rows * D
    return boxes


def inbound_unpack_boxes(cfg: int, n_heads_local: int, row_ranges: Sequence[Sequence[int]], D: int):
    """Behind the inbound exchange: the receive buffer, one block [cfg, H_l, S_i, D] per source rank i -> contiguous [cfg, H_l, S, D], the
    rows of rank i at row_ranges[i] = (a_i, b_i)."""
    S = row_ranges[-1][1]
    boxes, off = [], 0
    for a, b in row_ranges:
        n = b - a
        boxes.append(Box(off, a * D, (cfg, n_heads_local, n), (n_heads_local * n * D, n * D, D), (n_heads_local * S * D, S * D, D)))
        off += cfg * n_heads_local * n * D
    return boxes


def outbound_pack_boxes(cfg: int, n_heads_local: int, row_ranges: Sequence[Sequence[int]], D: int, strides: Sequence[int]):
    """Before the outbound exchange: o [cfg, H_l, S, D] with element strides `strides` = (video, head, row) — head-major or token-major
    storage — -> the send buffer, one token-major block [cfg, S_j, H_l, D] per destination rank j."""
    boxes, off = [], 0
    for a, b in row_ranges:
        n = b - a
        boxes.append(Box(a * strides[2], off, (cfg, n_heads_local, n), tuple(strides), (n * n_heads_local * D, D, n_heads_local * D)))
        off += cfg * n * n_heads_local * D
    return boxes


def outbound_unpack_boxes(cfg: int, head_counts: Sequence[int], n_rows: int, D: int):
    """Behind the outbound exchange: the receive buffer, one block [cfg, S_r, H_i, D] per source rank i -> the storage [cfg, S_r, H, D]
    (the heads of rank i interleaved at their place of every row)."""
    H = sum(head_counts)
    boxes, h0, off = [], 0, 0
    for hi in head_counts:
        boxes.append(Box(off, h0 * D, (cfg, hi, n_rows), (n_rows * hi * D, D, hi * D), (n_rows * H * D, D, H * D)))
        h0, off = h0 + hi, off + cfg * n_rows * hi * D
    return boxes


def _elements_behind(t: torch.Tensor) -> int:
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _check_boxes(src: torch.Tensor, dst: torch.Tensor, boxes: Sequence[Box], D: int) -> None:
    """every row of every box inside the two allocations (ValueError before anything runs: the kernel itself cannot know)"""
    if src.dtype != dst.dtype or src.device != dst.device:
        raise ValueError(f"copy_boxes: source {src.dtype} on {src.device}, destination {dst.dtype} on {dst.device}")
    for b in boxes:
        if min(b.extent) < 0 or min(b.src_stride) < 0 or min(b.dst_stride) < 0 or b.src_offset < 0 or b.dst_offset < 0:
            raise ValueError(f"copy_boxes: negative member in {b}")
        if min(b.extent) == 0:
            continue
        for t, off, st, side in ((src, b.src_offset, b.src_stride, "source"), (dst, b.dst_offset, b.dst_stride, "destination")):
            last = off + sum((n - 1) * s for n, s in zip(b.extent, st)) + D
            if last > _elements_behind(t):
                raise ValueError(f"copy_boxes: {b} ends {last} elements behind the {side}'s first, which has {_elements_behind(t)}")


def copy_boxes_torch(pairs, boxes: Sequence[Box], D: int, ranges=None) -> None:
    """The torch statement of copy_boxes: one strided copy_ per tensor and box."""
    for i, (src, dst) in enumerate(pairs):
        b0, nb = ranges[i] if ranges is not None else (0, len(boxes))
        _check_boxes(src, dst, boxes[b0:b0 + nb], D)
        for b in boxes[b0:b0 + nb]:
            if min(b.extent) == 0:
                continue
            d = torch.as_strided(dst, tuple(b.extent) + (D,), tuple(b.dst_stride) + (1,), dst.storage_offset() + b.dst_offset)
            d.copy_(torch.as_strided(src, tuple(b.extent) + (D,), tuple(b.src_stride) + (1,), src.storage_offset() + b.src_offset))


def copy_boxes(pairs, boxes: Sequence[Box], D: int, ranges=None) -> None:
    """svg_copy_boxes: pairs = up to COPY_MAX_TENSORS (src, dst) tensors (any shape: the boxes address elements behind each tensor's first),
    boxes = up to COPY_MAX_BOXES Box; ranges[i] = (first box, count) of pair i (default: every pair copies every box).  ONE launch.  CPU
    tensors take copy_boxes_torch."""
    pairs = list(pairs)
    if not pairs[0][0].is_cuda:
        return copy_boxes_torch(pairs, boxes, D, ranges)
    lib = load()
    for i, (src, dst) in enumerate(pairs):
        _gpu(src, dst)
        b0, nb = ranges[i] if ranges is not None else (0, len(boxes))
        _check_boxes(src, dst, boxes[b0:b0 + nb], D)
    ts = (CopyTensor * len(pairs))()
    for i, (src, dst) in enumerate(pairs):
        b0, nb = ranges[i] if ranges is not None else (0, len(boxes))
        ts[i] = CopyTensor(src.data_ptr(), dst.data_ptr(), b0, nb)
    bs = (CopyBox * len(boxes))()
    for i, b in enumerate(boxes):
        bs[i] = CopyBox(b.src_offset, b.dst_offset, (C.c_int32 * 3)(*b.extent), 0, (C.c_int64 * 3)(*b.src_stride), (C.c_int64 * 3)(*b.dst_stride))
    _check(lib.svg_copy_boxes(ts, len(pairs), bs, len(boxes), D, _dtype_code(pairs[0][0]), _stream()), "svg_copy_boxes")


# The layouts that run through svg_copy_boxes on the GPU; one that is not listed takes the torch copies (tools/ab_token_shards.py compares
# the two, profiles/token_shards_ab.jsonl holds what it found).
COPY_BOX_LAYOUTS = {"inbound_pack", "inbound_unpack", "outbound_pack", "outbound_unpack"}


def copy_box_jobs(jobs, D: int, layout: str) -> int:
    """jobs = [(src, dst, boxes)]: the copies of one step of a layer-call, in as few launches as COPY_MAX_TENSORS and COPY_MAX_BOXES allow —
    one where the world has at most COPY_MAX_BOXES ranks (tensors with equal boxes share them; a tensor with strides of its own, a v that
    is a view of a fused projection, brings its own).  -> launches (the torch statement: copies).  A tensor without elements is skipped."""
    jobs = [(s, d, list(b)) for s, d, b in jobs if s.numel() and d.numel() and any(min(x.extent) > 0 for x in b)]
    if not jobs:
        return 0
    native = jobs[0][0].is_cuda and layout in COPY_BOX_LAYOUTS
    if not native:
        for s, d, b in jobs:
            copy_boxes_torch([(s, d)], b, D)
        return sum(len(b) for _, _, b in jobs)
    # a tensor with more boxes than one launch takes is several jobs; the first COPY_MAX_BOXES boxes of every tensor first, so that tensors
    # with equal boxes still share them
    most = max(len(b) for _, _, b in jobs)
    chunks = [(s, d, b[i:i + COPY_MAX_BOXES]) for i in range(0, most, COPY_MAX_BOXES) for s, d, b in jobs if b[i:i + COPY_MAX_BOXES]]
    launches, pairs, boxes, ranges = 0, [], [], []

    def flush():
        nonlocal launches, pairs, boxes, ranges
        if pairs:
            copy_boxes(pairs, boxes, D, ranges)
            launches += 1
        pairs, boxes, ranges = [], [], []

    for s, d, b in chunks:
        at = next((r for r in ranges if boxes[r[0]:r[0] + r[1]] == b), None)
        if len(pairs) == COPY_MAX_TENSORS or (at is None and len(boxes) + len(b) > COPY_MAX_BOXES):
            flush()
            at = None
        if at is None:
            at = (len(boxes), len(b))
            boxes += b
        pairs.append((s, d))
        ranges.append(at)
    flush()
    return launches


def __getattr__(name: str):
    """kmeans_centre, kmeans_assign_e4m3, kmeans_loop_e4m3: the allocating wrappers of include/svg_attn_kmeans_e4m3.h live in
    svg/_kmeans_e4m3.py (a module of its own like svg/_kmeans_stepped.py; their poison rows: tests/test_gpu_kmeans_e4m3.py) and are
    attributes of this module all the same."""
    if name in ("kmeans_centre", "kmeans_assign_e4m3", "kmeans_loop_e4m3"):
        from . import _kmeans_e4m3

        return getattr(_kmeans_e4m3, name)
    if name in ("cluster_means", "centroid_tail_attention"):   # (include/svg_attn_centroid_tail.h, likewise: svg/_centroid_tail.py)
        from . import _centroid_tail

        return getattr(_centroid_tail, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
