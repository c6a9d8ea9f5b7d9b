"""Cosmos attention processors — same class names / class-level configuration / call protocol as the reference module
svg/models/cosmos/attention.py (`proc(attn, hidden_states, encoder_hidden_states, attention_mask, image_rotary_emb, timestep)`
-> hidden_states).  The sparse core (online profiler, band attention with fused layout transformation, SVG2) is the Wan one:
the reference's cosmos/utils.py equals wan/utils.py and both `attention_core_logic`s are the same code."""
from __future__ import annotations

from typing import Optional

import torch

from ...timer import time_logging_decorator
from .. import _core
from ..wan.attention import (  # noqa: F401
    WanAttn_SAPAttn_Processor,
    WanAttn_SVGAttn_Processor2_0,
    prepare_flashinfer_attention,
    prepare_flexattention,
)


def apply_rotary_emb_half(x: torch.Tensor, freqs_cis) -> torch.Tensor:
    """diffusers `apply_rotary_emb(use_real=True, use_real_unbind_dim=-2)` (ref: cosmos/attention.py:61-66): the channel
    halves are the real / imaginary parts, cos / sin: [S, D]."""
    cos, sin = freqs_cis
    cos, sin = cos[None, None].to(x.device), sin[None, None].to(x.device)
    x_real, x_imag = x.reshape(*x.shape[:-1], 2, -1).unbind(-2)
    x_rot = torch.cat([-x_imag, x_real], dim=-1)
    return (x.float() * cos + x_rot.float() * sin).to(x.dtype)


class _CosmosPlumbing:
    """QKV / per-head RMSNorm / half-split RoPE / output projection of the Cosmos processors (ref :40-124)."""

    frame_shard_form = False   # (svg.distributed.enable_frame_shards: HunyuanVideo and Wan only; refused in attention_core_logic)

    @time_logging_decorator("Level 2 - qkv")
    def get_qkv(self, attn, hidden_states, encoder_hidden_states):
        return attn.to_q(hidden_states), attn.to_k(encoder_hidden_states), attn.to_v(encoder_hidden_states)

    @time_logging_decorator("Level 2 - transpose")
    def get_transpose_qkv(self, attn, query, key, value):
        return tuple(x.unflatten(2, (attn.heads, -1)).transpose(1, 2).contiguous() for x in (query, key, value))

    @time_logging_decorator("Level 2 - qk_norm")
    def get_qk_norm(self, attn, query, key):
        nq, nk = getattr(attn, "norm_q", None), getattr(attn, "norm_k", None)
        if _core.qk_norm_inplace(nq, nk, query, key):      # per-head RMSNorm on libsvgattn (GPU tensors)
            return query, key
        return (nq(query) if nq is not None else query), (nk(key) if nk is not None else key)

    @time_logging_decorator("Level 2 - rotary_emb")
    def get_rotary_emb(self, query, key, image_rotary_emb):
        if image_rotary_emb is not None:
            query, key = apply_rotary_emb_half(query, image_rotary_emb), apply_rotary_emb_half(key, image_rotary_emb)
        return query, key

    # on the GPU: transpose + qk_norm + rotary_emb as ONE pass over q and k (svg_qk_norm_rope_transpose, rope_kind 3), v read in place where
    # to_v wrote it; the cross call: one norm-only transpose pass per tensor.  False: the staged steps above, as the reference runs them
    fused_prologue = True

    @time_logging_decorator("Level 2 - transpose + qk_norm + rotary_emb (fused)")
    def get_fused_prologue(self, attn, query, key, value, image_rotary_emb, cross: bool):
        """get_transpose_qkv -> get_qk_norm -> get_rotary_emb in one kernel (bit-identical to the three steps; ref :40-124): returns
        (q, k, v) head-major — q and k contiguous, v possibly the head view of the projection's output — or None when the pass does not
        apply (CPU tensors, a norm module _norm_desc does not recognise, a table of another shape, ...): the caller runs the three steps."""
        if not self.fused_prologue or not all(t.is_cuda for t in (query, key, value)):
            return None
        nq, nk = getattr(attn, "norm_q", None), getattr(attn, "norm_k", None)
        if nq is None or nk is None:
            return None
        H = attn.heads
        if not cross:
            if image_rotary_emb is None:
                return None
            cos, sin = image_rotary_emb
            # (q_scale stays 1: prescale_q is not wired for Cosmos)
            return _core.qkv_from_projections(query, key, value, H, nq, nk, cos, sin, 0, query.shape[1], half_split=True)
        # cross call: Sq != Skv, one pass per tensor; the conditions under which the staged steps run the in-place HIP norm (qk_norm_inplace)
        if image_rotary_emb is not None:
            return None
        ts = (query, key, value)
        if not all(t.dim() == 3 and t.is_contiguous() and t.dtype == query.dtype and t.shape[-1] == query.shape[-1] for t in ts):
            return None
        D = query.shape[-1] // H
        if query.dtype not in (torch.bfloat16, torch.float16) or D not in _core._FAST_DIMS or H * D != query.shape[-1]:
            return None
        dq, dk = _core._norm_desc(nq, D, query.dtype, query.device), _core._norm_desc(nk, D, key.dtype, key.device)
        if dq is None or dk is None or dq[0] != dk[0] or dq[3] != dk[3]:
            return None
        q, _ = _core._native.qk_norm_rope_transpose(query, None, H, 0, dq[0], dq[1], dq[2], None, None, dq[3])
        k, _ = _core._native.qk_norm_rope_transpose(key, None, H, 0, dk[0], dk[1], dk[2], None, None, dk[3])
        # v as a head view: svg_cross_attention* and SDPA both take strided operands (as the Wan cross branch passes it)
        return q, k, value.unflatten(2, (H, -1)).transpose(1, 2)

    @time_logging_decorator("Level 2 - output")
    def get_o(self, attn, query, hidden_states):
        return attn.to_out[1](attn.to_out[0](hidden_states))

    def __call__(self, attn, hidden_states: torch.Tensor, encoder_hidden_states: Optional[torch.Tensor] = None,
                 attention_mask: Optional[torch.Tensor] = None, image_rotary_emb=None, timestep=None):
        cross = encoder_hidden_states is not None
        if timestep is None and not cross:
            from ..context import current_timestep

            timestep = current_timestep()
        if encoder_hidden_states is None:
            encoder_hidden_states = hidden_states
        query, key, value = self.get_qkv(attn, hidden_states, encoder_hidden_states)
        fused = self.get_fused_prologue(attn, query, key, value, image_rotary_emb, cross)
        if fused is not None:
            query, key, value = fused
        else:
            query, key, value = self.get_transpose_qkv(attn, query, key, value)
            query, key = self.get_qk_norm(attn, query, key)
            query, key = self.get_rotary_emb(query, key, image_rotary_emb)
        assert query.shape[3] == key.shape[3] == value.shape[3], "Does not support GQA"
        if cross and attention_mask is not None:   # ... with the text key-padding mask (ref :104-110): each video's key window, else SDPA
            hidden_states = _core.cross_attention_key_masked(query, key, value, attention_mask)
        elif cross:   # cross attention in Cosmos (ref :104-107): svg_cross_attention, SDPA where that does not apply
            hidden_states = _core.cross_attention(query, key, value, attention_mask)
        elif timestep is None:   # (SDPA; in token-shard mode the rows of the other ranks are keys too: _core.dense_attention)
            hidden_states = _core.self_attention_without_timestep(query, key, value, attention_mask, self.geometry())
        else:
            # (v may be the head view of to_v's output: the attention kernels read it in place, as from the Wan processors)
            assert query.is_contiguous() and key.is_contiguous() and value.stride(-1) == 1, "Query, key must be contiguous, value row-contiguous"
            hidden_states = self.attention_core_logic(query, key, value, timestep)
        hidden_states = hidden_states.transpose(1, 2).flatten(2, 3).type_as(query)
        return self.get_o(attn, query, hidden_states)


class Cosmos_SVG_AttnProcessor2_0(_CosmosPlumbing, WanAttn_SVGAttn_Processor2_0):
    """Sparse VideoGen 1 for Cosmos (ref: cosmos/attention.py:30-238)."""


class Cosmos_SAPAttn_Processor(_CosmosPlumbing, WanAttn_SAPAttn_Processor):
    """Sparse VideoGen 2 for Cosmos (ref: cosmos/attention.py:289-469)."""

    kmeans_e4m3 = False   # (its own switch, as on the Wan and HunyuanVideo SAP processors)
    centroid_tail = False   # (likewise)
