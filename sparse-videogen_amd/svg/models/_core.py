"""Model-independent attention core of the SVG1 / SVG2 processors.

The three model packages (hyvideo, wan, cog) keep the reference's processor classes and call into these functions from
their `attention_core_logic`.  On GPU tensors everything below is libsvgattn (HIP); on CPU tensors only the DENSE branch
exists (torch SDPA — the reference's own CPU-capable path, e.g. svg/models/wan/attention.py:279-281) and the sparse
branch raises: there is no CPU fallback for the sparse hot path.
"""
from __future__ import annotations

import contextlib
import dataclasses
import json
import weakref
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F

from .. import _native
from .. import distributed as _dist
from .. import kmeans_utils as _kmeans_utils
from .._kmeans_stepped import KmeansSteppedSide
from ..kmeans_utils import batch_kmeans_Euclid, density_calculation, identify_dynamic_map
from ..timer import time_logging_decorator


# ---------------------------------------------------------------------------------------------------------------
# precision of the sparse attention kernels: "bf16" (the input dtype: bf16 / fp16 MFMA, default) or "fp8" (e4m3 QK^T / PV,
# svg_band_attention_fp8 / svg_varblock_attention_fp8; head_dim 128 only — other head sizes stay on the 16-bit kernels).
# No reference counterpart (the reference lists fp8 attention as future work, README.md:117): an opt-in of this package.
# ---------------------------------------------------------------------------------------------------------------
_ATTENTION_DTYPE = {"value": "bf16"}


def set_attention_dtype(name: str) -> None:
    assert name in ("bf16", "fp8"), name
    _ATTENTION_DTYPE["value"] = name


def attention_dtype() -> str:
    return _ATTENTION_DTYPE["value"]


def _use_fp8(q: torch.Tensor) -> bool:
    return _ATTENTION_DTYPE["value"] == "fp8" and q.shape[-1] == 128


@dataclass
class Geometry:
    """Token layout of one model: [text?][video F*P][text?]"""

    context_length: int
    num_frame: int
    frame_size: int
    text_first: bool = False

    @property
    def video_length(self) -> int:
        return self.num_frame * self.frame_size

    @property
    def vid0(self) -> int:
        return self.context_length if self.text_first else 0

    @property
    def seq_len(self) -> int:
        return self.context_length + self.video_length


def is_full_attention(layer_idx: int, timestep, first_layers_fp, first_times_fp) -> bool:
    """ref: svg/models/hyvideo/attention.py:491-496 — dense for the first layers and the first (large) timesteps."""
    if layer_idx < first_layers_fp:
        return True
    from .context import timestep_value

    return timestep_value(timestep) > first_times_fp   # read back once per transformer forward, not once per layer



LN2 = 0.6931471805599453   # sm_scale of a kernel that applies sm_scale * log2(e) itself to a q that already carries the softmax scale

# Attention straight out of / into the projection layout (include/svg_attn.h, svg_attn_layout_t): q / k / v views that are not
# contiguous (a `proj(x).unflatten(2, (H, -1)).transpose(1, 2)` the caller did not copy) are read in place, and the result comes back as a
# [cfg, H, S, D] tensor STORED token-major, so that the processors' `hidden_states.transpose(1, 2).flatten(2, 3)` (ref:
# wan/attention.py:168-170, hyvideo/attention.py:202) is a view instead of a 2 S H D-byte copy.  The default schedules, one GPU (the head-sharded
# path gathers contiguous head slices); anything else falls back to copies inside svg/_native.py.  False: every output is contiguous.
TOKEN_MAJOR_IO = True

# The per-head band launches of `adaptive_band` as resident workgroups on the work queue (include/svg_attn_band_per_head_queue.h): the same
# bits, another mapping of q-tiles to workgroups.  Read at the adaptive branch of _svg1_layer_call, so every SVG1 processor with
# adaptive_band set follows it.  Off: the static mapping (figures: DESIGN §3.1.3 "One band per head"; on a real model unmeasured).
PER_HEAD_BAND_QUEUE = False


# ---------------------------------------------------------------------------------------------------------------
# Batches whose videos differ in their text length (HunyuanVideo: a list of prompts).  A length, or a mask built from one, may be given
# per video; neighbouring videos with equal values run as one group of heads, and a batch of equal values is ONE group and takes the
# single-mask path — the same entry point, the same launch.  Several groups are one svg_band_groups_attention call: a launch per group
# (DESIGN §3.1.3).
# ---------------------------------------------------------------------------------------------------------------
def _group_key(x):
    if isinstance(x, (tuple, list)):
        return tuple(_group_key(y) for y in x)
    return x.as_tuple() if hasattr(x, "as_tuple") else x


def video_groups(per_video, heads: int = 1):
    """(values, heads_per_group): neighbouring videos with equal values (ints, BandMasks, tuples of them) merged into one group of
    `heads` heads per video.  Equal NEIGHBOURS only — a group is a run of consecutive heads: (a, a, b, a) is three groups."""
    values, counts = [], []
    for x in per_video:
        if values and _group_key(values[-1]) == _group_key(x):
            counts[-1] += heads
        else:
            values.append(x)
            counts.append(heads)
    return values, counts


def per_video(x, cfg: int, what: str):
    """None when x is one value for the whole batch; otherwise the list of its `cfg` per-video values (ValueError for another count)."""
    if torch.is_tensor(x) and x.dim() >= 1:
        x = x.tolist()
    if not isinstance(x, (list, tuple)):
        return None
    if len(x) != cfg:
        raise ValueError(f"{what}: {len(x)} per-video values for a batch of {cfg} videos")
    return list(x)


def _no_sharding_of_groups(what: str) -> None:
    if _dist.token_shards_active():
        raise NotImplementedError(f"{what}: token-shard mode (svg.distributed.enable_token_shards) with per-video masks or lengths that differ "
                                  f"is not implemented; give every video the same length")
    if _dist.active():
        raise NotImplementedError(f"{what}: head sharding (svg.distributed) with per-video lengths that differ is not implemented; "
                                  f"run the batch on one GPU or give every video the same length")


def _dense_band_mask(S: int, valid_len) -> "_native.BandMask":
    real = S if valid_len is None else int(valid_len)
    return _native.BandMask(real_len=real, band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)


def _dense_sdpa(q, k, v, valid_len):
    S = q.shape[2]
    if valid_len is None or valid_len >= S:
        return F.scaled_dot_product_attention(q, k, v, dropout_p=0.0, is_causal=False)
    vl = int(valid_len)
    o = _native.empty_like(q)
    o[:, :, :vl] = F.scaled_dot_product_attention(q[:, :, :vl], k[:, :, :vl], v[:, :, :vl])
    o[:, :, vl:] = F.scaled_dot_product_attention(q[:, :, vl:], k[:, :, vl:], v[:, :, vl:])
    return o


def _state_kw(what: str, return_lse: bool, out_dtype, q_prescaled: bool, token_major_out: bool, fp8: bool = False, fused: bool = True) -> dict:
    """The keywords that ask a _native band call for the softmax state as well — (o, lse), or (o32, lse) with out_dtype=torch.float32: parts
    for merge_attention_states — or just the output layout without return_lse.  What has no such form raises here, before anything runs:
    there is no fall-back to a path without lse."""
    if not return_lse:
        if out_dtype is not None:
            raise ValueError(f"{what}(out_dtype={out_dtype}): fp32 rows go with return_lse=True")
        return dict(token_major_out=token_major_out)
    if q_prescaled or fp8 or not fused:
        raise ValueError(f"{what}(return_lse=True): the fused 16-bit path with a plain q; got q_prescaled = {q_prescaled}, fp8 = {fp8}, "
                         f"fused = {fused}")
    if _dist.active() or _dist.token_shards_active():
        raise NotImplementedError(f"{what}(return_lse=True): head sharding and token-shard mode (svg.distributed) exchange o only")
    return dict(return_lse=True, out_dtype=out_dtype, token_major_out=token_major_out and out_dtype is None)


# ---------------------------------------------------------------------------------------------------------------
# Frame-shard mode (svg.distributed.enable_frame_shards): q, k, v are [cfg, H, S_r, D] — ALL heads of this rank's rows
# frame_shard((geo.seq_len, geo.vid0, geo.num_frame, geo.frame_size), rank, world) — and every layer-call is one of the token-sharded
# schedules of svg/distributed.py.  What has no shard form is refused here, on the host, before any collective: every condition is the
# same on every rank, so all ranks raise together.
# ---------------------------------------------------------------------------------------------------------------
FRAME_SHARD_MAX_SAMPLED_ROWS = 64   # svg_sample_mse_shard_partial (include/svg_attn_profile_shard.h): sampled rows of one call


def rows_of_this_rank(what: str, geo: Geometry, shard_form: bool = True) -> int:
    """The rows an attention_core_logic receives: geo.seq_len — or, in frame-shard mode, the rows of this rank's frame_shard of the
    sequence.  shard_form False (the SVG2 processors, CogVideoX, Cosmos): frame-shard mode is refused.  In token-shard mode
    (svg.distributed.enable_token_shards): the rows of token_shard_range(geo.seq_len), for every processor."""
    if _dist.token_shards_active():
        a, b = _dist.token_shard_range(geo.seq_len)
        return b - a
    if not _dist.frame_shards_active():
        return geo.seq_len
    if not shard_form:
        raise NotImplementedError(f"{what}: frame-shard mode (svg.distributed.enable_frame_shards) exists for the SVG1 processors of "
                                  f"HunyuanVideo and Wan only")
    if geo.vid0 > 0:
        raise NotImplementedError(f"{what}: frame-shard mode needs the video at row 0; {geo.vid0} rows in front of it belong to no shard")
    group = _dist.frame_shards_group()
    shard = _dist.frame_shard((geo.seq_len, geo.vid0, geo.num_frame, geo.frame_size), torch.distributed.get_rank(group),
                              torch.distributed.get_world_size(group))
    return _native.band_shard_rows(shard, geo.frame_size)


def _one_mask(what: str, mask, cfg: int):
    """the one mask of a batch where per-video masks must be equal: frame-shard mode (and the adaptive band, which has refused others already)"""
    pm = per_video(mask, cfg, what)
    if pm is None:
        return mask
    vals, _ = video_groups(pm)
    if len(vals) > 1:
        raise NotImplementedError(f"{what}: frame-shard mode takes ONE mask (one text length) for the batch; per-video masks that differ "
                                  f"have no shard form")
    return vals[0]


def _frame_shard_setup(what: str, q, k, v, geo: Geometry, num_sampled_rows: Optional[int] = None, q_prescaled: bool = False,
                       return_lse: bool = False, out_dtype=None, fused: bool = True):
    """The refusals of frame-shard mode, each naming its limit; -> (geometry, group).  num_sampled_rows None: a call without the profiler
    (dense_attention), which also takes fp16."""
    if q_prescaled:
        raise ValueError(f"{what}: frame-shard mode takes a plain q (the shard kernels have no pre-scaled form); got q_prescaled = True")
    if _use_fp8(q):
        raise NotImplementedError(f"{what}: frame-shard mode runs the 16-bit kernels only; fp8 attention (set_attention_dtype('fp8')) has no "
                                  f"shard form")
    if not fused:
        raise NotImplementedError(f"{what}: frame-shard mode is the fused path only (fused=False places heads over the whole sequence)")
    if return_lse or out_dtype is not None:
        raise NotImplementedError(f"{what}: frame-shard mode returns o only (return_lse / out_dtype: the merged rows carry no lse)")
    dtypes = (torch.bfloat16,) if num_sampled_rows is not None else (torch.bfloat16, torch.float16)
    if q.dtype not in dtypes or k.dtype != q.dtype or v.dtype != q.dtype:
        raise NotImplementedError(f"{what}: frame-shard mode takes {' / '.join(str(d) for d in dtypes)} (the shard profiler is bfloat16 "
                                  f"only), got {q.dtype}")
    if q.shape[-1] != 128:
        raise NotImplementedError(f"{what}: frame-shard mode takes head_dim 128 (the shard kernels), got {q.shape[-1]}")
    if num_sampled_rows is not None and min(num_sampled_rows, geo.seq_len) > FRAME_SHARD_MAX_SAMPLED_ROWS:
        raise NotImplementedError(f"{what}: frame-shard mode samples at most {FRAME_SHARD_MAX_SAMPLED_ROWS} rows (the shard profiler), got "
                                  f"{min(num_sampled_rows, geo.seq_len)}")
    if geo.vid0 > 0:
        raise NotImplementedError(f"{what}: frame-shard mode needs the video at row 0; {geo.vid0} rows in front of it (CogVideoX's text) "
                                  f"belong to no shard")
    group = _dist.frame_shards_group()
    world = torch.distributed.get_world_size(group)
    if world > _dist.MERGE_MAX_PARTS:
        raise ValueError(f"{what}: frame-shard mode over {world} ranks, but merge_attention_states takes at most {_dist.MERGE_MAX_PARTS} parts — "
                         f"use a group of at most {_dist.MERGE_MAX_PARTS} ranks")
    _require_gpu(q, what)
    return (geo.seq_len, geo.vid0, geo.num_frame, geo.frame_size), group


@time_logging_decorator("Level 3 - Dense Flash Attention")
def dense_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, valid_len=None, q_prescaled: bool = False, return_lse: bool = False,
                    out_dtype=None, geometry: Optional[Geometry] = None, _local: bool = False):
    """Dense attention [cfg, H, S, D].  valid_len < S: two independent segments [0, valid) and [valid, S) — what the
    reference gets from flash_attn_varlen_func with cu_seqlens [0, valid, S] (hyvideo/attention.py:452-470).
    valid_len: one int for the batch, or a sequence of cfg ints, one per video (see video_groups).
    q_prescaled: q carries sm_scale * log2(e) (see qkv_from_projections(q_scale=...)); GPU only.
    return_lse: (out, lse), the softmax state of every row as _native.band_attention returns it; out_dtype=torch.float32: fp32 rows.  GPU,
    head_dim 128, plain q (ValueError), not under svg.distributed (NotImplementedError).
    geometry: the Geometry of the WHOLE sequence — required in frame-shard mode (svg.distributed.enable_frame_shards; ValueError without
    it), where q, k, v hold this rank's rows and the call is token_sharded_svg1_attention under the dense mask with every head in logical
    order; ignored otherwise.
    Token-shard mode (svg.distributed.enable_token_shards): q, k, v hold this rank's rows token_shard_range(S) of all heads and the call
    goes through run_token_sharded — whole heads of the whole sequence on every rank, bit for bit the single-GPU rows; return_lse, out_dtype
    and per-video lengths that differ are refused before any collective, as under enable()."""
    if _dist.token_shards_active() and not _local:
        _state_kw("dense_attention", return_lse, out_dtype, q_prescaled, True)
        lens = per_video(valid_len, q.shape[0], "dense_attention(valid_len)")
        if lens is not None:
            vals, _ = video_groups([int(x) for x in lens])
            if len(vals) > 1:
                _no_sharding_of_groups("dense_attention")
            valid_len = vals[0]
        if geometry is None and _dist.token_shard_row_counts() is None:
            raise ValueError("dense_attention: token-shard mode needs geometry= (the Geometry of the whole sequence) or a mode enabled with "
                             "row_counts: the tensors hold this rank's rows only")
        total = geometry.seq_len if geometry is not None else sum(_dist.token_shard_row_counts())
        return _dist.run_token_sharded(lambda qh, kh, vh: dense_attention(qh, kh, vh, valid_len, q_prescaled, _local=True), (q, k, v),
                                       total, _dist.token_shards_group())
    if _dist.frame_shards_active():
        if geometry is None:
            raise ValueError("dense_attention: frame-shard mode needs geometry= (the Geometry of the whole sequence; the tensors hold this "
                             "rank's rows only)")
        lens = per_video(valid_len, q.shape[0], "dense_attention(valid_len)")
        if lens is not None:
            vals, _ = video_groups([int(x) for x in lens])
            if len(vals) > 1:
                raise NotImplementedError("dense_attention: frame-shard mode takes ONE valid_len for the batch; per-video lengths that "
                                          "differ have no shard form")
            valid_len = vals[0]
        geo_t, group = _frame_shard_setup("dense_attention", q, k, v, geometry, None, q_prescaled, return_lse, out_dtype)
        return _dist.token_sharded_svg1_attention(q, k, v, _dense_band_mask(geometry.seq_len, valid_len), None, geo_t, group=group,
                                                  kinds="logical")
    S = q.shape[2]
    kw = _state_kw("dense_attention", return_lse, out_dtype, q_prescaled, TOKEN_MAJOR_IO and not _dist.active())
    lens = per_video(valid_len, q.shape[0], "dense_attention(valid_len)")
    if lens is not None:
        vals, heads = video_groups([int(x) for x in lens], q.shape[1])
        if len(vals) > 1:
            if q.is_cuda or return_lse:
                return _native.band_attention_groups(q, k, v, [_dense_band_mask(S, x) for x in vals], heads, q_prescaled=q_prescaled, **kw)
            assert not q_prescaled, "a pre-scaled q only exists on the GPU path"
            return torch.cat([_dense_sdpa(q[b:b + 1], k[b:b + 1], v[b:b + 1], x) for b, x in enumerate(lens)])
        valid_len = vals[0]
    if q.is_cuda or return_lse:   # (return_lse on CPU tensors: refused by the wrapper, never the SDPA call)
        return _native.band_attention(q, k, v, _dense_band_mask(S, valid_len), q_prescaled=q_prescaled, **kw)
    assert not q_prescaled, "a pre-scaled q only exists on the GPU path"
    return _dense_sdpa(q, k, v, valid_len)


def self_attention_without_timestep(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attention_mask=None, geometry: Optional[Geometry] = None):
    """The processors' self-attention branch for a call without a timestep: the reference's scaled_dot_product_attention call.  In token-shard
    mode (svg.distributed.enable_token_shards) q, k, v hold this rank's rows only, and SDPA over them would attend within the shard: there
    the call is dense_attention through run_token_sharded (a mask has no sharded form: NotImplementedError)."""
    if _dist.token_shards_active():
        if attention_mask is not None:
            raise NotImplementedError("self attention without a timestep: token-shard mode takes no attention_mask")
        return dense_attention(q, k, v, geometry=geometry)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=attention_mask, dropout_p=0.0, is_causal=False)


@time_logging_decorator("Level 3 - Cross Attention")
def cross_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense attention of q [cfg, H, Sq, D] over a short key set k, v [cfg, H, Skv, D] — the text / image-token cross attention of the
    Wan and Cosmos blocks (ref: wan/attention.py:174-188,198-201, cosmos/attention.py:104-107).  Without a mask, on the GPU, 16-bit, head_dim
    128: svg_cross_attention on the views as they are.  Anything else (CPU tensors, head_dim 64, fp32, any mask) is the reference's
    scaled_dot_product_attention call."""
    if attention_mask is None and _native.cross_attention_supported(q, k) and v.is_cuda and v.dtype == q.dtype:
        return _native.cross_attention(q, k, v, token_major_out=TOKEN_MAJOR_IO)
    return F.scaled_dot_product_attention(q, k, v, attn_mask=attention_mask, dropout_p=0.0, is_causal=False)


def cross_attention_pair(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_img: torch.Tensor, v_img: torch.Tensor,
                         attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """cross_attention(q, k, v, attention_mask) + cross_attention(q, k_img, v_img), head layout [cfg, H, Sq, D] — the text and the image
    branch of a Wan I2V block and the add behind them (ref: wan/attention.py:174-188,198-201).  Without a mask, on the GPU, 16-bit, head_dim
    128: ONE svg_cross_attention_pair launch, bit for bit the sum of the two calls; anything else is exactly those two calls and the add."""
    ts = (q, k, v, k_img, v_img)
    if attention_mask is None and _native.cross_attention_supported(q, k) and _native.cross_attention_supported(q, k_img) \
            and all(t.is_cuda and t.dtype == q.dtype for t in ts):
        with time_logging_decorator("Level 3 - Cross Attention"):
            return _native.cross_attention_pair(q, k, v, k_img, v_img, token_major_out=TOKEN_MAJOR_IO)
    return cross_attention(q, k, v, attention_mask) + cross_attention(q, k_img, v_img)


_KEY_WINDOW_CACHE = {}   # id(mask) -> (weak reference, mask._version, batch, Skv, windows or None)


def key_windows(attention_mask, batch: int, Skv: int):
    """The key windows of a key-padding mask: (begin, end) int32 [batch] on the mask's device when `attention_mask` is a BOOL tensor
    [batch, 1, 1, Skv] or [1, 1, 1, Skv] (broadcast over the batch) whose True entries form ONE non-empty contiguous run in every video —
    what the Cosmos transformer makes of the pipeline's text mask (ref: cosmos/custom_models.py:85-86); None for anything else (another
    dtype or shape, a hole, a video without a True: that video's rows are NaN in the reference, and stay so on its SDPA call).
    The hole test reads one flag back: once per mask object, which the model hands to every layer of a forward — keyed by object identity,
    guarded by a weak reference and the in-place version counter, as _HunyuanProcessorBase.get_cu_max_seqlen."""
    m = attention_mask
    if not torch.is_tensor(m) or m.dtype != torch.bool or m.dim() != 4 or Skv <= 0:
        return None
    if tuple(m.shape[1:]) != (1, 1, Skv) or m.shape[0] not in (1, batch):
        return None
    ent = _KEY_WINDOW_CACHE.get(id(m))
    if ent is not None and ent[0]() is m and ent[1:4] == (m._version, batch, Skv):
        return ent[4]
    if len(_KEY_WINDOW_CACHE) > 8:
        _KEY_WINDOW_CACHE.clear()
    rows = m.reshape(m.shape[0], Skv)
    pos = torch.arange(Skv, device=m.device, dtype=torch.int32)
    begin = torch.where(rows, pos, Skv).amin(dim=1).to(torch.int32)        # first True (Skv: none)
    end = (torch.where(rows, pos, -1).amax(dim=1) + 1).to(torch.int32)     # one behind the last True (0: none)
    one_run = _all_true((rows.sum(dim=1) == end - begin) & (end > begin))  # no hole, at least one key: the read-back
    win = None
    if one_run:
        win = (begin.expand(batch).contiguous(), end.expand(batch).contiguous())
    _KEY_WINDOW_CACHE[id(m)] = (weakref.ref(m), m._version, batch, Skv, win)
    return win


def _all_true(flags: torch.Tensor) -> bool:
    """the host read-back of key_windows (its own function: the tests count its calls)"""
    return bool(flags.all())


def cross_attention_key_masked(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attention_mask: Optional[torch.Tensor]) -> torch.Tensor:
    """cross_attention with a key-padding mask (the Cosmos blocks, ref: cosmos/attention.py:104-110): where key_windows describes the mask
    and the kernel takes the tensors (GPU, 16-bit, head_dim 128), svg_cross_attention_keyrange over each video's window — keys outside it
    are neither read nor paid for; anything else is cross_attention(q, k, v, attention_mask), i.e. the reference's SDPA call."""
    if attention_mask is not None and _native.cross_attention_supported(q, k) and v.is_cuda and v.dtype == q.dtype \
            and attention_mask.device == q.device:
        win = key_windows(attention_mask, q.shape[0], k.shape[-2])
        if win is not None:
            with time_logging_decorator("Level 3 - Cross Attention"):
                return _native.cross_attention_keyrange(q, k, v, win[1], win[0], token_major_out=TOKEN_MAJOR_IO)
    return cross_attention(q, k, v, attention_mask)


def _require_gpu(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the sparse path runs only on the GPU through libsvgattn (no CPU fallback); "
                           f"CPU tensors can only take the dense branch")


@time_logging_decorator("Level 3 - sample_mse")
def sample_mse(q, k, v, geo: Geometry, prof: "_native.ProfileDesc", num_sampled_rows: int, sample_max_row: int, skip_flag=None,
               generator=None, q_prescaled: bool = False):
    """ref: sample_mse svg/models/hyvideo/attention.py:376-399.  Rows are drawn with the CPU generator exactly like the
    reference (`torch.randint(low=0, high=sample_mse_max_row, size=(n,))` without device=) unless `generator` is given.
    -> [2, cfg, H] in q's dtype: the reference stores the MSEs in `query.dtype` (:388) before the argmin, so two candidates that
    round to the same bf16 value tie and resolve to index 0 (spatial) there — the fp32 results of the kernel are rounded the same way."""
    cfg, H, S, D = q.shape
    n = min(num_sampled_rows, S)
    rows = torch.randint(low=0, high=sample_max_row, size=(n,), generator=generator)
    mses = _native.sample_mse(q, k, v, rows.to(q.device, non_blocking=True), prof, skip_flag=skip_flag,   # (4-D views: no reshape copy)
                              sm_scale=LN2 if q_prescaled else None)   # (the profiler multiplies its scale by log2(e) itself)
    return mses.reshape(2, cfg, H).to(q.dtype)


_SWITCH_GEN = None
_SWITCH_SEED = None


def reseed_switch_generator(seed: Optional[int] = None) -> None:
    """(Re)build the CPU generator of the device-switched path from `seed` (default: the global seed, torch.initial_seed()).
    Called by svg.utils.seed.seed_everything and by the replace_*_attention install hooks, so that seeding a second video in the
    same process resets the sampled profiler rows exactly like a fresh process.  Under svg.distributed.enable() (and
    enable_frame_shards(), enable_token_shards()) the seed of rank 0 is broadcast: every rank draws the same rows, whatever it was seeded with (the sharded result equals the single-GPU one)."""
    global _SWITCH_GEN, _SWITCH_SEED
    base = torch.initial_seed() if seed is None else int(seed)
    use = base
    if _sharded_draws():
        grp = _dist.head_mode()[1] if _dist.head_mode()[0] else _dist.frame_shards_group()
        on_gpu = torch.distributed.get_backend(grp) == "nccl"
        t = torch.tensor([base % (2 ** 63)], dtype=torch.int64, device="cuda" if on_gpu else "cpu")
        torch.distributed.broadcast(t, src=torch.distributed.get_global_rank(grp, 0) if grp is not None else 0, group=grp)
        use = int(t.item())
    _SWITCH_GEN = torch.Generator().manual_seed(use % (2 ** 63))
    _SWITCH_SEED = (base, _sharded_draws())
    reseed_probe_generator(base)   # (the quality probe's rows start over with the video as well; a stream of its own, see _probe_generator)


def _sharded_draws() -> bool:
    """a mode of svg.distributed is on in which every rank must draw the same rows (enable, enable_frame_shards, enable_token_shards)"""
    return _dist.active() or _dist.frame_shards_active() or _dist.token_shards_active()


def _switch_generator():
    """CPU generator of the device-switched path.  The reference (and the host-side branch) draw the profiler's rows from the global
    CPU generator on SPARSE steps only; the switched path does not know on the host whether the step is dense, so it must not
    touch the global stream at all: it draws from this generator, derived from the global seed — re-derived whenever
    torch.initial_seed() changes (a later torch.manual_seed) or sharding is switched on, and by `reseed_switch_generator()`, which
    the seeding / install hooks call (re-seeding with the SAME seed cannot be seen from the seed alone).  (Deviation: at equal seeds
    the sampled rows differ from the reference's; every other consumer of the global CPU RNG sees the reference's stream.)"""
    if _SWITCH_GEN is None or _SWITCH_SEED != (torch.initial_seed(), _sharded_draws()):
        reseed_switch_generator()
    return _SWITCH_GEN


def dense_flag_on_device(timestep, first_times_fp):
    """int32 [1] on the timestep's device: 1 = this denoise step is a dense warm-up step (`timestep[0] > first_times_fp`,
    ref hyvideo/attention.py:495) — the comparison stays on the GPU; None when the timestep is not a GPU tensor."""
    if not (torch.is_tensor(timestep) and timestep.is_cuda):
        return None
    return (timestep.reshape(-1)[:1] > first_times_fp).to(torch.int32)


def svg1_attention_device_switch(q, k, v, geo: Geometry, mask: "_native.BandMask", dense_mask: "_native.BandMask",
                                 prof: "_native.ProfileDesc", num_sampled_rows: int, sample_max_row: int, dense_flag,
                                 _local: bool = False, q_prescaled: bool = False, return_lse: bool = False, out_dtype=None,
                                 quality: Optional["QualityRequest"] = None, adaptive: Optional["AdaptiveBand"] = None,
                                 band_store: Optional["BandStore"] = None, layer_idx=None):
    """Dense warm-up step or sparse step, decided on the device: the profiler and the attention kernel read
    `dense_flag`; on a dense step the profiler returns at once and the kernel runs `dense_mask` without the head placement.
    Same attention results as the host-side branch of attention_core_logic (ref: hyvideo/attention.py:491-524) for the same sampled
    rows; the rows come from a dedicated CPU generator (`_switch_generator`).  The returned best_mask_idx is -1 on a dense step.
    mask, dense_mask: one BandMask for the batch, or a sequence of cfg of them, one per video (see video_groups).
    return_lse: (out, best_mask_idx, lse) with the softmax state of every row under the mask the flag selects, as
    _native.band_attention_switch returns it — the layer-call as one part of a partitioned attention (merge_attention_states);
    out_dtype=torch.float32: fp32 rows.  Plain q only (ValueError), not under svg.distributed (NotImplementedError).
    Frame-shard mode (svg.distributed.enable_frame_shards): q, k, v [cfg, H, S_r, D] are all heads of this rank's frame_shard of the
    sequence `geo` describes, the call is token_sharded_svg1_layer_call with dense_mask / dense_flag, -> (out [cfg, H, S_r, D], best);
    the sampled rows are GLOBAL rows of the whole sequence; what has no shard form raises before any collective (_frame_shard_setup).
    quality: a QualityRequest (quality_request): the call is probed as well and its record queued (log_quality) — on EVERY call, the host
    does not know whether the step is dense; the record carries dense_flag and the writer drops those of dense steps.  Where the launch has
    an LSE form the call goes through it (the same o).  Refused under svg.distributed.
    adaptive: an AdaptiveBand, with band_store a BandStore and layer_idx the layer's key in it: the call runs one band per head from the
    store (the layer's first call fills it with the mask's band) through svg_band_attention_switch_per_head_lse, K is probed on rows from
    the probe's generator (neither the global RNG nor the switched path's generator moves) and svg_band_width_update steps the bands for
    the layer's next call, with dense_flag as its skip flag — all on the device, no host synchronisation.  With `quality` as well the
    rows are drawn once, its one dense probe feeds both and the record gains "band".  ValueError, before anything runs, where the launch
    has no LSE form (head_dim 64, fp8, a pre-scaled q, out_dtype); NotImplementedError under svg.distributed and for per-video masks
    that differ.  None: nothing changes."""
    return _svg1_layer_call("svg1_attention_device_switch", True, q, k, v, geo, mask, prof, num_sampled_rows, sample_max_row,
                            dense_mask=dense_mask, dense_flag=dense_flag, _local=_local, q_prescaled=q_prescaled, return_lse=return_lse,
                            out_dtype=out_dtype, quality=quality, adaptive=adaptive, band_store=band_store, layer_idx=layer_idx)


def svg1_sparse_attention(q, k, v, geo: Geometry, mask: "_native.BandMask", prof: "_native.ProfileDesc",
                          num_sampled_rows: int, sample_max_row: int, fused: bool = True, _local: bool = False,
                          q_prescaled: bool = False, return_lse: bool = False, out_dtype=None,
                          quality: Optional["QualityRequest"] = None, adaptive: Optional["AdaptiveBand"] = None,
                          band_store: Optional["BandStore"] = None, layer_idx=None):
    """The sparse branch of attention_core_logic (ref: hyvideo/attention.py:507-524):
    online profiling -> best_mask_idx -> placement -> block-sparse attention -> inverse placement.
    fused=True folds both placements into the attention kernel (bit-identical result, ~5.9 GB less HBM traffic at
    Hunyuan 720p); fused=False runs the three kernels of the reference pipeline.
    mask: one BandMask for the batch, or a sequence of cfg of them, one per video (see video_groups); the profiler's masks do not depend
    on the prompt length, so the profiling pass is the same either way.
    return_lse, out_dtype, frame-shard mode, quality, adaptive / band_store / layer_idx: as svg1_attention_device_switch, without a flag —
    every call of this branch is a sparse step, the launches are _native.band_attention and svg_band_attention_per_head_lse — and on the
    fused 16-bit path only: fp8 and fused=False have no LSE form (return_lse, adaptive: ValueError; quality: the error alone, no kept mass)
    and no shard form.  The rows come from the global CPU generator like the reference's, in frame-shard mode from the switched path's
    (every rank draws the same)."""
    return _svg1_layer_call("svg1_sparse_attention", False, q, k, v, geo, mask, prof, num_sampled_rows, sample_max_row, fused=fused,
                            _local=_local, q_prescaled=q_prescaled, return_lse=return_lse, out_dtype=out_dtype, quality=quality,
                            adaptive=adaptive, band_store=band_store, layer_idx=layer_idx)


def _svg1_layer_call(what: str, switched: bool, q, k, v, geo: Geometry, mask, prof, num_sampled_rows: int, sample_max_row: int, *,
                     dense_mask=None, dense_flag=None, fused: bool = True, _local: bool = False, q_prescaled: bool = False,
                     return_lse: bool = False, out_dtype=None, quality=None, adaptive=None, band_store=None, layer_idx=None):
    """The SVG1 layer-call, once: refusals -> frame shards, token shards or head shards -> profiler -> band launch ->
    probes.  switched: svg1_attention_device_switch (dense_mask and dense_flag given, fused) / svg1_sparse_attention; what the two do
    differently is decided on the five lines below and nowhere else."""
    what_gpu = "SVG1 attention" if switched else "SVG1 sparse attention"   # (as _require_gpu and the groups' refusals name the call)
    fp8 = not switched and _use_fp8(q)   # (the switched launch has no fp8 form: the processors switch on the device at bf16 only)
    flag_kw = dict(dense_flag=dense_flag) if switched else {}   # (what the probes get of the flag: the host branch passes none)
    timer = time_logging_decorator("Level 3 - sparse_flex_attention") if not switched else contextlib.nullcontext()   # (the switched launch: no label)
    rows_from = _switch_generator if switched else (lambda: None)   # (None: the global CPU generator, as the reference draws)
    if adaptive is not None:
        _refuse_adaptive_band(what, q, band_store, q_prescaled, fused, out_dtype, mask, (("dense_mask", dense_mask),) if switched else ())
        band_bounds = adaptive.bounds(_one_mask(f"{what}(mask)", mask, q.shape[0]).band, q.shape[2])   # (masks that differ: refused above)
    if quality is not None:
        _refuse_quality_when_sharded(what)
    cfg, H = q.shape[0], q.shape[1]
    if _dist.frame_shards_active():   # q, k, v: this rank's rows; -> (out [cfg, H, S_r, D], best_mask_idx)
        mask = _one_mask(f"{what}(mask)", mask, cfg)
        if dense_mask is not None:
            dense_mask = _one_mask(f"{what}(dense_mask)", dense_mask, cfg)
        geometry, group = _frame_shard_setup(what, q, k, v, geo, num_sampled_rows, q_prescaled, return_lse, out_dtype, fused)
        # (global rows, from the broadcast-seeded generator of the switched path on both branches: every rank draws the same)
        rows = torch.randint(low=0, high=sample_max_row, size=(min(num_sampled_rows, geo.seq_len),), generator=_switch_generator())
        out, best = _dist.token_sharded_svg1_layer_call(q, k, v, mask, prof, geometry, rows, group=group, dense_mask=dense_mask,
                                                        dense_flag=dense_flag)
        return out, best.reshape(cfg, H)
    probe_lse = (quality is not None and not return_lse and _quality_lse_form(q, q_prescaled, fused)) or (adaptive is not None and not return_lse)
    kw = _state_kw(what, return_lse or probe_lse, out_dtype, q_prescaled, TOKEN_MAJOR_IO, fp8=fp8, fused=fused)
    _require_gpu(q, what_gpu)
    pm, pd = per_video(mask, cfg, f"{what}(mask)"), per_video(dense_mask, cfg, f"{what}(dense_mask)")
    groups = None
    if pm is not None or pd is not None:   # (mask, dense_mask) pairs; the host branch's dense_mask is None: it groups masks
        pairs, heads = video_groups(list(zip(pm or [mask] * cfg, pd or [dense_mask] * cfg)), H)
        mask, dense_mask = pairs[0]
        if len(pairs) > 1:
            _no_sharding_of_groups(what_gpu)
            groups = ([m for m, _ in pairs], [d for _, d in pairs], heads)
    if not _local and (_dist.token_shards_active() or _dist.active()):
        def whole_heads(qh, kh, vh):   # (quality, adaptive, return_lse: refused above in these modes)
            return _svg1_layer_call(what, switched, qh, kh, vh, geo, mask, prof, num_sampled_rows, sample_max_row, dense_mask=dense_mask,
                                    dense_flag=dense_flag, fused=fused, _local=True, q_prescaled=q_prescaled)

        if _dist.token_shards_active():   # q, k, v: this rank's rows; whole heads of the whole sequence inside, rows back
            return _dist.run_token_sharded(whole_heads, (q, k, v), geo.seq_len, _dist.token_shards_group())
        return _dist.run_sharded(whole_heads, (q, k, v), _dist.current_group())   # enable(): this rank's heads only, outputs all-gathered
    mses = sample_mse(q, k, v, geo, prof, num_sampled_rows, sample_max_row, skip_flag=dense_flag, generator=rows_from(), q_prescaled=q_prescaled)
    best_mask_idx = torch.argmin(mses, dim=0)  # [cfg, H] int64; NaN wins like torch.argmin in the reference
    pk = dict(head_perm_flag=best_mask_idx, vid0=geo.vid0, num_frame=geo.num_frame, frame_size=geo.frame_size)

    def final_best():   # (-1 on a dense step, which only the device knows; computed after the launch)
        return torch.where(dense_flag.reshape(()) != 0, torch.full_like(best_mask_idx, -1), best_mask_idx) if switched else best_mask_idx

    if adaptive is not None:   # (fused, 16-bit, one mask for the batch, no sharding: refused above otherwise)
        from .. import _adaptive_band

        qk = dict(work_queue=True) if PER_HEAD_BAND_QUEUE else {}   # (off: nothing new is passed)
        if switched:
            run = lambda band: _adaptive_band.band_attention_switch_per_head(q, k, v, mask, dense_mask, dense_flag, band,   # noqa: E731
                                                                             token_major_out=TOKEN_MAJOR_IO, **pk, **qk)
        else:
            run = lambda band: _adaptive_band.band_attention_per_head(q, k, v, mask, band, token_major_out=TOKEN_MAJOR_IO, **pk, **qk)   # noqa: E731
        with timer:
            out = _adaptive_band_call(run, adaptive, band_store, layer_idx, mask, band_bounds, q, k, v, quality, **flag_kw)
        return (out[0], final_best(), out[1]) if return_lse else (out[0], final_best())
    if fused:
        with timer:
            if groups is not None:
                if fp8:
                    raise NotImplementedError("SVG1 sparse attention: fp8 attention with per-video lengths that differ is not implemented")
                alt = dict(alt_masks=groups[1], use_alt_flag=dense_flag) if switched else {}
                out = _native.band_attention_groups(q, k, v, groups[0], groups[2], q_prescaled=q_prescaled, **alt, **kw, **pk)
            elif fp8:   # (the fp8 pre-pass folds whatever scale it is given into its quantisation of q)
                out = _native.band_attention_fp8(q.contiguous(), k.contiguous(), v.contiguous(), mask, sm_scale=LN2 if q_prescaled else None, **pk)
            else:
                if _local:   # (enable(): contiguous head slices are gathered; token-shard mode: token-major rows are what the outbound exchange sends)
                    kw["token_major_out"] = TOKEN_MAJOR_IO and _dist.token_shards_active()
                if switched:
                    out = _native.band_attention_switch(q, k, v, mask, dense_mask, dense_flag, q_prescaled=q_prescaled, **kw, **pk)
                else:
                    out = _native.band_attention(q, k, v, mask, q_prescaled=q_prescaled, **kw, **pk)
        best_idx = final_best()
        if quality is not None:
            o_p, lse_p = out if (return_lse or probe_lse) else (out, None)
            log_quality(quality, o_p, lse_p, q, k, v, q_prescaled, **flag_kw)
            if probe_lse:
                out = o_p
        return (out[0], best_idx, out[1]) if return_lse else (out, best_idx)
    # the three kernels of the reference pipeline (the host branch only; no LSE form, no shard form)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    qo, ko, vo = _native.empty_like(q), _native.empty_like(k), _native.empty_like(v)
    with time_logging_decorator("Level 3 - fast_sparse_head_placement"):
        _native.head_placement([q, k, v], [qo, ko, vo], best_mask_idx, geo.context_length, geo.num_frame, geo.frame_size,
                               geo.text_first, inverse=False)
    with time_logging_decorator("Level 3 - sparse_flex_attention"):
        if groups is not None:
            hs = _native.band_attention_groups(qo, ko, vo, groups[0], groups[2], q_prescaled=q_prescaled)
        else:
            hs = _native.band_attention(qo, ko, vo, mask, q_prescaled=q_prescaled)
    out = _native.empty_like(hs)
    with time_logging_decorator("Level 3 - fast_hidden_states_placement"):
        _native.head_placement([hs], [out], best_mask_idx, geo.context_length, geo.num_frame, geo.frame_size, geo.text_first,
                               inverse=True)
    if quality is not None:   # (no LSE form: the error alone)
        log_quality(quality, out, None, q, k, v, q_prescaled)
    return out, best_mask_idx


# ---------------------------------------------------------------------------------------------------------------
# SVG2
# ---------------------------------------------------------------------------------------------------------------
class CentroidStore:
    """Per-layer k-means state (ref: class-level dicts of Hunyuan_SAPAttn_Processor2_0, hyvideo/attention.py:566-568).
    Unlike the reference it can be reset between videos (`clear()`).
    Stored centroids carry the batch size (cfg, the number of videos) of the call that produced them: a layer-call with a different
    cfg is a first call of that layer — random initial points and `iter_init` iterations — and never warm-starts from centroids of
    the wrong shape (`has(layer_idx, cfg, heads)`).  Centroids written into `q` / `k` directly carry it in their shape, [cfg * H, K, D]."""

    def __init__(self):
        self.q = {}
        self.k = {}
        self.cfg = {}

    def has(self, layer_idx, cfg=None, heads=None):
        if layer_idx not in self.q:
            return False
        if cfg is None:
            return True
        if heads:   # (the shape decides: it is right for centroids written directly as well)
            c = self.q[layer_idx]
            return c.reshape(-1, *c.shape[-2:]).shape[0] == cfg * heads
        return self.cfg.get(layer_idx) == cfg

    def put(self, layer_idx, q, k, cfg):
        self.q[layer_idx], self.k[layer_idx], self.cfg[layer_idx] = q, k, cfg

    def clear(self):
        self.q.clear()
        self.k.clear()
        self.cfg.clear()


class _KeptMassStore:
    """Per-layer state of a knob steered by kept mass (TopPStore, BandStore): `state[layer]`, a [cfg * H] DEVICE tensor of the subclass's
    `dtype` — the value of every head for the layer's NEXT sparse call, stepped in place by the knob's controller — and `kept[layer]`,
    fp32 [cfg * H], the kept mass its last sparse call measured.  Nothing here is ever read back by the package.  A call with a different
    cfg * H (or on another device) starts the layer again from the initial value; `clear()` forgets every layer (call between videos)."""
    dtype = as_init = None   # (the subclass: the vector's dtype and the Python type `init` is converted to)

    def __init__(self):
        self.state = {}
        self.kept = {}

    def has(self, layer_idx, n=None) -> bool:
        return layer_idx in self.state and (n is None or self.state[layer_idx].numel() == n)

    def get(self, layer_idx, n: int, init, device) -> torch.Tensor:
        """The layer's [n] values; filled with `init` (and the last kept mass forgotten) where the layer has none of that size."""
        t = self.state.get(layer_idx)
        if t is None or t.numel() != n or t.device != torch.device(device):
            t = torch.full((n,), self.as_init(init), dtype=self.dtype, device=device)
            self.state[layer_idx] = t
            self.kept.pop(layer_idx, None)
        return t

    def clear(self):
        self.state.clear()
        self.kept.clear()


class TopPStore(_KeptMassStore):
    """The state of the adaptive top-p (AdaptiveTopP), beside CentroidStore: `p[layer]`, fp32 — the thresholds svg_top_p_update steps; the
    initial value is the processor's scalar top_p."""
    dtype, as_init = torch.float32, float
    p = property(lambda self: self.state)


def _check_kept_mass_knob(knob, dead_name: str) -> None:
    """What AdaptiveTopP and AdaptiveBand check alike: gains and dead zone not NaN and >= 0, 1 to 64 probe rows"""
    name, dead = type(knob).__name__, getattr(knob, dead_name)
    ok = lambda x: x == x and x >= 0   # noqa: E731  (not NaN, not negative)
    if not (ok(knob.gain_up) and ok(knob.gain_down) and ok(dead)):
        raise ValueError(f"{name}: gains and {dead_name} are >= 0, got {knob.gain_up}, {knob.gain_down}, {dead}")
    if not 1 <= int(knob.rows) <= 64:
        raise ValueError(f"{name}: 1 to 64 probe rows, got {knob.rows}")


@dataclass
class AdaptiveTopP:
    """The SVG2 knob "keep this much attention mass": every head's top_p is steered, on the device, so that the kept mass measured after each
    sparse layer-call — mean over probe rows of exp(lse_sparse - lse_dense) — approaches `target` (include/svg_attn_adaptive_top_p.h
    svg_top_p_update):
        e = target - kept;  step = gain_up * e if e > 0, gain_down * (e + band) if e < -band, else 0;  top_p = clamp(top_p + step, p_min, p_max)
    A head below target is raised quickly, a head more than `band` above it is lowered slowly; inside the band nothing moves.  The first
    sparse call of a layer runs with the processor's scalar top_p.
    The default gains are UNTUNED: nobody has measured which suit a real model.  gain_up = gain_down = 0 measures and moves nothing.
    rows: probe rows per head and call (1..64).  valid_len: the dense `valid` of the call as QualityRequest carries it (set by the
    processors, per call)."""
    target: float
    gain_up: float = 1.0
    gain_down: float = 0.25
    band: float = 0.02
    p_min: float = 0.1
    p_max: float = 1.0
    rows: int = 64
    valid_len: object = None

    def __post_init__(self):
        _check_kept_mass_knob(self, "band")
        if not 0 <= self.p_min <= self.p_max <= 1:
            raise ValueError(f"AdaptiveTopP: 0 <= p_min <= p_max <= 1, got {self.p_min}, {self.p_max}")


def _refuse_kmeans_e4m3_when_sharded(what: str, head_shard=None) -> None:
    """on the host, before any collective, on every rank alike"""
    if head_shard is not None or _dist._STATE["enabled"] or _dist.frame_shards_active() or _dist.token_shards_active():
        raise NotImplementedError(f"{what}: kmeans_e4m3 under svg.distributed (enable, enable_frame_shards, enable_token_shards) is not "
                                  f"implemented: the stepped Lloyd loop of a head shard has no e4m3 form; unset kmeans_e4m3 or run on one GPU")


def _refuse_centroid_tail_when_sharded(what: str, head_shard=None) -> None:
    """on the host, before any collective, on every rank alike"""
    if head_shard is not None or _dist._STATE["enabled"] or _dist.frame_shards_active() or _dist.token_shards_active():
        raise NotImplementedError(f"{what}: centroid_tail under svg.distributed (enable, enable_frame_shards, enable_token_shards) is not "
                                  f"implemented: the means and the tail read whole heads of the whole sequence; unset centroid_tail or run on one GPU")


def _refuse_centroid_tail(what: str, q: torch.Tensor, block_rows: int, adaptive=None, head_shard=None) -> None:
    """What the centroid tail refuses, all of it before anything runs: there is no silent fall-back to the sparse part alone."""
    _refuse_centroid_tail_when_sharded(what, head_shard)
    if adaptive is not None:
        raise ValueError(f"{what}: centroid_tail together with adaptive_top_p is not implemented — the controller steers on the kept mass of "
                         f"the sparse part alone; unset one of them")
    S, D = q.shape[-2], q.shape[-1]
    if D != 128 or _use_fp8(q) or q.dtype not in (torch.bfloat16, torch.float16) or S < 160 * block_rows:
        raise ValueError(f"{what}(centroid_tail=True): the tail is merged with the sparse call through its row log-sum-exp — head_dim 128, bf16 / "
                         f"fp16 (not fp8), S >= 160 block-rows; got D = {D}, {q.dtype}, fp8 = {_use_fp8(q)}, S = {S}, block-rows = {block_rows}")


def _refuse_kept_mass_knob_when_sharded(what: str, knob: str) -> None:
    """knob: the processors' option, adaptive_top_p or adaptive_band"""
    if _dist._STATE["enabled"] or _dist.frame_shards_active() or _dist.token_shards_active():
        raise NotImplementedError(f"{what}: {knob} under svg.distributed (enable, enable_frame_shards, enable_token_shards) is not "
                                  f"implemented: the probe reads whole heads of the whole sequence; unset {knob} or run on one GPU")


def _refuse_adaptive_without_lse(what: str, q: torch.Tensor, block_rows: int) -> None:
    """ValueError where the variable-block launch of this call has no LSE form with the plain call's o: there is no silent fall-back."""
    S, D = q.shape[-2], q.shape[-1]
    if D != 128 or _use_fp8(q) or q.dtype not in (torch.bfloat16, torch.float16) or S < 160 * block_rows:
        raise ValueError(f"{what}(adaptive=...): the controller needs the row log-sum-exp of the sparse call — head_dim 128, bf16 / fp16 (not "
                         f"fp8), S >= 160 block-rows; got D = {D}, {q.dtype}, fp8 = {_use_fp8(q)}, S = {S}, block-rows = {block_rows}")


def probe_plan(valid_len, n_rows: int, cfg: int, S: int):
    """The rows a layer-call is probed on: [(videos b0 .. b0 + nb, valid_len of the group or None, rows int64 [R] on the CPU)], one entry
    per group of videos with one valid length (video_groups).  Rows: uniform over the valid rows, from the probe's own CPU generator."""
    lens = per_video(valid_len, cfg, "quality probe(valid_len)")
    vals, counts = video_groups(lens if lens is not None else [valid_len] * cfg)
    plan, b0 = [], 0
    for vl, nb in zip(vals, counts):
        vl = None if vl is None or int(vl) <= 0 or int(vl) >= S else int(vl)
        rows = torch.randint(low=0, high=S if vl is None else vl, size=(max(1, min(int(n_rows), 64)),), generator=_probe_generator())
        plan.append((slice(b0, b0 + nb), vl, rows))
        b0 += nb
    return plan


def _knob_probe_plan(quality, adaptive, cfg: int, S: int):
    """The probe_plan of a layer-call under a kept-mass knob, drawn once: where the call is also probed for `quality`, that request's valid
    length and row count (its one dense probe then feeds the controller as well), else the knob's."""
    src = quality if quality is not None else adaptive
    return probe_plan(src.valid_len, src.rows, cfg, S)


def _kept_mass_step(update, store: _KeptMassStore, layer_idx, state: torch.Tensor, lse: torch.Tensor, q, k, plan, lse_dense=None):
    """After a sparse layer-call that ran with the per-head values state [cfg * H] (the store's tensor) and returned lse [cfg, H, S]: probe
    (K only; lse_dense: what a quality probe on the same plan already measured, one [nb, H, R] per group), then the knob's controller —
    update(lse_sparse, rows, lse_dense, state, kept) on every group's heads: state is stepped in place, the kept mass lands in the store.
    No host synchronisation."""
    from .. import _probe

    cfg, H, S, _ = q.shape
    lse = lse.reshape(cfg, H, S)
    kept = _native.empty((cfg * H,), dtype=torch.float32, device=q.device)
    for i, (sl, vl, rows) in enumerate(plan):
        ld = lse_dense[i] if lse_dense is not None else _probe.sample_dense_lse(q[sl], k[sl], rows, vl)
        hs = slice(sl.start * H, sl.stop * H)
        update(lse[sl], rows.to(q.device, non_blocking=True), ld, state[hs], kept[hs])
    store.kept[layer_idx] = kept


def adaptive_step(adaptive: AdaptiveTopP, top_p_store: TopPStore, layer_idx, p: torch.Tensor, lse: torch.Tensor, q, k, plan, lse_dense=None):
    """_kept_mass_step with svg_top_p_update: the thresholds p [cfg * H] of the call are stepped in place."""
    a = adaptive
    _kept_mass_step(lambda *t: _native.top_p_update(*t, a.target, a.gain_up, a.gain_down, a.band, a.p_min, a.p_max),
                    top_p_store, layer_idx, p, lse, q, k, plan, lse_dense)


# ---------------------------------------------------------------------------------------------------------------
# SVG1's adaptive band width: one band per head on the device, steered by measured kept mass (include/svg_attn_adaptive_band.h)
# ---------------------------------------------------------------------------------------------------------------
class BandStore(_KeptMassStore):
    """The state of the adaptive band (AdaptiveBand): `band[layer]`, int32 — the bands svg_band_width_update steps; the initial value is
    the mask's band."""
    dtype, as_init = torch.int32, int
    band = property(lambda self: self.state)


@dataclass
class AdaptiveBand:
    """The SVG1 knob "keep this much attention mass": every head's band width is steered, on the device, so that the kept mass measured after
    each sparse layer-call — mean over probe rows of exp(lse_sparse - lse_dense) — approaches `target` (include/svg_attn_adaptive_band.h
    svg_band_width_update):
        e = target - kept;  x = gain_up * e if e > 0, gain_down * (e + dead) if e < -dead, else 0;  n = rint(clamp(x, -65536, 65536))
        band = clamp(band + n * quantum, band_min, band_max)
    The gains are QUANTA per unit of kept mass.  A head below target is widened quickly, a head more than `dead` above it is narrowed slowly;
    inside the dead zone nothing moves.  The first sparse call of a layer runs every head with the mask's band (what `sparsity` gives).
    The default gains are UNTUNED: nobody has measured which suit a real model, nor what per-head bands are worth on one.  gain_up =
    gain_down = 0 measures and moves nothing.
    band_min / band_max: None — the smallest / largest value congruent to the mask's band modulo `quantum` inside [1, S + 1], so the
    residue of the mask's band survives every step (Wan's is a multiple of 128 plus 1); a given bound that is not congruent raises
    ValueError at the call (bounds()).  rows: probe rows per head and call (1..64).  valid_len: the dense `valid` of the call as
    QualityRequest carries it (set by the processors, per call)."""
    target: float
    gain_up: float = 8.0
    gain_down: float = 2.0
    dead: float = 0.02
    quantum: int = 128
    band_min: Optional[int] = None
    band_max: Optional[int] = None
    rows: int = 64
    valid_len: object = None

    def __post_init__(self):
        _check_kept_mass_knob(self, "dead")
        if int(self.quantum) != self.quantum or not 1 <= int(self.quantum) <= 4096:
            raise ValueError(f"AdaptiveBand: quantum is an integer in [1, 4096], got {self.quantum}")
        for name in ("band_min", "band_max"):
            b = getattr(self, name)
            if b is not None and (int(b) != b or int(b) < 1):
                raise ValueError(f"AdaptiveBand: {name} is None or an integer >= 1, got {b}")
        if self.band_min is not None and self.band_max is not None and self.band_min > self.band_max:
            raise ValueError(f"AdaptiveBand: band_min <= band_max, got {self.band_min}, {self.band_max}")

    def bounds(self, mask_band: int, S: int):
        """(band_min, band_max) of a call under a mask of band `mask_band` over S rows: the given bounds, checked — congruent to mask_band
        modulo quantum, 1 <= band_min <= band_max <= S + 1 — or, for None, the extreme congruent values inside [1, S + 1]."""
        qn, b = int(self.quantum), int(mask_band)
        if not 1 <= b <= S + 1:
            raise ValueError(f"AdaptiveBand: the mask's band lies in [1, S + 1] = [1, {S + 1}], got {b}")
        r = b % qn
        lo = r if r >= 1 else qn
        hi = r + ((S + 1 - r) // qn) * qn
        for name, given in (("band_min", self.band_min), ("band_max", self.band_max)):
            if given is not None and (int(given) - b) % qn != 0:
                raise ValueError(f"AdaptiveBand: {name} = {given} is not congruent to the mask's band {b} modulo quantum = {qn}: every step "
                                 f"is a whole number of quanta, so the bound would change the band's residue")
        lo = lo if self.band_min is None else int(self.band_min)
        hi = hi if self.band_max is None else int(self.band_max)
        if not 1 <= lo <= hi <= S + 1:
            raise ValueError(f"AdaptiveBand: 1 <= band_min <= band_max <= S + 1 = {S + 1}, got {lo}, {hi}")
        return lo, hi


def _refuse_adaptive_band(what: str, q: torch.Tensor, band_store, q_prescaled: bool, fused: bool, out_dtype, mask, extra_masks=()) -> None:
    """What the adaptive band refuses, all of it before anything runs: there is no silent fall-back to the launch's one band."""
    _refuse_kept_mass_knob_when_sharded(what, "adaptive_band")
    if band_store is None:
        raise ValueError(f"{what}(adaptive=...) needs a band_store (BandStore): the bands live there between calls")
    D = q.shape[-1]
    if D != 128 or _use_fp8(q) or q.dtype not in (torch.bfloat16, torch.float16) or q_prescaled or not fused or out_dtype is not None:
        raise ValueError(f"{what}(adaptive=...): the per-head band runs the row log-sum-exp form of the fused launch — head_dim 128, bf16 / "
                         f"fp16 (not fp8), a plain q, fused=True, no out_dtype; got D = {D}, {q.dtype}, fp8 = {_use_fp8(q)}, q_prescaled = "
                         f"{q_prescaled}, fused = {fused}, out_dtype = {out_dtype}")
    cfg = q.shape[0]
    for m, name in ((mask, "mask"),) + tuple(extra_masks):
        pm = per_video(m, cfg, f"{what}({name})")
        if pm is not None and len(video_groups(pm)[0]) > 1:
            raise NotImplementedError(f"{what}(adaptive=...): per-video masks that differ (the groups launch) have no per-head band form; "
                                      f"give every video the same text length")


def adaptive_band_step(adaptive: AdaptiveBand, band_store: BandStore, layer_idx, band: torch.Tensor, lse: torch.Tensor, q, k, plan,
                       bounds, lse_dense=None, skip_flag=None):
    """_kept_mass_step with svg_band_width_update: the bands `band` [cfg * H] of the call are stepped in place inside `bounds`.  skip_flag: the
    dense_flag of the switched path (a dense step measures and moves nothing)."""
    a = adaptive
    _kept_mass_step(lambda *t: _native.band_width_update(*t, a.target, a.gain_up, a.gain_down, a.dead, a.quantum, bounds[0], bounds[1],
                                                         skip_flag=skip_flag), band_store, layer_idx, band, lse, q, k, plan, lse_dense)


def _adaptive_band_call(run, adaptive: AdaptiveBand, band_store: BandStore, layer_idx, mask, bounds, q, k, v, quality, dense_flag=None):
    """One layer-call under per-head bands: `run(band)` launches the per-head (switch) form and returns (out, lse); then the probe — one
    plan for the quality record and the controller — and the controller step.  -> (out, lse)"""
    cfg, H, S, _ = q.shape
    band = band_store.get(layer_idx, cfg * H, mask.band, q.device)
    out, lse = run(band)
    plan = _knob_probe_plan(quality, adaptive, cfg, S)
    lse_d = None
    if quality is not None:   # (the rows are drawn once: the quality probe's dense lse feeds the controller)
        lse_d = log_quality(quality, out, lse, q, k, v, dense_flag=dense_flag, plan=plan, band=band.clone())
    adaptive_band_step(adaptive, band_store, layer_idx, band, lse, q, k, plan, bounds, lse_d, skip_flag=dense_flag)
    return out, lse


KMEANS_TWO_STREAMS = True    # q-side and k-side k-means loops on two streams (kmeans_clustering below); False: one after the other
_SIDE_STREAMS = {}


def _side_stream(device) -> "torch.cuda.Stream":
    dev = torch.device(device)
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SIDE_STREAMS[key]


@time_logging_decorator("Level 3.5 - kmeans clustering")
def kmeans_clustering(store: CentroidStore, layer_idx: int, q_video, k_video, num_q_centroids, num_k_centroids, iter_init,
                      iter_step, head_shard=None, e4m3=False):
    """ref: kmeans_init / kmeans_step / kmeans_clustering, hyvideo/attention.py:576-626: random init from the data on the
    first call of a layer, warm start from the previous denoise step's centroids afterwards.
    head_shard = (h0, h1, H): q_video / k_video hold heads [h0, h1) of H (svg.distributed) — the random initial points are drawn
    for all H heads, in the order of the unsharded call, and this rank keeps its rows; the stopping rule's maximum centre shift is
    all-reduced — so that the result does not depend on the sharding.
    cfg > 1: one stopping rule per video (the loops run with group = H, the heads of one video; sharded: this rank's heads of one
    video, the per-video maxima all-reduced), so that each video's clustering is the one it gets alone.
    e4m3: all but the last iteration of the call assign with e4m3 operands (batch_kmeans_Euclid(fp8_iters=iters - 1): the returned labels
    stay the 16-bit arg-max against the centroids that entered the last iteration).  Refused under svg.distributed."""
    if e4m3:
        _refuse_kmeans_e4m3_when_sharded("kmeans_clustering", head_shard)
    if _dist.token_shards_active() and head_shard is None:
        raise NotImplementedError("kmeans_clustering: token-shard mode clusters inside svg2_sparse_attention only (whole heads of the whole "
                                  "sequence); a call on this rank's rows (zero_step_kmeans_init) has no sharded form")
    cfg, H, N, D = q_video.shape
    first = not store.has(layer_idx, cfg, H)
    iters = iter_init if first else iter_step
    f8 = dict(fp8_iters=iters - 1) if e4m3 and iters > 1 else {}   # (off: the call of before, argument for argument)
    qi = None if first else store.q[layer_idx]
    ki = None if first else store.k[layer_idx]
    red = _dist.all_reduce_max_ if head_shard is not None else None
    if first and (head_shard is not None or cfg > 1):
        # ref svg/kmeans_utils.py:706-709, drawn here video by video (q side, then k side, of all H heads) in the order of a cfg = 1 call:
        # video 0 gets the initial points a call on it alone gets at the same seed; a head-sharded rank keeps its rows of each draw
        h0, h1, H_all = head_shard if head_shard is not None else (0, H, H)
        qd, kd = [], []
        for _ in range(cfg):
            qd.append(torch.randint(0, N, (H_all, num_q_centroids), device=q_video.device)[h0:h1])
            kd.append(torch.randint(0, N, (H_all, num_k_centroids), device=k_video.device)[h0:h1])

        def draw(x, idx):
            return torch.gather(x.reshape(cfg * H, N, D), 1, torch.cat(idx)[..., None].expand(-1, -1, D)).contiguous()

        qi, ki = draw(q_video, qd), draw(k_video, kd)
    # (check_every=0: the reference's stopping rule evaluated on the device — same result, no read-back per iteration)
    grp = None if cfg == 1 else H   # (cfg == 1: the ungrouped loop, exactly as before)

    def run_q():
        return batch_kmeans_Euclid(q_video.reshape(cfg * H, N, D), num_q_centroids, max_iters=iters, init_centroids=qi,
                                   return_sorted_indices=True, check_every=0, shift_reduce=red, group=grp, **f8)

    def run_k():
        return batch_kmeans_Euclid(k_video.reshape(cfg * H, N, D), num_k_centroids, max_iters=iters, init_centroids=ki,
                                   return_sorted_indices=True, check_every=0, shift_reduce=red, group=grp, **f8)

    if red is not None and _kmeans_utils.STEPPED_LOOP_UNDER_SHARDS and q_video.is_cuda:
        # Sharded: the library's loop in steps (svg_kmeans_stepped_*), the two sides in lock-step.  Per iteration the q side's launches run on
        # the side stream beside the k side's; the ONE all-reduce over both sides' group maxima and the two commits follow on the current
        # stream, in the same order on every rank.  The element-wise MAX keeps each side's and each group's rule its own: the bits of the two
        # separate loops of the switch-off path below.
        xq, xk = q_video.reshape(cfg * H, N, D), k_video.reshape(cfg * H, N, D)
        G = 1 if grp is None else cfg   # (1e-4 below: the tol the loops of the other paths run with, batch_kmeans_Euclid's default)
        maxima = _native.empty((2 * G,), dtype=torch.float32, device=q_video.device)
        sides = [KmeansSteppedSide(xq, qi.reshape(cfg * H, num_q_centroids, D).contiguous(), 1e-4, group=grp, maxima=maxima[:G]),
                 KmeansSteppedSide(xk, ki.reshape(cfg * H, num_k_centroids, D).contiguous(), 1e-4, group=grp, maxima=maxima[G:])]
        beside = None
        if KMEANS_TWO_STREAMS:
            cur = torch.cuda.current_stream(q_video.device)
            side = _side_stream(q_video.device)

            def beside(runs):   # (every tensor of the q side is allocated on the current stream and outlives the last join)
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    runs[0]()
                runs[1]()
                cur.wait_stream(side)

        (ql, qc, qs, qit, qidx), (kl, kc, ks, kit, kidx) = (
            (lab.to(torch.int64), cent, cnt, n_it.to(torch.int64), srt)
            for lab, cent, cnt, n_it, srt in _kmeans_utils.lloyd_stepped(sides, maxima, iters, shift_reduce=red, beside=beside))
    elif KMEANS_TWO_STREAMS and red is None and q_video.is_cuda:
        # The two Lloyd loops are independent until the block map: the q side runs on a side stream beside the k side, so that the
        # HBM-bound update / sort / commit launches of one side share the chip with the MFMA-bound assignment of the other
        # (Wan 2.1 720p: 3.5 instead of 3.9 - 4.1 ms per layer-call, 86 instead of 99 ms for the 50-iteration init; bit-identical results —
        # profiles/r05d_svg2_two_streams.txt).  A sharded call keeps one stream: its stopping rule all-reduces on the current stream.
        cur = torch.cuda.current_stream(q_video.device)
        side = _side_stream(q_video.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            ql, qc, qs, qit, qidx = run_q()
        kl, kc, ks, kit, kidx = run_k()
        cur.wait_stream(side)
        for t_ in (ql, qc, qs, qit, qidx):   # allocated on the side stream's pool, consumed on the current stream from here on
            if isinstance(t_, torch.Tensor) and t_.is_cuda:
                t_.record_stream(cur)
    else:
        ql, qc, qs, qit, qidx = run_q()
        kl, kc, ks, kit, kidx = run_k()
    store.put(layer_idx, qc, kc, cfg)
    if first:
        print(f"Centroids initialized at layer {layer_idx}. Init step: {iter_init}")
    return (ql, qc, qs, qit, qidx), (kl, kc, ks, kit, kidx)


def _sparse_plus_centroid_tail(q, k, v, dyn_map, q_sizes, k_sizes, qidx, kidx, tail_k, KC: int, token_major: bool):
    """svg2_sparse_attention(centroid_tail=True) from the block map on: the sparse launch in its LSE form into a contiguous head-major
    part, the means of the call's own key clusters, the tail launch into the second part, and the merge — token-major wherever the plain
    call's output would be.  tail_k = (the video keys [cfg, H, V, D], their cluster sizes [cfg * H, KC], their sorted indices [cfg * H, V])
    as the k-means returned them.  -> (out, merged lse [cfg, H, S])"""
    cfg, H, S, D = q.shape
    QB, KB = q_sizes.shape[-1], k_sizes.shape[-1]
    maps = dyn_map.view(cfg * H, QB, KB).contiguous()
    qsz, rows = q_sizes.view(cfg * H, QB).contiguous(), qidx.contiguous()
    o_s, lse_s = _native.varblock_attention(q, k, v, maps, qsz, k_sizes.view(cfg * H, KB).contiguous(), q_row_idx=rows,
                                            kv_row_idx=kidx.contiguous(), rows_covered=True, return_lse=True)
    kv, ks, kidx_v = tail_k
    V = kv.shape[2]
    ks, kidx_v = ks.reshape(cfg * H, KC).contiguous(), kidx_v.reshape(cfg * H, V).contiguous()
    kbar = _native.cluster_means(kv, kidx_v, ks)
    vbar = _native.cluster_means(v[:, :, :V], kidx_v, ks)   # (a view of the caller's v: read in place, token-major or not)
    if KB != KC:   # HunyuanVideo: the last block-row — the unused prompt — selects nothing but itself; its rows get no tail
        maps = maps.clone()
        maps[:, -1, :] = True
    o_t, lse_t = _native.centroid_tail_attention(q, kbar, vbar, maps, qsz, ks, q_row_idx=rows)
    return _native.merge_attention_states([o_s.reshape(cfg, H, S, D), o_t.reshape(cfg, H, S, D)],
                                          [lse_s.reshape(cfg, H, S), lse_t.reshape(cfg, H, S)], token_major_out=token_major, return_lse=True)


def svg2_sparse_attention(q, k, v, geo: Geometry, store: CentroidStore, layer_idx: int, num_q_centroids: int,
                          num_k_centroids: int, top_p: float, min_kc_ratio: float, iter_init: int, iter_step: int,
                          prompt_length=0, logging_file: Optional[str] = None, timestep=None, _head_shard=None,
                          quality: Optional["QualityRequest"] = None, adaptive: Optional[AdaptiveTopP] = None,
                          top_p_store: Optional[TopPStore] = None, kmeans_e4m3: bool = False, centroid_tail: bool = False):
    """The sparse branch of the SAP processors (ref: hyvideo/attention.py:747-804, wan/attention.py:529-559):
    k-means on the video tokens -> top-p block map -> (Hunyuan) two pseudo clusters for prompt / unused prompt ->
    variable-block attention with the token permutation fused in (the result is already in the original order).
    q, k, v: [cfg, H, S, D]; cfg > 1 (several videos: a list of prompts, num_videos_per_prompt > 1) clusters each video with its own
    stopping rule, so every video's output, labels and block map are the ones a cfg = 1 call on that video alone gives.
    prompt_length: one int for the batch, or a sequence of cfg ints, one per video — the sizes of the two text pseudo-clusters are per
    head in the kernel already, so the videos still share one launch.
    quality: a QualityRequest (quality_request): the call is probed as well and its record, with the per-head densities, queued
    (log_quality).  The kept mass is logged where svg_varblock_attention_lse runs the body the plain call runs — head_dim 128, 16-bit,
    block-rows large enough for the two-phase body (S >= 160 block-rows) — elsewhere the error alone.  Refused under svg.distributed.
    adaptive: an AdaptiveTopP, with top_p_store a TopPStore: the block map of this call is built from the store's per-head thresholds of
    the layer (its first sparse call fills them with `top_p`), the attention runs its LSE form, K is probed on rows from the probe's
    generator (neither the global RNG nor the switched path's generator moves) and svg_top_p_update steps the thresholds for the layer's
    next call — all on the device, no host synchronisation.  With `quality` as well the rows are drawn once and its one dense probe feeds
    both.  ValueError, before anything runs, where the launch has no LSE form (head_dim other than 128, fp8, S < 160 block-rows);
    NotImplementedError under svg.distributed.  None: nothing changes.
    kmeans_e4m3: the k-means of this call assigns with e4m3 operands in all but its last iteration (kmeans_clustering(e4m3=True));
    NotImplementedError under svg.distributed.  False: nothing changes.
    centroid_tail: the key clusters the block map does not select are not dropped: each enters its rows as one pseudo key — the mean key and
    the mean value of the cluster (cluster_means of THIS call's labels: Jensen's bound needs the mean, the stored centroids may be one
    update away), weighted with the cluster's size (include/svg_attn_centroid_tail.h) — and that state is merged with the sparse call's
    (merge_attention_states).  HunyuanVideo: the video clusters only, and the unused-prompt rows get no tail.  A `quality` record is then
    measured on the merged output and lse and carries "centroid_tail": true.  NotImplementedError under svg.distributed; ValueError
    together with `adaptive`, and where the launch has no LSE form (the rule of `adaptive`).  False: nothing changes."""
    if kmeans_e4m3:
        _refuse_kmeans_e4m3_when_sharded("svg2_sparse_attention", _head_shard)
    if centroid_tail:
        _refuse_centroid_tail("svg2_sparse_attention", q, num_q_centroids + (2 if geo.context_length else 0), adaptive, _head_shard)
    if quality is not None:
        _refuse_quality_when_sharded("svg2_sparse_attention")
    if adaptive is not None:
        _refuse_kept_mass_knob_when_sharded("svg2_sparse_attention", "adaptive_top_p")
        if top_p_store is None:
            raise ValueError("svg2_sparse_attention(adaptive=...) needs a top_p_store (TopPStore): the thresholds live there between calls")
        # (block-rows of the launch: the query clusters, and Hunyuan's two text pseudo-clusters behind them)
        _refuse_adaptive_without_lse("svg2_sparse_attention", q, num_q_centroids + (2 if geo.context_length else 0))
    _require_gpu(q, "SVG2 sparse attention")
    pl = per_video(prompt_length, q.shape[0], "svg2_sparse_attention(prompt_length)")
    if pl is not None:
        pl = [int(x) for x in pl]
        prompt_length = pl[0] if len(set(pl)) == 1 else tuple(pl)
        if isinstance(prompt_length, tuple):
            _no_sharding_of_groups("SVG2 sparse attention")
    if (_dist.active() or _dist.token_shards_active()) and _head_shard is None:
        grp = _dist.head_mode()[1]
        mine = _dist.shard_heads(q.shape[1], torch.distributed.get_rank(grp), torch.distributed.get_world_size(grp))
        shard = (mine[0], mine[-1] + 1, q.shape[1]) if mine else (0, 0, q.shape[1])
        if _dist.token_shards_active():   # q, k, v: this rank's rows; whole heads of the whole sequence inside, rows back
            return _dist.run_token_sharded(lambda qh, kh, vh: svg2_sparse_attention(
                qh, kh, vh, geo, store, layer_idx, num_q_centroids, num_k_centroids, top_p, min_kc_ratio, iter_init, iter_step,
                prompt_length, logging_file, timestep, _head_shard=shard), (q, k, v), geo.seq_len, grp)
        # svg.distributed.enable(): this rank's heads only, outputs all-gathered
        return _dist.run_sharded(lambda qh, kh, vh: svg2_sparse_attention(
            qh, kh, vh, geo, store, layer_idx, num_q_centroids, num_k_centroids, top_p, min_kc_ratio, iter_init, iter_step,
            prompt_length, logging_file, timestep, _head_shard=shard), (q, k, v), grp)
    cfg, H, S, D = q.shape
    assert not geo.text_first, "SVG2 is defined for text-last models (Hunyuan, Wan)"
    V, ctx = geo.video_length, geo.context_length
    q, k = q.contiguous(), k.contiguous()   # (the k-means reads them as [H, N, D]; v may stay a strided view: only the attention kernel reads it)
    # the video tokens as VIEWS when the loop runs inside the library (svg_kmeans_loop[_grouped]_strided reads heads S * D apart in place:
    # the cfg * H heads of a contiguous [cfg, H, S, D] are uniformly S * D apart), and when a shard's loop runs in steps
    # (svg_kmeans_stepped_iterate reads the same views); the torch statement of the loop (sharded, STEPPED_LOOP_UNDER_SHARDS off) takes the
    # copies the reference makes
    in_place = ctx and ((_head_shard is None and not _dist.active()) or (_head_shard is not None and _kmeans_utils.STEPPED_LOOP_UNDER_SHARDS))
    qv = (q[:, :, :V] if in_place else q[:, :, :V].contiguous()) if ctx else q
    kv = (k[:, :, :V] if in_place else k[:, :, :V].contiguous()) if ctx else k
    with time_logging_decorator("Level 3 - semantic aware permutation"):
        (ql, qc, qs, _, qidx), (kl, kc, ks, _, kidx) = kmeans_clustering(store, layer_idx, qv, kv, num_q_centroids,
                                                                         num_k_centroids, iter_init, iter_step,
                                                                         head_shard=_head_shard, **({"e4m3": True} if kmeans_e4m3 else {}))
        q_sizes = qs.view(cfg, H, num_q_centroids)
        k_sizes = ks.view(cfg, H, num_k_centroids)
        p_heads = None if adaptive is None else top_p_store.get(layer_idx, cfg * H, top_p, q.device)
        dyn_map = identify_dynamic_map(qc.view(cfg, H, num_q_centroids, D), kc.view(cfg, H, num_k_centroids, D), q_sizes,
                                       k_sizes, top_p if adaptive is None else p_heads.view(cfg, H), min_kc_ratio)
    tail_k = (kv, ks, kidx) if centroid_tail else None   # (the video keys, their cluster sizes and sorted indices, before the text clusters)
    if ctx:
        with time_logging_decorator("Level 3 - dynamic map post processing"):
            dyn_map, q_sizes, k_sizes, qidx, kidx = dynamic_map_post_processing(dyn_map, q_sizes, k_sizes, qidx, kidx, V, ctx,
                                                                                prompt_length)
    QB, KB = q_sizes.shape[-1], k_sizes.shape[-1]
    f8 = _use_fp8(q)
    # (rows_covered: the cluster sizes of every head add up to S — k-means counts over the V video tokens plus the text pseudo-clusters of
    #  dynamic_map_post_processing — so the kernel writes every output row and the wrapper skips the zero fill)
    # (one launch over the cfg * H heads; the token-major output is [cfg, S, H, D] in memory: svg_attn_layout_t with heads_per_batch = H)
    # (the LSE entry always runs the two-phase 16x16x32 body; the plain call picks it from S >= 160 QB on: only there is its o the same)
    probe_lse = adaptive is not None or (quality is not None and _quality_lse_form(q, False) and S >= 160 * QB)
    token_major = TOKEN_MAJOR_IO and (_head_shard is None or _dist.token_shards_active())
    if centroid_tail:
        out, lse_p = _sparse_plus_centroid_tail(q, k, v, dyn_map, q_sizes, k_sizes, qidx, kidx, tail_k, num_k_centroids, token_major)
    else:
        out = _native.varblock_attention(q, k, v, dyn_map.view(cfg * H, QB, KB).contiguous(),
                                         q_sizes.view(cfg * H, QB).contiguous(), k_sizes.view(cfg * H, KB).contiguous(),
                                         q_row_idx=qidx.contiguous(), kv_row_idx=kidx.contiguous(), fp8=f8, token_major_out=token_major,
                                         rows_covered=True, return_lse=probe_lse)
        out, lse_p = out if probe_lse else (out, None)
    plan = lse_d = None
    if adaptive is not None:   # the rows of this call, drawn once: the quality probe below measures on them as well
        plan = _knob_probe_plan(quality, adaptive, cfg, S)
    if quality is not None:
        lse_d = log_quality(quality, out, lse_p, q, k, v, density=density_calculation(dyn_map, q_sizes, k_sizes), plan=plan,
                            top_p=None if adaptive is None else p_heads.clone(), **({"centroid_tail": True} if centroid_tail else {}))
    if adaptive is not None:
        adaptive_step(adaptive, top_p_store, layer_idx, p_heads, lse_p, q, k, plan, lse_d)
    if logging_file is not None:
        from .context import timestep_value

        densities = density_calculation(dyn_map, q_sizes, k_sizes)
        if _head_shard is not None:   # one log line per layer-call with all heads, written by rank 0
            densities = _dist.all_gather_heads(densities.reshape(cfg, H, 1, 1), _head_shard[2], _dist.head_mode()[1]).reshape(cfg, -1)
        if _head_shard is None or torch.distributed.get_rank(_dist.head_mode()[1]) == 0:
            DENSITY_LOG.push(logging_file, {"timestep": timestep_value(timestep) if timestep is not None else None,
                                            "layer": layer_idx}, densities)
    return out.reshape(cfg, H, S, D)   # (out is [cfg, H, S, D] already, in either storage order: a view)


# ---------------------------------------------------------------------------------------------------------------
# attention_core_logic of the processors, one body per method.  What a model family does differently is an argument of
# its processor's one call:
#   valid_lens(cfg, geo) HunyuanVideo: the dense `valid` of the call (video_valid_lens) — the quality probe, the dense masks of the
#                        switch, the knob's probe and the dense call follow it — and with it masks per video (a block_mask tuple)
#   dense(q, k, v, valid, geo)  HunyuanVideo: _core.dense_attention itself; without it the processor's flash_attention (Wan, Cosmos,
#                        CogVideoX), whose decorator enters dense_attention's timer label a second time
#   shard_form           the frame-shard form of rows_of_this_rank: the class's frame_shard_form; CogVideoX has none and passes False
# ---------------------------------------------------------------------------------------------------------------
def _core_logic_setup(proc, query, timestep, shard_form, valid_lens):
    """What every attention_core_logic starts with -> (geometry, valid, quality request)"""
    cfg, seq_len = query.shape[0], query.shape[2]
    geo, name = proc.geometry(), type(proc).__name__
    assert seq_len == rows_of_this_rank(name, geo, shard_form), (
        f"Query Shape: {seq_len} is not equivalent to {geo.context_length} + {geo.num_frame} * {geo.frame_size}")
    valid = valid_lens(cfg, geo) if valid_lens is not None else None
    return geo, valid, quality_request(name, proc.quality_log, proc.quality_rows, valid, timestep, proc.layer_idx)


def _knob(proc, option: str, valid_lens, valid):
    """The processor's kept-mass knob (adaptive_band / adaptive_top_p) for this call, refused when sharded; HunyuanVideo: the probe's rows and
    keys follow the call's valid lengths"""
    knob = getattr(proc, option)
    if knob is None:
        return None
    _refuse_kept_mass_knob_when_sharded(type(proc).__name__, option)
    return knob if valid_lens is None else dataclasses.replace(knob, valid_len=valid)


def svg1_core_logic(proc, query, key, value, timestep, profile_desc, owner: str, install_hook: str, *, valid_lens=None, dense=None,
                    shard_form=None, thresholds=None, band_knob: bool = True, whole_sequence_rows: bool = False):
    """attention_core_logic of the SVG1 processors: the warm-up test — on the host by layer, on the device by timestep where the
    timestep is a GPU tensor (device_switch) — then the dense call, svg1_attention_device_switch or svg1_sparse_attention.
    profile_desc: the model's (its utils); owner, install_hook: the class and function the "block_mask is not set" error names.
    thresholds: (first_layers, first_times) where they are not the class's own (CogVideoX scales them); band_knob False: no adaptive_band
    (CogVideoX); whole_sequence_rows: the profiler's rows come from the whole sequence, not from the first sample_mse_max_row (CogVideoX)."""
    shape = query.size()
    geo, valid, quality = _core_logic_setup(proc, query, timestep, proc.frame_shard_form if shard_form is None else shard_form, valid_lens)
    cfg, total = shape[0], geo.seq_len   # (total: seq_len, except in the sharded modes: the masks and the sampled rows are the whole sequence's)
    first_layers, first_times = thresholds if thresholds is not None else (proc.first_layers_fp, proc.first_times_fp)
    ab = {}
    if band_knob and proc.adaptive_band is not None:
        ab = dict(adaptive=_knob(proc, "adaptive_band", valid_lens, valid), band_store=proc.band_store, layer_idx=proc.layer_idx)
    # the layer test is host data; the timestep test stays on the device when the timestep is a GPU tensor (device_switch)
    dense_flag = None
    if proc.device_switch and attention_dtype() == "bf16" and proc.fused_placement and proc.layer_idx >= first_layers \
            and proc.block_mask is not None and query.is_cuda:
        dense_flag = dense_flag_on_device(timestep, first_times)
    if dense_flag is None and is_full_attention(proc.layer_idx, timestep, first_layers, first_times):
        out = proc.flash_attention(query, key, value) if dense is None else dense(query, key, value, valid, geo)
        return out.reshape(shape)
    mask = proc.block_mask   # (HunyuanVideo: or a tuple, one mask per video, as prompt_length)
    if mask is None:
        raise RuntimeError(f"{owner}.block_mask is not set: call {install_hook} first")
    if valid_lens is not None and isinstance(mask, tuple) and len(mask) != cfg:
        raise ValueError(f"{owner}: block_mask has {len(mask)} entries for a batch of {cfg} videos")
    prof = profile_desc(geo.context_length, geo.num_frame, geo.frame_size)
    max_row = total if whole_sequence_rows else min(proc.sample_mse_max_row, total)
    if dense_flag is not None:
        dense_masks = tuple(_dense_band_mask(total, x) for x in valid) if isinstance(valid, tuple) else _dense_band_mask(total, valid)
        out, best = svg1_attention_device_switch(query, key, value, geo, mask, dense_masks, prof, proc.num_sampled_rows, max_row, dense_flag,
                                                 q_prescaled=proc._q_prescaled, quality=quality, **ab)
    else:
        out, best = svg1_sparse_attention(query, key, value, geo, mask, prof, proc.num_sampled_rows, max_row, fused=proc.fused_placement,
                                          q_prescaled=proc._q_prescaled, quality=quality, **ab)
    proc.last_best_mask_idx = best
    return out.reshape(shape)


def svg2_core_logic(proc, query, key, value, timestep, layer_idx, prompt_length, *, valid_lens=None, dense=None):
    """attention_core_logic of the SAP processors: the warm-up test on the host, then the dense call (zero_step_kmeans_init: the layer's
    k-means runs on dense steps too) or svg2_sparse_attention.  layer_idx: the key of the layer's centroids and thresholds — the stores
    are the processor's, class-level or per instance as the family keeps them; prompt_length: 0, the class's integer or a tuple with one entry
    per video."""
    shape = query.size()
    geo, valid, quality = _core_logic_setup(proc, query, timestep, proc.frame_shard_form, valid_lens)
    adaptive = _knob(proc, "adaptive_top_p", valid_lens, valid)
    e4m3 = {}   # (off: the calls below are the calls of before, argument for argument)
    if proc.kmeans_e4m3:
        _refuse_kmeans_e4m3_when_sharded(type(proc).__name__)
        e4m3 = dict(e4m3=True)
    if proc.centroid_tail:   # (on dense steps too: every rank refuses on its first call)
        _refuse_centroid_tail_when_sharded(type(proc).__name__)
    if is_full_attention(proc.layer_idx, timestep, proc.first_layers_fp, proc.first_times_fp):
        if proc.zero_step_kmeans_init and query.is_cuda:
            V = geo.video_length
            kmeans_clustering(proc.centroid_store, layer_idx, query[:, :, :V], key[:, :, :V],   # (views: read in place)
                              proc.num_q_centroids, proc.num_k_centroids, proc.kmeans_iter_init, proc.kmeans_iter_step, **e4m3)
        out = proc.flash_attention(query, key, value) if dense is None else dense(query, key, value, valid, geo)
        return out.reshape(shape)
    out = svg2_sparse_attention(query, key, value, geo, proc.centroid_store, layer_idx, proc.num_q_centroids, proc.num_k_centroids,
                                proc.top_p_kmeans, proc.min_kc_ratio, proc.kmeans_iter_init, proc.kmeans_iter_step,
                                prompt_length=prompt_length if isinstance(prompt_length, tuple) else int(prompt_length),
                                logging_file=proc.logging_file, timestep=timestep, quality=quality, adaptive=adaptive, top_p_store=proc.top_p_store,
                                **({"kmeans_e4m3": True} if e4m3 else {}), **({"centroid_tail": True} if proc.centroid_tail else {}))
    return out.reshape(shape)


class _DensityLog:
    """Density logging off the critical path.  The reference reads `densities.mean().item()` / `.tolist()` back in
    every sparse layer-call (hyvideo/attention.py:786-802): one device synchronisation per layer.  Here the per-head densities are
    copied to pinned host memory asynchronously and the JSON lines (same fields, same order) are written once their copy has
    completed — opportunistically on later calls, and in any case by `flush()` (registered with atexit; call it before reading
    the file)."""

    def __init__(self):
        self.pending = []   # (path, meta, pinned host tensor, event)

    def push(self, path: str, meta: dict, densities: torch.Tensor) -> None:
        host = _native.empty(densities.shape, dtype=torch.float32, pin_memory=densities.is_cuda)
        host.copy_(densities.float(), non_blocking=True)
        ev = None
        if densities.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        self.pending.append((path, meta, host, ev))
        self.flush(wait=False)

    def flush(self, wait: bool = True) -> None:
        while self.pending:
            path, meta, host, ev = self.pending[0]
            if ev is not None:
                if wait:
                    ev.synchronize()
                elif not ev.query():
                    return
            entry = dict(meta, avg_density=float(host.mean()), density=host.tolist())
            if host.dim() == 2 and host.shape[0] > 1:   # several videos: their own averages too (a cfg == 1 entry is unchanged)
                entry["video_avg_density"] = [float(r.mean()) for r in host]
            with open(path, "a") as f:
                f.write(json.dumps(entry) + "\n")
            self.pending.pop(0)


DENSITY_LOG = _DensityLog()


def flush_density_log() -> None:
    """Write every pending density record (see _DensityLog)."""
    DENSITY_LOG.flush(wait=True)


import atexit  # noqa: E402

atexit.register(flush_density_log)


# ---------------------------------------------------------------------------------------------------------------
# Quality probe: what a sparse layer-call cost in accuracy.  The density log says how much compute was kept; this says how much ATTENTION
# was kept and what the output lost, on a few sampled rows per head: the dense truth of those rows from one pass over K and V
# (svg/_probe.py sample_dense_rows), the sparse call's own output and — where the launch has an LSE form — its row log-sum-exp.
#   kept mass of a row = exp(lse_sparse - lse_dense): the share of the dense softmax row on the keys the sparse form kept
#   output error       = o_sparse - o_dense
# ---------------------------------------------------------------------------------------------------------------
def quality_figures(o_s: torch.Tensor, lse_s, o_d: torch.Tensor, lse_d: torch.Tensor) -> dict:
    """The figures of sparse_quality from the gathered rows: o_s [cfg, H, R, D] (any float type), lse_s [cfg, H, R] or None, o_d / lse_d
    the dense rows.  A row the sparse form gives no key (lse_s = -inf) has kept mass 0."""
    diff = o_s.float() - o_d.float()
    num = diff.square().sum(dim=(-2, -1))
    out = {"rel_l2": torch.sqrt(num / o_d.float().square().sum(dim=(-2, -1))), "mse": diff.square().mean(dim=(-2, -1)), "kept_mass": None}
    if lse_s is not None:
        out["kept_mass"] = torch.exp(lse_s.float() - lse_d.float()).mean(dim=-1)
    return out


def sparse_quality(o_sparse: torch.Tensor, lse_sparse, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, rows: torch.Tensor, valid_len=None,
                   sm_scale: Optional[float] = None, dense_lse_out: Optional[list] = None) -> dict:
    """A sparse attention result against dense attention on the sampled `rows` (int64 [R], R <= 64, CPU or device):
    {"rel_l2" [cfg, H]: sqrt(sum_rows |o_s - o_d|^2 / sum_rows |o_d|^2), "mse" [cfg, H]: mean squared difference over rows and D,
    "kept_mass" [cfg, H]: mean over rows of exp(lse_s - lse_d), None when lse_sparse is None} — device tensors, no host synchronisation.
    o_sparse [cfg, H, S, D] and lse_sparse [cfg, H, S] (or [cfg * H, S]) are the sparse call's FULL outputs in the caller's row order,
    head-major or token-major storage alike (views); the rows are gathered here.  q, k, v [cfg, H, S, D] views, valid_len as in
    dense_attention (one int), sm_scale as in the attention wrappers (LN2 for a q that carries the softmax scale).  GPU only.
    dense_lse_out: a list that receives the probe's dense lse [cfg, H, R] (the adaptive top-p steers by it)."""
    from .. import _probe

    cfg, H, S, D = q.shape
    o_d, lse_d = _probe.sample_dense_rows(q, k, v, rows, valid_len, sm_scale)
    idx = rows.to(q.device, non_blocking=True)
    o_s = o_sparse.reshape(cfg, H, S, D).index_select(2, idx) if o_sparse.dim() != 4 else o_sparse.index_select(2, idx)
    lse_s = None if lse_sparse is None else lse_sparse.reshape(cfg, H, S).index_select(2, idx)
    if dense_lse_out is not None:
        dense_lse_out.append(lse_d)
    return quality_figures(o_s, lse_s, o_d, lse_d)


_PROBE_GEN = None
_PROBE_SEED = None
_PROBE_SALT = 0x51A17E   # the probe's stream is the global seed's, offset: never the rows the switched path draws


def reseed_probe_generator(seed: Optional[int] = None) -> None:
    """(Re)build the CPU generator of the quality probe's rows from `seed` (default: the global seed, torch.initial_seed())."""
    global _PROBE_GEN, _PROBE_SEED
    base = torch.initial_seed() if seed is None else int(seed)
    _PROBE_GEN = torch.Generator().manual_seed((base + _PROBE_SALT) % (2 ** 63))
    _PROBE_SEED = torch.initial_seed()


def _probe_generator():
    """CPU generator of the quality probe's rows, beside `_switch_generator`: derived from the global seed, re-derived when
    torch.initial_seed() changes.  Drawing from it advances neither the global CPU stream nor the switched path's generator, so a
    processor with `quality_log` set computes the attention output and best_mask_idx it computes without."""
    if _PROBE_GEN is None or _PROBE_SEED != torch.initial_seed():
        reseed_probe_generator()
    return _PROBE_GEN


@dataclass
class QualityRequest:
    """What a processor with `quality_log` set hands its core call: where to log, how many rows to probe, the dense `valid` of the call
    (an int, a tuple with one entry per video, or None) and the record's timestep / layer."""
    path: str
    rows: int = 64
    valid_len: object = None
    timestep: object = None
    layer: Optional[int] = None


def _refuse_quality_when_sharded(what: str) -> None:
    # (the modes' own switches, whatever the group's size: a group of one rank refuses like every other, so all ranks raise together)
    if _dist._STATE["enabled"] or _dist.frame_shards_active() or _dist.token_shards_active():
        raise NotImplementedError(f"{what}: quality_log under svg.distributed (enable, enable_frame_shards, enable_token_shards) is not "
                                  f"implemented: the probe reads whole heads of the whole sequence; unset quality_log or run on one GPU")


def quality_request(what: str, path, rows: int, valid_len=None, timestep=None, layer=None) -> Optional[QualityRequest]:
    """The processors' hook: None without a path (nothing changes); with one, the request — refused under every mode of svg.distributed,
    on the host, before any collective, on every rank alike."""
    if path is None:
        return None
    _refuse_quality_when_sharded(what)
    return QualityRequest(str(path), int(rows), valid_len, timestep, layer)


def _quality_lse_form(q: torch.Tensor, q_prescaled: bool, fused: bool = True) -> bool:
    """does the sparse launch have a form that also returns the row log-sum-exp (with the same o)?  head_dim 128, 16-bit, plain q, fused"""
    return bool(fused and not q_prescaled and not _use_fp8(q) and q.shape[-1] == 128 and q.dtype in (torch.bfloat16, torch.float16))


class _QualityLog:
    """The deferred writer of the quality records, the machinery of _DensityLog: the figures of a layer-call travel to pinned host memory
    in one asynchronous copy and the JSON line {"timestep", "layer", "rel_l2", "mse", "kept_mass" (null without an LSE form), "density"
    (SVG2)} is written once the copy has completed — opportunistically on later calls, and by flush().  A record that carries the
    device-switch flag of a DENSE step is dropped: the host does not know the step's kind when it launches the probe."""

    def __init__(self):
        self.pending = []   # (path, meta, shape, has kept mass, has density, has flag, has timestep, pinned host tensor, event[, has top_p])

    def push(self, path: str, meta: dict, figures: dict, density=None, dense_flag=None, timestep=None, top_p=None, band=None) -> None:
        """timestep: a device tensor whose first element is the record's timestep, read with the figures (no read-back on the host).
        top_p [cfg * H] (the adaptive SVG2 path): the thresholds the call ran with — the record gains a "top_p" list, and only then;
        band [cfg * H] (the adaptive SVG1 path): the bands the call ran with — a "band" list of integers, likewise"""
        rel = figures["rel_l2"]
        parts = [rel.float().reshape(-1), figures["mse"].float().reshape(-1)]
        kept = figures.get("kept_mass")
        if kept is not None:
            parts.append(kept.float().reshape(-1))
        if density is not None:
            parts.append(density.float().reshape(-1))
        if top_p is not None:
            parts.append(top_p.float().reshape(-1))
        if band is not None:   # (bands are at most S + 1 < 2^24: exact in fp32)
            parts.append(band.float().reshape(-1))
        if dense_flag is not None:
            parts.append(dense_flag.reshape(-1)[:1].float())
        if timestep is not None:
            parts.append(timestep.reshape(-1)[:1].float())
        flat = torch.cat(parts)
        host = _native.empty(flat.shape, dtype=torch.float32, pin_memory=flat.is_cuda)
        host.copy_(flat, non_blocking=True)
        ev = None
        if flat.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        self.pending.append((path, meta, tuple(rel.shape), kept is not None, density is not None, dense_flag is not None,
                             timestep is not None, host, ev, top_p is not None, band is not None))
        self.flush(wait=False)

    def flush(self, wait: bool = True) -> None:
        while self.pending:
            path, meta, shape, has_kept, has_density, has_flag, has_ts, host, ev, *more = self.pending[0]
            has_top_p = bool(more and more[0])   # (the thresholds of the adaptive SVG2 path, where the record carries them)
            has_band = bool(len(more) > 1 and more[1])   # (the bands of the adaptive SVG1 path)
            if ev is not None:
                if wait:
                    ev.synchronize()
                elif not ev.query():
                    return
            n = 1
            for s in shape:
                n *= s
            take = lambda i: host[i * n:(i + 1) * n].reshape(shape).tolist()   # noqa: E731
            if not (has_flag and float(host[-1 - int(has_ts)]) != 0.0):
                if has_ts:
                    meta = dict(meta, timestep=float(host[-1]))
                entry = dict(meta, rel_l2=take(0), mse=take(1), kept_mass=take(2) if has_kept else None)
                if has_density:
                    entry["density"] = take(2 + int(has_kept))
                if has_top_p:
                    entry["top_p"] = take(2 + int(has_kept) + int(has_density))
                if has_band:
                    bands = host[(2 + int(has_kept) + int(has_density) + int(has_top_p)) * n:][:n].reshape(shape).tolist()
                    entry["band"] = [[int(b) for b in row] for row in bands] if len(shape) == 2 else bands
                with open(path, "a") as f:
                    f.write(json.dumps(entry) + "\n")
            self.pending.pop(0)


QUALITY_LOG = _QualityLog()


def flush_quality_log() -> None:
    """Write every pending quality record (see _QualityLog)."""
    QUALITY_LOG.flush(wait=True)


atexit.register(flush_quality_log)


def log_quality(quality: QualityRequest, out: torch.Tensor, lse, q, k, v, q_prescaled: bool = False, dense_flag=None, density=None,
                plan=None, top_p=None, band=None, centroid_tail: bool = False):
    """Probe one sparse layer-call (out [cfg, H, S, D] in either storage order, lse [cfg, H, S] or None) and queue its record.  Rows:
    uniform over the valid rows of the sequence, from the probe's own CPU generator.  Videos whose valid lengths differ are probed group by
    group (video_groups), one native call per group.
    plan: the rows, where the caller has drawn them already (probe_plan); top_p [cfg * H]: the thresholds the call ran with, for the record
    (the adaptive SVG2 path); band [cfg * H]: the bands it ran with (the adaptive SVG1 path).  -> the dense lse of the probed rows, one [nb, H, R] per group, for a caller that steers by it."""
    from .context import timestep_value

    cfg, H, S, D = q.shape
    out = out.reshape(cfg, H, S, D)
    lse = None if lse is None else lse.reshape(cfg, H, S)
    figs, lse_dense = [], []
    for sl, vl, rows in plan if plan is not None else probe_plan(quality.valid_len, quality.rows, cfg, S):
        want = {} if plan is None else {"dense_lse_out": lse_dense}   # (asked for by the caller that drew the plan, nobody else)
        figs.append(sparse_quality(out[sl], None if lse is None else lse[sl], q[sl], k[sl], v[sl], rows, vl, LN2 if q_prescaled else None, **want))
    fig = {key: (None if figs[0][key] is None else torch.cat([f[key] for f in figs])) for key in figs[0]}
    ts = quality.timestep
    on_device = torch.is_tensor(ts) and ts.is_cuda   # (the switched path never reads the timestep back: it travels with the figures)
    meta = {"timestep": None if ts is None or on_device else timestep_value(ts), "layer": quality.layer}
    if centroid_tail:   # (the record of a call whose output and lse are the merged ones; without the option the record is the one of before)
        meta["centroid_tail"] = True
    QUALITY_LOG.push(quality.path, meta, fig, density=density, dense_flag=dense_flag, timestep=ts if on_device else None, top_p=top_p,
                     **({} if band is None else {"band": band}))
    return lse_dense


_SMALL_TENSORS = {}   # (values, dtype, device) -> tensor: a batch's prompt lengths, uploaded once and not once per layer-call


def _small_tensor(values: tuple, dtype, device) -> torch.Tensor:
    key = (values, dtype, str(device))
    if key not in _SMALL_TENSORS:
        if len(_SMALL_TENSORS) > 8:
            _SMALL_TENSORS.clear()
        _SMALL_TENSORS[key] = torch.tensor(values, dtype=dtype, device=device)
    return _SMALL_TENSORS[key]


def dynamic_map_post_processing(dyn_map, qc_sz, kc_sz, q_sorted_indices, k_sorted_indices, video_length, context_length,
                                prompt_length):
    """ref: hyvideo/attention.py:657-702 — append the prompt / unused-prompt pseudo clusters (prompt_length: one int, or a sequence of
    cfg ints: the two sizes are then per video).  The q,k,v write-back of
    the reference (permuted video tokens copied in front of the text tokens) is not needed: the attention kernel
    gathers rows through the (identity-padded) sorted indices."""
    dyn_map = F.pad(dyn_map, (0, 2, 0, 2), value=0)
    dyn_map[:, :, -2, :-1] = True
    dyn_map[:, :, :-1, -2] = True
    dyn_map[:, :, -1, -1] = True
    pl = per_video(prompt_length, qc_sz.shape[0], "dynamic_map_post_processing(prompt_length)")
    if pl is not None:   # per video: [cfg, 1] against the [cfg, H] columns of the sizes
        prompt_length = _small_tensor(tuple(int(x) for x in pl), qc_sz.dtype, qc_sz.device).view(-1, 1)
    unprompt = context_length - prompt_length
    qc_sz = F.pad(qc_sz, (0, 2), value=0)
    qc_sz[:, :, -2] = prompt_length
    qc_sz[:, :, -1] = unprompt
    kc_sz = F.pad(kc_sz, (0, 2), value=0)
    kc_sz[:, :, -2] = prompt_length
    kc_sz[:, :, -1] = unprompt
    tail = torch.arange(video_length, video_length + context_length, device=q_sorted_indices.device, dtype=torch.int32)
    tail = tail.expand(q_sorted_indices.shape[0], -1)
    q_sorted_indices = torch.cat([q_sorted_indices, tail], dim=1)
    k_sorted_indices = torch.cat([k_sorted_indices, tail], dim=1)
    return dyn_map, qc_sz, kc_sz, q_sorted_indices, k_sorted_indices


# ---------------------------------------------------------------------------------------------------------------------
# Pre-attention prologue on libsvgattn (the reference's `_kernels` fast path: hyvideo/attention.py:157-188,
# wan/attention.py:42-48, cog/attention.py:19-34).  Each helper returns False when the HIP path does not apply (CPU tensors,
# unsupported head_dim / dtype, a norm module it does not recognise) so that the caller runs the model's own torch modules —
# exactly the reference's `except ImportError` branch.
# ---------------------------------------------------------------------------------------------------------------------
_FAST_DIMS = (32, 64, 128, 256)


def _fast_ok(*ts) -> bool:
    if not all(t.is_cuda for t in ts):
        return False                      # CPU tensors: the model's own torch modules (the reference's CPU-capable path)
    _native.load()                        # GPU tensors without the library: raise, never fall back silently
    return all(t.is_cuda and t.is_contiguous() and t.dtype in (torch.bfloat16, torch.float16) and t.dim() == 4
               and t.shape[-1] in _FAST_DIMS for t in ts)


def _norm_desc(norm, D: int, dtype, device):
    """(kind, weight, bias, eps) of an RMSNorm / LayerNorm over head_dim, or None if the module is something else."""
    if norm is None:
        return None
    w = getattr(norm, "weight", None)
    if w is not None and tuple(w.shape) != (D,):
        return None
    eps = getattr(norm, "eps", None)
    if eps is None:
        return None
    b = getattr(norm, "bias", None)
    is_layer = isinstance(norm, torch.nn.LayerNorm) or b is not None
    cast = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype).contiguous()  # noqa: E731
    return (2 if is_layer else 1), cast(w), cast(b), float(eps)


def qk_norm_inplace(norm_q, norm_k, query, key) -> bool:
    """In-place QK normalisation over head_dim (ref fast path: `_kernels.rms_norm_forward` / `layer_norm_forward`)."""
    if norm_q is None or norm_k is None or not _fast_ok(query, key):
        return False
    D = query.shape[-1]
    dq, dk = _norm_desc(norm_q, D, query.dtype, query.device), _norm_desc(norm_k, D, key.dtype, key.device)
    if dq is None or dk is None or dq[0] != dk[0] or dq[3] != dk[3]:
        return False
    if query.shape[0] == key.shape[0] and query.shape[2] == key.shape[2]:
        _native.qk_norm_rope(query, key, dq[0], dq[1], dq[2], dk[1], dk[2], dq[3])
    else:   # cross attention: different sequence lengths, one call per tensor
        _native.qk_norm_rope(query, None, dq[0], dq[1], dq[2], None, None, dq[3])
        _native.qk_norm_rope(key, None, dk[0], dk[1], dk[2], None, None, dk[3])
    return True


def _tables(a, b, rows: int, cols: int, device):
    a = a.detach().to(device=device, dtype=torch.float32).reshape(-1, a.shape[-1]).contiguous()
    b = b.detach().to(device=device, dtype=torch.float32).reshape(-1, b.shape[-1]).contiguous()
    return (a, b) if a.shape == (rows, cols) and b.shape == (rows, cols) else None


def _rope_kind(complex_pairs: bool, half_split: bool) -> int:
    """rope_kind of include/svg_attn.h: 1 interleaved pairs, 2 complex pairs, 3 half-split (channel i against i + D / 2)"""
    assert not (complex_pairs and half_split), "complex_pairs and half_split are mutually exclusive"
    return 2 if complex_pairs else 3 if half_split else 1


def qk_rope_inplace(query, key, cos, sin, rope_lo: int, rope_hi: int, complex_pairs: bool = False, norm_q=None,
                    norm_k=None, q_scale: float = 1.0, half_split: bool = False) -> bool:
    """In-place rotary embedding of positions [rope_lo, rope_hi) — optionally fused with the QK normalisation (one pass over
    q and k instead of three).  cos / sin: [rope_hi - rope_lo, D] fp32 (complex_pairs: real / imag [.., D / 2]).
    half_split: the two channel halves rotate against each other (Cosmos; tables [.., D], every column read) instead of neighbours.
    q_scale != 1: folded into the pass's last rounding of q (the attention core then runs its pre-scaled kernels)."""
    rk = _rope_kind(complex_pairs, half_split)
    if not _fast_ok(query, key) or rope_hi <= rope_lo:
        return False
    D = query.shape[-1]
    tb = _tables(cos, sin, rope_hi - rope_lo, D // 2 if complex_pairs else D, query.device)
    if tb is None:
        return False
    kind, qw, qb, kw, kb, eps = 0, None, None, None, None, 0.0
    if norm_q is not None or norm_k is not None:
        dq, dk = _norm_desc(norm_q, D, query.dtype, query.device), _norm_desc(norm_k, D, key.dtype, key.device)
        if dq is None or dk is None or dq[0] != dk[0] or dq[3] != dk[3]:
            return False
        kind, qw, qb, kw, kb, eps = dq[0], dq[1], dq[2], dk[1], dk[2], dq[3]
    _native.qk_norm_rope(query, key, kind, qw, qb, kw, kb, eps, rk, tb[0], tb[1], rope_lo, rope_hi, q_scale=q_scale)
    return True


def prescale_supported(query) -> bool:
    """the pre-scaled attention kernels exist for 16-bit GPU tensors with head_dim 64 / 128"""
    return bool(query.is_cuda and query.dtype in (torch.bfloat16, torch.float16) and query.shape[-1] in (64, 128))


def value_in_place(value: torch.Tensor, heads: int):
    """The v projection's output [bsz, S, heads * D] as the [bsz, heads, S, D] VIEW the attention kernels read in place
    (svg_attn_layout_t; TOKEN_MAJOR_IO, one GPU, head_dim 64 / 128, 16-bit, on the GPU) — or None: the caller makes the head-major copy.
    Token-shard mode (svg.distributed.enable_token_shards) takes the view as well: run_token_sharded's inbound pack reads it in place."""
    if not (TOKEN_MAJOR_IO and value.is_cuda and value.dim() == 3 and value.is_contiguous() and not _dist.active()):
        return None
    if value.dtype not in (torch.bfloat16, torch.float16) or value.shape[-1] not in (heads * 64, heads * 128):
        return None
    return value.unflatten(2, (heads, -1)).transpose(1, 2)


def qkv_from_projections(query, key, value, heads: int, norm_q, norm_k, cos, sin, rope_lo: int, rope_hi: int,
                         complex_pairs: bool = False, q_scale: float = 1.0, half_split: bool = False):
    """Projection outputs [bsz, S, heads * D] -> head-major q, k, v [bsz, heads, S, D] with QK-norm + RoPE applied to q, k in
    the same pass (svg_qk_norm_rope_transpose): replaces three transpose copies + norm + norm + rope.  None: not applicable.
    half_split: half-split RoPE (rope_kind 3, tables [rope_hi - rope_lo, D]) instead of interleaved pairs."""
    rope_kind = _rope_kind(complex_pairs, half_split)
    ts = (query, key, value)
    if not all(t.is_cuda for t in ts):
        return None
    _native.load()
    if not all(t.dim() == 3 and t.is_contiguous() and t.dtype in (torch.bfloat16, torch.float16) for t in ts):
        return None
    D = query.shape[-1] // heads
    if D not in _FAST_DIMS or query.shape != key.shape or value.shape != query.shape:
        return None
    kind, qw, qb, kw, kb, eps = 0, None, None, None, None, 0.0
    if norm_q is not None or norm_k is not None:
        dq, dk = _norm_desc(norm_q, D, query.dtype, query.device), _norm_desc(norm_k, D, key.dtype, key.device)
        if dq is None or dk is None or dq[0] != dk[0] or dq[3] != dk[3]:
            return None
        kind, qw, qb, kw, kb, eps = dq[0], dq[1], dq[2], dk[1], dk[2], dq[3]
    rk, tb = 0, (None, None)
    if cos is not None:
        tb = _tables(cos, sin, rope_hi - rope_lo, D // 2 if complex_pairs else D, query.device)
        if tb is None:
            return None
        rk = rope_kind
    q, k = _native.qk_norm_rope_transpose(query, key, heads, heads, kind, qw, qb, kw, kb, eps, rk, tb[0], tb[1], rope_lo, rope_hi,
                                          q_scale=q_scale)   # q_scale != 1: q leaves the prologue carrying the softmax scale
    v = value_in_place(value, heads) if q_scale == 1.0 else None   # (a pre-scaled q takes the entry points without strides)
    if v is None:
        v, _ = _native.qk_norm_rope_transpose(value, None, heads, 0)
    return q, k, v


def _seg_norm(norm_q, norm_k, D: int, dtype, device):
    """(kind, q weight, q bias, k weight, k bias, eps) of one stream's QK norms for the joint prologue: both absent -> kind 0; both
    recognised with the same kind and eps -> theirs; anything else -> None (the fused path does not apply)."""
    if norm_q is None and norm_k is None:
        return 0, None, None, None, None, 1e-6
    dq, dk = _norm_desc(norm_q, D, dtype, device), _norm_desc(norm_k, D, dtype, device)
    if dq is None or dk is None or dq[0] != dk[0] or dq[3] != dk[3]:
        return None
    return dq[0], dq[1], dq[2], dk[1], dk[2], dq[3]


def joint_qkv_from_projections(video_qkv, text_qkv, heads: int, norm_q, norm_k, norm_added_q, norm_added_k, cos, sin, rope_lo: int,
                               rope_hi: int, q_scale: float = 1.0, complex_pairs: bool = False):
    """MMDiT joint prologue: the video stream's projection outputs (q, k, v) [bsz, S_v, heads * D] and the text stream's [bsz, T, heads * D]
    -> head-major q, k, v [bsz, heads, S_v + T, D], rows [video, text], each stream with its own QK norm (text norms may be None: no norm),
    RoPE on joint positions [rope_lo, rope_hi), q_scale folded into q's last rounding — ONE launch (svg_qk_norm_rope_transpose_joint).
    Replaces qkv_from_projections on the video stream + the text stream's transposes / norm_added_q / norm_added_k + three torch.cat
    (ref: hyvideo/attention.py:268-306).  None: not applicable (the conditions of qkv_from_projections) — the caller takes the staged path."""
    ts = tuple(video_qkv) + tuple(text_qkv)
    if len(ts) != 6 or not all(t.is_cuda for t in ts):
        return None
    _native.load()
    if not all(t.dim() == 3 and t.is_contiguous() and t.dtype in (torch.bfloat16, torch.float16) for t in ts):
        return None
    vq, tq = video_qkv[0], text_qkv[0]
    D = vq.shape[-1] // heads
    if D not in _FAST_DIMS or D * heads != vq.shape[-1] or any(t.dtype != vq.dtype for t in ts):
        return None
    if any(t.shape != vq.shape for t in video_qkv) or any(t.shape != tq.shape for t in text_qkv) or tq.shape[0] != vq.shape[0] \
            or tq.shape[2] != vq.shape[2]:
        return None
    nv = _seg_norm(norm_q, norm_k, D, vq.dtype, vq.device)
    nt = _seg_norm(norm_added_q, norm_added_k, D, vq.dtype, vq.device)
    if nv is None or nt is None:
        return None
    rk, tb = 0, (None, None)
    if cos is not None:
        tb = _tables(cos, sin, rope_hi - rope_lo, D // 2 if complex_pairs else D, vq.device)
        if tb is None:
            return None
        rk = 2 if complex_pairs else 1
    segs = [_native.JointSegment(*qkv, kind, qw, qb, kw, kb, eps) for qkv, (kind, qw, qb, kw, kb, eps) in ((video_qkv, nv), (text_qkv, nt))]
    return _native.qk_norm_rope_transpose_joint(segs, heads, rk, tb[0], tb[1], rope_lo, rope_hi, q_scale=q_scale)


def joined_rows(a: torch.Tensor, b: torch.Tensor) -> Optional[torch.Tensor]:
    """`torch.cat([a, b], dim=1)` as a VIEW when b starts exactly where a ends in the same storage with the same strides (two adjacent row
    slices of one [B, S, N] tensor, e.g. the single-stream blocks' `norm_hidden_states[:, :-T]` and `[:, -T:]`); None otherwise."""
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        return None
    if a.dtype != b.dtype or a.device != b.device or a.stride() != b.stride():
        return None
    if a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr():
        return None
    if b.storage_offset() != a.storage_offset() + a.shape[1] * a.stride(1):
        return None
    return a.as_strided((a.shape[0], a.shape[1] + b.shape[1], a.shape[2]), a.stride(), a.storage_offset())
