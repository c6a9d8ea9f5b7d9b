"""Head-sharded execution of one attention layer-call over the GPUs of a node (one process per GPU, RCCL over xGMI).

The hot path has no cross-head dependency at any stage (profiler, layout transformation, k-means, block map, attention
are all per head — SURVEY.md §8e), so a layer-call splits by heads with NO collective inside the path.  The only
exchange is the one the next operator needs: `to_out` consumes all heads of a token, so the per-rank outputs
[1, H/N, S, D] are all-gathered once per layer-call (N-1 peers x H/N x S x D x 2 B each; at Hunyuan 720p and N = 8 that is
7 x 91 MB inbound per GPU, spread over the 7 xGMI links of the full mesh).  The reference has no multi-GPU version of
this path (its deprecated forks use xfuser ring/Ulysses with dense attention); parity is defined as equality with the
single-GPU result, which is bitwise because per-head arithmetic does not change.

Dense attention can also stay TOKEN-sharded (`token_sharded_dense_attention`): every rank keeps all heads of its tokens, sees the
other ranks' keys shard by shard and merges the partial results with their row log-sum-exp — any head count, every rank busy, the
exchange of the next shard behind the compute of this one; equal to the single-GPU result to rounding, not bitwise.
`token_sharded_band_attention` is the same schedule (_attend_over_key_shards, stated there once) for band (SVG1) attention in logical
order: each step is one window of the mask at the global coordinates of the two shards, and pairs of shards the mask rules out exchange
and compute nothing.
`token_sharded_svg1_attention` is that schedule for a real SVG1 layer-call: the sequence sharded by whole frames in the model's own row
order, heads in logical order and token-major heads in one launch per step (svg_band_shard_attention_lse[_f32]).
`token_sharded_sample_mse` is the online profiler of such a sequence — no K / V travels: the sampled q rows are exchanged, each rank streams
its own shard into one partial (svg_sample_mse_shard_partial), the partials are gathered and merged to the same bits on every rank
(svg_sample_mse_from_parts) — and `token_sharded_svg1_layer_call` chains the two: a sharded SVG1 layer-call from q, k, v alone.  Both
carry the processors' device switch between the sparse and the dense warm-up mask (dense_mask / dense_flag:
svg_band_shard_attention_switch_lse[_f32]), and `enable_frame_shards` is the mode in which the SVG1 processors of HunyuanVideo and Wan run
them (svg/models/_core.py).

`enable_token_shards` is the third mode and the one every processor has: activations sharded by rows, `run_token_sharded` exchanges rows for
whole heads in front of the attention core (one all_to_all_single per tensor), runs the single-GPU core on this rank's heads of the whole
sequence and exchanges back — bit for bit the single-GPU result; the layouts either side of the exchanges are one svg_copy_boxes launch
each (_native.copy_box_jobs).
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import _native

# ---------------------------------------------------------------------------------------------------------------
# opt-in switch for the processors (svg/models/_core.py): svg.distributed.enable(group) makes every SVG1 / SVG2 layer-call run
# this rank's heads only and all-gather the result; nothing changes for a process that never calls it.
# ---------------------------------------------------------------------------------------------------------------
_STATE: Dict[str, object] = {"enabled": False, "group": None, "frames": False, "frames_group": None,
                             "tokens": False, "tokens_group": None, "tokens_unit": 128, "tokens_counts": None}


def enable(group=None) -> None:
    """Shard every attention layer-call of the installed processors over the ranks of `group` (default: the world group).
    The processors keep receiving full [cfg, H, S, D] tensors (replicated activations); each rank computes
    `shard_heads(H, rank, world)` and the outputs are all-gathered, so the caller sees the same tensors as on one GPU —
    bitwise, because nothing in the path mixes heads (the k-means stopping rule, a maximum over all heads, is all-reduced)."""
    assert dist.is_available() and dist.is_initialized(), "svg.distributed.enable: call torch.distributed.init_process_group first"
    if _STATE["frames"]:
        raise RuntimeError("svg.distributed.enable: frame-shard mode (enable_frame_shards) is on; disable() it first — one mode at a time")
    if _STATE["tokens"]:
        raise RuntimeError("svg.distributed.enable: token-shard mode (enable_token_shards) is on; disable() it first — one mode at a time")
    _STATE["enabled"], _STATE["group"] = True, group


def enable_token_shards(group=None, unit: int = 128, row_counts: Optional[Sequence[int]] = None) -> None:
    """The third mode: the processors receive q, k, v of ALL heads of this rank's ROWS — `token_range(seq_len, rank, world, unit)` of the
    model's own row order, or with `row_counts` (world ints that sum to the sequence length) the contiguous ranges those counts give, so that
    a caller who shards by `frame_shard` switches modes without re-sharding — and every self-attention layer-call runs through
    run_token_sharded over the ranks of `group`: one all-to-all to whole heads of the whole sequence, the single-GPU core on this rank's
    heads, one all-to-all back.  Nothing needs frames kept together (CogVideoX's text in front of the video is just rows, HunyuanVideo's
    text falls on the last ranks), so it covers what the single-GPU core covers — SVG1 and SVG2, all four model families, bf16 / fp16,
    head_dim 64 / 128, fp8, a pre-scaled q — and the result is the single-GPU one bit for bit.  The rotary tables are the caller's: its own
    rows of them (token_shard_range).  Cross attention stays local.  enable and enable_frame_shards must be off."""
    assert dist.is_available() and dist.is_initialized(), "svg.distributed.enable_token_shards: call torch.distributed.init_process_group first"
    if _STATE["enabled"] or _STATE["frames"]:
        raise RuntimeError(f"svg.distributed.enable_token_shards: {'head sharding (enable)' if _STATE['enabled'] else 'frame-shard mode'} is on; "
                           f"disable() it first — one mode at a time")
    if int(unit) < 1:
        raise ValueError(f"svg.distributed.enable_token_shards: unit must be positive, got {unit}")
    if row_counts is not None:
        row_counts = tuple(int(x) for x in row_counts)
        if len(row_counts) != dist.get_world_size(group) or min(row_counts) < 0:
            raise ValueError(f"svg.distributed.enable_token_shards: row_counts {row_counts} for a group of {dist.get_world_size(group)} ranks")
    _STATE["tokens"], _STATE["tokens_group"], _STATE["tokens_unit"], _STATE["tokens_counts"] = True, group, int(unit), row_counts


def token_shards_active() -> bool:
    """token-shard mode is on (whatever the group's size: a group of one rank holds the whole sequence and runs the same calls)"""
    return bool(_STATE["tokens"]) and dist.is_initialized()


def token_shards_group():
    return _STATE["tokens_group"]


def token_shard_row_counts() -> Optional[Tuple[int, ...]]:
    """the row_counts token-shard mode was enabled with, or None (rows by token_range)"""
    return _STATE["tokens_counts"]


def token_shard_ranges(seq_len: int) -> List[Tuple[int, int]]:
    """[a, b) of every rank's rows of a sequence of seq_len rows in token-shard mode; the same list on every rank"""
    world = dist.get_world_size(_STATE["tokens_group"])
    counts = _STATE["tokens_counts"]
    if counts is None:
        return [token_range(int(seq_len), r, world, int(_STATE["tokens_unit"])) for r in range(world)]
    if sum(counts) != int(seq_len):
        raise ValueError(f"svg.distributed: row_counts {counts} add up to {sum(counts)}, the sequence has {seq_len} rows")
    out, a = [], 0
    for n in counts:
        out.append((a, a + n))
        a += n
    return out


def token_shard_range(seq_len: int, rank: Optional[int] = None) -> Tuple[int, int]:
    """[a, b): the rows of a sequence of seq_len rows that `rank` (default: this rank) holds in token-shard mode — what a caller slices its
    hidden states and its rotary tables with"""
    rank = dist.get_rank(_STATE["tokens_group"]) if rank is None else int(rank)
    return token_shard_ranges(seq_len)[rank]


def head_mode():
    """(on, group) of the mode in which a rank computes whole HEADS — enable() with more than one rank, or token-shard mode: the modes in
    which the k-means stopping rule is reduced, the switch generator's seed is broadcast and the density log is gathered"""
    if active():
        return True, _STATE["group"]
    if token_shards_active():
        return True, _STATE["tokens_group"]
    return False, None


def enable_frame_shards(group=None) -> None:
    """The second, separate mode: the SVG1 processors of HunyuanVideo and Wan receive q, k, v of ALL heads of this rank's whole frames
    (`frame_shard(geometry, rank, world)`; the rows behind the video on the last rank) and run every layer-call through
    token_sharded_svg1_layer_call / token_sharded_svg1_attention over the ranks of `group` — activations stay sharded by rows from one layer
    to the next, K / V shards and the profiler's parts are what travels.  Equal to the single-GPU result to rounding.  The rotary tables
    and the text are the caller's: its own rows of the tables, HunyuanVideo's text on the last rank.  Head sharding (enable) must be off."""
    assert dist.is_available() and dist.is_initialized(), "svg.distributed.enable_frame_shards: call torch.distributed.init_process_group first"
    if _STATE["enabled"]:
        raise RuntimeError("svg.distributed.enable_frame_shards: head sharding (enable) is on; disable() it first — one mode at a time")
    if _STATE["tokens"]:
        raise RuntimeError("svg.distributed.enable_frame_shards: token-shard mode (enable_token_shards) is on; disable() it first — one mode "
                           "at a time")
    _STATE["frames"], _STATE["frames_group"] = True, group


def disable() -> None:
    """all three modes off"""
    _STATE["enabled"], _STATE["group"] = False, None
    _STATE["frames"], _STATE["frames_group"] = False, None
    _STATE["tokens"], _STATE["tokens_group"], _STATE["tokens_unit"], _STATE["tokens_counts"] = False, None, 128, None


def frame_shards_active() -> bool:
    """frame-shard mode is on (whatever the group's size: a group of one rank holds the whole sequence and runs the same calls)"""
    return bool(_STATE["frames"]) and dist.is_initialized()


def frame_shards_group():
    return _STATE["frames_group"]


def active() -> bool:
    return bool(_STATE["enabled"]) and dist.is_initialized() and dist.get_world_size(_STATE["group"]) > 1


def current_group():
    return _STATE["group"]


def all_reduce_max_(t: torch.Tensor) -> torch.Tensor:
    """in-place MAX over the ranks of the enabled group (identity when sharding is off) — the k-means stopping rule's
    `center_shift` is a maximum over ALL heads (ref: svg/kmeans_utils.py:721-723)"""
    on, group = head_mode()   # (token-shard mode: its ranks hold whole heads inside run_token_sharded, as those of enable())
    if on:
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
    return t


def run_sharded(fn: Callable[..., Tuple[torch.Tensor, ...]], head_tensors: Sequence[torch.Tensor], group=None):
    """fn(*[t[:, my heads] for t in head_tensors]) -> tensor or tuple of tensors with the head dimension at dim 1; every result is
    all-gathered back to all heads (global order).  Ragged splits (H % world != 0) are allowed."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    H = head_tensors[0].shape[1]
    mine = shard_heads(H, rank, world)
    if not mine:
        raise ValueError(f"svg.distributed: rank {rank} of {world} owns no head of {H} — head sharding needs num_heads >= world size "
                         f"(use a smaller process group for this model)")
    sl = slice(mine[0], mine[-1] + 1)
    res = fn(*[t[:, sl].contiguous() for t in head_tensors])
    single = not isinstance(res, (tuple, list))
    outs = [_gather_per_head(r, H, group) for r in ([res] if single else res)]
    return outs[0] if single else tuple(outs)


def shard_heads(num_heads: int, rank: int, world: int) -> List[int]:
    """Heads owned by `rank`: a contiguous block, sizes differing by at most one (24 heads / 8 GPUs -> 3 each)."""
    base, rem = divmod(num_heads, world)
    start = rank * base + min(rank, rem)
    return list(range(start, start + base + (1 if rank < rem else 0)))


def head_counts(num_heads: int, world: int) -> List[int]:
    return [len(shard_heads(num_heads, r, world)) for r in range(world)]


def all_gather_heads(o_local: torch.Tensor, num_heads: int, group=None) -> torch.Tensor:
    """[cfg, H_local, S, D] on every rank -> [cfg, H, S, D] on every rank (heads in global order)."""
    world = dist.get_world_size(group)
    counts = head_counts(num_heads, world)
    cfg, _, S, D = o_local.shape
    if len(set(counts)) == 1:
        out = _native.empty((world * cfg, counts[0], S, D), dtype=o_local.dtype, device=o_local.device)
        dist.all_gather_into_tensor(out, o_local.contiguous(), group=group)  # concatenated along dim 0
        return out.view(world, cfg, counts[0], S, D).permute(1, 0, 2, 3, 4).reshape(cfg, num_heads, S, D)
    # ragged split: pad every shard to the largest one
    mx = max(counts)
    pad = torch.zeros((cfg, mx, S, D), dtype=o_local.dtype, device=o_local.device)
    pad[:, : o_local.shape[1]] = o_local
    out = _native.empty((world * cfg, mx, S, D), dtype=o_local.dtype, device=o_local.device)
    dist.all_gather_into_tensor(out, pad, group=group)
    out = out.view(world, cfg, mx, S, D)
    return torch.cat([out[r, :, : counts[r]] for r in range(world)], dim=1)


def _gather_per_head(r: torch.Tensor, num_heads: int, group=None) -> torch.Tensor:
    """[cfg, H_local, ...] on every rank (o, or a per-head extra such as best_mask_idx [cfg, H_local]) -> [cfg, H, ...] on every rank"""
    extra = r.shape[2:]
    r4 = r.reshape(r.shape[0], r.shape[1], -1, 1) if r.dim() != 4 else r
    g = all_gather_heads(r4, num_heads, group)
    return g.reshape(g.shape[0], num_heads, *extra)


# ---------------------------------------------------------------------------------------------------------------
# token-shard mode (enable_token_shards): activations sharded by rows, one all-to-all to head shards in front of the attention core and
# one back behind it — the shape of the reference's context-parallel code (svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169)
# ---------------------------------------------------------------------------------------------------------------
EXCHANGE_STATS: Dict[str, int] = {}   # of the last run_token_sharded on this rank: elements received from OTHER ranks, layout launches


def _all_to_all(recv: torch.Tensor, send: torch.Tensor, out_splits: List[int], in_splits: List[int], group) -> int:
    """one all_to_all_single of flat buffers; on a backend that cannot exchange device tensors (gloo) staged through host memory.
    -> elements received from other ranks"""
    if send.is_cuda and dist.get_backend(group) == "gloo":
        host = _native.empty(recv.numel(), dtype=recv.dtype, device="cpu")
        dist.all_to_all_single(host, send.cpu(), output_split_sizes=out_splits, input_split_sizes=in_splits, group=group)
        recv.copy_(host)
    else:
        dist.all_to_all_single(recv, send, output_split_sizes=out_splits, input_split_sizes=in_splits, group=group)
    return sum(out_splits) - out_splits[dist.get_rank(group)]


def _boxable(t: torch.Tensor) -> bool:
    """can the copy kernel address this [cfg, H, S, D] view in place?  (unit stride on D, every other stride and the base 16-byte aligned)"""
    return t.stride(3) == 1 and all(s % 8 == 0 for s in t.stride()[:3]) and t.data_ptr() % 16 == 0


def run_token_sharded(fn: Callable[..., Tuple[torch.Tensor, ...]], head_tensors: Sequence[torch.Tensor], seq_len: int, group=None,
                      ranges: Optional[Sequence[Tuple[int, int]]] = None):
    """The counterpart of run_sharded for activations that live sharded by ROWS.  head_tensors (q, k, v) are [cfg, H, S_r, D] — all heads
    of this rank's rows `ranges[rank]` (default: token_shard_ranges(seq_len), the rows of token-shard mode), unit stride on D only: v may be
    the head view of to_v's output.
    Inbound: each becomes [cfg, H_l, S, D] with the heads shard_heads(H, rank, world) — ONE all_to_all_single per tensor (send block for
    destination j [cfg, H_j, S_r, D], receive block from source i [cfg, H_l, S_i, D]).  Core: fn(q_h, k_h, v_h) on the head shard -> o
    [cfg, H_l, S, D], or a tuple whose further members are per-head tensors (best_mask_idx [cfg, H_l]) that are all-gathered as by
    run_sharded.  Outbound: o becomes [cfg, H, S_r, D]: send block for destination j [cfg, S_j, H_l, D] — when fn returns o stored
    token-major ([cfg, S, H_l, D]: token_major_out of the _native wrappers) and cfg == 1, every send block is a contiguous row slice and
    nothing is packed — the received [cfg, S_r, H_i, D] blocks are interleaved into [cfg, S_r, H, D] and the result is the
    [cfg, H, S_r, D] VIEW of that storage, so a processor's `.transpose(1, 2).flatten(2, 3)` stays a view.
    The layouts either side of the exchanges are _native.copy_box_jobs: one svg_copy_boxes launch per step on the GPU (inbound unpack of
    q, k, v: one; inbound pack, only for a send buffer that is not contiguous already — cfg > 1, v as a head view: one; outbound unpack:
    one; outbound pack, only without token-major storage or with cfg > 1: one), the torch statement of the same boxes on CPU tensors.
    Ragged head counts and ragged row counts are allowed.  A world in which some rank owns no head raises ValueError on every rank before
    any collective; every rank enters every collective.
    gloo cannot all_to_all device tensors: there (the tests: ranks that share one GPU) each exchange is staged through host memory, as
    bench_step.py's host_staged does.  RCCL exchanges the device buffers directly.  No exchange was ever timed: no multi-GPU run exists."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    ts = list(head_tensors)
    cfg, H, S_r, D = ts[0].shape
    counts = head_counts(H, world)
    if min(counts) == 0:
        raise ValueError(f"svg.distributed: {world} ranks but {H} heads — some rank owns no head; token-shard mode needs num_heads >= world "
                         f"size (use a smaller process group for this model)")
    if ranges is None:
        ranges = token_shard_ranges(seq_len) if _STATE["tokens"] else [token_range(int(seq_len), r, world, 128) for r in range(world)]
    ranges = [(int(a), int(b)) for a, b in ranges]
    S = int(seq_len)
    if len(ranges) != world or ranges[0][0] != 0 or ranges[-1][1] != S or any(ranges[i][1] != ranges[i + 1][0] for i in range(world - 1)):
        raise ValueError(f"svg.distributed.run_token_sharded: row ranges {ranges} do not tile the {S} rows over {world} ranks")
    if any(tuple(t.shape) != (cfg, H, ranges[rank][1] - ranges[rank][0], D) for t in ts):
        raise ValueError(f"svg.distributed.run_token_sharded: rank {rank} holds rows {ranges[rank]} of {H} heads, got "
                         f"{[tuple(t.shape) for t in ts]}")
    H_l = counts[rank]
    n_rows = [b - a for a, b in ranges]
    dev, stats = ts[0].device, {"received_elements": 0, "launches": 0}
    kernel_ok = ts[0].is_cuda and D in (64, 128) and ts[0].dtype in (torch.bfloat16, torch.float16)
    how = lambda layout: layout if kernel_ok else "torch"   # noqa: E731  (what the kernel does not take: the torch copies)

    # ---- inbound: [cfg, H, S_r, D] -> [cfg, H_l, S, D]
    sends, jobs = [], []
    for t in ts:
        if not _boxable(t):
            t = t.contiguous()
        if cfg == 1 and t.is_contiguous():
            sends.append(t.reshape(-1))   # (a view: the blocks [H_j, S_r, D] lie behind one another already)
            continue
        send = _native.empty(cfg * H * S_r * D, dtype=t.dtype, device=dev)
        jobs.append((t, send, _native.inbound_pack_boxes(cfg, counts, S_r, D, t.stride()[:3])))
        sends.append(send)
    stats["launches"] += _native.copy_box_jobs(jobs, D, how("inbound_pack"))
    recvs = []
    for send in sends:
        recv = _native.empty(cfg * H_l * S * D, dtype=send.dtype, device=dev)
        stats["received_elements"] += _all_to_all(recv, send, [cfg * H_l * n * D for n in n_rows], [cfg * c * S_r * D for c in counts], group)
        recvs.append(recv)
    if world == 1:
        heads = [r.view(cfg, H_l, S, D) for r in recvs]
    else:
        heads = [_native.empty((cfg, H_l, S, D), dtype=r.dtype, device=dev) for r in recvs]
        boxes = _native.inbound_unpack_boxes(cfg, H_l, ranges, D)
        stats["launches"] += _native.copy_box_jobs([(r, x, boxes) for r, x in zip(recvs, heads)], D, how("inbound_unpack"))

    # ---- the core, on whole heads of the whole sequence
    res = fn(*heads)
    single = not isinstance(res, (tuple, list))
    res = [res] if single else list(res)
    o = res[0]
    if tuple(o.shape) != (cfg, H_l, S, D):
        raise ValueError(f"svg.distributed.run_token_sharded: fn returned {tuple(o.shape)}, expected {(cfg, H_l, S, D)}")

    # ---- outbound: [cfg, H_l, S, D] -> [cfg, H, S_r, D], stored [cfg, S_r, H, D]
    if not _boxable(o):
        o = o.contiguous()
    if cfg == 1 and o.permute(0, 2, 1, 3).is_contiguous():
        send = o.permute(0, 2, 1, 3).reshape(-1)   # (token-major storage: the blocks [S_j, H_l, D] are row slices of it)
    else:
        send = _native.empty(cfg * H_l * S * D, dtype=o.dtype, device=dev)
        stats["launches"] += _native.copy_box_jobs([(o, send, _native.outbound_pack_boxes(cfg, H_l, ranges, D, o.stride()[:3]))], D,
                                                   how("outbound_pack"))
    recv = _native.empty(cfg * S_r * H * D, dtype=o.dtype, device=dev)
    stats["received_elements"] += _all_to_all(recv, send, [cfg * S_r * c * D for c in counts], [cfg * n * H_l * D for n in n_rows], group)
    if world == 1:
        store = recv.view(cfg, S_r, H, D)
    else:
        store = _native.empty((cfg, S_r, H, D), dtype=o.dtype, device=dev)
        stats["launches"] += _native.copy_box_jobs([(recv, store, _native.outbound_unpack_boxes(cfg, counts, S_r, D))], D,
                                                   how("outbound_unpack"))
    outs = [store.permute(0, 2, 1, 3)] + [_gather_per_head(r, H, group) for r in res[1:]]   # per-head extras: as run_sharded gathers them
    EXCHANGE_STATS.clear()
    EXCHANGE_STATS.update(stats)
    return outs[0] if single else tuple(outs)


def sharded_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_fn: Callable[..., torch.Tensor],
                      per_head_args: Sequence[torch.Tensor] = (), group=None) -> torch.Tensor:
    """Run `attn_fn(q_h, k_h, v_h, *args_h)` on this rank's heads of full [cfg, H, S, D] tensors and all-gather.
    per_head_args are tensors with a head dimension at dim 1 (e.g. best_mask_idx [cfg, H]) sliced the same way."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    H = q.shape[1]
    mine = shard_heads(H, rank, world)
    sl = slice(mine[0], mine[-1] + 1) if mine else slice(0, 0)
    o_local = attn_fn(q[:, sl].contiguous(), k[:, sl].contiguous(), v[:, sl].contiguous(), *[a[:, sl] for a in per_head_args])
    return all_gather_heads(o_local, H, group)


# ---------------------------------------------------------------------------------------------------------------
# token shards <-> head shards (the two exchanges either side of the attention when activations live token-sharded)
# ---------------------------------------------------------------------------------------------------------------
def token_range(num_tokens: int, rank: int, world: int, unit: int = 1) -> Tuple[int, int]:
    """Tokens [a, b) of the sequence that live on `rank` between attention calls: contiguous, in whole `unit`s, a trailing partial
    unit goes to the last rank.  Nothing on the token-sharded side (norms, GEMMs, prologue with absolute RoPE positions, glue) needs
    frames kept together, so the unit is a tile of tokens, not a frame: HunyuanVideo 720p, S = 119056 over 8 ranks with unit = 128 gives
    14976 / 14848 (+16) tokens, largest / mean 1.006; unit = tokens per frame (33 frames -> 5, 4, 4, ...) gives 1.21 and costs the
    GEMM / glue side of an 8-GPU step about 8 %."""
    n_units = num_tokens // unit
    base, rem = divmod(n_units, world)
    a = (rank * base + min(rank, rem)) * unit
    b = a + (base + (1 if rank < rem else 0)) * unit
    if rank == world - 1:
        b = num_tokens
    return a, b


def _owner_lists(num_heads: int, world: int, head_lists) -> List[List[int]]:
    return [list(h) for h in head_lists] if head_lists is not None else [shard_heads(num_heads, r, world) for r in range(world)]


def tokens_to_heads(x_local: torch.Tensor, num_tokens: int, group=None, unit: int = 1, head_lists=None, presorted: bool = False,
                    out: Optional[torch.Tensor] = None, recv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inbound exchange of a layer-call.  x_local [H, S_r, ...]: ALL heads of this rank's tokens `token_range(num_tokens, rank,
    world, unit)` (head-major, as the fused prologue writes it) -> [H_local, num_tokens, ...]: this rank's heads of ALL tokens.
    One all_to_all_single (every peer sends to every peer directly: the 7 xGMI links of a rank run concurrently), then one
    strided copy per source rank into the sequence dimension.  Received per rank: (world - 1) / world of H_local * S * E bytes.
    head_lists: per-rank head ids when ownership is not `shard_heads` (bench.py: chunked_head_layout); presorted=True says
    x_local's heads are already ordered owner by owner."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    H = x_local.shape[0]
    rest = tuple(x_local.shape[2:])
    E = math.prod(rest)
    owners = _owner_lists(H, world, head_lists)
    tr = [token_range(num_tokens, r, world, unit) for r in range(world)]
    S_me = tr[rank][1] - tr[rank][0]
    assert x_local.shape[1] == S_me, f"rank {rank} holds {x_local.shape[1]} tokens, token_range says {S_me}"
    Hl = len(owners[rank])
    order = [h for o in owners for h in o]
    if not presorted and order != list(range(H)):
        x_local = x_local.index_select(0, torch.tensor(order, device=x_local.device))
    send = x_local.contiguous().view(-1)   # (no copy for the head-major tensor the fused prologue writes)
    # recv: optional caller-owned staging buffer (a step that runs this exchange 180 times allocates nothing: ExchangeBuffers)
    if recv is None:
        recv = _native.empty(Hl * num_tokens * E, dtype=x_local.dtype, device=x_local.device)
    else:
        assert recv.dtype == x_local.dtype and recv.numel() >= Hl * num_tokens * E
        recv = recv.view(-1)[: Hl * num_tokens * E]
    dist.all_to_all_single(recv, send, output_split_sizes=[Hl * (b - a) * E for a, b in tr],
                           input_split_sizes=[len(o) * S_me * E for o in owners], group=group)
    if out is None:
        out = _native.empty((Hl, num_tokens) + rest, dtype=x_local.dtype, device=x_local.device)
    off = 0
    for a, b in tr:
        n = Hl * (b - a) * E
        out[:, a:b].copy_(recv[off:off + n].view((Hl, b - a) + rest))
        off += n
    return out


def heads_to_tokens(o_local: torch.Tensor, num_heads: int, group=None, unit: int = 1, head_lists=None,
                    send: Optional[torch.Tensor] = None, recv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Outbound exchange, the inverse of tokens_to_heads: o_local [H_local, S, ...] (this rank's heads, all tokens) ->
    [H, S_r, ...] (all heads of this rank's tokens; heads in global order) — what a token-sharded `to_out` consumes, world
    times fewer received bytes than all-gathering the heads."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    S = o_local.shape[1]
    rest = tuple(o_local.shape[2:])
    E = math.prod(rest)
    owners = _owner_lists(num_heads, world, head_lists)
    tr = [token_range(S, r, world, unit) for r in range(world)]
    Hl = len(owners[rank])
    assert o_local.shape[0] == Hl
    S_me = tr[rank][1] - tr[rank][0]
    if send is None:
        send = torch.cat([o_local[:, a:b].reshape(-1) for a, b in tr])
    else:   # caller-owned staging (see ExchangeBuffers): one strided copy per destination rank, no allocation
        assert send.dtype == o_local.dtype and send.numel() >= Hl * S * E
        send = send.view(-1)[: Hl * S * E]
        off = 0
        for a, b in tr:
            n = Hl * (b - a) * E
            send[off:off + n].view((Hl, b - a) + rest).copy_(o_local[:, a:b])
            off += n
    if recv is None:
        recv = _native.empty(num_heads * S_me * E, dtype=o_local.dtype, device=o_local.device)
    else:
        assert recv.dtype == o_local.dtype and recv.numel() >= num_heads * S_me * E
        recv = recv.view(-1)[: num_heads * S_me * E]
    dist.all_to_all_single(recv, send, output_split_sizes=[len(o) * S_me * E for o in owners],
                           input_split_sizes=[Hl * (b - a) * E for a, b in tr], group=group)
    out = recv.view((num_heads, S_me) + rest)
    order = [h for o in owners for h in o]
    if order != list(range(num_heads)):
        inv = _native.empty(num_heads, dtype=torch.long)
        inv[torch.tensor(order)] = torch.arange(num_heads)
        out = out.index_select(0, inv.to(out.device))
    return out


# ---------------------------------------------------------------------------------------------------------------
# token-sharded DENSE attention: no exchange of q or o at all — every rank keeps all heads of its own tokens and sees the other ranks'
# keys shard by shard, merging the partial results with their row log-sum-exp (svg_cross_attention_lse + svg_merge_attention_states).
# ref: the context-parallel dense attention of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169 (xfuser ring / Ulysses),
#      flashinfer's run(..., return_lse=True) + merge_state in svg/kernels/ops/attention_ops.py:178-188
# ---------------------------------------------------------------------------------------------------------------
MERGE_MAX_PARTS = _native.MERGE_MAX_PARTS   # svg_merge_attention_states (include/svg_attn.h): parts of one N-way merge


def _native_attn(q, k, v, return_lse=False):
    return _native.cross_attention(q, k, v, return_lse=return_lse)


def _native_merge(o_parts, lse_parts):
    return _native.merge_attention_states(o_parts, lse_parts)


def _native_attn_f32(q, k, v, return_lse=False):
    """the step of fp32_parts=True: the part before its rounding; the calls without lse (world == 1, overlap=False) are the plain ones"""
    if not return_lse:
        return _native.cross_attention(q, k, v)
    return _native.cross_attention(q, k, v, return_lse=True, out_dtype=torch.float32)


def _attend_over_key_shards(q_local: torch.Tensor, k_local: torch.Tensor, v_local: torch.Tensor, n_rows: Sequence[int],
                            plan: Sequence[Sequence[bool]], step: Callable, merge_fn: Callable, group, who: str,
                            post_before_own_part: bool) -> torch.Tensor:
    """The key-shard exchange schedule of token_sharded_dense_attention(overlap=True), token_sharded_band_attention and
    token_sharded_svg1_attention: this rank's rows q_local attend over the K / V shard of every rank whose keys they need, one part per
    shard, and the parts are merged with their row log-sum-exp.
    n_rows[r]: the rows rank r holds (k_local, v_local [..., H, n_rows[rank], D]).  plan[r][s]: do rank r's rows need rank s's shard —
    the same table on every rank.  step(src_rank, k_s, v_s) -> (o, lse): this rank's rows over the shard of src_rank.
    k and v of a shard travel as ONE message.  At step j every rank sends its OWN shard directly to rank + j and receives the shard of
    rank - j from its owner (all_to_all_single with one non-empty split each way: a shift by j; no forwarding around a ring, every link
    carries a shard once).  A pair the plan rules out sends nothing and receives nothing — every rank still enters the collective of the
    step, with zero-size splits — and a step in which no rank receives keys is skipped by all ranks.  While a step's part is computed the
    exchange of the next step is in flight.  A part is computed only where the plan keeps the pair and both shards have rows.
    post_before_own_part: the first exchange is posted before the part over the rank's own shard is computed (dense) or after it (band,
    SVG1); the own part is the first one computed either way.
    At the end ONE merge_fn(o_parts, lse_parts) over the parts ordered by SOURCE rank, so the arithmetic of a row does not depend on the
    rank that computed it.  More than MERGE_MAX_PARTS parts on some rank: ValueError on every rank, in the name of `who`, before the first
    collective and before any step.  A rank without rows returns an empty tensor, rows that see no key at all zeros."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    most = max(sum(row) for row in plan)
    if most > MERGE_MAX_PARTS:
        raise ValueError(f"{who}: a rank sees the keys of {most} shards, but merge_attention_states takes at most "
                         f"{MERGE_MAX_PARTS} parts — use a group of at most {MERGE_MAX_PARTS} ranks")
    lead, D = tuple(k_local.shape[:-2]), k_local.shape[-1]
    per_tok = 2 * D * math.prod(lead)
    # the steps in which some rank receives keys, the same list on every rank
    steps = [j for j in range(1, world) if any(plan[r][(r - j) % world] for r in range(world))]
    send = torch.stack([k_local, v_local]).contiguous().view(-1) if steps else None

    def shift(j):
        """this rank's shard to rank + j if that rank needs it, the shard of rank - j if this rank needs it: (source rank, buffer, work)"""
        dst, src = (rank + j) % world, (rank - j) % world
        recv = _native.empty(n_rows[src] * per_tok if plan[rank][src] else 0, dtype=send.dtype, device=send.device)
        ins, outs = [0] * world, [0] * world
        ins[dst] = send.numel() if plan[dst][rank] else 0
        outs[src] = recv.numel()
        work = dist.all_to_all_single(recv, send[:ins[dst]], output_split_sizes=outs, input_split_sizes=ins, group=group, async_op=True)
        return src, recv, work

    def has_part(src):
        return plan[rank][src] and n_rows[rank] > 0 and n_rows[src] > 0   # (an empty shard has no keys: no part)

    parts = {}
    nxt = shift(steps[0]) if steps and post_before_own_part else None
    if has_part(rank):
        parts[rank] = step(rank, k_local, v_local)
    if steps and not post_before_own_part:
        nxt = shift(steps[0])
    for i in range(len(steps)):
        src, recv, work = nxt
        work.wait()
        nxt = shift(steps[i + 1]) if i + 1 < len(steps) else None     # in flight while this step computes
        if has_part(src):
            k_s, v_s = recv.view((2,) + lead + (n_rows[src], D)).unbind(0)
            parts[src] = step(src, k_s, v_s)
    if n_rows[rank] == 0:
        return _native.empty_like(q_local)
    if not parts:   # (a plan that gives these rows no key at all)
        return torch.zeros_like(q_local)
    order = sorted(parts)
    return merge_fn([parts[r][0] for r in order], [parts[r][1] for r in order])


def _check_device_switch_pair(who: str, dense_mask, dense_flag) -> None:
    if (dense_mask is None) != (dense_flag is None):
        raise ValueError(f"{who}: dense_mask and dense_flag go together (the device switch), or neither")


def token_sharded_dense_attention(q_local: torch.Tensor, k_local: torch.Tensor, v_local: torch.Tensor, num_tokens: int, group=None,
                                  unit: int = 1, overlap: bool = True, attn_fn: Optional[Callable] = None,
                                  merge_fn: Optional[Callable] = None, fp32_parts: bool = False) -> torch.Tensor:
    """Dense attention over a sequence that lives token-sharded: q_local, k_local, v_local [..., H, S_r, D] are ALL heads of this rank's
    tokens `token_range(num_tokens, rank, world, unit)` (ragged shards allowed); returns the attention output of this rank's rows over
    ALL num_tokens keys, [..., H, S_r, D].  Nothing is sharded by heads, so it works for any head count (12 heads on 8 GPUs) and leaves
    no rank idle.
    overlap=False (the baseline): k and v are all-gathered, then ONE attn_fn(q, k, v) launch.
    overlap=True: the schedule of _attend_over_key_shards under a plan that is true for every pair — world steps; at step j the rank
    computes (o_j, lse_j) = attn_fn(q, k_s, v_s, True) of its rows over the shard of rank s = (rank - j) mod world, and the first exchange
    is posted before the own part.  world > MERGE_MAX_PARTS: ValueError (the N-way merge takes at most 8 parts).
    attn_fn(q, k, v, return_lse=False) -> o or (o, lse) and merge_fn(o_parts, lse_parts) -> o default to the native calls
    (_native.cross_attention, _native.merge_attention_states); they exist so that the schedule can be tested without a GPU.
    fp32_parts (the native default functions with overlap=True; nothing else changes): the steps return their rows BEFORE the rounding
    (_native.cross_attention(..., out_dtype=torch.float32)) and the merge takes them as they are
    (_native.merge_attention_states(..., out_dtype=q's dtype)); the output has q's dtype.  Twice the bytes of every part.  A caller's own
    attn_fn / merge_fn are called as without it — they decide what a part is.
    Unlike head sharding, the result equals the single-GPU one TO ROUNDING, not bit for bit.  overlap=True, fp32_parts=False: the output
    is rounded twice, once per part and once in the merge — rel. L2 against the exact result 2.84e-3 on bf16 where one call has 2.35e-3
    and one rounding 1.66e-3 (the two roundings add in quadrature).  overlap=True, fp32_parts=True: the merge's rounding is
    the only one, and the result meets the tolerance of one call.  overlap=False runs the single-GPU arithmetic on this rank's rows."""
    if fp32_parts:
        from functools import partial

        attn_fn = attn_fn or _native_attn_f32
        if merge_fn is None:
            merge_fn = partial(_native.merge_attention_states, out_dtype=q_local.dtype)
    attn_fn = attn_fn or _native_attn
    merge_fn = merge_fn or _native_merge
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    tr = [token_range(num_tokens, r, world, unit) for r in range(world)]
    n_tok = [b - a for a, b in tr]
    S_me = n_tok[rank]
    assert q_local.shape[-2] == S_me and k_local.shape == v_local.shape and k_local.shape[-2] == S_me, (
        f"rank {rank} holds {q_local.shape[-2]} / {k_local.shape[-2]} tokens, token_range says {S_me}")
    if overlap and world > MERGE_MAX_PARTS:
        raise ValueError(f"token_sharded_dense_attention(overlap=True): {world} ranks, but merge_attention_states takes at most "
                         f"{MERGE_MAX_PARTS} parts — use a group of at most {MERGE_MAX_PARTS} ranks or overlap=False")
    if world == 1:
        return attn_fn(q_local, k_local, v_local)
    if not overlap:
        kv = (2,) + tuple(k_local.shape[:-2]) + (max(n_tok), k_local.shape[-1])   # k and v of a shard, padded to the largest, as one message
        pad = torch.zeros(kv, dtype=k_local.dtype, device=k_local.device)
        pad[0][..., :S_me, :] = k_local
        pad[1][..., :S_me, :] = v_local
        full = _native.empty((world * 2,) + kv[1:], dtype=k_local.dtype, device=k_local.device)   # concatenated along dim 0
        dist.all_gather_into_tensor(full, pad, group=group, async_op=True).wait()
        full = full.view((world,) + kv)
        if S_me == 0:
            return _native.empty_like(q_local)
        k_all = torch.cat([full[r, 0][..., :n_tok[r], :] for r in range(world)], dim=-2)
        v_all = torch.cat([full[r, 1][..., :n_tok[r], :] for r in range(world)], dim=-2)
        return attn_fn(q_local, k_all, v_all)
    # every pair exchanges, a pair with an empty shard included: a rank without rows still receives the shards it does not use
    return _attend_over_key_shards(q_local, k_local, v_local, n_tok, [[True] * world] * world,
                                   lambda src, k_s, v_s: attn_fn(q_local, k_s, v_s, True), merge_fn, group,
                                   "token_sharded_dense_attention(overlap=True)", post_before_own_part=True)


# ---------------------------------------------------------------------------------------------------------------
# token-sharded BAND (SVG1) attention: the schedule above with the band mask evaluated at the global coordinates of the two shards
# (svg_band_window_attention_lse[_f32]) — and only the shards a rank's rows can see travel at all.
# ---------------------------------------------------------------------------------------------------------------
def band_exchange_plan(mask, num_tokens: int, world: int, unit: int = 128) -> List[List[bool]]:
    """plan[r][s]: do the rows of rank r (`token_range(num_tokens, r, world, unit)`) see any key of rank s's shard under the band mask
    `mask` (_native.BandMask) over num_tokens rows?  Host only, closed form (_native.band_window_has_keys); the same table on every rank.
    A pair that is False exchanges nothing and computes nothing in token_sharded_band_attention."""
    tr = [token_range(num_tokens, r, world, unit) for r in range(world)]
    return [[_native.band_window_has_keys(mask, num_tokens, tr[r], tr[s]) for s in range(world)] for r in range(world)]


def token_sharded_band_attention(q_local: torch.Tensor, k_local: torch.Tensor, v_local: torch.Tensor, num_tokens: int, mask, group=None,
                                 unit: int = 128, fp32_parts: bool = True, attn_fn: Optional[Callable] = None,
                                 merge_fn: Optional[Callable] = None) -> torch.Tensor:
    """Band (SVG1) attention over a sequence that lives token-sharded, in the LOGICAL order of the mask: q_local, k_local, v_local
    [..., H, S_r, D] are ALL heads of this rank's tokens `token_range(num_tokens, rank, world, unit)` (ragged shards allowed); returns this
    rank's rows of band attention under `mask` (_native.BandMask over num_tokens rows), [..., H, S_r, D].  Any head count, no rank idle.
    The schedule of _attend_over_key_shards under band_exchange_plan: a step is attn_fn(q, k_s, v_s, (q0, q1), (k0, k1)) -> (o, lse)
    with the token ranges of this rank and of the shard's owner, and the own part is computed before the first exchange is posted.  What
    the mask rules out does not happen: a pair (rank, s) whose window holds no allowed element exchanges and computes nothing.
    attn_fn and merge_fn default to the native calls (_native.band_window_attention, _native.merge_attention_states; fp32_parts: the
    parts travel to the merge before their rounding, so the result is rounded once); they exist so that the schedule can be tested
    on gloo without a GPU.  unit must be a multiple of 64 (ValueError): the key windows start on the mask's key tiles.  More ranks than
    MERGE_MAX_PARTS are refused only when some rank really has more than MERGE_MAX_PARTS non-empty parts (ValueError on every rank).
    What this does NOT do: there is no head permutation — token-major heads (the frame-major placement of the temporal heads) need their
    placement first, since a window of such a head is not a window of physical rows — and nothing is wired into the processors or
    bench_step.py.  Equal to the single-GPU result to rounding, not bit for bit."""
    if unit <= 0 or unit % 64 != 0:
        raise ValueError(f"token_sharded_band_attention: unit must be a positive multiple of 64 (key windows start on key tiles), got {unit}")
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    tr = [token_range(num_tokens, r, world, unit) for r in range(world)]
    n_tok = [b - a for a, b in tr]
    S_me = n_tok[rank]
    assert q_local.shape[-2] == S_me and k_local.shape == v_local.shape and k_local.shape[-2] == S_me, (
        f"rank {rank} holds {q_local.shape[-2]} / {k_local.shape[-2]} tokens, token_range says {S_me}")
    if attn_fn is None:
        def attn_fn(q, k, v, q_range, k_range):
            return _native.band_window_attention(q, k, v, mask, num_tokens, q_range[0], k_range[0],
                                                 out_dtype=torch.float32 if fp32_parts else None)
    if merge_fn is None:
        def merge_fn(o_parts, lse_parts):
            return _native.merge_attention_states(o_parts, lse_parts, out_dtype=q_local.dtype if fp32_parts else None)
    return _attend_over_key_shards(q_local, k_local, v_local, n_tok, band_exchange_plan(mask, num_tokens, world, unit),
                                   lambda src, k_s, v_s: attn_fn(q_local, k_s, v_s, tr[rank], tr[src]), merge_fn, group,
                                   "token_sharded_band_attention", post_before_own_part=False)


# ---------------------------------------------------------------------------------------------------------------
# frame-sharded SVG1 attention: the same schedule for a sequence that lives sharded by whole FRAMES in the model's own (frame-major) row
# order, heads in logical order and token-major heads in one launch per step (svg_band_shard_attention_lse[_f32]).
# ---------------------------------------------------------------------------------------------------------------
def frame_range(num_frame: int, rank: int, world: int) -> Tuple[int, int]:
    """[f0, f1) of the frames rank `rank` of `world` holds: whole frames, the first num_frame % world ranks one more (33 frames over 8
    ranks: 5, 4, 4, ...).  Whole frames cost balance — the largest shard over the mean is 1.21 there; a rank may hold none."""
    base, rem = divmod(int(num_frame), int(world))
    f0 = rank * base + min(rank, rem)
    return f0, f0 + base + (1 if rank < rem else 0)


def frame_shard(geometry, rank: int, world: int):
    """The shard (_native.BandShard) of rank `rank`: its frames of frame_range and, on the LAST rank, the tail — every row behind the video
    (HunyuanVideo's text and the padding behind it).  geometry = (num_tokens, vid0, num_frame, frame_size).  A sequence with rows in FRONT
    of the video (vid0 > 0: CogVideoX's text) has no frame-sharded form yet — a shard carries rows behind the video only — ValueError."""
    S, vid0, F, P = (int(x) for x in geometry)
    if vid0 != 0:
        raise ValueError(f"frame_shard: {vid0} rows in front of the video belong to no shard (a shard's tail lies behind the video)")
    f0, f1 = frame_range(F, rank, world)
    tail0 = vid0 + F * P
    n_tail = S - tail0 if rank == world - 1 else 0
    return _native.BandShard(f0, f1 - f0, tail0, n_tail)


def _frame_shards(geometry, world: int):
    """(frame_shard of every rank, the rows each of them holds)"""
    shards = [frame_shard(geometry, r, world) for r in range(world)]
    return shards, [_native.band_shard_rows(s, int(geometry[3])) for s in shards]


_SHARD_KINDS = {"both": (False, True), "logical": (False,), "token_major": (True,)}


def band_shard_exchange_plan(mask, geometry, world: int, kinds: str = "both", dense_mask=None) -> List[List[bool]]:
    """plan[r][s]: do the rows of rank r's shard (frame_shard) see any key of rank s's shard under `mask` — for ANY kind of head that
    occurs: kinds = "logical", "token_major", or "both" where the flags live on the device (no flag is read back)?  Host only, closed form
    (_native.band_shard_has_keys); the same table on every rank.  A rank without rows neither sends nor receives.
    dense_mask: the alternate mask of a device switch, whose flag is not read back either — the element-wise OR with the plan of
    `dense_mask` for heads in logical order: a pair that either setting of the flag needs is kept."""
    S, vid0, F, P = (int(x) for x in geometry)
    sh, rows = _frame_shards(geometry, world)
    plan = [[rows[r] > 0 and rows[s] > 0 and any(_native.band_shard_has_keys(mask, S, (vid0, F, P), sh[r], sh[s], kind)
                                                 for kind in _SHARD_KINDS[kinds]) for s in range(world)] for r in range(world)]
    if dense_mask is not None:
        alt = band_shard_exchange_plan(dense_mask, geometry, world, "logical")
        plan = [[a or b for a, b in zip(ra, rb)] for ra, rb in zip(plan, alt)]
    return plan


def token_sharded_svg1_attention(q_local: torch.Tensor, k_local: torch.Tensor, v_local: torch.Tensor, mask, best_mask_idx, geometry,
                                 group=None, fp32_parts: bool = True, kinds: str = "both", attn_fn: Optional[Callable] = None,
                                 merge_fn: Optional[Callable] = None, dense_mask=None, dense_flag=None) -> torch.Tensor:
    """One SVG1 layer-call over a sequence that lives sharded by whole frames: q_local, k_local, v_local [..., H, S_r, D] are ALL heads of
    this rank's rows `frame_shard(geometry, rank, world)` — its frames as the model stores them, on the last rank the text and padding
    behind them; best_mask_idx (int [BH] on the device, != 0: a token-major head) is what the device switch produced and is never read
    back; geometry = (num_tokens, vid0, num_frame, frame_size).  Returns this rank's rows of band attention under `mask`
    (_native.BandMask over num_tokens rows, in each head's logical order) with the head placement and its inverse applied, in the rank's
    own row order, [..., H, S_r, D].
    The schedule of _attend_over_key_shards under band_shard_exchange_plan: a step is attn_fn(q, k_s, v_s, q_shard, k_shard) -> (o, lse)
    with the shards of this rank and of the keys' owner, both kinds of head in one launch, and the own part is computed before the first
    exchange is posted.  A pair (rank, s) that the plan rules out for every kind of head in `kinds` exchanges and computes nothing.  attn_fn and
    merge_fn default to the native calls (_native.band_shard_attention, _native.merge_attention_states; fp32_parts: one rounding); they
    exist so that the schedule can be tested on gloo without a GPU.
    dense_mask, dense_flag (both or neither, ValueError otherwise): the processors' device switch — dense_flag (int32 [1] on the device)
    != 0 runs `dense_mask` (over num_tokens rows) with every head in logical order instead, decided by the kernel
    (_native.band_shard_attention_switch); the flag is never read back, so the exchange keeps a pair that EITHER setting needs: the plan
    is the element-wise OR of the plan of `mask` under `kinds` and the plan of `dense_mask` with heads in logical order
    (band_shard_exchange_plan(..., dense_mask=dense_mask)), and the limit of MERGE_MAX_PARTS is checked on that.  An injected attn_fn
    keeps its five arguments and looks after the flag itself.
    What svg.models._core runs in frame-shard mode (enable_frame_shards); not wired into bench_step.py.  Equal to the single-GPU result
    to rounding, not bit for bit."""
    _check_device_switch_pair("token_sharded_svg1_attention", dense_mask, dense_flag)
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    S, vid0, F, P = (int(x) for x in geometry)
    sh, n_tok = _frame_shards(geometry, world)
    S_me = n_tok[rank]
    assert q_local.shape[-2] == S_me and k_local.shape == v_local.shape and k_local.shape[-2] == S_me, (
        f"rank {rank} holds {q_local.shape[-2]} / {k_local.shape[-2]} rows, frame_shard says {S_me}")
    if attn_fn is None:
        def attn_fn(q, k, v, q_shard, k_shard):
            if dense_mask is not None:
                return _native.band_shard_attention_switch(q, k, v, mask, dense_mask, dense_flag, S, (vid0, F, P), q_shard, k_shard,
                                                           out_dtype=torch.float32 if fp32_parts else None, flags=best_mask_idx)
            return _native.band_shard_attention(q, k, v, mask, S, (vid0, F, P), q_shard, k_shard,
                                                out_dtype=torch.float32 if fp32_parts else None, flags=best_mask_idx)
    if merge_fn is None:
        def merge_fn(o_parts, lse_parts):
            return _native.merge_attention_states(o_parts, lse_parts, out_dtype=q_local.dtype if fp32_parts else None)
    return _attend_over_key_shards(q_local, k_local, v_local, n_tok,
                                   band_shard_exchange_plan(mask, geometry, world, kinds, dense_mask=dense_mask),
                                   lambda src, k_s, v_s: attn_fn(q_local, k_s, v_s, sh[rank], sh[src]), merge_fn, group,
                                   "token_sharded_svg1_attention", post_before_own_part=False)


# ---------------------------------------------------------------------------------------------------------------
# the online profiler on frame shards: no K / V travels — every rank streams its own shard once; what travels is the sampled q rows and one
# partial per rank (svg_sample_mse_shard_partial, svg_sample_mse_from_parts), and every rank ends with the same mse bits.
# ---------------------------------------------------------------------------------------------------------------
def sampled_row_owners(rows, geometry, world: int) -> List[Tuple[int, int]]:
    """(owner rank, row index in that rank's frame_shard) of every sampled row (global indices, a host sequence): a video row lives with
    its frame, every row behind the video on the last rank.  Host only; the same list on every rank."""
    S, vid0, F, P = (int(x) for x in geometry)
    sh, _ = _frame_shards(geometry, world)
    out = []
    for g in (int(x) for x in rows):
        if not 0 <= g < S:
            raise ValueError(f"sampled row {g} outside the {S} rows of the sequence")
        if g < F * P:
            f = g // P
            r = next(r for r in range(world) if sh[r].f0 <= f < sh[r].f0 + sh[r].n_frames)
            out.append((r, g - sh[r].f0 * P))
        else:
            r = world - 1
            out.append((r, P * sh[r].n_frames + g - sh[r].tail_begin))
    return out


def token_sharded_sample_mse(q_local: torch.Tensor, k_local: torch.Tensor, v_local: torch.Tensor, rows: torch.Tensor, prof, geometry,
                             group=None, skip_flag: Optional[torch.Tensor] = None, partial_fn: Optional[Callable] = None,
                             combine_fn: Optional[Callable] = None) -> torch.Tensor:
    """The online profiler (sample_mse) of a sequence that lives sharded by whole frames: q_local, k_local, v_local [..., H, S_r, D] are ALL
    heads of this rank's rows `frame_shard(geometry, rank, world)`; rows is a CPU int64 tensor of sampled GLOBAL rows, the same on every
    rank (the ranks draw from the broadcast-seeded generator); prof the _native.ProfileDesc of the whole sequence; geometry = (num_tokens,
    vid0, num_frame, frame_size).  Returns mse fp32 [2, BH] (BH: the leading dimensions and H), the same bits on every rank.
    The host computes each row's owner and local index (sampled_row_owners).  Each rank puts the rows it owns into a zeroed [BH, R, D]
    buffer; ONE sum over the ranks on an integer view of the bits — every word is non-zero on one rank at most, so no floating-point add is
    involved and the exchange runs over gloo — gives every rank q[:, rows].  Each rank then runs partial_fn(q_rows, k_local, v_local,
    rows_on_device, k_shard) -> part [3, BH, R, D + 4] over its own shard, or fills _native.neutral_profile_part when it holds no rows; the
    parts are all-gathered and combine_fn(parts, R) -> mse merges them in rank order on every rank.  No K / V travels: a rank reads 1 / world of
    what a full call reads and receives (world - 1) parts of 3 BH R (D + 4) fp32.  Nothing is read back and nothing synchronises the device.
    partial_fn and combine_fn default to the native calls (_native.sample_mse_shard_partial, _native.sample_mse_from_parts, both with
    skip_flag); they exist so that the schedule can be tested on gloo without a GPU.  A partial_fn whose parts are not fp32 says so in an
    attribute `part_dtype` (the neutral part of a rank without rows is made in it).
    Not wired into bench_step.py.  Equal to sample_mse on the whole sequence to rounding, not bit for bit."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    S, vid0, F, P = (int(x) for x in geometry)
    if world > _native.PROFILE_MAX_PARTS:
        raise ValueError(f"token_sharded_sample_mse: {world} ranks, but sample_mse_from_parts takes at most {_native.PROFILE_MAX_PARTS} parts")
    sh, n_rows = _frame_shards(geometry, world)
    S_me = n_rows[rank]
    assert q_local.shape[-2] == S_me and k_local.shape == v_local.shape and k_local.shape[-2] == S_me, (
        f"rank {rank} holds {q_local.shape[-2]} / {k_local.shape[-2]} rows, frame_shard says {S_me}")
    D = q_local.shape[-1]
    R = int(rows.numel())
    device = q_local.device
    if partial_fn is None:
        def partial_fn(q_rows, k, v, rows_dev, k_shard):
            return _native.sample_mse_shard_partial(q_rows, k, v, rows_dev, prof, k_shard, S, skip_flag=skip_flag)
    if combine_fn is None:
        def combine_fn(parts, n_rows):
            return _native.sample_mse_from_parts(parts, n_rows, q_local.dtype, prof.emulate_bf16, skip_flag=skip_flag)
    BH = math.prod(q_local.shape[:-2])
    q3, k3, v3 = (x.reshape(BH, S_me, D) for x in (q_local, k_local, v_local))
    # the sampled rows: this rank's into their places of a zeroed buffer, an exact sum over the ranks on the bits
    own = sampled_row_owners(rows.tolist(), geometry, world)
    pos = [i for i, (r, _) in enumerate(own) if r == rank]
    q_rows = torch.zeros((BH, R, D), dtype=q_local.dtype, device=device)
    if pos:
        src = torch.tensor([own[i][1] for i in pos], dtype=torch.int64).to(device, non_blocking=True)
        q_rows.index_copy_(1, torch.tensor(pos, dtype=torch.int64).to(device, non_blocking=True), q3.index_select(1, src))
    if world > 1:
        dist.all_reduce(q_rows.view(torch.int32), op=dist.ReduceOp.SUM, group=group)
    if S_me > 0:
        part = partial_fn(q_rows, k3, v3, rows.to(device, non_blocking=True), sh[rank])
    else:
        part = _native.neutral_profile_part(BH, R, D, device).to(getattr(partial_fn, "part_dtype", torch.float32))
    if world == 1:
        return combine_fn([part], R)
    gathered = _native.empty((world * part.shape[0],) + tuple(part.shape[1:]), dtype=part.dtype, device=device)   # concatenated along dim 0
    dist.all_gather_into_tensor(gathered, part.contiguous(), group=group)
    gathered = gathered.view((world,) + tuple(part.shape))
    return combine_fn([gathered[r] for r in range(world)], R)


def token_sharded_svg1_layer_call(q_local: torch.Tensor, k_local: torch.Tensor, v_local: torch.Tensor, mask, prof, geometry, rows: torch.Tensor,
                                  group=None, fp32_parts: bool = True, partial_fn: Optional[Callable] = None,
                                  combine_fn: Optional[Callable] = None, attn_fn: Optional[Callable] = None,
                                  merge_fn: Optional[Callable] = None, dense_mask=None, dense_flag=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One SVG1 layer-call of a sequence that lives sharded by whole frames, from q, k, v alone: token_sharded_sample_mse picks each head's
    mask — the MSEs rounded to q's dtype before the argmin as svg.models._core.sample_mse rounds them, so two candidates that round to one
    value tie to index 0 and NaN wins — and token_sharded_svg1_attention(..., best_mask_idx, kinds="both") runs the attention under it.
    Returns (o_local [..., H, S_r, D], best_mask_idx int64 [BH], the same on every rank and never read back).  The *_fn arguments go to the two
    schedules (tests on gloo without a GPU).
    dense_mask, dense_flag (both or neither): the processors' device switch — dense_flag (int32 [1] on the device, never read back and
    nothing synchronises) is the profiler's skip_flag and the attention's switch (token_sharded_svg1_attention); the returned best_mask_idx
    is -1 on a dense step, as svg.models._core.svg1_attention_device_switch returns it.
    What svg.models._core runs in frame-shard mode; not wired into bench_step.py."""
    _check_device_switch_pair("token_sharded_svg1_layer_call", dense_mask, dense_flag)
    mse = token_sharded_sample_mse(q_local, k_local, v_local, rows, prof, geometry, group=group, skip_flag=dense_flag, partial_fn=partial_fn,
                                   combine_fn=combine_fn)
    best_mask_idx = torch.argmin(mse.to(q_local.dtype), dim=0)
    o_local = token_sharded_svg1_attention(q_local, k_local, v_local, mask, best_mask_idx, geometry, group=group, fp32_parts=fp32_parts,
                                           kinds="both", attn_fn=attn_fn, merge_fn=merge_fn, dense_mask=dense_mask, dense_flag=dense_flag)
    if dense_flag is not None:
        best_mask_idx = torch.where(dense_flag.reshape(()) != 0, torch.full_like(best_mask_idx, -1), best_mask_idx)
    return o_local, best_mask_idx


class ExchangeBuffers:
    """Staging of the two exchanges either side of a head-sharded attention inside a token-sharded stack, allocated ONCE for a
    (heads, tokens, head_dim, dtype, group) and reused by every layer of every step: tokens_to_heads receives into `recv_in`
    and scatters into one of three persistent [H_local, S, D] tensors (q, k, v); heads_to_tokens packs into `send_out` and
    receives into `recv_out` ([H, S_r, D], returned as a view — consume it before the next call)."""

    def __init__(self, num_heads: int, num_tokens: int, head_dim: int, dtype, device, group=None, unit: int = 1):
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        assert num_heads % world == 0, "ExchangeBuffers: equal head shards (use run_sharded for ragged splits)"
        self.group, self.unit, self.H, self.S, self.D = group, unit, num_heads, num_tokens, head_dim
        self.Hl = num_heads // world
        a, b = token_range(num_tokens, rank, world, unit)
        self.S_me = b - a
        mk = lambda *shape: _native.empty(shape, dtype=dtype, device=device)   # noqa: E731
        self.qkv = [mk(self.Hl, num_tokens, head_dim) for _ in range(3)]
        self.recv_in = mk(self.Hl * num_tokens * head_dim)
        self.send_out = mk(self.Hl * num_tokens * head_dim)
        self.recv_out = mk(num_heads * self.S_me * head_dim)
        self.bytes_in = 0     # received by this rank from OTHER ranks, accumulated (reset by the caller per step)
        self.bytes_out = 0
        self._esz = self.recv_in.element_size()

    def tokens_to_heads(self, x_local: torch.Tensor, which: int) -> torch.Tensor:
        """x_local [H, S_r, D] (all heads of my tokens) -> persistent [H_local, S, D] buffer number `which` (0 q, 1 k, 2 v)"""
        out = tokens_to_heads(x_local, self.S, self.group, self.unit, out=self.qkv[which], recv=self.recv_in)
        self.bytes_in += self.Hl * (self.S - self.S_me) * self.D * self._esz
        return out

    def heads_to_tokens(self, o_local: torch.Tensor) -> torch.Tensor:
        """o_local [H_local, S, D] -> [H, S_r, D] (a view of the receive buffer)"""
        out = heads_to_tokens(o_local, self.H, self.group, self.unit, send=self.send_out, recv=self.recv_out)
        self.bytes_out += (self.H - self.Hl) * self.S_me * self.D * self._esz
        return out


_SIDE_STREAMS: Dict[object, list] = {}


def side_streams(device) -> list:
    """two side streams per device, created once (a torch.cuda.Stream per call would leak HIP streams over a long run)"""
    key = (device.type, device.index)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = [torch.cuda.Stream(device=device) for _ in range(2)]
    return _SIDE_STREAMS[key]


def chunked_head_layout(num_heads: int, rank: int, world: int, max_chunks: int = 3):
    """Head ownership for overlapping the output all-gather with compute: heads are taken in super-groups of world * n
    consecutive heads, n per rank, so the all-gather of local chunk c (n heads per rank) is the contiguous, naturally ordered
    slice [c * world * n, (c + 1) * world * n) of the full [H, ...] output.  Returns (n_chunks, n_per_chunk, my_heads)."""
    assert num_heads % world == 0, (f"chunked_head_layout: {num_heads} heads do not split evenly over {world} ranks — the "
                                    "overlapped scheme needs equal chunks; use sharded_attention / run_sharded (ragged splits) instead")
    local = num_heads // world
    n_chunks = 1 if world == 1 else max(c for c in range(max_chunks, 0, -1) if local % c == 0)
    n_per = local // n_chunks
    mine = [c * world * n_per + rank * n_per + i for c in range(n_chunks) for i in range(n_per)]
    return n_chunks, n_per, mine


def gather_chunk(full: torch.Tensor, o_chunk: torch.Tensor, chunk: int, n_per: int, world: int, group=None, async_op: bool = True):
    """All-gather local chunk `chunk` ([n_per, S, D] on every rank) into its slice of `full` [H, S, D]; returns the work handle."""
    dst = full[chunk * world * n_per:(chunk + 1) * world * n_per]
    return dist.all_gather_into_tensor(dst, o_chunk.contiguous(), group=group, async_op=async_op)


def overlapped_sharded_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, attn_fn: Callable[..., torch.Tensor],
                                 per_head_args: Sequence[torch.Tensor] = (), group=None, max_chunks: int = 3) -> torch.Tensor:
    """`sharded_attention` with the exchange hidden behind compute (what `bench.py --gpus N` times): this rank's heads are
    processed in up to `max_chunks` chunks (`chunked_head_layout`); the all-gather of chunk c runs on the communicator's stream
    while chunk c + 1 computes, and on CUDA the chunk launches alternate between two streams so that the next chunk's workgroups
    fill the idle CUs of a launch's last round.  Needs num_heads % world == 0 and cfg == 1 (one contiguous [H, S, D] output).
    attn_fn(q_c, k_c, v_c, *args_c) -> [1, n, S, D] for tensors sliced to the chunk's n heads."""
    rank, world = dist.get_rank(group), dist.get_world_size(group)
    cfg, H, S, D = q.shape
    assert cfg == 1, "overlapped_sharded_attention: cfg must be 1 (use sharded_attention otherwise)"
    n_chunks, n_per, _ = chunked_head_layout(H, rank, world, max_chunks)
    full = _native.empty((H, S, D), dtype=q.dtype, device=q.device)
    cuda = q.is_cuda
    main = torch.cuda.current_stream() if cuda else None
    side = side_streams(q.device) if cuda and n_chunks > 1 else None
    works = []
    for c in range(n_chunks):
        h0 = c * world * n_per + rank * n_per
        sl = slice(h0, h0 + n_per)
        st = side[c % 2] if side else main
        if side:
            st.wait_stream(main)
        ctx = torch.cuda.stream(st) if cuda else _NullCtx()
        with ctx:
            o_c = attn_fn(q[:, sl].contiguous(), k[:, sl].contiguous(), v[:, sl].contiguous(), *[a[:, sl] for a in per_head_args])
            works.append((gather_chunk(full, o_c[0], c, n_per, world, group), o_c))   # keep o_c alive until its gather is done
    if side:
        for st in side:
            main.wait_stream(st)
    for w, _ in works:
        w.wait()
    return full.unsqueeze(0)


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False
