"""Token-shard mode (svg.distributed.enable_token_shards / run_token_sharded) without a GPU: the box builders of the four exchange layouts
against direct indexing, the runner on gloo (2 and 3 ranks) against the whole-sequence call, the bytes a rank receives, the refusals with
every collective replaced by a failure, the exclusion of the three modes, and the validation table of svg_copy_boxes through the library
(rejected calls and calls whose boxes are all empty never launch, so placeholder pointers are never dereferenced)."""
import ctypes as C
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2   # include/svg_attn.h
PH = 0x10000                           # placeholder device pointer (16-byte aligned; never dereferenced: no call below launches)
ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------------------
# the box builders: one process plays every rank, the exchange is slicing
# ---------------------------------------------------------------------------------------------------------
def _ranges(counts):
    out, a = [], 0
    for n in counts:
        out.append((a, a + n))
        a += n
    return out


def _exchange(sends, splits_of):
    """all_to_all_single of flat buffers in one process: rank j receives block j of every rank's send buffer, in rank order"""
    world = len(sends)
    blocks = []
    for i in range(world):
        sp, off, row = splits_of(i), 0, []
        for n in sp:
            row.append(sends[i][off:off + n])
            off += n
        assert off == sends[i].numel()
        blocks.append(row)
    return [torch.cat([blocks[i][j] for i in range(world)]) for j in range(world)]


@pytest.mark.parametrize("cfg", [1, 2])
@pytest.mark.parametrize("v_view", [False, True])
def test_box_builders_reproduce_the_four_layouts(cfg, v_view):
    D, heads, rows = 64, [2, 2, 1], [131, 64, 70]
    H, S, world = sum(heads), sum(rows), 3
    rr, hr = _ranges(rows), _ranges(heads)
    g = torch.Generator().manual_seed(1)
    full = torch.randn(cfg, H, S, D, generator=g).to(torch.bfloat16)
    # ---- inbound: every rank's [cfg, H, S_r, D] (optionally the head view of a fused [cfg, S_r, 3 H D] projection) -> [cfg, H_l, S, D]
    sends = []
    for (a, b) in rr:
        n = b - a
        if v_view:
            fused = torch.full((cfg, n, 3 * H * D), 7.0, dtype=torch.bfloat16)
            x = fused[:, :, 2 * H * D:].unflatten(2, (H, D)).transpose(1, 2)
            x.copy_(full[:, :, a:b])
            assert not x.is_contiguous() and x.stride(3) == 1
        else:
            x = full[:, :, a:b].contiguous()
        send = torch.full((cfg * H * n * D,), -1.0, dtype=torch.bfloat16)
        nat.copy_boxes_torch([(x, send)], nat.inbound_pack_boxes(cfg, heads, n, D, x.stride()[:3]), D)
        for j, (h0, h1) in enumerate(hr):   # block j is [cfg, H_j, S_r, D], blocks in rank order
            off = cfg * h0 * n * D
            assert torch.equal(send[off:off + cfg * (h1 - h0) * n * D].view(cfg, h1 - h0, n, D), full[:, h0:h1, a:b])
        sends.append(send)
    recvs = _exchange(sends, lambda i: [cfg * hj * rows[i] * D for hj in heads])
    o_local = []
    for j, (h0, h1) in enumerate(hr):
        out = torch.full((cfg, h1 - h0, S, D), -1.0, dtype=torch.bfloat16)
        nat.copy_boxes_torch([(recvs[j], out)], nat.inbound_unpack_boxes(cfg, h1 - h0, rr, D), D)
        assert torch.equal(out, full[:, h0:h1])
        o_local.append(out)
    # ---- outbound, from head-major and from token-major storage: [cfg, H_l, S, D] -> storage [cfg, S_r, H, D]
    for token_major in (False, True):
        sends = []
        for j, (h0, h1) in enumerate(hr):
            o = o_local[j].permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3) if token_major else o_local[j]
            send = torch.full((cfg * (h1 - h0) * S * D,), -1.0, dtype=torch.bfloat16)
            nat.copy_boxes_torch([(o, send)], nat.outbound_pack_boxes(cfg, h1 - h0, rr, D, o.stride()[:3]), D)
            if cfg == 1 and token_major:   # the send buffer IS the token-major storage: what run_token_sharded sends without packing
                assert torch.equal(send, o.permute(0, 2, 1, 3).reshape(-1))
            sends.append(send)
        recvs = _exchange(sends, lambda j: [cfg * n * heads[j] * D for n in rows])
        for i, (a, b) in enumerate(rr):
            store = torch.full((cfg, b - a, H, D), -1.0, dtype=torch.bfloat16)
            nat.copy_boxes_torch([(recvs[i], store)], nat.outbound_unpack_boxes(cfg, heads, b - a, D), D)
            assert torch.equal(store.permute(0, 2, 1, 3), full[:, :, a:b])


def test_boxes_outside_an_allocation_are_refused_before_anything_runs():
    src, dst = torch.zeros(4 * 64, dtype=torch.bfloat16), torch.zeros(4 * 64, dtype=torch.bfloat16)
    inside = nat.Box(0, 0, (1, 1, 4), (0, 0, 64), (0, 0, 64))
    nat.copy_boxes_torch([(src, dst)], [inside], 64)
    for bad in (nat.Box(64, 0, (1, 1, 4), (0, 0, 64), (0, 0, 64)), nat.Box(0, 0, (1, 2, 4), (0, 0, 64), (0, 64, 64)),
                nat.Box(0, -64, (1, 1, 4), (0, 0, 64), (0, 0, 64))):
        with pytest.raises(ValueError):
            nat.copy_boxes_torch([(src, dst)], [bad], 64)
    nat.copy_boxes_torch([(src, dst)], [nat.Box(64, 0, (1, 0, 4), (0, 0, 64), (0, 0, 64))], 64)   # a zero extent copies nothing


# ---------------------------------------------------------------------------------------------------------
# run_token_sharded on gloo against the whole-sequence call
# ---------------------------------------------------------------------------------------------------------
def _fn(q, k, v):
    """a torch `fn` whose rows depend on the whole sequence of their head; small integers in fp32, so every sum is exact whatever its order"""
    o = q * k.sum(dim=2, keepdim=True) + v.flip(2) + torch.cumsum(k, dim=2)
    return o, (q.sum(dim=(2, 3)) > 0).to(torch.int64)


# (H, S, unit, row_counts, cfg, v as a head view, D)
CASES = {
    3: [(5, 64 * 4 + 30, 64, None, 1, False, 64),            # heads 2, 2, 1; rows 128, 64, 94 (a trailing partial unit)
        (5, 265, 128, (131, 64, 70), 2, True, 64),           # explicit row_counts, cfg 2, v a view
        (6, 384, 128, None, 1, True, 128)],                  # even: the byte formula
    2: [(5, 286, 64, None, 2, False, 64),                    # heads 3, 2; rows 128, 158
        (4, 512, 128, None, 1, True, 128),                   # even: the byte formula
        (5, 200, 128, (0, 200), 1, False, 64)],              # a rank without rows still enters every collective
}


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, str(ROOT / "sparse-videogen_amd"))
    from svg import distributed as sd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = []
    for H, S, unit, row_counts, cfg, v_view, D in CASES[world]:
        g = torch.Generator().manual_seed(7)
        q, k, v = (torch.randint(-3, 4, (cfg, H, S, D), generator=g).float() for _ in range(3))
        o_ref, extra_ref = _fn(q, k, v)
        sd.enable_token_shards(unit=unit, row_counts=row_counts)
        a, b = sd.token_shard_range(S)
        expect = sd.token_range(S, rank, world, unit) if row_counts is None else (sum(row_counts[:rank]), sum(row_counts[:rank + 1]))
        ql, kl = q[:, :, a:b].contiguous(), k[:, :, a:b].contiguous()
        if v_view:   # the head view of a fused projection's output [cfg, S_r, 3 H D]
            fused = torch.zeros(cfg, b - a, 3 * H * D)
            vl = fused[:, :, 2 * H * D:].unflatten(2, (H, D)).transpose(1, 2)
            vl.copy_(v[:, :, a:b])
        else:
            vl = v[:, :, a:b].contiguous()
        o, extra = sd.run_token_sharded(_fn, (ql, kl, vl), S, sd.token_shards_group())
        stats = dict(sd.EXCHANGE_STATS)
        sd.disable()
        counts = sd.head_counts(H, world)
        Hl = counts[rank]
        out.append(dict(
            range_ok=(a, b) == expect,
            equal=torch.equal(o, o_ref[:, :, a:b]) and torch.equal(extra, extra_ref) and tuple(o.shape) == (cfg, H, b - a, D),
            view=o.transpose(1, 2).flatten(2, 3)._base is not None or o.numel() == 0,   # the processors' reshape stays a view
            received=stats["received_elements"],
            # three tensors in: this rank's heads of the other ranks' rows; one out: the other ranks' heads of this rank's rows
            formula=3 * cfg * Hl * (S - (b - a)) * D + cfg * (H - Hl) * (b - a) * D,
            even=(4 * (world - 1) * cfg * (H // world) * S * D) // world if H % world == 0 and (b - a) * world == S else None))
    ret[rank] = out
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_run_token_sharded_equals_the_whole_sequence_call(world):
    ret = mp.Manager().dict()
    port = 41500 + (os.getpid() % 2000) + world
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    assert sorted(ret.keys()) == list(range(world))
    for rank in range(world):
        for case, got in zip(CASES[world], ret[rank]):
            assert got["range_ok"] and got["equal"] and got["view"], (rank, case, got)
            assert got["received"] == got["formula"], (rank, case, got)
            if got["even"] is not None:   # (N - 1) / N of four tensors of cfg * H / N * S * D elements
                assert got["received"] == got["even"], (rank, case, got)
    assert any(g["even"] is not None for g in ret[0])


# ---------------------------------------------------------------------------------------------------------
# refusals and mode exclusion, in one process
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def one_rank_group():
    from svg import distributed as sd

    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        yield sd
    finally:
        sd.disable()
        dist.destroy_process_group()


@pytest.fixture
def no_collectives(one_rank_group, monkeypatch):
    """a world of three ranks in which entering any collective is a failure"""
    def fail(*a, **kw):
        raise AssertionError("a collective was entered")

    for name in ("all_to_all_single", "all_gather_into_tensor", "all_gather", "all_reduce", "broadcast", "barrier"):
        monkeypatch.setattr(dist, name, fail)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 3)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 1)
    return one_rank_group


def test_refusals_come_before_any_collective(no_collectives, monkeypatch):
    sd = no_collectives
    from svg.models import _core

    sd.enable_token_shards(unit=64)
    S = 64 * 3
    a, b = sd.token_shard_range(S)
    assert (a, b) == (64, 128)
    x2 = torch.zeros(1, 2, b - a, 64)
    with pytest.raises(ValueError, match="owns no head"):       # 2 heads over 3 ranks
        sd.run_token_sharded(lambda q, k, v: q, (x2, x2, x2), S, None)
    geo = _core.Geometry(0, 3, 64)
    x = torch.zeros(2, 5, b - a, 64)
    prof = nat.ProfileDesc(0, 3, 64, 1)
    mask = nat.BandMask(real_len=S, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
    other = nat.BandMask(real_len=S - 8, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
    monkeypatch.setattr(_core, "_require_gpu", lambda *a, **kw: None)   # (CPU tensors: the refusals under test come first or next)
    with pytest.raises(NotImplementedError, match="return_lse"):
        _core.svg1_sparse_attention(x, x, x, geo, mask, prof, 8, S, return_lse=True)
    with pytest.raises(NotImplementedError, match="return_lse"):
        _core.dense_attention(x, x, x, return_lse=True, geometry=geo)
    with pytest.raises(ValueError, match="out_dtype"):
        _core.dense_attention(x, x, x, out_dtype=torch.float32, geometry=geo)
    with pytest.raises(NotImplementedError, match="per-video"):
        _core.svg1_sparse_attention(x, x, x, geo, [mask, other], prof, 8, S)
    with pytest.raises(NotImplementedError, match="per-video"):
        _core.svg1_attention_device_switch(x, x, x, geo, [mask, other], mask, prof, 8, S, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="per-video"):
        _core.dense_attention(x, x, x, valid_len=[S, S - 8], geometry=geo)
    with pytest.raises(NotImplementedError, match="per-video"):
        _core.svg2_sparse_attention(x, x, x, geo, _core.CentroidStore(), 0, 4, 4, 0.9, 0.1, 2, 1, prompt_length=[0, 8])
    assert _core.rows_of_this_rank("any processor", geo, shard_form=False) == b - a


def test_the_three_modes_exclude_one_another(one_rank_group):
    sd = one_rank_group
    assert not sd.token_shards_active() and not sd.frame_shards_active() and not sd.active()
    sd.enable_token_shards(unit=64)
    assert sd.token_shards_active() and not sd.frame_shards_active() and not sd.active() and sd.token_shards_group() is None
    assert sd.token_shard_range(200) == (0, 200) and sd.token_shard_range(200, 0) == (0, 200)
    for other in (sd.enable, sd.enable_frame_shards):
        with pytest.raises(RuntimeError, match="token-shard mode"):
            other()
    sd.disable()
    assert not sd.token_shards_active()
    sd.enable()
    with pytest.raises(RuntimeError, match="one mode at a time"):
        sd.enable_token_shards()
    sd.disable()
    sd.enable_frame_shards()
    assert sd.frame_shards_active()
    with pytest.raises(RuntimeError, match="one mode at a time"):
        sd.enable_token_shards()
    sd.disable()
    assert not sd.frame_shards_active()
    with pytest.raises(ValueError):
        sd.enable_token_shards(row_counts=(10, 20))   # two counts for one rank
    sd.enable_token_shards(row_counts=(30,))
    assert sd.token_shard_range(30) == (0, 30)
    with pytest.raises(ValueError):
        sd.token_shard_range(31)
    sd.disable()


# ---------------------------------------------------------------------------------------------------------
# svg_copy_boxes: exported, typed as the header declares it, and its return codes in the header's order
# ---------------------------------------------------------------------------------------------------------
def test_entry_is_declared_exported_and_bound():
    header = (ROOT / "include" / "svg_attn_shard_exchange.h").read_text()
    assert "int svg_copy_boxes(const svg_copy_tensor_t* tensors, int32_t n_tensors, const svg_copy_box_t* boxes, int32_t n_boxes" in header
    assert '#include "svg_attn_shard_exchange.h"' in (ROOT / "include" / "svg_attn.h").read_text()
    assert list(nat.SHARD_EXCHANGE_SIGNATURES) == ["svg_copy_boxes"]
    assert C.sizeof(nat.CopyBox) == 80 and C.sizeof(nat.CopyTensor) == 24
    assert nat.load().svg_copy_boxes.argtypes == nat.SHARD_EXCHANGE_SIGNATURES["svg_copy_boxes"][1]
    assert int(nat.load().svg_abi_version()) == nat.SVG_ABI_VERSION == 4


def _box(src_offset=0, dst_offset=0, extent=(0, 2, 16), src_stride=(0, 1024, 64), dst_stride=(0, 2048, 128)):
    return nat.CopyBox(src_offset, dst_offset, (C.c_int32 * 3)(*extent), 0, (C.c_int64 * 3)(*src_stride), (C.c_int64 * 3)(*dst_stride))


def _call(tensors=((PH, 2 * PH, 0, 1),), boxes=None, n_tensors=None, n_boxes=None, D=64, dtype=0, null=()):
    """svg_copy_boxes on placeholder pointers; the default box has a zero extent, so even an accepted call launches nothing"""
    boxes = [_box()] if boxes is None else boxes
    ts = (nat.CopyTensor * max(len(tensors), 1))(*[nat.CopyTensor(*t) for t in tensors])
    bs = (nat.CopyBox * max(len(boxes), 1))(*boxes)
    return nat.load().svg_copy_boxes(None if "tensors" in null else ts, len(tensors) if n_tensors is None else n_tensors,
                                     None if "boxes" in null else bs, len(boxes) if n_boxes is None else n_boxes, D, dtype, None)


VALIDATION = [
    (dict(), OK),
    (dict(null=("tensors",)), BAD_ARG),
    (dict(null=("boxes",)), BAD_ARG),
    (dict(n_tensors=0), BAD_ARG),
    (dict(n_tensors=4), BAD_ARG),
    (dict(n_boxes=0), BAD_ARG),
    (dict(n_boxes=17), BAD_ARG),
    (dict(tensors=((None, 2 * PH, 0, 1),)), BAD_ARG),
    (dict(tensors=((PH, None, 0, 1),)), BAD_ARG),
    (dict(tensors=((PH, 2 * PH, 0, 2),)), BAD_ARG),            # boxes [0, 2) of one
    (dict(tensors=((PH, 2 * PH, -1, 1),)), BAD_ARG),
    (dict(boxes=[_box(extent=(1, -1, 16))]), BAD_ARG),
    (dict(boxes=[_box(src_stride=(0, -1024, 64))]), BAD_ARG),
    (dict(boxes=[_box(dst_stride=(0, 2048, -128))]), BAD_ARG),
    (dict(boxes=[_box(dst_offset=-64)]), BAD_ARG),
    (dict(tensors=((PH, PH, 0, 1),)), BAD_ARG),                # src == dst
    # BAD_ARG wins over UNSUPPORTED, whichever member carries it
    (dict(n_boxes=17, D=96), BAD_ARG),
    (dict(tensors=((PH, PH, 0, 1),), D=96), BAD_ARG),
    (dict(tensors=((PH, PH, 0, 1),), dtype=2), BAD_ARG),
    (dict(boxes=[_box(extent=(1, -1, 16), src_offset=4)]), BAD_ARG),
    (dict(D=96), UNSUPPORTED),
    (dict(D=32), UNSUPPORTED),
    (dict(D=256), UNSUPPORTED),
    (dict(dtype=2), UNSUPPORTED),                               # fp32
    (dict(dtype=-1), UNSUPPORTED),
    (dict(tensors=((PH + 8, 2 * PH, 0, 1),)), UNSUPPORTED),     # a base that is not 16-byte aligned
    (dict(tensors=((PH, 2 * PH + 2, 0, 1),)), UNSUPPORTED),
    (dict(boxes=[_box(src_offset=4)]), UNSUPPORTED),            # an offset of 8 bytes
    (dict(boxes=[_box(dst_offset=12)]), UNSUPPORTED),
    (dict(boxes=[_box(src_stride=(0, 1028, 64))]), UNSUPPORTED),
    (dict(boxes=[_box(dst_stride=(0, 2048, 132))]), UNSUPPORTED),
    (dict(D=128), OK),
    (dict(dtype=1), OK),
    (dict(tensors=((PH, 2 * PH, 0, 1), (3 * PH, 4 * PH, 1, 1), (5 * PH, 6 * PH, 0, 2)), boxes=[_box(), _box(extent=(3, 0, 16))]), OK),
    (dict(boxes=[_box(extent=(2, 2, 0))] * 16), OK),            # 16 boxes, every one empty: nothing to copy
]


@pytest.mark.parametrize("kw,expected", VALIDATION)
def test_validation_order(kw, expected):
    assert _call(**kw) == expected
