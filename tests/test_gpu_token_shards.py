"""Token-shard mode on the GPU (svg.distributed.enable_token_shards; csrc/shard_exchange.hip, include/svg_attn_shard_exchange.h).

1. svg_copy_boxes against the torch statement of the same boxes (_native.copy_boxes_torch), bit for bit, on the four layouts of a world of 3
   ranks with rows (131, 64, 70) and 5 heads (2, 2, 1): cfg 1 and 2, head_dim 64 and 128, bf16 and fp16, v as a view of a fused
   [cfg, S_r, 3 H D] projection; boxes with a zero extent; every destination poisoned and over-allocated on both sides, so a word outside
   the boxes that is written and a word inside them that is not both show; a library that does nothing is caught.  The smallest shapes at
   which a wrong stride, a wrong box offset or a row tail that does not fill a workgroup's tile (64 / 128 rows) shows.
2. Two ranks on one GPU over gloo, core level: each rank holds its token_shard_range rows and every core function returns the rows of the
   whole-sequence call, torch.equal — the geometries of tests/test_gpu_distributed.py.
3. The same at processor level: attention_core_logic of the Wan SVG2, the HunyuanVideo SVG1 (text on the last rank) and the CogVideoX
   (head_dim 64, text first) processors against the same processor on the whole sequence.

Equality is exact everywhere: a rank runs the single-GPU arithmetic on whole heads; nothing is merged or rounded twice."""
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from poisoned import poisoned, unwritten
from test_gpu_poison import DoNothingLibrary

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
HEADS, ROWS = [2, 2, 1], [131, 64, 70]
PAD = 256   # elements of poison in front of and behind every destination


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _ranges(counts):
    out, a = [], 0
    for n in counts:
        out.append((a, a + n))
        a += n
    return out


def _bits(t):
    return t.view(torch.int16)


def _dst_pair(n, dtype):
    """two equal poisoned allocations of n elements with PAD elements of poison on either side: (whole, the n elements) twice"""
    out = []
    for _ in range(2):
        whole = poisoned(n + 2 * PAD, dtype=dtype)
        out.append((whole, whole[PAD:PAD + n]))
    return out


def _both(nat, jobs_of, D, layout, expect_launches=1):
    """run the jobs through the kernel and through the torch statement on equal poisoned destinations; -> the kernel's destinations"""
    (jobs_k, wholes_k), (jobs_t, wholes_t) = jobs_of(0), jobs_of(1)
    assert nat.copy_box_jobs(jobs_k, D, layout) == expect_launches
    for s, d, b in jobs_t:
        nat.copy_boxes_torch([(s, d)], b, D)
    torch.cuda.synchronize()
    for wk, wt in zip(wholes_k, wholes_t):
        assert torch.equal(_bits(wk), _bits(wt)), f"{layout}: the kernel and the torch statement differ"
        assert bool(unwritten(wk[:PAD]).all()) and bool(unwritten(wk[-PAD:]).all()), f"{layout}: a word outside the destination was written"
    return [d for _, d, _ in jobs_k]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("cfg", [1, 2])
def test_copy_boxes_equals_the_torch_statement(nat, cfg, D, dtype):
    H, S = sum(HEADS), sum(ROWS)
    rr, hr = _ranges(ROWS), _ranges(HEADS)
    g = torch.Generator().manual_seed(5)
    full = [torch.randn(cfg, H, S, D, generator=g).to(dtype).cuda() for _ in range(3)]   # q, k, v of the whole sequence
    for rank in range(3):
        a, b = rr[rank]
        n, (h0, h1) = b - a, hr[rank]
        Hl = h1 - h0
        # ---- inbound pack: q, k contiguous, v the head view of a fused projection; at cfg 1 only v needs packing.  One launch.
        ql, kl = (x[:, :, a:b].contiguous() for x in full[:2])
        fused = torch.randn(cfg, n, 3 * H * D, generator=g).to(dtype).cuda()
        vl = fused[:, :, 2 * H * D:].unflatten(2, (H, D)).transpose(1, 2)
        vl.copy_(full[2][:, :, a:b])
        srcs = [vl] if cfg == 1 else [ql, kl, vl]
        pairs = _dst_pair(cfg * H * n * D, dtype), _dst_pair(cfg * H * n * D, dtype), _dst_pair(cfg * H * n * D, dtype)

        def pack_jobs(i):
            ds = [p[i] for p in pairs[:len(srcs)]]
            return [(s, d, nat.inbound_pack_boxes(cfg, HEADS, n, D, s.stride()[:3])) for s, (_, d) in zip(srcs, ds)], [w for w, _ in ds]

        sends = _both(nat, pack_jobs, D, "inbound_pack")
        for s, send in zip(srcs, sends):          # fully written, and block j is [cfg, H_j, S_r, D]
            assert not bool(unwritten(send).any())
            off = cfg * hr[1][0] * n * D
            assert torch.equal(send[off:off + cfg * HEADS[1] * n * D].view(cfg, HEADS[1], n, D), s[:, hr[1][0]:hr[1][1]])
        # ---- inbound unpack: the three receive buffers of this rank (block i [cfg, H_l, S_i, D]) -> [cfg, H_l, S, D].  One launch.
        recvs = [torch.cat([x[:, h0:h1, ra:rb].reshape(-1) for ra, rb in rr]) for x in full]
        pairs = [_dst_pair(cfg * Hl * S * D, dtype) for _ in range(3)]
        boxes = nat.inbound_unpack_boxes(cfg, Hl, rr, D)

        def unpack_jobs(i):
            return [(r, p[i][1], boxes) for r, p in zip(recvs, pairs)], [p[i][0] for p in pairs]

        heads = _both(nat, unpack_jobs, D, "inbound_unpack")
        for x, out in zip(full, heads):
            assert torch.equal(out.view(cfg, Hl, S, D), x[:, h0:h1])
        # ---- outbound pack from head-major and from token-major storage: -> block j [cfg, S_j, H_l, D].  One launch each.
        o_hm = full[0][:, h0:h1].contiguous()
        o_tm = o_hm.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
        for o in (o_hm, o_tm):
            pair = _dst_pair(cfg * Hl * S * D, dtype)
            send, = _both(nat, lambda i: ([(o, pair[i][1], nat.outbound_pack_boxes(cfg, Hl, rr, D, o.stride()[:3]))], [pair[i][0]]), D,
                          "outbound_pack")
            off = cfg * Hl * D * rr[1][0]
            assert torch.equal(send[off:off + cfg * ROWS[1] * Hl * D].view(cfg, ROWS[1], Hl, D), o[:, :, rr[1][0]:rr[1][1]].transpose(1, 2))
        # ---- outbound unpack: block i [cfg, S_r, H_i, D] -> storage [cfg, S_r, H, D].  One launch.
        recv = torch.cat([full[0][:, x0:x1, a:b].transpose(1, 2).reshape(-1) for x0, x1 in hr])
        pair = _dst_pair(cfg * n * H * D, dtype)
        store, = _both(nat, lambda i: ([(recv, pair[i][1], nat.outbound_unpack_boxes(cfg, HEADS, n, D))], [pair[i][0]]), D, "outbound_unpack")
        assert torch.equal(store.view(cfg, n, H, D).permute(0, 2, 1, 3), full[0][:, :, a:b])


@pytest.mark.parametrize("D", [64, 128])
def test_boxes_with_a_zero_extent_copy_nothing(nat, D):
    dtype = torch.bfloat16
    src = torch.randn(2 * 3 * 70 * D).to(dtype).cuda()
    real = nat.Box(0, 0, (2, 3, 70), (3 * 70 * D, 70 * D, D), (3 * 70 * D, 70 * D, D))
    empty = [nat.Box(8 * D, 16 * D, ext, real.src_stride, real.dst_stride) for ext in ((0, 3, 70), (2, 0, 70), (2, 3, 0))]
    for boxes, written in ((empty, False), (empty[:1] + [real] + empty[1:], True)):
        whole = poisoned(src.numel() + 2 * PAD, dtype=dtype)
        dst = whole[PAD:PAD + src.numel()]
        nat.copy_boxes([(src, dst)], boxes, D)
        torch.cuda.synchronize()
        assert bool(unwritten(whole[:PAD]).all()) and bool(unwritten(whole[-PAD:]).all())
        if written:
            assert torch.equal(_bits(dst), _bits(src))
        else:
            assert bool(unwritten(dst).all())


def test_more_boxes_or_tensors_than_a_launch_takes_are_split(nat):
    """20 boxes of one layout over 4 tensors: launches of at most 16 boxes and 3 tensors, the same bits as the torch statement"""
    D, dtype, n = 64, torch.float16, 24
    counts = [n] * 20
    rr = _ranges(counts)
    srcs = [torch.randn(20 * n * D).to(dtype).cuda() for _ in range(4)]
    boxes = nat.inbound_unpack_boxes(1, 1, rr, D)
    pairs = [_dst_pair(20 * n * D, dtype) for _ in range(4)]
    outs = _both(nat, lambda i: ([(s, p[i][1], boxes) for s, p in zip(srcs, pairs)], [p[i][0] for p in pairs]), D, "inbound_unpack",
                 expect_launches=4)   # boxes 0..15 for three tensors, then for the fourth; boxes 16..19 likewise
    for s, o in zip(srcs, outs):
        assert torch.equal(_bits(s), _bits(o))


def test_do_nothing_library_is_caught(nat, monkeypatch):
    lib = DoNothingLibrary()
    monkeypatch.setattr(nat, "load", lambda strict=True: lib)
    D, dtype = 128, torch.bfloat16
    src = torch.randn(4 * 70 * D).to(dtype).cuda()
    dst = poisoned(4 * 70 * D, dtype=dtype)
    assert nat.copy_box_jobs([(src, dst, nat.inbound_unpack_boxes(1, 4, [(0, 70)], D))], D, "inbound_unpack") == 1
    torch.cuda.synchronize()
    assert lib.calls == ["svg_copy_boxes"]
    assert bool(unwritten(dst).all()), "the destination was written although the library did nothing"


# ---------------------------------------------------------------------------------------------------------
# two ranks on one GPU over gloo, a fresh child process per rank
# ---------------------------------------------------------------------------------------------------------
def _setup_rank(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT), str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from svg import _native as nat_
    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    return nat_, torch.device("cuda", 0)


def structured_qkv(H, D, ctx, F, P, text_first, seed):
    """randn q, k, v [1, H, S, D] bf16 whose keys are alike at one patch position on even heads (temporal) and alike within a frame on odd
    heads (spatial), so that both kinds of head occur for a reason"""
    V, S = F * P, F * P + ctx
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(1, H, S, D, generator=g) for _ in range(3))
    pos, frm = torch.randn(P, D, generator=g), torch.randn(F, D, generator=g)
    v0 = ctx if text_first else 0
    for h in range(H):
        add = 3 * (frm.repeat_interleave(P, 0) if h % 2 else pos.repeat(F, 1))
        q[0, h, v0:v0 + V] += add
        k[0, h, v0:v0 + V] += add
    return tuple(x.to(torch.bfloat16) for x in (q, k, v))


def _local(x, a, b, as_view=False):
    """this rank's rows of [cfg, H, S, D]; as_view: as the head view of a fused [cfg, S_r, 3 H D] projection's output"""
    if not as_view:
        return x[:, :, a:b].contiguous()
    cfg, H, _, D = x.shape
    fused = torch.zeros(cfg, b - a, 3 * H * D, dtype=x.dtype, device=x.device)
    view = fused[:, :, 2 * H * D:].unflatten(2, (H, D)).transpose(1, 2)
    view.copy_(x[:, :, a:b])
    return view


def _core_worker(rank, world, port, ret):
    nat_, dev = _setup_rank(rank, world, port)
    from svg import distributed as sd
    from svg.models import _core
    from svg.models.hyvideo.utils import dense_mask, profile_desc

    res = {}
    # ---- SVG1 (Hunyuan-like geometry: 5 heads, 4 x 200 + 40 rows) and dense attention
    H, D, F_, P_, ctx, L = 5, 128, 4, 200, 40, 11
    V = F_ * P_
    S = V + ctx
    q, k, v = (x.to(dev) for x in structured_qkv(H, D, ctx, F_, P_, False, 3))
    geo = _core.Geometry(ctx, F_, P_)
    mask = nat_.BandMask(real_len=V + L, band=256, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    dense = dense_mask(S, V + L)
    prof = profile_desc(ctx, F_, P_)

    def sparse(qq, kk, vv):
        torch.manual_seed(11)   # sample_mse draws its rows from the CPU generator: the same on every rank
        return _core.svg1_sparse_attention(qq, kk, vv, geo, mask, prof, 32, V)

    def switch(value):
        def run(qq, kk, vv):
            _core.reseed_switch_generator(11)
            flag = torch.full((1,), value, dtype=torch.int32, device=dev)
            return _core.svg1_attention_device_switch(qq, kk, vv, geo, mask, dense, prof, 32, V, flag)
        return run

    def dense_call(qq, kk, vv):
        return (_core.dense_attention(qq, kk, vv, V + L, geometry=geo),)

    calls = {"sparse": sparse, "switch0": switch(0), "switch1": switch(1), "dense": dense_call}
    whole = {name: fn(q, k, v) for name, fn in calls.items()}
    sd.enable_token_shards(unit=128)
    a, b = sd.token_shard_range(S)
    res["range"] = (a, b)
    ql, kl, vl = _local(q, a, b), _local(k, a, b), _local(v, a, b, as_view=True)
    for name, fn in calls.items():
        got = fn(ql, kl, vl)
        stats = dict(sd.EXCHANGE_STATS)
        torch.cuda.synchronize()
        o_w, o_l = whole[name][0], got[0]
        entry = dict(equal=bool(torch.equal(o_l, o_w[:, :, a:b])) and o_l.shape == ql.shape, launches=stats["launches"],
                     view=o_l.transpose(1, 2).flatten(2, 3)._base is not None)
        if len(got) > 1:
            entry["best"], entry["best_equal"] = got[1].cpu(), bool(torch.equal(got[1], whole[name][1]))
        res[name] = entry
    sd.disable()
    # ---- SVG2 (Wan-like: no text, 5 heads, 5 x 300 rows), first call (random initial points) and warm-started call
    H2, F2, P2 = 5, 5, 300
    S2 = F2 * P2
    g = torch.Generator().manual_seed(3)
    q2, k2, v2 = (torch.randn(1, H2, S2, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(3))
    geo2 = _core.Geometry(0, F2, P2)

    def svg2(store, qq, kk, vv):
        outs = []
        for call in range(2):
            torch.manual_seed(5 + call)
            torch.cuda.manual_seed(5 + call)
            outs.append(_core.svg2_sparse_attention(qq, kk, vv, geo2, store, 0, 12, 30, 0.9, 0.1, 4, 2))
        return outs

    ref2 = svg2(_core.CentroidStore(), q2, k2, v2)
    sd.enable_token_shards(unit=128)
    a2, b2 = sd.token_shard_range(S2)
    sh2 = svg2(_core.CentroidStore(), _local(q2, a2, b2), _local(k2, a2, b2), _local(v2, a2, b2, as_view=True))
    sd.disable()
    torch.cuda.synchronize()
    res["range2"] = (a2, b2)
    res["svg2"] = [bool(torch.equal(x, y[:, :, a2:b2])) and bool(torch.isfinite(x.float()).all()) for x, y in zip(sh2, ref2)]
    ret[rank] = res
    dist.destroy_process_group()


def test_core_functions_in_token_shard_mode_two_ranks_one_gpu():
    world = 2
    ret = mp.Manager().dict()
    port = 36500 + (os.getpid() % 2000)
    mp.spawn(_core_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    assert [got[r]["range"] for r in (0, 1)] == [(0, 384), (384, 840)] and [got[r]["range2"] for r in (0, 1)] == [(0, 768), (768, 1500)]
    for r in (0, 1):
        for name in ("sparse", "switch0", "switch1", "dense"):
            g = got[r][name]
            assert g["equal"] and g["view"], (r, name, g)
            # cfg 1, v a head view: v is packed, q, k, v are unpacked, o leaves the core token-major (no pack) and is unpacked
            assert g["launches"] == 3, (r, name, g["launches"])
        for name in ("sparse", "switch0", "switch1"):
            assert got[r][name]["best_equal"] and got[r][name]["best"].shape == (1, 5), (r, name)
        assert got[r]["switch1"]["best"].tolist() == [[-1] * 5]                       # a dense step
        for name in ("sparse", "switch0"):
            assert sorted(set(got[r][name]["best"].flatten().tolist())) == [0, 1], got[r][name]["best"]   # both kinds of head occur
        assert got[r]["svg2"] == [True, True], (r, got[r]["svg2"])


def _processor_worker(rank, world, port, ret, model):
    nat_, dev = _setup_rank(rank, world, port)
    from svg import distributed as sd
    from svg.models import _core

    if model == "wan_sap":
        from svg.models.wan.attention import WanAttn_SAPAttn_Processor as cls
        H, D, ctx, F_, P_, text_first = 5, 128, 0, 5, 300, False
        cls.num_q_centroids, cls.num_k_centroids, cls.top_p_kmeans, cls.min_kc_ratio = 12, 30, 0.9, 0.1
        cls.kmeans_iter_init, cls.kmeans_iter_step = 4, 2
        cls.first_layers_fp, cls.first_times_fp = 1, 0.5
        times = {"sparse": 0.25, "dense": 0.75}
    elif model == "hy":
        from svg.models.hyvideo.attention import Hunyuan_SVGAttn_Processor2_0 as cls
        from svg.models.hyvideo.utils import generate_temporal_head_mask_mod
        H, D, ctx, F_, P_, text_first = 5, 128, 40, 4, 200, False
        cls.prompt_length = 11
        cls.block_mask = generate_temporal_head_mask_mod(ctx, 11, F_, P_, mul=2)
        cls.first_layers_fp, cls.first_times_fp = 1, 0.5
        times = {"sparse": 0.25, "dense": 0.75}
    else:
        from svg.models.cog.attention import CogVideoX_SparseAttn_Processor2_0 as cls
        from svg.models.cog.utils import generate_temporal_head_mask_mod
        H, D, ctx, F_, P_, text_first = 5, 64, 40, 4, 200, True
        cls.block_mask = generate_temporal_head_mask_mod(ctx, F_, P_, mul=2, attn_sink=False)
        cls.first_layers_fp, cls.first_times_fp = 1 / 42, 0.5      # fractions of 42 layers / 1000 timesteps: layer 1, timestep 500
        times = {"sparse": 250.0, "dense": 750.0}
    cls.context_length, cls.num_frame, cls.frame_size = ctx, F_, P_
    cls.num_sampled_rows, cls.sample_mse_max_row = 32, 10000
    S = ctx + F_ * P_
    q, k, v = (x.to(dev) for x in structured_qkv(H, D, ctx, F_, P_, text_first, 17))
    # (layer, timestep): a sparse step twice (SVG2: first and warm-started call), a dense warm-up step, a layer below first_layers_fp
    steps = [("sparse", 1, times["sparse"]), ("sparse_again", 1, times["sparse"]), ("dense", 1, times["dense"]),
             ("host_dense", 0, times["sparse"])]

    def run(qq, kk, vv):
        _core.reseed_switch_generator(11)
        procs, out = {}, {}
        for i, (what, layer, t) in enumerate(steps):
            torch.manual_seed(5 + i)
            torch.cuda.manual_seed(5 + i)
            proc = procs.setdefault(layer, cls(layer))      # (SVG2: one processor per layer keeps its centroids)
            ts = torch.tensor([t], device=dev)
            args = (qq, kk, vv, ts) + ((layer, None) if model == "hy" else ())
            out[what] = (proc.attention_core_logic(*args), getattr(proc, "last_best_mask_idx", None))
        return out

    whole = run(q, k, v)
    sd.enable_token_shards(unit=128)
    a, b = sd.token_shard_range(S)
    local = run(_local(q, a, b), _local(k, a, b), _local(v, a, b, as_view=True))
    sd.disable()
    torch.cuda.synchronize()
    res = {"range": (a, b)}
    for what, _, _ in steps:
        (ow, bw), (ol, bl) = whole[what], local[what]
        res[what] = dict(equal=bool(torch.equal(ol, ow[:, :, a:b])) and ol.shape == (1, H, b - a, D),
                         finite=bool(torch.isfinite(ol.float()).all()),
                         best_equal=(bw is None and bl is None) or bool(torch.equal(bw, bl)), best=None if bl is None else bl.cpu())
    ret[rank] = res
    dist.destroy_process_group()


@pytest.mark.parametrize("model", ["wan_sap", "hy", "cog"])
def test_processor_in_token_shard_mode_two_ranks_one_gpu(model):
    world = 2
    ret = mp.Manager().dict()
    port = 38500 + (os.getpid() % 2000) + ["wan_sap", "hy", "cog"].index(model)
    mp.spawn(_processor_worker, args=(world, port, ret, model), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    assert [got[r]["range"] for r in (0, 1)] == ([(0, 768), (768, 1500)] if model == "wan_sap" else [(0, 384), (384, 840)])
    for r in (0, 1):
        for what in ("sparse", "sparse_again", "dense", "host_dense"):
            g = got[r][what]
            assert g["equal"] and g["finite"] and g["best_equal"], (model, r, what, g)
        if model != "wan_sap":
            assert got[r]["dense"]["best"].tolist() == [[-1] * 5]
        if model == "hy":   # (on these inputs CogVideoX's profiler picks one mask for every head; equality is what is asserted there)
            assert sorted(set(got[r]["sparse"]["best"].flatten().tolist())) == [0, 1], got[r]["sparse"]["best"]
