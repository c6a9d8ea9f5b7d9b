"""The online profiler on frame shards on the GPU (include/svg_attn_profile_shard.h; csrc/profiler.hip: profile16_kernel on
ProfileShardPolicy, profile_shard_reduce_kernel, profile_combine_parts_kernel): one part of the whole sequence against svg_sample_mse bit for bit, the parts of
frame shards merged against the oracle, shards whose stored index jumps inside a key tile, a sampled text row, a shard no sampled row sees
under the spatial mask, strided k / v, the skip flag, the poison rows of the two entries and their wrappers, and
svg.distributed.token_sharded_svg1_layer_call on two ranks sharing the GPU.

Geometry: F 5, P 300 (no multiple of 64: key tiles straddle frames and, on a shard's own grid, lie elsewhere than on the sequence's),
32 text rows behind the video for hy and none for wan, H 3, D 128, bf16; the structured data of tests/test_gpu_kernels.py::test_sample_mse
(head 0 temporal, head 1 spatial).  Tolerances: those of that test and nothing tighter — fp32 against O.sample_mse_fp32 rtol 3e-2 atol 1e-6,
emulate against O.sample_mse rtol 8e-2 atol 1e-5.
The argmin assertions (heads 0 and 1) cannot flip inside those.  Seen on the CPU with O.sample_mse_fp32 for the row sets whose argmin is
asserted (R 48: video rows, with a text row, rows of frame 0; hy and wan): head 0 has 0.73 to 0.97 under the spatial mask and at most 5e-17
under the temporal one, head 1 has 0.21 to 0.31 under the temporal mask and at most 1.1e-5 under the spatial one (0 for wan and for the rows
of frame 0) — the structured data makes the right mask nearly exact.  After the largest allowed error the larger value is still above
0.92 x 0.21 = 0.19 and the smaller below 1.08 x 1.1e-5 + 1e-5 = 2.2e-5; O.sample_mse (bf16) shows the same picture (the small values round
to 0).  Head 2 is unstructured: its two MSEs lie within 13 % of each other (2.8e-3 / 3.2e-3), so nothing is asserted about its argmin.

ref: sample_mse, svg/models/hyvideo/attention.py:376-399 (wan/attention.py:211-234)."""
import ctypes as C
import functools
import inspect
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import svg_oracle as O
from poisoned import assert_fully_written, poisoned, unwritten
from sparse_lse_cases import T_SINGLE, masked_attention_lse
from test_gpu_kernels import _prof_desc, dev
from test_gpu_poison import DoNothingLibrary

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
F_, P_, H, D = 5, 300, 3, 128
V = F_ * P_
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def ctx_of(model):
    return 32 if model == "hy" else 0


@functools.lru_cache(maxsize=None)
def inputs(model):
    """q, k, v [1, H, S, D] bf16 as test_sample_mse builds them: head 0 "temporal" (keys alike at one patch position), head 1 "spatial" """
    g = torch.Generator().manual_seed(6)
    S = V + ctx_of(model)
    q, k, v = (torch.randn(1, H, S, D, generator=g) for _ in range(3))
    pos, frm = torch.randn(P_, D, generator=g), torch.randn(F_, D, generator=g)
    k[0, 0, :V] += 3 * pos.repeat(F_, 1)
    q[0, 0, :V] += 3 * pos.repeat(F_, 1)
    k[0, 1, :V] += 3 * frm.repeat_interleave(P_, 0)
    q[0, 1, :V] += 3 * frm.repeat_interleave(P_, 0)
    return tuple(x.to(BF16) for x in (q, k, v))


@functools.lru_cache(maxsize=None)
def rows_of(kind, R):
    g = torch.Generator().manual_seed(60 + R)
    if kind == "frame0":                                      # rows of frame 0 only, distinct
        return torch.randperm(P_, generator=g)[:R]
    rows = torch.randint(0, min(V, 700), (R,), generator=g)
    if kind == "text":                                        # a sampled text row (hy) among video rows
        rows[R // 2] = V + 3
    return rows


@functools.lru_cache(maxsize=None)
def oracle(model, kind, R):
    """(fp32 oracle, bf16 oracle as float) [2, H], computed once"""
    q, k, v = inputs(model)
    masks = list(O.profile_masks(model, ctx_of(model), F_, P_))
    rows = rows_of(kind, R)
    return O.sample_mse_fp32(q, k, v, rows, masks)[:, 0], O.sample_mse(q, k, v, rows, masks)[:, 0].float()


def shard_keys(shard):
    f0, n, tail0, n_tail = shard
    return torch.cat([torch.arange(f0 * P_, (f0 + n) * P_), torch.arange(tail0, tail0 + n_tail)])


def whole(model):
    return (0, F_, V, ctx_of(model))


def frame_shards(model, world):
    from svg.distributed import frame_shard

    S = V + ctx_of(model)
    return [s for s in (frame_shard((S, 0, F_, P_), r, world).as_tuple() for r in range(world)) if s[1] or s[3]]


@functools.lru_cache(maxsize=None)
def device_shard(model, shard):
    """(k, v) [H, Sk, D] of a shard on the device, contiguous"""
    _, k, v = inputs(model)
    keys = shard_keys(shard)
    return dev(k[0][:, keys]), dev(v[0][:, keys])


def part_of(nat, model, rows, shard, emulate, **kw):
    q = inputs(model)[0]
    k, v = device_shard(model, shard)
    S = V + ctx_of(model)
    return nat.sample_mse_shard_partial(dev(q[0][:, rows]), k, v, dev(rows), _prof_desc(nat, model, ctx_of(model), F_, P_, emulate), shard, S,
                                        **kw)


def merged(nat, model, rows, shards, emulate):
    parts = [part_of(nat, model, rows, s, emulate) for s in shards]
    return nat.sample_mse_from_parts(parts, rows.numel(), BF16, emulate).cpu()


def single_call(nat, model, rows, emulate):
    q, k, v = (dev(x[0]) for x in inputs(model))
    return nat.sample_mse(q, k, v, dev(rows), _prof_desc(nat, model, ctx_of(model), F_, P_, emulate)).cpu()


def check_against_the_oracle(nat, model, kind, R, shards):
    """the assertions of a set of shards that covers the keys: the merged MSEs against the two oracles at the tolerances of test_sample_mse,
    and the argmin — the oracle's, the single call's, and 1 for head 0 / 0 for head 1 as constructed"""
    rows = rows_of(kind, R)
    ref32, refbf = oracle(model, kind, R)
    got32, gotbf = merged(nat, model, rows, shards, False), merged(nat, model, rows, shards, True)
    print(f"{model} {kind} R={R} shards {shards}:\n  fp32 {got32.tolist()}\n  ref  {ref32.tolist()}\n  emul {gotbf.tolist()}\n  ref  {refbf.tolist()}")
    assert got32.shape == (2, H) and got32.dtype == torch.float32
    torch.testing.assert_close(got32, ref32, rtol=3e-2, atol=1e-6)
    torch.testing.assert_close(gotbf, refbf, rtol=8e-2, atol=1e-5)
    one = single_call(nat, model, rows, False)
    assert torch.equal(got32.argmin(0)[:2], ref32.argmin(0)[:2]) and torch.equal(got32.argmin(0)[:2], one.argmin(0)[:2])
    assert got32.argmin(0)[0] == 1 and got32.argmin(0)[1] == 0
    return got32, gotbf


# ---------------------------------------------------------------------------------------------------------
# 1. the whole sequence, one part: the bits of svg_sample_mse
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [5, 48, 64])
@pytest.mark.parametrize("emulate", [False, True], ids=["fp32", "emulate"])
@pytest.mark.parametrize("model", ["hy", "wan"])
def test_one_part_of_the_whole_sequence_is_sample_mse_bit_for_bit(nat, model, emulate, R):
    rows = rows_of("text" if model == "hy" else "video", R)
    want = single_call(nat, model, rows, emulate)
    part = part_of(nat, model, rows, whole(model), emulate)
    assert part.shape == (3, H, R, D + 4) and part.dtype == torch.float32 and part.is_contiguous()
    got = nat.sample_mse_from_parts([part], R, BF16, emulate).cpu()
    assert torch.isfinite(want).all()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (got, want)
    pc = part.cpu()
    assert bool((pc[..., D + 2:] == 0).all()) and torch.isfinite(pc[..., D]).all() and bool((pc[0, ..., D + 1] > 0).all())
    assert torch.equal(pc[1, ..., D], pc[0, ..., D]) and torch.equal(pc[2, ..., D], pc[0, ..., D])     # one reference for the three outputs


# ---------------------------------------------------------------------------------------------------------
# 2. the shards of frame_shard for 2 and 3 ranks, merged
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("model", ["hy", "wan"])
def test_frame_shards_merged(nat, model, world):
    shards = frame_shards(model, world)
    assert len(shards) == world and sum(s[1] for s in shards) == F_ and shards[-1][3] == ctx_of(model)
    check_against_the_oracle(nat, model, "video", 48, shards)


# ---------------------------------------------------------------------------------------------------------
# 3. seams: the stored index jumps inside a key tile (frames [0, 2) and the tail: local key 600 is row 1500), and a shard that is the
#    tail alone; 4. a sampled text row among video rows
# ---------------------------------------------------------------------------------------------------------
SEAMS = {"frames_0_2_and_the_tail": [(0, 2, V, 32), (2, 3, 0, 0)], "all_frames_and_the_tail_alone": [(0, F_, 0, 0), (0, 0, V, 32)],
         "a_tail_in_two": [(0, 2, V + 20, 12), (2, 3, V, 20)]}


@pytest.mark.parametrize("name", list(SEAMS))
def test_seams(nat, name):
    check_against_the_oracle(nat, "hy", "video", 48, SEAMS[name])


@pytest.mark.parametrize("shards", [[(0, F_, V, 32)], [(0, 3, 0, 0), (3, 2, V, 32)], SEAMS["frames_0_2_and_the_tail"]], ids=["whole", "two", "seam"])
def test_a_sampled_text_row(nat, shards):
    assert int((rows_of("text", 48) >= V).sum()) == 1
    check_against_the_oracle(nat, "hy", "text", 48, shards)


# ---------------------------------------------------------------------------------------------------------
# 5. a far shard: the rows come from frame 0, the shard is frames [3, 5) — no key under the spatial mask
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["hy", "wan"])
def test_a_far_shard(nat, model):
    R = 48
    rows = rows_of("frame0", R)
    far, near = (3, 2, 0, 0), (0, 3, V, ctx_of(model))
    part = part_of(nat, model, rows, far, False)
    pc = part.cpu()
    assert bool((pc[1, ..., D + 1] == 0).all()) and bool((pc[1, ..., :D] == 0).all())        # output 1: l == 0 and O == 0 ...
    assert torch.isfinite(pc[..., D]).all()                                                    # ... and a finite m
    assert bool((pc[0, ..., D + 1] > 0).all()) and bool((pc[2, ..., D + 1] > 0).all())        # the golden rows and the temporal mask see it
    got32, gotbf = check_against_the_oracle(nat, model, "frame0", R, [near, far])
    # a neutral part, anywhere in the list: the same bits
    for em, want in ((False, got32), (True, gotbf)):
        parts = [part_of(nat, model, rows, s, em) for s in (near, far)]
        neutral = nat.neutral_profile_part(H, R, D, "cuda")
        for lst in ([neutral] + parts, [parts[0], neutral, parts[1]], parts + [neutral]):
            got = nat.sample_mse_from_parts(lst, R, BF16, em).cpu()
            assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------
# 6. k and v as views of one fused projection buffer: the bits of the contiguous call
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emulate", [False, True], ids=["fp32", "emulate"])
def test_strided_k_v(nat, emulate):
    model, shard = "hy", (3, 2, V, 32)
    rows = rows_of("text", 48)
    q, k, v = inputs(model)
    keys = shard_keys(shard)
    n = len(keys)
    fused = dev(torch.cat([x[0][:, keys].transpose(0, 1).reshape(n, H * D) for x in (q, k, v)], dim=1))     # [S_r, 3 H D]
    kv, vv = (fused[:, i * H * D:(i + 1) * H * D].unflatten(1, (H, D)).transpose(0, 1) for i in (1, 2))
    assert not kv.is_contiguous() and kv.stride() == (D, 3 * H * D, 1) and torch.equal(kv.cpu(), k[0][:, keys])
    want = part_of(nat, model, rows, shard, emulate)
    S = V + ctx_of(model)
    real = nat.load().svg_sample_mse_shard_partial
    got = nat.sample_mse_shard_partial(dev(q[0][:, rows]), kv, vv, dev(rows), _prof_desc(nat, model, 32, F_, P_, emulate), shard, S)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # ... and it was the layout that read them: the raw entry on the same views
    part = poisoned(3, H, 48, D + 4, dtype=torch.float32)
    ws = poisoned(nat.load().svg_sample_mse_shard_workspace_bytes(H, 48, D, n), dtype=torch.uint8)
    k4, v4 = kv.unsqueeze(0), vv.unsqueeze(0)
    lay = nat.attn_layout(k4, k4, v4, k4)
    qr, rd, pd, sh = dev(q[0][:, rows]), dev(rows), _prof_desc(nat, model, 32, F_, P_, emulate), nat.BandShard(*shard)
    rc = real(qr.data_ptr(), kv.data_ptr(), vv.data_ptr(), rd.data_ptr(), 48, H, S, D, 0, 1.0 / D ** 0.5, C.byref(pd), C.byref(sh),
              part.data_ptr(), ws.data_ptr(), ws.numel(), None, C.byref(lay), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and torch.equal(part.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------
# 7. skip_flag = 1: part and out_mse keep their poison
# ---------------------------------------------------------------------------------------------------------
def test_skip_flag(nat):
    assert nat.allocations_poisoned()
    rows = rows_of("video", 48)
    one, zero = torch.ones(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    shard = (3, 2, V, 32)
    part = part_of(nat, "hy", rows, shard, False, skip_flag=one)
    torch.cuda.synchronize()
    assert bool(unwritten(part).all())
    live = part_of(nat, "hy", rows, shard, False, skip_flag=zero)
    assert torch.equal(live.view(torch.int32), part_of(nat, "hy", rows, shard, False).view(torch.int32))
    mse = nat.sample_mse_from_parts([live], 48, BF16, False, skip_flag=one)
    torch.cuda.synchronize()
    assert bool(unwritten(mse).all())
    assert_fully_written(nat.sample_mse_from_parts([live], 48, BF16, False, skip_flag=zero), "out_mse")


# ---------------------------------------------------------------------------------------------------------
# 8. poison rows: the wrappers and the two entries called raw, at a shard that holds rows without a key under one output (stored:
#    zeros) and ends inside a key tile, with R = 5 (three waves without rows) and R = 64.  The do-nothing library of
#    tests/test_gpu_poison.py: every output must then still hold the poison; on the real library every word is written.
# ---------------------------------------------------------------------------------------------------------
def _wrapper_outs(nat, model, R):
    rows = rows_of("frame0", R)
    part = part_of(nat, model, rows, (3, 2, 0, 0), False)
    return {"part": part, "out_mse": nat.sample_mse_from_parts([part, part_of(nat, model, rows, (0, 3, V, ctx_of(model)), False)], R, BF16, False)}


def _raw_outs(nat, model, R):
    lib = nat.load()
    rows = rows_of("frame0", R)
    S = V + ctx_of(model)
    q = inputs(model)[0]
    qr, rd, pd = dev(q[0][:, rows]), dev(rows), _prof_desc(nat, model, ctx_of(model), F_, P_, False)
    parts = []
    for shard in ((3, 2, 0, 0), (0, 3, V, ctx_of(model))):
        k, v = device_shard(model, shard)
        sh = nat.BandShard(*shard)
        part = poisoned(3, H, R, D + 4, dtype=torch.float32)
        ws = poisoned(lib.svg_sample_mse_shard_workspace_bytes(H, R, D, k.shape[1]), dtype=torch.uint8)
        rc = lib.svg_sample_mse_shard_partial(qr.data_ptr(), k.data_ptr(), v.data_ptr(), rd.data_ptr(), R, H, S, D, 0, 1.0 / D ** 0.5, C.byref(pd),
                                              C.byref(sh), part.data_ptr(), ws.data_ptr(), ws.numel(), None, None,
                                              torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        parts.append(part)
    out = poisoned(2, H, dtype=torch.float32)
    ws = poisoned(lib.svg_sample_mse_from_parts_workspace_bytes(H), dtype=torch.uint8)
    pp = (C.c_void_p * 2)(*[p.data_ptr() for p in parts])
    rc = lib.svg_sample_mse_from_parts(C.cast(pp, C.c_void_p), 2, R, H, D, 0, 0, out.data_ptr(), ws.data_ptr(), ws.numel(), None,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return {"part": parts[0], "near part": parts[1], "out_mse": out}


@pytest.mark.parametrize("R", [5, 64])
@pytest.mark.parametrize("how", [_wrapper_outs, _raw_outs], ids=["wrapper", "entry"])
@pytest.mark.parametrize("model", ["hy", "wan"])
def test_real_library_writes_every_word(nat, model, how, R):
    assert nat.allocations_poisoned()
    outs = how(nat, model, R)
    torch.cuda.synchronize()
    for what, t in outs.items():
        assert_fully_written(t, f"{model} R={R}: {what}")
    ref32 = oracle(model, "frame0", R)[0]
    torch.testing.assert_close(outs["out_mse"].cpu(), ref32, rtol=3e-2, atol=1e-6)
    assert bool((outs["part"][1, ..., D + 1] == 0).all())       # the rows without a key are there, and they were stored


def test_do_nothing_library_is_caught(nat, monkeypatch):
    lib = DoNothingLibrary()
    monkeypatch.setattr(nat, "load", lambda strict=True: lib)
    outs = _wrapper_outs(nat, "hy", 48)
    torch.cuda.synchronize()
    assert [c for c in lib.calls if not c.endswith("_workspace_bytes")] == ["svg_sample_mse_shard_partial"] * 2 + ["svg_sample_mse_from_parts"]
    for what, t in outs.items():
        with pytest.raises(AssertionError, match="still hold the poison pattern"):
            assert_fully_written(t, what)
        assert bool(unwritten(t).all()), f"{what} was partly written although the library did nothing"


def test_the_wrappers_allocate_through_the_switch(nat):
    """tests/test_gpu_poison.py finds the allocating wrappers among the `def`s of svg._native and their rows in its own file; these are
    bound by assignment and their rows are here: they are the functions that allocate through the switch, and this file calls them"""
    import ast

    src = inspect.getsource(sys.modules[__name__])
    for public, private in (("sample_mse_shard_partial", nat._sample_mse_shard_partial), ("sample_mse_from_parts", nat._sample_mse_from_parts),
                            ("neutral_profile_part", nat._neutral_profile_part)):
        assert getattr(nat, public) is private
        names = {c.func.id for c in ast.walk(ast.parse(inspect.getsource(private))) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
        assert "empty" in names and f"nat.{public}(" in src
    n = nat.neutral_profile_part(H, 5, D, "cuda")
    assert_fully_written(n, "neutral part")


# ---------------------------------------------------------------------------------------------------------
# 9. token_sharded_svg1_layer_call: two ranks on one GPU over gloo, a fresh child process per rank
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT), str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import test_gpu_profile_shard as T
    from svg import _native as nat_
    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    from svg import distributed as sd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    model, R = "hy", 48
    S = T.V + 32
    geo = (S, 0, T.F_, T.P_)
    q, k, v = (x[0] for x in T.inputs(model))
    rows = T.rows_of("text", R)
    prof = T._prof_desc(nat_, model, 32, T.F_, T.P_, False)
    mp_ = dict(real_len=S, band=384, colfull_lo=T.V, colfull_hi=S, rowfull_lo=T.V, rowfull_hi=S)
    mask = nat_.BandMask(**mp_)
    sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
    mine = T.shard_keys(sh[rank])
    ql, kl, vl = (x[:, mine].to(device) for x in (q, k, v))
    res = {"shard": sh[rank]}
    mse = sd.token_sharded_sample_mse(ql, kl, vl, rows, prof, geo)
    o, best = sd.token_sharded_svg1_layer_call(ql, kl, vl, mask, prof, geo, rows)
    # the single-process statement: the same two partial calls and the combine
    q_rows, rd = q[:, rows].to(device), rows.to(device)
    parts = [nat_.sample_mse_shard_partial(q_rows, k[:, T.shard_keys(s)].to(device), v[:, T.shard_keys(s)].to(device), rd, prof, s, S) for s in sh]
    stated = nat_.sample_mse_from_parts(parts, R, T.BF16, False)
    res["mse"] = mse.cpu()
    res["bits"] = bool(torch.equal(mse.view(torch.int32), stated.view(torch.int32)))
    res["best"] = best.cpu()
    res["best_stated"] = torch.argmin(stated.to(T.BF16), dim=0).cpu()
    # float64: the rank's rows under the band mask at each head's coordinates (token-major where best != 0) over all keys
    em = O.band_mask(S, **mp_)
    idx = torch.arange(S)
    refs = []
    for h in range(T.H):
        c = torch.where(idx < T.V, (idx % T.P_) * T.F_ + idx // T.P_, idx) if int(res["best"][h]) else idx
        refs.append(masked_attention_lse(q[None, h:h + 1, mine], k[None, h:h + 1], v[None, h:h + 1], em[c[mine]][:, c])[0])
    ref = torch.cat(refs, dim=1)[0]
    res["shape"] = o.shape == ql.shape and o.dtype == T.BF16
    res["err"] = ((o.float().cpu() - ref).norm() / ref.float().norm()).item()
    torch.cuda.synchronize()
    ret[rank] = res
    dist.destroy_process_group()


def test_token_sharded_svg1_layer_call_two_ranks_one_gpu():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 40500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    assert [got[r]["shard"] for r in (0, 1)] == [(0, 3, V, 0), (3, 2, V, 32)]              # 3 / 2 frames, the text on the last rank
    assert torch.equal(got[0]["mse"].view(torch.int32), got[1]["mse"].view(torch.int32))   # the same bits on both ranks
    ref32 = oracle("hy", "text", 48)[0]
    torch.testing.assert_close(got[0]["mse"], ref32, rtol=3e-2, atol=1e-6)
    for r in (0, 1):
        t = T_SINGLE[BF16]
        print(f"rank {r}: mse {got[r]['mse'].tolist()} best {got[r]['best'].tolist()} rel_l2 {got[r]['err']:.3e} (limit {t:.1e})")
        assert got[r]["bits"] and got[r]["shape"], got[r]
        assert torch.equal(got[r]["best"], got[r]["best_stated"]) and got[r]["best"].dtype == torch.int64
        assert got[r]["best"][:2].tolist() == [1, 0]                                      # head 0 temporal, head 1 spatial, as constructed
        assert got[r]["err"] <= t, (got[r]["err"], t)
