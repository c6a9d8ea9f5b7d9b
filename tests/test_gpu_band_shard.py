"""Band attention of a frame shard of the rows over a frame shard of the keys on the GPU (include/svg_attn_band_shard.h; csrc/attention.hip:
band_attn_m16_kernel on BandShardLsePolicy / BandShardF32Policy, BandShardOf of csrc/band_policy.h): the whole sequence as both shards against the
device-switch entries bit for bit, every (q shard, k shard) pair of the cases of tests/band_shard_cases.py against float64 with the inputs
inside NaN frames, the parts of a q shard over the k shards merged against the float64 statement over all keys and against the single
switch call, a launch of mixed head kinds against two launches of one kind, strided views, svg.distributed.token_sharded_svg1_attention on
two ranks sharing the GPU, and the poison rows of the two entries and the wrapper.

Geometries (tests/band_shard_cases.py): hy — P 80, F 7, prompt 37, S 624, band 128, shards of 3 / 2 / 2 frames with the text and padding on
the last; wan — S 560, band 129, full columns [0, 80); p75 — a frame of 75 rows, shards of 2 / 1 / 1 frames (Fl = 1); cog — 24 text rows in
front (vid0 > 0); long — P 400, F 6, S 2464, two shards of five q-tiles and 19 / 20 key tiles each (the small shards above are one
q-tile: this one has several per row region, tiles on the fast path and the row cursor's cheap step across frame wraps).  They hold: a shard of one frame and, in section 1, of all frames; a q shard whose rows in logical order see no key of
a k shard (wan, first against last); k shards that end inside a key tile (160, 224, 240 and 75, 107, 150 rows).  Bounds: those of
tests/sparse_lse_cases.py and check_attn, as the window tests use them; no new number.

ref: the head placement of svg/models/hyvideo/placement.py:156-184; BlockSparseAttentionWrapper.run(..., return_lse=True) + merge_state,
svg/kernels/ops/attention_ops.py:178-188."""
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

import band_shard_cases as BC
from poisoned import assert_fully_written, poisoned, unwritten
from sparse_lse_cases import DTYPES, T_SINGLE, check_lse, merged_limit, rel_l2
from test_gpu_kernels import check_attn, dev
from test_gpu_poison import DoNothingLibrary

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
H, D = BC.H, BC.D
MERGE_CASES = ["hy", "wan", "p75", "long"]        # (cog: the 24 rows in front of the video belong to no shard, so its parts do not cover the keys)


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def mask_of(nat, name):
    return nat.BandMask(**BC.CASES[name]["mask"])


def flags_of(flags=BC.FLAGS):
    return torch.tensor(flags, dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def device_shard(name, dtype, shard):
    return tuple(dev(x) for x in BC.shard_inputs(name, dtype, shard))


def run_pair(nat, name, dtype, qs, ks, flags=BC.FLAGS, **kw):
    S, vid0, F, P = BC.geometry(name)
    q = device_shard(name, dtype, qs)[0]
    _, k, v = device_shard(name, dtype, ks)
    return nat.band_shard_attention(q, k, v, mask_of(nat, name), S, (vid0, F, P), qs, ks, flags=flags_of(flags), **kw)


def _f32_matches(o32, lse32, o, lse):
    """what the header says of the _f32 form: o32 rounded to nearest even is o, lse is bit-identical"""
    assert o32.dtype == torch.float32 and o32.is_contiguous() and o32.shape == o.shape
    assert torch.equal(o32.to(o.dtype), o) and torch.equal(lse32, lse)


def framed(x, pad=80):
    """x inside a larger buffer full of NaN: a view with stride(-1) == 1 that the wrapper reads in place"""
    big = torch.full(x.shape[:-2] + (x.shape[-2] + 2 * pad, x.shape[-1]), float("nan"), dtype=x.dtype, device=x.device)
    view = big[..., pad:pad + x.shape[-2], :]
    view.copy_(x)
    assert not view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def switch_result(nat, name, dtype, f32):
    """the single call on the whole sequence: svg_band_attention_switch_lse[_f32] with the same flags (flag 0: the sparse mask)"""
    S, vid0, F, P = BC.geometry(name)
    q, k, v = (dev(x) for x in BC.inputs(name, dtype))
    dense = nat.BandMask(S, S + 1, 0, 0, 0, 0)
    return nat.band_attention_switch(q, k, v, mask_of(nat, name), dense, torch.zeros(1, dtype=torch.int32, device="cuda"),
                                     head_perm_flag=flags_of(), vid0=vid0, num_frame=F, frame_size=P, return_lse=True,
                                     out_dtype=torch.float32 if f32 else None)


# ---------------------------------------------------------------------------------------------------------
# 1. the whole sequence as both shards (f0 = 0, Fl = F, the full tail): the bits of the device-switch entries under the same flags
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MERGE_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_sequence_is_the_switch_entry_bit_for_bit(nat, dtype, name):
    w = BC.whole(name)
    for flags in (BC.FLAGS, (1, 1, 1, 1), (0, 0, 0, 0)):
        S, vid0, F, P = BC.geometry(name)
        q, k, v = (dev(x) for x in BC.inputs(name, dtype))
        dense, zero = nat.BandMask(S, S + 1, 0, 0, 0, 0), torch.zeros(1, dtype=torch.int32, device="cuda")
        kw = dict(head_perm_flag=flags_of(flags), vid0=vid0, num_frame=F, frame_size=P, return_lse=True)
        o_s, lse_s = nat.band_attention_switch(q, k, v, mask_of(nat, name), dense, zero, **kw)
        o, lse = run_pair(nat, name, dtype, w, w, flags)
        assert torch.equal(o, o_s) and torch.equal(lse, lse_s), (name, flags)
        o32_s, lse32_s = nat.band_attention_switch(q, k, v, mask_of(nat, name), dense, zero, out_dtype=torch.float32, **kw)
        o32, lse32 = run_pair(nat, name, dtype, w, w, flags, out_dtype=torch.float32)
        assert torch.equal(o32, o32_s) and torch.equal(lse32, lse32_s), (name, flags)
    # flags = None: every head in logical order
    o_n, lse_n = nat.band_shard_attention(q, k, v, mask_of(nat, name), S, (vid0, F, P), w, w)
    assert torch.equal(o_n, o) and torch.equal(lse_n, lse)


# ---------------------------------------------------------------------------------------------------------
# 2. every (q shard, k shard) pair against float64, the inputs inside NaN frames; 4. the strided layout is the contiguous one bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_pair_matches_float64(nat, dtype, name):
    S, vid0, F, P = BC.geometry(name)
    bm = mask_of(nat, name)
    unseen = {}
    for iq, qs in enumerate(BC.shards(name)):
        for ik, ks in enumerate(BC.shards(name)):
            q = device_shard(name, dtype, qs)[0]
            _, k, v = device_shard(name, dtype, ks)
            o, lse = nat.band_shard_attention(framed(q), framed(k), framed(v), bm, S, (vid0, F, P), qs, ks, flags=flags_of())
            o_ref, lse_ref = BC.pair_reference(name, dtype, qs, ks)
            n = q.shape[-2]
            assert o.dtype == dtype and o.shape == (1, H, n, D) and o.is_contiguous()
            assert lse.dtype == torch.float32 and lse.shape == (1, H, n) and lse.is_contiguous()
            assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()      # nothing outside the shards was read
            check_lse(lse, lse_ref, dtype, f"{name} q shard {qs} k shard {ks}")
            seen = torch.isfinite(lse_ref)
            unseen[iq, ik] = [int((~seen[0, h]).sum()) for h in range(H)]
            oc = o.float().cpu()
            assert torch.equal(oc[~seen], torch.zeros_like(oc[~seen]))                  # rows that see no key of the shard: exact zeros
            if seen.any():
                check_attn(oc[seen], o_ref[seen].float(), dtype)
            o32, lse32 = nat.band_shard_attention(framed(q), framed(k), framed(v), bm, S, (vid0, F, P), qs, ks, flags=flags_of(),
                                                  out_dtype=torch.float32)
            _f32_matches(o32, lse32, o, lse)
            # contiguous tensors: the same bits
            o_c, lse_c = run_pair(nat, name, dtype, qs, ks)
            assert torch.equal(o_c, o) and torch.equal(lse_c, lse)
            _f32_matches(*run_pair(nat, name, dtype, qs, ks, out_dtype=torch.float32), o, lse)
    if name == "wan":   # the first shard against the last: no key for the heads in logical order, every row served on the token-major heads
        assert unseen[0, 2] == [240, 0, 240, 0] and unseen[2, 0] == [0, 0, 0, 0]


@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_on_views_of_a_fused_projection(nat, dtype):
    name = "hy"
    S, vid0, F, P = BC.geometry(name)
    bm = mask_of(nat, name)
    qs, ks = BC.shards(name)[1], BC.shards(name)[2]
    (q, _, _), (_, k, v) = BC.shard_inputs(name, dtype, qs), BC.shard_inputs(name, dtype, ks)
    nq, nk = q.shape[-2], k.shape[-2]
    qp = dev(q.transpose(1, 2).reshape(1, nq, H * D))
    kvp = dev(torch.cat([x.transpose(1, 2).reshape(1, nk, H * D) for x in (k, v)], dim=2))
    qv = qp.unflatten(2, (H, D)).transpose(1, 2)
    kv_ = kvp[:, :, :H * D].unflatten(2, (H, D)).transpose(1, 2)
    vv = kvp[:, :, H * D:].unflatten(2, (H, D)).transpose(1, 2)
    assert not qv.is_contiguous() and not kv_.is_contiguous() and torch.equal(kv_.cpu(), k)
    o_c, lse_c = run_pair(nat, name, dtype, qs, ks)
    out = nat.token_major_empty(qv)
    out.fill_(float("nan"))
    o, lse = nat.band_shard_attention(qv, kv_, vv, bm, S, (vid0, F, P), qs, ks, flags=flags_of(), out=out)
    assert o is out and out.transpose(1, 2).is_contiguous() and not out.is_contiguous()
    assert torch.equal(o, o_c) and torch.equal(lse, lse_c) and lse.is_contiguous()
    _f32_matches(*nat.band_shard_attention(qv, kv_, vv, bm, S, (vid0, F, P), qs, ks, flags=flags_of(), out_dtype=torch.float32), o_c, lse_c)


# ---------------------------------------------------------------------------------------------------------
# 3. the parts of a q shard over all k shards, merged: against float64 over ALL keys and against the single switch call
#    16-bit parts: merged_limit (one call's tolerance and one more output rounding, in quadrature); fp32 parts: T_SINGLE
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MERGE_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_merged_shards_equal_the_whole(nat, dtype, name):
    o_sw, lse_sw = (x.cpu() for x in switch_result(nat, name, dtype, False))
    for qs in BC.shards(name):
        rows = BC.shard_rows(name, qs)
        ref, lse_ref = BC.rows_reference(name, dtype, qs)
        parts = [run_pair(nat, name, dtype, qs, ks) for ks in BC.shards(name)]
        o, lse = nat.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
        limit, r = merged_limit(ref, dtype)
        e16 = rel_l2(o.float().cpu(), ref)
        parts32 = [run_pair(nat, name, dtype, qs, ks, out_dtype=torch.float32) for ks in BC.shards(name)]
        o_f, lse_f = nat.merge_attention_states([p[0] for p in parts32], [p[1] for p in parts32], return_lse=True, out_dtype=dtype)
        e32 = rel_l2(o_f.float().cpu(), ref)
        sw = o_sw[:, :, rows].float()
        d16, d32 = rel_l2(o.float().cpu(), sw), rel_l2(o_f.float().cpu(), sw)
        print(f"{name} {dtype} q shard {qs}: merged rel_l2 16-bit parts {e16:.3e} (limit {limit:.3e}, one rounding {r:.3e}), fp32 parts "
              f"{e32:.3e} (limit {T_SINGLE[dtype]:.1e}); against the switch call {d16:.3e} / {d32:.3e}")
        assert e16 <= limit, (e16, limit)
        assert e32 <= T_SINGLE[dtype], (e32, T_SINGLE[dtype])
        check_attn(o_f, ref.float(), dtype)
        check_lse(lse, lse_ref, dtype, f"merged {name} q shard {qs}", factor=2.0)
        check_lse(lse_f, lse_ref, dtype, f"merged fp32 {name} q shard {qs}", factor=2.0)
        # ... and the single switch call on the whole sequence, within the same limits
        assert d16 <= limit and d32 <= T_SINGLE[dtype], (d16, d32)
        check_lse(lse_f, lse_sw[:, :, rows].double(), dtype, f"merged fp32 {name} against the switch call", factor=2.0)


@pytest.mark.parametrize("name", ["hy", "wan"])
def test_mixed_kinds_are_the_two_single_kind_launches(nat, name):
    dtype = torch.bfloat16
    for qs in BC.shards(name):
        for ks in BC.shards(name):
            for kw in ({}, dict(out_dtype=torch.float32)):
                o, lse = run_pair(nat, name, dtype, qs, ks, **kw)
                one = {f: run_pair(nat, name, dtype, qs, ks, (f,) * H, **kw) for f in (0, 1)}
                for h in range(H):
                    o1, lse1 = one[BC.FLAGS[h]]
                    assert torch.equal(o[:, h], o1[:, h]) and torch.equal(lse[:, h], lse1[:, h]), (name, qs, ks, h)


# ---------------------------------------------------------------------------------------------------------
# 5. token_sharded_svg1_attention: two ranks on one GPU over gloo, a fresh child process per rank
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT), str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import band_shard_cases as BC_
    from svg import _native as nat_
    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    from svg import distributed as sd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    dtype, name = torch.bfloat16, "hy"
    geo = BC_.geometry(name)
    S, vid0, F, P = geo
    mask = nat_.BandMask(**BC_.CASES[name]["mask"])
    flags = torch.tensor(BC_.FLAGS, dtype=torch.int64, device=device)
    sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
    ql, kl, vl = (x.to(device) for x in BC_.shard_inputs(name, dtype, sh[rank]))
    res = {}
    o = sd.token_sharded_svg1_attention(ql, kl, vl, mask, flags, geo)
    # the single-process statement of the same calls: the rank's rows over each shard the plan keeps, merged in shard order
    plan = sd.band_shard_exchange_plan(mask, geo, world)
    parts = []
    for s in range(world):
        if plan[rank][s]:
            _, ks_, vs_ = (x.to(device) for x in BC_.shard_inputs(name, dtype, sh[s]))
            parts.append(nat_.band_shard_attention(ql, ks_, vs_, mask, S, (vid0, F, P), sh[rank], sh[s], out_dtype=torch.float32, flags=flags))
    stated = nat_.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], out_dtype=dtype)
    res["bits"] = bool(torch.equal(o, stated)) and o.shape == ql.shape and o.dtype == dtype
    o16 = sd.token_sharded_svg1_attention(ql, kl, vl, mask, flags, geo, fp32_parts=False)
    res["shape16"] = o16.shape == ql.shape and o16.dtype == dtype
    ref = BC_.rows_reference(name, dtype, sh[rank])[0]
    ref_n = ref.float().norm().clamp(min=1e-20)
    res["err"] = ((o.float().cpu() - ref).norm() / ref_n).item()
    res["err16"] = ((o16.float().cpu() - ref).norm() / ref_n).item()
    res["r"] = ((ref.to(dtype).float() - ref).norm() / ref_n).item()
    res["shard"], res["parts"] = sh[rank], len(parts)
    torch.cuda.synchronize()
    ret[rank] = res
    dist.destroy_process_group()


def test_token_sharded_svg1_attention_two_ranks_one_gpu():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 48500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    assert [got[r]["shard"] for r in (0, 1)] == [(0, 4, 560, 0), (4, 3, 560, 64)]       # 4 / 3 frames, the text and padding on the last rank
    for r in (0, 1):
        t = T_SINGLE[torch.bfloat16]
        limit16 = (t ** 2 + got[r]["r"] ** 2) ** 0.5                                     # merged_limit
        print(f"rank {r}: rel_l2 fp32 parts {got[r]['err']:.3e} (limit {t:.1e}), 16-bit parts {got[r]['err16']:.3e} (limit {limit16:.3e})")
        assert got[r]["bits"] and got[r]["shape16"] and got[r]["parts"] == 2, got[r]
        assert got[r]["err"] <= t, (got[r]["err"], t)
        assert got[r]["err16"] <= limit16, (got[r]["err16"], limit16)


# ---------------------------------------------------------------------------------------------------------
# 6. poison rows: the wrapper's two forms and the two entries called raw, at a pair that holds rows without a key (stored: zeros, -inf)
#    and a pair whose k shard ends inside a key tile.  The do-nothing library of tests/test_gpu_poison.py: every output must then still
#    hold the poison, so the outputs really come from the poisoned callables; on the real library every word is written.
# ---------------------------------------------------------------------------------------------------------
POISON_PAIRS = [("wan", 0, 2), ("hy", 1, 2), ("p75", 1, 0)]


def _wrapper_outs(nat, name, iq, ik, f32):
    got = run_pair(nat, name, torch.bfloat16, BC.shards(name)[iq], BC.shards(name)[ik], **(dict(out_dtype=torch.float32) if f32 else {}))
    return {"o32" if f32 else "o": got[0], "lse": got[1]}


def _raw_outs(nat, name, iq, ik, f32):
    S, vid0, F, P = BC.geometry(name)
    qs, ks = BC.shards(name)[iq], BC.shards(name)[ik]
    q = device_shard(name, torch.bfloat16, qs)[0]
    _, k, v = device_shard(name, torch.bfloat16, ks)
    n = q.shape[-2]
    o = poisoned(1, H, n, D, dtype=torch.float32 if f32 else torch.bfloat16)
    lse = poisoned(1, H, n, dtype=torch.float32)
    flags = flags_of()
    bm, pd, a, b = mask_of(nat, name), nat.PermDesc(flags.data_ptr(), vid0, F, P), nat.BandShard(*qs), nat.BandShard(*ks)
    fn = getattr(nat.load(), "svg_band_shard_attention_lse_f32" if f32 else "svg_band_shard_attention_lse")
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), H, S, D, 0, 1.0 / D ** 0.5, C.byref(bm), C.byref(pd),
            C.byref(a), C.byref(b), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    return {"o32" if f32 else "o": o, "lse": lse}


@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
@pytest.mark.parametrize("how", [_wrapper_outs, _raw_outs], ids=["wrapper", "entry"])
@pytest.mark.parametrize("name,iq,ik", POISON_PAIRS, ids=[f"{n}/{a}-{b}" for n, a, b in POISON_PAIRS])
def test_real_library_writes_every_word(nat, name, iq, ik, how, f32):
    assert nat.allocations_poisoned()
    outs = how(nat, name, iq, ik, f32)
    torch.cuda.synchronize()
    for what, t in outs.items():
        assert_fully_written(t, f"{name} {iq}-{ik}: {what}")
    o_ref, lse_ref = BC.pair_reference(name, torch.bfloat16, BC.shards(name)[iq], BC.shards(name)[ik])
    check_lse(outs["lse"], lse_ref, torch.bfloat16, f"{name} {iq}-{ik}")
    seen = torch.isfinite(lse_ref)
    oc = outs["o32" if f32 else "o"].float().cpu()
    assert torch.equal(oc[~seen], torch.zeros_like(oc[~seen]))
    check_attn(oc[seen], o_ref[seen].float(), torch.bfloat16)
    if (name, iq, ik) == ("wan", 0, 2):
        assert int((~seen).sum()) == 2 * 240          # the rows without a key are there, and they were stored


@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
def test_do_nothing_library_is_caught(nat, monkeypatch, f32):
    lib = DoNothingLibrary()
    monkeypatch.setattr(nat, "load", lambda strict=True: lib)
    outs = _wrapper_outs(nat, "hy", 1, 2, f32)
    torch.cuda.synchronize()
    assert lib.calls == ["svg_band_shard_attention_lse_f32" if f32 else "svg_band_shard_attention_lse"]
    for what, t in outs.items():
        with pytest.raises(AssertionError, match="still hold the poison pattern"):
            assert_fully_written(t, what)
        assert bool(unwritten(t).all()), f"{what} was partly written although the library did nothing"


def test_the_wrapper_allocates_through_the_switch(nat):
    """tests/test_gpu_poison.py finds the allocating wrappers among the `def`s of svg._native and their rows in its own file; this wrapper
    is bound by assignment and its rows are here: it is the function that allocates through the switch, and this file calls it"""
    import ast

    assert nat.band_shard_attention is nat._band_shard_attention
    defs = {n.name: n for n in ast.parse(inspect.getsource(nat)).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    calls = {name: {c.func.id for c in ast.walk(n) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)} for name, n in defs.items()}
    allocating = {"empty", "empty_like"}          # (the closure tests/test_gpu_poison.py test_table_covers_the_wrappers computes)
    while True:
        more = {name for name, cs in calls.items() if cs & allocating} - allocating
        if not more:
            break
        allocating |= more
    # (lse itself, o through the layout plan, which allocates through the switch)
    assert "_layout_plan" in allocating and {"empty", "_layout_plan"} <= calls["_band_shard_attention"]
    assert "nat.band_shard_attention(" in inspect.getsource(sys.modules[__name__])
