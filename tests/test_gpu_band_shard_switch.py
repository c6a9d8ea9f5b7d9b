"""The device switch of band attention on frame shards on the GPU (include/svg_attn_band_shard_switch.h; csrc/attention.hip:
band_attn_m16_switch_kernel on BandShardLsePolicy / BandShardF32Policy): for every (q shard, k shard) pair of the cases of
tests/band_shard_cases.py a flag of 0 against the plain shard entry under the sparse mask and the head flags, a flag of 1 against the plain
shard entry under the alternate mask without flags — bit for bit, 16-bit and fp32 forms, bf16 and fp16 — and both against float64; the whole
sequence as both shards against svg_band_attention_switch_lse[_f32]; one set of arguments launched twice with the flag flipped on the
device; rows without a key under one mask and with keys under the other; strided views; the poison rows of the wrapper and the entries;
and two ranks sharing the GPU over gloo: token_sharded_svg1_layer_call with the switch, and the Wan and HunyuanVideo SVG1 processors in
frame-shard mode against the same processors on the whole sequence.

The alternate mask of a case is what the processors pass: the dense mask with the case's real_len (two segments where real_len < S).
Bounds: those of tests/sparse_lse_cases.py and check_attn, as tests/test_gpu_band_shard.py uses them; no new number.

ref: the dense warm-up / sparse branch of svg/models/hyvideo/attention.py:491-524."""
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
import sparse_lse_cases as SC
from oracle import svg_oracle as O
from poisoned import assert_fully_written, poisoned, unwritten
from sparse_lse_cases import DTYPES, T_SINGLE, check_lse
from test_gpu_kernels import check_attn, dev
from test_gpu_poison import DoNothingLibrary

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
H, D = BC.H, BC.D
WHOLE_CASES = ["hy", "wan", "p75", "long"]


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def mask_of(nat, name):
    return nat.BandMask(**BC.CASES[name]["mask"])


def alt_params(name):
    S = BC.CASES[name]["S"]
    return dict(real_len=BC.CASES[name]["mask"]["real_len"], band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)


def alt_of(nat, name):
    return nat.BandMask(**alt_params(name))


def flags_of(flags=BC.FLAGS):
    return torch.tensor(flags, dtype=torch.int64, device="cuda")


def flag_of(value):
    return torch.full((1,), value, dtype=torch.int32, device="cuda")


@functools.lru_cache(maxsize=None)
def device_shard(name, dtype, shard):
    return tuple(dev(x) for x in BC.shard_inputs(name, dtype, shard))


@functools.lru_cache(maxsize=None)
def alt_reference(name, dtype, q_shard, k_shard):
    """float64 (o, lse) of the rows of q_shard over the keys of k_shard under the alternate mask, every head in logical order"""
    em = O.band_mask(BC.CASES[name]["S"], **alt_params(name))
    q, _, _ = BC.shard_inputs(name, dtype, q_shard)
    _, k, v = BC.shard_inputs(name, dtype, k_shard)
    return SC.masked_attention_lse(q, k, v, em[BC.shard_rows(name, q_shard)][:, BC.shard_rows(name, k_shard)])


def operands(name, dtype, qs, ks):
    q = device_shard(name, dtype, qs)[0]
    _, k, v = device_shard(name, dtype, ks)
    return q, k, v


def run_switch(nat, name, dtype, qs, ks, flag, flags=BC.FLAGS, **kw):
    S, vid0, F, P = BC.geometry(name)
    q, k, v = operands(name, dtype, qs, ks)
    return nat.band_shard_attention_switch(q, k, v, mask_of(nat, name), alt_of(nat, name), flag if torch.is_tensor(flag) else flag_of(flag), S,
                                           (vid0, F, P), qs, ks, flags=flags_of(flags), **kw)


def run_plain(nat, name, dtype, qs, ks, alt, flags=BC.FLAGS, **kw):
    """what the header promises: the plain shard entry under mask and the flags, or under alt_mask without flags"""
    S, vid0, F, P = BC.geometry(name)
    q, k, v = operands(name, dtype, qs, ks)
    if alt:
        return nat.band_shard_attention(q, k, v, alt_of(nat, name), S, (vid0, F, P), qs, ks, flags=None, **kw)
    return nat.band_shard_attention(q, k, v, mask_of(nat, name), S, (vid0, F, P), qs, ks, flags=flags_of(flags), **kw)


def same_bits(a, b):
    return all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))


def check_against_float64(o, lse, ref, dtype, what):
    o_ref, lse_ref = ref
    check_lse(lse, lse_ref, dtype, what)
    seen = torch.isfinite(lse_ref)
    oc = o.float().cpu()
    assert torch.equal(oc[~seen], torch.zeros_like(oc[~seen])), what      # rows that see no key of the shard: exact zeros
    if seen.any():
        check_attn(oc[seen], o_ref[seen].float(), dtype)
    return int((~seen).sum())


# ---------------------------------------------------------------------------------------------------------
# 1. every (q shard, k shard) pair: flag 0 / flag 1 are the two plain shard calls bit for bit, both forms; and within the bounds of float64
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BC.CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_pair_is_the_plain_shard_entry_bit_for_bit(nat, dtype, name):
    for qs in BC.shards(name):
        for ks in BC.shards(name):
            for alt in (0, 1):
                what = f"{name} q shard {qs} k shard {ks} flag {alt}"
                got = run_switch(nat, name, dtype, qs, ks, alt)
                assert same_bits(got, run_plain(nat, name, dtype, qs, ks, alt)), what
                got32 = run_switch(nat, name, dtype, qs, ks, alt, out_dtype=torch.float32)
                assert got32[0].dtype == torch.float32 and same_bits(got32, run_plain(nat, name, dtype, qs, ks, alt, out_dtype=torch.float32)), what
                assert torch.equal(got32[0].to(dtype), got[0]) and torch.equal(got32[1], got[1]), what
                ref = alt_reference(name, dtype, qs, ks) if alt else BC.pair_reference(name, dtype, qs, ks)
                check_against_float64(*got, ref, dtype, what)
    # any non-zero flag selects the alternate mask
    qs, ks = BC.shards(name)[0], BC.shards(name)[-1]
    assert same_bits(run_switch(nat, name, dtype, qs, ks, -3), run_plain(nat, name, dtype, qs, ks, 1))


# ---------------------------------------------------------------------------------------------------------
# 2. the whole sequence as both shards: the bits of svg_band_attention_switch_lse[_f32] for either flag value
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", WHOLE_CASES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_sequence_is_the_switch_entry_bit_for_bit(nat, dtype, name):
    w = BC.whole(name)
    S, vid0, F, P = BC.geometry(name)
    q, k, v = (dev(x) for x in BC.inputs(name, dtype))
    for flags in (BC.FLAGS, (1, 1, 1, 1)):
        for alt in (0, 1):
            kw = dict(head_perm_flag=flags_of(flags), vid0=vid0, num_frame=F, frame_size=P, return_lse=True)
            for f32 in (None, torch.float32):
                want = nat.band_attention_switch(q, k, v, mask_of(nat, name), alt_of(nat, name), flag_of(alt), out_dtype=f32, **kw)
                got = nat.band_shard_attention_switch(q, k, v, mask_of(nat, name), alt_of(nat, name), flag_of(alt), S, (vid0, F, P), w, w,
                                                      flags=flags_of(flags), out_dtype=f32)
                assert same_bits(got, want), (name, flags, alt, f32)


# ---------------------------------------------------------------------------------------------------------
# 3. one set of arguments, launched twice, the flag flipped in between by a torch op on the device: the two results, no host read
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
def test_the_flag_is_read_by_the_kernel(nat, f32):
    name, dtype = "hy", torch.bfloat16
    qs, ks = BC.shards(name)[0], BC.shards(name)[1]
    kw = dict(out_dtype=torch.float32) if f32 else {}
    timestep = torch.tensor([0.25], device="cuda")
    flag = (timestep > 0.5).to(torch.int32)                                  # as dense_flag_on_device makes it: 0
    first = run_switch(nat, name, dtype, qs, ks, flag, **kw)
    flag.copy_((timestep + 0.5 > 0.5).to(torch.int32))                       # the same tensor, now 1; nothing came back to the host
    second = run_switch(nat, name, dtype, qs, ks, flag, **kw)
    flag.zero_()
    third = run_switch(nat, name, dtype, qs, ks, flag, **kw)
    assert same_bits(first, run_plain(nat, name, dtype, qs, ks, 0, **kw))
    assert same_bits(second, run_plain(nat, name, dtype, qs, ks, 1, **kw))
    assert same_bits(third, first) and not torch.equal(first[0], second[0])


# ---------------------------------------------------------------------------------------------------------
# 4. rows without a key under one mask, with keys under the other: wan, the first shard's rows against the last shard's keys
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_without_a_key_under_the_mask_and_with_keys_under_alt_mask(nat, dtype):
    name = "wan"
    qs, ks = BC.shards(name)[0], BC.shards(name)[2]
    for kw in ({}, dict(out_dtype=torch.float32)):
        o, lse = run_switch(nat, name, dtype, qs, ks, 0, **kw)
        unseen = check_against_float64(o, lse, BC.pair_reference(name, dtype, qs, ks), dtype, "wan 0-2 flag 0")
        assert unseen == 2 * 240                                            # the two heads in logical order: no key of the last shard
        logical = [h for h in range(H) if not BC.FLAGS[h]]
        assert bool(torch.isinf(lse[0, logical]).all()) and bool((lse[0, logical] < 0).all()) and not bool(o[0, logical].float().any())
        o1, lse1 = run_switch(nat, name, dtype, qs, ks, 1, **kw)
        assert check_against_float64(o1, lse1, alt_reference(name, dtype, qs, ks), dtype, "wan 0-2 flag 1") == 0
        assert bool(torch.isfinite(lse1).all()) and bool(o1[0, logical].float().abs().sum() > 0)
    # ... and the other way round: an alternate mask that gives these rows nothing (band 129 in logical order for every head)
    S, vid0, F, P = BC.geometry(name)
    q, k, v = operands(name, dtype, qs, ks)
    dense = alt_of(nat, name)
    o, lse = nat.band_shard_attention_switch(q, k, v, dense, mask_of(nat, name), flag_of(1), S, (vid0, F, P), qs, ks, flags=flags_of())
    assert bool(torch.isinf(lse).all()) and not bool(o.float().any())
    o, lse = nat.band_shard_attention_switch(q, k, v, dense, mask_of(nat, name), flag_of(0), S, (vid0, F, P), qs, ks, flags=flags_of())
    assert bool(torch.isfinite(lse).all())


# ---------------------------------------------------------------------------------------------------------
# 5. strided input (the projection layout) equals contiguous, bit for bit
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_shards_on_views_of_a_fused_projection(nat, dtype):
    name = "hy"
    S, vid0, F, P = BC.geometry(name)
    qs, ks = BC.shards(name)[1], BC.shards(name)[2]
    (q, _, _), (_, k, v) = BC.shard_inputs(name, dtype, qs), BC.shard_inputs(name, dtype, ks)
    nq, nk = q.shape[-2], k.shape[-2]
    qp = dev(q.transpose(1, 2).reshape(1, nq, H * D))
    kvp = dev(torch.cat([x.transpose(1, 2).reshape(1, nk, H * D) for x in (k, v)], dim=2))
    qv = qp.unflatten(2, (H, D)).transpose(1, 2)
    kv_ = kvp[:, :, :H * D].unflatten(2, (H, D)).transpose(1, 2)
    vv = kvp[:, :, H * D:].unflatten(2, (H, D)).transpose(1, 2)
    assert not qv.is_contiguous() and not kv_.is_contiguous() and torch.equal(kv_.cpu(), k)
    for alt in (0, 1):
        args = (mask_of(nat, name), alt_of(nat, name), flag_of(alt), S, (vid0, F, P), qs, ks)
        want = run_switch(nat, name, dtype, qs, ks, alt)
        out = nat.token_major_empty(qv)
        out.fill_(float("nan"))
        o, lse = nat.band_shard_attention_switch(qv, kv_, vv, *args, flags=flags_of(), out=out)
        assert o is out and out.transpose(1, 2).is_contiguous() and not out.is_contiguous()
        assert same_bits((o, lse), want) and lse.is_contiguous()
        o32, lse32 = nat.band_shard_attention_switch(qv, kv_, vv, *args, flags=flags_of(), out_dtype=torch.float32)
        assert same_bits((o32, lse32), run_switch(nat, name, dtype, qs, ks, alt, out_dtype=torch.float32)) and o32.is_contiguous()


# ---------------------------------------------------------------------------------------------------------
# 6. poison rows: the wrapper's two forms and the two entries called raw, under either flag, at a pair that holds rows without a key
#    (stored: zeros, -inf) and pairs whose k shard ends inside a key tile.  The do-nothing library of tests/test_gpu_poison.py: every
#    output must then still hold the poison; on the real library every word is written.
# ---------------------------------------------------------------------------------------------------------
POISON_PAIRS = [("wan", 0, 2), ("hy", 1, 2), ("p75", 1, 0)]


def _wrapper_outs(nat, name, iq, ik, f32, alt):
    got = run_switch(nat, name, torch.bfloat16, BC.shards(name)[iq], BC.shards(name)[ik], alt, **(dict(out_dtype=torch.float32) if f32 else {}))
    return {"o32" if f32 else "o": got[0], "lse": got[1]}


def _raw_outs(nat, name, iq, ik, f32, alt):
    S, vid0, F, P = BC.geometry(name)
    qs, ks = BC.shards(name)[iq], BC.shards(name)[ik]
    q, k, v = operands(name, torch.bfloat16, qs, ks)
    n = q.shape[-2]
    o = poisoned(1, H, n, D, dtype=torch.float32 if f32 else torch.bfloat16)
    lse = poisoned(1, H, n, dtype=torch.float32)
    flags, flag = flags_of(), flag_of(alt)
    bm, am, pd, a, b = mask_of(nat, name), alt_of(nat, name), nat.PermDesc(flags.data_ptr(), vid0, F, P), nat.BandShard(*qs), nat.BandShard(*ks)
    fn = getattr(nat.load(), "svg_band_shard_attention_switch_lse_f32" if f32 else "svg_band_shard_attention_switch_lse")
    rc = fn(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), H, S, D, 0, 1.0 / D ** 0.5, C.byref(bm), C.byref(pd),
            C.byref(am), flag.data_ptr(), C.byref(a), C.byref(b), None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()                                                # (flag and flags stay alive until the launch is through)
    return {"o32" if f32 else "o": o, "lse": lse}


@pytest.mark.parametrize("alt", [0, 1], ids=["flag0", "flag1"])
@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
@pytest.mark.parametrize("how", [_wrapper_outs, _raw_outs], ids=["wrapper", "entry"])
@pytest.mark.parametrize("name,iq,ik", POISON_PAIRS, ids=[f"{n}/{a}-{b}" for n, a, b in POISON_PAIRS])
def test_real_library_writes_every_word(nat, name, iq, ik, how, f32, alt):
    assert nat.allocations_poisoned()
    outs = how(nat, name, iq, ik, f32, alt)
    torch.cuda.synchronize()
    for what, t in outs.items():
        assert_fully_written(t, f"{name} {iq}-{ik} flag {alt}: {what}")
    qs, ks = BC.shards(name)[iq], BC.shards(name)[ik]
    ref = alt_reference(name, torch.bfloat16, qs, ks) if alt else BC.pair_reference(name, torch.bfloat16, qs, ks)
    unseen = check_against_float64(outs["o32" if f32 else "o"], outs["lse"], ref, torch.bfloat16, f"{name} {iq}-{ik} flag {alt}")
    if (name, iq, ik) == ("wan", 0, 2):
        assert unseen == (0 if alt else 2 * 240)          # the rows without a key are there under the sparse mask, and they were stored


@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
def test_do_nothing_library_is_caught(nat, monkeypatch, f32):
    lib = DoNothingLibrary()
    monkeypatch.setattr(nat, "load", lambda strict=True: lib)
    outs = _wrapper_outs(nat, "hy", 1, 2, f32, 0)
    torch.cuda.synchronize()
    assert lib.calls == ["svg_band_shard_attention_switch_lse_f32" if f32 else "svg_band_shard_attention_switch_lse"]
    for what, t in outs.items():
        with pytest.raises(AssertionError, match="still hold the poison pattern"):
            assert_fully_written(t, what)
        assert bool(unwritten(t).all()), f"{what} was partly written although the library did nothing"


def test_the_wrapper_allocates_through_the_switch(nat):
    """tests/test_gpu_poison.py finds the allocating wrappers among the `def`s of svg._native and their rows in its own file; this wrapper
    is bound by assignment, as band_shard_attention is, and its rows are here: it runs the function that allocates through the switch"""
    import ast

    assert nat.band_shard_attention_switch is nat._band_shard_attention_switch
    fn = ast.parse(inspect.getsource(nat._band_shard_attention_switch))
    assert "_band_shard_attention" in {c.func.id for c in ast.walk(fn) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
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
    assert "nat.band_shard_attention_switch(" in inspect.getsource(sys.modules[__name__])


# ---------------------------------------------------------------------------------------------------------
# 7. two ranks on one GPU over gloo, a fresh child process per rank, one pair per test (mp.spawn ends the pair when either rank fails).
#    q / k that make heads 0 and 2 temporal and heads 1 and 3 spatial, so that the profiler's choice is the same on shards and on the whole
#    sequence for a reason and not by luck.  The layer-call on `long` (6 frames of 400 rows, 64 rows behind them), the Wan processor on
#    `wan`, the HunyuanVideo processor on `hy`.
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def structured_inputs(name):
    """BC.inputs with keys alike at one patch position on heads 0 and 2 (temporal) and alike within a frame on heads 1 and 3 (spatial), as
    tests/test_gpu_profile_shard.py builds them; bf16 [1, H, S, D]"""
    S, vid0, F, P = BC.geometry(name)
    V = F * P
    q, k, v = (x.float().clone() for x in BC.inputs(name, torch.bfloat16))
    g = torch.Generator().manual_seed(17)
    pos, frm = torch.randn(P, D, generator=g), torch.randn(F, D, generator=g)
    for h in range(H):
        add = 3 * (frm.repeat_interleave(P, 0) if h % 2 else pos.repeat(F, 1))
        q[0, h, :V] += add
        k[0, h, :V] += add
    return tuple(x.to(torch.bfloat16) for x in (q, k, v))


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


def _layer_worker(rank, world, port, ret):
    nat_, device = _setup_rank(rank, world, port)
    import band_shard_cases as BC_
    import test_gpu_band_shard_switch as T
    from svg import distributed as sd
    from svg.models.hyvideo.utils import profile_desc

    name, dtype, R = "long", torch.bfloat16, 48
    geo = BC_.geometry(name)
    S, vid0, F, P = geo
    q, k, v = T.structured_inputs(name)
    rows = torch.randint(0, S, (R,), generator=torch.Generator().manual_seed(23))
    prof = profile_desc(S - F * P, F, P)
    mask, dense = nat_.BandMask(**BC_.CASES[name]["mask"]), nat_.BandMask(**T.alt_params(name))
    sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
    mine = BC_.shard_rows(name, sh[rank])
    ql, kl, vl = (x[:, :, mine].to(device) for x in (q, k, v))
    plan = sd.band_shard_exchange_plan(mask, geo, world, "both", dense_mask=dense)
    res = {"shard": sh[rank]}
    for value in (0, 1):
        flag = torch.full((1,), value, dtype=torch.int32, device=device)
        o, best = sd.token_sharded_svg1_layer_call(ql, kl, vl, mask, prof, geo, rows, dense_mask=dense, dense_flag=flag)
        # the single-process statement of the same calls: a partial per shard and the combine, the argmin, the switch call per pair, the merge
        rd = rows.to(device)
        q_rows = q[0][:, rows].to(device)
        parts = [nat_.sample_mse_shard_partial(q_rows, k[0][:, BC_.shard_rows(name, s)].to(device), v[0][:, BC_.shard_rows(name, s)].to(device),
                                               rd, prof, s, S, skip_flag=flag) for s in sh]
        mse = nat_.sample_mse_from_parts(parts, R, dtype, prof.emulate_bf16, skip_flag=flag)
        idx = torch.argmin(mse.to(dtype), dim=0)
        att = []
        for s in range(world):
            if plan[rank][s]:
                ks_, vs_ = (x[:, :, BC_.shard_rows(name, sh[s])].to(device) for x in (k, v))
                att.append(nat_.band_shard_attention_switch(ql, ks_, vs_, mask, dense, flag, S, (vid0, F, P), sh[rank], sh[s],
                                                            out_dtype=torch.float32, flags=idx))
        stated = nat_.merge_attention_states([p[0] for p in att], [p[1] for p in att], out_dtype=dtype)
        torch.cuda.synchronize()
        res[value] = dict(bits=bool(torch.equal(o, stated)) and o.shape == ql.shape and o.dtype == dtype, o=o.cpu(), best=best.cpu(),
                          idx=idx.cpu(), parts=len(att))
    ret[rank] = res
    dist.destroy_process_group()


def test_token_sharded_svg1_layer_call_switch_two_ranks_one_gpu():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 34500 + (os.getpid() % 2000)
    mp.spawn(_layer_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    name, dtype = "long", torch.bfloat16
    S, vid0, F, P = BC.geometry(name)
    assert [got[r]["shard"] for r in (0, 1)] == [(0, 3, 2400, 0), (3, 3, 2400, 64)]      # 3 / 3 frames, the rows behind the video on the last rank
    q, k, v = structured_inputs(name)
    em = {0: BC.element_mask(name), 1: O.band_mask(S, **alt_params(name))}
    idx_all = torch.arange(S)
    for r in (0, 1):
        mine = BC.shard_rows(name, got[r]["shard"])
        for value in (0, 1):
            g = got[r][value]
            assert g["bits"] and g["parts"] == 2, (r, value, g["bits"], g["parts"])
            assert g["best"].dtype == torch.int64 and torch.equal(g["best"], got[0][value]["best"])
            if value:
                assert g["best"].tolist() == [-1] * H                                   # a dense step
            else:
                assert torch.equal(g["best"], g["idx"]) and g["best"].tolist() == [1, 0, 1, 0]   # temporal, spatial, ... as constructed
            refs = []
            for h in range(H):
                tm = bool(g["best"][h] > 0)
                c = BC.mask_coords(name, idx_all, tm)
                refs.append(SC.masked_attention_lse(q[:, h:h + 1, mine], k[:, h:h + 1], v[:, h:h + 1], em[value][c[mine]][:, c])[0])
            ref = torch.cat(refs, dim=1)
            err = SC.rel_l2(g["o"].float(), ref)
            print(f"rank {r} flag {value}: best {g['best'].tolist()} rel_l2 {err:.3e} (limit {T_SINGLE[dtype]:.1e})")
            assert err <= T_SINGLE[dtype], (r, value, err)


def _processor_worker(rank, world, port, ret, model):
    nat_, device = _setup_rank(rank, world, port)
    import band_shard_cases as BC_
    import test_gpu_band_shard_switch as T
    from svg import distributed as sd
    from svg.models import _core
    from svg.models.hyvideo.attention import Hunyuan_SVGAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0

    name = model                                                            # (Wan has no rows behind the video: the case `wan`)
    geo = BC_.geometry(name)
    S, vid0, F, P = geo
    cls = Hunyuan_SVGAttn_Processor2_0 if model == "hy" else WanAttn_SVGAttn_Processor2_0
    cls.context_length, cls.num_frame, cls.frame_size = S - F * P, F, P
    cls.first_layers_fp, cls.first_times_fp = 1, 0.5
    cls.num_sampled_rows, cls.sample_mse_max_row = 32, 10000
    cls.block_mask = nat_.BandMask(**BC_.CASES[name]["mask"])
    if model == "hy":
        cls.prompt_length = BC_.CASES[name]["mask"]["real_len"] - F * P
    q, k, v = (x.to(device) for x in T.structured_inputs(name))
    sh = sd.frame_shard(geo, rank, world).as_tuple()
    mine = BC_.shard_rows(name, sh).to(device)
    # (layer, timestep): a sparse step and a dense warm-up step of the device switch, and a layer below first_layers_fp (dense on the host)
    steps = [("sparse", 1, 0.25), ("dense", 1, 0.75), ("host_dense", 0, 0.25)]
    torch.manual_seed(11)

    def run(qq, kk, vv):
        _core.reseed_switch_generator(11)                                   # the same sampled rows in both modes (frame-shard mode: broadcast)
        out = {}
        for what, layer, t in steps:
            proc = cls(layer)
            ts = torch.tensor([t], device=device)
            args = (qq.clone(), kk.clone(), vv.clone(), ts) + ((layer, None) if model == "hy" else ())
            o = proc.attention_core_logic(*args)
            out[what] = (o, proc.last_best_mask_idx)
        return out

    whole = run(q, k, v)
    sd.enable_frame_shards()
    ql, kl, vl = (x[:, :, mine].contiguous() for x in (q, k, v))
    local = run(ql, kl, vl)
    sd.disable()
    torch.cuda.synchronize()
    res = {"shard": sh}
    for what, _, _ in steps:
        (ow, bw), (ol, bl) = whole[what], local[what]
        want = ow[:, :, mine].float()
        res[what] = dict(shape=ol.shape == ql.shape and ol.dtype == ql.dtype, err=((ol.float() - want).norm() / want.norm()).item(),
                         best_whole=None if bw is None else bw.cpu(), best_local=None if bl is None else bl.cpu())
    ret[rank] = res
    dist.destroy_process_group()


@pytest.mark.parametrize("model", ["wan", "hy"])
def test_processor_in_frame_shard_mode_two_ranks_one_gpu(model):
    """attention_core_logic of the SVG1 processor on this rank's frames (HunyuanVideo: the text on the last rank) against the same
    processor on the whole sequence in the same process: the rank's rows within the bound of fp32 parts merged with one rounding (T_SINGLE,
    as tests/test_gpu_band_shard.py holds merged shards against the single switch call), last_best_mask_idx equal, -1 on the dense step"""
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 32500 + (os.getpid() % 2000) + (1 if model == "hy" else 0)
    mp.spawn(_processor_worker, args=(world, port, ret, model), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    want_shards = [(0, 4, 560, 0), (4, 3, 560, 64 if model == "hy" else 0)]           # 4 / 3 frames
    assert [got[r]["shard"] for r in (0, 1)] == want_shards
    t = T_SINGLE[torch.bfloat16]
    for r in (0, 1):
        for what in ("sparse", "dense", "host_dense"):
            g = got[r][what]
            print(f"{model} rank {r} {what}: rel_l2 against the whole-sequence processor {g['err']:.3e} (limit {t:.1e}), best "
                  f"{None if g['best_local'] is None else g['best_local'].tolist()}")
            assert g["shape"], (r, what)
            assert g["err"] <= t, (r, what, g["err"], t)
        for what in ("sparse", "dense"):
            g = got[r][what]
            assert g["best_local"].shape == (1, H) and g["best_local"].dtype == torch.int64
            assert torch.equal(g["best_local"], g["best_whole"]), (r, what, g["best_local"], g["best_whole"])
        assert got[r]["dense"]["best_local"].tolist() == [[-1] * H]
        assert got[r]["host_dense"]["best_local"] is None                  # (no profiler ran on that layer)
        if model == "wan":
            assert got[r]["sparse"]["best_local"].tolist() == [[1, 0, 1, 0]]    # temporal, spatial, ... as constructed
