"""Band attention over a row window and a key window of the mask on the GPU (include/svg_attn_band_window.h; csrc/attention.hip:
band_attn_m16_kernel on BandWindowLsePolicy / BandWindowF32Policy, BandWindowOf of csrc/band_policy.h): every (row window, key window) pair of the
four band models against float64, the whole-sequence window against the sibling entries bit for bit, windows that sit inside larger
buffers full of NaN, strided views, the protocol the form exists for — the parts of a row window over the key windows merged, against
the float64 statement over all keys — a replayed q-tile inside a key window, and svg.distributed.token_sharded_band_attention on two
ranks sharing the GPU.

Inputs, references and bounds are those of tests/sparse_lse_cases.py (the geometry of band_case: S = 790 / 750, 3 heads, head_dim 128) and
tests/band_replay_cases.py; no new number.  Key cuts at 256 and 640 (key windows start on key tiles), and key windows that end off the
tile grid in front of S, (0, 100) and (256, 700); row cuts at 256 and 640 and, off the tiles, at 300 and 601.
tests/test_band_window_cpu.py shows the float64 identity of section 5 on the CPU.

ref: BlockSparseAttentionWrapper.run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188."""
import ctypes as C
import functools
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import band_replay_cases as RC
import sparse_lse_cases as SC
from sparse_lse_cases import DTYPES, T_SINGLE, check_lse, merged_limit, rel_l2
from test_gpu_kernels import check_attn, dev

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
NINF = float("-inf")
H, D = SC.BAND_H, SC.D
ROW_CUTS = [[0, 256, 640], [0, 300, 601]]
KEY_CUTS = [0, 256, 640]
# key windows that END off the 64-key tile grid and in front of S: the partial last tile, the redirect of rows behind the window, the cheap
# step of the row cursor and fk_hi are bounded by the window's end there, not by S (100: inside the second tile; 700: 60 keys into tile 10)
KEY_ENDS_OFF_THE_GRID = [(0, 100), (256, 700)]


def windows(cuts, S):
    return list(zip(cuts, cuts[1:] + [S]))


def row_windows(S):
    return [w for cuts in ROW_CUTS for w in windows(cuts, S)]


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


@functools.lru_cache(maxsize=None)
def device_inputs(model, dtype):
    return tuple(dev(x) for x in SC.band_inputs(model, dtype))


@functools.lru_cache(maxsize=None)
def window_reference(model, dtype, rows, keys):
    """float64 (o, lse) of the rows `rows` over the keys `keys` under the model's element mask, sliced"""
    q, k, v = SC.band_inputs(model, dtype)
    em = SC.band_case(model)[2]
    (a, b), (c, d) = rows, keys
    return SC.masked_attention_lse(q[:, :, a:b], k[:, :, c:d], v[:, :, c:d], em[a:b, c:d])


def run_window(nat, model, dtype, rows, keys, **kw):
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    (a, b), (c, d) = rows, keys
    return nat.band_window_attention(q[:, :, a:b].contiguous(), k[:, :, c:d].contiguous(), v[:, :, c:d].contiguous(), nat.BandMask(**prm), S, a,
                                     c, **kw)


def _f32_matches(o32, lse32, o, lse):
    """what the header says of the _f32 form: o32 rounded to nearest even is o, lse is bit-identical"""
    assert o32.dtype == torch.float32 and o32.is_contiguous() and o32.shape == o.shape
    assert torch.equal(o32.to(o.dtype), o) and torch.equal(lse32, lse)


# ---------------------------------------------------------------------------------------------------------
# 1. each window against float64
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", SC.BAND_MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_each_window_matches_float64(nat, dtype, model):
    S = SC.band_case(model)[0]
    unseen = {}
    for rows in row_windows(S):
        for keys in windows(KEY_CUTS, S) + KEY_ENDS_OFF_THE_GRID:
            o, lse = run_window(nat, model, dtype, rows, keys)
            o_ref, lse_ref = window_reference(model, dtype, rows, keys)
            n = rows[1] - rows[0]
            assert o.dtype == dtype and o.shape == (1, H, n, D)
            assert lse.dtype == torch.float32 and lse.shape == (1, H, n) and lse.is_contiguous()
            check_lse(lse, lse_ref, dtype, f"{model} rows {rows} keys {keys}")
            seen = torch.isfinite(lse_ref)
            unseen[rows, keys] = int((~seen).sum())
            oc = o.float().cpu()
            assert torch.equal(oc[~seen], torch.zeros_like(oc[~seen]))          # rows that see no key of the window: exact zeros
            if seen.any():
                check_attn(oc[seen], o_ref[seen].float(), dtype)
            o32, lse32 = run_window(nat, model, dtype, rows, keys, out_dtype=torch.float32)
            _f32_matches(o32, lse32, o, lse)
            assert torch.equal(o32.cpu()[~seen], torch.zeros_like(o32.cpu()[~seen]))
    if model == "wan":   # band 385: the rows in front of 256 see no key from 640 on — a launch of rows without keys, and a mixed one
        assert unseen[(640, S), (256, 700)] == 0 and unseen[(0, 256), (0, 100)] == 0
        assert unseen[(0, 256), (640, S)] == H * 256
        assert unseen[(0, 300), (640, S)] == H * 256
        assert unseen[(256, 640), (640, S)] == 0


def test_empty_windows_are_answered_without_a_launch(nat):
    S, prm, _, _ = SC.band_case("hy")
    q, k, v = device_inputs("hy", torch.bfloat16)
    bm = nat.BandMask(**prm)
    o, lse = nat.band_window_attention(q[:, :, 300:300], k[:, :, :256], v[:, :, :256], bm, S, 300, 0)
    assert o.shape == (1, H, 0, D) and lse.shape == (1, H, 0)
    o, lse = nat.band_window_attention(q[:, :, :300], k[:, :, 256:256], v[:, :, 256:256], bm, S, 0, 256)
    assert o.dtype == torch.bfloat16 and not o.any() and (lse == NINF).all() and lse.shape == (1, H, 300)
    o32, lse = nat.band_window_attention(q[:, :, :300], k[:, :, 256:256], v[:, :, 256:256], bm, S, 0, 256, out_dtype=torch.float32)
    assert o32.dtype == torch.float32 and not o32.any() and (lse == NINF).all()


# ---------------------------------------------------------------------------------------------------------
# 2. the window that is the whole sequence: the siblings' bits
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", SC.BAND_MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_sequence_window_is_the_sibling_bit_for_bit(nat, dtype, model):
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    bm = nat.BandMask(**prm)
    o_s, lse_s = nat.band_attention(q, k, v, bm, return_lse=True)
    o, lse = nat.band_window_attention(q, k, v, bm, S, 0, 0)
    assert torch.equal(o, o_s) and torch.equal(lse, lse_s)
    o32_s, lse32_s = nat.band_attention(q, k, v, bm, return_lse=True, out_dtype=torch.float32)
    o32, lse32 = nat.band_window_attention(q, k, v, bm, S, 0, 0, out_dtype=torch.float32)
    assert torch.equal(o32, o32_s) and torch.equal(lse32, lse32_s)


# ---------------------------------------------------------------------------------------------------------
# 3. the window reads only its buffers and writes only its outputs
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_window_reads_only_its_buffers(nat, dtype, f32):
    model, pad = "hy", 96
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    bm = nat.BandMask(**prm)
    lib = nat.load()
    for rows, keys in (((300, 601), (256, 640)), ((601, S), (640, S)), ((0, 300), (0, 256)), ((300, 601), (256, 700)), ((0, 300), (0, 100)),
                       ((601, S), (256, 700))):
        (a, b), (c, d) = rows, keys
        Sq, Sk = b - a, d - c
        tight = nat.band_window_attention(q[:, :, a:b].contiguous(), k[:, :, c:d].contiguous(), v[:, :, c:d].contiguous(), bm, S, a, c,
                                          out_dtype=torch.float32 if f32 else None)

        def framed(x, n, fill, dt=None):
            big = torch.full((1, H, n + 2 * pad, x.shape[-1]), fill, dtype=dt or x.dtype, device="cuda")
            return big, big[:, :, pad:pad + n]

        qbig, qv = framed(q, Sq, float("nan"))
        kbig, kv_ = framed(k, Sk, float("nan"))
        vbig, vv = framed(v, Sk, float("nan"))
        qv.copy_(q[:, :, a:b]), kv_.copy_(k[:, :, c:d]), vv.copy_(v[:, :, c:d])
        SENT = 7.5
        obig, ov = framed(q, Sq, SENT)
        lse_big = torch.full((H * Sq + 2 * pad,), SENT, dtype=torch.float32, device="cuda")
        o32_big = torch.full((H * Sq * D + 2 * pad,), SENT, dtype=torch.float32, device="cuda")
        lse_v, o32_v = lse_big[pad:pad + H * Sq], o32_big[pad:pad + H * Sq * D]
        lay = nat.attn_layout(qv, kv_, vv, ov)
        args = (H, S, a, Sq, c, Sk, D, nat._dtype_code(q), 1.0 / D ** 0.5, C.byref(bm), C.byref(lay), torch.cuda.current_stream().cuda_stream)
        if f32:
            rc = lib.svg_band_window_attention_lse_f32(qv.data_ptr(), kv_.data_ptr(), vv.data_ptr(), o32_v.data_ptr(), lse_v.data_ptr(), *args)
        else:
            rc = lib.svg_band_window_attention_lse(qv.data_ptr(), kv_.data_ptr(), vv.data_ptr(), ov.data_ptr(), lse_v.data_ptr(), *args)
        assert rc == 0
        torch.cuda.synchronize()
        got_o = o32_v.view(1, H, Sq, D) if f32 else ov
        assert torch.isfinite(got_o.float()).all()
        assert torch.equal(got_o, tight[0]) and torch.equal(lse_v.view(1, H, Sq), tight[1])
        # the sentinels: around lse and o32, around the rows of o (and all of o where the fp32 form writes none)
        for big, n in ((lse_big, H * Sq), (o32_big, H * Sq * D)):
            assert (big[:pad] == SENT).all() and (big[pad + n:] == SENT).all()
        assert (obig[:, :, :pad] == SENT).all() and (obig[:, :, pad + Sq:] == SENT).all()
        if f32:
            assert (obig == SENT).all()
        else:
            assert (o32_big == SENT).all()
        assert torch.isnan(qbig[:, :, :pad].float()).all() and torch.isnan(kbig[:, :, pad + Sk:].float()).all()


# ---------------------------------------------------------------------------------------------------------
# 4. strided views: a slice of a fused QKV projection, a token-major o
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_window_on_views_of_a_fused_projection(nat, dtype):
    model = "hy"
    S, prm, _, _ = SC.band_case(model)
    q, k, v = SC.band_inputs(model, dtype)
    bm = nat.BandMask(**prm)
    qkv = dev(torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2))
    for rows, keys in (((300, 601), (256, 640)), ((640, S), (0, 256))):
        (a, b), (c, d) = rows, keys
        qv = qkv[:, a:b, 0:H * D].unflatten(2, (H, D)).transpose(1, 2)
        kv_ = qkv[:, c:d, H * D:2 * H * D].unflatten(2, (H, D)).transpose(1, 2)
        vv = qkv[:, c:d, 2 * H * D:].unflatten(2, (H, D)).transpose(1, 2)
        assert not qv.is_contiguous() and torch.equal(qv.cpu(), q[:, :, a:b]) and torch.equal(kv_.cpu(), k[:, :, c:d])
        o_c, lse_c = run_window(nat, model, dtype, rows, keys)
        out = nat.token_major_empty(qv)
        out.fill_(float("nan"))
        o, lse = nat.band_window_attention(qv, kv_, vv, bm, S, a, c, out=out)
        assert o is out and out.transpose(1, 2).is_contiguous() and not out.is_contiguous()
        assert torch.equal(o, o_c) and torch.equal(lse, lse_c) and lse.is_contiguous()
        o2, lse2 = nat.band_window_attention(qv, kv_, vv, bm, S, a, c)
        assert o2.is_contiguous() and torch.equal(o2, o_c) and torch.equal(lse2, lse_c)
        _f32_matches(*nat.band_window_attention(qv, kv_, vv, bm, S, a, c, out_dtype=torch.float32), o_c, lse_c)


# ---------------------------------------------------------------------------------------------------------
# 5. the point: the parts of a row window over the key windows, merged, against the float64 statement over ALL keys
#    16-bit parts: merged_limit (one call's tolerance and one more output rounding, in quadrature); fp32 parts: T_SINGLE
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", SC.BAND_MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_merged_key_windows_equal_the_whole(nat, dtype, model):
    S = SC.band_case(model)[0]
    o_ref, lse_ref = SC.band_reference(model, dtype)
    for rows in row_windows(S):
        a, b = rows
        ref = o_ref[:, :, a:b]
        parts = [run_window(nat, model, dtype, rows, keys) for keys in windows(KEY_CUTS, S)]
        o, lse = nat.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
        limit, r = merged_limit(ref, dtype)
        e16 = rel_l2(o.float().cpu(), ref)
        parts32 = [run_window(nat, model, dtype, rows, keys, out_dtype=torch.float32) for keys in windows(KEY_CUTS, S)]
        o_f, lse_f = nat.merge_attention_states([p[0] for p in parts32], [p[1] for p in parts32], return_lse=True, out_dtype=dtype)
        e32 = rel_l2(o_f.float().cpu(), ref)
        print(f"{model} {dtype} rows {rows}: merged rel_l2 16-bit parts {e16:.3e} (limit {limit:.3e}, one rounding {r:.3e}), "
              f"fp32 parts {e32:.3e} (limit {T_SINGLE[dtype]:.1e})")
        assert e16 <= limit, (e16, limit)
        assert e32 <= T_SINGLE[dtype], (e32, T_SINGLE[dtype])
        check_attn(o_f, ref.float(), dtype)
        check_lse(lse, lse_ref[:, :, a:b], dtype, f"merged {model} rows {rows}", factor=2.0)
        check_lse(lse_f, lse_ref[:, :, a:b], dtype, f"merged fp32 {model} rows {rows}", factor=2.0)


# ---------------------------------------------------------------------------------------------------------
# 6. bf16 under replay: the all-six spike case of tests/band_replay_cases.py in logical order, cut into two key windows
# ---------------------------------------------------------------------------------------------------------
def test_window_under_replay(nat):
    """a q-tile whose validation fails stores neither o nor lse; its replay stores both: the replay counter moves, NaN-filled o comes
    back whole and finite, and o and lse are those of the float64 statement of each window"""
    case = RC.queue_case("all6")
    g = case.geo
    q, k, v = (dev(x) for x in RC.inputs(case))              # logical order: the window entries take no head permutation
    em = RC.bool_mask("band", g)
    bm = nat.BandMask(**g.mask_params("band"))
    cut = 640
    spiked_rows = sorted({s.row for s in case.spikes})
    for c, d in ((0, cut), (cut, g.S)):
        assert any(c <= s.key < d for s in case.spikes)        # each key window holds a spike
        nat.band_replays(reset=True)
        out = torch.full_like(q, float("nan"))
        o, lse = nat.band_window_attention(q, k[:, :, c:d].contiguous(), v[:, :, c:d].contiguous(), bm, g.S, 0, c, out=out)
        n = nat.band_replays(reset=True)
        o32, lse32 = nat.band_window_attention(q, k[:, :, c:d].contiguous(), v[:, :, c:d].contiguous(), bm, g.S, 0, c, out_dtype=torch.float32)
        n32 = nat.band_replays(reset=True)
        print(f"window replay keys [{c}, {d}): replays = {n} (fp32 form {n32})")
        assert n >= 1 and n32 == n
        assert o is out and torch.isfinite(out.float()).all()
        _f32_matches(o32, lse32, out, lse)
        o_ref, lse_ref = SC.masked_attention_lse(*RC.inputs(case)[:1], RC.inputs(case)[1][:, :, c:d], RC.inputs(case)[2][:, :, c:d], em[:, c:d])
        check_lse(lse, lse_ref, case.dtype, f"replay keys [{c}, {d})")
        seen = torch.isfinite(lse_ref)
        check_attn(out.float().cpu()[seen], o_ref[seen].float(), case.dtype)
        rows = [s.row for s in case.spikes if c <= s.key < d]
        assert (lse.cpu()[0, :, rows] > 200).all()            # the +400 spikes (log2 domain: about 277) show in lse of their window
    assert len(spiked_rows) == 6


# ---------------------------------------------------------------------------------------------------------
# 7. token_sharded_band_attention: two ranks on one GPU over gloo
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT), str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import sparse_lse_cases as SC_
    from svg import _native as nat_
    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    from svg import distributed as sd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    dtype, unit = torch.bfloat16, 128
    S, prm, _, _ = SC_.band_case("hy")
    mask = nat_.BandMask(**prm)
    q, k, v = SC_.band_inputs("hy", dtype)
    tr = [sd.token_range(S, r, world, unit) for r in range(world)]
    a, b = tr[rank]
    ql, kl, vl = (x[:, :, a:b].contiguous().to(device) for x in (q, k, v))
    res = {}
    o = sd.token_sharded_band_attention(ql, kl, vl, S, mask, unit=unit)
    # the single-process statement of the same calls: the rank's rows over each shard the plan keeps, merged in shard order
    plan = sd.band_exchange_plan(mask, S, world, unit)
    parts = [nat_.band_window_attention(ql, k[:, :, lo:hi].contiguous().to(device), v[:, :, lo:hi].contiguous().to(device), mask, S, a, lo,
                                        out_dtype=torch.float32) for s, (lo, hi) in enumerate(tr) if plan[rank][s]]
    stated = nat_.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], out_dtype=dtype)
    res["bits"] = bool(torch.equal(o, stated)) and o.shape == ql.shape and o.dtype == dtype
    o16 = sd.token_sharded_band_attention(ql, kl, vl, S, mask, unit=unit, fp32_parts=False)
    res["shape16"] = o16.shape == ql.shape and o16.dtype == dtype
    ref = SC_.band_reference("hy", dtype)[0][:, :, a:b]
    ref_n = ref.float().norm().clamp(min=1e-20)
    res["err"] = ((o.float().cpu() - ref).norm() / ref_n).item()
    res["err16"] = ((o16.float().cpu() - ref).norm() / ref_n).item()
    res["r"] = ((ref.to(dtype).float() - ref).norm() / ref_n).item()
    res["tokens"], res["parts"] = (a, b), len(parts)
    torch.cuda.synchronize()
    ret[rank] = res
    dist.destroy_process_group()


def test_token_sharded_band_attention_two_ranks_one_gpu():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 47500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    assert [got[r]["tokens"] for r in (0, 1)] == [(0, 384), (384, 790)]          # ragged: the tail goes to the last rank
    for r in (0, 1):
        t = T_SINGLE[torch.bfloat16]
        limit16 = (t ** 2 + got[r]["r"] ** 2) ** 0.5                              # merged_limit
        print(f"rank {r}: rel_l2 fp32 parts {got[r]['err']:.3e} (limit {t:.1e}), 16-bit parts {got[r]['err16']:.3e} (limit {limit16:.3e})")
        assert got[r]["bits"] and got[r]["shape16"] and got[r]["parts"] == 2, got[r]
        assert got[r]["err"] <= t, (got[r]["err"], t)
        assert got[r]["err16"] <= limit16, (got[r]["err16"], limit16)
