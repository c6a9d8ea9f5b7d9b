"""svg_cross_attention_lse and svg_merge_attention_states on the GPU (csrc/attention_cross.hip on CrossLsePolicy, csrc/merge_states.hip):
the row log-sum-exp of the cross-attention family against a float64 reference, with o bit-identical to the entry without it; layouts, key
windows, the exact path of the max-free softmax, the resident loop; the N-way merge against a float64 merge of the same inputs; partials
over key shards merged against the oracle over all keys; and svg.distributed.token_sharded_dense_attention on two ranks sharing the GPU.
The shapes are the smallest that cross every edge of the 256-row q-tile, the 32-row wave and the 64-key tile.

ref: flashinfer's run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188; the context-parallel dense attention
of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169."""
import math
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from lse_ops_torch import attention_lse, merge_states
from oracle import svg_oracle as O
from test_gpu_kernels import check_attn, dev, rel_l2
from poisoned import poisoned_like

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
# the relative rounding step of the probabilities the body sums ((__bf16)x / (_Float16)x, round to nearest): it bounds the relative error
# of the row sum, hence the absolute error of its log
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
T_SINGLE = {torch.bfloat16: 3e-3, torch.float16: 1e-3}   # check_attn's rel. L2 bound of one call


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _qkv(B, H, Sq, Skv, dtype, seed, D=128):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g).to(dtype)
    k, v = (torch.randn(B, H, Skv, D, generator=g).to(dtype) for _ in range(2))
    return q, k, v


def lse_ref(q, k, lo=0, hi=None, scale=None):
    """float64 log sum_j exp(scale * q.k_j) over the keys [lo, hi) of CPU tensors"""
    s = torch.matmul(q.double(), k[..., lo:hi, :].double().transpose(-1, -2)) * (scale if scale is not None else 1.0 / math.sqrt(q.shape[-1]))
    return torch.logsumexp(s, dim=-1)


def check_lse(lse, ref, dtype, what=""):
    lse = lse.double().cpu()
    assert lse.shape == ref.shape
    err = (lse - ref).abs()
    bound = U[dtype] + 1e-5 * (1 + ref.abs())
    print(f"{what} lse max err {err.max().item():.3e} (bound {bound.min().item():.3e})")
    assert torch.isfinite(lse).all() and (err <= bound).all(), (err.max().item(), bound.min().item())


# ---------------------------------------------------------------------------------------------------------
# (a) the LSE form against the plain form and a float64 reference
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq", [1, 255, 257, 800])
@pytest.mark.parametrize("Skv", [1, 37, 64, 65, 257, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_form_matches_plain_form_and_float64(nat, dtype, Skv, Sq):
    B, H = 2, 3
    q, k, v = _qkv(B, H, Sq, Skv, dtype, seed=Sq * 1009 + Skv)
    dq, dk, dv = dev(q), dev(k), dev(v)
    plain = nat.cross_attention(dq, dk, dv)
    o, lse = nat.cross_attention(dq, dk, dv, return_lse=True)
    assert lse.dtype == torch.float32 and lse.shape == (B, H, Sq) and lse.is_contiguous()
    assert o.dtype == dtype and torch.equal(o, plain)
    check_lse(lse, lse_ref(q, k), dtype)


# ---------------------------------------------------------------------------------------------------------
# (b) layouts: lse is contiguous fp32 with the bits of the contiguous call
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_layouts_equal_contiguous(nat, dtype):
    B, H, D, Sq, Skv = 2, 3, 128, 700, 257
    g = torch.Generator().manual_seed(9)
    q = dev(torch.randn(B, Sq, H * D, generator=g).to(dtype)).unflatten(2, (H, D)).transpose(1, 2)      # projection views [B, S, H * D]
    kv = dev(torch.randn(B, Skv, 2 * H * D, generator=g).to(dtype))                                     # one fused [B, Skv, 2 * H * D]
    k, v = (kv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(2))
    assert not q.is_contiguous() and not k.is_contiguous()
    o_ref, lse_ref_ = nat.cross_attention(q.contiguous(), k.contiguous(), v.contiguous(), return_lse=True)
    check_lse(lse_ref_, lse_ref(q.cpu(), k.cpu()), dtype)
    for kw in ({}, {"token_major_out": True}, {"out": poisoned_like(o_ref)}):
        o, lse = nat.cross_attention(q, k, v, return_lse=True, **kw)
        assert lse.dtype == torch.float32 and lse.is_contiguous() and torch.equal(lse, lse_ref_), kw
        assert torch.equal(o, o_ref), kw
        if kw.get("token_major_out"):
            assert o.transpose(1, 2).is_contiguous()
        if "out" in kw:
            assert o is kw["out"]
    o3, lse3 = nat.cross_attention(q[0], k[0], v[0], return_lse=True)                                   # [H, S, D] views
    assert lse3.shape == (H, Sq) and torch.equal(lse3, lse_ref_[0]) and torch.equal(o3, o_ref[0])


# ---------------------------------------------------------------------------------------------------------
# (c) key windows
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_over_key_windows(nat, dtype):
    B, H, Sq, Skv = 3, 2, 300, 320
    windows = [(70, 300), (5, 6), (40, 40)]            # a begin that is no multiple of 64; one key; empty
    q, k, v = _qkv(B, H, Sq, Skv, dtype, seed=21)
    kn, vn = k.clone(), v.clone()
    for b, (lo, hi) in enumerate(windows):             # a NaN in every key row outside the window
        kn[b, :, :lo], kn[b, :, hi:], vn[b, :, :lo], vn[b, :, hi:] = (float("nan"),) * 4
    kv_begin = torch.tensor([w[0] for w in windows], dtype=torch.int32, device="cuda")
    kv_end = torch.tensor([w[1] for w in windows], dtype=torch.int32, device="cuda")
    plain = nat.cross_attention_keyrange(dev(q), dev(kn), dev(vn), kv_end, kv_begin)
    o, lse = nat.cross_attention_keyrange(dev(q), dev(kn), dev(vn), kv_end, kv_begin, return_lse=True)
    assert torch.equal(o, plain) and lse.shape == (B, H, Sq) and lse.is_contiguous()
    assert not torch.isnan(o.float()).any() and not torch.isnan(lse).any()
    for b, (lo, hi) in enumerate(windows):
        if hi > lo:
            check_lse(lse[b], lse_ref(q[b], k[b], lo, hi), dtype, f"window [{lo}, {hi})")
            check_attn(o[b], O.masked_attention(q[b], k[b, :, lo:hi], v[b, :, lo:hi], None), dtype)
        else:
            assert (lse[b] == float("-inf")).all() and (o[b] == 0).all()
    # kv_begin None: from key 0
    o0, lse0 = nat.cross_attention_keyrange(dev(q), dev(k), dev(v), kv_end, return_lse=True)
    check_lse(lse0[0], lse_ref(q[0], k[0], 0, 300), dtype, "window [0, 300)")


# ---------------------------------------------------------------------------------------------------------
# (d) the exact path of the max-free softmax: large scores, the reference rises in the last key tile
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_lse_large_scores_dominant_key_in_last_tile(nat, dtype):
    B, H, Sq, Skv, D = 1, 2, 600, 512, 128
    g = torch.Generator().manual_seed(3)
    k = torch.randn(B, H, Skv, D, generator=g)
    v = torch.randn(B, H, Skv, D, generator=g)
    pick = torch.randint(Skv - 64, Skv, (B, H, Sq), generator=g)       # the dominant key of a row: in the last key tile
    q = 18.0 * torch.gather(k, 2, pick[..., None].expand(B, H, Sq, D)) + 0.1 * torch.randn(B, H, Sq, D, generator=g)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    ref = lse_ref(q, k)
    assert ref.min() > 120 and ref.max() < 400                         # scores of magnitude ~200
    o, lse = nat.cross_attention(dev(q), dev(k), dev(v), return_lse=True)
    assert torch.equal(o, nat.cross_attention(dev(q), dev(k), dev(v))) and torch.isfinite(o.float()).all()
    check_lse(lse, ref, dtype)


# ---------------------------------------------------------------------------------------------------------
# (e) resident loop: more work items than compute units
# ---------------------------------------------------------------------------------------------------------
def test_lse_resident_loop(nat):
    B, H, Sq, Skv, dtype = 1, 8, 25600, 64, torch.bfloat16             # 800 work items: every workgroup runs several q-tiles
    q, k, v = _qkv(B, H, Sq, Skv, dtype, seed=11)
    dq, dk, dv = dev(q), dev(k), dev(v)
    o, lse = nat.cross_attention(dq, dk, dv, return_lse=True)
    o2, lse2 = nat.cross_attention(dq, dk, dv, return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(o, nat.cross_attention(dq, dk, dv))
    for h in (0, 3, 7):
        check_lse(lse[:, h], lse_ref(q[:, h], k[:, h]), dtype, f"head {h}")


# ---------------------------------------------------------------------------------------------------------
# (f) the merge kernel against a float64 merge of the same inputs
# ---------------------------------------------------------------------------------------------------------
def _ordinal(x):
    """16-bit floats as integers whose difference counts representable values (sign-magnitude -> ordered)"""
    i = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def check_merge(o, lse, o_parts, lse_parts, dtype):
    """every output element within 1 ulp of the 16-bit type of the float64 result rounded to it (fp32 arithmetic cannot be further off);
    merged lse within 1e-5 * (1 + |lse|)"""
    ref_o, ref_l = merge_states([p.double().cpu() for p in o_parts], [p.double().cpu() for p in lse_parts], return_lse=True)
    d = (_ordinal(o.cpu()) - _ordinal(ref_o.to(dtype))).abs()
    print(f"merge: max ulp distance {d.max().item()}, elements off by one {(d == 1).float().mean().item():.2e}")
    assert d.max().item() <= 1
    if lse is not None:
        lse = lse.double().cpu()
        fin = torch.isfinite(ref_l)
        assert torch.equal(lse[~fin], ref_l[~fin])
        assert ((lse[fin] - ref_l[fin]).abs() <= 1e-5 * (1 + ref_l[fin].abs())).all()


def _partials(nat, n, Sq, D, dtype, seed, B=2, H=3, keys_per_part=40):
    """n partial results of the same rows: D 128 — the GPU's own, over n key shards; D 64 (no cross kernel there) — the torch statement's"""
    q, k, v = _qkv(B, H, Sq, n * keys_per_part, dtype, seed, D)
    o_parts, lse_parts = [], []
    for i in range(n):
        sl = slice(i * keys_per_part, (i + 1) * keys_per_part)
        if D == 128:
            o_i, l_i = nat.cross_attention(dev(q), dev(k[:, :, sl]), dev(v[:, :, sl]), return_lse=True)
        else:
            o_i, l_i = attention_lse(q.float(), k[:, :, sl].float(), v[:, :, sl].float())
            o_i, l_i = dev(o_i.to(dtype)), dev(l_i)
        o_parts.append(o_i)
        lse_parts.append(l_i)
    return o_parts, lse_parts


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("Sq", [1, 257])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_matches_float64_merge(nat, dtype, D, Sq, n):
    o_parts, lse_parts = _partials(nat, n, Sq, D, dtype, seed=n * 31 + Sq + D)
    o, lse = nat.merge_attention_states(o_parts, lse_parts, return_lse=True)
    assert o.shape == o_parts[0].shape and o.dtype == dtype and o.is_contiguous()
    assert lse.shape == lse_parts[0].shape and lse.dtype == torch.float32 and lse.is_contiguous()
    if n == 1:                                                         # copies the bits
        assert torch.equal(o.view(torch.int16), o_parts[0].view(torch.int16)) and torch.equal(lse, lse_parts[0])
    check_merge(o, lse, o_parts, lse_parts, dtype)
    assert torch.equal(nat.merge_attention_states(o_parts, lse_parts), o)   # without the merged lse


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_edge_cases_and_layouts(nat, dtype, D):
    Sq = 257
    o_parts, lse_parts = _partials(nat, 3, Sq, D, dtype, seed=5 + D)
    ninf = float("-inf")
    # a part with -inf rows: it contributes nothing there, and what its o holds is not looked at
    o1, l1 = o_parts[1].clone(), lse_parts[1].clone()
    o1[:, :, 100:200], l1[:, :, 100:200] = float("nan"), ninf
    o, lse = nat.merge_attention_states([o_parts[0], o1, o_parts[2]], [lse_parts[0], l1, lse_parts[2]], return_lse=True)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    check_merge(o, lse, [o_parts[0], o1, o_parts[2]], [lse_parts[0], l1, lse_parts[2]], dtype)
    o_two, lse_two = nat.merge_attention_states([o_parts[0], o_parts[2]], [lse_parts[0], lse_parts[2]], return_lse=True)
    assert torch.equal(o[:, :, 100:200], o_two[:, :, 100:200]) and torch.equal(lse[:, :, 100:200], lse_two[:, :, 100:200])
    # all parts -inf: zeros and -inf
    l_all = [torch.where(torch.arange(Sq, device="cuda") < 50, torch.tensor(ninf, device="cuda"), l) for l in lse_parts]
    o, lse = nat.merge_attention_states(o_parts, l_all, return_lse=True)
    assert (o[:, :, :50] == 0).all() and (lse[:, :, :50] == ninf).all() and torch.isfinite(lse[:, :, 50:]).all()
    check_merge(o, lse, o_parts, l_all, dtype)
    # one part 200 above the rest: that part, bit for bit
    l_dom = [lse_parts[0], lse_parts[1] + 200.0, lse_parts[2]]
    o, lse = nat.merge_attention_states(o_parts, l_dom, return_lse=True)
    assert torch.equal(o.view(torch.int16), o_parts[1].view(torch.int16)) and torch.equal(lse, l_dom[1])
    # a strided token-major out, and a caller's buffer
    ref = nat.merge_attention_states(o_parts, lse_parts)
    tm = nat.merge_attention_states(o_parts, lse_parts, token_major_out=True)
    assert tm.transpose(1, 2).is_contiguous() and not tm.is_contiguous() and torch.equal(tm, ref)
    big = torch.full((2, Sq + 7, 3, D), -77.0, dtype=dtype, device="cuda")   # token-major with rows behind the end
    out = big[:, :Sq].permute(0, 2, 1, 3)
    assert nat.merge_attention_states(o_parts, lse_parts, out=out) is out and torch.equal(out, ref) and (big[:, Sq:] == -77.0).all()
    o3 = nat.merge_attention_states([p[0] for p in o_parts], [p[0] for p in lse_parts])   # [H, S, D]
    assert o3.shape == (3, Sq, D) and torch.equal(o3, ref[0])


def test_merge_of_nine_parts_raises(nat):
    o_parts, lse_parts = _partials(nat, 1, 1, 128, torch.bfloat16, seed=1)
    with pytest.raises(ValueError, match="1 to 8"):
        nat.merge_attention_states(o_parts * 9, lse_parts * 9)
    lib = nat.load()
    import ctypes as C

    arr_o = (C.c_void_p * 9)(*[o_parts[0].data_ptr()] * 9)
    arr_l = (C.c_void_p * 9)(*[lse_parts[0].data_ptr()] * 9)
    out = poisoned_like(o_parts[0])
    rc = lib.svg_merge_attention_states(C.cast(arr_o, C.c_void_p), C.cast(arr_l, C.c_void_p), 9, out.data_ptr(), None, 6, 1, 128, 0, None, None)
    assert rc == -1                                                    # SVG_ERR_BAD_ARG, before any launch


# ---------------------------------------------------------------------------------------------------------
# (g) end to end: partials over key shards, merged, against the oracle over all keys
# ---------------------------------------------------------------------------------------------------------
def merged_limit(ref, dtype):
    """sqrt(t^2 + r^2): t the single-call tolerance of check_attn, r the error of ONE rounding of the exact result to the 16-bit type — a
    merged result carries one more independent output rounding than a single call, and independent roundings add in quadrature"""
    r = rel_l2(ref.to(dtype), ref)
    return math.sqrt(T_SINGLE[dtype] ** 2 + r ** 2), r


@pytest.mark.parametrize("cuts", [[0, 250, 500, 750, 1000], [0, 1, 1000]], ids=["4x250", "1+999"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sharded_keys_merged_match_oracle(nat, dtype, cuts):
    """measured on the MI355X, rel. L2 to the oracle (limit): bf16 2.84e-3 at 4 x 250 keys, 2.85e-3 at 1 + 999 (3.43e-3; one rounding
    1.66e-3, one call over all keys 2.35e-3); fp16 3.56e-4 / 3.59e-4 (1.02e-3; 2.07e-4, 2.94e-4) — DESIGN 3.1.4"""
    B, H, Sq, Skv = 2, 3, 300, 1000
    q, k, v = _qkv(B, H, Sq, Skv, dtype, seed=77)
    dq, dk, dv = dev(q), dev(k), dev(v)
    parts = [nat.cross_attention(dq, dk[:, :, a:b], dv[:, :, a:b], return_lse=True) for a, b in zip(cuts[:-1], cuts[1:])]   # strided slices
    o, lse = nat.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
    ref = O.masked_attention(q, k, v, None)
    limit, r = merged_limit(ref, dtype)
    single = rel_l2(nat.cross_attention(dq, dk, dv).cpu(), ref)
    err = rel_l2(o.cpu(), ref)
    print(f"merged rel_l2 {err:.3e} (limit {limit:.3e}; one rounding {r:.3e}; one call over all keys {single:.3e})")
    torch.testing.assert_close(o.float().cpu(), ref, atol=1e-2, rtol=1e-2)
    assert err <= limit, (err, limit)
    check_lse(lse, lse_ref(q, k), dtype, "merged")


# ---------------------------------------------------------------------------------------------------------
# (h) token_sharded_dense_attention: two ranks on one GPU over gloo
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT), str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle import svg_oracle as O_
    from svg import _native as nat_
    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    from svg import distributed as sd

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    H, S, D, unit, dtype = 5, 1100, 128, 128, torch.bfloat16
    g = torch.Generator().manual_seed(13)
    q, k, v = (torch.randn(1, H, S, D, generator=g).to(dtype) for _ in range(3))
    tr = [sd.token_range(S, r, world, unit) for r in range(world)]
    a, b = tr[rank]
    ql, kl, vl = (x[:, :, a:b].contiguous().to(device) for x in (q, k, v))
    res = {}
    o = sd.token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=True)
    # the single-process statement of the same arithmetic: the rank's rows over each shard, merged in shard order
    parts = [nat_.cross_attention(ql, k[:, :, lo:hi].contiguous().to(device), v[:, :, lo:hi].contiguous().to(device), return_lse=True)
             for lo, hi in tr]
    stated = nat_.merge_attention_states([p[0] for p in parts], [p[1] for p in parts])
    res["overlap_bits"] = bool(torch.equal(o, stated)) and o.shape == ql.shape
    ref = O_.masked_attention(q[:, :, a:b], k, v, None)
    ref_n = ref.float().norm().clamp(min=1e-20)
    res["err"] = ((o.float().cpu() - ref).norm() / ref_n).item()
    res["r"] = ((ref.to(dtype).float() - ref).norm() / ref_n).item()
    o_base = sd.token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=False)
    res["baseline_bits"] = bool(torch.equal(o_base, nat_.cross_attention(ql, k.to(device), v.to(device))))
    res["tokens"] = (a, b)
    torch.cuda.synchronize()
    ret[rank] = res
    dist.destroy_process_group()


def test_token_sharded_dense_attention_two_ranks_one_gpu():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 43500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    assert [got[r]["tokens"] for r in (0, 1)] == [(0, 512), (512, 1100)]          # ragged: the tail goes to the last rank
    for r in (0, 1):
        limit = math.sqrt(T_SINGLE[torch.bfloat16] ** 2 + got[r]["r"] ** 2)
        print(f"rank {r}: rel_l2 {got[r]['err']:.3e} (limit {limit:.3e})")
        assert got[r]["overlap_bits"] and got[r]["baseline_bits"], got[r]
        assert got[r]["err"] <= limit, (got[r]["err"], limit)
