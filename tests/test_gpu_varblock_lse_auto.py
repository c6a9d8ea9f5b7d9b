"""svg_varblock_attention_lse_auto[_f32] on the GPU (csrc/attention_varblock_lse.hip: the 128-row lock-step body and the head_dim-64
two-phase body on VarblockLsePolicyOf / VarblockF32PolicyOf; at head_dim 128 from Sq = 160 QB on the 16x16x32 kernels): o bit-identical to
the plain variant -1 call, lse and the fp32 rows against a float64 masked softmax, o32 rounded == o, two key partitions merged, one
layer-call below S = 160 block-rows.  Bounds: tests/sparse_lse_cases.py, none of its own.  Outputs are poisoned allocations: a row nothing
wrote stays NaN and fails."""
import pytest
import torch

import sparse_lse_cases as SC
from poisoned import assert_fully_written
from test_gpu_kernels import check_attn, dev, rel_l2

pytestmark = pytest.mark.gpu
H = 2
# name: (S, q cluster sizes, k cluster sizes, block map per head).  "lockstep": S < 160 QB — an empty cluster, two tiles with a remainder;
# head 0: a block-row that selects every key and one that selects none.  "two_phase": S >= 160 QB — 256-row tiles, a key-less block-row.
CASES = {
    "lockstep": (384, (200, 0, 184), (130, 64, 1, 189), [[[1, 1, 1, 1], [1, 0, 1, 0], [0, 0, 0, 0]], [[1, 0, 1, 1], [0, 1, 0, 0], [1, 1, 1, 1]]]),
    "two_phase": (512, (300, 212), (130, 64, 1, 317), [[[1, 0, 1, 1], [0, 1, 0, 1]], [[1, 1, 1, 1], [0, 0, 0, 0]]]),
}


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _case(name, D, dtype, perm):
    """-> (q, k, v, block map, q sizes, k sizes, kwargs with the row index arrays) on the GPU, float64 (o, lse) in the caller's row order"""
    S, qs, ks, bmap = CASES[name]
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(H, S, D, generator=g).to(dtype) for _ in range(3))
    bmap, rsz, csz = torch.tensor(bmap, dtype=torch.bool), torch.tensor([qs] * H, dtype=torch.int32), torch.tensor([ks] * H, dtype=torch.int32)
    qi, ki = (torch.stack([torch.randperm(S, generator=g) for _ in range(H)]) if perm else torch.arange(S).repeat(H, 1) for _ in range(2))
    o_s, lse_s = SC.vb_reference_of(q.gather(1, qi[..., None].expand(-1, -1, D)), k.gather(1, ki[..., None].expand(-1, -1, D)),
                                    v.gather(1, ki[..., None].expand(-1, -1, D)), bmap, rsz, csz)
    ref = torch.zeros_like(o_s).scatter_(1, qi[..., None].expand(-1, -1, D), o_s), torch.zeros_like(lse_s).scatter_(1, qi, lse_s)
    kw = dict(q_row_idx=dev(qi.int()), kv_row_idx=dev(ki.int())) if perm else {}
    return (dev(q), dev(k), dev(v), dev(bmap), dev(rsz), dev(csz)), kw, ref


@pytest.mark.parametrize("perm", [False, True], ids=["sorted", "row_idx"])
@pytest.mark.parametrize("dtype", SC.DTYPES)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("case", list(CASES))
def test_state_from_the_body_of_the_plain_call(nat, case, D, dtype, perm):
    args, kw, ref = _case(case, D, dtype, perm)
    keyless = ~torch.isfinite(ref[1])
    assert keyless.any() and not keyless.all(1).any()
    plain = nat.varblock_attention(*args, rows_covered=False, **kw)
    o, lse = nat.varblock_attention(*args, rows_covered=True, return_lse=True, body="auto", **kw)
    o32, lse32 = nat.varblock_attention(*args, rows_covered=True, return_lse=True, body="auto", out_dtype=torch.float32, **kw)
    for t, name in ((o, "o"), (lse, "lse"), (o32, "o32"), (lse32, "lse of o32")):
        assert_fully_written(t, f"{case} {name}")
    assert torch.equal(o, plain) and o32.dtype == torch.float32 and torch.equal(o32.to(dtype), o)
    for x in (lse, lse32):
        assert x.dtype == torch.float32 and x.shape == o.shape[:-1] and x.is_contiguous()
        SC.check_lse(x, ref[1], dtype, case)                       # (-inf exactly on the key-less block-row)
    assert (lse - lse32)[~keyless.cuda()].abs().max().item() <= 2 * float(SC.lse_bound(ref[1][~keyless], dtype).min())
    check_attn(o, ref[0].float(), dtype)
    err32 = rel_l2(o32.cpu(), ref[0].float())
    print(f"{case} D {D} {dtype} o32 rel_l2 {err32:.3e} (limit {SC.T_SINGLE[dtype]:.1e})")
    assert err32 <= SC.T_SINGLE[dtype]
    assert (o.cpu()[keyless] == 0).all() and (o32.cpu()[keyless] == 0).all()
    # rows_covered=False: the same state (every row is covered here: the fills change nothing)
    o_f, lse_f = nat.varblock_attention(*args, return_lse=True, body="auto", **kw)
    assert torch.equal(o_f, o) and torch.equal(lse_f, lse)


@pytest.mark.parametrize("dtype", SC.DTYPES)
@pytest.mark.parametrize("D", [64, 128])
def test_two_key_partitions_merge_to_the_one_call_result(nat, D, dtype):
    """lock-step case, key clusters [0, 2) and [2, 4): merged_limit (16-bit parts), T_SINGLE (fp32 parts)"""
    args, kw, ref = _case("lockstep", D, dtype, True)
    parts = [dev(m) for m in SC.split_key_clusters(args[3].cpu(), (0, 2, 4))]
    call = lambda m, **f32: nat.varblock_attention(*args[:3], m, *args[4:], rows_covered=True, return_lse=True, body="auto", **f32, **kw)   # noqa: E731
    p16, p32 = [call(m) for m in parts], [call(m, out_dtype=torch.float32) for m in parts]
    o16, lse16 = nat.merge_attention_states([p[0] for p in p16], [p[1] for p in p16], return_lse=True)
    o32 = nat.merge_attention_states([p[0] for p in p32], [p[1] for p in p32], out_dtype=dtype)
    limit, r = SC.merged_limit(ref[0].float(), dtype)
    e16, e32 = rel_l2(o16.cpu(), ref[0].float()), rel_l2(o32.cpu(), ref[0].float())
    print(f"merged D {D} {dtype}: 16-bit parts {e16:.3e} (limit {limit:.3e}), fp32 parts {e32:.3e} (limit {SC.T_SINGLE[dtype]:.1e})")
    assert e16 <= limit and e32 <= SC.T_SINGLE[dtype]
    SC.check_lse(lse16, ref[1], dtype, "merged", factor=2.0)


def test_layer_call_below_160_block_rows_measures_and_changes_nothing(nat):
    """svg2_sparse_attention at S = 900 < 160 * 6 with a zero-gain controller and lse_auto: the plain call's bits, a kept mass per head"""
    from svg.models import _core

    geo = _core.Geometry(context_length=0, num_frame=6, frame_size=150, text_first=False)
    g = torch.Generator().manual_seed(3)
    q, k, v = (dev(torch.randn(1, 3, 900, 128, generator=g).to(torch.bfloat16)) for _ in range(3))
    tps, outs = _core.TopPStore(), []
    for kw in ({}, dict(adaptive=_core.AdaptiveTopP(0.999, gain_up=0.0, gain_down=0.0), top_p_store=tps, lse_auto=True)):
        torch.manual_seed(11)
        _core.reseed_probe_generator(11)
        with torch.no_grad():
            outs.append(_core.svg2_sparse_attention(q, k, v, geo, _core.CentroidStore(), 0, 6, 12, 0.6, 0.1, 3, 2, **kw))
    kept = tps.kept[0]
    assert torch.equal(outs[0], outs[1]) and kept.shape == (3,) and bool(((kept > 0) & (kept <= 1 + 1e-4)).all()), kept
