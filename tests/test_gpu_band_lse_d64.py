"""svg_band_attention[_switch]_lse_d64[_f32] on the GPU (csrc/attention_band_d64.hip: attn_body_pp2 on BandLsePolicy64 / BandF32Policy64): o
bit-identical to the plain head_dim-64 call, lse against a float64 masked softmax, o32 rounded == o, two key-partitioned parts merged.
Bounds: tests/sparse_lse_cases.py, none of its own.  Outputs are poisoned allocations: a row nothing wrote stays NaN and fails."""
import pytest
import torch

import sparse_lse_cases as SC
from oracle import svg_oracle as O
from poisoned import assert_fully_written
from test_gpu_kernels import check_attn, dev, rel_l2

pytestmark = pytest.mark.gpu
H, D, F_, P_ = 2, 64, 4, 70   # (the video of the placement cases: 280 rows from row 0, text behind it)
TEXT = dict(real_len=291, colfull_lo=280, colfull_hi=291, rowfull_lo=280, rowfull_hi=291)
CASES = {"text300": (300, dict(TEXT, band=40)), "nokeys300": (300, dict(TEXT, band=0, colfull_lo=0, colfull_hi=0)),
         "tile64": (64, dict(O.dense_band_params(64), band=17)), "tile65": (65, dict(O.dense_band_params(65), band=17))}


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _inputs(S, dtype, seed=5):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, H, S, D, generator=g).to(dtype) for _ in range(3))


def _placed_reference(q, k, v, best, prm):
    S = q.shape[2]
    place = lambda x, inv=False: O.head_placement(x, best, S - F_ * P_, F_, P_, inverse=inv)   # noqa: E731
    o, lse = SC.masked_attention_lse(place(q), place(k), place(v), O.band_mask(S, **prm))
    return place(o, True), place(lse[..., None], True)[..., 0]


def _check_state(o, lse, o32, lse32, plain, ref, dtype, what):
    for t, name in ((o, "o"), (lse, "lse"), (o32, "o32"), (lse32, "lse of o32")):
        assert_fully_written(t, f"{what} {name}")
    assert torch.equal(o, plain) and o32.dtype == torch.float32 and torch.equal(o32.to(dtype), o)
    for x in (lse, lse32):
        assert x.dtype == torch.float32 and x.shape == o.shape[:-1] and x.is_contiguous()
        SC.check_lse(x, ref[1], dtype, what)
    check_attn(o, ref[0].float(), dtype)
    assert (o.cpu()[~torch.isfinite(ref[1])] == 0).all() and (o32.cpu()[~torch.isfinite(ref[1])] == 0).all()   # rows without keys


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_lse_and_fp32_rows_match_plain_entry_and_float64(nat, dtype, case):
    S, prm = CASES[case]
    q, k, v = _inputs(S, dtype)
    dq, dk, dv, bm = dev(q), dev(k), dev(v), nat.BandMask(**prm)
    ref = SC.masked_attention_lse(q, k, v, O.band_mask(S, **prm))
    assert bool((~torch.isfinite(ref[1])).any()) == (case == "nokeys300")
    o, lse = nat.band_attention_lse_d64(dq, dk, dv, bm)
    o32, lse32 = nat.band_attention_lse_d64(dq, dk, dv, bm, out_dtype=torch.float32)
    _check_state(o, lse, o32, lse32, nat.band_attention(dq, dk, dv, bm), ref, dtype, case)


@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_token_major_head_beside_a_logical_one_on_strided_views(nat, dtype):
    """head 0 token-major, head 1 logical; q, k, v views of a fused projection, o token-major: lse in the row order o is written in"""
    S, prm = CASES["text300"]
    q, k, v = _inputs(S, dtype)
    best = torch.tensor([[1, 0]])
    kw = dict(head_perm_flag=dev(best), vid0=0, num_frame=F_, frame_size=P_)
    qkv = dev(torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2))
    qv, kv_, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    bm = nat.BandMask(**prm)
    plain = nat.band_attention(qv, kv_, vv, bm, token_major_out=True, **kw)
    o, lse = nat.band_attention_lse_d64(qv, kv_, vv, bm, token_major_out=True, **kw)
    o32, lse32 = nat.band_attention_lse_d64(qv, kv_, vv, bm, out_dtype=torch.float32, **kw)
    ref = _placed_reference(q, k, v, best, prm)
    _check_state(o, lse, o32, lse32, plain, ref, dtype, "placement")


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_device_switch_selects_the_sparse_or_the_dense_mask(nat, dtype, flag):
    S, prm = CASES["text300"]
    q, k, v = _inputs(S, dtype)
    dq, dk, dv, best = dev(q), dev(k), dev(v), torch.tensor([[1, 0]])
    kw = dict(head_perm_flag=dev(best), vid0=0, num_frame=F_, frame_size=P_)
    bm, alt, fl = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S, 291)), dev(torch.tensor([flag], dtype=torch.int32))
    plain = nat.band_attention_switch(dq, dk, dv, bm, alt, fl, **kw)
    o, lse = nat.band_attention_switch_lse_d64(dq, dk, dv, bm, alt, fl, **kw)
    o32, lse32 = nat.band_attention_switch_lse_d64(dq, dk, dv, bm, alt, fl, out_dtype=torch.float32, **kw)
    ref = _placed_reference(q, k, v, best * (1 - flag), dict(O.dense_band_params(S, 291)) if flag else prm)   # (dense: logical rows)
    _check_state(o, lse, o32, lse32, plain, ref, dtype, f"switch flag {flag}")


@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_two_key_partitioned_parts_merge_to_dense_attention(nat, dtype):
    """keys [0, 130) and [130, 300) as full columns under band 0; merged == dense: merged_limit (16-bit parts), T_SINGLE (fp32 parts)"""
    S, cut = 300, 130
    q, k, v = _inputs(S, dtype)
    dq, dk, dv = dev(q), dev(k), dev(v)
    masks = [nat.BandMask(S, 0, lo, hi, 0, 0) for lo, hi in ((0, cut), (cut, S))]
    o_ref, lse_ref = SC.masked_attention_lse(q, k, v, None)
    p16 = [nat.band_attention_lse_d64(dq, dk, dv, m) for m in masks]
    p32 = [nat.band_attention_lse_d64(dq, dk, dv, m, out_dtype=torch.float32) for m in masks]
    o16, lse16 = nat.merge_attention_states([p[0] for p in p16], [p[1] for p in p16], return_lse=True)
    o32 = nat.merge_attention_states([p[0] for p in p32], [p[1] for p in p32], out_dtype=dtype)
    limit, r = SC.merged_limit(o_ref.float(), dtype)
    e16, e32 = rel_l2(o16.cpu(), o_ref.float()), rel_l2(o32.cpu(), o_ref.float())
    print(f"merged {dtype}: 16-bit parts {e16:.3e} (limit {limit:.3e}), fp32 parts {e32:.3e} (limit {SC.T_SINGLE[dtype]:.1e})")
    assert e16 <= limit and e32 <= SC.T_SINGLE[dtype] and e32 <= e16
    SC.check_lse(lse16, lse_ref, dtype, "merged", factor=2.0)
