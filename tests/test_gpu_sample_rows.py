"""svg_sample_dense_rows on the GPU (svg/_probe.py sample_dense_rows): dense attention of a few sampled rows against the float64 statement
tests/sparse_lse_cases.py masked_attention_lse on those rows.

Shapes, the smallest that reach every branch of the kernel: S = 70 (two tiles, the last ragged, a chunk per tile), 790 (a ragged tile with
several chunks; with valid_len = 761 both key segments, the rows 760 / 761 on either side of the seam, and chunks without a tile of a row's
segment), 4100 (65 tiles: more tiles than the 64 chunks, so chunks of two tiles and chunks without any); BH = 1, 3; head_dim 64, 128; bf16,
fp16; R = 1 (one lane), 17 (a partial second wave), 64 (full).  The rows are fixed lists with 0, S - 1 and a duplicate.
Bounds: o32 within the single-call rel. L2 bound T_SINGLE (the rows carry no output rounding: margin), lse by check_lse; every word of the
poisoned outputs written and finite; a permutation of `rows` permutes the results bit for bit (the chunks merge in chunk order)."""
import functools

import pytest
import torch

import sparse_lse_cases as SC
from poisoned import load_native, unwritten
from test_gpu_kernels import rel_l2

pytestmark = pytest.mark.gpu

VALID = 761


@pytest.fixture(scope="module")
def nat():
    return load_native()


@functools.lru_cache(maxsize=None)
def inputs(S, BH, D, dtype):
    g = torch.Generator().manual_seed(S * 7 + BH * 3 + D)
    return tuple(torch.randn(1, BH, S, D, generator=g).to(dtype) for _ in range(3))


def rows_for(S, R):
    """fixed rows: 0, S - 1, a duplicate, the rows around valid_len = 761 where the sequence has them, then a fixed scatter"""
    if R == 1:
        return [S - 1]
    head = [0, S - 1, 5, 5] + ([760, 761, 789] if S > 789 else [33, 34, 69])
    fill = [(i * 2654435761 + 12345) % S for i in range(64)]
    return (head + fill)[:R]


def segment_mask(rows, S, valid_len):
    """bool [R, S]: the keys dense_attention(valid_len=) gives each sampled row"""
    r = torch.tensor(rows)[:, None]
    key = torch.arange(S)[None, :]
    if valid_len <= 0 or valid_len >= S:
        return torch.ones(len(rows), S, dtype=torch.bool)
    return torch.where(r < valid_len, key < valid_len, key >= valid_len)


def reference(q, k, v, rows, valid_len):
    """float64 (o [cfg, H, R, D], lse [cfg, H, R]) of the sampled rows"""
    S = q.shape[2]
    return SC.masked_attention_lse(q[:, :, rows], k, v, segment_mask(rows, S, valid_len))


def check(o32, lse, ref_o, ref_lse, dtype, what):
    assert o32.dtype == torch.float32 and lse.dtype == torch.float32
    assert not unwritten(o32).any() and not unwritten(lse).any(), f"{what}: words the kernels left unwritten"
    assert torch.isfinite(o32).all() and torch.isfinite(lse).all(), what
    err = rel_l2(o32.cpu(), ref_o)
    print(f"{what} o32 rel. L2 {err:.3e} (bound {SC.T_SINGLE[dtype]:.1e})")
    assert err <= SC.T_SINGLE[dtype], (what, err)
    SC.check_lse(lse, ref_lse, dtype, what)


@pytest.mark.parametrize("valid_len", [0, VALID])
@pytest.mark.parametrize("R", [1, 17, 64])
@pytest.mark.parametrize("dtype", SC.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("BH", [1, 3])
@pytest.mark.parametrize("S", [70, 790, 4100])
def test_sample_dense_rows_against_float64(nat, S, BH, D, dtype, R, valid_len):
    from svg import _probe

    q, k, v = inputs(S, BH, D, dtype)
    rows = rows_for(S, R)
    ref_o, ref_lse = reference(q, k, v, rows, valid_len)
    qd, kd, vd = (x.cuda() for x in (q, k, v))
    o32, lse = _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows), valid_len=valid_len)
    assert o32.shape == (1, BH, R, D) and lse.shape == (1, BH, R)
    what = f"S={S} BH={BH} D={D} {dtype} R={R} valid_len={valid_len}"
    check(o32, lse, ref_o, ref_lse, dtype, what)
    # the same rows in another order (a device tensor this time): the same bits, permuted
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(R))
    o2, lse2 = _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows)[perm].cuda(), valid_len=valid_len)
    assert torch.equal(o2, o32[:, :, perm.cuda()]) and torch.equal(lse2, lse[:, :, perm.cuda()]), what
    if R > 3 and rows[2] == rows[3]:                     # the duplicate: two output rows, the same bits
        assert torch.equal(o32[:, :, 2], o32[:, :, 3]) and torch.equal(lse[:, :, 2], lse[:, :, 3])


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_token_major_views_are_read_in_place(nat, D, dtype):
    """q, k, v as the [cfg, H, S, D] views of a [cfg = 2, S, H, D] storage (svg_attn_layout_t with heads_per_batch = H): the bits of the
    contiguous call, and the float64 statement"""
    from svg import _probe

    cfg, H, S, R = 2, 3, 790, 17
    g = torch.Generator().manual_seed(11 + D)
    store = [torch.randn(cfg, S, H, D, generator=g).to(dtype) for _ in range(3)]
    rows = rows_for(S, R)
    q, k, v = (x.permute(0, 2, 1, 3) for x in store)
    ref_o, ref_lse = reference(q, k, v, rows, VALID)
    qd, kd, vd = (x.cuda().permute(0, 2, 1, 3) for x in store)
    assert not qd.is_contiguous() and nat._strided_ok(qd) and nat._strided_ok(kd, True)
    o32, lse = _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows), valid_len=VALID)
    assert o32.shape == (cfg, H, R, D) and o32.is_contiguous() and lse.shape == (cfg, H, R)
    check(o32, lse, ref_o, ref_lse, dtype, f"token-major D={D} {dtype}")
    oc, lc = _probe.sample_dense_rows(qd.contiguous(), kd.contiguous(), vd.contiguous(), torch.tensor(rows), valid_len=VALID)
    assert torch.equal(oc, o32) and torch.equal(lc, lse)


def test_sm_scale_and_the_default(nat):
    """sm_scale None is 1 / sqrt(D); another scale is another softmax (the statement with that scale)"""
    from svg import _probe

    S, BH, D, dtype, R = 790, 3, 128, torch.bfloat16, 17
    q, k, v = inputs(S, BH, D, dtype)
    rows = rows_for(S, R)
    qd, kd, vd = (x.cuda() for x in (q, k, v))
    a = _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows))
    b = _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows), valid_len=None, sm_scale=D ** -0.5)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    o32, lse = _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows), sm_scale=0.03)
    ref_o, ref_lse = SC.masked_attention_lse(q[:, :, rows], k, v, None, scale=0.03)
    check(o32, lse, ref_o, ref_lse, dtype, "sm_scale=0.03")
