"""fp32 parts and their merge on the GPU: svg_cross_attention_lse_f32 / svg_band_attention_lse_f32 / svg_varblock_attention_lse_f32 (the
epilogue of attn_m16_tile storing acc_o * inv as fp32 instead of rounding it: csrc/attn_m16.h HasRowO32) and
svg_merge_attention_states_f32 (csrc/merge_states.hip).

  1. same accumulators: o32 rounded to nearest even IS the o of the _lse sibling, bit for bit, and lse is bit-identical — on the shapes
     that cross every edge of the 256-row q-tile, the 32-row wave and the 64-key tile (Sq 1 / 257 / 300, Skv 1 / 64 / 65 / 1000), on
     projection views, key windows, head placement, real_len < S, the replay of the bf16 band kernel, row index arrays, key-less and
     uncovered rows;
  2. the merge against a float64 merge of the same fp32 parts rounded once: within 1 ulp of the 16-bit type;
  3. the point: partitioned attention through fp32 parts meets T_SINGLE — the bound of ONE call — against the float64 statement over all
     keys, and is no further off than the 16-bit parts merged on the same inputs: dense key shards, band + text keys, three ranges of key
     clusters;
  4. svg.distributed.token_sharded_dense_attention(fp32_parts=True) on two ranks sharing the GPU.

ref: flashinfer's run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188 (16-bit parts)."""
import ctypes as C_
import math
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import band_replay_cases as C
import sparse_lse_cases as SC
from lse_ops_torch import attention_lse, merge_states
from oracle import svg_oracle as O
from sparse_lse_cases import DTYPES, T_SINGLE, check_lse, rel_l2
from test_gpu_kernels import dev
from poisoned import poisoned_like

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
NINF = float("-inf")
F32 = dict(return_lse=True, out_dtype=torch.float32)


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _ordinal(x):
    """16-bit floats as integers whose difference counts representable values (sign-magnitude -> ordered)"""
    i = x.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def same_accumulators(got, want, dtype):
    """got = (o32, lse) of the fp32 form, want = (o, lse) of the _lse sibling: o32.to(T) (torch: round to nearest even) has the bits of o
    wherever o is finite, the rest agrees in kind; lse is bit-identical.
    Measured on the MI355X: 0 of 4.8 M (fp16) / 4.8 M (bf16) elements differ.  (fp16: the sibling's 16-bit store is compiled to a mix of
    v_fma_mixlo_f16 — the exact product rounded once — and v_pk_mul_f32 + v_cvt_pk_f16_f32 — rounded twice; the plain fp32 product missed it
    by one fp16 step on 153 of those elements, so csrc/attn_m16.h o32_values follows the store's own expression: DESIGN 3.1.4 "fp32 parts".)"""
    (o32, lse32), (o, lse) = got, want
    assert o32.dtype == torch.float32 and o32.shape == o.shape and o32.is_contiguous()
    assert lse32.dtype == torch.float32 and lse32.shape == lse.shape and lse32.is_contiguous()
    assert o.dtype == dtype
    r = o32.to(dtype)
    fin = torch.isfinite(o.float())
    d = (_ordinal(r)[fin] - _ordinal(o)[fin]).abs()
    print(f"o32.to({dtype}) against the 16-bit o: {int((d != 0).sum())} of {d.numel()} elements differ, by at most {int(d.max()) if d.numel() else 0} ulp")
    assert d.numel() == 0 or int(d.max()) <= 1          # both are roundings of the same product: never further apart than neighbours
    assert torch.equal(r.contiguous().view(torch.int16)[fin], o.contiguous().view(torch.int16)[fin])
    assert torch.equal(torch.isnan(r.float()), torch.isnan(o.float())) and torch.equal(r.float()[~fin].nan_to_num(), o.float()[~fin].nan_to_num())
    assert torch.equal(lse32.view(torch.int32), lse.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------
# 1. same accumulators
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq", [1, 257, 300])
@pytest.mark.parametrize("Skv", [1, 64, 65, 1000])
@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_plain_on_projection_views(nat, dtype, Skv, Sq):
    B, H, D = 1, 3, 128
    g = torch.Generator().manual_seed(Sq * 1009 + Skv)
    q = dev(torch.randn(B, Sq, H * D, generator=g).to(dtype)).unflatten(2, (H, D)).transpose(1, 2)      # views of a [B, S, H * D] projection
    kv = dev(torch.randn(B, Skv, 2 * H * D, generator=g).to(dtype))
    k, v = (kv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(2))
    want = nat.cross_attention(q, k, v, return_lse=True)
    got = nat.cross_attention(q, k, v, **F32)
    same_accumulators(got, want, dtype)
    assert torch.isfinite(got[0]).all()
    # contiguous tensors: the same bits
    got_c = nat.cross_attention(q.contiguous(), k.contiguous(), v.contiguous(), **F32)
    assert torch.equal(got_c[0], got[0]) and torch.equal(got_c[1], got[1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_windowed(nat, dtype):
    """left-padded, ragged and empty windows, one per head (BH 3); a NaN in every key row outside the window"""
    B, H, Sq, Skv = 3, 1, 300, 320
    windows = [(70, 320), (5, 133), (40, 40)]
    g = torch.Generator().manual_seed(21)
    q = torch.randn(B, H, Sq, 128, generator=g).to(dtype)
    k, v = (torch.randn(B, H, Skv, 128, generator=g).to(dtype) for _ in range(2))
    for b, (lo, hi) in enumerate(windows):
        k[b, :, :lo], k[b, :, hi:], v[b, :, :lo], v[b, :, hi:] = (float("nan"),) * 4
    kv_begin = torch.tensor([w[0] for w in windows], dtype=torch.int32, device="cuda")
    kv_end = torch.tensor([w[1] for w in windows], dtype=torch.int32, device="cuda")
    want = nat.cross_attention_keyrange(dev(q), dev(k), dev(v), kv_end, kv_begin, return_lse=True)
    got = nat.cross_attention_keyrange(dev(q), dev(k), dev(v), kv_end, kv_begin, **F32)
    same_accumulators(got, want, dtype)
    assert torch.isfinite(got[0]).all()
    assert (got[0][2] == 0).all() and (got[1][2] == NINF).all()          # the empty window: zeros and -inf
    assert torch.isfinite(got[1][:2]).all() and (got[0][:2] != 0).any()


def test_cross_c_entry_does_not_read_the_o_member_of_the_layout(nat):
    """the layout describes q, k and v; garbage in its o member changes nothing"""
    dtype, B, H, Sq, Skv = torch.bfloat16, 1, 3, 257, 65
    g = torch.Generator().manual_seed(4)
    q = dev(torch.randn(B, H, Sq, 128, generator=g).to(dtype))
    k, v = (dev(torch.randn(B, H, Skv, 128, generator=g).to(dtype)) for _ in range(2))
    ref32, ref_lse = nat.cross_attention(q, k, v, **F32)
    lay = nat.attn_layout(q, k, v, q)
    lay.o = nat.TensorStrides(-3, 5, 1)
    o32 = torch.full_like(ref32, float("nan"))
    lse = poisoned_like(ref_lse)
    rc = nat.load().svg_cross_attention_lse_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), o32.data_ptr(), lse.data_ptr(), B * H, Sq, Skv, 128, 0,
                                                1.0 / math.sqrt(128), None, None, 1, C_.byref(lay), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(o32, ref32) and torch.equal(lse, ref_lse)


@pytest.mark.parametrize("model", SC.BAND_MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_band_cases(nat, dtype, model):
    """the cases of tests/sparse_lse_cases.py (hy: real_len 761 < S 790; wan, cog, dense2), BH 3"""
    S, prm, mask, _ = SC.band_case(model)
    q, k, v = (dev(x) for x in SC.band_inputs(model, dtype))
    bm = nat.BandMask(**prm)
    want = nat.band_attention(q, k, v, bm, return_lse=True)
    got = nat.band_attention(q, k, v, bm, **F32)
    same_accumulators(got, want, dtype)
    check_lse(got[1], SC.band_reference(model, dtype)[1], dtype, f"band {model}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_band_under_head_placement_and_on_views(nat, dtype):
    """heads 0 and 2 token-major: o32 and lse are in the caller's (physical) row order; the same call on views of a fused projection"""
    F_, P_ = SC.GEOM["F_"], SC.GEOM["P_"]
    S, prm, mask, vid0 = SC.band_case("wan")
    q, k, v = SC.band_inputs("wan", dtype)
    kw = dict(head_perm_flag=dev(torch.tensor([[1, 0, 1]])), vid0=vid0, num_frame=F_, frame_size=P_)
    bm = nat.BandMask(**prm)
    want = nat.band_attention(dev(q), dev(k), dev(v), bm, return_lse=True, **kw)
    got = nat.band_attention(dev(q), dev(k), dev(v), bm, **F32, **kw)
    same_accumulators(got, want, dtype)
    plain = nat.band_attention(dev(q), dev(k), dev(v), bm, **F32)
    assert not torch.equal(plain[1][0, 0], got[1][0, 0]) and torch.equal(plain[1][0, 1], got[1][0, 1])   # (the placement moved rows)
    H, D = SC.BAND_H, SC.D
    qkv = dev(torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2))
    qv, kv_, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not qv.is_contiguous()
    got_v = nat.band_attention(qv, kv_, vv, bm, **F32, **kw)
    assert got_v[0].is_contiguous() and torch.equal(got_v[0], got[0]) and torch.equal(got_v[1], got[1])


def test_band_under_replay(nat):
    """the spike case of the existing replay test in which every q-tile of real rows is replayed (bf16): a q-tile whose validation fails
    stores nothing, its replay stores o32 and lse.  Only the counter is read."""
    case = C.queue_case("all6")
    g, kind = case.geo, case.kinds[0]
    qd, kd, vd = (O.head_placement(x, C.BEST, g.CTX, g.F, g.P, inverse=True).cuda().contiguous() for x in C.inputs(case))
    kw = dict(head_perm_flag=C.BEST.cuda(), vid0=0, num_frame=g.F, frame_size=g.P)
    bm = nat.BandMask(**g.mask_params(kind))
    nat.band_replays(reset=True)
    want = nat.band_attention(qd, kd, vd, bm, return_lse=True, **kw)
    n_lse = nat.band_replays(reset=True)
    got = nat.band_attention(qd, kd, vd, bm, **F32, **kw)
    n = nat.band_replays(reset=True)
    print(f"{case.name}: replays {n} (lse entry {n_lse})")
    assert n == n_lse == 12                            # every q-tile of real rows, both heads (tests/test_gpu_band_speculative.py)
    assert torch.isfinite(got[0]).all()
    same_accumulators(got, want, case.dtype)


@pytest.mark.parametrize("case", SC.VB_CASES, ids=lambda c: "-".join(str(x) for x in c))
@pytest.mark.parametrize("dtype", DTYPES)
def test_varblock_cases(nat, dtype, case):
    q, k, v, bmap, rsz, csz = SC.vb_inputs(case, dtype)
    args = [dev(x) for x in (q, k, v, bmap, rsz, csz)]
    want = nat.varblock_attention(*args, return_lse=True)
    got = nat.varblock_attention(*args, **F32)
    same_accumulators(got, want, dtype)
    check_lse(got[1], SC.vb_reference(case, dtype)[1], dtype, f"varblock {case}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_varblock_edge_cases_and_strided_v(nat, dtype):
    """the edge cases of the existing LSE test — a block-row without active blocks, a key cluster of size 0, a block-row whose only active
    cluster is the empty one, rows no block-row covers (rows_covered=False: zeros and -inf) — and the same call on views of a fused QKV
    projection (strided q, k and v)"""
    case = SC.VB_CASES[1]
    hq, hkv, S, MB, NB, _ = case
    q, k, v, bmap, rsz, csz = (x.clone() for x in SC.vb_inputs(case, dtype))
    bmap[:, 2] = False
    csz[:, 8] += csz[:, 7]
    csz[:, 7] = 0
    bmap[:, 4] = False
    bmap[:, 4, 7] = True
    short = 7
    rsz[torch.arange(hkv), rsz.argmax(dim=1)] -= short
    rest = [dev(x) for x in (bmap, rsz, csz)]
    want = nat.varblock_attention(dev(q), dev(k), dev(v), *rest, return_lse=True)
    got = nat.varblock_attention(dev(q), dev(k), dev(v), *rest, **F32)
    same_accumulators(got, want, dtype)
    o32, lse = got[0].cpu(), got[1].cpu()
    grp = hq // hkv
    for h in range(hkv):
        off = torch.cat((torch.zeros(1, dtype=torch.long), rsz[h].long().cumsum(0)))
        for rows in (slice(int(off[2]), int(off[3])), slice(int(off[4]), int(off[5])), slice(S - short, S)):
            assert (lse[h * grp:(h + 1) * grp, rows] == NINF).all() and (o32[h * grp:(h + 1) * grp, rows] == 0).all()
    H, D = q.shape[0], q.shape[2]
    qkv = dev(torch.cat([x.transpose(0, 1).reshape(1, S, H * D) for x in (q, k, v)], dim=2))
    qv, kv_, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not vv.is_contiguous()
    got_v = nat.varblock_attention(qv, kv_, vv, *rest, **F32)
    assert got_v[0].shape == (1, H, S, D) and got_v[0].is_contiguous()
    assert torch.equal(got_v[0][0], got[0]) and torch.equal(got_v[1][0], got[1])


def test_varblock_with_row_index_arrays(nat):
    """q_row_idx / kv_row_idx: o32 and lse in the caller's row order; a q cluster without keys"""
    torch.manual_seed(5)
    H, S, D, QC, KC, dtype = 3, 3000, 128, 13, 37, torch.bfloat16
    q, k, v = (dev(torch.randn(H, S, D).to(dtype)) for _ in range(3))
    ql = torch.randint(0, QC, (H, S), dtype=torch.int32)
    kl = torch.randint(0, KC, (H, S), dtype=torch.int32)
    bmap = torch.rand(H, QC, KC) > 0.5
    bmap[:, 3] = False
    qidx, qcnt = nat.argsort_labels(dev(ql), QC)
    kidx, kcnt = nat.argsort_labels(dev(kl), KC)
    kw = dict(q_row_idx=qidx, kv_row_idx=kidx, rows_covered=True)
    want = nat.varblock_attention(q, k, v, dev(bmap), qcnt, kcnt, return_lse=True, **kw)
    got = nat.varblock_attention(q, k, v, dev(bmap), qcnt, kcnt, **F32, **kw)
    same_accumulators(got, want, dtype)
    none = dev(ql == 3)
    assert (got[1][none] == NINF).all() and (got[0][none] == 0).all() and torch.isfinite(got[1][~none]).all()


# ---------------------------------------------------------------------------------------------------------
# 2. the merge kernel against a float64 merge of the same fp32 parts, rounded once
# ---------------------------------------------------------------------------------------------------------
def check_merge(o, lse, o_parts, lse_parts, dtype, one_ulp=True):
    """against the float64 merge of the SAME fp32 parts rounded once; merged lse within 1e-5 * (1 + |lse|), the tolerance of
    tests/test_gpu_attention_lse.py test_merge_matches_float64_merge.
    one_ulp (parts whose terms share a sign per element, _partials): every output element within 1 ulp of the 16-bit type — fp32
    arithmetic is then far below a 16-bit ulp, only rounding-boundary cases differ.
    Always: |o - ref| <= 1 ulp of T at ref + (n + 3) 2^-23 sum_i w_i |o_i| / sum_i w_i, the forward error of n fp32 multiply-adds, the
    division and exp2 / log of the hardware (2 ulp) on the TERMS — which is what a result that cancels to far below its terms carries, and
    what bf16's 8 exponent bits resolve (N(0, 1) parts: an fp32 emulation of the statement is 20 bf16 ulps off at |o| = 3e-8)."""
    od, ld = [p.double().cpu() for p in o_parts], [p.double().cpu() for p in lse_parts]
    ref_o, ref_l = merge_states(od, ld, return_lse=True)
    ref_t = ref_o.to(dtype)
    d = (_ordinal(o.cpu()) - _ordinal(ref_t)).abs()
    print(f"merge: max ulp distance {d.max().item()}, elements off by one {(d == 1).float().mean().item():.2e}")
    if one_ulp:
        assert d.max().item() <= 1
    L = torch.stack(ld)
    m = L.max(0).values
    w = torch.exp(L - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    terms = torch.where(w[..., None] > 0, w[..., None] * torch.stack(od).abs(), torch.zeros_like(w[..., None])).sum(0)
    terms = terms / torch.where(w.sum(0) > 0, w.sum(0), torch.ones_like(m))[..., None]
    ulp = (ref_t.double().abs() * 2.0 ** -(7 if dtype == torch.bfloat16 else 10)).clamp(min=2.0 ** -24 if dtype == torch.float16 else 0.0)
    assert ((o.double().cpu() - ref_o).abs() <= ulp + (len(od) + 3) * 2.0 ** -23 * terms).all()
    if lse is not None:
        lse = lse.double().cpu()
        fin = torch.isfinite(ref_l)
        assert torch.equal(lse[~fin], ref_l[~fin])
        assert ((lse[fin] - ref_l[fin]).abs() <= 1e-5 * (1 + ref_l[fin].abs())).all()


def _partials(nat, n, Sq, D, dtype, seed, B=1, H=3, keys_per_part=40, signed_columns=True):
    """n fp32 parts of the same rows: D 128 — the GPU's own, over n key shards; D 64 (no attention kernel hands out fp32 there) — the torch
    statement's in fp32.  -> parts, lse, and the q / k / v shards (for the 16-bit sibling).
    signed_columns: v[..., c] = s_c (0.1 + |N(0, 1)|) with a random sign per column, so the n terms of an output element share a sign and
    the merged element is no smaller than the smallest of them: the premise of the 1-ulp check (check_merge).  False: N(0, 1) values, whose
    merged elements may cancel to far below their terms."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g).to(dtype)
    k, v = (torch.randn(B, H, n * keys_per_part, D, generator=g) for _ in range(2))
    if signed_columns:
        v = (0.1 + v.abs()) * (torch.randint(0, 2, (D,), generator=g) * 2 - 1).float()
    k, v = k.to(dtype), v.to(dtype)
    o_parts, lse_parts = [], []
    for i in range(n):
        sl = slice(i * keys_per_part, (i + 1) * keys_per_part)
        if D == 128:
            o_i, l_i = nat.cross_attention(dev(q), dev(k[:, :, sl]), dev(v[:, :, sl]), **F32)
        else:
            o_i, l_i = (dev(x) for x in attention_lse(q.float(), k[:, :, sl].float(), v[:, :, sl].float()))
        assert o_i.dtype == torch.float32
        o_parts.append(o_i)
        lse_parts.append(l_i)
    return o_parts, lse_parts, (q, k, v)


@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("Sq", [1, 257])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_f32_matches_float64_merge(nat, dtype, D, Sq, n):
    o_parts, lse_parts, (q, k, v) = _partials(nat, n, Sq, D, dtype, seed=n * 31 + Sq + D)
    o, lse = nat.merge_attention_states(o_parts, lse_parts, out_dtype=dtype, return_lse=True)
    assert o.shape == o_parts[0].shape and o.dtype == dtype and o.is_contiguous()
    assert lse.shape == lse_parts[0].shape and lse.dtype == torch.float32 and lse.is_contiguous()
    check_merge(o, lse, o_parts, lse_parts, dtype)
    assert torch.equal(nat.merge_attention_states(o_parts, lse_parts, out_dtype=dtype), o)   # without the merged lse
    # N(0, 1) values: elements that cancel to far below their terms are held to the forward error of the fp32 statement on the terms
    o_parts_n, lse_parts_n, _ = _partials(nat, n, Sq, D, dtype, seed=n * 31 + Sq + D, signed_columns=False)
    check_merge(*nat.merge_attention_states(o_parts_n, lse_parts_n, out_dtype=dtype, return_lse=True), o_parts_n, lse_parts_n, dtype, one_ulp=False)
    if n == 1:                                                         # the part rounded once: the bits of the plain 16-bit entry
        assert torch.equal(o.view(torch.int16), o_parts[0].to(dtype).view(torch.int16)) and torch.equal(lse, lse_parts[0])
        if D == 128:
            assert torch.equal(o.view(torch.int16), nat.cross_attention(dev(q), dev(k), dev(v)).view(torch.int16))


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_f32_edge_cases_and_layouts(nat, dtype, D):
    Sq, B, H = 257, 2, 3
    o_parts, lse_parts, _ = _partials(nat, 3, Sq, D, dtype, seed=5 + D, B=B)
    kw = dict(out_dtype=dtype, return_lse=True)
    # a part with -inf rows: it contributes nothing there, and what its o holds is not looked at
    o1, l1 = o_parts[1].clone(), lse_parts[1].clone()
    o1[:, :, 100:200], l1[:, :, 100:200] = float("nan"), NINF
    o, lse = nat.merge_attention_states([o_parts[0], o1, o_parts[2]], [lse_parts[0], l1, lse_parts[2]], **kw)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    check_merge(o, lse, [o_parts[0], o1, o_parts[2]], [lse_parts[0], l1, lse_parts[2]], dtype)
    o_two, lse_two = nat.merge_attention_states([o_parts[0], o_parts[2]], [lse_parts[0], lse_parts[2]], **kw)
    assert torch.equal(o[:, :, 100:200], o_two[:, :, 100:200]) and torch.equal(lse[:, :, 100:200], lse_two[:, :, 100:200])
    # all parts -inf: zeros and -inf
    l_all = [torch.where(torch.arange(Sq, device="cuda") < 50, torch.tensor(NINF, device="cuda"), l) for l in lse_parts]
    o, lse = nat.merge_attention_states(o_parts, l_all, **kw)
    assert (o[:, :, :50] == 0).all() and (lse[:, :, :50] == NINF).all() and torch.isfinite(lse[:, :, 50:]).all()
    check_merge(o, lse, o_parts, l_all, dtype)
    # a part 100 below the largest leaves the others' result alone (its weight e^-100 is below fp32's reach beside 1)
    l_low = [lse_parts[0], torch.maximum(lse_parts[0], lse_parts[2]) - 100.0, lse_parts[2]]
    o, lse = nat.merge_attention_states(o_parts, l_low, **kw)
    assert torch.equal(o.view(torch.int16), o_two.view(torch.int16)) and torch.equal(lse, lse_two)
    # a strided token-major out, and a caller's buffer (its dtype decides)
    ref = nat.merge_attention_states(o_parts, lse_parts, out_dtype=dtype)
    tm = nat.merge_attention_states(o_parts, lse_parts, out_dtype=dtype, token_major_out=True)
    assert tm.dtype == dtype and tm.transpose(1, 2).is_contiguous() and not tm.is_contiguous() and torch.equal(tm, ref)
    big = torch.full((B, Sq + 7, H, D), -77.0, dtype=dtype, device="cuda")   # token-major with rows behind the end
    out = big[:, :Sq].permute(0, 2, 1, 3)
    assert nat.merge_attention_states(o_parts, lse_parts, out=out) is out and torch.equal(out, ref) and (big[:, Sq:] == -77.0).all()
    o3 = nat.merge_attention_states([p[0] for p in o_parts], [p[0] for p in lse_parts], out_dtype=dtype)   # [H, S, D]
    assert o3.shape == (H, Sq, D) and torch.equal(o3, ref[0])


# ---------------------------------------------------------------------------------------------------------
# 3. the point of the change: partitioned attention at the tolerance of one call
# ---------------------------------------------------------------------------------------------------------
def check_point(nat, parts32, parts16, ref, dtype, what):
    """fp32 parts merged by the fp32 merge: within T_SINGLE — the bound of ONE call — of the float64 statement over all keys, and no
    further off than the 16-bit parts merged on the same inputs"""
    o = nat.merge_attention_states([p[0] for p in parts32], [p[1] for p in parts32], out_dtype=dtype)
    o16 = nat.merge_attention_states([p[0] for p in parts16], [p[1] for p in parts16])
    err, err16 = rel_l2(o.cpu(), ref), rel_l2(o16.cpu(), ref)
    r = rel_l2(ref.to(dtype), ref)
    print(f"{what} {dtype}: fp32 parts rel_l2 {err:.3e} (limit {T_SINGLE[dtype]:.1e}); 16-bit parts {err16:.3e}; one rounding {r:.3e}")
    assert o.dtype == dtype
    torch.testing.assert_close(o.float().cpu(), ref, atol=1e-2, rtol=1e-2)
    assert err <= T_SINGLE[dtype], (err, T_SINGLE[dtype])
    assert err <= err16, (err, err16)
    return o


@pytest.mark.parametrize("cuts", [[0, 250, 500, 750, 1000], [0, 1, 1000]], ids=["4x250", "1+999"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sharded_keys_through_fp32_parts_meet_the_single_call_bound(nat, dtype, cuts):
    """the inputs and cuts of tests/test_gpu_attention_lse.py test_sharded_keys_merged_match_oracle.  Measured on the MI355X, rel. L2 to the
    oracle, fp32 parts / 16-bit parts (one rounding; limit T_SINGLE): bf16 2.30e-3 / 2.84e-3 at 4 x 250 keys, 2.34e-3 / 2.85e-3 at 1 + 999
    (1.66e-3; 3e-3); fp16 2.88e-4 / 3.56e-4 and 2.94e-4 / 3.59e-4 (2.07e-4; 1e-3) — DESIGN 3.1.4"""
    B, H, Sq, Skv = 2, 3, 300, 1000
    g = torch.Generator().manual_seed(77)
    q = torch.randn(B, H, Sq, 128, generator=g).to(dtype)
    k, v = (torch.randn(B, H, Skv, 128, generator=g).to(dtype) for _ in range(2))
    dq, dk, dv = dev(q), dev(k), dev(v)
    shards = list(zip(cuts[:-1], cuts[1:]))
    parts32 = [nat.cross_attention(dq, dk[:, :, a:b], dv[:, :, a:b], **F32) for a, b in shards]                # strided slices
    parts16 = [nat.cross_attention(dq, dk[:, :, a:b], dv[:, :, a:b], return_lse=True) for a, b in shards]
    check_point(nat, parts32, parts16, O.masked_attention(q, k, v, None), dtype, f"key shards {cuts}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_band_over_video_keys_and_dense_over_text_keys_through_fp32_parts(nat, dtype):
    """protocol (a) of tests/test_gpu_sparse_attention_lse.py.  Measured on the MI355X, fp32 parts / 16-bit parts: bf16 2.28e-3 / 2.83e-3,
    fp16 2.87e-4 / 3.54e-4 (limit 3e-3 / 1e-3) — DESIGN 3.1.3"""
    Vn, real = SC.V, SC.REAL
    q, k, v = (dev(x) for x in SC.band_inputs("hy", dtype))
    bm = nat.BandMask(**SC.VIDEO_BAND)
    qv, kvid, vvid, ktxt, vtxt = q[:, :, :Vn], k[:, :, :Vn], v[:, :, :Vn], k[:, :, Vn:real], v[:, :, Vn:real]
    parts32 = [nat.band_attention(qv, kvid, vvid, bm, **F32), nat.cross_attention(qv, ktxt, vtxt, **F32)]
    parts16 = [nat.band_attention(qv, kvid, vvid, bm, return_lse=True), nat.cross_attention(qv, ktxt, vtxt, return_lse=True)]
    o_ref = SC.band_reference("hy", dtype)[0][:, :, :Vn].float()
    check_point(nat, parts32, parts16, o_ref, dtype, "band + text keys")


@pytest.mark.parametrize("dtype", DTYPES)
def test_varblock_over_three_key_cluster_ranges_through_fp32_parts(nat, dtype):
    """protocol (b) of tests/test_gpu_sparse_attention_lse.py.  Measured on the MI355X, fp32 parts / 16-bit parts: bf16 2.30e-3 / 2.82e-3,
    fp16 2.88e-4 / 3.53e-4 (limit 3e-3 / 1e-3) — DESIGN 3.1.3"""
    case = SC.VB_CASES[0]
    NB = case[4]
    q, k, v, bmap, rsz, csz = SC.vb_inputs(case, dtype)
    bmap = bmap.clone()
    bmap[:, 0] = False
    bmap[:, 0, 3:20] = True                             # block-row 0: keys of part 0 only
    base = [dev(x) for x in (q, k, v)]
    maps = [dev(b) for b in SC.split_key_clusters(bmap, [0, 30, 71, NB])]
    parts32 = [nat.varblock_attention(*base, b, dev(rsz), dev(csz), **F32) for b in maps]
    parts16 = [nat.varblock_attention(*base, b, dev(rsz), dev(csz), return_lse=True) for b in maps]
    o_ref = SC.vb_reference_of(q, k, v, bmap, rsz, csz)[0].float()
    o = check_point(nat, parts32, parts16, o_ref, dtype, "three key-cluster ranges")
    r0 = int(rsz[0, 0])                                 # the rows of block-row 0: part 0 rounded once
    assert torch.equal(o[:, :r0], parts32[0][0][:, :r0].to(dtype))


# ---------------------------------------------------------------------------------------------------------
# 4. token_sharded_dense_attention(fp32_parts=True): two ranks on one GPU over gloo
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
    o = sd.token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=True, fp32_parts=True)
    # the single-process statement of the same calls: the rank's rows over each shard as fp32 parts, merged in shard order
    parts = [nat_.cross_attention(ql, k[:, :, lo:hi].contiguous().to(device), v[:, :, lo:hi].contiguous().to(device), return_lse=True,
                                  out_dtype=torch.float32) for lo, hi in tr]
    stated = nat_.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], out_dtype=dtype)
    res["bits"] = bool(torch.equal(o, stated)) and o.shape == ql.shape and o.dtype == dtype
    ref = O_.masked_attention(q[:, :, a:b], k, v, None)
    res["err"] = ((o.float().cpu() - ref).norm() / ref.float().norm().clamp(min=1e-20)).item()
    o_base = sd.token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=False, fp32_parts=True)
    res["baseline_bits"] = bool(torch.equal(o_base, nat_.cross_attention(ql, k.to(device), v.to(device))))
    res["tokens"] = (a, b)
    torch.cuda.synchronize()
    ret[rank] = res
    dist.destroy_process_group()


def test_token_sharded_dense_attention_fp32_parts_two_ranks_one_gpu():
    """5 heads, S = 1100, unit 128 (the shape of the 16-bit test): bit-identical to the single-process statement, within T_SINGLE of the
    oracle.  Measured on the MI355X: rank 0 2.32e-3, rank 1 2.31e-3 (16-bit parts: 2.86e-3 / 2.85e-3)"""
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 47500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    assert [got[r]["tokens"] for r in (0, 1)] == [(0, 512), (512, 1100)]          # ragged: the tail goes to the last rank
    for r in (0, 1):
        print(f"rank {r}: rel_l2 {got[r]['err']:.3e} (limit {T_SINGLE[torch.bfloat16]:.1e})")
        assert got[r]["bits"] and got[r]["baseline_bits"], got[r]
        assert got[r]["err"] <= T_SINGLE[torch.bfloat16], got[r]["err"]
