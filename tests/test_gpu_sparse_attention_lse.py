"""svg_band_attention_lse and svg_varblock_attention_lse on the GPU (csrc/attention.hip on BandLsePolicy, csrc/attention_varblock.hip on
VarblockLsePolicy): the row log-sum-exp of the band (SVG1) and variable-block (SVG2) bodies against a float64 statement, with o
bit-identical to the entry without it — under head placement, on strided views, under the replay of the bf16 band kernel, with row index
arrays, remainder packing and key-less rows — and the two protocols the output exists for: a band over the video keys merged with a dense
call over the text keys, and variable-block attention over three ranges of key clusters merged, both against the float64 statement of the
whole.  Inputs, references and bounds: tests/sparse_lse_cases.py (the bounds are those of tests/test_gpu_attention_lse.py).

ref: BlockSparseAttentionWrapper.run(..., return_lse=True) + a dense call with return_lse=True + merge_state,
svg/kernels/ops/attention_ops.py:178-188."""
import sys
from pathlib import Path

import pytest
import torch

import band_replay_cases as C
import sparse_lse_cases as SC
from oracle import svg_oracle as O
from sparse_lse_cases import DTYPES, check_lse, merged_limit, rel_l2
from test_gpu_kernels import check_attn, dev

pytestmark = pytest.mark.gpu
NINF = float("-inf")


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _lse_ok(lse, shape):
    assert lse.dtype == torch.float32 and lse.shape == shape and lse.is_contiguous()


# ---------------------------------------------------------------------------------------------------------
# band
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", SC.BAND_MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_band_lse_matches_plain_entry_and_float64(nat, dtype, model):
    S, prm, mask, _ = SC.band_case(model)
    q, k, v = SC.band_inputs(model, dtype)
    dq, dk, dv = dev(q), dev(k), dev(v)
    bm = nat.BandMask(**prm)
    plain = nat.band_attention(dq, dk, dv, bm)
    o, lse = nat.band_attention(dq, dk, dv, bm, return_lse=True)
    _lse_ok(lse, (1, SC.BAND_H, S))
    assert o.dtype == dtype and torch.equal(o, plain)
    o_ref, lse_ref = SC.band_reference(model, dtype)
    check_lse(lse, lse_ref, dtype, f"band {model}")
    check_attn(o, o_ref.float(), dtype)


def test_band_lse_under_head_placement(nat):
    """heads 0 and 2 token-major: lse is in the caller's (physical) row order, the row o is written to"""
    dtype = torch.bfloat16
    F_, P_ = SC.GEOM["F_"], SC.GEOM["P_"]
    S, prm, mask, vid0 = SC.band_case("wan")
    q, k, v = SC.band_inputs("wan", dtype)
    best = torch.tensor([[1, 0, 1]])
    kw = dict(head_perm_flag=dev(best), vid0=vid0, num_frame=F_, frame_size=P_)
    bm = nat.BandMask(**prm)
    plain = nat.band_attention(dev(q), dev(k), dev(v), bm, **kw)
    o, lse = nat.band_attention(dev(q), dev(k), dev(v), bm, return_lse=True, **kw)
    _lse_ok(lse, (1, SC.BAND_H, S))
    assert torch.equal(o, plain)
    qp, kp, vp = (O.head_placement(x, best, 0, F_, P_) for x in (q, k, v))
    o_log, lse_log = SC.masked_attention_lse(qp, kp, vp, mask)
    lse_ref = O.head_placement(lse_log[..., None], best, 0, F_, P_, inverse=True)[..., 0]
    assert not torch.equal(lse_ref[0, 0], lse_log[0, 0]) and torch.equal(lse_ref[0, 1], lse_log[0, 1])
    check_lse(lse, lse_ref, dtype, "band wan, head placement")
    check_attn(o, O.head_placement(o_log, best, 0, F_, P_, inverse=True).float(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_band_lse_on_views_token_major_and_out(nat, dtype):
    """a non-contiguous view of a fused QKV projection with a token-major output; a caller's buffer"""
    S, prm, mask, _ = SC.band_case("hy")
    q, k, v = SC.band_inputs("hy", dtype)
    H, D = SC.BAND_H, SC.D
    qkv = dev(torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2))
    qv, kv_, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not qv.is_contiguous() and torch.equal(qv.cpu(), q)
    bm = nat.BandMask(**prm)
    o_ref, lse_ref = SC.band_reference("hy", dtype)
    plain = nat.band_attention(qv, kv_, vv, bm, token_major_out=True)
    o, lse = nat.band_attention(qv, kv_, vv, bm, token_major_out=True, return_lse=True)
    _lse_ok(lse, (1, H, S))
    assert o.transpose(1, 2).is_contiguous() and not o.is_contiguous() and torch.equal(o, plain)
    check_lse(lse, lse_ref, dtype, "band hy, views")
    out = torch.full_like(dev(q), float("nan"))
    plain_c = nat.band_attention(dev(q), dev(k), dev(v), bm)
    o2, lse2 = nat.band_attention(dev(q), dev(k), dev(v), bm, out=out, return_lse=True)
    assert o2 is out and torch.equal(out, plain_c) and torch.equal(out, o)
    check_lse(lse2, lse_ref, dtype, "band hy, out=")
    assert torch.equal(lse2, lse)


# ---------------------------------------------------------------------------------------------------------
# band under replay (bf16): the spike cases of tests/band_replay_cases.py, launched as tests/test_gpu_band_replay_paths.py launches them
# ---------------------------------------------------------------------------------------------------------
def _replay_cases():
    return [C.queue_case("all6"), C.queue_case("024"), C.sweep_case(132), C.ragged_case(), C.queue_case("all6").without_spikes()]


@pytest.mark.parametrize("case", _replay_cases(), ids=lambda c: c.name)
def test_band_lse_under_replay(nat, case):
    """a q-tile whose validation fails stores neither o nor lse; its replay stores both.  Only the counter is read."""
    g, kind = case.geo, case.kinds[0]
    qd, kd, vd = (O.head_placement(x, C.BEST, g.CTX, g.F, g.P, inverse=True).cuda().contiguous() for x in C.inputs(case))
    kw = dict(head_perm_flag=C.BEST.cuda(), vid0=0, num_frame=g.F, frame_size=g.P)
    bm = nat.BandMask(**g.mask_params(kind))
    nat.band_replays(reset=True)
    plain = torch.full_like(qd, float("nan"))
    nat.band_attention(qd, kd, vd, bm, out=plain, **kw)
    n_plain = nat.band_replays(reset=True)
    out = torch.full_like(qd, float("nan"))
    _, lse = nat.band_attention(qd, kd, vd, bm, out=out, return_lse=True, **kw)
    n = nat.band_replays(reset=True)
    print(f"{case.name}: replays {n} (plain entry {n_plain})")
    assert n == n_plain                               # (14 or 16 work items: both entries run the static mapping)
    if not case.spikes:
        assert n == 0
    elif case.name.startswith("queue_all6"):
        assert n == 12                                # every q-tile of real rows, both heads (tests/test_gpu_band_speculative.py)
    elif not case.name.startswith("sweep"):
        assert n > 0                                  # +400 spikes off the check points
    assert torch.equal(out, plain) and torch.isfinite(out.float()).all()
    _lse_ok(lse, (1, g.H, g.S))
    q, k, v = C.inputs(case)
    _, lse_log = SC.masked_attention_lse(q, k, v, C.bool_mask(kind, g))
    lse_ref = O.head_placement(lse_log[..., None], C.BEST, g.CTX, g.F, g.P, inverse=True)[..., 0]
    check_lse(lse, lse_ref, case.dtype, case.name)
    check_attn(O.head_placement(out.cpu(), C.BEST, g.CTX, g.F, g.P), C.oracle(case, kind), case.dtype)


# ---------------------------------------------------------------------------------------------------------
# variable block
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.VB_CASES, ids=lambda c: "-".join(str(x) for x in c))
@pytest.mark.parametrize("dtype", DTYPES)
def test_varblock_lse_matches_variant3_and_float64(nat, dtype, case):
    q, k, v, bmap, rsz, csz = SC.vb_inputs(case, dtype)
    args = [dev(x) for x in (q, k, v, bmap, rsz, csz)]
    plain = nat.varblock_attention(*args, variant=3)
    o, lse = nat.varblock_attention(*args, return_lse=True)
    _lse_ok(lse, q.shape[:-1])
    assert o.dtype == dtype and torch.equal(o, plain)
    assert torch.equal(nat.varblock_attention(*args, variant=3, return_lse=True)[1], lse)
    o_ref, lse_ref = SC.vb_reference(case, dtype)
    check_lse(lse, lse_ref, dtype, f"varblock {case}")
    check_attn(o, o_ref.float(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_varblock_lse_edge_cases(nat, dtype):
    """a block-row without active blocks, a key cluster of size 0, a block-row whose only active cluster is the empty one, and q_sizes
    that leave the last rows of every head uncovered (rows_covered=False: -inf there, zeros in o)"""
    case = SC.VB_CASES[1]
    hq, hkv, S, MB, NB, _ = case
    q, k, v, bmap, rsz, csz = (x.clone() for x in SC.vb_inputs(case, dtype))
    bmap[:, 2] = False                                  # block-row 2: no key
    csz[:, 8] += csz[:, 7]                              # key cluster 7: size 0 (its keys go to cluster 8)
    csz[:, 7] = 0
    bmap[:, 4] = False
    bmap[:, 4, 7] = True                                # block-row 4: only the empty cluster
    short = 7
    big = rsz.argmax(dim=1)
    rsz[torch.arange(hkv), big] -= short                # rows [S - 7, S) of every head: no block-row covers them
    assert (rsz > 0).all() and int(rsz[0].sum()) == S - short
    args = [dev(x) for x in (q, k, v, bmap, rsz, csz)]
    plain = nat.varblock_attention(*args, variant=3)
    o, lse = nat.varblock_attention(*args, return_lse=True)
    assert torch.equal(o, plain)
    o_ref, lse_ref = SC.vb_reference_of(q, k, v, bmap, rsz, csz)
    check_lse(lse, lse_ref, dtype, "varblock edge cases")
    check_attn(o, o_ref.float(), dtype)
    lse_c, o_c = lse.cpu(), o.float().cpu()
    g = hq // hkv
    for h in range(hkv):
        off = torch.cat((torch.zeros(1, dtype=torch.long), rsz[h].long().cumsum(0)))
        for rows in (slice(int(off[2]), int(off[3])), slice(int(off[4]), int(off[5])), slice(S - short, S)):
            assert (lse_c[h * g:(h + 1) * g, rows] == NINF).all() and (o_c[h * g:(h + 1) * g, rows] == 0).all()


def test_varblock_lse_with_row_index_arrays(nat):
    """q_row_idx / kv_row_idx: lse is in the caller's row order"""
    torch.manual_seed(5)
    H, S, D, QC, KC, dtype = 3, 3000, 128, 13, 37, torch.bfloat16
    q, k, v = (torch.randn(H, S, D).to(dtype) for _ in range(3))
    ql = torch.randint(0, QC, (H, S), dtype=torch.int32)
    kl = torch.randint(0, KC, (H, S), dtype=torch.int32)
    bmap = torch.rand(H, QC, KC) > 0.5
    bmap[:, 3] = False                                  # a q cluster without keys
    qidx, qcnt = nat.argsort_labels(dev(ql), QC)
    kidx, kcnt = nat.argsort_labels(dev(kl), KC)
    kw = dict(q_row_idx=qidx, kv_row_idx=kidx, rows_covered=True)
    plain = nat.varblock_attention(dev(q), dev(k), dev(v), dev(bmap), qcnt, kcnt, variant=3, **kw)
    o, lse = nat.varblock_attention(dev(q), dev(k), dev(v), dev(bmap), qcnt, kcnt, return_lse=True, **kw)
    _lse_ok(lse, (H, S))
    assert torch.equal(o, plain)
    for h in range(H):
        em = bmap[h][ql[h].long()][:, kl[h].long()]
        o_ref, lse_ref = SC.masked_attention_lse(q[h], k[h], v[h], em)
        assert ((lse_ref == NINF) == (ql[h] == 3)).all()
        check_lse(lse[h], lse_ref, dtype, f"varblock row index arrays, head {h}")
        check_attn(o[h], o_ref.float(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_varblock_lse_strided(nat, dtype):
    """views of a fused QKV projection, token-major output: same bits as the contiguous call"""
    case = SC.VB_CASES[1]
    q, k, v, bmap, rsz, csz = SC.vb_inputs(case, dtype)
    H, S, D = q.shape
    qkv = dev(torch.cat([x.transpose(0, 1).reshape(1, S, H * D) for x in (q, k, v)], dim=2))
    qv, kv_, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not qv.is_contiguous() and torch.equal(qv[0].cpu(), q)
    rest = [dev(x) for x in (bmap, rsz, csz)]
    o_c, lse_c = nat.varblock_attention(dev(q), dev(k), dev(v), *rest, return_lse=True)
    o, lse = nat.varblock_attention(qv, kv_, vv, *rest, token_major_out=True, return_lse=True)
    _lse_ok(lse, (1, H, S))
    assert o.transpose(1, 2).is_contiguous() and torch.equal(o[0], o_c) and torch.equal(lse[0], lse_c)
    check_lse(lse[0], SC.vb_reference(case, dtype)[1], dtype, "varblock strided")


# ---------------------------------------------------------------------------------------------------------
# the protocols: against the float64 statement of the whole, never against the code under test
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_protocol_band_over_video_keys_merged_with_dense_over_text_keys(nat, dtype):
    """(a) the first 750 rows of the hy mask over S = 790 (tests/test_sparse_attention_lse_cpu.py shows the identity in float64).  Measured on
    the MI355X, rel. L2 to the float64 statement (limit): bf16 2.83e-3 (3.43e-3; one rounding 1.66e-3), fp16 3.54e-4 (1.02e-3; 2.07e-4) —
    DESIGN 3.1.3"""
    Vn, real = SC.V, SC.REAL
    q, k, v = SC.band_inputs("hy", dtype)
    dq, dk, dv = dev(q), dev(k), dev(v)
    o_b, lse_b = nat.band_attention(dq[:, :, :Vn], dk[:, :, :Vn], dv[:, :, :Vn], nat.BandMask(**SC.VIDEO_BAND), return_lse=True)
    o_t, lse_t = nat.cross_attention(dq[:, :, :Vn], dk[:, :, Vn:real], dv[:, :, Vn:real], return_lse=True)
    o, lse = nat.merge_attention_states([o_b, o_t], [lse_b, lse_t], return_lse=True)
    o_ref, lse_ref = (x[:, :, :Vn] for x in SC.band_reference("hy", dtype))
    limit, r = merged_limit(o_ref.float(), dtype)
    err = rel_l2(o.cpu(), o_ref.float())
    print(f"protocol (a) {dtype}: merged rel_l2 {err:.3e} (limit {limit:.3e}; one rounding {r:.3e})")
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), atol=1e-2, rtol=1e-2)
    assert err <= limit, (err, limit)
    check_lse(lse, lse_ref, dtype, "protocol (a) merged", factor=2.0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_protocol_varblock_over_three_key_cluster_ranges_merged(nat, dtype):
    """(b) the block map cut into the key clusters [0, 30), [30, 71), [71, 100); block-row 0 sees keys of the first part only.  Measured on
    the MI355X, rel. L2 to the float64 statement (limit): bf16 2.82e-3 (3.43e-3; one rounding 1.66e-3), fp16 3.53e-4 (1.02e-3; 2.07e-4) —
    DESIGN 3.1.3"""
    case = SC.VB_CASES[0]
    hq, hkv, S, MB, NB, _ = case
    q, k, v, bmap, rsz, csz = SC.vb_inputs(case, dtype)
    bmap = bmap.clone()
    cuts = [0, 30, 71, NB]
    bmap[:, 0] = False
    bmap[:, 0, 3:20] = True                             # block-row 0: keys of part 0 only
    parts_map = SC.split_key_clusters(bmap, cuts)
    base = [dev(x) for x in (q, k, v)]
    parts = [nat.varblock_attention(*base, dev(b), dev(rsz), dev(csz), return_lse=True) for b in parts_map]
    o, lse = nat.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
    o_ref, lse_ref = SC.vb_reference_of(q, k, v, bmap, rsz, csz)
    limit, r = merged_limit(o_ref.float(), dtype)
    err = rel_l2(o.cpu(), o_ref.float())
    print(f"protocol (b) {dtype}: merged rel_l2 {err:.3e} (limit {limit:.3e}; one rounding {r:.3e})")
    torch.testing.assert_close(o.float().cpu(), o_ref.float(), atol=1e-2, rtol=1e-2)
    assert err <= limit, (err, limit)
    check_lse(lse, lse_ref, dtype, "protocol (b) merged", factor=2.0)
    r0 = int(rsz[0, 0])                                 # (hkv = 1) the rows of block-row 0: part 0's bits, weight 1
    assert (parts[1][1][:, :r0] == NINF).all() and (parts[2][1][:, :r0] == NINF).all()
    assert torch.equal(o[:, :r0], parts[0][0][:, :r0]) and torch.equal(lse[:, :r0], parts[0][1][:, :r0])


# ---------------------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------------------
def test_ops_sparse_attn_forward_return_lse(nat):
    """svg/kernels/ops at the smallest geometry of tests/test_gpu_bsr.py.  return_lse=True always runs the two-phase body (variant 3), so
    o has the bits of the variant-3 call; the op without it picks 128-row tiles at this size (Sq < 160 block-rows), a different schedule,
    and agrees at the tolerance of tests/test_gpu_bsr.py (the reference's own, test_sparse_attn.py:91-96)."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "sparse-videogen_amd"))
    from svg.kernels.ops import attention_ops as ops
    from svg.kernels.ops import attention_ops_wan as W

    F, L, P, heads, D, dt = 5, 16, 40, 2, 128, torch.float16
    S = F * P + L
    torch.manual_seed(F + L)
    q, k, v = (torch.randn(S, heads, D).to(dt) for _ in range(3))
    meta = ops.init_sparse_attn(L, F, P, 1.4, 1)
    for kind in ("temporal", "spatial"):
        plain = ops.sparse_attn_forward(q.cuda(), k.cuda(), v.cuda(), meta, kind)
        o, lse = ops.sparse_attn_forward(q.cuda(), k.cuda(), v.cuda(), meta, kind, return_lse=True)
        assert o.shape == (S, heads, D) and o.is_contiguous()
        _lse_ok(lse, (S, heads))
        torch.testing.assert_close(o.float(), plain.float(), rtol=5e-3, atol=5e-3)
        indptr, indices, (R, Cb) = meta.temporal_mask_metadata if kind == "temporal" else meta.spatial_mask_metadata
        bm, qs, ks = nat.bsr_to_block_map(indptr, indices, (S - L) // R, (S - L) // Cb, R, Cb, L, heads)
        qh, kh, vh = (x.cuda().permute(1, 0, 2).contiguous() for x in (q, k, v))
        assert torch.equal(o, nat.varblock_attention(qh, kh, vh, bm, qs, ks, variant=3).permute(1, 0, 2))
        em = torch.stack([O.block_mask_to_element_mask(bm[h].bool().cpu(), qs[h].cpu(), ks[h].cpu()) for h in range(heads)])
        o_ref, lse_ref = SC.masked_attention_lse(q.permute(1, 0, 2), k.permute(1, 0, 2), v.permute(1, 0, 2), em)
        check_lse(lse.permute(1, 0), lse_ref, dt, f"ops {kind}")
        check_attn(o.permute(1, 0, 2), o_ref.float(), dt)
    Fw, Pw, mul = 4, 150, 0.6
    Sw = Fw * Pw
    qw, kw_, vw = (torch.randn(Sw, heads, D).to(dt) for _ in range(3))
    wmeta = W.WanFAMetadata(Fw, Pw, W.gen_temporal_mask(Fw, Pw, mul), None)
    o, lse = W.wan_sparse_attn_forward(qw.cuda(), kw_.cuda(), vw.cuda(), wmeta, return_lse=True)
    _lse_ok(lse, (Sw, heads))
    torch.testing.assert_close(o.float(), W.wan_sparse_attn_forward(qw.cuda(), kw_.cuda(), vw.cuda(), wmeta).float(), rtol=5e-3, atol=5e-3)
    bs = W.get_factor(Fw, Pw)
    blk = torch.from_numpy(W.ref_gen_temporal_mask(Fw, Pw, mul) != -1)
    em = blk.repeat_interleave(bs, 0).repeat_interleave(bs, 1)
    o_ref, lse_ref = SC.masked_attention_lse(qw.permute(1, 0, 2), kw_.permute(1, 0, 2), vw.permute(1, 0, 2), em)
    check_lse(lse.permute(1, 0), lse_ref, dt, "ops wan")
    check_attn(o.permute(1, 0, 2), o_ref.float(), dt)
