"""The LSE / fp32 forms of the production launch forms of band attention on the GPU (include/svg_attn_band_lse_forms.h; csrc/attention.hip:
band_attn_m16_switch_kernel and band_attn_m16_queue_kernel on BandLsePolicy / BandF32Policy, the groups entries): the device switch
under either flag, the switch under replay, svg_band_attention_lse through the work queue, groups of heads under masks of their own, the
fp32 rows of each, rows without keys and rows behind real_len, and the protocol the forms exist for — a layer-call on the device switch
over the video keys merged with dense attention over the text keys, against the float64 statement of the whole.

Inputs, references and bounds are those of tests/sparse_lse_cases.py and tests/band_replay_cases.py; tests/test_band_lse_forms_cpu.py shows
the float64 identities of section 7 on the CPU.  Bit equalities are asserted where the header claims them: o against the entry without
lse, o32 rounded against o, lse of the fp32 form against lse, the queue against the static mapping, groups against one call per group.

ref: BlockSparseAttentionWrapper.run(..., return_lse=True) + a dense call with return_lse=True + merge_state,
svg/kernels/ops/attention_ops.py:178-188; the dense / sparse decision: hyvideo/attention.py:491-496."""
import contextlib
import functools

import pytest
import torch

import band_replay_cases as C
import sparse_lse_cases as SC
from oracle import svg_oracle as O
from sparse_lse_cases import DTYPES, T_SINGLE, check_lse, merged_limit, rel_l2
from test_gpu_kernels import _band_case, check_attn, dev

pytestmark = pytest.mark.gpu
NINF = float("-inf")
F_, P_, CTX = SC.GEOM["F_"], SC.GEOM["P_"], SC.GEOM["ctx"]
BEST = torch.tensor([[1, 0, 1]])          # every second head token-major
TEXT_FIRST = {"hy": False, "wan": False, "cog": True}
CTX_OF = {"hy": CTX, "wan": 0, "cog": CTX}


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def flag_of(x):
    return torch.tensor([x], dtype=torch.int32, device="cuda")


def _lse_ok(lse, shape):
    assert lse.dtype == torch.float32 and tuple(lse.shape) == tuple(shape) and lse.is_contiguous()


def _f32_matches(o32, lse32, o, lse):
    """what the header says of the _f32 forms: o32 rounded to nearest even is o, lse is bit-identical"""
    assert o32.dtype == torch.float32 and o32.is_contiguous() and o32.shape == o.shape
    assert torch.equal(o32.to(o.dtype), o) and torch.equal(lse32, lse)


# ---------------------------------------------------------------------------------------------------------
# 1. the device switch, both flags
# ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def switch_reference(model, dtype, flag):
    """float64 (o, lse) in the caller's row order.  flag 0: the model's mask in logical order, heads 0 and 2 token-major — the inputs
    carried to logical order, the result back; flag 1: the dense mask of the same real_len on the rows as they are."""
    S, prm, mask, _ = SC.band_case(model)
    q, k, v = SC.band_inputs(model, dtype)
    if flag:
        return SC.masked_attention_lse(q, k, v, O.band_mask(S, **O.dense_band_params(S, prm["real_len"])))
    pl = functools.partial(O.head_placement, best_mask_idx=BEST, context_length=CTX_OF[model], num_frame=F_, frame_size=P_,
                           text_first=TEXT_FIRST[model])
    o_log, lse_log = SC.masked_attention_lse(pl(q), pl(k), pl(v), mask)
    return pl(o_log, inverse=True), pl(lse_log[..., None], inverse=True)[..., 0]


def switch_kw(model):
    return dict(head_perm_flag=dev(BEST), vid0=SC.band_case(model)[3], num_frame=F_, frame_size=P_)


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("model", ["hy", "wan", "cog"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_switch_lse_matches_plain_switch_and_float64(nat, dtype, model, flag):
    S, prm, _, _ = SC.band_case(model)
    dq, dk, dv = (dev(x) for x in SC.band_inputs(model, dtype))
    bm, alt = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S, prm["real_len"]))
    sw, kw = flag_of(flag), switch_kw(model)
    plain = nat.band_attention_switch(dq, dk, dv, bm, alt, sw, **kw)
    o, lse = nat.band_attention_switch(dq, dk, dv, bm, alt, sw, return_lse=True, **kw)
    _lse_ok(lse, (1, SC.BAND_H, S))
    assert o.dtype == dtype and torch.equal(o, plain)
    o_ref, lse_ref = switch_reference(model, dtype, flag)
    if not flag:
        assert not torch.equal(lse_ref[0, 0], SC.band_reference(model, dtype)[1][0, 0])   # (the placement moves rows of head 0)
    check_lse(lse, lse_ref, dtype, f"switch {model} flag {flag}")
    check_attn(o, o_ref.float(), dtype)
    _f32_matches(*nat.band_attention_switch(dq, dk, dv, bm, alt, sw, return_lse=True, out_dtype=torch.float32, **kw), o, lse)


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_switch_lse_on_views_token_major(nat, dtype, flag):
    """views of a fused QKV projection with a token-major output: the bits of the contiguous call, lse contiguous [B, H, S]"""
    model = "hy"
    S, prm, _, _ = SC.band_case(model)
    q, k, v = SC.band_inputs(model, dtype)
    H, D = SC.BAND_H, SC.D
    qkv = dev(torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2))
    qv, kv_, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not qv.is_contiguous() and torch.equal(qv.cpu(), q)
    bm, alt = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S, prm["real_len"]))
    sw, kw = flag_of(flag), switch_kw(model)
    plain = nat.band_attention_switch(qv, kv_, vv, bm, alt, sw, token_major_out=True, **kw)
    o, lse = nat.band_attention_switch(qv, kv_, vv, bm, alt, sw, token_major_out=True, return_lse=True, **kw)
    _lse_ok(lse, (1, H, S))
    assert o.transpose(1, 2).is_contiguous() and not o.is_contiguous() and torch.equal(o, plain)
    o_c, lse_c = nat.band_attention_switch(dev(q), dev(k), dev(v), bm, alt, sw, return_lse=True, **kw)
    assert torch.equal(o, o_c) and torch.equal(lse, lse_c)
    check_lse(lse, switch_reference(model, dtype, flag)[1], dtype, f"switch views flag {flag}")
    _f32_matches(*nat.band_attention_switch(qv, kv_, vv, bm, alt, sw, return_lse=True, out_dtype=torch.float32, **kw), o_c, lse_c)
    out = torch.full_like(dev(q), float("nan"))
    o2, lse2 = nat.band_attention_switch(dev(q), dev(k), dev(v), bm, alt, sw, out=out, return_lse=True, **kw)
    assert o2 is out and torch.equal(out, o_c) and torch.equal(lse2, lse_c)


# ---------------------------------------------------------------------------------------------------------
# 2. the switch under replay (bf16): tests/band_replay_cases.py switch_case, launched as tests/test_gpu_band_replay_paths.py launches it
# ---------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def queue_cap(nat, cap):
    lib = nat.load()
    assert lib.svg_debug_band_queue_cap(cap) == 0
    try:
        yield
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0


@functools.lru_cache(maxsize=4)
def _device_inputs(case):
    g = case.geo
    return [O.head_placement(x, C.BEST, g.CTX, g.F, g.P, inverse=True).cuda().contiguous() for x in C.inputs(case)]


def device_inputs(case):
    """q, k, v of the case on the device: head 1 in its physical order"""
    return _device_inputs(case._replace(name=""))


def perm_kw(case):
    return dict(head_perm_flag=C.BEST.cuda(), vid0=0, num_frame=case.geo.F, frame_size=case.geo.P)


@functools.lru_cache(maxsize=None)
def replay_lse_reference(case, kind, placed):
    """float64 lse in the caller's row order: under the mask `kind` on the logical inputs, carried to the physical rows (placed), or on
    the physical inputs as they are (the alternate mask runs without the head permutation)"""
    g = case.geo
    if not placed:
        phys = [O.head_placement(x, C.BEST, g.CTX, g.F, g.P, inverse=True) for x in C.inputs(case)]
        return SC.masked_attention_lse(*phys, C.bool_mask(kind, g))[1]
    lse_log = SC.masked_attention_lse(*C.inputs(case), C.bool_mask(kind, g))[1]
    return O.head_placement(lse_log[..., None], C.BEST, g.CTX, g.F, g.P, inverse=True)[..., 0]


@pytest.mark.parametrize("flag", [0, 1])
def test_switch_lse_under_replay(nat, flag):
    """a q-tile whose validation fails stores neither o nor lse; its replay stores both: NaN-filled o comes back whole, the replays
    are those of the plain switch entry, and the +400 rows carry their spike in lse"""
    case = C.switch_case()
    g = case.geo
    q, k, v = device_inputs(case)
    mask, alt = nat.BandMask(**g.mask_params("band")), nat.BandMask(**g.mask_params("dense_real"))
    sw, kw = flag_of(flag), perm_kw(case)
    nat.band_replays(reset=True)
    plain = torch.full_like(q, float("nan"))
    nat.band_attention_switch(q, k, v, mask, alt, sw, out=plain, **kw)
    n_plain = nat.band_replays(reset=True)
    out = torch.full_like(q, float("nan"))
    _, lse = nat.band_attention_switch(q, k, v, mask, alt, sw, out=out, return_lse=True, **kw)
    n = nat.band_replays(reset=True)
    o32, lse32 = nat.band_attention_switch(q, k, v, mask, alt, sw, return_lse=True, out_dtype=torch.float32, **kw)
    n32 = nat.band_replays(reset=True)
    print(f"switch lse flag={flag}: replays={n} (plain switch entry {n_plain}; fp32 form {n32})")
    assert n == n_plain == n32 and n >= 1
    if not flag:
        assert n == 12                                # every q-tile of real rows, both heads
    assert torch.equal(out, plain) and torch.isfinite(out.float()).all()
    _lse_ok(lse, (1, g.H, g.S))
    _f32_matches(o32, lse32, out, lse)
    lse_ref = replay_lse_reference(case._replace(name=""), "dense_real" if flag else "band", not flag)
    check_lse(lse, lse_ref, case.dtype, f"switch replay flag {flag}")
    rows = sorted({s.row for s in case.spikes})       # logical rows; head 0 is contiguous: its physical rows
    spiked = lse.cpu()[0, 0, rows].double()
    assert (spiked > 200).all()                       # 400 in the log2 domain: about 277
    assert ((spiked - lse_ref[0, 0, rows]).abs() <= SC.lse_bound(lse_ref[0, 0, rows], case.dtype)).all()


# ---------------------------------------------------------------------------------------------------------
# 3. svg_band_attention_lse through the work queue
# ---------------------------------------------------------------------------------------------------------
_STATIC = {}


def static_lse_results(nat, subset):
    """cap 0, 14 work items: the static mapping -> (o, lse, replays, o32, lse32, replays of the fp32 form); once per subset"""
    if subset not in _STATIC:
        case = C.queue_case(subset)
        q, k, v = device_inputs(case)
        bm, kw = nat.BandMask(**case.geo.mask_params("band")), perm_kw(case)
        assert nat.load().svg_debug_band_queue_cap(0) == 0
        nat.band_replays(reset=True)
        o, lse = nat.band_attention(q, k, v, bm, return_lse=True, **kw)
        n = nat.band_replays(reset=True)
        o32, lse32 = nat.band_attention(q, k, v, bm, return_lse=True, out_dtype=torch.float32, **kw)
        _STATIC[subset] = (o, lse, n, o32, lse32, nat.band_replays(reset=True))
    return _STATIC[subset]


@pytest.mark.parametrize("cap", C.QUEUE_CAPS)
@pytest.mark.parametrize("subset", C.QUEUE_SUBSETS)
def test_lse_entry_through_the_queue_equals_the_static_mapping(nat, subset, cap):
    """14 work items on 1, 2 or 3 resident workgroups of band_attn_m16_queue_kernel on BandLsePolicy, replayed q-tiles among them: o and lse have
    the bits of the static mapping, and the replays are the same.  (svg_band_attention_lse_f32 has no queue form and keeps the static
    mapping under any cap: its results must not move either.)"""
    case = C.queue_case(subset)
    want = len(case.replaying_pairs())
    o_s, lse_s, n_s, o32_s, lse32_s, n32_s = static_lse_results(nat, subset)
    q, k, v = device_inputs(case)
    bm, kw = nat.BandMask(**case.geo.mask_params("band")), perm_kw(case)
    with queue_cap(nat, cap):
        nat.band_replays(reset=True)
        out = torch.full_like(q, float("nan"))
        _, lse = nat.band_attention(q, k, v, bm, out=out, return_lse=True, **kw)
        n = nat.band_replays(reset=True)
        plain = nat.band_attention(q, k, v, bm, **kw)                 # the plain entry through the same capped queue
        n_plain = nat.band_replays(reset=True)
        o32, lse32 = nat.band_attention(q, k, v, bm, return_lse=True, out_dtype=torch.float32, **kw)
        n32 = nat.band_replays(reset=True)
    print(f"queue lse {subset} cap={cap}: replays={n} (static {n_s}, plain entry {n_plain}, fp32 form {n32})")
    assert torch.equal(out, o_s) and torch.equal(lse, lse_s) and torch.equal(out, plain)
    assert torch.equal(o32, o32_s) and torch.equal(lse32, lse32_s)
    _f32_matches(o32, lse32, out, lse)
    assert n == n_s == n_plain == n32 == n32_s == want
    lse_ref = replay_lse_reference(case._replace(name=""), "band", True)
    check_lse(lse, lse_ref, case.dtype, f"queue {subset} cap {cap}")


# ---------------------------------------------------------------------------------------------------------
# 4. groups: BH = 6 as heads (2, 4), two hy masks of different text lengths
# ---------------------------------------------------------------------------------------------------------
G_LENS, G_H = (11, 29), 2                  # video 0 with 11 text keys; videos 1 and 2 with 29
G_BEST = torch.tensor([[1, 0], [0, 1], [1, 1]])


def g_masks(nat):
    S = SC.V + CTX
    prms = [_band_case("hy", **dict(SC.GEOM, L=L))[1] for L in G_LENS]
    return [nat.BandMask(**p) for p in prms], [nat.BandMask(**O.dense_band_params(S, p["real_len"])) for p in prms]


@functools.lru_cache(maxsize=None)
def g_inputs(dtype):
    g = torch.Generator().manual_seed(9)
    return tuple(torch.randn(3, G_H, SC.V + CTX, SC.D, generator=g).to(dtype) for _ in range(3))


@pytest.mark.parametrize("layout", [False, True], ids=["contiguous", "layout"])
@pytest.mark.parametrize("form", ["single", "switch0", "switch1"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_groups_lse_equals_one_call_per_group(nat, dtype, form, layout):
    q, k, v = (dev(x) for x in g_inputs(dtype))
    if layout:   # the projection layout: [cfg, S, H * D] in memory, read in place; the output comes back token-major
        q, k, v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, k, v))
        assert not q.is_contiguous()
    masks, alts = g_masks(nat)
    heads = [G_H, 2 * G_H]
    S = q.shape[2]
    kw = dict(head_perm_flag=G_BEST.cuda(), vid0=0, num_frame=F_, frame_size=P_, token_major_out=layout)
    sw = None if form == "single" else flag_of(int(form[-1]))
    gkw = dict(kw) if sw is None else dict(kw, alt_masks=alts, use_alt_flag=sw)
    plain = nat.band_attention_groups(q, k, v, masks, heads, **gkw)
    o, lse = nat.band_attention_groups(q, k, v, masks, heads, return_lse=True, **gkw)
    _lse_ok(lse, (3, G_H, S))
    assert torch.equal(o, plain) and o.stride() == plain.stride()
    if layout:
        assert o.stride() == (S * G_H * 128, 128, G_H * 128, 1)      # written in place, token-major
    gkw32 = {x: y for x, y in gkw.items() if x != "token_major_out"}
    o32, lse32 = nat.band_attention_groups(q, k, v, masks, heads, return_lse=True, out_dtype=torch.float32, **gkw32)
    _f32_matches(o32, lse32, o.contiguous(), lse)
    for g, sl in enumerate((slice(0, 1), slice(1, 3))):
        kw1 = dict(kw, head_perm_flag=G_BEST[sl].cuda())
        kw32 = {x: y for x, y in kw1.items() if x != "token_major_out"}
        if sw is None:
            one = nat.band_attention(q[sl], k[sl], v[sl], masks[g], return_lse=True, **kw1)
            one32 = nat.band_attention(q[sl], k[sl], v[sl], masks[g], return_lse=True, out_dtype=torch.float32, **kw32)
        else:
            one = nat.band_attention_switch(q[sl], k[sl], v[sl], masks[g], alts[g], sw, return_lse=True, **kw1)
            one32 = nat.band_attention_switch(q[sl], k[sl], v[sl], masks[g], alts[g], sw, return_lse=True, out_dtype=torch.float32, **kw32)
        assert torch.equal(o[sl], one[0]) and torch.equal(lse[sl], one[1]), (form, g)
        assert torch.equal(o32[sl], one32[0]) and torch.equal(lse32[sl], one32[1]), (form, g)
    # against the float64 statement, the heads the placement leaves frame-major (and every head on a dense step)
    qc, kc, vc = g_inputs(dtype)
    for b, L in enumerate((G_LENS[0], G_LENS[1], G_LENS[1])):
        S_, prm, mask, _ = _band_case("hy", **dict(SC.GEOM, L=L))
        em = O.band_mask(S, **O.dense_band_params(S, prm["real_len"])) if form == "switch1" else mask
        _, lse_ref = SC.masked_attention_lse(qc[b], kc[b], vc[b], em)
        for h in range(G_H):
            if form == "switch1" or int(G_BEST[b, h]) == 0:
                check_lse(lse[b, h], lse_ref[h], dtype, f"groups {form} video {b} head {h}")


# ---------------------------------------------------------------------------------------------------------
# 6. rows without keys, rows behind real_len
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_behind_real_len_and_rows_without_keys(nat, dtype):
    """hy (real_len 761 < S 790): the rows behind real_len attend to their own segment, finite lse.  A cog-style mask whose band is 0
    and that names no full column: the text rows see every key, a video row sees none — o = 0, lse = -inf, under the switch with flag 0;
    flag 1 (the dense mask) gives the same rows their keys back."""
    S, prm, _, _ = SC.band_case("hy")
    dq, dk, dv = (dev(x) for x in SC.band_inputs("hy", dtype))
    real = prm["real_len"]
    bm, alt = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S, real))
    for flag in (0, 1):
        o, lse = nat.band_attention_switch(dq, dk, dv, bm, alt, flag_of(flag), return_lse=True, **switch_kw("hy"))
        pad = lse[..., real:].cpu()
        assert real < S and torch.isfinite(pad).all()
        q, k, v = (x[:, :, real:] for x in SC.band_inputs("hy", dtype))
        o_pad, lse_pad = SC.masked_attention_lse(q, k, v, None)
        check_lse(pad, lse_pad, dtype, f"rows behind real_len, flag {flag}")
        check_attn(o[:, :, real:], o_pad.float(), dtype)
    S, prm, _, vid0 = SC.band_case("cog")
    dq, dk, dv = (dev(x) for x in SC.band_inputs("cog", dtype))
    prm0 = dict(prm, band=0, colfull_lo=0, colfull_hi=0)
    bm, alt = nat.BandMask(**prm0), nat.BandMask(**O.dense_band_params(S))
    em = O.band_mask(S, **prm0)
    assert vid0 == CTX and em[:vid0].all() and not em[vid0:].any()
    kw = switch_kw("cog")
    plain = nat.band_attention_switch(dq, dk, dv, bm, alt, flag_of(0), **kw)
    o, lse = nat.band_attention_switch(dq, dk, dv, bm, alt, flag_of(0), return_lse=True, **kw)
    assert torch.equal(o, plain)
    assert (lse[..., vid0:] == NINF).all() and (o[:, :, vid0:] == 0).all()
    o_ref, lse_ref = SC.masked_attention_lse(*SC.band_inputs("cog", dtype), em)
    check_lse(lse, lse_ref, dtype, "rows without keys")     # (the placement permutes video rows only: all of them -inf)
    check_attn(o, o_ref.float(), dtype)
    o32, lse32 = nat.band_attention_switch(dq, dk, dv, bm, alt, flag_of(0), return_lse=True, out_dtype=torch.float32, **kw)
    _f32_matches(o32, lse32, o, lse)
    assert (o32[:, :, vid0:] == 0).all()
    _, lse1 = nat.band_attention_switch(dq, dk, dv, bm, alt, flag_of(1), return_lse=True, **kw)
    assert torch.isfinite(lse1).all()
    # the same mask through the groups entry and through the single-mask entry (the queue rule)
    og, lseg = nat.band_attention_groups(dq, dk, dv, [bm, bm], [1, 2], return_lse=True, **kw)
    ob, lseb = nat.band_attention(dq, dk, dv, bm, return_lse=True, **kw)
    assert torch.equal(og, o) and torch.equal(lseg, lse) and torch.equal(ob, o) and torch.equal(lseb, lse)


# ---------------------------------------------------------------------------------------------------------
# 7. the protocol: a layer-call on the device switch over the video keys + dense attention over the text keys, merged
# ---------------------------------------------------------------------------------------------------------
def _protocol_reference(q, k, v, L, best, flag):
    """float64 statement of the whole for the video rows of one video [H, S, D] with L text keys, in the caller's row order: the hy mask
    (flag 0; a token-major head sees its band in token-major order, the text keys are outside the placement) or dense attention over the
    real keys (flag 1)"""
    Vn = SC.V
    S, prm, mask, _ = _band_case("hy", **dict(SC.GEOM, L=L))
    real = Vn + L
    if flag:
        return SC.masked_attention_lse(q[:, :Vn], k[:, :real], v[:, :real], None)
    pl = functools.partial(O.head_placement, best_mask_idx=best[None], context_length=CTX, num_frame=F_, frame_size=P_)
    o_log, lse_log = SC.masked_attention_lse(pl(q[None]), pl(k[None]), pl(v[None]), mask)
    return pl(o_log, inverse=True)[0, :, :Vn], pl(lse_log[..., None], inverse=True)[0, :, :Vn, 0]


@pytest.mark.parametrize("flag", [0, 1])
@pytest.mark.parametrize("groups", [False, True], ids=["one_mask", "two_groups"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_protocol_device_switch_over_video_keys_merged_with_text_keys(nat, dtype, groups, flag):
    """The hy geometry (750 video keys, 40 text slots).  Video rows: _core.svg1_attention_device_switch(return_lse=True) over the video keys
    under VIDEO_BAND (dense step: every video key), cross attention over the text keys, merge_attention_states — against the float64
    statement of the whole: within merged_limit with 16-bit parts, within T_SINGLE, the bound of one call, with fp32 parts.
    two_groups: two videos with 11 and 29 text keys.  The band over the video keys does not depend on the text length, so their two masks
    differ only in where an EMPTY interval of full columns sits: equal masks would be merged into one group by _core.video_groups, these
    run as two launches of svg_band_groups_attention_lse; the text keys of each video are its window of svg_cross_attention_keyrange.
    Measured on the MI355X, rel. L2 to the float64 statement, 16-bit parts (limit) / fp32 parts (limit T_SINGLE): bf16 2.81e-3 ... 2.84e-3
    (3.43e-3) / 2.26e-3 ... 2.32e-3 (3e-3); fp16 3.52e-4 ... 3.57e-4 (1.02e-3) / 2.84e-4 ... 2.90e-4 (1e-3) — DESIGN 3.1.3."""
    from svg.models import _core
    from svg.models.wan.utils import profile_desc

    Vn = SC.V
    lens = G_LENS if groups else (SC.GEOM["L"],)
    H = SC.BAND_H
    if groups:
        gen = torch.Generator().manual_seed(21)
        q, k, v = (torch.randn(2, H, Vn + CTX, SC.D, generator=gen).to(dtype) for _ in range(3))
    else:
        q, k, v = SC.band_inputs("hy", dtype)
    dq, dk, dv = dev(q), dev(k), dev(v)
    geo, prof = _core.Geometry(0, F_, P_), profile_desc(0, F_, P_)
    band = [nat.BandMask(**dict(SC.VIDEO_BAND, colfull_lo=b, colfull_hi=b)) for b in range(len(lens))]
    dense = nat.BandMask(**O.dense_band_params(Vn))
    kv_end = torch.tensor(lens, dtype=torch.int32, device="cuda")
    sw = flag_of(flag)
    res = {}
    for name, kw in (("16-bit parts", dict()), ("fp32 parts", dict(out_dtype=torch.float32))):
        torch.manual_seed(0)
        _core.reseed_switch_generator()
        o_b, best, lse_b = _core.svg1_attention_device_switch(dq[:, :, :Vn], dk[:, :, :Vn], dv[:, :, :Vn], geo, band if groups else band[0],
                                                              dense, prof, 16, Vn, sw, return_lse=True, **kw)
        o_t, lse_t = nat.cross_attention_keyrange(dq[:, :, :Vn], dk[:, :, Vn:], dv[:, :, Vn:], kv_end, return_lse=True, **kw)
        res[name] = (nat.merge_attention_states([o_b, o_t], [lse_b, lse_t], return_lse=True, out_dtype=dtype if kw else None), best)
    (o16, lse16), best = res["16-bit parts"]
    (o32, lse32), best32 = res["fp32 parts"]
    assert torch.equal(best, best32) and bool((best == -1).all()) == bool(flag)
    # the placement the profiler chose, as the kernel saw it (flag 0); plain call: the same best_mask_idx, no state
    torch.manual_seed(0)
    _core.reseed_switch_generator()
    o_plain, best_plain = _core.svg1_attention_device_switch(dq[:, :, :Vn], dk[:, :, :Vn], dv[:, :, :Vn], geo, band if groups else band[0],
                                                             dense, prof, 16, Vn, sw)
    assert torch.equal(best_plain, best)
    refs = [_protocol_reference(q[b], k[b], v[b], L, best[b].cpu().clamp(min=0), flag) for b, L in enumerate(lens)]
    o_ref, lse_ref = torch.stack([r[0] for r in refs]), torch.stack([r[1] for r in refs])
    limit, r = merged_limit(o_ref.float(), dtype)
    e16, e32 = rel_l2(o16.cpu(), o_ref.float()), rel_l2(o32.cpu(), o_ref.float())
    print(f"protocol switch flag={flag} groups={groups} {dtype}: 16-bit parts rel_l2 {e16:.3e} (limit {limit:.3e}; one rounding {r:.3e}), "
          f"fp32 parts {e32:.3e} (limit {T_SINGLE[dtype]:.1e}); token-major heads {int((best == 1).sum())}")
    torch.testing.assert_close(o16.float().cpu(), o_ref.float(), atol=1e-2, rtol=1e-2)
    assert e16 <= limit, (e16, limit)
    assert e32 <= T_SINGLE[dtype], (e32, T_SINGLE[dtype])
    check_lse(lse16, lse_ref, dtype, "protocol merged, 16-bit parts", factor=2.0)
    check_lse(lse32, lse_ref, dtype, "protocol merged, fp32 parts", factor=2.0)
