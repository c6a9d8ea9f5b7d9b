"""SVG1's per-head band width on the GPU (include/svg_attn_adaptive_band.h): band attention from a device vector of bands against
svg_band_attention_lse head by head, bit for bit; its device switch; the float64 statement under the per-head element mask; the controller
kernel against its law; the loop closed in svg1_attention_device_switch and in the SVG1 processors of HunyuanVideo and Wan.

Bounds, none of them from the code under test: o and lse are compared for EQUALITY with the entries they restate; against float64 by the
project's check_attn (T_SINGLE) and check_lse, every row; kept by the rule of tests/test_gpu_adaptive_top_p.py (fp64 arithmetic rounded
once: 1 fp32 ulp beside the float64 statement rounded to fp32); the band EXACTLY the fp32 law (tests/adaptive_band_cases.py law32) on
the kept bits the kernel wrote.  Geometry: tests/sparse_lse_cases.py (F = 5, P = 150, ctx = 40, L = 11), 4 heads."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import adaptive_band_cases as BC
import adaptive_top_p_cases as AC
import kept_mass_cases as KM
import sparse_lse_cases as SC
from oracle import svg_oracle as O
from poisoned import load_native, unwritten
from sparse_lse_cases import DTYPES, check_lse
from test_gpu_kernels import check_attn, dev

pytestmark = pytest.mark.gpu
DT = torch.bfloat16
F_, P_, CTX = SC.GEOM["F_"], SC.GEOM["P_"], SC.GEOM["ctx"]
H = BC.H
MODELS = SC.BAND_MODELS
PERMS = {"logical": None, "one_token_major": [0, 0, 1, 0]}


@pytest.fixture(scope="module")
def nat():
    return load_native()


@pytest.fixture(scope="module")
def ab(nat):
    from svg import _adaptive_band

    return _adaptive_band


def i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


def perm_kw(model, perm):
    if PERMS[perm] is None:
        return {}
    return dict(head_perm_flag=dev(torch.tensor([PERMS[perm]])), vid0=SC.band_case(model)[3], num_frame=F_, frame_size=P_)


@functools.lru_cache(maxsize=None)
def device_inputs(model, dtype):
    return tuple(dev(x) for x in BC.inputs(model, dtype))


@functools.lru_cache(maxsize=None)
def head_by_head(model, dtype, perm, bands):
    """(o, lse) of svg_band_attention_lse called on every head ALONE with mask.band = bands[h] (clamped as the kernel clamps)"""
    from svg import _native as nat

    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    kw = perm_kw(model, perm)
    os_, ls_ = [], []
    for h, b in enumerate(bands):
        kwh = dict(kw, head_perm_flag=kw["head_perm_flag"][:, h:h + 1].contiguous()) if kw else {}
        o, lse = nat.band_attention(q[:, h:h + 1], k[:, h:h + 1], v[:, h:h + 1], nat.BandMask(**dict(prm, band=BC.clamp_band(b, S))),
                                    return_lse=True, **kwh)
        os_.append(o), ls_.append(lse)
    return torch.cat(os_, dim=1), torch.cat(ls_, dim=1)


def projection_views(q, k, v):
    """q, k, v as views of one fused QKV projection output [1, S, 3 H D]"""
    S, D = q.shape[2], q.shape[3]
    qkv = torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2).contiguous()
    views = tuple(qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not views[0].is_contiguous() and torch.equal(views[0], q)
    return views


def written(o, lse):
    assert not bool(unwritten(o).any()) and not bool(unwritten(lse).any()), "words of o / lse left unwritten (poisoned)"


# ---------------------------------------------------------------------------------------------------------
# 1. per-head bits, 2. uniform band, 3. clamp
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous", "projection"])
@pytest.mark.parametrize("perm", list(PERMS))
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_head_has_the_bits_of_the_single_mask_entry_under_its_band(nat, ab, dtype, model, perm, layout):
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    if layout == "projection":
        q, k, v = projection_views(q, k, v)
    for name, bands in BC.band_sets(S).items():
        o, lse = ab.band_attention_per_head(q, k, v, nat.BandMask(**prm), i32(bands), token_major_out=layout == "projection",
                                            **perm_kw(model, perm))
        assert lse.dtype == torch.float32 and tuple(lse.shape) == (1, H, S) and lse.is_contiguous() and o.dtype == dtype
        assert (layout == "projection") == (not o.is_contiguous())
        written(o, lse)
        o_ref, lse_ref = head_by_head(model, dtype, perm, tuple(bands))
        for h in range(H):
            assert torch.equal(o[:, h], o_ref[:, h]), (name, h, bands[h])
            assert torch.equal(lse[:, h], lse_ref[:, h]), (name, h, bands[h])


@pytest.mark.parametrize("perm", list(PERMS))
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_uniform_band_equals_one_call_of_the_single_mask_entry(nat, ab, dtype, model, perm):
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    bm = nat.BandMask(**prm)
    o_ref, lse_ref = nat.band_attention(q, k, v, bm, return_lse=True, **perm_kw(model, perm))
    o, lse = ab.band_attention_per_head(q, k, v, bm, i32([prm["band"]] * H), **perm_kw(model, perm))
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)
    assert torch.equal(ab.band_attention_per_head(q, k, v, bm, i32([prm["band"]] * H), return_lse=False, **perm_kw(model, perm)), o_ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_kernel_clamps_the_band(nat, ab, dtype):
    model = "hy"
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    o, lse = ab.band_attention_per_head(q, k, v, nat.BandMask(**prm), i32([0, -5, 2 ** 30, 129]), **perm_kw(model, "one_token_major"))
    o_ref, lse_ref = head_by_head(model, dtype, "one_token_major", (1, 1, S + 1, 129))
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref)


# ---------------------------------------------------------------------------------------------------------
# 4. the switch form
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous", "projection"])
@pytest.mark.parametrize("model", ["hy", "wan", "cog"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_switch_form_under_either_flag(nat, ab, dtype, model, layout):
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    bm, alt = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S, prm["real_len"]))
    kw = perm_kw(model, "one_token_major")
    bands = BC.band_sets(S)["wide"]
    band = i32(bands)
    # flag 1: the alternate mask as it is, the bits of svg_band_attention_switch_lse under that flag; band ignored
    o_alt, lse_alt = nat.band_attention_switch(q, k, v, bm, alt, i32([1]), return_lse=True, **kw)
    if layout == "projection":
        q, k, v = projection_views(q, k, v)
    tm = layout == "projection"
    o1, lse1 = ab.band_attention_switch_per_head(q, k, v, bm, alt, i32([1]), band, token_major_out=tm, **kw)
    written(o1, lse1)
    assert torch.equal(o1, o_alt) and torch.equal(lse1, lse_alt)
    # flag 0: the per-head form
    o0, lse0 = ab.band_attention_switch_per_head(q, k, v, bm, alt, i32([0]), band, token_major_out=tm, **kw)
    written(o0, lse0)
    o_ref, lse_ref = head_by_head(model, dtype, "one_token_major", tuple(bands))
    assert torch.equal(o0, o_ref) and torch.equal(lse0, lse_ref)
    assert not torch.equal(o0, o1)
    assert band.tolist() == bands                                   # neither flag writes the band vector


# ---------------------------------------------------------------------------------------------------------
# 5. against float64 under the per-head element mask: the project's bounds, every row
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_against_float64_under_the_per_head_element_mask(nat, ab, dtype, model):
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, dtype)
    for name, bands in BC.band_sets(S).items():
        o, lse = ab.band_attention_per_head(q, k, v, nat.BandMask(**prm), i32(bands))
        o_ref, lse_ref = BC.reference(model, dtype, tuple(bands))
        check_lse(lse, lse_ref, dtype, f"per-head {model} {name}")
        for h in range(H):                                          # (head by head: no head hides behind another's norm)
            check_attn(o[:, h:h + 1], o_ref[:, h:h + 1].float(), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_against_float64_with_a_token_major_head(nat, ab, dtype):
    model = "hy"
    S, prm, _, _ = SC.band_case(model)
    q, k, v = BC.inputs(model, dtype)
    bands = BC.band_sets(S)["wide"]
    best = torch.tensor([PERMS["one_token_major"]])
    pl = functools.partial(O.head_placement, best_mask_idx=best, context_length=CTX, num_frame=F_, frame_size=P_, text_first=False)
    qp, kp, vp = pl(q), pl(k), pl(v)
    parts = [SC.masked_attention_lse(qp[:, h:h + 1], kp[:, h:h + 1], vp[:, h:h + 1], BC.element_mask(model, b)) for h, b in enumerate(bands)]
    o_ref = pl(torch.cat([p[0] for p in parts], dim=1), inverse=True)
    lse_ref = pl(torch.cat([p[1] for p in parts], dim=1)[..., None], inverse=True)[..., 0]
    o, lse = ab.band_attention_per_head(*device_inputs(model, dtype), nat.BandMask(**prm), i32(bands), **perm_kw(model, "one_token_major"))
    check_lse(lse, lse_ref, dtype, "per-head hy, head 2 token-major")
    for h in range(H):
        check_attn(o[:, h:h + 1], o_ref[:, h:h + 1].float(), dtype)


# ---------------------------------------------------------------------------------------------------------
# 6. the controller
# ---------------------------------------------------------------------------------------------------------
LAW = dict(target=0.9, gain_up=16.0, gain_down=16.0, dead=0.02, quantum=128, band_min=128, band_max=768)


def controller_case(R):
    """7 heads over S = 790: far below target (up, to band_max), everything kept (down, to band_min), a -inf row, a NaN head, a head in the
    dead zone, one just below target (a small step up), one above the dead zone (a small step down)"""
    BHu, S = 7, 790
    delta = torch.zeros(BHu, R)
    delta[0] = 5.0                                              # keeps < 1 %
    delta[1] = 0.0                                              # keeps everything
    delta[2] = 0.05
    delta[4] = -math.log(0.91)                                  # kept 0.91: inside the dead zone [0.9, 0.92]
    delta[5] = -math.log(0.80)                                  # kept 0.80: e = 0.1 -> 1.6 quanta -> 2
    delta[6] = -math.log(0.99)                                  # kept 0.99: e + dead = -0.07 -> -1.12 quanta -> -1
    rows, ls, ld = KM.controller_inputs(200 + R, BHu, S, R, lambda g: delta)    # (head 2: a -inf row, head 3: NaN)
    band0 = [384, 128, 256, 640, 512, 384, 768]
    return S, rows, ls, ld, band0


def run_controller(nat, R, law=LAW, skip=None, rows=None, band0=None):
    S, rows0, ls, ld, b0 = controller_case(R)
    rows = rows0 if rows is None else rows
    band = i32(b0 if band0 is None else band0)
    kept = nat.empty((band.numel(),), dtype=torch.float32, device="cuda")
    nat.band_width_update(ls.cuda(), torch.tensor(rows).cuda(), ld.cuda(), band, kept, law["target"], law["gain_up"], law["gain_down"],
                          law["dead"], law["quantum"], law["band_min"], law["band_max"], skip_flag=skip)
    return kept.cpu(), band.cpu()


@pytest.mark.parametrize("R", [1, 17, 64])
def test_controller_kept_mass_and_the_exact_law(nat, R):
    S, rows, ls, ld, band0 = controller_case(R)
    kept, band = run_controller(nat, R)
    fin = [h for h in range(7) if h != 3]
    assert math.isnan(float(kept[3])) and torch.isfinite(kept[fin]).all(), kept          # every word written (poisoned: NaN bits of all ones)
    assert not bool(unwritten(kept).any())
    ref_kept = AC.kept_mass(ls.numpy(), rows, ld.numpy())
    uk = AC.ulps32(kept.numpy()[fin], ref_kept[fin].astype(np.float32))
    print(f"R={R} kept {kept.tolist()} float64 {ref_kept.tolist()} ulps {uk.tolist()}")
    assert (uk <= 1).all()
    if R == 1:
        assert float(kept[2]) == 0.0                                                     # the -inf row added nothing
    want = BC.law32(band0, kept.numpy(), **LAW)
    print(f"R={R} band {band0} -> {band.tolist()} law {want.tolist()}")
    assert band.tolist() == want.tolist()                                                # exact, no head excluded
    assert band[0] == LAW["band_max"] and band[1] == LAW["band_min"]                     # both clamps reached
    assert band[3] == band0[3]                                                           # the NaN head: unchanged
    assert band[4] == band0[4]                                                           # the dead zone
    assert band[5] == band0[5] + 2 * 128 and band[6] == band0[6] - 128                  # a step up, a step down
    assert (band.numpy() == BC.law64(band0, kept.numpy().astype(np.float64), **LAW)).all()   # (no case here sits on a rounding boundary)
    kept2, band2 = run_controller(nat, R)                                                # the same call: the same bits
    assert torch.equal(kept2.view(torch.int32), kept.view(torch.int32)) and torch.equal(band2, band)


def test_controller_skip_flag_out_of_range_row_and_zero_gains(nat):
    S, rows, ls, ld, band0 = controller_case(17)
    kept_ref, _ = run_controller(nat, 17)
    kept, band = run_controller(nat, 17, skip=i32([1]))                                  # a dense step: kept written, no band moves
    assert band.tolist() == band0 and torch.equal(kept.view(torch.int32), kept_ref.view(torch.int32))
    kept, band = run_controller(nat, 17, skip=i32([0]))                                  # the flag at zero: as without
    assert band.tolist() == BC.law32(band0, kept.numpy(), **LAW).tolist() and band.tolist() != band0
    for bad in (S, -1):                                                                  # a row outside [0, S): kept NaN, band unchanged
        kept, band = run_controller(nat, 17, rows=rows[:5] + [bad] + rows[6:])
        assert torch.isnan(kept).all() and band.tolist() == band0
    kept, band = run_controller(nat, 17, law=dict(LAW, gain_up=0.0, gain_down=0.0))      # zero gains move nothing
    assert band.tolist() == band0 and torch.equal(kept.view(torch.int32), kept_ref.view(torch.int32))
    # a vector that holds anything at all is clamped, never wrapped
    kept, band = run_controller(nat, 17, band0=[2 ** 31 - 1, -2 ** 31, 0, 5, 384, 384, 384])
    assert band.tolist() == BC.law32([2 ** 31 - 1, -2 ** 31, 0, 5, 384, 384, 384], kept.numpy(), **LAW).tolist()
    rest = band[[0, 1, 2, 4, 5, 6]]                                                      # (head 3 has no measurement: its 5 stays)
    assert LAW["band_min"] <= int(rest.min()) and int(rest.max()) <= LAW["band_max"] and band[3] == 5


# ---------------------------------------------------------------------------------------------------------
# 7. the loop closed in svg1_attention_device_switch: a local head and a diffuse head
# ---------------------------------------------------------------------------------------------------------
def loop_inputs():
    """Wan geometry (no text), 4 heads: heads 0, 1 local — q is the key of its own row plus noise, scaled so that the row's own key holds
    nearly all the mass —, heads 2, 3 diffuse (independent q and k of small norm: every key weighs about the same)"""
    S, D = F_ * P_, SC.D
    g = torch.Generator().manual_seed(41)
    k = torch.randn(1, H, S, D, generator=g)
    q = torch.randn(1, H, S, D, generator=g) * 0.3
    q[:, :2] = k[:, :2] * 3.0 + torch.randn(1, 2, S, D, generator=g) * 0.1
    v = torch.randn(1, H, S, D, generator=g)
    return tuple(x.to(DT).cuda() for x in (q, k, v))


def loop_call(nat, q, k, v, seed, **kw):
    from svg.models import _core
    from svg.models.wan.utils import generate_temporal_head_mask_mod as wan_mm, profile_desc

    geo = _core.Geometry(0, F_, P_, text_first=False)
    S = geo.seq_len
    mask = wan_mm(0, 0, F_, P_, mul=1.2)
    torch.manual_seed(seed)
    _core.reseed_switch_generator(seed)
    _core.reseed_probe_generator(seed)
    outs = []
    for _ in range(3):
        outs.append(_core.svg1_attention_device_switch(q, k, v, geo, mask, nat.BandMask(**O.dense_band_params(S)), profile_desc(0, F_, P_), 16,
                                                       400, i32([0]), **kw))
    return outs, mask, S


def test_closed_loop_follows_the_law_and_zero_gains_change_nothing(nat, monkeypatch):
    from svg.models import _core

    q, k, v = loop_inputs()
    plain, mask, S = loop_call(nat, q, k, v, 9)
    # zero gains: the output of the plain call, a constant store
    store = _core.BandStore()
    zero = _core.AdaptiveBand(0.9, gain_up=0.0, gain_down=0.0, quantum=64)
    outs, _, _ = loop_call(nat, q, k, v, 9, adaptive=zero, band_store=store, layer_idx=7)
    for (o0, b0), (o1, b1) in zip(plain, outs):
        assert torch.equal(o0, o1) and torch.equal(b0, b1)
    assert store.band[7].tolist() == [mask.band] * H and store.band[7].dtype == torch.int32
    kept = store.kept[7].cpu()
    print(f"zero gains: kept {kept.tolist()} at band {mask.band}")
    assert kept.shape == (H,) and bool(((kept > 0) & (kept <= 1 + 1e-4)).all())
    # gains: after each call the store is the law on the logged kept mass, exactly
    law = dict(target=0.9, gain_up=16.0, gain_down=32.0, dead=0.02, quantum=64)
    trace, orig_step = [], _core.adaptive_band_step

    def spy(adaptive, st, layer, band, *a, **kw):
        before = band.clone()
        orig_step(adaptive, st, layer, band, *a, **kw)
        trace.append((before.cpu(), st.kept[layer].cpu().clone(), band.cpu().clone()))

    monkeypatch.setattr(_core, "adaptive_band_step", spy)
    store = _core.BandStore()
    ad = _core.AdaptiveBand(**law)
    lo, hi = ad.bounds(mask.band, S)
    loop_call(nat, q, k, v, 9, adaptive=ad, band_store=store, layer_idx=7)
    assert len(trace) == 3 and trace[0][0].tolist() == [mask.band] * H
    for i, (before, kept, after) in enumerate(trace):
        want = BC.law32(before.numpy(), kept.numpy(), band_min=lo, band_max=hi, **law)
        print(f"call {i}: band {before.tolist()} kept {kept.tolist()} -> {after.tolist()}")
        assert after.tolist() == want.tolist()
        if i:
            assert torch.equal(before, trace[i - 1][2])                                  # the state carries from call to call
    assert torch.equal(store.band[7].cpu(), trace[-1][2])
    end = trace[-1][2]
    assert bool((end[:2] < mask.band).all()), "the local heads keep their mass in a narrower band"
    assert bool((end[2:] > mask.band).all()), "the diffuse heads are starved at the mask's band"
    assert all((int(b) - mask.band) % 64 == 0 for b in end)                              # the residue survives


def sparse_loop_call(nat, q, k, v, seed, **kw):
    """three calls of svg1_sparse_attention — the host-side branch: no flag, the profiler's rows from the global CPU stream"""
    from svg.models import _core
    from svg.models.wan.utils import generate_temporal_head_mask_mod as wan_mm, profile_desc

    geo = _core.Geometry(0, F_, P_, text_first=False)
    mask = wan_mm(0, 0, F_, P_, mul=1.2)
    torch.manual_seed(seed)
    _core.reseed_probe_generator(seed)
    outs = [_core.svg1_sparse_attention(q, k, v, geo, mask, profile_desc(0, F_, P_), 16, 400, **kw) for _ in range(3)]
    return outs, mask, geo.seq_len, torch.get_rng_state()


def test_closed_loop_through_the_host_side_branch(nat, monkeypatch):
    """svg1_sparse_attention(adaptive=...): svg_band_attention_per_head_lse and the controller without a skip flag"""
    from svg.models import _core

    q, k, v = loop_inputs()
    plain, mask, S, rng0 = sparse_loop_call(nat, q, k, v, 9)
    store = _core.BandStore()
    zero = _core.AdaptiveBand(0.9, gain_up=0.0, gain_down=0.0, quantum=64)
    outs, _, _, rng1 = sparse_loop_call(nat, q, k, v, 9, adaptive=zero, band_store=store, layer_idx=2)
    for (o0, b0), (o1, b1) in zip(plain, outs):
        assert torch.equal(o0, o1) and torch.equal(b0, b1)
    assert torch.equal(rng0, rng1)                                                       # the probe's rows leave the global stream alone
    assert store.band[2].tolist() == [mask.band] * H and store.kept[2].shape == (H,)
    with_lse, _, _, _ = sparse_loop_call(nat, q, k, v, 9, adaptive=zero, band_store=_core.BandStore(), layer_idx=2, return_lse=True)
    ref_lse, _, _, _ = sparse_loop_call(nat, q, k, v, 9, return_lse=True)
    for a, b in zip(with_lse, ref_lse):
        assert len(a) == 3 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    law = dict(target=0.9, gain_up=16.0, gain_down=32.0, dead=0.02, quantum=64)
    trace, orig_step = [], _core.adaptive_band_step

    def spy(adaptive, st, layer, band, *a, **kw):
        assert kw.get("skip_flag") is None                                               # every call of this branch is a sparse step
        before = band.clone()
        orig_step(adaptive, st, layer, band, *a, **kw)
        trace.append((before.cpu(), st.kept[layer].cpu().clone(), band.cpu().clone()))

    monkeypatch.setattr(_core, "adaptive_band_step", spy)
    store = _core.BandStore()
    ad = _core.AdaptiveBand(**law)
    lo, hi = ad.bounds(mask.band, S)
    sparse_loop_call(nat, q, k, v, 9, adaptive=ad, band_store=store, layer_idx=2)
    assert len(trace) == 3 and trace[0][0].tolist() == [mask.band] * H
    for i, (before, kept, after) in enumerate(trace):
        print(f"host branch, call {i}: band {before.tolist()} kept {kept.tolist()} -> {after.tolist()}")
        assert after.tolist() == BC.law32(before.numpy(), kept.numpy(), band_min=lo, band_max=hi, **law).tolist()
        if i:
            assert torch.equal(before, trace[i - 1][2])
    end = trace[-1][2]
    assert torch.equal(store.band[2].cpu(), end) and bool((end[:2] < mask.band).all()) and bool((end[2:] > mask.band).all())


# ---------------------------------------------------------------------------------------------------------
# 8. the processors, through the stand-in attention modules
# ---------------------------------------------------------------------------------------------------------
def wan_module(monkeypatch):
    from standins import Attention
    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanP
    from svg.models.wan.utils import generate_temporal_head_mask_mod as wan_mm

    for name, val in dict(context_length=0, num_frame=F_, frame_size=P_, first_layers_fp=0, first_times_fp=900.0, num_sampled_rows=16,
                          sample_mse_max_row=400, block_mask=wan_mm(0, 0, F_, P_, mul=1.2), quality_rows=64, quality_log=None,
                          adaptive_band=None).items():
        monkeypatch.setattr(WanP, name, val, raising=False)
    WanP.reset_state()
    torch.manual_seed(1)
    dim, S = H * SC.D, F_ * P_
    attn = Attention(dim, H, qk_norm="rms", across_heads=True, dtype=DT).cuda()
    hidden = (torch.randn(1, S, dim) * 0.3).to(DT).cuda()
    ang = torch.rand(S, SC.D // 2) * 6.28
    kw = dict(rotary_emb=(ang.cos().cuda(), ang.sin().cuda()))
    return WanP, attn, (hidden,), kw


def hy_module(monkeypatch):
    from standins import Attention
    from svg.models.hyvideo.attention import Hunyuan_SVGAttn_Processor2_0 as HyP
    from svg.models.hyvideo.utils import generate_temporal_head_mask_mod as hy_mm
    from test_gpu_processors import rope_tables

    L, V = SC.GEOM["L"], F_ * P_
    for name, val in dict(context_length=CTX, num_frame=F_, frame_size=P_, prompt_length=L, block_mask=hy_mm(CTX, L, F_, P_, mul=1.2),
                          first_layers_fp=0, first_times_fp=900.0, num_sampled_rows=16, sample_mse_max_row=V, quality_log=None,
                          quality_rows=64, adaptive_band=None).items():
        monkeypatch.setattr(HyP, name, val, raising=False)
    HyP.reset_state()
    torch.manual_seed(2)
    dim = H * SC.D
    attn = Attention(dim, H, added_kv=True, dtype=DT).cuda()
    hidden = (torch.randn(1, V, dim) * 0.3).to(DT).cuda()
    enc = (torch.randn(1, CTX, dim) * 0.3).to(DT).cuda()
    amask = torch.zeros(1, V + CTX, dtype=torch.bool)
    amask[:, :V + L] = True
    kw = dict(encoder_hidden_states=enc, attention_mask=amask.cuda(), image_rotary_emb=rope_tables(V, SC.D))
    return HyP, attn, (hidden,), kw


def module_calls(cls, attn, args, kw, layer, n=3, timestep=100.0, seed=13):
    from svg.models import _core

    attn.set_processor(cls(layer))
    torch.manual_seed(seed)
    _core.reseed_switch_generator(seed)
    _core.reseed_probe_generator(seed)
    outs, bests = [], []
    with torch.no_grad():
        for _ in range(n):
            out = attn(*args, timestep=torch.tensor([timestep]).cuda(), **kw)
            outs.append(out if torch.is_tensor(out) else out[0])
            bests.append(attn.processor.last_best_mask_idx.clone())
    return outs, bests


@pytest.mark.parametrize("make", [wan_module, hy_module], ids=["wan", "hunyuan"])
def test_processors(nat, monkeypatch, tmp_path, make):
    from svg import _probe
    from svg.models import _core

    cls, attn, args, kw = make(monkeypatch)
    base, best0 = module_calls(cls, attn, args, kw, 3)
    assert not cls.band_store.band                                                      # None: the store is never touched
    # zero gains: the same output, a constant store
    monkeypatch.setattr(cls, "adaptive_band", _core.AdaptiveBand(0.9, gain_up=0.0, gain_down=0.0))
    outs, best1 = module_calls(cls, attn, args, kw, 3)
    for a, b, c, d in zip(base, outs, best0, best1):
        assert torch.equal(a, b) and torch.equal(c, d)
    assert cls.band_store.band[3].tolist() == [cls.block_mask.band] * H and cls.band_store.kept[3].shape == (H,)
    # gains: the store moves, best_mask_idx does not
    cls.reset_state()
    assert not cls.band_store.band and not cls.band_store.kept
    monkeypatch.setattr(cls, "adaptive_band", _core.AdaptiveBand(0.999, gain_up=64.0, gain_down=4.0, quantum=64))
    outs_a, best2 = module_calls(cls, attn, args, kw, 3)
    moved = cls.band_store.band[3].clone()
    print(f"{cls.__name__}: bands {moved.tolist()} from {cls.block_mask.band}, kept {cls.band_store.kept[3].tolist()}")
    assert moved.tolist() != [cls.block_mask.band] * H
    for c, d in zip(best0, best2):
        assert torch.equal(c, d)
    # a dense warm-up step measures and moves nothing
    module_calls(cls, attn, args, kw, 4, n=1, timestep=950.0)
    assert cls.band_store.band[4].tolist() == [cls.block_mask.band] * H
    # with quality_log as well: one dense probe per call feeds both, the record carries the bands the call ran with
    calls = {"rows": 0, "lse": 0}
    orig_rows, orig_lse = _probe.sample_dense_rows, _probe.sample_dense_lse
    monkeypatch.setattr(_probe, "sample_dense_rows", lambda *a, **k2: calls.__setitem__("rows", calls["rows"] + 1) or orig_rows(*a, **k2))
    monkeypatch.setattr(_probe, "sample_dense_lse", lambda *a, **k2: calls.__setitem__("lse", calls["lse"] + 1) or orig_lse(*a, **k2))
    cls.reset_state()
    path = str(tmp_path / "q.jsonl")
    monkeypatch.setattr(cls, "quality_log", path)
    outs_b, _ = module_calls(cls, attn, args, kw, 3)
    assert calls == {"rows": 3, "lse": 0}
    for a, b in zip(outs_a, outs_b):
        assert torch.equal(a, b)                                                        # the same rows, the same lse bits: the same trajectory
    assert torch.equal(cls.band_store.band[3], moved)
    _core.flush_quality_log()
    rec = [json.loads(x) for x in open(path)]
    assert len(rec) == 3 and rec[0]["band"] == [[cls.block_mask.band] * H] and all(r["kept_mass"] is not None for r in rec)
    assert rec[2]["band"] != rec[0]["band"] and all(isinstance(b, int) for b in rec[2]["band"][0])
    # without the option the record has no such list
    monkeypatch.setattr(cls, "adaptive_band", None)
    path2 = str(tmp_path / "q2.jsonl")
    monkeypatch.setattr(cls, "quality_log", path2)
    module_calls(cls, attn, args, kw, 3, n=1)
    _core.flush_quality_log()
    assert all("band" not in json.loads(x) for x in open(path2))
    cls.reset_state()


# ---------------------------------------------------------------------------------------------------------
# 9. poison: raw calls on outputs this test allocates itself
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("switch", [None, 0, 1], ids=["per_head", "switch0", "switch1"])
def test_every_word_of_o_lse_and_kept_is_written(nat, switch):
    import ctypes as C

    from poisoned import assert_fully_written, poisoned, poisoned_like

    lib = nat.load()
    model = "hy"                                                     # rows behind real_len and text rows included
    S, prm, _, _ = SC.band_case(model)
    q, k, v = device_inputs(model, DT)
    o, lse = poisoned_like(q), poisoned(1, H, S, dtype=torch.float32)
    band = i32([1, 129, 2 ** 30, -3])
    bm, alt = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S, prm["real_len"]))
    flag = i32([switch or 0])
    common = (q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), lse.data_ptr(), H, S, SC.D, 0, 1.0 / math.sqrt(SC.D), C.byref(bm))
    st = torch.cuda.current_stream().cuda_stream
    if switch is None:
        rc = lib.svg_band_attention_per_head_lse(*common, band.data_ptr(), None, None, st)
    else:
        rc = lib.svg_band_attention_switch_per_head_lse(*common, C.byref(alt), flag.data_ptr(), band.data_ptr(), None, None, st)
    assert rc == 0
    assert_fully_written(o, "o"), assert_fully_written(lse, "lse")
    kept = poisoned(H, dtype=torch.float32)
    rows = torch.tensor([0, S - 1, 7], device="cuda")
    ld = torch.zeros(H, 3, device="cuda")
    rc = lib.svg_band_width_update(lse.data_ptr(), rows.data_ptr(), ld.data_ptr(), 3, H, S, 0.9, 1.0, 1.0, 0.02, 128, 1, S + 1, None,
                                   kept.data_ptr(), band.data_ptr(), st)
    assert rc == 0
    assert_fully_written(kept, "kept")


def test_refusals_before_anything_runs(nat, monkeypatch):
    import torch.distributed as dist

    from svg import distributed as sd
    from svg.models import _core

    cls, attn, args, kw = wan_module(monkeypatch)
    monkeypatch.setattr(cls, "adaptive_band", _core.AdaptiveBand(0.9))
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{40500 + os.getpid() % 2000}", rank=0, world_size=1)
    try:
        sd.enable()
        with pytest.raises(NotImplementedError, match="adaptive_band"):
            module_calls(cls, attn, args, kw, 3, n=1)
    finally:
        sd.disable()
        dist.destroy_process_group()
    assert not cls.band_store.band
