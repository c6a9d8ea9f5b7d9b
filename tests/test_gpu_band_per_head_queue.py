"""The per-head band launches as resident workgroups on the work queue (include/svg_attn_band_per_head_queue.h:
svg_band_attention_per_head_queue_lse, svg_band_attention_switch_per_head_queue_lse; csrc/attention.hip band_attn_m16_per_head_queue_kernel,
band_attn_m16_per_head_switch_queue_kernel).  Which workgroup computes which (head, q-tile), in what order, and which pairs lane 0 drops on
a head whose band does not cut the full rows out must not show in the output: every check is torch.equal on o and on lse against the
statically mapped per-head wrapper on the same inputs, plus "no NaN in o".  The outputs are the wrappers' own allocations, which this module
has poisoned (0xFF bytes: NaN in bf16, fp16 and fp32), so equality with the static launch also shows that every element was written.
Launches this small take the static mapping unless svg_debug_band_queue_cap is set, so every check sets it (to a value no launch reaches,
or to the cap the check is about) and takes it back in a finally.

Geometries: `tiny` and `many` of tests/test_gpu_band_queue.py — 4 x 13 and 6 x 49 work items, S = 3256 and 12 256 —, the replay inputs of
tests/band_replay_cases.py (geometry A, 14 work items), and the closed loop of tests/test_gpu_adaptive_band.py."""
import contextlib

import pytest
import torch

import band_replay_cases as RC
from oracle import svg_oracle as O
from svg import _adaptive_band as ab
from svg import _native as nat

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu

D = 128
NO_CAP = 1 << 20   # svg_debug_band_queue_cap with a cap no launch reaches: the queue also for launches of one round
# name -> (heads, frames, frame size, context, prompt length, band): work items = heads * q-tiles
GEOS = {
    "tiny": (4, 5, 600, 256, 64, 384),
    "many": (6, 6, 2000, 256, 64, 3072),
}
QUANTUM = 128


@contextlib.contextmanager
def queue_cap(cap):
    lib = nat.load()
    assert lib.svg_debug_band_queue_cap(cap) == 0
    try:
        yield
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0


_INPUTS = {}


def make(geo, dtype):
    """q, k, v, mask, alternate (dense) mask, the head flags (alternating) and geometry keywords; built once per (geometry, dtype)"""
    if (geo, dtype) not in _INPUTS:
        H, F, P, ctx, L, band = GEOS[geo]
        V = F * P
        S = V + ctx
        g = torch.Generator(device="cuda").manual_seed(17)
        q, k, v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.float32, generator=g).to(dtype) for _ in range(3))
        mask = nat.BandMask(real_len=V + L, band=band, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
        alt = nat.BandMask(real_len=V + L, band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
        flag = torch.tensor([[h % 2 for h in range(H)]], device="cuda", dtype=torch.int64)
        _INPUTS[geo, dtype] = (q, k, v, mask, alt, dict(head_perm_flag=flag, vid0=0, num_frame=F, frame_size=P))
    return _INPUTS[geo, dtype]


def band_vector(kind, geo):
    H, F, P, ctx, _, hint = GEOS[geo]
    S = F * P + ctx
    if kind == "uniform":
        vals = [hint]
    elif kind == "mixed":
        vals = [1, QUANTUM, hint // 2, hint, 2 * hint, S + 1]
    else:
        vals = [S + 1]
    return torch.tensor([vals[h % len(vals)] for h in range(H)], dtype=torch.int32, device="cuda")


def projection_views(q, k, v):
    """q, k, v as views of one fused QKV projection output [1, S, 3 H D]"""
    H, S = q.shape[1], q.shape[2]
    qkv = torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2).contiguous()
    views = tuple(qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not views[0].is_contiguous()
    return views


def same(got, want):
    o, lse = got
    o_ref, lse_ref = want
    assert not torch.isnan(o).any(), "a q-tile was never computed"
    assert torch.equal(o, o_ref), "o differs from the static per-head launch"
    assert torch.equal(lse, lse_ref), "lse differs from the static per-head launch (or holds unwritten words)"


# ---------------------------------------------------------------------------------------------------------
# the per-head form
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["contiguous", "token_major_o"])
@pytest.mark.parametrize("bands", ["uniform", "mixed", "wide"])
@pytest.mark.parametrize("geo", sorted(GEOS))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_per_head_queue_has_the_bits_of_the_static_launch(dtype, geo, bands, layout):
    q, k, v, mask, _, kw = make(geo, dtype)
    band = band_vector(bands, geo)
    tm = layout == "token_major_o"
    if tm:
        q, k, v = projection_views(q, k, v)
    want = ab.band_attention_per_head(q, k, v, mask, band, token_major_out=tm, **kw)
    with queue_cap(NO_CAP):
        got = ab.band_attention_per_head(q, k, v, mask, band, token_major_out=tm, work_queue=True, **kw)
    assert got[0].is_contiguous() != tm
    same(got, want)


# ---------------------------------------------------------------------------------------------------------
# the switch form
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bands", ["mixed", "wide"])
@pytest.mark.parametrize("geo", sorted(GEOS))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_switch_queue_under_either_flag(dtype, geo, bands):
    q, k, v, mask, alt, kw = make(geo, dtype)
    band = band_vector(bands, geo)
    before = band.clone()
    zero, one = (torch.tensor([f], dtype=torch.int32, device="cuda") for f in (0, 1))
    with queue_cap(NO_CAP):
        got0 = ab.band_attention_switch_per_head(q, k, v, mask, alt, zero, band, work_queue=True, **kw)
        one_form = ab.band_attention_per_head(q, k, v, mask, band, work_queue=True, **kw)
        got1 = ab.band_attention_switch_per_head(q, k, v, mask, alt, one, band, work_queue=True, **kw)
    same(got0, one_form)                                            # flag 0: the per-head queue form
    same(got0, ab.band_attention_switch_per_head(q, k, v, mask, alt, zero, band, **kw))
    same(got1, nat.band_attention_switch(q, k, v, mask, alt, one, return_lse=True, **kw))   # flag 1: the alternate mask as it is
    same(got1, ab.band_attention_switch_per_head(q, k, v, mask, alt, one, band, **kw))
    assert not torch.equal(got0[0], got1[0])
    assert torch.equal(band, before)                                # band is never written


# ---------------------------------------------------------------------------------------------------------
# residency and counters
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["per_head", "switch0", "switch1"])
def test_three_resident_workgroups_give_the_bits_of_the_uncapped_launch(form):
    q, k, v, mask, alt, kw = make("many", torch.bfloat16)
    band = band_vector("mixed", "many")
    flag = torch.tensor([1 if form == "switch1" else 0], dtype=torch.int32, device="cuda")

    def run():
        if form == "per_head":
            return ab.band_attention_per_head(q, k, v, mask, band, work_queue=True, **kw)
        return ab.band_attention_switch_per_head(q, k, v, mask, alt, flag, band, work_queue=True, **kw)

    with queue_cap(NO_CAP):
        want = run()
    with queue_cap(3):
        got = run()
        again = run()                                               # the capped launch handed its counters back zeroed too
    same(got, want)
    same(again, want)


def test_back_to_back_launches_on_one_stream_and_on_two():
    q, k, v, mask, alt, kw = make("many", torch.bfloat16)
    band = band_vector("mixed", "many")
    zero = torch.tensor([0], dtype=torch.int32, device="cuda")
    want = ab.band_attention_per_head(q, k, v, mask, band, **kw)
    torch.cuda.synchronize()
    with queue_cap(NO_CAP):
        outs = [ab.band_attention_per_head(q, k, v, mask, band, work_queue=True, **kw) for _ in range(2)]   # one stream, no host work between
        outs.append(ab.band_attention_switch_per_head(q, k, v, mask, alt, zero, band, work_queue=True, **kw))
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(2)]
        outs2 = []
        for s in streams:                                           # one launch each, in flight together: separate counter blocks
            with torch.cuda.stream(s):
                outs2.append(ab.band_attention_per_head(q, k, v, mask, band, work_queue=True, **kw))
    for got in outs + outs2:
        same(got, want)


# ---------------------------------------------------------------------------------------------------------
# replay: the inputs of tests/band_replay_cases.py that make the bf16 overflow test fire
# ---------------------------------------------------------------------------------------------------------
def replay_inputs(case):
    g = case.geo
    q, k, v = (O.head_placement(x, RC.BEST, g.CTX, g.F, g.P, inverse=True).cuda().contiguous() for x in RC.inputs(case))
    kw = dict(head_perm_flag=RC.BEST.cuda(), vid0=0, num_frame=g.F, frame_size=g.P)
    return q, k, v, kw


def counted(fn):
    nat.band_replays(reset=True)
    out = fn()
    return out, nat.band_replays(reset=True)


@pytest.mark.parametrize("cap", [NO_CAP, 2], ids=["queue", "queue_cap2"])
@pytest.mark.parametrize("bands", ["hint", "one_wide"])
def test_replay_on_the_queue_forms(bands, cap):
    """geometry A with a +400 spike in each of the six q-tiles of real rows of both heads: twelve q-tiles fail their validation under the
    hint and run once more.  The queue forms replay as often as the static per-head entry and end on its bits."""
    case = RC.switch_case()                                         # every spiked pair allowed by the band mask and by the dense one
    g = case.geo
    q, k, v, kw = replay_inputs(case)
    mask, alt = nat.BandMask(**g.mask_params("band")), nat.BandMask(**g.mask_params("dense_real"))
    band = torch.tensor([g.BAND, g.BAND if bands == "hint" else g.S + 1], dtype=torch.int32, device="cuda")
    zero, one = (torch.tensor([f], dtype=torch.int32, device="cuda") for f in (0, 1))
    want, n_static = counted(lambda: ab.band_attention_per_head(q, k, v, mask, band, **kw))
    want1, n_static1 = counted(lambda: ab.band_attention_switch_per_head(q, k, v, mask, alt, one, band, **kw))
    with queue_cap(cap):
        got, n = counted(lambda: ab.band_attention_per_head(q, k, v, mask, band, work_queue=True, **kw))
        got0, n0 = counted(lambda: ab.band_attention_switch_per_head(q, k, v, mask, alt, zero, band, work_queue=True, **kw))
        got1, n1 = counted(lambda: ab.band_attention_switch_per_head(q, k, v, mask, alt, one, band, work_queue=True, **kw))
    print(f"replays {bands} cap={cap}: static {n_static} queue {n} switch queue flag 0 {n0}; flag 1: static {n_static1} queue {n1}")
    assert n_static >= 1 and n_static1 >= 1
    if bands == "hint":
        assert n_static == len(case.replaying_pairs()) == 12
    same(got, want)
    same(got0, want)
    same(got1, want1)
    assert n == n_static and n0 == n_static and n1 == n_static1


# ---------------------------------------------------------------------------------------------------------
# the layer-call
# ---------------------------------------------------------------------------------------------------------
def test_layer_call_with_the_switch_on(monkeypatch):
    from svg.models import _core
    from test_gpu_adaptive_band import H, loop_call, loop_inputs

    q, k, v = loop_inputs()
    seen = []
    orig = ab.band_attention_switch_per_head
    monkeypatch.setattr(ab, "band_attention_switch_per_head", lambda *a, **kw: seen.append(kw.get("work_queue", False)) or orig(*a, **kw))

    def three_calls(on, adaptive):
        monkeypatch.setattr(_core, "PER_HEAD_BAND_QUEUE", on)
        store = _core.BandStore()
        with queue_cap(NO_CAP):
            outs, mask, _ = loop_call(nat, q, k, v, 9, adaptive=adaptive, band_store=store, layer_idx=7)
        return outs, store.band[7].clone(), store.kept[7].clone(), mask

    fixed = _core.AdaptiveBand(0.9, gain_up=0, gain_down=0, quantum=64)
    off, band_off, _, mask = three_calls(False, fixed)
    on, band_on, _, _ = three_calls(True, fixed)
    assert seen == [False] * 3 + [True] * 3
    for (o0, b0), (o1, b1) in zip(off, on):
        assert not torch.isnan(o1).any() and torch.equal(o0, o1) and torch.equal(b0, b1)
    assert band_off.tolist() == band_on.tolist() == [mask.band] * H
    moving = _core.AdaptiveBand(target=0.9, gain_up=16.0, gain_down=32.0, dead=0.02, quantum=64)
    off, band_off, kept_off, _ = three_calls(False, moving)
    on, band_on, kept_on, _ = three_calls(True, moving)
    print(f"bands after three calls: static {band_off.tolist()} queue {band_on.tolist()}")
    assert band_off.tolist() != [mask.band] * H                     # the bands moved, and to the same place on both paths
    assert torch.equal(band_off, band_on) and torch.equal(kept_off, kept_on)
    for (o0, b0), (o1, b1) in zip(off, on):
        assert torch.equal(o0, o1) and torch.equal(b0, b1)
