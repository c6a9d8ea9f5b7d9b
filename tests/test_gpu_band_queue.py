"""The band kernels at head_dim 128 as resident workgroups on a work queue (csrc/band_policy.h BandQueue, band_attn_m16_queue_kernel):
which workgroup computes which (head, q-tile), and in what order, must not show in the output.  Every row visits the same keys in
the same order with the same arithmetic whatever the order of the q-tiles, so the checks are torch.equal, not tolerances:
  * one launch over all heads into an output pre-filled with NaN leaves no NaN (every q-tile was handed out) and equals the
    concatenation of one launch per head (other queue state: other lists, other tail) — bf16 / fp16, spatial / temporal / alternating
    heads, contiguous and strided tensors, plain / pre-scaled / device-switched entries, launches of 1, 2 and more than 256 work items;
  * launches back to back on one stream and on two streams give equal outputs (the last workgroup hands the counters back zeroed,
    streams own separate counter blocks);
  * a cap on the number of resident workgroups changes no bit (no dependence on how many workgroups are resident).
Launches with no more q-tiles than compute units take the static mapping unless svg_debug_band_queue_cap is set; the checks of the
first kind set it (to a value no launch reaches), so that the 1-, 2- and 52-item launches go through the queue as well."""
import pytest
import torch

from svg import _native as nat

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu

D = 128
# name -> (heads, frames, frame size, context, prompt length, band): work items = heads * q-tiles
GEOS = {
    "one_item": (1, 1, 200, 0, 0, 64),
    "two_items": (2, 2, 128, 0, 0, 64),
    "tiny": (4, 5, 600, 256, 64, 384),                # the benchmark's tiny workload: 4 x 13 work items
    "many": (6, 6, 2000, 256, 64, 3072),              # 6 x 49 = 294 work items: more than one per compute unit, edge tiers and a tail
}


def make(geo, dtype, seed=0):
    H, F, P, ctx, L, band = GEOS[geo]
    V = F * P
    S = V + ctx
    g = torch.Generator(device="cuda").manual_seed(seed)
    q, k, v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.float32, generator=g).to(dtype) for _ in range(3))
    if ctx:
        mask = nat.BandMask(real_len=V + L, band=band, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    else:
        mask = nat.BandMask(real_len=S, band=band, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
    return q, k, v, mask, dict(vid0=0, num_frame=F, frame_size=P)


def heads_flag(pattern, H):
    f = {"spatial": lambda h: 0, "temporal": lambda h: 1, "alt": lambda h: h % 2}[pattern]
    return torch.tensor([[f(h) for h in range(H)]], device="cuda", dtype=torch.int64)


def nan_filled(like):
    return torch.full_like(like, float("nan"))


def per_head(fn, q, k, v, flag):
    """the launch `fn(q, k, v, flag, out)` head by head"""
    outs = []
    for h in range(q.shape[1]):
        o = nan_filled(q[:, h:h + 1])
        fn(q[:, h:h + 1].contiguous(), k[:, h:h + 1].contiguous(), v[:, h:h + 1].contiguous(), flag[:, h:h + 1].contiguous(), o)
        outs.append(o)
    return torch.cat(outs, dim=1)


NO_CAP = 1 << 20   # svg_debug_band_queue_cap with a cap no launch reaches: the queue also for launches of one round


def check(fn, q, k, v, flag):
    lib = nat.load()
    assert lib.svg_debug_band_queue_cap(NO_CAP) == 0
    try:
        o = nan_filled(q)
        fn(q, k, v, flag, o)
        ref = per_head(fn, q, k, v, flag)
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0
    assert not torch.isnan(o).any(), "a q-tile was never computed"
    assert torch.equal(o, ref)
    return o


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("pattern", ["spatial", "temporal", "alt"])
@pytest.mark.parametrize("geo", sorted(GEOS))
def test_one_launch_equals_per_head_launches(geo, pattern, dtype):
    q, k, v, mask, perm = make(geo, dtype)
    flag = heads_flag(pattern, q.shape[1])
    check(lambda q_, k_, v_, f_, o_: nat.band_attention(q_, k_, v_, mask, head_perm_flag=f_, out=o_, **perm), q, k, v, flag)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("geo", ["tiny", "many"])
def test_prescaled_entry(geo, dtype):
    q, k, v, mask, perm = make(geo, dtype, seed=1)
    q = (q.float() * nat.softmax_q_scale(D)).to(dtype)
    flag = heads_flag("alt", q.shape[1])
    check(lambda q_, k_, v_, f_, o_: nat.band_attention(q_, k_, v_, mask, head_perm_flag=f_, out=o_, q_prescaled=True, **perm), q, k, v, flag)


@pytest.mark.parametrize("use_alt", [0, 1])
@pytest.mark.parametrize("geo", ["tiny", "many"])
def test_device_switched_entry(geo, use_alt):
    q, k, v, mask, perm = make(geo, torch.bfloat16, seed=2)
    S = q.shape[2]
    alt = nat.BandMask(real_len=mask.real_len, band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
    sw = torch.tensor([use_alt], device="cuda", dtype=torch.int32)
    flag = heads_flag("alt", q.shape[1])
    o = check(lambda q_, k_, v_, f_, o_: nat.band_attention_switch(q_, k_, v_, mask, alt, sw, head_perm_flag=f_, out=o_, **perm), q, k, v, flag)
    # and the switched launch is the plain launch of the mask it selected
    if use_alt:
        plain = nat.band_attention(q, k, v, alt)
    else:
        plain = nat.band_attention(q, k, v, mask, head_perm_flag=flag, **perm)
    assert torch.equal(o, plain)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("geo", ["tiny", "many"])
def test_strided_tensors(geo, dtype):
    """q, k, v as views of a fused QKV projection [1, S, 3 * H * D], o token-major: svg_band_attention_strided"""
    q, k, v, mask, perm = make(geo, dtype, seed=3)
    H, S = q.shape[1], q.shape[2]
    flag = heads_flag("alt", H)
    ref = nat.band_attention(q, k, v, mask, head_perm_flag=flag, **perm)
    qkv = torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2)
    qs, ks, vs = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    assert not qs.is_contiguous()
    out = nat.token_major_empty(qs)
    out.fill_(float("nan"))
    o = nat.band_attention(qs, ks, vs, mask, head_perm_flag=flag, out=out, **perm)
    torch.cuda.synchronize()
    assert not torch.isnan(o).any()
    assert torch.equal(o, ref)


def test_back_to_back_launches_on_one_stream_and_on_two():
    q, k, v, mask, perm = make("many", torch.bfloat16, seed=4)
    flag = heads_flag("alt", q.shape[1])
    run = lambda o_: nat.band_attention(q, k, v, mask, head_perm_flag=flag, out=o_, **perm)
    outs = [nan_filled(q) for _ in range(4)]
    for o in outs:   # one stream, no host work in between
        run(o)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    assert not torch.isnan(outs[0]).any()
    streams = [torch.cuda.Stream() for _ in range(2)]
    outs2 = [[nan_filled(q) for _ in range(3)] for _ in streams]
    torch.cuda.synchronize()   # (the fills ran on the default stream)
    for i in range(3):   # launches of the two streams are in flight together
        for s, os_ in zip(streams, outs2):
            with torch.cuda.stream(s):
                run(os_[i])
    torch.cuda.synchronize()
    for os_ in outs2:
        for o in os_:
            assert torch.equal(o, outs[0])


@pytest.mark.parametrize("cap", [1, 7, 40])
def test_capped_number_of_resident_workgroups(cap):
    q, k, v, mask, perm = make("many", torch.bfloat16, seed=5)
    flag = heads_flag("alt", q.shape[1])
    ref = nat.band_attention(q, k, v, mask, head_perm_flag=flag, **perm)
    lib = nat.load()
    assert lib.svg_debug_band_queue_cap(cap) == 0
    try:
        o = nan_filled(q)
        nat.band_attention(q, k, v, mask, head_perm_flag=flag, out=o, **perm)
        o2 = nan_filled(q)
        nat.band_attention(q, k, v, mask, head_perm_flag=flag, out=o2, **perm)   # the capped launch handed its counters back zeroed too
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0
    assert torch.equal(o, ref) and torch.equal(o2, ref)


def test_against_static_mapping_of_the_counting_launch():
    """svg_band_attention_notify keeps the static one-workgroup-per-q-tile mapping: the same bits as the queue launch"""
    q, k, v, mask, perm = make("many", torch.bfloat16, seed=6)
    H, S = q.shape[1], q.shape[2]
    flag = heads_flag("alt", H)
    o = nat.band_attention(q, k, v, mask, head_perm_flag=flag, **perm)
    done = nat.notify_counters(H, 1, q.device)
    o_static = nat.band_attention(q, k, v, mask, head_perm_flag=flag, done=done, done_nseg=1, **perm)
    torch.cuda.synchronize()
    assert torch.equal(o, o_static)
    assert (done[:H] == nat.band_notify_target(S, mask)).all()
