"""The row cursor of the 16x16x32 band kernels (csrc/band_policy.h RowWalk, csrc/attn_m16.h): a lane keeps the physical row of its key
row and steps it from tile to tile — += 64 on a contiguous head, += sp64 with a wrap at the end of the video on a token-major head —
and divides only on the first tile of a q-tile, after a segment jump and on tiles that straddle an end of the video or S.

Head_dim 128, two heads per launch: head 0 contiguous, head 1 token-major.  Two expectations per case:
  1. torch.equal with the same call on head 1's q, k, v gathered into logical order beforehand (index_select by the placement
     permutation), run as a contiguous head, the output scattered back: the same rows, the same key order, the same arithmetic — and no
     use of the token-major addressing under test;
  2. the fp32 oracle (oracle/svg_oracle.py) within the bounds of tests/test_gpu_m16.py (check_attn).
Geometries (frames x frame size; context 256, prompt 64, band 512 unless noted) are the smallest that reach each path:
  33 x 100   the benchmark's 64 % F = 31: the frame index wraps on most tiles; band, text-column and pad segments
  8 x 300    64 % F = 0: never wraps           3 x 1000   64 / F = 21
  64 x 40, 65 x 40, 100 x 30   F >= 64: 64 / F is 1 or 0
  1 x 2000   token-major = identity
  33 x 101   another remainder of V modulo 64 (V is no multiple of 64 in 33 x 100 either): the video ends inside a tile
  5 x 600 at vid0 = 226   text first, columns and rows full on [0, 226): the video starts inside a tile
  33 x 100, band 64       a handful of tiles per q-tile: guarded tail only
  33 x 100, band S + 1    dense mode: one long segment
each through the work queue (svg_debug_band_queue_cap as in tests/test_gpu_band_queue.py) and through the static mapping, bf16 and fp16;
and 33 x 100 through the device-switched, the pre-scaled and a strided entry whose K and V row strides differ."""
import functools
import math

import pytest
import torch

from oracle import svg_oracle as O
from svg import _native as nat
from test_gpu_kernels import check_attn

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu

D = 128
CTX, PROMPT, BAND = 256, 64, 512
LN2 = math.log(2.0)
# name -> (frames, frame size, first video row, band or None for S + 1)
GEOS = {
    "33x100": (33, 100, 0, BAND),
    "8x300": (8, 300, 0, BAND),
    "3x1000": (3, 1000, 0, BAND),
    "64x40": (64, 40, 0, BAND),
    "65x40": (65, 40, 0, BAND),
    "100x30": (100, 30, 0, BAND),
    "1x2000": (1, 2000, 0, BAND),
    "33x101": (33, 101, 0, BAND),
    "5x600_text_first": (5, 600, 226, BAND),
    "33x100_band64": (33, 100, 0, 64),
    "33x100_dense": (33, 100, 0, None),
}
NO_CAP = 1 << 20   # svg_debug_band_queue_cap with a cap no launch reaches: the queue also for launches of one round


def geometry(geo):
    """S, the mask parameters, the placement arguments, and the gather index (logical row -> physical row) of a token-major head"""
    F, P, vid0, band = GEOS[geo]
    V = F * P
    if vid0:   # text first
        S = vid0 + V
        prm = dict(real_len=S, band=band or S + 1, colfull_lo=0, colfull_hi=vid0, rowfull_lo=0, rowfull_hi=vid0)
    else:
        S = V + CTX
        prm = dict(real_len=V + PROMPT, band=band or S + 1, colfull_lo=V, colfull_hi=V + PROMPT, rowfull_lo=V, rowfull_hi=V + PROMPT)
    if band is None:
        prm = O.dense_band_params(S, prm["real_len"])
    idx = torch.arange(S)
    i = torch.arange(V)
    idx[vid0:vid0 + V] = vid0 + (i % F) * P + i // F
    return S, prm, dict(vid0=vid0, num_frame=F, frame_size=P), idx


@functools.lru_cache(maxsize=None)
def inputs(geo, dtype, prescaled=False):
    """q, k, v [1, 2, S, D] on the host (q carrying the softmax scale if asked) and the oracle's output for flags [0, 1]; computed once"""
    S, prm, _, idx = geometry(geo)
    g = torch.Generator().manual_seed(len(geo) * 131 + S)
    q, k, v = (torch.randn(1, 2, S, D, generator=g).to(dtype) for _ in range(3))
    if prescaled:
        q = (q.float() * nat.softmax_q_scale(D)).to(dtype)
    mask = O.band_mask(S, **prm)
    scale = LN2 if prescaled else None
    ref = torch.empty(1, 2, S, D)
    ref[:, 0] = O.masked_attention(q[:, 0], k[:, 0], v[:, 0], mask, scale=scale)
    ref[:, 1].index_copy_(1, idx, O.masked_attention(*(x[:, 1].index_select(1, idx) for x in (q, k, v)), mask, scale=scale))
    return q, k, v, ref


def flags(*f):
    return torch.tensor([list(f)], device="cuda", dtype=torch.int64)


def check(geo, dtype, run, queue, prescaled=False):
    """run(q, k, v, flag) -> o, an entry point bound to the case's mask and placement arguments"""
    S, prm, perm, idx = geometry(geo)
    q, k, v, ref = inputs(geo, dtype, prescaled)
    q, k, v = (x.cuda() for x in (q, k, v))
    idx = idx.cuda()
    lib = nat.load()
    assert lib.svg_debug_band_queue_cap(NO_CAP if queue else 0) == 0
    try:
        o = run(q, k, v, flags(0, 1))
        gathered = run(*(x[:, 1:2].index_select(2, idx) for x in (q, k, v)), flags(0))
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0
    want = torch.empty_like(gathered).index_copy_(2, idx, gathered)
    assert torch.equal(o[:, 1:2], want), f"{int((o[:, 1:2] != want).any(dim=-1).sum())} rows of the token-major head differ"
    check_attn(o, ref, dtype)


@pytest.mark.parametrize("queue", [True, False], ids=["queue", "static"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("geo", list(GEOS))
def test_token_major_head_equals_gathered_contiguous_head(geo, dtype, queue):
    S, prm, perm, _ = geometry(geo)
    mask = nat.BandMask(**prm)
    check(geo, dtype, lambda q, k, v, f: nat.band_attention(q, k, v, mask, head_perm_flag=f, **perm), queue)


def test_device_switched_entry():
    S, prm, perm, _ = geometry("33x100")
    mask, alt = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S))
    sw = torch.zeros(1, device="cuda", dtype=torch.int32)   # selects `mask`, with the head permutation
    check("33x100", torch.bfloat16, lambda q, k, v, f: nat.band_attention_switch(q, k, v, mask, alt, sw, head_perm_flag=f, **perm), False)


@pytest.mark.parametrize("queue", [True, False], ids=["queue", "static"])
def test_prescaled_entry(queue):
    S, prm, perm, _ = geometry("33x100")
    mask = nat.BandMask(**prm)
    check("33x100", torch.bfloat16, lambda q, k, v, f: nat.band_attention(q, k, v, mask, head_perm_flag=f, q_prescaled=True, **perm), queue,
          prescaled=True)


@pytest.mark.parametrize("queue", [True, False], ids=["queue", "static"])
def test_strided_entry_with_different_k_and_v_row_strides(queue):
    """k as the first D columns of rows 2 D wide, v of rows 3 D wide: the two byte offsets of a request come from two strides"""
    S, prm, perm, _ = geometry("33x100")
    mask = nat.BandMask(**prm)

    def run(q, k, v, f):
        kw = torch.zeros(*k.shape[:-1], 2 * D, device="cuda", dtype=k.dtype)
        vw = torch.zeros(*v.shape[:-1], 3 * D, device="cuda", dtype=v.dtype)
        kw[..., :D], vw[..., :D] = k, v
        ks, vs = kw[..., :D], vw[..., :D]
        assert ks.stride(2) == 2 * D and vs.stride(2) == 3 * D and not ks.is_contiguous()
        o = nat.band_attention(q, ks, vs, mask, head_perm_flag=f, **perm)
        assert torch.equal(o, nat.band_attention(q, k, v, mask, head_perm_flag=f, **perm))   # and the strides change no bit
        return o

    check("33x100", torch.bfloat16, run, queue)
