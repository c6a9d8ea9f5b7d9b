"""What the tests of the frame-shard form of band attention share (tests/test_band_shard_cpu.py, tests/test_gpu_band_shard.py;
include/svg_attn_band_shard.h).  Plain module, no GPU.

  * the geometries: small videos of whole frames with the text behind them (hy), without text (wan), with a frame size that is no multiple
    of 16 (p75) and with the text in front (cog: the video's frames are shards, the rows in front of it belong to none);
  * the statement of a shard in the terms of the model, not of the kernel's maps: row r of a shard is a row of the SEQUENCE (frame-major:
    vid0 + f * P + p, or a row of the tail), and the mask sees that row at its own index for a head in logical order and at
    vid0 + p * F + f for a token-major head (the placement of oracle.svg_oracle.head_placement);
  * float64 references on those coordinates, computed once and shared; the bounds are those of tests/sparse_lse_cases.py.
"""
import functools

import torch

import sparse_lse_cases as SC
from oracle import svg_oracle as O

H, D = 4, 128
FLAGS = (0, 1, 0, 1)                       # half the heads token-major
# name -> S, vid0, F, P, the six integers of the mask, the frames of the shards (the tail — every row behind the video — on the last one)
CASES = {
    # HunyuanVideo-like: 560 video rows, prompt 37, padding to 624; the text rows are full rows and full columns
    "hy": dict(S=624, vid0=0, F=7, P=80, mask=dict(real_len=597, band=128, colfull_lo=560, colfull_hi=597, rowfull_lo=560, rowfull_hi=597),
               frames=[(0, 3), (3, 5), (5, 7)]),
    # Wan-like: no text, the first frame's columns are full; band 129 = the narrow mask (a pair of shards without an element, below)
    "wan": dict(S=560, vid0=0, F=7, P=80, mask=dict(real_len=560, band=129, colfull_lo=0, colfull_hi=80, rowfull_lo=0, rowfull_hi=0),
                frames=[(0, 3), (3, 5), (5, 7)]),
    # a frame of 75 rows (no multiple of 16), shards of one frame (Fl = 1) and of two
    "p75": dict(S=332, vid0=0, F=4, P=75, mask=dict(real_len=320, band=64, colfull_lo=300, colfull_hi=320, rowfull_lo=300, rowfull_hi=320),
                frames=[(0, 2), (2, 3), (3, 4)]),
    # shards of several q-tiles and 19 / 20 key tiles: more than one q-tile per row region, tiles on the fast path for both kinds of head,
    # the row cursor's cheap step across frame wraps (Fl = 3: 64 = 21 * 3 + 1), the text columns as a key segment of their own
    "long": dict(S=2464, vid0=0, F=6, P=400, mask=dict(real_len=2440, band=512, colfull_lo=2400, colfull_hi=2440, rowfull_lo=2400,
                                                      rowfull_hi=2440), frames=[(0, 3), (3, 6)]),
    # CogVideoX-like: 24 text rows FIRST (full rows, full columns); the shards are the video's frames alone
    "cog": dict(S=584, vid0=24, F=7, P=80, mask=dict(real_len=584, band=128, colfull_lo=0, colfull_hi=24, rowfull_lo=0, rowfull_hi=24),
                frames=[(0, 4), (4, 7)]),
}


def geometry(name):
    c = CASES[name]
    return c["S"], c["vid0"], c["F"], c["P"]


def shards(name):
    """[(f0, n_frames, tail_begin, n_tail)] of the case: its frame shards, the rows behind the video on the last one"""
    S, vid0, F, P = geometry(name)
    fr = CASES[name]["frames"]
    tail0 = vid0 + F * P
    return [(a, b - a, tail0, (S - tail0) if i == len(fr) - 1 else 0) for i, (a, b) in enumerate(fr)]


def whole(name):
    """the shard that is the whole sequence (vid0 = 0)"""
    S, vid0, F, P = geometry(name)
    assert vid0 == 0
    return (0, F, F * P, S - F * P)


def shard_rows(name, shard):
    """sequence rows a shard holds, in the shard's own (physical) order"""
    S, vid0, F, P = geometry(name)
    f0, n, tail0, n_tail = shard
    return torch.cat([torch.arange(vid0 + f0 * P, vid0 + (f0 + n) * P), torch.arange(tail0, tail0 + n_tail)])


def mask_coords(name, rows, token_major):
    """where the mask sees the sequence rows `rows`: at their own index, or — a token-major head, a row of the video — at
    vid0 + p * F + f"""
    S, vid0, F, P = geometry(name)
    if not token_major:
        return rows.clone()
    i = rows - vid0
    tm = vid0 + (i % P) * F + i // P
    return torch.where((i >= 0) & (i < F * P), tm, rows)


@functools.lru_cache(maxsize=None)
def element_mask(name):
    return O.band_mask(CASES[name]["S"], **CASES[name]["mask"])


@functools.lru_cache(maxsize=None)
def inputs(name, dtype, seed=3):
    """q, k, v [1, H, S, D] of the whole sequence, in the model's row order"""
    S = CASES[name]["S"]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, H, S, D, generator=g).to(dtype) for _ in range(3))


def shard_inputs(name, dtype, shard):
    rows = shard_rows(name, shard)
    return tuple(x[:, :, rows].contiguous() for x in inputs(name, dtype))


def pair_mask(name, q_shard, k_shard, token_major):
    """bool [Sq, Sk]: which (row of q_shard, row of k_shard) pairs the mask allows for a head of this kind, in the shards' physical order"""
    em = element_mask(name)
    cq = mask_coords(name, shard_rows(name, q_shard), token_major)
    ck = mask_coords(name, shard_rows(name, k_shard), token_major)
    return em[cq][:, ck]


@functools.lru_cache(maxsize=None)
def pair_reference(name, dtype, q_shard, k_shard, flags=FLAGS):
    """float64 (o [1, H, Sq, D], lse [1, H, Sq]) of the rows of q_shard over the keys of k_shard, head h of kind flags[h]"""
    q, _, _ = shard_inputs(name, dtype, q_shard)
    _, k, v = shard_inputs(name, dtype, k_shard)
    outs = [SC.masked_attention_lse(q[:, h:h + 1], k[:, h:h + 1], v[:, h:h + 1], pair_mask(name, q_shard, k_shard, bool(flags[h])))
            for h in range(H)]
    return torch.cat([o for o, _ in outs], dim=1), torch.cat([l for _, l in outs], dim=1)


@functools.lru_cache(maxsize=None)
def rows_reference(name, dtype, q_shard, flags=FLAGS):
    """float64 (o, lse) of the rows of q_shard over ALL keys of the sequence"""
    S = CASES[name]["S"]
    rows = shard_rows(name, q_shard)
    q, k, v = inputs(name, dtype)
    em = element_mask(name)
    outs = []
    for h in range(H):
        cq = mask_coords(name, rows, bool(flags[h]))
        ck = mask_coords(name, torch.arange(S), bool(flags[h]))
        outs.append(SC.masked_attention_lse(q[:, h:h + 1, rows], k[:, h:h + 1], v[:, h:h + 1], em[cq][:, ck]))
    return torch.cat([o for o, _ in outs], dim=1), torch.cat([l for _, l in outs], dim=1)
