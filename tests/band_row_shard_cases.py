"""What the row-shard tests share (include/svg_attn_band_row_shard.h): F = 5 frames of P = 192 rows and 40 text rows, one head in logical
order and one token-major, a HunyuanVideo-like and a Wan-like mask.  A shard is stated in the model's terms, as tests/band_shard_cases.py
does: its rows are rows of the SEQUENCE, and the mask sees a video row f * P + p of a token-major head at p * F + f."""
import functools

import torch

import sparse_lse_cases as SC
from oracle import svg_oracle as O

F, P, S, H, D = 5, 192, 1000, 2, 128
V = F * P
GEO = (S, 0, F, P)
FLAGS = (0, 1)
MASKS = {"hy": dict(real_len=S, band=192, colfull_lo=V, colfull_hi=S, rowfull_lo=V, rowfull_hi=S),
         "wan": dict(real_len=S, band=193, colfull_lo=0, colfull_hi=P, rowfull_lo=0, rowfull_hi=0)}
# three shards, the tail on the last; the middle one has a == b under (320, 704) and b < a under (320, 640), the outer ones a < b
CUTS = {"704": (320, 704), "640": (320, 640)}


def shards(cuts):
    edges = (0,) + tuple(cuts) + (V,)
    return [(a, b - a, V, S - V if b == V else 0) for a, b in zip(edges[:-1], edges[1:])]


def shard_rows(shard):
    row0, n, tail0, n_tail = shard
    return torch.cat([torch.arange(row0, row0 + n), torch.arange(tail0, tail0 + n_tail)])


def mask_coords(rows, token_major):
    return torch.where(rows < V, (rows % P) * F + rows // P, rows) if token_major else rows.clone()


@functools.lru_cache(maxsize=None)
def inputs(dtype):
    g = torch.Generator().manual_seed(11)
    return tuple(torch.randn(1, H, S, D, generator=g).to(dtype) for _ in range(3))


def pair_mask(mask, q_shard, k_shard, token_major):
    """bool [Sq, Sk] in the shards' stored order"""
    em = O.band_mask(S, **MASKS[mask])
    return em[mask_coords(shard_rows(q_shard), token_major)][:, mask_coords(shard_rows(k_shard), token_major)]


@functools.lru_cache(maxsize=None)
def reference(mask, dtype):
    """float64 (o, lse) of dense masked attention over the whole sequence, in the model's row order"""
    q, k, v = inputs(dtype)
    whole = (0, V, V, S - V)
    outs = [SC.masked_attention_lse(q[:, h:h + 1], k[:, h:h + 1], v[:, h:h + 1], pair_mask(mask, whole, whole, bool(FLAGS[h])))
            for h in range(H)]
    return torch.cat([o for o, _ in outs], dim=1), torch.cat([l for _, l in outs], dim=1)
