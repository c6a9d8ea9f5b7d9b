"""What the tests of svg_band_attention_lse / svg_varblock_attention_lse share (tests/test_sparse_attention_lse_cpu.py,
tests/test_gpu_sparse_attention_lse.py).  Plain module, no GPU.

  * the float64 statement: attention under a boolean element mask with its row log-sum-exp — masked_fill(-inf), logsumexp; a row without
    keys gives zeros and -inf;
  * the bounds.  They are the project's limits for this epilogue, restated from tests/test_gpu_attention_lse.py (U, T_SINGLE, check_lse,
    merged_limit there) — no new numbers.  The one difference: a row whose reference is -inf (no key) must come back as -inf exactly, where
    the cross-attention test had no such rows and asserted that every lse is finite;
  * the inputs and the float64 references of the band and variable-block cases, computed once and shared.
Masks come from oracle.svg_oracle (band_mask, hy_mask, ... through test_gpu_kernels._band_case; block_mask_to_element_mask), merge
statements from tests/lse_ops_torch.py.

ref: BlockSparseAttentionWrapper.run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188."""
import functools
import math

import torch

from lse_ops_torch import merge_states
from oracle import svg_oracle as O
from test_gpu_kernels import _band_case, random_partition_batch, rel_l2

DTYPES = [torch.bfloat16, torch.float16]
# the relative rounding step of the probabilities the body sums (round to nearest): it bounds the relative error of the row sum, hence the
# absolute error of its log (tests/test_gpu_attention_lse.py)
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
T_SINGLE = {torch.bfloat16: 3e-3, torch.float16: 1e-3}   # check_attn's rel. L2 bound of one call (tests/test_gpu_kernels.py)
NINF = float("-inf")


def masked_attention_lse(q, k, v, mask, scale=None):
    """float64: o = softmax(q k^T * scale + mask) v and lse = log sum_j exp(scale * q.k_j) over the keys the mask gives the row; q [..., Sq,
    D], k / v [..., Skv, D] (broadcast over the leading dimensions), mask bool [Sq, Skv] (or broadcastable) or None.  A row without keys:
    zeros and -inf."""
    qd, kd, vd = q.double(), k.double(), v.double()
    s = torch.matmul(qd, kd.transpose(-1, -2)) * (1.0 / math.sqrt(q.shape[-1]) if scale is None else scale)
    if mask is not None:
        s = s.masked_fill(~mask, NINF)
    lse = torch.logsumexp(s, dim=-1)
    seen = torch.isfinite(lse)
    p = torch.exp(s - torch.where(seen, lse, torch.zeros_like(lse))[..., None])   # (a row without keys: exp(-inf - 0) = 0)
    return torch.matmul(p, vd), lse


def lse_bound(ref, dtype):
    return U[dtype] + 1e-5 * (1 + ref.abs())


def check_lse(lse, ref, dtype, what="", factor=1.0):
    """|lse - ref| <= factor * (U[dtype] + 1e-5 (1 + |ref|)) where ref is finite; -inf exactly where it is not"""
    lse = lse.double().cpu()
    assert lse.shape == ref.shape, (lse.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(lse[~fin], ref[~fin]), f"{what}: rows without keys must be -inf"
    err = (lse[fin] - ref[fin]).abs()
    bound = factor * lse_bound(ref[fin], dtype)
    if err.numel():
        print(f"{what} lse max err {err.max().item():.3e} (bound {bound.min().item():.3e})")
    assert torch.isfinite(lse[fin]).all() and (err <= bound).all(), (what, err.max().item(), bound.min().item())


def merged_limit(ref, dtype):
    """sqrt(t^2 + r^2): t the single-call tolerance of check_attn, r the error of ONE rounding of the exact result to the 16-bit type — a
    merged result carries one more independent output rounding than a single call (tests/test_gpu_attention_lse.py)"""
    r = rel_l2(ref.to(dtype), ref)
    return math.sqrt(T_SINGLE[dtype] ** 2 + r ** 2), r


# ---------------------------------------------------------------------------------------------------------
# band cases: the geometry of tests/test_gpu_kernels.py test_band_attention
# ---------------------------------------------------------------------------------------------------------
GEOM = dict(F_=5, P_=150, ctx=40, L=11, mul=2.3)
BAND_MODELS = ["hy", "wan", "cog", "dense2"]
BAND_H, D = 3, 128
V = GEOM["F_"] * GEOM["P_"]          # 750 video rows
REAL = V + GEOM["L"]                 # hy: 761 real rows
# protocol (a): the band of the hy mask over the video keys alone; the text keys [V, REAL) go to a dense call of their own
VIDEO_BAND = dict(real_len=V, band=256, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)


def band_case(model):
    """-> S, the six integers of the band mask, the element mask, vid0"""
    return _band_case(model, **GEOM)


@functools.lru_cache(maxsize=None)
def band_inputs(model, dtype, seed=2):
    S = band_case(model)[0]
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(1, BAND_H, S, D, generator=g).to(dtype) for _ in range(3))


@functools.lru_cache(maxsize=None)
def band_reference(model, dtype, seed=2):
    """float64 (o, lse) of band_inputs under the model's element mask"""
    q, k, v = band_inputs(model, dtype, seed)
    return masked_attention_lse(q, k, v, band_case(model)[2])


# ---------------------------------------------------------------------------------------------------------
# variable-block cases (hq, hkv, S, MB, NB, keep): random_partition_batch sizes as in tests/test_gpu_kernels.py test_varblock_attention;
# a block is active with probability `keep`
# ---------------------------------------------------------------------------------------------------------
VB_CASES = [(4, 1, 4096, 20, 100, 0.3), (4, 4, 256, 10, 50, 0.8)]


@functools.lru_cache(maxsize=None)
def vb_inputs(case, dtype):
    hq, hkv, S, MB, NB, keep = case
    gen = torch.Generator().manual_seed(hq * 1000 + S + MB)
    rsz = random_partition_batch(S, MB, hkv, gen)
    csz = random_partition_batch(S, NB, hkv, gen)
    bmap = torch.rand(hkv, MB, NB, generator=gen) < keep
    q = torch.randn(hq, S, D, generator=gen).to(dtype)
    k = torch.randn(hkv, S, D, generator=gen).to(dtype)
    v = torch.randn(hkv, S, D, generator=gen).to(dtype)
    return q, k, v, bmap, rsz, csz


def vb_reference_of(q, k, v, bmap, rsz, csz):
    """float64 (o [hq, Sq, D], lse [hq, Sq]) under the element mask of the block map; rows behind sum(rsz[h]) (no block-row covers them):
    zeros and -inf"""
    hq, hkv = q.shape[0], k.shape[0]
    g = hq // hkv
    o = torch.zeros(q.shape, dtype=torch.float64)
    lse = torch.full(q.shape[:-1], NINF, dtype=torch.float64)
    for h in range(hkv):
        em = O.block_mask_to_element_mask(bmap[h], rsz[h], csz[h])       # [covered rows, covered keys]
        nq, nk = em.shape
        o[h * g:(h + 1) * g, :nq], lse[h * g:(h + 1) * g, :nq] = masked_attention_lse(q[h * g:(h + 1) * g, :nq], k[h:h + 1, :nk], v[h:h + 1, :nk], em)
    return o, lse


@functools.lru_cache(maxsize=None)
def vb_reference(case, dtype):
    return vb_reference_of(*vb_inputs(case, dtype))


def split_key_clusters(bmap, cuts):
    """the block map restricted to the key clusters [a, b) of every consecutive pair of `cuts`: same shape, False outside"""
    col = torch.arange(bmap.shape[-1])
    return [bmap & ((col >= a) & (col < b)) for a, b in zip(cuts[:-1], cuts[1:])]

