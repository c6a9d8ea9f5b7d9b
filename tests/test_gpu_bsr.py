"""Uniform-block (BSR) sparse attention ops (svg/kernels/ops/attention_ops.py mirror) on the GPU: the reference's test
(svg/kernels/test/test_sparse_attn.py:181-260) compares sparse_attn_forward with dense attention under the element mask its own
generators produce; those masks are the goldens here (tests/golden/make_golden_bsr.py)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import svg_oracle as O

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu
GOLD = np.load(str(Path(__file__).parent / "golden" / "bsr_golden.npz"))
P = 40


@pytest.fixture(scope="module")
def ops():
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "sparse-videogen_amd"))
    from svg.kernels.ops import attention_ops
    return attention_ops


def golden_mask(kind, F, L, mul):
    S = F * P + L
    return torch.from_numpy(np.unpackbits(GOLD[f"{kind}_{F}_{L}_{mul}"])[: S * S].reshape(S, S).astype(bool))


def close(a, b):
    rtol, atol = {torch.float16: (5e-3, 5e-3), torch.bfloat16: (3e-2, 2e-2)}[a.dtype]   # test_sparse_attn.py:91-96
    torch.testing.assert_close(a.float().cpu(), b.float().cpu(), rtol=rtol, atol=atol)


@pytest.mark.parametrize("F,L", [(5, 16), (13, 77), (5, 0)])
@pytest.mark.parametrize("heads,D", [(4, 64), (2, 128)])
@pytest.mark.parametrize("kind,mul", [("spatial", 0), ("spatial", 1), ("spatial", 2), ("temporal", 0.5), ("temporal", 1),
                                      ("temporal", 1.4), ("temporal", 1.8)])
def test_sparse_attn_forward(ops, kind, mul, F, L, heads, D):
    torch.manual_seed(F + L)
    S = F * P + L
    dt = torch.float16
    q, k, v = (torch.randn(S, heads, D).to(dt) for _ in range(3))
    gen = ops._gen_spatial_mask if kind == "spatial" else ops._gen_temporal_mask
    md = gen(F, P, mul)
    meta = ops.FAMetadata(L, F, P, md if kind == "temporal" else None, md if kind == "spatial" else None, None)
    o = ops.sparse_attn_forward(q.cuda(), k.cuda(), v.cuda(), meta, kind)
    mask = golden_mask(kind, F, L, mul)
    qh, kh, vh = (x.permute(1, 0, 2)[None] for x in (q, k, v))
    ref = O.masked_attention(qh, kh, vh, mask)[0].permute(1, 0, 2)
    close(o, ref.to(dt))


def test_init_sparse_attn_and_gqa(ops):
    torch.manual_seed(1)
    F, L, Hq, Hkv, D = 5, 16, 8, 2, 128
    S = F * P + L
    meta = ops.init_sparse_attn(L, F, P, 1.4, 1)
    q = torch.randn(S, Hq, D).to(torch.bfloat16)
    k, v = torch.randn(S, Hkv, D).to(torch.bfloat16), torch.randn(S, Hkv, D).to(torch.bfloat16)
    for kind, mul in (("temporal", 1.4), ("spatial", 1)):
        o = ops.sparse_attn_forward(q.cuda(), k.cuda(), v.cuda(), meta, kind)
        mask = golden_mask(kind, F, L, mul)
        kr, vr = k.repeat_interleave(Hq // Hkv, dim=1), v.repeat_interleave(Hq // Hkv, dim=1)
        ref = O.masked_attention(q.permute(1, 0, 2)[None], kr.permute(1, 0, 2)[None], vr.permute(1, 0, 2)[None], mask)[0]
        close(o, ref.permute(1, 0, 2).to(torch.bfloat16))


@pytest.mark.parametrize("kind,mul,heads,D", [("spatial", 2, 24, 128), ("temporal", 1.8, 32, 64), ("temporal", 1.8, 24, 128),
                                               ("spatial", 2, 32, 64)])
def test_sparse_attn_forward_reference_grid_fullsize(ops, kind, mul, heads, D):
    """The reference's own grid (svg/kernels/test/test_sparse_attn.py:160-161, 205-206): F = 21, P = 3600, 16 prompt tokens, 24 / 32
    heads, D 64 / 128, fp16 — S = 75616.  The dense reference of the whole problem is out of reach on the CPU, so spot rows of three
    heads are compared with the oracle under the element mask expanded from the REFERENCE generators' block masks (golden), text
    first like gen_mask_block2element (:66-86)."""
    F, P_, L = 21, 3600, 16
    S = F * P_ + L
    dt = torch.float16
    g = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = (torch.randn(S, heads, D, device="cuda", dtype=dt, generator=g) for _ in range(3))
    gen = ops._gen_spatial_mask if kind == "spatial" else ops._gen_temporal_mask
    md = gen(F, P_, mul)
    meta = ops.FAMetadata(L, F, P_, md if kind == "temporal" else None, md if kind == "spatial" else None, None)
    o = ops.sparse_attn_forward(q, k, v, meta, kind)
    blk = torch.from_numpy(GOLD[f"blk_{kind}_{F}_{P_}_{mul}"])
    bs = P_ if kind == "spatial" else P_ // 10
    rows = [0, 1, L - 1, L, L + 1, L + bs - 1, L + bs, L + 3 * P_ - 1, L + 3 * P_, L + 10 * P_ + 1799, S - bs - 1, S - bs, S - 1]
    rows += torch.randint(0, S, (20,), generator=torch.Generator().manual_seed(2)).tolist()
    rt = torch.tensor(rows)
    kk = torch.arange(S)
    mask = torch.ones(len(rows), S, dtype=torch.bool)
    vid = rt >= L
    bi = ((rt[vid] - L) // bs)
    mask[vid, L:] = blk[bi][:, (kk[L:] - L) // bs]
    for h in (0, heads // 2, heads - 1):
        ref = O.masked_attention(q[rows, h].float().cpu(), k[:, h].float().cpu(), v[:, h].float().cpu(), mask)
        close(o[rows, h], ref.to(dt))


@pytest.mark.parametrize("F,P_,mul,heads,D", [(5, 40, 1.4, 4, 64), (4, 150, 0.6, 2, 128), (3, 96, 2.0, 4, 64)])
def test_wan_sparse_attn_forward(F, P_, mul, heads, D):
    """The Wan (video-only) BSR op, svg/kernels/ops/attention_ops_wan.py mirror: dense attention under the element mask expanded from
    the block mask the REFERENCE's generator returns (fixture), like the reference's test_sparse_attn_wan.py"""
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "sparse-videogen_amd"))
    from svg.kernels.ops import attention_ops_wan as W

    g = np.load(str(Path(__file__).parent / "golden" / "triton_golden.npz"))
    bs = int(g[f"wbsr_{F}_{P_}_{mul}_bs"])
    S = F * P_
    nb = S // bs
    blk = torch.from_numpy(np.unpackbits(g[f"wbsr_{F}_{P_}_{mul}"])[: nb * nb].reshape(nb, nb).astype(bool))
    torch.manual_seed(F + P_)
    dt = torch.float16
    q, k, v = (torch.randn(S, heads, D).to(dt) for _ in range(3))
    meta = W.WanFAMetadata(F, P_, W.gen_temporal_mask(F, P_, mul), None)
    assert meta.temporal_mask_metadata[2] == (bs, bs)
    o = W.wan_sparse_attn_forward(q.cuda(), k.cuda(), v.cuda(), meta)
    mask = blk.repeat_interleave(bs, 0).repeat_interleave(bs, 1)
    ref = O.masked_attention(q.permute(1, 0, 2)[None], k.permute(1, 0, 2)[None], v.permute(1, 0, 2)[None], mask)[0].permute(1, 0, 2)
    close(o, ref.to(dt))


@pytest.mark.parametrize("Hq,Hkv,D,S,MB,NB,density,dt", [(4, 4, 64, 256, 10, 50, 0.7, torch.float16), (16, 4, 128, 512, 20, 50, 0.2, torch.bfloat16)])
def test_variable_block_operator_module(Hq, Hkv, D, S, MB, NB, density, dt):
    """svg/kernels/ops/attention_ops_wan_dyn_blk._test_variable_block_sparse_attention — the function the reference's own test calls
    (svg/kernels/test/test_sparse_attn_dyn_blk_wan.py:74-133), with that test's inputs and check (GQA included)"""
    import sys
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "sparse-videogen_amd"))
    from svg.kernels.ops.attention_ops_wan_dyn_blk import _test_variable_block_sparse_attention

    gen = torch.Generator().manual_seed(S + MB)

    def partition(n_blocks):                      # random_partition_batch of the reference's test (:9-36)
        out = torch.empty(Hkv, n_blocks, dtype=torch.int32)
        for i in range(Hkv):
            cuts = torch.sort(torch.randperm(S - 1, generator=gen)[: n_blocks - 1] + 1).values
            out[i] = torch.diff(torch.cat([torch.tensor([0]), cuts, torch.tensor([S])]))
        return out

    rows, cols = partition(MB), partition(NB)
    bmap = torch.rand(Hkv, MB, NB, generator=gen) > density
    q = torch.randn(Hq, S, D, generator=gen).to(dt)
    k, v = torch.randn(Hkv, S, D, generator=gen).to(dt), torch.randn(Hkv, S, D, generator=gen).to(dt)
    o = _test_variable_block_sparse_attention(q.cuda(), k.cuda(), v.cuda(), Hq, Hkv, D, bmap, rows, cols)
    assert o.shape == (Hkv, Hq // Hkv, S, D)
    qg = q.reshape(Hkv, -1, S, D)
    for h in range(Hkv):
        em = O.block_mask_to_element_mask(bmap[h], rows[h], cols[h])
        for gi in range(Hq // Hkv):
            ref = O.masked_attention(qg[h, gi].float(), k[h].float(), v[h].float(), em)
            torch.testing.assert_close(o[h, gi].float().cpu(), ref, atol=1e-2, rtol=1e-2)      # the reference's tolerance (:133)
