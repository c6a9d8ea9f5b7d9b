"""Full-size (HunyuanVideo 720p / 129 frames, S = 119056) checks of the headline kernel through size-independent
properties and spot rows against the oracle (a dense CPU oracle of the whole problem would be 174 TFLOP)."""
import math

import pytest
import torch

from oracle import svg_oracle as O

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)
from poisoned import poisoned_like

pytestmark = pytest.mark.gpu

H, D, F_, P_, CTX, L = 2, 128, 33, 3600, 256, 64
V = F_ * P_
S = V + CTX


@pytest.fixture(scope="module")
def setup():
    from svg import _native as nat

    nat.load()
    torch.manual_seed(0)
    g = torch.Generator(device="cuda").manual_seed(7)
    q, k, v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    width = O.sparsity_to_width(0.25, CTX, F_, P_)
    prm = O.hy_band_params(S, CTX, L, F_, P_, width)
    assert prm["band"] == 15616
    return nat, q, k, v, prm


def _oracle_rows(q, k, v, rows, prm, temporal):
    """Attention output of selected *logical* rows of one head, fp32, under the band mask in logical order."""
    qh, kh, vh = q.float().cpu(), k.float().cpu(), v.float().cpu()
    if temporal:  # logical order = token-major
        def perm(x):
            return torch.cat([x[:V].reshape(F_, P_, D).transpose(0, 1).reshape(V, D), x[V:]])
        qh, kh, vh = perm(qh), perm(kh), perm(vh)
    kk = torch.arange(S)[None, :]
    qq = torch.tensor(rows)[:, None]
    real, band = prm["real_len"], prm["band"]
    rq, rk = qq < real, kk < real
    m = (rq & rk & (((qq - kk).abs() < band) | ((kk >= prm["colfull_lo"]) & (kk < prm["colfull_hi"])) |
                    ((qq >= prm["rowfull_lo"]) & (qq < prm["rowfull_hi"])))) | (~rq & ~rk)
    return O.masked_attention(qh[rows], kh, vh, m)


def test_fullsize_spot_rows_and_fused_equals_materialised(setup):
    nat, q, k, v, prm = setup
    best = torch.tensor([[0, 1]], device="cuda")
    mask = nat.BandMask(**prm)
    o = nat.band_attention(q, k, v, mask, head_perm_flag=best, vid0=0, num_frame=F_, frame_size=P_)
    # (1) fused layout transformation is bit-identical to placement -> attention -> inverse placement
    qp, kp, vp = (poisoned_like(x) for x in (q, k, v))
    nat.head_placement([q, k, v], [qp, kp, vp], best, CTX, F_, P_, False, False)
    om = nat.band_attention(qp, kp, vp, mask)
    oi = poisoned_like(om)
    nat.head_placement([om], [oi], best, CTX, F_, P_, False, True)
    assert torch.equal(oi, o)
    # (2) spot rows (band interior, both band edges, sequence ends, prompt rows, pad rows) against the oracle
    rows = [0, 1, 63, 64, 255, 256, 15615, 15616, 15617, 60000, 60001, V - 15616, V - 1, V, V + 1, V + L - 1, V + L, S - 1]
    rows += torch.randint(0, S, (30,), generator=torch.Generator().manual_seed(1)).tolist()
    for h, temporal in ((0, False), (1, True)):
        ref = _oracle_rows(q[0, h], k[0, h], v[0, h], rows, prm, temporal)
        got = om[0, h].float().cpu()[rows]  # om is in logical order for both heads
        torch.testing.assert_close(got, ref, atol=1e-2, rtol=1e-2)
        assert ((got - ref).norm() / ref.norm()).item() < 3e-3


def test_fullsize_rows_sum_to_one(setup):
    """v = 1 -> every output element is 1 (softmax rows sum to one), for sparse and dense masks."""
    nat, q, k, v, prm = setup
    ones = torch.ones_like(v)
    for m in (prm, O.dense_band_params(S, V + L)):
        o = nat.band_attention(q, k, ones, nat.BandMask(**m))
        assert (o.float() - 1).abs().max().item() <= 2 ** -7


def test_fullsize_linearity_in_v(setup):
    """attention is linear in V: o(v1 + v2) = o(v1) + o(v2) up to bf16 rounding."""
    nat, q, k, v, prm = setup
    mask = nat.BandMask(**prm)
    g = torch.Generator(device="cuda").manual_seed(9)
    v2 = torch.randn(v.shape, device="cuda", dtype=torch.bfloat16, generator=g)
    o1 = nat.band_attention(q, k, v, mask).float()
    o2 = nat.band_attention(q, k, v2, mask).float()
    o12 = nat.band_attention(q, k, (v.float() + v2.float()).to(torch.bfloat16), mask).float()
    err = ((o12 - (o1 + o2)).norm() / (o1 + o2).norm()).item()
    assert err < 6e-3, err


# ---------------------------------------------------------------------------------------------------------
# the other two SVG1 models at their production geometry (the reference's install hooks: svg/models/wan/inference.py:41-44,
# svg/models/cog/inference.py:31-34 with the v1.5 numbers F = 11, P = 4080)
# ---------------------------------------------------------------------------------------------------------
FULLSIZE = {
    # name: (D, F, P, ctx, text_first, sparsity)
    "wan720p": (128, 21, 3600, 0, False, 0.30),
    "cog15_768p": (64, 11, 4080, 226, True, 0.25),
}


@pytest.mark.parametrize("model", sorted(FULLSIZE))
def test_fullsize_spot_rows_wan_cog(model):
    """Wan 2.1 720p (S = 75600: `<=` band of ceil'ed width + first-frame sink columns, no text) and CogVideoX-v1.5 (S = 45106,
    D = 64, text FIRST) at full size: (1) the fused layout transformation equals placement -> attention -> inverse placement bit
    for bit, (2) spot rows of a spatial and a temporal head — band edges, sink / text columns, sequence ends — against the oracle
    under the REFERENCE's mask predicate (svg/models/wan/utils.py:25-41, svg/models/cog/utils.py:30-46) evaluated on those rows."""
    from svg import _native as nat

    nat.load()
    D_, F2, P2, ctx, text_first, sparsity = FULLSIZE[model]
    V2 = F2 * P2
    S2 = V2 + ctx
    vid0 = ctx if text_first else 0
    mul = O.sparsity_to_width(sparsity, ctx, F2, P2)
    if model == "wan720p":
        prm = O.wan_band_params(S2, F2, P2, mul)
        assert prm["band"] == 12416 + 1
        ref_mask = lambda rows: O.wan_mask(S2, F2, P2, mul, rows=rows)        # noqa: E731
        edge = 12416
    else:
        prm = O.cog_band_params(S2, ctx, F2, P2, mul)
        ref_mask = lambda rows: O.cog_mask(S2, ctx, F2, P2, mul, rows=rows)   # noqa: E731
        edge = prm["band"]
    g = torch.Generator(device="cuda").manual_seed(17)
    q, k, v = (torch.randn(1, 2, S2, D_, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    best = torch.tensor([[0, 1]], device="cuda")
    mask = nat.BandMask(**prm)
    o = nat.band_attention(q, k, v, mask, head_perm_flag=best, vid0=vid0, num_frame=F2, frame_size=P2)
    qp, kp, vp = (poisoned_like(x) for x in (q, k, v))
    nat.head_placement([q, k, v], [qp, kp, vp], best, ctx, F2, P2, text_first, False)
    om = nat.band_attention(qp, kp, vp, mask)
    oi = poisoned_like(om)
    nat.head_placement([om], [oi], best, ctx, F2, P2, text_first, True)
    assert torch.equal(oi, o)
    rows = [0, 1, vid0, vid0 + 1, P2 - 1, P2, P2 + 1, vid0 + edge - 1, vid0 + edge, vid0 + edge + 1, S2 // 2, S2 // 2 + 1,
            S2 - edge - 2, S2 - edge - 1, S2 - edge, S2 - 2, S2 - 1]
    if ctx:
        rows += [ctx - 1, ctx, ctx + 1]
    rows += torch.randint(0, S2, (24,), generator=torch.Generator().manual_seed(3)).tolist()
    m = ref_mask(rows)

    def logical(x):   # token order the mask is applied in: temporal heads are token-major inside the video part
        x = x.float().cpu()
        vidp = x[vid0:vid0 + V2].reshape(F2, P2, D_).transpose(0, 1).reshape(V2, D_)
        return torch.cat([x[:vid0], vidp, x[vid0 + V2:]])

    for h, temporal in ((0, False), (1, True)):
        qh, kh, vh = ((logical(x[0, h]) if temporal else x[0, h].float().cpu()) for x in (q, k, v))
        ref = O.masked_attention(qh[rows], kh, vh, m)
        got = om[0, h].float().cpu()[rows]     # om is in logical order for both heads
        torch.testing.assert_close(got, ref, atol=1e-2, rtol=1e-2)
        assert ((got - ref).norm() / ref.norm()).item() < 3e-3


# ---------------------------------------------------------------------------------------------------------
# online profiler (sample_mse) at the production geometries against the oracle: the kernel was rewritten in
# round 5 and was held to the oracle only at S <= 8532.  A full profiling mask is [S, S] (56 GB at HunyuanVideo 720p): the oracle
# evaluates the sampled ROWS of the two masks (O.profile_mask_rows == rows of O.profile_masks, tests/test_oracle_golden.py).
# ref: svg/models/hyvideo/attention.py:376-399, svg/models/hyvideo/utils.py:47-93 (wan/utils.py:63-110, cog/utils.py:61-88)
# ---------------------------------------------------------------------------------------------------------
PROFILE_GEOM = {
    # name: (oracle model, BH, D, F, P, ctx, sampled rows, sample_max_row)   — the install hooks' numbers
    "hy720p": ("hy", 24, 128, 33, 3600, 256, 64, 10000),
    "wan720p": ("wan", 40, 128, 21, 3600, 0, 64, 10000),
    "cog15_768p": ("cog", 96, 64, 11, 4080, 226, 32, 45106),        # cfg 2 x 48 heads
}


def _profile_desc(nat, model, ctx, F2, P2, emulate):
    V2 = F2 * P2
    pv = nat.ProfileVariant
    if model == "hy":
        bb = int((P2 * 1.5) // 128)
        var, vid0 = (pv(0, 0, V2, bb, 0, V2, V2 + ctx), pv(1, 0, V2, bb, 0, V2, V2 + ctx)), 0
    elif model == "wan":
        bb = int((P2 * 2) // 128)
        var, vid0 = (pv(0, 0, V2, bb, P2, 0, 0), pv(1, 0, V2, bb, P2, 0, 0)), 0
    else:
        bb = int((P2 * 1.5) // 128)
        span = min(V2 + ctx, math.ceil(V2 / 128) * 128)
        var, vid0 = (pv(0, 0, span, bb, 0, 0, ctx), pv(1, ctx, V2, bb, 0, 0, 0)), ctx
    d = nat.ProfileDesc(vid0, F2, P2, int(emulate))
    d.variant[0], d.variant[1] = var
    return d


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("name", sorted(PROFILE_GEOM))
def test_fullsize_sample_mse_vs_oracle(name, dtype):
    """every head of the model at full sequence length; structured data (even heads: q / k share a per-POSITION component — most of a
    row's softmax mass sits on its position in the other frames, the temporal mask's keys; odd heads: a per-FRAME component — the mass
    sits in the row's own frame, the spatial mask's) so that both decisions occur; mse within 3e-2 of the fp32 oracle and the same
    argmin on every head"""
    from svg import _native as nat

    nat.load()
    model, BH, D_, F2, P2, ctx, R, max_row = PROFILE_GEOM[name]
    V2 = F2 * P2
    S2 = V2 + ctx
    vid0 = ctx if model == "cog" else 0
    g = torch.Generator(device="cuda").manual_seed(23)
    q, k, v = (torch.randn(BH, S2, D_, device="cuda", generator=g) for _ in range(3))
    pos = torch.randn(BH, 1, P2, D_, device="cuda", generator=g)
    frm = torch.randn(BH, F2, 1, D_, device="cuda", generator=g)
    kind = torch.arange(BH, device="cuda") % 2
    add = (pos * (kind == 0)[:, None, None, None] + frm * (kind == 1)[:, None, None, None]).reshape(BH, V2, D_)   # +sqrt(D) in logit
    q[:, vid0:vid0 + V2] += add
    k[:, vid0:vid0 + V2] += add
    del add
    q, k, v = (x.to(dtype) for x in (q, k, v))
    rows = torch.randint(vid0, min(max_row, vid0 + V2), (R,), generator=torch.Generator().manual_seed(5))
    got = nat.sample_mse(q, k, v, rows.cuda(), _profile_desc(nat, model, ctx, F2, P2, False)).cpu()
    got_em = nat.sample_mse(q, k, v, rows.cuda(), _profile_desc(nat, model, ctx, F2, P2, True)).cpu()
    masks = list(O.profile_mask_rows(model, ctx, F2, P2, rows))
    ref = torch.empty(2, BH)
    for h0 in range(0, BH, 8):      # 8 heads at a time: the fp32 scores of all 96 CogVideoX heads would be 1.1 GB, fine, but q/k/v in fp32 too
        sl = slice(h0, min(BH, h0 + 8))
        ref[:, sl] = O.sample_mse_fp32(q[None, sl].cpu(), k[None, sl].cpu(), v[None, sl].cpu(), rows, masks, True)[:, 0]
    assert torch.isfinite(ref).all() and torch.isfinite(got).all() and torch.isfinite(got_em).all()
    torch.testing.assert_close(got, ref, rtol=3e-2, atol=1e-7)
    assert torch.all((ref[0] - ref[1]).abs() > 0.1 * ref.max(0).values), "the case is built so that no head is a near-tie"
    assert torch.equal(got.argmin(0), ref.argmin(0))
    assert torch.equal(got_em.argmin(0), ref.argmin(0))     # the torch-rounding emulation (the reference computes in the 16-bit type) decides alike
    best = ref.argmin(0)
    assert torch.equal(best, (torch.arange(BH) % 2 == 0).long()), "even heads temporal, odd heads spatial, as constructed"
    # (a head's MSE under its RIGHT mask can be ~1e-7 — the mask holds nearly all of the softmax mass —: errors are shown against the
    #  tolerance the assertion above applies, rtol * |ref| + atol, 1.0 = at the bound)
    print(f"[sample_mse {name} {dtype}] temporal heads {int(best.sum())} / {BH}; worst |got - ref| / (3e-2 |ref| + 1e-7) = "
          f"{((got - ref).abs() / (3e-2 * ref.abs() + 1e-7)).max().item():.3f}; mse range {ref.min().item():.2e} .. {ref.max().item():.2e}")
