"""svg_cross_attention on the GPU: dense attention of Sq query rows over a short key set (csrc/attention_cross.hip, cross_policy.h) against
the CPU oracle, bit-exact strided / token-major layouts, the resident-workgroup loop, the bounds of what the kernel reads and writes, the
overflow path of the max-free softmax, the Wan 2.1 720p production shapes, and the Wan / Cosmos processors' routing.

ref: the cross-attention branch of the reference's processors, F.scaled_dot_product_attention with attn_mask None
(svg/models/wan/attention.py:174-188,198-201, svg/models/cosmos/attention.py:104-107)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import svg_oracle as O
from test_gpu_kernels import check_attn, dev, rel_l2
from poisoned import poisoned_like

pytestmark = pytest.mark.gpu
DT = torch.bfloat16


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _qkv(B, H, Sq, Skv, dtype, seed, D=128):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g).to(dtype)
    k, v = (torch.randn(B, H, Skv, D, generator=g).to(dtype) for _ in range(2))
    return q, k, v


# ---------------------------------------------------------------------------------------------------------
# parity against the oracle
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("Sq", [1, 255, 256, 800, 2049])
@pytest.mark.parametrize("Skv", [1, 37, 64, 65, 257, 512, 1000])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cross_attention_matches_oracle(nat, dtype, Skv, Sq, B, H):
    q, k, v = _qkv(B, H, Sq, Skv, dtype, seed=Sq * 1009 + Skv)
    o = nat.cross_attention(dev(q), dev(k), dev(v))
    assert o.shape == q.shape and o.dtype == dtype and o.is_contiguous()
    ref = O.masked_attention(q, k, v, None)
    print(f"rel_l2 {rel_l2(o.cpu(), ref):.3e}")
    check_attn(o, ref, dtype)


def test_cross_attention_takes_bh_s_d_and_a_scale(nat):
    q, k, v = _qkv(1, 3, 300, 77, DT, seed=1)
    o = nat.cross_attention(dev(q[0]), dev(k[0]), dev(v[0]), sm_scale=0.05)
    assert o.shape == (3, 300, 128)
    check_attn(o, O.masked_attention(q[0], k[0], v[0], None, scale=0.05), DT)


# ---------------------------------------------------------------------------------------------------------
# layouts: bit-exact against the contiguous call
# ---------------------------------------------------------------------------------------------------------
def _is_token_major(o):
    return o.transpose(1, 2).is_contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Sq,Skv", [(700, 512), (257, 257), (1300, 77)])
def test_cross_attention_strided_equals_contiguous(nat, Sq, Skv, dtype):
    B, H, D = 2, 3, 128
    g = torch.Generator().manual_seed(Sq + Skv)
    q = dev(torch.randn(B, Sq, H * D, generator=g).to(dtype)).unflatten(2, (H, D)).transpose(1, 2)      # projection views [B, S, H * D]
    k, v = (dev(torch.randn(B, Skv, H * D, generator=g).to(dtype)).unflatten(2, (H, D)).transpose(1, 2) for _ in range(2))
    assert not q.is_contiguous() and not k.is_contiguous()
    ref = nat.cross_attention(q.contiguous(), k.contiguous(), v.contiguous())
    check_attn(ref, O.masked_attention(q.cpu(), k.cpu(), v.cpu(), None), dtype)
    o = nat.cross_attention(q, k, v, token_major_out=True)            # everything strided, o token-major
    assert o.shape == ref.shape and _is_token_major(o) and torch.equal(o, ref)
    flat = o.transpose(1, 2).flatten(2, 3)                            # the processors' next line: a view
    assert flat.data_ptr() == o.data_ptr() and flat.shape == (B, Sq, H * D)
    o2 = nat.cross_attention(q, k, v)                                  # strided in, head-major out
    assert o2.is_contiguous() and torch.equal(o2, ref)
    kv = dev(torch.randn(B, Skv, 2 * H * D, generator=g).to(dtype))    # k and v as slices of one fused [B, Skv, 2 * H * D] projection
    k2, v2 = (kv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(2))
    ref2 = nat.cross_attention(q.contiguous(), k2.contiguous(), v2.contiguous())
    o3 = nat.cross_attention(q, k2, v2, token_major_out=True)
    assert _is_token_major(o3) and torch.equal(o3, ref2)
    out = poisoned_like(ref)                                          # a caller's buffer
    assert nat.cross_attention(q, k, v, out=out) is out and torch.equal(out, ref)


def test_cross_attention_copies_views_the_layout_cannot_describe(nat):
    q, k, v = _qkv(1, 2, 300, 64, DT, seed=5)
    qd = dev(torch.cat([q, q], dim=-1))[..., 1:129]                    # 2-byte aligned rows: not a layout the entry takes
    assert qd.data_ptr() % 16 != 0
    ref = nat.cross_attention(qd.contiguous(), dev(k), dev(v))
    assert torch.equal(nat.cross_attention(qd, dev(k), dev(v)), ref)


# ---------------------------------------------------------------------------------------------------------
# resident loop: more work items than compute units
# ---------------------------------------------------------------------------------------------------------
def test_cross_attention_resident_loop(nat):
    B, H, Sq, Skv = 1, 8, 25600, 512                                   # 800 work items: every workgroup runs several q-tiles
    q, k, v = _qkv(B, H, Sq, Skv, DT, seed=11)
    dq, dk, dv = dev(q), dev(k), dev(v)
    o = nat.cross_attention(dq, dk, dv)
    o_again = nat.cross_attention(dq, dk, dv)
    torch.cuda.synchronize()
    assert torch.equal(o, o_again)
    oc = o.cpu()
    for h in range(H):
        check_attn(oc[:, h], O.masked_attention(q[:, h], k[:, h], v[:, h], None), DT)


# ---------------------------------------------------------------------------------------------------------
# what the kernel reads and writes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Skv", [37, 257])
def test_keys_behind_skv_are_not_read(nat, Skv):
    B, H, Sq, pad = 2, 3, 700, 91
    q, k, v = _qkv(B, H, Sq, Skv, DT, seed=Skv)
    nan = torch.full((B, H, pad, 128), float("nan"), dtype=DT)
    kb, vb = dev(torch.cat([k, nan], dim=2)), dev(torch.cat([v, nan], dim=2))
    kv_, vv = kb[:, :, :Skv], vb[:, :, :Skv]
    assert not kv_.is_contiguous() and torch.isnan(kb[:, :, Skv:]).all()
    o = nat.cross_attention(dev(q), kv_, vv)
    ref = nat.cross_attention(dev(q), kv_.contiguous(), vv.contiguous())
    assert torch.isfinite(o.float()).all() and torch.equal(o, ref)
    check_attn(o, O.masked_attention(q, k, v, None), DT)


@pytest.mark.parametrize("Sq", [300, 512, 1])
def test_every_row_is_written_and_nothing_else(nat, Sq):
    B, H, Skv, pad, sentinel = 2, 3, 130, 300, -77.0
    q, k, v = _qkv(B, H, Sq, Skv, DT, seed=Sq)
    big = torch.full((B, H, Sq + pad, 128), sentinel, dtype=DT, device="cuda")
    out = big[:, :, :Sq]
    r = nat.cross_attention(dev(q), dev(k), dev(v), out=out)
    torch.cuda.synchronize()
    assert r is out
    assert (big[:, :, Sq:] == sentinel).all()
    assert not (out == sentinel).any() and torch.isfinite(out.float()).all()
    check_attn(out, O.masked_attention(q, k, v, None), DT)


# ---------------------------------------------------------------------------------------------------------
# large logits: the overflow path of the max-free softmax
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_large_logits_with_one_dominant_key(nat, dtype):
    B, H, Sq, Skv, D = 1, 2, 600, 512, 128
    g = torch.Generator().manual_seed(3)
    k = torch.randn(B, H, Skv, D, generator=g)
    v = torch.randn(B, H, Skv, D, generator=g)
    pick = torch.randint(0, Skv, (B, H, Sq), generator=g)              # the dominant key of a row: anywhere, so in any key tile
    q = 10.0 * torch.gather(k, 2, pick[..., None].expand(B, H, Sq, D)) + 0.1 * torch.randn(B, H, Sq, D, generator=g)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    logits = torch.matmul(q.float(), k.float().transpose(-1, -2)) / D ** 0.5
    top2 = logits.topk(2, dim=-1).values
    assert top2[..., 0].min() > 60 and (top2[..., 0] - top2[..., 1]).min() > 20 and (logits.argmax(-1) == pick).all()
    o = nat.cross_attention(dev(q), dev(k), dev(v))
    assert torch.isfinite(o.float()).all()
    check_attn(o, O.masked_attention(q, k, v, None), dtype)


# ---------------------------------------------------------------------------------------------------------
# production size: Wan 2.1 14B 720p, text keys and I2V image keys
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Skv", [512, 257])
def test_wan_720p_shape_spot_rows(nat, Skv):
    H, Sq, D, n_spot = 40, 75600, 128, 512
    g = torch.Generator(device="cuda").manual_seed(Skv)
    q = torch.randn(1, Sq, H * D, generator=g, device="cuda", dtype=torch.float32).to(DT).unflatten(2, (H, D)).transpose(1, 2)
    k, v = (torch.randn(1, Skv, H * D, generator=g, device="cuda", dtype=torch.float32).to(DT).unflatten(2, (H, D)).transpose(1, 2)
            for _ in range(2))
    o = nat.cross_attention(q, k, v, token_major_out=True)             # the processors' call: head views in, token-major out
    torch.cuda.synchronize()
    assert _is_token_major(o)
    rows = torch.randperm(Sq, generator=torch.Generator().manual_seed(0))[:n_spot - 4].sort().values
    rows = torch.cat([torch.tensor([0, 255, 256]), rows, torch.tensor([Sq - 1])])   # tile seams and the ragged last q-tile
    ref = O.masked_attention(q[:, :, rows.cuda()].cpu(), k.cpu(), v.cpu(), None)
    check_attn(o[:, :, rows.cuda()], ref, DT)


# ---------------------------------------------------------------------------------------------------------
# processors
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def kernel_calls(nat, monkeypatch):
    """counts the calls of _native.cross_attention (the kernel path of _core.cross_attention)"""
    calls = []
    real = nat.cross_attention

    def counted(*a, **kw):
        calls.append(a[0].shape)
        return real(*a, **kw)

    monkeypatch.setattr(nat, "cross_attention", counted)
    return calls


def _sdpa_only(monkeypatch):
    """_core.cross_attention replaced by the call the processors made before the kernel existed"""
    from svg.models import _core

    monkeypatch.setattr(_core, "cross_attention", lambda q, k, v, attention_mask=None: F.scaled_dot_product_attention(
        q, k, v, attn_mask=attention_mask, dropout_p=0.0, is_causal=False))


def _wan_attn(heads, hd, i2v):
    from standins import Attention, RMSNorm

    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanP

    dim = heads * hd
    attn = Attention(dim, heads, qk_norm="rms", across_heads=True, dtype=DT)
    if i2v:
        attn.add_k_proj, attn.add_v_proj, attn.norm_added_k = torch.nn.Linear(dim, dim), torch.nn.Linear(dim, dim), RMSNorm(dim)
    attn.to(DT).cuda()
    attn.set_processor(WanP(0))
    return attn


def _wan_reference(attn, hidden, enc, heads, i2v):
    """the fp32 torch restatement of test_gpu_processors.py::test_wan_i2v_image_cross_attention_branch_and_fp8"""
    a = attn.cpu().float()
    x, e = hidden.float().cpu(), enc.float().cpu()
    split = lambda t: t.unflatten(2, (heads, -1)).transpose(1, 2)   # noqa: E731
    e_txt = e[:, 257:] if i2v else e
    q = split(a.norm_q(a.to_q(x)))
    o = F.scaled_dot_product_attention(q, split(a.norm_k(a.to_k(e_txt))), split(a.to_v(e_txt)))
    if i2v:
        e_img = e[:, :257]
        o = o + F.scaled_dot_product_attention(q, split(a.norm_added_k(a.add_k_proj(e_img))), split(a.add_v_proj(e_img)))
    ref = a.to_out[0](o.transpose(1, 2).flatten(2, 3))
    attn.to(DT).cuda()
    return ref


@pytest.mark.parametrize("i2v", [False, True])
def test_wan_cross_attention_runs_the_kernel(kernel_calls, i2v):
    torch.manual_seed(2)
    heads, hd, S, n_txt = 2, 128, 800, 40
    attn = _wan_attn(heads, hd, i2v)
    hidden = (torch.randn(1, S, heads * hd) * 0.3).to(DT).cuda()
    enc = (torch.randn(1, (257 if i2v else 0) + n_txt, heads * hd) * 0.3).to(DT).cuda()
    with torch.no_grad():
        out = attn(hidden, encoder_hidden_states=enc)
        ref = _wan_reference(attn, hidden, enc, heads, i2v)
    assert len(kernel_calls) == (2 if i2v else 1) and all(s == (1, heads, S, hd) for s in kernel_calls)
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


def test_wan_cross_attention_head_dim_64_stays_on_sdpa(kernel_calls, monkeypatch):
    torch.manual_seed(3)
    heads, hd, S = 4, 64, 800
    attn = _wan_attn(heads, hd, True)
    hidden = (torch.randn(1, S, heads * hd) * 0.3).to(DT).cuda()
    enc = (torch.randn(1, 257 + 40, heads * hd) * 0.3).to(DT).cuda()
    with torch.no_grad():
        out = attn(hidden, encoder_hidden_states=enc)
        assert len(kernel_calls) == 0
        _sdpa_only(monkeypatch)
        assert torch.equal(out, attn(hidden, encoder_hidden_states=enc))


def test_wan_cross_attention_with_a_mask_stays_on_sdpa(kernel_calls, monkeypatch):
    torch.manual_seed(4)
    heads, hd, S, n_txt = 2, 128, 800, 40
    attn = _wan_attn(heads, hd, False)
    hidden = (torch.randn(1, S, heads * hd) * 0.3).to(DT).cuda()
    enc = (torch.randn(1, n_txt, heads * hd) * 0.3).to(DT).cuda()
    mask = torch.ones(1, 1, 1, n_txt, dtype=torch.bool, device="cuda")
    mask[..., 25:] = False
    with torch.no_grad():
        out = attn(hidden, encoder_hidden_states=enc, attention_mask=mask)
        assert len(kernel_calls) == 0
        _sdpa_only(monkeypatch)
        assert torch.equal(out, attn(hidden, encoder_hidden_states=enc, attention_mask=mask))


def test_cosmos_cross_attention_runs_the_kernel(kernel_calls):
    from standins import Attention

    from svg.models.cosmos.attention import Cosmos_SVG_AttnProcessor2_0 as CosP

    torch.manual_seed(5)
    heads, hd, S, n_txt = 2, 128, 800, 77
    dim = heads * hd
    attn = Attention(dim, heads, qk_norm="rms", dtype=DT).cuda()      # per-head RMSNorm(hd)
    attn.set_processor(CosP(0))
    hidden = (torch.randn(1, S, dim) * 0.3).to(DT).cuda()
    enc = (torch.randn(1, n_txt, dim) * 0.3).to(DT).cuda()
    with torch.no_grad():
        out = attn(hidden, encoder_hidden_states=enc, timestep=None)
        a = attn.cpu().float()
        x, e = hidden.float().cpu(), enc.float().cpu()
        split = lambda t: t.unflatten(2, (heads, -1)).transpose(1, 2)   # noqa: E731
        q, k, v = a.norm_q(split(a.to_q(x))), a.norm_k(split(a.to_k(e))), split(a.to_v(e))
        ref = a.to_out[0](F.scaled_dot_product_attention(q, k, v).transpose(1, 2).flatten(2, 3))
    assert kernel_calls == [(1, heads, S, hd)]
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


def test_cosmos_cross_attention_head_dim_64_stays_on_sdpa(kernel_calls, monkeypatch):
    from standins import Attention

    from svg.models.cosmos.attention import Cosmos_SVG_AttnProcessor2_0 as CosP

    torch.manual_seed(6)
    heads, hd, S = 4, 64, 800
    attn = Attention(heads * hd, heads, qk_norm="rms", dtype=DT).cuda()
    attn.set_processor(CosP(0))
    hidden = (torch.randn(1, S, heads * hd) * 0.3).to(DT).cuda()
    enc = (torch.randn(1, 77, heads * hd) * 0.3).to(DT).cuda()
    with torch.no_grad():
        out = attn(hidden, encoder_hidden_states=enc, timestep=None)
        assert len(kernel_calls) == 0
        _sdpa_only(monkeypatch)
        assert torch.equal(out, attn(hidden, encoder_hidden_states=enc, timestep=None))
