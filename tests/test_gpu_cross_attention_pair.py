"""svg_cross_attention_pair on the GPU: cross attention over two key sets in one launch (csrc/attention_cross.hip, CrossPairPolicy of
cross_policy.h, the add-on-store of attn_m16.h) — the text and the image keys of a Wan I2V block.  The acceptance criterion is bit
equality with the path it replaces: cross_attention(q, k_a, v_a) + cross_attention(q, k_b, v_b), two launches and torch's 16-bit add.
That path is the reference of every test here; no tolerance is involved.

ref: svg/models/wan/attention.py:174-188,198-201 (the two scaled_dot_product_attention calls) and :210-229 (the add)."""
import pytest
import torch
from poisoned import poisoned_like

pytestmark = pytest.mark.gpu
DT = torch.bfloat16
D = 128


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _rand(shape, dtype, g, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).cuda()


def _sets(B, H, Sq, Skv_a, Skv_b, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (_rand((B, H, Sq, D), dtype, g),) + tuple(_rand((B, H, S, D), dtype, g) for S in (Skv_a, Skv_a, Skv_b, Skv_b))


def two_launches(nat, q, ka, va, kb, vb, **kw):
    """the parent's path: two svg_cross_attention launches and torch's add"""
    return nat.cross_attention(q, ka, va, **kw) + nat.cross_attention(q, kb, vb, **kw)


def _is_token_major(o):
    return o.transpose(1, 2).is_contiguous()


# ---------------------------------------------------------------------------------------------------------
# bit equality with the two-launch path
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Skv_a,Skv_b", [(40, 257), (512, 257), (64, 1), (65, 64), (1, 1000)])
@pytest.mark.parametrize("Sq", [1, 255, 256, 257, 800])
@pytest.mark.parametrize("B,H", [(1, 1), (2, 3)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pair_equals_two_launches_and_the_add(nat, dtype, B, H, Sq, Skv_a, Skv_b):
    q, ka, va, kb, vb = _sets(B, H, Sq, Skv_a, Skv_b, dtype, seed=Sq * 1009 + Skv_a * 31 + Skv_b)
    o = nat.cross_attention_pair(q, ka, va, kb, vb)
    assert o.shape == q.shape and o.dtype == dtype and o.is_contiguous()
    assert torch.equal(o, two_launches(nat, q, ka, va, kb, vb))


def test_pair_takes_bh_s_d_and_a_scale(nat):
    q, ka, va, kb, vb = (t[0] for t in _sets(1, 3, 300, 77, 130, DT, seed=1))
    o = nat.cross_attention_pair(q, ka, va, kb, vb, sm_scale=0.05)
    assert o.shape == (3, 300, D)
    assert torch.equal(o, two_launches(nat, q, ka, va, kb, vb, sm_scale=0.05))


# ---------------------------------------------------------------------------------------------------------
# layouts: bit-exact against the contiguous call
# ---------------------------------------------------------------------------------------------------------
def _proj_views(B, H, S, dtype, g, fused=1):
    """head views of a [B, S, fused * H * D] projection output, one per fused slice"""
    buf = _rand((B, S, fused * H * D), dtype, g)
    return [buf[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(fused)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Sq,Skv_a,Skv_b", [(700, 512, 257), (257, 40, 257), (1300, 77, 64)])
def test_pair_strided_equals_contiguous(nat, Sq, Skv_a, Skv_b, dtype):
    B, H = 2, 3
    g = torch.Generator().manual_seed(Sq + Skv_a + Skv_b)
    q, = _proj_views(B, H, Sq, dtype, g)
    ka, va = _proj_views(B, H, Skv_a, dtype, g) + _proj_views(B, H, Skv_a, dtype, g)
    kb, vb = _proj_views(B, H, Skv_b, dtype, g) + _proj_views(B, H, Skv_b, dtype, g)      # set B: buffers of another Skv, another batch stride
    assert not q.is_contiguous() and ka.stride(0) != kb.stride(0)
    cont = [t.contiguous() for t in (q, ka, va, kb, vb)]
    ref = nat.cross_attention_pair(*cont)
    assert torch.equal(ref, two_launches(nat, *cont))
    o = nat.cross_attention_pair(q, ka, va, kb, vb, token_major_out=True)                  # everything strided, o token-major
    assert o.shape == ref.shape and _is_token_major(o) and torch.equal(o, ref)
    flat = o.transpose(1, 2).flatten(2, 3)                                                 # the processors' next line: a view
    assert flat.data_ptr() == o.data_ptr() and flat.shape == (B, Sq, H * D)
    o2 = nat.cross_attention_pair(q, ka, va, kb, vb)                                       # strided in, head-major out
    assert o2.is_contiguous() and torch.equal(o2, ref)
    assert torch.equal(nat.cross_attention_pair(q, cont[1], cont[2], kb, vb), ref)         # only set B strided
    assert torch.equal(nat.cross_attention_pair(q, ka, va, cont[3], cont[4]), ref)         # only set A strided
    ka2, va2 = _proj_views(B, H, Skv_a, dtype, g, fused=2)                                 # k and v as slices of one fused kv projection, either set
    kb2, vb2 = _proj_views(B, H, Skv_b, dtype, g, fused=2)
    assert ka2.stride(2) == 2 * H * D and ka.stride(2) == H * D
    ref_a = two_launches(nat, cont[0], ka2.contiguous(), va2.contiguous(), cont[3], cont[4])
    o3 = nat.cross_attention_pair(q, ka2, va2, kb, vb, token_major_out=True)
    assert _is_token_major(o3) and torch.equal(o3, ref_a)
    ref_b = two_launches(nat, cont[0], cont[1], cont[2], kb2.contiguous(), vb2.contiguous())
    assert torch.equal(nat.cross_attention_pair(q, ka, va, kb2, vb2, token_major_out=True), ref_b)
    out = poisoned_like(ref)                                                              # a caller's buffer
    assert nat.cross_attention_pair(q, ka, va, kb, vb, out=out) is out and torch.equal(out, ref)
    out_tm = nat.token_major_empty(ref)
    assert nat.cross_attention_pair(q, ka, va, kb, vb, out=out_tm) is out_tm and torch.equal(out_tm, ref)


@pytest.mark.parametrize("which", ["q", "k_b", "v_a"])
def test_pair_copies_views_the_layout_cannot_describe(nat, which):
    ts = dict(zip(("q", "k_a", "v_a", "k_b", "v_b"), _sets(1, 2, 300, 64, 257, DT, seed=5)))
    ref = two_launches(nat, *ts.values())
    t = ts[which]
    ts[which] = torch.cat([t, t], dim=-1)[..., 1:129]                  # 2-byte aligned rows: not a layout the entry takes
    assert ts[which].data_ptr() % 16 != 0
    ref_odd = two_launches(nat, *(x.contiguous() for x in ts.values()))
    assert not torch.equal(ref_odd, ref)
    assert torch.equal(nat.cross_attention_pair(*ts.values()), ref_odd)


def test_pair_writes_through_an_out_the_layout_cannot_describe(nat):
    q, ka, va, kb, vb = _sets(1, 2, 300, 64, 257, DT, seed=6)
    big = torch.zeros(1, 2, 300, 2 * D, dtype=DT, device="cuda")
    out = big[..., 1:129]
    assert nat.cross_attention_pair(q, ka, va, kb, vb, out=out) is out
    assert torch.equal(out, two_launches(nat, q, ka, va, kb, vb)) and (big[..., 129:] == 0).all() and (big[..., :1] == 0).all()


# ---------------------------------------------------------------------------------------------------------
# resident loop: more work items than compute units
# ---------------------------------------------------------------------------------------------------------
def test_pair_resident_loop(nat):
    B, H, Sq = 2, 3, 12800                                             # BH 6 x 50 q-tiles = 300 work items: workgroups run several
    q, ka, va, kb, vb = _sets(B, H, Sq, 512, 257, DT, seed=11)
    assert B * H * ((Sq + 255) // 256) > torch.cuda.get_device_properties(0).multi_processor_count
    o = nat.cross_attention_pair(q, ka, va, kb, vb)
    o_again = nat.cross_attention_pair(q, ka, va, kb, vb)
    ref = two_launches(nat, q, ka, va, kb, vb)
    torch.cuda.synchronize()
    assert torch.equal(o, ref) and torch.equal(o_again, ref)


# ---------------------------------------------------------------------------------------------------------
# what the kernel reads and writes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Sq", [1, 300, 512])
def test_every_row_is_written_and_nothing_else(nat, Sq):
    B, H, pad, sentinel = 2, 3, 300, -77.0
    q, ka, va, kb, vb = _sets(B, H, Sq, 130, 257, DT, seed=Sq)
    ref = two_launches(nat, q, ka, va, kb, vb)
    big = torch.full((B, H, Sq + pad, D), sentinel, dtype=DT, device="cuda")
    out = big[:, :, :Sq]
    r = nat.cross_attention_pair(q, ka, va, kb, vb, out=out)
    torch.cuda.synchronize()
    assert r is out
    assert (big[:, :, Sq:] == sentinel).all()
    assert not (out == sentinel).any() and torch.isfinite(out.float()).all()
    assert torch.equal(out, ref)                                       # (the sentinel in o before the launch is not added to anything)


@pytest.mark.parametrize("padded", ["a", "b"])
@pytest.mark.parametrize("Skv", [37, 257])
def test_keys_behind_skv_are_not_read(nat, Skv, padded):
    B, H, Sq, pad, other = 2, 3, 700, 91, 130
    Skv_a, Skv_b = (Skv, other) if padded == "a" else (other, Skv)
    q, ka, va, kb, vb = _sets(B, H, Sq, Skv_a, Skv_b, DT, seed=Skv)
    ref = two_launches(nat, q, ka, va, kb, vb)
    nan = torch.full((B, H, pad, D), float("nan"), dtype=DT, device="cuda")
    k, v = (ka, va) if padded == "a" else (kb, vb)
    k_buf, v_buf = torch.cat([k, nan], dim=2), torch.cat([v, nan], dim=2)
    kv_, vv = k_buf[:, :, :Skv], v_buf[:, :, :Skv]
    assert not kv_.is_contiguous() and torch.isnan(k_buf[:, :, Skv:]).all()
    o = nat.cross_attention_pair(q, kv_, vv, kb, vb) if padded == "a" else nat.cross_attention_pair(q, ka, va, kv_, vv)
    assert torch.isfinite(o.float()).all() and torch.equal(o, ref)


# ---------------------------------------------------------------------------------------------------------
# large logits in one set only: the overflow path of the max-free softmax, in one pass and not in the other
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dominant", ["a", "b"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_one_dominant_key_in_one_set(nat, dtype, dominant):
    B, H, Sq = 1, 2, 600
    Skv_a, Skv_b = 512, 257
    g = torch.Generator().manual_seed(3)
    ka, va, kb, vb = (torch.randn(B, H, S, D, generator=g) for S in (Skv_a, Skv_a, Skv_b, Skv_b))
    k_dom = ka if dominant == "a" else kb
    pick = torch.randint(0, k_dom.shape[2], (B, H, Sq), generator=g)   # the dominant key of a row: anywhere, so in any key tile
    q = 10.0 * torch.gather(k_dom, 2, pick[..., None].expand(B, H, Sq, D)) + 0.1 * torch.randn(B, H, Sq, D, generator=g)
    q, ka, va, kb, vb = (t.to(dtype) for t in (q, ka, va, kb, vb))
    logits = torch.matmul(q.float(), (ka if dominant == "a" else kb).float().transpose(-1, -2)) / D ** 0.5
    top2 = logits.topk(2, dim=-1).values
    assert top2[..., 0].min() > 60 and (top2[..., 0] - top2[..., 1]).min() > 20 and (logits.argmax(-1) == pick).all()
    dev = [t.cuda() for t in (q, ka, va, kb, vb)]
    o = nat.cross_attention_pair(*dev)
    assert torch.isfinite(o.float()).all() and torch.equal(o, two_launches(nat, *dev))


# ---------------------------------------------------------------------------------------------------------
# processors
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def kernel_calls(nat, monkeypatch):
    """the calls of _native.cross_attention_pair and of _native.cross_attention, by name"""
    calls = []
    real_pair, real = nat.cross_attention_pair, nat.cross_attention

    def counted_pair(*a, **kw):
        calls.append(("pair", tuple(a[0].shape)))
        return real_pair(*a, **kw)

    def counted(*a, **kw):
        calls.append(("single", tuple(a[0].shape)))
        return real(*a, **kw)

    monkeypatch.setattr(nat, "cross_attention_pair", counted_pair)
    monkeypatch.setattr(nat, "cross_attention", counted)
    return calls


def _wan_i2v_attn(heads, hd):
    from standins import Attention, RMSNorm

    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanP

    dim = heads * hd
    attn = Attention(dim, heads, qk_norm="rms", across_heads=True, dtype=DT)
    attn.add_k_proj, attn.add_v_proj, attn.norm_added_k = torch.nn.Linear(dim, dim), torch.nn.Linear(dim, dim), RMSNorm(dim)
    attn.to(DT).cuda()
    attn.set_processor(WanP(0))
    return attn


def _inputs(heads, hd, S, n_txt, batch=1):
    hidden = (torch.randn(batch, S, heads * hd) * 0.3).to(DT).cuda()
    enc = (torch.randn(batch, 257 + n_txt, heads * hd) * 0.3).to(DT).cuda()
    return hidden, enc


@pytest.mark.parametrize("batch", [1, 2])
def test_wan_i2v_switch_on_is_one_pair_launch_and_the_same_bits(kernel_calls, monkeypatch, batch):
    torch.manual_seed(2)
    heads, hd, S, n_txt = 2, 128, 800, 40
    attn = _wan_i2v_attn(heads, hd)
    assert attn.processor.i2v_pair_launch is False
    hidden, enc = _inputs(heads, hd, S, n_txt, batch)
    with torch.no_grad():
        off = attn(hidden, encoder_hidden_states=enc)
        assert kernel_calls == [("single", (batch, heads, S, hd))] * 2
        del kernel_calls[:]
        monkeypatch.setattr(attn.processor, "i2v_pair_launch", True)
        on = attn(hidden, encoder_hidden_states=enc)
    assert kernel_calls == [("pair", (batch, heads, S, hd))]
    assert torch.isfinite(off.float()).all() and torch.equal(on, off)


def test_wan_i2v_switch_on_head_dim_64_falls_back(kernel_calls, monkeypatch):
    torch.manual_seed(3)
    heads, hd, S = 4, 64, 800
    attn = _wan_i2v_attn(heads, hd)
    hidden, enc = _inputs(heads, hd, S, 40)
    with torch.no_grad():
        off = attn(hidden, encoder_hidden_states=enc)
        monkeypatch.setattr(attn.processor, "i2v_pair_launch", True)
        on = attn(hidden, encoder_hidden_states=enc)
    assert kernel_calls == [] and torch.equal(on, off)


def test_wan_i2v_switch_on_with_a_mask_falls_back(kernel_calls, monkeypatch):
    torch.manual_seed(4)
    heads, hd, S, n_txt = 2, 128, 800, 40
    attn = _wan_i2v_attn(heads, hd)
    hidden, enc = _inputs(heads, hd, S, n_txt)
    mask = torch.ones(1, 1, 1, n_txt, dtype=torch.bool, device="cuda")
    mask[..., 25:] = False
    with torch.no_grad():
        off = attn(hidden, encoder_hidden_states=enc, attention_mask=mask)
        assert kernel_calls == [("single", (1, heads, S, hd))]         # the image branch has no mask; the text branch is SDPA
        del kernel_calls[:]
        monkeypatch.setattr(attn.processor, "i2v_pair_launch", True)
        on = attn(hidden, encoder_hidden_states=enc, attention_mask=mask)
    assert kernel_calls == [("single", (1, heads, S, hd))] and torch.equal(on, off)


def test_core_pair_equals_the_two_core_calls(nat):
    """_core.cross_attention_pair on the processors' head views, kernel route, against the calls it replaces"""
    from svg.models import _core

    g = torch.Generator().manual_seed(9)
    B, H, Sq = 2, 3, 500
    q, = _proj_views(B, H, Sq, DT, g)
    k, v = _proj_views(B, H, 512, DT, g) + _proj_views(B, H, 512, DT, g)
    k_img, v_img = _proj_views(B, H, 257, DT, g) + _proj_views(B, H, 257, DT, g)
    o = _core.cross_attention_pair(q, k, v, k_img, v_img)
    assert o.shape == (B, H, Sq, D) and torch.equal(o, _core.cross_attention(q, k, v) + _core.cross_attention(q, k_img, v_img))
