"""svg_cross_attention_keyrange on the GPU: cross attention over one key window per video (csrc/attention_cross.hip, the windowed form of
cross_policy.h) against the CPU oracle with the equivalent bool [B, 1, 1, Skv] mask, bit-exact against the call on the sliced keys, the
bounds of what the kernel reads and writes, the clamping of the device-side window values, layouts, the resident loop with items of
different cost, and the Cosmos processor's routing of its text key-padding mask.

ref: F.scaled_dot_product_attention with the bool mask the Cosmos transformer builds from the pipeline's text mask
(svg/models/cosmos/custom_models.py:85-86, svg/models/cosmos/attention.py:104-110)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import svg_oracle as O
from test_gpu_kernels import check_attn, dev, rel_l2
from poisoned import poisoned_like

pytestmark = pytest.mark.gpu
DT = torch.bfloat16
D = 128


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _qkv(B, H, Sq, Skv, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Sq, D, generator=g).to(dtype)
    k, v = (torch.randn(B, H, Skv, D, generator=g).to(dtype) for _ in range(2))
    return q, k, v


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device="cuda")


def _cut(windows, Skv):
    return [(min(b, Skv), min(e, Skv)) for b, e in windows]


def _mask(windows, Skv):
    """the bool [B, 1, 1, Skv] key-padding mask of one window per video"""
    m = torch.zeros(len(windows), 1, 1, Skv, dtype=torch.bool)
    for b, (lo, hi) in enumerate(windows):
        m[b, 0, 0, lo:hi] = True
    return m


def _run(nat, q, k, v, windows, **kw):
    return nat.cross_attention_keyrange(q, k, v, _i32(e for _, e in windows), _i32(b for b, _ in windows), **kw)


def _padded(k, v, windows, pad=91):
    """k, v as [B, H, Skv] views of [B, H, Skv + pad] allocations, NaN behind Skv and outside each video's window"""
    B, H, Skv, _ = k.shape
    kb, vb = (torch.full((B, H, Skv + pad, D), float("nan"), dtype=k.dtype) for _ in range(2))
    for b, (lo, hi) in enumerate(windows):
        kb[b, :, lo:hi], vb[b, :, lo:hi] = k[b, :, lo:hi], v[b, :, lo:hi]
    kb, vb = kb.cuda(), vb.cuda()
    return kb, vb, kb[:, :, :Skv], vb[:, :, :Skv]


# ---------------------------------------------------------------------------------------------------------
# parity against the oracle
# ---------------------------------------------------------------------------------------------------------
# whole set (cut to Skv), ending on a tile edge, ragged end | one tile not the first, one key, unaligned on both sides |
# ragged last tiles, the last key alone in its tile, empty
WINDOW_GROUPS = [[(0, 1 << 20), (0, 64), (0, 100)], [(64, 128), (65, 66), (70, 200)], [(192, 257), (256, 257), (40, 40)]]


@pytest.mark.parametrize("group", range(3))
@pytest.mark.parametrize("Sq", [1, 300, 513])
@pytest.mark.parametrize("Skv", [37, 130, 257])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_keyrange_matches_oracle(nat, dtype, Skv, Sq, group):
    B, H = 3, 2
    windows = _cut(WINDOW_GROUPS[group], Skv)
    q, k, v = _qkv(B, H, Sq, Skv, dtype, seed=Sq * 1009 + Skv * 7 + group)
    o = _run(nat, dev(q), dev(k), dev(v), windows)
    assert o.shape == q.shape and o.dtype == dtype and o.is_contiguous()
    ref = O.masked_attention(q, k, v, _mask(windows, Skv))
    print(f"windows {windows} rel_l2 {rel_l2(o.cpu(), ref):.3e}")
    assert torch.isfinite(o.float()).all()
    for b, (lo, hi) in enumerate(windows):
        if hi <= lo:                                                   # an empty window: zeros, exactly
            assert (o[b] == 0).all()
    check_attn(o, ref, dtype)


@pytest.mark.parametrize("n", [1, 3, 6])
def test_keyrange_takes_bh_s_d_windows_per_group_of_heads_and_a_scale(nat, n):
    BH, Sq, Skv = 6, 300, 130
    q, k, v = _qkv(1, BH, Sq, Skv, DT, seed=n)
    windows = [(0, 77), (64, 130), (3, 4), (0, 130), (100, 129), (65, 128)][:n]
    o = _run(nat, dev(q[0]), dev(k[0]), dev(v[0]), windows, sm_scale=0.05)
    assert o.shape == (BH, Sq, D)
    per_head = [windows[h // (BH // n)] for h in range(BH)]            # heads [i * BH / n, (i + 1) * BH / n) share window i
    check_attn(o, O.masked_attention(q[0], k[0], v[0], _mask(per_head, Skv)[:, 0], scale=0.05), DT)
    end_only = nat.cross_attention_keyrange(dev(q[0]), dev(k[0]), dev(v[0]), _i32(e for _, e in windows), sm_scale=0.05)   # kv_begin None: from key 0
    check_attn(end_only, O.masked_attention(q[0], k[0], v[0], _mask([(0, e) for _, e in per_head], Skv)[:, 0], scale=0.05), DT)


# ---------------------------------------------------------------------------------------------------------
# the same bits as svg_cross_attention on the sliced keys
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("windows", [
    [(0, 1), (0, 37), (0, 64)], [(0, 100), (0, 257), (0, 129)],                                  # begin == 0
    [(64, 128), (64, 100), (128, 257)], [(192, 257), (256, 257), (128, 129)],                    # begin a positive multiple of 64: the tiles coincide
], ids=["from0_a", "from0_b", "aligned_a", "aligned_b"])
def test_keyrange_equals_the_call_on_the_sliced_keys(nat, windows, dtype):
    B, H, Sq, Skv = 3, 2, 300, 257
    q, k, v = (dev(x) for x in _qkv(B, H, Sq, Skv, dtype, seed=windows[0][1]))
    o = _run(nat, q, k, v, windows)
    for b, (lo, hi) in enumerate(windows):
        sliced = nat.cross_attention(q[b:b + 1], k[b:b + 1, :, lo:hi], v[b:b + 1, :, lo:hi])
        assert torch.equal(o[b:b + 1], sliced), (b, lo, hi)


# ---------------------------------------------------------------------------------------------------------
# what the kernel reads and writes
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Skv,windows", [(37, [(0, 37), (5, 20), (36, 37)]), (257, [(0, 100), (70, 200), (192, 257)]),
                                         (257, [(64, 128), (65, 66), (256, 257)])])
def test_nothing_outside_the_window_is_read(nat, Skv, windows):
    B, H, Sq = 3, 2, 700
    q, k, v = _qkv(B, H, Sq, Skv, DT, seed=Skv + windows[0][1])
    kb, vb, kv_, vv = _padded(k, v, windows)
    assert not kv_.is_contiguous() and torch.isnan(kb[:, :, Skv:]).all() and torch.isnan(kb[1, :, :windows[1][0]]).all()
    o = _run(nat, dev(q), kv_, vv, windows)
    clean = _run(nat, dev(q), dev(k), dev(v), windows)
    assert torch.isfinite(o.float()).all() and torch.equal(o, clean)
    check_attn(o, O.masked_attention(q, k, v, _mask(windows, Skv)), DT)


@pytest.mark.parametrize("Skv", [37, 257])
def test_window_values_are_clamped(nat, Skv):
    B, H, Sq = 4, 2, 300
    q, k, v = _qkv(B, H, Sq, Skv, DT, seed=Skv)
    raw = [(-5, Skv + 1000), (20, 7), (Skv + 7, Skv + 90), (-9, -1)]   # whole set | begin > end | both behind Skv | both negative
    kb, vb, kv_, vv = _padded(k, v, [(0, Skv), (0, 0), (0, 0), (0, 0)])   # (memory the test owns behind Skv, NaN wherever nothing may be read)
    o = _run(nat, dev(q), kv_, vv, raw)
    torch.cuda.synchronize()
    whole = nat.cross_attention(dev(q[:1]), kv_[:1], vv[:1])
    assert torch.equal(o[:1], whole)
    assert (o[1:] == 0).all()
    check_attn(o[:1], O.masked_attention(q[:1], k[:1], v[:1], None), DT)


@pytest.mark.parametrize("Sq", [300, 512, 1])
def test_every_row_is_written_zeros_included_and_nothing_else(nat, Sq):
    B, H, Skv, pad, sentinel = 3, 2, 130, 300, -77.0
    windows = [(0, 100), (70, 70), (64, 130)]                          # video 1: an empty window
    q, k, v = _qkv(B, H, Sq, Skv, DT, seed=Sq)
    big = torch.full((B, H, Sq + pad, D), sentinel, dtype=DT, device="cuda")
    out = big[:, :, :Sq]
    r = _run(nat, dev(q), dev(k), dev(v), windows, out=out)
    torch.cuda.synchronize()
    assert r is out
    assert (big[:, :, Sq:] == sentinel).all()
    assert not (out == sentinel).any() and torch.isfinite(out.float()).all()
    assert (out[1] == 0).all()
    check_attn(out, O.masked_attention(q, k, v, _mask(windows, Skv)), DT)


# ---------------------------------------------------------------------------------------------------------
# layouts: bit-exact against the contiguous call
# ---------------------------------------------------------------------------------------------------------
def _is_token_major(o):
    return o.transpose(1, 2).is_contiguous()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("Sq,Skv", [(700, 512), (257, 257), (1300, 77)])
def test_keyrange_strided_equals_contiguous(nat, Sq, Skv, dtype):
    B, H = 3, 2
    windows = _cut([(0, 100), (70, 200), (40, 1 << 20)], Skv)
    g = torch.Generator().manual_seed(Sq + Skv)
    q = dev(torch.randn(B, Sq, H * D, generator=g).to(dtype)).unflatten(2, (H, D)).transpose(1, 2)      # projection views [B, S, H * D]
    k, v = (dev(torch.randn(B, Skv, H * D, generator=g).to(dtype)).unflatten(2, (H, D)).transpose(1, 2) for _ in range(2))
    assert not q.is_contiguous() and not k.is_contiguous()
    ref = _run(nat, q.contiguous(), k.contiguous(), v.contiguous(), windows)
    check_attn(ref, O.masked_attention(q.cpu(), k.cpu(), v.cpu(), _mask(windows, Skv)), dtype)
    o = _run(nat, q, k, v, windows, token_major_out=True)              # everything strided, o token-major
    assert o.shape == ref.shape and _is_token_major(o) and torch.equal(o, ref)
    flat = o.transpose(1, 2).flatten(2, 3)                             # the processors' next line: a view
    assert flat.data_ptr() == o.data_ptr() and flat.shape == (B, Sq, H * D)
    o2 = _run(nat, q, k, v, windows)                                   # strided in, head-major out
    assert o2.is_contiguous() and torch.equal(o2, ref)
    kv = dev(torch.randn(B, Skv, 2 * H * D, generator=g).to(dtype))    # k and v as slices of one fused [B, Skv, 2 * H * D] projection
    k2, v2 = (kv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(2))
    ref2 = _run(nat, q.contiguous(), k2.contiguous(), v2.contiguous(), windows)
    o3 = _run(nat, q, k2, v2, windows, token_major_out=True)
    assert _is_token_major(o3) and torch.equal(o3, ref2)
    out = poisoned_like(ref)                                          # a caller's buffer
    assert _run(nat, q, k, v, windows, out=out) is out and torch.equal(out, ref)


def test_keyrange_copies_views_the_layout_cannot_describe(nat):
    windows = [(3, 50)]
    q, k, v = _qkv(1, 2, 300, 64, DT, seed=5)
    qd = dev(torch.cat([q, q], dim=-1))[..., 1:129]                    # 2-byte aligned rows: not a layout the entry takes
    assert qd.data_ptr() % 16 != 0
    ref = _run(nat, qd.contiguous(), dev(k), dev(v), windows)
    assert torch.equal(_run(nat, qd, dev(k), dev(v), windows), ref)


# ---------------------------------------------------------------------------------------------------------
# resident loop: more work items than compute units, items of two different costs
# ---------------------------------------------------------------------------------------------------------
def test_keyrange_resident_loop(nat):
    B, H, Sq, Skv = 2, 8, 12800, 512                                   # 800 work items: 2 key tiles each in video 0, 4 in video 1
    windows = [(0, 100), (300, 512)]
    q, k, v = _qkv(B, H, Sq, Skv, DT, seed=11)
    dq, dk, dv = dev(q), dev(k), dev(v)
    o = _run(nat, dq, dk, dv, windows)
    o_again = _run(nat, dq, dk, dv, windows)
    torch.cuda.synchronize()
    assert torch.equal(o, o_again)
    oc, mask = o.cpu(), _mask(windows, Skv)
    for h in range(H):
        check_attn(oc[:, h], O.masked_attention(q[:, h], k[:, h], v[:, h], mask[:, 0]), DT)


# ---------------------------------------------------------------------------------------------------------
# Cosmos processor
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def kernel_calls(nat, monkeypatch):
    """counts the calls of _native.cross_attention_keyrange and of _native.cross_attention"""
    calls = {"keyrange": [], "plain": []}
    real_kr, real = nat.cross_attention_keyrange, nat.cross_attention

    def counted_kr(*a, **kw):
        calls["keyrange"].append(a[0].shape)
        return real_kr(*a, **kw)

    def counted(*a, **kw):
        calls["plain"].append(a[0].shape)
        return real(*a, **kw)

    monkeypatch.setattr(nat, "cross_attention_keyrange", counted_kr)
    monkeypatch.setattr(nat, "cross_attention", counted)
    return calls


def _cosmos(heads, hd, B, S, n_txt, seed):
    from standins import Attention

    from svg.models.cosmos.attention import Cosmos_SVG_AttnProcessor2_0 as CosP

    torch.manual_seed(seed)
    dim = heads * hd
    attn = Attention(dim, heads, qk_norm="rms", dtype=DT).cuda()      # per-head RMSNorm(hd)
    attn.set_processor(CosP(0))
    hidden = (torch.randn(B, S, dim) * 0.3).to(DT).cuda()
    enc = (torch.randn(B, n_txt, dim) * 0.3).to(DT).cuda()
    return attn, hidden, enc


def test_cosmos_key_padding_mask_runs_the_keyrange_kernel(kernel_calls):
    heads, hd, B, S, n_txt = 2, 128, 2, 800, 77
    attn, hidden, enc = _cosmos(heads, hd, B, S, n_txt, seed=5)
    mask = _mask([(0, 25), (0, 60)], n_txt).cuda()
    with torch.no_grad():
        out = attn(hidden, encoder_hidden_states=enc, attention_mask=mask, timestep=None)
        a = attn.cpu().float()
        x, e = hidden.float().cpu(), enc.float().cpu()
        split = lambda t: t.unflatten(2, (heads, -1)).transpose(1, 2)   # noqa: E731
        q, k, v = a.norm_q(split(a.to_q(x))), a.norm_k(split(a.to_k(e))), split(a.to_v(e))
        ref = a.to_out[0](F.scaled_dot_product_attention(q, k, v, attn_mask=mask.cpu()).transpose(1, 2).flatten(2, 3))
    assert kernel_calls == {"keyrange": [(B, heads, S, hd)], "plain": []}
    torch.testing.assert_close(out.float().cpu(), ref, atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("kind", ["hole", "one_video_all_false"])
def test_cosmos_masks_that_are_no_windows_stay_on_sdpa(kernel_calls, monkeypatch, kind):
    from svg.models import _core

    heads, hd, B, S, n_txt = 2, 128, 2, 800, 77
    attn, hidden, enc = _cosmos(heads, hd, B, S, n_txt, seed=6)
    mask = _mask([(0, 25), (0, 60)], n_txt).cuda()
    if kind == "hole":
        mask[1, 0, 0, 30] = False
    else:
        mask[1] = False
    with torch.no_grad():
        out = attn(hidden, encoder_hidden_states=enc, attention_mask=mask, timestep=None)
        assert kernel_calls == {"keyrange": [], "plain": []}
        monkeypatch.setattr(_core, "cross_attention_key_masked", lambda q, k, v, attention_mask: F.scaled_dot_product_attention(
            q, k, v, attn_mask=attention_mask, dropout_p=0.0, is_causal=False))
        plain = attn(hidden, encoder_hidden_states=enc, attention_mask=mask, timestep=None)
    # (the same bits, NaN included: SDPA's rows of a video without a key are the reference's behaviour, and stay)
    assert out.shape == plain.shape and torch.equal(out.view(torch.int16), plain.view(torch.int16))
    assert torch.isfinite(out[0].float()).all()
