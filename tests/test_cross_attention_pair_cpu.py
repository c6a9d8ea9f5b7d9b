"""svg_cross_attention_pair without a GPU: the export, the argument validation (every check runs on the host before any launch — rows
that pass placeholder pointers are skipped where a GPU is visible, as in test_cross_attention_cpu.py), the routing of
_core.cross_attention_pair for tensors the kernel does not take (CPU tensors: the two scaled_dot_product_attention calls and the add, bit
for bit), and the Wan processors' switch (`i2v_pair_launch`, off by default)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from svg import _native as nat

BAD_ARG, UNSUPPORTED = -1, -2
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
S_ROWS = 1 << 24      # the row bound: the LDS-DMA row offset is __umul24(row, row stride in bytes)


def layout(H=2, Sq=256, Skv=64, row=128, **kw):
    q = nat.TensorStrides(H * Sq * row, Sq * row, row)
    k = nat.TensorStrides(H * Skv * row, Skv * row, row)
    lay = nat.AttnLayout(H, 0, q, k, k, q)
    for name, val in kw.items():
        setattr(lay, name, val)
    return lay


def k_row(row, **kw):
    lay = layout(**kw)
    lay.k.row = row
    return lay


def v_row(row, **kw):
    lay = layout(**kw)
    lay.v.row = row
    return lay


def pair(q=PH, k_a=PH, v_a=PH, k_b=PH, v_b=PH, o=PH, BH=2, Sq=256, Skv_a=64, Skv_b=257, D=128, dtype=0, lay=None, lay_b=None):
    ref = lambda x: C.byref(x) if x is not None else None   # noqa: E731
    return [q, k_a, v_a, k_b, v_b, o, BH, Sq, Skv_a, Skv_b, D, dtype, 1.0, ref(lay), ref(lay_b), None]


CASES = [
    ("null_q", pair(q=None), BAD_ARG),
    ("null_k_a", pair(k_a=None), BAD_ARG),
    ("null_v_a", pair(v_a=None), BAD_ARG),
    ("null_k_b", pair(k_b=None), BAD_ARG),
    ("null_v_b", pair(v_b=None), BAD_ARG),
    ("null_o", pair(o=None), BAD_ARG),
    ("BH0", pair(BH=0), BAD_ARG),
    ("Sq0", pair(Sq=0), BAD_ARG),
    ("Skv_a0", pair(Skv_a=0), BAD_ARG),
    ("Skv_b0", pair(Skv_b=0), BAD_ARG),
    ("Skv_b_neg", pair(Skv_b=-5), BAD_ARG),
    ("D64", pair(D=64), UNSUPPORTED),
    ("D96", pair(D=96), UNSUPPORTED),
    ("dtype_f32", pair(dtype=2), UNSUPPORTED),
    ("dtype_f32_layouts", pair(dtype=2, lay=layout(), lay_b=layout(Skv=257)), UNSUPPORTED),
    ("Sq_rows", pair(Sq=S_ROWS), UNSUPPORTED),
    ("Skv_a_rows", pair(Skv_a=S_ROWS), UNSUPPORTED),
    ("Skv_b_rows", pair(Skv_b=S_ROWS), UNSUPPORTED),
    ("a_kv_span_2e32", pair(Skv_a=1024, lay=k_row(1 << 22)), UNSUPPORTED),
    ("b_kv_span_2e32", pair(Skv_b=1024, lay_b=v_row(1 << 22)), UNSUPPORTED),
    ("layout_heads0", pair(lay=layout(heads_per_batch=0)), BAD_ARG),
    ("layout_heads_not_dividing", pair(BH=3, lay=layout(H=2)), BAD_ARG),
    ("layout_row_lt_D", pair(lay=layout(row=64)), BAD_ARG),
    ("layout_row_unaligned", pair(lay=layout(row=132)), UNSUPPORTED),
    ("layout_row_2e23", pair(lay=k_row(1 << 23)), UNSUPPORTED),
    ("layout_b_k_row_lt_D", pair(lay_b=k_row(64)), BAD_ARG),
    ("layout_b_v_row_unaligned", pair(lay_b=v_row(132)), UNSUPPORTED),
    ("layout_b_k_row_2e23", pair(lay=layout(), lay_b=k_row(1 << 23)), UNSUPPORTED),
    ("unaligned_k_b", pair(k_b=PH + 2, lay_b=layout(Skv=257)), UNSUPPORTED),
]


def test_library_exports_cross_attention_pair():
    lib = nat.load()
    assert "svg_cross_attention_pair" in nat.SIGNATURES
    assert lib.svg_cross_attention_pair.argtypes == nat.SIGNATURES["svg_cross_attention_pair"][1]
    assert len(nat.SIGNATURES["svg_cross_attention_pair"][1]) == 16
    assert int(lib.svg_abi_version()) == 4


@pytest.mark.parametrize("args,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_cross_attention_pair_rejects(args, expected):
    if any(a in (PH, PH + 2) for a in args[:6]) and torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert nat.load().svg_cross_attention_pair(*args) == expected


def test_layout_b_contributes_only_its_key_and_value_strides():
    """what else layout_b holds (heads, q / o strides) is not read: nonsense there is not an error — the call gets as far as the next check"""
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    lay_b = layout(Skv=257, heads_per_batch=0)
    lay_b.q.row = lay_b.o.row = 3
    assert nat.load().svg_cross_attention_pair(*pair(dtype=2, lay=layout(), lay_b=lay_b)) == UNSUPPORTED   # (the dtype, checked last)
    lay_b.k.row = 3
    assert nat.load().svg_cross_attention_pair(*pair(dtype=2, lay=layout(), lay_b=lay_b)) == BAD_ARG


def test_native_cross_attention_pair_refuses_cpu_tensors():
    q, k, kb = (torch.zeros(1, 2, n, 128, dtype=torch.bfloat16) for n in (8, 4, 5))
    with pytest.raises(RuntimeError):
        nat.cross_attention_pair(q, k, k, kb, kb)                      # no CPU fallback inside the binding


def _head_views(B, H, S, D, dtype, g):
    return torch.randn(B, S, H * D, generator=g).to(dtype).unflatten(2, (H, D)).transpose(1, 2)    # the processors' head views


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_core_cross_attention_pair_on_cpu_is_two_sdpa_calls_and_the_add(D, masked, dtype, monkeypatch):
    from svg.models import _core

    def no_kernel(*a, **kw):
        raise AssertionError("CPU tensors must not reach the binding")

    monkeypatch.setattr(nat, "cross_attention_pair", no_kernel)
    monkeypatch.setattr(nat, "cross_attention", no_kernel)
    g = torch.Generator().manual_seed(D + masked)
    B, H, Sq, Skv, Simg = 2, 3, 33, 17, 21
    q = _head_views(B, H, Sq, D, dtype, g)
    k, v = (_head_views(B, H, Skv, D, dtype, g) for _ in range(2))
    k_img, v_img = (_head_views(B, H, Simg, D, dtype, g) for _ in range(2))
    mask = None
    if masked:
        mask = torch.rand(B, 1, Sq, Skv, generator=g) > 0.3
        mask[..., 0] = True
    ref = (F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, is_causal=False)
           + F.scaled_dot_product_attention(q, k_img, v_img, attn_mask=None, dropout_p=0.0, is_causal=False))
    out = _core.cross_attention_pair(q, k, v, k_img, v_img, mask)
    assert out.dtype == ref.dtype and out.shape == (B, H, Sq, D) and torch.equal(out, ref)


def _wan_i2v_attn(heads, hd, dtype):
    from standins import Attention, RMSNorm

    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanP

    dim = heads * hd
    attn = Attention(dim, heads, qk_norm="rms", across_heads=True, dtype=dtype)
    attn.add_k_proj, attn.add_v_proj, attn.norm_added_k = torch.nn.Linear(dim, dim), torch.nn.Linear(dim, dim), RMSNorm(dim)
    attn.to(dtype)
    attn.set_processor(WanP(0))
    return attn


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hd", [64, 128])
def test_wan_processor_switch_on_equals_switch_off_on_cpu(hd, dtype, monkeypatch):
    torch.manual_seed(hd)
    heads, S, n_txt = 2, 100, 40
    attn = _wan_i2v_attn(heads, hd, dtype)
    hidden = (torch.randn(2, S, heads * hd) * 0.3).to(dtype)
    enc = (torch.randn(2, 257 + n_txt, heads * hd) * 0.3).to(dtype)
    from svg.models import _core

    calls = []
    real = _core.cross_attention_pair
    monkeypatch.setattr(_core, "cross_attention_pair", lambda *a, **kw: (calls.append(a[0].shape), real(*a, **kw))[1])
    with torch.no_grad():
        off = attn(hidden, encoder_hidden_states=enc)
        assert calls == []
        monkeypatch.setattr(attn.processor, "i2v_pair_launch", True)
        on = attn(hidden, encoder_hidden_states=enc)
        assert calls == [(2, heads, S, hd)]
        self_attn = attn(hidden)                                     # not a cross call: the switch changes nothing
    assert off.shape == hidden.shape and torch.isfinite(off.float()).all() and torch.equal(on, off)
    assert calls == [(2, heads, S, hd)] and self_attn.shape == hidden.shape


def test_wan_processors_have_the_switch_off_by_default():
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor, WanAttn_SVGAttn_Processor2_0

    for cls in (WanAttn_SVGAttn_Processor2_0, WanAttn_SAPAttn_Processor):
        assert cls.i2v_pair_launch is False and cls(0).i2v_pair_launch is False
