"""svg_cross_attention without a GPU: the export, the argument validation (every check runs on the host before any launch — rows
that pass placeholder pointers are skipped where a GPU is visible, as in test_entry_validation_cpu.py) and the routing of
_core.cross_attention for tensors the kernel does not take (CPU tensors: the reference's scaled_dot_product_attention call, bit for bit)."""
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


def k_row(row):
    lay = layout()
    lay.k.row = row
    return lay


def cross(q=PH, k=PH, v=PH, o=PH, BH=2, Sq=256, Skv=64, D=128, dtype=0, lay=None):
    return [q, k, v, o, BH, Sq, Skv, D, dtype, 1.0, C.byref(lay) if lay is not None else None, None]


CASES = [
    ("null_q", cross(q=None), BAD_ARG),
    ("null_k", cross(k=None), BAD_ARG),
    ("null_v", cross(v=None), BAD_ARG),
    ("null_o", cross(o=None), BAD_ARG),
    ("BH0", cross(BH=0), BAD_ARG),
    ("Sq0", cross(Sq=0), BAD_ARG),
    ("Skv0", cross(Skv=0), BAD_ARG),
    ("Skv_neg", cross(Skv=-5), BAD_ARG),
    ("D64", cross(D=64), UNSUPPORTED),
    ("D96", cross(D=96), UNSUPPORTED),
    ("dtype_f32", cross(dtype=2), UNSUPPORTED),
    ("dtype_f32_layout", cross(dtype=2, lay=layout()), UNSUPPORTED),
    ("Sq_rows", cross(Sq=S_ROWS), UNSUPPORTED),
    ("Skv_rows", cross(Skv=S_ROWS), UNSUPPORTED),
    ("kv_span_2e32", cross(Skv=1024, lay=k_row(1 << 22)), UNSUPPORTED),
    ("layout_heads0", cross(lay=layout(heads_per_batch=0)), BAD_ARG),
    ("layout_heads_not_dividing", cross(BH=3, lay=layout(H=2)), BAD_ARG),
    ("layout_row_lt_D", cross(lay=layout(row=64)), BAD_ARG),
    ("layout_row_unaligned", cross(lay=layout(row=132)), UNSUPPORTED),
    ("layout_row_2e23", cross(lay=k_row(1 << 23)), UNSUPPORTED),
]


def test_library_exports_cross_attention():
    lib = nat.load()
    assert "svg_cross_attention" in nat.SIGNATURES
    assert lib.svg_cross_attention.argtypes == nat.SIGNATURES["svg_cross_attention"][1]
    assert int(lib.svg_abi_version()) == 4


@pytest.mark.parametrize("args,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_cross_attention_rejects(args, expected):
    if any(a == PH for a in args) and torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert nat.load().svg_cross_attention(*args) == expected


def test_cross_attention_supported_is_false_off_the_kernels_ground():
    q, k = torch.zeros(1, 2, 8, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 4, 128, dtype=torch.bfloat16)
    assert not nat.cross_attention_supported(q, k)                     # CPU tensors
    with pytest.raises(RuntimeError):
        nat.cross_attention(q, k, k)                                   # ... and no CPU fallback inside the binding


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("D", [64, 128])
def test_core_cross_attention_on_cpu_is_sdpa(D, masked, dtype):
    from svg.models import _core

    g = torch.Generator().manual_seed(D + masked)
    B, H, Sq, Skv = 2, 3, 33, 17
    q = torch.randn(B, Sq, H * D, generator=g).to(dtype).unflatten(2, (H, D)).transpose(1, 2)    # the processors' head views
    k, v = (torch.randn(B, Skv, H * D, generator=g).to(dtype).unflatten(2, (H, D)).transpose(1, 2) for _ in range(2))
    mask = None
    if masked:
        mask = torch.rand(B, 1, Sq, Skv, generator=g) > 0.3
        mask[..., 0] = True
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, is_causal=False)
    out = _core.cross_attention(q, k, v, mask)
    assert out.dtype == ref.dtype and out.shape == ref.shape and torch.equal(out, ref)
