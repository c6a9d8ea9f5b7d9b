"""svg_cross_attention_keyrange without a GPU: the export, the argument validation (every check runs on the host before any launch — rows
that pass placeholder pointers are skipped where a GPU is visible, as in test_cross_attention_cpu.py), _core.key_windows (which masks are
key windows, and its one read-back per mask object) and the routing of _core.cross_attention_key_masked for CPU tensors (the reference's
scaled_dot_product_attention call, bit for bit).

ref: the bool [B, 1, 1, S_text] mask of the Cosmos transformer (svg/models/cosmos/custom_models.py:85-86, cosmos/attention.py:104-110)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from svg import _native as nat
from svg.models import _core

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


def keyrange(q=PH, k=PH, v=PH, o=PH, BH=2, Sq=256, Skv=64, D=128, dtype=0, begin=PH, end=PH, hpw=1, lay=None):
    return [q, k, v, o, BH, Sq, Skv, D, dtype, 1.0, begin, end, hpw, C.byref(lay) if lay is not None else None, None]


CASES = [
    ("null_q", keyrange(q=None), BAD_ARG),
    ("null_k", keyrange(k=None), BAD_ARG),
    ("null_v", keyrange(v=None), BAD_ARG),
    ("null_o", keyrange(o=None), BAD_ARG),
    ("BH0", keyrange(BH=0), BAD_ARG),
    ("Sq0", keyrange(Sq=0), BAD_ARG),
    ("Skv0", keyrange(Skv=0), BAD_ARG),
    ("Skv_neg", keyrange(Skv=-5), BAD_ARG),
    ("D64", keyrange(D=64), UNSUPPORTED),
    ("D96", keyrange(D=96), UNSUPPORTED),
    ("dtype_f32", keyrange(dtype=2), UNSUPPORTED),
    ("dtype_f32_layout", keyrange(dtype=2, lay=layout()), UNSUPPORTED),
    ("Sq_rows", keyrange(Sq=S_ROWS), UNSUPPORTED),
    ("Skv_rows", keyrange(Skv=S_ROWS), UNSUPPORTED),
    ("kv_span_2e32", keyrange(Skv=1024, lay=k_row(1 << 22)), UNSUPPORTED),
    ("layout_heads0", keyrange(lay=layout(heads_per_batch=0)), BAD_ARG),
    ("layout_heads_not_dividing", keyrange(BH=3, lay=layout(H=2)), BAD_ARG),
    ("layout_row_lt_D", keyrange(lay=layout(row=64)), BAD_ARG),
    ("layout_row_unaligned", keyrange(lay=layout(row=132)), UNSUPPORTED),
    ("layout_row_2e23", keyrange(lay=k_row(1 << 23)), UNSUPPORTED),
    ("null_kv_end", keyrange(end=None), BAD_ARG),
    ("null_kv_end_null_begin", keyrange(begin=None, end=None), BAD_ARG),
    ("heads_per_window0", keyrange(hpw=0), BAD_ARG),
    ("heads_per_window_neg", keyrange(hpw=-2), BAD_ARG),
    ("heads_per_window_not_dividing", keyrange(BH=6, hpw=4), BAD_ARG),
    ("heads_per_window_above_BH", keyrange(BH=2, hpw=4), BAD_ARG),
]


def test_library_exports_cross_attention_keyrange():
    lib = nat.load()
    assert "svg_cross_attention_keyrange" in nat.SIGNATURES
    assert lib.svg_cross_attention_keyrange.argtypes == nat.SIGNATURES["svg_cross_attention_keyrange"][1]
    assert len(nat.SIGNATURES["svg_cross_attention_keyrange"][1]) == 15
    assert int(lib.svg_abi_version()) == 4


@pytest.mark.parametrize("args,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_cross_attention_keyrange_rejects(args, expected):
    if any(a == PH for a in args) and torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert nat.load().svg_cross_attention_keyrange(*args) == expected


def test_binding_has_no_cpu_fallback():
    q, k = torch.zeros(1, 2, 8, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        nat.cross_attention_keyrange(q, k, k, torch.tensor([4], dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------
# key_windows
# ---------------------------------------------------------------------------------------------------------
def runs(S, *spans):
    """bool [len(spans), 1, 1, S]: video b keeps the keys of spans[b] = (begin, end), or of each span of a list of them"""
    m = torch.zeros(len(spans), 1, 1, S, dtype=torch.bool)
    for b, sp in enumerate(spans):
        for lo, hi in (sp if isinstance(sp, list) else [sp]):
            m[b, 0, 0, lo:hi] = True
    return m


def windows_of(mask, batch, S):
    w = _core.key_windows(mask, batch, S)
    if w is None:
        return None
    begin, end = w
    assert begin.dtype == end.dtype == torch.int32 and begin.shape == end.shape == (batch,) and begin.device == mask.device
    return list(zip(begin.tolist(), end.tolist()))


KW_CASES = [
    ("right_padding", runs(77, (0, 25), (0, 60)), 2, [(0, 25), (0, 60)]),
    ("left_padding", runs(77, (52, 77), (17, 77)), 2, [(52, 77), (17, 77)]),
    ("middle", runs(512, (100, 230)), 1, [(100, 230)]),
    ("full", runs(64, (0, 64), (0, 64)), 2, [(0, 64), (0, 64)]),
    ("one_key", runs(130, (65, 66), (129, 130)), 2, [(65, 66), (129, 130)]),
    ("broadcast", runs(77, (0, 25)), 3, [(0, 25)] * 3),
    ("three_runs", runs(300, (0, 100), (64, 128), (299, 300)), 3, [(0, 100), (64, 128), (299, 300)]),
    ("hole", runs(77, (0, 25), [(0, 10), (11, 60)]), 2, None),
    ("hole_of_one_in_a_broadcast_mask", runs(77, [(0, 1), (2, 3)]), 2, None),
    ("one_video_all_false", runs(77, (0, 25), (0, 0), (0, 9)), 3, None),
    ("all_false", runs(77, (0, 0)), 1, None),
    ("float_mask", runs(77, (0, 25), (0, 60)).float(), 2, None),
    ("additive_float_mask", torch.zeros(2, 1, 1, 77).masked_fill(~runs(77, (0, 25), (0, 60)), float("-inf")), 2, None),
    ("int64_mask", runs(77, (0, 25), (0, 60)).to(torch.int64), 2, None),
    ("per_row_mask", runs(77, (0, 25), (0, 60)).expand(2, 1, 33, 77), 2, None),
    ("per_head_mask", runs(77, (0, 25), (0, 60)).expand(2, 3, 1, 77), 2, None),
    ("three_dims", runs(77, (0, 25), (0, 60))[:, 0], 2, None),
    ("other_batch", runs(77, (0, 25), (0, 60)), 3, None),
    ("not_a_tensor", None, 2, None),
]


@pytest.mark.parametrize("mask,batch,expected", [c[1:] for c in KW_CASES], ids=[c[0] for c in KW_CASES])
def test_key_windows(mask, batch, expected):
    assert windows_of(mask, batch, mask.shape[-1] if mask is not None else 77) == expected


def test_key_windows_of_another_key_count():
    assert _core.key_windows(runs(77, (0, 25), (0, 60)), 2, 78) is None


def test_key_windows_reads_back_once_per_mask_object(monkeypatch):
    reads = []
    real = _core._all_true
    monkeypatch.setattr(_core, "_all_true", lambda flags: (reads.append(1), real(flags))[1])
    mask = runs(77, (0, 25), (3, 60))
    first = _core.key_windows(mask, 2, 77)
    for _ in range(3):                                                 # every layer of a forward passes the same object
        again = _core.key_windows(mask, 2, 77)
        assert again[0] is first[0] and again[1] is first[1]
    assert len(reads) == 1
    ent = _core._KEY_WINDOW_CACHE[id(mask)]
    assert ent[0]() is mask and ent[1] == mask._version
    same_values = mask.clone()                                         # another object: its own read-back
    assert windows_of(same_values, 2, 77) == [(0, 25), (3, 60)] and len(reads) == 2
    mask[1, 0, 0, 60:70] = True                                        # edited in place: a fresh answer
    assert windows_of(mask, 2, 77) == [(0, 25), (3, 70)] and len(reads) == 3
    mask[0, 0, 0, 10] = False                                          # ... now with a hole
    assert _core.key_windows(mask, 2, 77) is None and len(reads) == 4
    assert _core.key_windows(mask, 2, 77) is None and len(reads) == 4  # None is cached too
    bad = runs(77, (0, 25), (3, 60)).float()                           # rejected by dtype: no read-back at all
    assert _core.key_windows(bad, 2, 77) is None and len(reads) == 4


def test_key_windows_cache_does_not_outlive_its_mask():
    for i in range(40):                                                # recycled ids never hit, and the cache stays small
        m = runs(64, (i % 7, 30 + i % 5))
        assert windows_of(m, 1, 64) == [(i % 7, 30 + i % 5)]
        del m
    assert len(_core._KEY_WINDOW_CACHE) <= 9


# ---------------------------------------------------------------------------------------------------------
# routing on CPU tensors
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", ["windows", "broadcast", "hole", "per_row", "none"])
@pytest.mark.parametrize("D", [64, 128])
def test_core_cross_attention_key_masked_on_cpu_is_sdpa(D, kind, dtype, monkeypatch):
    def no_kernel(*a, **kw):
        raise AssertionError("CPU tensors must not reach the binding")

    monkeypatch.setattr(nat, "cross_attention_keyrange", no_kernel)
    monkeypatch.setattr(nat, "cross_attention", no_kernel)
    g = torch.Generator().manual_seed(D)
    B, H, Sq, Skv = 2, 3, 33, 17
    q = torch.randn(B, Sq, H * D, generator=g).to(dtype).unflatten(2, (H, D)).transpose(1, 2)    # the processors' head views
    k, v = (torch.randn(B, Skv, H * D, generator=g).to(dtype).unflatten(2, (H, D)).transpose(1, 2) for _ in range(2))
    mask = {"windows": runs(Skv, (0, 9), (4, 17)), "broadcast": runs(Skv, (0, 9)), "hole": runs(Skv, (0, 9), [(0, 3), (5, 17)]),
            "per_row": torch.rand(B, 1, Sq, Skv, generator=g) > 0.3, "none": None}[kind]
    if kind == "per_row":
        mask[..., 0] = True
    ref = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, is_causal=False)
    out = _core.cross_attention_key_masked(q, k, v, mask)
    assert out.dtype == ref.dtype and out.shape == ref.shape and torch.equal(out, ref)
