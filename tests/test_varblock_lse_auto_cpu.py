"""svg_varblock_attention_lse_auto[_f32] without a GPU (include/svg_attn_varblock_lse_auto.h): one validation table of the two entries in
the documented order — every row is rejected on the host before any launch, the placeholder pointers are never read — and what the
wrappers refuse.  (The entries have no variant and no fp8 argument: the trace, block-row-order, mixed and fp8 schedules cannot be asked for.)
Argument lists: vb_args of tests/test_sparse_attention_lse_cpu.py (Hq 4, Hkv 2, Sq = Skv = 512, QB 4 — 128-row tiles —, KB 8)."""
import pytest
import torch

from svg import _native as nat
from test_sparse_attention_lse_cpu import BAD_ARG, PH, UNSUPPORTED, WORKSPACE, contiguous_layout, vb_args, vb_need

NAMES = ("svg_varblock_attention_lse_auto", "svg_varblock_attention_lse_auto_f32")
CASES = [
    ("null_lse_before_D96", vb_args(lse=None, D=96), BAD_ARG),
    ("null_o_before_short_workspace", vb_args(o=None, ws_bytes=0), BAD_ARG),          # (o32 of the _f32 entry)
    ("null_q_D64", vb_args(q=None, D=64), BAD_ARG),
    ("null_block_map", vb_args(bmap=None), BAD_ARG),
    ("null_workspace", vb_args(ws=None), BAD_ARG),
    ("Hq_not_multiple_of_Hkv", vb_args(Hq=3, D=64), BAD_ARG),
    ("KB_beyond_run_list", vb_args(KB=4033, ws_bytes=0), UNSUPPORTED),
    ("short_workspace_before_D96", vb_args(ws_bytes=vb_need() - 1, D=96), WORKSPACE),
    ("layout_heads0_before_D96", vb_args(lay=contiguous_layout(4, 512, 512, heads_per_batch=0), D=96), BAD_ARG),
    ("D96", vb_args(D=96), UNSUPPORTED),
    ("D96_two_phase_tiles", vb_args(D=96, QB=2), UNSUPPORTED),
    ("o_8_bytes_off_f32_tensors", vb_args(o=PH + 8, dtype=2), UNSUPPORTED),            # (_f32: the unaligned o32; the other: the dtype)
    ("layout_on_128_row_tiles", vb_args(lay=contiguous_layout(4, 512, 512)), UNSUPPORTED),
    ("layout_on_128_row_tiles_D64", vb_args(lay=contiguous_layout(4, 512, 512), D=64), UNSUPPORTED),
    ("dtype_f32", vb_args(dtype=2), UNSUPPORTED),
    ("dtype_f32_D64_two_phase_tiles", vb_args(dtype=2, D=64, QB=2), UNSUPPORTED),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("args,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_validation_table(name, args, expected):
    assert set(nat.VARBLOCK_LSE_AUTO_ENTRIES) == set(NAMES) and not set(NAMES) & set(nat.SIGNATURES)   # a table of their own
    assert getattr(nat.load(), name)(*args) == expected


def test_wrappers_refuse_before_the_library_is_loaded(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda *a, **k: pytest.fail("refused before the library is loaded"))
    q = torch.zeros(2, 64, 64, dtype=torch.bfloat16)
    bmap, sz = torch.ones(2, 1, 1, dtype=torch.bool), torch.full((2, 1), 64, dtype=torch.int32)
    with pytest.raises(ValueError, match="head_dim 128"):                    # without body: the 16x16x32 body only, as before
        nat.varblock_attention(q, q, q, bmap, sz, sz, return_lse=True)
    for kw in (dict(body="auto"), dict(body="auto", return_lse=True, variant=3), dict(body="auto", return_lse=True, fp8=True),
               dict(body="lockstep", return_lse=True)):
        with pytest.raises(ValueError, match="body"):
            nat.varblock_attention(q, q, q, bmap, sz, sz, **kw)
    q96 = torch.zeros(2, 64, 96, dtype=torch.bfloat16)
    for x in (q96, q.float()):
        with pytest.raises(ValueError, match="head_dim 128 or 64"):
            nat.varblock_attention(x, x, x, bmap, sz, sz, return_lse=True, body="auto")
    with pytest.raises(ValueError, match="token_major_out"):
        nat.varblock_attention_lse_auto(q, q, q, bmap, sz, sz, out_dtype=torch.float32, token_major_out=True)


def test_core_keeps_its_refusals_without_lse_auto_and_drops_the_size_rule_with_it():
    """on CPU tensors: with lse_auto the S >= 160 block-rows rule is gone (the call gets as far as asking for the GPU); fp8 and the tail at
    head_dim 64 are still refused"""
    from svg.models import _core

    geo = _core.Geometry(context_length=0, num_frame=6, frame_size=150, text_first=False)
    ad = _core.AdaptiveTopP(0.95)
    for D, kw in ((128, dict(adaptive=ad, top_p_store=_core.TopPStore())), (64, dict(adaptive=ad, top_p_store=_core.TopPStore())),
                  (128, dict(centroid_tail=True))):
        q = torch.zeros(1, 2, 900, D, dtype=torch.bfloat16)                     # 900 < 160 * 6
        if D == 128:
            with pytest.raises(ValueError, match="160 block-rows"):
                _core.svg2_sparse_attention(q, q, q, geo, _core.CentroidStore(), 0, 6, 12, 0.6, 0.0, 2, 1, **kw)
        with pytest.raises(RuntimeError, match="GPU"):
            _core.svg2_sparse_attention(q, q, q, geo, _core.CentroidStore(), 0, 6, 12, 0.6, 0.0, 2, 1, lse_auto=True, **kw)
    q64 = torch.zeros(1, 2, 900, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head_dim 64 has none"):
        _core.svg2_sparse_attention(q64, q64, q64, geo, _core.CentroidStore(), 0, 6, 12, 0.6, 0.0, 2, 1, centroid_tail=True, lse_auto=True)
    with pytest.raises(ValueError, match="not fp8"):
        _core.svg2_sparse_attention(q.float(), q.float(), q.float(), geo, _core.CentroidStore(), 0, 6, 12, 0.6, 0.0, 2, 1, adaptive=ad,
                                    top_p_store=_core.TopPStore(), lse_auto=True)
