"""CPU checks of the joint (MMDiT) prologue: _core.joined_rows, the C entry point's argument validation (no GPU is touched: every
case is rejected before a launch), the ctypes struct layout, and joint_qkv_from_projections declining CPU tensors."""
import ctypes

import pytest
import torch


@pytest.mark.parametrize("B", [1, 2])
def test_joined_rows_is_a_view_of_adjacent_slices(B):
    from svg.models import _core

    x = torch.randn(B, 37, 16)
    for cut in (0, 1, 30, 37):
        a, b = x[:, :cut], x[:, cut:]
        j = _core.joined_rows(a, b)
        assert j is not None and torch.equal(j, torch.cat([a, b], dim=1))
        assert j.data_ptr() == x.data_ptr()                        # a view, not a copy
    a, b = x[:, 3:10], x[:, 10:20]                                  # a middle piece of the rows
    assert torch.equal(_core.joined_rows(a, b), torch.cat([a, b], dim=1))


def test_joined_rows_refuses_what_is_not_adjacent():
    from svg.models import _core

    x = torch.randn(2, 37, 16)
    assert _core.joined_rows(x[:, :10], x[:, 11:]) is None         # gap
    assert _core.joined_rows(x[:, :10], x[:, 9:]) is None          # overlap
    assert _core.joined_rows(x[:, 10:], x[:, :10]) is None         # wrong order
    assert _core.joined_rows(x[:, :10], torch.randn(2, 27, 16)) is None   # separate tensors
    y = torch.randn(2, 40, 16)
    assert _core.joined_rows(x[:, :10], y[:, 10:]) is None         # another storage
    z = torch.randn(2, 37, 32)
    assert _core.joined_rows(z[:, :10, :16], z[:, 10:, 16:]) is None     # same storage, b not where a ends
    assert _core.joined_rows(x[:1, :10], x[1:, 10:]) is None       # batch sizes differ
    t = torch.randn(2, 16, 37).transpose(1, 2)
    assert _core.joined_rows(x[:, :10], t[:, 10:]) is None         # strides differ


def test_struct_layout():
    from svg import _native

    assert ctypes.sizeof(_native.PrologueSegment) == 72
    assert _native.PrologueSegment.rows.offset == 24 and _native.PrologueSegment.q_weight.offset == 32
    assert _native.PrologueSegment.eps.offset == 64


def test_joint_entry_point_validation_returns_error_codes():
    from svg import _native

    lib = _native.load()
    fake_in, fake_out = 0x10000, 0x20000      # never dereferenced: every call below is rejected before a launch
    seg = (_native.PrologueSegment * 2)()
    for s in seg:
        s.q_in = s.k_in = s.v_in = fake_in
        s.rows, s.norm_kind, s.eps = 8, 1, 1e-6

    def call(n_seg=1, outs=(fake_out, fake_out + 0x1000, fake_out + 0x2000), bsz=1, H=2, D=64, dtype=0, rk=0, lo=0, hi=0, q_scale=1.0):
        return lib.svg_qk_norm_rope_transpose_joint(seg, n_seg, *outs, bsz, H, D, dtype, rk, None, None, lo, hi, q_scale, None)

    BAD, UNSUP = -1, -2
    assert lib.svg_qk_norm_rope_transpose_joint(None, 1, fake_out, None, None, 1, 2, 64, 0, 0, None, None, 0, 0, 1.0, None) == BAD
    assert call(n_seg=0) == BAD and call(n_seg=3) == BAD
    assert call(outs=(None, None, None)) == BAD
    assert call(outs=(None, fake_out + 0x1000, fake_out + 0x2000)) == BAD       # q input without its output
    assert call(outs=(fake_in, fake_out, fake_out + 0x1000)) == BAD             # an input equal to an output
    assert call(bsz=0) == BAD and call(H=0) == BAD and call(q_scale=0.0) == BAD
    assert call(rk=1) == BAD                                                    # RoPE without tables
    assert call(rk=3) == BAD
    assert call(H=1 << 24, D=128) == BAD                                        # total above INT32_MAX / (H * D)
    seg[0].norm_kind = 5
    assert call() == BAD
    seg[0].norm_kind, seg[0].rows = 1, -1
    assert call() == BAD
    seg[0].rows = 0
    assert call() == BAD                                                        # nothing to do
    seg[0].rows, seg[1].q_in = 8, None
    assert call(n_seg=2) == BAD                                                 # segment 1 has rows but no q
    seg[1].q_in = fake_in
    assert call(D=48) == UNSUP and call(dtype=7) == UNSUP


def test_joint_qkv_from_projections_declines_cpu_tensors():
    from svg.models import _core

    t = [torch.randn(1, 8, 256, dtype=torch.bfloat16) for _ in range(6)]
    assert _core.joint_qkv_from_projections(t[:3], t[3:], 2, None, None, None, None, None, None, 0, 8) is None
