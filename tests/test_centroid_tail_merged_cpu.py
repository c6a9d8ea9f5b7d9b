"""The merged centroid-tail entries without a GPU (include/svg_attn_centroid_tail_merged.h): the header where svg_attn.h includes it, its
prototypes against the ctypes table, and the validation on placeholder pointers in the documented order — the parent's five steps first."""
import ctypes as C
import re

import pytest

from svg import _native as nat
from test_centroid_tail_cpu import BAD_ARG, BIG, PA, PB, PC, PH, ROOT, UNSUPPORTED, WORKSPACE, host_only, layout

ENTRIES = ["svg_centroid_tail_merged_attention_lse", "svg_centroid_tail_merged_attention_lse_f32"]


def test_header_follows_the_parent_and_matches_the_table():
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', (ROOT / "include" / "svg_attn.h").read_text(), flags=re.M)
    assert includes[includes.index("svg_attn_centroid_tail.h") + 1] == "svg_attn_centroid_tail_merged.h"
    src = (ROOT / "include" / "svg_attn_centroid_tail_merged.h").read_text()
    assert "in this order" in src and "SVG_ABI_VERSION is unchanged" in src
    protos = re.findall(r"\bint (svg_\w+)\s*\(([^;{]*?)\)\s*;", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert [n for n, _ in protos] == ENTRIES == list(nat.CENTROID_TAIL_MERGED_ENTRIES) and not set(ENTRIES) & set(nat.SIGNATURES)
    kind = lambda p: "ptr" if "*" in p else "size" if "size_t" in p else "f32" if "float" in p else "i32"   # noqa: E731
    ctype = lambda a: {C.c_size_t: "size", C.c_float: "f32", C.c_int32: "i32"}.get(a, "ptr")                # noqa: E731
    for name, params in protos:
        res, args = nat.CENTROID_TAIL_MERGED_ENTRIES[name]
        assert res is C.c_int and [ctype(a) for a in args] == [kind(p) for p in params.split(",")], name
        assert getattr(nat.load(), name).argtypes == args


def args(q=PH, kbar=PA, vbar=PB, o_s=PC, lse_s=PA, o=PC, lse=PH, H=2, Sq=777, KC=70, D=128, dtype=0, cols=None, QB=6, ws=PH, nb=BIG, lay=None):
    return [q, kbar, vbar, o_s, lse_s, o, lse, H, Sq, KC, D, dtype, 0.088, PA, KC if cols is None else cols, PB, PC, QB, None, ws, nb, lay, None]


def o_layout(row=2 * 128, batch=777 * 2 * 128):   # (a token-major q member and an o member of its own: these entries address o through it)
    s = nat.TensorStrides(777 * 2 * 128, 128, 2 * 128)
    return C.byref(nat.AttnLayout(2, 0, s, s, s, nat.TensorStrides(batch, 128, row)))


CASES = [   # 1. - 5.: the parent's steps on the shared arguments, 6. and 7.: the sparse part
    ("null_before_everything_else", args(lse=None, o_s=None, cols=3, D=64, nb=0), BAD_ARG),
    ("map_cols_before_the_sparse_part", args(cols=69, o_s=None), BAD_ARG),
    ("layout_o_stride_not_multiple_of_8", args(lay=o_layout(batch=777 * 2 * 128 + 4)), UNSUPPORTED),
    ("layout_o_before_workspace", args(lay=o_layout(row=64), nb=0), BAD_ARG),
    ("layout_junk_o_member_is_read", args(lay=layout()), BAD_ARG),
    ("short_workspace_before_unsupported_and_sparse_part", args(nb=None, D=64, lse_s=None), WORKSPACE),
    ("D64_before_the_sparse_part", args(D=64, o_s=None), UNSUPPORTED),
    ("o_not_16_byte_aligned_before_the_sparse_part", args(o=PC + 2, lse_s=None), UNSUPPORTED),
    ("null_o_sparse", args(o_s=None), BAD_ARG),
    ("null_lse_sparse_before_alignment", args(lse_s=None, o_s=PC + 8), BAD_ARG),
    ("o_sparse_not_16_byte_aligned", args(o_s=PC + 8), UNSUPPORTED),
    ("o_sparse_not_16_byte_aligned_under_a_layout", args(o_s=PC + 8, lay=o_layout()), UNSUPPORTED),
]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("a,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_merged_entries_reject(entry, a, expected):
    host_only()
    lib = nat.load()
    if a[20] is None:
        a = a[:20] + [int(lib.svg_centroid_tail_workspace_bytes(a[7], a[17], a[9])) - 1] + a[21:]
    assert getattr(lib, entry)(*a) == expected
