"""The cosine / dot-product k-means entries without a GPU (include/svg_attn_kmeans_metric.h): the exports and the header against the
ctypes table, and the return codes of the four entries in their documented order — every check runs on the host before any launch
(rows that pass placeholder pointers are skipped where a GPU is visible, as in tests/test_kmeans_e4m3_cpu.py)."""
import re
from pathlib import Path

import pytest
import torch

from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH, PA, PB, PC = 0x10000, 0x20000, 0x30000, 0x40000   # placeholder device pointers (16-byte aligned; never dereferenced by a rejected call)
ROOT = Path(__file__).resolve().parent.parent
BIG = 1 << 40


def test_entries_header_and_wrappers():
    lib = nat.load()
    for name, (res, args) in nat.KMEANS_METRIC_ENTRIES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert not set(nat.KMEANS_METRIC_ENTRIES) & set(nat.SIGNATURES) and int(lib.svg_abi_version()) == nat.SVG_ABI_VERSION == 4
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', (ROOT / "include" / "svg_attn.h").read_text(), flags=re.M)
    assert "svg_attn_kmeans_metric.h" in includes[:-4]
    src = (ROOT / "include" / "svg_attn_kmeans_metric.h").read_text()
    protos = re.findall(r"^(?:int|size_t) (svg_\w+)\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.M)
    assert {n for n, _ in protos} == set(nat.KMEANS_METRIC_ENTRIES) and "in this order" in src
    for name, params in protos:
        assert len(params.split(",")) == len(nat.KMEANS_METRIC_ENTRIES[name][1]), name
    sib = nat.SIGNATURES["svg_kmeans_loop_grouped_strided"][1]      # the loop: that argument list with the metric in front of group
    assert nat.KMEANS_METRIC_ENTRIES["svg_kmeans_loop_metric"][1] == sib[:15] + [sib[15]] + sib[15:]
    for name in ("kmeans_assign_metric", "kmeans_update_metric", "kmeans_loop_metric"):
        assert callable(getattr(nat, name))
    from svg import kmeans_metric as KU

    x = torch.zeros(2, 64, 128, dtype=torch.bfloat16)
    for fn in (KU.batch_kmeans_Cosine, KU.batch_kmeans_Dot):
        with pytest.raises(AssertionError, match="requires GPU tensors"):
            fn(x, 4, max_iters=3)
    with pytest.raises(AssertionError, match="CUDA"):
        KU.triton_centroid_update_cosine(x, torch.zeros(2, 64, dtype=torch.int64), x[:, :4])


def test_loop_workspace_bytes():
    loop = nat.load().svg_kmeans_loop_metric_workspace_bytes
    assert loop(4, 700, 129, 128, 2) >= nat.load().svg_kmeans_loop_grouped_workspace_bytes(4, 700, 129, 128, 2) + 4 * 129 * 128 * 2
    assert loop(4, 700, 8192, 64, 4) > 0
    for bad in ((4, 700, 129, 128, 3), (4, 700, 129, 128, 0), (0, 700, 129, 128, 1), (4, 0, 129, 128, 2), (4, 700, 0, 128, 2),
                (4, 700, 8193, 128, 2), (4, 700, 129, 96, 2)):
        assert loop(*bad) == 0, bad


def assign_args(x=PH, c=PA, lab=PC, B=4, N=700, K=129, D=128, dtype=0, metric=1, ws=PH, nb=BIG):
    return ["svg_kmeans_assign_metric", x, c, lab, B, N, K, D, dtype, metric, ws, nb, None]


def update_args(x=PH, lab=PA, ci=PB, co=PC, cnt=PH, srt=PH, sh=PH, B=4, N=700, K=129, D=64, dtype=1, metric=2, ws=PH, nb=BIG):
    return ["svg_kmeans_update_metric", x, lab, ci, co, cnt, srt, sh, B, N, K, D, dtype, metric, ws, nb, None]


def loop_args(x=PH, xbs=None, c0=PA, ca=PB, cb=PC, lab=PH, cnt=PH, srt=PH, out=PH, n=PH, B=4, N=700, K=129, D=128, dtype=0, metric=1, group=2,
              iters=5, tol=1e-4, ws=PH, nb=BIG):
    return ["svg_kmeans_loop_metric", x, N * D if xbs is None else xbs, c0, ca, cb, lab, cnt, srt, out, n, B, N, K, D, dtype, metric, group, iters,
            tol, ws, nb, None]


CASES = [
    ("assign_null_x", assign_args(x=None), BAD_ARG), ("assign_null_labels", assign_args(lab=None), BAD_ARG),
    ("assign_null_workspace", assign_args(ws=None), BAD_ARG), ("assign_N0", assign_args(N=0), BAD_ARG),
    ("assign_metric_euclid", assign_args(metric=0), BAD_ARG), ("assign_metric_3", assign_args(metric=3), BAD_ARG),
    ("assign_metric_before_unsupported", assign_args(metric=0, D=96), BAD_ARG), ("assign_D96", assign_args(D=96), UNSUPPORTED),
    ("assign_K8193", assign_args(K=8193), UNSUPPORTED), ("assign_unsupported_before_workspace", assign_args(dtype=2, nb=16), UNSUPPORTED),
    ("assign_short_workspace", assign_args(nb="iter"), WORKSPACE), ("update_null_labels", update_args(lab=None), BAD_ARG),
    ("update_null_out", update_args(co=None), BAD_ARG), ("update_null_shift", update_args(sh=None), BAD_ARG),
    ("update_K0", update_args(K=0), BAD_ARG), ("update_metric_euclid", update_args(metric=0), BAD_ARG),
    ("update_metric_neg", update_args(metric=-1), BAD_ARG), ("update_dtype_f32", update_args(dtype=2), UNSUPPORTED),
    ("update_short_workspace", update_args(nb="iter"), WORKSPACE), ("loop_null_c_init", loop_args(c0=None), BAD_ARG),
    ("loop_null_n_iters", loop_args(n=None), BAD_ARG), ("loop_max_iters0", loop_args(iters=0), BAD_ARG), ("loop_group0", loop_args(group=0), BAD_ARG),
    ("loop_group_not_dividing_B", loop_args(group=3), BAD_ARG), ("loop_metric_euclid", loop_args(metric=0), BAD_ARG),
    ("loop_metric_3", loop_args(metric=3), BAD_ARG), ("loop_metric_before_unsupported", loop_args(metric=3, K=9000), BAD_ARG),
    ("loop_D96", loop_args(D=96), UNSUPPORTED), ("loop_unsupported_before_workspace", loop_args(dtype=2, nb=16), UNSUPPORTED),
    ("loop_short_workspace", loop_args(nb="loop"), WORKSPACE), ("loop_workspace_of_the_euclidean_loop_is_short", loop_args(nb="sibling"), WORKSPACE),
    ("loop_workspace_before_alias", loop_args(nb="loop", ca=PA), WORKSPACE), ("loop_c_init_is_work_a", loop_args(ca=PA), BAD_ARG),
    ("loop_out_is_work_b", loop_args(out=PC), BAD_ARG), ("loop_alias_before_stride", loop_args(cb=PB, xbs=700 * 128 + 4), BAD_ARG),
    ("loop_stride_below_N_D", loop_args(xbs=700 * 128 - 8), BAD_ARG), ("loop_stride_not_multiple_of_8", loop_args(xbs=700 * 128 + 4), UNSUPPORTED),
    ("loop_x_not_16_byte_aligned", loop_args(x=PH + 8), UNSUPPORTED),
]


@pytest.mark.parametrize("a,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_entries_reject(a, expected):
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    lib = nat.load()
    name, a = a[0], list(a[1:])
    if isinstance(a[-2], str):      # one byte less than the entry needs; "sibling": what the Euclidean loop of these sizes needs
        B, N, K, D = a[3:7] if name == "svg_kmeans_assign_metric" else (a[7:11] if name == "svg_kmeans_update_metric" else a[10:14])
        need = {"iter": lambda: lib.svg_kmeans_workspace_bytes(B, N, K, D) - 1,
                "loop": lambda: lib.svg_kmeans_loop_metric_workspace_bytes(B, N, K, D, a[16]) - 1,
                "sibling": lambda: lib.svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, a[16])}[a[-2]]()
        a[-2] = int(need)
        assert a[-2] > 0
    assert getattr(lib, name)(*a) == expected
