"""The return codes of the Euclidean k-means entries on arguments they refuse (include/svg_attn.h: svg_kmeans_xsq, _iter, _assign, _update,
_loop, _loop_strided, _loop_grouped, _loop_grouped_strided), host only: every check runs before any launch, so the rows pass placeholder
pointers and are skipped where a GPU is visible, as in tests/test_kmeans_metric_cpu.py.  No row passes every check.

tests/golden/kmeans_reject_codes.json holds what the library returned BEFORE the k-means host path shared one call record and one list
of checks (tests/golden/make_golden_kmeans_reject_codes.py names the commit).  It is the definition of "every entry refuses what it
refused, with the code it gave" — the order of the checks included (rows that break two at once) — and is never regenerated from newer
code."""
import json
from pathlib import Path

import pytest
import torch

from svg import _native as nat

GOLDEN = Path(__file__).resolve().parent / "golden" / "kmeans_reject_codes.json"
PH, PA, PB, PC, PD = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000   # placeholder device pointers, 16-byte aligned, never dereferenced
BIG = 1 << 40
B, N, K, D = 4, 700, 129, 128

# (parameter, default) per entry in the order of its prototype; xsq is NULL in every row: it is allowed to be
SHAPE = [("B", B), ("N", N), ("K", K), ("D", D), ("dtype", 0)]
WS = [("ws", PH), ("nb", BIG), ("stream", None)]
CENTS = [("c_init", PA), ("c_work_a", PB), ("c_work_b", PC)]
OUTS = [("labels", PH), ("counts", PH), ("sorted_idx", PH), ("centroids_out", PD), ("n_iters", PH)]
LOOP_TAIL = [("max_iters", 5), ("tol", 1e-4)]
ENTRIES = {
    "svg_kmeans_xsq": [("x", PH), ("xsq_out", PH), ("B", B), ("N", N), ("D", D), ("dtype", 0), ("stream", None)],
    "svg_kmeans_iter": [("x", PH), ("xsq", None), ("centroids_in", PA), ("centroids_out", PB), ("labels", PH), ("counts", PH), ("sorted_idx", PH),
                        ("shift", PH)] + SHAPE + WS,
    "svg_kmeans_assign": [("x", PH), ("centroids", PA), ("labels", PH)] + SHAPE + WS,
    "svg_kmeans_update": [("x", PH), ("labels", PH), ("centroids_in", PA), ("centroids_out", PB), ("counts", PH), ("sorted_idx", PH),
                          ("shift", PH)] + SHAPE + WS,
    "svg_kmeans_loop": [("x", PH), ("xsq", None)] + CENTS + OUTS + SHAPE + LOOP_TAIL + WS,
    "svg_kmeans_loop_strided": [("x", PH), ("stride", N * D)] + CENTS + OUTS + SHAPE + LOOP_TAIL + WS,
    "svg_kmeans_loop_grouped": [("x", PH), ("xsq", None)] + CENTS + OUTS + SHAPE + [("group", 2)] + LOOP_TAIL + WS,
    "svg_kmeans_loop_grouped_strided": [("x", PH), ("stride", N * D)] + CENTS + OUTS + SHAPE + [("group", 2)] + LOOP_TAIL + WS,
}
ALIASES = [("c_init_is_work_a", {"c_work_a": PA}), ("c_init_is_work_b", {"c_work_b": PA}), ("work_a_is_work_b", {"c_work_b": PB}),
           ("out_is_work_a", {"centroids_out": PB}), ("out_is_work_b", {"centroids_out": PC})]


def rows(entry):
    """-> [(row id, overrides)] of one entry; nb = "short": one byte less than the entry needs for the row's sizes"""
    params = [p for p, _ in ENTRIES[entry]]
    out = [(f"null_{p}", {p: None}) for p, v in ENTRIES[entry] if isinstance(v, int) and v >= PH and p not in ("nb", "stride")]
    out += [(f"{p}_0", {p: 0}) for p in ("B", "N", "K", "max_iters", "group") if p in params]
    if "group" in params:
        out += [("group_not_dividing_B", {"group": 3})]
    out += [(n, o) for n, o in (("K_8193", {"K": 8193}), ("D_96", {"D": 96}), ("dtype_2", {"dtype": 2})) if next(iter(o)) in params]
    if "nb" in params:
        # the pairs that pin the order of two checks: the metric table's *_before_* choices, and the single iteration's own order
        out += [("short_workspace", {"nb": "short"}), ("bad_arg_before_unsupported", {"N": 0, "K": 8193}),
                ("unsupported_K_and_workspace", {"K": 8193, "nb": 16}), ("unsupported_dtype_and_workspace", {"dtype": 2, "nb": 16}),
                ("unsupported_D_and_workspace", {"D": 96, "nb": "short"})]
    if "c_init" in params:
        out += ALIASES + [("workspace_before_alias", {"nb": "short", "c_work_a": PA}), ("unsupported_before_alias", {"D": 96, "c_work_b": PB})]
    if "stride" in params:
        out += [("stride_below_N_D", {"stride": N * D - 8}), ("stride_not_multiple_of_8", {"stride": N * D + 4}), ("x_not_16_byte_aligned", {"x": PH + 8}),
                ("alias_and_stride", {"c_work_b": PB, "stride": N * D + 4}), ("null_and_stride", {"c_init": None, "stride": N * D - 8}),
                ("size_and_alignment", {"K": 0, "x": PH + 8}), ("workspace_and_stride", {"nb": "short", "stride": N * D + 4})]
    assert len({n for n, _ in out}) == len(out)
    return out


def cases():
    return [(f"{entry}.{rid}", entry, over) for entry in ENTRIES for rid, over in rows(entry)]


def call(lib, entry, over):
    a = dict(ENTRIES[entry])
    assert set(over) <= set(a)
    a.update(over)
    if a.get("nb") == "short":
        bytes_of = {"svg_kmeans_loop": lambda: lib.svg_kmeans_loop_workspace_bytes(a["B"], a["N"], a["K"], a["D"]),
                    "svg_kmeans_loop_strided": lambda: lib.svg_kmeans_loop_workspace_bytes(a["B"], a["N"], a["K"], a["D"])}
        grouped = lambda: lib.svg_kmeans_loop_grouped_workspace_bytes(a["B"], a["N"], a["K"], a["D"], a["group"])  # noqa: E731
        single = lambda: lib.svg_kmeans_workspace_bytes(a["B"], a["N"], a["K"], a["D"])  # noqa: E731
        a["nb"] = int(bytes_of.get(entry, grouped if "group" in a else single)()) - 1
        assert a["nb"] > 0
    return int(getattr(lib, entry)(*[a[p] for p, _ in ENTRIES[entry]]))


def record_all(lib):
    return {cid: call(lib, entry, over) for cid, entry, over in cases()}


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_golden_holds_these_rows_and_none_that_passes(golden):
    assert sorted(golden) == sorted(c[0] for c in cases())
    assert all(code in (-1, -2, -3) for code in golden.values())   # SVG_ERR_BAD_ARG, _UNSUPPORTED, _WORKSPACE: never 0, never a launch
    for entry, params in ENTRIES.items():
        assert len(params) == len(nat.SIGNATURES[entry][1]), entry


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_entry_rejects_as_the_golden_says(golden, case):
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    cid, entry, over = case
    assert call(nat.load(), entry, over) == golden[cid]
