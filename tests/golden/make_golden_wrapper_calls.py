#!/usr/bin/env python3
"""Writes tests/golden/wrapper_calls.json for tests/test_wrapper_layout_plan_cpu.py::test_wrapper_calls_equal_the_golden: the call
transcript of the attention wrappers of svg._native, svg._probe and svg._adaptive on that module's cases — entries called, which tensor
every pointer is, layouts, scalar arguments, what is returned and what the wrapper filled itself — recorded with a stand-in library on
CPU tensors, so it needs neither a GPU nor the built library.

The committed file was written by this script on commit 2c47837 ("SVG2: per-head top-p on the device, steered by measured kept mass"),
the last one whose wrappers each decided their layout by hand: it is the reference for the wrappers' one layout plan and must not be
regenerated from later code.  To reproduce it, check that commit out, copy this script and the test module into it, and run

    python tests/golden/make_golden_wrapper_calls.py
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "sparse-videogen_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import test_wrapper_layout_plan_cpu as T  # noqa: E402


def main():
    records = T.record_all()
    T.GOLDEN.write_text(T.dumps(records))
    refused = sum("raises" in r for r in records.values())
    print("wrote", T.GOLDEN, len(records), "cases,", refused, "of them refused,", T.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
