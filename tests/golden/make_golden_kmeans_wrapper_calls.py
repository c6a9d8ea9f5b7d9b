#!/usr/bin/env python3
"""Writes tests/golden/kmeans_wrapper_calls.json for tests/test_kmeans_wrapper_calls_cpu.py::test_wrapper_calls_equal_the_golden: the call
transcript of the k-means wrappers (kmeans_loop, kmeans_loop_e4m3, kmeans_loop_metric, kmeans_assign[_metric], kmeans_update[_metric],
kmeans_assign_e4m3, KmeansSteppedSide) on that module's cases, recorded with a stand-in library on CPU tensors, so it needs neither a GPU
nor the built library.

The committed file was written by this script on commit 535eece ("flash-kmeans: cosine and dot-product metrics on the device loop"), the
last one on which each loop wrapper carried its own view rule, cache lookup and allocations: it is the reference for their shared helper
and must not be regenerated from later code.  To reproduce it, check that commit out, copy this script and the test module into it, and
run

    python tests/golden/make_golden_kmeans_wrapper_calls.py
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "sparse-videogen_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import test_kmeans_wrapper_calls_cpu as W  # noqa: E402


def main():
    records = W.record_all()
    W.GOLDEN.write_text(W.T.dumps(records))
    print("wrote", W.GOLDEN, len(records), "cases,", sum(len(r) for r in records.values()), "wrapper calls,", W.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
