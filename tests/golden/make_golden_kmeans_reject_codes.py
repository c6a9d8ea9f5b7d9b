#!/usr/bin/env python3
"""Writes tests/golden/kmeans_reject_codes.json for tests/test_kmeans_euclid_reject_cpu.py: the return code of every row of that module's
table — the Euclidean k-means entries on arguments they refuse — from the built library, on a machine WITHOUT a GPU (the rows pass
placeholder pointers; none of them reaches a launch).

The committed file was written by this script on commit 535eece ("flash-kmeans: cosine and dot-product metrics on the device loop"), the
last one whose k-means entries each spelled out their own checks: it is the reference for the shared checks of the call record and must
not be regenerated from later code.  To reproduce it, check that commit out, build it, copy this script and the test module into it, and
run

    python tests/golden/make_golden_kmeans_reject_codes.py
"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "sparse-videogen_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import torch  # noqa: E402

import test_kmeans_euclid_reject_cpu as T  # noqa: E402


def main():
    assert not torch.cuda.is_available(), "placeholder pointers: run where no GPU is visible"
    records = T.record_all(T.nat.load())
    assert all(code in (-1, -2, -3) for code in records.values()), {k: v for k, v in records.items() if v not in (-1, -2, -3)}
    T.GOLDEN.write_text(json.dumps(records, indent=0, sort_keys=True) + "\n")
    print("wrote", T.GOLDEN, len(records), "rows")


if __name__ == "__main__":
    main()
