#!/usr/bin/env python3
"""Writes tests/golden/svg1_layer_calls.json for tests/test_svg1_layer_call_cpu.py::test_layer_calls_equal_the_golden_transcript: the call
transcript of svg.models._core.svg1_attention_device_switch / svg1_sparse_attention and of the seven processors' attention_core_logic on
that module's cases — what they call below themselves, with which tensors, scalars, masks, keywords and sampled rows, under which timer
labels, what they leave in the CPU generators, what they return or refuse — recorded with stand-ins on CPU tensors, so it needs neither
a GPU nor the built library.  It imports this repository's code only.

The committed file was written by this script on commit 9ed2a93 ("Adaptive top-p and adaptive band: one kept-mass controller"), the last
one on which the layer-call was written out in both `_core` functions and in every processor: it is the reference for the one body they
share and must not be regenerated from later code.  To reproduce it, check that commit out, copy this script and the test module into it,
and run

    python tests/golden/make_golden_svg1_layer_calls.py
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "sparse-videogen_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

import test_svg1_layer_call_cpu as T  # noqa: E402


def main():
    records = T.record_all()
    again = T.record_all()
    assert records == again, "the transcript is not reproducible: " + str(T._differing(records, again)[:5])
    T.GOLDEN.write_text(T.dumps(records))
    refused = sum("raises" in r for r in records.values())
    print("wrote", T.GOLDEN, len(records), "cases,", refused, "of them refused,", T.GOLDEN.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
