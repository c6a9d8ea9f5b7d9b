#!/usr/bin/env python3
"""Writes tests/golden/band_replay_golden.npz for tests/test_gpu_band_speculative.py::test_replay_path_equals_the_kernel_before_the_change:
the band kernel's OWN bf16 output (not an oracle value) on that test's inputs, all 2 x 1344 rows in logical order, as it was before the
overflow test of the max-free softmax left the tile loop.  Run it on a GPU with the library of that commit:

    python sparse-videogen_amd/build.py --tag parent          # in a checkout of commit 68e34ea; copy lib/libsvgattn_parent.so here
    python tests/golden/make_golden_band_replay.py sparse-videogen_amd/lib/libsvgattn_parent.so

Before it writes, the output is checked against the fp32 oracle at the bf16 tolerance of tests/test_gpu_kernels.py."""
import ctypes
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent.parent
for p in (ROOT, ROOT / "sparse-videogen_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))
import torch  # noqa: E402
from svg import _native as nat  # noqa: E402

import test_gpu_band_speculative as T  # noqa: E402


def use_library(path):
    """point svg._native at the library of another commit, which may lack entry points this checkout declares"""
    lib = ctypes.CDLL(str(Path(path).resolve()))
    for name, (res, args) in nat.SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    assert int(lib.svg_abi_version()) == nat.SVG_ABI_VERSION
    nat._lib = lib


def main():
    if len(sys.argv) > 1:
        use_library(sys.argv[1])
    sp = T.replay_everywhere_spikes()
    q, k, v = T.build("band", sp, 5)
    o = T.launch("band", q, k, v, "static")
    assert torch.isfinite(o.float()).all()
    T.check_attn(o, T.reference("band", sp, 5), torch.bfloat16)
    out = o.reshape(-1, T.D).contiguous().view(torch.int16).numpy().view(np.uint16)
    np.savez_compressed(T.GOLDEN, attn_out_u16=out)
    print("wrote", T.GOLDEN, out.shape, T.GOLDEN.stat().st_size, "bytes; build:", nat.build_info())


if __name__ == "__main__":
    main()
