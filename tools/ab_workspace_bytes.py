#!/usr/bin/env python3
"""svg_varblock_workspace_bytes and svg_varblock_attention_fp8_workspace_bytes of two builds of the library over a grid of arguments:
callers size buffers by them and svg/_native.py reads the workspace at fixed offsets, so a refactoring of the layout code must return
the same number for every argument.  Host-only: runs without a GPU.
    python tools/ab_workspace_bytes.py [lib A, default lib/libsvgattn_parent.so] [lib B, default lib/libsvgattn.so]
Exit code 1 if any value differs."""
import ctypes as C
import itertools
import sys
from pathlib import Path

L = Path(__file__).resolve().parent.parent / "sparse-videogen_amd" / "lib"
paths = [Path(sys.argv[1]) if len(sys.argv) > 1 else L / "libsvgattn_parent.so", Path(sys.argv[2]) if len(sys.argv) > 2 else L / "libsvgattn.so"]
libs = [C.CDLL(str(p.resolve())) for p in paths]
for lib in libs:
    lib.svg_varblock_workspace_bytes.restype = C.c_size_t
    lib.svg_varblock_workspace_bytes.argtypes = [C.c_int32] * 5
    lib.svg_varblock_attention_fp8_workspace_bytes.restype = C.c_size_t
    lib.svg_varblock_attention_fp8_workspace_bytes.argtypes = [C.c_int32] * 7

HEADS = [(1, 1), (4, 4), (8, 2), (40, 40), (24, 8), (0, 1), (4, 0), (-1, 1)]                      # Hq == Hkv, Hq != Hkv, zero, negative
QB = [1, 3, 7, 100, 257, 300, 1023, 4095, 4096, 32767, 32768, 0, -5]                              # odd and even, both packing limits
KB = [1, 31, 32, 33, 127, 500, 1000, 1023, 1024, 1025, 1031, 2000, 4031, 4032, 4033, 5000, 0, -1]  # both sides of 1024 and of 4032
SQ = [1, 17, 63, 64, 65, 255, 256, 1000, 75600, 115200, 1 << 20, 0, -64]                          # Sq < 64, production sizes
SKV = [1, 75600, 115456, 0, -1]
DS = [64, 128, 96]

n = bad = zeros = 0
for (hq, hkv), qb, kb, sq in itertools.product(HEADS, QB, KB, SQ):
    a, b = (lib.svg_varblock_workspace_bytes(hq, hkv, qb, kb, sq) for lib in libs)
    n += 1
    zeros += a == 0
    if a != b:
        bad += 1
        print("DIFF svg_varblock_workspace_bytes", (hq, hkv, qb, kb, sq), a, b)
    for skv, d in itertools.product(SKV, DS):
        a, b = (lib.svg_varblock_attention_fp8_workspace_bytes(hq, hkv, qb, kb, sq, skv, d) for lib in libs)
        n += 1
        zeros += a == 0
        if a != b:
            bad += 1
            print("DIFF svg_varblock_attention_fp8_workspace_bytes", (hq, hkv, qb, kb, sq, skv, d), a, b)
print(f"A = {paths[0].name}, B = {paths[1].name}: {n} argument tuples ({zeros} of them return 0), {bad} differ")
sys.exit(1 if bad else 0)
