#!/usr/bin/env python3
"""Golden vectors of the reference's CogVideoX token reorder helpers (`token_reorder_to_token_major` / `token_reorder_to_frame_major` of
svg/models/cog/placement.py, torch only; the module imports triton at load time), executed on one seeded [1, 2, F * P + ctx, 4] input.
Writes tests/golden/placement_golden.npz, read by tests/test_processors_cpu.py::test_token_reorder_helpers_match_the_reference.
    python tests/golden/make_golden_placement.py <checkout of the reference>"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

OUT = Path(__file__).resolve().parent / "placement_golden.npz"
F_, P_, CTX = 3, 5, 4


def main(ref_root: str):
    spec = importlib.util.spec_from_file_location("_ref_cog_placement", Path(ref_root) / "svg/models/cog/placement.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    x = torch.randn(1, 2, F_ * P_ + CTX, 4, generator=torch.Generator().manual_seed(0))
    out = {
        "geometry": np.array([F_, P_, CTX], dtype=np.int64),
        "x": x.numpy(),
        "cog_to_token_major": ref.token_reorder_to_token_major(x.clone(), CTX, F_ * P_, F_, P_).numpy(),
        "cog_to_frame_major": ref.token_reorder_to_frame_major(x.clone(), CTX, F_ * P_, F_, P_).numpy(),
    }
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} B)")


if __name__ == "__main__":
    main(sys.argv[1])
