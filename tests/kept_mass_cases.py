"""What the tests of the two kept-mass controllers share (svg_top_p_update, svg_band_width_update; csrc/kept_mass_control.hip): the float64
statement of the kept mass, the fp32 distance its bound is stated in, the parameters as the C ABI carries them, and the builder of
controller inputs.  No GPU needed."""
import math

import numpy as np
import torch


def kept_mass(lse_sparse, rows, lse_dense):
    """float64 [BH]: mean_i exp(lse_sparse[h, rows[i]] - lse_dense[h, i]); a -inf in lse_sparse counts 0.  numpy in, numpy out."""
    ls = np.asarray(lse_sparse, dtype=np.float64)[:, np.asarray(rows)]
    ld = np.asarray(lse_dense, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        term = np.where(np.isneginf(ls), 0.0, np.exp(ls - ld))
    return term.mean(axis=1)


def params32(kw):
    """the law's parameters as the C ABI's floats carry them"""
    return {name: float(np.float32(val)) for name, val in kw.items()}


def ulps32(a, b):
    """distance in fp32 units in the last place between two float32 arrays of finite values of one sign (0 included)"""
    ia = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def controller_inputs(seed, BH, S, R, delta, inf_head=2, nan_head=3):
    """(rows, lse_sparse [BH, S], lse_dense [BH, R]) of one controller call, CPU fp32.  rows: 0, S - 1 and a duplicate, then random ones (R = 1:
    S - 1 alone); lse_sparse normal * 3; lse_dense = lse_sparse[:, rows] + delta(g), delta given the generator after those draws -> [BH, R],
    the log of 1 / kept mass of every row.  Then the last row of head `inf_head` gets lse_sparse = -inf (a row the sparse form gave no key:
    it counts 0) and head `nan_head` all NaN (a head without a usable measurement); None: no such head."""
    g = torch.Generator().manual_seed(seed)
    rows = [S - 1] if R == 1 else ([0, S - 1, 5, 5] + torch.randint(0, S, (64,), generator=g).tolist())[:R]
    ls = torch.randn(BH, S, generator=g) * 3
    ld = ls[:, rows] + delta(g)
    if inf_head is not None:
        ls[inf_head, rows[-1]] = -math.inf
    if nan_head is not None:
        ls[nan_head] = math.nan
    return rows, ls, ld
