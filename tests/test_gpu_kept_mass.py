"""The kept mass is one piece of device code with two users (csrc/kept_mass_control.hip head_kept_mass; svg_top_p_update,
svg_band_width_update): here the two entries are run on the same lse_sparse, rows and lse_dense, with zero gains, and tested against each
other — the same bits — and against the float64 statement (tests/kept_mass_cases.py).

Shapes: BH = 3, S = 70; R = 1 (one lane), 33 (one row beyond the 32-lane stage of the butterfly sum), 64 (the full wave); rows 0, S - 1 and a
duplicate; head 2 has a row without a key (-inf).  Bound, not from the code under test: kept is fp64 arithmetic rounded once to fp32, the
float64 statement rounded to fp32 can differ by that one rounding — 1 fp32 ulp (the rule of tests/test_gpu_adaptive_top_p.py).  Zero gains
with the state inside its clamps move nothing, so both state vectors keep their bits.  A row outside [0, S) makes every head's kept mass
NaN and leaves the state alone, on either entry."""
import functools

import numpy as np
import pytest
import torch

import kept_mass_cases as KM
from poisoned import load_native, unwritten

pytestmark = pytest.mark.gpu
BH, S = 3, 70
P0 = [0.5, 0.25, 0.77]
BAND0 = [1, 33, S + 1]


@pytest.fixture(scope="module")
def nat():
    return load_native()


@functools.lru_cache(maxsize=None)
def inputs(R):
    """lse_dense - lse_sparse in [0, 1): a kept mass in (1 / e, 1]"""
    return KM.controller_inputs(300 + R, BH, S, R, lambda g: torch.rand(BH, R, generator=g), inf_head=2, nan_head=None)


def run_both(nat, rows, ls, ld):
    """-> (kept of svg_top_p_update, kept of svg_band_width_update, top_p after, band after), zero gains, on poisoned kept buffers"""
    ls, rows, ld = ls.cuda(), torch.tensor(rows).cuda(), ld.cuda()
    p, band = torch.tensor(P0).cuda(), torch.tensor(BAND0, dtype=torch.int32).cuda()
    kept_p = nat.empty((BH,), dtype=torch.float32, device="cuda")
    kept_b = nat.empty((BH,), dtype=torch.float32, device="cuda")
    assert bool(unwritten(kept_p).all()) and bool(unwritten(kept_b).all())
    nat.top_p_update(ls, rows, ld, p, kept_p, 0.9, 0.0, 0.0, 0.02, 0.0, 1.0)
    nat.band_width_update(ls, rows, ld, band, kept_b, 0.9, 0.0, 0.0, 0.02, 1, 1, S + 1)
    return kept_p.cpu(), kept_b.cpu(), p.cpu(), band.cpu()


@pytest.mark.parametrize("R", [1, 33, 64])
def test_both_entries_write_the_same_kept_mass(nat, R):
    rows, ls, ld = inputs(R)
    assert len(rows) == R and S - 1 in rows and (R == 1 or (0 in rows and len(set(rows)) < R))
    kept_p, kept_b, p, band = run_both(nat, rows, ls, ld)
    assert not bool(unwritten(kept_p).any()) and not bool(unwritten(kept_b).any())     # every word written
    assert torch.equal(kept_p.view(torch.int32), kept_b.view(torch.int32)), (kept_p.tolist(), kept_b.tolist())
    ref = KM.kept_mass(ls.numpy(), rows, ld.numpy())
    for name, kept in (("top_p", kept_p), ("band", kept_b)):
        assert bool(torch.isfinite(kept).all()), (name, kept)
        u = KM.ulps32(kept.numpy(), ref.astype(np.float32))
        print(f"R={R} {name}: kept {kept.tolist()} float64 {ref.tolist()} ulps {u.tolist()}")
        assert (u <= 1).all(), name
    if R == 1:
        assert float(kept_p[2]) == 0.0                                                 # the -inf row added nothing
    assert torch.equal(p.view(torch.int32), torch.tensor(P0).view(torch.int32)) and band.tolist() == BAND0


@pytest.mark.parametrize("bad", [S, -1])
def test_a_row_out_of_range_gives_nan_and_moves_nothing_on_either_entry(nat, bad):
    rows, ls, ld = inputs(33)
    kept_p, kept_b, p, band = run_both(nat, rows[:5] + [bad] + rows[6:], ls, ld)
    for name, kept in (("top_p", kept_p), ("band", kept_b)):
        assert bool(torch.isnan(kept).all()) and not bool(unwritten(kept).any()), (name, kept)
    assert torch.equal(p.view(torch.int32), torch.tensor(P0).view(torch.int32)) and band.tolist() == BAND0
