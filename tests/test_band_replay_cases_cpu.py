"""tests/band_replay_cases.py on the CPU: the inputs of tests/test_gpu_band_replay_paths.py mean what the GPU tests assume they mean.
For every case the GPU file launches:
  * every spiked (row, key) is allowed by every mask the case uses, and the spiked rows are distinct unless the case pairs them;
  * each spike raises exactly ONE score per head it is built for — to `mag` in the log2 domain, within the rounding of q and k to the
    case's 16-bit type — and changes no other score of any head;
  * with the spikes removed no allowed score exceeds about +8 (log2 domain): what the kernel's reference holds before a spike arrives;
  * the oracle output is finite;
  * for the pairs of section 5 (b) the oracle row is the closed-form weighted mean of the two v rows, and neither weight is small.
Also: the builder that moved here from tests/test_gpu_band_speculative.py still makes the inputs of the committed golden fixture, the
geometry helpers agree with the library's work order, and the pre-scaled q carries the library's factor."""
import math
from collections import Counter

import numpy as np
import pytest
import torch

import band_replay_cases as C
from svg import _native as nat

CASES = {c.name: c for c in C.all_cases()}


def test_case_names_are_unique_and_the_list_is_complete():
    assert len(CASES) == len(C.all_cases())
    n_queue, n_sweep, n_pair = len(C.QUEUE_SUBSETS), len(C.SWEEP_MAGS), len(C.PAIR_MAGS) * len(C.PAIR_SECOND_TILE)
    assert len(CASES) == n_queue + 2 + 1 + n_sweep + n_pair + 1 + 2


def log2_scores(case, q, k):
    scale = 1.0 if case.prescaled else case.geo.c_log2
    return torch.matmul(q.double(), k.double().transpose(-1, -2))[0] * scale      # [H, S, S]


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_mean_what_the_gpu_tests_assume(name):
    case = CASES[name]
    g = case.geo
    masks = [C.bool_mask(kind, g) for kind in case.kinds]
    for s in case.spikes:
        assert 0 <= s.row < g.REAL and 0 <= s.key < g.REAL
        for m in masks:
            assert m[s.row, s.key], s
    per_row = Counter(s.row for s in case.spikes)
    pair_rows = {r for r, _, _ in case.pairs}
    assert all(n == (2 if r in pair_rows else 1) for r, n in per_row.items())      # a row of its own for every unpaired spike
    q, k, v = C.inputs(case)
    q0, k0, v0 = C.inputs(case._replace(spikes=(), pairs=()))
    assert torch.equal(v, v0)
    s1, s0 = log2_scores(case, q, k), log2_scores(case, q0, k0)
    allowed = masks[0].clone()
    for m in masks[1:]:
        allowed |= m
    assert float(s0[:, allowed].max()) < 8.5
    diff = s1 - s0
    want = torch.zeros_like(diff)
    eps = 2.0 ** -8 if case.dtype == torch.bfloat16 else 2.0 ** -11      # half an ulp of k, and of q where it is pre-scaled
    for s in case.spikes:
        for h in s.heads(g.H):
            want[h, s.row, s.key] = s.mag
            assert abs(float(diff[h, s.row, s.key]) - s.mag) <= eps * s.mag, (s, float(diff[h, s.row, s.key]))
    assert torch.equal(diff != 0, want != 0), "a spike touches a score it should not"
    for kind in case.kinds:
        assert torch.isfinite(C.oracle(case, kind)).all()


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.pairs))
def test_pair_rows_are_weighted_means_of_two_v_rows(name):
    """the closed form: softmax over the two spiked scores alone (every other key is below them by 50 and more in the log2 domain)"""
    case = CASES[name]
    q, k, v = C.inputs(case)
    s = log2_scores(case, q, k)
    ref = C.oracle(case, "band")
    for row, ka, kb in case.pairs:
        for h in range(case.geo.H):
            others = s[h, row].clone()
            others[[ka, kb]] = -math.inf
            assert float(others[C.bool_mask("band", case.geo)[row]].max()) < min(float(s[h, row, ka]), float(s[h, row, kb])) - 40
            wa = 1.0 / (1.0 + 2.0 ** float(s[h, row, kb] - s[h, row, ka]))
            assert 0.1 <= wa <= 0.9, (name, row, h, wa)      # a real mixture: an error of either weight shows in the row
            mean = wa * v[0, h, ka].double() + (1.0 - wa) * v[0, h, kb].double()
            assert float((ref[0, h, row].double() - mean).abs().max()) < 1e-3, (name, row, h)


def test_replaying_pairs_and_q_tiles():
    a = C.GEO_A
    assert a.S == 1344 and a.q_tiles("band") == [(0, 256), (256, 512), (512, 768), (768, 1024), (1024, 1280), (1280, 1320), (1320, 1344)]
    assert a.q_tiles("dense") == [(256 * i, min(1344, 256 * i + 256)) for i in range(6)]
    b = C.GEO_B
    assert (b.V, b.REAL, b.S) == (1200, 1240, 1300) and b.S % C.BN == 20
    assert b.q_tiles("band") == [(0, 256), (256, 512), (512, 768), (768, 1024), (1024, 1200), (1200, 1240), (1240, 1300)]
    assert b.q_tiles("dense_real") == [(0, 256), (256, 512), (512, 768), (768, 1024), (1024, 1240), (1240, 1300)]
    assert b.V // C.BN == 18 and (b.REAL - 1) // C.BN == 19          # the text columns straddle key tiles 18 and 19
    assert len(C.queue_case("all6").replaying_pairs()) == 12 and len(C.queue_case("024").replaying_pairs()) == 6
    for which in ("first", "last"):
        case = C.queue_case(which)
        (h, (reg, j)), = case.replaying_pairs()
        assert (h, j if reg == 0 else 5) == C.queue_edge_item(which)
    r = C.ragged_case()
    assert C.q_tiles_of("band", [s.row for s in r.spikes], b) == 4 and C.q_tiles_of("dense_real", [s.row for s in r.spikes], b) == 3
    # the rows of section 5: wave 0 of q-tile 2 and wave 7 of q-tile 1 (32 rows per wave), both schedules start at key tile 0
    assert (C.ROW_W0 - 512) // 32 == 0 and (C.ROW_W7 - 256) // 32 == 7
    band = C.bool_mask("band")
    assert band[C.ROW_W0, 3 * 64:9 * 64].all() and band[C.ROW_W7, 0:9 * 64].all() and band[512:768, 0:64].any() and band[256:512, 0:64].any()


@pytest.mark.parametrize("kind,geo", [("band", C.GEO_A), ("band", C.GEO_B), ("dense_real", C.GEO_B), ("dense_real", C.GEO_A)])
def test_q_tiles_are_the_work_items_of_the_library(kind, geo):
    order = C.queue_order(geo, kind)
    nqt = len(geo.q_tiles(kind))
    assert sorted(i for _, i, _ in order) == list(range(geo.H * nqt))


def test_prescaled_q_carries_the_library_factor():
    case = C.queue_case("all6", prescaled=True)
    q, _, _ = C.inputs(case)
    q0, _, _ = C.inputs(case._replace(prescaled=False, dtype=torch.float32))
    assert torch.equal(q, (q0 * nat.softmax_q_scale(case.geo.D)).to(torch.bfloat16))


def test_moved_builder_still_makes_the_inputs_of_the_golden_fixture():
    """tests/golden/band_replay_golden.npz holds the kernel's output on build("band", replay_everywhere_spikes(), 5); the oracle on the
    inputs the moved builder makes must lie within the bf16 tolerance of it, spiked rows included"""
    from pathlib import Path

    gold = np.load(Path(__file__).resolve().parent / "golden" / "band_replay_golden.npz")["attn_out_u16"]
    gold = torch.from_numpy(gold.view(np.int16)).view(torch.bfloat16).float().view(1, C.GEO_A.H, C.GEO_A.S, C.GEO_A.D)
    ref = C.reference("band", C.replay_everywhere_spikes(), 5)
    torch.testing.assert_close(gold, ref, atol=1e-2, rtol=1e-2)
    assert torch.equal(ref, C.oracle(C.queue_case("all6"), "band"))      # the all-six case IS that input
    _, _, v = C.build("band", C.replay_everywhere_spikes(), 5)
    for row, key, _ in C.replay_everywhere_spikes():
        torch.testing.assert_close(gold[0, :, row], v[0, :, key].float(), atol=1e-2, rtol=1e-2)
