"""The cases and rules of tests/kmeans_exact_cases.py without a GPU and without the library: they are SOUND (the fp32 torch statement of each
kernel meets them — bit for bit on the exact inputs) and SHARP (five mutants of that statement fail them; two of those pass the
`assert_close(rtol=1e-2, atol=1e-2)` the centroids were checked with before).  tests/test_gpu_kmeans_exact.py applies the same rules to
csrc/kmeans.hip.

Figures this module prints (pytest -s; profiles/kmeans_exact_pytest_cpu.txt): the share of rows with an exact top-two tie per assignment
case, the share of centroid elements with two accepted roundings, the share of rows inside eps per real-valued case."""
import pytest
import torch

import kmeans_exact_cases as KC
from oracle import svg_oracle as O

DT = KC.DTYPES


def _name(dtype):
    return str(dtype).replace("torch.", "")


# ---------------------------------------------------------------------------------------------------------
# A. assignment on exact inputs
# ---------------------------------------------------------------------------------------------------------
def _assert_assign_exact(x, c, what):
    s32, s64 = KC.scores32(x, c), KC.scores64(x, c)
    assert s32.dtype == torch.float32 and torch.equal(s32.double(), s64), f"{what}: an fp32 score is not the float64 score"
    assert float(s64.abs().max()) < 2 ** 11 + 2 ** 10 and torch.equal(s64 * 2, (s64 * 2).round())   # multiples of 0.5 far below 2^24
    ref = KC.assign_ref64(x, c)
    assert torch.equal(s64.argmax(-1), ref), f"{what}: the arg-max of x.c - csq / 2 is not the arg-min of the distance"
    assert torch.equal(s32.argmax(-1), ref), f"{what}: the fp32 statement differs from the float64 labels"
    return s64, ref


@pytest.mark.parametrize("D", KC.DIMS)
@pytest.mark.parametrize("N,K", KC.ASSIGN_SHAPES)
def test_assign_cases_are_exact_in_fp32(N, K, D):
    for dtype in DT:
        x, c = KC.assign_case(N, K, D, dtype)
        assert x.dtype == dtype and x.shape == (2, N, D) and c.shape == (2, K, D) and not torch.equal(x[0], x[1])
        assert int(x.float().abs().max()) <= 3 and torch.equal(x.float(), x.float().round())
        _assert_assign_exact(x, c, f"N={N} K={K} D={D} {_name(dtype)}")


def test_assign_shapes_cover_the_edges():
    shapes = set(KC.ASSIGN_SHAPES)
    assert {(257, K) for K in (1, 2, 63, 64, 65, 128, 129, 200)} <= shapes                       # every K at N = 257
    assert {(N, K) for K in (65, 129) for N in (1, 33, 255, 256, 257, 700)} <= shapes            # every N at K = 65 and K = 129
    assert (33, 200) in shapes                                                                   # K above N
    assert KC.KBN == 64 and KC.WG_POINTS == 256
    assert set(KC.ROUTE_SHAPES) <= shapes and len(KC.ROUTE_SHAPES) == 2


@pytest.mark.parametrize("D", KC.DIMS)
def test_assign_cases_have_natural_ties(D):
    """at least 1 % of the rows of A have an exact top-two tie between two distinct centroids: "lowest index wins" decides real labels"""
    rows = ties = 0
    for N, K in KC.ASSIGN_SHAPES:
        x, c = KC.assign_case(N, K, D, DT[0])
        share = KC.exact_tie_share(KC.scores64(x, c))
        print(f"[natural ties] N={N} K={K} D={D}: {share:.4f}")
        rows, ties = rows + 2 * N, ties + share * 2 * N   # (a case has a few hundred rows: the share is asserted over all of A)
    print(f"[natural ties] D={D}: {ties / rows:.4f} of all rows of A")
    assert ties / rows >= 0.01


def test_tie_sets_sit_on_their_seams():
    t = {k: KC.tile_coords(k) for s in KC.TIE_SETS.values() for k in s}
    assert KC.TIE_K >= 129 and all(k < KC.TIE_K for k in t)
    for k, co in t.items():    # the index formula the sets are derived from
        assert k == 64 * co["tile"] + 32 * co["bb"] + 8 * co["rq"] + 4 * co["g"] + co["j"]
    same = lambda a, b, *keys: all(t[a][k] == t[b][k] for k in keys)   # noqa: E731
    a, b = KC.TIE_SETS["same_chain"]
    assert same(a, b, "tile", "g", "chain")
    a, b = KC.TIE_SETS["other_chain"]
    assert same(a, b, "tile", "g", "bb") and t[a]["chain"] != t[b]["chain"]
    a, b = KC.TIE_SETS["other_half"]
    assert same(a, b, "tile", "g") and t[a]["bb"] != t[b]["bb"]
    a, b = KC.TIE_SETS["next_tile"]
    assert same(a, b, "g", "bb", "rq", "j") and t[b]["tile"] == t[a]["tile"] + 1
    a, b = KC.TIE_SETS["cross_lane"]
    assert a < b and same(a, b, "tile") and t[a]["g"] == 1 and t[b]["g"] == 0   # the lowest copy is NOT in the lane that stores the label
    a, b = KC.TIE_SETS["ragged_tile"]
    assert t[b]["tile"] == (KC.TIE_K - 1) // 64 and KC.TIE_K % 64 == 1 and t[a]["tile"] < t[b]["tile"]
    assert len(KC.TIE_POINTS) >= 8 and KC.ZERO_POINT not in KC.TIE_POINTS and max(KC.TIE_POINTS) >= KC.WG_POINTS
    assert all(KC.ZERO_CENTROID not in s for s in KC.TIE_SETS.values())


@pytest.mark.parametrize("D", KC.DIMS)
@pytest.mark.parametrize("name", sorted(KC.TIE_SETS))
def test_planted_ties_go_to_the_lowest_copy(name, D):
    for dtype in DT:
        x, c = KC.tie_case(name, D, dtype)
        s64, ref = _assert_assign_exact(x, c, f"{name} D={D} {_name(dtype)}")
        copies = KC.TIE_SETS[name]
        pts = list(KC.TIE_POINTS)
        assert all(torch.equal(KC.bits16(x[:, p]), KC.bits16(c[:, k])) for p in pts for k in copies)
        assert (ref[:, pts] == min(copies)).all()
        top = s64[:, pts].topk(len(copies) + 1, dim=-1).values       # exactly the copies tie at the top
        assert (top[..., :-1] == top[..., :1]).all() and (top[..., -1] < top[..., 0]).all()
        assert (ref[:, KC.ZERO_POINT] == KC.ZERO_CENTROID).all()
        assert torch.equal(KC.bits16(x[:, KC.ZERO_POINT]), KC.bits16(c[:, KC.ZERO_CENTROID]))   # distance exactly 0


# ---------------------------------------------------------------------------------------------------------
# B. update on exact inputs
# ---------------------------------------------------------------------------------------------------------
def test_update_layout_meets_every_branch():
    assert KC.slots(128) == 16 and KC.slots(64) == 32
    assert int(KC.update_layout(4, 500, 128)[0].sum()) == 42017 and int(KC.update_layout(4, 500, 64)[0].sum()) == 83809
    assert KC.update_groups(4, 500) == 192 and KC.update_groups(1, 40) == 40
    for D in KC.DIMS:
        S = KC.slots(D)
        sz = KC.update_sizes(S)
        assert len(sz) == 18 and sz[10] == 4 * S + 1 and sz[17] == 25 * S + 7
        for B, K in KC.UPDATE_CONFIGS:
            per = KC.update_layout(B, K, D)
            assert (per.sum(1) == per[0].sum()).all()
            for b in range(B):
                rule = torch.tensor([sz[(7 * k + b) % 18] for k in range(K)])
                off = (per[b] != rule).nonzero().flatten().tolist()
                assert len(off) <= (b > 0) and all(rule[k] == sz[17] and per[b, k] > 11 * S for k in off)   # the one cluster that balances N
                assert set(per[b][per[b] == rule].tolist()) == set(sz)                                       # every size, untouched
        # B = 4, K = 500: a workgroup walks two or three clusters; every ordered pair of consecutive sizes of a walk (k, k + 192) occurs,
        # as 192 = 12 mod 18 moves the size index by 7 * 12 = 12 mod 18: three residues per walk, all 18 sizes as predecessors
        G = KC.update_groups(4, 500)
        assert all(len(range(k, 500, G)) in (2, 3) for k in range(G))
        per = KC.update_layout(4, 500, D)
        first = {(int(per[b, k]), int(per[b, k + G])) for b in range(4) for k in range(500 - G)}
        assert {a for a, _ in first} >= set(sz) and {n for _, n in first} >= set(sz)
        assert any(a == 0 for a, _ in first) and any(n == 0 for _, n in first)                               # empty clusters mid-walk


@pytest.mark.parametrize("D", KC.DIMS)
@pytest.mark.parametrize("B,K", KC.UPDATE_CONFIGS)
def test_update_cases_are_exact_in_fp32(B, K, D):
    for dtype in DT:
        x, labels, c_old, per = KC.update_case(B, K, D, dtype)
        sums64, counts = KC.cluster_sums64(x, labels, K)
        assert torch.equal(counts, per) and int(x.float().abs().max()) <= 3 and int(c_old.float().abs().max()) <= 3
        assert torch.equal(KC.cluster_sums32(x, labels, K).double(), sums64)
        lo, hi, cnt = KC.update_reference(B, K, D, dtype)
        share = KC.ambiguous_share(lo, hi)
        print(f"[ambiguous rounding] B={B} K={K} D={D} {_name(dtype)}: {share:.3e} of {lo.numel()} elements")
        assert share <= KC.AMBIGUOUS_CAP
        # the torch statement of the update (the oracle's) obeys the exact rule, counts included
        c_ref, cnt_ref = O.kmeans_update(x, labels.long(), c_old)
        KC.check_centroids_exact(c_ref, lo, hi, "oracle update")
        assert torch.equal(cnt_ref, cnt)
        assert torch.equal(KC.bits16(c_ref)[cnt == 0], KC.bits16(c_old)[cnt == 0]) and int((cnt == 0).sum()) > 0


def test_shift_reference_is_zero_when_nothing_moves():
    x, labels, c_old, _ = KC.update_case(1, 40, 128, DT[0])
    c1, _ = O.kmeans_update(x, labels.long(), c_old)
    c2, _ = O.kmeans_update(x, labels.long(), c1)
    assert torch.equal(KC.bits16(c1), KC.bits16(c2)) and float(KC.shift_ref64(c2, c1).max()) == 0.0
    assert float(KC.shift_ref64(c1, c_old).min()) > 1.0


# ---------------------------------------------------------------------------------------------------------
# C / D. real-valued data
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", KC.DIMS)
@pytest.mark.parametrize("kind", KC.REAL_KINDS)
def test_real_cases_hold_their_caps_and_the_fp32_statement_obeys_the_rules(kind, D):
    for dtype in DT:
        x, ca = KC.real_case(kind, D, dtype)
        assert x.shape == (KC.REAL_B, KC.REAL_N, D) and ca.shape == (KC.REAL_B, KC.REAL_K, D)
        if kind == "outlier_channels":
            assert float(x[..., ::16].float().min()) > 10 and float(x[..., 1::16].float().abs().max()) < 12
        what = f"{kind} D={D} {_name(dtype)}"
        lab_a = KC.scores32(x, ca).argmax(-1)
        share_a, _ = KC.check_labels_margin(lab_a, x, ca, f"[fp32 statement] {what} points as centroids")
        # (b) on the CPU: the means the torch statement makes of (a)'s labels
        cb, _ = O.kmeans_update(x, lab_a, ca)
        KC.check_centroids_bound(cb, x, lab_a, ca, f"[fp32 statement] {what} update")
        lab_b = KC.scores32(x, cb).argmax(-1)
        share_b, _ = KC.check_labels_margin(lab_b, x, cb, f"[fp32 statement] {what} means as centroids")
        print(f"[near ties] {what}: points as centroids {share_a:.4f} (half eps {KC.near_tie_share(x, ca, 0.5):.4f}), means as centroids "
              f"{share_b:.4f} (half eps {KC.near_tie_share(x, cb, 0.5):.4f})")
        assert max(share_a, share_b) <= KC.NEAR_TIE_CAP


@pytest.mark.parametrize("D", KC.DIMS)
def test_loop_case_does_not_converge_in_three_iterations(D):
    """D runs max_iters = 1, 2, 3 and expects n_iters = max_iters with the centroids one update ahead: the oracle's loop must not stop before"""
    for dtype in DT:
        x, c0 = KC.real_case("blobs", D, dtype)
        assert O.batch_kmeans_euclid(x, KC.REAL_K, max_iters=4, init_centroids=c0)[3] == 4


def test_ulp16():
    v = torch.tensor([1.0, 1.999, 2.0, -3.5, 0.0, 2.0 ** -20], dtype=torch.float64)
    assert KC.ulp16(v, torch.bfloat16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -27]
    assert KC.ulp16(v, torch.float16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24]


# ---------------------------------------------------------------------------------------------------------
# E. the NaN shift
# ---------------------------------------------------------------------------------------------------------
def test_nan_case_converges_without_the_nan_and_never_with_it():
    x, c0 = KC.nan_case()
    K = KC.NAN_SHAPE["K"]
    n_clean = O.batch_kmeans_euclid(x, K, max_iters=KC.NAN_MAX_ITERS, tol=KC.NAN_TOL, init_centroids=c0)[3]
    assert 2 <= n_clean < KC.NAN_MAX_ITERS, n_clean
    for b in range(2):   # each batch on its own (the stopping groups of group = 1) converges too
        assert O.batch_kmeans_euclid(x[b:b + 1], K, max_iters=KC.NAN_MAX_ITERS, tol=KC.NAN_TOL, init_centroids=c0[b:b + 1])[3] < KC.NAN_MAX_ITERS
    for pattern, bits in KC.NAN_PATTERNS.items():
        xn, _ = KC.nan_case(pattern)
        assert (KC.bits16(xn)[1, KC.NAN_ROW].int() & 0xFFFF == bits).all() and torch.equal(xn[0], x[0])
        assert O.batch_kmeans_euclid(xn, K, max_iters=KC.NAN_MAX_ITERS, tol=KC.NAN_TOL, init_centroids=c0)[3] == KC.NAN_MAX_ITERS   # NaN < tol is False


# ---------------------------------------------------------------------------------------------------------
# mutants of the torch statement: the new rules see them
# ---------------------------------------------------------------------------------------------------------
def _old_tolerance_passes(c, ref):
    try:
        torch.testing.assert_close(c.float(), ref.float(), rtol=1e-2, atol=1e-2)   # the centroid check of test_kmeans_iter and its kin
        return True
    except AssertionError:
        return False


def _exact_rule_passes(c, lo, hi):
    try:
        KC.check_centroids_exact(c, lo, hi, "mutant")
        return True
    except AssertionError:
        return False


def _row_mutant(x, labels, c_old, per, size, which, sign):
    """the update with one row of the first cluster of `size` rows of batch 0 left out (sign -1) or summed twice (+1): `which` = -1 the last
    row of the cluster in sorted order, 0 the first"""
    sums, counts = KC.cluster_sums64(x, labels, c_old.shape[1])
    k = int((per[0] == size).nonzero()[0])
    row = int((labels[0] == k).nonzero()[which])
    sums[0, k] += sign * x[0, row].double()
    return KC.centroids_from_sums(sums, counts, c_old)[0], k


@pytest.mark.parametrize("D", KC.DIMS)
def test_update_mutants_fail_the_exact_rule(D):
    """(1) the last row of a cluster of 4S + 1 rows dropped — the one-row tail —, (5) one row of a cluster of 25S + 7 rows counted twice.
    (5) passes the old tolerance on these very inputs: it moves an element by at most 3 / (25S + 7) < 0.01.  (1) moves an element by
    |x| / (4S + 1), up to 3 / 65 at means near 0, which the old absolute tolerance does see on integer inputs; the old check was blind to it
    where it was used, on values around 2 (rtol 1e-2 of 2 plus atol 1e-2 = 0.03): the twin 2 + x / 8 of the case, under the centroid bound of
    the real-valued rule (power-of-two counts put its quotients ON rounding boundaries, so the exact rule is not for it), shows it at D = 64
    in fp16 (129 rows: 2.375 / 129 = 0.018).  At D = 128 (65 rows: 2.375 / 65 = 0.037), and in bf16, whose spacing of 2^-6 at 2 turns the
    0.018 into one or two steps of 0.0156, the old check does see it: its gap for a dropped row begins at about 100 rows."""
    S = KC.slots(D)
    for dtype in DT:
        x, labels, c_old, per = KC.update_case(1, 40, D, dtype)
        lo, hi, _ = KC.update_reference(1, 40, D, dtype)
        ref, _ = O.kmeans_update(x, labels.long(), c_old)
        assert _exact_rule_passes(ref, lo, hi)
        m1, k1 = _row_mutant(x, labels, c_old, per, 4 * S + 1, -1, -1)
        m5, k5 = _row_mutant(x, labels, c_old, per, 25 * S + 7, 0, +1)
        assert not _exact_rule_passes(m1, lo, hi) and not _exact_rule_passes(m5, lo, hi)
        assert _old_tolerance_passes(m5, ref), "mutant (5) should pass the old tolerance: the gap"
        # the centroid bound of the real-valued rule sees both as well
        for m in (m1, m5):
            with pytest.raises(AssertionError):
                KC.check_centroids_bound(m, x, labels, c_old, "mutant")
        # values around 2: the twin of the case
        x2 = (2 + x.float() / 8).to(dtype)
        assert torch.equal(x2.float(), 2 + x.float() / 8)
        ref2, _ = O.kmeans_update(x2, labels.long(), c_old)
        KC.check_centroids_bound(ref2, x2, labels, c_old, "twin, torch statement")
        t1, _ = _row_mutant(x2, labels, c_old, per, 4 * S + 1, -1, -1)
        t5, _ = _row_mutant(x2, labels, c_old, per, 25 * S + 7, 0, +1)
        for t in (t1, t5):
            with pytest.raises(AssertionError):
                KC.check_centroids_bound(t, x2, labels, c_old, "twin, mutant")
        assert _old_tolerance_passes(t5, ref2)
        if D == 64 and dtype == torch.float16:
            assert _old_tolerance_passes(t1, ref2), "mutant (1) should pass the old tolerance at values around 2: the gap"


@pytest.mark.parametrize("D", KC.DIMS)
def test_assign_mutants_fail_the_exact_rule(D):
    for dtype in DT:
        # (2) ties go to the highest index: natural ties and every planted one
        x, c = KC.assign_case(257, 129, D, dtype)
        ref = KC.assign_ref64(x, c)
        highest = lambda s: s.shape[-1] - 1 - s.flip(-1).argmax(-1)   # noqa: E731
        assert not torch.equal(highest(KC.scores32(x, c)), ref)
        for name, copies in KC.TIE_SETS.items():
            xt, ct = KC.tie_case(name, D, dtype)
            got, want = highest(KC.scores32(xt, ct)), KC.assign_ref64(xt, ct)
            assert (got[:, list(KC.TIE_POINTS)] == max(copies)).all() and (want[:, list(KC.TIE_POINTS)] == min(copies)).all()
        # (3) centroid K - 1 ignored at K = 65 (the one centroid of the second tile)
        x, c = KC.assign_case(700, 65, D, dtype)
        ref = KC.assign_ref64(x, c)
        assert int((ref == 64).sum()) > 0 and not torch.equal(KC.scores32(x, c)[..., :64].argmax(-1), ref)
        # (4) batch 0's csq for batch 1
        x, c = KC.assign_case(257, 129, D, dtype)
        ref = KC.assign_ref64(x, c)
        csq = (c * c).float().sum(-1)
        got = KC.scores32(x, c, csq=csq[[0, 0]]).argmax(-1)
        assert torch.equal(got[0], ref[0]) and not torch.equal(got[1], ref[1])
        # ... and rule C sees (3) and (4) on real-valued data
        xr, cr = KC.real_case("blobs", D, dtype)
        with pytest.raises(AssertionError):
            KC.check_labels_margin(KC.scores32(xr, cr)[..., :-1].argmax(-1), xr, cr, "mutant (3)")
        with pytest.raises(AssertionError):
            KC.check_labels_margin(KC.scores32(xr, cr, csq=(cr * cr).float().sum(-1)[[0, 0]]).argmax(-1), xr, cr, "mutant (4)")
