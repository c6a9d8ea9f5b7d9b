"""csrc/kmeans.hip (assign, update, the device Lloyd loop) against references that leave no room — the cases and rules of
tests/kmeans_exact_cases.py, shown sound and sharp without a GPU by tests/test_kmeans_exact_cases_cpu.py:

  A  assignment on small-integer inputs: labels torch.equal to the float64 arg-min, every row; K on and around the 64-centroid tile, N on
     and around the 256-point workgroup, ties planted at every seam of "lowest index wins"; the same labels through kmeans_iter, the
     library loop and its strided form;
  B  update on small-integer inputs and given labels: cluster sizes around every row path of kmeans_update_kernel, workgroups that walk
     two or three clusters; centroid bits, counts, sorted indices, shift;
  C  assignment on real-valued data under the derived margin eps, centroids under the derived bound;
  D  the loop for max_iters 1, 2, 3, step by step under the rules of C;
  E  a NaN shift — either sign bit — never converges.

Every output is checked for the poison pattern (tests/poisoned.py) before it is compared."""
import pytest
import torch

import kmeans_exact_cases as KC
from poisoned import assert_fully_written

pytestmark = pytest.mark.gpu

PARAMS = [(D, dtype) for D in KC.DIMS for dtype in KC.DTYPES]
IDS = [f"{D}-{str(dtype).replace('torch.', '')}" for D, dtype in PARAMS]


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def dev(t):
    return t.cuda().contiguous()


def written(what, **outs):
    for name, t in outs.items():
        assert_fully_written(t, f"{what}: {name}")


def assign(nat, x, c, what):
    labels = nat.kmeans_assign(dev(x), dev(c))
    written(what, labels=labels)
    assert labels.dtype == torch.int32 and labels.shape == x.shape[:2]
    return labels.cpu().long()


def assert_labels_equal(lab, ref, what):
    bad = lab != ref
    if bad.any():
        b, n = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} labels differ from the float64 arg-min (first index on ties); first "
                             f"[{b}, {n}]: got {int(lab[b, n])}, exact {int(ref[b, n])}")


# ---------------------------------------------------------------------------------------------------------
# A. assignment on exact inputs
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", PARAMS, ids=IDS)
@pytest.mark.parametrize("N,K", KC.ASSIGN_SHAPES)
def test_assign_exact(nat, N, K, D, dtype):
    x, c = KC.assign_case(N, K, D, dtype)
    what = f"kmeans_assign N={N} K={K}"
    assert_labels_equal(assign(nat, x, c, what), KC.assign_ref64(x, c), what)


@pytest.mark.parametrize("D,dtype", PARAMS, ids=IDS)
@pytest.mark.parametrize("name", sorted(KC.TIE_SETS))
def test_assign_planted_ties(nat, name, D, dtype):
    """one centroid value at the indices TIE_SETS[name], nine points bit-equal to it: the label is the lowest copy (and every other row
    the float64 arg-min); a point that IS a centroid (distance exactly 0) gets it"""
    x, c = KC.tie_case(name, D, dtype)
    what = f"kmeans_assign, copies at {KC.TIE_SETS[name]} ({name})"
    lab = assign(nat, x, c, what)
    got = lab[:, list(KC.TIE_POINTS)]
    assert (got == min(KC.TIE_SETS[name])).all(), f"{what}: the tied points got {got.tolist()}"
    assert (lab[:, KC.ZERO_POINT] == KC.ZERO_CENTROID).all()
    assert_labels_equal(lab, KC.assign_ref64(x, c), what)


@pytest.mark.parametrize("D,dtype", PARAMS, ids=IDS)
@pytest.mark.parametrize("N,K", KC.ROUTE_SHAPES)
def test_assign_exact_other_routes(nat, N, K, D, dtype):
    """the same labels through kmeans_iter, batch_kmeans_Euclid(max_iters=1, check_every=0) — the loop inside the library — and that loop
    on a [B, N + 40, D][:, :N] view (svg_kmeans_loop_strided); the update that follows is exact on these inputs too"""
    from svg.kmeans_utils import batch_kmeans_Euclid
    x, c = KC.assign_case(N, K, D, dtype)
    ref = KC.assign_ref64(x, c)
    lo, hi = KC.centroids_from_sums(*KC.cluster_sums64(x, ref, K), c)
    xd, cd = dev(x), dev(c)

    buf = nat.KmeansBuffers(KC.ASSIGN_B, N, K, D, xd.device)
    c_out = nat.empty_like(cd)
    nat.kmeans_iter(xd, None, cd, c_out, buf)
    what = f"kmeans_iter N={N} K={K}"
    written(what, labels=buf.labels, centroids=c_out, counts=buf.counts, sorted_idx=buf.sorted_idx, shift=buf.shift)
    assert_labels_equal(buf.labels.cpu().long(), ref, what)
    KC.check_sort(buf.counts, buf.sorted_idx, ref, K, what)
    KC.check_centroids_exact(c_out, lo, hi, what)
    KC.check_shift(buf.shift, c_out, c, what)

    big = torch.full((KC.ASSIGN_B, N + 40, D), 3.0, dtype=dtype)     # rows behind N: nearer to nothing, never read
    big[:, :N] = x
    view = big.cuda()[:, :N]
    assert not view.is_contiguous()
    for what, xin in ((f"library loop N={N} K={K}", xd), (f"strided library loop N={N} K={K}", view)):
        lab, cent, cnt, nit, sidx = batch_kmeans_Euclid(xin, K, max_iters=1, check_every=0, init_centroids=cd, return_sorted_indices=True)
        written(what, labels=lab, centroids=cent, counts=cnt, sorted_idx=sidx, n_iters=nit)
        assert int(nit) == 1
        assert_labels_equal(lab.cpu(), ref, what)
        KC.check_sort(cnt, sidx, ref, K, what)
        KC.check_centroids_exact(cent, lo, hi, what)     # max_iters = 1 without convergence: the centroids one update ahead of the labels


# ---------------------------------------------------------------------------------------------------------
# B. update on exact inputs
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", PARAMS, ids=IDS)
@pytest.mark.parametrize("B,K", KC.UPDATE_CONFIGS)
def test_update_exact(nat, B, K, D, dtype):
    x, labels, c_old, _ = KC.update_case(B, K, D, dtype)
    lo, hi, counts_ref = KC.update_reference(B, K, D, dtype)
    what = f"kmeans_update B={B} K={K} N={x.shape[1]}"
    xd, ld = dev(x), dev(labels)
    cent, counts, sidx, shift = nat.kmeans_update(xd, ld, dev(c_old))
    written(what, centroids=cent, counts=counts, sorted_idx=sidx, shift=shift)
    assert torch.equal(counts.cpu(), counts_ref)
    KC.check_sort(counts, sidx, labels, K, what)
    KC.check_centroids_exact(cent, lo, hi, what)
    KC.check_shift(shift, cent, c_old, what)
    assert float(shift.min()) > 0
    if B == 1:   # from its own output nothing moves (empty clusters keep their bits): the same centroids, a shift of exactly 0
        cent2, counts2, sidx2, shift2 = nat.kmeans_update(xd, ld, cent)
        written(what + " again", centroids=cent2, counts=counts2, sorted_idx=sidx2, shift=shift2)
        assert torch.equal(KC.bits16(cent2.cpu()), KC.bits16(cent.cpu())) and torch.equal(sidx2, sidx) and torch.equal(counts2, counts)
        assert shift2.cpu().tolist() == [0.0] * B


# ---------------------------------------------------------------------------------------------------------
# C. assignment on real-valued data: the derived margin
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", PARAMS, ids=IDS)
@pytest.mark.parametrize("kind", KC.REAL_KINDS)
def test_assign_real_valued_margin(nat, kind, D, dtype):
    """(a) 129 data points as centroids, (b) the library's own update of (a)'s labels as centroids.  A label outside rule C would be a
    finding about the MFMA's accumulation (the error model behind eps assumes fp32 round-to-nearest partial sums)."""
    x, ca = KC.real_case(kind, D, dtype)
    what = f"kmeans_assign {kind}"
    lab_a = assign(nat, x, ca, what + " (a)")
    KC.check_labels_margin(lab_a, x, ca, what + " (a) points as centroids")
    cent, counts, sidx, shift = nat.kmeans_update(dev(x), dev(lab_a.to(torch.int32)), dev(ca))
    written(what, centroids=cent, counts=counts, sorted_idx=sidx, shift=shift)
    KC.check_sort(counts, sidx, lab_a, KC.REAL_K, what)
    KC.check_centroids_bound(cent, x, lab_a, ca, what + " update of (a)")
    KC.check_shift(shift, cent, ca, what)
    cb = cent.cpu()
    KC.check_labels_margin(assign(nat, x, cb, what + " (b)"), x, cb, what + " (b) means as centroids")


# ---------------------------------------------------------------------------------------------------------
# D. loop steps under the sharp rules
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,dtype", PARAMS, ids=IDS)
def test_loop_steps(nat, D, dtype):
    """batch_kmeans_Euclid(max_iters=m, check_every=0), m = 1, 2, 3: iteration m assigned with the centroids run(m - 1) returned (rule C under
    them), and the returned centroids are the update of the returned labels (the centroid bound); counts and sorted indices exact"""
    from svg.kmeans_utils import batch_kmeans_Euclid
    x, c0 = KC.real_case("blobs", D, dtype)
    xd, c0d = dev(x), dev(c0)
    prev = c0
    for m in (1, 2, 3):
        what = f"library loop, max_iters={m}"
        lab, cent, cnt, nit, sidx = batch_kmeans_Euclid(xd, KC.REAL_K, max_iters=m, check_every=0, init_centroids=c0d, return_sorted_indices=True)
        written(what, labels=lab, centroids=cent, counts=cnt, sorted_idx=sidx, n_iters=nit)
        assert int(nit) == m
        lab = lab.cpu()
        KC.check_labels_margin(lab, x, prev, what)
        KC.check_sort(cnt, sidx, lab, KC.REAL_K, what)
        KC.check_centroids_bound(cent, x, lab, prev, what)
        prev = cent.cpu()


# ---------------------------------------------------------------------------------------------------------
# E. a NaN shift never converges
# ---------------------------------------------------------------------------------------------------------
def _n_iters(x, c0, **kw):
    from svg.kmeans_utils import batch_kmeans_Euclid
    out = batch_kmeans_Euclid(dev(x), KC.NAN_SHAPE["K"], max_iters=KC.NAN_MAX_ITERS, tol=KC.NAN_TOL, init_centroids=dev(c0), **kw)
    written(f"batch_kmeans_Euclid({kw})", labels=out[0], counts=out[2])
    n = out[3]
    return n.cpu().tolist() if torch.is_tensor(n) else n


@pytest.mark.parametrize("pattern", sorted(KC.NAN_PATTERNS))
def test_nan_shift_runs_to_max_iters(nat, pattern):
    """one row of batch 1 is NaN in every channel (0x7FC0, 0xFFC0): its centroid, hence the shift of batch 1, is NaN, and `NaN < tol` is
    False (ref svg/kmeans_utils.py:723; kmeans_commit_kernel) — the loop runs to max_iters, whatever the NaN's sign bit.  With one stopping
    group per batch, batch 0 stops where it stops without the NaN."""
    x, c0 = KC.nan_case()
    xn, _ = KC.nan_case(pattern)
    clean = _n_iters(x, c0, check_every=0)
    clean_groups = _n_iters(x, c0, check_every=0, group=1)
    assert clean < KC.NAN_MAX_ITERS and max(clean_groups) == clean
    assert _n_iters(xn, c0, check_every=0) == KC.NAN_MAX_ITERS
    assert _n_iters(xn, c0, check_every=0, group=1) == [clean_groups[0], KC.NAN_MAX_ITERS]
    assert _n_iters(xn, c0, check_every=1) == KC.NAN_MAX_ITERS     # the host-checked loop reads the same shift
