"""The e4m3 k-means assignment on the GPU (include/svg_attn_kmeans_e4m3.h; csrc/kmeans.hip) against the float64 statement of
tests/kmeans_e4m3_cases.py, shown sound and sharp without a GPU by tests/test_kmeans_e4m3_cpu.py:

  1  exact inputs: small integers survive the quantiser, so the labels are torch.equal to the float64 arg-min — every shape and planted tie
     of tests/kmeans_exact_cases.py at head_dim 128, and the same with a planted offset handed in as mu;
  2  real-valued inputs around the centre svg_kmeans_centre computes: rule C against the e4m3 statement;
  3  svg_kmeans_centre within (K + 1) 2^-24 mean_k |c| of the float64 mean;
  4  the loop: fp8_iters = 0 is svg_kmeans_loop_grouped_strided bit for bit; fp8_iters = n - 1 of n is, bit for bit, the e4m3 loop of n - 1
     iterations followed by one 16-bit iteration from its centroids — a last iteration that converges and a NaN row included;
  5  quality: the inertia of the mixed loop against the 16-bit loop stays within the spread other initial points give the 16-bit loop;
  6  the Wan SAP layer-call with kmeans_e4m3 on: a valid plan, a finite output, an error against the float64 dense rows that moves by no
     more than other initial points move it; with the default the output of before.

Every output is checked for the poison pattern (tests/poisoned.py) before it is compared: these are the poison rows of the wrappers
kmeans_centre, kmeans_assign_e4m3 and kmeans_loop_e4m3."""
import pytest
import torch

import kmeans_e4m3_cases as EC
import kmeans_exact_cases as KC
import sparse_lse_cases as SC
from poisoned import assert_fully_written
from test_gpu_processors import _clustered

pytestmark = pytest.mark.gpu

D = EC.D
IDS = [str(dt).replace("torch.", "") for dt in KC.DTYPES]


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def dev(t):
    return t.cuda().contiguous()


def written(what, **outs):
    for name, t in outs.items():
        assert_fully_written(t, f"{what}: {name}")


def assign(nat, x, c, mu, what):
    labels = nat.kmeans_assign_e4m3(dev(x), dev(c), None if mu is None else dev(mu))
    written(what, labels=labels)
    assert labels.dtype == torch.int32 and labels.shape == x.shape[:2]
    return labels.cpu().long()


def assert_labels_equal(lab, ref, what):
    bad = lab != ref
    if bad.any():
        b, n = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} labels differ from the float64 arg-min (first index on ties); first "
                             f"[{b}, {n}]: got {int(lab[b, n])}, exact {int(ref[b, n])}")


def same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    return torch.equal(KC.bits16(a), KC.bits16(b)) if a.dtype in KC.DTYPES else torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------
# 1. exact inputs
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KC.DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K", KC.ASSIGN_SHAPES)
def test_assign_exact(nat, N, K, dtype):
    x, c = KC.assign_case(N, K, D, dtype)
    ref = KC.assign_ref64(x, c)
    what = f"kmeans_assign_e4m3 N={N} K={K}"
    assert_labels_equal(assign(nat, x, c, None, what), ref, what)
    xo, co, mu = EC.with_offset(x, c)
    assert_labels_equal(assign(nat, xo, co, mu, what + " offset"), ref, what + f", offset {EC.OFFSET} as mu")


@pytest.mark.parametrize("dtype", KC.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", sorted(KC.TIE_SETS))
def test_assign_planted_ties(nat, name, dtype):
    x, c = KC.tie_case(name, D, dtype)
    ref = KC.assign_ref64(x, c)
    xo, co, mu = EC.with_offset(x, c)
    for what, lab in ((f"kmeans_assign_e4m3, copies at {KC.TIE_SETS[name]} ({name})", assign(nat, x, c, None, name)),
                      (f"the same with offset {EC.OFFSET} as mu", assign(nat, xo, co, mu, name))):
        got = lab[:, list(KC.TIE_POINTS)]
        assert (got == min(KC.TIE_SETS[name])).all(), f"{what}: the tied points got {got.tolist()}"
        assert (lab[:, KC.ZERO_POINT] == KC.ZERO_CENTROID).all()
        assert_labels_equal(lab, ref, what)


# ---------------------------------------------------------------------------------------------------------
# 2. real-valued inputs, 3. the centre
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KC.DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", KC.REAL_KINDS)
def test_assign_real_valued_margin(nat, kind, dtype):
    """Rule C's eps models fp32 round-to-nearest partial sums, and the centre is part of the definition.  (Measured once WITHOUT a centre,
    "outlier_channels", bf16 — eight channels carry the score, the products of the others are 2^-9 of theirs: one label of 3000 lay outside the
    rule, margin 0.27 against eps 0.19, which fp32 partial sums cannot produce; DESIGN §3.3.  Around the centre: no label off the statement.)"""
    x, c = KC.real_case(kind, D, dtype)
    mu = nat.kmeans_centre(dev(c))
    written("kmeans_centre", mu=mu)
    mu = mu.cpu()
    what = f"kmeans_assign_e4m3 {kind}"
    EC.check_labels_margin(assign(nat, x, c, mu, what), x, c, mu, what + " around svg_kmeans_centre's mu")


@pytest.mark.parametrize("dtype", KC.DTYPES, ids=IDS)
@pytest.mark.parametrize("K", [1, 15, 16, 17, 129, 1000])
def test_centre(nat, K, dtype):
    g = torch.Generator().manual_seed(50 + K)
    c = (torch.randn(3, K, D, generator=g) * 2 + torch.arange(D) % 16 * 3.0).to(dtype)
    mu = nat.kmeans_centre(dev(c))
    written(f"kmeans_centre K={K}", mu=mu)
    assert mu.dtype == torch.float32 and mu.shape == (3, D)
    err, bound = (mu.cpu().double() - EC.centre64(c)).abs(), EC.centre_bound(c)
    print(f"kmeans_centre K={K}: max error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------------------------------------
# 4. the loop
# ---------------------------------------------------------------------------------------------------------
def strided(x):
    big = torch.full((x.shape[0], x.shape[1] + 40, x.shape[2]), 3.0, dtype=x.dtype)
    big[:, :x.shape[1]] = x
    view = big.cuda()[:, :x.shape[1]]
    assert not view.is_contiguous()
    return view


def loop_written(what, out):
    written(what, labels=out[0], centroids=out[1], counts=out[2], n_iters=out[3], sorted_idx=out[4])
    return out


@pytest.mark.parametrize("dtype", KC.DTYPES, ids=IDS)
@pytest.mark.parametrize("N,K", KC.ROUTE_SHAPES)
def test_loop_without_e4m3_iterations_is_the_16_bit_loop(nat, N, K, dtype):
    """B = 4, group = 2, batches further apart than N * D: all five results of svg_kmeans_loop_grouped_strided, bit for bit"""
    xs, cs = zip(*(KC.assign_case(N, K, D, dtype, seed=s) for s in (0, 1)))
    x, c0 = strided(torch.cat(xs)), dev(torch.cat(cs))
    for iters in (1, 3):
        want = loop_written("kmeans_loop", nat.kmeans_loop(x, None, c0, iters, 1e-4, group=2))
        got = loop_written("kmeans_loop_e4m3(fp8_iters=0)", nat.kmeans_loop_e4m3(x, c0, iters, 1e-4, 0, group=2))
        assert all(same_bits(a, b) for a, b in zip(got, want)), f"max_iters {iters}"


def compose(nat, x, c0, n, tol, group, what):
    """the mixed loop of n iterations against the e4m3 loop of n - 1 followed by one 16-bit iteration from its centroids"""
    G = 1 if group is None else x.shape[0] // group
    mixed = loop_written(what + " mixed", nat.kmeans_loop_e4m3(x, c0, n, tol, n - 1, group=group))
    first = loop_written(what + " e4m3 part", nat.kmeans_loop_e4m3(x, c0, n - 1, tol, n - 1, group=group))
    assert first[3].cpu().flatten().tolist() == [n - 1] * G          # an e4m3 iteration never stops a group
    last = loop_written(what + " 16-bit part", nat.kmeans_loop(x, None, first[1], 1, tol, group=group))
    assert mixed[3].cpu().flatten().tolist() == [n] * G and last[3].cpu().flatten().tolist() == [1] * G
    for name, a, b in zip(("labels", "centroids", "counts", "sorted_idx"), (mixed[0], mixed[1], mixed[2], mixed[4]),
                          (last[0], last[1], last[2], last[4])):
        assert same_bits(a, b), f"{what}: {name} of the mixed loop differ from the composition"
    lab16 = nat.kmeans_assign(x.contiguous(), first[1])
    written(what, labels16=lab16)
    assert torch.equal(mixed[0], lab16), f"{what}: the final labels are not the 16-bit arg-max against the centroids of the last iteration"
    return mixed, first, last


@pytest.mark.parametrize("dtype", KC.DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [2, 3, 5])
def test_mixed_loop_is_the_composition(nat, n, dtype):
    x, c0 = KC.real_case("blobs", D, dtype)
    xd, c0d = (strided(x), dev(c0)) if n != 3 else (dev(x), dev(c0))
    group = {2: None, 3: 1, 5: 2}[n]
    mixed, first, last = compose(nat, xd, c0d, n, 0.0, group, f"n={n}")       # tol 0: never converges, the last update is returned
    # the e4m3 iterations are not the 16-bit ones: the path differs, the labels stay a 16-bit arg-max
    plain = nat.kmeans_loop(xd, None, c0d, n, 0.0, group=group)
    print(f"n={n}: labels equal to the all-16-bit loop's {float((plain[0] == mixed[0]).double().mean()):.4f}")
    # a last iteration that converges returns the centroids it started from: those of the e4m3 part
    mixed, first, last = compose(nat, xd, c0d, n, 1e9, group, f"n={n}, converging")
    assert same_bits(mixed[1], first[1])


@pytest.mark.parametrize("pattern", sorted(KC.NAN_PATTERNS))
def test_mixed_loop_with_a_nan_row(nat, pattern):
    """a NaN row of batch 1: its centroid and its shift are NaN from the first update on; the composition holds bit for bit — with tol 1e9
    batch 0's group converges in the last iteration and returns the centroids of the e4m3 part, batch 1's NaN shift never does"""
    x, c0 = KC.nan_case(pattern)
    xd, c0d = dev(x), dev(c0)
    compose(nat, xd, c0d, 3, KC.NAN_TOL, 1, f"nan row {pattern}")
    mixed, first, _ = compose(nat, xd, c0d, 3, 1e9, 1, f"nan row {pattern}, converging")
    assert same_bits(mixed[1][0], first[1][0]) and torch.isnan(mixed[1][1].float()).any()


# ---------------------------------------------------------------------------------------------------------
# 5. quality
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KC.REAL_KINDS)
def test_mixed_loop_inertia_stays_within_the_spread_of_initial_points(nat, kind):
    x, _ = KC.real_case(kind, D, torch.bfloat16)
    xd, n = dev(x), EC.QUALITY_ITERS

    def inertia(draw, f8):
        c0 = dev(EC.initial_points(x, KC.REAL_K, draw))
        out = loop_written(f"draw {draw} fp8_iters {f8}", nat.kmeans_loop_e4m3(xd, c0, n, 0.0, f8) if f8 else nat.kmeans_loop(xd, None, c0, n, 0.0))
        assert int(out[3]) == n
        return float(EC.inertia64(x, out[1].cpu(), out[0].cpu()).sum())

    base = inertia(0, 0)
    ratio = inertia(0, n - 1) / base
    others = [inertia(d, 0) / base for d in range(1, EC.QUALITY_DRAWS + 1)]
    spread = max(others) - min(others)
    print(f"{kind}: mixed / 16-bit inertia {ratio:.4f} (|1 - ratio| = {abs(ratio - 1):.4f}); 16-bit loop over five other draws "
          f"{min(others):.4f} .. {max(others):.4f} (spread {spread:.4f})")
    assert abs(ratio - 1) <= spread


# ---------------------------------------------------------------------------------------------------------
# 6. the layer-call
# ---------------------------------------------------------------------------------------------------------
def test_wan_sap_layer_call(nat, monkeypatch):
    from svg.models import _core
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor as SapP

    H, F_, P_, QC, KC_ = 3, 6, 150, 4, 12
    S = F_ * P_
    for name, val in dict(context_length=0, num_frame=F_, frame_size=P_, first_layers_fp=0, first_times_fp=900.0, num_q_centroids=QC,
                          num_k_centroids=KC_, top_p_kmeans=0.6, min_kc_ratio=0.1, kmeans_iter_init=3, kmeans_iter_step=2,
                          zero_step_kmeans_init=False, logging_file=None, quality_log=None, quality_rows=64).items():
        monkeypatch.setattr(SapP, name, val, raising=False)
    gen = torch.Generator().manual_seed(3)
    q = _clustered(H, S, D, 12, gen)[None].to(torch.bfloat16).cuda()
    k = _clustered(H, S, D, 20, gen)[None].to(torch.bfloat16).cuda()
    v = torch.randn(1, H, S, D, generator=gen).to(torch.bfloat16).cuda()
    t = torch.tensor([100.0])
    rows = torch.randperm(S, generator=gen)[:64]
    o_d, _ = SC.masked_attention_lse(q.cpu()[:, :, rows], k.cpu(), v.cpu(), None)
    plans = []
    orig = _core.kmeans_clustering
    monkeypatch.setattr(_core, "kmeans_clustering", lambda *a, **kw: (plans.append((kw, orig(*a, **kw))), plans[-1][1])[1])

    def two_calls(seed):
        """the init call and a warm-started call of one layer -> their outputs and the relative L2 error of the second on the sampled rows"""
        torch.manual_seed(seed)
        proc = SapP(5)
        with torch.no_grad():
            a = proc.attention_core_logic(q, k, v, t)
            b = proc.attention_core_logic(q, k, v, t)
        written(f"seed {seed}", first=a, second=b)
        rel = float((b.cpu().double()[:, :, rows] - o_d).norm() / o_d.norm())
        return a, b, rel

    seeds = (11, 12, 13, 14, 15)
    off = [two_calls(s) for s in seeds]
    assert all(not kw.get("e4m3") for kw, _ in plans)
    # a processor that never heard of the option: the layer-call's body without the argument
    torch.manual_seed(seeds[0])
    store = _core.CentroidStore()
    with torch.no_grad():
        plain = [_core.svg2_sparse_attention(q, k, v, SapP(5).geometry(), store, 5, QC, KC_, 0.6, 0.1, 3, 2) for _ in range(2)]
    assert torch.equal(plain[0], off[0][0]) and torch.equal(plain[1], off[0][1])
    plans.clear()
    monkeypatch.setattr(SapP, "kmeans_e4m3", True)
    a, b, rel_on = two_calls(seeds[0])
    assert [kw.get("e4m3") for kw, _ in plans] == [True, True]
    for _, sides in plans:
        for (lab, cent, sizes, _, sidx), K in zip(sides, (QC, KC_)):
            written("plan", labels=lab, centroids=cent, sizes=sizes, sorted_idx=sidx)
            assert sizes.shape == (H, K) and (sizes.sum(-1) == S).all()
            assert torch.equal(sidx.long().sort(-1).values.cpu(), torch.arange(S).expand(H, S))
            assert torch.equal(torch.gather(lab, 1, sidx.long()).sort(-1).values, torch.gather(lab, 1, sidx.long()))   # sorted by cluster
    assert torch.isfinite(a.float()).all() and torch.isfinite(b.float()).all()
    rels = [r for _, _, r in off]
    print(f"rel. L2 against the float64 dense rows: kmeans_e4m3 on {rel_on:.4f}, off {rels[0]:.4f}; off over five seeds "
          f"{min(rels):.4f} .. {max(rels):.4f}")
    assert abs(rel_on - rels[0]) <= max(rels) - min(rels)
