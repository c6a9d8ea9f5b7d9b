"""What the tests of the flash-kmeans kernels share (tests/test_kmeans_exact_cases_cpu.py, tests/test_gpu_kmeans_exact.py): case generators,
float64 references and the rules that replace a chosen tolerance.  Plain module, torch on CPU, no library.

  * EXACT inputs (A: assignment, B: update).  x and centroids are integers in [-3, 3].  Then every product and every partial sum of both
    kernels is an integer or a multiple of 0.5 far below 2^24 (|x.c| <= 9 D < 2^11, csq <= 9 D, the accumulator start -csq / 2 a
    multiple of 0.5, a cluster sum <= 3 * 839), hence exactly representable in fp32 in ANY summation order: the float64 statement fixes
    labels and centroid sums bit for bit.  Labels: torch.equal, no share of rows left out, ties to the lowest index.  Centroids: the
    bits of rne16(fp32(sum) / fp32(count)), either neighbour where +-2 fp32 ulps on the quotient (the library is built with
    -ffast-math: the division may be a reciprocal multiply) change the 16-bit rounding.
  * REAL-VALUED inputs (C, D).  The tolerance is derived from the arithmetic: a label must be the float64 arg-max of
    s_k = x.c_k - csq_k / 2 unless the row's top-two margin is at most eps = 2 (2 D + 2) 2^-24 max_k (sum_d |x_d c_kd| + csq_k / 2) — twice
    the worst-case fp32 accumulation error of ONE score (D + 1 additions of the dot product on top of the start value, D - 1 of the csq
    sum, each relative 2^-24 of a partial sum bounded by the sum of magnitudes) —, and then one of the candidates within eps of the
    maximum.  A centroid element lies within ulp16(m) / 2 + (cnt + 1) 2^-24 mean_rows |x| of the float64 mean m: the output rounding plus
    the fp32 sum (cnt - 1 additions) and the division.
  * the NaN case of the stopping rule (E) and the mutants of the torch statement that the CPU module must see fail.

ref: batch_kmeans_Euclid / _euclid_assign_kernel / triton_centroid_update_sorted_euclid, svg/kmeans_utils.py:464-554, 375-421, 684-733;
csrc/kmeans.hip."""
import functools

import torch

from oracle import svg_oracle as O
from test_gpu_kernels import _blobs

DTYPES = [torch.bfloat16, torch.float16]
DIMS = [64, 128]
MANT = {torch.bfloat16: 7, torch.float16: 10}       # stored mantissa bits of the 16-bit types
MIN_EXP = {torch.bfloat16: -126, torch.float16: -14}
U32 = 2.0 ** -24                                    # unit roundoff of fp32
KBN = 64                                            # centroids per tile of kmeans_assign_kernel (kBN, csrc/attn_core.h)
WG_POINTS = 256                                     # points per workgroup of kmeans_assign_kernel (NW * 32)
NUM_CU = 256


def bits16(t):
    return t.contiguous().view(torch.int16)


def _ints(shape, gen, dtype):
    return torch.randint(-3, 4, shape, generator=gen).to(dtype)


# ---------------------------------------------------------------------------------------------------------
# A. assignment on exact inputs
# ---------------------------------------------------------------------------------------------------------
ASSIGN_B = 2
# every K at N = 257 (one point into the second workgroup); every N at K = 65 and K = 129 (one centroid into the second / third tile);
# more centroids than points
ASSIGN_SHAPES = sorted({(257, K) for K in (1, 2, 63, 64, 65, 128, 129, 200)}
                       | {(N, K) for K in (65, 129) for N in (1, 33, 255, 256, 257, 700)} | {(33, 200)})
ROUTE_SHAPES = [(257, 129), (700, 65)]              # the other routes to the same labels (kmeans_iter, the library loop, its strided form)


@functools.lru_cache(maxsize=None)
def assign_case(N, K, D, dtype, seed=0):
    """-> x [B, N, D], c [B, K, D]: integers in [-3, 3], different per batch"""
    g = torch.Generator().manual_seed(100003 * seed + 1009 * N + 17 * K + D)
    return _ints((ASSIGN_B, N, D), g, dtype), _ints((ASSIGN_B, K, D), g, dtype)


def assign_ref64(x, c):
    """labels int64 [B, N] = argmin_k sum_d (x - c_k)^2 in float64, first index on ties (torch.argmin returns the first minimal index)"""
    xd, cd = x.double(), c.double()
    out = torch.empty(x.shape[:2], dtype=torch.int64)
    for n0 in range(0, x.shape[1], 128):
        d = ((xd[:, n0:n0 + 128, None, :] - cd[:, None, :, :]) ** 2).sum(-1)
        out[:, n0:n0 + 128] = d.argmin(-1)
    return out


def csq64(c):
    """|c_k|^2 as csq_kernel defines it — products rounded to the input type, then summed — with the sum in float64"""
    return (c * c).double().sum(-1)


def scores64(x, c):
    """s[b, n, k] = x.c_k - csq_k / 2 in float64: argmax_k s = argmin_k |x - c_k|^2 (|x|^2 is common to a row)"""
    return torch.einsum("bnd,bkd->bnk", x.double(), c.double()) - 0.5 * csq64(c)[:, None, :]


def scores32(x, c, csq=None):
    """the fp32 torch statement of kmeans_assign_kernel: fp32 dot products on top of the start value -csq / 2, csq an fp32 sum of rounded
    products.  `csq` overrides the norms (mutant 4)."""
    csq = (c * c).float().sum(-1) if csq is None else csq
    return torch.einsum("bnd,bkd->bnk", x.float(), c.float()) - 0.5 * csq[:, None, :]


def exact_tie_share(s):
    """share of rows whose two largest scores are equal (two distinct indices tie for the label)"""
    if s.shape[-1] < 2:
        return 0.0
    top = s.topk(2, dim=-1).values
    return (top[..., 0] == top[..., 1]).double().mean().item()


def tile_coords(k):
    """where kmeans_assign_kernel keeps the score of centroid k: tile t = k // 64; inside the tile the index is 32 bb + 8 rq + 4 g + j — bb the
    MFMA block of 32 centroids, (rq, j) the accumulator register 4 rq + j, g the half-wave (the lane of a point that holds it) — and the
    arg-max epilogue runs four chains of eight registers per lane: chain 2 bb + rq // 2."""
    t, r = divmod(k, KBN)
    return dict(tile=t, bb=r // 32, rq=(r % 32) // 8, g=(r % 8) // 4, j=r % 4, chain=2 * (r // 32) + ((r % 32) // 8) // 2)


# "lowest index wins" is promised at four levels (inside a chain, across the chains of a lane, across tiles, across the two lanes of a
# point); the copies of one centroid are placed so that each pair meets at one seam.  Derived from tile_coords (asserted in the CPU
# module): 9 and 10 are registers 5 and 6 of chain 0 of lane g = 0; 25 is chain 1 of the same lane; 41 is bb = 1 (chain 2); 73 = 64 + 9 is
# the next tile; 13 sits in the g = 1 lane and 16 in the g = 0 lane, so the lowest copy reaches the label only through the cross-lane
# merge (`ob == best && oi < best_idx`); 128 is the only centroid of the last, ragged tile at K = 129.
TIE_SETS = {"same_chain": (9, 10), "other_chain": (9, 25), "other_half": (9, 41), "next_tile": (9, 73), "cross_lane": (13, 16),
            "ragged_tile": (70, 128)}
TIE_N, TIE_K = 257, 129
TIE_POINTS = (0, 1, 31, 32, 63, 64, 130, 255, 256)   # nine points: both ends of a wave's 32, several waves, both workgroups
ZERO_POINT, ZERO_CENTROID = 7, 5                    # c[:, 5] = x[:, 7]: distance exactly 0


@functools.lru_cache(maxsize=None)
def tie_case(name, D, dtype):
    """assign_case(257, 129) with one centroid value copied to the indices TIE_SETS[name] and TIE_POINTS bit-equal to it (their label
    must be the lowest copy), and a data point copied into a centroid"""
    x, c = (t.clone() for t in assign_case(TIE_N, TIE_K, D, dtype, seed=1 + sorted(TIE_SETS).index(name)))
    g = torch.Generator().manual_seed(4242 + D + sorted(TIE_SETS).index(name))
    v = _ints((ASSIGN_B, D), g, dtype)
    x[:, list(TIE_POINTS)] = v[:, None]
    for k in TIE_SETS[name]:
        c[:, k] = v
    c[:, ZERO_CENTROID] = x[:, ZERO_POINT]
    return x, c


# ---------------------------------------------------------------------------------------------------------
# B. update on exact inputs
# ---------------------------------------------------------------------------------------------------------
def slots(D):
    """row slots of kmeans_update_kernel: 256 threads / (D / 8) lanes per row"""
    return 256 // (D // 8)


def update_sizes(S):
    """cluster sizes around every branch of kmeans_update_kernel for S row slots: a slot has at most three rows up to 3S ("at most three
    rows" branch, rows prefetched), the first slot has four from 3S + 1 (the prefetched batch of four; other slots follow up to 4S), one-row
    tails from 4S + 1, the steady four-row loop from 7S + 1 (25S + 7: the first batch, five passes of the steady loop and a tail of two rows in
    slots 0 - 6, of one row in the others)"""
    return [0, 1, S - 1, S, S + 1, 3 * S - 1, 3 * S, 3 * S + 1, 4 * S - 1, 4 * S, 4 * S + 1, 7 * S - 1, 7 * S, 7 * S + 1, 8 * S - 1, 8 * S,
            8 * S + 1, 25 * S + 7]


# B = 4, K = 500: min(K, ceil(3 * 256 CUs / B)) = 192 workgroups per batch, each walks clusters k, k + 192, k + 384 — every transition between
# the branches, empty clusters mid-walk, the prefetch `pre[]` carried from one cluster to the next.  B = 1, K = 40: one cluster per workgroup.
UPDATE_CONFIGS = [(4, 500), (1, 40)]


def update_groups(B, K):
    return max(1, min(K, (3 * NUM_CU + B - 1) // B))


@functools.lru_cache(maxsize=None)
def update_layout(B, K, D):
    """-> sizes int64 [B, K]: cluster k of batch b has update_sizes[(7 k + b) % 18] rows.  N is batch 0's total (42 017 at D = 128, 83 809
    at D = 64 for K = 500); the totals of the other batches differ by a few hundred rows (K is no multiple of 18), which the FIRST cluster of
    25S + 7 rows of that batch takes or gives (it stays above 11S: the same path)."""
    S = slots(D)
    sz = update_sizes(S)
    per = torch.tensor([[sz[(7 * k + b) % 18] for k in range(K)] for b in range(B)], dtype=torch.int64)
    N = int(per[0].sum())
    for b in range(1, B):
        a = int((per[b] == sz[17]).nonzero()[0])
        per[b, a] += N - int(per[b].sum())
    return per


@functools.lru_cache(maxsize=None)
def update_case(B, K, D, dtype):
    """-> x [B, N, D] and c_old [B, K, D] integers in [-3, 3], labels int32 [B, N] in shuffled row order, sizes int64 [B, K]"""
    per = update_layout(B, K, D)
    N = int(per[0].sum())
    g = torch.Generator().manual_seed(31 * K + D)
    labels = torch.stack([torch.repeat_interleave(torch.arange(K), per[b])[torch.randperm(N, generator=g)] for b in range(B)])
    return _ints((B, N, D), g, dtype), labels.to(torch.int32), _ints((B, K, D), g, dtype), per


def cluster_sums64(x, labels, K, absolute=False):
    """float64 sums [B, K, D] of the rows of every cluster (of their magnitudes with `absolute`), counts int64 [B, K]"""
    B, N, D = x.shape
    lab = labels.long()
    xd = x.double().abs() if absolute else x.double()
    sums = torch.zeros(B, K, D, dtype=torch.float64).scatter_add_(1, lab[..., None].expand(-1, -1, D), xd)
    counts = torch.zeros(B, K, dtype=torch.int64).scatter_add_(1, lab, torch.ones_like(lab))
    return sums, counts


def cluster_sums32(x, labels, K):
    """the fp32 torch statement of the update's sums (scatter order, not the kernel's: on exact inputs the order cannot matter)"""
    B, N, D = x.shape
    return torch.zeros(B, K, D, dtype=torch.float32).scatter_add_(1, labels.long()[..., None].expand(-1, -1, D), x.float())


def _magnitude_step(q, n):
    """fp32 q moved by n ulps in magnitude (0 stays 0)"""
    return torch.where(q != 0, (q.view(torch.int32) + n).view(torch.float32), q)


def centroids_from_sums(sums, counts, c_old):
    """-> (lo, hi): the 16-bit roundings (RNE) of fp32(sum) / fp32(count) moved by -2 and +2 fp32 ulps.  They are equal — the one accepted bit
    pattern — unless the quotient lies within 2 ulps of a rounding boundary of the 16-bit type; then they are its two neighbours, and the
    correctly rounded quotient gives one of them.  Empty clusters: the bits of c_old."""
    q = sums.float() / counts.clamp(min=1).float()[..., None]
    empty = (counts == 0)[..., None]
    lo = torch.where(empty, c_old, _magnitude_step(q, -2).to(c_old.dtype))
    hi = torch.where(empty, c_old, _magnitude_step(q, 2).to(c_old.dtype))
    return lo, hi


@functools.lru_cache(maxsize=None)
def update_reference(B, K, D, dtype):
    """-> (lo, hi, counts int32): update_case's accepted centroid bits and its exact counts"""
    x, labels, c_old, per = update_case(B, K, D, dtype)
    sums, counts = cluster_sums64(x, labels, K)
    assert torch.equal(counts, per)
    return centroids_from_sums(sums, counts, c_old) + (counts.to(torch.int32),)


def ambiguous_share(lo, hi):
    return (bits16(lo) != bits16(hi)).double().mean().item()


AMBIGUOUS_CAP = 1e-3      # a condition of the exact-centroid rule, not a measurement: at most 0.1 % of the elements may have two accepted patterns


def check_centroids_exact(got, lo, hi, what=""):
    """every element of `got` carries the bits of lo or of hi"""
    got = got.cpu()
    share = ambiguous_share(lo, hi)
    bad = (bits16(got) != bits16(lo)) & (bits16(got) != bits16(hi))
    print(f"{what}: ambiguous-rounding share {share:.2e}, elements off the exact rule {int(bad.sum())} of {bad.numel()}")
    assert share <= AMBIGUOUS_CAP, f"{what}: {share:.2e} of the elements have two accepted roundings"
    if bad.any():
        b, k, d = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} centroid elements differ from the exact mean, first [{b}, {k}, {d}]: "
                             f"got {got[b, k, d].item()!r}, exact {lo[b, k, d].item()!r} / {hi[b, k, d].item()!r}")


def shift_ref64(c_new, c_old):
    """float64 [B]: max_k sqrt(sum_d rne16(c_new - c_old)^2) from the centroids the update itself returned (the difference of two 16-bit
    values in fp32, rounded to the type, as kmeans_update_kernel forms it)"""
    df = (c_new.cpu().float() - c_old.float()).to(c_old.dtype).double()
    return (df * df).sum(-1).sqrt().max(dim=-1).values


def check_shift(shift, c_new, c_old, what=""):
    """relative D 2^-24: the squares are exact in fp32 (16-bit factors), a sum of D non-negative terms errs by at most (D - 1) u, the square
    root halves that and adds a few ulps.  A reference of exactly 0 (nothing moved) must come back as exactly 0."""
    ref = shift_ref64(c_new, c_old)
    got = shift.double().cpu()
    D = c_old.shape[-1]
    err = (got - ref).abs()
    print(f"{what}: shift {got.tolist()} reference {ref.tolist()} (relative bound {D * U32:.2e})")
    assert torch.isfinite(got).all() and (err <= D * U32 * ref).all(), (what, got.tolist(), ref.tolist())


def check_sort(counts, sorted_idx, labels, K, what=""):
    lab = labels.cpu().long()
    ref_counts = torch.zeros(lab.shape[0], K, dtype=torch.int64).scatter_add_(1, lab, torch.ones_like(lab)).to(torch.int32)
    assert torch.equal(counts.cpu(), ref_counts), f"{what}: counts"
    assert torch.equal(sorted_idx.cpu(), O.stable_argsort(lab).to(torch.int32)), f"{what}: sorted indices"


# ---------------------------------------------------------------------------------------------------------
# C / D. real-valued data: the derived margin and the centroid bound
# ---------------------------------------------------------------------------------------------------------
REAL_B, REAL_N, REAL_K = 2, 1500, 129
REAL_KINDS = ["blobs", "outlier_channels"]
OUTLIER_OFFSET = 20.0     # added to every 16th channel: the outlier channels of real hidden states
NEAR_TIE_CAP = 0.05       # a condition of rule C: at most 5 % of a case's rows may lie inside eps


@functools.lru_cache(maxsize=None)
def real_case(kind, D, dtype):
    """-> x [2, 1500, D], c (a) [2, 129, D]: 129 data points as centroids"""
    x, _ = _blobs(REAL_B, REAL_N, REAL_K, D, 0.5, seed=33 + D, dtype=torch.float32)
    if kind == "outlier_channels":
        x[..., ::16] += OUTLIER_OFFSET
    x = x.to(dtype)
    return x, x[:, 100:100 + REAL_K].clone()


def margin_reference(x, c):
    """-> s float64 [B, N, K] and eps float64 [B, N] = 2 (2 D + 2) 2^-24 max_k (sum_d |x_d c_kd| + csq_k / 2)"""
    D = x.shape[-1]
    s = scores64(x, c)
    mag = torch.einsum("bnd,bkd->bnk", x.double().abs(), c.double().abs()) + 0.5 * csq64(c)[:, None, :]
    return s, 2 * (2 * D + 2) * U32 * mag.max(dim=-1).values


def near_tie_share(x, c, scale=1.0):
    s, eps = margin_reference(x, c)
    top = s.topk(2, dim=-1).values
    return ((top[..., 0] - top[..., 1]) <= scale * eps).double().mean().item()


def check_labels_margin(labels, x, c, what=""):
    """rule C: the float64 arg-max, except on rows whose float64 top-two margin is at most eps: there one of the candidates within eps of
    the maximum.  At most NEAR_TIE_CAP of the rows may be such rows.  -> (share inside eps, labels that differ from the arg-max)"""
    lab = labels.cpu().long()
    s, eps = margin_reference(x, c)
    assert lab.shape == s.shape[:2] and int(lab.min()) >= 0 and int(lab.max()) < s.shape[-1], f"{what}: labels out of range"
    top = s.topk(2, dim=-1).values
    inside = (top[..., 0] - top[..., 1]) <= eps
    ref = s.argmax(-1)
    got = torch.gather(s, 2, lab[..., None])[..., 0]
    wrong_clear = ~inside & (lab != ref)
    wrong_near = inside & (got < top[..., 0] - eps)
    share, differ = inside.double().mean().item(), int((lab != ref).sum())
    print(f"{what}: near-tie share {share:.4f} (cap {NEAR_TIE_CAP}), labels off the float64 arg-max {differ} of {lab.numel()}, "
          f"outside rule C {int(wrong_clear.sum()) + int(wrong_near.sum())}")
    assert share <= NEAR_TIE_CAP, f"{what}: {share:.4f} of the rows lie inside eps"
    if wrong_clear.any() or wrong_near.any():
        b, n = (wrong_clear | wrong_near).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(wrong_clear.sum())} labels differ from the float64 arg-max on rows with a margin above eps and "
                             f"{int(wrong_near.sum())} near-tie rows carry a label further than eps from the maximum; first [{b}, {n}]: label "
                             f"{int(lab[b, n])} (score {got[b, n].item():.9g}), arg-max {int(ref[b, n])} ({top[b, n, 0].item():.9g}), second "
                             f"{top[b, n, 1].item():.9g}, eps {eps[b, n].item():.3g}")
    return share, differ


def ulp16(v, dtype):
    """the spacing of the 16-bit type at |v| (float64 in and out); subnormal spacing below the smallest normal"""
    e = torch.frexp(v.abs().clamp(min=2.0 ** MIN_EXP[dtype]))[1] - 1
    return torch.ldexp(torch.ones_like(v), e - MANT[dtype])


def centroid_bound(x, labels, K):
    """-> float64 mean m [B, K, D], bound [B, K, D] = ulp16(m) / 2 + (cnt + 1) 2^-24 mean_rows |x|, counts [B, K]"""
    sums, counts = cluster_sums64(x, labels, K)
    mags, _ = cluster_sums64(x, labels, K, absolute=True)
    n = counts.clamp(min=1).double()[..., None]
    m = sums / n
    return m, 0.5 * ulp16(m, x.dtype) + (n + 1) * U32 * (mags / n), counts


def check_centroids_bound(got, x, labels, c_old, what=""):
    """non-empty clusters inside the bound around the float64 mean; empty clusters the bits of c_old"""
    got = got.cpu()
    m, bound, counts = centroid_bound(x, labels.cpu(), c_old.shape[1])
    empty = (counts == 0)[..., None].expand_as(m)
    err = (got.double() - m).abs()
    ratio = torch.where(empty, torch.zeros_like(err), err / bound)
    print(f"{what}: max |c - mean| / bound {ratio.max().item():.3f}, bound at most {bound[~empty].max().item():.3e}, empty clusters "
          f"{int((counts == 0).sum())}")
    assert torch.equal(bits16(got)[empty], bits16(c_old)[empty]), f"{what}: an empty cluster must keep the bits of its old centroid"
    assert torch.isfinite(got.float()[~empty]).all() and (ratio <= 1).all(), f"{what}: max |c - mean| / bound = {ratio.max().item():.3f}"


# ---------------------------------------------------------------------------------------------------------
# E. a NaN shift never converges
# ---------------------------------------------------------------------------------------------------------
NAN_SHAPE = dict(B=2, N=600, K=8, D=128)
NAN_TOL, NAN_MAX_ITERS = 1e-4, 8
NAN_ROW = 123                                     # the row of batch 1 that gets a NaN in every channel
NAN_PATTERNS = {"sign_clear": 0x7FC0, "sign_set": 0xFFC0}


@functools.lru_cache(maxsize=None)
def nan_case(pattern=None):
    """well-separated bf16 blobs that converge in fewer than NAN_MAX_ITERS iterations -> (x, c0); with `pattern` every channel of row
    NAN_ROW of batch 1 holds that bit pattern (written through an int16 view)"""
    s = NAN_SHAPE
    x, centers = _blobs(s["B"], s["N"], s["K"], s["D"], 0.3, seed=5)
    c0 = (centers.float() + 0.2 * torch.randn(s["B"], s["K"], s["D"], generator=torch.Generator().manual_seed(6))).to(torch.bfloat16)
    if pattern is not None:
        x = x.clone()
        bits = NAN_PATTERNS[pattern]
        x.view(torch.int16)[1, NAN_ROW, :] = bits - 65536 if bits >= 32768 else bits
        assert torch.isnan(x[1, NAN_ROW]).all() and int(torch.isnan(x).sum()) == s["D"]
    return x, c0
