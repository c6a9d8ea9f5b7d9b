"""The cosine and dot-product k-means on the GPU (include/svg_attn_kmeans_metric.h) against the float64 statement of its arithmetic:
the bias-free assignment on exact integers, the weighted, normalising update against fp64 within a derived bound, and the device loop
(planted directions, manual composition, strided view, groups, power-of-two row scales) bit for bit."""
import pytest
import torch

import poisoned

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
MANT = {torch.bfloat16: 7, torch.float16: 10}


@pytest.fixture(scope="module")
def nat():
    return poisoned.load_native()


def spacing(ref, dtype, floor=2.0 ** -6):
    return 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(floor))) - MANT[dtype])


def update64(x, lab, c_old, metric):
    """the update of the header in float64, m rounded to the dtype where the kernel rounds it -> (unit centroids, counts)"""
    B, N, D = x.shape
    K = c_old.shape[1]
    xd = x.double()
    if metric == "cosine":
        xd = xd / xd.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    s = torch.zeros(B, K, D, dtype=torch.float64).scatter_add_(1, lab.long()[..., None].expand(-1, -1, D), xd)
    cnt = torch.zeros(B, K, dtype=torch.int64).scatter_add_(1, lab.long(), torch.ones(B, N, dtype=torch.int64))
    m = torch.where(cnt[..., None] > 0, s / cnt.clamp_min(1)[..., None], c_old.double()).to(x.dtype).double()
    return m / m.norm(dim=-1, keepdim=True).clamp_min(1e-12), cnt


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("N,K", [(1, 1), (255, 63), (257, 65), (513, 130)])
def test_assignment_is_the_exact_argmax(nat, N, K, D, dtype):
    """integers in [-3, 3]: every dot product is an exact fp32 integer, so the labels ARE the fp64 arg-max; duplicated centroid rows plant
    ties (lowest index wins), a zero row gets label 0"""
    g = torch.Generator().manual_seed(1000 * N + K + D)
    x = torch.randint(-3, 4, (2, N, D), generator=g).to(dtype)
    c = torch.randint(-3, 4, (2, K, D), generator=g).to(dtype)
    if K > 2:
        c[:, K - 1], c[:, K // 2] = c[:, 0], c[:, 1]
    x[:, N // 2] = 0
    ref = torch.einsum("bnd,bkd->bnk", x.double(), c.double()).argmax(-1)      # (the first index of the maximum)
    assert K <= 2 or not (ref == K - 1).any()                                  # the copy at K - 1 ties with row 0 and never wins
    for metric in ("cosine", "dot"):
        lab = nat.kmeans_assign_metric(x.cuda(), c.cuda(), metric).cpu()
        assert torch.equal(lab.long(), ref) and (lab[:, N // 2] == 0).all(), metric


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_update_against_float64(nat, metric, D, dtype):
    """N = 600, K = 7: cluster 0 empty, 1 a single row, 2 of 300 rows (the four-in-flight path at both head sizes), the rest small; one row
    scaled by 2^10 and one by 2^-10.  The fp64 statement rounds m where the kernel does; what differs is the accumulation order, which can
    flip that rounding: at most 2 spacings after the division (if a binade is crossed), one more for the final rounding -> 3 spacings of
    the dtype at max(|ref|, 2^-6)."""
    from svg.kmeans_metric import triton_centroid_update_cosine

    B, N, K = 2, 600, 7
    g = torch.Generator().manual_seed(D + (metric == "dot"))
    lab = torch.cat([torch.full((1,), 1), torch.full((300,), 2), torch.arange(299) % 4 + 3]).to(torch.int32)
    lab = torch.stack([lab[torch.randperm(N, generator=g)] for _ in range(B)])
    x = torch.randn(B, N, D, generator=g)
    for b in range(B):                                                         # two rows of the large cluster
        i, j = (lab[b] == 2).nonzero()[:2, 0].tolist()
        x[b, i] *= 2.0 ** 10
        x[b, j] *= 2.0 ** -10
    x, c_old = x.to(dtype), torch.randn(B, K, D, generator=g).to(dtype)
    cent, counts, srt, shift = (t.cpu() for t in nat.kmeans_update_metric(x.cuda(), lab.cuda(), c_old.cuda(), metric))
    ref, cnt = update64(x, lab, c_old, metric)
    assert torch.equal(counts.long(), cnt) and torch.equal(srt.long(), torch.argsort(lab.long(), dim=-1, stable=True))
    err = (cent.double() - ref).abs() / spacing(ref, dtype)
    print(f"{metric} D={D} {dtype}: worst error {err.max():.3f} spacings, empty cluster {err[:, 0].max():.3f}")
    assert err.max() <= 3                                                      # (cluster 0: the normalised old centroid)
    sref = (cent.double() - c_old.double()).norm(dim=-1).max(dim=1).values
    assert ((shift.double() - sref).abs() <= 2.0 ** -7 * sref).all()
    if metric == "dot":                                                        # the reference's name for the same entry
        assert torch.equal(triton_centroid_update_cosine(x.cuda(), lab.long().cuda(), c_old.cuda()).cpu(), cent)


def planted(dtype, N=700, K=5, D=128):
    """x [2, N, D]: rows s 8 e_(8 k) (s in 1..3, k the planted label) plus noise in {-1, 0, 1} on an eighth of the channels — every cosine
    gap exceeds 0.5 —; batch 1 carries no noise, so its first update returns the initial centroids e_(8 k): it converges at once"""
    g = torch.Generator().manual_seed(7)
    lab = torch.stack([torch.randperm(N, generator=g) % K for _ in range(2)])
    x = torch.zeros(2, N, D)
    x.scatter_(2, (8 * lab)[..., None], 8.0 * torch.randint(1, 4, (2, N, 1), generator=g))
    x[0] += torch.randint(-1, 2, (N, D), generator=g) * (torch.rand(N, D, generator=g) < 0.125)
    c0 = torch.zeros(2, K, D)
    c0[:, torch.arange(K), 8 * torch.arange(K)] = 1.0
    top = torch.einsum("bnd,bkd->bnk", torch.nn.functional.normalize(x.double(), dim=-1), c0.double()).topk(2).values
    assert (top[..., 0] - top[..., 1] > 0.5).all()
    return x.to(dtype).cuda(), c0.to(dtype).cuda(), lab


def same(a, b):
    return all(torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_loop_recovers_planted_directions_and_is_its_two_halves(nat, metric, dtype):
    from svg import kmeans_metric as KU

    x, c0, lab = planted(dtype)
    fn = KU.batch_kmeans_Cosine if metric == "cosine" else KU.batch_kmeans_Dot
    ids, cent, sizes, n_it, srt = fn(x, 5, max_iters=8, tol=1e-4, init_centroids=c0, return_sorted_indices=True)
    assert torch.equal(ids.cpu(), lab) and int(n_it) < 8
    assert torch.equal(sizes.cpu().long(), torch.stack([torch.bincount(l, minlength=5) for l in lab]))
    assert ((cent.double().norm(dim=-1) - 1).abs() <= 2 * 2.0 ** -MANT[dtype]).all()
    cur = c0            # the reference's loop on the two entries (e_(8 k) is its own normalisation, bit for bit)
    for it in range(8):
        l2 = nat.kmeans_assign_metric(x, cur, metric)
        new, cnt, s2, shift = nat.kmeans_update_metric(x, l2, cur, metric)
        if shift.max() < 1e-4:
            break
        cur = new
    assert same((ids.int(), cent, sizes, srt), (l2, cur, cnt, s2)) and int(n_it) == it + 1
    # the initial normalisation (cosine): a loop that stops in its first iteration returns the normalised c_init; one rounding of the
    # quotient by an fp32 norm: within one spacing of the fp64 quotient
    if metric != "cosine":
        return
    c3 = (3 * c0 + 0.25).to(dtype)
    out = KU.batch_kmeans_Cosine(x, 5, max_iters=1, tol=float("inf"), init_centroids=c3)[1].double().cpu()
    ref = torch.nn.functional.normalize(c3.double().cpu(), dim=-1)
    assert ((out - ref).abs() <= spacing(ref, dtype, 2.0 ** -20)).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("metric", ["cosine", "dot"])
def test_loop_views_groups_and_row_scales(nat, metric, dtype):
    x, c0, _ = planted(dtype)
    base = nat.kmeans_loop_metric(x, c0, 8, 1e-4, metric)
    q = torch.cat([x, torch.full_like(x[:, :37], 5.0)], dim=1)
    assert not q[:, :700].is_contiguous() and same(nat.kmeans_loop_metric(q[:, :700], c0, 8, 1e-4, metric), base)
    grouped = nat.kmeans_loop_metric(x, c0, 8, 1e-4, metric, group=1)
    assert grouped[3].tolist()[1] == 1 < grouped[3].tolist()[0]
    for b in range(2):
        alone = nat.kmeans_loop_metric(x[b:b + 1].contiguous(), c0[b:b + 1].contiguous(), 8, 1e-4, metric)
        assert same([t[b:b + 1] for t in grouped[:3] + grouped[4:]], alone[:3] + alone[4:])
        assert int(alone[3]) == grouped[3].tolist()[b]
    if metric == "cosine":      # the assignment is scale-free, and a power of two commutes with the weights
        p = torch.randint(-3, 4, (2, 700, 1), generator=torch.Generator().manual_seed(3)).cuda()
        assert same(nat.kmeans_loop_metric((x.float() * 2.0 ** p).to(dtype), c0, 8, 1e-4, metric), base)
