"""The float64 statement of the e4m3 k-means assignment (include/svg_attn_kmeans_e4m3.h; csrc/kmeans.hip kmeans_assign_e4m3_kernel and its
centroid pre-pass) and of the Lloyd loop that uses it for its first iterations, shared by tests/test_kmeans_e4m3_cpu.py and
tests/test_gpu_kmeans_e4m3.py.  Plain module, torch on CPU, no library; e4m3 itself is tests/fp8_exact_cases.py's table.

  * quantiser: a row r = t - mu (the difference in fp32, as the kernels take it), e = floor(log2(448 / max_d |r_d|)) from frexp — max =
    f 2^x with f in [0.5, 1), 448 = 0.875 * 2^9: e = 9 - x for f <= 0.875, else 8 - x —, 0 for a zero row, at most 127;
    q(r) = e4m3_rne(r 2^e) (r 2^e is exact: a power of two), the row stands for q(r) 2^-e.
  * score: s_k = sum_d q(x - mu)_d q(c_k - mu)_d 2^-(e_x + e_k) - csq'_k / 2 in float64, csq'_k the sum of squares of the UNquantised fp32
    row c_k - mu; label = the lowest index of the maximum.
  * rule C of tests/kmeans_exact_cases.py restated on the dequantised operands x8 = q(x - mu) 2^-e_x, c8 likewise: the kernel's score
    differs from the statement's only by fp32 accumulation, so a label must be the statement's arg-max unless the row's top-two margin is
    at most eps = 2 (2 D + 2) 2^-24 max_k (sum_d |x8_d c8_kd| + csq'_k / 2), and then a candidate within eps of the maximum; at most
    NEAR_TIE_CAP of a case's rows may lie inside eps (a condition of the rule).
  * the mixed loop: iterations it < fp8_iters assign with the score above around mu = the channel mean of the INITIAL centroids, the
    others with the 16-bit score of kmeans_exact_cases.scores64; every iteration updates to the 16-bit rounding of the float64 cluster
    means (empty clusters keep their centroid).  No stopping rule (the loops it is compared with run with tol = 0)."""
import torch

import fp8_exact_cases as F8
import kmeans_exact_cases as KC

D = 128                      # the only head_dim of the e4m3 kernels
U32 = KC.U32
NEAR_TIE_CAP = KC.NEAR_TIE_CAP
OFFSET = 40                  # planted integer offset of the exact cases: x + 40 and c + 40 are integers below 2^6, exact in bf16 and fp16


def centre64(c):
    """float64 [B, D]: the channel mean of the centroids c [B, K, D]"""
    return c.double().mean(dim=1)


def row_exponent(r32):
    """r32 float32 [..., D] -> e int64 [...]: the largest e with max_d |r_d| 2^e <= 448, 0 for a zero row, at most 127"""
    m = r32.abs().amax(dim=-1).double()
    f, x = torch.frexp(m)
    e = torch.where(f <= 0.875, 9, 8) - x.long()
    return torch.where(m > 0, e.clamp(max=127), torch.zeros_like(e))


def centred32(t, mu=None):
    """the fp32 rows t - mu (mu [B, D] of any float type, taken as fp32; None: zeros)"""
    r = t.float()
    return r if mu is None else r - mu.float()[:, None, :]


def quantise(t, mu=None, rounding="rne"):
    """-> (bytes uint8 [B, R, D], e int64 [B, R], r32): the e4m3 image of the rows of t around mu.  rounding = "truncate": the mutant that
    rounds towards zero."""
    r = centred32(t, mu)
    e = row_exponent(r)
    y = torch.ldexp(r.double(), e[..., None])
    if rounding == "rne":
        b = F8.e4m3_bytes(y)
    else:
        lo, _, _ = F8.e4m3_neighbours(y)
        b = (lo + 128 * torch.signbit(y).long()).to(torch.uint8)
    return b, e, r


def dequantise(b, e):
    return torch.ldexp(F8.e4m3_decode(b), -e[..., None])


def operands64(x, c, mu=None, rounding="rne"):
    """-> x8 [B, N, D], c8 [B, K, D] (dequantised, float64), csq' [B, K] (float64 sum of squares of the fp32 rows c - mu)"""
    xb, xe, _ = quantise(x, mu, rounding)
    cb, ce, cr = quantise(c, mu, rounding)
    return dequantise(xb, xe), dequantise(cb, ce), (cr.double() ** 2).sum(-1)


def scores64(x, c, mu=None, rounding="rne"):
    x8, c8, csq = operands64(x, c, mu, rounding)
    return torch.einsum("bnd,bkd->bnk", x8, c8) - 0.5 * csq[:, None, :]


def lowest_argmax(s):
    """the lowest index of the maximum of the last dimension"""
    K = s.shape[-1]
    idx = torch.arange(K).expand(s.shape)
    return torch.where(s == s.amax(dim=-1, keepdim=True), idx, torch.full_like(idx, K)).amin(dim=-1)


def assign64(x, c, mu=None, rounding="rne"):
    return lowest_argmax(scores64(x, c, mu, rounding))


def margin_reference(x, c, mu=None):
    """-> s float64 [B, N, K], eps float64 [B, N] = 2 (2 D + 2) 2^-24 max_k (sum_d |x8_d c8_kd| + csq'_k / 2)"""
    x8, c8, csq = operands64(x, c, mu)
    s = torch.einsum("bnd,bkd->bnk", x8, c8) - 0.5 * csq[:, None, :]
    mag = torch.einsum("bnd,bkd->bnk", x8.abs(), c8.abs()) + 0.5 * csq[:, None, :]
    return s, 2 * (2 * x.shape[-1] + 2) * U32 * mag.max(dim=-1).values


def near_tie_share(x, c, mu=None):
    s, eps = margin_reference(x, c, mu)
    top = s.topk(2, dim=-1).values
    return ((top[..., 0] - top[..., 1]) <= eps).double().mean().item()


def check_labels_margin(labels, x, c, mu=None, what=""):
    """rule C on the e4m3 statement -> (share inside eps, labels that differ from the statement's arg-max)"""
    lab = labels.cpu().long()
    s, eps = margin_reference(x, c, mu)
    assert lab.shape == s.shape[:2] and int(lab.min()) >= 0 and int(lab.max()) < s.shape[-1], f"{what}: labels out of range"
    top = s.topk(2, dim=-1).values
    inside = (top[..., 0] - top[..., 1]) <= eps
    ref = lowest_argmax(s)
    got = torch.gather(s, 2, lab[..., None])[..., 0]
    wrong_clear = ~inside & (lab != ref)
    wrong_near = inside & (got < top[..., 0] - eps)
    share, differ = inside.double().mean().item(), int((lab != ref).sum())
    print(f"{what}: near-tie share {share:.4f} (cap {NEAR_TIE_CAP}), labels off the e4m3 statement's arg-max {differ} of {lab.numel()}, "
          f"outside rule C {int(wrong_clear.sum()) + int(wrong_near.sum())}")
    assert share <= NEAR_TIE_CAP, f"{what}: {share:.4f} of the rows lie inside eps"
    if wrong_clear.any() or wrong_near.any():
        b, n = (wrong_clear | wrong_near).nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(wrong_clear.sum())} labels differ from the statement's arg-max on rows with a margin above eps and "
                             f"{int(wrong_near.sum())} near-tie rows carry a label further than eps from the maximum; first [{b}, {n}]: label "
                             f"{int(lab[b, n])} (score {got[b, n].item():.9g}), arg-max {int(ref[b, n])} ({top[b, n, 0].item():.9g}), second "
                             f"{top[b, n, 1].item():.9g}, eps {eps[b, n].item():.3g}")
    return share, differ


def with_offset(x, c):
    """the exact cases moved by OFFSET in every channel: still integers both 16-bit types hold exactly -> (x, c, mu float32 [B, D])"""
    mu = torch.full((x.shape[0], x.shape[-1]), float(OFFSET))
    xo, co = (x.float() + OFFSET).to(x.dtype), (c.float() + OFFSET).to(c.dtype)
    assert torch.equal(xo.float() - OFFSET, x.float()) and torch.equal(co.float() - OFFSET, c.float())
    return xo, co, mu


def centre_bound(c):
    """float64 [B, D]: (K + 1) 2^-24 mean_k |c| — an fp32 sum of K terms in any order and one division"""
    return (c.shape[1] + 1) * U32 * c.double().abs().mean(dim=1)


# ---------------------------------------------------------------------------------------------------------
# the mixed loop and its quality measure
# ---------------------------------------------------------------------------------------------------------
def update64(x, labels, c_old):
    """the 16-bit rounding of the float64 cluster means; empty clusters keep c_old"""
    sums, counts = KC.cluster_sums64(x, labels, c_old.shape[1])
    mean = (sums / counts.clamp(min=1).double()[..., None]).to(c_old.dtype)
    return torch.where((counts == 0)[..., None], c_old, mean)


def mixed_loop64(x, c0, iters, fp8_iters):
    """-> (labels int64 [B, N] of the last iteration, centroids after its update)"""
    mu = centre64(c0).float()
    cur, labels = c0, None
    for it in range(iters):
        labels = assign64(x, cur, mu) if it < fp8_iters else lowest_argmax(KC.scores64(x, cur))
        cur = update64(x, labels, cur)
    return labels, cur


def inertia64(x, c, labels):
    """float64 [B]: sum_n |x_n - c_label(n)|^2"""
    cl = torch.gather(c.double(), 1, labels.long()[..., None].expand(-1, -1, x.shape[-1]))
    return ((x.double() - cl) ** 2).sum(dim=(1, 2))


QUALITY_ITERS = 10
QUALITY_DRAWS = 5


def initial_points(x, K, draw):
    """K distinct rows of every batch of x as initial centroids; draw 0 is real_case's own choice (rows 100 .. 100 + K)"""
    if draw == 0:
        return x[:, 100:100 + K].clone()
    g = torch.Generator().manual_seed(7700 + draw)
    idx = torch.stack([torch.randperm(x.shape[1], generator=g)[:K] for _ in range(x.shape[0])])
    return torch.gather(x, 1, idx[..., None].expand(-1, -1, x.shape[-1])).contiguous()
