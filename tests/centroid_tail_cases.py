"""What the tests of the centroid tail share (include/svg_attn_centroid_tail.h; tests/test_centroid_tail_cpu.py,
tests/test_gpu_centroid_tail.py).  Plain module, no GPU.

  * the float64 statements: the cluster means; the attention state of a row over the keys its block-row's map row selects ("sparse"), over
    the pseudo keys of the clusters it does not select ("tail": key kbar_c, value vbar_c, score sm q . kbar_c + ln n_c), and their merge.
    Rows and keys carry LABELS (the block-row of a row, the cluster of a key; -1: in none), so one statement serves the kernel cases (labels
    from sizes and index arrays) and the layer cases (labels from the k-means of the call, with HunyuanVideo's two text clusters behind);
  * the bounds: none of its own — T_SINGLE, check_lse and merged_limit of tests/sparse_lse_cases.py;
  * the inputs, computed once and shared: the kernel shapes of the issue (H = 2, S = 777, q_sizes [200, 0, 1, 300, 17, 259], KC 70 / 200),
    the case that is exact by construction (clusters of identical rows), and the fixed Gaussian mixtures of the layer cases."""
import functools
import math

import torch

from lse_ops_torch import merge_states

D = 128
NINF = float("-inf")
DTYPES = [torch.bfloat16, torch.float16]


# ---------------------------------------------------------------------------------------------------------
# statements
# ---------------------------------------------------------------------------------------------------------
def means64(x, labels, K):
    """float64 [B, K, D]: the mean of the rows of x [B, N, D] with label c; an empty cluster gives zeros.  labels [B, N] (-1: no cluster)"""
    B, N, Dx = x.shape
    out = torch.zeros(B, K, Dx, dtype=torch.float64)
    cnt = torch.zeros(B, K, dtype=torch.float64)
    lab = labels.long()
    for b in range(B):
        ok = lab[b] >= 0
        out[b].index_add_(0, lab[b][ok], x[b][ok].double())
        cnt[b].index_add_(0, lab[b][ok], torch.ones(int(ok.sum()), dtype=torch.float64))
    return out / cnt.clamp(min=1)[..., None]


def labels_from_sizes(sizes, idx, N):
    """[B, N] int64: the cluster of every row, from the sizes [B, K] and the sorted indices idx [B, N] (None: identity); -1 for a row behind
    sum(sizes[b])"""
    B = sizes.shape[0]
    lab = torch.full((B, N), -1, dtype=torch.int64)
    for b in range(B):
        order = torch.arange(N) if idx is None else idx[b].long()
        n = int(sizes[b].sum())
        lab[b, order[:n]] = torch.repeat_interleave(torch.arange(sizes.shape[1]), sizes[b].long())
    return lab


def state64(q, k, v, mask, bias=None, scale=None):
    """float64 (o, lse) of q [S, D] over k, v [n, D] under mask bool [S, n] with an additive bias [n] on the scaled scores; a row without
    keys: zeros and -inf"""
    s = q.double() @ k.double().T * (1.0 / math.sqrt(q.shape[-1]) if scale is None else scale)
    if bias is not None:
        s = s + bias.double()[None]
    s = s.masked_fill(~mask, NINF)
    lse = torch.logsumexp(s, dim=-1)
    seen = torch.isfinite(lse)
    p = torch.exp(s - torch.where(seen, lse, torch.zeros_like(lse))[:, None])
    return p @ v.double(), lse


def statement(q, k, v, q_labels, k_labels, bmap, kbar, vbar, k_sizes, tail_map=None, scale=None):
    """The three states of every row, float64, per head: q [H, S, D]; k, v [H, Skv, D]; q_labels [H, S], k_labels [H, Skv] (-1: none);
    bmap bool [H, QB, KB]; kbar, vbar [H, KC, D] with KC <= KB; k_sizes [H, KC]; tail_map: the map the tail reads (None: bmap).
    -> dict of o_sparse, lse_sparse, o_tail, lse_tail, o, lse (the merge) and covered bool [H, S]"""
    H, S, _ = q.shape
    KC = kbar.shape[1]
    tmap = bmap if tail_map is None else tail_map
    out = {n: [] for n in ("o_sparse", "lse_sparse", "o_tail", "lse_tail")}
    for h in range(H):
        cov = q_labels[h] >= 0
        a = q_labels[h].clamp(min=0)
        kl = k_labels[h]
        em = bmap[h].bool()[a][:, kl.clamp(min=0)] & (kl >= 0)[None] & cov[:, None]
        o_s, l_s = state64(q[h], k[h], v[h], em, None, scale)
        tm = ~tmap[h].bool()[a][:, :KC] & (k_sizes[h] > 0)[None] & cov[:, None]
        o_t, l_t = state64(q[h], kbar[h], vbar[h], tm, torch.log(k_sizes[h].double().clamp(min=1)), scale)
        for n, t in zip(out, (o_s, l_s, o_t, l_t)):
            out[n].append(t)
    out = {n: torch.stack(t) for n, t in out.items()}
    out["o"], out["lse"] = merge_states([out["o_sparse"], out["o_tail"]], [out["lse_sparse"], out["lse_tail"]], return_lse=True)
    out["covered"] = q_labels >= 0
    return out


def dense64(q, k, v, scale=None):
    """float64 dense attention per head -> (o [H, S, D], lse [H, S])"""
    res = [state64(q[h], k[h], v[h], torch.ones(q.shape[1], k.shape[1], dtype=torch.bool), None, scale) for h in range(q.shape[0])]
    return torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res])


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp(min=1e-300)).item()


# ---------------------------------------------------------------------------------------------------------
# kernel cases: H = 2, S = 777
# ---------------------------------------------------------------------------------------------------------
H, S = 2, 777
Q_SIZES = [200, 0, 1, 300, 17, 259]      # sums to S; block-row 1 is empty, block-row 2 one row
ONES_ROW, ZEROS_ROW = 4, 5               # the map row that selects every cluster (no tail), the one that selects none
KCS = [70, 200]                          # a ragged second tile / four tiles
SHORT_LAST = 200                         # head 1 of the `short` variant: its last block-row leaves 59 rows uncovered


@functools.lru_cache(maxsize=None)
def kernel_case(KC, dtype, with_idx, short=False):
    """inputs of the tail entry alone: random centroids, weights in [0, 4000] with several zeros and a one
    -> dict(q, kbar, vbar, bmap, q_sizes, k_sizes, idx)"""
    g = torch.Generator().manual_seed(1000 * KC + (7 if with_idx else 0) + (3 if dtype == torch.float16 else 0))
    q = torch.randn(H, S, D, generator=g).to(dtype)
    kbar, vbar = (torch.randn(H, KC, D, generator=g).to(dtype) for _ in range(2))
    ks = torch.randint(0, 4001, (H, KC), generator=g, dtype=torch.int32)
    ks[:, [3, 17, KC - 1]] = 0
    ks[0, 64 if KC > 64 else 5] = 0
    ks[:, 9], ks[:, 10] = 1, 4000
    bmap = torch.rand(H, len(Q_SIZES), KC, generator=g) < 0.3
    bmap[:, ONES_ROW], bmap[:, ZEROS_ROW] = True, False
    qs = torch.tensor([Q_SIZES, Q_SIZES], dtype=torch.int32)
    if short:
        qs[1, -1] = SHORT_LAST
    idx = torch.stack([torch.randperm(S, generator=g) for _ in range(H)]).to(torch.int32) if with_idx else None
    return dict(q=q, kbar=kbar, vbar=vbar, bmap=bmap, q_sizes=qs, k_sizes=ks, idx=idx)


@functools.lru_cache(maxsize=None)
def kernel_reference(KC, dtype, with_idx, short=False):
    """the tail's float64 (o, lse, covered) of kernel_case"""
    c = kernel_case(KC, dtype, with_idx, short)
    ql = labels_from_sizes(c["q_sizes"], c["idx"], S)
    no_keys = torch.zeros(H, 0, D)
    st = statement(c["q"], no_keys, no_keys, ql, torch.zeros(H, 0, dtype=torch.int64), c["bmap"], c["kbar"], c["vbar"], c["k_sizes"])
    return st["o_tail"], st["lse_tail"], st["covered"]


def partition_with_zeros_and_a_one(n, K, g, zeros=5):
    """int32 [K] summing to n: `zeros` clusters of size 0 at random places, one cluster of size exactly 1"""
    m = K - zeros
    sz = torch.ones(m, dtype=torch.int64)
    extra = torch.multinomial(torch.ones(m - 1), n - m, replacement=True, generator=g)
    sz[1:] += torch.bincount(extra, minlength=m - 1)
    full = torch.zeros(K, dtype=torch.int64)
    full[torch.randperm(K, generator=g)[:m].sort().values] = sz[torch.randperm(m, generator=g)]
    assert int(full.sum()) == n and int((full == 0).sum()) == zeros and int((full == 1).sum()) >= 1
    return full.to(torch.int32)


@functools.lru_cache(maxsize=None)
def merge_case(KC, dtype, with_idx):
    """the protocol: 777 keys in KC clusters (zeros and a one among the sizes), kbar / vbar their float64 means rounded once
    -> dict(q, k, v, kbar, vbar, bmap, q_sizes, k_sizes, q_idx, kv_idx)"""
    g = torch.Generator().manual_seed(2000 * KC + (7 if with_idx else 0) + (3 if dtype == torch.float16 else 0))
    q, k, v = (torch.randn(H, S, D, generator=g).to(dtype) for _ in range(3))
    ks = torch.stack([partition_with_zeros_and_a_one(S, KC, g) for _ in range(H)])
    bmap = torch.rand(H, len(Q_SIZES), KC, generator=g) < 0.3
    bmap[:, ONES_ROW], bmap[:, ZEROS_ROW] = True, False
    qs = torch.tensor([Q_SIZES, Q_SIZES], dtype=torch.int32)
    perm = lambda: torch.stack([torch.randperm(S, generator=g) for _ in range(H)]).to(torch.int32)   # noqa: E731
    q_idx, kv_idx = (perm(), perm()) if with_idx else (None, None)
    kl = labels_from_sizes(ks, kv_idx, S)
    kbar, vbar = means64(k, kl, KC).to(dtype), means64(v, kl, KC).to(dtype)
    return dict(q=q, k=k, v=v, kbar=kbar, vbar=vbar, bmap=bmap, q_sizes=qs, k_sizes=ks, q_idx=q_idx, kv_idx=kv_idx)


@functools.lru_cache(maxsize=None)
def merge_reference(KC, dtype, with_idx):
    c = merge_case(KC, dtype, with_idx)
    return statement(c["q"], c["k"], c["v"], labels_from_sizes(c["q_sizes"], c["q_idx"], S), labels_from_sizes(c["k_sizes"], c["kv_idx"], S),
                     c["bmap"], c["kbar"], c["vbar"], c["k_sizes"])


# ---------------------------------------------------------------------------------------------------------
# exact by construction: clusters of identical (key, value) rows — sparse + tail IS dense attention
# ---------------------------------------------------------------------------------------------------------
EX_S, EX_KC, EX_Q_SIZES = 1024, 48, [300, 200, 400, 124]


@functools.lru_cache(maxsize=None)
def exact_case(dtype):
    """-> dict(q, k, v, kbar, vbar, bmap, q_sizes, k_sizes): cluster c of head h is k_sizes[h, c] in [1, 60] copies of one (key, value) row,
    laid out cluster after cluster; every map row selects at least one cluster and leaves out at least one"""
    g = torch.Generator().manual_seed(77 + (3 if dtype == torch.float16 else 0))
    ks = torch.randint(1, 42, (H, EX_KC), generator=g)
    for h in range(H):
        while int(ks[h].sum()) != EX_S:
            step = 1 if int(ks[h].sum()) < EX_S else -1
            c = int(torch.randint(0, EX_KC, (1,), generator=g))
            if 1 <= int(ks[h, c]) + step <= 60:
                ks[h, c] += step
    kbar, vbar = (torch.randn(H, EX_KC, D, generator=g).to(dtype) for _ in range(2))
    k = torch.stack([torch.repeat_interleave(kbar[h], ks[h], dim=0) for h in range(H)])
    v = torch.stack([torch.repeat_interleave(vbar[h], ks[h], dim=0) for h in range(H)])
    q = torch.randn(H, EX_S, D, generator=g).to(dtype)
    bmap = torch.rand(H, len(EX_Q_SIZES), EX_KC, generator=g) < 0.5
    bmap[:, :, 0], bmap[:, :, 1] = True, False
    bmap[:, 0, 2:] = False      # block-row 0: one cluster exact, 47 by their centroids
    bmap[:, 1, 2:] = True       # block-row 1: one cluster by its centroid
    qs = torch.tensor([EX_Q_SIZES] * H, dtype=torch.int32)
    return dict(q=q, k=k, v=v, kbar=kbar, vbar=vbar, bmap=bmap, q_sizes=qs, k_sizes=ks.to(torch.int32))


@functools.lru_cache(maxsize=None)
def exact_reference(dtype):
    c = exact_case(dtype)
    return dense64(c["q"], c["k"], c["v"])


# ---------------------------------------------------------------------------------------------------------
# layer cases: fixed Gaussian mixtures; a Wan-like geometry without text and a HunyuanVideo-like one with text and prompt_length < ctx
# ---------------------------------------------------------------------------------------------------------
LAYER_H, F_, P_ = 2, 4, 256
V = F_ * P_                                  # 1024 video tokens
QC, KC_LAYER, TOP_P, MIN_KC_RATIO = 4, 16, 0.7, 0.0
ITER_INIT, ITER_STEP = 4, 2
GEOMETRIES = {"wan": dict(ctx=0, prompt=0), "hy": dict(ctx=64, prompt=40)}    # S = 1024 >= 160 * 4; S = 1088 >= 160 * 6
MODES = 12


@functools.lru_cache(maxsize=None)
def layer_inputs(kind, cfg, dtype):
    """q, k, v [cfg, H, S, D]: the video tokens of a head around MODES directions (a token's query points at its mode's keys, weakly), the
    text tokens plain noise"""
    ctx = GEOMETRIES[kind]["ctx"]
    g = torch.Generator().manual_seed(31 + ctx + cfg)
    shape = (cfg, LAYER_H, MODES, D)
    ck, cv = 0.5 * torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    mode = torch.randint(0, MODES, (cfg, LAYER_H, V), generator=g)
    pick = lambda c: torch.gather(c, 2, mode[..., None].expand(-1, -1, -1, D))   # noqa: E731
    k = pick(ck) + torch.randn(cfg, LAYER_H, V, D, generator=g)
    q = pick(ck) + torch.randn(cfg, LAYER_H, V, D, generator=g)
    v = pick(cv) + 0.5 * torch.randn(cfg, LAYER_H, V, D, generator=g)
    text = [torch.randn(cfg, LAYER_H, ctx, D, generator=g) for _ in range(3)]
    return tuple(torch.cat([x, t], dim=2).to(dtype) for x, t in zip((q, k, v), text))


def layer_statement(kind, q, k, v, q_labels, k_labels, dyn_map, dtype):
    """The float64 statement of svg2_sparse_attention(centroid_tail=True) on one video from the call's own labels [H, V] and map
    [H, QC, KC]: q, k, v [H, S, D].  The means are the float64 means of the labelled rows rounded once to the 16-bit type — the tensor
    svg_cluster_means is specified to return.  HunyuanVideo: rows and keys of the prompt are cluster QC / KC, of the unused prompt QC + 1 /
    KC + 1 (dynamic_map_post_processing), and the tail reads a map whose last row is all ones."""
    from oracle import svg_oracle as O

    geo = GEOMETRIES[kind]
    Hh, KC = q.shape[0], dyn_map.shape[-1]
    ks = torch.stack([torch.bincount(k_labels[h], minlength=KC) for h in range(Hh)])
    kbar, vbar = means64(k[:, :V], k_labels, KC).to(dtype), means64(v[:, :V], k_labels, KC).to(dtype)
    bmap, tail_map, ql, kl = dyn_map.bool(), None, q_labels, k_labels
    if geo["ctx"]:
        qs = torch.stack([torch.bincount(q_labels[h], minlength=dyn_map.shape[-2]) for h in range(Hh)])
        bmap = O.dynamic_map_post_processing(bmap[None], qs[None], ks[None], torch.zeros(Hh, V, dtype=torch.int64), V, geo["ctx"], geo["prompt"])[0][0]
        text = lambda n: torch.cat([torch.full((geo["prompt"],), n), torch.full((geo["ctx"] - geo["prompt"],), n + 1)]).expand(Hh, -1)   # noqa: E731
        ql, kl = torch.cat([q_labels, text(dyn_map.shape[-2])], dim=1), torch.cat([k_labels, text(KC)], dim=1)
        tail_map = bmap.clone()
        tail_map[:, -1] = True
    return statement(q, k, v, ql, kl, bmap, kbar, vbar, ks, tail_map)


def lloyd64(x, K, iters, g):
    """a plain float64 Lloyd loop on x [N, D] from K random rows -> labels [N] (the CPU premise test's clustering; the GPU tests take the
    library's)"""
    xd = x.double()
    c = xd[torch.randperm(x.shape[0], generator=g)[:K]]
    for _ in range(iters):
        lab = torch.cdist(xd, c).argmin(dim=1)
        c = torch.where((torch.bincount(lab, minlength=K) > 0)[:, None], means64(x[None], lab[None], K)[0], c)
    return torch.cdist(xd, c).argmin(dim=1)
