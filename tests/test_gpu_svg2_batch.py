"""SVG2 on a batch of videos (cfg > 1): the grouped Lloyd loop (svg_kmeans_loop_grouped[_strided]: one stopping rule per video), the
layer-call svg2_sparse_attention at cfg = 2 / 3, and the SAP processors of Hunyuan, Wan and Cosmos.  The contract under test: every
video of a batch gets, bit for bit, what a cfg = 1 call on that video alone gives."""
import ctypes as C
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import svg_oracle as O

ROOT = Path(__file__).resolve().parent.parent
from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)
from poisoned import poisoned, poisoned_like

pytestmark = pytest.mark.gpu


def _clustered(B, N, D, modes, gen, spread=0.4):
    centers = torch.randn(B, modes, D, generator=gen) * 2.0
    lab = torch.randint(0, modes, (B, N), generator=gen)
    return torch.gather(centers, 1, lab[..., None].expand(-1, -1, D)) + spread * torch.randn(B, N, D, generator=gen)


def _eq(a, b):
    return torch.equal(a.cpu(), b.cpu())


# ---------------------------------------------------------------------------------------------------------------------------------
# 1-3: the C ABI of the grouped loop
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("tol,iters", [(1e9, 4), (1e-4, 12), (0.0, 3)])   # fires at once / fires on the way (or not) / never fires
@pytest.mark.parametrize("strided", [False, True])
def test_grouped_loop_one_group_equals_ungrouped(D, dt, tol, iters, strided):
    from svg import _native as nat

    gen = torch.Generator().manual_seed(D + iters)
    B, N, K = 6, 1500, 24
    if strided:   # the video tokens of a [B, S, D] tensor with text rows behind them: batches S * D apart
        full = _clustered(B, N + 40, D, 10, gen).to(dt).cuda()
        x = full[:, :N]
        assert not x.is_contiguous()
    else:
        x = _clustered(B, N, D, 10, gen).to(dt).cuda()
    init = x[:, :K].contiguous()
    a = nat.kmeans_loop(x, None, init, iters, tol)
    b = nat.kmeans_loop(x, None, init, iters, tol, group=B)
    for t1, t2 in zip(a, b):
        assert _eq(t1.reshape(-1), t2.reshape(-1))
    assert b[3].shape == (1,)


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_grouped_loop_groups_are_independent(strided, dt):
    """Group 0: every point lies exactly on one of its initial centroids -> shift 0, it stops after one iteration.  Group 1: random
    data that does not converge within max_iters.  Each group equals a one-group call on it alone; the ungrouped loop runs group 0
    on to max_iters (the rule the grouped loop replaces)."""
    from svg import _native as nat

    gen = torch.Generator().manual_seed(7)
    H, N, D, K, iters, tol = 3, 1200, 128, 16, 6, 1e-6
    pts = torch.randn(H, K, D, generator=gen) * 2.0
    g0 = torch.gather(pts, 1, torch.randint(0, K, (H, N), generator=gen)[..., None].expand(-1, -1, D))
    g0[:, :K] = pts                                  # every centroid is one of the points: no cluster is empty
    g1 = torch.randn(H, N, D, generator=gen)
    xb = torch.cat([g0, g1]).to(dt)
    if strided:
        full = torch.zeros(2 * H, N + 24, D, dtype=dt)
        full[:, :N] = xb
        x = full.cuda()[:, :N]
    else:
        x = xb.cuda()
    init = x[:, :K].contiguous()
    grouped = nat.kmeans_loop(x, None, init, iters, tol, group=H)
    n_g = grouped[3].cpu().tolist()
    for g in range(2):
        sl = slice(g * H, (g + 1) * H)
        alone = nat.kmeans_loop(x[sl], None, init[sl].contiguous(), iters, tol)
        for t_g, t_a in zip((grouped[0], grouped[1], grouped[2], grouped[4]), (alone[0], alone[1], alone[2], alone[4])):
            assert _eq(t_g[sl], t_a)
        assert n_g[g] == int(alone[3].item())
    assert n_g == [1, iters]
    assert _eq(grouped[1][:H], init[:H])             # a stopped group returns the OLD centroids
    ungrouped = nat.kmeans_loop(x, None, init, iters, tol)
    assert int(ungrouped[3].item()) == iters != n_g[0]


def test_grouped_loop_bad_arguments():
    from svg import _native as nat

    lib = nat.load()
    B, N, K, D = 4, 512, 8, 64
    x = torch.randn(B, N, D, dtype=torch.bfloat16, device="cuda")
    init = x[:, :K].contiguous()
    ca, cb, cent = (poisoned_like(init) for _ in range(3))
    labels = poisoned(B, N, dtype=torch.int32)
    sorted_idx = poisoned_like(labels)
    counts = poisoned(B, K, dtype=torch.int32)
    n_it = torch.zeros(B, dtype=torch.int32, device="cuda")
    need = lib.svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, 2)
    assert need > 0 and lib.svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, 3) == 0
    assert lib.svg_kmeans_loop_grouped_workspace_bytes(B, N, K, D, B) == lib.svg_kmeans_loop_workspace_bytes(B, N, K, D)
    ws = poisoned(need, dtype=torch.uint8)

    def call(group, ws_bytes, strided=False):
        ptrs = (init.data_ptr(), ca.data_ptr(), cb.data_ptr(), labels.data_ptr(), counts.data_ptr(), sorted_idx.data_ptr(), cent.data_ptr(),
                n_it.data_ptr(), B, N, K, D, nat.SVG_DTYPE_BF16, group, 2, 1e-4, ws.data_ptr(), ws_bytes, C.c_void_p(0))
        if strided:
            return lib.svg_kmeans_loop_grouped_strided(x.data_ptr(), N * D, *ptrs)
        return lib.svg_kmeans_loop_grouped(x.data_ptr(), None, *ptrs)

    for strided in (False, True):
        assert call(3, need, strided) == -1      # B % group != 0: SVG_ERR_BAD_ARG
        assert call(0, need, strided) == -1      # group <= 0
        assert call(-2, need, strided) == -1
        assert call(2, need - 1, strided) == -3  # short workspace: SVG_ERR_WORKSPACE
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4-5: the layer-call
# ---------------------------------------------------------------------------------------------------------------------------------
H_, D_, F_, P_, QC, KC = 3, 128, 8, 250, 10, 24


def _layer_data(cfg, model, seed, dt=torch.bfloat16):
    gen = torch.Generator().manual_seed(seed)
    ctx, L = (256, 40) if model == "hy" else (0, 0)
    S = F_ * P_ + ctx
    q = _clustered(cfg * H_, S, D_, 12, gen).reshape(cfg, H_, S, D_).to(dt).cuda()
    k = _clustered(cfg * H_, S, D_, 20, gen).reshape(cfg, H_, S, D_).to(dt).cuda()
    v = torch.randn(cfg, H_, S, D_, generator=gen).to(dt).cuda()
    return q, k, v, ctx, L


def _seeded_store(q, k, V, cfg):
    """a store warm-started from per-video centroids (random points of each video's tokens)"""
    from svg.models import _core

    st = _core.CentroidStore()
    st.put(0, q[:, :, :V][:, :, ::7][:, :, :QC].reshape(cfg * H_, QC, D_).contiguous(),
           k[:, :, :V][:, :, ::5][:, :, :KC].reshape(cfg * H_, KC, D_).contiguous(), cfg)
    return st


def _video_store(st, c):
    from svg.models import _core

    one = _core.CentroidStore()
    one.put(0, st.q[0][c * H_:(c + 1) * H_].contiguous(), st.k[0][c * H_:(c + 1) * H_].contiguous(), 1)
    return one


@pytest.mark.parametrize("token_major", [True, False])
@pytest.mark.parametrize("model", ["hy", "wan"])
@pytest.mark.parametrize("cfg", [2, 3])
def test_layer_call_each_video_equals_its_cfg1_call(cfg, model, token_major):
    from svg.kmeans_utils import identify_dynamic_map
    from svg.models import _core

    q, k, v, ctx, L = _layer_data(cfg, model, 10 + cfg)
    V = F_ * P_
    S = V + ctx
    geo = _core.Geometry(ctx, F_, P_)
    old = _core.TOKEN_MAJOR_IO
    _core.TOKEN_MAJOR_IO = token_major
    try:
        # warm start from the same per-video centroids: outputs, labels, sizes, sorted indices, iteration counts, block maps
        st_b = _seeded_store(q, k, V, cfg)
        singles = [_video_store(st_b, c) for c in range(cfg)]
        cl_b = _core.kmeans_clustering(_seeded_store(q, k, V, cfg), 0, q[:, :, :V], k[:, :, :V], QC, KC, 5, 3)
        o_b = _core.svg2_sparse_attention(q, k, v, geo, st_b, 0, QC, KC, 0.6, 0.1, 5, 3, prompt_length=L)
        assert o_b.shape == (cfg, H_, S, D_)
        if token_major:
            assert o_b.stride() == (S * H_ * D_, D_, H_ * D_, 1)   # stored [cfg, S, H, D]
        else:
            assert o_b.is_contiguous()
        qit_b, kit_b = cl_b[0][3].cpu().tolist(), cl_b[1][3].cpu().tolist()
        assert len(qit_b) == len(kit_b) == cfg
        map_b = identify_dynamic_map(cl_b[0][1].view(cfg, H_, QC, D_), cl_b[1][1].view(cfg, H_, KC, D_), cl_b[0][2].view(cfg, H_, QC),
                                     cl_b[1][2].view(cfg, H_, KC), 0.6, 0.1)
        for c in range(cfg):
            qs, ks = q[c:c + 1].contiguous(), k[c:c + 1].contiguous()
            one = singles[c]
            cl_1 = _core.kmeans_clustering(_video_store(_seeded_store(q, k, V, cfg), c), 0, qs[:, :, :V], ks[:, :, :V], QC, KC, 5, 3)
            o_1 = _core.svg2_sparse_attention(qs, ks, v[c:c + 1], geo, one, 0, QC, KC, 0.6, 0.1, 5, 3, prompt_length=L)
            assert _eq(o_b[c], o_1[0]), (c, "output")
            hs = slice(c * H_, (c + 1) * H_)
            for side in range(2):
                lb, cb, sb, itb, ib = cl_b[side]
                l1, c1, s1, it1, i1 = cl_1[side]
                assert _eq(lb[hs], l1) and _eq(cb[hs], c1) and _eq(sb[hs], s1) and _eq(ib[hs], i1), (c, side)
                assert (qit_b, kit_b)[side][c] == int(it1.item())
            assert _eq(st_b.q[0][hs], one.q[0]) and _eq(st_b.k[0][hs], one.k[0])
            map_1 = identify_dynamic_map(cl_1[0][1][None], cl_1[1][1][None], cl_1[0][2][None], cl_1[1][2][None], 0.6, 0.1)
            assert _eq(map_b[c], map_1[0]), (c, "block map")
        # the init path: video 0 of the batch gets the initial points of a cfg = 1 call at the same seed
        torch.manual_seed(21)
        torch.cuda.manual_seed(21)
        st_i = _core.CentroidStore()
        o_i = _core.svg2_sparse_attention(q, k, v, geo, st_i, 0, QC, KC, 0.6, 0.1, 5, 3, prompt_length=L)
        torch.manual_seed(21)
        torch.cuda.manual_seed(21)
        st_1 = _core.CentroidStore()
        o_1 = _core.svg2_sparse_attention(q[:1].contiguous(), k[:1].contiguous(), v[:1], geo, st_1, 0, QC, KC, 0.6, 0.1, 5, 3, prompt_length=L)
        assert _eq(o_i[0], o_1[0]) and _eq(st_i.q[0][:H_], st_1.q[0]) and _eq(st_i.k[0][:H_], st_1.k[0])
        assert st_i.cfg[0] == cfg and torch.isfinite(o_i.float()).all()
    finally:
        _core.TOKEN_MAJOR_IO = old


@pytest.mark.parametrize("dt,tol", [(torch.bfloat16, 3e-3), (torch.float16, 1e-3)])
def test_layer_call_cfg2_against_oracle(dt, tol):
    """cfg = 2, Hunyuan layout: the fp32 oracle composed from the same initial centroids — k-means (O.batch_kmeans_euclid), the block
    map (exact mode, on the kernels' centroids), the permutation (stable argsort of the labels), masked attention."""
    from svg.models import _core

    cfg = 2
    q, k, v, ctx, L = _layer_data(cfg, "hy", 31, dt)
    V = F_ * P_
    S = V + ctx
    geo = _core.Geometry(ctx, F_, P_)
    st0 = _seeded_store(q, k, V, cfg)
    qc0, kc0 = st0.q[0].clone(), st0.k[0].clone()
    st = _seeded_store(q, k, V, cfg)
    (ql, qc, qs, _, qidx), (kl, kc, ks, _, kidx) = _core.kmeans_clustering(_seeded_store(q, k, V, cfg), 0, q[:, :, :V], k[:, :, :V],
                                                                           QC, KC, 5, 2)
    o = _core.svg2_sparse_attention(q, k, v, geo, st, 0, QC, KC, 0.6, 0.1, 5, 2, prompt_length=L)
    ql, kl = ql.cpu(), kl.cpu()
    assert _eq(qidx, O.stable_argsort(ql).to(torch.int32)) and _eq(kidx, O.stable_argsort(kl).to(torch.int32))
    for x, init, lab in ((q, qc0, ql), (k, kc0, kl)):
        for c in range(cfg):
            hs = slice(c * H_, (c + 1) * H_)
            rl, _, _, _ = O.batch_kmeans_euclid(x[c, :, :V].cpu(), init.shape[1], max_iters=2, init_centroids=init[hs].cpu(), tol=1e-4)
            assert (lab[hs] != rl).float().mean() < 2e-2
    dmap = O.identify_dynamic_map(qc.view(cfg, H_, QC, D_).cpu(), kc.view(cfg, H_, KC, D_).cpu(), qs.view(cfg, H_, QC).cpu(),
                                  ks.view(cfg, H_, KC).cpu(), 0.6, 0.1, exact=True)
    from svg.kmeans_utils import identify_dynamic_map

    kmap = identify_dynamic_map(qc.view(cfg, H_, QC, D_), kc.view(cfg, H_, KC, D_), qs.view(cfg, H_, QC), ks.view(cfg, H_, KC), 0.6, 0.1)
    assert _eq(kmap.bool(), dmap)
    num = den = 0.0
    for c in range(cfg):
        for h in range(H_):
            bh = c * H_ + h
            em = torch.zeros(S, S, dtype=torch.bool)
            em[:V, :V] = dmap[c, h][ql[bh]][:, kl[bh]]
            em[:V, V:V + L] = True
            em[V:V + L, : V + L] = True
            em[V + L:, V + L:] = True
            ref = O.masked_attention(q[c, h].cpu(), k[c, h].cpu(), v[c, h].cpu(), em)
            num += float(((o[c, h].float().cpu() - ref) ** 2).sum())
            den += float((ref ** 2).sum())
    assert (num / den) ** 0.5 < tol


def test_layer_call_fp8_at_cfg2():
    """the fp8 attention path runs at cfg > 1, each video equal to its cfg = 1 call"""
    from svg.models import _core

    cfg = 2
    q, k, v, ctx, L = _layer_data(cfg, "wan", 41)
    V = F_ * P_
    geo = _core.Geometry(ctx, F_, P_)
    _core.set_attention_dtype("fp8")
    try:
        st = _seeded_store(q, k, V, cfg)
        ones = [_video_store(st, c) for c in range(cfg)]
        o_b = _core.svg2_sparse_attention(q, k, v, geo, st, 0, QC, KC, 0.6, 0.1, 5, 2)
        for c in range(cfg):
            o_1 = _core.svg2_sparse_attention(q[c:c + 1].contiguous(), k[c:c + 1].contiguous(), v[c:c + 1], geo, ones[c], 0, QC, KC, 0.6,
                                              0.1, 5, 2)
            assert _eq(o_b[c], o_1[0])
    finally:
        _core.set_attention_dtype("bf16")
    assert torch.isfinite(o_b.float()).all()


def test_density_log_per_video(tmp_path):
    from svg.models import _core

    cfg = 2
    q, k, v, ctx, L = _layer_data(cfg, "hy", 51)
    V = F_ * P_
    geo = _core.Geometry(ctx, F_, P_)
    log = tmp_path / "d.jsonl"
    _core.svg2_sparse_attention(q, k, v, geo, _seeded_store(q, k, V, cfg), 3, QC, KC, 0.6, 0.1, 5, 2, prompt_length=L,
                                logging_file=str(log))
    _core.flush_density_log()
    import json

    (entry,) = [json.loads(s) for s in log.read_text().splitlines()]
    assert entry["layer"] == 3 and len(entry["density"]) == cfg and len(entry["video_avg_density"]) == cfg
    assert abs(sum(entry["video_avg_density"]) / cfg - entry["avg_density"]) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: processors
# ---------------------------------------------------------------------------------------------------------------------------------
class _PerVideoLinear(torch.nn.Module):
    """nn.Linear applied video by video: the projections of a batch then round exactly like those of one video (a GEMM's kernel
    choice may depend on the number of rows), so that what is compared is the processors' attention core."""

    def __init__(self, lin):
        super().__init__()
        self.lin = lin

    def forward(self, x):
        return torch.cat([self.lin(x[i:i + 1]) for i in range(x.shape[0])])


def _per_video(attn):
    for name in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_add_out"):
        m = getattr(attn, name, None)
        if isinstance(m, torch.nn.Linear):
            setattr(attn, name, _PerVideoLinear(m))
    attn.to_out[0] = _PerVideoLinear(attn.to_out[0])
    return attn


def _configure_sap(cls, ctx, F, P, L=0):
    cls.context_length, cls.num_frame, cls.frame_size = ctx, F, P
    if hasattr(cls, "prompt_length"):
        cls.prompt_length = L
    cls.first_layers_fp, cls.first_times_fp = 0, 900.0
    cls.num_q_centroids, cls.num_k_centroids, cls.top_p_kmeans, cls.min_kc_ratio = QC, KC, 0.6, 0.1
    cls.kmeans_iter_init, cls.kmeans_iter_step, cls.zero_step_kmeans_init = 5, 2, True


def _run_processor(cfg, call, set_store, get_store):
    """call(videos: slice, timestep) -> the processor's output for those videos.  cfg = 2: a dense step with the k-means init, then a
    sparse warm-started step; each video against a cfg = 1 processor state of its own (video 0: the same seed; video 1: warm-started from
    its slice of the batch's centroids).  Then a cfg = 1 call on the batch's processor re-initialises that layer's centroids."""
    from svg.models import _core

    everything = slice(0, cfg)
    stores = [_core.CentroidStore() for _ in range(cfg)]
    set_store(_core.CentroidStore())
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    with torch.no_grad():
        d_b = call(everything, 950.0)
    st_b = get_store()
    assert st_b.cfg[0] == cfg
    set_store(stores[0])
    torch.manual_seed(3)
    torch.cuda.manual_seed(3)
    with torch.no_grad():
        d_0 = call(slice(0, 1), 950.0)
    assert _eq(st_b.q[0][:H_P], stores[0].q[0]) and _eq(st_b.k[0][:H_P], stores[0].k[0])   # video 0: the init of a cfg = 1 call
    for c in range(cfg):
        if c:
            set_store(_core.CentroidStore())   # (the dense output does not read the centroids; this call's k-means is thrown away)
            with torch.no_grad():
                d_c = call(slice(c, c + 1), 950.0)
            stores[c].put(0, st_b.q[0][c * H_P:(c + 1) * H_P].clone(), st_b.k[0][c * H_P:(c + 1) * H_P].clone(), 1)
        else:
            d_c = d_0
        assert _eq(d_b[c], d_c[0]), (c, "dense step")
    set_store(st_b)
    with torch.no_grad():
        s_b = call(everything, 100.0)
    for c in range(cfg):
        set_store(stores[c])
        with torch.no_grad():
            s_c = call(slice(c, c + 1), 100.0)
        assert _eq(s_b[c], s_c[0]), (c, "sparse step")
        assert _eq(st_b.q[0][c * H_P:(c + 1) * H_P], stores[c].q[0]) and _eq(st_b.k[0][c * H_P:(c + 1) * H_P], stores[c].k[0])
    # another cfg on the same layer: a first call (random init, iter_init iterations), never a warm start from the cfg = 2 centroids
    set_store(st_b)
    torch.manual_seed(9)
    torch.cuda.manual_seed(9)
    with torch.no_grad():
        r_b = call(slice(1, 2), 100.0)
    assert st_b.cfg[0] == 1 and st_b.q[0].shape[0] == H_P
    set_store(_core.CentroidStore())
    torch.manual_seed(9)
    torch.cuda.manual_seed(9)
    with torch.no_grad():
        r_1 = call(slice(1, 2), 100.0)
    assert _eq(r_b, r_1)
    assert torch.isfinite(s_b.float()).all()


H_P, HD_P = 2, 128


def test_hunyuan_sap_processor_cfg2():
    from standins import Attention

    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0 as P

    torch.manual_seed(0)
    dim = H_P * HD_P
    ctx, F, P_, L = 256, 8, 250, 21
    _configure_sap(P, ctx, F, P_, L)
    attn = _per_video(Attention(dim, H_P, added_kv=True, dtype=torch.bfloat16).cuda())
    proc = P(0)
    attn.set_processor(proc)
    V = F * P_
    hidden = (torch.randn(2, V, dim) * 0.3).to(torch.bfloat16).cuda()
    enc = (torch.randn(2, ctx, dim) * 0.3).to(torch.bfloat16).cuda()
    ang = torch.rand(V, HD_P) * 6.28
    rope = (ang.cos().cuda(), ang.sin().cuda())

    def call(sl, t):
        h, e = attn(hidden[sl], encoder_hidden_states=enc[sl], attention_mask=None, image_rotary_emb=rope, timestep=torch.tensor([t]))
        return torch.cat([h, e], dim=1)

    def set_store(s):
        proc.centroid_store = s   # (shadows the class-level store: a processor state of its own per run)

    try:
        _run_processor(2, call, set_store, lambda: proc.centroid_store)
    finally:
        P.reset_state()


def _wan_like(cosmos):
    from standins import Attention

    if cosmos:
        from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor as P
    else:
        from svg.models.wan.attention import WanAttn_SAPAttn_Processor as P
    torch.manual_seed(1)
    dim = H_P * HD_P
    F, P_ = 8, 250
    _configure_sap(P, 0, F, P_)
    attn = _per_video(Attention(dim, H_P, qk_norm="rms", across_heads=not cosmos, dtype=torch.bfloat16).cuda())
    proc = P(0)
    attn.set_processor(proc)
    S = F * P_
    hidden = (torch.randn(2, S, dim) * 0.3).to(torch.bfloat16).cuda()
    ang = torch.rand(S, HD_P // 2) * 6.28
    if cosmos:
        cos, sin = torch.cat([ang.cos(), ang.cos()], -1).cuda(), torch.cat([ang.sin(), ang.sin()], -1).cuda()

        def call(sl, t):
            return attn(hidden[sl], image_rotary_emb=(cos, sin), timestep=torch.tensor([t]))
    else:
        rope = (ang.cos().cuda(), ang.sin().cuda())

        def call(sl, t):
            return attn(hidden[sl], rotary_emb=rope, timestep=torch.tensor([t]))

    def set_store(s):
        proc.centroid_store = s

    _run_processor(2, call, set_store, lambda: proc.centroid_store)


def test_wan_sap_processor_cfg2():
    _wan_like(False)


def test_cosmos_sap_processor_cfg2():
    _wan_like(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# 7: production size
# ---------------------------------------------------------------------------------------------------------------------------------
def test_wan720p_layer_call_cfg2():
    """Wan 2.1 720p (40 heads, S = 75 600, 300 / 1000 centroids), one warm-started layer-call at cfg = 2: each video bit-identical to its
    cfg = 1 call."""
    from svg.models import _core

    cfg, H, D, F, P = 2, 40, 128, 21, 3600
    S = F * P
    gen = torch.Generator(device="cuda").manual_seed(5)
    q, k, v = (torch.randn(cfg, H, S, D, generator=gen, device="cuda", dtype=torch.bfloat16) for _ in range(3))
    geo = _core.Geometry(0, F, P)
    Kq, Kk = 300, 1000
    st = _core.CentroidStore()
    st.put(0, q[:, :, ::97][:, :, :Kq].reshape(cfg * H, Kq, D).contiguous(), k[:, :, ::31][:, :, :Kk].reshape(cfg * H, Kk, D).contiguous(), cfg)
    ones = []
    for c in range(cfg):
        one = _core.CentroidStore()
        one.put(0, st.q[0][c * H:(c + 1) * H].clone(), st.k[0][c * H:(c + 1) * H].clone(), 1)
        ones.append(one)
    o_b = _core.svg2_sparse_attention(q, k, v, geo, st, 0, Kq, Kk, 0.9, 0.1, 50, 2)
    for c in range(cfg):
        o_1 = _core.svg2_sparse_attention(q[c:c + 1], k[c:c + 1], v[c:c + 1], geo, ones[c], 0, Kq, Kk, 0.9, 0.1, 50, 2)
        assert torch.equal(o_b[c], o_1[0]), c
        assert torch.equal(st.q[0][c * H:(c + 1) * H], ones[c].q[0])
    assert torch.isfinite(o_b.float()).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# 8: head-sharded, 2 ranks on one GPU over gloo
# ---------------------------------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, str(ROOT / "sparse-videogen_amd"))
    from svg import _native as nat_
    from svg import distributed as sd
    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    from svg.models import _core

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(3)
    ok = True
    for ctx, L in ((0, 0), (128, 20)):
        cfg, H, D, F, P = 2, 5, 128, 5, 300
        S = F * P + ctx
        q, k, v = (_clustered(cfg * H, S, D, 12, g).reshape(cfg, H, S, D).to(torch.bfloat16).to(dev) for _ in range(3))
        geo = _core.Geometry(ctx, F, P)

        def svg2(store):
            outs = []
            for call in range(2):   # the first call (random initial points), then a warm start
                torch.manual_seed(5 + call)
                torch.cuda.manual_seed(5 + call)
                outs.append(_core.svg2_sparse_attention(q, k, v, geo, store, 0, 12, 30, 0.9, 0.1, 4, 2, prompt_length=L))
            return outs + [store.q[0], store.k[0]]

        ref = svg2(_core.CentroidStore())
        sd.enable()
        sh = svg2(_core.CentroidStore())
        sd.disable()
        ok &= all(torch.equal(a.reshape(-1), b.reshape(-1)) for a, b in zip(ref[:2], sh[:2]))
        ok &= all(torch.isfinite(a.float()).all() for a in sh[:2])
    ret[rank] = bool(ok)
    dist.destroy_process_group()


def test_head_sharded_svg2_cfg2_equals_unsharded():
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 41500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    assert dict(ret) == {0: True, 1: True}
