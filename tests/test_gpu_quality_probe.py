"""The processors' quality probe on the GPU (quality_log / quality_rows; svg/models/_core.py log_quality), at the stand-in geometries of
tests/test_gpu_processors.py.

  * with quality_log set the attention output and last_best_mask_idx are torch.equal to those without: SVG1 host path, SVG1 device switch
    (sparse and dense step), SVG2; the global CPU stream ends where it ends without the log;
  * under a dense mask the logged kept mass is 1 and the logged rel. L2 is the rounding of the sparse output;
  * under the model's mask / an SVG2 plan the logged figures are the float64 ones on the same rows;
  * CogVideoX (head_dim 64: no LSE form) logs kept_mass null and an error that matches float64;
  * a device-switch dense step leaves no line.

Bounds, none of them from the code under test.  With b(lse) = U + 1e-5 (1 + |lse|) the bound of check_lse on either log-sum-exp, a kept mass
exp(lse_s - lse_d) is off by a factor within exp(+-(b_s + b_d)): |kept - ref| <= ref (exp(2 max b) - 1), per row and so for the mean.  The
logged rel. L2 is ||o_s' - o_d'|| / ||o_d'|| with o_s' the kernel's 16-bit rows (within merged_limit of the exact rows: the single-call
bound and one output rounding) and o_d' the probe's fp32 rows (within T_SINGLE); by the triangle inequality
|rel' - rel| <= (lim ||o_s|| / ||o_d|| + T (1 + rel)) / (1 - T).  Under a dense mask the issue's own bound holds: rel. L2 <= merged_limit."""
import json
import math

import pytest
import torch

import sparse_lse_cases as SC
from oracle import svg_oracle as O
from poisoned import poison_on  # noqa: F401  (the suite runs on poisoned allocations)
from test_gpu_processors import _clustered

pytestmark = pytest.mark.gpu
DT = torch.bfloat16
T = SC.T_SINGLE[DT]


def lines(path):
    from svg.models import _core

    _core.flush_quality_log()
    try:
        return [json.loads(x) for x in open(path)]
    except FileNotFoundError:
        return []


@pytest.fixture
def probed(monkeypatch):
    """the rows of every probe call, in order (sparse_quality's sixth argument)"""
    from svg.models import _core

    seen = []
    orig = _core.sparse_quality

    def spy(o, lse, q, k, v, rows, *a, **kw):
        seen.append(rows.clone())
        return orig(o, lse, q, k, v, rows, *a, **kw)

    monkeypatch.setattr(_core, "sparse_quality", spy)
    return seen


def lse_b(lse):
    return float(SC.lse_bound(lse[torch.isfinite(lse)], DT).max())


def check_record(rec, o_s, lse_s, o_d, lse_d, what):
    """a logged record against the float64 rows: o_s / lse_s the exact sparse result on the probed rows ([cfg, H, R, D] / [cfg, H, R]; lse_s
    None where the launch has no LSE form), o_d / lse_d the exact dense rows"""
    nd = o_d.norm(dim=(-2, -1))
    rel = (o_s - o_d).norm(dim=(-2, -1)) / nd
    lim = torch.tensor([[SC.merged_limit(o_s[c, h], DT)[0] for h in range(o_s.shape[1])] for c in range(o_s.shape[0])])
    tol = (lim * o_s.norm(dim=(-2, -1)) / nd + T * (1 + rel)) / (1 - T)
    got = torch.tensor(rec["rel_l2"], dtype=torch.float64)
    print(f"{what}: rel_l2 logged {got.flatten().tolist()} float64 {rel.flatten().tolist()} tolerance {tol.flatten().tolist()}")
    assert got.shape == rel.shape and ((got - rel).abs() <= tol).all(), what
    mse = torch.tensor(rec["mse"], dtype=torch.float64)
    R, D = o_d.shape[-2:]
    torch.testing.assert_close(mse, got ** 2 * nd ** 2 / (R * D), rtol=3 * T, atol=0)      # the same difference, over R D instead of ||o_d||^2
    if lse_s is None:
        assert rec["kept_mass"] is None, what
        return
    kept = torch.exp(lse_s - lse_d).mean(-1)
    ktol = kept * (math.exp(2 * max(lse_b(lse_s), lse_b(lse_d))) - 1)
    gk = torch.tensor(rec["kept_mass"], dtype=torch.float64)
    print(f"{what}: kept_mass logged {gk.flatten().tolist()} float64 {kept.flatten().tolist()} tolerance {ktol.flatten().tolist()}")
    assert gk.shape == kept.shape and ((gk - kept).abs() <= ktol).all(), what


def svg1_float64(q, k, v, best, geo, mask_prm, text_first=False):
    """the SVG1 layer-call in float64: placement by best_mask_idx, attention under the band mask, inverse placement — (o, lse) in the
    caller's row order"""
    ctx, F_, P_ = geo
    S = q.shape[2]
    qp, kp, vp = (O.head_placement(t, best, ctx, F_, P_, text_first=text_first) for t in (q, k, v))
    o, lse = SC.masked_attention_lse(qp, kp, vp, O.band_mask(S, *mask_prm))
    o = O.head_placement(o, best, ctx, F_, P_, text_first=text_first, inverse=True)
    lse = O.head_placement(lse[..., None], best, ctx, F_, P_, text_first=text_first, inverse=True)[..., 0]
    return o, lse


def wan_setup(monkeypatch, cls, H=3, D=128, F_=5, P_=160, **attrs):
    from svg.models.wan.utils import generate_temporal_head_mask_mod as wan_mm

    base = dict(context_length=0, num_frame=F_, frame_size=P_, first_layers_fp=0, first_times_fp=900.0, num_sampled_rows=16,
                sample_mse_max_row=400, block_mask=wan_mm(0, 0, F_, P_, mul=1.2), quality_rows=64, quality_log=None)
    base.update(attrs)
    for name, val in base.items():
        monkeypatch.setattr(cls, name, val, raising=False)
    g = torch.Generator().manual_seed(17)
    return tuple(torch.randn(1, H, F_ * P_, D, generator=g).to(DT).cuda() for _ in range(3))


def run(proc, args, seed=3):
    from svg.models import _core

    torch.manual_seed(seed)
    _core.reseed_switch_generator(seed)
    _core.reseed_probe_generator(seed)
    with torch.no_grad():
        out = proc.attention_core_logic(*args)
    return out, proc.last_best_mask_idx, torch.get_rng_state()


def test_wan_svg1_host_path_logs_the_float64_figures_and_changes_nothing(monkeypatch, tmp_path, probed):
    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanP

    q, k, v = wan_setup(monkeypatch, WanP)
    t = torch.tensor([100.0])
    out0, best0, rng0 = run(WanP(2), (q, k, v, t))
    path = str(tmp_path / "q.jsonl")
    monkeypatch.setattr(WanP, "quality_log", path)
    out1, best1, rng1 = run(WanP(2), (q, k, v, t))
    assert torch.equal(out0, out1) and torch.equal(best0, best1) and torch.equal(rng0, rng1)
    rec = lines(path)
    assert len(rec) == 1 and len(probed) == 1 and rec[0]["timestep"] == 100.0 and rec[0]["layer"] == 2 and "density" not in rec[0]
    rows = probed[0]
    assert rows.numel() == 64 and rows.dtype == torch.int64 and not rows.is_cuda
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    o_s, lse_s = svg1_float64(qc, kc, vc, best1.cpu(), (0, 5, 160), WanP.block_mask.as_tuple())
    o_d, lse_d = SC.masked_attention_lse(qc[:, :, rows], kc, vc, None)
    assert torch.exp(lse_s[:, :, rows] - lse_d).mean() < 0.999          # the mask drops something on these rows
    check_record(rec[0], o_s[:, :, rows], lse_s[:, :, rows], o_d, lse_d, "wan svg1 host path")
    # fewer rows are fewer rows
    monkeypatch.setattr(WanP, "quality_rows", 5)
    run(WanP(2), (q, k, v, t))
    assert probed[1].numel() == 5 and len(lines(path)) == 2


def test_wan_svg1_device_switch_sparse_step_logs_dense_step_leaves_no_line(monkeypatch, tmp_path, probed):
    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanP

    q, k, v = wan_setup(monkeypatch, WanP)
    path = str(tmp_path / "q.jsonl")
    for ts, n_lines in ((100.0, 1), (950.0, 1)):                      # a sparse step, then a dense warm-up step
        t = torch.tensor([ts]).cuda()
        monkeypatch.setattr(WanP, "quality_log", None)
        out0, best0, rng0 = run(WanP(1), (q, k, v, t))
        monkeypatch.setattr(WanP, "quality_log", path)
        out1, best1, rng1 = run(WanP(1), (q, k, v, t))
        assert torch.equal(out0, out1) and torch.equal(best0, best1) and torch.equal(rng0, rng1)
        assert bool((best1 == -1).all()) == (ts > 900.0)
        assert len(lines(path)) == n_lines                           # the probe ran on both; the writer dropped the dense step's record
    assert len(probed) == 2
    rec = lines(path)[0]
    assert rec["timestep"] == 100.0 and rec["layer"] == 1           # the timestep travelled with the figures: no read-back on the host
    rows = probed[0]
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    monkeypatch.setattr(WanP, "quality_log", None)
    _, best, _ = run(WanP(1), (q, k, v, torch.tensor([100.0]).cuda()))
    o_s, lse_s = svg1_float64(qc, kc, vc, best.cpu(), (0, 5, 160), WanP.block_mask.as_tuple())
    o_d, lse_d = SC.masked_attention_lse(qc[:, :, rows], kc, vc, None)
    check_record(rec, o_s[:, :, rows], lse_s[:, :, rows], o_d, lse_d, "wan svg1 device switch")


def test_dense_mask_keeps_all_mass(monkeypatch, tmp_path, probed):
    """the sparse call under a mask that keeps every key: kept mass 1 within exp(2 (U + 1e-5 (1 + |lse|))) - 1, rel. L2 within merged_limit
    (the sparse output is rounded once)"""
    from svg import _native as nat
    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanP

    S = 800
    q, k, v = wan_setup(monkeypatch, WanP, block_mask=nat.BandMask(**O.dense_band_params(S)))
    path = str(tmp_path / "q.jsonl")
    monkeypatch.setattr(WanP, "quality_log", path)
    run(WanP(0), (q, k, v, torch.tensor([100.0])))
    rec = lines(path)[0]
    rows = probed[0]
    o_d, lse_d = SC.masked_attention_lse(q.cpu()[:, :, rows], k.cpu(), v.cpu(), None)
    kept, rel = torch.tensor(rec["kept_mass"]), torch.tensor(rec["rel_l2"])
    kb = math.exp(2 * lse_b(lse_d)) - 1
    lim = max(SC.merged_limit(o_d[0, h], DT)[0] for h in range(o_d.shape[1]))
    print(f"dense mask: kept_mass {kept.tolist()} (within {kb:.3e} of 1), rel_l2 {rel.tolist()} (limit {lim:.3e})")
    assert ((kept - 1).abs() <= kb).all() and (rel <= lim).all()


def test_per_video_lengths_are_probed_group_by_group(tmp_path, probed):
    """dense_attention with per-video valid lengths set against the probe with the same lengths: the probe's dense rows are the keys
    dense_attention gives them (two segments, another seam per video), one native call per group of videos"""
    from svg.models import _core

    g = torch.Generator().manual_seed(23)
    q, k, v = (torch.randn(3, 2, 790, 128, generator=g).to(DT).cuda() for _ in range(3))
    lens = (761, 761, 700)
    out, lse = _core.dense_attention(q, k, v, lens, return_lse=True)
    path = str(tmp_path / "q.jsonl")
    _core.reseed_probe_generator(5)
    _core.log_quality(_core.QualityRequest(path, 64, lens, 7.0, 4), out, lse, q, k, v)
    rec = lines(path)[0]
    assert len(probed) == 2 and int(probed[0].max()) < 761 and int(probed[1].max()) < 700
    kept, rel = torch.tensor(rec["kept_mass"]), torch.tensor(rec["rel_l2"])
    assert kept.shape == (3, 2) and rel.shape == (3, 2) and rec["timestep"] == 7.0 and rec["layer"] == 4
    kb = math.exp(2 * (SC.U[DT] + 1e-5 * (1 + float(lse[torch.isfinite(lse)].abs().max())))) - 1
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    lim = 0.0
    for sl, rows, vl in ((slice(0, 2), probed[0], 761), (slice(2, 3), probed[1], 700)):
        o_d, _ = SC.masked_attention_lse(qc[sl][:, :, rows], kc[sl][:, :, :vl], vc[sl][:, :, :vl], None)
        lim = max(lim, max(SC.merged_limit(o_d[c, h], DT)[0] for c in range(o_d.shape[0]) for h in range(2)))
    print(f"per-video lengths: kept_mass {kept.tolist()} (within {kb:.3e} of 1), rel_l2 {rel.tolist()} (limit {lim:.3e})")
    assert ((kept - 1).abs() <= kb).all() and (rel <= lim).all()


@pytest.mark.parametrize("switch", [False, True], ids=["host", "device_switch"])
def test_hunyuan_svg1_with_per_video_prompt_lengths(monkeypatch, tmp_path, probed, switch):
    """HunyuanVideo, two videos with prompts of different lengths (a mask and a valid length per video: the groups launch): output and
    best_mask_idx unchanged, one probe call per video over that video's valid rows, each video's figures against its own float64 statement"""
    from svg.models.hyvideo.attention import Hunyuan_SVGAttn_Processor2_0 as HyP
    from svg.models.hyvideo.utils import generate_temporal_head_mask_mod as hy_mm

    ctx, F_, P_, H, D, lens = 64, 5, 160, 2, 128, (21, 40)
    V = F_ * P_
    S = V + ctx
    masks = tuple(hy_mm(ctx, L, F_, P_, mul=1.2) for L in lens)
    for name, val in dict(context_length=ctx, num_frame=F_, frame_size=P_, prompt_length=lens, block_mask=masks, first_layers_fp=0,
                          first_times_fp=900.0, num_sampled_rows=16, sample_mse_max_row=V, quality_log=None, quality_rows=64).items():
        monkeypatch.setattr(HyP, name, val, raising=False)
    g = torch.Generator().manual_seed(31)
    q, k, v = (torch.randn(2, H, S, D, generator=g).to(DT).cuda() for _ in range(3))
    t = torch.tensor([100.0]).cuda() if switch else torch.tensor([100.0])
    out0, best0, rng0 = run(HyP(3), (q, k, v, t, 3, None))
    path = str(tmp_path / "q.jsonl")
    monkeypatch.setattr(HyP, "quality_log", path)
    out1, best1, rng1 = run(HyP(3), (q, k, v, t, 3, None))
    assert torch.equal(out0, out1) and torch.equal(best0, best1) and torch.equal(rng0, rng1)
    rec = lines(path)
    assert len(rec) == 1 and len(probed) == 2 and rec[0]["timestep"] == 100.0 and rec[0]["layer"] == 3
    qc, kc, vc, best = q.cpu(), k.cpu(), v.cpu(), best1.cpu()
    for b, (L, rows) in enumerate(zip(lens, probed)):
        valid = V + L
        assert int(rows.max()) < valid
        sl = slice(b, b + 1)
        o_s, lse_s = svg1_float64(qc[sl], kc[sl], vc[sl], best[sl], (ctx, F_, P_), masks[b].as_tuple())
        o_d, lse_d = SC.masked_attention_lse(qc[sl][:, :, rows], kc[sl][:, :, :valid], vc[sl][:, :, :valid], None)
        one = {key: [rec[0][key][b]] for key in ("rel_l2", "mse", "kept_mass")}
        check_record(one, o_s[:, :, rows], lse_s[:, :, rows], o_d, lse_d, f"hunyuan svg1 video {b} ({'device switch' if switch else 'host path'})")


def test_cog_logs_the_error_alone(monkeypatch, tmp_path, probed):
    """CogVideoX, head_dim 64: no LSE form of the launch — kept_mass null, the error against float64; output and best_mask_idx unchanged"""
    from svg.models.cog.attention import CogVideoX_SparseAttn_Processor2_0 as CogP
    from svg.models.cog.utils import generate_temporal_head_mask_mod as cog_mm

    ctx, F_, P_, H, D = 26, 4, 180, 2, 64
    for name, val in dict(context_length=ctx, num_frame=F_, frame_size=P_, first_layers_fp=0.0, first_times_fp=0.2, num_sampled_rows=16,
                          block_mask=cog_mm(ctx, F_, P_, mul=1.5), quality_log=None, quality_rows=64).items():
        monkeypatch.setattr(CogP, name, val, raising=False)
    S = ctx + F_ * P_
    g = torch.Generator().manual_seed(29)
    q, k, v = (torch.randn(2, H, S, D, generator=g).to(DT).cuda() for _ in range(3))
    t = torch.tensor([100.0])
    out0, best0, rng0 = run(CogP(0), (q, k, v, t))
    path = str(tmp_path / "q.jsonl")
    monkeypatch.setattr(CogP, "quality_log", path)
    out1, best1, rng1 = run(CogP(0), (q, k, v, t))
    assert torch.equal(out0, out1) and torch.equal(best0, best1) and torch.equal(rng0, rng1)
    rec = lines(path)
    assert len(rec) == 1 and rec[0]["kept_mass"] is None and list(rec[0]) == ["timestep", "layer", "rel_l2", "mse", "kept_mass"]
    rows = probed[0]
    qc, kc, vc = q.cpu(), k.cpu(), v.cpu()
    o_s, _ = svg1_float64(qc, kc, vc, best1.cpu(), (ctx, F_, P_), CogP.block_mask.as_tuple(), text_first=True)
    o_d, lse_d = SC.masked_attention_lse(qc[:, :, rows], kc, vc, None)
    check_record(rec[0], o_s[:, :, rows], None, o_d, lse_d, "cog")


def test_wan_svg2_logs_the_float64_figures_and_changes_nothing(monkeypatch, tmp_path, probed):
    """SVG2: the plan re-derived from the kernels' labels and block map as tests/test_gpu_processors.py does; S = 900 >= 160 block-rows,
    so the launch has its LSE form and the kept mass is logged, with the densities"""
    from svg.kmeans_utils import batch_kmeans_Euclid, density_calculation, identify_dynamic_map
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor as SapP

    H, D, F_, P_, QC, KC = 3, 128, 6, 150, 4, 12
    S = F_ * P_
    for name, val in dict(context_length=0, num_frame=F_, frame_size=P_, first_layers_fp=0, first_times_fp=900.0, num_q_centroids=QC,
                          num_k_centroids=KC, top_p_kmeans=0.6, min_kc_ratio=0.1, kmeans_iter_init=3, kmeans_iter_step=2,
                          zero_step_kmeans_init=False, logging_file=None, quality_log=None, quality_rows=64).items():
        monkeypatch.setattr(SapP, name, val, raising=False)
    gen = torch.Generator().manual_seed(3)
    q = _clustered(H, S, D, 12, gen)[None].to(DT).cuda()
    k = _clustered(H, S, D, 20, gen)[None].to(DT).cuda()
    v = torch.randn(1, H, S, D, generator=gen).to(DT).cuda()
    t = torch.tensor([100.0])

    def two_calls(proc):
        torch.manual_seed(11)
        with torch.no_grad():
            a = proc.attention_core_logic(q, k, v, t)
            cents = (proc.centroid_store.q[proc.layer_idx].clone(), proc.centroid_store.k[proc.layer_idx].clone())
            b = proc.attention_core_logic(q, k, v, t)
        return a, b, cents, torch.get_rng_state()

    a0, b0, _, rng0 = two_calls(SapP(5))
    path = str(tmp_path / "q.jsonl")
    monkeypatch.setattr(SapP, "quality_log", path)
    a1, b1, (qc0, kc0), rng1 = two_calls(SapP(5))
    assert torch.equal(a0, a1) and torch.equal(b0, b1) and torch.equal(rng0, rng1)
    rec = lines(path)
    assert len(rec) == 2 and len(probed) == 2 and all(r["layer"] == 5 and r["kept_mass"] is not None and "density" in r for r in rec)
    # the second, warm-started call in float64
    ql, qc, qs, _ = batch_kmeans_Euclid(q[0].contiguous(), QC, max_iters=2, init_centroids=qc0)
    kl, kc, ks, _ = batch_kmeans_Euclid(k[0].contiguous(), KC, max_iters=2, init_centroids=kc0)
    dmap = identify_dynamic_map(qc[None], kc[None], qs[None], ks[None], 0.6, 0.1)
    assert 0.05 < dmap.float().mean() < 0.95
    torch.testing.assert_close(torch.tensor(rec[1]["density"]), density_calculation(dmap, qs[None], ks[None]).float().cpu(), rtol=1e-5, atol=0)
    dmap, ql, kl = dmap[0].cpu(), ql.cpu(), kl.cpu()
    rows = probed[1]
    qh, kh, vh = q.cpu(), k.cpu(), v.cpu()
    o_s = torch.zeros(1, H, rows.numel(), D, dtype=torch.float64)
    lse_s = torch.zeros(1, H, rows.numel(), dtype=torch.float64)
    for h in range(H):
        em = dmap[h][ql[h]][:, kl[h]]                                       # [S, S] element mask of the head's plan
        o_s[0, h], lse_s[0, h] = SC.masked_attention_lse(qh[0, h, rows], kh[0, h], vh[0, h], em[rows])
    o_d, lse_d = SC.masked_attention_lse(qh[:, :, rows], kh, vh, None)
    assert torch.exp(lse_s - lse_d).mean() < 0.999
    check_record(rec[1], o_s, lse_s, o_d, lse_d, "wan svg2")
