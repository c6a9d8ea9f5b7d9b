"""SVG2's per-head top-p on the GPU (include/svg_attn_adaptive_top_p.h): the block map from a device vector of thresholds against the
scalar entry head by head, the K-only probe against svg_sample_dense_rows bit for bit and against float64, the controller kernel against
the float64 law (tests/adaptive_top_p_cases.py), and the loop closed in the Wan SAP processor.

Bounds, none of them from the code under test: maps and the probe's lse are compared for EQUALITY with the entries they restate; the lse
against float64 by check_lse; kept is fp64 arithmetic rounded once to fp32 — the float64 statement rounded to fp32 can differ by the one
rounding (exp and a sum of <= 64 terms in fp64 carry ~1e-15): 1 fp32 ulp; the step is fp32 — e = target - kept rounds once (|e| < 0.5
here: <= 2^-26), e + band on the slow side once more (scaled by gain_down <= 1/2), the products are exact (the tests' gains are powers
of two), and the sum rounds once (half an ulp of the result, which is >= p_min >= 0.1) — 2 fp32 ulp of the result beside the float64
law on the device's own kept, the law given the parameters as the ABI's floats carry them (AC.params32); the processor's kept mass
against float64 by the bound of tests/test_gpu_quality_probe.py."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import adaptive_top_p_cases as AC
import kept_mass_cases as KM
import sparse_lse_cases as SC
from poisoned import load_native, unwritten
from test_gpu_processors import _clustered
from test_gpu_sample_rows import VALID, inputs, reference, rows_for

pytestmark = pytest.mark.gpu
DT = torch.bfloat16


@pytest.fixture(scope="module")
def nat():
    return load_native()


# ---------------------------------------------------------------------------------------------------------
# the per-head map
# ---------------------------------------------------------------------------------------------------------
BH = 5
P_HEADS = [0.0, 1.0, 0.6, 0.6005, 0.35]          # 0.6 and 0.6005 round to the same bf16 (0.6015625)


@functools.lru_cache(maxsize=None)
def centroids(QC, KC, D, dtype):
    g = torch.Generator().manual_seed(QC * 31 + KC * 7 + D)
    qc = (torch.randn(BH, QC, D, generator=g) * 1.2).to(dtype).cuda()
    kc = (torch.randn(BH, KC, D, generator=g) * 1.2).to(dtype).cuda()
    ks = torch.randint(0, 90, (BH, KC), generator=g, dtype=torch.int32).cuda()      # (empty clusters included)
    return qc, kc, ks


def per_head(nat, qc, kc, ks, p, preserve):
    out = nat.empty((qc.shape[0], qc.shape[1], kc.shape[1]), dtype=torch.uint8, device=qc.device)
    m = nat.identify_dynamic_map_per_head(qc, kc, ks, torch.tensor(p, dtype=torch.float32).cuda(), preserve, out)
    assert int(out.max()) <= 1, "bytes of the map left unwritten (poisoned: 255)"
    return m


@pytest.mark.parametrize("preserve", [0, 3])
@pytest.mark.parametrize("D,dtype", [(128, torch.bfloat16), (64, torch.float16)], ids=["D128-bf16", "D64-fp16"])
@pytest.mark.parametrize("KC", [12, 300, 1100])
@pytest.mark.parametrize("QC", [4, 20])
def test_per_head_map_is_the_scalar_map_of_every_head(nat, QC, KC, D, dtype, preserve):
    qc, kc, ks = centroids(QC, KC, D, dtype)
    assert float(torch.tensor(0.6).to(torch.bfloat16)) == float(torch.tensor(0.6005).to(torch.bfloat16))
    m = per_head(nat, qc, kc, ks, P_HEADS, preserve)
    alone = [nat.identify_dynamic_map(qc[h:h + 1], kc[h:h + 1], ks[h:h + 1], P_HEADS[h], preserve)[0] for h in range(BH)]
    for h in range(BH):
        assert torch.equal(m[h], alone[h]), (h, P_HEADS[h])
    assert bool((m[0].sum(-1) == max(1, preserve)).all())                            # p = 0: the first block of a row (and the preserved)
    assert 0 < int(m[4].sum()) < m[4].numel()
    # a uniform tensor: the scalar call
    assert torch.equal(per_head(nat, qc, kc, ks, [0.6] * BH, preserve), nat.identify_dynamic_map(qc, kc, ks, 0.6, preserve))
    # one head's p raised: only that head's map changes, to a superset
    raised = list(P_HEADS)
    raised[4] = 0.9
    m2 = per_head(nat, qc, kc, ks, raised, preserve)
    assert torch.equal(m2[:4], m[:4]) and bool((m[4] <= m2[4]).all())
    if KC >= 300:
        assert int(m2[4].sum()) > int(m[4].sum())


def test_a_nan_threshold_keeps_every_block_and_kmeans_utils_routes_a_tensor(nat):
    from svg import kmeans_utils

    qc, kc, ks = centroids(20, 300, 128, torch.bfloat16)
    p = [0.3, float("nan"), 0.3, 0.3, 0.3]
    m = per_head(nat, qc, kc, ks, p, 0)
    assert bool(m[1].all()) and not bool(m[0].all())
    # svg.kmeans_utils.identify_dynamic_map: [B, H] tensor -> the per-head entry, a float -> the path it had
    t = torch.tensor(P_HEADS, dtype=torch.float32).cuda().view(1, BH)
    via = kmeans_utils.identify_dynamic_map(qc[None], kc[None], None, ks[None], t, 0.01)
    assert via.shape == (1, BH, 20, 300) and torch.equal(via[0], per_head(nat, qc, kc, ks, P_HEADS, 3))
    assert torch.equal(kmeans_utils.identify_dynamic_map(qc[None], kc[None], None, ks[None], 0.6, 0.01)[0],
                       nat.identify_dynamic_map(qc, kc, ks, 0.6, 3))


# ---------------------------------------------------------------------------------------------------------
# the K-only probe
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("valid_len", [0, VALID])
@pytest.mark.parametrize("R", [1, 17, 64])
@pytest.mark.parametrize("dtype", SC.DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("BH_", [1, 3])
@pytest.mark.parametrize("S", [70, 790, 4100])
def test_sample_dense_lse_has_the_bits_of_sample_dense_rows(nat, S, BH_, D, dtype, R, valid_len):
    from svg import _probe

    q, k, v = inputs(S, BH_, D, dtype)
    rows = rows_for(S, R)
    _, ref_lse = reference(q, k, v, rows, valid_len)
    qd, kd, vd = (x.cuda() for x in (q, k, v))
    what = f"S={S} BH={BH_} D={D} {dtype} R={R} valid_len={valid_len}"
    lse = _probe.sample_dense_lse(qd, kd, torch.tensor(rows), valid_len=valid_len)
    assert lse.shape == (1, BH_, R) and lse.dtype == torch.float32 and not unwritten(lse).any() and torch.isfinite(lse).all(), what
    _, lse_rows = _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows), valid_len=valid_len)
    assert torch.equal(lse, lse_rows), (what, (lse - lse_rows).abs().max())
    SC.check_lse(lse, ref_lse, dtype, what)
    perm = torch.randperm(R, generator=torch.Generator().manual_seed(R))
    lse2 = _probe.sample_dense_lse(qd, kd, torch.tensor(rows)[perm].cuda(), valid_len=valid_len)
    assert torch.equal(lse2, lse[:, :, perm.cuda()]), what


def test_sample_dense_lse_reads_token_major_views_in_place(nat):
    from svg import _probe

    cfg, H, S, R, D = 2, 3, 790, 17, 128
    g = torch.Generator().manual_seed(11 + D)
    store = [torch.randn(cfg, S, H, D, generator=g).to(DT) for _ in range(3)]
    rows = rows_for(S, R)
    q, k, v = (x.permute(0, 2, 1, 3) for x in store)
    _, ref_lse = reference(q, k, v, rows, VALID)
    qd, kd, vd = (x.cuda().permute(0, 2, 1, 3) for x in store)
    assert not qd.is_contiguous() and nat._strided_ok(qd) and nat._strided_ok(kd, True)
    lse = _probe.sample_dense_lse(qd, kd, torch.tensor(rows), valid_len=VALID)
    assert lse.shape == (cfg, H, R) and lse.is_contiguous() and not unwritten(lse).any()
    SC.check_lse(lse, ref_lse, DT, "token-major")
    assert torch.equal(lse, _probe.sample_dense_lse(qd.contiguous(), kd.contiguous(), torch.tensor(rows), valid_len=VALID))
    assert torch.equal(lse, _probe.sample_dense_rows(qd, kd, vd, torch.tensor(rows), valid_len=VALID)[1])


# ---------------------------------------------------------------------------------------------------------
# the update kernel
# ---------------------------------------------------------------------------------------------------------
LAW = dict(target=0.8, gain_up=1.0, gain_down=0.5, band=0.02, p_min=0.2, p_max=0.9)


@pytest.mark.parametrize("R", [1, 17, 64])
def test_top_p_update_against_the_float64_law(nat, R):
    BHu, S = 7, 300

    def delta(g):
        d = torch.rand(BHu, R, generator=g)                     # lse_dense - lse_sparse >= 0: a kept mass in (1 / e, 1]
        d[0] = 5.0                                              # head 0 keeps < 1 %: far below target, driven to p_max
        d[1] = 0.0                                              # head 1 keeps everything: far above the band, driven to p_min
        return d

    rows, ls, ld = KM.controller_inputs(100 + R, BHu, S, R, delta)      # (head 2: a -inf row, head 3: NaN)
    p0 = torch.tensor([0.5, 0.25, 0.3, 0.77, 0.9, 0.2, 0.61])

    def run():
        p = p0.clone().cuda()
        kept = nat.empty((BHu,), dtype=torch.float32, device="cuda")
        nat.top_p_update(ls.cuda(), torch.tensor(rows).cuda(), ld.cuda(), p, kept, LAW["target"], LAW["gain_up"], LAW["gain_down"],
                         LAW["band"], LAW["p_min"], LAW["p_max"])
        return kept.cpu(), p.cpu()

    kept, p = run()
    fin = [h for h in range(BHu) if h != 3]
    assert math.isnan(float(kept[3])) and torch.isfinite(kept[fin]).all(), kept          # every word written (poisoned: NaN)
    ref_kept = AC.kept_mass(ls.numpy(), rows, ld.numpy())
    assert np.isnan(ref_kept[3])
    uk = AC.ulps32(kept.numpy()[fin], ref_kept[fin].astype(np.float32))
    print(f"R={R} kept {kept.tolist()} float64 {ref_kept.tolist()} ulps {uk.tolist()}")
    assert (uk <= 1).all()
    if R == 1:
        assert float(kept[2]) == 0.0                                                     # the -inf row added nothing
    ref_p = AC.law(p0.numpy(), kept.numpy(), **AC.params32(LAW))
    up = AC.ulps32(p.numpy(), ref_p.astype(np.float32))
    print(f"R={R} top_p {p.tolist()} float64 law {ref_p.tolist()} ulps {up.tolist()}")
    assert (up <= 2).all()
    assert float(p[0]) == np.float32(LAW["p_max"]) and float(p[1]) == np.float32(LAW["p_min"])     # both clamps reached
    assert float(p[3]) == float(p0[3])                                                                 # the NaN head: unchanged
    kept2, p2 = run()                                                                                  # the same call: the same bits
    assert torch.equal(kept2.view(torch.int32), kept.view(torch.int32)) and torch.equal(p2, p)


# ---------------------------------------------------------------------------------------------------------
# the Wan SAP processor
# ---------------------------------------------------------------------------------------------------------
H, D, F_, P_, QC, KC = 3, 128, 6, 150, 4, 12
S = F_ * P_


def lse_b(lse):
    return float(SC.lse_bound(lse[torch.isfinite(lse)], DT).max())


@pytest.fixture
def sap(monkeypatch):
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor as SapP

    for name, val in dict(context_length=0, num_frame=F_, frame_size=P_, first_layers_fp=0, first_times_fp=900.0, num_q_centroids=QC,
                          num_k_centroids=KC, top_p_kmeans=0.6, min_kc_ratio=0.1, kmeans_iter_init=3, kmeans_iter_step=2,
                          zero_step_kmeans_init=False, logging_file=None, quality_log=None, quality_rows=64, adaptive_top_p=None).items():
        monkeypatch.setattr(SapP, name, val, raising=False)
    gen = torch.Generator().manual_seed(3)
    q = _clustered(H, S, D, 12, gen)[None].to(DT).cuda()
    k = _clustered(H, S, D, 20, gen)[None].to(DT).cuda()
    v = torch.randn(1, H, S, D, generator=gen).to(DT).cuda()
    return SapP, (q, k, v, torch.tensor([100.0]))


def three_calls(proc, args, before=None):
    from svg.models import _core

    torch.manual_seed(11)
    _core.reseed_probe_generator(11)
    outs, cents = [], []
    with torch.no_grad():
        for i in range(3):
            if before is not None:
                before(i, proc)
            outs.append(proc.attention_core_logic(*args))
            cents.append((proc.centroid_store.q[proc.layer_idx].clone(), proc.centroid_store.k[proc.layer_idx].clone()))
    return outs, cents, torch.get_rng_state()


def test_zero_gains_measure_and_change_nothing(nat, sap):
    from svg.models import _core

    SapP, args = sap
    outs0, cents0, rng0 = three_calls(SapP(5), args)
    SapP.adaptive_top_p = _core.AdaptiveTopP(0.999, gain_up=0.0, gain_down=0.0)
    proc = SapP(5)
    outs1, cents1, rng1 = three_calls(proc, args)
    for a, b in zip(outs0, outs1):
        assert torch.equal(a, b)
    for (qa, ka), (qb, kb) in zip(cents0, cents1):
        assert torch.equal(qa, qb) and torch.equal(ka, kb)
    assert torch.equal(rng0, rng1)
    kept, p = proc.top_p_store.kept[5], proc.top_p_store.p[5]
    assert kept.shape == (H,) and kept.dtype == torch.float32 and bool(((kept > 0) & (kept <= 1 + 1e-4)).all()), kept
    assert p.tolist() == [pytest.approx(0.6)] * H
    proc.reset_state()
    assert not proc.top_p_store.has(5) and not proc.centroid_store.has(5)


@pytest.mark.parametrize("gain_up", [4.0, 0.5], ids=["gain4", "gain0.5"])     # 4: one step reaches p_max; 0.5: thresholds in between
def test_the_loop_steers_every_head_by_the_law(nat, sap, monkeypatch, gain_up):
    from svg.kmeans_utils import batch_kmeans_Euclid, identify_dynamic_map
    from svg.models import _core

    SapP, args = sap
    q, k, v, _ = args
    law = dict(target=0.999, gain_up=gain_up, gain_down=0.25, band=0.02, p_min=0.1, p_max=1.0)
    SapP.adaptive_top_p = _core.AdaptiveTopP(law["target"], gain_up=law["gain_up"])
    plans, orig_plan = [], _core.probe_plan
    monkeypatch.setattr(_core, "probe_plan", lambda *a, **kw: plans.append(orig_plan(*a, **kw)) or plans[-1])
    maps, orig_map = [], _core.identify_dynamic_map

    def spy_map(qc, kc, qs, ks, p, ratio):
        m = orig_map(qc, kc, qs, ks, p, ratio)
        maps.append((qc.clone(), kc.clone(), ks.clone(), p.clone(), ratio, m.clone()))
        return m

    monkeypatch.setattr(_core, "identify_dynamic_map", spy_map)
    proc = SapP(5)
    state = []                                                   # (centroids, thresholds) in front of every call

    def before(i, proc):
        st = proc.centroid_store
        state.append(None if i == 0 else (st.q[5].clone(), st.k[5].clone()))

    trace = []
    orig_step = _core.adaptive_step

    def spy_step(adaptive, store, layer, p, *a, **kw):
        p_before = p.clone()
        orig_step(adaptive, store, layer, p, *a, **kw)
        trace.append((p_before.cpu(), store.kept[layer].cpu().clone(), p.cpu().clone()))

    monkeypatch.setattr(_core, "adaptive_step", spy_step)
    three_calls(proc, args, before)
    assert len(trace) == 3 and len(maps) == 3 and len(plans) == 3
    assert trace[0][0].tolist() == [pytest.approx(0.6)] * H                                   # the first call runs with the scalar
    below = trace[0][1] < law["target"]
    assert bool(below.any()), "precondition: at least one head starts below the target"
    qh, kh, vh = q.cpu(), k.cpu(), v.cpu()
    for i, (p_before, kept, p_after) in enumerate(trace):
        # the map the call used: head by head the scalar function's map at the head's p
        qc, kc, ks, p_used, ratio, m = maps[i]
        assert torch.equal(p_used.reshape(-1).cpu(), p_before) and ratio == 0.1
        for h in range(H):
            alone = identify_dynamic_map(qc[:, h:h + 1], kc[:, h:h + 1], None, ks[:, h:h + 1], float(p_before[h]), ratio)
            assert torch.equal(m[:, h:h + 1], alone), (i, h)
        # the state after the call: the law on the call's own kept mass
        up = AC.ulps32(p_after.numpy(), AC.law(p_before.numpy(), kept.numpy(), **AC.params32(law)).astype(np.float32))
        print(f"call {i}: top_p {p_before.tolist()} kept {kept.tolist()} -> {p_after.tolist()} (ulps from the law {up.tolist()})")
        assert (up <= 2).all()
        if i > 0:
            assert torch.equal(p_before, trace[i - 1][2])                                     # the state carries from call to call
        if i == 0:
            continue
        # the kept mass in float64, the plan re-derived from the kernels' labels (warm start from the centroids in front of the call)
        ql, qc2, qs2, _ = batch_kmeans_Euclid(q[0].contiguous(), QC, max_iters=2, init_centroids=state[i][0])
        kl, kc2, ks2, _ = batch_kmeans_Euclid(k[0].contiguous(), KC, max_iters=2, init_centroids=state[i][1])
        dmap = identify_dynamic_map(qc2[None], kc2[None], qs2[None], ks2[None], p_before.cuda().view(1, H), 0.1)
        assert torch.equal(dmap, m)
        dmap, ql, kl = dmap[0].cpu(), ql.cpu(), kl.cpu()
        (_, vl, rows), = plans[i]
        assert vl is None and rows.numel() == 64
        lse_s = torch.zeros(1, H, rows.numel(), dtype=torch.float64)
        for h in range(H):
            em = dmap[h][ql[h]][:, kl[h]]
            _, lse_s[0, h] = SC.masked_attention_lse(qh[0, h, rows], kh[0, h], vh[0, h], em[rows])
        _, lse_d = SC.masked_attention_lse(qh[:, :, rows], kh, vh, None)
        ref = torch.exp(lse_s - lse_d).mean(-1)[0]
        ktol = ref * (math.exp(2 * max(lse_b(lse_s), lse_b(lse_d))) - 1)
        print(f"call {i}: kept {kept.tolist()} float64 {ref.tolist()} tolerance {ktol.tolist()}")
        assert ((kept.double() - ref).abs() <= ktol).all()
    p_end = trace[-1][2]
    assert bool(((p_end > trace[0][0]) | (p_end == law["p_max"]))[below].all()), (trace[0], p_end)


def test_quality_log_and_the_controller_share_one_probe(nat, sap, monkeypatch, tmp_path):
    import json

    from svg import _probe
    from svg.models import _core

    SapP, args = sap
    calls = {"rows": 0, "lse": 0}
    orig_rows, orig_lse = _probe.sample_dense_rows, _probe.sample_dense_lse
    monkeypatch.setattr(_probe, "sample_dense_rows", lambda *a, **kw: calls.__setitem__("rows", calls["rows"] + 1) or orig_rows(*a, **kw))
    monkeypatch.setattr(_probe, "sample_dense_lse", lambda *a, **kw: calls.__setitem__("lse", calls["lse"] + 1) or orig_lse(*a, **kw))
    SapP.adaptive_top_p = _core.AdaptiveTopP(0.999, gain_up=4.0)
    outs_a, _, _ = three_calls(SapP(5), args)
    assert calls == {"rows": 0, "lse": 3}
    path = str(tmp_path / "q.jsonl")
    SapP.quality_log = path
    proc = SapP(5)
    outs_b, _, _ = three_calls(proc, args)
    assert calls == {"rows": 3, "lse": 3}                                # one probe per call: the log's, fed to the controller as well
    for a, b in zip(outs_a, outs_b):
        assert torch.equal(a, b)                                         # the same rows, the same lse bits: the same trajectory
    _core.flush_quality_log()
    rec = [json.loads(x) for x in open(path)]
    assert len(rec) == 3 and rec[0]["top_p"] == [[pytest.approx(0.6)] * H] and all("top_p" in r and r["kept_mass"] is not None for r in rec)
    assert rec[2]["top_p"][0] != rec[0]["top_p"][0]
    torch.testing.assert_close(torch.tensor(rec[2]["kept_mass"][0]), proc.top_p_store.kept[5].cpu(), rtol=1e-5, atol=0)
    # without the option the record has no such list
    SapP.adaptive_top_p = None
    path2 = str(tmp_path / "q2.jsonl")
    SapP.quality_log = path2
    three_calls(SapP(5), args)
    _core.flush_quality_log()
    assert all("top_p" not in json.loads(x) for x in open(path2))


def test_dense_warm_up_steps_leave_the_state_alone(nat, sap):
    from svg.models import _core

    SapP, args = sap
    SapP.adaptive_top_p = _core.AdaptiveTopP(0.999)
    proc = SapP(5)
    with torch.no_grad():
        proc.attention_core_logic(*args[:3], torch.tensor([950.0]))      # timestep above first_times_fp: dense
    assert not proc.top_p_store.p and not proc.top_p_store.kept


def test_refusals(nat, sap):
    import torch.distributed as dist

    from svg import distributed as sd
    from svg.models import _core

    SapP, args = sap
    SapP.adaptive_top_p = _core.AdaptiveTopP(0.95)
    q64 = torch.zeros(1, H, S, 64, dtype=DT, device="cuda")
    proc = SapP(5)
    with pytest.raises(ValueError, match="head_dim 128"):
        proc.attention_core_logic(q64, q64, q64, args[3])
    assert not proc.centroid_store.q and not proc.top_p_store.p          # before anything ran
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{38500 + os.getpid() % 2000}", rank=0, world_size=1)
    try:
        sd.enable()
        with pytest.raises(NotImplementedError, match="adaptive_top_p"):
            proc.attention_core_logic(*args)
    finally:
        sd.disable()
        dist.destroy_process_group()
