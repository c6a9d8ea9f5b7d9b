"""SVG2 on a batch of videos, the parts that run without a GPU: the torch statement of the Lloyd loop with one stopping rule per group
(svg.kmeans_utils.lloyd_device_rule, driven by the oracle's iteration), its head-sharded form over gloo, the block-map post-processing at
cfg = 2, the CentroidStore batch-size rule and the density-log entries."""
import json
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import svg_oracle as O

ROOT = Path(__file__).resolve().parent.parent


def _step_fn(x):
    """one Lloyd iteration of the oracle on x [B, N, D] in the form lloyd_device_rule takes (per-batch shift)"""
    xsq = O.kmeans_xsq(x)

    def step(cur, it):
        labels = O.kmeans_assign(x, xsq, cur)
        c_new, counts = O.kmeans_update(x, labels, cur)
        shift = (c_new.float() - cur.float()).norm(dim=-1).amax(dim=1)
        return c_new, labels.to(torch.int32), counts, O.stable_argsort(labels).to(torch.int32), shift

    return step


def _data(B, N, D, gen, modes=6):
    centers = torch.randn(B, modes, D, generator=gen) * 2.0
    lab = torch.randint(0, modes, (B, N), generator=gen)
    return (torch.gather(centers, 1, lab[..., None].expand(-1, -1, D)) + 0.3 * torch.randn(B, N, D, generator=gen)).to(torch.bfloat16)


@pytest.mark.parametrize("check_every", [0, 1, 3])
def test_grouped_rule_equals_per_group_runs(check_every):
    from svg.kmeans_utils import lloyd_device_rule

    gen = torch.Generator().manual_seed(2)
    H, N, D, K, iters, tol = 3, 400, 32, 6, 15, 1e-3
    xs = [_data(H, N, D, gen), torch.randn(H, N, D, generator=gen).to(torch.bfloat16), _data(H, N, D, gen)]
    xs[2][1, 5, 3] = float("nan")   # a NaN in group 2: its shift is NaN, it never converges
    x = torch.cat(xs)
    init = x[:, :K].clone()
    init[2 * H + 1] = x[2 * H + 1, 10:10 + K]   # (the NaN row is not an initial centroid of its own)
    lab, cent, cnt, srt, n = lloyd_device_rule(_step_fn(x), init, iters, tol, group=H, check_every=check_every)
    assert n.shape == (3,)
    for g in range(3):
        sl = slice(g * H, (g + 1) * H)
        l1, c1, k1, s1, n1 = lloyd_device_rule(_step_fn(x[sl]), init[sl], iters, tol)
        assert n1.shape == ()
        assert torch.equal(lab[sl], l1) and torch.equal(cnt[sl], k1) and torch.equal(srt[sl], s1) and int(n[g]) == int(n1)
        assert torch.equal(cent[sl].view(torch.int16), c1.view(torch.int16))   # (bitwise: NaN centroids included)
        if g != 2:   # the reference's loop (oracle) on that group alone
            rl, rc, rk, rit = O.batch_kmeans_euclid(x[sl], K, max_iters=iters, tol=tol, init_centroids=init[sl])
            assert torch.equal(lab[sl], rl.to(torch.int32)) and torch.equal(cent[sl], rc) and torch.equal(cnt[sl], rk) and int(n[g]) == rit
    assert int(n[2]) == iters and int(n[0]) < iters
    # one group over all batches is the ungrouped rule; it is not the per-group one here (group 0 runs on with the others)
    _, _, _, _, n_all = lloyd_device_rule(_step_fn(x), init, iters, tol)
    _, _, _, _, n_one = lloyd_device_rule(_step_fn(x), init, iters, tol, group=3 * H)
    assert int(n_all) == int(n_one[0]) == iters != int(n[0])


def _sharded_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    sys.path.insert(0, str(ROOT / "sparse-videogen_amd"))
    sys.path.insert(0, str(ROOT))
    from svg.distributed import shard_heads
    from svg.kmeans_utils import lloyd_device_rule

    dist.init_process_group("gloo", rank=rank, world_size=world)
    gen = torch.Generator().manual_seed(4)
    cfg, H, N, D, K, iters, tol = 2, 5, 300, 32, 5, 12, 1e-3
    x = torch.cat([_data(H, N, D, gen), torch.randn(H, N, D, generator=gen).to(torch.bfloat16)])   # video 0 converges, video 1 does not
    init = x[:, :K].clone()
    full = lloyd_device_rule(_step_fn(x), init, iters, tol, group=H)
    mine = shard_heads(H, rank, world)
    rows = torch.tensor([c * H + h for c in range(cfg) for h in mine])

    def red(t):
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t

    part = lloyd_device_rule(_step_fn(x[rows]), init[rows], iters, tol, group=len(mine), shift_reduce=red)
    ok = all(torch.equal(a[rows], b) for a, b in zip(full[:4], part[:4])) and torch.equal(full[4], part[4])
    ok &= int(full[4][0]) < iters == int(full[4][1])
    ret[rank] = bool(ok)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_grouped_rule_gloo(world):
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 31500 + (os.getpid() % 2000) + world
    mp.spawn(_sharded_worker, args=(world, port, ret), nprocs=world, join=True)
    assert dict(ret) == {r: True for r in range(world)}


def test_dynamic_map_post_processing_cfg2_equals_per_video():
    from svg.models._core import dynamic_map_post_processing

    gen = torch.Generator().manual_seed(1)
    cfg, H, QC, KC, V, ctx, L = 2, 3, 5, 7, 60, 16, 6
    dmap = torch.rand(cfg, H, QC, KC, generator=gen) > 0.5
    qs = torch.randint(1, 20, (cfg, H, QC), generator=gen, dtype=torch.int32)
    ks = torch.randint(1, 20, (cfg, H, KC), generator=gen, dtype=torch.int32)
    qi = torch.stack([torch.randperm(V, generator=gen) for _ in range(cfg * H)]).to(torch.int32)
    ki = torch.stack([torch.randperm(V, generator=gen) for _ in range(cfg * H)]).to(torch.int32)
    out = dynamic_map_post_processing(dmap, qs, ks, qi, ki, V, ctx, L)
    for c in range(cfg):
        hs = slice(c * H, (c + 1) * H)
        one = dynamic_map_post_processing(dmap[c:c + 1], qs[c:c + 1], ks[c:c + 1], qi[hs], ki[hs], V, ctx, L)
        for a, b in zip(out[:3], one[:3]):
            assert torch.equal(a[c:c + 1], b)
        for a, b in zip(out[3:], one[3:]):
            assert torch.equal(a[hs], b)
    assert out[0].shape == (cfg, H, QC + 2, KC + 2) and out[3].shape == (cfg * H, V + ctx)


def test_centroid_store_batch_size_rule(monkeypatch):
    """a layer called with another cfg than its stored centroids is a first call: random initial points, iter_init iterations"""
    from svg.models import _core

    calls = []

    def fake_kmeans(x, K, max_iters, init_centroids, **kw):   # records what kmeans_clustering asks for
        calls.append((x.shape[0], max_iters, init_centroids, kw.get("group")))
        B, N, D = x.shape
        c = init_centroids if init_centroids is not None else x[:, :K].contiguous()
        return (torch.zeros(B, N, dtype=torch.int64), c.reshape(B, K, D).clone(), torch.zeros(B, K, dtype=torch.int32),
                torch.zeros(()), torch.zeros(B, N, dtype=torch.int32))

    monkeypatch.setattr(_core, "batch_kmeans_Euclid", fake_kmeans)
    st = _core.CentroidStore()
    H, N, D = 2, 40, 8
    x1, x2 = torch.randn(1, H, N, D), torch.randn(2, H, N, D)
    assert not st.has(0)
    _core.kmeans_clustering(st, 0, x1, x1, 3, 4, 50, 2)
    assert st.has(0) and st.has(0, 1) and not st.has(0, 2) and st.cfg[0] == 1
    _core.kmeans_clustering(st, 0, x1, x1, 3, 4, 50, 2)                      # same cfg: warm start
    _core.kmeans_clustering(st, 0, x2, x2, 3, 4, 50, 2)                      # another cfg: a first call
    _core.kmeans_clustering(st, 0, x2, x2, 3, 4, 50, 2)                      # ... then warm starts at that cfg
    assert [(b, it, g) for b, it, _, g in calls] == [(2, 50, None), (2, 50, None), (2, 2, None), (2, 2, None), (4, 50, H), (4, 50, H),
                                                     (4, 2, H), (4, 2, H)]
    assert calls[0][2] is None and calls[2][2] is not None
    assert calls[4][2] is not None and calls[4][2].shape == (2 * H, 3, D)    # drawn video by video from the batch's own tokens
    assert calls[6][2].shape == (2 * H, 3, D) and st.q[0].shape == (2 * H, 3, D) and st.cfg[0] == 2
    st.clear()
    assert not st.has(0) and st.cfg == {}
    # centroids written into the dicts directly: their shape [cfg * H, K, D] tells the batch size
    st.q[0], st.k[0] = torch.randn(H, 3, D), torch.randn(H, 4, D)
    assert st.has(0, 1, H) and not st.has(0, 2, H)
    calls.clear()
    _core.kmeans_clustering(st, 0, x1, x1, 3, 4, 50, 2)
    assert [(b, it) for b, it, _, _ in calls] == [(2, 2), (2, 2)]


def test_density_log_entries(tmp_path):
    from svg.models._core import _DensityLog

    log = _DensityLog()
    p = tmp_path / "d.jsonl"
    d1 = torch.tensor([[0.25, 0.5, 0.125]])
    d2 = torch.tensor([[0.25, 0.5, 0.125], [0.75, 1.0, 0.5]])
    log.push(str(p), {"timestep": 500.0, "layer": 7}, d1)
    log.push(str(p), {"timestep": 500.0, "layer": 8}, d2)
    log.flush()
    l1, l2 = p.read_text().splitlines()
    # cfg == 1: the entry of a single video, byte for byte
    assert l1 == json.dumps({"timestep": 500.0, "layer": 7, "avg_density": float(d1.mean()), "density": d1.tolist()})
    e2 = json.loads(l2)
    assert e2["density"] == d2.tolist() and e2["avg_density"] == float(d2.mean())
    assert e2["video_avg_density"] == [float(d2[0].mean()), float(d2[1].mean())]
