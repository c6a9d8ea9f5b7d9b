#!/usr/bin/env python3
"""SVG2 layer-call on a batch of videos: the time of one warm-started layer-call (2 k-means iterations on q and k, block map,
variable-block attention) at cfg = 1 and cfg = 2, same process, same workloads as bench_svg2.py, split by stage.

    python tools/bench_svg2_batch.py [--workload wan720p|hy720p|all] [--steps K] [--warmup W]

Prints one JSON line per workload: the median stage times (ms) at each cfg, the cfg = 2 / cfg = 1 ratio of the totals and the
per-video k-means iteration counts of the last timed call (cfg = 2 runs one stopping rule per video)."""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "sparse-videogen_amd"))
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from bench_svg2 import WORKLOADS, clustered  # noqa: E402


def layer_call(workload, cfg, steps, warmup):
    from svg import _native as nat
    from svg.kmeans_utils import identify_dynamic_map
    from svg.models import _core

    dev = torch.device("cuda", 0)
    H, D, F_, P_, ctx, L, QC, KC = WORKLOADS[workload]
    V = F_ * P_
    S = V + ctx
    gen = torch.Generator(device=dev).manual_seed(0)
    q = clustered(cfg * H, S, D, 64, dev, gen).view(cfg, H, S, D)
    k = clustered(cfg * H, S, D, 64, dev, gen).view(cfg, H, S, D)
    v = torch.randn(cfg, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    geo = _core.Geometry(ctx, F_, P_)
    store = _core.CentroidStore()
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    qv, kv = (q[:, :, :V], k[:, :, :V]) if ctx else (q, k)
    _core.kmeans_clustering(store, 0, qv, kv, QC, KC, 50, 2)   # the first call of the layer (50 iterations from random points)
    torch.cuda.synchronize()
    times = {"kmeans_2it_qk": [], "identify_map": [], "attention": [], "total": []}
    iters = None
    for it in range(warmup + steps):
        t = [ev() for _ in range(4)]
        t[0].record()
        (ql, qc, qs, qit, qidx), (kl, kc, ks, kit, kidx) = _core.kmeans_clustering(store, 0, qv, kv, QC, KC, 50, 2)
        t[1].record()
        q_sizes, k_sizes = qs.view(cfg, H, QC), ks.view(cfg, H, KC)
        dmap = identify_dynamic_map(qc.view(cfg, H, QC, D), kc.view(cfg, H, KC, D), q_sizes, k_sizes, 0.9, 0.1)
        if ctx:
            dmap, q_sizes, k_sizes, qidx, kidx = _core.dynamic_map_post_processing(dmap, q_sizes, k_sizes, qidx, kidx, V, ctx, L)
        t[2].record()
        QB, KB = q_sizes.shape[-1], k_sizes.shape[-1]
        # (what svg2_sparse_attention runs: one launch over cfg * H heads, output stored token-major [cfg, S, H, D])
        o = nat.varblock_attention(q, k, v, dmap.view(cfg * H, QB, KB).contiguous(), q_sizes.view(cfg * H, QB).contiguous(),
                                   k_sizes.view(cfg * H, KB).contiguous(), q_row_idx=qidx.contiguous(), kv_row_idx=kidx.contiguous(),
                                   token_major_out=_core.TOKEN_MAJOR_IO, rows_covered=True)
        t[3].record()
        torch.cuda.synchronize()
        if it >= warmup:
            times["kmeans_2it_qk"].append(t[0].elapsed_time(t[1]))
            times["identify_map"].append(t[1].elapsed_time(t[2]))
            times["attention"].append(t[2].elapsed_time(t[3]))
            times["total"].append(t[0].elapsed_time(t[3]))
        iters = {"q": [int(n) for n in qit.reshape(-1).tolist()], "k": [int(n) for n in kit.reshape(-1).tolist()]}
    assert torch.isfinite(o.float()).all()
    del q, k, v, o
    torch.cuda.empty_cache()
    return {key: round(statistics.median(val), 3) for key, val in times.items()}, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=sorted(WORKLOADS) + ["all"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from svg import _native as nat

    nat.load()
    names = ["wan720p", "hy720p"] if a.workload == "all" else [a.workload]
    for name in names:
        t1, it1 = layer_call(name, 1, a.steps, a.warmup)
        t2, it2 = layer_call(name, 2, a.steps, a.warmup)
        print(json.dumps({"workload": name, "cfg1_ms": t1, "cfg2_ms": t2, "ratio_total": round(t2["total"] / t1["total"], 3),
                          "iters_cfg1": it1, "iters_cfg2_per_video": it2, "steps": a.steps}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
