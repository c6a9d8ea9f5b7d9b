"""A/B on one box, one process, one library: the Lloyd loop under the cosine and the dot-product metric (svg_kmeans_loop_metric,
include/svg_attn_kmeans_metric.h) against the Euclidean loop of the same build (svg_kmeans_loop[_strided]).

    python tools/ab_kmeans_metric.py [--alternations 7] [--min-ms 500] [--out profiles/kmeans_metric_ab.jsonl] [--tiny] [--workloads a,b]

Workloads, head_dim 128, bf16:
  wan_720p      40 heads, N = 21 x 3600 = 75 600 video tokens, no text; K = 300 and K = 1000
  hunyuan_720p  24 heads, N = 33 x 3600 = 118 800 video tokens of S = N + 256, read in place; K = 400 and K = 1000
Timed per (workload, K, metric), A = Euclid, B = the metric: the 2-iteration stage and the 50-iteration initialisation, both from the same
random rows of x, with tol = 0 (no group ever stops: every iteration does all its work on both sides).  Per iteration the metric loop
launches one kernel less (no |c|^2 pass) and its update has one barrier more per cluster and, for cosine, a lane reduction per row.  A warm-up
of both, then `alternations` (at least 7) rounds of (A window, B window); a window is as many repetitions between two device events as make
at least `min-ms` (at least 500) of work.  One JSON line per case: a_ms / b_ms means over the windows, the windows, their spreads (max - min),
b_over_a, the granted shader clock of one further window of either side (svg._native.ClockProbe; null where the counters do not move), and
  slower = b_ms - a_ms > 3 x A's spread,  faster = a_ms - b_ms > 3 x A's spread with every alternation won        (the rule of DESIGN §3.3)
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT, ROOT / "tools"):
    sys.path.insert(0, str(p))

from ab_kmeans_e4m3 import clock_of  # noqa: E402
from ab_kmeans_stepped import clustered_heads  # noqa: E402
from ab_sparse_lse import alternate, r4  # noqa: E402

WORKLOADS = {"wan_720p": dict(H=40, F=21, P=3600, ctx=0, Ks=(300, 1000)), "hunyuan_720p": dict(H=24, F=33, P=3600, ctx=256, Ks=(400, 1000))}
TINY = {"tiny_wan": dict(H=2, F=5, P=300, ctx=0, Ks=(12, 30)), "tiny_hunyuan": dict(H=2, F=4, P=200, ctx=40, Ks=(12,))}
STAGES = {"warm": 2, "init": 50}
D = 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/kmeans_metric_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--workloads", default=None, help="comma-separated subset")
    a = ap.parse_args()
    from svg import _native as nat

    nat.load()
    dev = torch.device("cuda", 0)
    out_path = Path(a.out or ROOT / "profiles" / "kmeans_metric_ab.jsonl")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 7)
    min_ms = 5.0 if a.tiny else max(a.min_ms, 500.0)
    gen = torch.Generator(device=dev).manual_seed(3)
    table = TINY if a.tiny else WORKLOADS
    work = nat.WorkspaceCache()
    with open(out_path, "a") as f:
        for name in [n for n in table if a.workloads is None or n in a.workloads.split(",")]:
            w = table[name]
            H, V = w["H"], w["F"] * w["P"]
            S = V + w["ctx"]
            x = clustered_heads(H, S, dev, gen)[0][:, :V]             # [H, V, D]: a view where there is text, read in place by both sides
            for K in w["Ks"]:
                idx = torch.randint(0, V, (H, K), device=dev, generator=gen)
                c0 = torch.gather(x, 1, idx[..., None].expand(-1, -1, D)).contiguous()
                for stage, iters in STAGES.items():
                    for metric in ("cosine", "dot"):
                        fa = lambda: nat.kmeans_loop(x, None, c0, iters, 0.0, work=work)                 # noqa: E731
                        fb = lambda: nat.kmeans_loop_metric(x, c0, iters, 0.0, metric, work=work)        # noqa: E731
                        wa, wb, calls = alternate(fa, fb, alternations, min_ms)
                        a_ms, b_ms = sum(wa) / len(wa), sum(wb) / len(wb)
                        a_spread = max(wa) - min(wa)
                        rec = {"kind": "kmeans_metric", "workload": name, "heads": H, "N": V, "S": S, "head_dim": D, "dtype": "bf16", "K": K,
                               "what": stage, "max_iters": iters, "tol": 0.0, "a": "euclid", "b": metric, "alternations": alternations,
                               "repetitions_per_window": calls, "a_ms": round(a_ms, 4), "b_ms": round(b_ms, 4), "a_windows": r4(wa),
                               "b_windows": r4(wb), "a_spread_ms": round(a_spread, 4), "b_spread_ms": round(max(wb) - min(wb), 4),
                               "b_over_a": round(b_ms / a_ms, 4), "a_clock_mhz": clock_of(nat, dev, fa, calls),
                               "b_clock_mhz": clock_of(nat, dev, fb, calls), "slower": bool(b_ms - a_ms > 3 * a_spread),
                               "faster": bool(all(y < z for z, y in zip(wa, wb)) and a_ms - b_ms > 3 * a_spread),
                               "when": time.strftime("%Y-%m-%d %H:%M:%S")}
                        f.write(json.dumps(rec) + "\n")
                        f.flush()
                        print(json.dumps(rec), flush=True)
            del x
            work.clear()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
