"""A/B on one box, one process: the k-means stage of one rank's head shard of a sharded SVG2 layer-call (svg.models._core.kmeans_clustering
with a head_shard) — the library's loop in steps (svg_kmeans_stepped_*, svg.kmeans_utils.lloyd_stepped: both sides in lock-step, one reduce
per iteration) against the torch statement lloyd_device_rule on svg_kmeans_iter (one loop per side, one reduce per iteration and side).
ONE GPU, an IDENTITY reduce: no collective runs and none is timed; no multi-GPU run exists for this project.

    python tools/ab_kmeans_stepped.py [--alternations 7] [--min-ms 500] [--out profiles/kmeans_stepped_ab.jsonl] [--tiny]

Workloads, one rank's shard of 8, cfg = 1, head_dim 128, bf16:
  wan_720p      5 of 40 heads, N = 21 x 3600 = 75 600 video tokens, no text; 300 query and 1000 key clusters
  hunyuan_720p  3 of 24 heads, N = 33 x 3600 = 118 800 video tokens of S = N + 256 (bench_svg2.py --workload hy720p), 400 and 1000 clusters;
                the stage starts from the contiguous [1, H, S, D] q and k as svg2_sparse_attention does: B reads the video tokens in place,
                A takes the two .contiguous() copies
Stages: warm (2 iterations from the previous call's centroids) and init (50 iterations from random rows).
A = STEPPED_LOOP_UNDER_SHARDS off, B = on; a warm-up of both, then `alternations` (at least 7) rounds of (A window, B window); a window is as
many repetitions between two device events as make at least `min-ms` (at least 500) of work.  One JSON line per (workload, stage): a_ms /
b_ms means over the windows, the windows, their spreads (max - min), the shift_reduce calls per stage of either side, same_bits, and
  won = every alternation is won by B AND a_ms - b_ms > 3 x A's spread
— the rule of the svg_copy_boxes A/B.  kmeans_utils.STEPPED_LOOP_UNDER_SHARDS defaults to on only if every case is won; a
case that is not won is written down as such.  (The shader clock is not recorded.)
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

from ab_sparse_lse import alternate, r4  # noqa: E402

# heads of this rank, heads of the model, frames, frame size, text rows, query / key clusters
WORKLOADS = {"wan_720p": dict(H=5, H_all=40, F=21, P=3600, ctx=0, QC=300, KC=1000),
             "hunyuan_720p": dict(H=3, H_all=24, F=33, P=3600, ctx=256, QC=400, KC=1000)}
TINY = {"tiny_wan": dict(H=2, H_all=4, F=5, P=300, ctx=0, QC=12, KC=30), "tiny_hunyuan": dict(H=2, H_all=4, F=4, P=200, ctx=40, QC=12, KC=30)}
STAGES = {"warm": 2, "init": 50}
D = 128


def clustered_heads(H, S, dev, gen):
    """[1, H, S, D] bf16: rows around 64 directions per head (tokens of a video are not white noise: the loops sort and update real clusters)"""
    centers = torch.randn(H, 64, D, device=dev, generator=gen) * 2.0
    idx = torch.randint(0, 64, (H, S), device=dev, generator=gen)
    x = torch.gather(centers, 1, idx[..., None].expand(-1, -1, D)) + 0.7 * torch.randn(H, S, D, device=dev, generator=gen)
    return x.to(torch.bfloat16)[None].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/kmeans_stepped_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    from svg import _native as nat
    from svg import distributed as sd
    from svg import kmeans_utils as ku
    from svg.models import _core

    nat.load()
    dev = torch.device("cuda", 0)
    out_path = Path(a.out or ROOT / "profiles" / "kmeans_stepped_ab.jsonl")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 7)
    min_ms = 5.0 if a.tiny else max(a.min_ms, 500.0)
    reduces = [0]

    def identity_reduce(t):
        reduces[0] += 1
        return t

    sd.all_reduce_max_ = identity_reduce      # (kmeans_clustering reads it at every call; sharding itself stays off: one process)
    gen = torch.Generator(device=dev).manual_seed(3)
    with open(out_path, "a") as f:
        for name, w in (TINY if a.tiny else WORKLOADS).items():
            H, V = w["H"], w["F"] * w["P"]
            S = V + w["ctx"]
            q, k = clustered_heads(H, S, dev, gen), clustered_heads(H, S, dev, gen)
            shard = (0, H, w["H_all"])
            for stage, iters in STAGES.items():
                warm_store = _core.CentroidStore()
                torch.manual_seed(7)
                _core.kmeans_clustering(warm_store, 0, q[:, :, :V].contiguous(), k[:, :, :V].contiguous(), w["QC"], w["KC"], 2, 2, head_shard=shard)
                q0, k0 = warm_store.q[0].clone(), warm_store.k[0].clone()

                def run(on):
                    """the stage as svg2_sparse_attention runs it: the video tokens (views or copies), then kmeans_clustering"""
                    ku.STEPPED_LOOP_UNDER_SHARDS = on
                    if w["ctx"]:
                        qv, kv = (q[:, :, :V], k[:, :, :V]) if on else (q[:, :, :V].contiguous(), k[:, :, :V].contiguous())
                    else:
                        qv, kv = q, k
                    if stage == "warm":
                        store = warm_store
                        store.put(0, q0, k0, 1)          # (every repetition starts from the same centroids)
                    else:
                        store = _core.CentroidStore()
                        torch.manual_seed(11)            # (the same random rows on both sides)
                        torch.cuda.manual_seed(11)
                    return _core.kmeans_clustering(store, 0, qv, kv, w["QC"], w["KC"], iters, iters, head_shard=shard)

                fa, fb = (lambda: run(False)), (lambda: run(True))
                reduces[0] = 0
                ra = fa()
                a_reduces, reduces[0] = reduces[0], 0
                rb = fb()
                b_reduces = reduces[0]
                torch.cuda.synchronize()
                same = all(torch.equal(x.view(torch.int16) if x.dtype == torch.bfloat16 else x, y.view(torch.int16) if y.dtype == torch.bfloat16 else y)
                           for sa, sb in zip(ra, rb) for x, y in zip(sa, sb))
                n_iters = [int(ra[0][3]), int(ra[1][3])]
                del ra, rb
                wa, wb, calls = alternate(fa, fb, alternations, min_ms)
                a_ms, b_ms = sum(wa) / len(wa), sum(wb) / len(wb)
                a_spread = max(wa) - min(wa)
                rec = {"kind": "kmeans_stepped", "workload": name, "stage": stage, "max_iters": iters, "n_iters_q_k": n_iters,
                       "heads": H, "heads_of_the_model": w["H_all"], "N": V, "S": S, "head_dim": D, "dtype": "bf16", "cfg": 1,
                       "q_clusters": w["QC"], "k_clusters": w["KC"], "video_tokens_in_place": {"a": False, "b": True} if w["ctx"] else "no text",
                       "two_streams": {"a": False, "b": bool(_core.KMEANS_TWO_STREAMS)},
                       "alternations": alternations, "repetitions_per_window": calls,
                       "a": "lloyd_device_rule on svg_kmeans_iter (switch off)", "b": "svg_kmeans_stepped_* (switch on)",
                       "a_ms": round(a_ms, 4), "b_ms": round(b_ms, 4), "a_windows": r4(wa), "b_windows": r4(wb),
                       "a_spread_ms": round(a_spread, 4), "b_spread_ms": round(max(wb) - min(wb), 4),
                       "a_shift_reduce_calls": a_reduces, "b_shift_reduce_calls": b_reduces,
                       "every_alternation_won": bool(all(y < x for x, y in zip(wa, wb))),
                       "gain_ms": round(a_ms - b_ms, 4), "gain_over_a_spread": round((a_ms - b_ms) / a_spread, 2) if a_spread > 0 else None,
                       "same_bits": bool(same), "reduce": "identity (one GPU)", "collective_timed": False, "shader_clock": "not recorded",
                       "when": time.strftime("%Y-%m-%d %H:%M:%S")}
                rec["won"] = bool(rec["every_alternation_won"] and (a_ms - b_ms) > 3 * a_spread)
                f.write(json.dumps(rec) + "\n")
                f.flush()
                print(json.dumps(rec), flush=True)
            del q, k
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
