"""A/B on one box, one process, one library: the SVG2 k-means with e4m3 assignments in all but the last Lloyd iteration of a call
(svg_kmeans_loop_e4m3, include/svg_attn_kmeans_e4m3.h; the processors' kmeans_e4m3) against the 16-bit loop of today.

    python tools/ab_kmeans_e4m3.py [--alternations 7] [--min-ms 500] [--out profiles/kmeans_e4m3_ab.jsonl] [--tiny] [--no-layer-call]

Workloads, cfg = 1, head_dim 128, bf16:
  wan_720p      40 heads, N = 21 x 3600 = 75 600 video tokens, no text; 300 query and 1000 key clusters
  hunyuan_720p  24 heads, N = 33 x 3600 = 118 800 video tokens of S = N + 256, read in place; 400 and 1000 clusters
Timed, A = 16-bit, B = e4m3: the 2-iteration stage ("warm": kmeans_clustering from the previous call's centroids, both sides, as the
layer-call runs it), the 50-iteration initialisation ("init"), and the assignment alone on the K = 1000 side with its centroid pre-pass
("assign": svg_kmeans_assign against svg_kmeans_assign_e4m3 around svg_kmeans_centre's mu).  A warm-up of both, then `alternations` (at
least 7) rounds of (A window, B window); a window is as many repetitions between two device events as make at least `min-ms` (at least 500)
of work.  One JSON line per (workload, what): a_ms / b_ms means over the windows, the windows, their spreads (max - min), the granted shader
clock of one further window of either side (svg._native.ClockProbe; null where the counters do not move), and
  won = every alternation is won by B AND a_ms - b_ms > 3 x A's spread                                     (the rule of DESIGN §3.3)
and per workload a "quality" line: label agreement and inertia ratio of the mixed loop against the 16-bit loop from the same initial
points (both stages), the 16-bit loop's inertia over five other draws of the initial points relative to the first, and — unless
--no-layer-call — the kept mass and rel. L2 of the layer-call's quality probe (svg2_sparse_attention(quality=...)) with the option off and on.
The option ships off whatever the result; a case that is not won is written down as such.
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT, ROOT / "tools"):
    sys.path.insert(0, str(p))

from ab_kmeans_stepped import clustered_heads  # noqa: E402
from ab_sparse_lse import alternate, r4  # noqa: E402

WORKLOADS = {"wan_720p": dict(H=40, F=21, P=3600, ctx=0, QC=300, KC=1000),
             "hunyuan_720p": dict(H=24, F=33, P=3600, ctx=256, QC=400, KC=1000)}
TINY = {"tiny_wan": dict(H=2, F=5, P=300, ctx=0, QC=12, KC=30), "tiny_hunyuan": dict(H=2, F=4, P=200, ctx=40, QC=12, KC=30)}
STAGES = {"warm": 2, "init": 50}
D = 128


def inertia(x, cent, labels):
    """sum over heads and rows of |x - c_label|^2 (fp32 per head, float64 over heads); x [H, N, D] (a view is fine)"""
    tot = 0.0
    for h in range(x.shape[0]):
        d = x[h].float() - cent[h].float()[labels[h].long()]
        tot += float((d * d).sum().double())
    return tot


def clock_of(nat, dev, fn, calls):
    probe = nat.ClockProbe(dev)
    probe.start()
    for _ in range(calls):
        fn()
    probe.arm_stop()
    mhz = probe.result()
    torch.cuda.synchronize()
    return mhz


def timed(nat, dev, rec, fa, fb, alternations, min_ms):
    wa, wb, calls = alternate(fa, fb, alternations, min_ms)
    a_ms, b_ms = sum(wa) / len(wa), sum(wb) / len(wb)
    a_spread = max(wa) - min(wa)
    rec.update({"alternations": alternations, "repetitions_per_window": calls, "a": "16-bit assignment in every iteration",
                "b": "e4m3 assignment in all but the last iteration", "a_ms": round(a_ms, 4), "b_ms": round(b_ms, 4), "a_windows": r4(wa),
                "b_windows": r4(wb), "a_spread_ms": round(a_spread, 4), "b_spread_ms": round(max(wb) - min(wb), 4),
                "a_clock_mhz": clock_of(nat, dev, fa, calls), "b_clock_mhz": clock_of(nat, dev, fb, calls),
                "every_alternation_won": bool(all(y < x for x, y in zip(wa, wb))), "gain_ms": round(a_ms - b_ms, 4),
                "gain_over_a_spread": round((a_ms - b_ms) / a_spread, 2) if a_spread > 0 else None, "when": time.strftime("%Y-%m-%d %H:%M:%S")})
    rec["won"] = bool(rec["every_alternation_won"] and (a_ms - b_ms) > 3 * a_spread)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/kmeans_e4m3_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--no-layer-call", action="store_true")
    ap.add_argument("--workloads", default=None, help="comma-separated subset")
    a = ap.parse_args()
    from svg import _native as nat
    from svg.models import _core

    nat.load()
    dev = torch.device("cuda", 0)
    out_path = Path(a.out or ROOT / "profiles" / "kmeans_e4m3_ab.jsonl")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 7)
    min_ms = 5.0 if a.tiny else max(a.min_ms, 500.0)
    gen = torch.Generator(device=dev).manual_seed(3)
    table = TINY if a.tiny else WORKLOADS
    names = [n for n in table if a.workloads is None or n in a.workloads.split(",")]
    with open(out_path, "a") as f:
        def emit(rec):
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        for name in names:
            w = table[name]
            H, V = w["H"], w["F"] * w["P"]
            S = V + w["ctx"]
            q, k = clustered_heads(H, S, dev, gen), clustered_heads(H, S, dev, gen)
            qv, kv = q[:, :, :V], k[:, :, :V]                      # (views where there is text: read in place)
            base = {"kind": "kmeans_e4m3", "workload": name, "heads": H, "N": V, "S": S, "head_dim": D, "dtype": "bf16", "cfg": 1,
                    "q_clusters": w["QC"], "k_clusters": w["KC"], "two_streams": bool(_core.KMEANS_TWO_STREAMS)}
            warm_store = _core.CentroidStore()
            torch.manual_seed(7)
            _core.kmeans_clustering(warm_store, 0, qv, kv, w["QC"], w["KC"], 2, 2)
            q0, k0 = warm_store.q[0].clone(), warm_store.k[0].clone()

            def stage_call(stage, on, seed=11):
                if stage == "warm":
                    store = warm_store
                    store.put(0, q0, k0, 1)                        # (every repetition starts from the same centroids)
                else:
                    store = _core.CentroidStore()
                    torch.manual_seed(seed)                        # (the same random rows on both sides)
                    torch.cuda.manual_seed(seed)
                iters = STAGES[stage]
                return _core.kmeans_clustering(store, 0, qv, kv, w["QC"], w["KC"], iters, iters, e4m3=on)

            quality = dict(base, what="quality")
            for stage, iters in STAGES.items():
                ra, rb = stage_call(stage, False), stage_call(stage, True)
                torch.cuda.synchronize()
                for side, x, sa, sb in (("q", qv[0], ra[0], rb[0]), ("k", kv[0], ra[1], rb[1])):
                    # (labels [H, N] against the centroids that ENTERED the last iteration are not returned: the returned centroids are their
                    #  update, the exact means of the returned labels' clusters — the same measure on both sides)
                    ia, ib = inertia(x, sa[1], sa[0]), inertia(x, sb[1], sb[0])
                    quality[f"{stage}_{side}_label_agreement"] = round(float((sa[0] == sb[0]).double().mean()), 5)
                    quality[f"{stage}_{side}_inertia_ratio"] = round(ib / ia, 5)
                    if stage == "init":
                        draws = []
                        for seed in range(21, 26):
                            rd = stage_call("init", False, seed=seed)[0 if side == "q" else 1]
                            draws.append(round(inertia(x, rd[1], rd[0]) / ia, 5))
                        quality[f"init_{side}_inertia_16bit_other_draws"] = draws
                del ra, rb
                emit(timed(nat, dev, dict(base, what=stage, max_iters=iters, fp8_iters=iters - 1), lambda: stage_call(stage, False),
                           lambda: stage_call(stage, True), alternations, min_ms))
            xk = kv[0].contiguous()
            mu = nat.kmeans_centre(k0)
            la, lb = nat.kmeans_assign(xk, k0), nat.kmeans_assign_e4m3(xk, k0, mu)
            quality["assign_k_label_agreement"] = round(float((la == lb).double().mean()), 5)
            emit(timed(nat, dev, dict(base, what="assign", K=w["KC"]), lambda: nat.kmeans_assign(xk, k0),
                       lambda: nat.kmeans_assign_e4m3(xk, k0, mu), alternations, min_ms))
            del xk, la, lb
            if not a.no_layer_call:
                v = torch.randn(1, H, S, D, device=dev, generator=gen).to(torch.bfloat16)
                geo = _core.Geometry(w["ctx"], w["F"], w["P"])
                for on in (False, True):
                    with tempfile.TemporaryDirectory() as tmp:
                        path = str(Path(tmp) / "q.jsonl")
                        store = _core.CentroidStore()
                        torch.manual_seed(11)
                        torch.cuda.manual_seed(11)
                        _core.reseed_probe_generator(11)
                        for _ in range(2):                             # the init call, then a warm-started call: its record is kept
                            _core.svg2_sparse_attention(q, k, v, geo, store, 0, w["QC"], w["KC"], 0.9, 0.1, 50 if not a.tiny else 5, 2,
                                                        prompt_length=w["ctx"], quality=_core.quality_request("ab_kmeans_e4m3", path, 64),
                                                        kmeans_e4m3=on)
                        _core.flush_quality_log()
                        rec = [json.loads(x) for x in open(path)][-1]
                    mean = lambda t: None if t is None else round(float(torch.tensor(t, dtype=torch.float64).mean()), 5)   # noqa: E731
                    tag = "on" if on else "off"
                    quality[f"layer_call_kept_mass_{tag}"], quality[f"layer_call_rel_l2_{tag}"] = mean(rec["kept_mass"]), mean(rec["rel_l2"])
                    quality[f"layer_call_density_{tag}"] = mean(rec.get("density"))
                del v
            quality["when"] = time.strftime("%Y-%m-%d %H:%M:%S")
            emit(quality)
            del q, k, qv, kv
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
