"""A/B on one box, one process, one library: the SVG2 layer-call with the centroid tail (include/svg_attn_centroid_tail.h; the SAP
processors' centroid_tail, off by default) against the layer-call of today.

    python tools/ab_centroid_tail.py [--alternations 7] [--min-ms 500] [--out profiles/centroid_tail_ab.jsonl] [--tiny] [--workloads a,b]

Workloads, cfg = 1, head_dim 128, bf16, q / k / v of a head around 64 shared directions (a token's query points at its mode's keys):
  wan_720p      40 heads, S = 21 x 3600 = 75 600 video tokens, no text; 300 query and 1000 key clusters
  hunyuan_720p  24 heads, 33 x 3600 = 118 800 video tokens + 256 text tokens; 400 and 1000 clusters
Per workload, at top_p 0.9 / 0.8 / 0.7 (min_kc_ratio 0.1), one JSON line each:
  * the warm-started layer-call (2 k-means iterations, block map, attention), A = centroid_tail off — launch for launch the call of before
    the option existed —, B = on: a warm-up of both, then `alternations` (at least 7) rounds of (A window, B window), a window as many
    calls between two device events as make at least `min-ms` of work; means, windows, spreads, the granted shader clock of one further
    window of either side (svg._native.ClockProbe; null where the counters do not move);
  * the quality probe's figures of that call off and on (svg2_sparse_attention(quality=...): kept mass, rel. L2 against dense attention
    on 64 sampled rows per head, density), from the same seeds;
and at top_p 0.9 a "stages" line: the operands of one call captured, then every launch of the option alone — the sparse launch in its
plain and in its LSE form, the two svg_cluster_means, the tail launch, the merge — ms per call over three windows, the tail's algorithmic
TFLOP/s (4 S KC D H: every centroid, selected or not) beside the sparse launch's (4 S^2 D H x density), and the clock of the tail launch.
A last line per workload says which (top_p, on) pairs beat (0.9, off) in BOTH time and rel. L2.  No threshold is fixed in advance and the
option stays off whatever comes out.
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import json
import math
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT, ROOT / "tools"):
    sys.path.insert(0, str(p))

from ab_kmeans_e4m3 import clock_of  # noqa: E402
from ab_sparse_lse import alternate, r4, window  # noqa: E402

WORKLOADS = {"wan_720p": dict(H=40, F=21, P=3600, ctx=0, QC=300, KC=1000),
             "hunyuan_720p": dict(H=24, F=33, P=3600, ctx=256, QC=400, KC=1000)}
TINY = {"tiny_wan": dict(H=2, F=4, P=512, ctx=0, QC=4, KC=30), "tiny_hunyuan": dict(H=2, F=4, P=512, ctx=40, QC=4, KC=30)}
TOP_PS = (0.9, 0.8, 0.7)
MIN_KC_RATIO, ITER_INIT, ITER_STEP, D, MODES = 0.1, 50, 2, 128, 64


def mixture(H, V, ctx, dev, gen):
    """q, k, v [1, H, V + ctx, D] bf16: the video tokens of a head around MODES directions shared by q and k, the text tokens noise"""
    ck, cv = 0.5 * torch.randn(H, MODES, D, device=dev, generator=gen), torch.randn(H, MODES, D, device=dev, generator=gen)
    mode = torch.randint(0, MODES, (H, V), device=dev, generator=gen)
    pick = lambda c: torch.gather(c, 1, mode[..., None].expand(-1, -1, D))   # noqa: E731
    noise = lambda n, s=1.0: s * torch.randn(H, n, D, device=dev, generator=gen)   # noqa: E731
    q, k, v = pick(ck) + noise(V), pick(ck) + noise(V), pick(cv) + noise(V, 0.5)
    return tuple(torch.cat([x, noise(ctx)], dim=1).to(torch.bfloat16)[None].contiguous() for x in (q, k, v))


def mean_of(t):
    return None if t is None else round(float(torch.tensor(t, dtype=torch.float64).mean()), 5)


def windows3(fn, min_ms):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    calls = max(2, int(math.ceil(min_ms / max(window(fn, 2), 1e-3))))
    ws = [window(fn, calls) for _ in range(3)]
    return round(sum(ws) / 3, 4), r4(ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/centroid_tail_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--workloads", default=None, help="comma-separated subset")
    a = ap.parse_args()
    from svg import _native as nat
    from svg.models import _core

    nat.load()
    dev = torch.device("cuda", 0)
    out_path = Path(a.out or ROOT / "profiles" / "centroid_tail_ab.jsonl")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 7)
    min_ms = 5.0 if a.tiny else max(a.min_ms, 500.0)
    iter_init = 5 if a.tiny else ITER_INIT
    gen = torch.Generator(device=dev).manual_seed(3)
    table = TINY if a.tiny else WORKLOADS
    names = [n for n in table if a.workloads is None or n in a.workloads.split(",")]
    with open(out_path, "a") as f:
        def emit(rec):
            rec["when"] = time.strftime("%Y-%m-%d %H:%M:%S")
            f.write(json.dumps(rec) + "\n")
            f.flush()
            print(json.dumps(rec), flush=True)

        for name in names:
            w = table[name]
            H, V, ctx, QC, KC = w["H"], w["F"] * w["P"], w["ctx"], w["QC"], w["KC"]
            S = V + ctx
            q, k, v = mixture(H, V, ctx, dev, gen)
            geo = _core.Geometry(ctx, w["F"], w["P"])
            base = {"kind": "centroid_tail", "workload": name, "heads": H, "S": S, "video_tokens": V, "head_dim": D, "dtype": "bf16", "cfg": 1,
                    "q_clusters": QC, "k_clusters": KC, "min_kc_ratio": MIN_KC_RATIO}

            def warm_store():
                store = _core.CentroidStore()
                torch.manual_seed(11)
                torch.cuda.manual_seed(11)
                _core.kmeans_clustering(store, 0, q[:, :, :V], k[:, :, :V], QC, KC, iter_init, ITER_STEP)
                return store

            def layer_call(store, top_p, on, **kw):
                return _core.svg2_sparse_attention(q, k, v, geo, store, 0, QC, KC, top_p, MIN_KC_RATIO, iter_init, ITER_STEP, prompt_length=ctx,
                                                   **({"centroid_tail": True} if on else {}), **kw)

            results = {}
            for top_p in TOP_PS:
                rec = dict(base, what="layer_call", top_p=top_p, a="centroid_tail off (the launches of before)", b="centroid_tail on")
                for on in (False, True):     # the probe's figures, from the same centroids, seeds and probe rows
                    with tempfile.TemporaryDirectory() as tmp:
                        path = str(Path(tmp) / "q.jsonl")
                        store = warm_store()
                        _core.reseed_probe_generator(11)
                        layer_call(store, top_p, on, quality=_core.quality_request("ab_centroid_tail", path, 64))
                        _core.flush_quality_log()
                        r = [json.loads(x) for x in open(path)][-1]
                    tag = "on" if on else "off"
                    assert ("centroid_tail" in r) == on
                    rec[f"kept_mass_{tag}"], rec[f"rel_l2_{tag}"], rec[f"density_{tag}"] = mean_of(r["kept_mass"]), mean_of(r["rel_l2"]), mean_of(r.get("density"))
                sa, sb = warm_store(), warm_store()
                fa, fb = (lambda: layer_call(sa, top_p, False)), (lambda: layer_call(sb, top_p, True))
                wa, wb, calls = alternate(fa, fb, alternations, min_ms)
                a_ms, b_ms = sum(wa) / len(wa), sum(wb) / len(wb)
                rec.update({"alternations": alternations, "calls_per_window": calls, "a_ms": round(a_ms, 4), "b_ms": round(b_ms, 4),
                            "a_windows": r4(wa), "b_windows": r4(wb), "a_spread_ms": round(max(wa) - min(wa), 4),
                            "b_spread_ms": round(max(wb) - min(wb), 4), "cost_ms": round(b_ms - a_ms, 4), "b_over_a": round(b_ms / a_ms, 4),
                            "a_clock_mhz": clock_of(nat, dev, fa, calls), "b_clock_mhz": clock_of(nat, dev, fb, calls)})
                results[top_p] = rec
                emit(rec)
                del sa, sb

            # ---- the launches of the option one by one, on the operands of one call at top_p 0.9 ----
            store = warm_store()
            (ql, qc, qs, _, qidx), (kl, kc, ks, _, kidx) = _core.kmeans_clustering(store, 0, q[:, :, :V], k[:, :, :V], QC, KC, iter_init, ITER_STEP)
            q_sizes, k_sizes = qs.view(1, H, QC), ks.view(1, H, KC)
            dyn = _core.identify_dynamic_map(qc.view(1, H, QC, D), kc.view(1, H, KC, D), q_sizes, k_sizes, TOP_PS[0], MIN_KC_RATIO)
            qi, ki = qidx, kidx
            if ctx:
                dyn, q_sizes, k_sizes, qi, ki = _core.dynamic_map_post_processing(dyn, q_sizes, k_sizes, qidx, kidx, V, ctx, ctx)
            QB, KB = q_sizes.shape[-1], k_sizes.shape[-1]
            density = float(_core.density_calculation(dyn, q_sizes, k_sizes).mean())
            maps, qsz, ksz = dyn.view(H, QB, KB).contiguous(), q_sizes.view(H, QB).contiguous(), k_sizes.view(H, KB).contiguous()
            qi, ki, ks, kidx = qi.contiguous(), ki.contiguous(), ks.reshape(H, KC).contiguous(), kidx.reshape(H, V).contiguous()
            tmaps = maps.clone()
            if ctx:
                tmaps[:, -1, :] = True
            sparse = lambda **kw: nat.varblock_attention(q, k, v, maps, qsz, ksz, q_row_idx=qi, kv_row_idx=ki, rows_covered=True, **kw)   # noqa: E731
            means = lambda: (nat.cluster_means(k[:, :, :V], kidx, ks), nat.cluster_means(v[:, :, :V], kidx, ks))   # noqa: E731
            kbar, vbar = means()
            tail = lambda: nat.centroid_tail_attention(q, kbar, vbar, tmaps, qsz, ks, q_row_idx=qi)   # noqa: E731
            (o_s, l_s), (o_t, l_t) = sparse(return_lse=True), tail()
            merge = lambda: nat.merge_attention_states([o_s, o_t], [l_s.view(1, H, S), l_t], token_major_out=True, return_lse=True)   # noqa: E731
            rec = dict(base, what="stages", top_p=TOP_PS[0], density=round(density, 5),
                       unselected_share_of_non_empty_clusters=round(float(((~tmaps[:, :QC, :KC].bool()) & (ks > 0)[:, None]).double().mean()), 5))
            for key, fn in (("sparse_plain", lambda: sparse(token_major_out=True)), ("sparse_lse", lambda: sparse(return_lse=True)),
                            ("means", means), ("tail", tail), ("merge", merge)):
                rec[f"{key}_ms"], rec[f"{key}_windows"] = windows3(fn, min_ms / 2)
            tail_flop, sparse_flop = 4.0 * S * KC * D * H, 4.0 * S * S * D * H * density
            rec.update({"tail_tflop": round(tail_flop / 1e12, 4), "tail_tflops": round(tail_flop / rec["tail_ms"] / 1e9, 2),
                        "sparse_tflop": round(sparse_flop / 1e12, 4), "sparse_tflops": round(sparse_flop / rec["sparse_lse_ms"] / 1e9, 2),
                        "tail_clock_mhz": clock_of(nat, dev, tail, 20), "sparse_clock_mhz": clock_of(nat, dev, lambda: sparse(return_lse=True), 5)})
            rec["tail_rate_over_sparse_rate"] = round(rec["tail_tflops"] / rec["sparse_tflops"], 4)
            emit(rec)
            ref = results[TOP_PS[0]]
            emit(dict(base, what="verdict", yardstick={"top_p": TOP_PS[0], "ms": ref["a_ms"], "rel_l2": ref["rel_l2_off"], "kept_mass": ref["kept_mass_off"]},
                      pairs=[{"top_p": p, "ms": r["b_ms"], "rel_l2": r["rel_l2_on"], "kept_mass": r["kept_mass_on"], "density": r["density_on"],
                              "beats_the_yardstick_in_time_and_error": bool(r["b_ms"] < ref["a_ms"] and r["rel_l2_on"] < ref["rel_l2_off"])}
                             for p, r in results.items()]))
            del q, k, v, o_s, o_t, l_s, l_t, kbar, vbar
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
