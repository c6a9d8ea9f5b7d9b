#!/usr/bin/env python3
"""A/B on one box, one process: what SVG2's adaptive top-p costs, and whether its K-only probe earns its place.

    python tools/ab_adaptive_top_p.py [--alternations 7] [--min-ms 300] [--out profiles/adaptive_top_p_ab.jsonl] [--tiny]

The Wan 720p SVG2 layer-call of bench_svg2.py (40 heads, S = 75 600, QC 300 / KC 1000, top_p 0.9, min_kc_ratio 0.1, 2 warm-started k-means
iterations on the 64-mode mixture) through svg.models._core.svg2_sparse_attention, both sides from the same library.
  (a) overhead    the plain call against the call with AdaptiveTopP(gain_up = gain_down = 0): the thresholds never move, so the block map is
                  the plain call's and the difference is the always-on cost — the per-head map entry, the LSE form of the attention, the
                  K-only probe (64 rows per head) and the update launch.  Each side keeps its own CentroidStore, warmed by the same
                  calls.  same_bits: the two outputs of the last windows.
  (b) probe cost  _probe.sample_dense_lse against _probe.sample_dense_rows on the same q, k (, v) and the same 64 rows: ms, GB/s over the
                  bytes of K (the K-only pass reads K once; the full probe K and V), lse_same_bits, and the project's rule for keeping a
                  second kernel: k_only_wins = the K-only probe is faster in EVERY alternation by more than 3 x the spread (max - min) of
                  sample_dense_rows' windows.
A warm-up of both sides, then `alternations` (at least 5) rounds of (A window, B window); a window is as many calls between two device
events as make at least `min-ms` of work.  One JSON line per part, appended to --out.  No speed claim is made for the sparse step itself.
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT):
    sys.path.insert(0, str(p))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fa, fb, alternations, min_ms):
    for fn in (fa, fb, fa, fb):
        fn()
    torch.cuda.synchronize()
    calls = [max(1, math.ceil(min_ms / max(window(fn, 1), 1e-3))) for fn in (fa, fb)]
    wa, wb = [], []
    for _ in range(alternations):
        wa.append(window(fa, calls[0]))
        wb.append(window(fb, calls[1]))
    return wa, wb, calls


def stats(w):
    return {"ms": round(sum(w) / len(w), 4), "windows": [round(x, 4) for x in w], "spread_ms": round(max(w) - min(w), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "adaptive_top_p_ab.jsonl"))
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    from bench_svg2 import WORKLOADS, clustered
    from svg import _native as nat
    from svg import _probe
    from svg.models import _core

    nat.load()
    alternations = 2 if a.tiny else max(5, a.alternations)
    H, D, F_, P_, ctx, _, QC, KC = WORKLOADS["small" if a.tiny else "wan720p"]
    if a.tiny:
        QC, KC = 6, 40      # (S = 5000 >= 160 block-rows: the LSE form's condition)
    S = F_ * P_
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    q = clustered(H, S, D, 64, dev, gen)[None]
    k = clustered(H, S, D, 64, dev, gen)[None]
    v = torch.randn(1, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    geo = _core.Geometry(ctx, F_, P_)
    workload = f"{'small' if a.tiny else 'wan720p'} cfg=1 H={H} D={D} S={S} QC={QC} KC={KC} top_p=0.9 min_kc_ratio=0.1 bf16"

    # ---- (a) the layer-call with and without the option ----
    stores = {"plain": _core.CentroidStore(), "adaptive": _core.CentroidStore()}
    tps = _core.TopPStore()
    zero = _core.AdaptiveTopP(0.95, gain_up=0.0, gain_down=0.0)
    last = {}

    def call(name, **kw):
        torch.manual_seed(0)     # (the first call of a layer draws its initial points from the global stream: the same ones on both sides)
        last[name] = _core.svg2_sparse_attention(q, k, v, geo, stores[name], 0, QC, KC, 0.9, 0.1, 50, 2, **kw)

    fa = lambda: call("plain")                                           # noqa: E731
    fb = lambda: call("adaptive", adaptive=zero, top_p_store=tps)        # noqa: E731
    wa, wb, calls = alternate(fa, fb, alternations, a.min_ms)
    sa, sb = stats(wa), stats(wb)
    rec_a = {"metric": "adaptive_top_p_overhead", "workload": workload, "alternations": alternations, "calls_per_window": calls,
             "plain": sa, "adaptive_zero_gains": sb, "overhead_ms": round(sb["ms"] - sa["ms"], 4),
             "overhead_over_plain_spread": round((sb["ms"] - sa["ms"]) / max(sa["spread_ms"], 1e-6), 2),
             "adaptive_over_plain": round(sb["ms"] / sa["ms"], 4), "same_bits": bool(torch.equal(last["plain"], last["adaptive"])),
             "kept_mass_min_max": [round(float(tps.kept[0].min()), 4), round(float(tps.kept[0].max()), 4)]}
    print(json.dumps(rec_a), flush=True)

    # ---- (b) the K-only probe against the full one ----
    rows = torch.randint(0, S, (64,), generator=torch.Generator().manual_seed(1)).to(dev)
    out = {}
    fr = lambda: out.__setitem__("rows", _probe.sample_dense_rows(q, k, v, rows)[1])     # noqa: E731
    fl = lambda: out.__setitem__("lse", _probe.sample_dense_lse(q, k, rows))             # noqa: E731
    wr, wl, calls = alternate(fr, fl, alternations, a.min_ms)
    sr, sl = stats(wr), stats(wl)
    k_bytes = H * S * D * 2
    rec_b = {"metric": "adaptive_top_p_probe", "workload": workload + " R=64", "alternations": alternations, "calls_per_window": calls,
             "sample_dense_rows": dict(sr, gb_per_s_over_k=round(k_bytes / sr["ms"] / 1e6, 1)),
             "sample_dense_lse": dict(sl, gb_per_s_over_k=round(k_bytes / sl["ms"] / 1e6, 1)),
             "lse_over_rows": round(sl["ms"] / sr["ms"], 4), "lse_same_bits": bool(torch.equal(out["rows"], out["lse"])),
             "k_only_wins": bool(all(r - l > 3 * sr["spread_ms"] for r, l in zip(wr, wl)))}
    print(json.dumps(rec_b), flush=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(rec_a) + "\n" + json.dumps(rec_b) + "\n")


if __name__ == "__main__":
    main()
