"""A/B on one box, one process: variable-block attention with the row log-sum-exp / fp32 rows from the body variant -1 picks
(include/svg_attn_varblock_lse_auto.h) against the plain variant -1 call, below Sq = 160 QB — the 128-row lock-step body.

    python tools/ab_varblock_lse_auto.py --parent <libsvgattn.so of the parent commit> [--alternations 7] [--min-ms 500]
                                         [--out profiles/varblock_lse_auto_ab.jsonl] [--tiny]

Workloads, bf16, head_dim 128, the mixture data and the plan of bench_svg2.py (warm-started k-means, top-p 0.9 block map, fused row
permutation): Cosmos-7B 720p (32 heads, S = 56 320, QC 400 / KC 1000) and Wan 480p at a raised cluster count (40 heads, S = 32 760, QC 300 /
KC 1000).  Both libraries are loaded side by side through ctypes and called on the same tensors and workspace.  Per pair: a warm-up, then
`alternations` (at least 5) rounds of (A window, B window), a window being as many calls between two device events as make `min-ms` of
work, with the shader clock granted to each window (svg._native.ClockProbe; null where the counters do not move).  One JSON line per pair:
  plain_vs_parent        A = svg_varblock_attention(variant -1) of the parent, B = of this build: expected bit-identical and inside A's
                         own window-to-window spread, which is the margin (inside_a_spread)
  lse_auto_vs_plain      A = the plain call of this build, B = svg_varblock_attention_lse_auto: what the lse store costs; same_bits: o
  f32_auto_vs_plain      B = svg_varblock_attention_lse_auto_f32: fp32 rows in the place of o; same_bits: o32 rounded to bf16 against o
  forced_256_vs_plain    B = svg_varblock_attention_lse: the 16x16x32 body on 256-row tiles — what the state cost before, with other bits
Fields per side: ms (mean over the windows), windows, spread_ms = max - min, sclk_mhz; b_over_a, diff_ms, inside_a_spread, same_bits,
lse_finite.  The cost inside a layer-call of a real model is not what this measures.
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import ctypes as C
import json
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT):
    sys.path.insert(0, str(p))

from ab_adaptive_band import alternate_clocked, stats  # noqa: E402  (tools/ is sys.path[0] when this file is run as a script)

PLAIN, AUTO, AUTO32, FORCED = ("svg_varblock_attention", "svg_varblock_attention_lse_auto", "svg_varblock_attention_lse_auto_f32",
                               "svg_varblock_attention_lse")


def typed(nat, path, names):
    lib = C.CDLL(str(Path(path).resolve()))
    sigs = {**nat.SIGNATURES, **nat.SPARSE_LSE_SIGNATURES, **nat.VARBLOCK_LSE_AUTO_ENTRIES}
    for name in names:
        getattr(lib, name).restype, getattr(lib, name).argtypes = sigs[name]
    return lib


def run_workload(nat, name, H, S, QC, KC, old, new, alternations, min_ms, probe):
    from bench_svg2 import clustered
    from svg.kmeans_utils import identify_dynamic_map
    from svg.models import _core

    D = 128
    assert S < 160 * QC, "the workloads of this tool sit below the threshold of the 256-row bodies"
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(0)
    q, k = (clustered(H, S, D, 64, dev, gen)[None] for _ in range(2))
    v = torch.randn(1, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    store = _core.CentroidStore()
    _core.kmeans_clustering(store, 0, q, k, QC, KC, 50, 2)                       # the first call of a layer: 50 iterations
    (_, qc, qs, _, qidx), (_, kc, ks, _, kidx) = _core.kmeans_clustering(store, 0, q, k, QC, KC, 50, 2)
    dmap = identify_dynamic_map(qc.view(1, H, QC, D), kc.view(1, H, KC, D), qs.view(1, H, QC), ks.view(1, H, KC), 0.9, 0.1)
    bmap, qsz, ksz = dmap.view(H, QC, KC).contiguous(), qs.view(H, QC).contiguous(), ks.view(H, KC).contiguous()
    qidx, kidx = qidx.contiguous(), kidx.contiguous()
    ws = nat.varblock_workspace(H, H, QC, KC, S, dev)
    o = [torch.empty_like(q) for _ in range(2)]
    o32 = torch.empty(1, H, S, D, dtype=torch.float32, device=dev)
    lse = torch.empty(1, H, S, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    mid = (H, H, S, S, D, 0, 1.0 / math.sqrt(D), bmap.data_ptr(), qsz.data_ptr(), ksz.data_ptr(), QC, KC, qidx.data_ptr(), kidx.data_ptr(),
           ws.data_ptr(), ws.numel())

    def call(lib, entry, out):
        fn = getattr(lib, entry)
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()) + ((lse.data_ptr(),) if entry != PLAIN else ()) + mid + (
            (-1, st) if entry == PLAIN else (None, st))

        def run():
            rc = fn(*args)
            if rc != 0:
                raise RuntimeError(f"{entry}: error {rc}")
        return run

    density = float(nat.map_density(bmap, qsz, ksz).mean())
    recs = []
    for label, la, ea, entry, out in (("plain_vs_parent", old, "parent: ", PLAIN, o[1]), ("lse_auto_vs_plain", new, "this build: ", AUTO, o[1]),
                                      ("f32_auto_vs_plain", new, "this build: ", AUTO32, o32), ("forced_256_vs_plain", new, "this build: ", FORCED, o[1])):
        fa, fb = call(la, PLAIN, o[0]), call(new, entry, out)
        for t in (o[0], out, lse):
            t.fill_(float("nan"))
        fa()
        fb()
        torch.cuda.synchronize()
        same = bool(torch.equal(o[0], out.to(torch.bfloat16)))
        finite = bool(torch.isfinite(lse).all()) if entry != PLAIN else None
        (wa, wb), (ma, mb), calls = alternate_clocked([fa, fb], alternations, min_ms, probe)
        sa, sb = dict(stats(wa), sclk_mhz=ma), dict(stats(wb), sclk_mhz=mb)
        diff = sb["ms"] - sa["ms"]
        rec = {"pair": label, "workload": name, "a": ea + PLAIN + " (variant -1)", "b": "this build: " + entry, "Hq": H, "S": S, "D": D,
               "dtype": "bfloat16", "QB": QC, "KB": KC, "map_density": round(density, 4), "alternations": alternations,
               "calls_per_window": calls, "a_side": sa, "b_side": sb, "b_over_a": round(sb["ms"] / sa["ms"], 4), "diff_ms": round(diff, 4),
               "inside_a_spread": bool(abs(diff) <= sa["spread_ms"]), "same_bits": same, "lse_finite": finite}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libsvgattn.so built from the parent commit")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/varblock_lse_auto_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_varblock_lse_auto: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    new, old = typed(nat, nat.lib_path(), [PLAIN, AUTO, AUTO32, FORCED]), typed(nat, a.parent, [PLAIN])
    probe = nat.ClockProbe(torch.device("cuda"))
    alternations, min_ms = (2, 10.0) if a.tiny else (max(a.alternations, 5), a.min_ms)
    loads = [("tiny", 2, 2000, 20, 40)] if a.tiny else [("cosmos7b_720p", 32, 56320, 400, 1000), ("wan480p_qc300", 40, 32760, 300, 1000)]
    out = Path(a.out or ROOT / "profiles" / "varblock_lse_auto_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as f:
        for name, H, S, QC, KC in loads:
            for rec in run_workload(nat, name, H, S, QC, KC, old, new, alternations, min_ms, probe):
                f.write(json.dumps(rec) + "\n")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
