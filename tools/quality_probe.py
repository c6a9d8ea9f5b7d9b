"""What a sparse layer-call cost in accuracy, at production size, on the benches' synthetic data — and what the probe itself costs.

    python tools/quality_probe.py [--workload hy720p|wan720p_svg2|tiny] [--rows 64] [--alternations 7] [--min-ms 300]
                                  [--out profiles/quality_probe.jsonl]

One sparse layer-call through svg/models/_core.py with a QualityRequest, i.e. exactly what a processor with `quality_log` set runs:
  hy720p        SVG1, HunyuanVideo 720p (bench.py's workload: 24 heads, S = 119 056, iid normal q, k, v, sparsity 0.25)
  wan720p_svg2  SVG2, Wan 2.1 720p (bench_svg2.py's workload and its 64-mode Gaussian mixture: 40 heads, S = 75 600, QC 300, KC 1000,
                top_p 0.9, min_kc_ratio 0.1; the second, warm-started call of the layer is the one reported)
Per head: the band (SVG1) or the density (SVG2), the kept mass and the rel. L2 of the logged record.  iid hidden states make every key
matter equally, so an SVG1 band keeps roughly its share of the keys and the error is large: the data decide the number.
Then the probe call (svg_sample_dense_rows) is timed alternating with _native.sample_mse on the same tensors and rows — the same bytes,
K and V once — in one process: a warm-up of both, `alternations` rounds of (window A, window B), a window being as many calls between two
device events as make `min-ms` of work.  Recorded, not gated: the ratio and both spreads go into the line.  The shader clock is not recorded.
GPU only; the line is APPENDED to the output."""
import argparse
import json
import math
import statistics
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT):
    sys.path.insert(0, str(p))

from ab_band_window import stats  # noqa: E402  (tools/ is sys.path[0] when this file is run as a script)
from ab_sparse_lse import alternate  # noqa: E402

SVG1 = {"hy720p": (24, 128, 33, 3600, 256, 64, 0.25), "tiny": (4, 128, 5, 600, 256, 64, 0.4)}   # bench.py WORKLOADS
SVG2 = {"wan720p_svg2": "wan720p"}                                                               # bench_svg2.py WORKLOADS


def logged(path):
    from svg.models import _core

    _core.flush_quality_log()
    return [json.loads(x) for x in open(path)]


def run_svg1(name, n_rows, path):
    from svg import _native as nat
    from svg.models import _core
    from svg.models.hyvideo.utils import profile_desc, sparsity_to_width

    H, D, F_, P_, ctx, L, sparsity = SVG1[name]
    V = F_ * P_
    S = V + ctx
    tf = math.floor(sparsity_to_width(sparsity, ctx, F_, P_) * P_ / 128) * 128
    mask = nat.BandMask(real_len=V + L, band=tf, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    g = torch.Generator(device="cuda").manual_seed(1234)
    q, k, v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    geo = _core.Geometry(ctx, F_, P_)
    prof = profile_desc(ctx, F_, P_)
    req = _core.QualityRequest(path, n_rows, V + L, None, 0)
    _, best = _core.svg1_sparse_attention(q, k, v, geo, mask, prof, 64, min(10000, S), quality=req)
    rec = logged(path)[-1]
    cfg = {"workload": name, "kind": "svg1", "H": H, "S": S, "D": D, "band": tf, "valid_len": V + L, "data": "iid normal",
           "best_mask_idx": best.reshape(-1).tolist()}
    return q, k, v, prof, V + L, rec, cfg


def run_svg2(name, n_rows, path):
    import bench_svg2
    from svg.models import _core
    from svg.models.wan.utils import profile_desc

    H, D, F_, P_, ctx, L, QC, KC = bench_svg2.WORKLOADS[SVG2[name]]
    S = F_ * P_ + ctx
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    q = bench_svg2.clustered(H, S, D, 64, dev, gen)[None]
    k = bench_svg2.clustered(H, S, D, 64, dev, gen)[None]
    v = torch.randn(1, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    geo = _core.Geometry(ctx, F_, P_)
    store = _core.CentroidStore()
    req = _core.QualityRequest(path, n_rows, None, None, 0)
    for _ in range(2):     # the first call of a layer (50 iterations from random points), then the warm-started one
        _core.svg2_sparse_attention(q, k, v, geo, store, 0, QC, KC, 0.9, 0.1, 50, 2, prompt_length=L, quality=req)
    rec = logged(path)[-1]
    cfg = {"workload": name, "kind": "svg2", "H": H, "S": S, "D": D, "QC": QC, "KC": KC, "top_p": 0.9, "min_kc_ratio": 0.1,
           "data": "64-mode Gaussian mixture per head (bench_svg2.py)"}
    return q, k, v, profile_desc(ctx, F_, P_), None, rec, cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="hy720p", choices=sorted(SVG1) + sorted(SVG2))
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--out", default=None, help="default: profiles/quality_probe.jsonl (appended to)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("quality_probe: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat
    from svg import _probe

    nat.load()
    out = Path(a.out or ROOT / "profiles" / "quality_probe.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = str(Path(tmp) / "quality.jsonl")
        q, k, v, prof, valid, rec, cfg = (run_svg1 if a.workload in SVG1 else run_svg2)(a.workload, a.rows, path)
    H = cfg["H"]
    flat = lambda x: None if x is None else [round(float(y), 5) for row in x for y in row]   # noqa: E731
    kept, rel, dens = flat(rec["kept_mass"]), flat(rec["rel_l2"]), flat(rec.get("density"))
    print(f"{a.workload}: {cfg['kind']}, {H} heads, S = {cfg['S']}, {cfg['data']}")
    for h in range(H):
        what = f"density {dens[h]:.4f}" if dens is not None else f"band {cfg['band']} mask {cfg['best_mask_idx'][h]}"
        print(f"  head {h:2d}  {what}  kept mass {kept[h] if kept is not None else float('nan'):.4f}  rel. L2 {rel[h]:.4f}")
    # the probe call beside the online profiler on the same tensors and rows: K and V once either way
    n = max(1, min(a.rows, 64))
    rows = torch.randint(0, valid or cfg["S"], (n,), generator=torch.Generator().manual_seed(0)).cuda()
    fa = lambda: nat.sample_mse(q, k, v, rows, prof)                            # noqa: E731
    fb = lambda: _probe.sample_dense_rows(q, k, v, rows, valid_len=valid)       # noqa: E731
    wa, wb, calls = alternate(fa, fb, max(a.alternations, 5), a.min_ms)
    line = dict(cfg)
    line.update({"rows": n, "kept_mass": kept, "rel_l2": rel, "mse": flat(rec["mse"]), "density": dens,
                 "kept_mass_mean": None if kept is None else round(statistics.fmean(kept), 5), "rel_l2_mean": round(statistics.fmean(rel), 5),
                 "a": "_native.sample_mse (svg_sample_mse)", "b": "_probe.sample_dense_rows (svg_sample_dense_rows)",
                 "alternations": max(a.alternations, 5), "repetitions_per_window": calls})
    line.update(stats(wa, wb))
    kv_bytes = 2 * H * cfg["S"] * cfg["D"] * 2
    med = statistics.median(y - x for x, y in zip(wa, wb))
    line.update({"b_over_a": round(line["b_ms"] / line["a_ms"], 4), "median_diff_ms": round(med, 6),
                 "a_gb_per_s_over_k_v": round(kv_bytes / line["a_ms"] / 1e6, 1), "b_gb_per_s_over_k_v": round(kv_bytes / line["b_ms"] / 1e6, 1),
                 "shader_clock": "not recorded"})
    text = json.dumps(line)
    print(text, flush=True)
    with out.open("a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
