"""A/B on one box, one process: what the row log-sum-exp costs on the band (SVG1) and variable-block (SVG2) bodies.

    python tools/ab_sparse_lse.py [--alternations 7] [--min-ms 1000] [--out profiles/sparse_attention_lse_ab.jsonl] [--tiny]

The LSE entry against the plain entry, alternating, on the same tensors, both from the same library (the plain kernels' listings are the
parent's, profiles/sparse_attention_lse_asm_diff.txt):
  band      HunyuanVideo 720p (24 heads, S = 33 x 3600 + 256 = 119 056, bf16, sparsity 0.25 -> band 15 616, every second head token-major
            through the fused placement: the attention call of bench.py) — _native.band_attention(...) against band_attention(...,
            return_lse=True).  The plain entry runs the work queue at this size and the LSE entry the static mapping, so the figure
            contains the static mapping's known distance to the queue besides the store itself.
  varblock  the Wan 720p SVG2 plan of bench_svg2.py (40 heads, S = 75 600, QC 300 / KC 1000, top-p 0.9 block map of warm-started k-means on
            clustered data, fused row permutation, rows_covered) — varblock_attention(...) against varblock_attention(..., return_lse=True):
            the same plan, launch order and workspace.
Per workload: a warm-up of both, then `alternations` (at least 5) rounds of (plain window, LSE window); a window is as many calls between
two device events as make at least `min-ms` of work.  One JSON line per workload:
  plain_ms / lse_ms            mean over the windows, *_windows the windows, *_spread_ms = max - min
  loss_ms, lse_over_plain, loss_over_plain_spread      (no pass / fail number: the plain entries are unchanged by construction)
  same_bits                    o of the two forms; lse_finite                      (the shader clock is not recorded)
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
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    est = min(window(fa, 2), window(fb, 2))
    calls = max(2, int(math.ceil(min_ms / max(est, 1e-3))))
    wa, wb = [], []
    for _ in range(alternations):
        wa.append(window(fa, calls))
        wb.append(window(fb, calls))
    return wa, wb, calls


def r4(xs):
    return [round(x, 4) for x in xs]


def record(nat, kind, name, cfg, plain, with_lse, alternations, min_ms):
    a = plain().clone()
    b, lse = with_lse()
    torch.cuda.synchronize()
    same = bool(torch.equal(a, b))
    finite = bool(torch.isfinite(lse).all())
    del a, b
    wp, wl, calls = alternate(plain, lambda: with_lse()[0], alternations, min_ms)
    ms_p, ms_l = sum(wp) / len(wp), sum(wl) / len(wl)
    spread_p = max(wp) - min(wp)
    loss = ms_l - ms_p
    rec = {"kind": kind, "workload": name}
    rec.update(cfg)
    rec.update({
        "alternations": alternations, "calls_per_window": calls,
        "plain_ms": round(ms_p, 4), "lse_ms": round(ms_l, 4), "plain_spread_ms": round(spread_p, 4), "lse_spread_ms": round(max(wl) - min(wl), 4),
        "plain_windows": r4(wp), "lse_windows": r4(wl),
        "loss_ms": round(loss, 4), "lse_over_plain": round(ms_l / ms_p, 4),
        "loss_over_plain_spread": round(loss / spread_p, 2) if spread_p > 0 else None,
        "same_bits": same, "lse_finite": finite,
    })
    return rec


def band(nat, tiny, alternations, min_ms):
    from svg.models.hyvideo.utils import sparsity_to_width

    H, D, F_, P_, ctx, L, sparsity = (2, 128, 5, 640, 64, 40, 0.25) if tiny else (24, 128, 33, 3600, 256, 64, 0.25)
    V = F_ * P_
    S = V + ctx
    tf = math.floor(sparsity_to_width(sparsity, ctx, F_, P_) * P_ / 128) * 128
    mask = nat.BandMask(real_len=V + L, band=tf, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    best = (torch.arange(H, device="cuda") % 2).view(1, H)
    o = torch.empty_like(q)
    kw = dict(head_perm_flag=best, vid0=0, num_frame=F_, frame_size=P_, out=o)
    cfg = {"BH": H, "S": S, "D": D, "dtype": "bfloat16", "band": tf, "real_len": V + L, "token_major_heads": int(best.sum())}
    return record(nat, "band", "tiny" if tiny else "hunyuan_720p", cfg, lambda: nat.band_attention(q, k, v, mask, **kw),
                  lambda: nat.band_attention(q, k, v, mask, return_lse=True, **kw), alternations, min_ms)


def varblock(nat, tiny, alternations, min_ms):
    from bench_svg2 import WORKLOADS, clustered
    from svg.kmeans_utils import identify_dynamic_map
    from svg.models import _core

    name = "small" if tiny else "wan720p"
    H, D, F_, P_, ctx, L, QC, KC = WORKLOADS[name]
    assert ctx == 0
    S = F_ * P_
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev).manual_seed(0)
    q = clustered(H, S, D, 64, dev, gen)[None]
    k = clustered(H, S, D, 64, dev, gen)[None]
    v = torch.randn(1, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen)
    store = _core.CentroidStore()
    _core.kmeans_clustering(store, 0, q, k, QC, KC, 50, 2)                       # the first call of a layer: 50 iterations
    (ql, qc, qs, _, qidx), (kl, kc, ks, _, kidx) = _core.kmeans_clustering(store, 0, q, k, QC, KC, 50, 2)
    q_sizes, k_sizes = qs.view(1, H, QC), ks.view(1, H, KC)
    dmap = identify_dynamic_map(qc.view(1, H, QC, D), kc.view(1, H, KC, D), q_sizes, k_sizes, 0.9, 0.1)
    args = (q.view(H, S, D), k.view(H, S, D), v.view(H, S, D), dmap.view(H, QC, KC).contiguous(), q_sizes.view(H, QC).contiguous(),
            k_sizes.view(H, KC).contiguous())
    ws = nat.varblock_workspace(H, H, QC, KC, S, dev)
    kw = dict(q_row_idx=qidx.contiguous(), kv_row_idx=kidx.contiguous(), rows_covered=True, workspace=ws)
    density = float(nat.map_density(dmap.view(H, QC, KC).contiguous(), q_sizes.view(H, QC).contiguous(), k_sizes.view(H, KC).contiguous()).mean())
    cfg = {"Hq": H, "Hkv": H, "S": S, "D": D, "dtype": "bfloat16", "QB": QC, "KB": KC, "map_density": round(density, 4),
           "plain_variant": "-1 (the two-phase 16x16x32 body: S >= 160 QB)" if S >= 160 * QC else "3"}
    variant = -1 if S >= 160 * QC else 3
    return record(nat, "varblock", "tiny" if tiny else "wan_720p_svg2", cfg, lambda: nat.varblock_attention(*args, variant=variant, **kw),
                  lambda: nat.varblock_attention(*args, variant=variant, return_lse=True, **kw), alternations, min_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=1000.0)
    ap.add_argument("--out", default=None, help="default: profiles/sparse_attention_lse_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_sparse_lse: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    out = Path(a.out or ROOT / "profiles" / "sparse_attention_lse_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 5)
    min_ms = 20.0 if a.tiny else a.min_ms
    with out.open("w") as f:
        for fn in (band, varblock):
            line = json.dumps(fn(nat, a.tiny, alternations, min_ms))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
