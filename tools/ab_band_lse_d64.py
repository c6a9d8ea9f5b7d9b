"""A/B on one box, one process: band attention at head_dim 64 with the row log-sum-exp / fp32 rows (include/svg_attn_band_lse_d64.h) against
the plain head_dim-64 entry of the PARENT library, at the CogVideoX geometries.

    python tools/ab_band_lse_d64.py --parent <libsvgattn.so of the parent commit> [--alternations 7] [--min-ms 500]
                                    [--out profiles/band_lse_d64_ab.jsonl] [--tiny]

Workloads: CogVideoX-v1.5 (11 frames x 4080 rows + 226 text rows, S = 45 106) and v1 480p (13 x 1350 + 226, S = 17 776), 96 heads (cfg 2 x
48), bf16, sparsity 0.25 through the processors' mask (svg/models/cog/utils.py), every second head token-major through the fused placement.
Both libraries are loaded side by side through ctypes and called on the same tensors.  Per pair: a warm-up, then `alternations` (at least
5) rounds of (A window, B window), a window being as many calls between two device events as make `min-ms` of work, with the shader clock
granted to each window (svg._native.ClockProbe; null where the counters do not move).  One JSON line per pair, A = svg_band_attention of
the parent throughout:
  lse_vs_parent_plain    B = svg_band_attention_lse_d64 of this build: what the lse store costs; same_bits compares o
  f32_vs_parent_plain    B = svg_band_attention_lse_d64_f32: fp32 rows (twice the output bytes) in the place of o; same_bits compares
                         o32 rounded to bf16 with o
  plain_vs_parent        B = svg_band_attention of this build: expected bit-identical and inside A's own spread
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

PLAIN, LSE, F32 = "svg_band_attention", "svg_band_attention_lse_d64", "svg_band_attention_lse_d64_f32"


def typed(nat, path, names):
    lib = C.CDLL(str(Path(path).resolve()))
    sigs = {**nat.SIGNATURES, **nat.BAND_LSE_D64_ENTRIES}
    for name in names:
        getattr(lib, name).restype, getattr(lib, name).argtypes = sigs[name]
    return lib


def run_workload(nat, name, H, ctx, F_, P_, old, new, alternations, min_ms, probe):
    from svg.models.cog.utils import generate_temporal_head_mask_mod
    from svg.models.hyvideo.utils import sparsity_to_width

    D, S = 64, ctx + F_ * P_
    mask = generate_temporal_head_mask_mod(ctx, F_, P_, mul=sparsity_to_width(0.25, ctx, F_, P_))
    g = torch.Generator(device="cuda").manual_seed(77)
    q, k, v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    best = (torch.arange(H, device="cuda") % 2).to(torch.int64).contiguous()
    perm = nat.PermDesc(best.data_ptr(), ctx, F_, P_)   # (text first: the video starts at row ctx)
    o = [torch.empty_like(q) for _ in range(2)]
    o32 = torch.empty(1, H, S, D, dtype=torch.float32, device="cuda")
    lse = torch.empty(1, H, S, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    mid = (H, S, D, 0, 1.0 / math.sqrt(D), C.byref(mask), C.byref(perm))

    def call(lib, entry, out):
        fn = getattr(lib, entry)
        args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()) + ((lse.data_ptr(),) if entry != PLAIN else ()) + mid + (
            (0, st) if entry == PLAIN else (None, st))

        def run():
            rc = fn(*args)
            if rc != 0:
                raise RuntimeError(f"{entry}: error {rc}")
        return run

    recs = []
    for label, entry, out in (("lse_vs_parent_plain", LSE, o[1]), ("f32_vs_parent_plain", F32, o32), ("plain_vs_parent", PLAIN, o[1])):
        fa, fb = call(old, PLAIN, o[0]), call(new, entry, out)
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
        rec = {"pair": label, "workload": name, "a": "parent: " + PLAIN, "b": "this build: " + entry, "BH": H, "S": S, "D": D,
               "dtype": "bfloat16", "band": mask.band, "alternations": alternations, "calls_per_window": calls, "a_side": sa, "b_side": sb,
               "b_over_a": round(sb["ms"] / sa["ms"], 4), "diff_ms": round(diff, 4), "inside_a_spread": bool(abs(diff) <= sa["spread_ms"]),
               "same_bits": same, "lse_finite": finite}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libsvgattn.so built from the parent commit")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/band_lse_d64_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_band_lse_d64: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    new, old = typed(nat, nat.lib_path(), [PLAIN, LSE, F32]), typed(nat, a.parent, [PLAIN])
    probe = nat.ClockProbe(torch.device("cuda"))
    alternations, min_ms = (2, 10.0) if a.tiny else (max(a.alternations, 5), a.min_ms)
    loads = [("tiny", 2, 26, 4, 180)] if a.tiny else [("cogvideox15_768p", 96, 226, 11, 4080), ("cogvideox1_480p", 96, 226, 13, 1350)]
    out = Path(a.out or ROOT / "profiles" / "band_lse_d64_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as f:
        for name, H, ctx, F_, P_ in loads:
            for rec in run_workload(nat, name, H, ctx, F_, P_, old, new, alternations, min_ms, probe):
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
