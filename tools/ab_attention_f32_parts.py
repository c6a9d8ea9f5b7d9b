"""A/B on one box, one process: what handing out fp32 parts costs, and what merging them costs.

    python tools/ab_attention_f32_parts.py [--alternations 7] [--min-ms 300] [--out profiles/attention_f32_parts_ab.jsonl] [--tiny]

The fp32 form (out_dtype=torch.float32: the epilogue stores acc_o * inv as fp32, twice the output bytes) against the 16-bit LSE form
(return_lse=True), alternating, on the same tensors, both from the same library and both allocating their output per call:
  cross     the Wan 720p text cross-attention shape (40 heads, 75 600 x 512, bf16) — _native.cross_attention
  band      HunyuanVideo 720p (24 heads, S = 33 x 3600 + 256 = 119 056, bf16, sparsity 0.25 -> band 15 616, every second head token-major
            through the fused placement: the attention call of bench.py) — _native.band_attention; both forms run the static mapping
and the fp32 merge of 8 parts beside the 16-bit merge of 8 parts (40 heads x 9450 rows, bf16 output, with the merged lse):
  merge     _native.merge_attention_states on fp32 parts / on bf16 parts; algorithmic bytes n x (o_i + lse_i) read, o + lse written
Per comparison: a warm-up of both, then `alternations` (at least 5) rounds of (16-bit window, fp32 window); a window is as many calls
between two device events as make at least `min-ms` of work.  One JSON line per comparison:
  lse16_ms / f32_ms            mean over the windows, *_windows the windows, *_spread_ms = max - min
  f32_over_lse16               the ratio of the means; ratio_min / ratio_max over the alternations (window i against window i)
  same_accumulators            o32.to(T) == o of the 16-bit form and lse bit-identical (attention); merge: *_GBps, *_TBps
No pass / fail number: the forms are opt-in.  --tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import json
import math
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT):
    sys.path.insert(0, str(p))

D = 128
F32 = dict(return_lse=True, out_dtype=torch.float32)


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


def timing(wa, wb, calls, alternations):
    ms_a, ms_b = sum(wa) / len(wa), sum(wb) / len(wb)
    ratios = [b / a for a, b in zip(wa, wb)]
    return {
        "alternations": alternations, "calls_per_window": calls,
        "lse16_ms": round(ms_a, 4), "f32_ms": round(ms_b, 4), "lse16_spread_ms": round(max(wa) - min(wa), 4),
        "f32_spread_ms": round(max(wb) - min(wb), 4), "lse16_windows": r4(wa), "f32_windows": r4(wb),
        "f32_over_lse16": round(ms_b / ms_a, 4), "ratio_min": round(min(ratios), 4), "ratio_max": round(max(ratios), 4),
    }


def attention_record(kind, name, cfg, lse16, f32, alternations, min_ms):
    o, lse = lse16()
    o32, lse32 = f32()
    torch.cuda.synchronize()
    same = bool(torch.equal(o32.to(o.dtype), o)) and bool(torch.equal(lse32, lse))
    del o, lse, o32, lse32
    wa, wb, calls = alternate(lse16, f32, alternations, min_ms)
    rec = {"kind": kind, "workload": name}
    rec.update(cfg)
    rec.update(timing(wa, wb, calls, alternations))
    rec["same_accumulators"] = same
    return rec


def cross(nat, tiny, alternations, min_ms):
    name, BH, Sq, Skv = ("tiny", 2, 700, 77) if tiny else ("wan14b_720p_text", 40, 75600, 512)
    g = torch.Generator(device="cuda").manual_seed(Sq + Skv)
    q = torch.randn(BH, Sq, D, generator=g, device="cuda").to(torch.bfloat16)
    k, v = (torch.randn(BH, Skv, D, generator=g, device="cuda").to(torch.bfloat16) for _ in range(2))
    cfg = {"BH": BH, "Sq": Sq, "Skv": Skv, "D": D, "dtype": "bfloat16", "o16_MB": round(BH * Sq * D * 2 / 1e6, 1), "o32_MB": round(BH * Sq * D * 4 / 1e6, 1)}
    return attention_record("cross", name, cfg, lambda: nat.cross_attention(q, k, v, return_lse=True), lambda: nat.cross_attention(q, k, v, **F32),
                            alternations, min_ms)


def band(nat, tiny, alternations, min_ms):
    from svg.models.hyvideo.utils import sparsity_to_width

    H, F_, P_, ctx, L, sparsity = (2, 5, 640, 64, 40, 0.25) if tiny else (24, 33, 3600, 256, 64, 0.25)
    V = F_ * P_
    S = V + ctx
    tf = math.floor(sparsity_to_width(sparsity, ctx, F_, P_) * P_ / 128) * 128
    mask = nat.BandMask(real_len=V + L, band=tf, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    best = (torch.arange(H, device="cuda") % 2).view(1, H)
    kw = dict(head_perm_flag=best, vid0=0, num_frame=F_, frame_size=P_)
    cfg = {"BH": H, "S": S, "D": D, "dtype": "bfloat16", "band": tf, "real_len": V + L, "token_major_heads": int(best.sum()),
           "o16_MB": round(H * S * D * 2 / 1e6, 1), "o32_MB": round(H * S * D * 4 / 1e6, 1)}
    return attention_record("band", "tiny" if tiny else "hunyuan_720p", cfg, lambda: nat.band_attention(q, k, v, mask, return_lse=True, **kw),
                            lambda: nat.band_attention(q, k, v, mask, **F32, **kw), alternations, min_ms)


def merge(nat, tiny, alternations, min_ms, dtype=torch.bfloat16):
    n, BH, Sq = (8, 2, 300) if tiny else (8, 40, 9450)
    g = torch.Generator(device="cuda").manual_seed(n)
    p32 = [torch.randn(BH, Sq, D, generator=g, device="cuda") for _ in range(n)]
    p16 = [x.to(dtype) for x in p32]
    lse_parts = [torch.randn(BH, Sq, generator=g, device="cuda") for _ in range(n)]
    out = torch.empty_like(p16[0])
    wa, wb, calls = alternate(lambda: nat.merge_attention_states(p16, lse_parts, out=out, return_lse=True),
                              lambda: nat.merge_attention_states(p32, lse_parts, out=out, return_lse=True), alternations, min_ms)
    rec = {"kind": "merge", "workload": "tiny" if tiny else "8_parts_40x9450", "n_parts": n, "BH": BH, "Sq": Sq, "D": D, "out_dtype": "bfloat16"}
    rec.update(timing(wa, wb, calls, alternations))
    o_bytes, l_bytes = BH * Sq * D * 2.0, BH * Sq * 4.0
    b16, b32 = (n + 1) * (o_bytes + l_bytes), n * (2 * o_bytes + l_bytes) + o_bytes + l_bytes
    rec.update({"lse16_MB": round(b16 / 1e6, 2), "f32_MB": round(b32 / 1e6, 2),
                "lse16_TBps": round(b16 / (rec["lse16_ms"] * 1e-3) / 1e12, 3), "f32_TBps": round(b32 / (rec["f32_ms"] * 1e-3) / 1e12, 3),
                "f32_TBps_min": round(b32 / (max(wb) * 1e-3) / 1e12, 3), "f32_TBps_max": round(b32 / (min(wb) * 1e-3) / 1e12, 3)})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--out", default=None, help="default: profiles/attention_f32_parts_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_attention_f32_parts: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    out = Path(a.out or ROOT / "profiles" / "attention_f32_parts_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 5)
    min_ms = 20.0 if a.tiny else a.min_ms
    with out.open("w") as f:
        for fn in (cross, band, merge):
            line = json.dumps(fn(nat, a.tiny, alternations, min_ms))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
