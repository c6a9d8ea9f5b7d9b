"""A/B on one box, one process: what the row log-sum-exp costs, and what the N-way merge costs.

    python tools/ab_cross_attention_lse.py [--alternations 7] [--calls 50] [--out profiles/cross_attention_lse_ab.jsonl] [--tiny]

LSE form against the plain entry (kind "lse"): _native.cross_attention(q, k, v) and _native.cross_attention(q, k, v, return_lse=True)
alternating, on the same tensors, both from the same library (the plain kernel's listing is the parent's,
profiles/cross_attention_lse_asm_diff.txt).  Per shape: a warm-up of both, then `alternations` rounds of (plain window, LSE window); a
window is at least `calls` calls between two device events (at least ~100 ms of work).  One JSON line per shape:
  plain_ms / lse_ms            mean over the windows, *_windows the windows, *_spread_ms = max - min
  loss_ms, loss_over_plain_spread, lse_within_3_spreads   (the LSE form is opt-in; it is expected inside the plain entry's own spread)
  same_bits                    o of the two forms
Merge kernel (kind "merge"): _native.merge_attention_states on n contiguous parts, with the merged lse, against torch's copy of one part
(`out.copy_(part)`: the measured copy rate of the same process, same tensors).  One JSON line per n:
  merge_ms, merge_GBps         algorithmic bytes: n x (o + lse) read, o + lse written
  copy_ms, copy_GBps           2 x o bytes
  merge_over_copy_rate, spec_copy_GBps (6290: the float4 copy of the microarchitecture guide, bench_hbm.py)
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

D = 128
PEAK_COPY_GBS = 6290.0
# name, BH, Sq, Skv, dtype
LSE_SHAPES = [
    ("wan14b_720p_text", 40, 75600, 512, torch.bfloat16),
    ("self_attention_shard_8ranks", 24, 14976, 14976, torch.bfloat16),
]
LSE_TINY = [("tiny", 2, 700, 77, torch.bfloat16)]
# n, BH, Sq
MERGE_SHAPES = [(2, 40, 9450), (8, 40, 9450)]
MERGE_TINY = [(2, 2, 300), (8, 2, 300)]


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def alternate(fa, fb, alternations, min_calls):
    est = min(window(fa, 3), window(fb, 3))
    calls = min(max(min_calls, int(math.ceil(100.0 / max(est, 1e-3)))), 20 * min_calls)
    wa, wb = [], []
    for _ in range(alternations):
        wa.append(window(fa, calls))
        wb.append(window(fb, calls))
    return wa, wb, calls


def r4(xs):
    return [round(x, 4) for x in xs]


def one_lse(nat, name, BH, Sq, Skv, dtype, alternations, min_calls):
    g = torch.Generator(device="cuda").manual_seed(Sq + Skv)
    q = torch.randn(BH, Sq, D, generator=g, device="cuda").to(dtype)
    k, v = (torch.randn(BH, Skv, D, generator=g, device="cuda").to(dtype) for _ in range(2))
    o = torch.empty_like(q)

    def plain():
        return nat.cross_attention(q, k, v, out=o)

    def with_lse():
        return nat.cross_attention(q, k, v, out=o, return_lse=True)

    a = plain().clone()
    b, lse = with_lse()
    torch.cuda.synchronize()
    same = bool(torch.equal(a, b)) and bool(torch.isfinite(lse).all())
    del a
    wp, wl, calls = alternate(plain, with_lse, alternations, min_calls)
    ms_p, ms_l = sum(wp) / len(wp), sum(wl) / len(wl)
    spread_p = max(wp) - min(wp)
    loss = ms_l - ms_p
    flops = 4.0 * BH * Sq * Skv * D
    return {
        "kind": "lse", "shape": name, "BH": BH, "Sq": Sq, "Skv": Skv, "D": D, "dtype": str(dtype).replace("torch.", ""),
        "alternations": alternations, "calls_per_window": calls,
        "plain_ms": round(ms_p, 4), "lse_ms": round(ms_l, 4), "plain_spread_ms": round(spread_p, 4), "lse_spread_ms": round(max(wl) - min(wl), 4),
        "plain_windows": r4(wp), "lse_windows": r4(wl),
        "loss_ms": round(loss, 4), "loss_over_plain_spread": round(loss / spread_p, 2) if spread_p > 0 else None,
        "lse_within_3_spreads": bool(loss <= 3 * spread_p),
        "plain_TFLOPs": round(flops / (ms_p * 1e-3) / 1e12, 1), "lse_TFLOPs": round(flops / (ms_l * 1e-3) / 1e12, 1), "same_bits": same,
    }


def one_merge(nat, n, BH, Sq, alternations, min_calls, dtype=torch.bfloat16):
    g = torch.Generator(device="cuda").manual_seed(n)
    o_parts = [torch.randn(BH, Sq, D, generator=g, device="cuda").to(dtype) for _ in range(n)]
    lse_parts = [torch.randn(BH, Sq, generator=g, device="cuda") for _ in range(n)]
    out = torch.empty_like(o_parts[0])

    def merge():
        return nat.merge_attention_states(o_parts, lse_parts, out=out, return_lse=True)

    def copy():
        return out.copy_(o_parts[0])

    wm, wc, calls = alternate(merge, copy, alternations, min_calls)
    ms_m, ms_c = sum(wm) / len(wm), sum(wc) / len(wc)
    o_bytes, l_bytes = BH * Sq * D * 2.0, BH * Sq * 4.0
    nbytes = (n + 1) * (o_bytes + l_bytes)
    gbps_m, gbps_c = nbytes / (ms_m * 1e-3) / 1e9, 2 * o_bytes / (ms_c * 1e-3) / 1e9
    return {
        "kind": "merge", "n_parts": n, "BH": BH, "Sq": Sq, "D": D, "dtype": str(dtype).replace("torch.", ""),
        "alternations": alternations, "calls_per_window": calls,
        "merge_ms": round(ms_m, 4), "merge_spread_ms": round(max(wm) - min(wm), 4), "merge_windows": r4(wm),
        "copy_ms": round(ms_c, 4), "copy_spread_ms": round(max(wc) - min(wc), 4), "copy_windows": r4(wc),
        "algorithmic_MB": round(nbytes / 1e6, 2), "merge_GBps": round(gbps_m, 1), "copy_GBps": round(gbps_c, 1),
        "merge_over_copy_rate": round(gbps_m / gbps_c, 3), "spec_copy_GBps": PEAK_COPY_GBS,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None, help="default: profiles/cross_attention_lse_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_cross_attention_lse: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    out = Path(a.out or ROOT / "profiles" / "cross_attention_lse_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 7)
    min_calls = 5 if a.tiny else max(a.calls, 50)
    with out.open("w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()

        for shape in (LSE_TINY if a.tiny else LSE_SHAPES):
            emit(one_lse(nat, *shape, alternations=alternations, min_calls=min_calls))
        for shape in (MERGE_TINY if a.tiny else MERGE_SHAPES):
            emit(one_merge(nat, *shape, alternations=alternations, min_calls=min_calls))


if __name__ == "__main__":
    main()
