"""A/B on one box, one process: svg_cross_attention (_native.cross_attention, token-major output) against the call it replaces in the
Wan / Cosmos processors — torch's scaled_dot_product_attention on the same strided head views — the two paths alternating.

    python tools/ab_cross_attention.py [--alternations 7] [--calls 50] [--out profiles/cross_attention_ab.jsonl] [--shape NAME] [--tiny]
    python tools/ab_cross_attention.py --keyrange [--out profiles/cross_attention_keyrange_ab.jsonl]     (the masked rows, below)

Per shape: a warm-up of both paths, then `alternations` rounds of (SDPA window, kernel window); a window is at least `calls` calls
between two device events (more for the small shapes: at least ~100 ms of work).  One JSON line per shape:
  sdpa_ms / kernel_ms          mean over the windows, *_windows the windows, *_spread = max - min
  kernel_wins_every_alternation, gain_ms, gain_over_sdpa_spread, faster (the project's rule: wins every alternation and
                               gain >= 3 x the SDPA path's own spread)
  kernel_TFLOPs / sdpa_TFLOPs  algorithmic, 4 B H Sq Skv D
  kernel_GBps                  q + o + k + v once
  floor_ms, bound              the larger of FLOPs / 2.5 PFLOP/s (dense bf16 / fp16 MFMA peak) and bytes / 8 TB/s (HBM3E peak)
  rel_l2_vs_sdpa               the two outputs on the same inputs
  varblock_ms                  (Wan 720p text shape only, for the record) _native.varblock_attention on the one-block form of the shape
--keyrange: svg_cross_attention_keyrange (_native.cross_attention_keyrange) at the Wan 720p text shape, one row per set of key windows
(one window per video: a text key-padding mask), THREE calls alternating: SDPA with the equivalent bool [B, 1, 1, Skv] mask, the windowed
kernel, and the unmasked svg_cross_attention over all Skv keys.  The fields above (kernel_* = the windowed kernel, FLOPs and bytes counted
over all Skv keys, so the rows compare with cross_attention_ab.jsonl), plus windows, key_tiles (64-key tiles the windows touch, per video),
unmasked_ms / _spread_ms / _windows, kernel_over_unmasked and kernel_wins_unmasked_every_alternation.
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import json
import math
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT):
    sys.path.insert(0, str(p))

PEAK_FLOPS = 2.5e15    # dense bf16 / fp16 MFMA, spec
PEAK_BYTES = 8.0e12    # HBM3E, spec
D = 128

# name, H, Sq, Skv, dtype, also time the variable-block route
SHAPES = [
    ("wan14b_720p_text", 40, 75600, 512, torch.bfloat16, True),
    ("wan14b_720p_i2v_image", 40, 75600, 257, torch.bfloat16, False),
    ("wan1.3b_480p_text", 12, 32760, 512, torch.bfloat16, False),
    ("small_sq4096", 12, 4096, 512, torch.bfloat16, False),
    ("small_sq1024", 12, 1024, 512, torch.bfloat16, False),
    ("wan14b_720p_text_fp16", 40, 75600, 512, torch.float16, False),
]
TINY = [("tiny", 2, 700, 77, torch.bfloat16, True), ("tiny_fp16", 2, 300, 64, torch.float16, False)]
# name, H, Sq, Skv, dtype, one (begin, end) per video
KEYRANGE = [
    ("wan14b_720p_text_window_0_512", 40, 75600, 512, torch.bfloat16, [(0, 512)]),
    ("wan14b_720p_text_window_0_128", 40, 75600, 512, torch.bfloat16, [(0, 128)]),
    ("wan14b_720p_text_window_0_100", 40, 75600, 512, torch.bfloat16, [(0, 100)]),
    ("wan14b_720p_text_window_412_512", 40, 75600, 512, torch.bfloat16, [(412, 512)]),
    ("wan14b_720p_text_cfg2_ends_100_37", 40, 75600, 512, torch.bfloat16, [(0, 100), (0, 37)]),
]
KEYRANGE_TINY = [("tiny_windows", 2, 700, 77, torch.bfloat16, [(0, 25), (30, 77)])]


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def head_views(H, Sq, Skv, dtype, seed, B=1):
    """q, k, v as the processors build them: `proj(x).unflatten(2, (H, -1)).transpose(1, 2)` views of [B, S, H * D] projection outputs"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda S: torch.randn(B, S, H * D, generator=g, device="cuda").to(dtype).unflatten(2, (H, D)).transpose(1, 2)   # noqa: E731
    return mk(Sq), mk(Skv), mk(Skv)


def one_keyrange(nat, name, H, Sq, Skv, dtype, windows, alternations, min_calls):
    B = len(windows)
    q, k, v = head_views(H, Sq, Skv, dtype, seed=Sq + Skv, B=B)
    begin = torch.tensor([w[0] for w in windows], dtype=torch.int32, device="cuda")
    end = torch.tensor([w[1] for w in windows], dtype=torch.int32, device="cuda")
    mask = torch.zeros(B, 1, 1, Skv, dtype=torch.bool, device="cuda")
    for b, (lo, hi) in enumerate(windows):
        mask[b, 0, 0, lo:hi] = True

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=0.0, is_causal=False)

    def kernel():
        return nat.cross_attention_keyrange(q, k, v, end, begin, token_major_out=True)

    def unmasked():
        return nat.cross_attention(q, k, v, token_major_out=True)

    a, b = sdpa(), kernel()
    torch.cuda.synchronize()
    rel = float((a.float() - b.float()).norm() / a.float().norm())
    del a, b
    est = min(window(sdpa, 5), window(kernel, 5), window(unmasked, 5))
    calls = min(max(min_calls, int(math.ceil(100.0 / max(est, 1e-3)))), 20 * min_calls)
    ws, wk, wu = [], [], []
    for _ in range(alternations):
        ws.append(window(sdpa, calls))
        wk.append(window(kernel, calls))
        wu.append(window(unmasked, calls))
    mean = lambda xs: sum(xs) / len(xs)   # noqa: E731
    ms_s, ms_k, ms_u = mean(ws), mean(wk), mean(wu)
    spread_s = max(ws) - min(ws)
    wins = all(x < y for x, y in zip(wk, ws))
    gain = ms_s - ms_k
    flops = 4.0 * B * H * Sq * Skv * D
    nbytes = 2.0 * B * H * D * (2 * Sq + 2 * Skv)
    r4 = lambda xs: [round(x, 4) for x in xs]   # noqa: E731
    return {
        "shape": name, "B": B, "H": H, "Sq": Sq, "Skv": Skv, "D": D, "dtype": str(dtype).replace("torch.", ""),
        "windows": [list(w) for w in windows], "key_tiles": [(hi - 1) // 64 - lo // 64 + 1 if hi > lo else 0 for lo, hi in windows],
        "alternations": alternations, "calls_per_window": calls,
        "sdpa_ms": round(ms_s, 4), "kernel_ms": round(ms_k, 4), "unmasked_ms": round(ms_u, 4),
        "sdpa_spread_ms": round(spread_s, 4), "kernel_spread_ms": round(max(wk) - min(wk), 4), "unmasked_spread_ms": round(max(wu) - min(wu), 4),
        "sdpa_windows": r4(ws), "kernel_windows": r4(wk), "unmasked_windows": r4(wu),
        "kernel_wins_every_alternation": wins, "gain_ms": round(gain, 4),
        "gain_over_sdpa_spread": round(gain / spread_s, 2) if spread_s > 0 else None,
        "faster": bool(wins and gain >= 3 * spread_s),
        "kernel_over_unmasked": round(ms_k / ms_u, 4), "kernel_wins_unmasked_every_alternation": all(x < y for x, y in zip(wk, wu)),
        "kernel_TFLOPs": round(flops / (ms_k * 1e-3) / 1e12, 1), "sdpa_TFLOPs": round(flops / (ms_s * 1e-3) / 1e12, 1),
        "kernel_GBps": round(nbytes / (ms_k * 1e-3) / 1e9, 1), "rel_l2_vs_sdpa": rel,
    }


def one_shape(nat, name, H, Sq, Skv, dtype, with_varblock, alternations, min_calls):
    q, k, v = head_views(H, Sq, Skv, dtype, seed=Sq + Skv)

    def sdpa():
        return F.scaled_dot_product_attention(q, k, v, attn_mask=None, dropout_p=0.0, is_causal=False)

    def kernel():
        return nat.cross_attention(q, k, v, token_major_out=True)

    a, b = sdpa(), kernel()
    torch.cuda.synchronize()
    rel = float((a.float() - b.float()).norm() / a.float().norm())
    del a, b
    est = min(window(sdpa, 5), window(kernel, 5))                    # warm-up of both paths, and the size of a window
    calls = max(min_calls, int(math.ceil(100.0 / max(est, 1e-3))))
    calls = min(calls, 20 * min_calls)
    ws, wk = [], []
    for _ in range(alternations):
        ws.append(window(sdpa, calls))
        wk.append(window(kernel, calls))
    ms_s, ms_k = sum(ws) / len(ws), sum(wk) / len(wk)
    spread_s, spread_k = max(ws) - min(ws), max(wk) - min(wk)
    wins = all(x < y for x, y in zip(wk, ws))
    gain = ms_s - ms_k
    flops = 4.0 * H * Sq * Skv * D
    nbytes = 2.0 * H * D * (2 * Sq + 2 * Skv)
    t_mfma, t_hbm = flops / PEAK_FLOPS * 1e3, nbytes / PEAK_BYTES * 1e3
    rec = {
        "shape": name, "B": 1, "H": H, "Sq": Sq, "Skv": Skv, "D": D, "dtype": str(dtype).replace("torch.", ""),
        "alternations": alternations, "calls_per_window": calls,
        "sdpa_ms": round(ms_s, 4), "kernel_ms": round(ms_k, 4), "sdpa_spread_ms": round(spread_s, 4), "kernel_spread_ms": round(spread_k, 4),
        "sdpa_windows": [round(x, 4) for x in ws], "kernel_windows": [round(x, 4) for x in wk],
        "kernel_wins_every_alternation": wins, "gain_ms": round(gain, 4),
        "gain_over_sdpa_spread": round(gain / spread_s, 2) if spread_s > 0 else None,
        "faster": bool(wins and gain >= 3 * spread_s),
        "kernel_TFLOPs": round(flops / (ms_k * 1e-3) / 1e12, 1), "sdpa_TFLOPs": round(flops / (ms_s * 1e-3) / 1e12, 1),
        "kernel_GBps": round(nbytes / (ms_k * 1e-3) / 1e9, 1),
        "floor_ms": round(max(t_mfma, t_hbm), 4), "bound": "MFMA" if t_mfma >= t_hbm else "HBM",
        "kernel_share_of_floor": round(max(t_mfma, t_hbm) / ms_k, 3), "rel_l2_vs_sdpa": rel,
    }
    if with_varblock:   # for the record only: the one-block form of the shape on the variable-block entry (plan, launch order, workspace per call)
        try:
            ones = torch.ones(H, 1, 1, dtype=torch.bool, device="cuda")
            qs = torch.full((H, 1), Sq, dtype=torch.int32, device="cuda")
            ks = torch.full((H, 1), Skv, dtype=torch.int32, device="cuda")

            def varblock():
                return nat.varblock_attention(q, k, v, ones, qs, ks, token_major_out=True, rows_covered=True)

            window(varblock, 3)
            rec["varblock_ms"] = round(sum(window(varblock, calls) for _ in range(3)) / 3, 4)
        except Exception as e:  # noqa: BLE001
            rec["varblock_ms"] = None
            rec["varblock_error"] = str(e)[:200]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None, help="default: profiles/cross_attention_ab.jsonl, with --keyrange profiles/cross_attention_keyrange_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--keyrange", action="store_true", help="the masked rows: svg_cross_attention_keyrange against SDPA with the bool mask and the unmasked kernel")
    ap.add_argument("--shape", default=None, help="only this shape (a kernel trace of one shape: rocprofv3 --kernel-trace --stats -- python ...)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_cross_attention: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    out = Path(a.out or ROOT / "profiles" / ("cross_attention_keyrange_ab.jsonl" if a.keyrange else "cross_attention_ab.jsonl"))
    out.parent.mkdir(parents=True, exist_ok=True)
    shapes = (KEYRANGE_TINY if a.tiny else KEYRANGE) if a.keyrange else (TINY if a.tiny else SHAPES)
    with out.open("w") as f:
        for shape in shapes:
            if a.shape and shape[0] != a.shape:
                continue
            rec = (one_keyrange if a.keyrange else one_shape)(nat, *shape, alternations=2 if a.tiny else max(a.alternations, 7),
                                                              min_calls=5 if a.tiny else max(a.calls, 50))
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
