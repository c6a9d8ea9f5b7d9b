"""A/B on one box, one process: svg_cross_attention_pair (_native.cross_attention_pair, token-major output) against the path it replaces
in a Wan I2V block — two svg_cross_attention launches (text keys, image keys; token-major outputs) and torch's add of the two results —
the two paths alternating, on the processors' strided head views of [1, S, H * D] projection outputs.

    python tools/ab_cross_attention_pair.py [--alternations 7] [--calls 50] [--out profiles/cross_attention_pair_ab.jsonl] [--shape NAME] [--tiny]

Per shape: both outputs compared bit for bit, a warm-up of both paths, then `alternations` rounds of (two-launch window, pair window); a
window is at least `calls` calls between two device events (at least ~100 ms of work).  One JSON line per shape:
  two_launch_ms / pair_ms      mean over the windows, *_windows the windows, *_spread_ms = max - min
  pair_wins_every_alternation, gain_ms, gain_over_two_launch_spread, faster (the project's rule: the pair wins every alternation by
                               more than 3 x the two-launch path's own spread)
  min_gain_ms                  the smallest gain of an alternation (what `faster` compares with 3 x the spread)
  outputs_equal                torch.equal of the two paths' outputs at this shape
  pair_GBps                    q twice, o written twice and read once, k and v of both sets once
  clock_recorded               False: the windows carry no shader-clock probe (event times only)
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

# name, H, Sq, Skv text, Skv image, dtype
SHAPES = [
    ("wan14b_720p_i2v", 40, 75600, 512, 257, torch.bfloat16),
    ("wan14b_720p_i2v_fp16", 40, 75600, 512, 257, torch.float16),
    ("wan1.3b_480p_i2v", 12, 32760, 512, 257, torch.bfloat16),
]
TINY = [("tiny", 2, 700, 77, 257, torch.bfloat16), ("tiny_fp16", 2, 300, 64, 40, torch.float16)]


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def head_view(H, S, dtype, g):
    """`proj(x).unflatten(2, (H, -1)).transpose(1, 2)` of a [1, S, H * D] projection output"""
    return torch.randn(1, S, H * D, generator=g, device="cuda").to(dtype).unflatten(2, (H, D)).transpose(1, 2)


def one_shape(nat, name, H, Sq, Skv, Simg, dtype, alternations, min_calls):
    g = torch.Generator(device="cuda").manual_seed(Sq + Skv + Simg)
    q, k, v, k_img, v_img = (head_view(H, S, dtype, g) for S in (Sq, Skv, Skv, Simg, Simg))

    def two_launch():   # the processors' lines: image branch, text branch, each flattened token-major (views), the add of get_o
        o_img = nat.cross_attention(q, k_img, v_img, token_major_out=True).transpose(1, 2).flatten(2, 3)
        o_txt = nat.cross_attention(q, k, v, token_major_out=True).transpose(1, 2).flatten(2, 3)
        return o_txt + o_img

    def pair():
        return nat.cross_attention_pair(q, k, v, k_img, v_img, token_major_out=True).transpose(1, 2).flatten(2, 3)

    a, b = two_launch(), pair()
    torch.cuda.synchronize()
    equal = bool(torch.equal(a, b))
    del a, b
    est = min(window(two_launch, 5), window(pair, 5))                # warm-up of both paths, and the size of a window
    calls = min(max(min_calls, int(math.ceil(100.0 / max(est, 1e-3)))), 20 * min_calls)
    wt, wp = [], []
    for _ in range(alternations):
        wt.append(window(two_launch, calls))
        wp.append(window(pair, calls))
    ms_t, ms_p = sum(wt) / len(wt), sum(wp) / len(wp)
    spread_t, spread_p = max(wt) - min(wt), max(wp) - min(wp)
    gains = [x - y for x, y in zip(wt, wp)]
    nbytes = 2.0 * H * D * (5 * Sq + 2 * Skv + 2 * Simg)
    r4 = lambda xs: [round(x, 4) for x in xs]   # noqa: E731
    return {
        "shape": name, "B": 1, "H": H, "Sq": Sq, "Skv_text": Skv, "Skv_image": Simg, "D": D, "dtype": str(dtype).replace("torch.", ""),
        "alternations": alternations, "calls_per_window": calls, "outputs_equal": equal, "clock_recorded": False,
        "two_launch_ms": round(ms_t, 4), "pair_ms": round(ms_p, 4), "two_launch_spread_ms": round(spread_t, 4), "pair_spread_ms": round(spread_p, 4),
        "two_launch_windows": r4(wt), "pair_windows": r4(wp),
        "pair_wins_every_alternation": all(x > 0 for x in gains), "gain_ms": round(ms_t - ms_p, 4), "min_gain_ms": round(min(gains), 4),
        "gain_over_two_launch_spread": round((ms_t - ms_p) / spread_t, 2) if spread_t > 0 else None,
        "faster": bool(min(gains) > 3 * spread_t),
        "pair_GBps": round(nbytes / (ms_p * 1e-3) / 1e9, 1),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None, help="default: profiles/cross_attention_pair_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--shape", default=None, help="only this shape")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_cross_attention_pair: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    out = Path(a.out or ROOT / "profiles" / "cross_attention_pair_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("w") as f:
        for shape in (TINY if a.tiny else SHAPES):
            if a.shape and shape[0] != a.shape:
                continue
            rec = one_shape(nat, *shape, alternations=2 if a.tiny else max(a.alternations, 7), min_calls=5 if a.tiny else max(a.calls, 50))
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
