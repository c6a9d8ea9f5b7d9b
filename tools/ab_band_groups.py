#!/usr/bin/env python3
"""What a launch per group of videos costs (svg_band_groups_attention) at HunyuanVideo 720p, bf16, cfg = 2 — in ONE process on the
same inputs, the three forms alternating:

    python tools/ab_band_groups.py [--reps 5] [--calls 3] [--out profiles/band_groups_ab.jsonl]

  grouped   band_attention_groups with the prompt lengths (37, 256): two groups of 24 heads, one call;
  singles   the two single-mask calls it stands for (band_attention on each video's 24 heads with that video's mask);
  one       ONE single-mask launch over both videos with equal lengths (256, 256): what a mask per head inside one launch could at best
            look like — it does a little MORE arithmetic than the two above (video 0 gets 219 more prompt rows and columns).

`grouped` and `singles` are the same launches and should agree within the run's own spread; `singles - one` is what a single launch
over both videos would save.  24 heads seeded per head as in bench.py, alternating spatial / temporal heads, sparsity 0.25.  One
alternation that is not recorded, then `reps` alternations; a repeat is `calls` calls between two HIP events.  The grouped output is
compared with the two single-mask outputs by torch.equal.  One JSON line, printed and appended to --out."""
import argparse
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "sparse-videogen_amd"))
sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from svg import _native as nat  # noqa: E402
from svg.models.hyvideo.utils import sparsity_to_width  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--lengths", default="37,256")
    ap.add_argument("--geometry", default="33,3600,256", help="frames, tokens per frame, text tokens (720p: 33,3600,256)")
    ap.add_argument("--out", default="", help="the JSON line is appended to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_band_groups.py measures on the GPU: none visible")
    dev = torch.device("cuda", 0)
    F_, P_, ctx = (int(x) for x in a.geometry.split(","))
    lens = tuple(int(x) for x in a.lengths.split(","))
    cfg, H, D = len(lens), 24, 128
    V = F_ * P_
    S = V + ctx
    band = math.floor(sparsity_to_width(0.25, ctx, F_, P_) * P_ / 128) * 128

    def mask(p):
        return nat.BandMask(real_len=V + p, band=band, colfull_lo=V, colfull_hi=V + p, rowfull_lo=V, rowfull_hi=V + p)

    def head_rows(c, h, which):   # bench.py head_rows, another stream per video
        gh = torch.Generator(device=dev).manual_seed(7919 * (3 * (c * H + h) + which) + 1234)
        return torch.randn(S, D, device=dev, dtype=torch.bfloat16, generator=gh)

    q, k, v = (torch.stack([torch.stack([head_rows(c, h, w) for h in range(H)]) for c in range(cfg)]) for w in range(3))
    best = torch.tensor([[h % 2 for h in range(H)]] * cfg, device=dev, dtype=torch.int64)
    pk = dict(vid0=0, num_frame=F_, frame_size=P_)
    outs = {t: torch.full_like(q, float("nan")) for t in ("grouped", "singles", "one")}
    masks = [mask(p) for p in lens]

    def grouped():
        nat.band_attention_groups(q, k, v, masks, [H] * cfg, head_perm_flag=best, out=outs["grouped"], **pk)

    def singles():
        for c in range(cfg):
            nat.band_attention(q[c:c + 1], k[c:c + 1], v[c:c + 1], masks[c], head_perm_flag=best[c:c + 1], out=outs["singles"][c:c + 1], **pk)

    def one():
        nat.band_attention(q, k, v, mask(max(lens)), head_perm_flag=best, out=outs["one"], **pk)

    fn = {"grouped": grouped, "singles": singles, "one": one}
    for f in fn.values():   # warm-up: code objects, LDS attribute, counter pool
        f()
        f()
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["grouped"], outs["singles"])) and not bool(torch.isnan(outs["grouped"]).any())
    ms = {t: [] for t in fn}
    for rep in range(-1, a.reps):   # (alternation -1 is not recorded: the clock settles during the first spans after an idle stretch)
        for t, f in fn.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            e1.synchronize()
            if rep >= 0:
                ms[t].append(e0.elapsed_time(e1) / a.calls)
    mean = lambda x: sum(x) / len(x)   # noqa: E731
    res = {
        "case": "hy_band_groups", "dtype": "bf16", "cfg": cfg, "heads": H, "S": S, "band": band, "lengths": list(lens), "reps": a.reps,
        "calls_per_repeat": a.calls, **{f"ms_{t}": [round(x, 4) for x in ms[t]] for t in fn},
        **{f"mean_ms_{t}": round(mean(ms[t]), 4) for t in fn},
        **{f"spread_ms_{t}": round(max(ms[t]) - min(ms[t]), 4) for t in fn},
        "grouped_minus_singles_ms": round(mean(ms["grouped"]) - mean(ms["singles"]), 4),
        "singles_minus_one_ms": round(mean(ms["singles"]) - mean(ms["one"]), 4),
        "ratio_singles_over_one": round(mean(ms["singles"]) / mean(ms["one"]), 5),
        "grouped_bit_identical_to_singles": same,
    }
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(res) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
