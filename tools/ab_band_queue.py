#!/usr/bin/env python3
"""Same-box A/B of the band attention launch of two builds of the library, in ONE process on the same inputs — made for the work
queue of the 16x16x32 band kernels (csrc/band_policy.h BandQueue) against the static mapping of the commit before it:

    python sparse-videogen_amd/build.py --tag parent            # in a checkout of the other commit; copy lib/libsvgattn_parent.so here
    python tools/ab_band_queue.py sparse-videogen_amd/lib/libsvgattn_parent.so [sparse-videogen_amd/lib/libsvgattn.so]
                                  [--reps 5] [--calls 3] [--heads alt|spatial|temporal] [--out profiles/band_queue_ab.jsonl]

Cases: bench.py's headline inputs (HunyuanVideo 720p, 24 heads seeded per head as there, alternating spatial / temporal heads — or, with
--heads, all contiguous (spatial) or all token-major (temporal): what a change in the row stepping of one kind of head shows on), the
480p geometry, and a 3-head launch of the 720p geometry (one rank's share at N = 8).  Per case the two libraries alternate A, B, A, B ...
`reps` times each after one alternation that is not recorded; a repeat is `calls` attention calls between two HIP events, with the granted shader clock of the span beside it
(nat.ClockProbe), so that cycles = ms x MHz are reported too.  The outputs of the two libraries are compared with torch.equal.
Printed and written as one JSON line per case:
  spread   max - min of A against itself over its repeats (what drift and noise do on this box in this call);
  gain     mean(A) - mean(B); `claimed` only if B is faster than A in EVERY alternation and gain >= 3 x spread;
  ratio    mean(B) / mean(A), for ms and for cycles."""
import argparse
import ctypes
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

LIBS = {}


def use(tag):
    """point svg._native at library `tag`; a library of an older commit may lack entry points this checkout declares"""
    if not isinstance(LIBS[tag], ctypes.CDLL):
        lib = ctypes.CDLL(LIBS[tag])
        for name, (res, args) in nat.SIGNATURES.items():
            fn = getattr(lib, name, None)
            if fn is not None:
                fn.restype, fn.argtypes = res, args
        assert int(lib.svg_abi_version()) == nat.SVG_ABI_VERSION
        LIBS[tag] = lib
    nat._lib = LIBS[tag]


HEAD_PATTERNS = {"alt": lambda h: h % 2, "spatial": lambda h: 0, "temporal": lambda h: 1}


def case_inputs(dev, heads, F_, P_, ctx, L, sparsity, pattern="alt"):
    D = 128
    V = F_ * P_
    S = V + ctx
    tf = math.floor(sparsity_to_width(sparsity, ctx, F_, P_) * P_ / 128) * 128
    mask = nat.BandMask(real_len=V + L, band=tf, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)

    def head_rows(h, which):   # bench.py head_rows
        gh = torch.Generator(device=dev).manual_seed(7919 * (3 * h + which) + 1234)
        return torch.randn(S, D, device=dev, dtype=torch.bfloat16, generator=gh)

    q, k, v = (torch.stack([head_rows(h, w) for h in heads])[None] for w in range(3))
    best = torch.tensor([[HEAD_PATTERNS[pattern](h) for h in heads]], device=dev, dtype=torch.int64)
    return q, k, v, mask, dict(head_perm_flag=best, vid0=0, num_frame=F_, frame_size=P_), tf


def one_repeat(fn, calls, probe):
    probe.start(max_ms=3000)   # (a span is a few calls of tens of ms)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    probe.arm_stop()
    e1.synchronize()
    mhz = probe.result()
    return e0.elapsed_time(e1) / calls, mhz


def run_case(name, dev, heads, geo, reps, calls, probe, pattern="alt"):
    q, k, v, mask, pk, band = case_inputs(dev, heads, *geo, pattern=pattern)
    outs = {t: torch.full_like(q, float("nan")) for t in "AB"}
    fn = {t: (lambda t=t: nat.band_attention(q, k, v, mask, out=outs[t], **pk)) for t in "AB"}
    for t in "AB":   # warm-up: code objects, LDS attribute, counter pool
        use(t)
        fn[t]()
        fn[t]()
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["A"], outs["B"])) and not bool(torch.isnan(outs["B"]).any())
    rows_differ = int((outs["A"] != outs["B"]).any(dim=-1).sum())
    rel_l2 = float((outs["A"].float() - outs["B"].float()).norm() / outs["A"].float().norm())
    ms, mhz = {"A": [], "B": []}, {"A": [], "B": []}
    for rep in range(-1, reps):   # (alternation -1 is not recorded: the clock settles during the first spans after an idle stretch)
        for t in "AB":
            use(t)
            a, b = one_repeat(fn[t], calls, probe)
            if rep >= 0:
                ms[t].append(a)
                mhz[t].append(b)
    cyc = {t: [a * b * 1e-3 if b else float("nan") for a, b in zip(ms[t], mhz[t])] for t in "AB"}   # Mcycles
    mean = lambda x: sum(x) / len(x)   # noqa: E731
    spread = max(ms["A"]) - min(ms["A"])
    gain = mean(ms["A"]) - mean(ms["B"])
    every = all(b < a for a, b in zip(ms["A"], ms["B"]))
    res = {
        "case": name, "head_pattern": pattern, "heads": len(heads), "S": int(q.shape[2]), "band": band, "reps": reps, "calls_per_repeat": calls,
        "ms_A": [round(x, 4) for x in ms["A"]], "ms_B": [round(x, 4) for x in ms["B"]],
        "mhz_A": mhz["A"], "mhz_B": mhz["B"],
        "mcycles_A": [round(x, 3) for x in cyc["A"]], "mcycles_B": [round(x, 3) for x in cyc["B"]],
        "spread_A_ms": round(spread, 4), "gain_ms": round(gain, 4), "B_faster_in_every_alternation": every,
        "claimed": bool(every and gain >= 3 * spread),
        "ratio_ms": round(mean(ms["B"]) / mean(ms["A"]), 5), "ratio_cycles": round(mean(cyc["B"]) / mean(cyc["A"]), 5),
        "bit_identical": same, "rows_that_differ": rows_differ, "rel_l2_A_B": rel_l2,
        "median_gain_ms": round(sorted(a - b for a, b in zip(ms["A"], ms["B"]))[len(ms["A"]) // 2], 4),
    }
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("lib_a")
    ap.add_argument("lib_b", nargs="?", default=str(ROOT / "sparse-videogen_amd" / "lib" / "libsvgattn.so"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--cases", default="hy720p,hy480p,hy720p_3_heads")
    ap.add_argument("--heads", default="alt", choices=sorted(HEAD_PATTERNS), help="which heads are token-major")
    ap.add_argument("--allow-different-bits", action="store_true", help="exit 0 also when the two outputs differ (they are reported)")
    ap.add_argument("--out", default="", help="JSON lines are appended to this file")
    a = ap.parse_args()
    LIBS["A"], LIBS["B"] = str(Path(a.lib_a).resolve()), str(Path(a.lib_b).resolve())
    dev = torch.device("cuda", 0)
    cases = {"hy720p": (list(range(24)), (33, 3600, 256, 64, 0.25)), "hy480p": (list(range(24)), (33, 1350, 256, 64, 0.25)),
             "hy720p_3_heads": ([0, 1, 2], (33, 3600, 256, 64, 0.25)), "tiny": ([0, 1, 2, 3], (5, 600, 256, 64, 0.4))}
    results = []
    use("A")
    # ONE probe for the whole run: every probe owns two streams, and the streams of a second one can land on the hardware queue of
    # the stream that carries the attention calls — which then wait behind the sleeping probe until its time limit
    probe = nat.ClockProbe(dev)
    for name in a.cases.split(","):
        heads, geo = cases[name]
        results.append(run_case(name, dev, heads, geo, a.reps, a.calls, probe, a.heads))
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps({"A": str(a.lib_a), "B": str(a.lib_b)}) + "\n")
            for r in results:
                f.write(json.dumps(r) + "\n")
    return 0 if a.allow_different_bits or all(r["bit_identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
