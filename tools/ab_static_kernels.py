#!/usr/bin/env python3
"""Same-box A/B of two builds of the library on the kernels a refactoring touched without changing their schedule — the statically
mapped band_attn_m16_kernel (the launch that counts completions, HunyuanVideo 720p) and varblock_attn_m16_kernel (the production-size
SVG2 cases of tests/test_gpu_fullsize_svg2.py): alternating spans as in tools/ab_band_queue.py, outputs compared with torch.equal.
    python tools/ab_static_kernels.py [lib A, default lib/libsvgattn_parent.so] [lib B, default lib/libsvgattn.so]"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "sparse-videogen_amd"))
sys.path.insert(0, str(ROOT))
import ab_band_queue as ab  # noqa: E402
import torch  # noqa: E402
from svg import _native as nat  # noqa: E402

L = ROOT / "sparse-videogen_amd" / "lib"
ab.LIBS["A"] = str(Path(sys.argv[1]).resolve()) if len(sys.argv) > 1 else str(L / "libsvgattn_parent.so")
ab.LIBS["B"] = str(Path(sys.argv[2]).resolve()) if len(sys.argv) > 2 else str(L / "libsvgattn.so")
dev = torch.device("cuda", 0)
ab.use("A")
probe = nat.ClockProbe(dev)


def alternate(name, fns, outs, reps=7, calls=3):
    for t in "AB":
        ab.use(t)
        fns[t]()
        fns[t]()
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["A"], outs["B"]))
    ms = {"A": [], "B": []}
    mhz = {"A": [], "B": []}
    for rep in range(-1, reps):
        for t in "AB":
            ab.use(t)
            a, b = ab.one_repeat(fns[t], calls, probe)
            if rep >= 0:
                ms[t].append(round(a, 4))
                mhz[t].append(b)
    mean = lambda x: sum(x) / len(x)
    cyc = {t: [a * b for a, b in zip(ms[t], mhz[t])] for t in "AB"}
    print(json.dumps({"case": name, "ms_A": ms["A"], "ms_B": ms["B"], "mhz_A": mhz["A"], "mhz_B": mhz["B"], "spread_A_ms": round(max(ms["A"]) - min(ms["A"]), 4),
                      "ratio_ms": round(mean(ms["B"]) / mean(ms["A"]), 5), "ratio_cycles": round(mean(cyc["B"]) / mean(cyc["A"]), 5),
                      "bit_identical": same}), flush=True)


# statically mapped band kernel: the counting launch on the headline inputs
q, k, v, mask, pk, band = ab.case_inputs(dev, list(range(24)), 33, 3600, 256, 64, 0.25)
outs = {t: torch.empty_like(q) for t in "AB"}
done = nat.notify_counters(24, 1, dev)


def band_static(t):
    done.zero_()
    return nat.band_attention(q, k, v, mask, out=outs[t], done=done, done_nseg=1, **pk)


alternate("hy720p band, counting launch (static mapping)", {t: (lambda t=t: band_static(t)) for t in "AB"}, outs)
del q, k, v, outs
torch.cuda.empty_cache()
from tests.test_gpu_fullsize_svg2 import build_case  # noqa: E402

for name in ("wan720p", "hy720p"):
    c = build_case(name)
    res = {}

    def vb(t):
        res[t] = nat.varblock_attention(c["q"], c["k"], c["v"], c["dmap"], c["q_sizes"], c["k_sizes"], q_row_idx=c["qidx"], kv_row_idx=c["kidx"])
        return res[t]

    for t in "AB":
        ab.use(t)
        vb(t)
    outs = {t: res[t].clone() for t in "AB"}

    alternate(f"varblock {name} (bf16, fused permutation)", {t: (lambda t=t: outs[t].copy_(vb(t))) for t in "AB"}, outs)
    del c
    torch.cuda.empty_cache()
