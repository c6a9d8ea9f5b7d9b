"""A/B on one box, one process: the LSE forms of the production launch forms of band attention (include/svg_attn_band_lse_forms.h, and
svg_band_attention_lse on the work queue) at HunyuanVideo 720p.

    python tools/ab_band_lse_forms.py --parent <libsvgattn.so of the parent commit> [--alternations 7] [--min-ms 1000]
                                      [--out profiles/band_lse_forms_ab.jsonl] [--tiny]

Workload: 24 heads, S = 33 x 3600 + 256 = 119 056, bf16, sparsity 0.25 -> band 15 616, every second head token-major through the fused
placement (the attention call of bench.py).  Both libraries are loaded side by side (ctypes handles of different files are independent,
as tools/ab_bitexact.py loads two builds) and called through the same ctypes signatures on the same tensors.  Per pair: a warm-up of
both, then `alternations` (at least 5) rounds of (A window, B window); a window is as many calls between two device events as make at
least `min-ms` of work.  One JSON line per pair, A the yardstick and B what is asked about:
  a  lse_vs_parent       A = svg_band_attention_lse of the parent (static mapping), B = of this build (work queue).  `gain` is claimed by
                         the project's rule only: B faster in every alternation and by at least 3 x A's own spread.
  b  lse_vs_plain        A = svg_band_attention, B = svg_band_attention_lse, both of this build, both on the queue: what the store costs.
  c  switch_lse_vs_plain A = svg_band_attention_switch, B = svg_band_attention_switch_lse, this build, flag 0 (a sparse step; both on the
                         static mapping).
  plain_vs_parent, switch_vs_parent   the plain entries of this build (B) against the parent's (A): bit-identical, ratio inside A's spread.
Fields: a_ms / b_ms (mean over the windows), *_windows, *_spread_ms = max - min, b_over_a, diff_ms, diff_over_a_spread,
inside_a_spread (|diff| <= A's spread), b_faster_in_every_alternation, same_bits (o of A and B), and for the LSE pairs lse_same_bits /
lse_finite.  The shader clock is not recorded.
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

from ab_sparse_lse import alternate, r4  # noqa: E402  (tools/ is sys.path[0] when this file is run as a script)


class Lib:
    """one build of the library with the three band entries this tool calls typed (the parent lacks the newer symbols: no nat.load())"""

    def __init__(self, nat, path, names):
        self.path = str(Path(path).resolve())
        self.lib = C.CDLL(self.path)
        sigs = {**nat.SIGNATURES, **nat.SPARSE_LSE_SIGNATURES, **nat.BAND_LSE_FORM_SIGNATURES}
        for name in names:
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = sigs[name]


def workload(nat, tiny):
    from svg.models.hyvideo.utils import sparsity_to_width

    H, D, F_, P_, ctx, L, sparsity = (2, 128, 5, 640, 64, 40, 0.25) if tiny else (24, 128, 33, 3600, 256, 64, 0.25)
    V = F_ * P_
    S = V + ctx
    tf = math.floor(sparsity_to_width(sparsity, ctx, F_, P_) * P_ / 128) * 128
    w = argparse.Namespace(H=H, S=S, D=D)
    w.mask = nat.BandMask(real_len=V + L, band=tf, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    w.alt = nat.BandMask(real_len=V + L, band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
    g = torch.Generator(device="cuda").manual_seed(0)
    w.q, w.k, w.v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    w.best = (torch.arange(H, device="cuda") % 2).view(1, H).to(torch.int64).contiguous()
    w.perm = nat.PermDesc(w.best.data_ptr(), 0, F_, P_)
    w.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    w.o = [torch.empty_like(w.q) for _ in range(2)]                                           # one output per side of a pair
    w.lse = [torch.empty(1, H, S, dtype=torch.float32, device="cuda") for _ in range(2)]
    w.cfg = {"BH": H, "S": S, "D": D, "dtype": "bfloat16", "band": tf, "real_len": V + L, "token_major_heads": int(w.best.sum())}
    return w


def call(lib, entry, w, side):
    """-> a function that launches `entry` of `lib` into output `side` on the current stream"""
    fn = getattr(lib.lib, entry)
    st = torch.cuda.current_stream().cuda_stream
    head = (w.q.data_ptr(), w.k.data_ptr(), w.v.data_ptr(), w.o[side].data_ptr())
    mid = (w.H, w.S, w.D, 0, 1.0 / math.sqrt(w.D), C.byref(w.mask), C.byref(w.perm))
    tail = {"svg_band_attention": (0, st), "svg_band_attention_lse": (None, st),
            "svg_band_attention_switch": (C.byref(w.alt), w.flag.data_ptr(), st),
            "svg_band_attention_switch_lse": (C.byref(w.alt), w.flag.data_ptr(), None, st)}[entry]
    args = head + ((w.lse[side].data_ptr(),) if entry.endswith("_lse") else ()) + mid + tail

    def run():
        rc = fn(*args)
        if rc != 0:
            raise RuntimeError(f"{entry} of {lib.path}: error {rc}")

    return run


def pair(label, w, fa, fb, lse_pair, alternations, min_ms, what):
    for t in w.o + w.lse:
        t.fill_(float("nan"))
    fa()
    fb()
    torch.cuda.synchronize()
    same = bool(torch.equal(w.o[0], w.o[1]))
    wa, wb, calls = alternate(fa, fb, alternations, min_ms)
    ms_a, ms_b = sum(wa) / len(wa), sum(wb) / len(wb)
    spread_a = max(wa) - min(wa)
    diff = ms_b - ms_a
    every = all(b < a for a, b in zip(wa, wb))
    rec = {"pair": label, "a": what[0], "b": what[1], "workload": "tiny" if w.S < 10000 else "hunyuan_720p"}
    rec.update(w.cfg)
    rec.update({
        "alternations": alternations, "calls_per_window": calls,
        "a_ms": round(ms_a, 4), "b_ms": round(ms_b, 4), "a_spread_ms": round(spread_a, 4), "b_spread_ms": round(max(wb) - min(wb), 4),
        "a_windows": r4(wa), "b_windows": r4(wb),
        "b_over_a": round(ms_b / ms_a, 4), "diff_ms": round(diff, 4),
        "diff_over_a_spread": round(diff / spread_a, 2) if spread_a > 0 else None,
        "inside_a_spread": bool(abs(diff) <= spread_a), "b_faster_in_every_alternation": every,
        "same_bits": same, "shader_clock": "not recorded",
    })
    if lse_pair == "both":
        rec["lse_same_bits"] = bool(torch.equal(w.lse[0], w.lse[1]))
    if lse_pair:
        rec["lse_finite"] = bool(torch.isfinite(w.lse[1]).all())
    if label == "lse_vs_parent":
        rec["gain"] = bool(every and -diff >= 3 * spread_a)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libsvgattn.so built from the parent commit")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=1000.0)
    ap.add_argument("--out", default=None, help="default: profiles/band_lse_forms_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_band_lse_forms: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    new = Lib(nat, nat.lib_path(), ["svg_band_attention", "svg_band_attention_lse", "svg_band_attention_switch", "svg_band_attention_switch_lse"])
    old = Lib(nat, a.parent, ["svg_band_attention", "svg_band_attention_lse", "svg_band_attention_switch"])
    out = Path(a.out or ROOT / "profiles" / "band_lse_forms_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 5)
    min_ms = 20.0 if a.tiny else a.min_ms
    w = workload(nat, a.tiny)
    pairs = [
        ("lse_vs_parent", (old, "svg_band_attention_lse"), (new, "svg_band_attention_lse"), "both"),
        ("lse_vs_plain", (new, "svg_band_attention"), (new, "svg_band_attention_lse"), "b"),
        ("switch_lse_vs_plain", (new, "svg_band_attention_switch"), (new, "svg_band_attention_switch_lse"), "b"),
        ("plain_vs_parent", (old, "svg_band_attention"), (new, "svg_band_attention"), None),
        ("switch_vs_parent", (old, "svg_band_attention_switch"), (new, "svg_band_attention_switch"), None),
    ]
    with out.open("w") as f:
        for label, (la, ea), (lb, eb), lse_pair in pairs:
            what = [("parent: " if lib is old else "this build: ") + e for lib, e in ((la, ea), (lb, eb))]
            line = json.dumps(pair(label, w, call(la, ea, w, 0), call(lb, eb, w, 1), lse_pair, alternations, min_ms, what))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
