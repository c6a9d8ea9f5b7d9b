#!/usr/bin/env python3
"""A/B on one box, one process: what SVG1's per-head band costs and that time follows the bands.

    python tools/ab_adaptive_band.py [--alternations 7] [--min-ms 300] [--out profiles/adaptive_band_ab.jsonl] [--tiny] [--queue]

The HunyuanVideo 720p layer-call of bench.py (24 heads, S = 119 056, F = 33, P = 3600, ctx = 256, prompt 64, sparsity 0.25, bf16, every second
head token-major), all sides from the same library.
  (a) launch form  svg_band_attention_switch_per_head_lse with every band equal to the mask's — flag 0 — against the parent's
                   svg_band_attention_switch_lse (the same static mapping idea, the same body) and against svg_band_attention_lse (the work
                   queue).  The criterion of the change: per_head - switch inside 3 x the spread (max - min) of the switch form's windows.
                   same_bits: o and lse of the three.
  (b) overhead     svg1_attention_device_switch, plain, against the call with AdaptiveBand(gain_up = gain_down = 0): the bands never move, so
                   the difference is the always-on cost — the LSE form, the K-only probe (64 rows per head) and the controller launch.
  (c) bands        the launch of (a) with every second head at half the band: time follows the bands.
A warm-up of both sides, then `alternations` (at least 5) rounds of (A window, B window); a window is as many calls between two device
events as make at least `min-ms` of work.  One JSON line per part, appended to --out.  Synthetic data; no claim about what per-head bands are
worth on a real model.  --tiny: small shapes, two alternations (a rehearsal of the script, not a measurement).

--queue: instead of (a) - (c), the per-head launches on the work queue (include/svg_attn_band_per_head_queue.h, work_queue=True) against the
statically mapped per-head entries of the same library — the parent's code, untouched (profiles/adaptive_band_queue_asm_diff.txt) —, appended
to profiles/adaptive_band_queue_ab.jsonl unless --out says otherwise:
  (q1) svg_band_attention_per_head_queue_lse against svg_band_attention_per_head_lse at (i) uniform bands, (ii) every second head at half
       the band, (iii) bands spread linearly from a quarter of the mask's band to the mask's band over the heads;
  (q2) svg_band_attention_switch_per_head_queue_lse against svg_band_attention_switch_per_head_lse at flag 0 and at flag 1, and at flag 1
       also against svg_band_attention_switch_lse.
Per row: ms, spread, ratio, same_bits, and the shader clock granted to each side's windows (nat.ClockProbe) where it can be read.  No
threshold: the rows are figures to set beside 32.391 ms (static per-head, uniform) and 31.147 ms (plain queue, uniform) of DESIGN §3.1.3."""
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


def alternate(fns, alternations, min_ms):
    for fn in list(fns) * 2:
        fn()
    torch.cuda.synchronize()
    calls = [max(1, math.ceil(min_ms / max(window(fn, 1), 1e-3))) for fn in fns]
    ws = [[] for _ in fns]
    for _ in range(alternations):
        for w, fn, c in zip(ws, fns, calls):
            w.append(window(fn, c))
    return ws, calls


def stats(w):
    return {"ms": round(sum(w) / len(w), 4), "windows": [round(x, 4) for x in w], "spread_ms": round(max(w) - min(w), 4)}


def alternate_clocked(fns, alternations, min_ms, probe):
    """alternate() with the granted shader clock of every window beside its ms (None where the probe's counters did not move)"""
    for fn in list(fns) * 2:
        fn()
    torch.cuda.synchronize()
    calls = [max(1, math.ceil(min_ms / max(window(fn, 1), 1e-3))) for fn in fns]
    ws, mhz = [[] for _ in fns], [[] for _ in fns]
    for _ in range(alternations):
        for w, m, fn, c in zip(ws, mhz, fns, calls):
            probe.start(max_ms=20000)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(c):
                fn()
            e1.record()
            probe.arm_stop()
            e1.synchronize()
            m.append(probe.result())
            w.append(e0.elapsed_time(e1) / c)
    return ws, mhz, calls


def queue_rows(a, nat, ab, q, k, v, mask, dense, pk, H, workload, alternations):
    """the --queue rows: every pair is (static entry, queue entry) on the same inputs"""
    dev = q.device
    probe = nat.ClockProbe(dev)   # (one probe for the whole run: tools/ab_band_queue.py)
    hint = mask.band
    uniform = torch.full((H,), hint, dtype=torch.int32, device=dev)
    halved = uniform.clone()
    halved[1::2] = hint // 2
    spread = torch.linspace(hint / 4, hint, H).round().to(torch.int32).to(dev)
    flags = {f: torch.full((1,), f, dtype=torch.int32, device=dev) for f in (0, 1)}
    recs = []

    def row(metric, sides, extra):
        out = {}
        fns = [lambda n=n, f=f: out.__setitem__(n, f()) for n, f in sides]
        ws, mhz, calls = alternate_clocked(fns, alternations, a.min_ms, probe)
        st = {n: dict(stats(w), sclk_mhz=m) for (n, _), w, m in zip(sides, ws, mhz)}
        base, new = sides[0][0], sides[-1][0]
        rec = {"metric": metric, "workload": workload, "alternations": alternations, "calls_per_window": calls, **extra, **st,
               f"{new}_minus_{base}_ms": round(st[new]["ms"] - st[base]["ms"], 4), f"{new}_over_{base}": round(st[new]["ms"] / st[base]["ms"], 4),
               "queue_faster_in_every_alternation": bool(all(y < x for x, y in zip(ws[0], ws[-1]))),
               "same_bits": bool(all(torch.equal(out[new][i], out[n][i]) for n, _ in sides[:-1] for i in (0, 1)))}
        if len(sides) == 3:
            mid = sides[1][0]
            rec[f"{new}_over_{mid}"] = round(st[new]["ms"] / st[mid]["ms"], 4)
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    for name, band in (("uniform", uniform), ("every_second_head_half_band", halved), ("linear_quarter_to_full", spread)):
        row("per_head_queue_vs_static", [("static", lambda b=band: ab.band_attention_per_head(q, k, v, mask, b, **pk)),
                                         ("queue", lambda b=band: ab.band_attention_per_head(q, k, v, mask, b, work_queue=True, **pk))],
            {"bands": name, "band_min_max": [int(band.min()), int(band.max())]})
    for f in (0, 1):
        sides = [("static", lambda f=f: ab.band_attention_switch_per_head(q, k, v, mask, dense, flags[f], uniform, **pk))]
        if f:
            sides.append(("switch_lse", lambda f=f: nat.band_attention_switch(q, k, v, mask, dense, flags[f], return_lse=True, **pk)))
        sides.append(("queue", lambda f=f: ab.band_attention_switch_per_head(q, k, v, mask, dense, flags[f], uniform, work_queue=True, **pk)))
        row("switch_per_head_queue_vs_static", sides, {"flag": f, "bands": "uniform"})
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--out", default="")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--queue", action="store_true", help="the rows of the per-head work-queue entries instead of (a) - (c)")
    a = ap.parse_args()
    a.out = a.out or str(ROOT / "profiles" / ("adaptive_band_queue_ab.jsonl" if a.queue else "adaptive_band_ab.jsonl"))
    from svg import _adaptive_band as ab
    from svg import _native as nat
    from svg.models import _core
    from svg.models.hyvideo.utils import dense_mask, generate_temporal_head_mask_mod, profile_desc, sparsity_to_width

    nat.load()
    alternations = 2 if a.tiny else max(5, a.alternations)
    H, D, F_, P_, ctx, L, sparsity = (4, 128, 5, 200, 64, 21, 0.25) if a.tiny else (24, 128, 33, 3600, 256, 64, 0.25)
    S = F_ * P_ + ctx
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    q, k, v = (torch.randn(1, H, S, D, device=dev, dtype=torch.bfloat16, generator=gen) for _ in range(3))
    # (tiny: the width of the test suites — at this size the sparsity's own width rounds to a band of no rows)
    mask = generate_temporal_head_mask_mod(ctx, L, F_, P_, mul=1.2 if a.tiny else sparsity_to_width(sparsity, ctx, F_, P_))
    dense = dense_mask(S, F_ * P_ + L)
    geo = _core.Geometry(ctx, F_, P_, text_first=False)
    best = (torch.arange(H, device=dev) % 2).view(1, H)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    pk = dict(head_perm_flag=best, vid0=0, num_frame=F_, frame_size=P_)
    workload = f"{'tiny' if a.tiny else 'hy720p'} cfg=1 H={H} D={D} S={S} band={mask.band} bf16, every second head token-major"
    if a.queue:
        recs = queue_rows(a, nat, ab, q, k, v, mask, dense, pk, H, workload, alternations)
        with open(a.out, "a") as f:
            f.write("".join(json.dumps(r) + "\n" for r in recs))
        return
    recs = []

    # ---- (a) the launch forms, every band the mask's ----
    uniform = torch.full((H,), mask.band, dtype=torch.int32, device=dev)
    out = {}
    f_sw = lambda: out.__setitem__("switch", nat.band_attention_switch(q, k, v, mask, dense, flag, return_lse=True, **pk))      # noqa: E731
    f_ph = lambda: out.__setitem__("per_head", ab.band_attention_switch_per_head(q, k, v, mask, dense, flag, uniform, **pk))   # noqa: E731
    f_qu = lambda: out.__setitem__("queue", nat.band_attention(q, k, v, mask, return_lse=True, **pk))                         # noqa: E731
    (w_sw, w_ph, w_qu), calls = alternate((f_sw, f_ph, f_qu), alternations, a.min_ms)
    s_sw, s_ph, s_qu = stats(w_sw), stats(w_ph), stats(w_qu)
    diff = s_ph["ms"] - s_sw["ms"]
    recs.append({"metric": "adaptive_band_launch_form", "workload": workload, "alternations": alternations, "calls_per_window": calls,
                 "switch_lse": s_sw, "switch_per_head_lse_uniform": s_ph, "band_attention_lse_queue": s_qu,
                 "per_head_minus_switch_ms": round(diff, 4), "per_head_over_switch": round(s_ph["ms"] / s_sw["ms"], 4),
                 "per_head_over_queue": round(s_ph["ms"] / s_qu["ms"], 4), "switch_spread_ms": s_sw["spread_ms"],
                 "inside_3x_spread": bool(diff <= 3 * s_sw["spread_ms"]),
                 "same_bits": bool(all(torch.equal(out["per_head"][i], out[o][i]) for o in ("switch", "queue") for i in (0, 1)))})
    print(json.dumps(recs[-1]), flush=True)

    # ---- (c) every second head at half the band ----
    halved = uniform.clone()
    halved[1::2] = mask.band // 2
    f_hv = lambda: ab.band_attention_switch_per_head(q, k, v, mask, dense, flag, halved, **pk)    # noqa: E731
    (w_un, w_hv), calls = alternate((f_ph, f_hv), alternations, a.min_ms)
    s_un, s_hv = stats(w_un), stats(w_hv)
    recs.append({"metric": "adaptive_band_time_follows_bands", "workload": workload, "alternations": alternations, "calls_per_window": calls,
                 "uniform": s_un, "every_second_head_half_band": s_hv, "halved_over_uniform": round(s_hv["ms"] / s_un["ms"], 4)})
    print(json.dumps(recs[-1]), flush=True)

    # ---- (b) the layer-call with zero gains against the plain call ----
    prof = profile_desc(ctx, F_, P_)
    store = _core.BandStore()
    zero = _core.AdaptiveBand(0.9, gain_up=0.0, gain_down=0.0)
    last = {}

    def call(name, **kw):
        _core.reseed_switch_generator(0)      # (the same profiler rows on both sides)
        last[name] = _core.svg1_attention_device_switch(q, k, v, geo, mask, dense, prof, 32, min(10000, S), flag, **kw)[0]

    fa = lambda: call("plain")                                                        # noqa: E731
    fb = lambda: call("adaptive", adaptive=zero, band_store=store, layer_idx=0)       # noqa: E731
    (wa, wb), calls = alternate((fa, fb), alternations, a.min_ms)
    sa, sb = stats(wa), stats(wb)
    recs.append({"metric": "adaptive_band_overhead", "workload": workload, "alternations": alternations, "calls_per_window": calls,
                 "plain": sa, "adaptive_zero_gains": sb, "overhead_ms": round(sb["ms"] - sa["ms"], 4),
                 "overhead_over_plain_spread": round((sb["ms"] - sa["ms"]) / max(sa["spread_ms"], 1e-6), 2),
                 "adaptive_over_plain": round(sb["ms"] / sa["ms"], 4), "same_bits": bool(torch.equal(last["plain"], last["adaptive"])),
                 "kept_mass_min_max": [round(float(store.kept[0].min()), 4), round(float(store.kept[0].max()), 4)]})
    print(json.dumps(recs[-1]), flush=True)
    with open(a.out, "a") as f:
        f.write("".join(json.dumps(r) + "\n" for r in recs))


if __name__ == "__main__":
    main()
