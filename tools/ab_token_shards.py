"""A/B on one box, one process: the layout work of one rank of a token-sharded layer-call (svg.distributed.run_token_sharded) — svg_copy_boxes
against the torch statement of the same boxes.  NO exchange runs and none is timed: no multi-GPU node exists for this project.

    python tools/ab_token_shards.py [--alternations 7] [--min-ms 500] [--out profiles/token_shards_ab.jsonl] [--tiny]

Workloads: HunyuanVideo 720p (24 heads, S = 33 x 3600 + 256 = 119 056, head_dim 128, bf16) and Wan 720p (40 heads, S = 75 600), both over 8
ranks with unit = 128, cfg = 1; the first, a middle and the last rank.  Per rank the four layouts of _native.py's builders:
  inbound_pack     v as the head view of a fused [1, S_r, 3 H D] projection -> the send buffer (q and k are contiguous: not packed at cfg 1)
  inbound_unpack   the receive buffers of q, k, v -> three [1, H_l, S, D] tensors (one launch of three tensors and 8 boxes)
  outbound_pack    o [1, H_l, S, D] stored HEAD-major -> the send buffer: the fall-back of a core without token_major_out; with token-major
                   storage, which every core of svg/models/_core.py writes, this step does not exist at cfg 1
  outbound_unpack  the receive buffer -> the storage [1, S_r, H, D]
A = _native.copy_boxes_torch (one strided copy_ per tensor and box), B = _native.copy_box_jobs (svg_copy_boxes).  A warm-up of both, then
`alternations` (at least 5) rounds of (A window, B window); a window is as many repetitions between two device events as make at least
`min-ms` of work.  One JSON line per (workload, rank, layout): a_ms / b_ms means over the windows, the windows, their spreads (max - min),
GB/s over the bytes read plus written, launches per layer-call of either side, same_bits, and
  won = every alternation is won by B AND a_ms - b_ms > 3 x A's spread
— no ratio is fixed in advance; a case that is not won is written down as such, and _native.COPY_BOX_LAYOUTS lists the layouts that go
through the kernel.  (The shader clock is not recorded.)
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT, ROOT / "tools"):
    sys.path.insert(0, str(p))

from ab_sparse_lse import alternate, r4  # noqa: E402

WORKLOADS = {"hunyuan_720p": dict(H=24, S=33 * 3600 + 256, D=128), "wan_720p": dict(H=40, S=21 * 3600, D=128)}
TINY = {"tiny": dict(H=10, S=5 * 300 + 40, D=64)}
WORLD, UNIT, CFG = 8, 128, 1


def jobs_of(nat, sd, w, rank, layout, dev):
    """[(src, dst, boxes)] of one layout on one rank; random sources, destinations of their own"""
    H, S, D = w["H"], w["S"], w["D"]
    counts = sd.head_counts(H, WORLD)
    ranges = [sd.token_range(S, r, WORLD, UNIT) for r in range(WORLD)]
    Hl, n = counts[rank], ranges[rank][1] - ranges[rank][0]
    mk = lambda *shape: torch.randn(*shape, device=dev, dtype=torch.float32).to(torch.bfloat16)   # noqa: E731
    out = lambda numel: torch.empty(numel, device=dev, dtype=torch.bfloat16)                      # noqa: E731
    if layout == "inbound_pack":
        v = mk(CFG, n, 3 * H * D)[:, :, 2 * H * D:].unflatten(2, (H, D)).transpose(1, 2)
        return [(v, out(CFG * H * n * D), nat.inbound_pack_boxes(CFG, counts, n, D, v.stride()[:3]))]
    if layout == "inbound_unpack":
        boxes = nat.inbound_unpack_boxes(CFG, Hl, ranges, D)
        return [(mk(CFG * Hl * S * D), out(CFG * Hl * S * D), boxes) for _ in range(3)]
    if layout == "outbound_pack":
        o = mk(CFG, Hl, S, D)
        return [(o, out(CFG * Hl * S * D), nat.outbound_pack_boxes(CFG, Hl, ranges, D, o.stride()[:3]))]
    return [(mk(CFG * n * H * D), out(CFG * n * H * D), nat.outbound_unpack_boxes(CFG, counts, n, D))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/token_shards_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    from svg import _native as nat
    from svg import distributed as sd

    nat.load()
    dev = torch.device("cuda", 0)
    out_path = Path(a.out or ROOT / "profiles" / "token_shards_ab.jsonl")
    out_path.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 5)
    min_ms = 5.0 if a.tiny else a.min_ms
    with open(out_path, "a") as f:
        for name, w in (TINY if a.tiny else WORKLOADS).items():
            for rank in (0, WORLD // 2, WORLD - 1):
                for layout in ("inbound_pack", "inbound_unpack", "outbound_pack", "outbound_unpack"):
                    jobs = jobs_of(nat, sd, w, rank, layout, dev)
                    twins = [(s, torch.empty_like(d), b) for s, d, b in jobs]

                    def fa():
                        for s, d, b in twins:
                            nat.copy_boxes_torch([(s, d)], b, w["D"])

                    launches = [0]

                    def fb():
                        launches[0] = nat.copy_box_jobs(jobs, w["D"], layout)

                    fa()
                    fb()
                    torch.cuda.synchronize()
                    same = all(torch.equal(x[1].view(torch.int16), y[1].view(torch.int16)) for x, y in zip(jobs, twins))
                    wa, wb, calls = alternate(fa, fb, alternations, min_ms)
                    a_ms, b_ms = sum(wa) / len(wa), sum(wb) / len(wb)
                    a_spread = max(wa) - min(wa)
                    nbytes = 2 * sum(d.numel() * d.element_size() for _, d, _ in jobs)   # read plus written
                    rec = {"kind": "token_shards_layout", "workload": name, "heads": w["H"], "S": w["S"], "head_dim": w["D"], "dtype": "bf16",
                           "world": WORLD, "unit": UNIT, "cfg": CFG, "rank": rank, "layout": layout, "tensors": len(jobs),
                           "boxes": len(jobs[0][2]), "bytes_read_plus_written": nbytes,
                           "alternations": alternations, "repetitions_per_window": calls,
                           "a": "copy_boxes_torch", "b": "svg_copy_boxes",
                           "a_ms": round(a_ms, 4), "b_ms": round(b_ms, 4), "a_windows": r4(wa), "b_windows": r4(wb),
                           "a_spread_ms": round(a_spread, 4), "b_spread_ms": round(max(wb) - min(wb), 4),
                           "a_gb_s": round(nbytes / a_ms / 1e6, 1), "b_gb_s": round(nbytes / b_ms / 1e6, 1),
                           "a_launches": sum(len(b) for _, _, b in jobs), "b_launches": launches[0],
                           "every_alternation_won": bool(all(y < x for x, y in zip(wa, wb))),
                           "gain_ms": round(a_ms - b_ms, 4), "gain_over_a_spread": round((a_ms - b_ms) / a_spread, 2) if a_spread > 0 else None,
                           "same_bits": bool(same), "exchange_timed": False, "shader_clock": "not recorded",
                           "when": time.strftime("%Y-%m-%d %H:%M:%S")}
                    rec["won"] = bool(rec["every_alternation_won"] and (a_ms - b_ms) > 3 * a_spread)
                    f.write(json.dumps(rec) + "\n")
                    f.flush()
                    print(json.dumps(rec), flush=True)
                    del jobs, twins
                    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
