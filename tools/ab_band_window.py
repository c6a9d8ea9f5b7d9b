"""Same box, one process: what one rank of a token-sharded band (SVG1) attention computes with the window form
(include/svg_attn_band_window.h) beside the full-sequence call, at HunyuanVideo 720p in LOGICAL order (no head permutation: the window
form has none).

    python tools/ab_band_window.py [--parent <libsvgattn.so of the parent commit>] [--alternations 7] [--min-ms 500]
                                   [--out profiles/band_window_ab.jsonl] [--tiny]

Workload: 24 heads, S = 33 x 3600 + 256 = 119 056, bf16, sparsity 0.25 -> band 15 616 (the production mask of bench.py).  The sequence is cut
into 8 row shards with svg.distributed.token_range(unit = 128).  For one rank — a middle one and the last one, which holds the text rows —
B is the sum of the window launches of that rank's rows over the key shards svg.distributed.band_exchange_plan keeps for it (each shard a
contiguous buffer of its own, as a received shard is), A the full-S svg_band_attention_lse call; a warm-up of both, then `alternations`
(at least 5) rounds of (A window, B window), a window being as many repetitions between two device events as make at least `min-ms` of
work.  One JSON line per rank: a_ms / b_ms (mean over the windows), the windows, their spreads (max - min), b_over_full_eighth = b_ms /
(a_ms / 8) — 1.0 would be a rank that costs exactly its share of the single-GPU call — parts_kept, the bytes of k and v the rank
receives from its peers with the plan and without it, the rows of its parts that see no key of their shard (lse = -inf, as it must be) and
the distance of the merged 16-bit parts from the rows of the full call (two roundings against one: the tests hold the bound, not this).
This is ONE GPU running one rank's launches: no exchange is timed and no multi-GPU timing exists.  The merge of the parts is not timed.
The shader clock is not recorded.
--parent: one more line, the plain svg_band_attention launch of this build (B) against the parent's (A) on the same tensors with the head
permutation of bench.py: bit-identical, and the difference inside A's own spread.
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

WORLD, UNIT = 8, 128


def workload(nat, tiny):
    from svg.models.hyvideo.utils import sparsity_to_width

    H, D, F_, P_, ctx, L, sparsity = (2, 128, 5, 640, 64, 40, 0.25) if tiny else (24, 128, 33, 3600, 256, 64, 0.25)
    V = F_ * P_
    S = V + ctx
    tf = math.floor(sparsity_to_width(sparsity, ctx, F_, P_) * P_ / 128) * 128
    w = argparse.Namespace(H=H, S=S, D=D, F=F_, P=P_)
    w.mask = nat.BandMask(real_len=V + L, band=tf, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    g = torch.Generator(device="cuda").manual_seed(0)
    w.q, w.k, w.v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    w.cfg = {"BH": H, "S": S, "D": D, "dtype": "bfloat16", "band": tf, "real_len": V + L, "world": WORLD, "unit": UNIT, "order": "logical"}
    return w


def typed(nat, path, names):
    lib = C.CDLL(str(Path(path).resolve()))
    sigs = {**nat.SIGNATURES, **nat.SPARSE_LSE_SIGNATURES, **nat.BAND_WINDOW_SIGNATURES}
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sigs[name]
    return lib


def checked(fn, args, what):
    def run():
        rc = fn(*args)
        if rc != 0:
            raise RuntimeError(f"{what}: error {rc}")

    return run


def stats(wa, wb):
    ms_a, ms_b = sum(wa) / len(wa), sum(wb) / len(wb)
    return {"a_ms": round(ms_a, 4), "b_ms": round(ms_b, 4), "a_spread_ms": round(max(wa) - min(wa), 4), "b_spread_ms": round(max(wb) - min(wb), 4),
            "a_windows": r4(wa), "b_windows": r4(wb)}


def rank_line(nat, lib, w, rank, label, alternations, min_ms):
    from svg.distributed import band_exchange_plan, token_range

    st = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / math.sqrt(w.D)
    tr = [token_range(w.S, r, WORLD, UNIT) for r in range(WORLD)]
    plan = band_exchange_plan(w.mask, w.S, WORLD, UNIT)
    a, b = tr[rank]
    kept = [s for s in range(WORLD) if plan[rank][s]]
    o_full, lse_full = torch.empty_like(w.q), torch.empty(1, w.H, w.S, dtype=torch.float32, device="cuda")
    fa = checked(lib.svg_band_attention_lse, (w.q.data_ptr(), w.k.data_ptr(), w.v.data_ptr(), o_full.data_ptr(), lse_full.data_ptr(), w.H, w.S,
                                              w.D, 0, scale, C.byref(w.mask), None, None, st), "svg_band_attention_lse")
    q_r = w.q[:, :, a:b].contiguous()
    shards = {s: (w.k[:, :, tr[s][0]:tr[s][1]].contiguous(), w.v[:, :, tr[s][0]:tr[s][1]].contiguous()) for s in kept}
    outs = {s: (torch.empty_like(q_r), torch.empty(1, w.H, b - a, dtype=torch.float32, device="cuda")) for s in kept}
    launches = [checked(lib.svg_band_window_attention_lse,
                        (q_r.data_ptr(), shards[s][0].data_ptr(), shards[s][1].data_ptr(), outs[s][0].data_ptr(), outs[s][1].data_ptr(), w.H, w.S,
                         a, b - a, tr[s][0], tr[s][1] - tr[s][0], w.D, 0, scale, C.byref(w.mask), None, st), f"window rank {rank} shard {s}")
                for s in kept]

    def fb():
        for run in launches:
            run()

    fa()
    fb()
    torch.cuda.synchronize()
    # what the parts are worth: merged, they are the rank's rows of the full call to rounding (the project's merged bound is the tests')
    merged = nat.merge_attention_states([outs[s][0] for s in kept], [outs[s][1] for s in kept])
    ref = o_full[:, :, a:b].float()
    merged_rel_l2 = ((merged.float() - ref).norm() / ref.norm()).item()
    wa, wb, calls = alternate(fa, fb, alternations, min_ms)
    rec = {"pair": label, "a": "svg_band_attention_lse over all S rows", "b": f"svg_band_window_attention_lse, rows of rank {rank} over the kept shards",
           "workload": "tiny" if w.S < 10000 else "hunyuan_720p", "rank": rank, "rows": [a, b], "parts_kept": len(kept), "kept_shards": kept}
    rec.update(w.cfg)
    rec.update({"alternations": alternations, "repetitions_per_window": calls})
    rec.update(stats(wa, wb))
    ms_a, ms_b = rec["a_ms"], rec["b_ms"]
    per_tok = 2 * w.H * w.D * 2      # k and v of one token, all heads, 16-bit
    rec.update({
        "b_over_a": round(ms_b / ms_a, 4), "b_over_full_eighth": round(ms_b / (ms_a / WORLD), 4),
        "bytes_received_with_plan": sum((tr[s][1] - tr[s][0]) * per_tok for s in kept if s != rank),
        "bytes_received_without_plan": sum((tr[s][1] - tr[s][0]) * per_tok for s in range(WORLD) if s != rank),
        "merged_vs_full_call_rel_l2": round(merged_rel_l2, 6), "lse_free_of_nan": not any(bool(torch.isnan(outs[s][1]).any()) for s in kept),
        "part_rows_without_keys": sum(int(torch.isinf(outs[s][1]).sum()) for s in kept),
        "multi_gpu_timing": "none: one GPU runs one rank's launches", "shader_clock": "not recorded",
    })
    return rec


def parent_line(nat, new, old, w, alternations, min_ms):
    st = torch.cuda.current_stream().cuda_stream
    best = (torch.arange(w.H, device="cuda") % 2).view(1, w.H).to(torch.int64).contiguous()
    perm = nat.PermDesc(best.data_ptr(), 0, w.F, w.P)
    o = [torch.full_like(w.q, float("nan")) for _ in range(2)]
    runs = [checked(lib.svg_band_attention, (w.q.data_ptr(), w.k.data_ptr(), w.v.data_ptr(), o[i].data_ptr(), w.H, w.S, w.D, 0,
                                             1.0 / math.sqrt(w.D), C.byref(w.mask), C.byref(perm), 0, st), "svg_band_attention")
            for i, lib in enumerate((old, new))]
    runs[0]()
    runs[1]()
    torch.cuda.synchronize()
    same = bool(torch.equal(o[0], o[1]))
    wa, wb, calls = alternate(runs[0], runs[1], alternations, min_ms)
    rec = {"pair": "plain_vs_parent", "a": "parent: svg_band_attention", "b": "this build: svg_band_attention",
           "workload": "tiny" if w.S < 10000 else "hunyuan_720p", "token_major_heads": int(best.sum())}
    rec.update(w.cfg)
    rec["order"] = "every second head token-major (bench.py)"
    rec.update({"alternations": alternations, "repetitions_per_window": calls})
    rec.update(stats(wa, wb))
    diff = rec["b_ms"] - rec["a_ms"]
    rec.update({"b_over_a": round(rec["b_ms"] / rec["a_ms"], 4), "diff_ms": round(diff, 4), "inside_a_spread": bool(abs(diff) <= rec["a_spread_ms"]),
                "same_bits": same, "shader_clock": "not recorded"})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsvgattn.so built from the parent commit (adds the plain_vs_parent line)")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/band_window_ab.jsonl")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_band_window: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    new = typed(nat, nat.lib_path(), ["svg_band_attention", "svg_band_attention_lse", "svg_band_window_attention_lse"])
    out = Path(a.out or ROOT / "profiles" / "band_window_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 5)
    min_ms = 20.0 if a.tiny else a.min_ms
    w = workload(nat, a.tiny)
    with out.open("w") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        emit(rank_line(nat, new, w, WORLD // 2 - 1, "middle_rank", alternations, min_ms))
        emit(rank_line(nat, new, w, WORLD - 1, "last_rank", alternations, min_ms))
        if a.parent:
            emit(parent_line(nat, new, typed(nat, a.parent, ["svg_band_attention"]), w, alternations, min_ms))


if __name__ == "__main__":
    main()
