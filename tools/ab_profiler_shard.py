"""Same box, one process: what one rank of a FRAME-sharded online profiler computes (include/svg_attn_profile_shard.h) beside the full
svg_sample_mse call, at HunyuanVideo 720p.

    python tools/ab_profiler_shard.py [--parent <libsvgattn.so of the parent commit>] [--alternations 7] [--min-ms 500]
                                      [--out profiles/profiler_shard_ab.jsonl] [--tiny]

Workload: 24 heads, S = 33 x 3600 + 256 = 119 056, bf16, R = 64 rows drawn below 10 000 (the reference's sample_mse_max_row), the
profile masks of HunyuanVideo.  The 33 frames go to 8 ranks as 5, 4, 4, ... (svg.distributed.frame_range), the 256 text and padding rows
to the last rank.  A is always the full svg_sample_mse call (all kernels of it); B is
  * svg_sample_mse_shard_partial of one rank — the first (5 frames), a middle one (4) and the last (4 frames and the 256 tail rows) — on
    the rank's own k / v as a contiguous buffer of their own and q[:, rows] gathered beforehand (partial kernel + reduce kernel);
  * svg_sample_mse_from_parts over the 8 parts.
A warm-up of both, then `alternations` (at least 5) rounds of (A window, B window), a window being as many repetitions between two device
events as make at least `min-ms` of work.  One JSON line per case, APPENDED to the output: a_ms / b_ms (mean over the windows), the windows,
their spreads (max - min), for a partial the GB/s over the shard's K and V (B) and over all K and V (A), b_over_full_eighth = b_ms /
(a_ms / 8) and b_over_row_share = b_ms / (a_ms x rows of the shard / S).  No value is fixed for those ratios: a shard's launch has about 14
tiles per workgroup where the full call has about 88, so the per-workgroup prologue — row ranking, class-table fill, first DMA — weighs more;
the line says what was found.  The 8 parts merged are compared with the full call's mse (rtol of the tests, not bits: other tiles).
This is ONE GPU running one rank's launches: no exchange is timed and no multi-GPU run exists.  The shader clock is not recorded.
--parent: both libraries in this process, the parent's always A, on the same tensors.  The shard form first: each of the 8 ranks' parts and
the merged result of the two libraries compared bit for bit (parts_equal_all_ranks, same_bits, merged_equal), then parent against this build
for the three partial cases and for from_parts (pairs *_vs_parent).  Last, svg_sample_mse of this build against the parent's
(plain_vs_parent): its attention listings are unchanged.  Expected everywhere: the same bits, and the median over the alternations of
(B - A) inside A's own spread; anything else is a finding.
--tiny: small shapes, two alternations (a rehearsal of the script, not a measurement)."""
import argparse
import ctypes as C
import json
import math
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT):
    sys.path.insert(0, str(p))

from ab_band_window import checked, stats  # noqa: E402  (tools/ is sys.path[0] when this file is run as a script)
from ab_sparse_lse import alternate  # noqa: E402

WORLD = 8
NOTE = {"multi_gpu_timing": "none: one GPU runs one rank's launches, no exchange was timed", "shader_clock": "not recorded"}


def workload(nat, tiny):
    from svg.models.hyvideo.utils import profile_desc

    H, D, F_, P_, ctx, R, max_row = (3, 128, 9, 320, 64, 48, 700) if tiny else (24, 128, 33, 3600, 256, 64, 10000)
    S = F_ * P_ + ctx
    w = argparse.Namespace(H=H, S=S, D=D, F=F_, P=P_, R=R, geo=(S, 0, F_, P_))
    g = torch.Generator(device="cuda").manual_seed(0)
    w.q, w.k, w.v = (torch.randn(H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    w.rows_cpu = torch.randint(0, max_row, (R,), generator=torch.Generator().manual_seed(0))
    w.rows = w.rows_cpu.cuda()
    w.q_rows = w.q[:, w.rows].contiguous()
    w.prof = profile_desc(ctx, F_, P_)
    w.scale = 1.0 / math.sqrt(D)
    w.cfg = {"BH": H, "S": S, "D": D, "dtype": "bfloat16", "R": R, "world": WORLD, "frames": F_, "frame_size": P_,
             "workload": "tiny" if tiny else "hunyuan_720p"}
    return w


def typed(nat, path, names):
    lib = C.CDLL(str(Path(path).resolve()))
    sigs = {**nat.SIGNATURES, **getattr(nat, "PROFILE_SHARD_SIGNATURES", {})}
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sigs[name]
    return lib


def shard_of(x, s, w):
    """the rows of shard s of an [H, S, D] tensor, as a buffer of its own"""
    parts = [x[:, s.f0 * w.P:(s.f0 + s.n_frames) * w.P]]
    if s.n_tail:
        parts.append(x[:, s.tail_begin:s.tail_begin + s.n_tail])
    return torch.cat(parts, dim=1).contiguous()


def full_call(lib, w, out):
    ws = torch.empty(lib.svg_sample_mse_workspace_bytes(w.H, w.R, w.D, w.S), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    run = checked(lib.svg_sample_mse, (w.q.data_ptr(), w.k.data_ptr(), w.v.data_ptr(), w.rows.data_ptr(), w.R, w.H, w.S, w.D, 0, w.scale,
                                       C.byref(w.prof), out.data_ptr(), ws.data_ptr(), ws.numel(), st), "svg_sample_mse")
    return run, ws


def partial_call(nat, lib, w, shard):
    k, v = shard_of(w.k, shard, w), shard_of(w.v, shard, w)
    n = k.shape[1]
    part = torch.empty(3, w.H, w.R, w.D + 4, dtype=torch.float32, device="cuda")
    ws = torch.empty(lib.svg_sample_mse_shard_workspace_bytes(w.H, w.R, w.D, n), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    run = checked(lib.svg_sample_mse_shard_partial,
                  (w.q_rows.data_ptr(), k.data_ptr(), v.data_ptr(), w.rows.data_ptr(), w.R, w.H, w.S, w.D, 0, w.scale, C.byref(w.prof),
                   C.byref(shard), part.data_ptr(), ws.data_ptr(), ws.numel(), None, None, st), f"svg_sample_mse_shard_partial {shard.as_tuple()}")
    return run, part, (k, v, ws)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsvgattn.so built from the parent commit (adds the *_vs_parent lines)")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/profiler_shard_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_profiler_shard: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat
    from svg.distributed import frame_shard

    nat.load()
    new = typed(nat, nat.lib_path(), ["svg_sample_mse", "svg_sample_mse_workspace_bytes", "svg_sample_mse_shard_partial",
                                      "svg_sample_mse_shard_workspace_bytes", "svg_sample_mse_from_parts", "svg_sample_mse_from_parts_workspace_bytes"])
    out = Path(a.out or ROOT / "profiles" / "profiler_shard_ab.jsonl")
    out.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 5)
    min_ms = 20.0 if a.tiny else a.min_ms
    w = workload(nat, a.tiny)
    sh = [frame_shard(w.geo, r, WORLD) for r in range(WORLD)]
    rows = [nat.band_shard_rows(s, w.P) for s in sh]
    mse_full = torch.empty(2, w.H, dtype=torch.float32, device="cuda")
    fa, keep_a = full_call(new, w, mse_full)
    kv_bytes = lambda n: 2 * w.H * n * w.D * 2   # noqa: E731  (K and V, 16-bit)
    with out.open("a") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        parts = {}
        for r in range(WORLD):                  # every rank's part once: the list the combine merges
            run, parts[r], keep = partial_call(nat, new, w, sh[r])
            run()
            torch.cuda.synchronize()
            del keep
        for rank, label in ((0, "first_rank"), (WORLD // 2 - 1, "middle_rank"), (WORLD - 1, "last_rank")):
            fb, part, keep_b = partial_call(nat, new, w, sh[rank])
            wa, wb, calls = alternate(fa, fb, alternations, min_ms)
            rec = {"pair": label, "a": "svg_sample_mse over all S rows", "b": f"svg_sample_mse_shard_partial, the shard of rank {rank}",
                   "rank": rank, "frames_of_rank": [sh[rank].f0, sh[rank].f0 + sh[rank].n_frames], "tail_rows": sh[rank].n_tail,
                   "rows": rows[rank]}
            rec.update(w.cfg)
            rec.update({"alternations": alternations, "repetitions_per_window": calls})
            rec.update(stats(wa, wb))
            rec.update({"a_gb_per_s_over_k_v": round(kv_bytes(w.S) / rec["a_ms"] / 1e6, 1),
                        "b_gb_per_s_over_the_shards_k_v": round(kv_bytes(rows[rank]) / rec["b_ms"] / 1e6, 1),
                        "b_over_full_eighth": round(rec["b_ms"] / (rec["a_ms"] / WORLD), 4), "row_share": round(rows[rank] / w.S, 5),
                        "b_over_row_share": round(rec["b_ms"] / (rec["a_ms"] * rows[rank] / w.S), 4),
                        "same_bits_as_the_first_run": bool(torch.equal(part.view(torch.int32), parts[rank].view(torch.int32)))})
            rec.update(NOTE)
            emit(rec)
            del keep_b
        # the combine over the 8 parts
        mse = torch.empty(2, w.H, dtype=torch.float32, device="cuda")
        ws = torch.empty(new.svg_sample_mse_from_parts_workspace_bytes(w.H), dtype=torch.uint8, device="cuda")
        pp = (C.c_void_p * WORLD)(*[parts[r].data_ptr() for r in range(WORLD)])
        fc = checked(new.svg_sample_mse_from_parts, (C.cast(pp, C.c_void_p), WORLD, w.R, w.H, w.D, 0, 0, mse.data_ptr(), ws.data_ptr(), ws.numel(),
                                                     None, torch.cuda.current_stream().cuda_stream), "svg_sample_mse_from_parts")
        wa, wb, calls = alternate(fa, fc, alternations, min_ms)
        rec = {"pair": "from_parts", "a": "svg_sample_mse over all S rows", "b": f"svg_sample_mse_from_parts over {WORLD} parts",
               "part_bytes": parts[0].numel() * 4}
        rec.update(w.cfg)
        rec.update({"alternations": alternations, "repetitions_per_window": calls})
        rec.update(stats(wa, wb))
        torch.cuda.synchronize()
        rel = ((mse - mse_full).abs() / mse_full.abs().clamp(min=1e-20)).max().item()
        rec.update({"b_over_a": round(rec["b_ms"] / rec["a_ms"], 4), "merged_vs_full_call_max_rel": round(rel, 6),
                    "merged_within_rtol_3e-2": bool(torch.allclose(mse, mse_full, rtol=3e-2, atol=1e-6)),
                    "argmin_equal": bool(torch.equal(mse.argmin(0), mse_full.argmin(0)))})
        rec.update(NOTE)
        emit(rec)
        if a.parent:
            old = typed(nat, a.parent, ["svg_sample_mse", "svg_sample_mse_workspace_bytes", "svg_sample_mse_shard_partial",
                                        "svg_sample_mse_shard_workspace_bytes", "svg_sample_mse_from_parts",
                                        "svg_sample_mse_from_parts_workspace_bytes"])

            def parent_line(pair, what, fo, fn, extra):
                wa, wb, calls = alternate(fo, fn, alternations, min_ms)
                rec = {"pair": pair, "a": f"parent: {what}", "b": f"this build: {what}"}
                rec.update(w.cfg)
                rec.update({"alternations": alternations, "repetitions_per_window": calls})
                rec.update(stats(wa, wb))
                med = statistics.median(y - x for x, y in zip(wa, wb))
                rec.update({"b_over_a": round(rec["b_ms"] / rec["a_ms"], 4), "median_diff_ms": round(med, 6),
                            "a_spread_unrounded_ms": round(max(wa) - min(wa), 6),
                            "median_diff_inside_a_spread": bool(abs(med) <= max(wa) - min(wa))})
                rec.update(extra)
                rec["shader_clock"] = "not recorded"
                emit(rec)

            # the shard form: every rank's part and the merged result of the two libraries bit for bit, then parent against this build
            parts_old, equal = {}, []
            for r in range(WORLD):
                run, parts_old[r], keep = partial_call(nat, old, w, sh[r])
                run()
                torch.cuda.synchronize()
                equal.append(bool(torch.equal(parts_old[r].view(torch.int32), parts[r].view(torch.int32))))
                del keep
            for rank, label in ((0, "first_rank"), (WORLD // 2 - 1, "middle_rank"), (WORLD - 1, "last_rank")):
                fo, part_o, keep_o = partial_call(nat, old, w, sh[rank])
                fn, part_n, keep_n = partial_call(nat, new, w, sh[rank])
                fo()
                fn()
                torch.cuda.synchronize()
                parent_line(f"{label}_vs_parent", f"svg_sample_mse_shard_partial, the shard of rank {rank}", fo, fn,
                            {"rank": rank, "rows": rows[rank], "parts_equal_all_ranks": equal,
                             "same_bits": bool(torch.equal(part_o.view(torch.int32), part_n.view(torch.int32)))})
                del keep_o, keep_n
            mse_o = torch.empty(2, w.H, dtype=torch.float32, device="cuda")
            ws_o = torch.empty(old.svg_sample_mse_from_parts_workspace_bytes(w.H), dtype=torch.uint8, device="cuda")
            pp_o = (C.c_void_p * WORLD)(*[parts_old[r].data_ptr() for r in range(WORLD)])
            fco = checked(old.svg_sample_mse_from_parts, (C.cast(pp_o, C.c_void_p), WORLD, w.R, w.H, w.D, 0, 0, mse_o.data_ptr(), ws_o.data_ptr(),
                                                          ws_o.numel(), None, torch.cuda.current_stream().cuda_stream),
                          "parent svg_sample_mse_from_parts")
            fco()
            fc()
            torch.cuda.synchronize()
            parent_line("from_parts_vs_parent", f"svg_sample_mse_from_parts over {WORLD} parts", fco, fc,
                        {"parts_equal_all_ranks": equal, "merged_equal": bool(torch.equal(mse_o.view(torch.int32), mse.view(torch.int32)))})
            mse_old = torch.empty(2, w.H, dtype=torch.float32, device="cuda")
            fo, keep_o = full_call(old, w, mse_old)
            fo()
            fa()
            torch.cuda.synchronize()
            same = bool(torch.equal(mse_old.view(torch.int32), mse_full.view(torch.int32)))
            wa, wb, calls = alternate(fo, fa, alternations, min_ms)
            rec = {"pair": "plain_vs_parent", "a": "parent: svg_sample_mse", "b": "this build: svg_sample_mse"}
            rec.update(w.cfg)
            rec.update({"alternations": alternations, "repetitions_per_window": calls})
            rec.update(stats(wa, wb))
            diff = rec["b_ms"] - rec["a_ms"]
            med = statistics.median(y - x for x, y in zip(wa, wb))
            rec.update({"b_over_a": round(rec["b_ms"] / rec["a_ms"], 4), "diff_ms": round(diff, 4),
                        "inside_a_spread": bool(abs(diff) <= rec["a_spread_ms"]), "median_diff_ms": round(med, 6),
                        "a_spread_unrounded_ms": round(max(wa) - min(wa), 6),
                        "median_diff_inside_a_spread": bool(abs(med) <= max(wa) - min(wa)), "same_bits": same, "shader_clock": "not recorded"})
            emit(rec)


if __name__ == "__main__":
    main()
