"""Same box, one process: what one rank of a FRAME-sharded SVG1 layer-call computes with the shard form (include/svg_attn_band_shard.h)
beside the full-sequence call, at HunyuanVideo 720p in the model's own row order, half the heads token-major.

    python tools/ab_band_shard.py [--parent <libsvgattn.so of the parent commit>] [--alternations 7] [--min-ms 500]
                                  [--out profiles/band_shard_ab.jsonl] [--tiny]

Workload: 24 heads, S = 33 x 3600 + 256 = 119 056, bf16, sparsity 0.25 -> band 15 616 (the production mask of bench.py), every second head
token-major (flags on the device).  The 33 frames go to 8 ranks as 5, 4, 4, ... (svg.distributed.frame_range), the 256 text and padding rows
to the last rank.  For one rank — the first, a middle one and the last — B is the sum of the shard launches of that rank's rows over the
key shards svg.distributed.band_shard_exchange_plan keeps for it (each shard a contiguous buffer of its own, as a received shard is; both
kinds of head in each launch), A the full-S svg_band_attention_switch_lse call with the same flags (switch flag 0: the sparse mask); a
warm-up of both, then `alternations` (at least 5) rounds of (A window, B window), a window being as many repetitions between two device
events as make at least `min-ms` of work.  One JSON line per rank, APPENDED to the output: a_ms / b_ms (mean over the windows), the
windows, their spreads (max - min), b_over_full_eighth = b_ms / (a_ms / 8), b_over_row_share = b_ms / (a_ms * rows of the rank / S) — whole
frames give the first rank 5 / 33 of the video, not 1 / 8: largest shard over mean 1.21, the known cost of this form —, parts_kept and the
bytes of k and v the rank receives with the plan and without it (for mixed head kinds and for heads in logical order alone: a token-major
head's rows touch every frame, so with both kinds nothing is skipped), the rows of its parts that see no key of their shard, and the
distance of the merged 16-bit parts from the rank's rows of the full call (two roundings against one: the tests hold the bound, not this).
This is ONE GPU running one rank's launches: no exchange is timed and no multi-GPU run exists.  The merge of the parts is not timed.
The shader clock is not recorded.
--parent: one more line, the plain svg_band_attention launch of this build (B) against the parent's (A) on the same tensors with the head
permutation of bench.py: bit-identical, and the difference inside A's own spread.
--switch: the device switch of the shard form (include/svg_attn_band_shard_switch.h) instead, for the same three ranks, appended to
profiles/band_shard_switch_ab.jsonl; alt_mask is the processors' dense warm-up mask (real_len of the sparse mask, two segments), the
launches of a rank run over the shards the OR-ed plan keeps (band_shard_exchange_plan(..., dense_mask=)).  Two lines per rank:
  flag 0  A = the plain svg_band_shard_attention_lse launches of the rank, B = svg_band_shard_attention_switch_lse with a flag of 0 on the
          same tensors: the same body, so the same bits are checked and b_over_a is reported with inside_a_spread — a difference outside
          A's own spread is a finding to report, not a failure;
  flag 1  A = the full-S svg_band_attention_switch_lse call with a flag of 1 (the dense mask, no head placement), B = the rank's switch
          launches with a flag of 1: b_over_full_eighth and b_over_row_share as above.  No threshold is set: nobody has measured it.
With --parent two more lines: the plain svg_band_attention launch and the plain shard launches of the first rank, this build (B) against
the parent's library (A) in the same process: bit-identical, the difference inside A's spread.
Again ONE GPU running one rank's launches: no exchange is timed and no multi-GPU run exists.
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

from ab_band_window import checked, parent_line, stats  # noqa: E402  (tools/ is sys.path[0] when this file is run as a script)
from ab_sparse_lse import alternate  # noqa: E402

WORLD = 8


def workload(nat, tiny):
    from svg.models.hyvideo.utils import sparsity_to_width

    H, D, F_, P_, ctx, L, sparsity = (2, 128, 9, 320, 64, 40, 0.25) if tiny else (24, 128, 33, 3600, 256, 64, 0.25)
    V = F_ * P_
    S = V + ctx
    tf = math.floor(sparsity_to_width(sparsity, ctx, F_, P_) * P_ / 128) * 128
    w = argparse.Namespace(H=H, S=S, D=D, F=F_, P=P_, geo=(S, 0, F_, P_))
    w.mask = nat.BandMask(real_len=V + L, band=tf, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)
    g = torch.Generator(device="cuda").manual_seed(0)
    w.q, w.k, w.v = (torch.randn(1, H, S, D, device="cuda", dtype=torch.bfloat16, generator=g) for _ in range(3))
    w.flags = (torch.arange(H, device="cuda") % 2).to(torch.int64).contiguous()
    w.cfg = {"BH": H, "S": S, "D": D, "dtype": "bfloat16", "band": tf, "real_len": V + L, "world": WORLD, "frames": F_, "frame_size": P_,
             "order": "the model's (frame-major), every second head token-major"}
    return w


def typed(nat, path, names):
    lib = C.CDLL(str(Path(path).resolve()))
    sigs = {**nat.SIGNATURES, **nat.BAND_LSE_FORM_SIGNATURES, **nat.BAND_SHARD_SIGNATURES, **nat.BAND_SHARD_SWITCH_SIGNATURES}
    for name in names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sigs[name]
    return lib


def shard_of(x, s, w):
    """the rows of shard s of a [1, H, S, D] tensor in the model's order, as a buffer of its own"""
    V = w.F * w.P
    parts = [x[:, :, s.f0 * w.P:(s.f0 + s.n_frames) * w.P]]
    if s.n_tail:
        parts.append(x[:, :, s.tail_begin:s.tail_begin + s.n_tail])
    assert s.n_tail == 0 or s.tail_begin == V
    return torch.cat(parts, dim=2).contiguous()


def rank_line(nat, lib, w, rank, label, alternations, min_ms):
    from svg.distributed import band_shard_exchange_plan, frame_shard

    st = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / math.sqrt(w.D)
    sh = [frame_shard(w.geo, r, WORLD) for r in range(WORLD)]
    rows = [nat.band_shard_rows(s, w.P) for s in sh]
    plan = band_shard_exchange_plan(w.mask, w.geo, WORLD, "both")
    plan_logical = band_shard_exchange_plan(w.mask, w.geo, WORLD, "logical")
    kept = [s for s in range(WORLD) if plan[rank][s]]
    kept_logical = [s for s in range(WORLD) if plan_logical[rank][s]]
    perm = nat.PermDesc(w.flags.data_ptr(), 0, w.F, w.P)
    dense = nat.BandMask(w.S, w.S + 1, 0, 0, 0, 0)
    use_alt = torch.zeros(1, dtype=torch.int32, device="cuda")
    o_full, lse_full = torch.empty_like(w.q), torch.empty(1, w.H, w.S, dtype=torch.float32, device="cuda")
    fa = checked(lib.svg_band_attention_switch_lse,
                 (w.q.data_ptr(), w.k.data_ptr(), w.v.data_ptr(), o_full.data_ptr(), lse_full.data_ptr(), w.H, w.S, w.D, 0, scale,
                  C.byref(w.mask), C.byref(perm), C.byref(dense), use_alt.data_ptr(), None, st), "svg_band_attention_switch_lse")
    q_r = shard_of(w.q, sh[rank], w)
    n = rows[rank]
    shards = {s: (shard_of(w.k, sh[s], w), shard_of(w.v, sh[s], w)) for s in kept}
    outs = {s: (torch.empty_like(q_r), torch.empty(1, w.H, n, dtype=torch.float32, device="cuda")) for s in kept}
    launches = [checked(lib.svg_band_shard_attention_lse,
                        (q_r.data_ptr(), shards[s][0].data_ptr(), shards[s][1].data_ptr(), outs[s][0].data_ptr(), outs[s][1].data_ptr(), w.H, w.S,
                         w.D, 0, scale, C.byref(w.mask), C.byref(perm), C.byref(sh[rank]), C.byref(sh[s]), None, st), f"shard rank {rank} over {s}")
                for s in kept]

    def fb():
        for run in launches:
            run()

    fa()
    fb()
    torch.cuda.synchronize()
    merged = nat.merge_attention_states([outs[s][0] for s in kept], [outs[s][1] for s in kept])
    ref = shard_of(o_full, sh[rank], w).float()
    merged_rel_l2 = ((merged.float() - ref).norm() / ref.norm()).item()
    wa, wb, calls = alternate(fa, fb, alternations, min_ms)
    rec = {"pair": label, "a": "svg_band_attention_switch_lse over all S rows", "b": f"svg_band_shard_attention_lse, rows of rank {rank} over the kept shards",
           "workload": "tiny" if w.S < 10000 else "hunyuan_720p", "rank": rank, "frames_of_rank": [sh[rank].f0, sh[rank].f0 + sh[rank].n_frames],
           "tail_rows": sh[rank].n_tail, "rows": n, "parts_kept": len(kept), "kept_shards": kept, "token_major_heads": int(w.flags.sum())}
    rec.update(w.cfg)
    rec.update({"alternations": alternations, "repetitions_per_window": calls})
    rec.update(stats(wa, wb))
    ms_a, ms_b = rec["a_ms"], rec["b_ms"]
    per_tok = 2 * w.H * w.D * 2      # k and v of one token, all heads, 16-bit
    rec.update({
        "b_over_a": round(ms_b / ms_a, 4), "b_over_full_eighth": round(ms_b / (ms_a / WORLD), 4),
        "row_share": round(n / w.S, 5), "b_over_row_share": round(ms_b / (ms_a * n / w.S), 4),
        "largest_shard_over_mean": round(max(rows) / (sum(rows) / WORLD), 4),
        "bytes_received_with_plan": sum(rows[s] * per_tok for s in kept if s != rank),
        "bytes_received_without_plan": sum(rows[s] * per_tok for s in range(WORLD) if s != rank),
        "parts_kept_logical_heads_only": len(kept_logical),
        "bytes_received_with_plan_logical_heads_only": sum(rows[s] * per_tok for s in kept_logical if s != rank),
        "merged_vs_full_call_rel_l2": round(merged_rel_l2, 6), "lse_free_of_nan": not any(bool(torch.isnan(outs[s][1]).any()) for s in kept),
        "part_rows_without_keys": sum(int(torch.isinf(outs[s][1]).sum()) for s in kept),
        "multi_gpu_timing": "none: one GPU runs one rank's launches, no exchange was timed", "shader_clock": "not recorded",
    })
    return rec


def rank_launches(nat, w, rank, dense):
    """the rank's q rows, the shards the OR-ed plan keeps for it as buffers of their own, and an output pair per shard"""
    from svg.distributed import band_shard_exchange_plan, frame_shard

    sh = [frame_shard(w.geo, r, WORLD) for r in range(WORLD)]
    plan = band_shard_exchange_plan(w.mask, w.geo, WORLD, "both", dense_mask=dense)
    kept = [s for s in range(WORLD) if plan[rank][s]]
    q_r = shard_of(w.q, sh[rank], w)
    n = nat.band_shard_rows(sh[rank], w.P)
    shards = {s: (shard_of(w.k, sh[s], w), shard_of(w.v, sh[s], w)) for s in kept}

    def outs():
        return {s: (torch.empty_like(q_r), torch.empty(1, w.H, n, dtype=torch.float32, device="cuda")) for s in kept}

    return sh, kept, q_r, n, shards, outs


def all_of(launches):
    def run():
        for one in launches:
            one()

    return run


def switch_lines(nat, lib, w, rank, label, alternations, min_ms):
    st = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / math.sqrt(w.D)
    dense = nat.BandMask(w.mask.real_len, w.S + 1, 0, 0, 0, 0)
    sh, kept, q_r, n, shards, outs = rank_launches(nat, w, rank, dense)
    perm = nat.PermDesc(w.flags.data_ptr(), 0, w.F, w.P)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    o_plain, o_sw = outs(), outs()
    head = lambda s, o: (q_r.data_ptr(), shards[s][0].data_ptr(), shards[s][1].data_ptr(), o[s][0].data_ptr(), o[s][1].data_ptr(), w.H, w.S, w.D,  # noqa: E731
                         0, scale, C.byref(w.mask), C.byref(perm))
    plain = all_of([checked(lib.svg_band_shard_attention_lse, head(s, o_plain) + (C.byref(sh[rank]), C.byref(sh[s]), None, st),
                            f"shard rank {rank} over {s}") for s in kept])
    switch = all_of([checked(lib.svg_band_shard_attention_switch_lse,
                             head(s, o_sw) + (C.byref(dense), flag.data_ptr(), C.byref(sh[rank]), C.byref(sh[s]), None, st),
                             f"shard switch rank {rank} over {s}") for s in kept])
    base = {"workload": "tiny" if w.S < 10000 else "hunyuan_720p", "rank": rank, "frames_of_rank": [sh[rank].f0, sh[rank].f0 + sh[rank].n_frames],
            "tail_rows": sh[rank].n_tail, "rows": n, "parts_kept": len(kept), "kept_shards": kept, "token_major_heads": int(w.flags.sum()),
            "alt_mask": "dense, real_len of the sparse mask"}
    base.update(w.cfg)
    notes = {"multi_gpu_timing": "none: one GPU runs one rank's launches, no exchange was timed", "shader_clock": "not recorded"}
    # flag 0: the switch entry beside the plain shard entry — the same body
    plain()
    switch()
    torch.cuda.synchronize()
    same = all(torch.equal(o_plain[s][0], o_sw[s][0]) and torch.equal(o_plain[s][1], o_sw[s][1]) for s in kept)
    wa, wb, calls = alternate(plain, switch, alternations, min_ms)
    rec0 = {"pair": f"{label}_flag0", "a": f"svg_band_shard_attention_lse, rows of rank {rank} over the kept shards",
            "b": "svg_band_shard_attention_switch_lse, flag 0, the same launches"}
    rec0.update(base)
    rec0.update({"alternations": alternations, "repetitions_per_window": calls})
    rec0.update(stats(wa, wb))
    diff = rec0["b_ms"] - rec0["a_ms"]
    rec0.update({"b_over_a": round(rec0["b_ms"] / rec0["a_ms"], 4), "diff_ms": round(diff, 4),
                 "inside_a_spread": bool(abs(diff) <= rec0["a_spread_ms"]), "same_bits": same})
    rec0.update(notes)
    # flag 1: the rank's dense launches beside the full-S dense call of the switch entry
    flag.fill_(1)
    o_full, lse_full = torch.empty_like(w.q), torch.empty(1, w.H, w.S, dtype=torch.float32, device="cuda")
    full = checked(lib.svg_band_attention_switch_lse,
                   (w.q.data_ptr(), w.k.data_ptr(), w.v.data_ptr(), o_full.data_ptr(), lse_full.data_ptr(), w.H, w.S, w.D, 0, scale,
                    C.byref(w.mask), C.byref(perm), C.byref(dense), flag.data_ptr(), None, st), "svg_band_attention_switch_lse")
    full()
    switch()
    torch.cuda.synchronize()
    merged = nat.merge_attention_states([o_sw[s][0] for s in kept], [o_sw[s][1] for s in kept])
    ref = shard_of(o_full, sh[rank], w).float()
    merged_rel_l2 = ((merged.float() - ref).norm() / ref.norm()).item()
    wa, wb, calls = alternate(full, switch, alternations, min_ms)
    rec1 = {"pair": f"{label}_flag1", "a": "svg_band_attention_switch_lse over all S rows, flag 1 (dense)",
            "b": f"svg_band_shard_attention_switch_lse, flag 1, rows of rank {rank} over the kept shards"}
    rec1.update(base)
    rec1.update({"alternations": alternations, "repetitions_per_window": calls})
    rec1.update(stats(wa, wb))
    rec1.update({"b_over_a": round(rec1["b_ms"] / rec1["a_ms"], 4), "b_over_full_eighth": round(rec1["b_ms"] / (rec1["a_ms"] / WORLD), 4),
                 "row_share": round(n / w.S, 5), "b_over_row_share": round(rec1["b_ms"] / (rec1["a_ms"] * n / w.S), 4),
                 "merged_vs_full_call_rel_l2": round(merged_rel_l2, 6),
                 "lse_free_of_nan": not any(bool(torch.isnan(o_sw[s][1]).any()) for s in kept),
                 "part_rows_without_keys": sum(int(torch.isinf(o_sw[s][1]).sum()) for s in kept), "threshold": "none set"})
    rec1.update(notes)
    return rec0, rec1


def shard_parent_line(nat, new, old, w, alternations, min_ms):
    """the plain shard launches of the first rank: this build (B) against the parent's library (A) in the same process"""
    st = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / math.sqrt(w.D)
    sh, kept, q_r, n, shards, outs = rank_launches(nat, w, 0, None)
    perm = nat.PermDesc(w.flags.data_ptr(), 0, w.F, w.P)
    o = [outs(), outs()]
    runs = [all_of([checked(lib.svg_band_shard_attention_lse,
                            (q_r.data_ptr(), shards[s][0].data_ptr(), shards[s][1].data_ptr(), o[i][s][0].data_ptr(), o[i][s][1].data_ptr(), w.H,
                             w.S, w.D, 0, scale, C.byref(w.mask), C.byref(perm), C.byref(sh[0]), C.byref(sh[s]), None, st),
                            f"shard rank 0 over {s}") for s in kept]) for i, lib in enumerate((old, new))]
    runs[0]()
    runs[1]()
    torch.cuda.synchronize()
    same = all(torch.equal(o[0][s][0], o[1][s][0]) and torch.equal(o[0][s][1], o[1][s][1]) for s in kept)
    wa, wb, calls = alternate(runs[0], runs[1], alternations, min_ms)
    rec = {"pair": "shard_vs_parent", "a": "parent: svg_band_shard_attention_lse, rows of rank 0 over the kept shards",
           "b": "this build: the same launches", "workload": "tiny" if w.S < 10000 else "hunyuan_720p", "parts_kept": len(kept),
           "token_major_heads": int(w.flags.sum())}
    rec.update(w.cfg)
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
    ap.add_argument("--out", default=None, help="default: profiles/band_shard_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    ap.add_argument("--switch", action="store_true", help="the device switch of the shard form (default output: profiles/band_shard_switch_ab.jsonl)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_band_shard: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    new = typed(nat, nat.lib_path(), ["svg_band_attention", "svg_band_attention_switch_lse", "svg_band_shard_attention_lse",
                                      "svg_band_shard_attention_switch_lse"])
    out = Path(a.out or ROOT / "profiles" / ("band_shard_switch_ab.jsonl" if a.switch else "band_shard_ab.jsonl"))
    out.parent.mkdir(parents=True, exist_ok=True)
    alternations = 2 if a.tiny else max(a.alternations, 5)
    min_ms = 20.0 if a.tiny else a.min_ms
    w = workload(nat, a.tiny)
    with out.open("a") as f:
        def emit(rec):
            line = json.dumps(rec)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if a.switch:
            for rank, label in ((0, "first_rank"), (WORLD // 2 - 1, "middle_rank"), (WORLD - 1, "last_rank")):
                for rec in switch_lines(nat, new, w, rank, label, alternations, min_ms):
                    emit(rec)
            if a.parent:
                old = typed(nat, a.parent, ["svg_band_attention", "svg_band_shard_attention_lse"])
                emit(parent_line(nat, new, old, w, alternations, min_ms))
                emit(shard_parent_line(nat, new, old, w, alternations, min_ms))
            return
        emit(rank_line(nat, new, w, 0, "first_rank", alternations, min_ms))
        emit(rank_line(nat, new, w, WORLD // 2 - 1, "middle_rank", alternations, min_ms))
        emit(rank_line(nat, new, w, WORLD - 1, "last_rank", alternations, min_ms))
        if a.parent:
            emit(parent_line(nat, new, typed(nat, a.parent, ["svg_band_attention"]), w, alternations, min_ms))


if __name__ == "__main__":
    main()
