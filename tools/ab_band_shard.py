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
    sigs = {**nat.SIGNATURES, **nat.BAND_LSE_FORM_SIGNATURES, **nat.BAND_SHARD_SIGNATURES}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsvgattn.so built from the parent commit (adds the plain_vs_parent line)")
    ap.add_argument("--alternations", type=int, default=7)
    ap.add_argument("--min-ms", type=float, default=500.0)
    ap.add_argument("--out", default=None, help="default: profiles/band_shard_ab.jsonl (appended to)")
    ap.add_argument("--tiny", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ab_band_shard: needs a GPU (a measurement path does not fall back)")
    from svg import _native as nat

    nat.load()
    new = typed(nat, nat.lib_path(), ["svg_band_attention", "svg_band_attention_switch_lse", "svg_band_shard_attention_lse"])
    out = Path(a.out or ROOT / "profiles" / "band_shard_ab.jsonl")
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

        emit(rank_line(nat, new, w, 0, "first_rank", alternations, min_ms))
        emit(rank_line(nat, new, w, WORLD // 2 - 1, "middle_rank", alternations, min_ms))
        emit(rank_line(nat, new, w, WORLD - 1, "last_rank", alternations, min_ms))
        if a.parent:
            emit(parent_line(nat, new, typed(nat, a.parent, ["svg_band_attention"]), w, alternations, min_ms))


if __name__ == "__main__":
    main()
