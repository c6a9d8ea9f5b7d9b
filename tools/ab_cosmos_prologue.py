"""A/B on one box, one process: the Cosmos prologue in one pass (svg_qk_norm_rope_transpose with rope_kind 3, half-split RoPE;
`fused_prologue = True` of the Cosmos processors) against the staged sequence it replaces (three `.transpose(1, 2).contiguous()` copies,
the in-place HIP norm, apply_rotary_emb_half in torch), at Cosmos-7B 720p (32 heads of 128, S = 16 frames x 3520 = 56 320 tokens, bsz 1,
bf16), on the same seeded inputs, the sides alternating.

    python tools/ab_cosmos_prologue.py [alternations >= 7] [reps per timing]

Prints one JSON line per case (HIP events after a device synchronise, warm-up calls in front of every timing):
  kernel     rope_kind 3 vs the staged sequence vs rope_kind 1 on the same bytes: ms per alternation, mean, spread (max - min over the
             alternations), algorithmic GB/s (each of q and k read once and written once), whether the fused q, k equal the staged ones,
             whether the fused side won every alternation
  processor  Cosmos_SVG_AttnProcessor2_0.__call__ on tests/standins.Attention(4096, 32, qk_norm="rms"), fused_prologue True / False, the
             sparse step and the cross call (512 text keys): ms per call, the torch.cuda.max_memory_allocated delta over one call, an
             output checksum
Exit code 1 when the staged side wins an alternation of a kernel or processor row, or outputs differ."""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT, ROOT / "tests"):
    sys.path.insert(0, str(p))

HEADS, HD, FRAMES, FRAME = 32, 128, 16, 3520
DIM, S, N_TXT = HEADS * HD, FRAMES * FRAME, 512
DT = torch.bfloat16


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(xs):
    return {"ms": round(sum(xs) / len(xs), 4), "ms_alternations": [round(x, 4) for x in xs], "spread_ms": round(max(xs) - min(xs), 4)}


def kernel_ab(alts, reps):
    from standins import RMSNorm
    from svg import _native as nat
    from svg.models import _core
    from svg.models.cosmos.attention import apply_rotary_emb_half

    g = torch.Generator().manual_seed(0)
    q_in, k_in, v_in = ((torch.randn(1, S, DIM, generator=g)).to(DT).cuda() for _ in range(3))
    nq, nk = RMSNorm(HD).to(DT).cuda(), RMSNorm(HD).to(DT).cuda()
    with torch.no_grad():
        for n in (nq, nk):
            n.weight.copy_(1 + 0.2 * torch.randn(HD, generator=g))
    ang = torch.rand(S, HD // 2, generator=g) * 6.28
    cos, sin = torch.cat([ang.cos(), ang.cos()], -1).cuda(), torch.cat([ang.sin(), ang.sin()], -1).cuda()
    qw, kw = nq.weight.detach(), nk.weight.detach()

    def fused():   # q, k: one pass; v: the head view of the projection's output, no copy
        q, k, v = _core.qkv_from_projections(q_in, k_in, v_in, HEADS, nq, nk, cos, sin, 0, S, half_split=True)
        return q, k

    def staged():   # get_transpose_qkv -> get_qk_norm -> get_rotary_emb of the processors
        q, k, v = (x.unflatten(2, (HEADS, -1)).transpose(1, 2).contiguous() for x in (q_in, k_in, v_in))
        assert _core.qk_norm_inplace(nq, nk, q, k)
        return apply_rotary_emb_half(q, (cos, sin)), apply_rotary_emb_half(k, (cos, sin))

    def kind1():   # the interleaved-pairs kernel on the same bytes
        return nat.qk_norm_rope_transpose(q_in, k_in, HEADS, HEADS, 1, qw, None, kw, None, 1e-6, 1, cos, sin, 0, S)

    with torch.no_grad():
        a, b = fused(), staged()
        torch.cuda.synchronize()
        equal = bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]))
        del a, b
        t = {"fused": [], "staged": [], "kind1": []}
        for _ in range(alts):
            t["fused"].append(timed(fused, reps))
            t["staged"].append(timed(staged, reps))
            t["kind1"].append(timed(kind1, reps))
    nbytes = 2 * 2 * S * DIM * 2   # q and k, read once and written once, 2 bytes per element
    gbs = lambda ms: round(nbytes / (ms * 1e-3) / 1e9, 1)  # noqa: E731
    wins = all(f < s for f, s in zip(t["fused"], t["staged"]))
    row = {"case": "kernel", "H": HEADS, "D": HD, "S": S, "bsz": 1, "dtype": "bf16", "alternations": alts, "reps": reps,
           "algorithmic_MB": round(nbytes / 1e6, 1)}
    for name in ("fused", "staged", "kind1"):
        st = stats(t[name])
        row.update({f"{name}_{k}": v for k, v in st.items()}, **{f"{name}_GBps": gbs(st["ms"])})
    f, o = row["fused_ms"], row["kind1_ms"]
    row.update({"staged_over_fused": round(row["staged_ms"] / f, 2), "fused_minus_kind1_ms": round(f - o, 4),
                "fused_over_kind1": round(f / o, 4), "kind_spread_ms": max(row["fused_spread_ms"], row["kind1_spread_ms"]),
                "fused_equals_staged": equal, "fused_wins_every_alternation": wins})
    print(json.dumps(row), flush=True)
    return wins and equal


def processor_ab(alts, reps):
    from standins import Attention
    from svg.models import _core
    from svg.models.cosmos.attention import Cosmos_SVG_AttnProcessor2_0 as P, prepare_flexattention
    from svg.models.cosmos.utils import sparsity_to_width

    torch.manual_seed(0)
    P.context_length, P.num_frame, P.frame_size = 0, FRAMES, FRAME
    P.first_layers_fp, P.first_times_fp, P.num_sampled_rows, P.sample_mse_max_row = 0, 900.0, 64, 10000
    w = sparsity_to_width(0.25, 0, FRAMES, FRAME)
    P.block_mask = prepare_flexattention(1, None, None, DT, None, 0, 0, FRAMES, FRAME, w, w)
    attn = Attention(DIM, HEADS, qk_norm="rms", dtype=DT).cuda()
    proc = P(0)
    attn.set_processor(proc)
    g = torch.Generator().manual_seed(1)
    hidden = (torch.randn(1, S, DIM, generator=g) * 0.3).to(DT).cuda()
    enc = (torch.randn(1, N_TXT, DIM, generator=g) * 0.3).to(DT).cuda()
    ang = torch.rand(S, HD // 2, generator=g) * 6.28
    rope = (torch.cat([ang.cos(), ang.cos()], -1).cuda(), torch.cat([ang.sin(), ang.sin()], -1).cuda())
    ts = torch.tensor([100.0])
    ok = True
    for name, kw in (("sparse_step", dict(image_rotary_emb=rope, timestep=ts)), ("cross_call", dict(encoder_hidden_states=enc, timestep=None))):
        res = {}

        def call():
            return attn(hidden, **kw)

        with torch.no_grad():
            for _ in range(alts):
                for fused in (True, False):
                    proc.fused_prologue = fused
                    torch.manual_seed(7)
                    _core.reseed_switch_generator(7)
                    ms = timed(call, reps, warm=1)
                    base_mem = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    torch.manual_seed(7)
                    _core.reseed_switch_generator(7)
                    out = call()
                    torch.cuda.synchronize()
                    peak = torch.cuda.max_memory_allocated() - base_mem
                    r = res.setdefault(fused, {"ms": [], "peak_delta_MB": 0.0, "checksum": float(out.double().sum())})
                    r["ms"].append(ms)
                    r["peak_delta_MB"] = round(peak / 2 ** 20, 1)
                    del out
        for fused in (True, False):
            r = res[fused]
            print(json.dumps({"case": "processor", "call": name, "fused_prologue": fused, **stats(r["ms"]), "peak_delta_MB": r["peak_delta_MB"],
                              "checksum": r["checksum"]}), flush=True)
        wins = all(a < b for a, b in zip(res[True]["ms"], res[False]["ms"]))
        same = res[True]["checksum"] == res[False]["checksum"]
        ok = ok and wins and same
        print(json.dumps({"case": "processor_delta", "call": name,
                          "saving_ms": round(sum(res[False]["ms"]) / alts - sum(res[True]["ms"]) / alts, 3),
                          "peak_drop_MB": round(res[False]["peak_delta_MB"] - res[True]["peak_delta_MB"], 1),
                          "fused_wins_every_alternation": wins, "checksums_equal": same}), flush=True)
    proc.fused_prologue = True
    return ok


def main():
    alts = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 7
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    torch.cuda.init()
    ok = kernel_ab(alts, reps)
    ok = processor_ab(alts, max(1, reps // 2)) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
