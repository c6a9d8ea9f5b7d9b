"""A/B on one box, one process: the HunyuanVideo joint text+video prologue (svg_qk_norm_rope_transpose_joint, joint_prologue = True)
against the staged path it replaces (video prologue, text transposes + torch norms, three torch.cat), at 720p (S_v = 118 800, T = 256,
24 heads of 128, bf16), on the same seeded inputs, the two paths alternating.

    python tools/ab_joint_prologue.py [reps]

Prints one JSON line per case:
  kernel     the joint launch vs the staged sequence: ms, algorithmic GB/s (each of q, k, v read once and written once), equal outputs;
             and svg_qk_norm_rope_transpose (q, k) + the v transpose on the same bytes, for the per-byte comparison
  processor  dense / SVG1 processor __call__, double- and single-stream stand-in blocks (tests/standins.Attention(3072, 24)),
             joint_prologue True / False: ms per call (HIP events after a device synchronise, 2 warm-up calls), the
             torch.cuda.max_memory_allocated delta over the call, an output checksum."""
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
for p in (ROOT / "sparse-videogen_amd", ROOT, ROOT / "tests"):
    sys.path.insert(0, str(p))

HEADS, HD = 24, 128
DIM = HEADS * HD
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


def rope(n, d):
    pos = torch.arange(n)[:, None].float()
    inv = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
    ang = (pos * inv[None]).repeat_interleave(2, dim=1)
    return ang.cos().cuda(), ang.sin().cuda()


def kernel_ab(reps, V, T):
    from standins import RMSNorm
    from svg import _native as nat
    from svg.models import _core

    g = torch.Generator().manual_seed(0)
    vid = [(torch.randn(1, V, DIM, generator=g)).to(DT).cuda() for _ in range(3)]
    txt = [(torch.randn(1, T, DIM, generator=g)).to(DT).cuda() for _ in range(3)]
    norms = [RMSNorm(HD).to(DT).cuda() for _ in range(4)]
    with torch.no_grad():
        for n in norms:
            n.weight.copy_(1 + 0.2 * torch.randn(HD, generator=g))
    cos, sin = rope(V, HD)

    def new():
        return _core.joint_qkv_from_projections(vid, txt, HEADS, *norms, cos, sin, 0, V)

    def old():   # the staged path of the double-stream processor: video prologue, text transposes + torch norms, three torch.cat
        q, k, v = _core.qkv_from_projections(*vid, HEADS, norms[0], norms[1], cos, sin, 0, V)
        eq, ek, ev = (t.unflatten(2, (HEADS, -1)).transpose(1, 2) for t in txt)
        eq, ek = norms[2](eq), norms[3](ek)
        return torch.cat([q, eq], dim=2), torch.cat([k, ek], dim=2), torch.cat([v, ev], dim=2)

    src = [torch.cat([a, b], dim=1) for a, b in zip(vid, txt)]   # the same bytes as one token-major stream

    def single():   # svg_qk_norm_rope_transpose on q, k + the v transpose (norm 1, RoPE on the video rows)
        nat.qk_norm_rope_transpose(src[0], src[1], HEADS, HEADS, 1, norms[0].weight, None, norms[1].weight, None, 1e-6, 1, cos, sin, 0, V)
        nat.qk_norm_rope_transpose(src[2], None, HEADS, 0)

    with torch.no_grad():
        a, b = new(), old()
        torch.cuda.synchronize()
        video_equal = all(torch.equal(x[:, :, :V], y[:, :, :V]) for x, y in zip(a, b))
        text_equal = all(torch.equal(x[:, :, V:], y[:, :, V:]) for x, y in zip(a, b))
        text_diff = sum(int((x[:, :, V:] != y[:, :, V:]).sum()) for x, y in zip(a, b))
        del a, b
        t_new, t_old, t_one = 0.0, 0.0, 0.0
        for _ in range(3):   # alternate
            t_new += timed(new, reps) / 3
            t_old += timed(old, reps) / 3
            t_one += timed(single, reps) / 3
    nbytes = 2 * 3 * (V + T) * DIM * 2
    gbs = lambda ms: nbytes / (ms * 1e-3) / 1e9  # noqa: E731
    print(json.dumps({"case": "kernel", "S_v": V, "T": T, "joint_ms": round(t_new, 4), "staged_ms": round(t_old, 4),
                      "joint_GBps": round(gbs(t_new), 1), "staged_GBps": round(gbs(t_old), 1),
                      "transpose_entry_points_ms": round(t_one, 4), "transpose_entry_points_GBps": round(gbs(t_one), 1),
                      "joint_per_byte_vs_entry_points": round(t_one / t_new, 4), "joint_fraction_of_6300GBps": round(gbs(t_new) / 6300, 3),
                      "video_rows_equal": video_equal, "text_rows_equal_to_torch_norm": text_equal, "text_elements_differing": text_diff,
                      "text_elements": 3 * T * DIM}), flush=True)


def processor_ab(reps, pattern):
    from standins import Attention, Block, Pipe, Transformer
    from svg.models import _core
    from svg.models.hyvideo.attention import HunyuanVideoAttnProcessor2_0_FlashAttention, _HunyuanProcessorBase
    from svg.models.hyvideo.inference import replace_hyvideo_attention

    torch.manual_seed(0)
    blocks = [Block(Attention(DIM, HEADS, added_kv=True, dtype=DT), "attn"), Block(Attention(DIM, HEADS, dtype=DT), "attn")]
    tr = Transformer(blocks[:1], "transformer_blocks")
    tr.single_transformer_blocks = torch.nn.ModuleList(blocks[1:])
    tr.cuda()
    cls = replace_hyvideo_attention(Pipe(tr), 720, 1280, 129, 64, first_layers_fp=0, first_times_fp=900.0, pattern="SVG",
                                    num_sampled_rows=64, sparsity=0.25)
    if pattern == "dense":
        for blk in blocks:
            blk.attn.set_processor(HunyuanVideoAttnProcessor2_0_FlashAttention(0))
    ctx, V = cls.context_length, cls.num_frame * cls.frame_size
    g = torch.Generator().manual_seed(1)
    base = (torch.randn(1, V + ctx, DIM, generator=g) * 0.3).to(DT).cuda()
    amask = torch.zeros(1, V + ctx, dtype=torch.bool, device="cuda")
    amask[:, :V + 64] = True
    rp = rope(V, HD)
    ts = torch.tensor([100.0])
    for name, blk, h, e in (("double", blocks[0], base[:, :V].contiguous(), base[:, V:].contiguous()),
                            ("single", blocks[1], base[:, :V], base[:, V:])):   # single stream: the two adjacent slices the block passes
        res = {}

        def call():
            return blk.attn(h, encoder_hidden_states=e, attention_mask=amask, image_rotary_emb=rp, timestep=ts)

        with torch.no_grad():
            for rnd in range(2):   # alternate the two paths
                for joint in (True, False):
                    _HunyuanProcessorBase.joint_prologue = joint
                    torch.manual_seed(7)
                    _core.reseed_switch_generator(7)
                    ms = timed(call, reps)
                    torch.cuda.synchronize()
                    base_mem = torch.cuda.memory_allocated()
                    torch.cuda.reset_peak_memory_stats()
                    torch.manual_seed(7)
                    out = call()
                    torch.cuda.synchronize()
                    peak = torch.cuda.max_memory_allocated() - base_mem
                    chk = sum(float(o.double().sum()) for o in out if o is not None)
                    r = res.setdefault(joint, {"ms": [], "peak_delta_MB": 0.0, "checksum": chk})
                    r["ms"].append(ms)
                    r["peak_delta_MB"] = round(peak / 2 ** 20, 1)
                    del out
        _HunyuanProcessorBase.joint_prologue = True
        for joint in (True, False):
            r = res[joint]
            print(json.dumps({"case": "processor", "processor": pattern, "block": name, "joint_prologue": joint,
                              "ms": round(sum(r["ms"]) / len(r["ms"]), 3), "ms_rounds": [round(x, 3) for x in r["ms"]],
                              "peak_delta_MB": r["peak_delta_MB"], "checksum": r["checksum"]}), flush=True)
        print(json.dumps({"case": "processor_delta", "processor": pattern, "block": name,
                          "saving_ms": round(sum(res[False]["ms"]) / 2 - sum(res[True]["ms"]) / 2, 3),
                          "peak_drop_MB": round(res[False]["peak_delta_MB"] - res[True]["peak_delta_MB"], 1),
                          "checksums_equal": res[True]["checksum"] == res[False]["checksum"]}), flush=True)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    torch.cuda.init()
    kernel_ab(max(reps, 10), 118800, 256)
    for pattern in ("dense", "SVG"):
        processor_ab(reps, pattern)


if __name__ == "__main__":
    main()
