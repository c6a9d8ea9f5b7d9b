"""svg_qk_norm_rope_transpose_joint (the MMDiT joint prologue) against the composition of the existing entry points, bit for bit, its
argument checks, and the HunyuanVideo processors on the copy-free joint path (joint_prologue = True) against the staged path (False)."""
import pytest
import torch

from standins import Attention, Block, Pipe, Transformer

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu


def _nat():
    from poisoned import load_native

    return load_native()


def _tables(n, d, kind):
    pos = torch.arange(n)[:, None].float()
    inv = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
    ang = pos * inv[None]
    if kind == 2:
        return ang.cos().cuda().contiguous(), ang.sin().cuda().contiguous()
    return ang.repeat_interleave(2, 1).cos().cuda().contiguous(), ang.repeat_interleave(2, 1).sin().cuda().contiguous()


def _segment(nat, bsz, rows, H, D, dt, norm, gen):
    mk = lambda: (torch.randn(bsz, rows, H * D, generator=gen) * 2).to(dt).cuda()  # noqa: E731
    w = lambda: (1 + 0.3 * torch.randn(D, generator=gen)).to(dt).cuda() if norm else None  # noqa: E731
    b = lambda: (0.2 * torch.randn(D, generator=gen)).to(dt).cuda() if norm == 2 else None  # noqa: E731
    return nat.JointSegment(mk(), mk(), mk(), norm, w(), b(), w(), b(), 1e-5 if norm == 2 else 1e-6)


def _composition(nat, segs, H, rk, cos, sin, lo, hi, q_scale):
    """The existing entry points per segment (svg_qk_norm_rope_transpose_qscale on q, k with the RoPE rows that fall into the segment,
    the plain transpose of v), concatenated along the rows."""
    outs, start = [], 0
    for sg in segs:
        n = sg.q.shape[1]
        if n == 0:
            continue
        a, b = max(lo, start), min(hi, start + n)
        kw = dict(rope_kind=0)
        if rk and b > a:
            kw = dict(rope_kind=rk, cos=cos[a - lo:b - lo].contiguous(), sin=sin[a - lo:b - lo].contiguous(), rope_lo=a - start, rope_hi=b - start)
        q, k = nat.qk_norm_rope_transpose(sg.q, sg.k, H, H, sg.norm_kind, sg.q_weight, sg.q_bias, sg.k_weight, sg.k_bias, sg.eps,
                                          q_scale=q_scale, **kw)
        v, _ = nat.qk_norm_rope_transpose(sg.v, None, H, 0)
        outs.append((q, k, v))
        start += n
    return tuple(torch.cat([o[i] for o in outs], dim=2) for i in range(3))


def _check_equal(nat, segs, H, rk=0, cos=None, sin=None, lo=0, hi=0, q_scale=1.0):
    got = nat.qk_norm_rope_transpose_joint(segs, H, rk, cos, sin, lo, hi, q_scale=q_scale)
    want = _composition(nat, segs, H, rk, cos, sin, lo, hi, q_scale)
    torch.cuda.synchronize()
    for g, w, name in zip(got, want, "qkv"):
        assert g.shape == w.shape, name
        assert torch.equal(g.view(torch.int16), w.view(torch.int16)), (name, (g != w).sum().item())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("norm", [0, 1, 2])
@pytest.mark.parametrize("rk", [1, 2])
def test_one_segment_equals_transpose_entry_point(dt, D, norm, rk):
    nat = _nat()
    gen = torch.Generator().manual_seed(D * 10 + norm + rk)
    H, S = 3, 301
    seg = _segment(nat, 1, S, H, D, dt, norm, gen)
    cos, sin = _tables(S - 17, D, rk)
    for q_scale in (1.0, nat.softmax_q_scale(D)):
        _check_equal(nat, [seg], H, rk, cos, sin, 17, S, q_scale)


@pytest.mark.parametrize("D", [32, 256])
def test_one_segment_other_head_dims(D):
    nat = _nat()
    gen = torch.Generator().manual_seed(D)
    seg = _segment(nat, 1, 77, 2, D, torch.bfloat16, 1, gen)
    cos, sin = _tables(77, D, 1)
    _check_equal(nat, [seg], 2, 1, cos, sin, 0, 77, nat.softmax_q_scale(D))


@pytest.mark.parametrize("sa,sb", [(1001, 7), (4096, 256), (0, 256)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_two_segments_equal_concatenated_calls(sa, sb, dt):
    nat = _nat()
    gen = torch.Generator().manual_seed(sa + sb)
    H, D, bsz = 3, 128, 2
    a = _segment(nat, bsz, sa, H, D, dt, 1, gen)
    b = _segment(nat, bsz, sb, H, D, dt, 2, gen)   # a different norm kind per segment
    S = sa + sb
    for lo, hi in ((0, sa), (sa // 3, sa // 2 + 1), (sa // 2, S), (0, S)):   # RoPE inside A, crossing into B, everything
        if hi <= lo:
            continue
        cos, sin = _tables(hi - lo, D, 1)
        for q_scale in (1.0, nat.softmax_q_scale(D)):
            _check_equal(nat, [a, b], H, 1, cos, sin, lo, hi, q_scale)
    _check_equal(nat, [a, b], H)   # no RoPE at all
    # the text stream without a norm (kind 0) next to an RMS-normalised video stream
    _check_equal(nat, [a, b._replace(norm_kind=0)], H)


def test_hunyuan_720p_shape():
    nat = _nat()
    gen = torch.Generator().manual_seed(720)
    H, D, sa, sb = 24, 128, 118800, 256
    a = _segment(nat, 1, sa, H, D, torch.bfloat16, 1, gen)
    b = _segment(nat, 1, sb, H, D, torch.bfloat16, 1, gen)
    cos, sin = _tables(sa, D, 1)
    _check_equal(nat, [a, b], H, 1, cos, sin, 0, sa)


def test_argument_checks_launch_nothing():
    nat = _nat()
    lib = nat.load()
    H, D, n = 2, 64, 40
    dt = torch.bfloat16
    src = [torch.randn(1, n, H * D).to(dt).cuda() for _ in range(3)]
    outs = [torch.full((1, H, n, D), 7.0, dtype=dt, device="cuda") for _ in range(3)]
    cos, sin = _tables(n, D, 1)
    P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(segs, o=outs, bsz=1, h=H, d=D, dtype=0, rk=1, lo=0, hi=n, q_scale=1.0, n_seg=None):
        arr = (nat.PrologueSegment * max(len(segs), 1))()
        for a, s in zip(arr, segs):
            a.q_in, a.k_in, a.v_in, a.rows, a.norm_kind, a.eps = P(s[0]), P(s[1]), P(s[2]), s[3], s[4], 1e-6
        return lib.svg_qk_norm_rope_transpose_joint(arr, len(segs) if n_seg is None else n_seg, P(o[0]), P(o[1]), P(o[2]), bsz, h, d, dtype,
                                                    rk, cos.data_ptr(), sin.data_ptr(), lo, hi, q_scale, nat._stream())

    good = (src[0], src[1], src[2], n, 1)
    BAD, UNSUP = -1, -2
    assert call([good], n_seg=0) == BAD and call([good, good, good]) == BAD
    assert call([(None, src[1], src[2], n, 1)]) == BAD                        # q output requested, no q input
    assert call([good], o=[None, outs[1], outs[2]]) == BAD                    # q input without its output
    assert call([good], o=[None, None, None]) == BAD
    assert call([(outs[0], src[1], src[2], n, 1)]) == BAD                     # an input equal to an output
    assert call([(src[0], src[1], outs[1], n, 1)]) == BAD
    assert call([(src[0], src[1], src[2], -1, 1)]) == BAD                     # rows < 0
    assert call([good, (src[0], src[1], src[2], -5, 1)]) == BAD
    assert call([(src[0], src[1], src[2], 0, 1)]) == BAD                      # nothing to do
    assert call([good], h=1 << 24, d=128) == BAD                              # total above INT32_MAX / (H * D)
    assert call([good], lo=-1) == BAD and call([good], hi=n + 1) == BAD and call([good], lo=5, hi=4) == BAD
    assert call([(src[0], src[1], src[2], n, 3)]) == BAD and call([good], rk=3) == BAD
    assert call([good], q_scale=0.0) == BAD and call([good], bsz=0) == BAD
    assert call([good], d=48) == UNSUP and call([good], dtype=5) == UNSUP
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == 7.0).all())                                         # nothing was launched
    assert call([good]) == 0                                                  # (and the valid call runs)
    torch.cuda.synchronize()
    assert not bool((outs[0] == 7.0).all())


# ---- processors ---------------------------------------------------------------------------------------------------------------
def _rope(n, d):
    pos = torch.arange(n)[:, None].float()
    inv = 1.0 / (10000 ** (torch.arange(0, d, 2).float() / d))
    ang = (pos * inv[None]).repeat_interleave(2, dim=1)
    return ang.cos(), ang.sin()


def _install(pattern):
    """A Hunyuan stand-in pipe (one double-stream, one single-stream block) with the processors of `pattern` installed."""
    from svg.models.hyvideo.attention import HunyuanVideoAttnProcessor2_0_FlashAttention
    from svg.models.hyvideo.inference import replace_hyvideo_attention

    heads, hd = 4, 128
    dim = heads * hd
    torch.manual_seed(3)
    dt = torch.bfloat16
    blocks = [Block(Attention(dim, heads, added_kv=True, dtype=dt), "attn"), Block(Attention(dim, heads, dtype=dt), "attn")]
    tr = Transformer(blocks[:1], "transformer_blocks")
    tr.single_transformer_blocks = torch.nn.ModuleList(blocks[1:])
    with torch.no_grad():
        for blk in blocks:
            for nm in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
                m = getattr(blk.attn, nm)
                if m is not None:
                    m.weight.copy_(1 + 0.2 * torch.randn(hd))
    tr.cuda()
    kw = dict(num_q_centroids=20, num_k_centroids=30, top_p_kmeans=0.9, kmeans_iter_init=3, kmeans_iter_step=2) if pattern == "SAP" else {}
    cls = replace_hyvideo_attention(Pipe(tr), 160, 320, 17, 21, first_layers_fp=0, first_times_fp=900.0,
                                    pattern="SVG" if pattern == "dense" else pattern, num_sampled_rows=32, sparsity=0.45, **kw)
    if pattern == "dense":
        for blk in blocks:
            blk.attn.set_processor(HunyuanVideoAttnProcessor2_0_FlashAttention(0))
    cls.sample_mse_max_row = cls.num_frame * cls.frame_size
    return blocks, cls, heads, hd


@pytest.mark.parametrize("pattern", ["dense", "SVG", "SAP"])
def test_processors_joint_prologue_against_staged_path(pattern, monkeypatch):
    from svg import _native as nat
    from svg.models import _core
    from svg.models.hyvideo.attention import _HunyuanProcessorBase

    blocks, cls, heads, hd = _install(pattern)
    ctx, V = cls.context_length, cls.num_frame * cls.frame_size
    dim = heads * hd
    gen = torch.Generator().manual_seed(11)
    base = (torch.randn(1, V + ctx, dim, generator=gen) * 0.3).to(torch.bfloat16).cuda()
    hidden, enc = base[:, :V], base[:, V:]
    amask = torch.zeros(1, V + ctx, dtype=torch.bool, device="cuda")
    amask[:, :V + 21] = True
    rope = _rope(V, hd)
    big = V * dim   # a cat at least this large copies q / k / v-sized data
    n_cat = {"n": 0}
    real_cat = torch.cat

    def counting_cat(ts, *a, **k):
        out = real_cat(ts, *a, **k)
        if out.numel() >= big:
            n_cat["n"] += 1
        return out

    def run(blk, h, e, joint, ts=torch.tensor([100.0])):
        captured = {}
        proc = blk.attn.processor
        core = type(proc).attention_core_logic

        def spy(self_, q, k, v, *a):
            captured["qkv"] = (q.clone(), k.clone(), v.clone())
            return core(self_, q, k, v, *a)

        monkeypatch.setattr(_HunyuanProcessorBase, "joint_prologue", joint)
        monkeypatch.setattr(type(proc), "attention_core_logic", spy)
        monkeypatch.setattr(torch, "cat", counting_cat)
        if pattern == "SAP":
            cls.reset_state()
        torch.manual_seed(7)
        _core.reseed_switch_generator(7)
        n_cat["n"] = 0
        with torch.no_grad():
            out = blk.attn(h, encoder_hidden_states=e, attention_mask=amask, image_rotary_emb=rope, timestep=ts)
        torch.cuda.synchronize()
        monkeypatch.setattr(torch, "cat", real_cat)
        monkeypatch.undo()
        return out, captured["qkv"], n_cat["n"]

    # double stream
    dbl = blocks[0]
    o_new, (q1, k1, v1), cats_new = run(dbl, hidden.contiguous(), enc.contiguous(), True)
    o_old, (q0, k0, v0), cats_old = run(dbl, hidden.contiguous(), enc.contiguous(), False)
    assert cats_new == 0 and cats_old == 3, (cats_new, cats_old)
    assert torch.equal(q1[:, :, :V], q0[:, :, :V]) and torch.equal(k1[:, :, :V], k0[:, :, :V]) and torch.equal(v1, v0)
    a = dbl.attn
    with torch.no_grad():
        tq, tk = (proj(enc).unflatten(2, (heads, -1)).transpose(1, 2).contiguous() for proj in (a.add_q_proj, a.add_k_proj))
        nq, nk = _core._norm_desc(a.norm_added_q, hd, tq.dtype, tq.device), _core._norm_desc(a.norm_added_k, hd, tq.dtype, tq.device)
        nat.qk_norm_rope(tq, tk, 1, nq[1], None, nk[1], None, nq[3])
        mod_q = a.norm_added_q(a.add_q_proj(enc).unflatten(2, (heads, -1)).transpose(1, 2))
    torch.cuda.synchronize()
    assert torch.equal(q1[:, :, V:], tq) and torch.equal(k1[:, :, V:], tk)
    # the text rows against the torch module (the staged path's arithmetic): at most one ulp apart; how often they differ
    diff = (q1[:, :, V:].float() != mod_q.float())
    ulp = ((q1[:, :, V:].view(torch.int16).int() - mod_q.contiguous().view(torch.int16).int()).abs().max().item())
    print(f"\n{pattern}: text q rows differing from the torch RMSNorm module: {diff.float().mean().item():.2%} (max {ulp} ulp)")
    assert ulp <= 1
    for x, y in zip(o_new, o_old):
        e = ((x.float() - y.float()).norm() / y.float().norm()).item()
        print(f"{pattern}: double-stream output rel. L2 joint vs staged {e:.2e}")
        assert e < 1e-3, e

    # single stream: adjacent slices -> no cat, same output; separate tensors -> the cat, same result
    sgl = blocks[1]
    o_j, _, cats_j = run(sgl, hidden, enc, True)
    o_s, _, cats_s = run(sgl, hidden, enc, False)
    o_sep, _, cats_sep = run(sgl, hidden.clone(), enc.clone(), True)
    assert cats_j == 0 and cats_s == 1 and cats_sep == 1, (cats_j, cats_s, cats_sep)
    for x, y, z in zip(o_j, o_s, o_sep):
        assert torch.equal(x, y) and torch.equal(x, z)
