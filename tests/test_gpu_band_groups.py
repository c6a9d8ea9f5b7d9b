"""Batches of prompts with different lengths (HunyuanVideo): svg_band_groups_attention and everything above it, on the GPU.

The smallest shape at which every row region of the Hunyuan mask exists and differs between the videos: F = 3 frames of P = 128 tokens
(V = 384), 128 text tokens (S = 512), band = 128, H = 2 heads, head_dim 128, three videos with prompt lengths (1, 37, 128) — 127 pad
rows; a real length off every 64-key tile edge; no pad rows at all.  Tolerances against the fp32 oracle are the project's
(tests/test_gpu_kernels.py: 3e-3 relative L2 for bf16, 1e-3 for fp16); equalities between launches are torch.equal."""
import copy

import pytest
import torch

from oracle import svg_oracle as O
from standins import Attention
from poisoned import poisoned_like

pytestmark = pytest.mark.gpu

F_, P_, CTX, H, BAND = 3, 128, 128, 2, 128
V = F_ * P_
S = V + CTX
LENS = (1, 37, 128)
TOL = {torch.bfloat16: 3e-3, torch.float16: 1e-3}
PERM = dict(vid0=0, num_frame=F_, frame_size=P_)


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def hy_mask(nat, p):
    return nat.BandMask(V + p, BAND, V, V + p, V, V + p)


def dense_mask(nat, p):
    return nat.BandMask(V + p, S + 1, 0, 0, 0, 0)


def rel_l2(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-20)).item()


_DATA = {}


def qkv(dt, D=128, cfg=len(LENS)):
    """the same q, k, v for every test of a (dtype, head_dim): [cfg, H, S, D] on the GPU, never written"""
    key = (dt, D, cfg)
    if key not in _DATA:
        gen = torch.Generator().manual_seed(7)
        _DATA[key] = tuple(torch.randn(cfg, H, S, D, generator=gen).to(dt).cuda() for _ in range(3))
    return _DATA[key]


_ORACLE = {}


def oracle(dt, kind, b):
    """fp32 masked attention of video b under its own mask, computed once per (dtype, mask family, video)"""
    key = (dt, kind, b)
    if key not in _ORACLE:
        q, k, v = (t[b].cpu() for t in qkv(dt))
        p = LENS[b]
        prm = (V + p, BAND, V, V + p, V, V + p) if kind == "sparse" else (V + p, S + 1, 0, 0, 0, 0)
        _ORACLE[key] = O.masked_attention(q, k, v, O.band_mask(S, *prm))
    return _ORACLE[key]


def heads_of(lens):
    from svg.models._core import video_groups

    return video_groups(lens, H)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the grouped call against the single-mask calls it stands for
# ---------------------------------------------------------------------------------------------------------------------------------
def _best(cfg):
    best = torch.tensor([[1, 0], [0, 1], [1, 1], [0, 0]])[:cfg]
    return best.cuda()


FORMS = ["plain", "strided", "prescaled", "switch0", "switch1", "switch1_strided", "switch0_prescaled", "perm", "perm_strided"]


@pytest.mark.parametrize("lens", [LENS, (37, 37, 128), (128, 1, 1)], ids=lambda x: "-".join(map(str, x)))
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_grouped_call_equals_single_mask_calls(nat, dt, form, lens):
    q, k, v = qkv(dt)
    cfg = len(lens)
    strided = form.endswith("strided")
    if strided:   # the projection layout: [cfg, S, H * D] in memory, read in place; the output comes back token-major
        q, k, v = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, k, v))
        assert not q.is_contiguous()
    best = _best(cfg) if form.startswith(("perm", "switch")) else None
    flag = torch.tensor([int(form[6])], dtype=torch.int32).cuda() if form.startswith("switch") else None
    pre = form.endswith("prescaled")
    vals, heads = heads_of(lens)
    assert len(vals) == len(set(lens)) and sum(heads) == cfg * H
    kw = dict(head_perm_flag=best, q_prescaled=pre, token_major_out=strided, **PERM)
    if flag is not None:
        got = nat.band_attention_groups(q, k, v, [hy_mask(nat, p) for p in vals], heads, alt_masks=[dense_mask(nat, p) for p in vals],
                                        use_alt_flag=flag, **kw)
    else:
        got = nat.band_attention_groups(q, k, v, [hy_mask(nat, p) for p in vals], heads, **kw)
    assert got.shape == q.shape
    if strided:
        assert got.stride() == (S * H * 128, 128, H * 128, 1)   # written in place, token-major: no copy on the way out
    for b, p in enumerate(lens):
        sl = slice(b, b + 1)
        kw1 = dict(kw, head_perm_flag=None if best is None else best[sl])
        if flag is not None:
            one = nat.band_attention_switch(q[sl], k[sl], v[sl], hy_mask(nat, p), dense_mask(nat, p), flag, **kw1)
        else:
            one = nat.band_attention(q[sl], k[sl], v[sl], hy_mask(nat, p), **kw1)
        assert torch.equal(got[sl], one), (form, b)


def test_grouped_call_at_head_dim_64(nat):
    q, k, v = qkv(torch.bfloat16, D=64)
    vals, heads = heads_of(LENS)
    best = _best(3)
    got = nat.band_attention_groups(q, k, v, [hy_mask(nat, p) for p in vals], heads, head_perm_flag=best, **PERM)
    for b, p in enumerate(LENS):
        one = nat.band_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], hy_mask(nat, p), head_perm_flag=best[b:b + 1], **PERM)
        assert torch.equal(got[b:b + 1], one), b


def test_one_group_is_the_single_mask_entry(nat):
    q, k, v = qkv(torch.bfloat16)
    m = hy_mask(nat, 37)
    assert torch.equal(nat.band_attention_groups(q, k, v, [m], [3 * H]), nat.band_attention(q, k, v, m))
    flag = torch.ones(1, dtype=torch.int32).cuda()
    assert torch.equal(nat.band_attention_groups(q, k, v, [m], [3 * H], alt_masks=[dense_mask(nat, 37)], use_alt_flag=flag),
                       nat.band_attention_switch(q, k, v, m, dense_mask(nat, 37), flag))


def test_grouped_call_into_out_and_from_views_it_cannot_take(nat):
    """`out=` (contiguous and not), and groups that are not whole videos of a strided view: copied, same values"""
    q, k, v = qkv(torch.bfloat16)
    vals, heads = heads_of(LENS)
    masks = [hy_mask(nat, p) for p in vals]
    want = nat.band_attention_groups(q, k, v, masks, heads)
    out = poisoned_like(q)
    assert nat.band_attention_groups(q, k, v, masks, heads, out=out) is out and torch.equal(out, want)
    out_tm = nat.token_major_empty(q)
    assert nat.band_attention_groups(q, k, v, masks, heads, out=out_tm) is out_tm and torch.equal(out_tm, want)
    qs, ks, vs = (t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, k, v))
    part = nat.band_attention_groups(qs, ks, vs, [masks[0], masks[0], masks[1], masks[2]], [1, 1, H, H])   # video 0 as two groups of one head
    assert torch.equal(part, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the grouped call against the fp32 oracle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sparse", "dense"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_grouped_call_against_oracle(nat, dt, kind):
    q, k, v = qkv(dt)
    vals, heads = heads_of(LENS)
    mk = hy_mask if kind == "sparse" else dense_mask
    got = nat.band_attention_groups(q, k, v, [mk(nat, p) for p in vals], heads).float().cpu()
    assert torch.isfinite(got).all()
    for b, p in enumerate(LENS):
        ref = oracle(dt, kind, b)
        err = rel_l2(got[b], ref)
        print(f"{kind} {dt} video {b} (prompt {p}): rel L2 {err:.3e}")
        assert err <= TOL[dt], (b, err)
        torch.testing.assert_close(got[b], ref, atol=1e-2, rtol=1e-2)
        real = V + p
        if real < S:   # pad rows attend only among themselves: few rows, an error there hides in an L2 over all rows
            err_pad = rel_l2(got[b][:, real:], ref[:, real:])
            print(f"    pad rows [{real}, {S}): rel L2 {err_pad:.3e}")
            assert err_pad <= TOL[dt], (b, "pad rows", err_pad)
            # ... and they read no real key: the oracle of the pad block alone
            q_, k_, v_ = (t[b, :, real:].cpu() for t in (q, k, v))
            assert rel_l2(got[b][:, real:], O.masked_attention(q_, k_, v_, None)) <= TOL[dt]


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. _core with sequences against the same functions called per video with scalars
# ---------------------------------------------------------------------------------------------------------------------------------
def _geo_prof():
    from svg.models import _core
    from svg.models.hyvideo.utils import profile_desc

    return _core.Geometry(CTX, F_, P_), profile_desc(CTX, F_, P_)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_core_dense_attention_per_video(dt):
    from svg.models import _core

    q, k, v = qkv(dt)
    got = _core.dense_attention(q, k, v, [V + p for p in LENS])
    for b, p in enumerate(LENS):
        assert torch.equal(got[b:b + 1], _core.dense_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], V + p)), b
        assert rel_l2(got[b].cpu(), oracle(dt, "dense", b)) <= TOL[dt]
    with pytest.raises(ValueError):
        _core.dense_attention(q, k, v, [V + 1, V + 37])


def test_equal_lengths_take_the_parent_path():
    from svg.models import _core

    q, k, v = qkv(torch.bfloat16)
    geo, prof = _geo_prof()
    n = V + 37
    assert torch.equal(_core.dense_attention(q[:2], k[:2], v[:2], [n, n]), _core.dense_attention(q[:2], k[:2], v[:2], n))
    assert torch.equal(_core.dense_attention(q, k, v, (n, n, n)), _core.dense_attention(q, k, v, n))
    from svg import _native

    m = hy_mask(_native, 37)
    outs = []
    for mask in ([m, hy_mask(_native, 37), m], m):
        torch.manual_seed(0)
        outs.append(_core.svg1_sparse_attention(q, k, v, geo, mask, prof, 16, V))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("fused", [True, False])
def test_core_svg1_sparse_attention_per_video(nat, fused):
    from svg.models import _core

    q, k, v = qkv(torch.bfloat16)
    geo, prof = _geo_prof()
    torch.manual_seed(0)
    got, best = _core.svg1_sparse_attention(q, k, v, geo, [hy_mask(nat, p) for p in LENS], prof, 16, V, fused=fused)
    assert best.shape == (3, H)
    for b, p in enumerate(LENS):
        torch.manual_seed(0)
        one, best1 = _core.svg1_sparse_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], geo, hy_mask(nat, p), prof, 16, V, fused=fused)
        assert torch.equal(best[b:b + 1], best1), b
        assert torch.equal(got[b:b + 1], one), b
        ref = oracle(torch.bfloat16, "sparse", b)   # heads the profiler left frame-major are the plain masked attention
        for h in range(H):
            if int(best[b, h]) == 0:
                assert rel_l2(got[b, h].cpu(), ref[h]) <= TOL[torch.bfloat16]


@pytest.mark.parametrize("dense_step", [0, 1])
def test_core_svg1_device_switch_per_video(nat, dense_step):
    from svg.models import _core

    q, k, v = qkv(torch.bfloat16)
    geo, prof = _geo_prof()
    flag = torch.tensor([dense_step], dtype=torch.int32).cuda()

    def run(sl, masks, dense):
        torch.manual_seed(0)
        _core.reseed_switch_generator()
        return _core.svg1_attention_device_switch(q[sl], k[sl], v[sl], geo, masks, dense, prof, 16, V, flag)

    got, best = run(slice(0, 3), [hy_mask(nat, p) for p in LENS], [dense_mask(nat, p) for p in LENS])
    assert bool((best == -1).all()) == bool(dense_step)
    for b, p in enumerate(LENS):
        one, best1 = run(slice(b, b + 1), hy_mask(nat, p), dense_mask(nat, p))
        assert torch.equal(best[b:b + 1], best1), b
        assert torch.equal(got[b:b + 1], one), b
        if dense_step:
            assert rel_l2(got[b].cpu(), oracle(torch.bfloat16, "dense", b)) <= TOL[torch.bfloat16]
    # one of the two given per video, the other for the batch
    got2, _ = run(slice(0, 3), [hy_mask(nat, p) for p in LENS], dense_mask(nat, 37))
    one2, _ = run(slice(0, 1), hy_mask(nat, LENS[0]), dense_mask(nat, 37))
    assert torch.equal(got2[:1], one2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. SVG2: per-video text pseudo-clusters, one launch
# ---------------------------------------------------------------------------------------------------------------------------------
QC, KC = 8, 16


def _clustered(cfg, modes, gen):
    centres = torch.randn(cfg * H, modes, 128, generator=gen) * 2.0
    pick = torch.randint(0, modes, (cfg * H, S), generator=gen)
    x = torch.gather(centres, 1, pick[..., None].expand(-1, -1, 128)) + 0.4 * torch.randn(cfg * H, S, 128, generator=gen)
    return x.reshape(cfg, H, S, 128)


def _seeded_store(q, k, cfg):
    from svg.models import _core

    st = _core.CentroidStore()
    st.put(0, q[:, :, :V][:, :, ::7][:, :, :QC].reshape(cfg * H, QC, 128).contiguous(),
           k[:, :, :V][:, :, ::5][:, :, :KC].reshape(cfg * H, KC, 128).contiguous(), cfg)
    return st


def _video_store(st, c):
    from svg.models import _core

    one = _core.CentroidStore()
    one.put(0, st.q[0][c * H:(c + 1) * H].contiguous(), st.k[0][c * H:(c + 1) * H].contiguous(), 1)
    return one


@pytest.mark.parametrize("token_major", [True, False])
def test_svg2_per_video_prompt_lengths_equal_cfg1_calls(token_major):
    from svg.models import _core

    gen = torch.Generator().manual_seed(13)
    cfg = 3
    q = _clustered(cfg, 6, gen).to(torch.bfloat16).cuda()
    k = _clustered(cfg, 9, gen).to(torch.bfloat16).cuda()
    v = torch.randn(cfg, H, S, 128, generator=gen).to(torch.bfloat16).cuda()
    geo = _core.Geometry(CTX, F_, P_)
    old = _core.TOKEN_MAJOR_IO
    _core.TOKEN_MAJOR_IO = token_major
    try:
        st_b = _seeded_store(q, k, cfg)
        singles = [_video_store(st_b, c) for c in range(cfg)]
        o_b = _core.svg2_sparse_attention(q, k, v, geo, st_b, 0, QC, KC, 0.6, 0.1, 5, 3, prompt_length=LENS)
        assert o_b.shape == (cfg, H, S, 128) and torch.isfinite(o_b.float()).all()
        for c, p in enumerate(LENS):
            o_1 = _core.svg2_sparse_attention(q[c:c + 1].contiguous(), k[c:c + 1].contiguous(), v[c:c + 1], geo, singles[c], 0, QC, KC, 0.6,
                                              0.1, 5, 3, prompt_length=p)
            assert torch.equal(o_b[c], o_1[0]), c
        # the lengths matter: video 0 under video 2's length is another result
        o_x = _core.svg2_sparse_attention(q[:1].contiguous(), k[:1].contiguous(), v[:1], geo, _video_store(_seeded_store(q, k, cfg), 0), 0, QC, KC,
                                          0.6, 0.1, 5, 3, prompt_length=LENS[2])
        assert not torch.equal(o_b[0], o_x[0])
        # equal lengths given per video: the scalar path
        a = _core.svg2_sparse_attention(q, k, v, geo, _seeded_store(q, k, cfg), 0, QC, KC, 0.6, 0.1, 5, 3, prompt_length=[37, 37, 37])
        b = _core.svg2_sparse_attention(q, k, v, geo, _seeded_store(q, k, cfg), 0, QC, KC, 0.6, 0.1, 5, 3, prompt_length=37)
        assert torch.equal(a, b)
    finally:
        _core.TOKEN_MAJOR_IO = old


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. the three processors on a batch of two prompts: B = 2, lengths (37, 128), a [2, 1, 1, S] mask.  On the parent commit the dense and
#    SVG1 calls raise (valid = the sum over both rows exceeds S) and the SAP call raises on int(tuple).
# ---------------------------------------------------------------------------------------------------------------------------------
PLENS = (37, 128)
DT = torch.bfloat16


class _PerVideoLinear(torch.nn.Module):
    """a Linear applied video by video: GEMMs are not bit-stable across batch sizes, and these tests compare B = 2 with B = 1 bit for bit"""

    def __init__(self, lin):
        super().__init__()
        self.lin = lin

    def forward(self, x):
        return torch.cat([self.lin(x[i:i + 1]) for i in range(x.shape[0])])


def _per_video(attn):
    for name in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_add_out"):
        m = getattr(attn, name, None)
        if isinstance(m, torch.nn.Linear):
            setattr(attn, name, _PerVideoLinear(m))
    attn.to_out[0] = _PerVideoLinear(attn.to_out[0])
    return attn


class _Setup:
    def __init__(self, added_kv=True):
        torch.manual_seed(0)
        dim = H * 128
        self.attn = _per_video(Attention(dim, H, added_kv=added_kv, dtype=DT).cuda())
        self.hidden = (torch.randn(2, V, dim) * 0.3).to(DT).cuda()
        self.enc = (torch.randn(2, CTX, dim) * 0.3).to(DT).cuda()
        ang = torch.rand(V, 128) * 6.28
        self.rope = (ang.cos().cuda(), ang.sin().cuda())
        m = torch.zeros(2, 1, 1, S, dtype=torch.bool)
        for b, p in enumerate(PLENS):
            m[b, ..., :V + p] = True
        self.mask = m.cuda()
        self.rows = [m[b:b + 1].clone().cuda() for b in range(2)]

    def call(self, sl, t, mask="rows", on_gpu=False):
        ts = torch.tensor([t]).cuda() if on_gpu else torch.tensor([t])
        am = None if mask is None else (self.mask if sl == slice(0, 2) else self.rows[sl.start])
        with torch.no_grad():
            h, e = self.attn(self.hidden[sl], encoder_hidden_states=self.enc[sl], attention_mask=am, image_rotary_emb=self.rope, timestep=ts)
        return torch.cat([h, e], dim=1)


ALL = slice(0, 2)


def _class_state(cls, names):
    """what the class itself defines of `names` (the SAP processor inherits most of them): _restore puts exactly that back"""
    return {n: (n in cls.__dict__, cls.__dict__.get(n)) for n in names}


def _restore(cls, saved):
    for n, (own, x) in saved.items():
        if own:
            setattr(cls, n, x)
        elif n in cls.__dict__:
            delattr(cls, n)


def _configure(cls, nat, lens):
    """class-level configuration as replace_hyvideo_attention leaves it (whose geometry is fixed at 256 text tokens), at this file's shape"""
    from svg.models.hyvideo.utils import generate_temporal_head_mask_mod

    cls.context_length, cls.num_frame, cls.frame_size = CTX, F_, P_
    cls.first_layers_fp, cls.first_times_fp = 0, 900.0
    cls.num_sampled_rows, cls.sample_mse_max_row = 16, V
    masks = tuple(generate_temporal_head_mask_mod(CTX, p, F_, P_, mul=1) for p in (lens if isinstance(lens, tuple) else (lens,)))
    assert masks[0].as_tuple() == hy_mask(nat, lens[0] if isinstance(lens, tuple) else lens).as_tuple()
    cls.prompt_length = lens
    cls.block_mask = masks if isinstance(lens, tuple) else masks[0]


@pytest.mark.parametrize("added_kv", [True, False], ids=["double_stream", "single_stream"])
def test_dense_processor_on_a_batch_of_prompts(added_kv):
    from svg.models.hyvideo.attention import HunyuanVideoAttnProcessor2_0_FlashAttention as P

    su = _Setup(added_kv)
    su.attn.set_processor(P(0))
    got = su.call(ALL, 950.0)
    assert torch.isfinite(got.float()).all()
    cpu = copy.deepcopy(su.attn).float().cpu()   # the same processor on CPU tensors is plain torch: two SDPA calls per video
    for b in range(2):
        assert torch.equal(got[b:b + 1], su.call(slice(b, b + 1), 950.0)), b
        with torch.no_grad():
            h, e = cpu(su.hidden[b:b + 1].float().cpu(), encoder_hidden_states=su.enc[b:b + 1].float().cpu(), attention_mask=su.rows[b].cpu(),
                       image_rotary_emb=tuple(t.cpu() for t in su.rope), timestep=torch.tensor([950.0]))
        torch.testing.assert_close(got[b:b + 1].float().cpu(), torch.cat([h, e], dim=1), atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("device_switch", [True, False])
def test_svg_processor_on_a_batch_of_prompts(nat, device_switch):
    from svg.models import _core
    from svg.models.hyvideo.attention import Hunyuan_SVGAttn_Processor2_0 as P

    names = ("context_length", "num_frame", "frame_size", "first_layers_fp", "first_times_fp", "num_sampled_rows", "sample_mse_max_row",
             "prompt_length", "block_mask", "device_switch")
    saved = _class_state(P, names)
    try:
        P.device_switch = device_switch
        su = _Setup()
        proc = P(0)
        su.attn.set_processor(proc)

        def run(sl, t, lens, mask):
            _configure(P, nat, lens)
            torch.manual_seed(0)
            _core.reseed_switch_generator()
            out = su.call(sl, t, mask=mask, on_gpu=device_switch)
            return out, proc.last_best_mask_idx

        for t in (100.0, 950.0):          # a sparse step and a dense warm-up step
            for mask in ("rows", None):   # valid from the mask rows, else from V + prompt_length[b]
                got, best = run(ALL, t, PLENS, mask)
                assert torch.isfinite(got.float()).all()
                for b, p in enumerate(PLENS):
                    one, best1 = run(slice(b, b + 1), t, p, mask)
                    assert torch.equal(got[b:b + 1], one), (t, mask, b)
                    if best is not None and (t < 900.0 or device_switch):
                        assert torch.equal(best[b:b + 1], best1), (t, mask, b)
        _configure(P, nat, (37, 128, 1))   # three lengths, two videos
        with pytest.raises(ValueError):
            su.call(ALL, 100.0, on_gpu=device_switch)
    finally:
        _restore(P, saved)


def test_sap_processor_on_a_batch_of_prompts(nat):
    from svg.models import _core
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0 as P

    names = ("context_length", "num_frame", "frame_size", "first_layers_fp", "first_times_fp", "num_sampled_rows", "sample_mse_max_row",
             "prompt_length", "block_mask", "num_q_centroids", "num_k_centroids", "top_p_kmeans", "min_kc_ratio", "kmeans_iter_init",
             "kmeans_iter_step", "zero_step_kmeans_init")
    saved = _class_state(P, names)
    try:
        P.num_q_centroids, P.num_k_centroids, P.top_p_kmeans, P.min_kc_ratio = QC, KC, 0.6, 0.1
        P.kmeans_iter_init, P.kmeans_iter_step, P.zero_step_kmeans_init = 5, 2, True
        su = _Setup()
        proc = P(0)
        su.attn.set_processor(proc)

        def run(sl, t, lens, store, mask="rows"):
            _configure(P, nat, lens)
            proc.centroid_store = store   # (shadows the class-level store: a processor state of its own per run)
            torch.manual_seed(3)
            torch.cuda.manual_seed(3)
            return su.call(sl, t, mask=mask)

        # the dense warm-up branch with the k-means initialisation (zero_step_kmeans_init)
        st_b = _core.CentroidStore()
        for mask in ("rows", None):
            d_b = run(ALL, 950.0, PLENS, st_b, mask)
            for b, p in enumerate(PLENS):
                assert torch.equal(d_b[b:b + 1], run(slice(b, b + 1), 950.0, p, _core.CentroidStore(), mask)), ("dense", b)
        assert st_b.cfg[0] == 2
        # a sparse step warm-started from the batch's centroids: each video against a cfg = 1 state holding its slice of them
        singles = []
        for b in range(2):
            one = _core.CentroidStore()
            one.put(0, st_b.q[0][b * H:(b + 1) * H].clone(), st_b.k[0][b * H:(b + 1) * H].clone(), 1)
            singles.append(one)
        s_b = run(ALL, 100.0, PLENS, st_b)
        assert torch.isfinite(s_b.float()).all()
        for b, p in enumerate(PLENS):
            assert torch.equal(s_b[b:b + 1], run(slice(b, b + 1), 100.0, p, singles[b])), ("sparse", b)
        _configure(P, nat, (37, 128, 1))
        with pytest.raises(ValueError):
            su.call(ALL, 100.0)
    finally:
        _restore(P, saved)
        if "centroid_store" in proc.__dict__:
            del proc.centroid_store
        P.reset_state()
