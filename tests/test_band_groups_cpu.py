"""Batches of prompts with different lengths (HunyuanVideo), the host side: the validation of svg_band_groups_attention, the grouping
of videos, the per-row valid lengths of a batched text mask, and the per-video forms of the CPU-capable functions."""
import pytest
import torch

from band_groups_cases import GROUP_CASES, PH
from oracle import svg_oracle as O
from standins import Attention, Block, Pipe, Transformer
from svg import _native as nat


# ---- 1. entry validation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call,expected", [c[1:] for c in GROUP_CASES], ids=[c[0] for c in GROUP_CASES])
def test_groups_entry_rejects(call, expected):
    name, args = call
    if any(a == PH for a in args) and torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert getattr(nat.load(), name)(*args) == expected


def test_groups_rows_cover_the_checks_of_the_header():
    ids = {c[0] for c in GROUP_CASES}
    for want in ("groups/bad_mask_last", "groups/n_groups0", "groups/group_heads0", "groups/sum_lt_BH", "groups/alt_without_flag",
                 "groups/flag_without_alt", "groups/layout_part_of_a_video", "groups/prescaled_with_layout", "groups/D96"):
        assert want in ids
    assert nat.SVG_ABI_VERSION == 4 and nat.load().svg_abi_version() == 4   # a new entry point does not bump the ABI version


# ---- 2. video_groups, and what _core hands the grouped call -----------------------------------------------------------------------------
def test_video_groups_merges_equal_neighbours_only():
    from svg.models._core import video_groups

    a, b = 5, 9
    assert video_groups((a, a, b, a)) == ([a, b, a], [2, 1, 1])
    assert video_groups((a, a, b, a), heads=24) == ([a, b, a], [48, 24, 24])
    assert video_groups((a, a, a), heads=3) == ([a], [9])
    assert video_groups((a,)) == ([a], [1])
    m = lambda r: nat.BandMask(r, 128, 0, 0, 0, 0)   # noqa: E731 — masks compare by value, not by identity
    vals, heads = video_groups((m(7), m(7), m(8), m(7)), heads=2)
    assert [x.real_len for x in vals] == [7, 8, 7] and heads == [4, 2, 2]
    vals, heads = video_groups(((m(7), m(1)), (m(7), m(2)), (m(7), m(2))), heads=2)   # pairs (mask, dense mask)
    assert [(x.real_len, y.real_len) for x, y in vals] == [(7, 1), (7, 2)] and heads == [2, 4]


class _Cuda:
    """a tensor stand-in that says it lives on the GPU: enough for _core to take its GPU branch up to the (patched) native call"""

    is_cuda = True

    def __init__(self, shape):
        self.shape = shape


def test_core_passes_exactly_the_groups(monkeypatch):
    from svg.models import _core

    calls = []

    def fake_groups(q, k, v, masks, group_heads, **kw):
        calls.append(([m.as_tuple() for m in masks], list(group_heads), kw))
        return "grouped"

    def fake_single(q, k, v, mask, **kw):
        calls.append((mask.as_tuple(), None, kw))
        return "single"

    monkeypatch.setattr(_core._native, "band_attention_groups", fake_groups)
    monkeypatch.setattr(_core._native, "band_attention", fake_single)
    S, H = 512, 3
    q = _Cuda((4, H, S, 128))
    assert _core.dense_attention(q, q, q, (400, 400, 421, 400)) == "grouped"
    masks, heads, kw = calls.pop()
    assert masks == [(400, S + 1, 0, 0, 0, 0), (421, S + 1, 0, 0, 0, 0), (400, S + 1, 0, 0, 0, 0)] and heads == [2 * H, H, H]
    assert kw["q_prescaled"] is False
    # equal lengths: ONE group, today's entry point with today's arguments
    assert _core.dense_attention(q, q, q, [400] * 4) == "single"
    by_list = calls.pop()
    assert _core.dense_attention(q, q, q, 400) == "single"
    assert by_list == calls.pop() and by_list[0] == (400, S + 1, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="4 videos"):
        _core.dense_attention(q, q, q, (400, 421))
    assert not calls


def test_differing_lengths_refuse_head_sharding(monkeypatch):
    from svg.models import _core

    monkeypatch.setattr(_core._dist, "active", lambda: True)
    monkeypatch.setattr(_core, "_require_gpu", lambda *a: None)
    q = _Cuda((2, 2, 512, 128))
    geo = _core.Geometry(128, 3, 128)
    m = [nat.BandMask(385, 128, 384, 385, 384, 385), nat.BandMask(421, 128, 384, 421, 384, 421)]
    with pytest.raises(NotImplementedError, match="head sharding"):
        _core.svg1_sparse_attention(q, q, q, geo, m, None, 8, 384)
    with pytest.raises(NotImplementedError, match="head sharding"):
        _core.svg1_attention_device_switch(q, q, q, geo, m, m[0], None, 8, 384, None)
    with pytest.raises(NotImplementedError, match="head sharding"):
        _core.svg2_sparse_attention(q, q, q, geo, _core.CentroidStore(), 0, 8, 16, 0.9, 0.1, 2, 1, prompt_length=(1, 37))


# ---- 3. get_cu_max_seqlen ---------------------------------------------------------------------------------------------------------------
def _mask(lens, S, shape4):
    m = torch.zeros(len(lens), S, dtype=torch.bool)
    for b, n in enumerate(lens):
        m[b, :n] = True
    return m[:, None, None, :].contiguous() if shape4 else m


@pytest.mark.parametrize("shape4", [False, True])
def test_get_cu_max_seqlen_per_row(shape4, monkeypatch):
    from svg.models.hyvideo import attention as A

    proc = A.HunyuanVideoAttnProcessor2_0_FlashAttention(0)
    reads = []
    real = A._row_sums
    monkeypatch.setattr(A, "_row_sums", lambda rows: (reads.append(1), real(rows))[1])
    S = 512
    m = _mask((385, 421, 512), S, shape4)
    assert proc.get_cu_max_seqlen(m, "cpu") == ((385, 421, 512), S)
    for _ in range(3):   # every layer of a forward hands over the same object: one read-back
        assert A.Hunyuan_SVGAttn_Processor2_0(1).get_cu_max_seqlen(m, "cpu") == ((385, 421, 512), S)
    assert len(reads) == 1
    m[1, ..., 421:430] = True   # an in-place edit: a new value
    assert proc.get_cu_max_seqlen(m, "cpu") == ((385, 430, 512), S)
    assert len(reads) == 2
    assert proc.get_cu_max_seqlen(None, "cpu") == (None, None)


@pytest.mark.parametrize("shape", [(1, 512), (1, 1, 1, 512), (512,)])
def test_get_cu_max_seqlen_one_row_is_unchanged(shape, monkeypatch):
    from svg.models.hyvideo import attention as A

    monkeypatch.setattr(A, "_row_sums", lambda rows: pytest.fail("a one-row mask takes the scalar read-back"))
    m = torch.zeros(512, dtype=torch.bool)
    m[:421] = True
    m = m.reshape(shape)
    out = A.HunyuanVideoAttnProcessor2_0_FlashAttention(0).get_cu_max_seqlen(m, "cpu")
    assert out == (421, 512) and isinstance(out[0], int)


# ---- 4. CPU-capable per-video forms -----------------------------------------------------------------------------------------------------
def test_dense_attention_on_cpu_tensors_per_video():
    from svg.models import _core

    torch.manual_seed(0)
    q, k, v = (torch.randn(3, 2, 96, 32) for _ in range(3))
    lens = (65, 80, 96)
    out = _core.dense_attention(q, k, v, lens)
    for b, n in enumerate(lens):
        assert torch.equal(out[b:b + 1], _core.dense_attention(q[b:b + 1], k[b:b + 1], v[b:b + 1], n))
        ref = O.masked_attention(q[b], k[b], v[b], O.band_mask(96, n, 97, 0, 0, 0, 0))
        torch.testing.assert_close(out[b], ref, atol=1e-5, rtol=1e-5)
    assert torch.equal(_core.dense_attention(q, k, v, [80, 80, 80]), _core.dense_attention(q, k, v, 80))


def test_dynamic_map_post_processing_per_video_against_oracle():
    from svg.models._core import dynamic_map_post_processing

    gen = torch.Generator().manual_seed(1)
    cfg, H, QC, KC, V, ctx = 3, 2, 5, 7, 60, 16
    lens = (1, 6, 16)
    dmap = torch.rand(cfg, H, QC, KC, generator=gen) > 0.5
    qs = torch.randint(1, 20, (cfg, H, QC), generator=gen, dtype=torch.int32)
    ks = torch.randint(1, 20, (cfg, H, KC), generator=gen, dtype=torch.int32)
    qi = torch.stack([torch.randperm(V, generator=gen) for _ in range(cfg * H)]).to(torch.int32)
    ki = torch.stack([torch.randperm(V, generator=gen) for _ in range(cfg * H)]).to(torch.int32)
    m, sq, sk, iq, ik = dynamic_map_post_processing(dmap, qs, ks, qi, ki, V, ctx, lens)
    assert sq.dtype == qs.dtype and sk.dtype == ks.dtype
    for c, L in enumerate(lens):
        hs = slice(c * H, (c + 1) * H)
        rm, rq, rk, ri = O.dynamic_map_post_processing(dmap[c:c + 1], qs[c:c + 1], ks[c:c + 1], qi[hs].long(), V, ctx, L)
        assert torch.equal(m[c:c + 1], rm) and torch.equal(sq[c:c + 1], rq) and torch.equal(sk[c:c + 1], rk)
        assert torch.equal(iq[hs].long(), ri)
        assert sq[c, :, -2:].tolist() == [[L, ctx - L]] * H and sk[c, :, -2:].tolist() == [[L, ctx - L]] * H
    same = dynamic_map_post_processing(dmap, qs, ks, qi, ki, V, ctx, [6] * cfg)
    for a, b in zip(same, dynamic_map_post_processing(dmap, qs, ks, qi, ki, V, ctx, 6)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="3 videos"):
        dynamic_map_post_processing(dmap, qs, ks, qi, ki, V, ctx, (1, 6))


# ---- 5. install hook and processors -----------------------------------------------------------------------------------------------------
def _pipe(heads=2, hd=32):
    dim = heads * hd
    blocks = [Block(Attention(dim, heads, added_kv=True), "attn"), Block(Attention(dim, heads), "attn")]
    tr = Transformer(blocks[:1], "transformer_blocks")
    tr.single_transformer_blocks = torch.nn.ModuleList(blocks[1:])
    return Pipe(tr), blocks


def test_replace_hyvideo_attention_with_a_sequence():
    from svg.models.hyvideo import attention as A
    from svg.models.hyvideo.inference import replace_hyvideo_attention
    from svg.models.hyvideo.utils import generate_temporal_head_mask_mod, sparsity_to_width

    saved = {c: (c.prompt_length, c.block_mask) for c in (A.Hunyuan_SVGAttn_Processor2_0, A.Hunyuan_SAPAttn_Processor2_0)}
    try:
        pipe, _ = _pipe()
        cls = replace_hyvideo_attention(pipe, 160, 320, 17, [21, 40], 0, 900.0, pattern="SVG", num_sampled_rows=8, sparsity=0.45)
        assert cls.prompt_length == (21, 40) and isinstance(cls.block_mask, tuple) and len(cls.block_mask) == 2
        w = sparsity_to_width(0.45, 256, 5, 200)
        assert [m.as_tuple() for m in cls.block_mask] == [generate_temporal_head_mask_mod(256, p, 5, 200, w).as_tuple() for p in (21, 40)]
        cls = replace_hyvideo_attention(pipe, 160, 320, 17, torch.tensor([21, 40]), 0, 900.0, pattern="SVG", num_sampled_rows=8, sparsity=0.45)
        assert cls.prompt_length == (21, 40)
        cls = replace_hyvideo_attention(pipe, 160, 320, 17, (21, 40, 256), 0, 900.0, pattern="SAP", num_q_centroids=4, num_k_centroids=8,
                                        top_p_kmeans=0.9)
        assert cls is A.Hunyuan_SAPAttn_Processor2_0 and cls.prompt_length == (21, 40, 256)
        # an int leaves every attribute what it is today
        cls = replace_hyvideo_attention(pipe, 160, 320, 17, torch.tensor(21), 0, 900.0, pattern="SVG", num_sampled_rows=8, sparsity=0.45)
        assert cls.prompt_length == 21 and isinstance(cls.prompt_length, int) and isinstance(cls.block_mask, nat.BandMask)
        assert cls.block_mask.as_tuple() == generate_temporal_head_mask_mod(256, 21, 5, 200, w).as_tuple()
    finally:
        for c, (pl, bm) in saved.items():
            c.prompt_length, c.block_mask = pl, bm


@pytest.mark.parametrize("pattern", ["SVG", "SAP"])
def test_a_tuple_of_the_wrong_length_raises_at_call_time(pattern):
    """three lengths, a batch of two videos: ValueError from the processor before anything runs (CPU tensors; dense and sparse step)"""
    from svg.models.hyvideo import attention as A
    from svg.models.hyvideo.inference import replace_hyvideo_attention

    saved = {c: (c.prompt_length, c.block_mask, c.context_length, c.num_frame, c.frame_size, c.first_times_fp)
             for c in (A.Hunyuan_SVGAttn_Processor2_0, A.Hunyuan_SAPAttn_Processor2_0)}
    try:
        pipe, blocks = _pipe()
        kw = dict(num_sampled_rows=8, sparsity=0.45) if pattern == "SVG" else dict(num_q_centroids=4, num_k_centroids=8, top_p_kmeans=0.9)
        cls = replace_hyvideo_attention(pipe, 16, 32, 5, (3, 9, 11), 0, 900.0, pattern=pattern, **kw)
        assert (cls.context_length, cls.num_frame, cls.frame_size) == (256, 2, 2)
        V, dim = 4, 64
        hidden, enc = torch.randn(2, V, dim), torch.randn(2, 256, dim)
        for t in (950.0, 100.0):
            with pytest.raises(ValueError, match="3 entries for a batch of 2 videos"):
                blocks[0].attn(hidden, encoder_hidden_states=enc, attention_mask=None, image_rotary_emb=None, timestep=torch.tensor([t]))
        # the right count, on the dense step (CPU tensors): every video its own two segments, as its own call gives
        cls.prompt_length = (3, 9)
        with torch.no_grad():
            h, e = blocks[0].attn(hidden, encoder_hidden_states=enc, attention_mask=None, image_rotary_emb=None, timestep=torch.tensor([950.0]))
            for b, p in enumerate((3, 9)):
                cls.prompt_length = p
                h1, e1 = blocks[0].attn(hidden[b:b + 1], encoder_hidden_states=enc[b:b + 1], attention_mask=None, image_rotary_emb=None,
                                        timestep=torch.tensor([950.0]))
                torch.testing.assert_close(h[b:b + 1], h1, atol=1e-5, rtol=1e-5)
                torch.testing.assert_close(e[b:b + 1], e1, atol=1e-5, rtol=1e-5)
                cls.prompt_length = (3, 9)
        # a mask with another number of rows than the batch has videos
        with pytest.raises(ValueError, match="3 entries for a batch of 2 videos"):
            blocks[0].attn(hidden, encoder_hidden_states=enc, attention_mask=_mask((10, 20, 30), V + 256, True), image_rotary_emb=None,
                           timestep=torch.tensor([950.0]))
    finally:
        for c, vals in saved.items():
            c.prompt_length, c.block_mask, c.context_length, c.num_frame, c.frame_size, c.first_times_fp = vals


# ---- 6. get_prompt_lengths --------------------------------------------------------------------------------------------------------------
class _Tok:
    """one token per word behind a template prefix of `crop` tokens; padding to max_length, attention mask 1 on real tokens"""

    crop = 4

    def __call__(self, prompts, max_length=None, **kw):
        class _Out:
            pass

        rows = []
        for p in prompts:
            n = min(self.crop + len(p.split("|", 1)[1].split()), max_length)
            rows.append([1] * n + [0] * (max_length - n))
        out = _Out()
        out.attention_mask = torch.tensor(rows)
        return out


def test_get_prompt_lengths_with_a_fake_tokenizer():
    from svg.models.hyvideo.utils import get_prompt_length, get_prompt_lengths

    class _P:
        tokenizer = _Tok()

    tmpl = {"template": "system text |{}", "crop_start": _Tok.crop}
    prompts = ["a cat", "a dog runs over the green hill", "x " * 40]
    assert get_prompt_lengths(_P(), prompts, prompt_template=tmpl, max_sequence_length=32, device="cpu") == [2, 7, 32]
    assert get_prompt_lengths(_P(), "a cat", prompt_template=tmpl, max_sequence_length=32, device="cpu") == [2]
    # get_prompt_length stays the reference's: the sum over the list, a 0-dim tensor
    total = get_prompt_length(_P(), prompts, prompt_template=tmpl, max_sequence_length=32, device="cpu")
    assert torch.is_tensor(total) and total.dim() == 0 and int(total) == 41
    with pytest.raises(RuntimeError, match="prompt_template"):
        get_prompt_lengths(_P(), prompts, prompt_template=None)
