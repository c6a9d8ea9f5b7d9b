"""The Cosmos processors' fused prologue (`fused_prologue = True`: transpose + per-head QK norm + half-split RoPE as one
svg_qk_norm_rope_transpose pass with rope_kind 3, v read in place; the cross call: one norm-only transpose pass per tensor) against the
staged steps (`fused_prologue = False`: three contiguous transposes, the in-place HIP norm, apply_rotary_emb_half in torch), which are
the reference's sequence.  The two are the same arithmetic with the same rounding points: every comparison is torch.equal."""
import inspect

import pytest
import torch
import torch.nn as nn

from standins import Attention

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu
DT = torch.bfloat16
HEADS, HD, F_, P_ = 2, 128, 5, 160
DIM, S, N_TXT = HEADS * HD, F_ * P_, 77
_KEYS = ("context_length", "num_frame", "frame_size", "first_layers_fp", "first_times_fp", "num_sampled_rows", "sample_mse_max_row",
         "block_mask", "num_q_centroids", "num_k_centroids", "top_p_kmeans", "min_kc_ratio", "kmeans_iter_init", "kmeans_iter_step",
         "zero_step_kmeans_init")


@pytest.fixture
def procs():
    """the two processor classes configured for F = 5 frames of P = 160 tokens, no text; their class-level configuration is put back"""
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor as SapP, Cosmos_SVG_AttnProcessor2_0 as SvgP
    from svg.models.cosmos.utils import generate_temporal_head_mask_mod as mm

    saved = {c: {n: c.__dict__[n] for n in _KEYS if n in c.__dict__} for c in (SvgP, SapP)}
    for c in (SvgP, SapP):
        c.context_length, c.num_frame, c.frame_size = 0, F_, P_
        c.first_layers_fp, c.first_times_fp, c.num_sampled_rows, c.sample_mse_max_row = 0, 900.0, 16, 400
    SvgP.block_mask = mm(0, 0, F_, P_, mul=1.2)
    SapP.num_q_centroids, SapP.num_k_centroids, SapP.top_p_kmeans, SapP.min_kc_ratio = 8, 16, 0.6, 0.1
    SapP.kmeans_iter_init, SapP.kmeans_iter_step, SapP.zero_step_kmeans_init = 5, 2, False
    yield SvgP, SapP
    for c, vals in saved.items():
        for n in _KEYS:
            if n in vals:
                setattr(c, n, vals[n])
            elif n in c.__dict__:
                delattr(c, n)


@pytest.fixture(scope="module")
def data():
    torch.manual_seed(4)
    attn = Attention(DIM, HEADS, qk_norm="rms", dtype=DT)      # per-head RMSNorm(128)
    with torch.no_grad():
        attn.norm_q.weight.copy_(1 + 0.1 * torch.randn(HD))
        attn.norm_k.weight.copy_(1 + 0.1 * torch.randn(HD))
    hidden = (torch.randn(2, S, DIM) * 0.3).to(DT).cuda()
    enc = (torch.randn(2, N_TXT, DIM) * 0.3).to(DT).cuda()
    # independent values in both table halves: more than the model's duplicated angles ask of the kernel
    cos, sin = torch.randn(S, HD).cuda(), torch.randn(S, HD).cuda()
    return attn.cuda(), hidden, enc, (cos, sin)


def run(cls, fused, attn, hidden, seed=11, **kw):
    """one call on a fresh processor; the global seeds (profiler rows: CPU generator; k-means initial points: device generator) reset"""
    proc = cls(0)
    proc.fused_prologue = fused
    attn.set_processor(proc)
    torch.manual_seed(seed)
    with torch.no_grad():
        out = attn(hidden, **kw)
    torch.cuda.synchronize()
    return out, getattr(proc, "last_best_mask_idx", None)


@pytest.fixture
def counts(monkeypatch):
    """calls of _native.qk_norm_rope_transpose (with their norm / rope kinds), _native.qk_norm_rope and apply_rotary_emb_half"""
    from svg import _native
    from svg.models.cosmos import attention as cosmos_attention

    calls = {"transpose": [], "inplace": [], "torch_rope": 0}

    def kinds(fn, a, kw):
        b = inspect.signature(fn).bind(*a, **kw)
        b.apply_defaults()
        return b.arguments["norm_kind"], b.arguments["rope_kind"]

    real_t, real_i, real_r = _native.qk_norm_rope_transpose, _native.qk_norm_rope, cosmos_attention.apply_rotary_emb_half

    def counted_t(*a, **kw):
        calls["transpose"].append(kinds(real_t, a, kw))
        return real_t(*a, **kw)

    def counted_i(*a, **kw):
        calls["inplace"].append(kinds(real_i, a, kw))
        return real_i(*a, **kw)

    def counted_r(*a, **kw):
        calls["torch_rope"] += 1
        return real_r(*a, **kw)

    monkeypatch.setattr(_native, "qk_norm_rope_transpose", counted_t)
    monkeypatch.setattr(_native, "qk_norm_rope", counted_i)
    monkeypatch.setattr(cosmos_attention, "apply_rotary_emb_half", counted_r)
    return calls


def fresh(calls):
    calls["transpose"].clear()
    calls["inplace"].clear()
    calls["torch_rope"] = 0


@pytest.mark.parametrize("timestep", [100.0, 950.0], ids=["sparse", "dense_warmup"])
def test_svg1_processor_fused_equals_staged(procs, data, timestep):
    SvgP, _ = procs
    attn, hidden, _, rope = data
    kw = dict(image_rotary_emb=rope, timestep=torch.tensor([timestep]))
    a, best_a = run(SvgP, True, attn, hidden[:1], **kw)
    b, best_b = run(SvgP, False, attn, hidden[:1], **kw)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    if timestep < SvgP.first_times_fp:
        assert best_a is not None and torch.equal(best_a, best_b)
    else:
        assert best_a is None and best_b is None


def test_sap_processor_fused_equals_staged(procs, data):
    _, SapP = procs
    attn, hidden, _, rope = data
    kw = dict(image_rotary_emb=rope, timestep=torch.tensor([100.0]))   # sparse step of a fresh layer: k-means from seeded initial points
    a, _ = run(SapP, True, attn, hidden[:1], **kw)
    b, _ = run(SapP, False, attn, hidden[:1], **kw)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_call_counts(procs, data, counts):
    SvgP, _ = procs
    attn, hidden, enc, rope = data
    self_kw = dict(image_rotary_emb=rope, timestep=torch.tensor([100.0]))
    cross_kw = dict(encoder_hidden_states=enc, timestep=None)
    run(SvgP, True, attn, hidden, **self_kw)
    assert counts == {"transpose": [(1, 3)], "inplace": [], "torch_rope": 0}       # q and k in ONE pass, v in place: no second launch
    fresh(counts)
    run(SvgP, True, attn, hidden, **cross_kw)
    assert counts == {"transpose": [(1, 0), (1, 0)], "inplace": [], "torch_rope": 0}   # q, and the short k: norm only
    fresh(counts)
    run(SvgP, False, attn, hidden, **self_kw)
    assert counts == {"transpose": [], "inplace": [(1, 0)], "torch_rope": 2}       # today's: in-place norm of q and k, torch RoPE twice
    fresh(counts)
    run(SvgP, False, attn, hidden, **cross_kw)
    assert counts == {"transpose": [], "inplace": [(1, 0), (1, 0)], "torch_rope": 0}   # Sq != Skv: one in-place norm per tensor


def _mask(windows):
    m = torch.zeros(len(windows), 1, 1, N_TXT, dtype=torch.bool)
    for b, (lo, hi) in enumerate(windows):
        m[b, 0, 0, lo:hi] = True
    return m.cuda()


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "key_padding_mask"])
def test_cross_call_fused_equals_staged(procs, data, masked):
    from svg.models import _core

    SvgP, _ = procs
    attn, hidden, enc, _ = data
    mask = _mask([(0, 25), (0, 60)]) if masked else None
    if masked:
        assert _core.key_windows(mask, 2, N_TXT) is not None
    kw = dict(encoder_hidden_states=enc, attention_mask=mask, timestep=None)
    a, _ = run(SvgP, True, attn, hidden, **kw)
    b, _ = run(SvgP, False, attn, hidden, **kw)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


class OddNorm(nn.Module):
    """a norm _core._norm_desc does not recognise (no eps): the processors run the module itself"""

    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim, dtype=DT))

    def forward(self, x):
        return (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-3)).to(x.dtype) * self.weight


@pytest.mark.parametrize("what", ["table_shape", "norm_module"])
def test_fallback_to_the_staged_path(procs, data, counts, what):
    SvgP, _ = procs
    attn, hidden, enc, rope = data
    saved = attn.norm_q, attn.norm_k
    try:
        if what == "table_shape":    # one table row for all positions: torch broadcasts it, the kernel's table is [S, D]
            rope = (rope[0][:1].contiguous(), rope[1][:1].contiguous())
        else:
            attn.norm_q, attn.norm_k = OddNorm(HD).cuda(), OddNorm(HD).cuda()
        kw = dict(image_rotary_emb=rope, timestep=torch.tensor([100.0]))
        a, best_a = run(SvgP, True, attn, hidden[:1], **kw)
        assert counts["transpose"] == [] and counts["torch_rope"] == 2           # the staged steps ran
        b, best_b = run(SvgP, False, attn, hidden[:1], **kw)
        assert torch.isfinite(a.float()).all() and torch.equal(a, b) and torch.equal(best_a, best_b)
        if what == "norm_module":    # ... and on the cross call
            fresh(counts)
            ckw = dict(encoder_hidden_states=enc, timestep=None)
            c, _ = run(SvgP, True, attn, hidden, **ckw)
            assert counts["transpose"] == [] and counts["inplace"] == []
            d, _ = run(SvgP, False, attn, hidden, **ckw)
            assert torch.equal(c, d)
    finally:
        attn.norm_q, attn.norm_k = saved
