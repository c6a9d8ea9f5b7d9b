"""CPU checks of the half-split RoPE kind and of the Cosmos processors' fused prologue: on CPU tensors the fused step does not apply (the
staged steps run, nothing native is called), and the C entry points' argument validation for rope_kind 3 (no GPU is touched: every call
is rejected before a launch)."""
import pytest
import torch

from standins import Attention

BAD, UNSUP = -1, -2
HEADS, HD, F_, P_ = 2, 32, 3, 20
DIM, S = HEADS * HD, F_ * P_


@pytest.fixture
def no_native(monkeypatch):
    from svg import _native

    def refuse(*a, **kw):
        raise AssertionError("a native prologue entry was called on CPU tensors")

    for name in ("qk_norm_rope_transpose", "qk_norm_rope", "rmsnorm_rope_transpose", "qk_norm_rope_transpose_joint"):
        monkeypatch.setattr(_native, name, refuse)


@pytest.mark.parametrize("sap", [False, True], ids=["svg1", "sap"])
def test_cpu_tensors_take_the_staged_path(no_native, monkeypatch, sap):
    from svg.models.cosmos import attention as cosmos_attention

    P = cosmos_attention.Cosmos_SAPAttn_Processor if sap else cosmos_attention.Cosmos_SVG_AttnProcessor2_0
    for n, v in dict(context_length=0, num_frame=F_, frame_size=P_, first_layers_fp=0, first_times_fp=900.0,
                     zero_step_kmeans_init=False).items():
        monkeypatch.setattr(P, n, v, raising=False)
    assert P.fused_prologue is True
    ropes = []
    real = cosmos_attention.apply_rotary_emb_half
    monkeypatch.setattr(cosmos_attention, "apply_rotary_emb_half", lambda *a: ropes.append(1) or real(*a))
    torch.manual_seed(0)
    attn = Attention(DIM, HEADS, qk_norm="rms")
    hidden, enc = torch.randn(2, S, DIM) * 0.3, torch.randn(2, 7, DIM) * 0.3
    rope = (torch.randn(S, HD), torch.randn(S, HD))
    calls = (dict(image_rotary_emb=rope, timestep=torch.tensor([950.0])),     # dense warm-up step (the sparse step has no CPU path)
             dict(image_rotary_emb=rope, timestep=None),                      # no timestep: plain SDPA
             dict(encoder_hidden_states=enc, timestep=None))                  # cross call
    outs = {}
    for fused in (True, False):
        proc = P(0)
        proc.fused_prologue = fused
        attn.set_processor(proc)
        with torch.no_grad():
            outs[fused] = [attn(hidden, **kw) for kw in calls]
    assert len(ropes) == 2 * 2 * 2      # both settings ran the torch RoPE on q and k of the two self-attention calls
    for a, b in zip(outs[True], outs[False]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_core_helpers_decline_cpu_tensors_and_conflicting_kinds():
    from svg.models import _core

    q = torch.randn(1, 8, DIM, dtype=torch.bfloat16)
    cs = torch.randn(8, HD)
    assert _core.qkv_from_projections(q, q.clone(), q.clone(), HEADS, None, None, cs, cs, 0, 8, half_split=True) is None
    x = torch.randn(1, HEADS, 8, HD, dtype=torch.bfloat16)
    assert _core.qk_rope_inplace(x, x.clone(), cs, cs, 0, 8, half_split=True) is False
    with pytest.raises(AssertionError):
        _core.qk_rope_inplace(x, x.clone(), cs, cs, 0, 8, complex_pairs=True, half_split=True)
    with pytest.raises(AssertionError):
        _core.qkv_from_projections(q, q.clone(), q.clone(), HEADS, None, None, cs, cs, 0, 8, complex_pairs=True, half_split=True)


def test_entry_point_validation_for_half_split():
    from svg import _native

    lib = _native.load()
    q, k, qo, ko, tb = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000      # never dereferenced: every call below is rejected before a launch

    def inplace(rk, cos=tb, sin=tb, S=16, D=64, lo=0, hi=16):
        a = lib.svg_qk_norm_rope(q, k, 1, 2, 2, S, D, 0, 1, None, None, None, None, 1e-6, rk, cos, sin, lo, hi, None)
        b = lib.svg_qk_norm_rope_qscale(q, k, 1, 2, 2, S, D, 0, 1, None, None, None, None, 1e-6, rk, cos, sin, lo, hi, 1.0, None)
        assert a == b
        return a

    def transpose(rk, cos=tb, sin=tb, S=16, D=64, lo=0, hi=16):
        a = lib.svg_qk_norm_rope_transpose(q, k, qo, ko, 1, 2, 2, S, D, 0, 1, None, None, None, None, 1e-6, rk, cos, sin, lo, hi, None)
        b = lib.svg_qk_norm_rope_transpose_qscale(q, k, qo, ko, 1, 2, 2, S, D, 0, 1, None, None, None, None, 1e-6, rk, cos, sin, lo, hi, 1.0,
                                                  None)
        assert a == b
        return a

    for call in (inplace, transpose):
        assert call(3, cos=None) == BAD and call(3, sin=None) == BAD            # kind 3 without its tables
        assert call(3, hi=17) == BAD and call(3, lo=-1) == BAD and call(3, lo=9, hi=8) == BAD
        assert call(4) == BAD and call(-1) == BAD
        assert call(3, D=96) == UNSUP and call(0, D=96) == UNSUP
    # the entries that do not know the kind
    seg = (_native.PrologueSegment * 1)()
    seg[0].q_in = seg[0].k_in = seg[0].v_in = q
    seg[0].rows, seg[0].norm_kind, seg[0].eps = 16, 1, 1e-6
    assert lib.svg_qk_norm_rope_transpose_joint(seg, 1, qo, ko, ko + 0x8000, 1, 2, 64, 0, 3, tb, tb, 0, 16, 1.0, None) == BAD
    assert lib.svg_rmsnorm_rope_transpose(q, k, None, qo, ko, None, 1, 2, 16, 64, 0, None, None, 0, 1e-6, 3, tb, tb, 0, 16, 1.0, None) == BAD
