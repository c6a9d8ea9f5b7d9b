"""svg_cross_attention_lse / svg_merge_attention_states without a GPU: the exports, the argument validation (every check runs on the
host before any launch — rows that pass placeholder pointers are skipped where a GPU is visible, as in test_cross_attention_cpu.py), the
torch statements of attention-with-LSE and of the N-way merge (tests/lse_ops_torch.py: merged key shards equal full attention), and the
schedule of svg.distributed.token_sharded_dense_attention on gloo CPU ranks with those statements as attn_fn / merge_fn.

ref: flashinfer's run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188; the context-parallel dense attention
of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169."""
import ctypes as C

import pytest
import torch

from gloo_ranks import run_ranks
from lse_ops_torch import attention_lse, merge_states
from svg import _native as nat

BAD_ARG, UNSUPPORTED = -1, -2
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
S_ROWS = 1 << 24


def test_library_exports_lse_and_merge():
    lib = nat.load()
    for name in ("svg_cross_attention_lse", "svg_merge_attention_states"):
        assert name in nat.SIGNATURES
        assert getattr(lib, name).argtypes == nat.SIGNATURES[name][1]
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def lse_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=4, Sq=256, Skv=64, D=128, dtype=0, kv_begin=None, kv_end=None, hpw=1, lay=None):
    return [q, k, v, o, lse, BH, Sq, Skv, D, dtype, 1.0, kv_begin, kv_end, hpw, C.byref(lay) if lay is not None else None, None]


def bad_layout(**kw):
    H, Sq, Skv, row = 2, 256, 64, 128
    q = nat.TensorStrides(H * Sq * row, Sq * row, row)
    k = nat.TensorStrides(H * Skv * row, Skv * row, row)
    lay = nat.AttnLayout(H, 0, q, k, k, q)
    for name, val in kw.items():
        setattr(lay, name, val)
    return lay


LSE_CASES = [
    ("null_q", lse_args(q=None), BAD_ARG),
    ("null_k", lse_args(k=None), BAD_ARG),
    ("null_v", lse_args(v=None), BAD_ARG),
    ("null_o", lse_args(o=None), BAD_ARG),
    ("null_lse", lse_args(lse=None), BAD_ARG),
    ("BH0", lse_args(BH=0), BAD_ARG),
    ("Sq0", lse_args(Sq=0), BAD_ARG),
    ("Skv_neg", lse_args(Skv=-5), BAD_ARG),
    ("window_hpw0", lse_args(kv_end=PH, hpw=0), BAD_ARG),
    ("window_hpw_not_dividing", lse_args(kv_end=PH, hpw=3), BAD_ARG),
    ("D64", lse_args(D=64), UNSUPPORTED),
    ("D96", lse_args(D=96), UNSUPPORTED),
    ("dtype_f32", lse_args(dtype=2), UNSUPPORTED),
    ("Sq_rows", lse_args(Sq=S_ROWS), UNSUPPORTED),
    ("Skv_rows", lse_args(Skv=S_ROWS), UNSUPPORTED),
    ("layout_heads0", lse_args(lay=bad_layout(heads_per_batch=0)), BAD_ARG),
]


@pytest.mark.parametrize("args,expected", [c[1:] for c in LSE_CASES], ids=[c[0] for c in LSE_CASES])
def test_cross_attention_lse_rejects(args, expected):
    if any(a == PH for a in args) and torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert nat.load().svg_cross_attention_lse(*args) == expected


def _ptrs(vals):
    return C.cast((C.c_void_p * 9)(*vals, *([None] * (9 - len(vals)))), C.c_void_p)


def merge_args(o_parts=(PH, PH), lse_parts=(PH, PH), n=2, o=PH, lse=PH, BH=4, Sq=256, D=128, dtype=0, lay=None):
    return [_ptrs(o_parts) if o_parts is not None else None, _ptrs(lse_parts) if lse_parts is not None else None, n, o, lse, BH, Sq, D, dtype,
            C.byref(lay) if lay is not None else None, None]


MERGE_CASES = [
    ("null_o_parts", merge_args(o_parts=None), BAD_ARG),
    ("null_lse_parts", merge_args(lse_parts=None), BAD_ARG),
    ("null_part", merge_args(o_parts=(PH, None)), BAD_ARG),
    ("null_part_lse", merge_args(lse_parts=(None, PH)), BAD_ARG),
    ("null_o", merge_args(o=None), BAD_ARG),
    ("n0", merge_args(n=0), BAD_ARG),
    ("n9", merge_args(o_parts=(PH,) * 9, lse_parts=(PH,) * 9, n=9), BAD_ARG),
    ("n_neg", merge_args(n=-1), BAD_ARG),
    ("BH0", merge_args(BH=0), BAD_ARG),
    ("Sq0", merge_args(Sq=0), BAD_ARG),
    ("D0", merge_args(D=0), BAD_ARG),
    ("D96", merge_args(D=96), UNSUPPORTED),
    ("D256", merge_args(D=256), UNSUPPORTED),
    ("dtype_f32", merge_args(dtype=2), UNSUPPORTED),
    ("Sq_rows", merge_args(Sq=S_ROWS), UNSUPPORTED),
    ("part_unaligned", merge_args(o_parts=(PH, PH + 8)), UNSUPPORTED),
    ("o_unaligned", merge_args(o=PH + 8), UNSUPPORTED),
    ("layout_heads0", merge_args(lay=bad_layout(heads_per_batch=0)), BAD_ARG),
    ("layout_heads_not_dividing", merge_args(BH=3, lay=bad_layout()), BAD_ARG),
    ("layout_o_row_lt_D", merge_args(lay=bad_layout(o=nat.TensorStrides(2 * 256 * 64, 256 * 64, 64))), BAD_ARG),
    ("layout_o_row_unaligned", merge_args(lay=bad_layout(o=nat.TensorStrides(2 * 256 * 132, 256 * 132, 132))), UNSUPPORTED),
]


@pytest.mark.parametrize("args,expected", [c[1:] for c in MERGE_CASES], ids=[c[0] for c in MERGE_CASES])
def test_merge_attention_states_rejects(args, expected):
    """(the pointer ARRAYS are real host memory; what they hold are placeholders)"""
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert nat.load().svg_merge_attention_states(*args) == expected


def test_bindings_refuse_cpu_tensors_and_too_many_parts():
    q, k = torch.zeros(1, 2, 8, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 4, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError):
        nat.cross_attention(q, k, k, return_lse=True)
    lse = torch.zeros(1, 2, 8)
    with pytest.raises(RuntimeError):
        nat.merge_attention_states([q, q], [lse, lse])
    with pytest.raises(ValueError, match="1 to 8"):
        nat.merge_attention_states([q] * 9, [lse] * 9)


# ---------------------------------------------------------------------------------------------------------
# the torch statements: merged key shards equal full attention
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", [[0, 1, 1000], [0, 250, 500, 750, 1000], [0, 400, 400, 1000]], ids=["1+999", "4x250", "empty_shard"])
def test_merged_key_shards_equal_full_attention(cuts):
    g = torch.Generator().manual_seed(len(cuts))
    q = torch.randn(2, 3, 37, 128, generator=g, dtype=torch.float64)
    k, v = (torch.randn(2, 3, 1000, 128, generator=g, dtype=torch.float64) for _ in range(2))
    o_full, lse_full = attention_lse(q, k, v)
    parts = [attention_lse(q, k[:, :, a:b], v[:, :, a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    o, lse = merge_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
    assert (o - o_full).abs().max() <= 1e-12 and (lse - lse_full).abs().max() <= 1e-12
    sdpa = torch.nn.functional.scaled_dot_product_attention(q, k, v)
    assert (o_full - sdpa).abs().max() <= 1e-12


def test_merge_statement_edge_cases():
    g = torch.Generator().manual_seed(0)
    o1, o2 = (torch.randn(5, 8, generator=g, dtype=torch.float64) for _ in range(2))
    l1 = torch.randn(5, generator=g, dtype=torch.float64)
    ninf = torch.full((5,), float("-inf"), dtype=torch.float64)
    o, lse = merge_states([o1, o2], [l1, ninf], return_lse=True)
    assert torch.equal(o, o1) and torch.equal(lse, l1)
    o, lse = merge_states([torch.full_like(o1, float("nan")), o2], [ninf, ninf], return_lse=True)
    assert torch.equal(o, torch.zeros_like(o)) and torch.equal(lse, ninf)
    o, lse = merge_states([o1], [l1], return_lse=True)
    assert torch.equal(o, o1) and torch.equal(lse, l1)


# ---------------------------------------------------------------------------------------------------------
# token_sharded_dense_attention on gloo CPU ranks
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world):
    from svg.distributed import token_range, token_sharded_dense_attention

    calls = []

    def attn_fn(q, k, v, return_lse=False):
        calls.append((k.shape[-2], return_lse))
        return attention_lse(q, k, v, return_lse=return_lse)

    H, S, D = 3, 700, 32
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(1, H, S, D, generator=g) for _ in range(3))
    ref = attention_lse(q.double(), k.double(), v.double(), return_lse=False).float()
    worst = 0.0
    ok = True
    for unit in (1, 128):
        a, b = token_range(S, rank, world, unit)
        ql, kl, vl = (x[:, :, a:b].contiguous() for x in (q, k, v))
        outs = {}
        for overlap in (False, True):
            calls.clear()
            o = token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=overlap, attn_fn=attn_fn, merge_fn=merge_states)
            ok &= o.shape == ql.shape
            if overlap:   # one part per rank, the own shard first, then the shards of rank - 1, rank - 2, ...
                want = [(token_range(S, (rank - j) % world, world, unit), True) for j in range(world)]
                ok &= calls == [(hi - lo, flag) for (lo, hi), flag in want]
            else:
                ok &= calls == [(S, False)]
            worst = max(worst, (o - ref[:, :, a:b]).abs().max().item())
            outs[overlap] = o
        worst = max(worst, (outs[True] - outs[False]).abs().max().item())
    return bool(ok), worst


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_dense_attention_gloo(world):
    """ragged token_range (700 tokens on three ranks: unit 1 -> 234 / 233 / 233, unit 128 -> 256 / 256 / 188), both overlap settings: every
    rank's rows equal the single-process result to 1e-5, and the two settings agree to the same bound"""
    for rank, (ok, worst) in run_ranks(_worker, world, 41500).items():
        assert ok, rank
        assert worst <= 1e-5, (rank, worst)


def test_token_sharded_dense_attention_names_the_merge_limit(monkeypatch):
    from svg import distributed as sd

    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 9)
    x = torch.zeros(1, 2, 900 // 9, 16)
    with pytest.raises(ValueError, match="at most 8 parts"):
        sd.token_sharded_dense_attention(x, x, x, 900, overlap=True)
