"""The centroid tail merged in the tail kernel's epilogue (include/svg_attn_centroid_tail_merged.h) on the GPU, on poisoned allocations:
the 16-bit form against today's three launches bit for bit, the fp32 form against the float64 statement of tests/centroid_tail_cases.py,
and svg2_sparse_attention(centroid_tail=True) with CENTROID_TAIL_MERGED on against off.  Bounds: tests/sparse_lse_cases.py."""
import functools

import pytest
import torch

import centroid_tail_cases as TC
from poisoned import assert_fully_written, unwritten
from sparse_lse_cases import T_SINGLE, check_lse, rel_l2
from test_gpu_centroid_tail import layer_call, opt
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
NINF = float("-inf")
WRAPPERS = ("varblock_attention", "cluster_means", "centroid_tail_attention", "merge_attention_states")


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def recorded_layer_call(kind, dtype, **kw):
    """one svg2_sparse_attention(centroid_tail=True) on TC.layer_inputs -> its output and the (name, args, kwargs) of every WRAPPERS call"""
    from svg import _native
    from svg.models import _core

    calls, mp = [], pytest.MonkeyPatch()
    for n in WRAPPERS:
        mp.setattr(_native, n, lambda *a, _n=n, _f=getattr(_native, n), **k: (calls.append((_n, a, k)), _f(*a, **k))[1], raising=False)
    try:
        out = layer_call(_core, kind, *(dev(x) for x in TC.layer_inputs(kind, 1, dtype)), centroid_tail=True, **kw)
    finally:
        mp.undo()
    return out, calls


@functools.lru_cache(maxsize=None)
def launch_inputs(kind, dtype):
    """What a layer-call on the Wan-like (S = 1024, QC 4, KC 16) / HunyuanVideo-like (S = 1088: 6 block-rows, a map of 18 columns over 16
    centroids) geometry hands its sparse and its tail launch — the library's own ragged clusters — with map rows edited: block-row 0 selects
    every cluster (no tail), block-row 1 none (no sparse part); HunyuanVideo's last block-row, which gets no tail, selects nothing either."""
    calls = {n: (a, k) for n, a, k in recorded_layer_call(kind, dtype)[1]}
    (q, k, v, smap, qsz, ksz), skw = calls["varblock_attention"]
    (_, kbar, vbar, tmap, _, ks), _ = calls["centroid_tail_attention"]
    smap, tmap = smap.clone(), tmap.clone()
    smap[:, 0], tmap[:, 0], smap[:, 1], tmap[:, 1] = True, True, False, False
    if kind == "hy":
        smap[:, -1] = False
    assert int(qsz.min()) > 0 and bool((qsz % 16 != 0).any()) and tmap.shape[2] == ks.shape[1] + (2 if kind == "hy" else 0)
    return dict(sparse=(q, k, v, smap, qsz, ksz), tail=(q, kbar, vbar, tmap, qsz, ks), rows=skw["q_row_idx"], kidx=skw["kv_row_idx"])


@pytest.mark.parametrize("in_place", [False, True], ids=["new_o", "in_place"])
@pytest.mark.parametrize("with_idx", [False, True], ids=["sorted", "q_row_idx"])
@pytest.mark.parametrize("token_major", [False, True], ids=["contiguous", "token_major"])
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
@pytest.mark.parametrize("kind", sorted(TC.GEOMETRIES))
def test_16_bit_form_has_the_bits_of_the_three_launches(nat, kind, dtype, token_major, with_idx, in_place):
    c = launch_inputs(kind, dtype)
    rows = c["rows"] if with_idx else None
    o_s, lse_s = nat.varblock_attention(*c["sparse"], q_row_idx=rows, kv_row_idx=c["kidx"], return_lse=True)
    o_t, lse_t = nat.centroid_tail_attention(*c["tail"], q_row_idx=rows)
    want, want_lse = nat.merge_attention_states([o_s, o_t], [lse_s, lse_t], token_major_out=token_major, return_lse=True)
    part = nat.token_major_empty(o_s).copy_(o_s) if token_major else o_s.clone()
    out = part if in_place else nat.token_major_empty(o_s) if token_major else None
    o, lse = nat.centroid_tail_attention(*c["tail"], q_row_idx=rows, merge_with=(part, lse_s), out=out)
    assert_fully_written(o, "o")
    assert o.is_contiguous() != token_major and (o.data_ptr() == part.data_ptr()) == in_place
    assert torch.equal(o, want) and torch.equal(lse, want_lse)
    no_tail, no_sparse = lse_t == NINF, lse_s == NINF
    assert (no_tail & ~no_sparse).any() and (no_sparse & ~no_tail).any() and (no_tail & no_sparse).any() == (kind == "hy")
    assert torch.equal(o[no_tail], o_s[no_tail]) and torch.equal(lse[no_tail], lse_s[no_tail])      # no tail: the sparse part's bits
    assert (o[no_tail & no_sparse] == 0).all() and (lse[no_tail & no_sparse] == NINF).all()


@pytest.mark.parametrize("with_idx", [False, True], ids=["sorted", "row_idx"])
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
@pytest.mark.parametrize("KC", TC.KCS)
def test_fp32_form_matches_the_float64_statement_and_is_not_behind_the_16_bit_form(nat, KC, dtype, with_idx):
    c, st = TC.merge_case(KC, dtype, with_idx), TC.merge_reference(KC, dtype, with_idx)
    sparse = [dev(c[n]) for n in ("q", "k", "v", "bmap", "q_sizes", "k_sizes")]
    tail = [sparse[0], dev(c["kbar"]), dev(c["vbar"])] + sparse[3:]
    kw = dict(q_row_idx=opt(c["q_idx"]), kv_row_idx=opt(c["kv_idx"]), return_lse=True)
    o32, lse_s = nat.varblock_attention(*sparse, out_dtype=torch.float32, **kw)
    o_f, lse_f = nat.centroid_tail_attention(*tail, q_row_idx=kw["q_row_idx"], merge_with=(o32, lse_s))
    o_h, lse_h = nat.centroid_tail_attention(*tail, q_row_idx=kw["q_row_idx"], merge_with=nat.varblock_attention(*sparse, **kw))
    assert o32.dtype == torch.float32 and o_f.dtype == dtype
    assert_fully_written(o_f, "o")
    e_f, e_h = rel_l2(o_f.cpu(), st["o"]), rel_l2(o_h.cpu(), st["o"])
    print(f"merged in the epilogue, KC {KC} {dtype}: rel_l2 to float64 fp32 parts {e_f:.3e}, 16-bit parts {e_h:.3e} (limit {T_SINGLE[dtype]:.1e})")
    assert e_f <= T_SINGLE[dtype] and e_f <= e_h
    check_lse(lse_f, st["lse"], dtype, f"merged fp32 KC {KC}")


@pytest.mark.parametrize("kind", sorted(TC.GEOMETRIES))
def test_layer_call_with_the_switch_on_has_the_bits_of_the_switch_off_and_one_launch_fewer(nat, monkeypatch, kind):
    from svg.models import _core

    assert _core.CENTROID_TAIL_MERGED is False
    off, calls_off = recorded_layer_call(kind, torch.bfloat16)
    monkeypatch.setattr(_core, "CENTROID_TAIL_MERGED", True)
    on, calls_on = recorded_layer_call(kind, torch.bfloat16)
    monkeypatch.setattr(_core, "CENTROID_TAIL_MERGED", "f32")
    f32, calls_f32 = recorded_layer_call(kind, torch.bfloat16)
    names = lambda calls: [n for n, _, _ in calls]   # noqa: E731
    today = ["varblock_attention", "cluster_means", "cluster_means", "centroid_tail_attention", "merge_attention_states"]
    assert names(calls_off) == today and names(calls_on) == names(calls_f32) == today[:-1]
    assert all("merge_with" not in k for _, _, k in calls_off)
    assert calls_on[-1][2]["out"] is calls_on[-1][2]["merge_with"][0] and calls_f32[-1][2]["merge_with"][0].dtype == torch.float32
    assert not unwritten(on).any() and not unwritten(f32).any()
    assert on.stride() == off.stride() == f32.stride() and torch.equal(on, off)
    # one rounding against two: each rounding moves an element by at most 2^-9 of itself (bf16), the tail's inner one by less (weight < 1)
    assert not torch.equal(f32, off) and rel_l2(f32.cpu(), off.cpu().double()) <= 3 * 2.0 ** -9
