"""The centroid tail without a GPU (include/svg_attn_centroid_tail.h): the exports, the header and its prototypes against the ctypes
signatures; the argument validation of both entries — every check runs on the host before any launch, in the documented order (rows that
pass placeholder pointers are skipped where a GPU is visible, as in tests/test_kmeans_e4m3_cpu.py) —; the refusals of the wrappers and of
svg2_sparse_attention; and the float64 identities of the statement in tests/centroid_tail_cases.py: sparse + tail IS dense attention on
clusters of identical rows, the merged log-sum-exp lies between the sparse and the dense one under exact means (Jensen), and on the fixed
mixtures of the GPU layer test the merged output is nearer to dense attention than the sparse one."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import centroid_tail_cases as TC
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH, PA, PB, PC = 0x10000, 0x20000, 0x30000, 0x40000   # placeholder device pointers (16-byte aligned; never dereferenced by a rejected call)
ROOT = Path(__file__).resolve().parent.parent
ENTRIES = {"svg_cluster_means", "svg_centroid_tail_workspace_bytes", "svg_centroid_tail_attention_lse"}
BIG = 1 << 40


# ---------------------------------------------------------------------------------------------------------
# exports, header, prototypes
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    lib = nat.load()
    assert set(nat.CENTROID_TAIL_ENTRIES) == ENTRIES
    others = set()
    for name in dir(nat):
        if (name.endswith("SIGNATURES") or name.endswith("ENTRIES")) and name != "CENTROID_TAIL_ENTRIES" and isinstance(getattr(nat, name), dict):
            others |= set(getattr(nat, name))
    assert "svg_varblock_attention_lse" in others and not ENTRIES & others
    for name, (res, args) in nat.CENTROID_TAIL_ENTRIES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4
    for name in ("cluster_means", "centroid_tail_attention"):
        assert callable(getattr(nat, name))
    with pytest.raises(AttributeError):
        nat.centroid_tail_nothing


def test_header_is_included_not_last_and_matches_the_signatures():
    main = (ROOT / "include" / "svg_attn.h").read_text()
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', main, flags=re.M)
    assert "svg_attn_centroid_tail.h" in includes and includes[-1] != "svg_attn_centroid_tail.h"
    src = (ROOT / "include" / "svg_attn_centroid_tail.h").read_text()
    assert "in this order" in src and "Jensen" in src and "SVG_ERR_WORKSPACE" in src and "SVG_ABI_VERSION is unchanged" in src
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert {n for _, n, _ in protos} == ENTRIES

    def c_class(t):
        for pat, c in ((r"\*", "ptr"), (r"\bsize_t\b", "size"), (r"\bint64_t\b", "i64"), (r"\b(int32_t|int)\b", "i32"), (r"\bfloat\b", "f32")):
            if re.search(pat, t):
                return c
        return "?" + t

    def py_class(a):
        if a is C.c_void_p or (isinstance(a, type) and issubclass(a, C._Pointer)):
            return "ptr"
        return {C.c_size_t: "size", C.c_int64: "i64", C.c_int32: "i32", C.c_int: "i32", C.c_float: "f32"}.get(a, "?" + repr(a))

    for ret, name, params in protos:
        ps = [x.strip() for x in params.split(",") if x.strip()]
        want = [c_class(x if x.endswith("*") else re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", x)) for x in ps]
        res, args = nat.CENTROID_TAIL_ENTRIES[name]
        assert [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


def test_workspace_bytes():
    ws = nat.load().svg_centroid_tail_workspace_bytes
    assert ws(2, 6, 70) >= 2 * 6 * 4 and ws(2, 6, 70) % 16 == 0
    assert ws(40, 302, 1000) >= 40 * 302 * 4 and ws(3, 7, 4032) > 0
    for bad in ((0, 6, 70), (2, 0, 70), (2, 6, 0), (2, 6, 4033), (-1, 6, 70)):
        assert ws(*bad) == 0, bad


# ---------------------------------------------------------------------------------------------------------
# the validation tables: codes and their order
# ---------------------------------------------------------------------------------------------------------
def host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


def strides(batch=2 * 700 * 128, head=128, row=2 * 128):
    return C.byref(nat.TensorStrides(batch, head, row))


def means_args(x=PH, st=None, hpb=2, srt=PA, cnt=PB, out=PC, B=4, N=700, K=129, D=128, dtype=0):
    return [x, st, hpb, srt, cnt, out, B, N, K, D, dtype, None]


MEANS_CASES = [
    ("null_x", means_args(x=None), BAD_ARG),
    ("null_sorted_idx", means_args(srt=None), BAD_ARG),
    ("null_counts", means_args(cnt=None), BAD_ARG),
    ("null_means", means_args(out=None), BAD_ARG),
    ("B0", means_args(B=0), BAD_ARG),
    ("N_neg", means_args(N=-1), BAD_ARG),
    ("K0", means_args(K=0), BAD_ARG),
    ("null_before_unsupported", means_args(out=None, D=96), BAD_ARG),
    ("heads_per_batch0", means_args(st=strides(), hpb=0), BAD_ARG),
    ("heads_per_batch_not_dividing_B", means_args(st=strides(), hpb=3), BAD_ARG),
    ("row_stride_below_D", means_args(st=strides(row=64)), BAD_ARG),
    ("negative_head_stride", means_args(st=strides(head=-128)), BAD_ARG),
    ("stride_fault_before_unsupported", means_args(st=strides(row=64), dtype=2), BAD_ARG),
    ("heads_per_batch_ignored_without_strides", means_args(hpb=0, D=96), UNSUPPORTED),
    ("D96", means_args(D=96), UNSUPPORTED),
    ("D256", means_args(D=256), UNSUPPORTED),
    ("dtype_f32", means_args(dtype=2), UNSUPPORTED),
    ("stride_not_multiple_of_8", means_args(st=strides(batch=2 * 700 * 128 + 4)), UNSUPPORTED),
    ("x_not_16_byte_aligned", means_args(x=PH + 8), UNSUPPORTED),
    ("means_not_16_byte_aligned", means_args(out=PC + 2), UNSUPPORTED),
]


def layout(hpb=2, batch=777 * 2 * 128, head=128, row=2 * 128):
    s = nat.TensorStrides(batch, head, row)
    junk = nat.TensorStrides(-5, 3, 1)     # (the k, v, o members are not read)
    return C.byref(nat.AttnLayout(hpb, 0, s, junk, junk, junk))


def tail_args(q=PH, kbar=PA, vbar=PB, o=PC, lse=PH, H=2, Sq=777, KC=70, D=128, dtype=0, bmap=PA, cols=None, qs=PB, ks=PC, QB=6, idx=None, ws=PH,
              nb=BIG, lay=None):
    return [q, kbar, vbar, o, lse, H, Sq, KC, D, dtype, 0.088, bmap, KC if cols is None else cols, qs, ks, QB, idx, ws, nb, lay, None]


TAIL_CASES = [
    # 1. pointers and sizes
    ("null_q", tail_args(q=None), BAD_ARG),
    ("null_kbar", tail_args(kbar=None), BAD_ARG),
    ("null_vbar", tail_args(vbar=None), BAD_ARG),
    ("null_o", tail_args(o=None), BAD_ARG),
    ("null_lse", tail_args(lse=None), BAD_ARG),
    ("null_block_map", tail_args(bmap=None), BAD_ARG),
    ("null_q_sizes", tail_args(qs=None), BAD_ARG),
    ("null_k_sizes", tail_args(ks=None), BAD_ARG),
    ("null_workspace", tail_args(ws=None), BAD_ARG),
    ("H0", tail_args(H=0), BAD_ARG),
    ("Sq_neg", tail_args(Sq=-3), BAD_ARG),
    ("KC0", tail_args(KC=0, cols=4), BAD_ARG),
    ("QB0", tail_args(QB=0), BAD_ARG),
    ("null_before_everything_else", tail_args(lse=None, cols=3, D=64, nb=0, lay=layout(hpb=0)), BAD_ARG),
    # 2. the map's row pitch
    ("map_cols_below_KC", tail_args(cols=69), BAD_ARG),
    ("map_cols_before_layout", tail_args(cols=69, lay=layout(row=2 * 128 + 4)), BAD_ARG),
    ("map_cols_before_workspace_and_unsupported", tail_args(cols=10, nb=0, D=64), BAD_ARG),
    # 3. the layout, with the codes of svg_varblock_attention_strided
    ("layout_heads_per_batch0", tail_args(lay=layout(hpb=0)), BAD_ARG),
    ("layout_heads_per_batch_not_dividing_H", tail_args(H=3, lay=layout(hpb=2)), BAD_ARG),
    ("layout_row_stride_below_D", tail_args(lay=layout(row=64)), BAD_ARG),
    ("layout_negative_batch_stride", tail_args(lay=layout(batch=-128)), BAD_ARG),
    ("layout_stride_not_multiple_of_8", tail_args(lay=layout(row=2 * 128 + 4)), UNSUPPORTED),
    ("layout_q_not_16_byte_aligned", tail_args(q=PH + 8, lay=layout()), UNSUPPORTED),
    ("layout_row_stride_2_23", tail_args(lay=layout(row=1 << 23)), UNSUPPORTED),
    ("layout_bad_arg_before_workspace", tail_args(lay=layout(row=64), nb=0), BAD_ARG),
    ("layout_unsupported_before_workspace", tail_args(lay=layout(row=2 * 128 + 4), nb=0), UNSUPPORTED),
    # 4. the workspace
    ("short_workspace", tail_args(nb=None), WORKSPACE),
    ("short_workspace_under_a_layout", tail_args(nb=None, lay=layout()), WORKSPACE),
    ("workspace_before_unsupported_D", tail_args(nb=None, D=64), WORKSPACE),
    ("workspace_before_unsupported_dtype", tail_args(nb=None, dtype=2), WORKSPACE),
    ("workspace_before_alignment", tail_args(nb=None, o=PC + 8), WORKSPACE),
    # 5. what the kernel does not cover
    ("D64", tail_args(D=64), UNSUPPORTED),
    ("D96", tail_args(D=96), UNSUPPORTED),
    ("dtype_f32", tail_args(dtype=2), UNSUPPORTED),
    ("KC4033", tail_args(KC=4033), UNSUPPORTED),
    ("KC4033_with_any_workspace", tail_args(KC=4033, nb=0), UNSUPPORTED),
    ("Sq_2_24", tail_args(Sq=1 << 24), UNSUPPORTED),
    ("kbar_not_16_byte_aligned", tail_args(kbar=PA + 8), UNSUPPORTED),
    ("o_not_16_byte_aligned", tail_args(o=PC + 2), UNSUPPORTED),
    ("q_not_16_byte_aligned", tail_args(q=PH + 8), UNSUPPORTED),
]


@pytest.mark.parametrize("a,expected", [c[1:] for c in MEANS_CASES], ids=[c[0] for c in MEANS_CASES])
def test_cluster_means_rejects(a, expected):
    host_only()
    assert nat.load().svg_cluster_means(*a) == expected


@pytest.mark.parametrize("a,expected", [c[1:] for c in TAIL_CASES], ids=[c[0] for c in TAIL_CASES])
def test_tail_rejects(a, expected):
    host_only()
    lib = nat.load()
    if a[18] is None:
        a = list(a)
        a[18] = int(lib.svg_centroid_tail_workspace_bytes(a[5], a[15], a[7])) - 1
        assert a[18] > 0
    assert lib.svg_centroid_tail_attention_lse(*a) == expected


# ---------------------------------------------------------------------------------------------------------
# the Python layer's refusals
# ---------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_the_device_is_looked_at():
    """CPU tensors: every ValueError comes before the device check, which is the RuntimeError of every libsvgattn wrapper"""
    bf, i32 = torch.bfloat16, torch.int32
    x, srt, cnt = torch.zeros(2, 64, 128, dtype=bf), torch.zeros(2, 64, dtype=i32), torch.zeros(2, 5, dtype=i32)
    with pytest.raises(ValueError, match="head_dim 64 / 128"):
        nat.cluster_means(torch.zeros(2, 64, 96, dtype=bf), srt, cnt)
    with pytest.raises(ValueError, match="bf16 / fp16"):
        nat.cluster_means(x.float(), srt, cnt)
    with pytest.raises(ValueError, match="int32"):
        nat.cluster_means(x, srt.long(), cnt)
    with pytest.raises(ValueError, match="sorted_idx"):
        nat.cluster_means(x, srt[:, :60], cnt)
    with pytest.raises(ValueError, match="counts"):
        nat.cluster_means(x, srt, cnt[:1])
    with pytest.raises(RuntimeError, match="GPU"):
        nat.cluster_means(x, srt, cnt)

    q, kb = torch.zeros(2, 100, 128, dtype=bf), torch.zeros(2, 7, 128, dtype=bf)
    bm, qs, ks = torch.zeros(2, 3, 9, dtype=torch.bool), torch.zeros(2, 3, dtype=i32), torch.zeros(2, 7, dtype=i32)
    tail = nat.centroid_tail_attention
    with pytest.raises(ValueError, match="head_dim 128"):
        tail(torch.zeros(2, 100, 64, dtype=bf), torch.zeros(2, 7, 64, dtype=bf), torch.zeros(2, 7, 64, dtype=bf), bm, qs, ks)
    with pytest.raises(ValueError, match="head_dim 128"):
        tail(q.float(), kb.float(), kb.float(), bm, qs, ks)
    with pytest.raises(ValueError, match="kbar, vbar"):
        tail(q, kb, kb[:, :6], bm, qs, ks)
    with pytest.raises(ValueError, match="dtype"):
        tail(q, kb, kb.half(), bm, qs, ks)
    with pytest.raises(ValueError, match="key clusters"):
        big = torch.zeros(2, 4033, 128, dtype=bf)
        tail(q, big, big, torch.zeros(2, 3, 4033, dtype=torch.bool), qs, torch.zeros(2, 4033, dtype=i32))
    with pytest.raises(ValueError, match="q_sizes"):
        tail(q, kb, kb, bm, qs.long(), ks)
    with pytest.raises(ValueError, match="k_sizes"):
        tail(q, kb, kb, bm, qs, ks[:, :6])
    with pytest.raises(ValueError, match="block_map"):
        tail(q, kb, kb, bm[:, :, :6], qs, ks)                       # fewer columns than key clusters
    with pytest.raises(ValueError, match="q_row_idx"):
        tail(q, kb, kb, bm, qs, ks, q_row_idx=torch.zeros(2, 100, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        tail(q, kb, kb, bm, qs, ks)                                 # a map with two further columns is fine


def test_processors_carry_the_switch_off():
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor

    for cls in (Hunyuan_SAPAttn_Processor2_0, WanAttn_SAPAttn_Processor, Cosmos_SAPAttn_Processor):
        assert cls.__dict__["centroid_tail"] is False


def test_core_refuses_adaptive_top_p_and_launches_without_an_lse_form():
    """on CPU tensors: the refusals come before the device is looked at, and before anything is stored"""
    from svg.models import _core

    geo = _core.Geometry(context_length=0, num_frame=6, frame_size=150, text_first=False)
    store, tps = _core.CentroidStore(), _core.TopPStore()
    q = torch.zeros(1, 2, 900, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="adaptive_top_p"):
        _core.svg2_sparse_attention(q, q, q, geo, store, 0, 4, 12, 0.6, 0.0, 2, 1, adaptive=_core.AdaptiveTopP(0.95), top_p_store=tps, centroid_tail=True)
    q64 = torch.zeros(1, 2, 900, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head_dim 128"):
        _core.svg2_sparse_attention(q64, q64, q64, geo, store, 0, 4, 12, 0.6, 0.0, 2, 1, centroid_tail=True)
    with pytest.raises(ValueError, match="160 block-rows"):
        _core.svg2_sparse_attention(q, q, q, geo, store, 0, 6, 12, 0.6, 0.0, 2, 1, centroid_tail=True)               # 900 < 160 * 6
    hy = _core.Geometry(context_length=60, num_frame=6, frame_size=150, text_first=False)
    qh = torch.zeros(1, 2, 960, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="160 block-rows"):
        _core.svg2_sparse_attention(qh, qh, qh, hy, store, 0, 5, 12, 0.6, 0.0, 2, 1, prompt_length=20, centroid_tail=True)   # 960 < 160 * (5 + 2)
    with pytest.raises(ValueError, match="fp8"):
        _core.svg2_sparse_attention(q.float(), q.float(), q.float(), geo, store, 0, 4, 12, 0.6, 0.0, 2, 1, centroid_tail=True)
    assert not tps.p and not store.q
    with pytest.raises(RuntimeError, match="GPU"):                                                                    # off: today's path, which asks for the GPU
        _core.svg2_sparse_attention(q, q, q, geo, store, 0, 6, 12, 0.6, 0.0, 2, 1, centroid_tail=False)


@pytest.mark.parametrize("mode", ["enable", "frame_shards", "token_shards"])
def test_centroid_tail_is_refused_under_every_distributed_mode(monkeypatch, mode):
    import os

    import torch.distributed as dist

    from svg import distributed as sd
    from svg.models import _core
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{38200 + os.getpid() % 2000}", rank=0, world_size=1)
    try:
        {"enable": sd.enable, "frame_shards": sd.enable_frame_shards, "token_shards": sd.enable_token_shards}[mode]()
        for name in ("all_reduce", "all_to_all_single", "all_gather_into_tensor", "broadcast", "all_gather"):
            monkeypatch.setattr(dist, name, lambda *a, _n=name, **k: pytest.fail(f"{_n}: a collective ran before the refusal"))
        geo = _core.Geometry(0, 4, 256)
        q = torch.zeros(1, 2, geo.seq_len, 128, dtype=torch.bfloat16)
        store = _core.CentroidStore()
        with pytest.raises(NotImplementedError, match="centroid_tail"):
            _core.svg2_sparse_attention(q, q, q, geo, store, 0, 4, 4, 0.9, 0.1, 2, 1, centroid_tail=True)
        with pytest.raises(NotImplementedError, match="centroid_tail"):
            _core.svg2_sparse_attention(q, q, q, geo, store, 0, 4, 4, 0.9, 0.1, 2, 1, _head_shard=(0, 2, 4), centroid_tail=True)
        t = torch.tensor([500.0])
        for cls in (WanAttn_SAPAttn_Processor, Hunyuan_SAPAttn_Processor2_0, Cosmos_SAPAttn_Processor):
            for attr, val in (("centroid_tail", True), ("num_frame", 4), ("frame_size", 256), ("context_length", 0), ("prompt_length", 0)):
                monkeypatch.setattr(cls, attr, val, raising=False)
            args = (q, q, q, t, 0, None) if cls is Hunyuan_SAPAttn_Processor2_0 else (q, q, q, t)
            if mode != "frame_shards":                     # (the SVG2 processors refuse that mode itself first, as before)
                with pytest.raises(NotImplementedError, match="centroid_tail"):
                    cls(0).attention_core_logic(*args)
        assert not store.q
    finally:
        sd.disable()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------
# float64 identities of the statement
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
def test_clusters_of_identical_rows_make_sparse_plus_tail_dense(dtype):
    """(a) n_c copies of (k_c, v_c) and ONE pseudo key of weight n_c are the same attention state: exp(s + ln n) = n exp(s)"""
    c = TC.exact_case(dtype)
    assert bool(c["bmap"].any(-1).all()) and bool((~c["bmap"]).any(-1).all())        # every map row selects a cluster and leaves one out
    assert int(c["k_sizes"].min()) >= 1 and int(c["k_sizes"].max()) <= 60 and (c["k_sizes"].sum(1) == TC.EX_S).all()
    ql = TC.labels_from_sizes(c["q_sizes"], None, TC.EX_S)
    kl = TC.labels_from_sizes(c["k_sizes"], None, TC.EX_S)
    st = TC.statement(c["q"], c["k"], c["v"], ql, kl, c["bmap"], c["kbar"], c["vbar"], c["k_sizes"])
    o_d, lse_d = TC.exact_reference(dtype)
    assert (st["o"] - o_d).abs().max().item() <= 1e-12 and (st["lse"] - lse_d).abs().max().item() <= 1e-12
    assert (st["lse_sparse"] < lse_d).all()                                            # (the tail is not idle in any row)


@pytest.mark.parametrize("KC", TC.KCS)
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
def test_merged_lse_lies_between_sparse_and_dense_under_exact_means(dtype, KC):
    """(b) Jensen: n_c exp(q . kbar_c) <= sum_{j in c} exp(q . k_j) when kbar_c is the exact mean — on every covered row"""
    c = TC.merge_case(KC, dtype, True)
    ql, kl = TC.labels_from_sizes(c["q_sizes"], c["q_idx"], TC.S), TC.labels_from_sizes(c["k_sizes"], c["kv_idx"], TC.S)
    kbar, vbar = TC.means64(c["k"], kl, KC), TC.means64(c["v"], kl, KC)                # exact: not rounded to the 16-bit type
    st = TC.statement(c["q"], c["k"], c["v"], ql, kl, c["bmap"], kbar, vbar, c["k_sizes"])
    _, lse_d = TC.dense64(c["q"], c["k"], c["v"])
    cov = st["covered"]
    assert cov.all()
    assert (st["lse_sparse"] <= st["lse"]).all() and (st["lse"] <= lse_d + 1e-12).all()
    rows_without_tail = TC.labels_from_sizes(c["q_sizes"], c["q_idx"], TC.S) == TC.ONES_ROW
    assert (st["lse_tail"][rows_without_tail] == TC.NINF).all() and torch.equal(st["o"][rows_without_tail], st["o_sparse"][rows_without_tail])
    assert (st["lse_sparse"][ql == TC.ZEROS_ROW] == TC.NINF).all() and torch.isfinite(st["lse"][ql == TC.ZEROS_ROW]).all()


@pytest.mark.parametrize("kind", sorted(TC.GEOMETRIES))
def test_premise_on_the_mixtures_of_the_layer_test(kind):
    """(c) on the inputs the GPU layer test runs, under a float64 Lloyd clustering and the oracle's top-p map: the statement's merged output
    is nearer to dense attention than its sparse output, and its kept mass is higher and at most 1"""
    from oracle import svg_oracle as O

    dtype = torch.bfloat16
    q, k, v = (x[0] for x in TC.layer_inputs(kind, 1, dtype))
    g = torch.Generator().manual_seed(5)
    ql = torch.stack([TC.lloyd64(q[h, :TC.V], TC.QC, 4, g) for h in range(TC.LAYER_H)])
    kl = torch.stack([TC.lloyd64(k[h, :TC.V], TC.KC_LAYER, 4, g) for h in range(TC.LAYER_H)])
    qc, kc = TC.means64(q[:, :TC.V], ql, TC.QC).to(dtype), TC.means64(k[:, :TC.V], kl, TC.KC_LAYER).to(dtype)
    qs = torch.stack([torch.bincount(ql[h], minlength=TC.QC) for h in range(TC.LAYER_H)])
    ks = torch.stack([torch.bincount(kl[h], minlength=TC.KC_LAYER) for h in range(TC.LAYER_H)])
    dmap = O.identify_dynamic_map(qc[None], kc[None], qs[None], ks[None], TC.TOP_P, TC.MIN_KC_RATIO, exact=True)[0]
    assert not bool(dmap.all())                                                        # the map drops something
    st = TC.layer_statement(kind, q, k, v, ql, kl, dmap, dtype)
    geo = TC.GEOMETRIES[kind]
    real = TC.V + geo["prompt"]
    o_d, lse_d = TC.dense64(q[:, :real], k[:, :real], v[:, :real])                     # dense over the video and the prompt
    vid = slice(0, TC.V)
    e_s, e_m = TC.rel_l2(st["o_sparse"][:, vid], o_d[:, vid]), TC.rel_l2(st["o"][:, vid], o_d[:, vid])
    kept_s, kept_m = (torch.exp(st[n][:, vid] - lse_d[:, vid]) for n in ("lse_sparse", "lse"))
    print(f"{kind}: rel. L2 sparse {e_s:.4f} -> merged {e_m:.4f}; kept mass {kept_s.mean().item():.4f} -> {kept_m.mean().item():.4f} "
          f"(max {kept_m.max().item():.6f}); density {float(O.density_calculation(dmap[None], qs[None], ks[None]).mean()):.3f}")
    assert e_m < e_s
    assert (kept_m >= kept_s).all() and kept_m.mean() > kept_s.mean()
