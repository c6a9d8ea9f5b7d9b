"""SVG2's per-head top-p without a GPU (include/svg_attn_adaptive_top_p.h: svg_identify_dynamic_map_per_head, svg_sample_dense_lse,
svg_top_p_update): the exports, the header and its place in svg_attn.h, the argument validation of the three entries — every check runs on
the host before any launch (rows that pass placeholder pointers are skipped where a GPU is visible, as in test_sample_rows_cpu.py) —, what
the Python wrappers refuse, the controller law as a float64 statement with its properties, what the oracle says about a per-head p, and the
semantics of TopPStore."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import adaptive_top_p_cases as AC
from oracle import svg_oracle as O
from svg import _native as nat
from svg import _probe, kmeans_utils
from svg.models import _core

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
S_ROWS = 1 << 24
NAN = float("nan")
ROOT = Path(__file__).resolve().parent.parent
ENTRIES = {"svg_identify_dynamic_map_per_head", "svg_sample_dense_lse_workspace_bytes", "svg_sample_dense_lse", "svg_top_p_update"}


def host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


def test_library_exports_the_entries():
    lib = nat.load()
    assert set(nat.ADAPTIVE_TOP_P_SIGNATURES) == ENTRIES
    others = (set(nat.SIGNATURES) | set(nat.SPARSE_LSE_SIGNATURES) | set(nat.SPARSE_F32_SIGNATURES) | set(nat.BAND_LSE_FORM_SIGNATURES)
              | set(nat.BAND_WINDOW_SIGNATURES) | set(nat.BAND_SHARD_SIGNATURES) | set(nat.BAND_SHARD_SWITCH_SIGNATURES)
              | set(nat.PROFILE_SHARD_SIGNATURES) | set(nat.SHARD_EXCHANGE_SIGNATURES) | set(nat.SAMPLE_ROWS_SIGNATURES))
    assert not ENTRIES & others
    for name, (res, args) in nat.ADAPTIVE_TOP_P_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    # the scalar entry's arguments with a pointer where it has the float
    scalar = list(nat.SIGNATURES["svg_identify_dynamic_map"][1])
    assert scalar[9] is C.c_float
    scalar[9] = C.c_void_p
    assert nat.ADAPTIVE_TOP_P_SIGNATURES["svg_identify_dynamic_map_per_head"][1] == scalar
    # svg_sample_dense_rows without v and o32
    rows = list(nat.SAMPLE_ROWS_SIGNATURES["svg_sample_dense_rows"][1])
    del rows[11], rows[2]
    assert nat.ADAPTIVE_TOP_P_SIGNATURES["svg_sample_dense_lse"][1] == rows
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_is_included_in_front_of_the_profile_shard_header_and_matches_the_signatures():
    main = (ROOT / "include" / "svg_attn.h").read_text()
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', main, flags=re.M)
    assert includes[-2:] == ["svg_attn_adaptive_top_p.h", "svg_attn_profile_shard.h"]
    src = (ROOT / "include" / "svg_attn_adaptive_top_p.h").read_text()
    assert "in this order" in src and "CALLER" in src
    assert re.search(r"NaN entry keeps EVERY block", src)                       # what a NaN threshold does is written down
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert {n for _, n, _ in protos} == ENTRIES

    def c_class(t):
        for pat, c in ((r"\*", "ptr"), (r"\bsize_t\b", "size"), (r"\b(int32_t|int)\b", "i32"), (r"\bfloat\b", "f32")):
            if re.search(pat, t):
                return c
        return "?" + t

    def py_class(a):
        if a is C.c_void_p or (isinstance(a, type) and issubclass(a, C._Pointer)):
            return "ptr"
        return {C.c_size_t: "size", C.c_int32: "i32", C.c_int: "i32", C.c_float: "f32"}.get(a, "?" + repr(a))

    for ret, name, params in protos:
        ps = [x.strip() for x in params.split(",") if x.strip()]
        want = [c_class(x if x.endswith("*") else re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", x)) for x in ps]
        res, args = nat.ADAPTIVE_TOP_P_SIGNATURES[name]
        assert [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


# ---------------------------------------------------------------------------------------------------------
# svg_identify_dynamic_map_per_head: the codes of the scalar entry, in its order, and a NULL top_p
# ---------------------------------------------------------------------------------------------------------
def map_args(qc=PH, kc=PH, ks=PH, out=PH, BH=4, QC=8, KC=12, D=128, dtype=0, top_p=PH, preserve=0):
    return [qc, kc, ks, out, BH, QC, KC, D, dtype, top_p, preserve, None]


MAP_CASES = [
    ("null_qc", map_args(qc=None), BAD_ARG),
    ("null_kc", map_args(kc=None), BAD_ARG),
    ("null_k_sizes", map_args(ks=None), BAD_ARG),
    ("null_out", map_args(out=None), BAD_ARG),
    ("null_top_p", map_args(top_p=None), BAD_ARG),
    ("BH0", map_args(BH=0), BAD_ARG),
    ("QC0", map_args(QC=0), BAD_ARG),
    ("KC_neg", map_args(KC=-1), BAD_ARG),
    ("null_top_p_before_KC", map_args(top_p=None, KC=4097), BAD_ARG),
    ("BH0_before_D", map_args(BH=0, D=96), BAD_ARG),
    ("KC4097", map_args(KC=4097), UNSUPPORTED),
    ("KC4097_second_form_D", map_args(KC=4097, D=96), UNSUPPORTED),
    ("D96_first_form", map_args(D=96), UNSUPPORTED),
    ("D96_second_form", map_args(D=96, KC=300), UNSUPPORTED),
    ("dtype_f32_first_form", map_args(dtype=2, KC=1100), UNSUPPORTED),
    ("dtype_f32_second_form", map_args(dtype=2, KC=1000), UNSUPPORTED),
]


@pytest.mark.parametrize("a,expected", [c[1:] for c in MAP_CASES], ids=[c[0] for c in MAP_CASES])
def test_identify_dynamic_map_per_head_rejects_like_the_scalar_entry(a, expected):
    host_only()
    lib = nat.load()
    assert lib.svg_identify_dynamic_map_per_head(*a) == expected
    if a[9] is not None:                                   # the same call with a float: the same code
        assert lib.svg_identify_dynamic_map(*(a[:9] + [0.5] + a[10:])) == expected


# ---------------------------------------------------------------------------------------------------------
# svg_sample_dense_lse: the table of svg_sample_dense_rows without v and o32
# ---------------------------------------------------------------------------------------------------------
def need(BH=4, R=8, S=300):
    return int(nat.load().svg_sample_dense_lse_workspace_bytes(BH, R, S))


def layout(H=2, S=300, D=128, **kw):
    t = nat.TensorStrides(H * S * D, S * D, D)
    lay = nat.AttnLayout(H, 0, t, t, t, t)
    for name, val in kw.items():
        setattr(lay, name, val)
    return lay


def lse_args(q=PH, k=PH, rows=PH, R=8, BH=4, S=300, D=128, dtype=0, valid_len=0, lse=PH, ws=PH, ws_bytes=None, lay=None):
    if ws_bytes is None:
        ws_bytes = 1 << 40
    return [q, k, rows, R, BH, S, D, dtype, 1.0, valid_len, lse, ws, ws_bytes, C.byref(lay) if lay is not None else None, None]


BAD_LAYOUT = dict(heads_per_batch=0)
LSE_CASES = [
    # 1. pointers and counts
    ("null_q", lse_args(q=None), BAD_ARG),
    ("null_k", lse_args(k=None), BAD_ARG),
    ("null_rows", lse_args(rows=None), BAD_ARG),
    ("null_lse", lse_args(lse=None), BAD_ARG),
    ("null_workspace", lse_args(ws=None), BAD_ARG),
    ("R0", lse_args(R=0), BAD_ARG),
    ("R65", lse_args(R=65), BAD_ARG),
    ("BH0", lse_args(BH=0), BAD_ARG),
    ("S0", lse_args(S=0), BAD_ARG),
    ("S_neg", lse_args(S=-5), BAD_ARG),
    ("null_before_S_rows", lse_args(lse=None, S=S_ROWS), BAD_ARG),
    ("R65_before_short_workspace", lse_args(R=65, ws_bytes=0), BAD_ARG),
    ("BH0_before_layout", lse_args(BH=0, lay=layout(**BAD_LAYOUT)), BAD_ARG),
    ("null_before_unsupported_D", lse_args(q=None, D=96), BAD_ARG),
    # 2. sizes the kernels cannot address
    ("S_rows", lse_args(S=S_ROWS), UNSUPPORTED),
    ("S_bytes_before_short_workspace", lse_args(S=1 << 23, D=256, ws_bytes=0), UNSUPPORTED),
    ("S_rows_before_short_workspace", lse_args(S=S_ROWS, ws_bytes=0), UNSUPPORTED),
    ("S_rows_before_layout", lse_args(S=S_ROWS, lay=layout(**BAD_LAYOUT)), UNSUPPORTED),
    # 3. workspace
    ("short_workspace", lse_args(ws_bytes=need() - 1), WORKSPACE),
    ("short_workspace_before_layout", lse_args(ws_bytes=need() - 1, lay=layout(**BAD_LAYOUT)), WORKSPACE),
    ("short_workspace_before_unsupported_D", lse_args(ws_bytes=need() - 1, D=96), WORKSPACE),
    ("short_workspace_before_dtype", lse_args(ws_bytes=need() - 1, dtype=2), WORKSPACE),
    ("misaligned_workspace", lse_args(ws=PH + 4), UNSUPPORTED),
    # 4. layout, as in svg_sample_mse_strided (q and k members)
    ("layout_heads0", lse_args(lay=layout(**BAD_LAYOUT)), BAD_ARG),
    ("layout_heads_not_dividing", lse_args(BH=3, lay=layout()), BAD_ARG),
    ("layout_row_stride_below_D", lse_args(lay=layout(q=nat.TensorStrides(2 * 300 * 128, 300 * 128, 64))), BAD_ARG),
    ("layout_row_stride_unaligned", lse_args(lay=layout(k=nat.TensorStrides(2 * 300 * 132, 300 * 132, 132))), UNSUPPORTED),
    ("layout_misaligned_k", lse_args(k=PH + 2, lay=layout()), UNSUPPORTED),
    ("layout_before_unsupported_D", lse_args(D=96, lay=layout(D=96, **BAD_LAYOUT)), BAD_ARG),
    ("layout_before_dtype", lse_args(dtype=2, lay=layout(**BAD_LAYOUT)), BAD_ARG),
    # 5. head_dim and dtype
    ("D96", lse_args(D=96), UNSUPPORTED),
    ("D256", lse_args(D=256), UNSUPPORTED),
    ("D0", lse_args(D=0), UNSUPPORTED),
    ("dtype_f32", lse_args(dtype=2), UNSUPPORTED),
    ("D96_with_layout", lse_args(D=96, lay=layout(D=96)), UNSUPPORTED),
]


@pytest.mark.parametrize("a,expected", [c[1:] for c in LSE_CASES], ids=[c[0] for c in LSE_CASES])
def test_sample_dense_lse_rejects_like_sample_dense_rows(a, expected):
    host_only()
    lib = nat.load()
    assert lib.svg_sample_dense_lse(*a) == expected
    if a[12] == 1 << 40 and a[1] in (None, PH):            # the same call of svg_sample_dense_rows (v = k, an o32): the same code
        assert lib.svg_sample_dense_rows(*(a[:2] + [a[1]] + a[2:10] + [PH] + a[10:])) == expected


def test_lse_workspace_bytes():
    f = nat.load().svg_sample_dense_lse_workspace_bytes
    assert f(0, 8, 300) == 0 and f(4, 0, 300) == 0 and f(4, 8, 0) == 0
    for name, values in dict(BH=list(range(1, 40)) + [255, 256, 257, 511, 512, 513, 600], R=list(range(1, 65)),
                             S=[1, 63, 64, 65, 70, 300, 790, 4096, 4097, 4100, 75600, (1 << 24) - 1]).items():
        for S in (70, 4100, 119056):
            got = [int(f(*[{"BH": 4, "R": 8, "S": S, name: x}[key] for key in ("BH", "R", "S")])) for x in values]
            assert all(g > 0 and g % 16 == 0 for g in got) and got == sorted(got), (name, S, got)
    for BH, S in [(1, 70), (3, 790), (3, 4100), (48, 119056), (40, 75600), (600, 4100)]:   # (m, l) of every chunk of every row
        chunks = max(1, min(512 // BH, (S + 63) // 64, 64))
        assert int(f(BH, 17, S)) >= BH * chunks * 17 * 2 * 4


# ---------------------------------------------------------------------------------------------------------
# svg_top_p_update
# ---------------------------------------------------------------------------------------------------------
def upd_args(ls=PH, rows=PH, ld=PH, R=8, BH=4, S=300, target=0.9, gu=1.0, gd=0.25, band=0.02, p_min=0.1, p_max=1.0, kept=PH, top_p=PH):
    return [ls, rows, ld, R, BH, S, target, gu, gd, band, p_min, p_max, kept, top_p, None]


UPD_CASES = [
    ("null_lse_sparse", upd_args(ls=None)), ("null_rows", upd_args(rows=None)), ("null_lse_dense", upd_args(ld=None)),
    ("null_kept", upd_args(kept=None)), ("null_top_p", upd_args(top_p=None)),
    ("R0", upd_args(R=0)), ("R65", upd_args(R=65)), ("R_neg", upd_args(R=-1)), ("BH0", upd_args(BH=0)), ("S0", upd_args(S=0)),
    ("S_neg", upd_args(S=-3)),
    ("gain_up_neg", upd_args(gu=-0.5)), ("gain_up_nan", upd_args(gu=NAN)), ("gain_down_neg", upd_args(gd=-1e-9)),
    ("gain_down_nan", upd_args(gd=NAN)), ("band_neg", upd_args(band=-0.01)), ("band_nan", upd_args(band=NAN)),
    ("p_min_neg", upd_args(p_min=-0.1)), ("p_max_above_1", upd_args(p_max=1.5)), ("p_min_above_p_max", upd_args(p_min=0.8, p_max=0.5)),
    ("p_min_nan", upd_args(p_min=NAN)), ("p_max_nan", upd_args(p_max=NAN)),
]


@pytest.mark.parametrize("a", [c[1] for c in UPD_CASES], ids=[c[0] for c in UPD_CASES])
def test_top_p_update_rejects(a):
    host_only()
    assert nat.load().svg_top_p_update(*a) == BAD_ARG


# ---------------------------------------------------------------------------------------------------------
# the Python wrappers
# ---------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_on_cpu_tensors():
    q = torch.zeros(1, 2, 70, 128, dtype=torch.bfloat16)
    ok = torch.tensor([0, 69, 5, 5])
    with pytest.raises(RuntimeError, match="GPU"):            # like every native op: no CPU fallback
        _probe.sample_dense_lse(q, q, ok)
    for bad in (torch.tensor([0, 70]), torch.tensor([-1, 3])):
        with pytest.raises(ValueError, match=r"outside \[0, 70\)"):
            _probe.sample_dense_lse(q, q, bad)
    with pytest.raises(ValueError, match="1 to 64"):
        _probe.sample_dense_lse(q, q, torch.zeros(65, dtype=torch.int64))
    with pytest.raises(ValueError, match="int64"):
        _probe.sample_dense_lse(q, q, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="one shape"):
        _probe.sample_dense_lse(q, q[:, :1], ok)
    # the map: a tensor p of the wrong size or type is refused before the device is looked at; a right one needs the GPU
    qc, kc, sz = torch.zeros(1, 2, 4, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 6, 128, dtype=torch.bfloat16), torch.ones(1, 2, 6)
    for bad in (torch.zeros(3), torch.zeros(1, 2, dtype=torch.float64)):
        with pytest.raises(ValueError, match="float32"):
            kmeans_utils.identify_dynamic_map(qc, kc, None, sz, bad)
    with pytest.raises(AssertionError, match="GPU"):
        kmeans_utils.identify_dynamic_map(qc, kc, None, sz, torch.full((1, 2), 0.5))
    with pytest.raises(ValueError, match="uint8"):
        nat.identify_dynamic_map_per_head(qc[0], kc[0], sz[0].int(), torch.zeros(2), 0, torch.zeros(2, 4, 5, dtype=torch.uint8))
    # the update
    ls, ld, p, kept = torch.zeros(2, 70), torch.zeros(2, 4), torch.full((2,), 0.5), torch.zeros(2)
    with pytest.raises(RuntimeError, match="GPU"):
        nat.top_p_update(ls, ok, ld, p, kept, 0.9, 1.0, 0.25, 0.02, 0.1, 1.0)
    with pytest.raises(ValueError, match="1 to 64"):
        nat.top_p_update(ls, torch.zeros(65, dtype=torch.int64), ld, p, kept, 0.9, 1.0, 0.25, 0.02, 0.1, 1.0)
    with pytest.raises(ValueError, match="lse_dense"):
        nat.top_p_update(ls, ok, ld[:, :3], p, kept, 0.9, 1.0, 0.25, 0.02, 0.1, 1.0)
    with pytest.raises(ValueError, match="kept"):
        nat.top_p_update(ls, ok, ld, p, torch.zeros(3), 0.9, 1.0, 0.25, 0.02, 0.1, 1.0)
    with pytest.raises(ValueError, match="lse_sparse"):
        nat.top_p_update(ls.double(), ok, ld, p, kept, 0.9, 1.0, 0.25, 0.02, 0.1, 1.0)
    with pytest.raises(ValueError, match="contiguous"):       # a strided view is refused, not read wrongly (the kernel indexes h * S + row)
        nat.top_p_update(torch.zeros(2, 140)[:, ::2], ok, ld, p, kept, 0.9, 1.0, 0.25, 0.02, 0.1, 1.0)


def test_the_allocating_wrappers_are_not_public_functions_of_the_native_module():
    """tests/test_gpu_poison.py keeps a row per public ALLOCATING wrapper of svg/_native.py: the two bindings there take their outputs, the
    allocations are in svg/kmeans_utils.py and svg/_adaptive.py, through _native.empty"""
    assert not hasattr(nat, "sample_dense_lse") and _probe.sample_dense_lse.__module__ == "svg._adaptive"
    src = (ROOT / "sparse-videogen_amd" / "svg" / "_adaptive.py").read_text()
    assert src.count("_native.empty(") == 2 and "torch.empty" not in src
    import ast
    import inspect

    for fn in (nat.identify_dynamic_map_per_head, nat.top_p_update):
        called = {c.func.id for c in ast.walk(ast.parse(inspect.getsource(fn))) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
        assert not called & {"empty", "empty_like"}


def test_adaptive_top_p_checks_its_arguments_and_documents_untuned_gains():
    a = _core.AdaptiveTopP(0.95)
    assert (a.gain_up, a.gain_down, a.band, a.p_min, a.p_max) == (1.0, 0.25, 0.02, 0.1, 1.0)
    assert "UNTUNED" in _core.AdaptiveTopP.__doc__
    for kw in (dict(gain_up=-1), dict(gain_down=NAN), dict(band=-0.1), dict(p_min=0.9, p_max=0.5), dict(p_max=1.2), dict(p_min=NAN),
               dict(rows=0), dict(rows=65)):
        with pytest.raises(ValueError):
            _core.AdaptiveTopP(0.95, **kw)


def test_svg2_sparse_attention_refuses_before_anything_runs():
    """no LSE form: ValueError (head_dim 64; S < 160 block-rows) — on CPU tensors: the refusal comes before the device is looked at"""
    geo = _core.Geometry(context_length=0, num_frame=6, frame_size=150, text_first=False)
    store, tps = _core.CentroidStore(), _core.TopPStore()
    ad = _core.AdaptiveTopP(0.95)
    q64 = torch.zeros(1, 2, 900, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="head_dim 128"):
        _core.svg2_sparse_attention(q64, q64, q64, geo, store, 0, 4, 12, 0.6, 0.0, 2, 1, adaptive=ad, top_p_store=tps)
    q = torch.zeros(1, 2, 900, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="160 block-rows"):
        _core.svg2_sparse_attention(q, q, q, geo, store, 0, 6, 12, 0.6, 0.0, 2, 1, adaptive=ad, top_p_store=tps)   # 900 < 160 * 6
    with pytest.raises(ValueError, match="top_p_store"):
        _core.svg2_sparse_attention(q, q, q, geo, store, 0, 4, 12, 0.6, 0.0, 2, 1, adaptive=ad)
    assert not tps.p and not store.q


@pytest.mark.parametrize("mode", ["enable", "frame_shards", "token_shards"])
def test_adaptive_top_p_is_refused_under_every_distributed_mode(monkeypatch, mode):
    import os

    import torch.distributed as dist

    from svg import distributed as sd
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{38500 + os.getpid() % 2000}", rank=0, world_size=1)
    try:
        {"enable": sd.enable, "frame_shards": sd.enable_frame_shards, "token_shards": sd.enable_token_shards}[mode]()
        for name in ("all_reduce", "all_to_all_single", "all_gather_into_tensor", "broadcast", "all_gather"):
            monkeypatch.setattr(dist, name, lambda *a, _n=name, **k: pytest.fail(f"{_n}: a collective ran before the refusal"))
        geo = _core.Geometry(0, 2, 64)
        q = torch.zeros(1, 2, geo.seq_len, 128, dtype=torch.bfloat16)
        ad, tps = _core.AdaptiveTopP(0.95), _core.TopPStore()
        with pytest.raises(NotImplementedError, match="adaptive_top_p"):
            _core.svg2_sparse_attention(q, q, q, geo, _core.CentroidStore(), 0, 4, 4, 0.9, 0.1, 2, 1, adaptive=ad, top_p_store=tps)
        t = torch.tensor([500.0])
        for cls in (WanAttn_SAPAttn_Processor, Hunyuan_SAPAttn_Processor2_0):
            for attr, val in (("adaptive_top_p", ad), ("num_frame", 2), ("frame_size", 64), ("context_length", 0), ("prompt_length", 0)):
                monkeypatch.setattr(cls, attr, val, raising=False)
            args = (q, q, q, t, 0, None) if cls is Hunyuan_SAPAttn_Processor2_0 else (q, q, q, t)
            if mode != "frame_shards":                     # (the SVG2 processors refuse that mode itself first, as before)
                with pytest.raises(NotImplementedError, match="adaptive_top_p"):
                    cls(0).attention_core_logic(*args)
        assert not tps.p
    finally:
        sd.disable()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------
# the controller law
# ---------------------------------------------------------------------------------------------------------
def test_controller_law_properties():
    kw = dict(target=0.9, gain_up=2.0, gain_down=0.5, band=0.05, p_min=0.2, p_max=0.95)
    p = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5])
    kept = np.array([0.7, 0.9, 0.93, 0.95, 0.99, 0.9500001])
    new = AC.law(p, kept, **kw)
    assert new[0] == pytest.approx(0.5 + 2.0 * 0.2) and new[0] > p[0]            # kept < target raises p
    assert new[1] == 0.5 and new[2] == 0.5                                          # nothing moves inside the band ...
    assert new[3] == pytest.approx(0.5, abs=1e-15)                                  # ... its far edge included
    assert new[4] == pytest.approx(0.5 + 0.5 * (0.9 - 0.99 + 0.05)) and new[4] < 0.5    # above the band: lowered, by the slow gain
    assert new[5] < 0.5 and 0.5 - new[5] < 1e-7                                     # continuous at the band's edge
    # clamps at both ends
    assert AC.law([0.9], [0.1], **kw)[0] == 0.95 and AC.law([0.21], [1.0], **dict(kw, gain_down=5.0))[0] == 0.2
    # kept not finite: unchanged, even outside the clamps
    for bad in (NAN, math.inf, -math.inf):
        assert AC.law([0.5, 0.05], [bad, bad], **kw).tolist() == [0.5, 0.05]
    # zero gains: a finite kept moves nothing inside the clamps
    assert AC.law(p, kept, **dict(kw, gain_up=0.0, gain_down=0.0)).tolist() == p.tolist()
    # monotone in kept: a head that kept less never ends with a smaller p
    ks = np.linspace(0, 1, 101)
    out = AC.law(np.full(101, 0.5), ks, **kw)
    assert (np.diff(out) <= 1e-15).all()


def test_kept_mass_statement():
    ls = np.array([[0.0, -1.0, -np.inf, 2.0], [np.nan, 0.0, 0.0, 0.0]])
    rows = [3, 0, 2, 2, 0]
    ld = np.array([[2.0, 0.5, 1.0, 1.0, 0.0], [0.0] * 5])
    k = AC.kept_mass(ls, rows, ld)
    assert k[0] == pytest.approx((1.0 + math.exp(-0.5) + 0 + 0 + 1.0) / 5) and math.isnan(k[1])


# ---------------------------------------------------------------------------------------------------------
# the oracle on a per-head p
# ---------------------------------------------------------------------------------------------------------
def clustered_centroids(B, H, QC, KC, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    qc = (torch.randn(B, H, QC, D, generator=g) * 1.5).to(dtype)
    kc = (torch.randn(B, H, KC, D, generator=g) * 1.5).to(dtype)
    return qc, kc, torch.randint(1, 50, (B, H, QC), generator=g), torch.randint(1, 50, (B, H, KC), generator=g)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_map_is_monotone_in_p(dtype):
    qc, kc, qs, ks = clustered_centroids(1, 3, 20, 40, 64, dtype, 5)
    ps = [0.0, 0.1, 0.3, 0.5, 0.5001, 0.7, 0.9, 0.99, 1.0]
    maps = [O.identify_dynamic_map(qc, kc, qs, ks, p, exact=True) for p in ps]
    for a, b in zip(maps, maps[1:]):
        assert bool((a <= b).all())                                      # p1 <= p2: map(p1) is a subset of map(p2)
    assert bool((maps[0].sum(-1) == 1).all()) and maps[-1].sum() > maps[0].sum()   # p = 0 keeps the first block of every row
    # a NaN keeps everything: every compare is false
    assert bool(O.identify_dynamic_map(qc, kc, qs, ks, NAN, exact=True).all())


def test_a_broadcast_p_tensor_skips_the_rounding_of_p():
    """the per-head oracle is a loop over heads with a Python float: four equal blocks of probability 0.25, cumulative sums 0.25, 0.5, 0.75,
    1 in bf16; p = 0.4995 rounds to bf16 0.5 — 0.5 > 0.5 is false and the third block stays — while an fp32 TENSOR p promotes the compare
    to fp32, where 0.5 > 0.4995 drops it"""
    qc = torch.zeros(1, 1, 1, 64, dtype=torch.bfloat16)
    kc = torch.zeros(1, 1, 4, 64, dtype=torch.bfloat16)
    qs, ks = torch.ones(1, 1, 1, dtype=torch.int64), torch.ones(1, 1, 4, dtype=torch.int64)
    p = 0.4995
    assert float(torch.tensor(p).to(torch.bfloat16)) == 0.5
    loop = AC.per_head_map(qc, kc, qs, ks, [p])
    promoted = O.identify_dynamic_map(qc, kc, qs, ks, torch.full((1, 1, 1, 1), p), exact=True)
    assert loop[0, 0, 0].tolist() == [True, True, True, False] and promoted[0, 0, 0].tolist() == [True, True, False, False]
    # heads with different p: the loop gives each head its scalar's map
    qc, kc, qs, ks = clustered_centroids(1, 3, 5, 12, 64, torch.bfloat16, 9)
    ps = [0.2, 0.9, 0.5]
    m = AC.per_head_map(qc, kc, qs, ks, ps)
    for h in range(3):
        assert torch.equal(m[:, h], O.identify_dynamic_map(qc, kc, qs, ks, ps[h], exact=True)[:, h])


# ---------------------------------------------------------------------------------------------------------
# TopPStore
# ---------------------------------------------------------------------------------------------------------
def test_top_p_store():
    s = _core.TopPStore()
    assert not s.has(3)
    t = s.get(3, 6, 0.6, "cpu")
    assert t.dtype == torch.float32 and t.shape == (6,) and t.tolist() == [pytest.approx(0.6)] * 6 and s.has(3) and s.has(3, 6)
    t[2] = 0.9
    s.kept[3] = torch.zeros(6)
    assert s.get(3, 6, 0.1, "cpu") is t and s.get(3, 6, 0.1, "cpu")[2] == pytest.approx(0.9)   # the same size: the state, not the initial value
    assert 3 in s.kept
    u = s.get(3, 12, 0.3, "cpu")                                   # another cfg * H: the layer starts again
    assert u is not t and u.tolist() == [pytest.approx(0.3)] * 12 and 3 not in s.kept and not s.has(3, 6)
    s.get(4, 6, 0.5, "cpu")
    s.clear()
    assert not s.has(3) and not s.has(4) and not s.kept


def test_processors_carry_the_option_and_the_store():
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor

    for cls in (WanAttn_SAPAttn_Processor, Cosmos_SAPAttn_Processor, Hunyuan_SAPAttn_Processor2_0):
        assert cls.adaptive_top_p is None and cls.quality_log is None
    for cls in (WanAttn_SAPAttn_Processor, Cosmos_SAPAttn_Processor):
        p = cls(0)
        p.top_p_store.get(0, 4, 0.5, "cpu")
        p.reset_state()
        assert isinstance(p.top_p_store, _core.TopPStore) and not p.top_p_store.has(0)
    Hunyuan_SAPAttn_Processor2_0.top_p_store.get(7, 4, 0.5, "cpu")
    Hunyuan_SAPAttn_Processor2_0.reset_state()
    assert not Hunyuan_SAPAttn_Processor2_0.top_p_store.has(7)
