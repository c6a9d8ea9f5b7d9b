"""SVG1's per-head band width without a GPU (include/svg_attn_adaptive_band.h: svg_band_attention_per_head_lse,
svg_band_attention_switch_per_head_lse, svg_band_width_update): the exports, the header and its place in svg_attn.h, the argument validation of
the three entries — every check runs on the host before any launch (rows that pass placeholder pointers are skipped where a GPU is visible, as
in test_adaptive_top_p_cpu.py) —, what the Python wrappers refuse and how they plan layouts, the controller law as an fp32 and a float64
statement, AdaptiveBand and its congruent bounds, BandStore, and every refusal of the core functions and the processors, raised before a
stand-in library sees a call."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import adaptive_band_cases as BC
from svg import _adaptive_band as ab
from svg import _native as nat
from svg.models import _core

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2   # include/svg_attn.h
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
NAN = float("nan")
ROOT = Path(__file__).resolve().parent.parent
ENTRIES = {"svg_band_attention_per_head_lse", "svg_band_attention_switch_per_head_lse", "svg_band_width_update"}


def host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


def test_library_exports_the_entries():
    lib = nat.load()
    assert set(nat.ADAPTIVE_BAND_ENTRIES) == ENTRIES
    others = set()
    for name in dir(nat):
        if name.endswith("SIGNATURES") and isinstance(getattr(nat, name), dict):
            others |= set(getattr(nat, name))
    assert not ENTRIES & others
    for name, (res, args) in nat.ADAPTIVE_BAND_ENTRIES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    # svg_band_attention_lse with the band vector behind the mask; the switch entry with it behind the flag
    one = list(nat.SPARSE_LSE_SIGNATURES["svg_band_attention_lse"][1])
    one.insert(11, C.c_void_p)
    assert nat.ADAPTIVE_BAND_ENTRIES["svg_band_attention_per_head_lse"][1] == one
    sw = list(nat.BAND_LSE_FORM_SIGNATURES["svg_band_attention_switch_lse"][1])
    perm = sw.pop(11)
    sw.insert(13, perm)
    sw.insert(13, C.c_void_p)
    assert nat.ADAPTIVE_BAND_ENTRIES["svg_band_attention_switch_per_head_lse"][1] == sw
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_is_included_and_matches_the_signatures():
    main = (ROOT / "include" / "svg_attn.h").read_text()
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', main, flags=re.M)
    assert includes[-3:] == ["svg_attn_adaptive_band.h", "svg_attn_adaptive_top_p.h", "svg_attn_profile_shard.h"]
    src = (ROOT / "include" / "svg_attn_adaptive_band.h").read_text()
    assert "in the order of svg_band_attention_lse" in src and "clamp is done in the kernel" in src
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
        res, args = nat.ADAPTIVE_BAND_ENTRIES[name]
        assert [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


def test_the_controller_file_is_built_without_contraction():
    import importlib.util

    spec = importlib.util.spec_from_file_location("svg_build_for_test", ROOT / "sparse-videogen_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert {"kept_mass_control.hip", "dynmap.hip"} <= mod.STRICT_FP
    csrc = ROOT / "sparse-videogen_amd" / "csrc"                   # both controllers live in that one file
    assert (csrc / "kept_mass_control.hip").exists() and not (csrc / "band_width_control.hip").exists() and not (csrc / "top_p_control.hip").exists()


# ---------------------------------------------------------------------------------------------------------
# the attention entries: the codes of svg_band_attention_lse / svg_band_attention_switch_lse, in their order
# ---------------------------------------------------------------------------------------------------------
S0 = 300


def mask(real=S0, band=64, cl=0, ch=0, rl=0, rh=0):
    return nat.BandMask(real, band, cl, ch, rl, rh)


def layout(H=2, S=S0, D=128, **kw):
    t = nat.TensorStrides(H * S * D, S * D, D)
    lay = nat.AttnLayout(H, 0, t, t, t, t)
    for name, val in kw.items():
        obj, field = name.split("_")
        setattr(getattr(lay, obj), field, val)
    return lay


def attn_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=4, S=S0, D=128, dtype=0, m=None, band=PH, perm=None, lay=None, alt="ok", flag=PH):
    m = mask() if m is None else m
    alt = mask(band=S0 + 1) if alt == "ok" else alt
    head = [q, k, v, o, lse, BH, S, D, dtype, 0.1, None if m == "null" else C.byref(m)]
    tail = [None if perm is None else C.byref(perm), None if lay is None else C.byref(lay), None]
    return head + [band] + tail, head + [None if alt is None else C.byref(alt), flag, band] + tail


BAD_PERM = nat.PermDesc(PH, 0, 0, 10)                              # flags with no frames
ATTN_CASES = [
    ("null_q", dict(q=None), BAD_ARG), ("null_k", dict(k=None), BAD_ARG), ("null_v", dict(v=None), BAD_ARG), ("null_o", dict(o=None), BAD_ARG),
    ("null_lse", dict(lse=None), BAD_ARG), ("null_band", dict(band=None), BAD_ARG), ("null_mask", dict(m="null"), BAD_ARG),
    ("BH0", dict(BH=0), BAD_ARG), ("S0", dict(S=0), BAD_ARG),
    ("null_band_before_D", dict(band=None, D=64), BAD_ARG), ("null_lse_before_dtype", dict(lse=None, dtype=2), BAD_ARG),
    ("mask_band_neg", dict(m=mask(band=-1)), BAD_ARG),                                   # mask->band is still validated
    ("mask_band_above_S_plus_1", dict(m=mask(band=S0 + 2)), BAD_ARG),
    ("mask_real_len", dict(m=mask(real=S0 + 1)), BAD_ARG), ("mask_colfull", dict(m=mask(cl=5, ch=4)), BAD_ARG),
    ("perm_without_frames", dict(perm=BAD_PERM), BAD_ARG),
    ("bad_mask_before_D", dict(m=mask(band=-1), D=64), BAD_ARG),
    ("S_2pow24", dict(S=1 << 24, m=mask(real=0)), UNSUPPORTED),
    ("layout_heads", dict(lay=layout(H=3)), BAD_ARG), ("layout_row_below_D", dict(lay=layout(q_row=64)), BAD_ARG),
    ("layout_row_misaligned", dict(lay=layout(k_row=132)), UNSUPPORTED), ("layout_before_D", dict(lay=layout(H=3), D=64), BAD_ARG),
    ("D64", dict(D=64), UNSUPPORTED), ("D96", dict(D=96), UNSUPPORTED), ("dtype_f32", dict(dtype=2), UNSUPPORTED),
]
SWITCH_ONLY = [
    ("null_alt", dict(alt=None), BAD_ARG), ("null_flag", dict(flag=None), BAD_ARG), ("null_alt_before_bad_mask", dict(alt=None, m=mask(band=-1)), BAD_ARG),
    ("alt_band", dict(alt=mask(band=S0 + 2)), BAD_ARG), ("alt_before_D", dict(alt=mask(real=-1), D=64), BAD_ARG),
]


@pytest.mark.parametrize("kw,expected", [c[1:] for c in ATTN_CASES], ids=[c[0] for c in ATTN_CASES])
def test_attention_entries_reject_like_the_single_mask_entries(kw, expected):
    host_only()
    lib = nat.load()
    one, sw = attn_args(**kw)
    assert lib.svg_band_attention_per_head_lse(*one) == expected
    assert lib.svg_band_attention_switch_per_head_lse(*sw) == expected
    if kw.get("band", PH) is not None and "BH" not in kw or kw.get("BH") == 0:           # the same call without the vector: the same code
        assert lib.svg_band_attention_lse(*(one[:11] + one[12:])) == expected
        assert lib.svg_band_attention_switch_lse(*(sw[:11] + [sw[14], sw[11], sw[12]] + sw[15:])) == expected


@pytest.mark.parametrize("kw,expected", [c[1:] for c in SWITCH_ONLY], ids=[c[0] for c in SWITCH_ONLY])
def test_switch_entry_rejects(kw, expected):
    host_only()
    assert nat.load().svg_band_attention_switch_per_head_lse(*attn_args(**kw)[1]) == expected


# ---------------------------------------------------------------------------------------------------------
# svg_band_width_update
# ---------------------------------------------------------------------------------------------------------
def upd_args(ls=PH, rows=PH, ld=PH, R=8, BH=4, S=S0, target=0.9, gu=1.0, gd=0.25, dead=0.02, quantum=128, bmin=1, bmax=S0 + 1, skip=None,
             kept=PH, band=PH):
    return [ls, rows, ld, R, BH, S, target, gu, gd, dead, quantum, bmin, bmax, skip, kept, band, None]


UPD_CASES = [
    ("null_lse_sparse", upd_args(ls=None)), ("null_rows", upd_args(rows=None)), ("null_lse_dense", upd_args(ld=None)),
    ("null_kept", upd_args(kept=None)), ("null_band", upd_args(band=None)),
    ("R0", upd_args(R=0)), ("R65", upd_args(R=65)), ("R_neg", upd_args(R=-1)), ("BH0", upd_args(BH=0)), ("S0", upd_args(S=0)),
    ("S_neg", upd_args(S=-3)),
    ("gain_up_neg", upd_args(gu=-0.5)), ("gain_up_nan", upd_args(gu=NAN)), ("gain_down_neg", upd_args(gd=-1e-9)),
    ("gain_down_nan", upd_args(gd=NAN)), ("dead_neg", upd_args(dead=-0.01)), ("dead_nan", upd_args(dead=NAN)),
    ("quantum0", upd_args(quantum=0)), ("quantum_neg", upd_args(quantum=-128)), ("quantum4097", upd_args(quantum=4097)),
    ("band_min0", upd_args(bmin=0)), ("band_min_neg", upd_args(bmin=-5)), ("band_min_above_max", upd_args(bmin=200, bmax=100)),
    ("band_max_above_S_plus_1", upd_args(bmax=S0 + 2)), ("band_max_int_max", upd_args(bmax=2 ** 31 - 1)),
]


@pytest.mark.parametrize("a", [c[1] for c in UPD_CASES], ids=[c[0] for c in UPD_CASES])
def test_band_width_update_rejects(a):
    host_only()
    assert nat.load().svg_band_width_update(*a) == BAD_ARG


# ---------------------------------------------------------------------------------------------------------
# the Python wrappers
# ---------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_before_the_device_is_looked_at():
    q = torch.zeros(1, 2, 70, 128, dtype=torch.bfloat16)
    band = torch.full((2,), 5, dtype=torch.int32)
    m, flag = mask(70, 5), torch.zeros(1, dtype=torch.int32)
    q64 = torch.zeros(1, 2, 70, 64, dtype=torch.bfloat16)
    for call in (lambda x, b: ab.band_attention_per_head(x, x, x, m, b), lambda x, b: ab.band_attention_switch_per_head(x, x, x, m, m, flag, b)):
        with pytest.raises(ValueError, match="head_dim 128"):
            call(q64, band)
        with pytest.raises(ValueError, match="head_dim 128"):
            call(q.float(), band)
        with pytest.raises(RuntimeError, match="GPU"):            # like every native op: no CPU fallback
            call(q, band)
    ls, ld, kept, rows = torch.zeros(2, 70), torch.zeros(2, 4), torch.zeros(2), torch.tensor([0, 69, 5, 5])
    args = (0.9, 1.0, 0.25, 0.02, 128, 1, 71)
    with pytest.raises(RuntimeError, match="GPU"):
        nat.band_width_update(ls, rows, ld, band, kept, *args)
    with pytest.raises(ValueError, match="1 to 64"):
        nat.band_width_update(ls, torch.zeros(65, dtype=torch.int64), ld, band, kept, *args)
    with pytest.raises(ValueError, match="int32"):
        nat.band_width_update(ls, rows, ld, band.float(), kept, *args)
    with pytest.raises(ValueError, match="lse_dense"):
        nat.band_width_update(ls, rows, ld[:, :3], band, kept, *args)
    with pytest.raises(ValueError, match="kept"):
        nat.band_width_update(ls, rows, ld, band, torch.zeros(3), *args)
    with pytest.raises(ValueError, match="lse_sparse"):
        nat.band_width_update(ls.double(), rows, ld, band, kept, *args)
    # strided views are refused, not read wrongly: lse_sparse, lse_dense and kept as band (the device check refuses the rest)
    with pytest.raises(ValueError, match="contiguous"):
        nat.band_width_update(torch.zeros(2, 140)[:, ::2], rows, ld, band, kept, *args)
    with pytest.raises(ValueError, match="contiguous"):
        nat.band_width_update(ls, rows, torch.zeros(2, 8)[:, ::2], band, kept, *args)
    with pytest.raises(ValueError, match="contiguous"):
        nat.band_width_update(ls, rows, ld, band, torch.zeros(4)[::2], *args)
    with pytest.raises(ValueError, match="contiguous"):
        nat.band_width_update(ls, rows, ld, torch.zeros(4, dtype=torch.int32)[::2], kept, *args)
    with pytest.raises(ValueError, match="skip_flag"):
        nat.band_width_update(ls, rows, ld, band, kept, *args, skip_flag=torch.zeros(1))


class FakeLib:
    """records the per-head attention calls instead of launching them"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


def test_allocating_wrappers_plan_layouts_and_allocate_through_the_switch(monkeypatch):
    """contiguous tensors: a NULL layout; views of a fused projection: a layout and, asked for, a token-major o; lse contiguous [B, H, S] either
    way.  The allocating wrappers live outside svg/_native.py (tests/test_gpu_poison.py keeps a row per public allocating wrapper there) and
    allocate through _native.empty / _layout_plan alone."""
    fake = FakeLib()
    monkeypatch.setattr(nat, "load", lambda strict=True: fake)
    monkeypatch.setattr(nat, "_gpu", lambda *ts: None)
    monkeypatch.setattr(nat, "_dev", lambda *ts: None)
    monkeypatch.setattr(nat, "_stream", lambda: 0)
    H, S, D = 2, 70, 128
    band, flag, m = torch.full((H,), 5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), mask(70, 5)
    q = torch.zeros(1, H, S, D, dtype=torch.bfloat16)
    o, lse = ab.band_attention_per_head(q, q, q, m, band)
    name, a = fake.calls[-1]
    assert name == "svg_band_attention_per_head_lse" and len(a) == len(nat.ADAPTIVE_BAND_ENTRIES[name][1]) and a[13] is None
    assert a[11] == band.data_ptr() and a[3] == o.data_ptr() and a[4] == lse.data_ptr() and o.is_contiguous() and lse.shape == (1, H, S)
    qkv = torch.zeros(1, S, 3 * H * D, dtype=torch.bfloat16)
    qv, kv, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    o, lse = ab.band_attention_switch_per_head(qv, kv, vv, m, m, flag, band, token_major_out=True)
    name, a = fake.calls[-1]
    assert name == "svg_band_attention_switch_per_head_lse" and len(a) == len(nat.ADAPTIVE_BAND_ENTRIES[name][1]) and a[15] is not None
    assert a[0] == qv.data_ptr() and a[12] == flag.data_ptr() and a[13] == band.data_ptr()
    assert o.transpose(1, 2).is_contiguous() and not o.is_contiguous() and lse.is_contiguous() and lse.shape == (1, H, S)
    assert ab.band_attention_per_head(q, q, q, m, band, return_lse=False).shape == q.shape
    with pytest.raises(ValueError, match="int32"):
        ab.band_attention_per_head(q, q, q, m, torch.zeros(3, dtype=torch.int32))
    src = (ROOT / "sparse-videogen_amd" / "svg" / "_adaptive_band.py").read_text()
    assert "torch.empty" not in src and src.count("_native.empty(") == 2 and src.count("_native._layout_plan(") == 2
    import ast
    import inspect

    called = {c.func.id for c in ast.walk(ast.parse(inspect.getsource(nat.band_width_update))) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)}
    assert not called & {"empty", "empty_like"} and not hasattr(nat, "band_attention_per_head")


# ---------------------------------------------------------------------------------------------------------
# the controller law
# ---------------------------------------------------------------------------------------------------------
KW = dict(target=0.9, gain_up=16.0, gain_down=4.0, dead=0.02, quantum=128, band_min=128, band_max=1024)


def test_controller_law_properties():
    band = [512] * 7
    kept = [0.7, 0.9, 0.91, 0.92, 0.99, 1.0, 0.85]
    new = BC.law32(band, kept, **KW)
    assert new[0] == 512 + 3 * 128                                  # e = 0.2 -> 3.2 quanta -> 3: kept < target widens
    assert new[1] == 512 and new[2] == 512 and new[3] == 512        # nothing moves inside the dead zone, its far edge included
    assert new[4] == 512 and new[5] == 512                          # 4 * -0.07, 4 * -0.08: less than half a quantum rounds to none
    assert new[6] == 512 + 128                                      # 0.8 quanta -> 1
    assert BC.law32([512], [1.0], **dict(KW, gain_down=16.0))[0] == 512 - 128          # -1.28 quanta -> -1: narrowed, by the slow gain
    # ties to even: 0.5 quanta stays, 1.5 quanta makes 2
    assert BC.law32([512, 512], [0.5, 0.5], **dict(KW, target=0.75, gain_up=2.0)).tolist() == [512, 512]
    assert BC.law32([512], [0.5], **dict(KW, target=0.75, gain_up=6.0))[0] == 512 + 256
    # both clamps; the step itself is bounded: 65536 quanta
    assert BC.law32([512], [0.0], **KW)[0] == 1024 and BC.law32([256], [1.0], **dict(KW, gain_down=64.0))[0] == 128
    assert BC.law32([0], [0.0], **dict(KW, gain_up=1e9, quantum=1, band_max=1 << 30))[0] == 65536
    # kept not finite, or a skipped step: unchanged, even outside the clamps
    for bad in (NAN, math.inf, -math.inf):
        assert BC.law32([512, 5], [bad, bad], **KW).tolist() == [512, 5]
    assert BC.law32([512, 5], [0.1, 0.1], skip=True, **KW).tolist() == [512, 5]
    # zero gains: a finite kept moves nothing inside the clamps; outside them the clamp still holds
    assert BC.law32(band, kept, **dict(KW, gain_up=0.0, gain_down=0.0)).tolist() == band
    assert BC.law32([5, 5000], [0.9, 0.9], **dict(KW, gain_up=0.0, gain_down=0.0)).tolist() == [128, 1024]
    # a NaN target moves nothing
    assert BC.law32(band, kept, **dict(KW, target=NAN)).tolist() == band
    # monotone in kept: a head that kept less never ends with a narrower band; the residue modulo the quantum survives every step
    ks = np.linspace(0, 1, 201).astype(np.float32)
    out = BC.law32(np.full(201, 513), ks, **dict(KW, band_min=1, band_max=1025))
    assert (np.diff(out) <= 0).all() and ((out - 513) % 128 == 0).all()
    # any vector content is clamped, never wrapped
    assert BC.law32([2 ** 31 - 1, -2 ** 31], [0.0, 1.0], **dict(KW, gain_up=1e9, gain_down=1e9, quantum=4096)).tolist() == [1024, 128]


def test_the_fp32_law_is_the_float64_statement_away_from_rounding_boundaries():
    g = np.random.default_rng(7)
    kept = g.uniform(0, 1.0, 4000).astype(np.float32)
    band = g.integers(1, 2000, 4000)
    for kw in (KW, dict(KW, gain_up=37.3, gain_down=11.1, dead=0.013, quantum=64, target=0.95)):
        kw32 = {k: (float(np.float32(v)) if isinstance(v, float) else v) for k, v in kw.items()}     # the parameters as the ABI carries them
        a, b = BC.law32(band, kept, **kw), BC.law64(band, kept.astype(np.float64), **kw32)
        e = kw32["target"] - kept.astype(np.float64)
        x = np.where(e > 0, kw32["gain_up"] * e, np.where(e < -kw32["dead"], kw32["gain_down"] * (e + kw32["dead"]), 0.0))
        near_tie = np.abs(np.abs(x - np.floor(x)) - 0.5) < 1e-4     # fp32 roundings of e, e + dead and the product: < 2^-20 of a quantum count
        near_edge = np.abs(e + kw32["dead"]) < 1e-6
        assert (a == b)[~near_tie & ~near_edge].all() and (~near_tie).sum() > 3900


# ---------------------------------------------------------------------------------------------------------
# AdaptiveBand, BandStore
# ---------------------------------------------------------------------------------------------------------
def test_adaptive_band_checks_its_arguments_and_documents_untuned_gains():
    a = _core.AdaptiveBand(0.95)
    assert (a.dead, a.quantum, a.band_min, a.band_max, a.rows, a.valid_len) == (0.02, 128, None, None, 64, None)
    assert a.gain_up >= 0 and a.gain_down >= 0 and "UNTUNED" in _core.AdaptiveBand.__doc__
    for kw in (dict(gain_up=-1), dict(gain_down=NAN), dict(dead=-0.1), dict(dead=NAN), dict(quantum=0), dict(quantum=4097), dict(quantum=1.5),
               dict(band_min=0), dict(band_max=-3), dict(band_min=300, band_max=200), dict(rows=0), dict(rows=65)):
        with pytest.raises(ValueError):
            _core.AdaptiveBand(0.95, **kw)


def test_default_bounds_keep_the_residue_of_the_masks_band():
    S = 790
    a = _core.AdaptiveBand(0.9)
    assert a.bounds(256, S) == (128, 768)                           # a Hunyuan band, a multiple of 128
    assert a.bounds(385, 750) == (1, 641)                           # a Wan band, a multiple of 128 plus 1: the residue survives
    assert a.bounds(128, 127) == (128, 128) and a.bounds(S + 1, S) == ((S + 1) % 128, S + 1)
    assert _core.AdaptiveBand(0.9, quantum=1).bounds(300, S) == (1, S + 1)
    assert _core.AdaptiveBand(0.9, band_min=129, band_max=513).bounds(385, 750) == (129, 513)
    assert _core.AdaptiveBand(0.9, band_max=513).bounds(385, 750) == (1, 513)
    for kw, band in ((dict(band_min=128), 385), (dict(band_max=512), 385), (dict(band_min=100), 256)):
        with pytest.raises(ValueError, match="congruent"):
            _core.AdaptiveBand(0.9, **kw).bounds(band, 750)
    with pytest.raises(ValueError, match=r"S \+ 1"):
        _core.AdaptiveBand(0.9, band_max=897).bounds(385, 750)      # congruent, but beyond S + 1
    for bad in (0, 752):
        with pytest.raises(ValueError, match="mask's band"):
            a.bounds(bad, 750)
    lo, hi = a.bounds(385, 750)
    out = BC.law32([385] * 3, [0.0, 1.0, 0.5], target=0.9, gain_up=1e4, gain_down=1e4, dead=0.02, quantum=128, band_min=lo, band_max=hi)
    assert out.tolist() == [641, 1, 641] and all((b - 385) % 128 == 0 for b in out)


def test_band_store():
    s = _core.BandStore()
    assert not s.has(3)
    t = s.get(3, 6, 256, "cpu")
    assert t.dtype == torch.int32 and t.shape == (6,) and t.tolist() == [256] * 6 and s.has(3) and s.has(3, 6)
    t[2] = 384
    s.kept[3] = torch.zeros(6)
    assert s.get(3, 6, 128, "cpu") is t and s.get(3, 6, 128, "cpu")[2] == 384     # the same size: the state, not the mask's band
    assert 3 in s.kept
    u = s.get(3, 12, 385, "cpu")                                   # another cfg * H: the layer starts again
    assert u is not t and u.tolist() == [385] * 12 and 3 not in s.kept and not s.has(3, 6)
    w = s.get(3, 12, 385, "meta")                                  # another device: likewise
    assert w is not u and w.device.type == "meta"
    s.get(4, 6, 256, "cpu")
    s.clear()
    assert not s.has(3) and not s.has(4) and not s.kept and not s.band


def test_processors_carry_the_option_and_the_store():
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0, Hunyuan_SVGAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor, WanAttn_SVGAttn_Processor2_0

    for cls in (Hunyuan_SVGAttn_Processor2_0, WanAttn_SVGAttn_Processor2_0):
        assert cls.adaptive_band is None and isinstance(cls.band_store, _core.BandStore)
        cls.band_store.get(7, 4, 256, "cpu")
        cls.reset_state()
        assert not cls.band_store.has(7)
        cls.band_store.get(7, 4, 256, "cpu")
        cls(0).reset_state()
        assert not cls.band_store.has(7)
    assert Hunyuan_SVGAttn_Processor2_0.band_store is not WanAttn_SVGAttn_Processor2_0.band_store
    # the SVG2 subclasses still reset what they reset, and the bands with it
    p = WanAttn_SAPAttn_Processor(0)
    p.top_p_store.get(0, 4, 0.5, "cpu"), p.band_store.get(0, 4, 256, "cpu")
    p.reset_state()
    assert not p.top_p_store.has(0) and not p.band_store.has(0)
    Hunyuan_SAPAttn_Processor2_0.top_p_store.get(7, 4, 0.5, "cpu")
    Hunyuan_SAPAttn_Processor2_0.reset_state()
    assert not Hunyuan_SAPAttn_Processor2_0.top_p_store.has(7)


# ---------------------------------------------------------------------------------------------------------
# refusals: all before a (stand-in) library sees a call
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda strict=True: pytest.fail("the library was reached before the refusal"))
    monkeypatch.setattr(_core, "sample_mse", lambda *a, **k: pytest.fail("the profiler ran before the refusal"))


def core_calls(q, geo, m, **kw):
    prof, flag = None, torch.zeros(1, dtype=torch.int32)
    dense = nat.BandMask(geo.seq_len, geo.seq_len + 1, 0, 0, 0, 0)
    yield "switch", lambda **more: _core.svg1_attention_device_switch(q, q, q, geo, m, dense, prof, 16, 100, flag, **dict(kw, **more))
    yield "sparse", lambda **more: _core.svg1_sparse_attention(q, q, q, geo, m, prof, 16, 100, **dict(kw, **more))


def test_core_functions_refuse_before_anything_runs(no_library):
    geo = _core.Geometry(0, 2, 64, text_first=False)
    S = geo.seq_len
    m = nat.BandMask(S, 65, 0, 0, 0, 0)
    ad, store = _core.AdaptiveBand(0.9, quantum=64), _core.BandStore()
    kw = dict(adaptive=ad, band_store=store, layer_idx=0)
    q = torch.zeros(2, 2, S, 128, dtype=torch.bfloat16)
    q64 = torch.zeros(2, 2, S, 64, dtype=torch.bfloat16)
    for name, call in core_calls(q64, geo, m, **kw):
        with pytest.raises(ValueError, match="head_dim 128"):     # CogVideoX's head size: no LSE form
            call()
    for name, call in core_calls(q, geo, m, **kw):
        with pytest.raises(ValueError, match="q_prescaled = True"):
            call(q_prescaled=True)
        with pytest.raises(ValueError, match="out_dtype"):
            call(return_lse=True, out_dtype=torch.float32)
        _core.set_attention_dtype("fp8")
        try:
            with pytest.raises(ValueError, match="fp8 = True"):
                call()
        finally:
            _core.set_attention_dtype("bf16")
        if name == "sparse":
            with pytest.raises(ValueError, match="fused = False"):
                call(fused=False)
    for name, call in core_calls(q, geo, m, adaptive=ad, layer_idx=0):
        with pytest.raises(ValueError, match="band_store"):
            call()
    # per-video masks that differ: the groups launch has no per-head form; equal ones are one mask
    m2 = nat.BandMask(S - 3, 65, 0, 0, 0, 0)
    for name, call in core_calls(q, geo, (m, m2), **kw):
        with pytest.raises(NotImplementedError, match="per-video masks"):
            call()
    # a bound that is not congruent to the mask's band, and a mask whose band the bounds cannot hold
    for name, call in core_calls(q, geo, m, adaptive=_core.AdaptiveBand(0.9, quantum=64, band_min=64), band_store=store, layer_idx=0):
        with pytest.raises(ValueError, match="congruent"):
            call()
    for name, call in core_calls(q, geo, nat.BandMask(S, 0, 0, 0, 0, 0), **kw):
        with pytest.raises(ValueError, match="mask's band"):
            call()
    assert not store.band and not store.kept


@pytest.mark.parametrize("mode", ["enable", "frame_shards", "token_shards"])
def test_adaptive_band_is_refused_under_every_distributed_mode(monkeypatch, no_library, mode):
    import os

    import torch.distributed as dist

    from svg import distributed as sd
    from svg.models.hyvideo.attention import Hunyuan_SVGAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{42500 + os.getpid() % 2000}", rank=0, world_size=1)
    try:
        {"enable": sd.enable, "frame_shards": sd.enable_frame_shards, "token_shards": sd.enable_token_shards}[mode]()
        for name in ("all_reduce", "all_to_all_single", "all_gather_into_tensor", "broadcast", "all_gather"):
            monkeypatch.setattr(dist, name, lambda *a, _n=name, **k: pytest.fail(f"{_n}: a collective ran before the refusal"))
        geo = _core.Geometry(0, 2, 64, text_first=False)
        S = geo.seq_len
        q = torch.zeros(1, 2, S, 128, dtype=torch.bfloat16)
        m = nat.BandMask(S, 65, 0, 0, 0, 0)
        ad, store = _core.AdaptiveBand(0.9, quantum=64), _core.BandStore()
        for _, call in core_calls(q, geo, m, adaptive=ad, band_store=store, layer_idx=0):
            with pytest.raises(NotImplementedError, match="adaptive_band"):
                call()
        t = torch.tensor([500.0])
        for cls in (WanAttn_SVGAttn_Processor2_0, Hunyuan_SVGAttn_Processor2_0):
            for attr, val in (("adaptive_band", ad), ("num_frame", 2), ("frame_size", 64), ("context_length", 0), ("prompt_length", 0),
                              ("block_mask", m), ("band_store", store), ("first_layers_fp", 0), ("first_times_fp", 900.0)):
                monkeypatch.setattr(cls, attr, val, raising=False)
            args = (q, q, q, t, 0, None) if cls is Hunyuan_SVGAttn_Processor2_0 else (q, q, q, t)
            if mode == "enable":                           # (the shard modes check the rows of this rank first, as before)
                with pytest.raises(NotImplementedError, match="adaptive_band"):
                    cls(0).attention_core_logic(*args)
        assert not store.band
    finally:
        sd.disable()
        dist.destroy_process_group()
