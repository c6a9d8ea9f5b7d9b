"""The per-head band launches on the work queue without a GPU (include/svg_attn_band_per_head_queue.h: svg_band_attention_per_head_queue_lse,
svg_band_attention_switch_per_head_queue_lse, svg_band_per_head_queue_order): the exports, the header and its place in svg_attn.h; the argument
validation — every bad call gets the code its static sibling gives, on the host before any launch (placeholder pointers: skipped where a GPU is
visible, as in test_adaptive_band_cpu.py) —; the order the device hands out, stated on the host: per head the indices that are not dropped are
exactly the q-tiles of that head under its own clamped band, drops occur on wide heads only (and do occur), and with uniform bands the order
is svg_band_queue_order's; and the Python path: work_queue=True and _core.PER_HEAD_BAND_QUEUE reach the _queue names with the arguments of
the static call, the defaults reach the old names, and every refusal still comes first."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from svg import _adaptive_band as ab
from svg import _native as nat
from svg.models import _core

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2   # include/svg_attn.h
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
ROOT = Path(__file__).resolve().parent.parent
ONE, SWITCH, ORDER = "svg_band_attention_per_head_queue_lse", "svg_band_attention_switch_per_head_queue_lse", "svg_band_per_head_queue_order"
SIBLING = {ONE: "svg_band_attention_per_head_lse", SWITCH: "svg_band_attention_switch_per_head_lse"}


def host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


# ---------------------------------------------------------------------------------------------------------
# exports and header
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    lib = nat.load()
    assert set(nat.ADAPTIVE_BAND_QUEUE_ENTRIES) == {ONE, SWITCH, ORDER}
    others = set(nat.ADAPTIVE_BAND_ENTRIES)
    for name in dir(nat):
        if name.endswith("SIGNATURES") and isinstance(getattr(nat, name), dict):
            others |= set(getattr(nat, name))
    assert not set(nat.ADAPTIVE_BAND_QUEUE_ENTRIES) & others
    for name, (res, args) in nat.ADAPTIVE_BAND_QUEUE_ENTRIES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    for name, sib in SIBLING.items():                             # exactly the arguments of the static siblings
        assert nat.ADAPTIVE_BAND_QUEUE_ENTRIES[name] == nat.ADAPTIVE_BAND_ENTRIES[sib]
        assert getattr(lib, name).argtypes == getattr(lib, sib).argtypes and getattr(lib, name).restype == getattr(lib, sib).restype
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_is_included_and_matches_the_signatures():
    main = (ROOT / "include" / "svg_attn.h").read_text()
    assert "#define SVG_ABI_VERSION 4\n" in main
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', main, flags=re.M)
    assert includes[-4:] == ["svg_attn_band_per_head_queue.h", "svg_attn_adaptive_band.h", "svg_attn_adaptive_top_p.h", "svg_attn_profile_shard.h"]
    src = (ROOT / "include" / "svg_attn_band_per_head_queue.h").read_text()
    assert "with respect to the hint" in src                       # the accepted limitation of the tail is stated
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert {n for _, n, _ in protos} == {ONE, SWITCH, ORDER}

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
        res, args = nat.ADAPTIVE_BAND_QUEUE_ENTRIES[name]
        assert [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)

    def params_of(header, name):
        text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
        return re.sub(r"\s+", " ", re.search(name + r"\s*\(([^;{]*?)\)\s*;", text, flags=re.S).group(1)).strip()

    for name, sib in SIBLING.items():                             # the parameters of the static siblings, same order, same names
        assert params_of("svg_attn_band_per_head_queue.h", name) == params_of("svg_attn_adaptive_band.h", sib)


# ---------------------------------------------------------------------------------------------------------
# validation: the code of the static sibling, whatever it is
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
    ("BH0", dict(BH=0), BAD_ARG), ("BH_neg", dict(BH=-3), BAD_ARG), ("S0", dict(S=0), BAD_ARG),
    ("null_band_before_D", dict(band=None, D=64), BAD_ARG), ("null_lse_before_dtype", dict(lse=None, dtype=2), BAD_ARG),
    ("mask_band_neg", dict(m=mask(band=-1)), BAD_ARG), ("mask_band_above_S_plus_1", dict(m=mask(band=S0 + 2)), BAD_ARG),
    ("mask_real_len", dict(m=mask(real=S0 + 1)), BAD_ARG), ("mask_colfull", dict(m=mask(cl=5, ch=4)), BAD_ARG),
    ("perm_without_frames", dict(perm=BAD_PERM), BAD_ARG), ("bad_mask_before_D", dict(m=mask(band=-1), D=64), BAD_ARG),
    ("S_2pow24", dict(S=1 << 24, m=mask(real=0)), UNSUPPORTED),
    ("layout_heads", dict(lay=layout(H=3)), BAD_ARG), ("layout_row_below_D", dict(lay=layout(q_row=64)), BAD_ARG),
    ("layout_row_misaligned", dict(lay=layout(k_row=132)), UNSUPPORTED), ("layout_before_D", dict(lay=layout(H=3), D=64), BAD_ARG),
    ("D64", dict(D=64), UNSUPPORTED), ("D96", dict(D=96), UNSUPPORTED), ("dtype_f32", dict(dtype=2), UNSUPPORTED),
    ("dtype_neg", dict(dtype=-1), UNSUPPORTED),
]
SWITCH_ONLY = [
    ("null_alt", dict(alt=None), BAD_ARG), ("null_flag", dict(flag=None), BAD_ARG),
    ("null_alt_before_bad_mask", dict(alt=None, m=mask(band=-1)), BAD_ARG), ("alt_band", dict(alt=mask(band=S0 + 2)), BAD_ARG),
    ("alt_real_len", dict(alt=mask(real=-1)), BAD_ARG), ("alt_before_D", dict(alt=mask(real=-1), D=64), BAD_ARG),
    ("alt_before_layout", dict(alt=mask(cl=3, ch=2), lay=layout(k_row=132)), BAD_ARG),
]


@pytest.mark.parametrize("kw,expected", [c[1:] for c in ATTN_CASES], ids=[c[0] for c in ATTN_CASES])
def test_queue_entries_reject_like_their_static_siblings(kw, expected):
    host_only()
    lib = nat.load()
    one, sw = attn_args(**kw)
    assert getattr(lib, ONE)(*one) == getattr(lib, SIBLING[ONE])(*one) == expected
    assert getattr(lib, SWITCH)(*sw) == getattr(lib, SIBLING[SWITCH])(*sw) == expected


@pytest.mark.parametrize("kw,expected", [c[1:] for c in SWITCH_ONLY], ids=[c[0] for c in SWITCH_ONLY])
def test_switch_queue_entry_rejects_like_its_static_sibling(kw, expected):
    host_only()
    lib = nat.load()
    sw = attn_args(**kw)[1]
    assert getattr(lib, SWITCH)(*sw) == getattr(lib, SIBLING[SWITCH])(*sw) == expected


# ---------------------------------------------------------------------------------------------------------
# the order
# ---------------------------------------------------------------------------------------------------------
def hy_mask(F, P, ctx, L, band):
    V = F * P
    return V + ctx, nat.BandMask(real_len=V + L, band=band, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)


def _cases():   # name -> (heads, S, mask): those of tests/test_band_queue_cpu.py
    out = {}
    for name, H, F, P, ctx, L, band in (("hy720p", 24, 33, 3600, 256, 64, 15616), ("hy480p", 24, 33, 1350, 256, 64, 5632),
                                        ("tiny", 4, 5, 600, 256, 64, 384), ("hy720p_3_heads", 3, 33, 3600, 256, 64, 15616)):
        S, m = hy_mask(F, P, ctx, L, band)
        out[name] = (H, S, m)
    S = 20 * 256 + 100
    out["no_text_rows"] = (5, S, nat.BandMask(real_len=S - 60, band=1024, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["no_pad_rows"] = (5, S, nat.BandMask(real_len=S, band=1024, colfull_lo=S - 100, colfull_hi=S, rowfull_lo=S - 100, rowfull_hi=S))
    out["band_covers_all"] = (3, S, nat.BandMask(real_len=S, band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["one_item"] = (1, 200, nat.BandMask(real_len=200, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["two_items"] = (2, 256, nat.BandMask(real_len=256, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["many_heads"] = (300, 700, nat.BandMask(real_len=650, band=128, colfull_lo=600, colfull_hi=650, rowfull_lo=600, rowfull_hi=650))
    return out


CASES = _cases()
VECTORS = ["hint", "ones", "wide", "alternating", "random"]


def hint_of(S, m):
    return min(m.band, S)


def band_vector(kind, BH, S, m):
    hint = hint_of(S, m)
    if kind == "hint":
        return [hint] * BH
    if kind == "ones":
        return [1] * BH
    if kind == "wide":
        return [S + 1] * BH
    if kind == "alternating":
        return [hint if h % 2 == 0 else S + 1 for h in range(BH)]
    return np.random.default_rng(BH * 1000003 + S).integers(-5, S + 11, BH).tolist()   # [-5, S + 10]: the clamp at both ends


def with_band(m, band):
    return nat.BandMask(m.real_len, band, m.colfull_lo, m.colfull_hi, m.rowfull_lo, m.rowfull_hi)


def plain_order(BH, S, m):
    lib = nat.load()
    n = lib.svg_band_queue_order(BH, S, C.byref(m), None, 0)
    buf = (C.c_int32 * (3 * n))()
    assert lib.svg_band_queue_order(BH, S, C.byref(m), C.cast(buf, C.c_void_p), 3 * n) == n
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(n)]


def nqt_of(S, m, _memo={}):
    """q-tiles of a one-head launch under this mask"""
    key = (S, m.real_len, m.band, m.colfull_lo, m.colfull_hi, m.rowfull_lo, m.rowfull_hi)
    if key not in _memo:
        _memo[key] = nat.load().svg_band_queue_order(1, S, C.byref(m), None, 0)
        assert _memo[key] > 0
    return _memo[key]


def per_head_order(BH, S, m, alt, use_alt, band):
    lib = nat.load()
    vec = (C.c_int32 * BH)(*band)
    alt_p = None if alt is None else C.byref(alt)
    n = getattr(lib, ORDER)(BH, S, C.byref(m), alt_p, use_alt, vec, None, 0)
    assert n > 0
    guard = 0x5A5A5A5A
    buf = (C.c_int32 * (4 * n + 4))(*([guard] * (4 * n + 4)))
    assert getattr(lib, ORDER)(BH, S, C.byref(m), alt_p, use_alt, vec, buf, 4 * n - 1) == -1   # too small: refused
    assert list(buf[4 * n - 1:]) == [guard] * 5                                                  # ... and nothing behind the buffer's end
    assert getattr(lib, ORDER)(BH, S, C.byref(m), alt_p, use_alt, vec, buf, 4 * n) == n
    assert list(buf[4 * n:]) == [guard] * 4
    assert list(vec) == list(band)                                 # the band vector is not written
    return [tuple(buf[4 * i:4 * i + 4]) for i in range(n)]


@pytest.mark.parametrize("use_alt", [0, 1])
@pytest.mark.parametrize("kind", VECTORS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_head_runs_exactly_its_own_q_tiles(name, kind, use_alt):
    BH, S, m = CASES[name]
    band = band_vector(kind, BH, S, m)
    alt = nat.BandMask(m.real_len, S + 1, 0, 0, 0, 0) if use_alt else None   # a dense alternate mask
    items = per_head_order(BH, S, m, alt, use_alt, band)
    assert all(0 <= x <= 8 and 0 <= h < BH for x, h, _, _ in items)
    clamped = [min(max(b, 1), S + 1) for b in band]
    seen = [[] for _ in range(BH)]
    for x, h, idx, block in items:
        if use_alt:
            assert block == 2 and idx >= 0
        else:
            assert block == (1 if clamped[h] > S else 0)
            assert idx >= 0 or block == 1, "an item was dropped on a head that cuts the full rows out"
        if idx >= 0:
            seen[h].append(idx)
    for h in range(BH):
        nqt_h = nqt_of(S, alt) if use_alt else nqt_of(S, with_band(m, clamped[h]))
        assert sorted(seen[h]) == list(range(nqt_h)), (h, clamped[h])
    if not use_alt:
        assert len(items) == BH * nqt_of(S, with_band(m, hint_of(S, m)))   # the queue is the hint's


def test_the_drop_is_exercised():
    """tiny with a wide head: the block that cuts the text rows out has one q-tile more than the wide one"""
    BH, S, m = CASES["tiny"]
    assert nqt_of(S, with_band(m, hint_of(S, m))) == nqt_of(S, with_band(m, S + 1)) + 1
    for kind in ("wide", "alternating"):
        band = band_vector(kind, BH, S, m)
        items = per_head_order(BH, S, m, None, 0, band)
        wide_heads = sum(1 for b in band if b > S)
        assert sum(1 for _, _, idx, _ in items if idx < 0) == wide_heads > 0
    assert not [i for i in per_head_order(BH, S, m, None, 0, band_vector("ones", BH, S, m)) if i[2] < 0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_uniform_bands_give_the_order_of_the_plain_queue(name):
    BH, S, m = CASES[name]
    hint = with_band(m, hint_of(S, m))
    nqt = nqt_of(S, hint)
    items = per_head_order(BH, S, m, None, 0, band_vector("hint", BH, S, m))
    assert [(x, h * nqt + idx) for x, h, idx, _ in items] == [(x, i) for x, i, _ in plain_order(BH, S, hint)]
    assert all(block == 0 for _, _, _, block in items)


def test_order_rejects_bad_arguments():
    lib = nat.load()
    BH, S, m = CASES["tiny"]
    vec = (C.c_int32 * BH)(*([m.band] * BH))
    fn = getattr(lib, ORDER)
    assert fn(BH, S, C.byref(m), None, 0, vec, None, 0) > 0
    assert fn(BH, S, None, None, 0, vec, None, 0) == -1
    assert fn(BH, S, C.byref(m), None, 0, None, None, 0) == -1
    assert fn(0, S, C.byref(m), None, 0, vec, None, 0) == -1 and fn(BH, 0, C.byref(m), None, 0, vec, None, 0) == -1
    assert fn(BH, S, C.byref(with_band(m, S + 2)), None, 0, vec, None, 0) == -1
    assert fn(BH, S, C.byref(m), C.byref(with_band(m, -1)), 0, vec, None, 0) == -1
    assert fn(BH, S, C.byref(m), None, 1, vec, None, 0) == -1     # the flag without an alternate mask


# ---------------------------------------------------------------------------------------------------------
# the wrappers and _core, on a recording stand-in library
# ---------------------------------------------------------------------------------------------------------
class FakeLib:
    """records the per-head attention calls instead of launching them"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*a):
            self.calls.append((name, a))
            return 0
        return fn


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(nat, "load", lambda strict=True: lib)
    monkeypatch.setattr(nat, "_gpu", lambda *ts: None)
    monkeypatch.setattr(nat, "_dev", lambda *ts: None)
    monkeypatch.setattr(nat, "_stream", lambda: 0)
    return lib


def plain(args):
    """the arguments of a recorded call without what differs from call to call: the addresses of fresh allocations and of byref objects"""
    return [a if isinstance(a, (int, float, type(None))) else type(a).__name__ for a in args]


def test_work_queue_selects_the_queue_entries_with_the_same_arguments(fake):
    H, S, D = 2, 70, 128
    band, flag, m = torch.full((H,), 5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), mask(70, 5)
    q = torch.zeros(1, H, S, D, dtype=torch.bfloat16)
    out = torch.zeros_like(q)
    qkv = torch.zeros(1, S, 3 * H * D, dtype=torch.bfloat16)
    qv, kv, vv = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
    for tensors, kw in (((q, q, q), dict(out=out)), ((qv, kv, vv), dict(out=nat.token_major_empty(qv), token_major_out=True))):
        for static_name, call in ((SIBLING[ONE], lambda **k: ab.band_attention_per_head(*tensors, m, band, **kw, **k)),
                                  (SIBLING[SWITCH], lambda **k: ab.band_attention_switch_per_head(*tensors, m, m, flag, band, **kw, **k))):
            del fake.calls[:]
            o0, lse0 = call()
            o1, lse1 = call(work_queue=False)
            o2, lse2 = call(work_queue=True)
            names = [n for n, _ in fake.calls]
            assert names == [static_name, static_name, static_name.replace("_lse", "_queue_lse")]
            assert names[2] in nat.ADAPTIVE_BAND_QUEUE_ENTRIES
            a0, a1, a2 = (list(a) for _, a in fake.calls)
            for a, lse in ((a0, lse0), (a1, lse1), (a2, lse2)):
                assert a[4] == lse.data_ptr() and lse.shape == (1, H, S) and lse.is_contiguous()
                a[4] = "lse"
            assert plain(a0) == plain(a1) == plain(a2) and a2[3] == kw["out"].data_ptr() and o2.data_ptr() == kw["out"].data_ptr()
            assert len(a2) == len(nat.ADAPTIVE_BAND_QUEUE_ENTRIES[names[2]][1])
    assert ab.band_attention_per_head(q, q, q, m, band, return_lse=False, work_queue=True).shape == q.shape


def core_calls(q, geo, m, **kw):
    prof, flag = None, torch.zeros(1, dtype=torch.int32)
    dense = nat.BandMask(geo.seq_len, geo.seq_len + 1, 0, 0, 0, 0)
    yield "switch", lambda **more: _core.svg1_attention_device_switch(q, q, q, geo, m, dense, prof, 16, 100, flag, **dict(kw, **more))
    yield "sparse", lambda **more: _core.svg1_sparse_attention(q, q, q, geo, m, prof, 16, 100, **dict(kw, **more))


@pytest.mark.parametrize("on", [False, True])
def test_core_switch_routes_both_layer_calls(monkeypatch, on):
    """_svg1_layer_call up to the launch, with the profiler, the controller and the device check stubbed out: what the wrappers are
    called with"""
    assert _core.PER_HEAD_BAND_QUEUE is False                       # the default stays off
    monkeypatch.setattr(_core, "PER_HEAD_BAND_QUEUE", on)
    seen = []

    def record(name):
        def fn(*a, **k):
            seen.append((name, k))
            return torch.zeros(1), torch.zeros(1)
        return fn

    monkeypatch.setattr(ab, "band_attention_per_head", record("one"))
    monkeypatch.setattr(ab, "band_attention_switch_per_head", record("switch"))
    monkeypatch.setattr(_core, "_require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(_core, "sample_mse", lambda q, *a, **k: torch.zeros(2, q.shape[0], q.shape[1]))
    monkeypatch.setattr(_core, "_adaptive_band_call", lambda run, *a, **k: run(torch.zeros(4, dtype=torch.int32)))
    geo = _core.Geometry(0, 2, 64, text_first=False)
    S = geo.seq_len
    q = torch.zeros(2, 2, S, 128, dtype=torch.bfloat16)
    m = nat.BandMask(S, 65, 0, 0, 0, 0)
    kw = dict(adaptive=_core.AdaptiveBand(0.9, quantum=64), band_store=_core.BandStore(), layer_idx=0)
    for name, call in core_calls(q, geo, m, **kw):
        call()
    assert [n for n, _ in seen] == ["switch", "one"]
    for _, k in seen:
        assert ("work_queue" in k) == on and k.get("work_queue", False) is on   # off: nothing new is passed
        assert k["token_major_out"] == _core.TOKEN_MAJOR_IO and k["num_frame"] == 2 and k["frame_size"] == 64


@pytest.fixture
def no_library(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda strict=True: pytest.fail("the library was reached before the refusal"))
    monkeypatch.setattr(_core, "sample_mse", lambda *a, **k: pytest.fail("the profiler ran before the refusal"))


def test_every_refusal_still_comes_first(monkeypatch, no_library):
    """the refusals of _refuse_adaptive_band (tests/test_adaptive_band_cpu.py) with the switch on"""
    monkeypatch.setattr(_core, "PER_HEAD_BAND_QUEUE", True)
    geo = _core.Geometry(0, 2, 64, text_first=False)
    S = geo.seq_len
    m = nat.BandMask(S, 65, 0, 0, 0, 0)
    ad, store = _core.AdaptiveBand(0.9, quantum=64), _core.BandStore()
    kw = dict(adaptive=ad, band_store=store, layer_idx=0)
    q = torch.zeros(2, 2, S, 128, dtype=torch.bfloat16)
    q64 = torch.zeros(2, 2, S, 64, dtype=torch.bfloat16)
    for name, call in core_calls(q64, geo, m, **kw):
        with pytest.raises(ValueError, match="head_dim 128"):
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
    m2 = nat.BandMask(S - 3, 65, 0, 0, 0, 0)
    for name, call in core_calls(q, geo, (m, m2), **kw):            # the groups form stays out of scope
        with pytest.raises(NotImplementedError, match="per-video masks"):
            call()
    for name, call in core_calls(q, geo, m, adaptive=_core.AdaptiveBand(0.9, quantum=64, band_min=64), band_store=store, layer_idx=0):
        with pytest.raises(ValueError, match="congruent"):
            call()
    for name, call in core_calls(q, geo, nat.BandMask(S, 0, 0, 0, 0, 0), **kw):
        with pytest.raises(ValueError, match="mask's band"):
            call()
    assert not store.band and not store.kept
