"""The LSE / fp32 forms of the device-switch and groups launches of band attention without a GPU (include/svg_attn_band_lse_forms.h):
the exports and prototypes, the argument validation (every check runs on the host before any launch — rows that pass placeholder pointers
are skipped where a GPU is visible, as in test_sparse_attention_lse_cpu.py), the combinations the wrappers and the _core functions refuse,
and the float64 identities the GPU protocol of tests/test_gpu_band_lse_forms.py rests on.

The argument faults are the rows of the plain siblings' tables — tests/test_entry_validation_cpu.py (svg_band_attention_switch[_strided])
and tests/band_groups_cases.py (svg_band_groups_attention) — carried over to the new argument lists: each must come back with the code
the plain entry returns.

ref: BlockSparseAttentionWrapper.run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188."""
import ast
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import sparse_lse_cases as SC
from band_groups_cases import GROUP_CASES
from lse_ops_torch import attention_lse, merge_states
from oracle import svg_oracle as O
from svg import _native as nat
from test_entry_validation_cpu import CASES as PLAIN_CASES
from test_gpu_kernels import _band_case

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2   # include/svg_attn.h
PH = 0x10000                           # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("svg_band_attention_switch_lse", "svg_band_attention_switch_lse_f32", "svg_band_groups_attention_lse",
         "svg_band_groups_attention_lse_f32")


def _host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


def test_library_exports_the_band_lse_forms():
    lib = nat.load()
    assert set(nat.BAND_LSE_FORM_SIGNATURES) == set(NAMES)
    assert not set(nat.BAND_LSE_FORM_SIGNATURES) & (set(nat.SIGNATURES) | set(nat.SPARSE_LSE_SIGNATURES) | set(nat.SPARSE_F32_SIGNATURES))
    for name, (res, args) in nat.BAND_LSE_FORM_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_prototypes_match_the_ctypes_signatures_and_call_sites():
    """the three checks of tests/test_sparse_attention_lse_cpu.py for include/svg_attn_band_lse_forms.h against BAND_LSE_FORM_SIGNATURES"""
    assert '#include "svg_attn_band_lse_forms.h"' in (ROOT / "include" / "svg_attn.h").read_text()
    src = (ROOT / "include" / "svg_attn_band_lse_forms.h").read_text()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert {n for _, n, _ in protos} == set(NAMES)

    def c_class(t):
        for pat, c in ((r"\*", "ptr"), (r"\bsize_t\b", "size"), (r"\b(int32_t|int)\b", "i32"), (r"\bfloat\b", "f32")):
            if re.search(pat, t):
                return c
        return "?" + t

    def py_class(a):
        if a is C.c_void_p or (isinstance(a, type) and issubclass(a, C._Pointer)):
            return "ptr"
        return {C.c_size_t: "size", C.c_int32: "i32", C.c_int: "i32", C.c_float: "f32"}.get(a, "?" + repr(a))

    lib = nat.load()
    for ret, name, params in protos:
        ps = [x.strip() for x in params.split(",") if x.strip()]
        want = [c_class(x if x.endswith("*") else re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", x)) for x in ps]
        res, args = nat.BAND_LSE_FORM_SIGNATURES[name]
        assert hasattr(lib, name) and [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)
    tree = ast.parse((ROOT / "sparse-videogen_amd" / "svg" / "_native.py").read_text())
    seen = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in NAMES:
            # (positional; the arguments between lse and layout travel as one starred tuple of the entry's middle arguments)
            assert not node.keywords and any(isinstance(a, ast.Starred) for a in node.args), (node.func.attr, node.lineno)
            seen.append(node.func.attr)
    assert sorted(seen) == sorted(NAMES)                 # one call site per entry


# ---------------------------------------------------------------------------------------------------------
# argument faults: the plain siblings' rows on the new argument lists
# ---------------------------------------------------------------------------------------------------------
def _switch_rows():
    """(id, plain call, new argument list without o / lse filled in differently): rows of svg_band_attention_switch[_strided].  A NULL
    layout is no fault of the new entries (it means contiguous tensors), so those rows of the strided table are left out."""
    rows = []
    for cid, (name, args), code in PLAIN_CASES:
        if name == "svg_band_attention_switch":
            rows.append((cid, (name, args), args[:4] + [PH] + args[4:-1] + [None, None], code))
        elif name == "svg_band_attention_switch_strided" and args[-2] is not None:
            rows.append((cid, (name, args), args[:4] + [PH] + args[4:], code))
    return rows


def _groups_rows():
    """rows of svg_band_groups_attention with q_prescaled = 0 (the new entries have no such argument)"""
    return [(cid, (name, args), args[:4] + [PH] + args[4:15] + args[16:], code) for cid, (name, args), code in GROUP_CASES if args[15] == 0]


SWITCH_ROWS, GROUPS_ROWS = _switch_rows(), _groups_rows()


def test_the_carried_over_tables_are_not_empty():
    ids = {r[0] for r in SWITCH_ROWS}
    for want in ("switch/null_alt", "switch/null_flag", "switch/bad_alt", "switch/bad_perm", "switch/dtype", "switch/D96",
                 "switch_strided/heads0", "switch_strided/row_unaligned", "switch_strided/bad_alt"):
        assert want in ids
    ids = {r[0] for r in GROUPS_ROWS}
    for want in ("groups/bad_mask_last", "groups/n_groups0", "groups/sum_lt_BH", "groups/alt_without_flag", "groups/flag_without_alt",
                 "groups/layout_part_of_a_video", "groups/D96", "groups/dtype_f32", "groups/bad_alt_last"):
        assert want in ids
    assert len(SWITCH_ROWS) >= 15 and len(GROUPS_ROWS) >= 30


@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
@pytest.mark.parametrize("plain,args,expected", [r[1:] for r in SWITCH_ROWS], ids=[r[0] for r in SWITCH_ROWS])
def test_switch_forms_return_the_plain_entrys_code(plain, args, expected, f32):
    _host_only()
    lib = nat.load()
    rc = getattr(lib, plain[0])(*plain[1])
    assert rc == expected and rc != OK
    assert getattr(lib, "svg_band_attention_switch_lse" + ("_f32" if f32 else ""))(*args) == rc


@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
@pytest.mark.parametrize("plain,args,expected", [r[1:] for r in GROUPS_ROWS], ids=[r[0] for r in GROUPS_ROWS])
def test_groups_forms_return_the_plain_entrys_code(plain, args, expected, f32):
    _host_only()
    lib = nat.load()
    rc = getattr(lib, plain[0])(*plain[1])
    assert rc == expected and rc != OK
    assert getattr(lib, "svg_band_groups_attention_lse" + ("_f32" if f32 else ""))(*args) == rc


def _mask(S, **kw):
    m = nat.BandMask(S, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def switch_args(o=PH, lse=PH, S=256, D=128, dtype=0, m="ok"):
    m = _mask(S) if m == "ok" else m
    alt = _mask(S, band=S + 1)
    return [PH, PH, PH, o, lse, 2, S, D, dtype, 1.0, C.byref(m), None, C.byref(alt), PH, None, None]


def groups_args(o=PH, lse=PH, S=256, D=128, dtype=0, switch=False, masks=None):
    marr = (nat.BandMask * 2)(*(masks or [_mask(S), _mask(S)]))
    aarr = (nat.BandMask * 2)(_mask(S, band=S + 1), _mask(S, band=S + 1)) if switch else None
    garr = (C.c_int32 * 2)(2, 4)
    return [PH, PH, PH, o, lse, 6, S, D, dtype, 1.0, marr, aarr, garr, 2, None, PH if switch else None, None, None]


OWN_CASES = [
    ("null_lse", dict(lse=None), BAD_ARG),
    ("null_o", dict(o=None), BAD_ARG),                      # (o32 of the _f32 forms)
    ("null_lse_before_unsupported_D", dict(lse=None, D=64), BAD_ARG),
    ("null_lse_before_a_bad_mask", dict(lse=None, m=_mask(256, band=-1)), BAD_ARG),
    ("bad_mask_before_unsupported_D", dict(m=_mask(256, band=-1), D=64), BAD_ARG),
    ("D64", dict(D=64), UNSUPPORTED),
    ("D96", dict(D=96), UNSUPPORTED),
    ("dtype_f32", dict(dtype=2), UNSUPPORTED),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kw,expected", [c[1:] for c in OWN_CASES], ids=[c[0] for c in OWN_CASES])
def test_what_the_new_entries_check_themselves(kw, expected, name):
    _host_only()
    kw = dict(kw)
    if "groups" in name:
        m = kw.pop("m", None)
        for switch in (False, True):
            args = groups_args(switch=switch, masks=None if m is None else [_mask(256), m], **kw)
            assert getattr(nat.load(), name)(*args) == expected, switch
    else:
        assert getattr(nat.load(), name)(*switch_args(**kw)) == expected


@pytest.mark.parametrize("name", [n for n in NAMES if n.endswith("_f32")])
def test_unaligned_o32_is_unsupported(name):
    _host_only()
    lib = nat.load()
    if "groups" in name:
        for switch in (False, True):
            assert getattr(lib, name)(*groups_args(o=PH + 8, switch=switch)) == UNSUPPORTED
            assert getattr(lib, name)(*groups_args(o=PH + 8, switch=switch, masks=[_mask(256), _mask(256, real_len=257)])) == BAD_ARG
    else:
        assert getattr(lib, name)(*switch_args(o=PH + 8)) == UNSUPPORTED
        assert getattr(lib, name)(*switch_args(o=PH + 8, m=_mask(256, real_len=257))) == BAD_ARG   # argument faults come first


# ---------------------------------------------------------------------------------------------------------
# the Python wrappers: what has no LSE form raises before anything is loaded or launched (CPU tensors get this far)
# ---------------------------------------------------------------------------------------------------------
def _wrapper_calls():
    q = torch.zeros(1, 2, 64, 128, dtype=torch.bfloat16)
    q64 = torch.zeros(1, 2, 64, 64, dtype=torch.bfloat16)
    mask = nat.BandMask(**O.dense_band_params(64))
    flag = torch.zeros(1, dtype=torch.int32)
    return [("switch", lambda x=q, **kw: nat.band_attention_switch(x, x, x, mask, mask, flag, **kw), q, q64),
            ("groups", lambda x=q, **kw: nat.band_attention_groups(x, x, x, [mask, mask], [1, 1], **kw), q, q64),
            ("groups_switch", lambda x=q, **kw: nat.band_attention_groups(x, x, x, [mask, mask], [1, 1], alt_masks=[mask, mask],
                                                                          use_alt_flag=flag, **kw), q, q64)]


@pytest.mark.parametrize("what,call,q,q64", _wrapper_calls(), ids=[c[0] for c in _wrapper_calls()])
def test_wrappers_refuse_what_has_no_lse_form(what, call, q, q64, monkeypatch):
    monkeypatch.setattr(nat, "load", lambda *a, **k: pytest.fail("refused before the library is loaded"))
    for kw in (dict(), dict(out_dtype=torch.float32)):
        with pytest.raises(ValueError, match="return_lse"):
            call(q_prescaled=True, return_lse=True, **kw)
        with pytest.raises(ValueError, match="return_lse"):
            call(q64, return_lse=True, **kw)
    with pytest.raises(ValueError, match="return_lse"):
        call(out_dtype=torch.float32)                                   # without return_lse
    with pytest.raises(ValueError, match="token_major_out"):
        call(out_dtype=torch.float32, return_lse=True, token_major_out=True)
    with pytest.raises(ValueError, match="out"):
        call(out_dtype=torch.float32, return_lse=True, out=torch.empty_like(q))
    with pytest.raises(ValueError, match="out_dtype"):
        call(out_dtype=torch.float16, return_lse=True)                  # only None and torch.float32
    monkeypatch.undo()
    for kw in (dict(), dict(out_dtype=torch.float32)):
        with pytest.raises(RuntimeError):                               # supported: on to the tensor checks, which refuse CPU tensors
            call(return_lse=True, **kw)


# ---------------------------------------------------------------------------------------------------------
# _core
# ---------------------------------------------------------------------------------------------------------
class _Cuda:
    """a tensor stand-in that says it lives on the GPU (tests/test_band_groups_cpu.py)"""

    is_cuda = True

    def __init__(self, shape):
        self.shape = shape


def _core_setup(monkeypatch):
    from svg.models import _core

    calls = []

    def fake(name, n_out):
        def f(q, k, v, *a, **kw):
            calls.append((name, kw))
            return ("o", "lse") if kw.get("return_lse") else "o"
        return f

    for name in ("band_attention", "band_attention_switch", "band_attention_groups"):
        monkeypatch.setattr(_core._native, name, fake(name, 1))
    monkeypatch.setattr(_core._native, "band_attention_fp8", lambda *a, **kw: "o8")
    monkeypatch.setattr(_core, "sample_mse", lambda *a, **kw: torch.zeros(2, 2, 3))
    monkeypatch.setattr(_core, "_switch_generator", lambda: None)
    return _core, calls


def test_core_functions_return_the_state_only_when_asked(monkeypatch):
    _core, calls = _core_setup(monkeypatch)
    S, H = 512, 3
    q = _Cuda((2, H, S, 128))
    geo = _core.Geometry(128, 3, 128)
    m = nat.BandMask(421, 128, 384, 421, 384, 421)
    m2 = nat.BandMask(400, 128, 384, 400, 384, 400)
    dm = nat.BandMask(421, S + 1, 0, 0, 0, 0)
    flag = torch.zeros(1, dtype=torch.int32)
    # the defaults: what they returned, through the keywords they passed
    out = _core.svg1_attention_device_switch(q, q, q, geo, m, dm, None, 8, 384, flag)
    assert len(out) == 2 and out[0] == "o" and set(calls.pop()[1]) == {"head_perm_flag", "vid0", "num_frame", "frame_size", "q_prescaled",
                                                                        "token_major_out"}
    out = _core.svg1_sparse_attention(q, q, q, geo, m, None, 8, 384)
    assert len(out) == 2 and out[0] == "o" and "return_lse" not in calls.pop()[1]
    assert _core.dense_attention(q, q, q, 400) == "o" and set(calls.pop()[1]) == {"q_prescaled", "token_major_out"}
    assert _core.dense_attention(q, q, q, (400, 421)) == "o" and calls.pop()[0] == "band_attention_groups"
    # with the state
    for kw, tm in ((dict(return_lse=True), _core.TOKEN_MAJOR_IO), (dict(return_lse=True, out_dtype=torch.float32), False)):
        for masks, entry in ((m, "band_attention_switch"), ([m, m2], "band_attention_groups")):
            out = _core.svg1_attention_device_switch(q, q, q, geo, masks, dm, None, 8, 384, flag, **kw)
            name, got = calls.pop()
            assert len(out) == 3 and (out[0], out[2]) == ("o", "lse") and torch.is_tensor(out[1]) and name == entry
            assert got["return_lse"] is True and got["out_dtype"] == kw.get("out_dtype") and got["token_major_out"] == tm
        for masks, entry in ((m, "band_attention"), ([m, m2], "band_attention_groups")):
            out = _core.svg1_sparse_attention(q, q, q, geo, masks, None, 8, 384, **kw)
            name, got = calls.pop()
            assert len(out) == 3 and (out[0], out[2]) == ("o", "lse") and name == entry and got["return_lse"] is True
        for lens, entry in ((400, "band_attention"), ((400, 421), "band_attention_groups")):
            assert _core.dense_attention(q, q, q, lens, **kw) == ("o", "lse")
            name, got = calls.pop()
            assert name == entry and got["return_lse"] is True and got["out_dtype"] == kw.get("out_dtype")
    assert not calls


def test_core_functions_refuse_what_has_no_lse_form(monkeypatch):
    _core, calls = _core_setup(monkeypatch)
    q = torch.zeros(2, 2, 512, 128, dtype=torch.bfloat16)    # CPU tensors: refused before the GPU check
    geo = _core.Geometry(128, 3, 128)
    m = nat.BandMask(421, 128, 384, 421, 384, 421)
    dm = nat.BandMask(421, 513, 0, 0, 0, 0)
    flag = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="return_lse"):
        _core.svg1_sparse_attention(q, q, q, geo, m, None, 8, 384, fused=False, return_lse=True)
    monkeypatch.setitem(_core._ATTENTION_DTYPE, "value", "fp8")
    with pytest.raises(ValueError, match="return_lse"):
        _core.svg1_sparse_attention(q, q, q, geo, m, None, 8, 384, return_lse=True)
    monkeypatch.undo()
    _core, calls = _core_setup(monkeypatch)
    for fn in (lambda **kw: _core.svg1_sparse_attention(q, q, q, geo, m, None, 8, 384, **kw),
               lambda **kw: _core.svg1_attention_device_switch(q, q, q, geo, m, dm, None, 8, 384, flag, **kw),
               lambda **kw: _core.dense_attention(q, q, q, 421, **kw)):
        with pytest.raises(ValueError, match="return_lse"):
            fn(q_prescaled=True, return_lse=True)
        with pytest.raises(ValueError, match="return_lse"):
            fn(out_dtype=torch.float32)
        monkeypatch.setattr(_core._dist, "active", lambda: True)
        with pytest.raises(NotImplementedError, match="svg.distributed"):
            fn(return_lse=True)
        monkeypatch.setattr(_core._dist, "active", lambda: False)
    assert not calls
    # CPU tensors never reach an SDPA call with return_lse: the native wrapper refuses them
    monkeypatch.undo()
    with pytest.raises(RuntimeError):
        _core.dense_attention(q, q, q, 421, return_lse=True)


# ---------------------------------------------------------------------------------------------------------
# the float64 identities of the GPU protocol (tests/test_gpu_band_lse_forms.py, section 7)
# ---------------------------------------------------------------------------------------------------------
def test_video_rows_of_two_text_lengths_equal_band_over_video_keys_merged_with_dense_over_text_keys():
    """the hy geometry (750 video keys, 40 text slots) with 11 and with 29 text keys: the video rows of the whole mask == merge(band over
    the video keys under VIDEO_BAND, dense over that video's text keys), and head placement commutes with the partition (it permutes
    video rows and video keys, the text keys are outside it)"""
    Vn, F_, P_ = SC.V, SC.GEOM["F_"], SC.GEOM["P_"]
    band = O.band_mask(Vn, **SC.VIDEO_BAND)
    g = torch.Generator().manual_seed(3)
    for L in (11, 29):
        S, prm, mask, _ = _band_case("hy", **dict(SC.GEOM, L=L))
        real = Vn + L
        assert (S, prm["real_len"], prm["band"]) == (790, real, 256)
        assert torch.equal(mask[:Vn, :Vn], band) and mask[:Vn, Vn:real].all() and not mask[:Vn, real:].any()
        q, k, v = (torch.randn(1, 2, S, 128, generator=g, dtype=torch.float64) for _ in range(3))
        o_ref, lse_ref = SC.masked_attention_lse(q, k, v, mask)
        o_b, lse_b = SC.masked_attention_lse(q[:, :, :Vn], k[:, :, :Vn], v[:, :, :Vn], band)
        o_t, lse_t = attention_lse(q[:, :, :Vn], k[:, :, Vn:real], v[:, :, Vn:real])
        o, lse = merge_states([o_b, o_t], [lse_b, lse_t], return_lse=True)
        assert (o - o_ref[:, :, :Vn]).abs().max() < 1e-12 and (lse - lse_ref[:, :, :Vn]).abs().max() < 1e-12
        # the dense mask of the warm-up steps over the video keys: every video key, merged with the text keys == dense over real_len
        o_d, lse_d = attention_lse(q[:, :, :Vn], k[:, :, :real], v[:, :, :real])
        o_v, lse_v = attention_lse(q[:, :, :Vn], k[:, :, :Vn], v[:, :, :Vn])
        o2, lse2 = merge_states([o_v, o_t], [lse_v, lse_t], return_lse=True)
        assert (o2 - o_d).abs().max() < 1e-12 and (lse2 - lse_d).abs().max() < 1e-12
        # placement: a token-major head's physical rows are a permutation of the logical video rows
        best = torch.tensor([[1, 0]])
        qv, kv, vv = (O.head_placement(x[:, :, :Vn], best, 0, F_, P_, inverse=True) for x in (q, k, v))
        o_p, lse_p = SC.masked_attention_lse(*(O.head_placement(x, best, 0, F_, P_) for x in (qv, kv, vv)), band)
        assert torch.equal(o_p, o_b) and torch.equal(lse_p, lse_b)
