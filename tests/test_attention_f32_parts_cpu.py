"""The fp32-part entries without a GPU — svg_cross_attention_lse_f32, svg_band_attention_lse_f32, svg_varblock_attention_lse_f32 (the
attention kernels handing out a row before its rounding) and svg_merge_attention_states_f32 (the merge that takes such rows and rounds
once): the exports and prototype tables, the argument validation (every check runs on the host before any launch — rows that pass
placeholder pointers are skipped where a GPU is visible, as in test_attention_lse_cpu.py), what the Python wrappers refuse, and the schedule
of svg.distributed.token_sharded_dense_attention(fp32_parts=True) on gloo CPU ranks with torch statements of an fp32 part and of the merge
that rounds once (tests/lse_ops_torch.py).

ref: flashinfer's run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188 (whose parts are 16-bit); the
context-parallel dense attention of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169."""
import ctypes as C
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import svg_oracle as O
from svg import _native as nat

ROOT = Path(__file__).resolve().parent.parent
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
S_ROWS = 1 << 24


def _host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


# ---------------------------------------------------------------------------------------------------------
# exports and prototypes
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_four_entries():
    lib = nat.load()
    for name in ("svg_cross_attention_lse_f32", "svg_merge_attention_states_f32"):
        assert name in nat.SIGNATURES and getattr(lib, name).argtypes == nat.SIGNATURES[name][1]
    assert set(nat.SPARSE_F32_SIGNATURES) == {"svg_band_attention_lse_f32", "svg_varblock_attention_lse_f32"}
    assert not set(nat.SPARSE_F32_SIGNATURES) & (set(nat.SIGNATURES) | set(nat.SPARSE_LSE_SIGNATURES))
    for name, (res, args) in nat.SPARSE_F32_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    # the arguments of the siblings, a float* in the place of o
    assert nat.SIGNATURES["svg_cross_attention_lse_f32"] == nat.SIGNATURES["svg_cross_attention_lse"]
    assert nat.SIGNATURES["svg_merge_attention_states_f32"] == nat.SIGNATURES["svg_merge_attention_states"]
    assert nat.SPARSE_F32_SIGNATURES["svg_band_attention_lse_f32"] == nat.SPARSE_LSE_SIGNATURES["svg_band_attention_lse"]
    assert nat.SPARSE_F32_SIGNATURES["svg_varblock_attention_lse_f32"] == nat.SPARSE_LSE_SIGNATURES["svg_varblock_attention_lse"]
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def _prototypes(header):
    import re

    src = (ROOT / "include" / header).read_text()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)


def test_header_prototypes_match_the_ctypes_signatures_and_call_sites():
    """the checks of tests/test_sparse_attention_lse_cpu.py for include/svg_attn_f32_parts.h against SPARSE_F32_SIGNATURES, and for the two
    prototypes of include/svg_attn.h: every prototype bound and exported, the same class per parameter, o32 a float*, and every call site
    in svg/_native.py passing as many arguments as the signature has.  svg_attn.h includes the header."""
    import ast
    import re

    assert '#include "svg_attn_f32_parts.h"' in (ROOT / "include" / "svg_attn.h").read_text()
    sparse = _prototypes("svg_attn_f32_parts.h")
    assert {n for _, n, _ in sparse} == set(nat.SPARSE_F32_SIGNATURES)
    main = [p for p in _prototypes("svg_attn.h") if p[1] in ("svg_cross_attention_lse_f32", "svg_merge_attention_states_f32")]
    assert len(main) == 2

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
    table = {**nat.SIGNATURES, **nat.SPARSE_F32_SIGNATURES}
    for ret, name, params in sparse + main:
        ps = [x.strip() for x in params.split(",") if x.strip()]
        want = [c_class(x if x.endswith("*") else re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", x)) for x in ps]
        res, args = table[name]
        assert hasattr(lib, name) and [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)
        if name != "svg_merge_attention_states_f32":
            assert re.sub(r"\s+", " ", ps[3]) == "float* o32" and re.sub(r"\s+", " ", ps[4]) == "float* lse", (name, ps[3:5])
        else:
            assert re.sub(r"\s+", " ", ps[0]) == "const float* const* o_parts"
    tree = ast.parse((ROOT / "sparse-videogen_amd" / "svg" / "_native.py").read_text())
    checked = 0
    names = set(nat.SPARSE_F32_SIGNATURES) | {"svg_cross_attention_lse_f32"}
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in names:
            assert not node.keywords and len(node.args) == len(table[node.func.attr][1]), (node.func.attr, node.lineno)
            checked += 1
    assert checked == 3                                  # one call site per attention entry


# ---------------------------------------------------------------------------------------------------------
# svg_cross_attention_lse_f32
# ---------------------------------------------------------------------------------------------------------
def layout_of(H, Sq, Skv, **kw):
    q = nat.TensorStrides(H * Sq * 128, Sq * 128, 128)
    k = nat.TensorStrides(H * Skv * 128, Skv * 128, 128)
    lay = nat.AttnLayout(H, 0, q, k, k, q)
    for name, val in kw.items():
        setattr(lay, name, val)
    return lay


def cross_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=4, Sq=256, Skv=64, D=128, dtype=0, kv_begin=None, kv_end=None, hpw=1, lay=None):
    return [q, k, v, o, lse, BH, Sq, Skv, D, dtype, 1.0, kv_begin, kv_end, hpw, C.byref(lay) if lay is not None else None, None]


CROSS_CASES = [
    ("null_o32", cross_args(o=None), BAD_ARG),
    ("null_o32_before_unsupported_D", cross_args(o=None, D=64), BAD_ARG),
    ("null_lse", cross_args(lse=None), BAD_ARG),
    ("null_q", cross_args(q=None), BAD_ARG),
    ("null_k", cross_args(k=None), BAD_ARG),
    ("null_v", cross_args(v=None), BAD_ARG),
    ("BH0", cross_args(BH=0), BAD_ARG),
    ("Sq0", cross_args(Sq=0), BAD_ARG),
    ("Skv_neg", cross_args(Skv=-5), BAD_ARG),
    ("window_hpw0", cross_args(kv_end=PH, hpw=0), BAD_ARG),
    ("window_hpw_not_dividing", cross_args(kv_end=PH, hpw=3), BAD_ARG),
    ("D64", cross_args(D=64), UNSUPPORTED),
    ("D96", cross_args(D=96), UNSUPPORTED),
    ("dtype_f32", cross_args(dtype=2), UNSUPPORTED),
    ("Sq_rows", cross_args(Sq=S_ROWS), UNSUPPORTED),
    ("Skv_rows", cross_args(Skv=S_ROWS), UNSUPPORTED),
    ("o32_unaligned", cross_args(o=PH + 8), UNSUPPORTED),
    ("layout_heads0", cross_args(lay=layout_of(2, 256, 64, heads_per_batch=0)), BAD_ARG),
    ("layout_q_row_lt_D", cross_args(lay=layout_of(2, 256, 64, q=nat.TensorStrides(2 * 256 * 64, 256 * 64, 64))), BAD_ARG),
]


@pytest.mark.parametrize("args,expected", [c[1:] for c in CROSS_CASES], ids=[c[0] for c in CROSS_CASES])
def test_cross_attention_lse_f32_rejects(args, expected):
    _host_only()
    assert nat.load().svg_cross_attention_lse_f32(*args) == expected


@pytest.mark.parametrize("args", [c[1] for c in CROSS_CASES if "o32" not in c[0]], ids=[c[0] for c in CROSS_CASES if "o32" not in c[0]])
def test_cross_attention_lse_f32_returns_the_siblings_code(args):
    _host_only()
    lib = nat.load()
    rc = lib.svg_cross_attention_lse(*args)
    assert rc != OK and lib.svg_cross_attention_lse_f32(*args) == rc


# ---------------------------------------------------------------------------------------------------------
# svg_band_attention_lse_f32
# ---------------------------------------------------------------------------------------------------------
def mask_of(**kw):
    p = dict(real_len=300, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
    p.update(kw)
    return nat.BandMask(**p)


def band_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=4, S=300, D=128, dtype=0, mask="default", perm=None, lay=None):
    m = mask_of() if mask == "default" else mask
    return [q, k, v, o, lse, BH, S, D, dtype, 1.0, C.byref(m) if m is not None else None, C.byref(perm) if perm is not None else None,
            C.byref(lay) if lay is not None else None, None]


BAND_CASES = [
    ("null_o32", band_args(o=None), BAD_ARG),
    ("null_o32_before_unsupported_D", band_args(o=None, D=64), BAD_ARG),
    ("null_lse", band_args(lse=None), BAD_ARG),
    ("null_lse_before_unsupported_D", band_args(lse=None, D=64), BAD_ARG),
    ("null_q", band_args(q=None), BAD_ARG),
    ("null_k", band_args(k=None), BAD_ARG),
    ("null_v", band_args(v=None), BAD_ARG),
    ("null_mask", band_args(mask=None), BAD_ARG),
    ("BH0", band_args(BH=0), BAD_ARG),
    ("S0", band_args(S=0), BAD_ARG),
    ("mask_real_len_beyond_S", band_args(mask=mask_of(real_len=301)), BAD_ARG),
    ("mask_band_negative", band_args(mask=mask_of(band=-1)), BAD_ARG),
    ("mask_before_unsupported_D", band_args(mask=mask_of(band=-1), D=64), BAD_ARG),
    ("perm_video_beyond_S", band_args(perm=nat.PermDesc(PH, 0, 4, 100)), BAD_ARG),
    ("S_rows", band_args(S=S_ROWS, mask=mask_of(real_len=0)), UNSUPPORTED),
    ("layout_heads0", band_args(lay=layout_of(2, 300, 300, heads_per_batch=0)), BAD_ARG),
    ("layout_heads_not_dividing", band_args(BH=3, lay=layout_of(2, 300, 300)), BAD_ARG),
    ("layout_null_q", band_args(q=None, lay=layout_of(2, 300, 300)), BAD_ARG),
    ("D64", band_args(D=64), UNSUPPORTED),
    ("D96", band_args(D=96), UNSUPPORTED),
    ("dtype_f32", band_args(dtype=2), UNSUPPORTED),
    ("o32_unaligned", band_args(o=PH + 8), UNSUPPORTED),
    ("o32_unaligned_with_layout", band_args(o=PH + 8, lay=layout_of(2, 300, 300)), UNSUPPORTED),
]


@pytest.mark.parametrize("args,expected", [c[1:] for c in BAND_CASES], ids=[c[0] for c in BAND_CASES])
def test_band_attention_lse_f32_rejects(args, expected):
    _host_only()
    assert nat.load().svg_band_attention_lse_f32(*args) == expected


@pytest.mark.parametrize("args", [c[1] for c in BAND_CASES if "o32" not in c[0]], ids=[c[0] for c in BAND_CASES if "o32" not in c[0]])
def test_band_attention_lse_f32_returns_the_siblings_code(args):
    """every argument fault of svg_band_attention_lse comes back with its code"""
    _host_only()
    lib = nat.load()
    rc = lib.svg_band_attention_lse(*args)
    assert rc != OK and lib.svg_band_attention_lse_f32(*args) == rc


# ---------------------------------------------------------------------------------------------------------
# svg_varblock_attention_lse_f32
# ---------------------------------------------------------------------------------------------------------
VB = dict(Hq=4, Hkv=2, Sq=512, Skv=512, QB=4, KB=8)


def vb_need(**kw):
    g = dict(VB)
    g.update(kw)
    return int(nat.load().svg_varblock_workspace_bytes(g["Hq"], g["Hkv"], g["QB"], g["KB"], g["Sq"]))


def vb_args(q=PH, k=PH, v=PH, o=PH, lse=PH, D=128, dtype=0, bmap=PH, qs=PH, ks=PH, ws=PH, ws_bytes=None, lay=None, **kw):
    g = dict(VB)
    g.update(kw)
    if ws_bytes is None:
        ws_bytes = 1 << 30
    return [q, k, v, o, lse, g["Hq"], g["Hkv"], g["Sq"], g["Skv"], D, dtype, 1.0, bmap, qs, ks, g["QB"], g["KB"], None, None, ws, ws_bytes,
            C.byref(lay) if lay is not None else None, None]


def _vb_cases():
    return [
        ("null_o32", vb_args(o=None), BAD_ARG),
        ("null_o32_before_unsupported_D", vb_args(o=None, D=64), BAD_ARG),
        ("null_lse", vb_args(lse=None), BAD_ARG),
        ("null_q", vb_args(q=None), BAD_ARG),
        ("null_k", vb_args(k=None), BAD_ARG),
        ("null_v", vb_args(v=None), BAD_ARG),
        ("null_block_map", vb_args(bmap=None), BAD_ARG),
        ("null_q_sizes", vb_args(qs=None), BAD_ARG),
        ("null_k_sizes", vb_args(ks=None), BAD_ARG),
        ("null_workspace", vb_args(ws=None), BAD_ARG),
        ("Hq0", vb_args(Hq=0), BAD_ARG),
        ("Hq_not_multiple_of_Hkv", vb_args(Hq=3), BAD_ARG),
        ("Sq0", vb_args(Sq=0), BAD_ARG),
        ("QB0", vb_args(QB=0), BAD_ARG),
        ("KB_beyond_run_list", vb_args(KB=4033), UNSUPPORTED),
        ("Sq_rows", vb_args(Sq=S_ROWS), UNSUPPORTED),
        ("short_workspace", vb_args(ws_bytes=vb_need() - 1), WORKSPACE),
        ("short_workspace_before_unsupported_D", vb_args(ws_bytes=vb_need() - 1, D=64), WORKSPACE),
        ("layout_heads0", vb_args(lay=layout_of(4, 512, 512, heads_per_batch=0)), BAD_ARG),
        ("D64", vb_args(D=64), UNSUPPORTED),
        ("D96", vb_args(D=96), UNSUPPORTED),
        ("dtype_f32", vb_args(dtype=2), UNSUPPORTED),
        ("o32_unaligned", vb_args(o=PH + 8), UNSUPPORTED),
    ]


VB_CASES = _vb_cases()


@pytest.mark.parametrize("args,expected", [c[1:] for c in VB_CASES], ids=[c[0] for c in VB_CASES])
def test_varblock_attention_lse_f32_rejects(args, expected):
    _host_only()
    assert nat.load().svg_varblock_attention_lse_f32(*args) == expected


@pytest.mark.parametrize("args", [c[1] for c in VB_CASES if "o32" not in c[0]], ids=[c[0] for c in VB_CASES if "o32" not in c[0]])
def test_varblock_attention_lse_f32_returns_the_siblings_code(args):
    _host_only()
    lib = nat.load()
    rc = lib.svg_varblock_attention_lse(*args)
    assert rc != OK and lib.svg_varblock_attention_lse_f32(*args) == rc


# ---------------------------------------------------------------------------------------------------------
# svg_merge_attention_states_f32
# ---------------------------------------------------------------------------------------------------------
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
    ("BH0", merge_args(BH=0), BAD_ARG),
    ("Sq0", merge_args(Sq=0), BAD_ARG),
    ("D0", merge_args(D=0), BAD_ARG),
    ("D32", merge_args(D=32), UNSUPPORTED),
    ("D256", merge_args(D=256), UNSUPPORTED),
    ("dtype_f32", merge_args(dtype=2), UNSUPPORTED),                # dtype is that of o: 16-bit
    ("Sq_rows", merge_args(Sq=S_ROWS), UNSUPPORTED),
    ("part_unaligned", merge_args(o_parts=(PH, PH + 8)), UNSUPPORTED),
    ("o_unaligned", merge_args(o=PH + 8), UNSUPPORTED),
    ("layout_heads0", merge_args(lay=layout_of(2, 256, 64, heads_per_batch=0)), BAD_ARG),
    ("layout_o_row_lt_D", merge_args(lay=layout_of(2, 256, 64, o=nat.TensorStrides(2 * 256 * 64, 256 * 64, 64))), BAD_ARG),
]


@pytest.mark.parametrize("args,expected", [c[1:] for c in MERGE_CASES], ids=[c[0] for c in MERGE_CASES])
def test_merge_attention_states_f32_rejects(args, expected):
    """(the pointer ARRAYS are real host memory; what they hold are placeholders) — and the 16-bit entry gives the same code"""
    _host_only()
    lib = nat.load()
    assert lib.svg_merge_attention_states_f32(*args) == expected
    assert lib.svg_merge_attention_states(*args) == expected


# ---------------------------------------------------------------------------------------------------------
# the Python wrappers: raised before anything is launched (CPU tensors get this far)
# ---------------------------------------------------------------------------------------------------------
def _wrapper_calls():
    q = torch.zeros(1, 2, 64, 128, dtype=torch.bfloat16)
    q3 = q[0]
    end = torch.tensor([64], dtype=torch.int32)
    mask = nat.BandMask(**O.dense_band_params(64))
    bmap = torch.ones(2, 1, 1, dtype=torch.bool)
    sz = torch.full((2, 1), 64, dtype=torch.int32)
    return q, {
        "cross_attention": lambda **kw: nat.cross_attention(q, q, q, **kw),
        "cross_attention_keyrange": lambda **kw: nat.cross_attention_keyrange(q, q, q, end, **kw),
        "band_attention": lambda **kw: nat.band_attention(q, q, q, mask, **kw),
        "varblock_attention": lambda **kw: nat.varblock_attention(q3, q3, q3, bmap, sz, sz, **kw),
    }


@pytest.mark.parametrize("name", ["cross_attention", "cross_attention_keyrange", "band_attention", "varblock_attention"])
def test_wrappers_refuse_out_dtype_without_its_conditions(name):
    q, calls = _wrapper_calls()
    call = calls[name]
    with pytest.raises(ValueError, match="return_lse"):
        call(out_dtype=torch.float32)                                   # without return_lse
    with pytest.raises(ValueError, match="token_major_out"):
        call(out_dtype=torch.float32, return_lse=True, token_major_out=True)
    if name != "varblock_attention":                                    # (varblock_attention has no `out`)
        with pytest.raises(ValueError, match="out"):
            call(out_dtype=torch.float32, return_lse=True, out=torch.empty_like(q))
    with pytest.raises(ValueError, match="out_dtype"):
        call(out_dtype=torch.float16, return_lse=True)                  # only None and torch.float32
    with pytest.raises(RuntimeError):                                   # a valid combination goes on to the tensor checks: CPU tensors
        call(out_dtype=torch.float32, return_lse=True)


def test_wrappers_without_an_lse_form_raise_as_return_lse_does():
    """no fall-back: the forms return_lse=True refuses are refused with out_dtype too"""
    q = torch.zeros(1, 2, 64, 128, dtype=torch.bfloat16)
    q64 = torch.zeros(1, 2, 64, 64, dtype=torch.bfloat16)
    mask = nat.BandMask(**O.dense_band_params(64))
    for kw in (dict(variant=1), dict(q_prescaled=True), dict(done=torch.zeros(4, dtype=torch.int32))):
        with pytest.raises(ValueError, match="return_lse"):
            nat.band_attention(q, q, q, mask, return_lse=True, out_dtype=torch.float32, **kw)
    with pytest.raises(ValueError, match="return_lse"):
        nat.band_attention(q64, q64, q64, mask, return_lse=True, out_dtype=torch.float32)
    bmap = torch.ones(2, 1, 1, dtype=torch.bool)
    sz = torch.full((2, 1), 64, dtype=torch.int32)
    for kw in (dict(fp8=True), dict(variant=0), dict(variant=9)):
        with pytest.raises(ValueError, match="return_lse"):
            nat.varblock_attention(q[0], q[0], q[0], bmap, sz, sz, return_lse=True, out_dtype=torch.float32, **kw)


def test_merge_wrapper_dtype_rules():
    p32 = torch.zeros(1, 2, 8, 128)
    p16 = torch.zeros(1, 2, 8, 128, dtype=torch.bfloat16)
    lse = torch.zeros(1, 2, 8)
    with pytest.raises(ValueError, match="one dtype"):
        nat.merge_attention_states([p32, p16], [lse, lse], out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="one dtype"):
        nat.merge_attention_states([p16, p32], [lse, lse])
    with pytest.raises(ValueError, match="out_dtype"):
        nat.merge_attention_states([p32, p32], [lse, lse])              # fp32 parts without an output dtype
    with pytest.raises(ValueError, match="out_dtype"):
        nat.merge_attention_states([p32, p32], [lse, lse], out_dtype=torch.float32)
    with pytest.raises(ValueError, match="out_dtype"):
        nat.merge_attention_states([p32, p32], [lse, lse], out=torch.empty_like(p16), out_dtype=torch.float16)
    with pytest.raises(ValueError, match="1 to 8"):
        nat.merge_attention_states([p32] * 9, [lse] * 9, out_dtype=torch.bfloat16)
    for kw in (dict(out_dtype=torch.bfloat16), dict(out_dtype=torch.float16), dict(out=torch.empty_like(p16))):
        with pytest.raises(RuntimeError):                               # valid: on to the tensor checks, which refuse CPU tensors
            nat.merge_attention_states([p32, p32], [lse, lse], **kw)
    with pytest.raises(RuntimeError):                                   # 16-bit parts: as before
        nat.merge_attention_states([p16, p16], [lse, lse])


# ---------------------------------------------------------------------------------------------------------
# token_sharded_dense_attention(fp32_parts=True) on gloo CPU ranks
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from lse_ops_torch import attention_lse, merge_states
    from svg.distributed import token_range, token_sharded_dense_attention

    dist.init_process_group("gloo", rank=rank, world_size=world)
    dtype = torch.bfloat16
    calls = []

    def attn_fn(q, k, v, return_lse=False):
        """an fp32 part (what the kernels hand out before their rounding); without lse: the plain call, q's dtype"""
        calls.append((k.shape[-2], return_lse, k.dtype))
        o, lse = attention_lse(q.float(), k.float(), v.float())
        return (o, lse) if return_lse else o.to(q.dtype)

    def merge_fn(o_parts, lse_parts):
        assert all(o.dtype == torch.float32 for o in o_parts)
        return merge_states(o_parts, lse_parts).to(dtype)                # one rounding

    H, S, D = 3, 700, 32
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(1, H, S, D, generator=g).to(dtype) for _ in range(3))
    ref = attention_lse(q.double(), k.double(), v.double(), return_lse=False)
    ok, worst = True, 0.0
    for unit in (1, 128):
        tr = [token_range(S, r, world, unit) for r in range(world)]
        a, b = tr[rank]
        ql, kl, vl = (x[:, :, a:b].contiguous() for x in (q, k, v))
        calls.clear()
        o = token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=True, attn_fn=attn_fn, merge_fn=merge_fn, fp32_parts=True)
        ok &= o.shape == ql.shape and o.dtype == dtype
        # the schedule is the one without fp32_parts: one part per rank, the own shard first, then rank - 1, rank - 2, ...
        ok &= calls == [(tr[(rank - j) % world][1] - tr[(rank - j) % world][0], True, dtype) for j in range(world)]
        # the single-process statement of the same arithmetic: this rank's rows over every shard, merged in shard order, rounded once
        parts = [attn_fn(ql, k[:, :, lo:hi].contiguous(), v[:, :, lo:hi].contiguous(), True) for lo, hi in tr]
        ok &= bool(torch.equal(o, merge_fn([p[0] for p in parts], [p[1] for p in parts])))
        # one rounding of an fp32 result: within half a bf16 step (2^-8 relative) of the float64 attention over all keys
        d = (o.double() - ref[:, :, a:b]).abs() - 2.0 ** -8 * ref[:, :, a:b].abs()
        worst = max(worst, d.max().item())
        calls.clear()
        base = token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=False, attn_fn=attn_fn, merge_fn=merge_fn, fp32_parts=True)
        ok &= calls == [(S, False, dtype)] and base.dtype == dtype      # overlap=False: untouched
    ret[rank] = (bool(ok), worst)
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_dense_attention_fp32_parts_gloo(world):
    """ragged token_range (700 tokens: unit 1 -> 234 / 233 / 233 on three ranks, unit 128 -> 256 / 256 / 188; 384 / 316 on two): every
    rank's rows are bit-identical to the single-process statement, and one rounding away from the float64 result"""
    mgr = mp.Manager()
    ret = mgr.dict()
    port = 45500 + (os.getpid() % 2000) + world
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == list(range(world))
    for rank, (ok, worst) in got.items():
        assert ok, rank
        assert worst <= 1e-5, (rank, worst)


def test_fp32_parts_selects_the_native_fp32_calls(monkeypatch):
    """with the default functions the steps ask for out_dtype=torch.float32 and the merge for q's dtype; world == 1 is the plain call"""
    from svg import distributed as sd

    seen = []
    monkeypatch.setattr(nat, "cross_attention", lambda q, k, v, **kw: seen.append(kw) or q)
    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 1)
    x = torch.zeros(1, 2, 16, 128, dtype=torch.float16)
    assert sd.token_sharded_dense_attention(x, x, x, 16, fp32_parts=True) is x and seen == [{}]
    sd._native_attn_f32(x, x, x, True)
    assert seen[1] == dict(return_lse=True, out_dtype=torch.float32)
