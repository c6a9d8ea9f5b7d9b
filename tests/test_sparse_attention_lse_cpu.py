"""svg_band_attention_lse / svg_varblock_attention_lse without a GPU: the exports, the argument validation (every check runs on the host
before any launch — rows that pass placeholder pointers are skipped where a GPU is visible, as in test_attention_lse_cpu.py), the
combinations the Python wrappers refuse, and the two float64 identities the GPU protocols of tests/test_gpu_sparse_attention_lse.py rest on
(tests/lse_ops_torch.py, tests/sparse_lse_cases.py).

ref: BlockSparseAttentionWrapper.run(..., return_lse=True) over video x video, a dense call over video x text, merge_state:
svg/kernels/ops/attention_ops.py:178-188."""
import ctypes as C

import pytest
import torch

import sparse_lse_cases as SC
from lse_ops_torch import attention_lse, merge_states
from oracle import svg_oracle as O
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
S_ROWS = 1 << 24


def test_library_exports_sparse_lse_entries():
    lib = nat.load()
    assert set(nat.SPARSE_LSE_SIGNATURES) == {"svg_band_attention_lse", "svg_varblock_attention_lse"}
    assert not set(nat.SPARSE_LSE_SIGNATURES) & set(nat.SIGNATURES)
    for name, (res, args) in nat.SPARSE_LSE_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_sparse_lse_header_prototypes_match_the_ctypes_signatures_and_call_sites():
    """tests/test_boundary_cpu.py checks include/svg_attn.h against SIGNATURES; the same three checks for include/svg_attn_sparse_lse.h
    against SPARSE_LSE_SIGNATURES: every prototype bound and exported, the same class per parameter, and every call site in
    svg/_native.py passing as many arguments as the signature has.  svg_attn.h includes the header."""
    import ast
    import re
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    assert '#include "svg_attn_sparse_lse.h"' in (root / "include" / "svg_attn.h").read_text()
    src = (root / "include" / "svg_attn_sparse_lse.h").read_text()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert {n for _, n, _ in protos} == set(nat.SPARSE_LSE_SIGNATURES)

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
        res, args = nat.SPARSE_LSE_SIGNATURES[name]
        assert hasattr(lib, name) and [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)
    tree = ast.parse((root / "sparse-videogen_amd" / "svg" / "_native.py").read_text())
    checked = 0
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in nat.SPARSE_LSE_SIGNATURES:
            assert not node.keywords and len(node.args) == len(nat.SPARSE_LSE_SIGNATURES[node.func.attr][1]), (node.func.attr, node.lineno)
            checked += 1
    assert checked == 2                                  # one call site per entry: the layout (or NULL) is an argument


# ---------------------------------------------------------------------------------------------------------
# svg_band_attention_lse
# ---------------------------------------------------------------------------------------------------------
def mask_of(**kw):
    p = dict(real_len=300, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
    p.update(kw)
    return nat.BandMask(**p)


def contiguous_layout(H, Sq, Skv, **kw):
    q = nat.TensorStrides(H * Sq * 128, Sq * 128, 128)
    k = nat.TensorStrides(H * Skv * 128, Skv * 128, 128)
    lay = nat.AttnLayout(H, 0, q, k, k, q)
    for name, val in kw.items():
        setattr(lay, name, val)
    return lay


def band_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=4, S=300, D=128, dtype=0, mask="default", perm=None, lay=None):
    m = mask_of() if mask == "default" else mask
    return [q, k, v, o, lse, BH, S, D, dtype, 1.0, C.byref(m) if m is not None else None, C.byref(perm) if perm is not None else None,
            C.byref(lay) if lay is not None else None, None]


BAND_CASES = [
    ("null_lse", band_args(lse=None), BAD_ARG),
    ("null_lse_before_unsupported_D", band_args(lse=None, D=64), BAD_ARG),
    ("null_q", band_args(q=None), BAD_ARG),
    ("null_k", band_args(k=None), BAD_ARG),
    ("null_v", band_args(v=None), BAD_ARG),
    ("null_o", band_args(o=None), BAD_ARG),
    ("null_mask", band_args(mask=None), BAD_ARG),
    ("BH0", band_args(BH=0), BAD_ARG),
    ("S0", band_args(S=0), BAD_ARG),
    ("mask_real_len_beyond_S", band_args(mask=mask_of(real_len=301)), BAD_ARG),
    ("mask_band_negative", band_args(mask=mask_of(band=-1)), BAD_ARG),
    ("mask_colfull_reversed", band_args(mask=mask_of(colfull_lo=9, colfull_hi=3)), BAD_ARG),
    ("mask_before_unsupported_D", band_args(mask=mask_of(band=-1), D=64), BAD_ARG),
    ("perm_video_beyond_S", band_args(perm=nat.PermDesc(PH, 0, 4, 100)), BAD_ARG),
    ("S_rows", band_args(S=S_ROWS, mask=mask_of(real_len=0)), UNSUPPORTED),
    ("layout_heads0", band_args(lay=contiguous_layout(2, 300, 300, heads_per_batch=0)), BAD_ARG),
    ("layout_heads_not_dividing", band_args(BH=3, lay=contiguous_layout(2, 300, 300)), BAD_ARG),
    ("layout_before_unsupported_D", band_args(D=64, lay=contiguous_layout(2, 300, 300, heads_per_batch=0)), BAD_ARG),
    ("D64", band_args(D=64), UNSUPPORTED),
    ("D96", band_args(D=96), UNSUPPORTED),
    ("dtype_f32", band_args(dtype=2), UNSUPPORTED),
]


@pytest.mark.parametrize("args,expected", [c[1:] for c in BAND_CASES], ids=[c[0] for c in BAND_CASES])
def test_band_attention_lse_rejects(args, expected):
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert nat.load().svg_band_attention_lse(*args) == expected


@pytest.mark.parametrize("args", [c[1] for c in BAND_CASES if c[1][4] is not None and c[1][12] is None and c[1][7] == 128 and c[1][8] == 0],
                         ids=[c[0] for c in BAND_CASES if c[1][4] is not None and c[1][12] is None and c[1][7] == 128 and c[1][8] == 0])
def test_band_attention_lse_returns_the_plain_entrys_code(args):
    """every argument fault of svg_band_attention comes back with svg_band_attention's code"""
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    lib = nat.load()
    plain = args[:4] + args[5:12] + [0, None]
    rc = lib.svg_band_attention(*plain)
    assert rc != OK and lib.svg_band_attention_lse(*args) == rc


# ---------------------------------------------------------------------------------------------------------
# svg_varblock_attention_lse
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
        ("null_lse", vb_args(lse=None), BAD_ARG),
        ("null_lse_before_unsupported_D", vb_args(lse=None, D=64), BAD_ARG),
        ("null_q", vb_args(q=None), BAD_ARG),
        ("null_k", vb_args(k=None), BAD_ARG),
        ("null_v", vb_args(v=None), BAD_ARG),
        ("null_o", vb_args(o=None), BAD_ARG),
        ("null_block_map", vb_args(bmap=None), BAD_ARG),
        ("null_q_sizes", vb_args(qs=None), BAD_ARG),
        ("null_k_sizes", vb_args(ks=None), BAD_ARG),
        ("null_workspace", vb_args(ws=None), BAD_ARG),
        ("Hq0", vb_args(Hq=0), BAD_ARG),
        ("Hq_not_multiple_of_Hkv", vb_args(Hq=3), BAD_ARG),
        ("Sq0", vb_args(Sq=0), BAD_ARG),
        ("Skv_neg", vb_args(Skv=-1), BAD_ARG),
        ("QB0", vb_args(QB=0), BAD_ARG),
        ("KB0", vb_args(KB=0), BAD_ARG),
        ("KB_beyond_run_list", vb_args(KB=4033), UNSUPPORTED),
        ("Sq_rows", vb_args(Sq=S_ROWS), UNSUPPORTED),
        ("short_workspace", vb_args(ws_bytes=vb_need() - 1), WORKSPACE),
        ("short_workspace_before_unsupported_D", vb_args(ws_bytes=vb_need() - 1, D=64), WORKSPACE),
        ("layout_heads0", vb_args(lay=contiguous_layout(4, 512, 512, heads_per_batch=0)), BAD_ARG),
        ("D64", vb_args(D=64), UNSUPPORTED),
        ("D96", vb_args(D=96), UNSUPPORTED),
        ("dtype_f32", vb_args(dtype=2), UNSUPPORTED),
    ]


VB_CASES = _vb_cases()


@pytest.mark.parametrize("args,expected", [c[1:] for c in VB_CASES], ids=[c[0] for c in VB_CASES])
def test_varblock_attention_lse_rejects(args, expected):
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert nat.load().svg_varblock_attention_lse(*args) == expected


_VB_PLAIN = [c for c in VB_CASES if c[1][4] is not None and c[1][21] is None and c[1][9] == 128 and c[1][10] == 0]


@pytest.mark.parametrize("args", [c[1] for c in _VB_PLAIN], ids=[c[0] for c in _VB_PLAIN])
def test_varblock_attention_lse_returns_the_plain_entrys_code(args):
    """every argument fault of svg_varblock_attention (variant 3) comes back with svg_varblock_attention's code"""
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    lib = nat.load()
    plain = args[:4] + args[5:21] + [3, None]
    rc = lib.svg_varblock_attention(*plain)
    assert rc != OK and lib.svg_varblock_attention_lse(*args) == rc


# ---------------------------------------------------------------------------------------------------------
# the Python wrappers: combinations without an LSE form raise before anything is loaded or launched (CPU tensors get this far)
# ---------------------------------------------------------------------------------------------------------
def test_band_wrapper_refuses_what_has_no_lse_form():
    q = torch.zeros(1, 2, 64, 128, dtype=torch.bfloat16)
    q64 = torch.zeros(1, 2, 64, 64, dtype=torch.bfloat16)
    mask = nat.BandMask(**O.dense_band_params(64))
    done = torch.zeros(4, dtype=torch.int32)
    for kw in (dict(variant=1), dict(variant=2), dict(variant=3), dict(variant=8), dict(done=done), dict(q_prescaled=True)):
        with pytest.raises(ValueError, match="return_lse"):
            nat.band_attention(q, q, q, mask, return_lse=True, **kw)
    with pytest.raises(ValueError, match="return_lse"):
        nat.band_attention(q64, q64, q64, mask, return_lse=True)
    with pytest.raises(RuntimeError):            # a supported combination goes on to the tensor checks: CPU tensors are refused
        nat.band_attention(q, q, q, mask, return_lse=True)


def test_varblock_wrapper_refuses_what_has_no_lse_form():
    q = torch.zeros(2, 64, 128, dtype=torch.bfloat16)
    q64 = torch.zeros(2, 64, 64, dtype=torch.bfloat16)
    bmap = torch.ones(2, 1, 1, dtype=torch.bool)
    sz = torch.full((2, 1), 64, dtype=torch.int32)
    for kw in (dict(fp8=True), dict(variant=0), dict(variant=1), dict(variant=2), dict(variant=4), dict(variant=5), dict(variant=6),
               dict(variant=7), dict(variant=9)):
        with pytest.raises(ValueError, match="return_lse"):
            nat.varblock_attention(q, q, q, bmap, sz, sz, return_lse=True, **kw)
    with pytest.raises(ValueError, match="return_lse"):
        nat.varblock_attention(q64, q64, q64, bmap, sz, sz, return_lse=True)
    for variant in (-1, 3, 8):
        with pytest.raises(RuntimeError):        # supported: on to the tensor checks, which refuse CPU tensors
            nat.varblock_attention(q, q, q, bmap, sz, sz, return_lse=True, variant=variant)


# ---------------------------------------------------------------------------------------------------------
# the float64 identities of the GPU protocols
# ---------------------------------------------------------------------------------------------------------
def test_hy_video_rows_equal_band_over_video_keys_merged_with_dense_over_text_keys():
    """(a) F = 5, P = 150, ctx = 40, L = 11, mul = 2.3: the first 750 rows of the hy mask over S = 790 == merge(band over S = 750 with
    real_len 750 / band 256 / no full rows or columns, dense over the text keys [750, 761))"""
    S, prm, mask, _ = SC.band_case("hy")
    Vn, real = SC.V, SC.REAL
    assert (S, Vn, real, prm["band"]) == (790, 750, 761, 256)
    band = O.band_mask(Vn, **SC.VIDEO_BAND)
    assert torch.equal(mask[:Vn, :Vn], band) and mask[:Vn, Vn:real].all() and not mask[:Vn, real:].any()
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(1, 2, S, 128, generator=g, dtype=torch.float64) for _ in range(3))
    o_ref, lse_ref = SC.masked_attention_lse(q, k, v, mask)
    o_band, lse_band = SC.masked_attention_lse(q[:, :, :Vn], k[:, :, :Vn], v[:, :, :Vn], band)
    o_text, lse_text = attention_lse(q[:, :, :Vn], k[:, :, Vn:real], v[:, :, Vn:real])
    o, lse = merge_states([o_band, o_text], [lse_band, lse_text], return_lse=True)
    assert (o - o_ref[:, :, :Vn]).abs().max() < 1e-12 and (lse - lse_ref[:, :, :Vn]).abs().max() < 1e-12
    # and the float64 statement agrees with the oracle's fp32 one
    torch.testing.assert_close(o_ref.float(), O.masked_attention(q, k, v, mask), atol=1e-5, rtol=1e-5)


def test_block_map_split_by_key_clusters_merged_equals_the_whole():
    """(b) a block map split by key-cluster ranges into 3 parts, merged, equals the whole; a row whose keys all lie in one part takes that
    part unchanged (its other parts are -inf, weight 0)"""
    hq, hkv, S, MB, NB = 4, 2, 300, 6, 15
    gen = torch.Generator().manual_seed(4)
    rsz = SC.random_partition_batch(S, MB, hkv, gen)
    csz = SC.random_partition_batch(S, NB, hkv, gen)
    bmap = torch.rand(hkv, MB, NB, generator=gen) < 0.5
    cuts = [0, 4, 11, NB]
    bmap[:, 0] = False
    bmap[:, 0, 1:3] = True                       # block-row 0: keys of part 0 only
    bmap[:, 1] = False                           # block-row 1: no key at all
    q = torch.randn(hq, S, 128, generator=gen, dtype=torch.float64)
    k, v = (torch.randn(hkv, S, 128, generator=gen, dtype=torch.float64) for _ in range(2))
    o_ref, lse_ref = SC.vb_reference_of(q, k, v, bmap, rsz, csz)
    parts = [SC.vb_reference_of(q, k, v, b, rsz, csz) for b in SC.split_key_clusters(bmap, cuts)]
    assert torch.equal(torch.stack(SC.split_key_clusters(bmap, cuts)).sum(0).bool(), bmap)
    o, lse = merge_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
    assert (o - o_ref).abs().max() < 1e-12
    fin = torch.isfinite(lse_ref)
    assert torch.equal(lse[~fin], lse_ref[~fin]) and (lse[fin] - lse_ref[fin]).abs().max() < 1e-12
    g = hq // hkv
    for h in range(hkv):
        r0, r1 = int(rsz[h, 0]), int(rsz[h, :2].sum())
        hs = slice(h * g, (h + 1) * g)
        assert torch.equal(o[hs, :r0], parts[0][0][hs, :r0]) and torch.equal(lse[hs, :r0], parts[0][1][hs, :r0])
        assert (lse_ref[hs, r0:r1] == SC.NINF).all() and (o_ref[hs, r0:r1] == 0).all()
