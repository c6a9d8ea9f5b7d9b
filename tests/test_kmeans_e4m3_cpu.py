"""The e4m3 k-means assignment without a GPU (include/svg_attn_kmeans_e4m3.h): the float64 statement of tests/kmeans_e4m3_cases.py is sound
(on small integers it IS the float64 arg-min) and sharp (the mutant quantisers fail its rule), its near-tie condition holds on every
real-valued case; the exports, the header and its prototypes against the ctypes signatures; the argument validation of the three entries —
every check runs on the host before any launch (rows that pass placeholder pointers are skipped where a GPU is visible, as in
tests/test_kmeans_stepped_cpu.py) —; and the refusals of the Python layer."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import kmeans_e4m3_cases as EC
import kmeans_exact_cases as KC
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH, PA, PB, PC = 0x10000, 0x20000, 0x30000, 0x40000   # placeholder device pointers (16-byte aligned; never dereferenced by a rejected call)
ROOT = Path(__file__).resolve().parent.parent
ENTRIES = {"svg_kmeans_centre", "svg_kmeans_assign_e4m3_workspace_bytes", "svg_kmeans_assign_e4m3", "svg_kmeans_loop_e4m3_workspace_bytes",
           "svg_kmeans_loop_e4m3"}
BIG = 1 << 40
D = EC.D


# ---------------------------------------------------------------------------------------------------------
# the statement: sound on exact inputs, its condition on real ones, sharp against mutants
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", KC.DTYPES, ids=str)
def test_integers_survive_the_quantiser(dtype):
    """integers in [-3, 3] times 2^e are e4m3 numbers: the dequantised rows are the rows, with and without the planted offset as mu"""
    x, c = KC.assign_case(257, 129, D, dtype)
    for t in (x, c):
        b, e, r = EC.quantise(t)
        assert torch.equal(EC.dequantise(b, e), t.double()) and int(e.min()) >= 7      # 3 * 2^7 = 384 <= 448 < 768
    xo, co, mu = EC.with_offset(x, c)
    b, e, _ = EC.quantise(xo, mu)
    assert torch.equal(EC.dequantise(b, e), x.double())
    b0, e0, _ = EC.quantise(xo)                                                          # without the centre the offset eats the mantissa
    assert not torch.equal(EC.dequantise(b0, e0), xo.double())


def test_row_exponent_is_the_floor_of_the_logarithm():
    m = torch.tensor([448.0, 448.0001, 447.9999, 224.0, 224.5, 1.0, 0.875, 0.8750001, 3.0, 1e-30, 3e38, 0.0, 2.0 ** -125], dtype=torch.float32)
    e = EC.row_exponent(m[:, None])
    for mi, ei in zip(m.double().tolist(), e.tolist()):
        if mi == 0:
            assert ei == 0
        elif mi < 2.0 ** -118:
            assert ei == 127
        else:
            assert mi * 2.0 ** ei <= 448 < mi * 2.0 ** (ei + 1), (mi, ei)
    assert e[:3].tolist() == [0, -1, 0] and int(e[10]) >= -120


@pytest.mark.parametrize("dtype", KC.DTYPES, ids=str)
@pytest.mark.parametrize("N,K", KC.ASSIGN_SHAPES)
def test_statement_is_the_exact_argmin_on_integers(N, K, dtype):
    x, c = KC.assign_case(N, K, D, dtype)
    ref = KC.assign_ref64(x, c)
    assert torch.equal(EC.assign64(x, c), ref)
    xo, co, mu = EC.with_offset(x, c)
    assert torch.equal(EC.assign64(xo, co, mu), ref)


@pytest.mark.parametrize("dtype", KC.DTYPES, ids=str)
@pytest.mark.parametrize("name", sorted(KC.TIE_SETS))
def test_statement_resolves_planted_ties_to_the_lowest_index(name, dtype):
    x, c = KC.tie_case(name, D, dtype)
    lab = EC.assign64(x, c)
    assert torch.equal(lab, KC.assign_ref64(x, c))
    assert (lab[:, list(KC.TIE_POINTS)] == min(KC.TIE_SETS[name])).all() and (lab[:, KC.ZERO_POINT] == KC.ZERO_CENTROID).all()


@pytest.mark.parametrize("dtype", KC.DTYPES, ids=str)
@pytest.mark.parametrize("kind", KC.REAL_KINDS)
@pytest.mark.parametrize("centred", [True, False], ids=["centred", "not_centred"])
def test_near_tie_share_is_under_the_cap(kind, centred, dtype):
    x, c = KC.real_case(kind, D, dtype)
    mu = EC.centre64(c).float() if centred else None
    share = EC.near_tie_share(x, c, mu)
    print(f"{kind} {dtype} centred={centred}: near-tie share {share:.5f}")
    assert share <= EC.NEAR_TIE_CAP
    EC.check_labels_margin(EC.assign64(x, c, mu), x, c, mu, "the statement under its own rule")


def test_mutant_without_centring_fails_on_outlier_channels():
    x, c = KC.real_case("outlier_channels", D, torch.bfloat16)
    mu = EC.centre64(c).float()
    with pytest.raises(AssertionError, match="differ from the statement's arg-max"):
        EC.check_labels_margin(EC.assign64(x, c, None), x, c, mu, "no centring")
    agree = (EC.assign64(x, c, None) == EC.assign64(x, c, mu)).double().mean().item()
    exact = lambda m: (EC.assign64(x, c, m) == KC.scores64(x, c).argmax(-1)).double().mean().item()   # noqa: E731
    print(f"labels equal to the 16-bit arg-max: centred {exact(mu):.3f}, not centred {exact(None):.3f}; mutant against statement {agree:.3f}")
    assert exact(mu) > 0.85 > exact(None)


@pytest.mark.parametrize("kind", KC.REAL_KINDS)
def test_mutant_that_truncates_fails(kind):
    x, c = KC.real_case(kind, D, torch.float16)
    mu = EC.centre64(c).float()
    with pytest.raises(AssertionError, match="differ from the statement's arg-max"):
        EC.check_labels_margin(EC.assign64(x, c, mu, rounding="truncate"), x, c, mu, "truncation")


def test_mixed_loop_statement_ends_near_the_exact_loop():
    """nine e4m3 assignments and one exact one: the inertia stays within the spread that other initial points give the exact loop"""
    x, _ = KC.real_case("blobs", D, torch.bfloat16)
    n = EC.QUALITY_ITERS

    def inertia(c0, f8):
        lab, cent = EC.mixed_loop64(x, c0, n, f8)
        return float(EC.inertia64(x, cent, lab).sum())

    c0 = EC.initial_points(x, KC.REAL_K, 0)
    base = inertia(c0, 0)
    ratio = inertia(c0, n - 1) / base
    others = [inertia(EC.initial_points(x, KC.REAL_K, d), 0) / base for d in range(1, EC.QUALITY_DRAWS + 1)]
    print(f"mixed / exact inertia {ratio:.4f}; exact loop over other draws {min(others):.4f} .. {max(others):.4f}")
    assert abs(ratio - 1) <= max(others) - min(others)


# ---------------------------------------------------------------------------------------------------------
# exports, header, prototypes
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    lib = nat.load()
    assert set(nat.KMEANS_E4M3_SIGNATURES) == ENTRIES
    others = set()
    for name in dir(nat):
        if (name.endswith("SIGNATURES") or name.endswith("ENTRIES")) and name != "KMEANS_E4M3_SIGNATURES" and isinstance(getattr(nat, name), dict):
            others |= set(getattr(nat, name))
    assert "svg_kmeans_loop_grouped_strided" in others and not ENTRIES & others
    for name, (res, args) in nat.KMEANS_E4M3_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4
    for name in ("kmeans_centre", "kmeans_assign_e4m3", "kmeans_loop_e4m3"):
        assert callable(getattr(nat, name))


def test_header_is_included_and_matches_the_signatures():
    main = (ROOT / "include" / "svg_attn.h").read_text()
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', main, flags=re.M)
    assert "svg_attn_kmeans_e4m3.h" in includes
    src = (ROOT / "include" / "svg_attn_kmeans_e4m3.h").read_text()
    assert "in this order" in src and "bit for bit" in src and "SVG_ERR_UNSUPPORTED" in src and "head_dim 64" in src
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
        res, args = nat.KMEANS_E4M3_SIGNATURES[name]
        assert [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)
    # the loop: the argument list of svg_kmeans_loop_grouped_strided plus fp8_iters in front of the workspace
    sib = nat.SIGNATURES["svg_kmeans_loop_grouped_strided"][1]
    assert nat.KMEANS_E4M3_SIGNATURES["svg_kmeans_loop_e4m3"][1] == sib[:18] + [C.c_int32] + sib[18:]


def test_workspace_bytes():
    lib = nat.load()
    loop, assign = lib.svg_kmeans_loop_e4m3_workspace_bytes, lib.svg_kmeans_assign_e4m3_workspace_bytes
    a = assign(4, 700, 129, 128)
    assert a >= 4 * 129 * (128 + 8)
    assert loop(4, 700, 129, 128, 2) >= lib.svg_kmeans_loop_grouped_workspace_bytes(4, 700, 129, 128, 2) + a + 4 * 128 * 4
    for bad in ((4, 700, 129, 128, 3), (4, 700, 129, 128, 0), (0, 700, 129, 128, 1), (4, 0, 129, 128, 2), (4, 700, 0, 128, 2),
                (4, 700, 8193, 128, 2), (4, 700, 129, 64, 2), (4, 700, 129, 96, 2)):
        assert loop(*bad) == 0, bad
    for bad in ((0, 700, 129, 128), (4, 0, 129, 128), (4, 700, 0, 128), (4, 700, 8193, 128), (4, 700, 129, 64)):
        assert assign(*bad) == 0, bad
    assert loop(4, 700, 8192, 128, 2) > 0 and assign(4, 700, 8192, 128) > 0


# ---------------------------------------------------------------------------------------------------------
# the validation table: codes and their order
# ---------------------------------------------------------------------------------------------------------
def host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


def centre_args(c=PA, mu=PH, B=4, K=129, D=128, dtype=0):
    return [c, mu, B, K, D, dtype, None]


def assign_args(x=PH, c=PA, mu=PB, lab=PC, B=4, N=700, K=129, D=128, dtype=0, ws=PH, nb=BIG):
    return [x, c, mu, lab, B, N, K, D, dtype, ws, nb, None]


def loop_args(x=PH, xbs=None, c0=PA, ca=PB, cb=PC, lab=PH, cnt=PH, srt=PH, out=PH, n=PH, B=4, N=700, K=129, D=128, dtype=0, group=2, iters=5,
              tol=1e-4, f8=4, ws=PH, nb=BIG):
    return [x, N * D if xbs is None else xbs, c0, ca, cb, lab, cnt, srt, out, n, B, N, K, D, dtype, group, iters, tol, f8, ws, nb, None]


CENTRE_CASES = [
    ("null_centroids", centre_args(c=None), BAD_ARG),
    ("null_mu", centre_args(mu=None), BAD_ARG),
    ("B0", centre_args(B=0), BAD_ARG),
    ("K_neg", centre_args(K=-1), BAD_ARG),
    ("null_before_unsupported", centre_args(mu=None, D=64), BAD_ARG),
    ("K8193", centre_args(K=8193), UNSUPPORTED),
    ("D64", centre_args(D=64), UNSUPPORTED),
    ("D96", centre_args(D=96), UNSUPPORTED),
    ("dtype_f32", centre_args(dtype=2), UNSUPPORTED),
]

ASSIGN_CASES = [
    ("null_x", assign_args(x=None), BAD_ARG),
    ("null_centroids", assign_args(c=None), BAD_ARG),
    ("null_labels", assign_args(lab=None), BAD_ARG),
    ("null_workspace", assign_args(ws=None), BAD_ARG),
    ("B0", assign_args(B=0), BAD_ARG),
    ("N0", assign_args(N=0), BAD_ARG),
    ("K_neg", assign_args(K=-2), BAD_ARG),
    ("null_before_unsupported", assign_args(lab=None, D=64), BAD_ARG),
    ("K8193", assign_args(K=8193), UNSUPPORTED),
    ("D64", assign_args(D=64), UNSUPPORTED),
    ("dtype_f32", assign_args(dtype=2), UNSUPPORTED),
    ("unsupported_before_workspace", assign_args(D=64, nb=16), UNSUPPORTED),
    ("short_workspace", assign_args(nb=None), WORKSPACE),
    ("workspace_before_alignment", assign_args(nb=None, x=PH + 8), WORKSPACE),
    ("x_not_16_byte_aligned", assign_args(x=PH + 8), UNSUPPORTED),
    ("mu_not_16_byte_aligned", assign_args(mu=PB + 4), UNSUPPORTED),
]

LOOP_CASES = [
    # 1. pointers, then sizes, group and fp8_iters
    ("null_x", loop_args(x=None), BAD_ARG),
    ("null_c_init", loop_args(c0=None), BAD_ARG),
    ("null_work_a", loop_args(ca=None), BAD_ARG),
    ("null_work_b", loop_args(cb=None), BAD_ARG),
    ("null_labels", loop_args(lab=None), BAD_ARG),
    ("null_counts", loop_args(cnt=None), BAD_ARG),
    ("null_sorted", loop_args(srt=None), BAD_ARG),
    ("null_out", loop_args(out=None), BAD_ARG),
    ("null_n_iters", loop_args(n=None), BAD_ARG),
    ("null_workspace", loop_args(ws=None), BAD_ARG),
    ("B0", loop_args(B=0), BAD_ARG),
    ("N_neg", loop_args(N=-1, xbs=128), BAD_ARG),
    ("K0", loop_args(K=0), BAD_ARG),
    ("max_iters0", loop_args(iters=0, f8=0), BAD_ARG),
    ("group0", loop_args(group=0), BAD_ARG),
    ("group_not_dividing_B", loop_args(group=3), BAD_ARG),
    ("fp8_iters_neg", loop_args(f8=-1), BAD_ARG),
    ("fp8_iters_above_max_iters", loop_args(iters=5, f8=6), BAD_ARG),
    ("fp8_iters_before_unsupported", loop_args(f8=6, D=64), BAD_ARG),
    ("null_before_unsupported", loop_args(n=None, K=9000), BAD_ARG),
    # 2. what the kernels do not cover — with fp8_iters = 0 as well
    ("K8193", loop_args(K=8193), UNSUPPORTED),
    ("D64", loop_args(D=64), UNSUPPORTED),
    ("D64_fp8_iters0", loop_args(D=64, f8=0), UNSUPPORTED),
    ("D96", loop_args(D=96), UNSUPPORTED),
    ("dtype_f32", loop_args(dtype=2), UNSUPPORTED),
    ("unsupported_before_workspace", loop_args(dtype=2, nb=16), UNSUPPORTED),
    ("unsupported_before_alias", loop_args(D=64, ca=PA), UNSUPPORTED),
    # 3. the workspace
    ("short_workspace", loop_args(nb=None), WORKSPACE),
    ("workspace_of_the_16_bit_loop_is_short", loop_args(nb="sibling"), WORKSPACE),
    ("workspace_before_alias", loop_args(nb=None, ca=PA), WORKSPACE),
    ("workspace_before_stride", loop_args(nb=None, xbs=8), WORKSPACE),
    # 4. aliased centroid buffers
    ("c_init_is_work_a", loop_args(ca=PA), BAD_ARG),
    ("c_init_is_work_b", loop_args(cb=PA), BAD_ARG),
    ("work_a_is_work_b", loop_args(cb=PB), BAD_ARG),
    ("out_is_work_a", loop_args(out=PB), BAD_ARG),
    ("out_is_work_b", loop_args(out=PC), BAD_ARG),
    ("alias_before_stride", loop_args(cb=PB, xbs=700 * 128 + 4), BAD_ARG),
    # 5. the stride checks of svg_kmeans_loop_strided, with its codes
    ("stride_below_N_D", loop_args(xbs=700 * 128 - 8), BAD_ARG),
    ("stride_not_multiple_of_8", loop_args(xbs=700 * 128 + 4), UNSUPPORTED),
    ("x_not_16_byte_aligned", loop_args(x=PH + 8), UNSUPPORTED),
]


@pytest.mark.parametrize("a,expected", [c[1:] for c in CENTRE_CASES], ids=[c[0] for c in CENTRE_CASES])
def test_centre_rejects(a, expected):
    host_only()
    assert nat.load().svg_kmeans_centre(*a) == expected


@pytest.mark.parametrize("a,expected", [c[1:] for c in ASSIGN_CASES], ids=[c[0] for c in ASSIGN_CASES])
def test_assign_rejects(a, expected):
    host_only()
    if a[10] is None:
        a = list(a)
        a[10] = int(nat.load().svg_kmeans_assign_e4m3_workspace_bytes(*a[4:8])) - 1
        assert a[10] > 0
    assert nat.load().svg_kmeans_assign_e4m3(*a) == expected


@pytest.mark.parametrize("a,expected", [c[1:] for c in LOOP_CASES], ids=[c[0] for c in LOOP_CASES])
def test_loop_rejects(a, expected):
    host_only()
    lib = nat.load()
    if a[20] is None or a[20] == "sibling":
        a = list(a)
        dims = (a[10], a[11], a[12], a[13], a[15])
        a[20] = int(lib.svg_kmeans_loop_e4m3_workspace_bytes(*dims)) - 1 if a[20] is None else int(lib.svg_kmeans_loop_grouped_workspace_bytes(*dims))
        assert a[20] > 0
    assert lib.svg_kmeans_loop_e4m3(*a) == expected


# ---------------------------------------------------------------------------------------------------------
# the Python layer's refusals
# ---------------------------------------------------------------------------------------------------------
def test_batch_kmeans_refuses_fp8_iters_outside_the_library_loop():
    """before the device is looked at: CPU tensors"""
    from svg.kmeans_utils import batch_kmeans_Euclid

    x = torch.zeros(2, 64, 128, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="check_every=0"):
        batch_kmeans_Euclid(x, 4, max_iters=3, fp8_iters=2)                                   # check_every defaults to 1
    with pytest.raises(ValueError, match="shift_reduce"):
        batch_kmeans_Euclid(x, 4, max_iters=3, check_every=0, shift_reduce=lambda t: t, fp8_iters=2)
    with pytest.raises(ValueError, match="outside"):
        batch_kmeans_Euclid(x, 4, max_iters=3, check_every=0, fp8_iters=4)
    with pytest.raises(ValueError, match="outside"):
        batch_kmeans_Euclid(x, 4, max_iters=3, check_every=0, fp8_iters=-1)
    with pytest.raises(AssertionError, match="requires GPU tensors"):                         # 0: today's path, which asks for the GPU
        batch_kmeans_Euclid(x, 4, max_iters=3, check_every=0, fp8_iters=0)


def test_kmeans_clustering_hands_all_but_the_last_iteration_to_e4m3(monkeypatch):
    from svg.models import _core

    seen = []

    def fake(x, K, **kw):
        seen.append(kw)
        B, N, Dd = x.shape
        z = torch.zeros(B, N, dtype=torch.int64)
        return z, torch.zeros(B, K, Dd, dtype=x.dtype), torch.zeros(B, K, dtype=torch.int32), torch.zeros((), dtype=torch.int64), z.to(torch.int32)

    monkeypatch.setattr(_core, "batch_kmeans_Euclid", fake)
    x = torch.zeros(1, 2, 64, 128, dtype=torch.bfloat16)
    for e4m3, want in ((True, [49, 49, 1, 1]), (False, [None] * 4)):
        seen.clear()
        st = _core.CentroidStore()
        _core.kmeans_clustering(st, 0, x, x, 3, 4, 50, 2, e4m3=e4m3)      # the init call, then a step call
        _core.kmeans_clustering(st, 0, x, x, 3, 4, 50, 2, e4m3=e4m3)
        assert [kw.get("fp8_iters") for kw in seen] == want and [kw["max_iters"] for kw in seen] == [50, 50, 2, 2]
    seen.clear()
    _core.kmeans_clustering(_core.CentroidStore(), 0, x, x, 3, 4, 1, 1, e4m3=True)            # one iteration: it is the 16-bit one
    assert ["fp8_iters" in kw for kw in seen] == [False, False]


def test_processors_carry_the_switch_off():
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor

    for cls in (Hunyuan_SAPAttn_Processor2_0, WanAttn_SAPAttn_Processor, Cosmos_SAPAttn_Processor):
        assert cls.__dict__["kmeans_e4m3"] is False


@pytest.mark.parametrize("mode", ["enable", "frame_shards", "token_shards"])
def test_kmeans_e4m3_is_refused_under_every_distributed_mode(monkeypatch, mode):
    import os

    import torch.distributed as dist

    from svg import distributed as sd
    from svg.models import _core
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor

    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{36200 + os.getpid() % 2000}", rank=0, world_size=1)
    try:
        {"enable": sd.enable, "frame_shards": sd.enable_frame_shards, "token_shards": sd.enable_token_shards}[mode]()
        for name in ("all_reduce", "all_to_all_single", "all_gather_into_tensor", "broadcast", "all_gather"):
            monkeypatch.setattr(dist, name, lambda *a, _n=name, **k: pytest.fail(f"{_n}: a collective ran before the refusal"))
        geo = _core.Geometry(0, 2, 64)
        q = torch.zeros(1, 2, geo.seq_len, 128, dtype=torch.bfloat16)
        store = _core.CentroidStore()
        with pytest.raises(NotImplementedError, match="kmeans_e4m3"):
            _core.svg2_sparse_attention(q, q, q, geo, store, 0, 4, 4, 0.9, 0.1, 2, 1, kmeans_e4m3=True)
        with pytest.raises(NotImplementedError, match="kmeans_e4m3"):
            _core.kmeans_clustering(store, 0, q, q, 4, 4, 2, 1, e4m3=True)
        with pytest.raises(NotImplementedError, match="kmeans_e4m3"):
            _core.kmeans_clustering(store, 0, q, q, 4, 4, 2, 1, head_shard=(0, 2, 4), e4m3=True)
        t = torch.tensor([500.0])
        for cls in (WanAttn_SAPAttn_Processor, Hunyuan_SAPAttn_Processor2_0, Cosmos_SAPAttn_Processor):
            for attr, val in (("kmeans_e4m3", True), ("num_frame", 2), ("frame_size", 64), ("context_length", 0), ("prompt_length", 0)):
                monkeypatch.setattr(cls, attr, val, raising=False)
            args = (q, q, q, t, 0, None) if cls is Hunyuan_SAPAttn_Processor2_0 else (q, q, q, t)
            if mode != "frame_shards":                     # (the SVG2 processors refuse that mode itself first, as before)
                with pytest.raises(NotImplementedError, match="kmeans_e4m3"):
                    cls(0).attention_core_logic(*args)
        assert not store.q
    finally:
        sd.disable()
        dist.destroy_process_group()
