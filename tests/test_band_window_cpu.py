"""Band attention over a row window and a key window of the mask without a GPU (include/svg_attn_band_window.h:
svg_band_window_attention_lse[_f32]; _native.band_window_attention / band_window_has_keys; svg.distributed.band_exchange_plan /
token_sharded_band_attention): the exports and prototypes, the argument validation in the order the header states (every check runs on the
host before any launch — rows that pass placeholder pointers are skipped where a GPU is visible, as in test_band_lse_forms_cpu.py), what the
wrapper refuses, the closed form of band_window_has_keys against the element mask, the float64 identity the GPU protocol of
tests/test_gpu_band_window.py rests on, and the schedule of token_sharded_band_attention on gloo CPU ranks.

ref: the context-parallel attention of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169 (dense only); flashinfer's
run(..., return_lse=True) + merge_state, svg/kernels/ops/attention_ops.py:178-188."""
import ctypes as C
import random
import re
from pathlib import Path

import pytest
import torch

import sparse_lse_cases as SC
from gloo_ranks import CountingAllToAll, run_ranks
from lse_ops_torch import attention_lse, merge_states
from oracle import svg_oracle as O
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2   # include/svg_attn.h
PH = 0x10000                           # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("svg_band_window_attention_lse", "svg_band_window_attention_lse_f32")


def _host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


# ---------------------------------------------------------------------------------------------------------
# exports and prototypes
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_window_entries():
    lib = nat.load()
    assert set(nat.BAND_WINDOW_SIGNATURES) == set(NAMES)
    others = (set(nat.SIGNATURES) | set(nat.SPARSE_LSE_SIGNATURES) | set(nat.SPARSE_F32_SIGNATURES) | set(nat.BAND_LSE_FORM_SIGNATURES))
    assert not set(NAMES) & others
    for name, (res, args) in nat.BAND_WINDOW_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_prototypes_match_the_ctypes_signatures():
    assert '#include "svg_attn_band_window.h"' in (ROOT / "include" / "svg_attn.h").read_text()
    src = (ROOT / "include" / "svg_attn_band_window.h").read_text()
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
        res, args = nat.BAND_WINDOW_SIGNATURES[name]
        assert hasattr(lib, name) and [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


# ---------------------------------------------------------------------------------------------------------
# argument validation, in the header's order: pointers, geometry, mask, layout (BAD_ARG); then what has no window form (UNSUPPORTED)
# ---------------------------------------------------------------------------------------------------------
def _mask(S, **kw):
    m = nat.BandMask(S, 64, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _layout(Sq, Sk, H=2, row=128, **kw):
    q = nat.TensorStrides(H * Sq * row, Sq * row, row)
    k = nat.TensorStrides(H * Sk * row, Sk * row, row)
    lay = nat.AttnLayout(H, 0, q, k, k, q)
    for name, val in kw.items():
        setattr(lay, name, val)
    return lay


def window_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=2, S=1024, q_begin=256, Sq=300, k_begin=128, Sk=500, D=128, dtype=0, m="ok", null_mask=False,
                lay=None):
    m = _mask(S) if m == "ok" else m
    return [q, k, v, o, lse, BH, S, q_begin, Sq, k_begin, Sk, D, dtype, 1.0, None if null_mask else C.byref(m),
            C.byref(lay) if lay is not None else None, None]


BAD_ROW = nat.TensorStrides(2 * 300 * 128, 300 * 128, 64)        # a row stride below D
UNALIGNED_ROW = nat.TensorStrides(2 * 300 * 132, 300 * 132, 132)   # rows that are no multiple of 16 bytes
CASES = [
    ("null_q", dict(q=None), BAD_ARG),
    ("null_k", dict(k=None), BAD_ARG),
    ("null_v", dict(v=None), BAD_ARG),
    ("null_o", dict(o=None), BAD_ARG),                              # (o32 of the _f32 form)
    ("null_lse", dict(lse=None), BAD_ARG),
    ("null_mask", dict(null_mask=True), BAD_ARG),
    ("null_lse_before_unsupported_D", dict(lse=None, D=64), BAD_ARG),
    ("null_o_before_a_misaligned_k_begin", dict(o=None, k_begin=32), BAD_ARG),
    ("BH0", dict(BH=0), BAD_ARG),
    ("S0", dict(S=0), BAD_ARG),
    ("Sq0", dict(Sq=0), BAD_ARG),
    ("Sk_negative", dict(Sk=-4), BAD_ARG),
    ("q_begin_negative", dict(q_begin=-1), BAD_ARG),
    ("k_begin_negative", dict(k_begin=-64), BAD_ARG),
    ("row_window_ends_behind_S", dict(q_begin=800, Sq=225), BAD_ARG),
    ("key_window_ends_behind_S", dict(k_begin=640, Sk=385), BAD_ARG),
    ("key_window_ends_behind_S_int32", dict(k_begin=2 ** 31 - 64, Sk=2 ** 31 - 1), BAD_ARG),
    ("geometry_before_unsupported_D", dict(Sq=0, D=64), BAD_ARG),
    ("geometry_before_a_misaligned_k_begin", dict(q_begin=900, k_begin=32), BAD_ARG),
    ("bad_mask_band", dict(m=_mask(1024, band=-1)), BAD_ARG),
    ("bad_mask_real_len_behind_S", dict(m=_mask(1024, real_len=1025)), BAD_ARG),
    ("bad_mask_before_unsupported_D", dict(m=_mask(1024, band=-1), D=64), BAD_ARG),
    ("bad_mask_before_a_misaligned_k_begin", dict(m=_mask(1024, colfull_lo=5, colfull_hi=4), k_begin=32), BAD_ARG),
    ("bad_layout_heads0", dict(lay=_layout(300, 500, heads_per_batch=0)), BAD_ARG),
    ("bad_layout_row_below_D", dict(lay=_layout(300, 500, q=BAD_ROW)), BAD_ARG),
    ("bad_layout_before_unsupported_D", dict(lay=_layout(300, 500, heads_per_batch=0), D=64), BAD_ARG),
    ("layout_row_unaligned", dict(lay=_layout(300, 500, q=UNALIGNED_ROW)), UNSUPPORTED),
    ("k_begin_32", dict(k_begin=32), UNSUPPORTED),
    ("k_begin_100", dict(k_begin=100, Sk=100), UNSUPPORTED),
    ("D64", dict(D=64), UNSUPPORTED),
    ("D96", dict(D=96), UNSUPPORTED),
    ("dtype_f32", dict(dtype=2), UNSUPPORTED),
    ("S_2pow24", dict(S=1 << 24), UNSUPPORTED),                     # check_rows of the plain entry, on S
    ("BH_S_D_2pow40", dict(BH=1 << 10, S=1 << 23), UNSUPPORTED),
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kw,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_validation_order(kw, expected, name):
    _host_only()
    assert getattr(nat.load(), name)(*window_args(**kw)) == expected


def test_the_table_holds_the_rows_the_header_promises():
    ids = {c[0] for c in CASES}
    for want in ("bad_mask_before_unsupported_D", "key_window_ends_behind_S", "row_window_ends_behind_S", "k_begin_32", "null_lse", "null_o"):
        assert want in ids


def test_misaligned_o32_is_unsupported_and_argument_faults_come_first():
    _host_only()
    lib = nat.load()
    assert lib.svg_band_window_attention_lse_f32(*window_args(o=PH + 8)) == UNSUPPORTED
    assert lib.svg_band_window_attention_lse_f32(*window_args(o=PH + 8, m=_mask(1024, real_len=1025))) == BAD_ARG
    assert lib.svg_band_window_attention_lse_f32(*window_args(o=PH + 8, q_begin=1000)) == BAD_ARG
    assert lib.svg_band_window_attention_lse(*window_args(o=PH + 8, D=64)) == UNSUPPORTED   # (a 16-bit o has no such rule; D has)


# ---------------------------------------------------------------------------------------------------------
# the wrapper: what has no window form raises before anything runs (CPU tensors get this far)
# ---------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_has_no_window_form(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda *a, **k: pytest.fail("nothing may be loaded or launched"))
    m = _mask(512)
    q, k = torch.zeros(1, 2, 100, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 128, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.band_window_attention(q, k, k, m, 512, 0, 64)
    with pytest.raises(ValueError, match="out_dtype"):
        nat.band_window_attention(q, k, k, m, 512, 0, 64, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="without out"):
        nat.band_window_attention(q, k, k, m, 512, 0, 64, out_dtype=torch.float32, out=torch.zeros_like(q))
    monkeypatch.setattr(nat, "_gpu", lambda *ts: None)   # (as if the tensors were on a GPU: the checks behind the device check)
    q64, k64 = q[..., :64], k[..., :64]
    with pytest.raises(ValueError, match="head_dim 128"):
        nat.band_window_attention(q64, k64, k64, m, 512, 0, 64)
    with pytest.raises(ValueError, match="head_dim 128"):
        nat.band_window_attention(q.float(), k.float(), k.float(), m, 512, 0, 64)
    with pytest.raises(ValueError, match="multiple of 64"):
        nat.band_window_attention(q, k, k, m, 512, 0, 32)
    with pytest.raises(ValueError, match="outside"):
        nat.band_window_attention(q, k, k, m, 512, 450, 64)
    with pytest.raises(ValueError, match="outside"):
        nat.band_window_attention(q, k, k, m, 512, 0, 448)
    with pytest.raises(ValueError, match="one dtype"):
        nat.band_window_attention(q, k, k.half(), m, 512, 0, 64)


# ---------------------------------------------------------------------------------------------------------
# band_window_has_keys against the element mask
# ---------------------------------------------------------------------------------------------------------
def _brute(mask_params, S, q_range, k_range):
    em = O.band_mask(S, **mask_params)
    return bool(em[q_range[0]:q_range[1], k_range[0]:k_range[1]].any())


def _random_mask(rng, S):
    real = rng.choice([S, S, rng.randint(0, S)])
    a, b = sorted(rng.randint(0, S) for _ in range(2))
    c, d = sorted(rng.randint(0, S) for _ in range(2))
    return dict(real_len=real, band=rng.choice([0, 1, 2, rng.randint(0, S + 1), rng.randint(0, 64)]),
                colfull_lo=a, colfull_hi=rng.choice([a, b]), rowfull_lo=c, rowfull_hi=rng.choice([c, d]))


def test_band_window_has_keys_on_random_masks_and_rectangles():
    rng = random.Random(11)
    seen = {True: 0, False: 0}
    for _ in range(300):
        S = rng.randint(1, 400)
        prm = _random_mask(rng, S)
        em = O.band_mask(S, **prm)
        for _ in range(8):
            q0, q1 = sorted(rng.randint(0, S) for _ in range(2))
            k0, k1 = sorted(rng.randint(0, S) for _ in range(2))
            want = bool(em[q0:q1, k0:k1].any())
            assert nat.band_window_has_keys(nat.BandMask(**prm), S, (q0, q1), (k0, k1)) == want, (S, prm, (q0, q1), (k0, k1))
            seen[want] += 1
    assert seen[True] > 250 and seen[False] > 250      # both answers occur (300 masks, 2400 rectangles)


@pytest.mark.parametrize("model", SC.BAND_MODELS)
def test_band_window_has_keys_on_the_model_masks(model):
    S, prm, em, _ = SC.band_case(model)
    cuts = [0, 1, 150, 256, 300, 384, 601, 640, 750, 761, S - 1, S]
    for q0 in cuts:
        for q1 in cuts:
            for k0 in cuts:
                for k1 in cuts:
                    want = bool(em[q0:q1, k0:k1].any()) if q1 > q0 and k1 > k0 else False
                    assert nat.band_window_has_keys(nat.BandMask(**prm), S, (q0, q1), (k0, k1)) == want, (q0, q1, k0, k1)


def test_band_exchange_plan_is_the_table_of_has_keys():
    from svg.distributed import band_exchange_plan, token_range

    S, prm, em, _ = SC.band_case("wan")
    narrow = dict(prm, band=257)
    for world in (1, 2, 3, 5):
        for p in (prm, narrow):
            plan = band_exchange_plan(nat.BandMask(**p), S, world, 128)
            emp = O.band_mask(S, **p)
            tr = [token_range(S, r, world, 128) for r in range(world)]
            assert plan == [[bool(emp[a:b, c:d].any()) for c, d in tr] for a, b in tr]
    assert band_exchange_plan(nat.BandMask(**narrow), S, 3, 128)[0] == [True, True, False]


# ---------------------------------------------------------------------------------------------------------
# the float64 identity: the parts of a row window over key windows that cover the sequence merge to the whole
# ---------------------------------------------------------------------------------------------------------
ROW_CUTS = [[0, 256, 640], [0, 300, 601]]
KEY_CUTS = [0, 256, 640]


def windows(cuts, S):
    return list(zip(cuts, cuts[1:] + [S]))


@pytest.mark.parametrize("model", SC.BAND_MODELS)
def test_window_parts_merge_to_the_whole_float64(model):
    S, _, em, _ = SC.band_case(model)
    q, k, v = (x.double() for x in SC.band_inputs(model, torch.bfloat16))
    o_ref, lse_ref = SC.band_reference(model, torch.bfloat16)
    empty_rows = 0
    for row_cuts in ROW_CUTS:
        for a, b in windows(row_cuts, S):
            parts = [SC.masked_attention_lse(q[:, :, a:b], k[:, :, c:d], v[:, :, c:d], em[a:b, c:d]) for c, d in windows(KEY_CUTS, S)]
            empty_rows += sum(int((~torch.isfinite(l)).sum()) for _, l in parts)
            o, lse = merge_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
            assert (o - o_ref[:, :, a:b]).abs().max() <= 1e-12
            fin = torch.isfinite(lse_ref[:, :, a:b])
            assert torch.equal(torch.isfinite(lse), fin) and (lse[fin] - lse_ref[:, :, a:b][fin]).abs().max() <= 1e-12
    if model == "wan":
        assert empty_rows > 0      # rows that see no key of a window exist: the first rows against the last key window


# ---------------------------------------------------------------------------------------------------------
# token_sharded_band_attention on gloo CPU ranks
# ---------------------------------------------------------------------------------------------------------
# wan_narrow: the wan mask of the same geometry with mul = 1.0 (band 257).  With mul = 2.3 (band 385) every pair of three 256-row
# shards of 750 rows holds an allowed element (512 - 255 = 257 < 385), so no pair can be skipped; with band 257 the first rank's rows
# [0, 256) see no key of [512, 750).
GLOO_MASKS = {
    "hy": lambda: (SC.band_case("hy")[0], SC.band_case("hy")[1]),
    "wan": lambda: (SC.band_case("wan")[0], SC.band_case("wan")[1]),
    "wan_narrow": lambda: (SC.V, O.wan_band_params(SC.V, SC.GEOM["F_"], SC.GEOM["P_"], 1.0)),
}


def _worker(rank, world):
    from svg import distributed as sd

    a2a = CountingAllToAll()
    H, D, unit = 2, 16, 128
    out = {}
    for name, make in GLOO_MASKS.items():
        S, prm = make()
        em = O.band_mask(S, **prm)
        mask = nat.BandMask(**prm)
        g = torch.Generator().manual_seed(5)
        q, k, v = (torch.randn(1, H, S, D, generator=g, dtype=torch.float64) for _ in range(3))
        ref = SC.masked_attention_lse(q, k, v, em)[0]
        tr = [sd.token_range(S, r, world, unit) for r in range(world)]
        a, b = tr[rank]
        calls = []

        def attn_fn(q_, k_, v_, q_range, k_range):
            calls.append((tuple(q_range), tuple(k_range)))
            assert q_.shape[-2] == q_range[1] - q_range[0] and k_.shape[-2] == k_range[1] - k_range[0] and k_range[0] % 64 == 0
            return SC.masked_attention_lse(q_, k_, v_, em[q_range[0]:q_range[1], k_range[0]:k_range[1]])

        a2a.reset()
        o = sd.token_sharded_band_attention(q[:, :, a:b].contiguous(), k[:, :, a:b].contiguous(), v[:, :, a:b].contiguous(), S, mask,
                                            unit=unit, attn_fn=attn_fn, merge_fn=merge_states)
        plan = sd.band_exchange_plan(mask, S, world, unit)
        per_tok = 2 * H * D * 8
        want_bytes = sum((tr[s][1] - tr[s][0]) * per_tok for s in range(world) if s != rank and plan[rank][s])
        all_bytes = sum((tr[s][1] - tr[s][0]) * per_tok for s in range(world) if s != rank)
        want_calls = sorted((tr[rank], tr[s]) for s in range(world) if plan[rank][s])
        out[name] = dict(err=(o - ref[:, :, a:b]).abs().max().item(), shape_ok=o.shape == (1, H, b - a, D), received=a2a.received,
                         want_bytes=want_bytes, all_bytes=all_bytes, calls_ok=sorted(calls) == want_calls,
                         own_first=(not calls) or calls[0] == (tr[rank], tr[rank]), skipped=sum(not x for row in plan for x in row))
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_band_attention_gloo(world):
    """ragged shards (790 rows: 384 / 406 and 256 / 256 / 278; 750 rows: 384 / 366 and 256 / 256 / 238), unit 128, float64 statements as
    attn_fn / merge_fn: every rank's rows equal the single-process result to 1e-5, the bytes a rank received are those of the shards
    band_exchange_plan keeps for it, attn_fn ran for exactly those pairs, and the narrow wan mask skips a pair on three ranks"""
    got = run_ranks(_worker, world, 45500)
    for rank, res in got.items():
        for name, r in res.items():
            assert r["shape_ok"] and r["calls_ok"] and r["own_first"], (rank, name, r)
            assert r["err"] <= 1e-5, (rank, name, r["err"])
            assert r["received"] == r["want_bytes"], (rank, name, r)
    if world == 3:
        assert got[0]["wan_narrow"]["skipped"] >= 1
        assert got[0]["wan_narrow"]["received"] < got[0]["wan_narrow"]["all_bytes"]      # rank 0 did not receive the last shard
        assert got[1]["wan_narrow"]["received"] == got[1]["wan_narrow"]["all_bytes"]


def test_token_sharded_band_attention_refuses_a_unit_off_the_key_tiles_and_too_many_parts(monkeypatch):
    from svg import distributed as sd

    x = torch.zeros(1, 2, 100, 16)
    with pytest.raises(ValueError, match="multiple of 64"):
        sd.token_sharded_band_attention(x, x, x, 100, _mask(100), unit=32)
    # nine ranks: refused where a rank sees nine shards (a dense mask), accepted where the band keeps it to three
    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 9)
    S = 9 * 128
    x = torch.zeros(1, 2, 128, 16, dtype=torch.float64)
    with pytest.raises(ValueError, match="at most 8 parts"):
        sd.token_sharded_band_attention(x, x, x, S, nat.BandMask(**O.dense_band_params(S)))
    plan = sd.band_exchange_plan(_mask(S, band=100), S, 9, 128)
    assert max(sum(row) for row in plan) == 3
    seen = []
    monkeypatch.setattr(sd.dist, "all_to_all_single", lambda *a, **k: pytest.fail("refused or not: decided before the first collective"))
    with pytest.raises(pytest.fail.Exception):
        sd.token_sharded_band_attention(x, x, x, S, _mask(S, band=100), attn_fn=lambda *a: seen.append(a[3:]) or (a[0], a[0][..., 0]),
                                        merge_fn=lambda o, l: o[0])
    assert seen == [((0, 128), (0, 128))]               # past the part-count check: the own shard ran, then the first exchange


# ---------------------------------------------------------------------------------------------------------
# one schedule: dense is band under a mask that allows everything
# ---------------------------------------------------------------------------------------------------------
def _dense_is_band_worker(rank, world):
    from svg import distributed as sd

    a2a = CountingAllToAll()
    H, D, unit = 3, 32, 128
    S = {3: 700, 4: 300}[world]
    g = torch.Generator().manual_seed(7)
    q, k, v = (torch.randn(1, H, S, D, generator=g) for _ in range(3))
    ref = attention_lse(q.double(), k.double(), v.double(), return_lse=False).float()
    tr = [sd.token_range(S, r, world, unit) for r in range(world)]
    a, b = tr[rank]
    ql, kl, vl = (x[:, :, a:b].contiguous() for x in (q, k, v))
    o_dense = sd.token_sharded_dense_attention(ql, kl, vl, S, unit=unit, overlap=True, merge_fn=merge_states,
                                               attn_fn=lambda q_, k_, v_, return_lse=False: attention_lse(q_, k_, v_, return_lse=return_lse))
    dense_splits = a2a.splits
    a2a.reset()
    o_band = sd.token_sharded_band_attention(ql, kl, vl, S, nat.BandMask(**O.dense_band_params(S)), unit=unit, merge_fn=merge_states,
                                             attn_fn=lambda q_, k_, v_, q_range, k_range: attention_lse(q_, k_, v_, return_lse=True))
    return dict(rows=[hi - lo for lo, hi in tr], shapes=(tuple(o_dense.shape), tuple(o_band.shape)), equal=torch.equal(o_dense, o_band),
                err=max((o - ref[:, :, a:b]).abs().max().item() if b > a else 0.0 for o in (o_dense, o_band)),
                dense_splits=dense_splits, band_splits=a2a.splits)


@pytest.mark.parametrize("world,rows", [(3, [256, 256, 188]), (4, [128, 128, 0, 44])])
def test_token_sharded_dense_attention_is_band_attention_under_a_dense_mask_gloo(world, rows):
    """float32 inputs, the torch statements as attn_fn / merge_fn of both: on every rank token_sharded_dense_attention(overlap=True) and
    token_sharded_band_attention under a mask that allows everything return the same bits, within 1e-5 of the single-process float64
    result.  Three ranks (700 rows): both post the same exchanges.  Four ranks (300 rows, one rank without rows, which returns
    [1, 3, 0, 32] from both): dense sends to the empty rank and band does not, so the split lists are not compared there."""
    got = run_ranks(_dense_is_band_worker, world, 27500)
    for rank, r in got.items():
        assert r["rows"] == rows
        assert r["shapes"] == ((1, 3, rows[rank], 32),) * 2, (rank, r["shapes"])
        assert r["equal"], rank
        assert r["err"] <= 1e-5, (rank, r["err"])
        if world == 3:
            assert r["dense_splits"] == r["band_splits"] and len(r["dense_splits"]) == 2, (rank, r["dense_splits"], r["band_splits"])
