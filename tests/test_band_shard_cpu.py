"""Band attention of a frame shard of the rows over a frame shard of the keys without a GPU (include/svg_attn_band_shard.h:
svg_band_shard_attention_lse[_f32], svg_debug_band_shard_map; _native.band_shard_attention / band_shard_has_keys / band_shard_coord[_inv];
svg.distributed.frame_range / frame_shard / band_shard_exchange_plan / token_sharded_svg1_attention): the exports and prototypes, the two
coordinate maps — the library's and the binding's — against brute force, band_shard_has_keys and the plan against the element mask at the
coordinates the model gives a shard's rows (tests/band_shard_cases.py), the argument validation in the order the header states (every check
runs on the host before any launch), what the wrapper refuses, and the schedule of token_sharded_svg1_attention on gloo CPU ranks with
mixed head kinds.

ref: the context-parallel attention of svg/models/wan_orig/distributed/xdit_context_parallel.py:120-169 (dense only); the head placement
of svg/models/hyvideo/placement.py:156-184."""
import bisect
import ctypes as C
import random
import re
from pathlib import Path

import pytest
import torch

import band_shard_cases as BC
import sparse_lse_cases as SC
from gloo_ranks import CountingAllToAll, run_ranks
from lse_ops_torch import merge_states
from oracle import svg_oracle as O
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2   # include/svg_attn.h
PH = 0x10000                           # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("svg_band_shard_attention_lse", "svg_band_shard_attention_lse_f32")
NAMES = ENTRIES + ("svg_debug_band_shard_map",)


def _host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


# ---------------------------------------------------------------------------------------------------------
# exports and prototypes
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_shard_entries():
    lib = nat.load()
    assert set(nat.BAND_SHARD_SIGNATURES) == set(NAMES)
    others = (set(nat.SIGNATURES) | set(nat.SPARSE_LSE_SIGNATURES) | set(nat.SPARSE_F32_SIGNATURES) | set(nat.BAND_LSE_FORM_SIGNATURES)
              | set(nat.BAND_WINDOW_SIGNATURES))
    assert not set(NAMES) & others
    for name, (res, args) in nat.BAND_SHARD_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_prototypes_match_the_ctypes_signatures():
    assert '#include "svg_attn_band_shard.h"' in (ROOT / "include" / "svg_attn.h").read_text()
    src = (ROOT / "include" / "svg_attn_band_shard.h").read_text()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    assert re.search(r"typedef struct svg_band_shard \{\s*int32_t f0, n_frames;\s*int32_t tail_begin, n_tail;\s*\} svg_band_shard_t;", src)
    assert [f for f, _ in nat.BandShard._fields_] == ["f0", "n_frames", "tail_begin", "n_tail"] and C.sizeof(nat.BandShard) == 16
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
        res, args = nat.BAND_SHARD_SIGNATURES[name]
        assert hasattr(lib, name) and [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


# ---------------------------------------------------------------------------------------------------------
# g and ginv against brute force: every (F, Fl, f0) with F <= 7, with and without a tail, video at row 0 and behind 3 rows
# ---------------------------------------------------------------------------------------------------------
def _brute_coords(vid0, F, P, S, shard, token_major):
    """mask coordinates of the shard's rows from the definition: a head in logical order sees sequence row vid0 + f * P + p at its own
    index, a token-major head at vid0 + p * F + f; the tail at its own index.  Sorted: g(l) is the l-th smallest."""
    f0, n, tail0, n_tail = shard
    vid = [(vid0 + p * F + f) if token_major else (vid0 + f * P + p) for f in range(f0, f0 + n) for p in range(P)]
    return sorted(vid) + list(range(tail0, tail0 + n_tail))


def _lib_map(vid0, F, P, S, shard, token_major, xs):
    lib = nat.load()
    pd, sh = nat.PermDesc(None, vid0, F, P), nat.BandShard(*shard)
    arr = (C.c_int32 * len(xs))(*xs)
    g, gi = (C.c_int32 * len(xs))(), (C.c_int32 * len(xs))()
    n = lib.svg_debug_band_shard_map(C.byref(pd), S, C.byref(sh), int(token_major), C.cast(arr, C.c_void_p), len(xs), C.cast(g, C.c_void_p),
                                     C.cast(gi, C.c_void_p))
    assert n == len(xs)
    return list(g), list(gi)


def test_g_and_ginv_against_brute_force():
    P, n_cases = 5, 0
    for vid0 in (0, 3):
        for F in range(1, 8):
            for Fl in range(0, F + 1):
                for f0 in range(0, F - Fl + 1):
                    for n_tail in (0, 4):
                        if Fl == 0 and n_tail == 0:
                            continue
                        tail0 = vid0 + F * P + 2                       # (a tail that starts two rows behind the video)
                        S = tail0 + 4 + 1
                        shard = (f0, Fl, tail0, n_tail)
                        for tm in (False, True):
                            gs = _brute_coords(vid0, F, P, S, shard, tm)
                            assert all(a < b for a, b in zip(gs, gs[1:]))                       # strictly increasing
                            n = len(gs)
                            want_inv = [bisect.bisect_left(gs, x) for x in range(-2, S + 3)]
                            for impl in ("binding", "library"):
                                if impl == "binding":
                                    g = [nat.band_shard_coord((vid0, F, P), shard, tm, l) for l in range(n)]
                                    gi = [nat.band_shard_coord_inv((vid0, F, P), shard, tm, x) for x in range(-2, S + 3)]
                                else:
                                    g = _lib_map(vid0, F, P, S, shard, tm, list(range(n)))[0]
                                    gi = _lib_map(vid0, F, P, S, shard, tm, list(range(-2, S + 3)))[1]
                                assert g == gs, (impl, vid0, F, shard, tm)
                                assert gi == want_inv, (impl, vid0, F, shard, tm)
                            n_cases += 1
    assert n_cases > 500


def test_the_whole_sequence_is_the_identity():
    for name in ("hy", "wan", "p75"):
        S, vid0, F, P = BC.geometry(name)
        for tm in (False, True):
            assert [nat.band_shard_coord((vid0, F, P), BC.whole(name), tm, l) for l in range(S)] == list(range(S))
            assert _lib_map(vid0, F, P, S, BC.whole(name), tm, list(range(S))) == (list(range(S)), list(range(S)))


def test_the_cases_state_the_maps_of_the_binding():
    """tests/band_shard_cases.py states a shard in the model's terms (sequence rows, placement); the binding in the kernel's (g of the
    index in the head's order): the same sets of coordinates"""
    for name in BC.CASES:
        S, vid0, F, P = BC.geometry(name)
        for shard in BC.shards(name):
            n = nat.band_shard_rows(shard, P)
            for tm in (False, True):
                want = sorted(BC.mask_coords(name, BC.shard_rows(name, shard), tm).tolist())
                assert [nat.band_shard_coord((vid0, F, P), shard, tm, l) for l in range(n)] == want


# ---------------------------------------------------------------------------------------------------------
# band_shard_has_keys and the plan against the boolean statement of the mask at the shards' coordinates
# ---------------------------------------------------------------------------------------------------------
def test_has_keys_on_the_cases():
    for name, c in BC.CASES.items():
        S, vid0, F, P = BC.geometry(name)
        bm = nat.BandMask(**c["mask"])
        sh = BC.shards(name)
        for qs in sh:
            for ks in sh:
                for tm in (False, True):
                    want = bool(BC.pair_mask(name, qs, ks, tm).any())
                    assert nat.band_shard_has_keys(bm, S, (vid0, F, P), qs, ks, tm) == want, (name, qs, ks, tm)
    # the pair the GPU tests and the gloo schedule rely on: on the narrow Wan mask the first shard's rows see no key of the last shard in
    # logical order (240 - 1 + 129 <= 400, and the full columns [0, 80) are the first shard's own) — and every key of it token-major
    S, vid0, F, P = BC.geometry("wan")
    bm = nat.BandMask(**BC.CASES["wan"]["mask"])
    first, last = BC.shards("wan")[0], BC.shards("wan")[2]
    assert not nat.band_shard_has_keys(bm, S, (vid0, F, P), first, last, False)
    assert nat.band_shard_has_keys(bm, S, (vid0, F, P), first, last, True)
    assert nat.band_shard_has_keys(bm, S, (vid0, F, P), last, first, False)      # (the full columns)


def _random_mask(rng, S):
    real = rng.choice([S, S, rng.randint(0, S)])
    a, b = sorted(rng.randint(0, S) for _ in range(2))
    c, d = sorted(rng.randint(0, S) for _ in range(2))
    return dict(real_len=real, band=rng.choice([0, 1, 2, 3, rng.randint(0, S + 1), rng.randint(0, 12)]),
                colfull_lo=a, colfull_hi=rng.choice([a, b]), rowfull_lo=c, rowfull_hi=rng.choice([c, d]))


def _random_shard(rng, vid0, F, P, S):
    f0 = rng.randint(0, F)
    n = rng.randint(0, F - f0)
    tail0 = vid0 + F * P
    t0 = rng.randint(tail0, S)
    nt = rng.choice([0, rng.randint(0, S - t0)])
    if n == 0 and nt == 0:
        return (0, F, tail0, 0)
    return (f0, n, t0, nt)


def test_has_keys_on_random_masks_and_shards():
    rng = random.Random(7)
    seen = {True: 0, False: 0}
    for _ in range(400):
        F, P, vid0 = rng.randint(1, 6), rng.randint(1, 9), rng.choice([0, 0, rng.randint(0, 5)])
        S = vid0 + F * P + rng.randint(0, 12)
        prm = _random_mask(rng, S)
        em = O.band_mask(S, **prm)
        bm = nat.BandMask(**prm)
        for _ in range(6):
            qs, ks = _random_shard(rng, vid0, F, P, S), _random_shard(rng, vid0, F, P, S)
            for tm in (False, True):
                cq = [c for c in _brute_coords(vid0, F, P, S, qs, tm)]
                ck = [c for c in _brute_coords(vid0, F, P, S, ks, tm)]
                want = bool(em[cq][:, ck].any())
                got = nat.band_shard_has_keys(bm, S, (vid0, F, P), qs, ks, tm)
                real_in_video = vid0 < prm["real_len"] < vid0 + F * P
                if tm and real_in_video:
                    assert got or not want, (S, prm, qs, ks)          # (documented: True where in doubt, never a dropped pair)
                else:
                    assert got == want, (S, vid0, F, P, prm, qs, ks, tm)
                    seen[want] += 1
    assert seen[True] > 500 and seen[False] > 500


def test_frame_range_and_frame_shard():
    from svg.distributed import frame_range, frame_shard

    assert [frame_range(33, r, 8) for r in range(8)] == [(0, 5), (5, 9), (9, 13), (13, 17), (17, 21), (21, 25), (25, 29), (29, 33)]
    assert [frame_range(7, r, 3) for r in range(3)] == [(0, 3), (3, 5), (5, 7)]
    assert [frame_range(2, r, 3) for r in range(3)] == [(0, 1), (1, 2), (2, 2)]
    sizes = [b - a for a, b in (frame_range(33, r, 8) for r in range(8))]
    assert abs(max(sizes) / (sum(sizes) / 8) - 1.21) < 0.005            # the known cost of whole frames at N = 8
    for name in ("hy", "wan", "p75"):
        world = len(BC.CASES[name]["frames"])
        if name != "p75":                                                # (p75 cuts 2 / 1 / 1 by hand)
            assert [frame_shard(BC.geometry(name), r, world).as_tuple() for r in range(world)] == BC.shards(name)
    with pytest.raises(ValueError, match="in front of the video"):
        frame_shard(BC.geometry("cog"), 0, 2)


def test_exchange_plan_is_the_table_of_has_keys():
    from svg.distributed import band_shard_exchange_plan, frame_shard

    for name in ("hy", "wan"):
        geo = BC.geometry(name)
        bm = nat.BandMask(**BC.CASES[name]["mask"])
        for world in (1, 2, 3, 5, 8):                                    # (8 ranks, 7 frames: the last rank holds the tail alone, or nothing)
            sh = [frame_shard(geo, r, world).as_tuple() for r in range(world)]
            rows = [nat.band_shard_rows(s, geo[3]) for s in sh]

            def table(kinds):
                return [[rows[r] > 0 and rows[s] > 0 and any(bool(BC.pair_mask(name, sh[r], sh[s], tm).any()) for tm in kinds)
                         for s in range(world)] for r in range(world)]

            assert band_shard_exchange_plan(bm, geo, world, "logical") == table([False])
            assert band_shard_exchange_plan(bm, geo, world, "token_major") == table([True])
            assert band_shard_exchange_plan(bm, geo, world) == table([False, True])
    bm = nat.BandMask(**BC.CASES["wan"]["mask"])
    assert band_shard_exchange_plan(bm, BC.geometry("wan"), 3, "logical")[0] == [True, True, False]
    assert band_shard_exchange_plan(bm, BC.geometry("wan"), 3, "both")[0] == [True, True, True]     # a token-major head sees every shard


# ---------------------------------------------------------------------------------------------------------
# argument validation, in the header's order: pointers, geometry, q shard, k shard, mask, (sizes,) layout; then what has no shard form
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


# a sequence of 1024 rows: 9 frames of 100 rows from row 0, 124 rows behind them; q shard: frames [2, 5) (300 rows), k shard: frames [7, 9)
# and the whole tail (324 rows)
def shard_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=2, S=1024, D=128, dtype=0, m="ok", null_mask=False, perm=(PH, 0, 9, 100), null_perm=False,
               qs=(2, 3, 0, 0), ks=(7, 2, 900, 124), null_qs=False, null_ks=False, lay=None):
    m = _mask(S) if m == "ok" else m
    pd, a, b = nat.PermDesc(*perm), nat.BandShard(*qs), nat.BandShard(*ks)
    return [q, k, v, o, lse, BH, S, D, dtype, 1.0, None if null_mask else C.byref(m), None if null_perm else C.byref(pd),
            None if null_qs else C.byref(a), None if null_ks else C.byref(b), C.byref(lay) if lay is not None else None, None]


BAD_ROW = nat.TensorStrides(2 * 300 * 128, 300 * 128, 64)          # a row stride below D
UNALIGNED_ROW = nat.TensorStrides(2 * 300 * 132, 300 * 132, 132)   # rows that are no multiple of 16 bytes
CASES = [
    ("null_q", dict(q=None), BAD_ARG),
    ("null_k", dict(k=None), BAD_ARG),
    ("null_v", dict(v=None), BAD_ARG),
    ("null_o", dict(o=None), BAD_ARG),                              # (o32 of the _f32 form)
    ("null_lse", dict(lse=None), BAD_ARG),
    ("null_mask", dict(null_mask=True), BAD_ARG),
    ("null_perm", dict(null_perm=True), BAD_ARG),
    ("null_q_shard", dict(null_qs=True), BAD_ARG),
    ("null_k_shard", dict(null_ks=True), BAD_ARG),
    ("null_lse_before_unsupported_D", dict(lse=None, D=64), BAD_ARG),
    ("null_flags_are_heads_in_logical_order", dict(perm=(None, 0, 9, 100), D=64), UNSUPPORTED),   # (accepted: only D stops it)
    ("BH0", dict(BH=0), BAD_ARG),
    ("S0", dict(S=0), BAD_ARG),
    ("num_frame0", dict(perm=(PH, 0, 0, 100)), BAD_ARG),
    ("frame_size0", dict(perm=(PH, 0, 9, 0)), BAD_ARG),
    ("vid0_negative", dict(perm=(PH, -1, 9, 100)), BAD_ARG),
    ("video_ends_behind_S", dict(perm=(PH, 125, 9, 100)), BAD_ARG),
    ("video_ends_behind_S_int32", dict(perm=(PH, 0, 1 << 16, 1 << 16)), BAD_ARG),
    ("q_shard_f0_negative", dict(qs=(-1, 3, 0, 0)), BAD_ARG),
    ("q_shard_frames_behind_F", dict(qs=(7, 3, 0, 0)), BAD_ARG),
    ("q_shard_n_frames_negative", dict(qs=(2, -1, 900, 10)), BAD_ARG),
    ("k_shard_frames_behind_F", dict(ks=(8, 2, 900, 124)), BAD_ARG),
    ("k_shard_frames_behind_F_int32", dict(ks=(2 ** 31 - 1, 2 ** 31 - 1, 900, 124)), BAD_ARG),
    ("q_shard_tail_inside_the_video", dict(qs=(2, 3, 899, 10)), BAD_ARG),
    ("k_shard_tail_ends_behind_S", dict(ks=(7, 2, 900, 125)), BAD_ARG),
    ("k_shard_tail_ends_behind_S_int32", dict(ks=(7, 2, 2 ** 31 - 1, 2 ** 31 - 1)), BAD_ARG),
    ("k_shard_n_tail_negative", dict(ks=(7, 2, 900, -1)), BAD_ARG),
    ("q_shard_empty", dict(qs=(2, 0, 0, 0)), BAD_ARG),
    ("k_shard_empty", dict(ks=(9, 0, 900, 0)), BAD_ARG),
    ("shard_before_unsupported_D", dict(qs=(7, 3, 0, 0), D=64), BAD_ARG),
    ("geometry_before_unsupported_D", dict(perm=(PH, 0, 0, 100), D=64), BAD_ARG),
    ("tail_alone_is_a_shard", dict(qs=(9, 0, 900, 124), D=64), UNSUPPORTED),                        # (accepted: only D stops it)
    ("a_tail_that_is_not_read", dict(qs=(2, 3, -5, 0), D=64), UNSUPPORTED),                         # (n_tail = 0: tail_begin is not read)
    ("bad_mask_band", dict(m=_mask(1024, band=-1)), BAD_ARG),
    ("bad_mask_real_len_behind_S", dict(m=_mask(1024, real_len=1025)), BAD_ARG),
    ("bad_mask_before_unsupported_D", dict(m=_mask(1024, band=-1), D=64), BAD_ARG),
    ("bad_layout_heads0", dict(lay=_layout(300, 324, heads_per_batch=0)), BAD_ARG),
    ("bad_layout_row_below_D", dict(lay=_layout(300, 324, q=BAD_ROW)), BAD_ARG),
    ("layout_row_unaligned", dict(lay=_layout(300, 324, q=UNALIGNED_ROW)), UNSUPPORTED),
    ("D64", dict(D=64), UNSUPPORTED),
    ("D96", dict(D=96), UNSUPPORTED),
    ("dtype_f32", dict(dtype=2), UNSUPPORTED),
    ("S_2pow24", dict(S=1 << 24), UNSUPPORTED),                     # check_rows of the plain entry, on S
    ("BH_S_D_2pow40", dict(BH=1 << 10, S=1 << 23), UNSUPPORTED),
]


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("kw,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_validation_order(kw, expected, name):
    _host_only()
    assert getattr(nat.load(), name)(*shard_args(**kw)) == expected


def test_the_table_holds_the_rows_the_header_promises():
    ids = {c[0] for c in CASES}
    for want in ("null_perm", "null_q_shard", "null_k_shard", "q_shard_frames_behind_F", "q_shard_tail_inside_the_video",
                 "k_shard_tail_ends_behind_S", "q_shard_empty", "k_shard_empty", "bad_mask_before_unsupported_D", "shard_before_unsupported_D"):
        assert want in ids


def test_misaligned_o32_is_unsupported_and_argument_faults_come_first():
    _host_only()
    lib = nat.load()
    assert lib.svg_band_shard_attention_lse_f32(*shard_args(o=PH + 8)) == UNSUPPORTED
    assert lib.svg_band_shard_attention_lse_f32(*shard_args(o=PH + 8, m=_mask(1024, real_len=1025))) == BAD_ARG
    assert lib.svg_band_shard_attention_lse_f32(*shard_args(o=PH + 8, qs=(7, 3, 0, 0))) == BAD_ARG
    assert lib.svg_band_shard_attention_lse(*shard_args(o=PH + 8, D=64)) == UNSUPPORTED   # (a 16-bit o has no such rule; D has)


def test_the_debug_map_refuses_what_the_entries_refuse():
    lib = nat.load()
    x = (C.c_int32 * 1)(0)
    out = (C.c_int32 * 1)()
    pd, ok, bad = nat.PermDesc(None, 0, 9, 100), nat.BandShard(2, 3, 0, 0), nat.BandShard(7, 3, 0, 0)
    args = lambda p, s: (p, 1024, s, 0, C.cast(x, C.c_void_p), 1, C.cast(out, C.c_void_p), None)   # noqa: E731
    assert lib.svg_debug_band_shard_map(*args(C.byref(pd), C.byref(ok))) == 1 and out[0] == 200
    assert lib.svg_debug_band_shard_map(*args(C.byref(pd), C.byref(bad))) == -1
    assert lib.svg_debug_band_shard_map(*args(None, C.byref(ok))) == -1
    assert lib.svg_debug_band_shard_map(*args(C.byref(nat.PermDesc(None, 200, 9, 100)), C.byref(ok))) == -1


# ---------------------------------------------------------------------------------------------------------
# the wrapper: what has no shard form raises before anything runs (CPU tensors get this far)
# ---------------------------------------------------------------------------------------------------------
def test_wrapper_refuses_what_has_no_shard_form(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda *a, **k: pytest.fail("nothing may be loaded or launched"))
    m = _mask(1024)
    geo = (0, 9, 100)
    qs, ks = (2, 3, 0, 0), (7, 2, 900, 124)
    q, k = torch.zeros(1, 2, 300, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 324, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.band_shard_attention(q, k, k, m, 1024, geo, qs, ks)
    with pytest.raises(ValueError, match="out_dtype"):
        nat.band_shard_attention(q, k, k, m, 1024, geo, qs, ks, out_dtype=torch.float16)
    with pytest.raises(ValueError, match="without out"):
        nat.band_shard_attention(q, k, k, m, 1024, geo, qs, ks, out_dtype=torch.float32, out=torch.zeros_like(q))
    monkeypatch.setattr(nat, "_gpu", lambda *ts: None)   # (as if the tensors were on a GPU: the checks behind the device check)
    with pytest.raises(ValueError, match="head_dim 128"):
        nat.band_shard_attention(q[..., :64], k[..., :64], k[..., :64], m, 1024, geo, qs, ks)
    with pytest.raises(ValueError, match="head_dim 128"):
        nat.band_shard_attention(q.float(), k.float(), k.float(), m, 1024, geo, qs, ks)
    with pytest.raises(ValueError, match="does not fit"):
        nat.band_shard_attention(q, k, k, m, 1024, (200, 9, 100), qs, ks)
    with pytest.raises(ValueError, match="outside a video"):
        nat.band_shard_attention(q, k, k, m, 1024, geo, (7, 3, 0, 0), ks)
    with pytest.raises(ValueError, match="behind the video"):
        nat.band_shard_attention(q, k, k, m, 1024, geo, qs, (7, 2, 899, 124))
    with pytest.raises(ValueError, match="empty shard"):
        nat.band_shard_attention(q, k, k, m, 1024, geo, (2, 0, 0, 0), ks)
    with pytest.raises(ValueError, match="the shards say"):
        nat.band_shard_attention(q, k[:, :, :300], k[:, :, :300], m, 1024, geo, qs, ks)
    with pytest.raises(ValueError, match="flags for"):
        nat.band_shard_attention(q, k, k, m, 1024, geo, qs, ks, flags=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="one dtype"):
        nat.band_shard_attention(q, k, k.half(), m, 1024, geo, qs, ks)


# ---------------------------------------------------------------------------------------------------------
# the float64 identity the GPU protocol rests on: the parts of a q shard over the k shards merge to the shard's rows of the whole
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hy", "wan", "p75"])
def test_shard_parts_merge_to_the_whole_float64(name):
    dtype = torch.bfloat16
    S, vid0, F, P = BC.geometry(name)
    q, k, v = BC.inputs(name, dtype)
    flags = torch.tensor(BC.FLAGS).view(1, BC.H)
    # the whole, as the model computes it: placement, the mask in logical order, inverse placement
    ctx = S - F * P
    ql, kl, vl = (O.head_placement(x.double(), flags, ctx, F, P) for x in (q, k, v))
    o_l, lse_l = SC.masked_attention_lse(ql, kl, vl, BC.element_mask(name))
    o_whole = O.head_placement(o_l, flags, ctx, F, P, inverse=True)
    lse_whole = O.head_placement(lse_l[..., None], flags, ctx, F, P, inverse=True)[..., 0]
    empty_rows = 0
    for qs in BC.shards(name):
        rows = BC.shard_rows(name, qs)
        o_ref, lse_ref = BC.rows_reference(name, dtype, qs)
        assert (o_ref - o_whole[:, :, rows]).abs().max() <= 1e-12 and torch.equal(torch.isfinite(lse_ref), torch.isfinite(lse_whole[:, :, rows]))
        parts = [BC.pair_reference(name, dtype, qs, ks) for ks in BC.shards(name)]
        empty_rows += sum(int((~torch.isfinite(l)).sum()) for _, l in parts)
        o, lse = merge_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True)
        assert (o - o_ref).abs().max() <= 1e-12
        fin = torch.isfinite(lse_ref)
        assert torch.equal(torch.isfinite(lse), fin) and (lse[fin] - lse_ref[fin]).abs().max() <= 1e-12
    if name == "wan":
        assert empty_rows >= 2 * 240      # the first shard's rows of the two heads in logical order against the last shard


# ---------------------------------------------------------------------------------------------------------
# token_sharded_svg1_attention on gloo CPU ranks
# ---------------------------------------------------------------------------------------------------------
def _worker(rank, world):
    from svg import distributed as sd

    a2a = CountingAllToAll()
    H, D = 4, 16
    out = {}
    for name, flags, kinds in (("hy", (0, 1, 0, 1), "both"), ("wan", (0, 1, 0, 1), "both"), ("wan", (0, 0, 0, 0), "logical")):
        geo = BC.geometry(name)
        S, vid0, F, P = geo
        em = BC.element_mask(name)
        mask = nat.BandMask(**BC.CASES[name]["mask"])
        g = torch.Generator().manual_seed(5)
        q, k, v = (torch.randn(1, H, S, D, generator=g, dtype=torch.float64) for _ in range(3))
        fl = torch.tensor(flags).view(1, H)
        ctx = S - F * P
        ql, kl, vl = (O.head_placement(x, fl, ctx, F, P) for x in (q, k, v))          # placement -> mask -> inverse placement
        ref = O.head_placement(SC.masked_attention_lse(ql, kl, vl, em)[0], fl, ctx, F, P, inverse=True)
        sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
        rows = BC.shard_rows(name, sh[rank])
        calls = []

        def attn_fn(q_, k_, v_, q_shard, k_shard):
            qs, ks = q_shard.as_tuple(), k_shard.as_tuple()
            calls.append((qs, ks))
            assert q_.shape[-2] == nat.band_shard_rows(qs, P) and k_.shape[-2] == nat.band_shard_rows(ks, P)
            parts = [SC.masked_attention_lse(q_[:, h:h + 1], k_[:, h:h + 1], v_[:, h:h + 1], BC.pair_mask(name, qs, ks, bool(flags[h])))
                     for h in range(H)]                                                   # both kinds of head in one call
            return torch.cat([o for o, _ in parts], dim=1), torch.cat([l for _, l in parts], dim=1)

        a2a.reset()
        o = sd.token_sharded_svg1_attention(q[:, :, rows].contiguous(), k[:, :, rows].contiguous(), v[:, :, rows].contiguous(), mask, fl, geo,
                                            kinds=kinds, attn_fn=attn_fn, merge_fn=merge_states)
        plan = sd.band_shard_exchange_plan(mask, geo, world, kinds)
        per_tok = 2 * H * D * 8
        n_rows = [nat.band_shard_rows(s, P) for s in sh]
        want_bytes = sum(n_rows[s] * per_tok for s in range(world) if s != rank and plan[rank][s])
        all_bytes = sum(n_rows[s] * per_tok for s in range(world) if s != rank)
        want_calls = sorted((sh[rank], sh[s]) for s in range(world) if plan[rank][s])
        out[name, kinds] = dict(err=(o - ref[:, :, rows]).abs().max().item(), shape_ok=o.shape == (1, H, len(rows), D), received=a2a.received,
                                want_bytes=want_bytes, all_bytes=all_bytes, calls_ok=sorted(calls) == want_calls,
                                own_first=(not calls) or calls[0] == (sh[rank], sh[rank]), skipped=sum(not x for row in plan for x in row))
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_svg1_attention_gloo(world):
    """frame shards of 7 frames (4 / 3 and 3 / 2 / 2, the text and padding on the last rank), float64 statements as attn_fn / merge_fn, heads
    0 and 2 in logical order and 1 and 3 token-major: every rank's rows equal the single-process placement -> mask -> inverse placement to
    1e-5, the bytes a rank received are those of the shards the plan keeps for it, attn_fn ran for exactly those pairs, and with heads in
    logical order alone the narrow Wan mask skips a pair on three ranks"""
    # (the geometry really skips one: shown on the CPU before any rank starts)
    from svg.distributed import band_shard_exchange_plan
    wan = nat.BandMask(**BC.CASES["wan"]["mask"])
    assert band_shard_exchange_plan(wan, BC.geometry("wan"), 3, "logical")[0][2] is False
    got = run_ranks(_worker, world, 46500)
    for rank, res in got.items():
        for key, r in res.items():
            assert r["shape_ok"] and r["calls_ok"] and r["own_first"], (rank, key, r)
            assert r["err"] <= 1e-5, (rank, key, r["err"])
            assert r["received"] == r["want_bytes"], (rank, key, r)
    if world == 3:
        narrow = got[0]["wan", "logical"]
        assert narrow["skipped"] >= 1 and narrow["received"] < narrow["all_bytes"]          # rank 0 did not receive the last shard
        assert got[1]["wan", "logical"]["received"] == got[1]["wan", "logical"]["all_bytes"]
        assert got[0]["wan", "both"]["received"] == got[0]["wan", "both"]["all_bytes"]      # a token-major head needs every shard


def test_token_sharded_svg1_attention_refuses_too_many_parts(monkeypatch):
    from svg import distributed as sd

    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 9)
    geo = (9 * 20, 0, 9, 20)
    x = torch.zeros(1, 2, 20, 16, dtype=torch.float64)
    with pytest.raises(ValueError, match="at most 8 parts"):
        sd.token_sharded_svg1_attention(x, x, x, nat.BandMask(**O.dense_band_params(180)), None, geo)
    plan = sd.band_shard_exchange_plan(_mask(180, band=10), geo, 9, "logical")
    assert max(sum(row) for row in plan) == 3
