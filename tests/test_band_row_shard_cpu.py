"""Band attention on row shards without a GPU (include/svg_attn_band_row_shard.h; svg/_band_row_shard.py; svg.distributed.row_shard and
balance="rows"): the coordinate maps of the library and of the binding against a brute-force sort of the shard's (position, frame) pairs,
the exchange plan's pair test against the element mask, the return codes in the header's order, the planner, what is refused under
balance="rows" and that the default stays the frame-shard path."""
import bisect
import ctypes as C

import pytest
import torch

import band_row_shard_cases as RC
from svg import _band_row_shard as rs
from svg import _native as nat
from test_band_shard_cpu import BAD_ARG, PH, UNSUPPORTED, _layout, _lib_map, _mask

ENTRIES = ("svg_band_row_shard_attention_lse", "svg_band_row_shard_attention_lse_f32")


def _brute(vid0, F, P, shard, token_major):
    """(mask coordinate, shard row it is stored at) of the shard's rows in the head's order: by (p, f) for a token-major head"""
    row0, n, tail0, n_tail = shard
    vid = [((i % P) * F + i // P if token_major else i, i - row0) for i in range(row0, row0 + n)]
    return sorted((vid0 + c, r) for c, r in vid) + [(tail0 + j, n + j) for j in range(n_tail)]


def _lib_row_map(vid0, F, P, S, shard, token_major, xs):
    pd, sh, arr = nat.PermDesc(None, vid0, F, P), rs.BandRowShard(*shard), (C.c_int32 * len(xs))(*xs)
    outs = [(C.c_int32 * len(xs))() for _ in range(3)]
    assert rs.load().svg_debug_band_row_shard_map(C.byref(pd), S, C.byref(sh), int(token_major), C.cast(arr, C.c_void_p), len(xs),
                                                  *[C.cast(o, C.c_void_p) for o in outs]) == len(xs)
    return [list(o) for o in outs]


def _check_maps(vid0, F, P, S, shard):
    assert sum((hi - lo) * c for lo, hi, c, _, _ in rs.band_row_shard_pieces(shard, P)) == shard[1]      # the piecewise counts
    for tm in (False, True):
        want = _brute(vid0, F, P, shard, tm)
        gs, xs = [c for c, _ in want], list(range(-2, S + 3))
        want_inv = [bisect.bisect_left(gs, x) for x in xs]                # the smallest index with g >= x
        g, _, phys = _lib_row_map(vid0, F, P, S, shard, tm, list(range(len(gs))))
        assert g == gs and phys == [r for _, r in want], (shard, tm)
        assert _lib_row_map(vid0, F, P, S, shard, tm, xs)[1] == want_inv, (shard, tm)
        assert [rs.band_row_shard_coord((vid0, F, P), shard, tm, l) for l in range(len(gs))] == gs
        assert [rs.band_row_shard_coord_inv((vid0, F, P), shard, tm, x) for x in xs] == want_inv, (shard, tm)


def test_maps_against_brute_force_every_shard_of_a_small_video():
    P, n = 5, 0
    for vid0, F in ((0, 1), (0, 4), (3, 3)):
        tail0 = vid0 + F * P + 2
        for row0 in range(F * P + 1):
            for rows in range(F * P - row0 + 1):
                for n_tail in (0, 3) if rows else (3,):
                    _check_maps(vid0, F, P, tail0 + 4, (row0, rows, tail0, n_tail))
                    n += 1
    assert n > 500


@pytest.mark.parametrize("shard", RC.shards(RC.CUTS["704"]) + RC.shards(RC.CUTS["640"])
                         + [(200, 100, RC.V, 0), (0, 0, RC.V, 40), (RC.P, 2 * RC.P, RC.V, 40)], ids=str)
def test_maps_of_the_cases(shard):
    """the GPU tests' shards, one inside a frame, a tail alone, whole frames — whose maps are those of svg_debug_band_shard_map"""
    _check_maps(0, RC.F, RC.P, RC.S, shard)
    if shard[1] and shard[0] % RC.P == 0 and shard[1] % RC.P == 0:
        frames = (shard[0] // RC.P, shard[1] // RC.P) + shard[2:]
        for tm in (False, True):
            ls, xs = list(range(shard[1] + shard[3])), list(range(-2, RC.S + 3))
            assert _lib_row_map(0, RC.F, RC.P, RC.S, shard, tm, ls)[0] == _lib_map(0, RC.F, RC.P, RC.S, frames, tm, ls)[0]
            assert _lib_row_map(0, RC.F, RC.P, RC.S, shard, tm, xs)[1] == _lib_map(0, RC.F, RC.P, RC.S, frames, tm, xs)[1]


@pytest.mark.parametrize("cuts", list(RC.CUTS))
@pytest.mark.parametrize("mask", list(RC.MASKS))
def test_has_keys_and_the_plan_against_the_element_mask(mask, cuts):
    bm, sh = nat.BandMask(**RC.MASKS[mask]), RC.shards(RC.CUTS[cuts])
    table = {tm: [[bool(RC.pair_mask(mask, q, k, tm).any()) for k in sh] for q in sh] for tm in (False, True)}
    for tm in (False, True):
        assert [[rs.band_row_shard_has_keys(bm, RC.S, (0, RC.F, RC.P), q, k, tm) for k in sh] for q in sh] == table[tm]
    assert table[False][0][2] == (mask == "hy")      # Wan-like: the first shard's rows in logical order see no key of the last


@pytest.mark.parametrize("world", [2, 3, 8])
def test_row_shard_covers_the_sequence_once(world):
    from svg.distributed import row_shard

    geo = (119056, 0, 33, 3600)                       # HunyuanVideo 720p
    sh = [row_shard(geo, r, world).as_tuple() for r in range(world)]
    assert [s[0] for s in sh] + [33 * 3600] == [0] + [s[0] + s[1] for s in sh]
    assert all(s[1] % 128 == 0 for s in sh[:-1]) and [s[3] for s in sh] == [0] * (world - 1) + [256]
    rows = [s[1] + s[3] for s in sh]
    assert sum(rows) == geo[0] and max(rows) / (sum(rows) / world) < 1.02


def row_args(q=PH, k=PH, v=PH, o=PH, lse=PH, BH=2, S=1024, D=128, dtype=0, m="ok", perm=(PH, 0, 9, 100), qs=(250, 300, 0, 0),
             ks=(650, 250, 900, 124), null=(), lay=None):
    m = _mask(S) if m == "ok" else m
    ptr = dict(mask=C.byref(m), perm=C.byref(nat.PermDesc(*perm)), qs=C.byref(rs.BandRowShard(*qs)), ks=C.byref(rs.BandRowShard(*ks)))
    ptr.update({name: None for name in null})
    return [q, k, v, o, lse, BH, S, D, dtype, 1.0, ptr["mask"], ptr["perm"], ptr["qs"], ptr["ks"], C.byref(lay) if lay is not None else None,
            None]


CASES = [
    ("null_q", dict(q=None), BAD_ARG), ("null_o", dict(o=None), BAD_ARG), ("null_lse_before_D", dict(lse=None, D=64), BAD_ARG),
    ("null_mask", dict(null=("mask",)), BAD_ARG), ("null_perm", dict(null=("perm",)), BAD_ARG),
    ("null_q_shard", dict(null=("qs",)), BAD_ARG), ("null_k_shard", dict(null=("ks",)), BAD_ARG),
    ("BH0", dict(BH=0), BAD_ARG), ("frame_size0", dict(perm=(PH, 0, 9, 0)), BAD_ARG), ("video_ends_behind_S", dict(perm=(PH, 125, 9, 100)), BAD_ARG),
    ("q_row0_negative", dict(qs=(-1, 300, 0, 0)), BAD_ARG), ("q_n_rows_negative", dict(qs=(250, -1, 900, 10)), BAD_ARG),
    ("q_rows_behind_the_video", dict(qs=(650, 251, 0, 0)), BAD_ARG), ("k_rows_behind_the_video_int32", dict(ks=(2 ** 31 - 1, 2 ** 31 - 1, 900, 124)), BAD_ARG),
    ("k_tail_inside_the_video", dict(ks=(650, 250, 899, 10)), BAD_ARG), ("k_tail_ends_behind_S", dict(ks=(650, 250, 900, 125)), BAD_ARG),
    ("k_n_tail_negative", dict(ks=(650, 250, 900, -1)), BAD_ARG), ("q_shard_empty", dict(qs=(250, 0, 0, 0)), BAD_ARG),
    ("k_shard_empty", dict(ks=(900, 0, 900, 0)), BAD_ARG), ("shard_before_unsupported_D", dict(qs=(650, 251, 0, 0), D=64), BAD_ARG),
    ("tail_alone_is_a_shard", dict(qs=(900, 0, 900, 124), D=64), UNSUPPORTED), ("a_tail_that_is_not_read", dict(qs=(250, 300, -5, 0), D=64), UNSUPPORTED),
    ("bad_mask_before_unsupported_D", dict(m=_mask(1024, band=-1), D=64), BAD_ARG),
    ("bad_layout_heads0", dict(lay=_layout(300, 374, heads_per_batch=0)), BAD_ARG), ("D64", dict(D=64), UNSUPPORTED),
    ("dtype_f32", dict(dtype=2), UNSUPPORTED), ("S_2pow24", dict(S=1 << 24), UNSUPPORTED),
]


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("kw,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_validation_order(kw, expected, name):
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    assert getattr(rs.load(), name)(*row_args(**kw)) == expected


def test_what_has_no_row_shard_form_says_so(monkeypatch):
    from svg import distributed as sd

    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 1)
    x, bm = torch.zeros(1, 2, RC.S, 128, dtype=torch.bfloat16), nat.BandMask(**RC.MASKS["hy"])
    with pytest.raises(NotImplementedError, match="device switch"):
        sd.token_sharded_svg1_attention(x, x, x, bm, None, RC.GEO, dense_mask=bm, dense_flag=torch.zeros(1, dtype=torch.int32), balance="rows")
    with pytest.raises(NotImplementedError, match="shard profiler"):
        sd.token_sharded_svg1_layer_call(x, x, x, bm, None, RC.GEO, torch.zeros(4, dtype=torch.int64), balance="rows")
    with pytest.raises(ValueError, match="balance"):
        sd.enable_frame_shards(balance="tokens")
    for kw, kind in (({}, "BandShard"), (dict(balance="frames"), "BandShard"), (dict(balance="rows"), "BandRowShard")):   # the default: frame shards
        calls = []
        sd.token_sharded_svg1_attention(x, x, x, bm, None, RC.GEO, merge_fn=lambda o, l: o[0], **kw,
                                        attn_fn=lambda q, k, v, qs, ks: calls.append((type(qs).__name__, type(ks).__name__)) or (q, None))
        assert calls == [(kind, kind)]
