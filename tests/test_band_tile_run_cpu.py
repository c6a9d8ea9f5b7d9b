"""The tile run of the 16x16x32 band kernels (csrc/band_policy.h BandPolicy::tile_run) through svg_debug_band_tile_run: for one wave of
one q-tile, the key tiles [run_lo, run_lo + run_n) whose vector phase skips the per-tile scalar decisions.  A row cursor that is stepped
where it must divide reads rows outside the tensor, so this runs on the host before anything runs on a GPU.  For every tile of every
(q-tile, wave, request distance, head kind):
  * inside the run (a) the tile is unmasked by the wave's fast-path interval, (b) it follows its predecessor by 64 keys, (c) the tile the
    phase resolves, dist + 1 further, exists, lies in the same segment and takes the stepped form — each evaluated by the entry with the
    per-tile functions the kernel uses outside a run;
  * the run is maximal, and more: NO tile outside it has (a) - (c) (the run is the one interval of such tiles);
  * the physical row of every lane after every tile, walked as the kernel walks it (run form inside the run), is the row the placement
    formula gives (the formula of tests/test_band_row_cursor_cpu.py).
"""
import ctypes as C
import random

import numpy as np
import pytest

import band_tile_run_cases as G
from oracle import svg_oracle as O
from svg import _native as nat

BN, BM, NW = 64, 256, 8


def tile_run(S, prm, vid0, F, P, token_major, qt, wave, dist, detail=True):
    lib = nat.load()
    mask = nat.BandMask(**prm)
    out4 = np.full(4, -7, dtype=np.int32)
    cap = (S + BN - 1) // BN + 3 if detail else 0
    tiles = np.full(4 * cap, -7, dtype=np.int32)
    rows = np.full(BN * cap, -7, dtype=np.int32)
    n = lib.svg_debug_band_tile_run(S, C.byref(mask), vid0, F, P, int(token_major), qt, wave, dist, out4.ctypes.data,
                                    tiles.ctypes.data if detail else None, tiles.size, rows.ctypes.data if detail else None, rows.size)
    assert n >= 0 and n == out4[2], (n, out4)
    m = n if detail else 0
    return int(out4[0]), int(out4[1]), n, int(out4[3]), tiles[:4 * m].reshape(m, 4), rows[:BN * m].reshape(m, BN)


def expected_rows(S, vid0, F, P, token_major, k0s):
    l = np.asarray(k0s, dtype=np.int64)[:, None] + np.arange(BN)[None, :]
    i = l - vid0
    inside = (i >= 0) & (i < F * P)
    phys = np.where(inside & bool(token_major), vid0 + (i % max(F, 1)) * P + i // max(F, 1), l)
    return np.where(l < S, phys, 0)


def check(S, prm, vid0, F, P, token_major, qt, wave, dist):
    """-> (run_n, nT, nqt) after asserting the three properties"""
    run_lo, run_n, nT, nqt, tiles, rows = tile_run(S, prm, vid0, F, P, token_major, qt, wave, dist)
    what = (S, prm, vid0, F, P, token_major, qt, wave, dist, run_lo, run_n, nT)
    assert 0 <= run_n and (run_n == 0 or (1 <= run_lo and run_lo + run_n + dist + 1 <= nT)), what
    if nT == 0:
        return 0, 0, nqt
    key0, full, follows, ahead = (tiles[:, j] for j in range(4))
    assert (np.diff(key0) >= BN).all(), what                       # tiles in increasing key order, never overlapping
    t = np.arange(nT)
    far = np.minimum(t + dist + 1, nT - 1)
    same_seg = (t + dist + 1 < nT) & (key0[far] == key0 + BN * (dist + 1))   # (keys increase: equal only if all tiles between follow on)
    ok = (full == 1) & (follows == 1) & (ahead == 1) & same_seg
    inside = (t >= run_lo) & (t < run_lo + run_n)
    assert ok[inside].all(), (what, "a tile of the run fails (a) - (c)", t[inside & ~ok][:4])
    assert not ok[~inside].any(), (what, "a tile outside the run has (a) - (c)", t[~inside & ok][:4])
    want = expected_rows(S, vid0, F, P, token_major, key0)
    bad = np.argwhere(rows != want)
    assert bad.size == 0, (what, bad[:4], rows[tuple(bad[0])], want[tuple(bad[0])])
    return run_n, nT, nqt


def check_mask(S, prm, vid0, F, P, qts=None, waves=range(NW)):
    """every (q-tile, wave, dist, head kind); -> tiles inside runs, tiles"""
    nqt = tile_run(S, prm, vid0, F, P, 0, 0, 0, 2, detail=False)[3]
    in_run = total = 0
    for qt in (range(nqt) if qts is None else [q for q in qts if q < nqt]):
        for wave in waves:
            for dist in (2, 3):
                for tm in (0, 1):
                    r, n, _ = check(S, prm, vid0, F, P, tm, qt, wave, dist)
                    in_run, total = in_run + r, total + n
    return in_run, total, nqt


F5, P600, CTX, L = 5, 600, 256, 64


def model_case(model, band):
    V = F5 * P600
    if model == "hy":
        S, vid0 = V + CTX, 0
        prm = O.hy_band_params(S, CTX, L, F5, P600, 1.0)
    elif model == "wan":
        S, vid0 = V, 0
        prm = O.wan_band_params(S, F5, P600, 1.0)
    elif model == "cog":
        S, vid0 = V + CTX, CTX
        prm = O.cog_band_params(S, CTX, F5, P600, 1.0)
    else:
        S, vid0 = V + CTX, CTX
        prm = O.cog_band_params(S, CTX, F5, P600, 1.0, attn_sink=True)
    prm["band"] = band
    return S, prm, vid0


@pytest.mark.parametrize("band", [128, 640, 1536])
@pytest.mark.parametrize("model", ["hy", "wan", "cog", "cog_sink"])
def test_model_masks_reduced(model, band):
    S, prm, vid0 = model_case(model, band)
    in_run, total, _ = check_mask(S, prm, vid0, F5, P600)
    assert total > 0 and (band == 128 or in_run > 0)   # (a band of 128 keys holds no 64-key tile that is FULL for 32 rows plus its look-ahead)


@pytest.mark.parametrize("name", G.ALL_CASES)
def test_the_geometries_the_gpu_test_runs(name):
    """tests/band_tile_run_cases.py, every (q-tile, wave, dist, head kind): walked here before a kernel reads a row of them"""
    S, prm, vid0, F_, P_, _, _ = G.geometry(name)
    check_mask(S, prm, vid0, F_, P_)


def test_the_softmax_path_geometries_of_the_gpu_test():
    for S, F_, P_, prms in ((1500, 5, 300, [O.dense_band_params(1500)]),
                            (1200, 4, 300, [O.dense_band_params(1200), dict(real_len=1200, band=200, colfull_lo=0, colfull_hi=0,
                                                                            rowfull_lo=0, rowfull_hi=0)])):
        for prm in prms:
            check_mask(S, prm, 0, F_, P_)


def test_cog_like_text_first():
    F_, P_, vid0 = 3, 272, 226
    S = vid0 + F_ * P_   # 1042: no multiple of 64, and the last q-tile is 18 rows
    for band in (128, 384, S + 1):
        prm = O.cog_band_params(S, vid0, F_, P_, 1.0)
        prm["band"] = band
        check_mask(S, prm, vid0, F_, P_)


@pytest.mark.parametrize("S", [1000, 1040, 1041, 3000 + 16])
def test_ragged_lengths(S):
    """S no multiple of 64; a last q-tile of 16 rows (1040, 3016): waves 1 .. 7 of it are idle and have no run"""
    F_, P_ = 4, 200
    for band in (200, 520):
        prm = dict(real_len=S, band=band, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
        _, _, nqt = check_mask(S, prm, 100, F_, P_)
        if S % BM == 16:
            for wave in range(1, NW):
                for dist in (2, 3):
                    assert tile_run(S, prm, 100, F_, P_, 0, nqt - 1, wave, dist, detail=False)[1] == 0


@pytest.mark.parametrize("valid", [None, 2900])
def test_dense_run_covers_the_segment(valid):
    """band = S + 1: one segment, every tile FULL for rows below real_len — the run of a contiguous head is the whole segment but its first
    tile and the dist + 1 tiles whose look-ahead leaves it (and the tile over S, where S is no multiple of 64)"""
    F_, P_, ctx = 5, 600, 256
    S = F_ * P_ + ctx
    prm = O.dense_band_params(S, valid)
    check_mask(S, prm, 0, F_, P_)
    real = S if valid is None else valid
    for dist in (2, 3):
        run_lo, run_n, nT, _, tiles, _ = tile_run(S, prm, 0, F_, P_, 0, 0, 0, dist)
        n_real = (real + BN - 1) // BN            # the segment of the rows below real_len
        assert nT == n_real and run_lo == 1
        last_full = real // BN - 1                 # last tile wholly below real_len
        last_cheap = (S - BN) // BN                # last tile the cursor steps onto
        assert run_lo + run_n - 1 == min(last_full, nT - dist - 2, last_cheap - dist - 1)


def test_short_bands_and_short_tile_loops():
    """bands so short that the run is empty or one tile, and q-tiles of fewer than dist + 2 key tiles"""
    S, F_, P_ = 2048, 4, 400
    seen = set()
    for band in (0, 1, 33, 64, 96, 97, 128, 160, 161, 192, 224, 225, 256, 289, 320, 352, 353, 384):
        prm = dict(real_len=S, band=band, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
        check_mask(S, prm, 0, F_, P_)
        for wave in range(NW):
            for dist in (2, 3):
                seen.add(tile_run(S, prm, 0, F_, P_, 0, 3, wave, dist, detail=False)[1])
    assert {0, 1} <= seen, seen
    for S in (64, 100, 192, 256, 300):   # nT = 1 .. 5
        prm = O.dense_band_params(S)
        check_mask(S, prm, 0, 1, S)
        for dist in (2, 3):
            _, run_n, nT, _, _, _ = tile_run(S, prm, 0, 1, S, 0, 0, 0, dist)
            assert nT == (S + BN - 1) // BN
            if nT < dist + 2:
                assert run_n == 0


def test_random_mask_family():
    rng = random.Random(4242)
    n_runs = 0
    for _ in range(300):
        S = rng.choice([300, 513, 777, 1024, 1301, 2049, 3333])
        real = rng.choice([S, S, rng.randint(1, S), max(1, S - rng.randint(0, 300))])
        band = rng.choice([0, 1, rng.randint(2, 200), rng.randint(100, S), rng.randint(100, S), S + 1])
        lo = min(S, rng.choice([0, 256, rng.randint(0, S - 1)]))
        cf = (lo, min(S, lo + rng.choice([0, 1, 64, rng.randint(1, 300)])))
        lo = min(S, rng.choice([0, 256, 512, rng.randint(0, S - 1)]))
        rf = (lo, min(S, lo + rng.choice([0, 1, 30, 256, rng.randint(1, 400)])))
        prm = dict(real_len=real, band=band, colfull_lo=cf[0], colfull_hi=cf[1], rowfull_lo=rf[0], rowfull_hi=rf[1])
        F_ = rng.choice([1, 2, 3, 5, 8, 21, 33, 63, 64, 65])
        vid0 = rng.choice([0, 0, 26, 64, 226])
        P_ = rng.randint(1, max(1, (S - vid0) // F_))
        if vid0 + F_ * P_ > S:
            vid0 = 0
        nqt = (S + BM - 1) // BM + 3   # (regions may add q-tiles; check_mask drops what does not exist)
        qts = sorted({0, 1, rng.randrange(nqt), rng.randrange(nqt), nqt - 4, nqt - 3, nqt - 2, nqt - 1})
        waves = sorted({0, 7, rng.randrange(NW)})
        in_run, _, _ = check_mask(S, prm, vid0, F_, P_, qts=qts, waves=waves)
        n_runs += in_run > 0
    assert n_runs > 100, n_runs   # the family does exercise runs


def test_bad_arguments_are_refused():
    lib = nat.load()
    S = 1000
    mask = nat.BandMask(**O.dense_band_params(S))
    out4 = np.zeros(4, dtype=np.int32)
    tiles = np.zeros(4 * 16, dtype=np.int32)
    rows = np.zeros(BN * 16, dtype=np.int32)

    def call(S=S, qt=0, wave=0, dist=2, F=2, P=100, tm=0, tw=tiles.size, rw=rows.size, o=out4.ctypes.data):
        return lib.svg_debug_band_tile_run(S, C.byref(mask), 0, F, P, tm, qt, wave, dist, o, tiles.ctypes.data, tw, rows.ctypes.data, rw)

    assert call() == 16
    assert call(qt=4) == -1 and call(qt=-1) == -1          # 4 q-tiles
    assert call(wave=8) == -1 and call(wave=-1) == -1
    assert call(dist=0) == -1
    assert call(tw=4 * 16 - 1) == -1 and call(rw=BN * 16 - 1) == -1   # too small: not overrun
    assert call(F=3, P=400) == -1                           # video longer than S
    assert call(F=0, P=0, tm=1) == -1                       # a token-major head needs a video
    assert call(o=None) == -1


def test_share_of_tiles_in_runs_hy720p(capsys):
    """HunyuanVideo 720p, the benchmark's mask: the share of (wave, key tile) pairs inside runs.  Recorded, not asserted."""
    from svg.models.hyvideo.utils import sparsity_to_width

    F_, P_, ctx, L_ = 33, 3600, 256, 64
    S = F_ * P_ + ctx
    prm = O.hy_band_params(S, ctx, L_, F_, P_, sparsity_to_width(0.25, ctx, F_, P_))
    nqt = tile_run(S, prm, 0, F_, P_, 0, 0, 0, 2, detail=False)[3]
    for tm in (0, 1):
        in_run = total = 0
        for qt in range(nqt):
            for wave in range(NW):
                r = tile_run(S, prm, 0, F_, P_, tm, qt, wave, 2 if wave < NW // 2 else 3, detail=False)
                in_run, total = in_run + r[1], total + r[2]
        with capsys.disabled():
            print(f"\nhy720p band={prm['band']} {'token-major' if tm else 'contiguous'} head: {in_run} of {total} wave-tiles inside runs "
                  f"= {in_run / total:.4f}")
        assert total > 0
    # a spot check of the walk at this size (index range, wrap of the frame index on most tiles): three q-tiles, both head kinds
    for qt in (0, nqt // 2, nqt - 1):
        for tm in (0, 1):
            check(S, prm, 0, F_, P_, tm, qt, 5, 3)
