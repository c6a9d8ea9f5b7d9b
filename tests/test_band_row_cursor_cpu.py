"""The row cursor of the 16x16x32 band kernels (csrc/band_policy.h RowWalk, row_walk_next) walked on the host by
svg_debug_band_row_cursor, against the division it replaces: a key tile that follows the latest resolved one by 64 keys and lies wholly
inside the range is stepped (contiguous head: phys += 64; token-major head: phys += sp64, minus V - 1 when that left the video), every
other tile divides.  Every row of every tile must be the row the placement formula gives — logical row l of a token-major head lives at
vid0 + ((l - vid0) % F) * P + (l - vid0) / F inside the video, at l outside it, and rows behind S resolve to 0 — for frame counts on both
sides of the tile size (64 / F = 0, 1, many; 64 % F = 0 and not), text in front of the video and behind it, and key sequences with a
segment jump, a tile over each end of the video and a tile over S."""
import ctypes as C

import numpy as np
import pytest

from svg import _native as nat

BN = 64
FRAMES = [1, 2, 3, 8, 21, 33, 63, 64, 65, 100]
SIZES = [1, 7, 64, 100]
TEXT = 256   # rows that are not video


def walk(S, vid0, F, P, token_major, k0s):
    lib = nat.load()
    k0 = np.asarray(k0s, dtype=np.int32)
    out = np.full(BN * len(k0), -7, dtype=np.int32)
    cheap = np.full(len(k0), -7, dtype=np.int32)
    n = lib.svg_debug_band_row_cursor(S, vid0, F, P, int(token_major), k0.ctypes.data, len(k0), out.ctypes.data, out.size, cheap.ctypes.data)
    assert n == len(k0)
    return out.reshape(len(k0), BN), cheap


def expected(S, vid0, F, P, token_major, k0s):
    l = np.asarray(k0s, dtype=np.int64)[:, None] + np.arange(BN)[None, :]
    i = l - vid0
    inside = (i >= 0) & (i < F * P)
    phys = np.where(inside & bool(token_major), vid0 + (i % F) * P + i // F, l)
    return np.where(l < S, phys, 0)


def key_sequence(S, vid0, V):
    """first keys of the tiles a q-tile may visit, in increasing order: a run over the start of the video, a run further inside it (a
    segment jump where the video is long enough), and a run over the end of the video, the text behind it and S"""
    tiles = (S + BN - 1) // BN
    a = vid0 // BN                                   # the tile with the first video row (straddles the start unless vid0 % 64 == 0)
    e = (vid0 + V - 1) // BN                         # the tile with the last video row
    picked = set(range(max(a - 1, 0), a + 5)) | set(range(a + 9, a + 13)) | set(range(max(e - 4, 0), tiles))
    return [t * BN for t in sorted(picked) if t < tiles]


@pytest.mark.parametrize("vid0", [0, 226])
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("F", FRAMES)
def test_cursor_matches_division(F, P, vid0):
    V = F * P
    S = vid0 + V + (TEXT if vid0 == 0 else 0) + 37
    S += S % BN == 0   # S is no multiple of 64: the last tile straddles it
    k0s = key_sequence(S, vid0, V)
    assert k0s == sorted(set(k0s)) and k0s[-1] + BN > S
    for token_major in (0, 1):
        got, cheap = walk(S, vid0, F, P, token_major, k0s)
        want = expected(S, vid0, F, P, token_major, k0s)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (token_major, bad[:4], got[tuple(bad[0])], want[tuple(bad[0])])
        # which tiles may be stepped is part of the contract: the first tile, a tile after a jump, and a tile that is not wholly inside
        # the range never are; (token-major) nor is the tile behind one that straddled the start of the video
        lo, hi = (vid0 + BN, vid0 + V - BN) if token_major else (-(1 << 30), S - BN)
        for j, k0 in enumerate(k0s):
            follows = j > 0 and k0 == k0s[j - 1] + BN
            assert cheap[j] == int(follows and lo <= k0 <= hi), (token_major, j, k0)


def test_steps_are_taken_where_the_benchmark_runs():
    """HunyuanVideo 720p (33 frames of 3600 tokens, 64 % 33 = 31: the frame index wraps on most tiles): a long run inside the video is
    stepped tile after tile and never drifts from the division"""
    F, P, ctx = 33, 3600, 256
    V = F * P
    S = V + ctx
    k0s = list(range(0, 700 * BN, BN)) + list(range(V // BN * BN - 5 * BN, S, BN))
    for token_major in (0, 1):
        got, cheap = walk(S, 0, F, P, token_major, k0s)
        assert np.array_equal(got, expected(S, 0, F, P, token_major, k0s))
        assert cheap[0] == 0 and cheap[1:700].all()   # all but the first tile


def test_bad_arguments_are_refused():
    lib = nat.load()
    k0 = np.zeros(2, dtype=np.int32)
    out = np.zeros(2 * BN, dtype=np.int32)
    assert lib.svg_debug_band_row_cursor(1000, 0, 3, 100, 1, k0.ctypes.data, 2, out.ctypes.data, 2 * BN - 1, None) == -1   # too small: not overrun
    assert lib.svg_debug_band_row_cursor(1000, 0, 3, 400, 1, k0.ctypes.data, 2, out.ctypes.data, 2 * BN, None) == -1      # video longer than S
    assert lib.svg_debug_band_row_cursor(1000, 0, 3, 100, 1, None, 2, out.ctypes.data, 2 * BN, None) == -1
    assert lib.svg_debug_band_row_cursor(1000, 0, 3, 100, 1, k0.ctypes.data, 2, out.ctypes.data, 2 * BN, None) == 2
