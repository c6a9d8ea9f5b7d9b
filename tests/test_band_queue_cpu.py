"""The work queue of the resident band kernels (csrc/band_policy.h BandQueue) on the host: svg_band_queue_order writes the eight
XCD lists and the tail the device takes from, so no GPU is needed to check that
  * every (head, q-tile) of a launch is handed out exactly once — full-size HunyuanVideo geometries, the tiny benchmark geometry,
    a 3-head launch, and masks with empty regions (no text rows, no rows behind real_len, a band that covers everything, one or two
    work items);
  * the order is the documented one: text-row q-tiles first and spread over the lists, full-length q-tiles before shortened ones,
    the tail by rank — longest first at either end of every head;
  * the Python mirror in tools/band_queue_sim.py (the dispatch model) is the same order, and the model's makespan for it lies
    within 0.005 of one chip-wide longest-first queue for the three launches the model was made for."""
import ctypes as C
import importlib.util
from pathlib import Path

import pytest

from svg import _native as nat

ROOT = Path(__file__).resolve().parent.parent


def _sim():
    spec = importlib.util.spec_from_file_location("band_queue_sim", ROOT / "tools" / "band_queue_sim.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def hy_mask(F, P, ctx, L, band):
    V = F * P
    return V + ctx, nat.BandMask(real_len=V + L, band=band, colfull_lo=V, colfull_hi=V + L, rowfull_lo=V, rowfull_hi=V + L)


def order(BH, S, mask):
    lib = nat.load()
    n = lib.svg_band_queue_order(BH, S, C.byref(mask), None, 0)
    assert n > 0
    buf = (C.c_int32 * (3 * n))()
    assert lib.svg_band_queue_order(BH, S, C.byref(mask), C.cast(buf, C.c_void_p), 3 * n) == n
    assert lib.svg_band_queue_order(BH, S, C.byref(mask), C.cast(buf, C.c_void_p), 3 * n - 1) == -1   # too small: refused, not overrun
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(n)]


# name -> (heads, S, mask)
def _cases():
    out = {}
    for name, H, F, P, ctx, L, band in (("hy720p", 24, 33, 3600, 256, 64, 15616), ("hy480p", 24, 33, 1350, 256, 64, 5632),
                                        ("tiny", 4, 5, 600, 256, 64, 384), ("hy720p_3_heads", 3, 33, 3600, 256, 64, 15616)):
        S, m = hy_mask(F, P, ctx, L, band)
        out[name] = (H, S, m)
    S = 20 * 256 + 100
    out["no_text_rows"] = (5, S, nat.BandMask(real_len=S - 60, band=1024, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["no_pad_rows"] = (5, S, nat.BandMask(real_len=S, band=1024, colfull_lo=S - 100, colfull_hi=S, rowfull_lo=S - 100, rowfull_hi=S))
    out["band_covers_all"] = (3, S, nat.BandMask(real_len=S, band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["band_half"] = (7, S, nat.BandMask(real_len=S - 60, band=S // 2, colfull_lo=S - 200, colfull_hi=S - 60, rowfull_lo=S - 200,
                                          rowfull_hi=S - 60))
    out["band_zero"] = (2, S, nat.BandMask(real_len=S - 60, band=0, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["one_item"] = (1, 200, nat.BandMask(real_len=200, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["two_items"] = (2, 256, nat.BandMask(real_len=256, band=64, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0))
    out["many_heads"] = (300, 700, nat.BandMask(real_len=650, band=128, colfull_lo=600, colfull_hi=650, rowfull_lo=600, rowfull_hi=650))
    return out


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_head_and_q_tile_exactly_once(name):
    BH, S, mask = CASES[name]
    items = order(BH, S, mask)
    assert len(items) % BH == 0
    ids = sorted(i for _, i, _ in items)
    assert ids == list(range(len(items))), "a (head, q-tile) pair is missing or handed out twice"
    assert all(0 <= x <= 8 for x, _, _ in items)
    # one q-tile has the same number of key tiles in every head
    nqt = len(items) // BH
    per_tile = {}
    for _, i, nT in items:
        assert per_tile.setdefault(i % nqt, nT) == nT


@pytest.mark.parametrize("name", ["hy720p", "hy480p", "tiny", "hy720p_3_heads"])
def test_order_is_text_rows_then_full_length_then_shortened_longest_first(name):
    BH, S, mask = CASES[name]
    items = order(BH, S, mask)
    nqt = len(items) // BH
    lists = [[(i, nT) for x, i, nT in items if x == l] for l in range(9)]
    heavy = max(nT for _, _, nT in items)
    n_heavy = sum(1 for _, _, nT in items if nT == heavy)
    assert n_heavy == BH                                   # one q-tile of text rows per head in these geometries
    per_list = [sum(1 for _, nT in l if nT == heavy) for l in lists[:8]]
    assert max(per_list) - min(per_list) <= 1, per_list   # spread over the XCDs
    longest = max(nT for _, _, nT in items if nT != heavy)
    for l in lists[:8]:
        nts = [nT for _, nT in l]
        k = per_list[lists.index(l)]
        assert all(n == heavy for n in nts[:k])            # first
        rest = nts[k:]
        last_full = max((j for j, n in enumerate(rest) if n == longest), default=-1)
        first_short = min((j for j, n in enumerate(rest) if n < longest), default=len(rest))
        assert last_full < first_short                     # full-length q-tiles before every shortened one
    # the tail goes by rank (distance from the full-length tiles), all heads abreast: at either end of a head the key tiles only go
    # down, and where the two ends of a head lose key tiles at the same rate (HunyuanVideo) the whole tail is sorted
    tail = lists[8]
    assert len(tail) <= 256 + 2 * BH
    for h in range(BH):
        for back in (False, True):
            nts = [nT for i, nT in tail if i // nqt == h and (i % nqt >= nqt // 2) == back]
            assert nts == sorted(nts, reverse=True)
    heads_of = [i // nqt for i, _ in tail]
    assert all(heads_of.count(h) == len(tail) // BH for h in range(BH))
    if name.startswith("hy"):
        nts = [nT for _, nT in tail]
        assert all(b <= a + 4 for a, b in zip(nts, nts[1:]))   # (one rank = 256 rows = 4 key tiles)
        assert min(nT for l in lists[:8] for _, nT in l) >= nts[0] - 4   # nothing outside the tail is shorter than its start
    # a chunk of 32 consecutive entries of a list stays within neighbouring q-tiles of at most two heads (more only where a head has
    # fewer than 32 q-tiles)
    for l in lists[:8]:
        body = [i for i, nT in l if nT != heavy]
        for c in range(0, len(body) - 31, 32):
            assert len({i // nqt for i in body[c:c + 32]}) <= 2 + 32 // nqt


@pytest.mark.parametrize("name", sorted(CASES))
def test_python_mirror_of_the_model_is_the_library_order(name):
    sim = _sim()
    BH, S, mask = CASES[name]
    geo = dict(S=S, real=mask.real_len, band=mask.band, cf_lo=mask.colfull_lo, cf_hi=mask.colfull_hi, rf_lo=mask.rowfull_lo,
               rf_hi=mask.rowfull_hi)
    has_rf = mask.rowfull_hi > mask.rowfull_lo and mask.rowfull_lo < mask.real_len and mask.band <= S
    tiles, heavy = sim.tiles_of(S, mask.real_len, mask.rowfull_lo if has_rf else 0, mask.rowfull_hi if has_rf else 0)
    nT = [sim.key_tiles(a, b, **geo) for a, b in tiles]
    q = sim.queue_of(BH, len(tiles), heavy[0] if heavy else 0, len(heavy), nT)
    mirror = [(x, h * len(tiles) + qt, nT[qt]) for x, lst in enumerate(sim.lists_of(q)) for h, qt in lst]
    assert mirror == order(BH, S, mask)


def test_model_makespan_within_half_a_percent_of_one_balanced_queue():
    sim = _sim()
    shipped = {"hy720p 24": 1.012, "hy480p 24": 1.052, "hy720p  3": 1.173}   # the static mapping, as the model has always given it
    for launch in sim.LAUNCHES:
        res = sim.run(*launch, verbose=False)
        assert abs(res["shipped"] - shipped[launch[0][:9]]) < 0.0015, (launch[0], res)
        assert res["queue"] <= res["balanced"] + 0.005, (launch[0], res)
        assert res["queue"] < res["shipped"]
