"""Inputs of the replay tests of the bf16 band kernels at head_dim 128 (SPEC, csrc/attn_m16.h): the geometries, the spike builder and the
case lists.  Plain module, no GPU: tests/test_gpu_band_speculative.py and tests/test_gpu_band_replay_paths.py launch these cases, and
tests/test_band_replay_cases_cpu.py checks on the CPU that the inputs mean what the GPU tests assume they mean.

Inputs are built in LOGICAL row order (what the mask speaks of); head 1 is token-major and is carried to its physical order with the
oracle's inverse head placement by the launching side, so that "key tile t of q-tile j" means the same for both heads.  The last ten
dimensions of q and k are zero except for the spikes: a spike lives in one dimension of its own (118 + slot; one query row, one key row,
of every head or of one), q = 4.0 and k = mag / (4 c), so it raises exactly one score — to `mag` in the log2 domain, against at most
about +8 for everything else — and no other.  Two spikes on one query row (two slots, two keys) make a row whose answer is a weighted
mean of two v rows.

Geometry A (the one of tests/test_gpu_band_speculative.py): S = 2 x 640 + 64 = 1344 = 21 key tiles, band 512; per head five band
q-tiles (0 .. 4), the text q-tile (5: rows 1280 .. 1319) and the q-tile of the rows behind real_len (6): 14 work items.
Geometry B is ragged: S = 2 x 600 + 100 = 1300, real_len 1240: the last key tile holds 20 keys, the q-tile regions are cut at 1200 and
1240, the last video q-tile has 176 rows, and the text columns 1200 .. 1239 straddle key tiles 18 and 19."""
import ctypes as C
import math
from typing import NamedTuple, Optional, Tuple

import torch

from oracle import svg_oracle as O

SPIKE_DIM0 = 118
BEST = torch.tensor([[0, 1]])    # head 0 contiguous, head 1 token-major
LN2 = math.log(2.0)
BM, BN = 256, 64                 # rows of a q-tile, keys of a key tile


class Geo(NamedTuple):
    D: int
    H: int
    F: int
    P: int
    CTX: int
    L: int
    BAND: int

    @property
    def V(self):
        return self.F * self.P

    @property
    def S(self):
        return self.V + self.CTX

    @property
    def REAL(self):
        return self.V + self.L

    @property
    def c_log2(self):
        """score in the log2 domain = (q . k) * c_log2"""
        return (1.0 / math.sqrt(self.D)) * math.log2(math.e)

    def mask_params(self, kind):
        """band: the HunyuanVideo-like band mask; dense: everything (real_len = S); dense_real: everything up to real_len"""
        if kind == "dense":
            return O.dense_band_params(self.S)
        if kind == "dense_real":
            return O.dense_band_params(self.S, self.REAL)
        assert kind == "band"
        return dict(real_len=self.REAL, band=self.BAND, colfull_lo=self.V, colfull_hi=self.REAL, rowfull_lo=self.V, rowfull_hi=self.REAL)

    def q_tile_cuts(self, kind):
        """row regions that no q-tile straddles (make_band_params; tools/band_queue_sim.py tiles_of)"""
        p = self.mask_params(kind)
        has_rf = p["rowfull_hi"] > p["rowfull_lo"] and p["rowfull_lo"] < p["real_len"] and p["band"] <= self.S
        cuts = {0, p["real_len"], self.S}
        if has_rf:
            cuts |= {p["rowfull_lo"], min(p["rowfull_hi"], p["real_len"])}
        return sorted(cuts)

    def q_tile_of(self, kind, row):
        """(region, q-tile within the region) of a logical row"""
        cuts = self.q_tile_cuts(kind)
        reg = max(i for i, c in enumerate(cuts[:-1]) if row >= c)
        return reg, (row - cuts[reg]) // BM

    def q_tiles(self, kind):
        """the q-tiles of one head in row order, as (first row, end row): the index is the q-tile number of the work queue"""
        cuts = self.q_tile_cuts(kind)
        return [(q, min(hi, q + BM)) for lo, hi in zip(cuts, cuts[1:]) for q in range(lo, hi, BM)]


GEO_A = Geo(D=128, H=2, F=2, P=640, CTX=64, L=40, BAND=512)
GEO_B = Geo(D=128, H=2, F=2, P=600, CTX=100, L=40, BAND=512)


class Spike(NamedTuple):
    row: int
    key: int
    mag: float
    head: Optional[int] = None    # None: every head
    slot: Optional[int] = None    # dimension SPIKE_DIM0 + slot; None: the position in the case's list

    def heads(self, H):
        return range(H) if self.head is None else (self.head,)


def as_spikes(spikes):
    sp = tuple(s if isinstance(s, Spike) else Spike(*s) for s in spikes)
    sp = tuple(s if s.slot is not None else s._replace(slot=i) for i, s in enumerate(sp))
    return sp


class Case(NamedTuple):
    name: str
    geo: Geo
    kinds: Tuple[str, ...]            # every mask a launch of this case runs under
    spikes: Tuple[Spike, ...]
    seed: int
    dtype: torch.dtype = torch.bfloat16
    prescaled: bool = False           # q carries softmax_q_scale(D) (q_prescaled=True; the oracle then runs with scale = ln 2)
    pairs: Tuple[Tuple[int, int, int], ...] = ()   # (row, key a, key b): rows with two spikes (section 5 b)

    def without_spikes(self):
        return self._replace(name=self.name + "/no_spikes", spikes=(), pairs=())

    def replaying_pairs(self):
        """(head, q-tile) pairs that hold a spike, under the first mask of the case"""
        return {(h, self.geo.q_tile_of(self.kinds[0], s.row)) for s in self.spikes for h in s.heads(self.geo.H)}


_MASKS = {}


def bool_mask(kind, geo=GEO_A):
    if (geo, kind) not in _MASKS:
        _MASKS[geo, kind] = O.band_mask(geo.S, **geo.mask_params(kind))
    return _MASKS[geo, kind]


def build_inputs(geo, kinds, spikes, seed, dtype=torch.bfloat16, prescaled=False):
    """-> logical q, k, v (`dtype`, CPU).  Every spiked (row, key) must be allowed by every mask of `kinds`."""
    spikes = as_spikes(spikes)
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(1, geo.H, geo.S, geo.D, generator=g) for _ in range(3))
    q[..., SPIKE_DIM0:] = 0
    k[..., SPIKE_DIM0:] = 0
    slots = [s.slot for s in spikes]
    assert len(set(slots)) == len(slots) and all(0 <= x < geo.D - SPIKE_DIM0 for x in slots), slots
    c = geo.c_log2
    for s in spikes:
        for kind in kinds:
            assert bool_mask(kind, geo)[s.row, s.key], (kind, s)
        for h in s.heads(geo.H):
            q[0, h, s.row, SPIKE_DIM0 + s.slot] = 4.0
            k[0, h, s.key, SPIKE_DIM0 + s.slot] = s.mag / (4.0 * c)
    if prescaled:
        q = q * c
    return tuple(x.to(dtype) for x in (q, k, v))


def build(kind, spikes, seed):
    """geometry A, bf16: per head the same list of (query row, key row, mag) in logical order -> logical q, k, v"""
    return build_inputs(GEO_A, (kind,), spikes, seed)


def inputs(case):
    return build_inputs(case.geo, case.kinds, case.spikes, case.seed, case.dtype, case.prescaled)


_REFS = {}


def oracle(case, kind):
    """O.masked_attention on the case's inputs (as rounded to its dtype) under the mask `kind`; computed once"""
    assert kind in case.kinds
    key = (case.geo, kind, case.spikes, case.seed, case.dtype, case.prescaled)
    if key not in _REFS:
        q, k, v = inputs(case)
        _REFS[key] = O.masked_attention(q, k, v, bool_mask(kind, case.geo), scale=LN2 if case.prescaled else None)
    return _REFS[key]


def reference(kind, spikes, seed):
    return oracle(Case("", GEO_A, (kind,), as_spikes(spikes), seed), kind)


def q_tiles_of(kind, rows, geo=GEO_A):
    """number of q-tiles (256 rows, cut at the row regions of the mask) that contain one of `rows`"""
    return len({geo.q_tile_of(kind, r) for r in rows})


def replay_everywhere_spikes():
    """geometry A: one +400 spike in every q-tile of real rows, off the check points (key tile index 3 of the band q-tiles 0 .. 4, whose
    schedules start at key tile max(0, 256 j - 511) // 64; index 5 of the text q-tile): each of them is replayed"""
    sp = [(256 * j + 40, (max(0, 256 * j - 511) // 64 + 3) * 64 + 5, 400.0) for j in range(5)]
    sp.append((GEO_A.V + 3, 64 * 5 + 1, 400.0))
    return sp


# ------------------------------------------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------------------------------------------
SEED_A = 5     # with this seed every q-tile of replay_everywhere_spikes() replays exactly once (tests/test_gpu_band_speculative.py)


def everywhere_subset(q_tiles, head=None, mag=400.0):
    """the spikes of replay_everywhere_spikes() in the q-tiles `q_tiles` (0 .. 5), each in the dimension it has there"""
    sp = replay_everywhere_spikes()
    return tuple(Spike(sp[j][0], sp[j][1], mag, head, j) for j in q_tiles)


def queue_order(geo, kind):
    """svg_band_queue_order (host only): [(list, head * q-tiles per head + q-tile, key tiles)] in the order the lists hand out"""
    from svg import _native as nat

    lib = nat.load()
    mask = nat.BandMask(**geo.mask_params(kind))
    n = lib.svg_band_queue_order(geo.H, geo.S, C.byref(mask), None, 0)
    assert n == geo.H * len(geo.q_tiles(kind)), n
    buf = (C.c_int32 * (3 * n))()
    assert lib.svg_band_queue_order(geo.H, geo.S, C.byref(mask), C.cast(buf, C.c_void_p), 3 * n) == n
    return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(n)]


def queue_edge_item(which):
    """geometry A, band mask: the (head, q-tile) the queue's lists hand out first / last among the q-tiles of real rows (0 .. 5)"""
    nqt = len(GEO_A.q_tiles("band"))
    real = [(i // nqt, i % nqt) for _, i, _ in queue_order(GEO_A, "band") if i % nqt <= 5]
    return real[0] if which == "first" else real[-1]


QUEUE_SUBSETS = ("all6", "024", "first", "last")
QUEUE_CAPS = (1, 2, 3)


def queue_case(subset, dtype=torch.bfloat16, prescaled=False):
    """section 1: geometry A, +400 spikes in a subset of the six q-tiles of real rows"""
    if subset == "all6":
        sp = everywhere_subset(range(6))
    elif subset == "024":
        sp = everywhere_subset((0, 2, 4))
    else:
        head, qt = queue_edge_item(subset)
        sp = everywhere_subset((qt,), head=head)
    tag = {torch.bfloat16: "bf16", torch.float16: "fp16"}[dtype] + ("_prescaled" if prescaled else "")
    return Case(f"queue_{subset}_{tag}", GEO_A, ("band",), sp, SEED_A, dtype, prescaled)


def switch_case():
    """section 2: the all-six pattern, every spiked pair allowed by the band mask and by the dense mask of the same real_len"""
    return Case("switch_all6", GEO_A, ("band", "dense_real"), everywhere_subset(range(6)), SEED_A)


# section 5: static mapping, spikes at key tile index 3 (and 5, 8) of a q-tile whose schedule starts at key tile 0, so the index is
# the key tile.  Row 514 is a row of wave 0 of q-tile 2 (rows 512 .. 767; sees keys 3 .. 1025).  The rows of wave 7 of that q-tile
# (736 .. 767) see key tile 3 partly or not at all — row 767 has no key before tile 4, which keeps the whole wave on the exact path of the
# start until then — so the wave-7 row is row 482 of the neighbouring q-tile 1 (rows 256 .. 511, schedule from key tile 0 too), which
# sees keys 0 .. 993.
ROW_W0, ROW_W7 = 514, 482
SWEEP_MAGS = (112, 118, 122, 126, 128, 130, 132, 134, 136, 138, 140, 142, 146, 160)
PAIR_MAGS = (60, 118, 126, 132, 140, 400)
PAIR_SECOND_TILE = {"off_check": 5, "on_check": 8}
SEED_SWEEP, SEED_PAIR = 11, 13


def sweep_case(mag):
    sp = (Spike(ROW_W0, 64 * 3 + 5, float(mag)), Spike(ROW_W7, 64 * 3 + 9, float(mag)))
    return Case(f"sweep_{mag}", GEO_A, ("band",), as_spikes(sp), SEED_SWEEP)


def pair_case(m, where):
    """magnitudes m and m - 1 on ONE row, at key tile 3 and at key tile 5 (off the check points) or 8 (on one): a row of wave 0 and a
    row of wave 7, four spikes"""
    t2 = PAIR_SECOND_TILE[where]
    pairs = ((ROW_W0, 64 * 3 + 5, 64 * t2 + 5), (ROW_W7, 64 * 3 + 9, 64 * t2 + 9))
    sp = []
    for row, ka, kb in pairs:
        sp += [Spike(row, ka, float(m)), Spike(row, kb, float(m - 1))]
    return Case(f"pair_{m}_{where}", GEO_A, ("band",), as_spikes(sp), SEED_PAIR, pairs=pairs)


SEED_B = 7
RAGGED_KINDS = ("band", "dense_real")


def ragged_case():
    """section 6: geometry B, +400 spikes, each on a row of its own and allowed by both masks"""
    g = GEO_B
    sp = (Spike(300, g.REAL - 1, 400.0),          # a video row against the last text key (key tile 19, beside the pad keys)
          Spike(g.V - 1, g.V - 101, 400.0),       # the last row of the short q-tile against a key in its band
          Spike(g.V + 10, 500, 400.0),            # a text row against a video key
          Spike(40, 64 * 3 + 5, 400.0))           # a row of q-tile 0 against a key of its fourth tile
    return Case("ragged", g, RAGGED_KINDS, as_spikes(sp), SEED_B)


def all_cases():
    """every case the GPU file launches (the spike-free companions included)"""
    cases = [queue_case(s) for s in QUEUE_SUBSETS]
    cases += [queue_case("all6", torch.float16), queue_case("all6", prescaled=True), switch_case()]
    cases += [sweep_case(m) for m in SWEEP_MAGS]
    cases += [pair_case(m, w) for m in PAIR_MAGS for w in PAIR_SECOND_TILE]
    cases += [ragged_case()]
    cases += [queue_case("all6").without_spikes(), ragged_case().without_spikes()]
    return cases
