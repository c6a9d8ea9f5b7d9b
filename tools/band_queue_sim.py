#!/usr/bin/env python3
"""CPU model of how a band-attention launch drains over 8 XCDs x 32 CUs (no GPU, no timing: a count of tile iterations).

    python tools/band_queue_sim.py

cost(workgroup or work item) = key tiles x the measured cost-vs-fill factor of DESIGN 3.1.3 + a constant.  Three schedules:
  shipped   the static mapping of BandPolicy::init (csrc/band_policy.h): dispatch id b runs on XCD b % 8, each XCD hands its ids
            to its 32 CUs in id order — what every launch did before the work queue and what the launches that count completions
            and the device-switched ones still do;
  queue     the work queue of BandQueue (csrc/band_policy.h), replayed by the Python mirror below (queue_of / decode / item;
            tests/test_band_queue_cpu.py holds it against the library's svg_band_queue_order): 256 resident workgroups, each
            taking from its XCD's list, when that is dry from the next XCD's, and last from the chip-wide tail;
  balanced  one chip-wide queue, longest first: the bound an order can reach.
Printed: makespan over the ideal sum / 256."""
import heapq
import math

FILL = {256: 1.0, 224: .93, 192: .86, 160: .79, 128: .67, 96: .62, 64: .60}
NUM_XCD, CHUNK, TAIL, BM, BN = 8, 32, 256, 256, 64


def tiles_of(S, real, rf_lo, rf_hi):
    """q-tiles in row order (make_band_params): they never straddle rowfull_lo / rowfull_hi / real_len"""
    has_rf = rf_hi > rf_lo and rf_lo < real
    a, b = (max(rf_lo, 0), min(rf_hi, real)) if has_rf else (0, 0)
    out, heavy = [], []
    cuts = [0, a, b, real, S]
    for i in range(4):
        q = cuts[i]
        while q < cuts[i + 1]:
            if has_rf and i == 1:
                heavy.append(len(out))
            out.append((q, min(cuts[i + 1], q + BM)))
            q += BM
    if len(heavy) >= len(out):
        heavy = []
    return out, heavy


def key_tiles(q0, qe, S, real, band, cf_lo, cf_hi, rf_lo, rf_hi):
    """BandPolicy::kv_schedule: key tiles of the q-tile of rows [q0, qe)"""
    segs = []
    if q0 < real:
        qr1 = min(qe, real)
        if q0 < rf_hi and qr1 > rf_lo:
            segs.append((0, math.ceil(real / BN)))
        else:
            segs.append((max(0, q0 - band + 1) // BN, math.ceil(min(real, qr1 - 1 + band) / BN)))
            ch = min(cf_hi, real)
            if ch > cf_lo:
                segs.append((cf_lo // BN, math.ceil(ch / BN)))
    if qe > real:
        segs.append((real // BN, math.ceil(S / BN)))
    segs.sort()
    n, end = 0, -1
    for lo, hi in segs:
        lo = max(lo, end)
        if hi > lo:
            n += hi - lo
            end = hi
    return n


def queue_of(BH, nqt, heavy_lo, n_heavy, nT):
    """make_band_queue: nT[qt] = key tiles of q-tile qt"""
    nl = nqt - n_heavy
    light = [nT[r if r < heavy_lo else r + n_heavy] for r in range(nl)]
    e_lo = e_hi = 0
    if nl:
        longest = max(light)
        e_lo = light.index(longest)
        e_hi = light[::-1].index(longest)
    r0 = max(0, max(e_lo, e_hi) - (TAIL + 2 * BH - 1) // (2 * BH))
    n_tail = BH * (max(0, e_lo - r0) + max(0, e_hi - r0))
    return dict(n_items=BH * nqt, BH=BH, nh=BH * n_heavy, n_heavy=n_heavy, heavy_lo=heavy_lo, nl=nl, e_lo=e_lo, e_hi=e_hi, r0=r0,
                n_tail=n_tail)


def decode(q, w):
    """BandQueue::decode: work item w -> (head, q-tile)"""
    if w < q["nh"]:
        return w // q["n_heavy"], q["heavy_lo"] + w % q["n_heavy"]
    nl, e_lo, e_hi, BH, r0 = q["nl"], q["e_lo"], q["e_hi"], q["BH"], q["r0"]

    def edge_tile(rank, back):
        return nl - e_hi + rank if back else e_lo - 1 - rank

    w2 = w - q["nh"]
    nf = nl - e_lo - e_hi
    if w >= q["n_items"] - q["n_tail"]:
        w2 = w - (q["n_items"] - q["n_tail"])
        m = min(e_lo, e_hi)
        both = (m - r0) * 2 * BH if m > r0 else 0
        if w2 < both:
            j = w2 % (2 * BH)
            head, r = j >> 1, edge_tile(r0 + w2 // (2 * BH), j & 1)
        else:
            w2 -= both
            head, r = w2 % BH, edge_tile(max(m, r0) + w2 // BH, e_hi > e_lo)
    elif w2 < BH * nf:
        head, r = w2 // nf, e_lo + w2 % nf
    else:
        w2 -= BH * nf
        b_lo, b_hi = min(e_lo, r0), min(e_hi, r0)
        t0 = 0
        while True:
            assert t0 < r0
            cl, ct = min(max(b_lo - t0, 0), CHUNK), min(max(b_hi - t0, 0), CHUNK)
            c = cl + ct
            if w2 < BH * c:
                head, j = w2 // c, w2 % c
                r = edge_tile(t0 + j, False) if j < cl else edge_tile(t0 + j - cl, True)
                break
            w2 -= BH * c
            t0 += CHUNK
    return head, (r if r < q["heavy_lo"] else r + q["n_heavy"])


def item(q, xcd, i):
    """BandQueue::item: entry i of XCD xcd's list, or -1 behind its end"""
    if i >= q["n_items"]:
        return -1
    nhx = (q["nh"] - xcd + NUM_XCD - 1) // NUM_XCD if q["nh"] > xcd else 0
    if i < nhx:
        return xcd + NUM_XCD * i
    i2 = i - nhx
    w = q["nh"] + ((i2 // CHUNK) * NUM_XCD + xcd) * CHUNK + i2 % CHUNK
    return w if w < q["n_items"] - q["n_tail"] else -1


def lists_of(q):
    """the eight lists and the tail as [(head, q-tile), ...]"""
    out = []
    for x in range(NUM_XCD):
        lst, i = [], 0
        while (w := item(q, x, i)) >= 0:
            lst.append(decode(q, w))
            i += 1
        out.append(lst)
    out.append([decode(q, q["n_items"] - q["n_tail"] + i) for i in range(q["n_tail"])])
    return out


def makespan_queue(lists, cost, n_wg=256):
    """n_wg resident workgroups, workgroup g on XCD g % 8; the one that is free first takes next (BandQueue::take): from its XCD's
    list, then from the other XCDs', then from the tail"""
    pos = [0] * (NUM_XCD + 1)
    free = [(0.0, g) for g in range(n_wg)]
    heapq.heapify(free)
    end = 0.0
    while free:
        t, g = heapq.heappop(free)
        for x in [(g + k) % NUM_XCD for k in range(NUM_XCD)] + [NUM_XCD]:
            if pos[x] < len(lists[x]):
                _, qt = lists[x][pos[x]]
                pos[x] += 1
                heapq.heappush(free, (t + cost[qt], g))
                break
        else:
            end = max(end, t)
    return end


def run(name, H, F, P, ctx, L, band, o_wg=8, verbose=True):
    V = F * P
    S = V + ctx
    real = V + L
    mask = dict(S=S, real=real, band=band, cf_lo=V, cf_hi=real, rf_lo=V, rf_hi=real)
    tiles, heavy = tiles_of(S, real, V, real)
    nqt, nhv = len(tiles), len(heavy)
    nT = [key_tiles(a, b, **mask) for a, b in tiles]

    def cost_of(qt):
        rows = max(64, tiles[qt][1] - tiles[qt][0])
        r = min(FILL, key=lambda x: abs(x - rows))
        return nT[qt] * FILL[r] + o_wg

    c = [cost_of(t) for t in range(nqt)]
    heavy_lo = heavy[0] if heavy else 0
    nh, total = H * nhv, nqt * H
    work = []
    for b in range(total):                              # BandPolicy::init
        if b < nh:
            qt = heavy_lo + b % nhv
        else:
            b2 = b - nh
            full = ((total - nh) // 256) * 256
            w2 = b2
            if b2 < full:
                x, s = b2 % 8, b2 // 8
                w2 = (s // 32) * 256 + x * 32 + (s % 32)
            nl = nqt - nhv
            r = w2 % nl
            qt = r if (not heavy or r < heavy_lo) else r + nhv
        work.append((b % 8, c[qt]))
    ideal = sum(w for _, w in work) / 256
    ends = []
    for x in range(8):
        cu = [0.0] * 32
        heapq.heapify(cu)
        for xx, w in work:
            if xx == x:
                heapq.heappush(cu, heapq.heappop(cu) + w)
        ends.append(max(cu))
    cu = [0.0] * 256
    heapq.heapify(cu)
    for w in sorted((w for _, w in work), reverse=True):
        heapq.heappush(cu, heapq.heappop(cu) + w)
    q = queue_of(H, nqt, heavy_lo, nhv, nT)
    res = dict(shipped=max(ends) / ideal, queue=makespan_queue(lists_of(q), c) / ideal, balanced=max(cu) / ideal)
    if verbose:
        print(f"{name}: {total / 256:.1f} workgroups per CU, {sum(nT) / nqt:.0f} key tiles per workgroup; makespan / ideal: shipped order "
              f"{res['shipped']:.3f}, work queue {res['queue']:.3f}, one balanced queue, longest first {res['balanced']:.3f}")
    return res


LAUNCHES = [("hy720p 24 heads band 15616", 24, 33, 3600, 256, 64, 15616),
            ("hy480p 24 heads band 5632 ", 24, 33, 1350, 256, 64, 5632),
            ("hy720p  3 heads band 15616", 3, 33, 3600, 256, 64, 15616)]

if __name__ == "__main__":
    for launch in LAUNCHES:
        run(*launch)
