"""Exact-arithmetic cases for the e4m3 attention path (csrc/attention_f8.hip, csrc/attn_f8.h, attn_body_f8g in attention_varblock.hip).
CPU only; imported by tests/test_fp8_exact_cases_cpu.py and tests/test_gpu_fp8_exact.py.

The distance tests of tests/test_gpu_fp8.py bound the e4m3 NOISE.  The cases here have none: every intermediate of the kernels is exactly
representable, so the kernels must reproduce the float64 result rounded once (up to the one inexact operation they have, the final
acc * (inv_v / l)).  At D = 128 and sm_scale = ln 2 / 8 (scale_log2 = 1 / 8):

  * q, k, v are exact in bf16 AND fp16 and, after the pre-pass's per-head scaling, in e4m3.  amax(k), amax(v) = 7 * 2^m per head (the scale
    448 / amax is a power of two), amax(q) = 5 * 2^m (log2(aq * ideal / 448) has fractional part ~0.515: the ceil of the pre-pass cannot flip
    on an ulp of log2f; the file is built with -ffast-math).
  * the exponent arguments x_ij = q_i . k_j / 8 are integers in [0, 12]: 2^(x - m_ref + 4) is an e4m3 number (2^-9 .. 2^8) for any
    reference m_ref the kernel may hold between the first-tile maximum and the row maximum.
  * v = small integers * 2^m: every partial sum of p * v8 and of p is exact in fp32 (emulate_f8pp asserts it as it goes).

Workspace layout of svg_band_attention_fp8_stage (run_f8 / f8_ws_bytes in csrc/attention_f8.hip), stated once, here:
    S_pad = ceil64(S), IMG = BH * S_pad * 128
    [0, IMG)            q8   [BH, S_pad, 128]         e4m3, rows >= S zero, LOGICAL token order (head placement applied)
    [IMG, 2 IMG)        k8   [BH, S_pad, 128]
    [2 IMG, 3 IMG)      vt8  [BH, S_pad / 64, 128, 64] byte position 32 g + 16 b + 4 j + i of a row <-> key 32 b + 8 j + 4 g + i of the tile
    [3 IMG, +12 BH)     amax [BH, 3] float bits of amax |q|, |k|, |v| (the pointer is rounded up to 64 bytes; 3 IMG is a multiple of 64, so
                        for a 64-byte aligned workspace nothing moves)
    then                scales [BH, 4] float: 2^e, 1 / sv, bits (127 + e) * 0x01010101, 0
    total               3 IMG + 28 BH + 256 (the rest is never written)

What the GPU tests were seen to catch (kernel source edited in a scratch build, one MI355X; red cases of the 40 of test_gpu_fp8_exact.py):
    mask interval of attn_body_f8pp one key longer / one key shorter    18 / 20 red (largest error in the dense case: 4 fp16 units)
    V^T slot formula of f8_quantize_kernel with g and b swapped         36 red, the pre-pass tests first
    l_run += stale psum (the sum from before the exact path's recomputation, not rescaled)      20 red
    l_run += psum moved in front of the exact path                      0 red: with l_run *= alpha behind it this is the same sum, exactly,
                                                                        while every term fits fp32 (it does for any x spread <= 13); it differs
                                                                        only once the stale sum overflows, which test_fp8_score_spikes sees
"""
import functools
import math

import torch

D = 128
KBN = 64                       # key tile
BM = 256                       # q-tile of the fp8 band kernel: 8 waves x 32 rows
SM_SCALE = math.log(2.0) / 8   # scale_log2 = 1 / 8; the production setting of q_prescaled in svg/models/_core.py is sm_scale = ln 2
SCALE_LOG2 = 0.125             # sm_scale * log2(e), exactly, in the arithmetic of the lossless cases
F8_MAX = 448.0
P_SHIFT = 4.0                  # kPShift of attn_f8.h
X_MAX = 12                     # exponent arguments of every case lie in [0, X_MAX]
X_SPREAD = 13                  # what e4m3 allows: 2^(-13 + 4) = 2^-9 is its smallest subnormal

# ---------------------------------------------------------------------------------------------------------------------------------------
# e4m3 (OCP, "fn": no infinities, S.1111.111 is NaN) as a table; round-to-nearest-even from float64 in one step
# ---------------------------------------------------------------------------------------------------------------------------------------
E4M3_VALUES = torch.arange(127, dtype=torch.uint8).view(torch.float8_e4m3fn).double()     # codes 0 .. 126 -> 0 .. 448, increasing


def e4m3_neighbours(y):
    """y float64 (any shape) -> (lo_code, hi_code, mid): the two adjacent e4m3 magnitudes |y| lies between (codes, hi = lo + 1, clamped
    at 448) and their midpoint"""
    a = y.abs().clamp(max=F8_MAX)
    hi = torch.searchsorted(E4M3_VALUES, a.contiguous(), right=True).clamp(max=126)      # first value > a
    lo = (hi - 1).clamp(min=0)
    lo = torch.where(a >= F8_MAX, hi, lo)               # 448 itself (and what saturates to it): no upper neighbour
    mid = (E4M3_VALUES[lo] + E4M3_VALUES[hi]) / 2
    return lo, hi, mid


def e4m3_bytes(y):
    """float64 -> uint8 e4m3 codes: round to nearest, ties to even, magnitudes above 448 saturate, the sign bit is the sign bit of y"""
    lo, hi, mid = e4m3_neighbours(y)
    a = y.abs().clamp(max=F8_MAX)
    up = (a > mid) | ((a == mid) & (lo % 2 == 1))
    code = torch.where(up, hi, lo)
    return (code + 128 * torch.signbit(y).long()).to(torch.uint8)


def e4m3_decode(b):
    return b.view(torch.float8_e4m3fn).double()


def is_e4m3_nan(b):
    return (b & 0x7F) == 0x7F


# ---------------------------------------------------------------------------------------------------------------------------------------
# rounding float64 ONCE to bf16 / fp16, and distance in units of the 16-bit format
# ---------------------------------------------------------------------------------------------------------------------------------------
_FMT = {torch.bfloat16: (8, -125), torch.float16: (11, -13)}      # significand bits, smallest frexp exponent of a normal number


def round_once(y, dtype):
    """float64 -> dtype with ONE rounding (torch's own conversion of a double goes through float32: two roundings)"""
    p, emin = _FMT[dtype]
    _, e = torch.frexp(y)
    quantum = torch.exp2((e.clamp(min=emin) - p).double())
    r = torch.round(y / quantum) * quantum             # torch.round: ties to even; the division by a power of two is exact
    out = r.to(dtype)
    assert torch.equal(out.double(), r)
    return out


def near_rounding_midpoint(y, dtype, rel):
    """elements of y (float64) within relative `rel` of the midpoint of two adjacent values of dtype"""
    p, emin = _FMT[dtype]
    _, e = torch.frexp(y)
    quantum = torch.exp2((e.clamp(min=emin) - p).double())
    u = y / quantum
    return ((u - torch.floor(u) - 0.5).abs() * quantum <= rel * y.abs()) & (y != 0)


def ordered(t):
    """16-bit float tensor -> int32 such that adjacent values of the format differ by 1 (+0 and -0 both map to 0)"""
    b = t.view(torch.int16).int()
    return torch.where(b >= 0, b, -(b & 0x7FFF))


# ---------------------------------------------------------------------------------------------------------------------------------------
# lossless inputs
# ---------------------------------------------------------------------------------------------------------------------------------------
def _random_q(gen, H, S):
    """q in {0, 1}: at most 12 ones per row on dims 0 .. 119"""
    order = torch.rand(H, S, 120, generator=gen).argsort(dim=-1)[..., :X_MAX]
    n = torch.randint(0, X_MAX + 1, (H, S, 1), generator=gen)
    q = torch.zeros(H, S, D, dtype=torch.float64)
    q.scatter_(-1, order, (torch.arange(X_MAX) < n).double())
    return q


def _random_k(gen, H, S):
    k = torch.zeros(H, S, D, dtype=torch.float64)
    k[..., :120] = (torch.rand(H, S, 120, generator=gen) < 0.5).double() * 8
    return k


def _random_v(gen, H, S):
    return torch.randint(-7, 8, (H, S, D), generator=gen).double() * 64


def _carriers(gen, q, k, v):
    """one element per head that fixes amax: q 5 on dim 127, k 56 on dim 126 (the other tensor is 0 there: x does not move), v 448"""
    for t, dim, val, mul in ((q, 127, 5.0, (1, 4, 1, 2)), (k, 126, 56.0, (1, 1, 2, 4)), (v, None, 448.0, (1, 1, 1, 1))):
        for h in range(t.shape[0]):
            r = int(torch.randint(0, t.shape[1], (1,), generator=gen))
            d = dim if dim is not None else int(torch.randint(0, D, (1,), generator=gen))
            t[h, r, d] = val * mul[h % 4]      # (a larger carrier: the head's other elements sit lower in e4m3, and e moves)


def lossless_inputs(kind, S, Hq, Hkv=None, seed=0):
    """-> q [Hq, S, D], k, v [Hkv, S, D] float64 (q head i reads kv head i // (Hq / Hkv)), checked by check_lossless.
    kind "random": random supports, and a different power-of-two magnitude per head (x = q . k / 8 does not move: q * 2^-a, k * 2^a,
    v * 2^b), so every head has scales of its own.
    kind "structured" (Hq = Hkv = 4): head 0 x_j = min(12, j // 64) (rises tile by tile: exact path with alpha < 1 on many tiles),
    head 1 x_j = max(0, 12 - j // 64) (falls: fast path behind the first tile), head 2 q = 0 (aq = 0 branch: plain mean of the allowed v),
    head 3 v = 0 (av = 0 branch: exactly 0).
    kind "zero_q" (gathering body): random supports, q head 1 = 0."""
    Hkv = Hq if Hkv is None else Hkv
    gen = torch.Generator().manual_seed(seed)
    q, k, v = _random_q(gen, Hq, S), _random_k(gen, Hkv, S), _random_v(gen, Hkv, S)
    if kind == "structured":
        assert Hq == Hkv == 4
        tile = torch.arange(S) // KBN
        dims = torch.arange(D)
        for h, steps in ((0, tile.clamp(max=X_MAX)), (1, (X_MAX - tile).clamp(min=0))):
            q[h] = (dims < X_MAX).double()
            k[h] = (dims[None, :] < steps[:, None]).double() * 8
    _carriers(gen, q, k, v)
    if kind == "structured":
        q[2] = 0
        v[3] = 0
    elif kind == "zero_q":
        q[1] = 0
    else:
        assert kind == "random"
    group = Hq // Hkv
    for h in range(Hkv):
        a, b = (0, 2, -1, 1)[h % 4], (0, -3, 2, -6)[h % 4]
        q[h * group:(h + 1) * group] *= 2.0 ** -a
        k[h] *= 2.0 ** a
        v[h] *= 2.0 ** b
    check_lossless(q, k, v)
    return q, k, v


def exponent_args(q, k):
    """x = scale_log2 * q . k = q . k / 8, float64 [Hq, S, S]"""
    group = q.shape[0] // k.shape[0]
    return torch.matmul(q, k.repeat_interleave(group, dim=0).transpose(-1, -2)) / 8


def head_scales(q, k, v):
    """the pre-pass's per-head scales from the ideal arithmetic: dict of float64 [H] tensors aq, ak, av, sk, sv, e, sq (k, v per kv head
    expanded to the q heads)"""
    group = q.shape[0] // k.shape[0]
    aq = q.abs().amax(dim=(-2, -1))
    ak = k.abs().amax(dim=(-2, -1)).repeat_interleave(group)
    av = v.abs().amax(dim=(-2, -1)).repeat_interleave(group)
    one = torch.ones_like(aq)
    sk = torch.where(ak > 0, F8_MAX / ak.clamp(min=1e-300), one)
    sv = torch.where(av > 0, F8_MAX / av.clamp(min=1e-300), one)
    ideal = SCALE_LOG2 / sk
    lg = torch.log2((aq * ideal / F8_MAX).clamp(min=1e-300))
    e = torch.where(aq > 0, torch.ceil(lg), torch.zeros_like(lg)).clamp(-120, 120)
    return dict(aq=aq, ak=ak, av=av, sk=sk, sv=sv, e=e, sq=ideal * torch.exp2(-e), log2_arg=lg)


def check_lossless(q, k, v):
    """the conditions of the module docstring, asserted: a changed seed or generator cannot silently leave the exact regime"""
    for t in (q, k, v):
        for dt in (torch.bfloat16, torch.float16):
            assert torch.equal(t.to(dt).double(), t), f"not exact in {dt}"
    sc = head_scales(q, k, v)

    def mantissa(a):
        return torch.frexp(a)[0]

    assert (mantissa(sc["ak"]) == 0.875).all() and (mantissa(sc["av"][sc["av"] > 0]) == 0.875).all()      # 7 * 2^m
    assert (mantissa(sc["aq"][sc["aq"] > 0]) == 0.625).all()                                            # 5 * 2^m
    frac = sc["log2_arg"][sc["aq"] > 0] % 1.0
    assert ((frac > 0.25) & (frac < 0.75)).all()                       # an ulp of log2f cannot move the ceil
    group = q.shape[0] // k.shape[0]
    for t, s in ((q, sc["sq"]), (k, sc["sk"][::group]), (v, sc["sv"][::group])):
        y = t * s[:, None, None]
        assert torch.equal(e4m3_decode(e4m3_bytes(y)), y), "not exact in e4m3 after the head's scaling"
        for eps in (1 - 2.0 ** -18, 1 + 2.0 ** -18):                  # ... and a few ulp of error in the scale change no byte
            assert torch.equal(e4m3_bytes(y * eps), e4m3_bytes(y))
    aq_scaled = (sc["aq"] * sc["sq"])[sc["aq"] > 0]
    assert ((aq_scaled > 224) & (aq_scaled <= 448)).all()
    x = exponent_args(q, k)
    assert torch.equal(x, x.round()), "exponent arguments must be integers"
    assert x.min() >= 0 and x.max() <= X_MAX and X_MAX <= X_SPREAD       # any set of allowed keys has max - min <= 13


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref64(x, v, mask):
    """sum_j 2^x_ij v_j / sum_j 2^x_ij over the allowed keys in float64; x [H, Sq, Sk], v [Hkv, Sk, D], mask bool [Sq, Sk] or [H, Sq, Sk];
    rows without keys give 0"""
    group = x.shape[0] // v.shape[0]
    w = torch.exp2(x) * mask.double()
    l = w.sum(-1, keepdim=True)
    o = torch.matmul(w, v.repeat_interleave(group, dim=0)) / l.clamp(min=1e-300)
    return torch.where(l > 0, o, torch.zeros_like(o))


def placement_index(S, vid0, F, P):
    """logical (token-major) row -> physical row of a head with the fused placement (f8_phys_row)"""
    l = torch.arange(S)
    i = l - vid0
    inside = (i >= 0) & (i < F * P)
    return torch.where(inside, vid0 + (i % F) * P + i // F, l)


def place(t, flags, S, vid0, F, P):
    """[H, S, D] physical order -> logical order on the heads whose flag is set"""
    idx = placement_index(S, vid0, F, P)
    out = t.clone()
    for h, f in enumerate(flags):
        if f:
            out[h] = t[h, idx]
    return out


def unplace(t, flags, S, vid0, F, P):
    idx = placement_index(S, vid0, F, P)
    out = t.clone()
    for h, f in enumerate(flags):
        if f:
            out[h, idx] = t[h]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the band policy's host arithmetic (csrc/band_policy.h: band_row_regions, kv_schedule, wave_fast_interval, classify, row_intervals) for
# BandPolicy<T, 128, 8>: what attn_body_f8pp asks its policy
# ---------------------------------------------------------------------------------------------------------------------------------------
TILE_SKIP, TILE_PARTIAL, TILE_FULL = 0, 1, 2


def band_q_tiles(S, prm):
    """-> [(q0, q_end, [first key of every tile, in the order the kernel visits them])] of the launch"""
    real, band = prm["real_len"], prm["band"]
    assert 0 <= real <= S
    rf_lo, rf_hi, cf_lo, cf_hi = prm["rowfull_lo"], prm["rowfull_hi"], prm["colfull_lo"], prm["colfull_hi"]
    has_rf = rf_hi > rf_lo and rf_lo < real and band <= S
    a, b = (max(rf_lo, 0), min(rf_hi, real)) if has_rf else (0, 0)
    cuts = [0, a, b, real, S]
    out = []
    for i in range(4):
        for q0 in range(cuts[i], cuts[i + 1], BM):
            q_end = min(cuts[i + 1], q0 + BM)
            segs = []
            if q0 < real:
                qr1 = min(q_end, real)
                if q0 < rf_hi and qr1 > rf_lo:
                    segs.append((0, (real + KBN - 1) // KBN))
                else:
                    segs.append((max(0, q0 - band + 1) // KBN, (min(real, qr1 - 1 + band) + KBN - 1) // KBN))
                    ch = min(cf_hi, real)
                    if ch > cf_lo:
                        segs.append((cf_lo // KBN, (ch + KBN - 1) // KBN))
            if q_end > real:
                segs.append((real // KBN, (S + KBN - 1) // KBN))
            segs.sort()
            merged = []
            for lo, hi in segs:                    # sorted, merged where one starts inside or directly behind the previous one
                if merged and lo <= merged[-1][1]:
                    merged[-1] = (merged[-1][0], max(merged[-1][1], hi))
                else:
                    merged.append((lo, hi))
            out.append((q0, q_end, [t * KBN for lo, hi in merged for t in range(lo, hi)]))
    return out


def _fast_interval(S, prm, q0, q_end, wave):
    real, band = prm["real_len"], prm["band"]
    w0 = q0 + 32 * wave
    w1 = min(w0 + 32, q_end)
    lo, hi = 1, 0
    if w0 < q_end and w1 <= real:
        full_rows = w0 >= prm["rowfull_lo"] and w1 <= prm["rowfull_hi"]
        lo = 0 if full_rows else max(w1 - band, 0)
        hi = min(real if full_rows else w0 + band - KBN, min(real, S) - KBN)
    return lo, hi


def _classify(S, prm, q0, q_end, k0, wave):
    real, band = prm["real_len"], prm["band"]
    rf_lo, rf_hi, cf_lo, cf_hi = prm["rowfull_lo"], prm["rowfull_hi"], prm["colfull_lo"], prm["colfull_hi"]
    lo, hi = _fast_interval(S, prm, q0, q_end, wave)
    if lo <= k0 <= hi:
        return TILE_FULL
    w0 = q0 + 32 * wave
    if w0 >= q_end:
        return TILE_SKIP
    w1, k1 = min(w0 + 32, q_end), min(k0 + KBN, S)
    every = False
    if k0 + KBN <= S:
        if w1 <= real and k1 <= real:
            every = ((k1 - 1 - w0 < band) and (w1 - 1 - k0 < band)) or (k0 >= cf_lo and k1 <= cf_hi) or (w0 >= rf_lo and w1 <= rf_hi)
        elif w0 >= real and k0 >= real:
            every = True
    if every:
        return TILE_FULL
    some = False
    if w0 < real and k0 < real:
        w1r, k1r = min(w1, real), min(k1, real)
        some = ((k0 - (w1r - 1) < band) and (w0 - (k1r - 1) < band)) or (k0 < cf_hi and k1r > cf_lo) or (w0 < rf_hi and w1r > rf_lo)
    if w1 > real and k1 > real:
        some = True
    return TILE_PARTIAL if some else TILE_SKIP


def row_intervals(S, prm, rows):
    """rows: int64 tensor of logical rows (may lie behind S) -> a0, alen, b0, blen (int64 tensors; lengths >= 0)"""
    real, band = prm["real_len"], prm["band"]
    rq = rows < real
    rowf = (rows >= prm["rowfull_lo"]) & (rows < prm["rowfull_hi"])
    band_lo, band_hi = (rows - band + 1).clamp(min=0), (rows + band).clamp(max=real)
    zero = torch.zeros_like(rows)
    lo = torch.where(rq, torch.where(rowf, zero, band_lo), zero + real)
    hi = torch.where(rq, torch.where(rowf, zero + real, band_hi), zero + S)
    ch = min(prm["colfull_hi"], real)
    blen = torch.where(rq & ~rowf, zero + max(ch - prm["colfull_lo"], 0), zero)
    return lo, (hi - lo).clamp(min=0), zero + prm["colfull_lo"], blen


def interval_mask(S, prm):
    """the element mask the kernel's per-row intervals describe, bool [S, S] — equal to oracle.svg_oracle.band_mask (asserted in the CPU
    tests)"""
    a0, alen, b0, blen = row_intervals(S, prm, torch.arange(S))
    k = torch.arange(S)[None, :]
    return ((k >= a0[:, None]) & (k < (a0 + alen)[:, None])) | ((k >= b0[:, None]) & (k < (b0 + blen)[:, None]))


# slot order of a lane half g: accumulator register e (0 .. 31: key block b = e >> 4, register r = e & 15) holds key
# 32 b + (r & 3) + 8 (r >> 2) + 4 g of the tile — the same order as byte position 16 b + 4 j + i of the V^T image with r = 4 j + i
def slot_keys():
    e = torch.arange(32)
    b, r = e >> 4, e & 15
    return torch.stack([32 * b + (r & 3) + 8 * (r >> 2) + 4 * g for g in range(2)])   # [2, 32]


MUTATIONS = ("mask_edge", "alpha", "drop_from_l")


def emulate_f8pp(x, v, S, prm, mutate=None):
    """attn_body_f8pp's sequence of fp32 operations in torch, on exponent arguments x [H, S, S] (float64, logical order) and v [H, S, D]:
    256-row q-tiles of 8 waves x 32 rows, the key tiles of band_q_tiles, lane halves g that own keys 32 b + 8 j + 4 g + i, probabilities
    2^(x - m_ref + 4) in e4m3 without a running maximum, the per-wave test psum <= 448 (off until every row of the wave has a finite
    reference), the exact path (row maximum, new reference, O and l rescaled by alpha, probabilities recomputed with delta), l summed over
    the two halves at the end, out = acc * (inv_v / l).  Lanes without a row (behind q_end) compute on q row 0 with the intervals of their
    own row number, as the kernel does: they take part in the wave's votes.
    The MFMA sums are formed in float64 and rounded to fp32 per tile (the hardware's summation order is not documented); on the lossless
    inputs every one of them must be exact, which is asserted here tile by tile.
    -> float32 [H, S, D]: the value in front of the conversion to the output type.
    mutate (the CPU tests show that each changes the result): "mask_edge" (m_alen one too short), "alpha" (O and l rescaled by 2 alpha),
    "drop_from_l" (the probability of register 5 of lane half 0 never enters l)."""
    assert mutate is None or mutate in MUTATIONS
    H = x.shape[0]
    f32 = torch.float32
    av = v.abs().amax(dim=(-2, -1))
    sv = torch.where(av > 0, F8_MAX / av.clamp(min=1e-300), torch.ones_like(av))
    v8 = v * sv[:, None, None]
    assert torch.equal(e4m3_decode(e4m3_bytes(v8)), v8)
    inv_v = (1.0 / sv).to(f32)
    S_pad = (S + KBN - 1) // KBN * KBN
    xp = torch.zeros(H, S, S_pad, dtype=torch.float64)      # pad keys: k8 rows of zeros
    xp[:, :, :S] = x
    vp = torch.zeros(H, S_pad, D, dtype=torch.float64)
    vp[:, :S] = v8
    keys = slot_keys()                                      # [2, 32]
    out = torch.zeros(H, S, D, dtype=f32)
    neg_inf = torch.tensor(float("-inf"), dtype=f32)

    for q0, q_end, tiles in band_q_tiles(S, prm):
        rows = q0 + torch.arange(BM)
        exists = rows < q_end
        src = torch.where(exists, rows, torch.zeros_like(rows))
        xq = xp[:, src].view(H, 8, 32, S_pad)                                  # [H, wave, row, key]
        a0, alen, b0, blen = (t.view(8, 32, 1, 1) for t in row_intervals(S, prm, rows))
        if mutate == "mask_edge":
            alen = (alen - 1).clamp(min=0)
        l_run = torch.zeros(H, 8, 32, 2, dtype=f32)
        acc = torch.zeros(H, 8, 32, D, dtype=f32)
        m_ref = torch.full((H, 8, 32), float("-inf"), dtype=f32)
        m_off = torch.full((H, 8, 32), -P_SHIFT, dtype=f32)
        thr = torch.full((H, 8), -1.0, dtype=f32)

        def probs(arg):                                     # -> p (fp32), psum in the kernel's order, p as e4m3 values
            p = torch.exp2(arg)
            psum = torch.zeros(arg.shape[:-1], dtype=f32)
            for e in range(32):
                if mutate == "drop_from_l" and e == 5:
                    psum[..., 1] = psum[..., 1] + p[..., 1, e]
                    continue
                psum = psum + p[..., e]
            return psum, p.to(torch.float8_e4m3fn).to(f32)

        for k0 in tiles:
            kk = k0 + keys                                                      # [2, 32]
            sc = (xq[..., kk] - m_off[..., None, None].double()).to(f32)        # [H, 8, 32, 2, 32]: x - m_off, an exact integer sum
            assert torch.equal(sc.double(), xq[..., kk] - m_off[..., None, None].double())
            ok = ((kk >= a0) & (kk < a0 + alen)) | ((kk >= b0) & (kk < b0 + blen))          # [8, 32, 2, 32]
            cls = torch.tensor([_classify(S, prm, q0, q_end, k0, w) for w in range(8)]).view(8, 1, 1, 1)
            ok = (cls == TILE_FULL) | ((cls == TILE_PARTIAL) & ok)
            sc = torch.where(ok, sc, neg_inf)
            psum, p8 = probs(sc)
            exact = (~(psum <= thr[..., None, None])).flatten(2).any(-1)                   # [H, 8]: the wave's vote
            mx = sc.flatten(3).amax(-1)                                                    # [H, 8, 32]: both lane halves
            m_prev = m_off + P_SHIFT
            m_new = torch.maximum(m_ref, mx + m_off)
            m_use = torch.where(torch.isinf(m_new), m_prev, m_new)
            delta = m_prev - m_use
            alpha = torch.exp2(delta.clamp(max=126.0))
            if mutate == "alpha":
                alpha = alpha * 2
            psum_x, p8_x = probs(sc + delta[..., None, None])
            ex3 = exact[..., None]
            m_ref = torch.where(ex3, m_new, m_ref)
            thr = torch.where(exact, torch.where(torch.isinf(m_new).any(-1), -1.0, F8_MAX).to(f32), thr)
            m_off = torch.where(ex3, m_use - P_SHIFT, m_off)
            l_run = torch.where(ex3[..., None], l_run * alpha[..., None], l_run)
            acc = torch.where(ex3[..., None], acc * alpha[..., None], acc)
            psum = torch.where(ex3[..., None], psum_x, psum)
            p8 = torch.where(ex3[..., None, None], p8_x, p8)
            assert not torch.isnan(p8).any() and not torch.isinf(p8).any()
            l64 = l_run.double() + psum.double()
            l_run = l_run + psum
            pv = torch.einsum("hwrgs,hgsd->hwrd", p8.double(), vp[:, kk])          # V^T P^T of the tile: 64 products per (row, d)
            a64 = acc.double() + pv
            acc = a64.to(f32)
            if mutate is None:      # the lossless regime: nothing above was rounded
                assert torch.equal(l_run.double(), l64) and torch.equal(acc.double(), a64), "a partial sum is not exact in fp32"
        l_tot = l_run[..., 0] + l_run[..., 1]
        inv = torch.where(l_tot > 0, inv_v[:, None, None] / l_tot.clamp(min=1e-30), torch.zeros_like(l_tot))
        o = (acc * inv[..., None]).view(H, BM, D)
        out[:, q0:q_end] = o[:, : q_end - q0]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# the pre-pass
# ---------------------------------------------------------------------------------------------------------------------------------------
def vt_slot_keys():
    """key (inside its 64-key tile) of byte position 0 .. 63 of a V^T row: position 32 g + 16 b + 4 j + i <-> key 32 b + 8 j + 4 g + i"""
    pos = torch.arange(64)
    g, b, j, i = pos >> 5, (pos >> 4) & 1, (pos >> 2) & 3, pos & 3
    return 32 * b + 8 * j + 4 * g + i


def workspace_offsets(BH, S):
    S_pad = (S + KBN - 1) // KBN * KBN
    img = BH * S_pad * D
    return dict(S_pad=S_pad, q8=0, k8=img, vt8=2 * img, amax=3 * img, scales=3 * img + 12 * BH, end=3 * img + 28 * BH, total=3 * img + 28 * BH + 256)


def prepass_reference(q, k, v, S, flags=None, vid0=0, F=1, P=1, sm_scale=SM_SCALE, scale_log2=None):
    """The workspace images of svg_band_attention_fp8_stage(stage = 1) from torch.  q, k, v: [BH, S, D] of any float dtype (PHYSICAL row
    order; heads with flags[h] set are gathered through the placement).  The products x * s are formed in float64 with the ideal scales.
    -> dict: q8, k8 uint8 [BH, S_pad, D]; vt8 uint8 [BH, S_pad / 64, D, 64]; prod_q, prod_k, prod_vt: the float64 products in the same
    layouts (what the bytes are the rounding of); amax float32 [BH, 3]; e int64 [BH]; scales float64 [BH, 2]: 2^e, 1 / sv; sq, sk, sv."""
    BH = q.shape[0]
    assert q.shape == k.shape == v.shape == (BH, S, D)
    qd, kd, vd = q.double(), k.double(), v.double()
    amax = torch.stack([t.abs().amax(dim=(-2, -1)) for t in (qd, kd, vd)], dim=1)                # exact: the inputs are 16-bit numbers
    aq, ak, av = amax.unbind(1)
    one = torch.ones_like(ak)
    sk = torch.where(ak > 0, F8_MAX / ak.clamp(min=1e-300), one)
    sv = torch.where(av > 0, F8_MAX / av.clamp(min=1e-300), one)
    if scale_log2 is None:      # as the entry point forms it; the lossless cases pass their exact 1 / 8
        scale_log2 = float(torch.tensor(sm_scale, dtype=torch.float32)) * 1.4426950408889634
    ideal = scale_log2 / sk
    e = torch.where(aq > 0, torch.ceil(torch.log2((aq * ideal / F8_MAX).clamp(min=1e-300))), torch.zeros_like(aq)).clamp(-120, 120)
    sq = ideal * torch.exp2(-e)
    if flags is not None:
        qd, kd, vd = (place(t, flags, S, vid0, F, P) for t in (qd, kd, vd))
    S_pad = (S + KBN - 1) // KBN * KBN

    def padded(t, s):
        out = torch.zeros(BH, S_pad, D, dtype=torch.float64)
        out[:, :S] = t * s[:, None, None]
        return out

    prod_q, prod_k, pv = padded(qd, sq), padded(kd, sk), padded(vd, sv)
    prod_vt = pv.view(BH, S_pad // KBN, KBN, D)[:, :, vt_slot_keys()].transpose(-1, -2).contiguous()       # [BH, tile, d, position]
    return dict(q8=e4m3_bytes(prod_q), k8=e4m3_bytes(prod_k), vt8=e4m3_bytes(prod_vt), prod_q=prod_q, prod_k=prod_k, prod_vt=prod_vt,
                amax=amax.float(), e=e.long(), scales=torch.stack([torch.exp2(e), 1.0 / sv], dim=1), sq=sq, sk=sk, sv=sv)


def prepass_dequantise(ref, S, flags=None, vid0=0, F=1, P=1):
    """the images of prepass_reference back to q, k, v in PHYSICAL row order, float64 (the round trip of the CPU tests)"""
    BH = ref["q8"].shape[0]
    qd = e4m3_decode(ref["q8"])[:, :S] / ref["sq"][:, None, None]
    kd = e4m3_decode(ref["k8"])[:, :S] / ref["sk"][:, None, None]
    vt = e4m3_decode(ref["vt8"])                                        # [BH, tile, d, position]
    vl = torch.empty_like(vt)
    vl[..., vt_slot_keys()] = vt                                        # position -> key
    vd = vl.transpose(-1, -2).reshape(BH, -1, D)[:, :S] / ref["sv"][:, None, None]
    if flags is not None:
        qd, kd, vd = (unplace(t, flags, S, vid0, F, P) for t in (qd, kd, vd))
    return qd, kd, vd


def near_midpoint(prod, rel=2.0 ** -18):
    """elements whose product lies within relative `rel` of the midpoint of two adjacent e4m3 values: the only places where a scale that
    is a few fp32 ulp off (the pre-pass is built with -ffast-math) may round to the other neighbour"""
    lo, hi, mid = e4m3_neighbours(prod)
    return (lo != hi) & ((prod.abs().clamp(max=F8_MAX) - mid).abs() <= rel * mid)


PREPASS_SEEDS = (31, 32)       # randn inputs of the pre-pass tests: tests/test_fp8_exact_cases_cpu.py shows that at most 1 % of their
                               # elements lie near a rounding midpoint


def random_prepass_inputs(seed, dtype):
    """randn q, k, v [4, 613, D] in dtype, with heads of different magnitude and one head with an outlier"""
    gen = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(BAND_BH, BAND_S, D, generator=gen) for _ in range(3))
    q[1] *= 5.0
    k[1] *= 0.2
    v[2] *= 50.0
    v[3, 77, 5] = 30.0
    return q.to(dtype), k.to(dtype), v.to(dtype)


def parse_workspace(ws, BH, S):
    """uint8 CPU tensor of the workspace -> dict of views: q8, k8 [BH, S_pad, D], vt8 [BH, S_pad / 64, D, 64], amax_bits int32 [BH, 3],
    scales float32 [BH, 4], scale_bits int32 [BH, 4], tail uint8 (never written)"""
    o = workspace_offsets(BH, S)
    S_pad = o["S_pad"]
    img = BH * S_pad * D
    return dict(q8=ws[o["q8"]:o["q8"] + img].view(BH, S_pad, D), k8=ws[o["k8"]:o["k8"] + img].view(BH, S_pad, D),
                vt8=ws[o["vt8"]:o["vt8"] + img].view(BH, S_pad // KBN, D, KBN),
                amax_bits=ws[o["amax"]:o["scales"]].view(torch.int32).view(BH, 3),
                scales=ws[o["scales"]:o["end"]].view(torch.float32).view(BH, 4),
                scale_bits=ws[o["scales"]:o["end"]].view(torch.int32).view(BH, 4), tail=ws[o["end"]:])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the cases of the GPU tests (shapes and masks), shared with the CPU tests that prove the reference meets the bound on them
# ---------------------------------------------------------------------------------------------------------------------------------------
BAND_S, BAND_BH = 613, 4        # 3 q-tiles of 256 (the last with idle waves), 10 key tiles (the 4 LDS stages wrap), S_pad = 640
PLACE = dict(flags=(0, 1, 1, 0), vid0=0, F=4, P=150)       # the rest (13 rows) is context


def _m(real_len, band, cf=(0, 0), rf=(0, 0)):
    return dict(real_len=real_len, band=band, colfull_lo=cf[0], colfull_hi=cf[1], rowfull_lo=rf[0], rowfull_hi=rf[1])


BAND_MASKS = {
    "dense": _m(BAND_S, BAND_S + 1),
    "band70": _m(BAND_S, 70),                                        # first tiles of a q-tile fully masked for some of its waves
    "real_len": _m(590, 200),                                        # rows behind real_len see the keys behind it
    "full_ranges": _m(BAND_S, 70, cf=(120, 135), rf=(250, 262)),     # straddle key 128 (key tile) and row 256 (q-tile)
    "placement": _m(BAND_S, 70, cf=(600, BAND_S), rf=(600, BAND_S)),  # with PLACE: video rows banded, context rows / columns full
}
BAND_INPUTS = ("random", "structured")


@functools.lru_cache(maxsize=None)
def band_case(inputs, mask_name):
    """-> dict: q, k, v float64 [4, 613, D] (physical order), prm, place (dict or None), mask bool [S, S], x (logical order), ref float64
    [4, 613, D] (physical order).  Computed once per process; callers must not modify it."""
    q, k, v = lossless_inputs(inputs, BAND_S, BAND_BH, seed=11 if inputs == "random" else 12)
    prm = BAND_MASKS[mask_name]
    pl = PLACE if mask_name == "placement" else None
    ql, kl, vl = (place(t, pl["flags"], BAND_S, pl["vid0"], pl["F"], pl["P"]) for t in (q, k, v)) if pl else (q, k, v)
    x = exponent_args(ql, kl)
    mask = interval_mask(BAND_S, prm)
    ref = ref64(x, vl, mask)
    if pl:
        ref = unplace(ref, pl["flags"], BAND_S, pl["vid0"], pl["F"], pl["P"])
    return dict(q=q, k=k, v=v, prm=prm, place=pl, mask=mask, x=x, v_logical=vl, ref=ref)


VB = dict(Hq=4, Hkv=2, S=357, MB=5, NB=9)
VB_Q_SIZES = ((100, 1, 77, 120, 59), (1, 130, 64, 65, 97))                                 # ragged, a 1-row block each
VB_K_SIZES = ((40, 3, 64, 65, 1, 30, 90, 50, 14), (64, 64, 1, 29, 70, 5, 60, 33, 31))


@functools.lru_cache(maxsize=None)
def varblock_case(permuted):
    """-> dict: q [4, 357, D], k, v [2, 357, D] float64, q_sizes, k_sizes int32, block_map bool [2, 5, 9] (block-row 2 of head 0 and
    block-row 0 of head 1 have no active key block), q_idx / k_idx int32 or None, element masks em [2, S, S] (in block order), ref float64
    [4, 357, D] in the caller's row order"""
    Hq, Hkv, S, MB, NB = (VB[n] for n in ("Hq", "Hkv", "S", "MB", "NB"))
    gen = torch.Generator().manual_seed(21)
    q, k, v = lossless_inputs("zero_q", S, Hq, Hkv, seed=22)
    q_sizes, k_sizes = torch.tensor(VB_Q_SIZES, dtype=torch.int32), torch.tensor(VB_K_SIZES, dtype=torch.int32)
    assert (q_sizes.sum(1) == S).all() and (k_sizes.sum(1) == S).all() and q_sizes.shape == (Hkv, MB) and k_sizes.shape == (Hkv, NB)
    bmap = torch.rand(Hkv, MB, NB, generator=gen) < 0.5
    bmap[0, 2] = False
    bmap[1, 0] = False
    bmap[0, 1, 4] = True                # the 1-row block reads the 1-key block
    q_idx = k_idx = None
    qb, kb, vb = q, k, v                # tensors in block order
    if permuted:
        q_idx = torch.stack([torch.randperm(S, generator=gen) for _ in range(Hq)]).to(torch.int32)
        k_idx = torch.stack([torch.randperm(S, generator=gen) for _ in range(Hkv)]).to(torch.int32)
        qb = torch.stack([q[h, q_idx[h].long()] for h in range(Hq)])
        kb = torch.stack([k[h, k_idx[h].long()] for h in range(Hkv)])
        vb = torch.stack([v[h, k_idx[h].long()] for h in range(Hkv)])
    from oracle import svg_oracle as O

    em = torch.stack([O.block_mask_to_element_mask(bmap[h], q_sizes[h], k_sizes[h]) for h in range(Hkv)])
    ref = ref64(exponent_args(qb, kb), vb, em.repeat_interleave(Hq // Hkv, dim=0))
    if permuted:
        out = torch.empty_like(ref)
        for h in range(Hq):
            out[h, q_idx[h].long()] = ref[h]
        ref = out
    return dict(q=q, k=k, v=v, q_sizes=q_sizes, k_sizes=k_sizes, block_map=bmap, q_idx=q_idx, k_idx=k_idx, em=em, ref=ref)


def assert_exact_or_adjacent(out, ref, dtype, what):
    """the bound of the exact tests: every element of `out` (16-bit, CPU) is dtype(ref) — ref float64 rounded ONCE — or a value adjacent
    to it in dtype (the kernels' final acc * (inv_v / l) is inexact by a few fp32 ulp, and exact ties are structurally common for these
    rationals); elements whose reference is 0 are exactly 0.  Prints the bit-equal share and returns it."""
    assert out.dtype == dtype and out.shape == ref.shape
    want = round_once(ref, dtype)
    dist = (ordered(out) - ordered(want)).abs()
    finite = torch.isfinite(out.float())
    assert finite.all(), f"{what}: {int((~finite).sum())} non-finite elements"
    zero = ref == 0
    bad_zero = zero & (out.float() != 0)
    assert not bad_zero.any(), f"{what}: {int(bad_zero.sum())} elements whose reference is exactly 0 are not 0 (first {bad_zero.nonzero()[0].tolist()})"
    bad = dist > 1
    share = float((dist == 0).double().mean())
    print(f"[fp8 exact] {what}: {100 * share:.3f} % bit-equal to {dtype}(ref64), {int((dist == 1).sum())} of {out.numel()} adjacent, {int(bad.sum())} further")
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {out.numel()} elements are neither {dtype}(ref64) nor adjacent to it; rows "
                             f"{sorted(set(bad.nonzero()[:, -2].tolist()))[:12]} ...; first at {i}: got {float(out[tuple(i)])}, "
                             f"reference {float(ref[tuple(i)])}, largest distance {int(dist.max())} units")
    return share
