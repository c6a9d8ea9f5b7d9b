"""Band (SVG1) attention on ROW shards — shards of any contiguous range of the video's rows, which cut through frames
(include/svg_attn_band_row_shard.h): the binding of the three entries from a table of its own, the coordinate maps on the host, the closed
form of "does this pair of shards hold an allowed element" for the exchange plan, and the allocating wrapper band_row_shard_attention.  What
svg.distributed runs under enable_frame_shards(balance="rows").  Outputs come from _native.empty / _layout_plan like every allocation of
the package."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native
from ._native import _F32, _I32, _VP, AttnLayout, BandMask, PermDesc


class BandRowShard(C.Structure):
    """svg_band_row_shard_t: the video rows [row0, row0 + n_rows) counted from vid0, frame-major, and behind them the sequence rows
    [tail_begin, tail_begin + n_tail) behind the video"""

    _fields_ = [("row0", C.c_int32), ("n_rows", C.c_int32), ("tail_begin", C.c_int32), ("n_tail", C.c_int32)]

    def as_tuple(self):
        return (self.row0, self.n_rows, self.tail_begin, self.n_tail)


BAND_ROW_SHARD_ENTRIES = {
    "svg_band_row_shard_attention_lse": (C.c_int, [_VP, _VP, _VP, _VP, _VP, _I32, _I32, _I32, _I32, _F32, C.POINTER(BandMask),
                                                   C.POINTER(PermDesc), C.POINTER(BandRowShard), C.POINTER(BandRowShard),
                                                   C.POINTER(AttnLayout), _VP]),
    "svg_debug_band_row_shard_map": (_I32, [C.POINTER(PermDesc), _I32, C.POINTER(BandRowShard), _I32, _VP, _I32, _VP, _VP, _VP]),
}
BAND_ROW_SHARD_ENTRIES["svg_band_row_shard_attention_lse_f32"] = BAND_ROW_SHARD_ENTRIES["svg_band_row_shard_attention_lse"]


def load():
    """_native.load() with the entries of this module typed (once per library object)"""
    lib = _native.load()
    if isinstance(lib, C.CDLL) and not getattr(lib, "_band_row_shard_bound", False):
        for name, (res, args) in BAND_ROW_SHARD_ENTRIES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        lib._band_row_shard_bound = True
    return lib


def _shard(s) -> BandRowShard:
    return s if isinstance(s, BandRowShard) else BandRowShard(*[int(x) for x in s])


def _check_shard(what: str, s: BandRowShard, S: int, vid0: int, F: int, P: int) -> None:
    if s.row0 < 0 or s.n_rows < 0 or s.row0 + s.n_rows > F * P or s.n_tail < 0:
        raise ValueError(f"{what}: rows [{s.row0}, {s.row0 + s.n_rows}) / a tail of {s.n_tail} rows outside a video of {F * P} rows")
    if s.n_tail > 0 and (s.tail_begin < vid0 + F * P or s.tail_begin + s.n_tail > S):
        raise ValueError(f"{what}: tail [{s.tail_begin}, {s.tail_begin + s.n_tail}) outside [{vid0 + F * P}, {S}) (the rows behind the video)")
    if s.n_rows == 0 and s.n_tail == 0:
        raise ValueError(f"{what}: an empty shard")


def band_row_shard_rows(shard) -> int:
    """rows a shard holds: n_rows + n_tail"""
    s = _shard(shard)
    return s.n_rows + s.n_tail


def band_row_shard_pieces(shard, frame_size: int):
    """The pieces of a token-major head's order over the shard's video rows, those that hold rows: [(p_lo, p_hi, c, fs, L)] — the positions
    [p_lo, p_hi) own the c frames [fs, fs + c) each and come at the shard indices L + (p - p_lo) * c + (f - fs).  At most three."""
    s, P = _shard(shard), int(frame_size)
    if s.n_rows == 0:
        return []
    e = s.row0 + s.n_rows
    a, fa, fb = s.row0 % P, s.row0 // P, (e - 1) // P
    b, n = e - fb * P, fb - fa + 1
    out, L = [], 0
    for lo, hi in ((0, min(a, b)), (min(a, b), max(a, b)), (max(a, b), P)):
        c, fs = n - (lo < a) - (lo >= b), fa + (lo < a)
        if hi > lo and c > 0:
            out.append((lo, hi, c, fs, L))
            L += (hi - lo) * c
    assert L == s.n_rows
    return out


def _tail_begin(s: BandRowShard, vid0: int, F: int, P: int) -> int:
    return s.tail_begin if s.n_tail > 0 else vid0 + F * P


def band_row_shard_coord(perm, shard, token_major: bool, l: int) -> int:
    """g(l): the mask coordinate of index l of a row shard in the order of a head in logical order (the shard's rows as stored) or of a
    token-major head (the shard's (frame, position) pairs by position, then frame), see include/svg_attn_band_row_shard.h"""
    vid0, F, P = _native._video(perm)
    s = _shard(shard)
    if l >= s.n_rows:
        return _tail_begin(s, vid0, F, P) + (l - s.n_rows)
    if not token_major:
        return vid0 + s.row0 + l
    lo, hi, c, fs, L = [pc for pc in band_row_shard_pieces(s, P) if pc[4] <= l][-1]
    return vid0 + (lo + (l - L) // c) * F + fs + (l - L) % c


def band_row_shard_coord_inv(perm, shard, token_major: bool, x: int) -> int:
    """ginv(x): the smallest index l of the shard with g(l) >= x, the shard's row count where there is none"""
    vid0, F, P = _native._video(perm)
    s = _shard(shard)
    y = max(x - vid0, 0)
    if token_major:
        p, r = y // F, y % F
        lv = s.n_rows
        for lo, hi, c, fs, L in reversed(band_row_shard_pieces(s, P)):   # the first index of a position at or behind p
            if p < hi:
                lv = L + (p - lo) * c + min(max(r - fs, 0), c) if p >= lo else L
    else:
        lv = max(y - s.row0, 0)
    if lv < s.n_rows:
        return lv
    return s.n_rows + min(max(x - _tail_begin(s, vid0, F, P), 0), s.n_tail)


def band_row_shard_has_keys(mask: BandMask, num_tokens: int, perm, q_shard, k_shard, token_major: bool) -> bool:
    """_native.band_shard_has_keys for row shards: does the band mask over num_tokens rows allow ANY pair (row of q_shard, key of k_shard)
    for a head of this kind?  Host only, closed form on the intervals and pieces of the two maps.  Exact, except under a mask whose
    real_len lies INSIDE the video (no SVG1 mask), where two token-major parts are judged on their hulls — True where in doubt, so a plan
    never drops a pair that holds an element."""
    vid0, F, P = _native._video(perm)
    S = int(num_tokens)
    real, band, cf_lo, cf_hi, rf_lo, rf_hi = mask.as_tuple()
    real = min(max(real, 0), S)
    qs, ks = _shard(q_shard), _shard(k_shard)
    kind = bool(token_major)

    def inv(s, x):
        return band_row_shard_coord_inv((vid0, F, P), s, kind, x)

    def coord(s, l):
        return band_row_shard_coord((vid0, F, P), s, kind, l)

    def count(s, a, b, lo=0, hi=None):   # indices in [lo, hi) whose coordinate lies in [a, b)
        if b <= a:
            return 0
        hi = band_row_shard_rows(s) if hi is None else hi
        return max(0, min(hi, inv(s, b)) - max(lo, inv(s, a)))

    if count(qs, real, S) > 0 and count(ks, real, S) > 0:          # rows behind real_len see the keys behind real_len
        return True
    nq, nk = inv(qs, real), inv(ks, real)                           # the real rows / keys: indices [0, nq) / [0, nk)
    if nq == 0 or nk == 0:
        return False
    if count(qs, max(rf_lo, 0), min(rf_hi, real)) > 0 or count(ks, max(cf_lo, 0), min(cf_hi, real)) > 0:   # a full row / a full column
        return True
    if band <= 0:
        return False

    def parts(s, n):
        """(first index, end index, is an interval of coordinates, piece) of the parts of the indices [0, n): the video rows of a head in
        logical order, each piece of a token-major head, the tail"""
        out = []
        if kind:
            for pc in band_row_shard_pieces(s, P):
                lo, hi, c, fs, L = pc
                if L < n:
                    out.append((L, min(n, L + (hi - lo) * c), c == F, pc))   # (all frames: the coordinates are consecutive)
        elif min(n, s.n_rows) > 0:
            out.append((0, min(n, s.n_rows), True, None))
        if n > s.n_rows:
            out.append((s.n_rows, n, True, None))
        return out

    for qa, qb, q_iv, qp in parts(qs, nq):
        for ka, kb, k_iv, kp in parts(ks, nk):
            if q_iv:      # an interval of rows [x, y]: a key within the band of it
                x, y = coord(qs, qa), coord(qs, qb - 1)
                if count(ks, x - band + 1, y + band, ka, kb) > 0:
                    return True
            elif k_iv:
                x, y = coord(ks, ka), coord(ks, kb - 1)
                if count(qs, x - band + 1, y + band, qa, qb) > 0:
                    return True
            elif qb < qp[4] + (qp[1] - qp[0]) * qp[2] or kb < kp[4] + (kp[1] - kp[0]) * kp[2]:   # real_len inside the video: the hulls
                if coord(ks, ka) - coord(qs, qb - 1) < band and coord(qs, qa) - coord(ks, kb - 1) < band:
                    return True
            else:
                # two whole pieces: row - key = m * F + d with the position distance m in [m0, m1] and the frame distance d in [d_lo, d_hi]
                d_lo, d_hi = qp[3] - (kp[3] + kp[2] - 1), qp[3] + qp[2] - 1 - kp[3]
                m_lo, m_hi = (-band - d_hi) // F + 1, -((d_lo - band) // F) - 1     # m * F + d_hi > -band, m * F + d_lo < band
                if max(m_lo, qp[0] - (kp[1] - 1)) <= min(m_hi, qp[1] - 1 - kp[0]):
                    return True
    return False


def band_row_shard_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask: BandMask, perm, q_shard, k_shard,
                             out_dtype: Optional[torch.dtype] = None, *, flags: Optional[torch.Tensor] = None,
                             out: Optional[torch.Tensor] = None):
    """Band attention of a ROW SHARD of the rows over a ROW SHARD of the keys (svg_band_row_shard_attention_lse[_f32]) -> (o, lse):
    _native.band_shard_attention for shards that cut through frames.  q [cfg, H, Sq, D] (or [BH, Sq, D]) holds the rows of q_shard, k / v
    those of k_shard — BandRowShard or (row0, n_rows, tail_begin, n_tail): the video rows [row0, row0 + n_rows) as the model stores them
    (frame-major) and the shard's tail behind them — of the sequence perm = (num_tokens, vid0, num_frame, frame_size) describes.  flags
    (int64 / bool [BH] on the GPU, or None: every head in logical order) marks the token-major heads, both kinds in ONE launch.  o has q's
    shape and dtype, lse is contiguous fp32 of shape q.shape[:-1] (a row that sees no key of the shard: o = 0, lse = -inf) — parts for
    merge_attention_states.  out_dtype=torch.float32 (without out): (o32, lse), the rows before their rounding.  Layouts and copies:
    _native._layout_plan.  head_dim 128, bf16 / fp16, GPU tensors: anything else raises before anything runs — there is no fall-back."""
    who = "band_row_shard_attention"
    if out_dtype not in (None, torch.float32):
        raise ValueError(f"{who}: out_dtype is None (q's dtype) or torch.float32, got {out_dtype}")
    f32 = out_dtype == torch.float32
    if f32 and out is not None:
        raise ValueError(f"{who}(out_dtype=torch.float32): fp32 rows are parts for merge_attention_states, without out")
    _native._gpu(q, k, v, out, flags)
    if not (q.dim() == k.dim() == v.dim() and q.dim() in (3, 4) and k.shape == v.shape and q.shape[:-2] == k.shape[:-2]
            and q.shape[-1] == k.shape[-1] and q.dtype == k.dtype == v.dtype):
        raise ValueError(f"{who}: q [.., Sq, D], k / v [.., Sk, D] of one dtype, got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}")
    Sq, Sk, D = q.shape[-2], k.shape[-2], q.shape[-1]
    if D != 128 or q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{who}: head_dim 128, bfloat16 / float16; got D = {D}, {q.dtype} (no shard form, no fall-back)")
    S, vid0, F, P = (int(x) for x in perm)
    if F <= 0 or P <= 0 or vid0 < 0 or vid0 + F * P > S:
        raise ValueError(f"{who}: a video of {F} frames of {P} rows from row {vid0} does not fit {S} rows")
    qs, ks = _shard(q_shard), _shard(k_shard)
    _check_shard(f"{who}: q shard", qs, S, vid0, F, P)
    _check_shard(f"{who}: k shard", ks, S, vid0, F, P)
    if Sq != band_row_shard_rows(qs) or Sk != band_row_shard_rows(ks):
        raise ValueError(f"{who}: q holds {Sq} rows, k {Sk}; the shards say {band_row_shard_rows(qs)} and {band_row_shard_rows(ks)}")
    if out is not None and (out.shape != q.shape or out.dtype != q.dtype):
        raise ValueError(f"{who}: out must have q's shape and dtype, got {tuple(out.shape)} {out.dtype}")
    BH = q.numel() // (Sq * D)
    flag = None
    if flags is not None:
        flag = flags.to(torch.int64).contiguous()
        if flag.numel() != BH:
            raise ValueError(f"{who}: {flag.numel()} flags for {BH} heads")
    load()
    lse = _native.empty(q.shape[:-1], dtype=torch.float32, device=q.device)
    pd = PermDesc(_native._ptr(flag), vid0, F, P)
    p = _native._layout_plan(q, k, v, o=_native._O32 if f32 else _native._O16, out=out)
    _native._call_lse("svg_band_row_shard_attention_lse", f32, p, lse, BH, S, D, _native._dtype_code(q), _native._sm_scale(None, D),
                      C.byref(mask), C.byref(pd), C.byref(qs), C.byref(ks))
    return p.result(), lse
