"""The online profiler on frame shards without a GPU (include/svg_attn_profile_shard.h: svg_sample_mse_shard_partial,
svg_sample_mse_from_parts and their workspace sizes; _native.sample_mse_shard_partial / sample_mse_from_parts / neutral_profile_part;
svg.distributed.sampled_row_owners / token_sharded_sample_mse / token_sharded_svg1_layer_call): the exports and prototypes, the argument
validation in the order the header states (every check runs on the host before any launch), what the wrappers refuse, and the two
schedules on gloo CPU ranks with float64 statements of the partial and the combine written here from oracle.svg_oracle.profile_masks.

ref: sample_mse, svg/models/hyvideo/attention.py:376-399 with the profiling masks of get_attention_mask, svg/models/hyvideo/utils.py:47-93
(wan/utils.py:63-110)."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

from gloo_ranks import run_ranks
from oracle import svg_oracle as O
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH = 0x10000                                          # placeholder device pointer (16-byte aligned; never dereferenced by a rejected call)
ROOT = Path(__file__).resolve().parent.parent
NAMES = ("svg_sample_mse_shard_workspace_bytes", "svg_sample_mse_shard_partial", "svg_sample_mse_from_parts_workspace_bytes",
         "svg_sample_mse_from_parts")


def _host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


# ---------------------------------------------------------------------------------------------------------
# exports and prototypes
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_entries():
    lib = nat.load()
    assert set(nat.PROFILE_SHARD_SIGNATURES) == set(NAMES)
    others = (set(nat.SIGNATURES) | set(nat.SPARSE_LSE_SIGNATURES) | set(nat.SPARSE_F32_SIGNATURES) | set(nat.BAND_LSE_FORM_SIGNATURES)
              | set(nat.BAND_WINDOW_SIGNATURES) | set(nat.BAND_SHARD_SIGNATURES))
    assert not set(NAMES) & others
    for name, (res, args) in nat.PROFILE_SHARD_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4
    assert lib.svg_strerror(WORKSPACE) and lib.svg_sample_mse_from_parts_workspace_bytes(0) == 0


def test_header_prototypes_match_the_ctypes_signatures():
    main = (ROOT / "include" / "svg_attn.h").read_text()
    assert main.rstrip().endswith('#include "svg_attn_profile_shard.h"\n#endif /* SVG_ATTN_H_ */')
    src = (ROOT / "include" / "svg_attn_profile_shard.h").read_text()
    for n in range(1, 11):                                     # the order of the checks is written down
        assert re.search(rf"^ \*\s+{n}\. ", src, flags=re.M), n
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
        res, args = nat.PROFILE_SHARD_SIGNATURES[name]
        assert hasattr(lib, name) and [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


def test_workspace_sizes():
    lib = nat.load()
    per_chunk = 3 * 2 * 64 * 132 * 4
    assert lib.svg_sample_mse_shard_workspace_bytes(2, 48, 128, 64) == per_chunk              # one tile: one chunk
    assert lib.svg_sample_mse_shard_workspace_bytes(2, 48, 128, 64 * 100) == 64 * per_chunk   # at most 64 chunks (a chunk per lane)
    assert lib.svg_sample_mse_shard_workspace_bytes(512, 48, 128, 64 * 100) == 256 * per_chunk  # one chunk per head from 512 heads on
    assert lib.svg_sample_mse_shard_workspace_bytes(0, 48, 128, 64) == 0
    assert lib.svg_sample_mse_from_parts_workspace_bytes(3) == 3 * 32 * 4 * 4


# ---------------------------------------------------------------------------------------------------------
# argument validation, in the header's order.  A sequence of 1024 rows: 9 frames of 100 rows from row 0, 124 rows behind them; the k
# shard: frames [7, 9) and the whole tail (324 rows).  No row passes every check: nothing is ever launched.
# ---------------------------------------------------------------------------------------------------------
BIG = 1 << 40


def _prof(vid0=0, F=9, P=100, coords=(0, 1)):
    d = nat.ProfileDesc(vid0, F, P, 0)
    V = F * P
    for i, c in enumerate(coords):
        d.variant[i] = nat.ProfileVariant(c, 0, V, 1, 0, V, V + 124)
    return d


def _layout(Sk=324, H=2, row=128, **kw):
    k = nat.TensorStrides(H * Sk * row, Sk * row, row)
    lay = nat.AttnLayout(H, 0, k, k, k, k)
    for name, val in kw.items():
        setattr(lay, name, val)
    return lay


def partial_args(q=PH, k=PH, v=PH, rows=PH, R=48, BH=2, S=1024, D=128, dtype=0, prof=None, null_prof=False, ks=(7, 2, 900, 124),
                 null_ks=False, part=PH, ws=PH, ws_bytes=BIG, lay=None):
    prof = _prof() if prof is None else prof
    sh = nat.BandShard(*ks)
    return [q, k, v, rows, R, BH, S, D, dtype, 1.0, None if null_prof else C.byref(prof), None if null_ks else C.byref(sh), part, ws,
            ws_bytes, None, C.byref(lay) if lay is not None else None, None]


BAD_ROW = nat.TensorStrides(2 * 324 * 128, 324 * 128, 64)          # a row stride below D
UNALIGNED_ROW = nat.TensorStrides(2 * 324 * 132, 324 * 132, 132)   # rows that are no multiple of 16 bytes
F16, TOO_MANY_ROWS = dict(dtype=1), dict(R=65)
PARTIAL_CASES = [
    # 1. NULL pointers
    ("null_q_rows", dict(q=None), BAD_ARG),
    ("null_k", dict(k=None), BAD_ARG),
    ("null_v", dict(v=None), BAD_ARG),
    ("null_rows", dict(rows=None), BAD_ARG),
    ("null_prof", dict(null_prof=True), BAD_ARG),
    ("null_k_shard", dict(null_ks=True), BAD_ARG),
    ("null_part", dict(part=None), BAD_ARG),
    ("null_workspace", dict(ws=None), BAD_ARG),
    ("null_part_before_too_many_rows", dict(part=None, **TOO_MANY_ROWS), BAD_ARG),
    ("null_part_before_unsupported_D", dict(part=None, D=64), BAD_ARG),
    # 2. sizes
    ("R0", dict(R=0), BAD_ARG),
    ("BH0", dict(BH=0), BAD_ARG),
    ("S0", dict(S=0), BAD_ARG),
    ("D0", dict(D=0), BAD_ARG),
    ("R_negative_before_f16", dict(R=-1, **F16), BAD_ARG),
    ("num_frame0", dict(prof=_prof(F=0)), BAD_ARG),
    ("frame_size0", dict(prof=_prof(P=0)), BAD_ARG),
    ("vid0_negative", dict(prof=_prof(vid0=-1)), BAD_ARG),
    ("video_ends_behind_S", dict(prof=_prof(vid0=125)), BAD_ARG),
    ("video_ends_behind_S_int32", dict(prof=_prof(F=1 << 16, P=1 << 16)), BAD_ARG),
    # 3. the shard, as check_band_shard checks it
    ("shard_f0_negative", dict(ks=(-1, 3, 0, 0)), BAD_ARG),
    ("shard_frames_behind_F", dict(ks=(8, 2, 900, 124)), BAD_ARG),
    ("shard_frames_behind_F_int32", dict(ks=(2 ** 31 - 1, 2 ** 31 - 1, 900, 124)), BAD_ARG),
    ("shard_n_frames_negative", dict(ks=(2, -1, 900, 10)), BAD_ARG),
    ("shard_n_tail_negative", dict(ks=(7, 2, 900, -1)), BAD_ARG),
    ("shard_tail_inside_the_video", dict(ks=(7, 2, 899, 10)), BAD_ARG),
    ("shard_tail_ends_behind_S", dict(ks=(7, 2, 900, 125)), BAD_ARG),
    ("shard_tail_ends_behind_S_int32", dict(ks=(7, 2, 2 ** 31 - 1, 2 ** 31 - 1)), BAD_ARG),
    ("shard_empty", dict(ks=(9, 0, 900, 0)), BAD_ARG),
    ("shard_before_too_many_rows", dict(ks=(8, 2, 900, 124), **TOO_MANY_ROWS), BAD_ARG),
    ("shard_before_f16", dict(ks=(9, 0, 900, 0), **F16), BAD_ARG),
    ("tail_alone_is_a_shard", dict(ks=(9, 0, 900, 124), **F16), UNSUPPORTED),                       # (accepted: only the dtype stops it)
    ("a_tail_that_is_not_read", dict(ks=(2, 3, -5, 0), **F16), UNSUPPORTED),                        # (n_tail = 0: tail_begin is not read)
    ("frames_that_end_before_F_with_a_tail", dict(ks=(2, 3, 950, 50), **F16), UNSUPPORTED),         # (accepted: the seam jumps)
    # 4. rows in front of the video belong to no shard
    ("vid0_24", dict(prof=_prof(vid0=24), ks=(7, 2, 924, 100)), BAD_ARG),
    ("vid0_24_before_too_many_rows", dict(prof=_prof(vid0=24), ks=(7, 2, 924, 100), **TOO_MANY_ROWS), BAD_ARG),
    # 5. R > 64
    ("R65", dict(**TOO_MANY_ROWS), UNSUPPORTED),
    ("R65_before_workspace", dict(ws_bytes=0, **TOO_MANY_ROWS), UNSUPPORTED),
    # 6. one-wrap stepping of a token-major variant
    ("frame_size_32_token_major", dict(prof=_prof(P=32), ks=(7, 2, 288, 10)), UNSUPPORTED),
    ("frame_size_32_token_major_before_workspace", dict(prof=_prof(P=32), ks=(7, 2, 288, 10), ws_bytes=0), UNSUPPORTED),
    ("frame_size_32_frame_major_is_accepted", dict(prof=_prof(P=32, coords=(0, 0)), ks=(7, 2, 288, 10), ws_bytes=0), WORKSPACE),
    # 7. S
    ("S_2pow24", dict(S=1 << 24), UNSUPPORTED),
    ("S_2pow24_before_workspace", dict(S=1 << 24, ws_bytes=0), UNSUPPORTED),
    # 8. workspace
    ("workspace_0", dict(ws_bytes=0), WORKSPACE),
    ("workspace_before_layout", dict(ws_bytes=0, lay=_layout(heads_per_batch=0)), WORKSPACE),
    ("workspace_before_f16", dict(ws_bytes=0, **F16), WORKSPACE),
    ("workspace_before_D64", dict(ws_bytes=0, D=64), WORKSPACE),
    # 9. layout, k and v members, against Sk
    ("bad_layout_heads0", dict(lay=_layout(heads_per_batch=0)), BAD_ARG),
    ("bad_layout_k_row_below_D", dict(lay=_layout(k=BAD_ROW)), BAD_ARG),
    ("bad_layout_v_row_below_D", dict(lay=_layout(v=BAD_ROW)), BAD_ARG),
    ("layout_v_row_unaligned", dict(lay=_layout(v=UNALIGNED_ROW)), UNSUPPORTED),
    ("bad_layout_before_f16", dict(lay=_layout(k=BAD_ROW), **F16), BAD_ARG),
    ("layout_k_unaligned_pointer", dict(k=PH + 8, lay=_layout()), UNSUPPORTED),
    ("layout_q_and_o_members_are_not_read", dict(lay=_layout(q=BAD_ROW, o=BAD_ROW), **F16), UNSUPPORTED),   # (BAD_ARG if they were)
    # 10. dtype, D
    ("f16", dict(**F16), UNSUPPORTED),
    ("dtype_f32", dict(dtype=2), UNSUPPORTED),
    ("D64", dict(D=64), UNSUPPORTED),
    ("D96", dict(D=96), UNSUPPORTED),
]


@pytest.mark.parametrize("kw,expected", [c[1:] for c in PARTIAL_CASES], ids=[c[0] for c in PARTIAL_CASES])
def test_partial_validation_order(kw, expected):
    _host_only()
    assert nat.load().svg_sample_mse_shard_partial(*partial_args(**kw)) == expected


def test_partial_workspace_is_the_stated_size():
    _host_only()
    lib = nat.load()
    need = lib.svg_sample_mse_shard_workspace_bytes(2, 48, 128, 324)
    assert need > 0
    assert lib.svg_sample_mse_shard_partial(*partial_args(ws_bytes=need - 1, **F16)) == WORKSPACE
    assert lib.svg_sample_mse_shard_partial(*partial_args(ws_bytes=need, **F16)) == UNSUPPORTED     # (enough: only the dtype stops it)


def parts_args(n=2, null_at=None, null_parts=False, R=48, BH=2, D=128, dtype=0, out=PH, ws=PH, ws_bytes=BIG):
    arr = (C.c_void_p * max(n, 1))(*[None if i == null_at else PH + 0x1000 * i for i in range(max(n, 1))])
    return [None if null_parts else C.cast(arr, C.c_void_p), n, R, BH, D, dtype, 0, out, ws, ws_bytes, None, None], arr


FROM_PARTS_CASES = [
    ("null_parts", dict(null_parts=True), BAD_ARG),
    ("null_out_mse", dict(out=None), BAD_ARG),
    ("null_workspace", dict(ws=None), BAD_ARG),
    ("null_out_before_too_many_rows", dict(out=None, R=65), BAD_ARG),
    ("n_parts_0", dict(n=0), BAD_ARG),
    ("n_parts_65", dict(n=65), BAD_ARG),
    ("n_parts_negative", dict(n=-1), BAD_ARG),
    ("R0", dict(R=0), BAD_ARG),
    ("BH0", dict(BH=0), BAD_ARG),
    ("D0", dict(D=0), BAD_ARG),
    ("null_part_1", dict(null_at=1), BAD_ARG),
    ("null_last_part_of_64", dict(n=64, null_at=63), BAD_ARG),
    ("null_part_before_too_many_rows", dict(null_at=0, R=65), BAD_ARG),
    ("R65", dict(R=65), UNSUPPORTED),
    ("R65_before_workspace", dict(R=65, ws_bytes=0), UNSUPPORTED),
    ("workspace_0", dict(ws_bytes=0), WORKSPACE),
    ("workspace_one_byte_short", dict(ws_bytes=2 * 32 * 4 * 4 - 1), WORKSPACE),
    ("workspace_before_f16", dict(ws_bytes=0, dtype=1), WORKSPACE),
    ("workspace_exact_f16", dict(ws_bytes=2 * 32 * 4 * 4, dtype=1), UNSUPPORTED),
    ("f16", dict(dtype=1), UNSUPPORTED),
    ("D64", dict(D=64), UNSUPPORTED),
    ("64_parts_are_accepted", dict(n=64, dtype=1), UNSUPPORTED),                                     # (only the dtype stops it)
]


@pytest.mark.parametrize("kw,expected", [c[1:] for c in FROM_PARTS_CASES], ids=[c[0] for c in FROM_PARTS_CASES])
def test_from_parts_validation_order(kw, expected):
    _host_only()
    args, keep = parts_args(**kw)
    assert nat.load().svg_sample_mse_from_parts(*args) == expected


# ---------------------------------------------------------------------------------------------------------
# the wrappers: what has no shard form raises before anything runs (CPU tensors get this far)
# ---------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_what_has_no_shard_form(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda *a, **k: None)
    prof, ks = _prof(), (7, 2, 900, 124)
    qr, k = torch.zeros(2, 48, 128, dtype=torch.bfloat16), torch.zeros(2, 324, 128, dtype=torch.bfloat16)
    rows = torch.arange(48)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.sample_mse_shard_partial(qr, k, k, rows, prof, ks, 1024)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.sample_mse_from_parts([torch.zeros(3, 2, 48, 132)], 48, torch.bfloat16, 0)
    monkeypatch.setattr(nat, "_gpu", lambda *ts: None)   # (as if the tensors were on a GPU: the checks behind the device check)
    monkeypatch.setattr(nat, "_dev", lambda *ts: None)
    with pytest.raises(ValueError, match="head_dim 128"):
        nat.sample_mse_shard_partial(qr.half(), k.half(), k.half(), rows, prof, ks, 1024)
    with pytest.raises(ValueError, match="head_dim 128"):
        nat.sample_mse_shard_partial(qr[..., :64], k[..., :64], k[..., :64], rows, prof, ks, 1024)
    with pytest.raises(ValueError, match="rows int64"):
        nat.sample_mse_shard_partial(qr, k, k, rows[:40], prof, ks, 1024)
    with pytest.raises(ValueError, match="belong to no shard"):
        nat.sample_mse_shard_partial(qr, k, k, rows, _prof(vid0=24), (7, 2, 924, 100), 1024)
    with pytest.raises(ValueError, match="outside a video"):
        nat.sample_mse_shard_partial(qr, k, k, rows, prof, (8, 2, 900, 124), 1024)
    with pytest.raises(ValueError, match="empty shard"):
        nat.sample_mse_shard_partial(qr, k, k, rows, prof, (9, 0, 900, 0), 1024)
    with pytest.raises(ValueError, match="the shard says"):
        nat.sample_mse_shard_partial(qr, k[:, :300], k[:, :300], rows, prof, ks, 1024)
    with pytest.raises(ValueError, match="1 to 64 parts"):
        nat.sample_mse_from_parts([], 48, torch.bfloat16, 0)
    with pytest.raises(ValueError, match="1 to 64 parts"):
        nat.sample_mse_from_parts([torch.zeros(3, 2, 48, 132)] * 65, 48, torch.bfloat16, 0)
    with pytest.raises(ValueError, match="of one shape"):
        nat.sample_mse_from_parts([torch.zeros(3, 2, 48, 132), torch.zeros(3, 2, 40, 132)], 48, torch.bfloat16, 0)
    with pytest.raises(ValueError, match="bfloat16"):
        nat.sample_mse_from_parts([torch.zeros(3, 2, 48, 132)], 48, torch.float16, 0)


def test_neutral_part():
    p = nat.neutral_profile_part(2, 5, 128, "cpu")
    assert p.shape == (3, 2, 5, 132) and p.dtype == torch.float32
    assert bool((p[..., :128] == 0).all()) and bool((p[..., 128] == float("-inf")).all()) and bool((p[..., 129:] == 0).all())
    assert nat.sample_mse_shard_partial is nat._sample_mse_shard_partial and nat.sample_mse_from_parts is nat._sample_mse_from_parts


def test_sampled_row_owners():
    from svg.distributed import frame_shard, sampled_row_owners

    geo = (5 * 30 + 7, 0, 5, 30)
    for world in (1, 2, 3, 8):
        held = [[] for _ in range(world)]
        for r in range(world):
            s = frame_shard(geo, r, world)
            held[r] = list(range(s.f0 * 30, (s.f0 + s.n_frames) * 30)) + list(range(s.tail_begin, s.tail_begin + s.n_tail))
        own = sampled_row_owners(range(geo[0]), geo, world)
        assert all(held[r][l] == g for g, (r, l) in enumerate(own))
    assert sampled_row_owners([156], geo, 8) == [(7, 6)]        # (8 ranks, 5 frames: the last rank holds the tail alone)
    with pytest.raises(ValueError, match="outside"):
        sampled_row_owners([157], geo, 2)


# ---------------------------------------------------------------------------------------------------------
# the schedules on gloo CPU ranks.  The float64 statements of a part and of the combine:
#   part[o, h, i] = (sum_j p_ij v_j, m_i, sum_j p_ij, 0, 0), p_ij = mask_o(rows[i], G(j)) 2^(s_ij - m_i), s = q . k log2(e) / sqrt(D), m_i the
#   golden maximum over the shard's keys; the combine: weights 2^(m_c - M), o = sum O_c w_c / sum l_c w_c, the mean squared difference.
# ---------------------------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634
H_, D_ = 3, 16


def shard_keys(shard, P):
    f0, n, tail0, n_tail = shard
    return torch.cat([torch.arange(f0 * P, (f0 + n) * P), torch.arange(tail0, tail0 + n_tail)])


def partial64(q_rows, k, v, rows, shard, masks, P):
    keys = shard_keys(shard, P)
    s = torch.matmul(q_rows, k.transpose(-2, -1)) * (LOG2E / q_rows.shape[-1] ** 0.5)      # [H, R, Sk]
    m = s.max(-1).values
    part = torch.zeros(3, q_rows.shape[0], q_rows.shape[1], q_rows.shape[2] + 4, dtype=torch.float64)
    for o, sel in enumerate([None, masks[0], masks[1]]):
        p = torch.exp2(s - m[..., None])
        if sel is not None:
            p = p * sel[rows][:, keys].double()
        part[o, :, :, :-4] = torch.matmul(p, v)
        part[o, :, :, -4] = m
        part[o, :, :, -3] = p.sum(-1)
    return part


def combine64(parts, R):
    P_ = torch.stack(list(parts))                                   # [n, 3, H, R, D + 4]
    m = P_[..., -4]
    M = m.max(0).values
    w = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp2(m - M))
    o = (P_[..., :-4] * w[..., None]).sum(0) / (P_[..., -3] * w).sum(0)[..., None]
    return torch.stack([((o[1] - o[0]) ** 2).mean((-2, -1)), ((o[2] - o[0]) ** 2).mean((-2, -1))])


def profile_inputs(model, F, P, ctx, seed=11):
    """structured data as tests/test_gpu_kernels.py::test_sample_mse builds it (head 0 temporal, head 1 spatial), float64; v scaled by
    2^-8: sample_mse_fp32 carries its own fp32 rounding, about 1e-7 of an MSE (9e-10 was seen at MSEs of 4e-3, v scaled by 2^-4), and
    that has to stay well below the 1e-9 the results are compared to; the float64 statement of the oracle is compared relatively"""
    g = torch.Generator().manual_seed(seed)
    V, S = F * P, F * P + ctx
    q, k, v = (torch.randn(H_, S, D_, generator=g, dtype=torch.float64) for _ in range(3))
    pos, frm = torch.randn(P, D_, generator=g, dtype=torch.float64), torch.randn(F, D_, generator=g, dtype=torch.float64)
    k[0, :V] += 3 * pos.repeat(F, 1)
    q[0, :V] += 3 * pos.repeat(F, 1)
    k[1, :V] += 3 * frm.repeat_interleave(P, 0)
    q[1, :V] += 3 * frm.repeat_interleave(P, 0)
    rows = torch.cat([torch.randint(0, V, (10,), generator=g), torch.tensor([S - 1, 0] if ctx else [V - 1, 0])])   # a text row (hy), row 0
    return q, k, v / 256, rows


SCHEDULE_CASES = [("hy", 5, 150, 20), ("wan", 5, 150, 0), ("hy", 2, 150, 20), ("wan", 2, 150, 0)]


def _mse_worker(rank, world):
    from svg import distributed as sd

    out = {}
    for model, F, P, ctx in SCHEDULE_CASES:
        S = F * P + ctx
        geo = (S, 0, F, P)
        q, k, v, rows = profile_inputs(model, F, P, ctx)
        masks = O.profile_masks(model, ctx, F, P)
        sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
        mine = shard_keys(sh[rank], P)
        seen = {}

        def partial_fn(q_rows, k_, v_, rows_dev, k_shard):
            seen["bits"] = bool(torch.equal(q_rows.view(torch.int64), q[:, rows].contiguous().view(torch.int64)))
            seen["shard"] = k_shard.as_tuple() == sh[rank] and k_.shape == (H_, len(mine), D_) and torch.equal(rows_dev, rows)
            return partial64(q_rows, k_, v_, rows_dev, k_shard.as_tuple(), masks, P)

        partial_fn.part_dtype = torch.float64
        n_parts = []

        def combine_fn(parts, R):
            n_parts.append(len(parts))
            return combine64(parts, R)

        prof = nat.ProfileDesc(0, F, P, 0)
        mse = sd.token_sharded_sample_mse(q[:, mine].contiguous(), k[:, mine].contiguous(), v[:, mine].contiguous(), rows, prof, geo,
                                          partial_fn=partial_fn, combine_fn=combine_fn)
        out[model, F] = dict(mse=mse, rows_held=len(mine), seen=dict(seen), n_parts=n_parts)
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_sample_mse_gloo(world):
    """frame shards of 5 frames (3 / 2 and 2 / 2 / 1) and of 2 frames — on three ranks the last one then holds no frame: the tail alone (hy) or
    nothing at all (wan: the neutral part) —, the text on the last rank: the merged MSEs equal sample_mse_fp32 of the whole sequence to 1e-9
    (and the float64 statement of it to 1e-12 of the largest), are identical on every rank, the gathered q rows are q[:, rows] bit for bit, and every rank
    combined `world` parts"""
    got = run_ranks(_mse_worker, world, 44500)
    for model, F, P, ctx in SCHEDULE_CASES:
        q, k, v, rows = profile_inputs(model, F, P, ctx)
        masks = list(O.profile_masks(model, ctx, F, P))
        ref32 = O.sample_mse_fp32(q[None], k[None], v[None], rows, masks)[:, 0]
        ref64 = O.sample_mse(q[None], k[None], v[None], rows, masks)[:, 0]
        assert ref64.dtype == torch.float64 and torch.isfinite(ref64).all() and float(ref64.max()) > 1e-6
        for rank in range(world):
            r = got[rank][model, F]
            e32, e64 = (r["mse"] - ref32.double()).abs().max().item(), (r["mse"] - ref64).abs().max().item()
            print(f"{model} F={F} world={world} rank {rank}: |mse - fp32 oracle| {e32:.2e}, |mse - float64| {e64:.2e}, mse {r['mse'].tolist()}")
            assert r["mse"].shape == (2, H_) and e32 <= 1e-9 and e64 <= 1e-12 * float(ref64.max()), (model, F, rank, e32, e64)
            assert torch.equal(r["mse"], got[0][model, F]["mse"])                      # the same bits on every rank
            assert r["n_parts"] == [world]
            if r["rows_held"]:
                assert r["seen"] == dict(bits=True, shard=True), (model, F, rank, r["seen"])
            else:
                assert r["seen"] == {}                                                   # no rows: the neutral part, no call
        if F == 2 and world == 3:
            assert got[2][model, F]["rows_held"] == ctx and got[1][model, F]["rows_held"] == P
        if F == 5:                                                                     # (two frames give a temporal head little to find)
            assert torch.equal(ref64.argmin(0)[:2], torch.tensor([1, 0])), (model, ref64)  # head 0 temporal, head 1 spatial, as constructed


def _layer_worker(rank, world):
    import sparse_lse_cases as SC
    from lse_ops_torch import merge_states
    from svg import distributed as sd

    model, F, P, ctx = "hy", 5, 150, 20
    S = F * P + ctx
    geo = (S, 0, F, P)
    q, k, v, rows = profile_inputs(model, F, P, ctx)
    masks = list(O.profile_masks(model, ctx, F, P))
    best = O.sample_mse(q[None], k[None], v[None], rows, masks)[:, 0].argmin(0)          # the single-process argmin
    mp_ = dict(real_len=S, band=200, colfull_lo=F * P, colfull_hi=S, rowfull_lo=F * P, rowfull_hi=S)
    em = O.band_mask(S, **mp_)
    sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
    mine = shard_keys(sh[rank], P)

    def coords(idx, tm):
        return torch.where(idx < F * P, (idx % P) * F + idx // P, idx) if tm else idx

    def attn_fn(q_, k_, v_, q_shard, k_shard):
        rq, rk = shard_keys(q_shard.as_tuple(), P), shard_keys(k_shard.as_tuple(), P)
        parts = [SC.masked_attention_lse(q_[None, h:h + 1], k_[None, h:h + 1], v_[None, h:h + 1],
                                         em[coords(rq, bool(best[h]))][:, coords(rk, bool(best[h]))]) for h in range(H_)]
        return torch.cat([o for o, _ in parts], dim=1)[0], torch.cat([l for _, l in parts], dim=1)[0]

    def partial_fn(q_rows, k_, v_, rows_dev, k_shard):
        return partial64(q_rows, k_, v_, rows_dev, k_shard.as_tuple(), masks, P)

    partial_fn.part_dtype = torch.float64
    o, idx = sd.token_sharded_svg1_layer_call(q[:, mine].contiguous(), k[:, mine].contiguous(), v[:, mine].contiguous(),
                                              nat.BandMask(**mp_), nat.ProfileDesc(0, F, P, 0), geo, rows, partial_fn=partial_fn,
                                              combine_fn=combine64, attn_fn=attn_fn, merge_fn=merge_states)
    refs = []
    for h in range(H_):
        c = coords(torch.arange(S), bool(best[h]))
        refs.append(SC.masked_attention_lse(q[None, h:h + 1, mine], k[None, h:h + 1], v[None, h:h + 1], em[c[mine]][:, c])[0])
    ref = torch.cat(refs, dim=1)[0]
    return dict(idx=idx, best=best, err=(o - ref).abs().max().item(), shape_ok=o.shape == (H_, len(mine), D_))


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_svg1_layer_call_gloo(world):
    """the layer-call from q, k, v alone: best_mask_idx is the single-process argmin on every rank (head 0 token-major, head 1 in logical
    order, as constructed), and the rank's rows of the attention under it equal the float64 statement over all keys"""
    got = run_ranks(_layer_worker, world, 42500)
    for rank, r in got.items():
        assert r["idx"].dtype == torch.int64 and torch.equal(r["idx"], r["best"]) and r["idx"][:2].tolist() == [1, 0], (rank, r)
        assert r["shape_ok"] and r["err"] <= 1e-9, (rank, r["err"])


def test_argmin_rounds_to_the_dtype_of_q_first(monkeypatch):
    """two MSEs that round to one bf16 value tie to index 0, and NaN wins, as svg.models._core.sample_mse has it"""
    from svg import distributed as sd

    mse = torch.tensor([[1.0, 1.0, 0.5, float("nan")], [1.0 - 2.0 ** -12, 0.5, float("nan"), 0.25]])
    assert torch.argmin(mse, dim=0).tolist() == [1, 1, 1, 0]                              # (fp32: head 0 would flip)
    monkeypatch.setattr(sd, "token_sharded_sample_mse", lambda *a, **k: mse)
    monkeypatch.setattr(sd, "token_sharded_svg1_attention", lambda q, k, v, mask, best, geo, **kw: (q, kw["kinds"]))
    x = torch.zeros(4, 8, 16, dtype=torch.bfloat16)
    (o, kinds), best = sd.token_sharded_svg1_layer_call(x, x, x, None, None, (8, 0, 1, 8), torch.arange(4))
    assert best.tolist() == [0, 1, 1, 0] and kinds == "both" and o is x


def test_token_sharded_sample_mse_refuses_too_many_ranks(monkeypatch):
    from svg import distributed as sd

    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 65)
    x = torch.zeros(2, 20, 16, dtype=torch.float64)
    with pytest.raises(ValueError, match="at most 64 parts"):
        sd.token_sharded_sample_mse(x, x, x, torch.arange(4), nat.ProfileDesc(0, 65, 20, 0), (65 * 20, 0, 65, 20))
