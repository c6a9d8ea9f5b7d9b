"""The device switch of band attention on frame shards without a GPU (include/svg_attn_band_shard_switch.h:
svg_band_shard_attention_switch_lse[_f32]; _native.band_shard_attention_switch; svg.distributed.band_shard_exchange_plan(dense_mask=),
token_sharded_svg1_attention / token_sharded_svg1_layer_call with dense_mask / dense_flag, enable_frame_shards; the frame-shard mode of
svg.models._core and of the processors): the exports and prototypes, the argument validation in the order the header states — every row
of the shard entries' table with the same code, and the rows of alt_mask / use_alt_flag —, the OR-ed exchange plan, the two schedules on
gloo CPU ranks with float64 statements for a flag of 0 and of 1, the two modes' mutual exclusion, and the refusals of frame-shard mode,
which are raised on the host before any collective.

ref: the dense warm-up / sparse branch of svg/models/hyvideo/attention.py:491-524; the head placement of
svg/models/hyvideo/placement.py:156-184."""
import ctypes as C
import os
import re
from pathlib import Path

import pytest
import torch
import torch.distributed as dist

import band_shard_cases as BC
import sparse_lse_cases as SC
import test_band_shard_cpu as B
import test_profile_shard_cpu as PS
from gloo_ranks import CountingAllToAll, run_ranks
from lse_ops_torch import merge_states
from oracle import svg_oracle as O
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED = 0, -1, -2   # include/svg_attn.h
PH = B.PH
ROOT = Path(__file__).resolve().parent.parent
ENTRIES = ("svg_band_shard_attention_switch_lse", "svg_band_shard_attention_switch_lse_f32")


# ---------------------------------------------------------------------------------------------------------
# exports and prototypes
# ---------------------------------------------------------------------------------------------------------
def test_library_exports_the_switch_entries():
    lib = nat.load()
    assert set(nat.BAND_SHARD_SWITCH_SIGNATURES) == set(ENTRIES)
    others = (set(nat.SIGNATURES) | set(nat.SPARSE_LSE_SIGNATURES) | set(nat.SPARSE_F32_SIGNATURES) | set(nat.BAND_LSE_FORM_SIGNATURES)
              | set(nat.BAND_WINDOW_SIGNATURES) | set(nat.BAND_SHARD_SIGNATURES) | set(nat.PROFILE_SHARD_SIGNATURES))
    assert not set(ENTRIES) & others
    for name, (res, args) in nat.BAND_SHARD_SWITCH_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    # the arguments of the shard entries plus alt_mask and use_alt_flag behind perm
    plain = nat.BAND_SHARD_SIGNATURES["svg_band_shard_attention_lse"][1]
    assert nat.BAND_SHARD_SWITCH_SIGNATURES[ENTRIES[0]][1] == plain[:12] + [C.POINTER(nat.BandMask), C.c_void_p] + plain[12:]
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_prototypes_match_the_ctypes_signatures():
    assert '#include "svg_attn_band_shard_switch.h"' in (ROOT / "include" / "svg_attn.h").read_text()
    src = (ROOT / "include" / "svg_attn_band_shard_switch.h").read_text()
    assert "in this order" in src                                   # the order of the checks is written down
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert {n for _, n, _ in protos} == set(ENTRIES)

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
        assert [re.search(r"([A-Za-z_0-9]+)$", x).group(1) for x in ps][12:14] == ["alt_mask", "use_alt_flag"]
        want = [c_class(x if x.endswith("*") else re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", x)) for x in ps]
        res, args = nat.BAND_SHARD_SWITCH_SIGNATURES[name]
        assert hasattr(lib, name) and [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


# ---------------------------------------------------------------------------------------------------------
# argument validation: the table of the shard entries (tests/test_band_shard_cpu.py), every row with the same code, and the rows of the
# two new arguments — NULL with the first check, alt_mask against S where band_run checks it (behind mask and the size limits)
# ---------------------------------------------------------------------------------------------------------
def switch_args(alt="ok", null_alt=False, flag=PH, **kw):
    args = B.shard_args(**kw)
    S = kw.get("S", 1024)
    alt = B._mask(S, band=S + 1) if alt == "ok" else alt
    args[12:12] = [None if null_alt else C.byref(alt), flag]
    return args


SWITCH_CASES = [
    ("null_alt_mask", dict(null_alt=True), BAD_ARG),
    ("null_use_alt_flag", dict(flag=None), BAD_ARG),
    ("null_alt_mask_before_unsupported_D", dict(null_alt=True, D=64), BAD_ARG),
    ("null_use_alt_flag_before_bad_geometry", dict(flag=None, perm=(PH, 0, 0, 100), D=64), BAD_ARG),
    ("null_alt_mask_before_bad_shard", dict(null_alt=True, qs=(7, 3, 0, 0)), BAD_ARG),
    ("bad_alt_mask_band", dict(alt=B._mask(1024, band=-1)), BAD_ARG),
    ("bad_alt_mask_real_len_behind_S", dict(alt=B._mask(1024, real_len=1025)), BAD_ARG),
    ("bad_alt_mask_before_unsupported_D", dict(alt=B._mask(1024, band=-1), D=64), BAD_ARG),
    ("bad_alt_mask_before_unsupported_dtype", dict(alt=B._mask(1024, band=-1), dtype=2), BAD_ARG),
    ("bad_alt_mask_before_bad_layout", dict(alt=B._mask(1024, band=-1), lay=B._layout(300, 324, q=B.UNALIGNED_ROW)), BAD_ARG),
    ("bad_shard_before_bad_alt_mask", dict(alt=B._mask(1024, band=-1), qs=(7, 3, 0, 0), D=64), BAD_ARG),
    ("size_limit_before_bad_alt_mask", dict(alt=B._mask(1 << 24, band=-1), S=1 << 24), UNSUPPORTED),   # (as svg_band_attention_switch)
    ("good_alt_mask_only_D_stops_it", dict(D=64), UNSUPPORTED),
]


@pytest.mark.parametrize("name", ENTRIES)
@pytest.mark.parametrize("kw,expected", [c[1:] for c in B.CASES + SWITCH_CASES], ids=[c[0] for c in B.CASES + SWITCH_CASES])
def test_validation_order(kw, expected, name):
    B._host_only()
    assert getattr(nat.load(), name)(*switch_args(**kw)) == expected


def test_the_table_holds_the_rows_the_header_promises():
    ids = {c[0] for c in B.CASES + SWITCH_CASES}
    for want in ("null_alt_mask", "null_use_alt_flag", "bad_alt_mask_band", "bad_alt_mask_before_unsupported_D", "null_perm", "null_q_shard",
                 "q_shard_frames_behind_F", "k_shard_tail_ends_behind_S", "q_shard_empty", "bad_mask_before_unsupported_D", "D64", "dtype_f32"):
        assert want in ids
    assert len(B.CASES) >= 40                                        # everything the shard entries refuse is asked again


def test_misaligned_o32_is_unsupported_and_argument_faults_come_first():
    B._host_only()
    lib = nat.load()
    assert lib.svg_band_shard_attention_switch_lse_f32(*switch_args(o=PH + 8)) == UNSUPPORTED
    assert lib.svg_band_shard_attention_switch_lse_f32(*switch_args(o=PH + 8, alt=B._mask(1024, real_len=1025))) == BAD_ARG
    assert lib.svg_band_shard_attention_switch_lse_f32(*switch_args(o=PH + 8, null_alt=True)) == BAD_ARG
    assert lib.svg_band_shard_attention_switch_lse(*switch_args(o=PH + 8, D=64)) == UNSUPPORTED


def test_wrapper_refuses_what_has_no_shard_form(monkeypatch):
    monkeypatch.setattr(nat, "load", lambda *a, **k: pytest.fail("nothing may be loaded or launched"))
    m, alt = B._mask(1024), B._mask(1024, band=1025)
    geo = (0, 9, 100)
    qs, ks = (2, 3, 0, 0), (7, 2, 900, 124)
    q, k = torch.zeros(1, 2, 300, 128, dtype=torch.bfloat16), torch.zeros(1, 2, 324, 128, dtype=torch.bfloat16)
    flag = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        nat.band_shard_attention_switch(q, k, k, m, alt, flag, 1024, geo, qs, ks)
    with pytest.raises(ValueError, match="out_dtype"):
        nat.band_shard_attention_switch(q, k, k, m, alt, flag, 1024, geo, qs, ks, out_dtype=torch.float16)
    monkeypatch.setattr(nat, "_gpu", lambda *ts: None)   # (as if the tensors were on a GPU: the checks behind the device check)
    monkeypatch.setattr(nat, "_dev", lambda *ts: None)
    with pytest.raises(ValueError, match="use_alt_flag is int32"):
        nat.band_shard_attention_switch(q, k, k, m, alt, flag.long(), 1024, geo, qs, ks)
    with pytest.raises(ValueError, match="head_dim 128"):
        nat.band_shard_attention_switch(q[..., :64], k[..., :64], k[..., :64], m, alt, flag, 1024, geo, qs, ks)
    with pytest.raises(ValueError, match="outside a video"):
        nat.band_shard_attention_switch(q, k, k, m, alt, flag, 1024, geo, (7, 3, 0, 0), ks)
    with pytest.raises(ValueError, match="the shards say"):
        nat.band_shard_attention_switch(q, k[:, :, :300], k[:, :, :300], m, alt, flag, 1024, geo, qs, ks)


# ---------------------------------------------------------------------------------------------------------
# the OR-ed plan: the flag is never read back, so a pair that either setting needs is kept
# ---------------------------------------------------------------------------------------------------------
def _dense(S, real=None):
    return nat.BandMask(**O.dense_band_params(S)) if real is None else nat.BandMask(real, S + 1, 0, 0, 0, 0)


def test_the_plan_keeps_a_pair_either_setting_needs():
    from svg.distributed import band_shard_exchange_plan

    geo = BC.geometry("wan")
    wan = nat.BandMask(**BC.CASES["wan"]["mask"])
    sparse = band_shard_exchange_plan(wan, geo, 3, "logical")
    assert sparse[0] == [True, True, False]                         # band 129: the first shard's rows see no key of the last
    both = band_shard_exchange_plan(wan, geo, 3, "logical", dense_mask=_dense(geo[0]))
    assert all(all(row) for row in both)                            # a dense warm-up step needs every pair
    dense_alone = band_shard_exchange_plan(_dense(geo[0]), geo, 3, "logical")
    assert both == [[a or b for a, b in zip(ra, rb)] for ra, rb in zip(sparse, dense_alone)]
    # an alternate mask that needs nothing more changes nothing; a rank without rows stays out (8 ranks, 7 frames)
    assert band_shard_exchange_plan(wan, geo, 3, "logical", dense_mask=wan) == sparse
    eight = band_shard_exchange_plan(wan, geo, 8, "logical", dense_mask=_dense(geo[0]))
    assert not any(eight[7]) and not any(row[7] for row in eight) and all(all(row[:7]) for row in eight[:7])
    # hy: the padding behind real_len sees itself only, under the dense mask too
    hy, g = BC.CASES["hy"], BC.geometry("hy")
    hy_plan = band_shard_exchange_plan(nat.BandMask(**hy["mask"]), g, 3, "both", dense_mask=_dense(g[0], hy["mask"]["real_len"]))
    assert all(all(row) for row in hy_plan)


def test_dense_mask_and_dense_flag_go_together(monkeypatch):
    from svg import distributed as sd

    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: pytest.fail("refused before the group is asked"))
    x = torch.zeros(1, 2, 20, 16, dtype=torch.float64)
    m = _dense(180)
    for fn, args in ((sd.token_sharded_svg1_attention, (x, x, x, m, None, (180, 0, 9, 20))),
                     (sd.token_sharded_svg1_layer_call, (x, x, x, m, None, (180, 0, 9, 20), torch.arange(4)))):
        with pytest.raises(ValueError, match="go together"):
            fn(*args, dense_mask=m)
        with pytest.raises(ValueError, match="go together"):
            fn(*args, dense_flag=torch.zeros(1, dtype=torch.int32))


def test_too_many_parts_is_judged_on_the_ored_plan(monkeypatch):
    from svg import distributed as sd

    monkeypatch.setattr(sd.dist, "get_rank", lambda group=None: 0)
    monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 9)
    geo = (9 * 20, 0, 9, 20)
    x = torch.zeros(1, 2, 20, 16, dtype=torch.float64)
    narrow = B._mask(180, band=10)
    assert max(sum(row) for row in sd.band_shard_exchange_plan(narrow, geo, 9, "logical")) == 3       # the sparse mask alone would pass
    with pytest.raises(ValueError, match="at most 8 parts"):
        sd.token_sharded_svg1_attention(x, x, x, narrow, None, geo, kinds="logical", dense_mask=_dense(180),
                                        dense_flag=torch.zeros(1, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------
# the schedules on gloo CPU ranks, float64 statements, mixed head kinds
# ---------------------------------------------------------------------------------------------------------
def _attention_worker(rank, world):
    from svg import distributed as sd

    a2a = CountingAllToAll()
    H, D = 4, 16
    out = {}
    for name, flags, kinds in (("hy", BC.FLAGS, "both"), ("wan", BC.FLAGS, "both"), ("wan", (0, 0, 0, 0), "logical")):
        geo = BC.geometry(name)
        S, vid0, F, P = geo
        c = BC.CASES[name]
        em = BC.element_mask(name)
        dense_prm = dict(real_len=c["mask"]["real_len"], band=S + 1, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)
        em_dense = O.band_mask(S, **dense_prm)
        mask, dense = nat.BandMask(**c["mask"]), nat.BandMask(**dense_prm)
        g = torch.Generator().manual_seed(5)
        q, k, v = (torch.randn(1, H, S, D, generator=g, dtype=torch.float64) for _ in range(3))
        fl = torch.tensor(flags).view(1, H)
        ctx = S - F * P
        ql, kl, vl = (O.head_placement(x, fl, ctx, F, P) for x in (q, k, v))          # flag 0: placement -> mask -> inverse placement
        ref = {0: O.head_placement(SC.masked_attention_lse(ql, kl, vl, em)[0], fl, ctx, F, P, inverse=True),
               1: SC.masked_attention_lse(q, k, v, em_dense)[0]}                        # flag 1: the dense mask, no placement
        sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
        rows = BC.shard_rows(name, sh[rank])
        plan = sd.band_shard_exchange_plan(mask, geo, world, kinds, dense_mask=dense)
        sparse_plan = sd.band_shard_exchange_plan(mask, geo, world, kinds)
        n_rows = [nat.band_shard_rows(s, P) for s in sh]
        per_tok = 2 * H * D * 8
        for flag in (0, 1):
            calls = []

            def attn_fn(q_, k_, v_, q_shard, k_shard):                                   # (five arguments: the flag is the statement's own)
                qs, ks = q_shard.as_tuple(), k_shard.as_tuple()
                calls.append((qs, ks))
                rq, rk = BC.shard_rows(name, qs), BC.shard_rows(name, ks)
                parts = []
                for h in range(H):
                    pm = em_dense[rq][:, rk] if flag else BC.pair_mask(name, qs, ks, bool(flags[h]))
                    parts.append(SC.masked_attention_lse(q_[:, h:h + 1], k_[:, h:h + 1], v_[:, h:h + 1], pm))
                return torch.cat([o for o, _ in parts], dim=1), torch.cat([l for _, l in parts], dim=1)

            a2a.reset()
            o = sd.token_sharded_svg1_attention(q[:, :, rows].contiguous(), k[:, :, rows].contiguous(), v[:, :, rows].contiguous(), mask, fl,
                                                geo, kinds=kinds, attn_fn=attn_fn, merge_fn=merge_states, dense_mask=dense,
                                                dense_flag=torch.full((1,), flag, dtype=torch.int32))
            out[name, kinds, flag] = dict(
                err=(o - ref[flag][:, :, rows]).abs().max().item(), shape_ok=o.shape == (1, H, len(rows), D), received=a2a.received,
                want_bytes=sum(n_rows[s] * per_tok for s in range(world) if s != rank and plan[rank][s]),
                sparse_bytes=sum(n_rows[s] * per_tok for s in range(world) if s != rank and sparse_plan[rank][s]),
                calls_ok=sorted(calls) == sorted((sh[rank], sh[s]) for s in range(world) if plan[rank][s]))
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_svg1_attention_switch_gloo(world):
    """frame shards of 7 frames, float64 statements as attn_fn / merge_fn, heads 0 and 2 in logical order and 1 and 3 token-major: with a
    flag of 0 every rank's rows equal the single-process placement -> mask -> inverse placement, with a flag of 1 dense-masked attention
    without placement, to 1e-5; the bytes a rank received are those of the OR-ed plan under either flag — on three ranks with heads in
    logical order more than the narrow Wan mask alone would have moved"""
    got = run_ranks(_attention_worker, world, 40500)
    for rank, res in got.items():
        assert len(res) == 6
        for key, r in res.items():
            assert r["shape_ok"] and r["calls_ok"], (rank, key, r)
            assert r["err"] <= 1e-5, (rank, key, r["err"])
            assert r["received"] == r["want_bytes"], (rank, key, r)
    if world == 3:
        for flag in (0, 1):
            r = got[0]["wan", "logical", flag]
            assert r["sparse_bytes"] < r["received"]                # the pair the sparse mask drops travels: the flag is not read


def _layer_worker(rank, world):
    from svg import distributed as sd

    model, F, P, ctx = "hy", 5, 150, 20
    H = PS.H_
    S = F * P + ctx
    geo = (S, 0, F, P)
    q, k, v, rows = PS.profile_inputs(model, F, P, ctx)
    masks = list(O.profile_masks(model, ctx, F, P))
    best = O.sample_mse(q[None], k[None], v[None], rows, masks)[:, 0].argmin(0)          # the single-process argmin: mixed head kinds
    mp_ = dict(real_len=S, band=200, colfull_lo=F * P, colfull_hi=S, rowfull_lo=F * P, rowfull_hi=S)
    em, em_dense = O.band_mask(S, **mp_), O.band_mask(S, **O.dense_band_params(S))
    sh = [sd.frame_shard(geo, r, world).as_tuple() for r in range(world)]
    mine = PS.shard_keys(sh[rank], P)

    def coords(idx, tm):
        return torch.where(idx < F * P, (idx % P) * F + idx // P, idx) if tm else idx

    def partial_fn(q_rows, k_, v_, rows_dev, k_shard):
        return PS.partial64(q_rows, k_, v_, rows_dev, k_shard.as_tuple(), masks, P)

    partial_fn.part_dtype = torch.float64
    res = {}
    for flag in (0, 1):
        def attn_fn(q_, k_, v_, q_shard, k_shard):
            rq, rk = PS.shard_keys(q_shard.as_tuple(), P), PS.shard_keys(k_shard.as_tuple(), P)
            parts = [SC.masked_attention_lse(q_[None, h:h + 1], k_[None, h:h + 1], v_[None, h:h + 1],
                                             em_dense[rq][:, rk] if flag else em[coords(rq, bool(best[h]))][:, coords(rk, bool(best[h]))])
                     for h in range(H)]
            return torch.cat([o for o, _ in parts], dim=1)[0], torch.cat([l for _, l in parts], dim=1)[0]

        o, idx = sd.token_sharded_svg1_layer_call(q[:, mine].contiguous(), k[:, mine].contiguous(), v[:, mine].contiguous(),
                                                  nat.BandMask(**mp_), nat.ProfileDesc(0, F, P, 0), geo, rows, partial_fn=partial_fn,
                                                  combine_fn=PS.combine64, attn_fn=attn_fn, merge_fn=merge_states,
                                                  dense_mask=nat.BandMask(**O.dense_band_params(S)),
                                                  dense_flag=torch.full((1,), flag, dtype=torch.int32))
        refs = []
        for h in range(H):
            c = torch.arange(S) if flag else coords(torch.arange(S), bool(best[h]))
            refs.append(SC.masked_attention_lse(q[None, h:h + 1, mine], k[None, h:h + 1], v[None, h:h + 1], (em_dense if flag else em)[c[mine]][:, c])[0])
        ref = torch.cat(refs, dim=1)[0]
        res[flag] = dict(idx=idx, err=(o - ref).abs().max().item(), shape_ok=o.shape == (H, len(mine), PS.D_))
    res["best"] = best
    return res


@pytest.mark.parametrize("world", [2, 3])
def test_token_sharded_svg1_layer_call_switch_gloo(world):
    """the layer-call with the device switch: with a flag of 0 best_mask_idx is the single-process argmin (head 0 token-major, head 1 in
    logical order) and the rows are the attention under it; with a flag of 1 best_mask_idx is -1 for every head and the rows are
    dense-masked attention without placement"""
    got = run_ranks(_layer_worker, world, 38500)
    for rank, r in got.items():
        assert r[0]["idx"].dtype == torch.int64 and torch.equal(r[0]["idx"], r["best"]) and r[0]["idx"][:2].tolist() == [1, 0], (rank, r)
        assert r[1]["idx"].dtype == torch.int64 and r[1]["idx"].tolist() == [-1] * PS.H_, (rank, r)
        for flag in (0, 1):
            assert r[flag]["shape_ok"] and r[flag]["err"] <= 1e-9, (rank, flag, r[flag]["err"])


def test_the_flag_reaches_the_profiler_and_the_attention(monkeypatch):
    """dense_flag is the profiler's skip_flag and the attention's dense_flag — the same tensor, no copy, nothing read back"""
    from svg import distributed as sd

    seen = {}
    mse = torch.tensor([[1.0, 0.5], [0.5, 1.0]])

    def fake_mse(*a, **k):
        seen["skip_flag"] = k["skip_flag"]
        return mse

    def fake_attn(q, k, v, mask, best, geo, **kw):
        seen.update(dense_mask=kw["dense_mask"], dense_flag=kw["dense_flag"], best=best)
        return q

    monkeypatch.setattr(sd, "token_sharded_sample_mse", fake_mse)
    monkeypatch.setattr(sd, "token_sharded_svg1_attention", fake_attn)
    monkeypatch.setattr(torch.Tensor, "item", lambda self: pytest.fail("no .item()"))
    x = torch.zeros(2, 8, 16, dtype=torch.bfloat16)
    m, dense = _dense(8), _dense(8)
    for value, want in ((0, [1, 0]), (1, [-1, -1]), (7, [-1, -1])):
        flag = torch.full((1,), value, dtype=torch.int32)
        o, best = sd.token_sharded_svg1_layer_call(x, x, x, m, None, (8, 0, 1, 8), torch.arange(4), dense_mask=dense, dense_flag=flag)
        assert seen["skip_flag"] is flag and seen["dense_flag"] is flag and seen["dense_mask"] is dense and o is x
        assert seen["best"].tolist() == [1, 0]                      # the attention gets the argmin itself: the kernel ignores it on a dense step
        assert best.tolist() == want and best.dtype == torch.int64
    sd.token_sharded_svg1_layer_call(x, x, x, m, None, (8, 0, 1, 8), torch.arange(4))
    assert seen["skip_flag"] is None and seen["dense_flag"] is None and seen["dense_mask"] is None


# ---------------------------------------------------------------------------------------------------------
# the two modes; the refusals of frame-shard mode in svg.models._core and the processors: host only, one process, before any collective
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture
def one_rank_group():
    from svg import distributed as sd

    port = 36500 + (os.getpid() % 2000)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        yield sd
    finally:
        sd.disable()
        dist.destroy_process_group()


def test_the_two_modes_exclude_each_other(one_rank_group):
    sd = one_rank_group
    assert not sd.frame_shards_active() and not sd.active()
    sd.enable_frame_shards()
    assert sd.frame_shards_active() and not sd.active() and sd.frame_shards_group() is None
    with pytest.raises(RuntimeError, match="one mode at a time"):
        sd.enable()
    assert sd.frame_shards_active() and not sd._STATE["enabled"]
    sd.disable()
    assert not sd.frame_shards_active() and not sd._STATE["frames"]
    sd.enable()
    assert sd._STATE["enabled"] and not sd.active()                 # (a world of one rank: active() keeps its meaning)
    with pytest.raises(RuntimeError, match="one mode at a time"):
        sd.enable_frame_shards()
    assert not sd.frame_shards_active()
    sd.disable()
    assert not sd._STATE["enabled"] and not sd._STATE["frames"] and sd.current_group() is None and sd.frame_shards_group() is None
    sd.enable_frame_shards()                                        # disable() restored both: either mode can be entered again
    sd.disable()
    sd.enable()


def _no_collectives(monkeypatch):
    for name in ("all_reduce", "all_to_all_single", "all_gather_into_tensor", "broadcast", "all_gather"):
        monkeypatch.setattr(dist, name, lambda *a, _n=name, **k: pytest.fail(f"{_n}: a collective ran before the refusal"))


def test_core_refusals_come_before_any_collective(one_rank_group, monkeypatch):
    from svg.models import _core

    sd = one_rank_group
    sd.enable_frame_shards()
    _no_collectives(monkeypatch)
    geo = _core.Geometry(64, 7, 80)                                  # hy: 560 video rows, 64 behind them; one rank holds them all
    S = geo.seq_len
    q = torch.zeros(1, 2, S, 128, dtype=torch.bfloat16)
    m, dense = nat.BandMask(**BC.CASES["hy"]["mask"]), _dense(S, 597)
    m2 = nat.BandMask(**{**BC.CASES["hy"]["mask"], "real_len": 590})
    prof = nat.ProfileDesc(0, 7, 80, 0)
    flag = torch.zeros(1, dtype=torch.int32)

    def switch(q=q, mask=m, dense=dense, n=32, geo=geo, **kw):
        return _core.svg1_attention_device_switch(q, q, q, geo, mask, dense, prof, n, S, flag, **kw)

    def sparse(q=q, mask=m, n=32, geo=geo, **kw):
        return _core.svg1_sparse_attention(q, q, q, geo, mask, prof, n, S, **kw)

    q2 = torch.zeros(2, 2, S, 128, dtype=torch.bfloat16)
    for call in (switch, sparse):
        with pytest.raises(NotImplementedError, match="ONE mask"):
            call(q=q2, mask=(m, m2))
        with pytest.raises(ValueError, match="plain q"):
            call(q_prescaled=True)
        with pytest.raises(NotImplementedError, match="returns o only"):
            call(return_lse=True)
        with pytest.raises(NotImplementedError, match="bfloat16"):
            call(q=q.half())
        with pytest.raises(NotImplementedError, match="head_dim 128"):
            call(q=q[..., :64])
        with pytest.raises(NotImplementedError, match="at most 64 rows"):
            call(n=65)
        with pytest.raises(NotImplementedError, match="in front of"):
            call(geo=_core.Geometry(24, 7, 80, text_first=True))
        monkeypatch.setattr(_core, "_ATTENTION_DTYPE", {"value": "fp8"})
        with pytest.raises(NotImplementedError, match="fp8"):
            call()
        monkeypatch.setattr(_core, "_ATTENTION_DTYPE", {"value": "bf16"})
        monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 9)
        with pytest.raises(ValueError, match="at most 8 parts"):
            call()
        monkeypatch.undo()
        _no_collectives(monkeypatch)
        with pytest.raises(RuntimeError, match="no CPU fallback"):     # everything else passed: only the device is missing
            call()
    with pytest.raises(NotImplementedError, match="ONE mask"):
        switch(q=q2, dense=(dense, _dense(S, 590)))
    with pytest.raises(NotImplementedError, match="fused path"):
        sparse(fused=False)
    # dense_attention: the geometry is required in this mode, and ignored outside it
    with pytest.raises(ValueError, match="needs geometry="):
        _core.dense_attention(q, q, q)
    with pytest.raises(NotImplementedError, match="ONE valid_len"):
        _core.dense_attention(q2, q2, q2, (597, 590), geometry=geo)
    with pytest.raises(ValueError, match="plain q"):
        _core.dense_attention(q, q, q, q_prescaled=True, geometry=geo)
    with pytest.raises(NotImplementedError, match="returns o only"):
        _core.dense_attention(q, q, q, return_lse=True, geometry=geo)
    with pytest.raises(NotImplementedError, match="bfloat16 / torch.float16"):
        _core.dense_attention(q.float(), q.float(), q.float(), geometry=geo)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _core.dense_attention(q.half(), q.half(), q.half(), 597, geometry=geo)      # (fp16 is fine without the profiler)
    sd.disable()
    small = torch.zeros(1, 2, 16, 8)
    assert _core.dense_attention(small, small, small, geometry=geo).shape == small.shape   # outside the mode: ignored, the SDPA branch


def test_processors_take_the_rows_of_their_shard_or_refuse(one_rank_group, monkeypatch):
    from svg.models import _core
    from svg.models.cog.attention import CogVideoX_SparseAttn_Processor2_0
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor, Cosmos_SVG_AttnProcessor2_0
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0, Hunyuan_SVGAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor, WanAttn_SVGAttn_Processor2_0

    sd = one_rank_group
    geo = _core.Geometry(0, 7, 80)
    assert _core.rows_of_this_rank("x", geo) == 560 and _core.rows_of_this_rank("x", geo, shard_form=False) == 560
    sd.enable_frame_shards()
    _no_collectives(monkeypatch)
    # three ranks: 3 / 2 / 2 frames, the rows behind the video on the last
    hy = _core.Geometry(64, 7, 80)
    for rank, want in ((0, 240), (1, 160), (2, 160 + 64)):
        monkeypatch.setattr(sd.dist, "get_rank", lambda group=None, r=rank: r)
        monkeypatch.setattr(sd.dist, "get_world_size", lambda group=None: 3)
        assert _core.rows_of_this_rank("x", hy) == want
    monkeypatch.undo()
    _no_collectives(monkeypatch)
    assert WanAttn_SVGAttn_Processor2_0.frame_shard_form and Hunyuan_SVGAttn_Processor2_0.frame_shard_form
    x = torch.zeros(1, 2, 16, 128, dtype=torch.bfloat16)
    t = torch.tensor([500.0])
    for proc, args in ((WanAttn_SAPAttn_Processor(0), (x, x, x, t)), (Cosmos_SVG_AttnProcessor2_0(0), (x, x, x, t)),
                       (Cosmos_SAPAttn_Processor(0), (x, x, x, t)), (CogVideoX_SparseAttn_Processor2_0(0), (x, x, x, t)),
                       (Hunyuan_SAPAttn_Processor2_0(0), (x, x, x, t, 0, None))):
        with pytest.raises(NotImplementedError, match="SVG1 processors of HunyuanVideo and Wan only"):
            proc.attention_core_logic(*args)
    # the Wan SVG1 processor: rows that are not this rank's shard are refused by the shape check, as before
    monkeypatch.setattr(WanAttn_SVGAttn_Processor2_0, "num_frame", 7)
    monkeypatch.setattr(WanAttn_SVGAttn_Processor2_0, "frame_size", 80)
    with pytest.raises(AssertionError, match="Query Shape"):
        WanAttn_SVGAttn_Processor2_0(0).attention_core_logic(x, x, x, t)
