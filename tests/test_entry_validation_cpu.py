"""Argument validation of every attention / profiler entry point, pinned as a table: each row is one rejected call and the error
code it must return (include/svg_attn.h).  Every check runs on the host before any launch, so on a machine without a GPU a row that
would get past validation fails with another code instead of running a kernel.  Rows that pass non-null placeholder pointers are
skipped where a GPU is visible: a regression in validation must never launch a kernel on a bogus address."""
import ctypes as C

import pytest
import torch

from svg import _native as nat

BAD_ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
BIG = 1 << 62         # workspace / counter sizes that pass every size check
S_ROWS = 1 << 24      # the row bound: the LDS-DMA row offset is __umul24(row, row stride in bytes)


def mask(S, **kw):
    m = nat.BandMask(S, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def perm(**kw):
    p = nat.PermDesc(PH, 0, 1, 1)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def layout(H=1, row=128, **kw):
    ts = [nat.TensorStrides(H * 256 * row, 256 * row, row) for _ in range(4)]
    lay = nat.AttnLayout(H, 0, *ts)
    for k, v in kw.items():
        setattr(lay, k, v)
    return lay


def prof(frame_size=64, coord=0):
    d = nat.ProfileDesc(0, 4, frame_size, 0)
    for i in range(2):
        d.variant[i].coord = coord
    return d


def ref(x):
    return C.byref(x) if x is not None else None


# ---- argument lists (positional, as include/svg_attn.h declares them) -------------------------------------------------------------
def band(q=PH, o=PH, BH=2, S=256, D=128, dtype=0, m="ok", p=None, variant=0):
    m = mask(S) if m == "ok" else m
    return ("svg_band_attention", [q, PH, PH, o, BH, S, D, dtype, 1.0, ref(m), ref(p), variant, None])


def band_strided(S=256, D=128, dtype=0, m="ok", lay="ok"):
    m = mask(S) if m == "ok" else m
    lay = layout(row=D) if lay == "ok" else lay
    return ("svg_band_attention_strided", [PH, PH, PH, PH, 2, S, D, dtype, 1.0, ref(m), None, ref(lay), None])


def prescaled(q=PH, S=256, D=128, dtype=0, m="ok", p=None):
    m = mask(S) if m == "ok" else m
    return ("svg_band_attention_prescaled", [q, PH, PH, PH, 2, S, D, dtype, ref(m), ref(p), None])


def notify(done=PH, words=BIG, S=256, D=128, dtype=0, m="ok"):
    m = mask(S) if m == "ok" else m
    return ("svg_band_attention_notify", [PH, PH, PH, PH, 2, S, D, dtype, 1.0, ref(m), None, done, min(words, 1 << 30), None])


def notify_seg(done=PH, words=1 << 30, nseg=2, S=256, D=128, dtype=0, m="ok", pre=False):
    m = mask(S) if m == "ok" else m
    if pre:
        return ("svg_band_attention_prescaled_notify_seg", [PH, PH, PH, PH, 2, S, D, dtype, ref(m), None, done, words, nseg, None])
    return ("svg_band_attention_notify_seg", [PH, PH, PH, PH, 2, S, D, dtype, 1.0, ref(m), None, done, words, nseg, None])


def switch(S=256, D=128, dtype=0, m="ok", alt="ok", flag=PH, p=None, form="", lay="ok"):
    m = mask(S) if m == "ok" else m
    alt = mask(S, band=S + 1) if alt == "ok" else alt
    if form == "prescaled":
        return ("svg_band_attention_switch_prescaled", [PH, PH, PH, PH, 2, S, D, dtype, ref(m), ref(p), ref(alt), flag, None])
    args = [PH, PH, PH, PH, 2, S, D, dtype, 1.0, ref(m), ref(p), ref(alt), flag]
    if form == "strided":
        lay = layout(row=D) if lay == "ok" else lay
        return ("svg_band_attention_switch_strided", args + [ref(lay), None])
    return ("svg_band_attention_switch", args + [None])


def fp8(ws=PH, ws_bytes=BIG, S=256, D=128, dtype=0, m="ok", p=None, stage=None):
    m = mask(S) if m == "ok" else m
    args = [PH, PH, PH, PH, 2, S, D, dtype, 1.0, ref(m), ref(p), ws, ws_bytes]
    if stage is not None:
        return ("svg_band_attention_fp8_stage", args + [stage, None])
    return ("svg_band_attention_fp8", args + [None])


def varblock(q=PH, Hq=4, Hkv=2, Sq=4096, Skv=4096, D=128, dtype=0, QB=16, KB=16, ws_bytes=BIG, variant=-1, form="", lay="ok"):
    args = [q, PH, PH, PH, Hq, Hkv, Sq, Skv, D, dtype, 1.0, PH, PH, PH, QB, KB, None, None, PH, ws_bytes]
    if form == "fp8":
        return ("svg_varblock_attention_fp8", args + [None])
    if form == "strided":
        lay = layout(H=Hq, row=D, kv_heads_per_batch=Hkv) if lay == "ok" else lay
        return ("svg_varblock_attention_strided", args + [ref(lay), None])
    return ("svg_varblock_attention", args + [variant, None])


def sample_mse(rows=PH, R=16, S=1024, D=128, dtype=0, ws_bytes=BIG, pd="ok", form="", lay="ok"):
    pd = prof() if pd == "ok" else pd
    args = [PH, PH, PH, rows, R, 2, S, D, dtype, 1.0, ref(pd), PH, PH, ws_bytes]
    if form == "flagged":
        return ("svg_sample_mse_flagged", args + [None, None])
    if form == "strided":
        lay = layout(row=D) if lay == "ok" else lay
        return ("svg_sample_mse_strided", args + [None, ref(lay), None])
    return ("svg_sample_mse", args + [None])


# ---- the table: (id, call, expected code) ---------------------------------------------------------------------------------------
CASES = [
    # svg_band_attention
    ("band/null_q", band(q=None), BAD_ARG),
    ("band/null_o", band(o=None), BAD_ARG),
    ("band/null_mask", band(m=None), BAD_ARG),
    ("band/BH0", band(BH=0), BAD_ARG),
    ("band/S0", band(S=0, m=mask(1)), BAD_ARG),
    ("band/real_len_gt_S", band(m=mask(256, real_len=257)), BAD_ARG),
    ("band/real_len_neg", band(m=mask(256, real_len=-1)), BAD_ARG),
    ("band/band_gt_S1", band(m=mask(256, band=258)), BAD_ARG),
    ("band/colfull_inverted", band(m=mask(256, colfull_lo=5, colfull_hi=4)), BAD_ARG),
    ("band/rowfull_inverted", band(m=mask(256, rowfull_lo=5, rowfull_hi=4)), BAD_ARG),
    ("band/perm_frames0", band(p=perm(num_frame=0)), BAD_ARG),
    ("band/perm_vid0_neg", band(p=perm(vid0=-1)), BAD_ARG),
    ("band/perm_past_S", band(p=perm(vid0=10, num_frame=4, frame_size=64)), BAD_ARG),
    ("band/variant5", band(variant=5), BAD_ARG),
    ("band/variant7", band(variant=7), BAD_ARG),
    ("band/variant5_bad_dtype", band(variant=5, dtype=7), BAD_ARG),
    ("band/variant5_D96", band(variant=5, D=96), BAD_ARG),
    ("band/dtype_f32", band(dtype=2), UNSUPPORTED),
    ("band/D96", band(D=96), UNSUPPORTED),
    ("band/lockstep_D96", band(D=96, variant=1), UNSUPPORTED),
    ("band/m16_D64", band(D=64, variant=8), UNSUPPORTED),
    ("band/frozen_f16", band(dtype=1, variant=6), UNSUPPORTED),
    ("band/frozen_D64", band(D=64, variant=6), UNSUPPORTED),
    ("band/w4_bad_dtype", band(dtype=2, variant=3), UNSUPPORTED),
    ("band/trace_product", band(variant=64), UNSUPPORTED),
    ("band/w4_trace_product", band(variant=32), UNSUPPORTED),
    ("band/elements_2e40", band(BH=1 << 20, S=8192), UNSUPPORTED),
    ("band/dma_D128", band(S=S_ROWS), UNSUPPORTED),
    ("band/rows_D64", band(S=S_ROWS, D=64), UNSUPPORTED),
    ("band/rows_D64_max", band(S=(1 << 25) - 1, D=64), UNSUPPORTED),
    # svg_band_attention_strided
    ("strided/null_layout", band_strided(lay=None), BAD_ARG),
    ("strided/null_layout_rows", band_strided(lay=None, S=S_ROWS, D=64), UNSUPPORTED),
    ("strided/bad_mask", band_strided(m=mask(256, band=300)), BAD_ARG),
    ("strided/heads0", band_strided(lay=layout(heads_per_batch=0)), BAD_ARG),
    ("strided/row_lt_D", band_strided(lay=layout(row=64)), BAD_ARG),
    ("strided/row_unaligned", band_strided(lay=layout(row=132)), UNSUPPORTED),
    ("strided/D96", band_strided(D=96, lay=layout(row=96)), UNSUPPORTED),
    ("strided/rows_D64", band_strided(S=S_ROWS, D=64, lay=layout(row=64)), UNSUPPORTED),
    # svg_band_attention_prescaled
    ("prescaled/null_q", prescaled(q=None), BAD_ARG),
    ("prescaled/null_mask", prescaled(m=None), BAD_ARG),
    ("prescaled/bad_mask", prescaled(m=mask(256, real_len=300)), BAD_ARG),
    ("prescaled/bad_perm", prescaled(p=perm(frame_size=0)), BAD_ARG),
    ("prescaled/dtype", prescaled(dtype=2), UNSUPPORTED),
    ("prescaled/D96", prescaled(D=96), UNSUPPORTED),
    ("prescaled/rows_D64", prescaled(S=S_ROWS, D=64), UNSUPPORTED),
    # svg_band_attention_notify / notify_seg / prescaled_notify_seg
    ("notify/null_done", notify(done=None), BAD_ARG),
    ("notify/null_done_rows", notify(done=None, S=S_ROWS, D=64), BAD_ARG),
    ("notify/small_counters", notify(words=3), WORKSPACE),
    ("notify/small_counters_bad_mask", notify(words=3, m=mask(256, band=-1)), BAD_ARG),
    ("notify/dtype", notify(dtype=2), UNSUPPORTED),
    ("notify/rows_D64", notify(S=S_ROWS, D=64), UNSUPPORTED),
    ("notify_seg/nseg0", notify_seg(nseg=0), BAD_ARG),
    ("notify_seg/null_done", notify_seg(done=None), BAD_ARG),
    ("notify_seg/small_counters", notify_seg(words=5), WORKSPACE),
    ("notify_seg/bad_mask", notify_seg(m=mask(256, colfull_lo=1, colfull_hi=0)), BAD_ARG),
    ("notify_seg/D96", notify_seg(D=96), UNSUPPORTED),
    ("notify_seg/rows_D64", notify_seg(S=S_ROWS, D=64), UNSUPPORTED),
    ("prescaled_notify_seg/nseg0", notify_seg(nseg=0, pre=True), BAD_ARG),
    ("prescaled_notify_seg/null_done", notify_seg(done=None, pre=True), BAD_ARG),
    ("prescaled_notify_seg/small_counters", notify_seg(words=5, pre=True), WORKSPACE),
    ("prescaled_notify_seg/bad_mask", notify_seg(m=mask(256, rowfull_lo=1, rowfull_hi=0), pre=True), BAD_ARG),
    ("prescaled_notify_seg/dtype", notify_seg(dtype=2, pre=True), UNSUPPORTED),
    ("prescaled_notify_seg/rows_D64", notify_seg(S=S_ROWS, D=64, pre=True), UNSUPPORTED),
    # svg_band_attention_switch / _strided / _prescaled
    ("switch/null_alt", switch(alt=None), BAD_ARG),
    ("switch/null_flag", switch(flag=None), BAD_ARG),
    ("switch/null_alt_rows", switch(alt=None, S=S_ROWS, D=64), BAD_ARG),
    ("switch/null_mask", switch(m=None), BAD_ARG),
    ("switch/bad_mask", switch(m=mask(256, real_len=-3)), BAD_ARG),
    ("switch/bad_alt", switch(alt=mask(256, band=500)), BAD_ARG),
    ("switch/bad_perm", switch(p=perm(num_frame=-1)), BAD_ARG),
    ("switch/dtype", switch(dtype=2), UNSUPPORTED),
    ("switch/D96", switch(D=96), UNSUPPORTED),
    ("switch/rows_D64", switch(S=S_ROWS, D=64), UNSUPPORTED),
    ("switch/rows_D64_bad_alt", switch(S=S_ROWS, D=64, alt=mask(S_ROWS, band=S_ROWS + 2)), UNSUPPORTED),
    ("switch_strided/null_layout", switch(form="strided", lay=None), BAD_ARG),
    ("switch_strided/null_layout_rows", switch(form="strided", lay=None, S=S_ROWS, D=64), BAD_ARG),
    ("switch_strided/null_alt", switch(form="strided", alt=None), BAD_ARG),
    ("switch_strided/bad_alt", switch(form="strided", alt=mask(256, real_len=999)), BAD_ARG),
    ("switch_strided/heads0", switch(form="strided", lay=layout(heads_per_batch=0)), BAD_ARG),
    ("switch_strided/row_unaligned", switch(form="strided", lay=layout(row=132)), UNSUPPORTED),
    ("switch_strided/D96", switch(form="strided", D=96, lay=layout(row=96)), UNSUPPORTED),
    ("switch_strided/rows_D64", switch(form="strided", S=S_ROWS, D=64, lay=layout(row=64)), UNSUPPORTED),
    ("switch_prescaled/null_alt", switch(form="prescaled", alt=None), BAD_ARG),
    ("switch_prescaled/null_flag", switch(form="prescaled", flag=None), BAD_ARG),
    ("switch_prescaled/bad_mask", switch(form="prescaled", m=mask(256, band=-2)), BAD_ARG),
    ("switch_prescaled/bad_alt", switch(form="prescaled", alt=mask(256, colfull_lo=3, colfull_hi=1)), BAD_ARG),
    ("switch_prescaled/bad_perm", switch(form="prescaled", p=perm(vid0=250, frame_size=16)), BAD_ARG),
    ("switch_prescaled/dtype", switch(form="prescaled", dtype=2), UNSUPPORTED),
    ("switch_prescaled/D96", switch(form="prescaled", D=96), UNSUPPORTED),
    ("switch_prescaled/rows_D64", switch(form="prescaled", S=S_ROWS, D=64), UNSUPPORTED),
    # svg_band_attention_fp8 / _stage
    ("fp8/null_ws", fp8(ws=None), BAD_ARG),
    ("fp8/null_mask", fp8(m=None), BAD_ARG),
    ("fp8/S0", fp8(S=0, m=mask(1)), BAD_ARG),
    ("fp8/D64", fp8(D=64), UNSUPPORTED),
    ("fp8/D64_bad_mask", fp8(D=64, m=mask(256, band=-1)), UNSUPPORTED),
    ("fp8/bad_mask", fp8(m=mask(256, real_len=257)), BAD_ARG),
    ("fp8/bad_perm", fp8(p=perm(num_frame=0)), BAD_ARG),
    ("fp8/small_ws", fp8(ws_bytes=1024), WORKSPACE),
    ("fp8/small_ws_bad_perm", fp8(ws_bytes=1024, p=perm(vid0=-1)), BAD_ARG),
    ("fp8/dtype", fp8(dtype=2), UNSUPPORTED),
    ("fp8/rows", fp8(S=S_ROWS), UNSUPPORTED),
    ("fp8_stage/stage0", fp8(stage=0), BAD_ARG),
    ("fp8_stage/stage3", fp8(stage=3), BAD_ARG),
    ("fp8_stage/small_ws", fp8(stage=1, ws_bytes=1024), WORKSPACE),
    ("fp8_stage/dtype", fp8(stage=2, dtype=2), UNSUPPORTED),
    ("fp8_stage/rows", fp8(stage=1, S=S_ROWS), UNSUPPORTED),
    # svg_varblock_attention / _strided / _fp8
    ("varblock/null_q", varblock(q=None), BAD_ARG),
    ("varblock/Hq0", varblock(Hq=0), BAD_ARG),
    ("varblock/Hq_not_multiple", varblock(Hq=3), BAD_ARG),
    ("varblock/QB0", varblock(QB=0), BAD_ARG),
    ("varblock/KB_max", varblock(KB=4033), UNSUPPORTED),
    ("varblock/small_ws", varblock(ws_bytes=64), WORKSPACE),
    ("varblock/variant10", varblock(variant=10), BAD_ARG),
    ("varblock/variant_neg2", varblock(variant=-2), BAD_ARG),
    ("varblock/variant10_bad_dtype", varblock(variant=10, dtype=5), BAD_ARG),
    ("varblock/dtype", varblock(dtype=2), UNSUPPORTED),
    ("varblock/D96", varblock(D=96), UNSUPPORTED),
    ("varblock/D96_variant3", varblock(D=96, variant=3), UNSUPPORTED),
    ("varblock/dma_Skv_D128", varblock(Skv=S_ROWS), UNSUPPORTED),
    ("varblock/rows_Sq_D64", varblock(Sq=S_ROWS, D=64), UNSUPPORTED),
    ("varblock/rows_Skv_D64", varblock(Skv=S_ROWS, D=64), UNSUPPORTED),
    ("varblock/rows_Skv_D64_small_ws", varblock(Skv=S_ROWS, D=64, ws_bytes=64), UNSUPPORTED),
    ("varblock_strided/null_layout", varblock(form="strided", lay=None), BAD_ARG),
    ("varblock_strided/small_ws", varblock(form="strided", ws_bytes=64), WORKSPACE),
    ("varblock_strided/heads_mismatch", varblock(form="strided", lay=layout(H=4, kv_heads_per_batch=1)), BAD_ARG),
    ("varblock_strided/small_blocks", varblock(form="strided", Sq=1024, QB=16), UNSUPPORTED),
    ("varblock_strided/dtype", varblock(form="strided", dtype=2), UNSUPPORTED),
    ("varblock_strided/rows_D64", varblock(form="strided", Skv=S_ROWS, D=64, lay=layout(H=4, row=64, kv_heads_per_batch=2)),
     UNSUPPORTED),
    ("varblock_fp8/null_q", varblock(form="fp8", q=None), BAD_ARG),
    ("varblock_fp8/Hq_not_multiple", varblock(form="fp8", Hq=3), BAD_ARG),
    ("varblock_fp8/D64", varblock(form="fp8", D=64), UNSUPPORTED),
    ("varblock_fp8/QB_max", varblock(form="fp8", QB=32768), UNSUPPORTED),
    ("varblock_fp8/small_ws", varblock(form="fp8", ws_bytes=64), WORKSPACE),
    ("varblock_fp8/dtype", varblock(form="fp8", dtype=2), UNSUPPORTED),
    ("varblock_fp8/rows_Skv", varblock(form="fp8", Skv=S_ROWS), UNSUPPORTED),
    ("varblock_fp8/rows_Sq", varblock(form="fp8", Sq=S_ROWS), UNSUPPORTED),
    # svg_sample_mse / _flagged / _strided
    ("sample_mse/null_rows", sample_mse(rows=None), BAD_ARG),
    ("sample_mse/null_desc", sample_mse(pd=None), BAD_ARG),
    ("sample_mse/R0", sample_mse(R=0), BAD_ARG),
    ("sample_mse/R_max", sample_mse(R=65), UNSUPPORTED),
    ("sample_mse/one_wrap", sample_mse(pd=prof(frame_size=32, coord=1)), UNSUPPORTED),
    ("sample_mse/small_ws", sample_mse(ws_bytes=64), WORKSPACE),
    ("sample_mse/dtype", sample_mse(dtype=2), UNSUPPORTED),
    ("sample_mse/D96", sample_mse(D=96), UNSUPPORTED),
    ("sample_mse/rows_D64", sample_mse(S=S_ROWS, D=64), UNSUPPORTED),
    ("sample_mse/rows_D128", sample_mse(S=S_ROWS), UNSUPPORTED),
    ("sample_mse_flagged/small_ws", sample_mse(form="flagged", ws_bytes=64), WORKSPACE),
    ("sample_mse_flagged/rows_D64", sample_mse(form="flagged", S=S_ROWS, D=64), UNSUPPORTED),
    ("sample_mse_strided/null_layout", sample_mse(form="strided", lay=None), BAD_ARG),
    ("sample_mse_strided/heads0", sample_mse(form="strided", lay=layout(heads_per_batch=0)), BAD_ARG),
    ("sample_mse_strided/D96", sample_mse(form="strided", D=96, lay=layout(row=96)), UNSUPPORTED),
    ("sample_mse_strided/rows_D64", sample_mse(form="strided", S=S_ROWS, D=64, lay=layout(row=64)), UNSUPPORTED),
]


def _uses_placeholder(args):
    return any(a == PH for a in args)


@pytest.mark.parametrize("call,expected", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_entry_point_rejects(call, expected):
    name, args = call
    if _uses_placeholder(args) and torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")
    lib = nat.load()
    assert getattr(lib, name)(*args) == expected


def test_table_covers_every_attention_entry_point():
    names = {c[1][0] for c in CASES}
    want = {n for n in nat.SIGNATURES if (n.startswith(("svg_band_attention", "svg_varblock_attention", "svg_sample_mse"))
                                          and not n.endswith(("_bytes", "_target", "_layout")))}
    assert want <= names, want - names
