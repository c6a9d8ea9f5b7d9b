"""Rejected calls of svg_band_groups_attention, as rows (id, (entry point, arguments), expected code) in the manner of
tests/test_entry_validation_cpu.py; tests/test_band_groups_cpu.py runs them.  Every check of the entry
runs on the host, for ALL groups, before the first launch: the pointers are placeholders and a row that got past validation would fail
with another code (on a machine without a GPU) instead of returning the one pinned here."""
import ctypes as C

from svg import _native as nat

BAD_ARG, UNSUPPORTED = -1, -2
PH = 0x10000          # placeholder device pointer (16-byte aligned; never dereferenced by a call that is rejected)
S_ROWS = 1 << 24      # the row bound of every band entry


def mask(S, **kw):
    m = nat.BandMask(S, 0, 0, 0, 0, 0)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def layout(H=2, S=256, row=128, **kw):
    ts = [nat.TensorStrides(H * S * row, S * row, row) for _ in range(4)]
    lay = nat.AttnLayout(H, 0, *ts)
    for k, v in kw.items():
        setattr(lay, k, v)
    return lay


def groups(q=PH, o=PH, BH=6, S=256, D=128, dtype=0, masks="ok", alts=None, heads=(2, 4), n=None, perm=None, flag=None, pre=0, lay=None):
    """argument list of svg_band_groups_attention (positional, as include/svg_attn.h declares it); masks / alts: lists of BandMask, None
    for a NULL pointer; heads: the host array, None for NULL"""
    n = (len(heads) if heads is not None else 1) if n is None else n
    if masks == "ok":
        masks = [mask(S) for _ in range(max(n, 1))]
    marr = None if masks is None else (nat.BandMask * len(masks))(*masks)
    aarr = None if alts is None else (nat.BandMask * len(alts))(*alts)
    garr = None if heads is None else (C.c_int32 * max(len(heads), 1))(*heads)
    return ("svg_band_groups_attention", [q, PH, PH, o, BH, S, D, dtype, 1.0, marr, aarr, garr, n, C.byref(perm) if perm is not None else None,
                                          flag, pre, C.byref(lay) if lay is not None else None, None])


def dense(S, n=2):
    return [mask(S, band=S + 1) for _ in range(n)]


GROUP_CASES = [
    # pointers and counts
    ("groups/null_q", groups(q=None), BAD_ARG),
    ("groups/null_o", groups(o=None), BAD_ARG),
    ("groups/null_masks", groups(masks=None), BAD_ARG),
    ("groups/null_group_heads", groups(heads=None, n=2), BAD_ARG),
    ("groups/n_groups0", groups(n=0), BAD_ARG),
    ("groups/n_groups_neg", groups(n=-1), BAD_ARG),
    ("groups/BH0", groups(BH=0, heads=(0,)), BAD_ARG),
    ("groups/S0", groups(S=0, masks=[mask(1), mask(1)]), BAD_ARG),
    ("groups/group_heads0", groups(heads=(6, 0)), BAD_ARG),
    ("groups/group_heads_neg", groups(heads=(8, -2)), BAD_ARG),
    ("groups/sum_lt_BH", groups(heads=(2, 3)), BAD_ARG),
    ("groups/sum_gt_BH", groups(heads=(4, 4)), BAD_ARG),
    # masks: every group is checked before the first launch — a bad mask in the LAST group must not follow a launch of the first
    ("groups/bad_mask_first", groups(masks=[mask(256, real_len=257), mask(256)]), BAD_ARG),
    ("groups/bad_mask_last", groups(masks=[mask(256), mask(256, real_len=257)]), BAD_ARG),
    ("groups/bad_mask_last_of_three", groups(heads=(2, 2, 2), masks=[mask(256), mask(256), mask(256, band=258)]), BAD_ARG),
    ("groups/colfull_inverted_last", groups(masks=[mask(256), mask(256, colfull_lo=5, colfull_hi=4)]), BAD_ARG),
    ("groups/bad_perm", groups(perm=nat.PermDesc(PH, 10, 4, 64)), BAD_ARG),
    # device switch: both or neither
    ("groups/alt_without_flag", groups(alts=dense(256)), BAD_ARG),
    ("groups/flag_without_alt", groups(flag=PH), BAD_ARG),
    ("groups/bad_alt_last", groups(alts=[mask(256, band=257), mask(256, band=500)], flag=PH), BAD_ARG),
    ("groups/bad_alt_last_prescaled", groups(alts=[mask(256, band=257), mask(256, real_len=-1)], flag=PH, pre=1), BAD_ARG),
    # strided tensors: whole videos per group
    ("groups/layout_part_of_a_video", groups(heads=(2, 4), lay=layout(H=4)), BAD_ARG),
    ("groups/layout_part_of_a_video_last", groups(heads=(4, 2), lay=layout(H=4)), BAD_ARG),
    ("groups/layout_heads0", groups(lay=layout(heads_per_batch=0)), BAD_ARG),
    ("groups/layout_bad_mask_last", groups(masks=[mask(256), mask(256, rowfull_lo=2, rowfull_hi=1)], lay=layout()), BAD_ARG),
    ("groups/layout_row_lt_D", groups(lay=layout(row=64)), BAD_ARG),
    # what the single-mask entries do not have
    ("groups/layout_row_unaligned", groups(lay=layout(row=132)), UNSUPPORTED),
    ("groups/prescaled_with_layout", groups(pre=1, lay=layout()), UNSUPPORTED),
    ("groups/switch_prescaled_with_layout", groups(alts=dense(256), flag=PH, pre=1, lay=layout()), UNSUPPORTED),
    ("groups/dtype_f32", groups(dtype=2), UNSUPPORTED),
    ("groups/D96", groups(D=96), UNSUPPORTED),
    ("groups/D256_prescaled", groups(D=256, pre=1), UNSUPPORTED),
    ("groups/switch_D96", groups(D=96, alts=dense(256), flag=PH), UNSUPPORTED),
    ("groups/layout_D96", groups(D=96, lay=layout(row=96)), UNSUPPORTED),
    ("groups/rows_D128", groups(S=S_ROWS), UNSUPPORTED),
    ("groups/rows_D64", groups(S=S_ROWS, D=64), UNSUPPORTED),
    ("groups/one_group_D96", groups(heads=(6,), D=96), UNSUPPORTED),
    ("groups/one_group_bad_mask", groups(heads=(6,), masks=[mask(256, band=-1)]), BAD_ARG),
]
