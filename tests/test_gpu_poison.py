"""Every `_native` wrapper that returns or fills tensors, on poisoned outputs and workspaces (svg._native.poison_allocations; tests/poisoned.py).

One table, TABLE: a row per wrapper and form, at the smallest shapes at which the launch geometry can leave something out (BH no multiple
of 8, S no multiple of 64 / 256, rows behind real_len, windows without a key, empty clusters, zero-length ranges).  A row's run(nat) calls
the wrapper and returns {output name: tensor}; its check(nat, outs) compares them with the reference of the existing test of that entry —
the oracle calls and bounds are those tests' (check_attn, sparse_lse_cases.check_lse, the check_merge of the two merge tests, torch.equal
where the entry is bit-exact): no new tolerance.

  (a) test_do_nothing_library_is_caught: `nat.load` returns a stand-in whose svg_* entries return 0 and touch nothing.  Every output of
      every row must then FAIL assert_fully_written — the wrapper's outputs really come from the poisoned callables, and the checker sees a
      kernel that writes nothing.  Outputs the WRAPPER fills itself by contract (Row.host_filled: the zero / -inf fill of
      varblock_attention without rows_covered) are the exception and must pass even then.  Nothing is launched except fills.
  (b) test_real_library_writes_everything: the same rows on the real library: every output passes assert_fully_written and its check.
      Where a header says an output is not written (the 16-bit o under the _f32 forms, lse without return_lse) the row lists it in
      `absent` and the test asserts that the wrapper does not return it.

In-place entries (rms_norm_forward, layer_norm_forward, the rope entries, qk_norm_rope) allocate nothing: they are rows of (b) against
their oracle, and (a) skips them (Row.in_place).

svg_cross_attention_pair rejects an empty key set (Skv_b <= 0: SVG_ERR_BAD_ARG, csrc/attention_cross.hip), so the pair row runs the
smallest second set there is, one key, and (b) asserts that the empty one is refused.

WORKSPACES.  The switch poisons them too (int32 words read as -1, floats as NaN).  Which region each launch sequence writes before it
reads, from the host code:
  * svg_argsort_labels (csrc/permute.hip): hist [B][nchunks][K] — sort_hist_kernel stores all K words of every (batch, chunk);
    sort_scan_kernel reads them, writes the offsets in place and counts; sort_scatter_kernel reads the offsets.  sorted_idx is written for
    every label in [0, K); a label outside is skipped by contract.
  * svg_kmeans_iter / _assign / _update (csrc/kmeans.hip): csq [B][K] — csq_kernel writes all before kmeans_assign_kernel reads; the
    argsort region behind it as above; shift is cleared by hipMemsetAsync before kmeans_update_kernel's atomic max.  _update alone does not
    touch csq.
  * svg_kmeans_loop[_grouped][_strided]: the iteration scratch as above; t_labels / t_sorted / t_counts / t_shift are written by the
    iteration before kmeans_commit_kernel reads them; the 4 G state words are cleared by hipMemsetAsync first; iteration 0 commits every
    group (stopped flag 0), so labels / sorted_idx / counts are written whole; the work centroid buffer kmeans_select_kernel reads is the
    one state[3G + g] names, written by that iteration's update; n_iters is copied from the state.
  * svg_varblock_attention[_strided|_lse|_lse_f32|_fp8] (csrc/attention_varblock.hip vb_ws): varblock_plan_kernel writes q_off, k_off and
    tile_off (tile_off2 only in the mixed body, which alone reads it); varblock_bitmap_kernel writes every bitmap word;
    varblock_pair_score_kernel takes the remainders from q_sizes in round 0 and from `rem` afterwards — varblock_pair_match_kernel wrote
    all of `rem` and `best` / `partner` rows in round 0; hist is cleared by hipMemsetAsync; varblock_work_kernel writes both words of every
    block-row; varblock_scan_kernel writes order[0]; varblock_scatter_kernel writes entries [0, order[0]), the only ones the body reads
    (order[1] is padding, never read).  The chain order (variant 7) writes its own order[0] and entries.
  * svg_sample_mse* (csrc/profiler.hip): part [3][BH][n_chunks][64][D + 4] — both kernel forms store O, m, l of every sampled row r < R
    for every chunk, chunks without tiles included (m = -inf, l = 0); profile_combine_kernel reads rows < R only ([D + 2], [D + 3] are
    padding) and writes every sq_part word profile_finalize_kernel reads.  With a raised skip flag nothing runs and the wrapper zero-fills.
  * svg_band_attention_fp8 (csrc/attention_f8.hip): amax is cleared by hipMemsetAsync; f8_quantize_kernel writes q8 / k8 / vt8 for all
    S_pad rows (zeros behind S) and the four scale words of every head.  svg_varblock_attention_fp8: amax cleared, q8 / k8 / v8 and the
    scale words written whole by f8_quantize1_kernel; the 512 bytes of slack are never read.
No region is read before it is written; no memset had to be added."""
import contextlib
import functools
from typing import Callable, NamedTuple

import pytest
import torch

import sparse_lse_cases as SC
from oracle import svg_oracle as O
from poisoned import assert_fully_written, load_native, unwritten
from test_gpu_kernels import _centroid_like, _labels_match, _prof_desc, check_attn

pytestmark = pytest.mark.gpu

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NINF = float("-inf")


@pytest.fixture(scope="module")
def nat():
    return load_native()


class Row(NamedTuple):
    name: str
    run: Callable          # run(nat) -> {output name: tensor}
    check: Callable        # check(nat, outs): against the reference of the entry's existing test
    absent: tuple = ()     # outputs the header says are not written: run returns None under these names
    host_filled: tuple = ()   # outputs the wrapper itself fills by contract, whatever the library does
    in_place: bool = False    # nothing allocated: the entry writes the caller's tensors


TABLE = []


def row(name, **kw):
    def deco(fn):
        run, check = fn()
        TABLE.append(Row(name, run, check, **kw))
        return fn
    return deco


def gpu(t):
    return None if t is None else t.cuda()


def flag(x):
    return torch.tensor([x], dtype=torch.int32).cuda()


@contextlib.contextmanager
def queue_cap(nat, cap):
    lib = nat.load()
    assert lib.svg_debug_band_queue_cap(cap) == 0
    try:
        yield
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0


def check_o_lse(dtype, ref, o=None, lse=None, o32=None):
    """o / o32 against check_attn's bounds on the rows that see a key, exact zeros on the others; lse against check_lse"""
    o_ref, lse_ref = ref
    seen = torch.isfinite(lse_ref)
    for t in (o, o32):
        if t is None:
            continue
        tc = t.float().cpu()
        assert torch.equal(tc[~seen], torch.zeros_like(tc[~seen])), "rows without a key: exact zeros"
        if seen.any():
            check_attn(tc[seen], o_ref[seen].float(), dtype)
    if lse is not None:
        assert lse.dtype == F32 and lse.is_contiguous()
        SC.check_lse(lse, lse_ref, dtype)


# =========================================================================================================
# band attention: the sparse_lse_cases geometry (S = 790 / 750, 3 heads; hy and dense2 have rows behind real_len)
# =========================================================================================================
@functools.lru_cache(maxsize=None)
def band_io(model, dtype, D=128):
    if D == 128:
        return SC.band_inputs(model, dtype), SC.band_reference(model, dtype)
    S = SC.band_case(model)[0]
    g = torch.Generator().manual_seed(2)
    qkv = tuple(torch.randn(1, SC.BAND_H, S, D, generator=g).to(dtype) for _ in range(3))
    return qkv, SC.masked_attention_lse(*qkv, SC.band_case(model)[2])


def bmask(nat, model):
    return nat.BandMask(**SC.band_case(model)[1])


def band_row(name, model, dtype=BF16, D=128, cap=None, **kw):
    def build():
        def run(nat):
            (q, k, v), _ = band_io(model, dtype, D)
            with queue_cap(nat, cap) if cap is not None else contextlib.nullcontext():
                return {"o": nat.band_attention(gpu(q), gpu(k), gpu(v), bmask(nat, model), **kw)}

        def check(nat, outs):
            assert outs["o"].dtype == dtype
            check_o_lse(dtype, band_io(model, dtype, D)[1], o=outs["o"])
        return run, check
    row(name)(build)


for _m in SC.BAND_MODELS:
    band_row(f"band/plain/{_m}", _m)
band_row("band/plain/hy/fp16", "hy", F16)
band_row("band/plain/dense2/D64", "dense2", F16, 64)
for _v in (1, 2, 3):
    band_row(f"band/variant{_v}/hy", "hy", variant=_v)
    band_row(f"band/variant{_v}/dense2/D64", "dense2", BF16, 64, variant=_v)
for _cap in (1, 3, 1 << 20):   # svg_debug_band_queue_cap: the work queue with 1 and 3 resident workgroups, and for a launch of one round
    band_row(f"band/queue{_cap}/hy", "hy", cap=_cap)
    band_row(f"band/queue{_cap}/wan", "wan", cap=_cap)
band_row("band/token_major_out/hy", "hy", token_major_out=True)


@row("band/prescaled/hy")
def _():
    from test_gpu_prescaled import LN2, prescale

    def run(nat):
        (q, k, v), _ = band_io("hy", BF16)
        return {"o": nat.band_attention(gpu(prescale(nat, q)), gpu(k), gpu(v), bmask(nat, "hy"), q_prescaled=True)}

    def check(nat, outs):
        (q, k, v), _ = band_io("hy", BF16)
        check_attn(outs["o"], O.masked_attention(prescale(nat, q), k, v, SC.band_case("hy")[2], scale=LN2), BF16)
    return run, check


def proj_views(q, k, v):
    """[B, H, S, D] views of token-major projections ([B, S, H * D]): what the *_strided entries read in place"""
    return tuple(gpu(x.transpose(1, 2).contiguous()).transpose(1, 2) for x in (q, k, v))


@row("band/strided/dense2")
def _():
    def run(nat):
        (q, k, v), _ = band_io("dense2", BF16)
        qv, kv, vv = proj_views(q, k, v)
        assert not qv.is_contiguous()
        return {"o": nat.band_attention(qv, kv, vv, bmask(nat, "dense2")), "o_tm": nat.band_attention(qv, kv, vv, bmask(nat, "dense2"),
                                                                                                      token_major_out=True)}

    def check(nat, outs):
        assert outs["o_tm"].stride(2) == SC.BAND_H * 128   # stored [B, S, H, D]
        for o in outs.values():
            check_o_lse(BF16, band_io("dense2", BF16)[1], o=o)
    return run, check


BEST = torch.tensor([[0, 1, 1]])


@functools.lru_cache(maxsize=None)
def placed_reference(model):
    """float64 (o, lse) of the fused head placement: placement -> attention -> inverse placement (tests/test_gpu_kernels.py
    test_band_attention_fused_placement)"""
    (q, k, v), _ = band_io(model, BF16)
    g = SC.GEOM
    cl, tf = (0 if model == "wan" else g["ctx"]), model == "cog"
    qp, kp, vp = (O.head_placement(x, BEST, cl, g["F_"], g["P_"], text_first=tf) for x in (q, k, v))
    o, lse = SC.masked_attention_lse(qp, kp, vp, SC.band_case(model)[2])
    back = lambda t: O.head_placement(t, BEST, cl, g["F_"], g["P_"], text_first=tf, inverse=True)  # noqa: E731
    return back(o), back(lse[..., None].expand(-1, -1, -1, 2).contiguous())[..., 0]


def perm_kw(model):
    return dict(head_perm_flag=gpu(BEST), vid0=SC.band_case(model)[3], num_frame=SC.GEOM["F_"], frame_size=SC.GEOM["P_"])


for _m in ("hy", "cog"):
    @row(f"band/fused_placement/{_m}")
    def _(model=_m):
        def run(nat):
            (q, k, v), _ = band_io(model, BF16)
            o, lse = nat.band_attention(gpu(q), gpu(k), gpu(v), bmask(nat, model), return_lse=True, **perm_kw(model))
            return {"o": o, "lse": lse, "o_plain": nat.band_attention(gpu(q), gpu(k), gpu(v), bmask(nat, model), **perm_kw(model))}

        def check(nat, outs):
            check_o_lse(BF16, placed_reference(model), o=outs["o"], lse=outs["lse"])
            check_o_lse(BF16, placed_reference(model), o=outs["o_plain"])
        return run, check


def lse_rows(name, call, reference, dtype=BF16):
    """the lse form and the fp32-row form of one launch: (o, lse) and (o32, lse) — no 16-bit o under the _f32 entry"""
    @row(name + "/lse")
    def _():
        def run(nat):
            o, lse = call(nat, {})
            return {"o": o, "lse": lse}

        def check(nat, outs):
            assert outs["o"].dtype == dtype
            check_o_lse(dtype, reference(), o=outs["o"], lse=outs["lse"])
        return run, check

    @row(name + "/lse_f32", absent=("o",))
    def _():
        def run(nat):
            got = call(nat, dict(out_dtype=F32))
            assert len(got) == 2
            return {"o32": got[0], "lse": got[1], "o": None}

        def check(nat, outs):
            assert outs["o32"].dtype == F32 and outs["o32"].is_contiguous()
            check_o_lse(dtype, reference(), o32=outs["o32"], lse=outs["lse"])
        return run, check


for _m in ("hy", "dense2", "wan"):
    lse_rows(f"band/{_m}", lambda nat, kw, m=_m: nat.band_attention(*map(gpu, band_io(m, BF16)[0]), bmask(nat, m), return_lse=True, **kw),
             lambda m=_m: band_io(m, BF16)[1])
lse_rows("band/hy/fp16", lambda nat, kw: nat.band_attention(*map(gpu, band_io("hy", F16)[0]), bmask(nat, "hy"), return_lse=True, **kw),
         lambda: band_io("hy", F16)[1], F16)
lse_rows("band/strided/hy", lambda nat, kw: nat.band_attention(*proj_views(*band_io("hy", BF16)[0]), bmask(nat, "hy"), return_lse=True, **kw),
         lambda: band_io("hy", BF16)[1])

# the device switch: flag 0 -> the hy mask, flag != 0 -> the dense mask over the real rows (the dense2 case on the same inputs)
for _f, _ref in ((0, "hy"), (1, "dense2")):
    @row(f"band/switch/flag{_f}")
    def _(f=_f, ref=_ref):
        def run(nat):
            (q, k, v), _ = band_io("hy", BF16)
            a = (gpu(q), gpu(k), gpu(v), bmask(nat, "hy"), bmask(nat, "dense2"), flag(f))
            return {"o": nat.band_attention_switch(*a), "o_tm": nat.band_attention_switch(*a, token_major_out=True)}

        def check(nat, outs):
            want = SC.masked_attention_lse(*band_io("hy", BF16)[0], SC.band_case(ref)[2])
            for o in outs.values():
                check_o_lse(BF16, want, o=o)
        return run, check

    lse_rows(f"band/switch/flag{_f}", lambda nat, kw, f=_f: nat.band_attention_switch(
        *map(gpu, band_io("hy", BF16)[0]), bmask(nat, "hy"), bmask(nat, "dense2"), flag(f), return_lse=True, **kw),
        lambda ref=_ref: SC.masked_attention_lse(*band_io("hy", BF16)[0], SC.band_case(ref)[2]))


@functools.lru_cache(maxsize=None)
def groups_reference():
    """heads 0, 1 under the hy mask, head 2 under the dense2 mask"""
    q, k, v = band_io("hy", BF16)[0]
    a = SC.masked_attention_lse(q[:, :2], k[:, :2], v[:, :2], SC.band_case("hy")[2])
    b = SC.masked_attention_lse(q[:, 2:], k[:, 2:], v[:, 2:], SC.band_case("dense2")[2])
    return torch.cat([a[0], b[0]], 1), torch.cat([a[1], b[1]], 1)


def groups_call(nat, **kw):
    return nat.band_attention_groups(*map(gpu, band_io("hy", BF16)[0]), [bmask(nat, "hy"), bmask(nat, "dense2")], [2, 1], **kw)


@row("band/groups")
def _():
    def run(nat):
        return {"o": groups_call(nat)}

    def check(nat, outs):
        check_o_lse(BF16, groups_reference(), o=outs["o"])
    return run, check


lse_rows("band/groups", lambda nat, kw: groups_call(nat, return_lse=True, **kw), groups_reference)


# ---- band window: rows x keys of the mask; a row that sees no key of the window: zeros and -inf, STORED ----
def window_rows(model, rows, keys):
    from test_gpu_band_window import run_window, window_reference

    lse_rows(f"band_window/{model}/rows{rows[0]}-{rows[1]}/keys{keys[0]}-{keys[1]}",
             lambda nat, kw: run_window(nat, model, BF16, rows, keys, **kw), lambda: window_reference(model, BF16, rows, keys))


S_WAN, S_HY = SC.band_case("wan")[0], SC.band_case("hy")[0]
window_rows("wan", (0, 256), (640, S_WAN))     # every row without a key
window_rows("wan", (0, 300), (640, S_WAN))     # mixed
window_rows("hy", (300, 601), (256, 700))      # both ends off the tile grid


# =========================================================================================================
# variable-block attention
# =========================================================================================================
@functools.lru_cache(maxsize=None)
def vb_case(kind):
    """-> (q, k, v, bmap, rsz, csz), rows_covered.  small: (4, 4, 256, 10, 50) with one all-False block row and one empty q cluster;
    short: its q sizes sum below S (the wrapper's zero fill is the contract); gqa: (4, 1, 4096, 20, 100)"""
    if kind == "gqa":
        return SC.vb_inputs(SC.VB_CASES[0], BF16), True
    q, k, v, bmap, rsz, csz = SC.vb_inputs(SC.VB_CASES[1], BF16)
    bmap, rsz = bmap.clone(), rsz.clone()
    bmap[:, 3] = False                       # a block row without a key block
    rsz[:, 5] += rsz[:, 6]                   # ... and an empty q cluster (its rows go to the neighbour)
    rsz[:, 6] = 0
    if kind == "short":
        rsz[:, 9] -= torch.minimum(rsz[:, 9] - 1, torch.tensor(7))    # the last rows of every head: no block-row covers them
        assert int(rsz.sum(1).max()) < q.shape[1]
    return (q, k, v, bmap, rsz, csz), kind != "short"


@functools.lru_cache(maxsize=None)
def vb_reference(kind):
    return SC.vb_reference_of(*vb_case(kind)[0])


def vb_call(nat, kind, **kw):
    args, covered = vb_case(kind)
    return nat.varblock_attention(*map(gpu, args), rows_covered=covered, **kw)


for _k in ("small", "gqa", "short"):
    _hf = dict(host_filled=("o",)) if _k == "short" else {}
    for _v in ((-1, 0, 1, 2, 3) if _k == "small" else (-1,)):
        @row(f"varblock/{_k}/variant{_v}", **_hf)
        def _(kind=_k, variant=_v):
            def run(nat):
                return {"o": vb_call(nat, kind, variant=variant)}

            def check(nat, outs):
                check_o_lse(BF16, vb_reference(kind), o=outs["o"])
            return run, check

    @row(f"varblock/{_k}/lse", **(dict(host_filled=("o", "lse")) if _k == "short" else {}))
    def _(kind=_k):
        def run(nat):
            o, lse = vb_call(nat, kind, return_lse=True)
            return {"o": o, "lse": lse}

        def check(nat, outs):
            check_o_lse(BF16, vb_reference(kind), o=outs["o"], lse=outs["lse"])
        return run, check

    @row(f"varblock/{_k}/lse_f32", absent=("o",), **(dict(host_filled=("o32", "lse")) if _k == "short" else {}))
    def _(kind=_k):
        def run(nat):
            got = vb_call(nat, kind, return_lse=True, out_dtype=F32)
            assert len(got) == 2
            return {"o32": got[0], "lse": got[1], "o": None}

        def check(nat, outs):
            assert outs["o32"].dtype == F32
            check_o_lse(BF16, vb_reference(kind), o32=outs["o32"], lse=outs["lse"])
        return run, check


@row("varblock/gqa/token_major_out")
def _():
    def run(nat):
        return {"o": vb_call(nat, "gqa", token_major_out=True)}

    def check(nat, outs):
        check_o_lse(BF16, vb_reference("gqa"), o=outs["o"])
    return run, check


# =========================================================================================================
# cross attention: Sq = 300, Skv = 77
# =========================================================================================================
@functools.lru_cache(maxsize=None)
def cross_io(dtype=BF16):
    g = torch.Generator().manual_seed(300 + 77)
    B, H, Sq, Skv, D = 2, 3, 300, 77, 128
    return tuple(torch.randn(B, H, s, D, generator=g).to(dtype) for s in (Sq, Skv, Skv))


KV_BEGIN, KV_END = torch.tensor([5, 40], dtype=torch.int32), torch.tensor([70, 40], dtype=torch.int32)   # video 1: a window of length 0


@functools.lru_cache(maxsize=None)
def cross_reference(ranged):
    q, k, v = cross_io()
    if not ranged:
        return SC.masked_attention_lse(q, k, v, None)
    col = torch.arange(k.shape[2])
    m = ((col[None] >= KV_BEGIN[:, None]) & (col[None] < KV_END[:, None]))[:, None, None, :]    # [B, 1, 1, Skv]
    return SC.masked_attention_lse(q, k, v, m.expand(-1, 1, q.shape[2], -1))


def cross_call(nat, ranged, **kw):
    q, k, v = map(gpu, cross_io())
    if ranged:
        return nat.cross_attention_keyrange(q, k, v, gpu(KV_END), gpu(KV_BEGIN), **kw)
    return nat.cross_attention(q, k, v, **kw)


for _r, _n in ((False, "cross/plain"), (True, "cross/keyrange_one_empty")):
    @row(_n)
    def _(ranged=_r):
        def run(nat):
            return {"o": cross_call(nat, ranged), "o_tm": cross_call(nat, ranged, token_major_out=True)}

        def check(nat, outs):
            for o in outs.values():
                check_o_lse(BF16, cross_reference(ranged), o=o)
        return run, check

    lse_rows(_n, lambda nat, kw, r=_r: cross_call(nat, r, return_lse=True, **kw), lambda r=_r: cross_reference(r))


@row("cross/pair_one_key_second_set")
def _():
    def sets():
        q, ka, va = cross_io()
        g = torch.Generator().manual_seed(5)
        kb, vb = (torch.randn(2, 3, 1, 128, generator=g).to(BF16) for _ in range(2))
        return q, ka, va, kb, vb

    def run(nat):
        return {"o": nat.cross_attention_pair(*map(gpu, sets())), "o_tm": nat.cross_attention_pair(*map(gpu, sets()), token_major_out=True)}

    def check(nat, outs):
        q, ka, va, kb, vb = map(gpu, sets())
        want = nat.cross_attention(q, ka, va) + nat.cross_attention(q, kb, vb)    # bit for bit (tests/test_gpu_cross_attention_pair.py)
        for o in outs.values():
            assert torch.equal(o, want)
        with pytest.raises(RuntimeError):   # an EMPTY second set is refused, nothing runs
            nat.cross_attention_pair(q, ka, va, kb[:, :, :0], vb[:, :, :0])
    return run, check


# =========================================================================================================
# merge_attention_states: 1, 2, 8 parts; rows where all parts are -inf; 16-bit and fp32 parts; token-major out
# =========================================================================================================
@functools.lru_cache(maxsize=None)
def merge_parts(n, f32):
    """n parts of Sq = 257 rows over 40 keys each (the torch statement's, float64 -> the part dtype); rows [0, 9) of every part: -inf"""
    from lse_ops_torch import attention_lse

    g = torch.Generator().manual_seed(n * 31 + 257)
    B, H, Sq, D = 1, 3, 257, 128
    q = torch.randn(B, H, Sq, D, generator=g).to(BF16)
    o_parts, lse_parts = [], []
    for _ in range(n):
        k, v = (torch.randn(B, H, 40, D, generator=g).to(BF16) for _ in range(2))
        o, lse = attention_lse(q.double(), k.double(), v.double())
        lse[:, :, :9] = NINF
        o_parts.append(o.to(F32 if f32 else BF16))
        lse_parts.append(lse.float())
    return tuple(o_parts), tuple(lse_parts)


for _n in (1, 2, 8):
    for _f32 in (False, True):
        @row(f"merge/{_n}parts/{'fp32' if _f32 else 'bf16'}")
        def _(n=_n, f32=_f32):
            kw = dict(out_dtype=BF16) if f32 else {}

            def run(nat):
                op, lp = ([gpu(t) for t in x] for x in merge_parts(n, f32))
                o, lse = nat.merge_attention_states(op, lp, return_lse=True, **kw)
                return {"o": o, "lse": lse, "o_tm": nat.merge_attention_states(op, lp, token_major_out=True, **kw)}

            def check(nat, outs):
                import test_gpu_attention_f32_parts as F
                import test_gpu_attention_lse as L

                op, lp = merge_parts(n, f32)
                assert outs["o"].dtype == BF16 and (outs["lse"][:, :, :9] == NINF).all()
                if n == 1:    # one part: its bits (fp32: rounded once), the rows without a key as they are (include/svg_attn.h)
                    assert torch.equal(outs["o"].cpu().view(torch.int16), op[0].to(BF16).view(torch.int16)) and torch.equal(outs["lse"].cpu(), lp[0])
                    assert torch.equal(outs["o_tm"], outs["o"]) and outs["o_tm"].stride(2) == 3 * 128
                    return
                assert (outs["o"][:, :, :9] == 0).all()       # all parts -inf: zeros and -inf
                if f32:
                    F.check_merge(outs["o"], outs["lse"], op, lp, BF16, one_ulp=False)
                    F.check_merge(outs["o_tm"], None, op, lp, BF16, one_ulp=False)
                else:
                    L.check_merge(outs["o"], outs["lse"], op, lp, BF16)
                assert torch.equal(outs["o_tm"], outs["o"]) and outs["o_tm"].stride(2) == 3 * 128
            return run, check


# =========================================================================================================
# layout: head_placement, permute_rows, argsort_labels
# =========================================================================================================
for _ctx, _tf in ((0, False), (16, False), (16, True)):
    for _inv in (False, True):
        @row(f"head_placement/ctx{_ctx}/{'text_first/' if _tf else ''}{'inverse' if _inv else 'forward'}")
        def _(ctx=_ctx, tf=_tf, inverse=_inv):
            cfg, H, F_, P_, D = 2, 3, 5, 77, 64

            def data():
                g = torch.Generator().manual_seed(ctx + inverse)
                return [torch.randn(cfg, H, ctx + F_ * P_, D, generator=g).to(BF16) for _ in range(3)], torch.tensor([[0, 1, 1], [1, 0, 1]])

            def run(nat):
                xs, best = data()
                outs = [nat.empty_like(gpu(x)) for x in xs]     # the caller's buffers, allocated as the package's own (svg/models/_core.py)
                nat.head_placement([gpu(x) for x in xs], outs, gpu(best), ctx, F_, P_, tf, inverse)
                return dict(zip("qkv", outs))

            def check(nat, outs):
                xs, best = data()
                for x, o in zip(xs, outs.values()):
                    assert torch.equal(o.cpu(), O.head_placement(x, best, ctx, F_, P_, text_first=tf, inverse=inverse))
            return run, check


for _S, _K in ((1, 3), (257, 9)):
    @row(f"argsort_permute/S{_S}/K{_K}")
    def _(S=_S, K=_K):
        def data():
            g = torch.Generator().manual_seed(S)
            labels = torch.randint(0, K - 2, (3, S), dtype=torch.int32, generator=g)    # labels K - 2, K - 1 never occur: counts 0
            labels[labels == 1] = 0                                                    # ... nor does label 1 where K > 3
            return labels, torch.randn(3, S, 64, generator=g).to(BF16)

        def run(nat):
            labels, x = data()
            sidx, counts = nat.argsort_labels(gpu(labels), K)
            y = nat.permute_rows(gpu(x), sidx) if not unwritten(sidx).any() else nat.permute_rows(gpu(x), torch.zeros_like(sidx))
            return {"sorted_idx": sidx, "counts": counts, "permuted": y, "back": nat.permute_rows(y, torch.zeros_like(sidx) if unwritten(sidx).any()
                                                                                                 else sidx, inverse=True)}

        def check(nat, outs):
            labels, x = data()
            ref_idx = O.stable_argsort(labels.long()).to(torch.int32)
            ref_counts = torch.stack([torch.bincount(l.long(), minlength=K) for l in labels]).int()
            assert (ref_counts == 0).any()
            assert torch.equal(outs["sorted_idx"].cpu(), ref_idx) and torch.equal(outs["counts"].cpu(), ref_counts)
            assert torch.equal(outs["permuted"].cpu(), torch.gather(x, 1, ref_idx.long()[..., None].expand(-1, -1, 64)))
            assert torch.equal(outs["back"].cpu(), x)
        return run, check


# =========================================================================================================
# k-means: N = 3000, K = 40, B = 3, one empty cluster
# =========================================================================================================
@functools.lru_cache(maxsize=None)
def km_io():
    """test_kmeans_iter's data: the last initial centroid far away — an empty cluster that keeps its centroid"""
    B, N, K, D = 3, 3000, 40, 128
    g = torch.Generator().manual_seed(7)
    centers = torch.randn(B, K, D, generator=g) * 2
    x = torch.gather(centers, 1, torch.randint(0, K, (B, N), generator=g)[..., None].expand(-1, -1, D)) + 0.5 * torch.randn(B, N, D, generator=g)
    x = x.to(BF16)
    c0 = x[:, :K].clone()
    c0[:, -1] = 100.0
    return x, c0


def check_km_update(x, c0, lab, cent, counts, sidx, shift):
    """everything downstream of the labels (tests/test_gpu_kernels.py test_kmeans_iter)"""
    assert torch.equal(sidx.cpu(), O.stable_argsort(lab).to(torch.int32))
    c_ref, cnt_ref = O.kmeans_update(x, lab, c0)
    assert torch.equal(counts.cpu(), cnt_ref)
    assert cnt_ref[:, -1].sum() == 0 and torch.equal(cent.cpu()[:, -1], c0[:, -1])
    torch.testing.assert_close(cent.float().cpu(), c_ref.float(), rtol=1e-2, atol=1e-2)
    if shift is not None:
        shift_ref = (c_ref.float() - c0.float()).norm(dim=-1).max(dim=-1).values
        torch.testing.assert_close(shift.cpu(), shift_ref, rtol=2e-2, atol=1e-3)


@row("kmeans/xsq_iter")
def _():
    def run(nat):
        x, c0 = map(gpu, km_io())
        xsq = nat.kmeans_xsq(x)
        buf = nat.KmeansBuffers(*x.shape[:2], c0.shape[1], x.shape[2], x.device)
        c_out = nat.empty_like(c0)
        nat.kmeans_iter(x, xsq, c0, c_out, buf)
        return {"xsq": xsq, "labels": buf.labels, "counts": buf.counts, "sorted_idx": buf.sorted_idx, "shift": buf.shift, "centroids": c_out}

    def check(nat, outs):
        x, c0 = km_io()
        torch.testing.assert_close(outs["xsq"].cpu(), O.kmeans_xsq(x), rtol=1e-2, atol=0)
        lab = outs["labels"].cpu().long()
        _labels_match(x, c0, lab)
        check_km_update(x, c0, lab, outs["centroids"], outs["counts"], outs["sorted_idx"], outs["shift"])
    return run, check


@row("kmeans/assign_update")
def _():
    def run(nat):
        x, c0 = map(gpu, km_io())
        labels = nat.kmeans_assign(x, c0)
        lab = labels if not unwritten(labels).any() else torch.zeros_like(labels)
        cent, counts, sidx, shift = nat.kmeans_update(x, lab, c0)
        return {"labels": labels, "centroids": cent, "counts": counts, "sorted_idx": sidx, "shift": shift}

    def check(nat, outs):
        x, c0 = km_io()
        lab = outs["labels"].cpu().long()
        _labels_match(x, c0, lab)
        check_km_update(x, c0, lab, outs["centroids"], outs["counts"], outs["sorted_idx"], outs["shift"])
    return run, check


def km_loop_row(name, strided=False, group=None):
    @row(name)
    def _():
        def run(nat):
            x, c0 = map(gpu, km_io())
            if strided:    # the video tokens of a longer sequence: batches further apart than N * D
                big = torch.zeros(x.shape[0], x.shape[1] + 56, x.shape[2], dtype=x.dtype, device=x.device)
                big[:, :x.shape[1]] = x
                x = big[:, :x.shape[1]]
                assert not x.is_contiguous()
            labels, cent, counts, n_it, sidx = nat.kmeans_loop(x, None, c0, 1, 1e-4, group=group)
            return {"labels": labels, "centroids": cent, "counts": counts, "n_iters": n_it, "sorted_idx": sidx}

        def check(nat, outs):
            x, c0 = km_io()
            assert outs["n_iters"].cpu().tolist() == (1 if group is None else [1] * (x.shape[0] // group))
            lab = outs["labels"].cpu().long()
            _labels_match(x, c0, lab)                # max_iters 1: the labels of c0, the centroids one update ahead (test_kmeans_loop_vs_oracle)
            check_km_update(x, c0, lab, outs["centroids"], outs["counts"], outs["sorted_idx"], None)
        return run, check


km_loop_row("kmeans/loop")
km_loop_row("kmeans/loop_strided", strided=True)
km_loop_row("kmeans/loop_grouped", group=1)
km_loop_row("kmeans/loop_grouped_strided", strided=True, group=3)


# =========================================================================================================
# block map: identify_dynamic_map (3, 12, 40, 64) with one head whose k_sizes are all 0; map_density; bsr_to_block_map
# =========================================================================================================
@functools.lru_cache(maxsize=None)
def dyn_io():
    qc, kc, ksz = _centroid_like(3, 12, 40, 64, BF16, 9)
    ksz[1] = 0
    return qc, kc, ksz


@row("dynamic_map_density")
def _():
    def run(nat):
        qc, kc, ksz = map(gpu, dyn_io())
        m = nat.identify_dynamic_map(qc, kc, ksz, 0.9, 4)
        mm = m if not unwritten(m).any() else torch.zeros_like(m)
        return {"map": m, "density": nat.map_density(mm, gpu(torch.full((3, 12), 5, dtype=torch.int32)), ksz)}

    def check(nat, outs):
        qc, kc, ksz = dyn_io()
        ref = O.identify_dynamic_map(qc[None], kc[None], None, ksz[None], 0.9, 0.1, exact=True)[0]
        assert torch.equal(outs["map"].cpu().bool(), ref)
        dref = O.density_calculation(ref[None], torch.full((1, 3, 12), 5), ksz[None].long())[0]
        assert torch.isnan(dref[1]) and torch.isfinite(dref[[0, 2]]).all()     # the head without keys: 0 / 0 in the reference, and in the kernel
        torch.testing.assert_close(outs["density"].cpu(), dref.float(), rtol=1e-5, atol=1e-6, equal_nan=True)
    return run, check


@row("bsr_to_block_map")
def _():
    MB, NB, R, Cb, L, heads = 5, 7, 128, 64, 11, 3

    def data():
        g = torch.Generator().manual_seed(57)
        dense = torch.rand(MB, NB, generator=g) < 0.5
        dense[2] = False                                   # a block row without a block
        indptr = torch.cat([torch.zeros(1, dtype=torch.int64), dense.sum(1).cumsum(0)]).to(torch.int32)
        return dense, indptr, dense.nonzero()[:, 1].to(torch.int32)

    def run(nat):
        _, indptr, indices = data()
        bm, qs, ks = nat.bsr_to_block_map(gpu(indptr), gpu(indices), MB, NB, R, Cb, L, heads)
        return {"block_map": bm, "q_sizes": qs, "k_sizes": ks}

    def check(nat, outs):
        dense = data()[0]
        # the statement of the header: the text block in front, attending to everything and attended by everything
        want = torch.ones(MB + 1, NB + 1, dtype=torch.bool)
        want[1:, 1:] = dense
        for h in range(heads):
            assert torch.equal(outs["block_map"][h].cpu().bool(), want)
            assert outs["q_sizes"][h].tolist() == [L] + [R] * MB and outs["k_sizes"][h].tolist() == [L] + [Cb] * NB
    return run, check


# =========================================================================================================
# the online profiler: hy, R = 5 (a chunk's partial rows behind R stay unwritten in the workspace, and are not read)
# =========================================================================================================
@row("sample_mse/hy/R5")
def _():
    F_, P_, ctx, D, H, R = 5, 150, 40, 128, 3, 5

    def data():
        g = torch.Generator().manual_seed(6)
        q, k, v = (torch.randn(1, H, F_ * P_ + ctx, D, generator=g).to(BF16) for _ in range(3))
        return q, k, v, torch.randint(0, F_ * P_, (R,), generator=g)

    def run(nat):
        q, k, v, rows = data()
        qv, kv, vv = proj_views(q, k, v)
        a = (gpu(rows), _prof_desc(nat, "hy", ctx, F_, P_, False))
        return {"mse": nat.sample_mse(gpu(q[0]), gpu(k[0]), gpu(v[0]), *a), "mse_strided": nat.sample_mse(qv[0], kv[0], vv[0], *a),
                "mse_fp16": nat.sample_mse(gpu(q[0].to(F16)), gpu(k[0].to(F16)), gpu(v[0].to(F16)), *a)}

    def check(nat, outs):
        q, k, v, rows = data()
        masks = list(O.profile_masks("hy", ctx, F_, P_))
        ref32 = O.sample_mse_fp32(q, k, v, rows, masks)[:, 0]
        for name in ("mse", "mse_strided"):
            assert outs[name].shape == (2, H)
            torch.testing.assert_close(outs[name].cpu(), ref32, rtol=3e-2, atol=1e-6)      # (tests/test_gpu_kernels.py test_sample_mse)
        ref16 = O.sample_mse_fp32(q.to(F16), k.to(F16), v.to(F16), rows, masks)[:, 0]
        torch.testing.assert_close(outs["mse_fp16"].cpu(), ref16, rtol=3e-2, atol=1e-6)
    return run, check


# =========================================================================================================
# prologue: the transposing forms allocate their outputs; the in-place entries are rows of (b) only
# =========================================================================================================
@row("prologue/qk_norm_rope_transpose")
def _():
    bsz, Hq, Hkv, S, L, D = 2, 6, 3, 533, 40, 128

    def data(nat):
        g = torch.Generator().manual_seed(13)
        q_in, k_in = (gpu(torch.randn(bsz, S, h * D, generator=g).to(BF16)) for h in (Hq, Hkv))
        qw, kw = (gpu(torch.randn(D, generator=g).to(BF16)) for _ in range(2))
        cs, sn = (gpu(torch.randn(S - L, D, generator=g)) for _ in range(2))
        return q_in, k_in, (1, qw, None, kw, None, 1e-6, 1, cs, sn, L, S)

    def run(nat):
        q_in, k_in, args = data(nat)
        q, k = nat.qk_norm_rope_transpose(q_in, k_in, Hq, Hkv, *args)
        v, none = nat.qk_norm_rope_transpose(k_in, None, Hkv, 0)
        assert none is None
        return {"q": q, "k": k, "v": v}

    def check(nat, outs):   # == transpose, then the in-place entry, bit for bit (tests/test_gpu_prologue.py)
        q_in, k_in, args = data(nat)
        q_ref = q_in.unflatten(2, (Hq, D)).transpose(1, 2).contiguous()
        k_ref = k_in.unflatten(2, (Hkv, D)).transpose(1, 2).contiguous()
        assert torch.equal(outs["v"], k_ref)
        nat.qk_norm_rope(q_ref, k_ref, *args)
        assert torch.equal(outs["q"], q_ref) and torch.equal(outs["k"], k_ref)
    return run, check


@row("prologue/joint_zero_length_text")
def _():
    import test_gpu_joint_prologue as J

    H, D, sa = 3, 128, 301

    def data(nat):
        g = torch.Generator().manual_seed(301)
        segs = [J._segment(nat, 2, sa, H, D, BF16, 1, g), J._segment(nat, 2, 0, H, D, BF16, 2, g)]    # a text stream of no rows
        return segs, J._tables(sa - 17, D, 1)

    def run(nat):
        segs, (cos, sin) = data(nat)
        q, k, v = nat.qk_norm_rope_transpose_joint(segs, H, 1, cos, sin, 17, sa, q_scale=nat.softmax_q_scale(D))
        q2, k2, v2 = nat.qk_norm_rope_transpose_joint(segs, H, with_v=False)
        assert v2 is None
        return {"q": q, "k": k, "v": v, "q_plain": q2, "k_plain": k2}

    def check(nat, outs):
        segs, (cos, sin) = data(nat)
        want = J._composition(nat, segs, H, 1, cos, sin, 17, sa, nat.softmax_q_scale(D))
        for n, w in zip("qkv", want):
            assert torch.equal(outs[n].view(torch.int16), w.view(torch.int16)), n
        want = J._composition(nat, segs, H, 0, None, None, 0, 0, 1.0)
        assert torch.equal(outs["q_plain"], want[0]) and torch.equal(outs["k_plain"], want[1])
    return run, check


@row("prologue/rmsnorm_rope_transpose")
def _():
    H, D, bsz, S, lo, hi = 5, 64, 2, 333, 7, 301

    def data():
        g = torch.Generator().manual_seed(H * D + 1)
        ins = tuple(gpu(torch.randn(bsz, S, H * D, generator=g).to(F16) * 1.7) for _ in range(3))
        qw, kw = (gpu(torch.randn(H * D, generator=g).mul(0.3).add(1.0).to(F16)) for _ in range(2))
        return ins, qw, kw, gpu(torch.randn(hi - lo, D, generator=g)), gpu(torch.randn(hi - lo, D, generator=g))

    def run(nat):
        (q_in, k_in, v_in), qw, kw, cs, sn = data()
        q, k, v = nat.rmsnorm_rope_transpose(q_in, k_in, v_in, H, qw, kw, 1e-6, 1, cs, sn, lo, hi, q_scale=0.1275)
        q1, k1, v1 = nat.rmsnorm_rope_transpose(q_in, None, None, H, qw, None, 1e-6, 1, cs, sn, lo, hi, q_scale=0.1275)
        assert k1 is None and v1 is None
        return {"q": q, "k": k, "v": v, "q_alone": q1}

    def check(nat, outs):   # == the three passes, bit for bit (tests/test_gpu_prologue.py test_rmsnorm_rope_transpose_equals_the_three_passes)
        (q_in, k_in, v_in), qw, kw, cs, sn = data()
        qn, kn = nat.rmsnorm_forward(q_in, qw, 1e-6), nat.rmsnorm_forward(k_in, kw, 1e-6)
        q_ref, k_ref = nat.qk_norm_rope_transpose(qn, kn, H, H, 0, None, None, None, None, 1e-6, 1, cs, sn, lo, hi, q_scale=0.1275)
        assert torch.equal(outs["q"], q_ref) and torch.equal(outs["k"], k_ref) and torch.equal(outs["q_alone"], q_ref)
        assert torch.equal(outs["v"], v_in.unflatten(2, (H, D)).transpose(1, 2).contiguous())
    return run, check


@row("prologue/in_place", in_place=True)
def _():
    from test_gpu_prologue import ulp_equal

    bsz, H, S, D, L = 1, 3, 151, 64, 15

    def data():
        g = torch.Generator().manual_seed(151)
        x, w, b = torch.randn(7, 32, generator=g).to(BF16), torch.randn(32, generator=g).to(BF16), torch.randn(32, generator=g).to(BF16)
        q, k = (torch.randn(bsz, H, S, D, generator=g).to(BF16) for _ in range(2))
        return x, w, b, q, k, torch.randn(S - L, D, generator=g), torch.randn(S - L, D, generator=g)

    def run(nat):
        x, w, b, q, k, cs, sn = data()
        outs = {"rms": gpu(x), "ln": gpu(x)}
        nat.rms_norm_forward(outs["rms"], gpu(w), 1e-5)
        nat.layer_norm_forward(outs["ln"], gpu(w), gpu(b))
        for kind, fn in (("cossin", nat.apply_qk_rope_inplace_cossin), ("txtlast", nat.apply_qk_rope_inplace_cossin_txtlast)):
            outs["q_" + kind], outs["k_" + kind] = gpu(q), gpu(k)
            fn(outs["q_" + kind], outs["k_" + kind], gpu(cs), gpu(sn), L)
        outs["q_complex"], outs["k_complex"] = gpu(q.to(F16)), gpu(k.to(F16))
        nat.apply_qk_rope_inplace_cossin_complex(outs["q_complex"], outs["k_complex"], gpu(cs[:, :D // 2].contiguous()),
                                                 gpu(sn[:, :D // 2].contiguous()), L)
        outs["q_fused"], outs["k_fused"] = gpu(q), gpu(k)
        nat.qk_norm_rope(outs["q_fused"], outs["k_fused"], 0, rope_kind=1, cos=gpu(cs), sin=gpu(sn), rope_lo=0, rope_hi=S - L)
        return outs

    def check(nat, outs):   # (tests/test_gpu_prologue.py test_rms_norm, test_layer_norm, test_apply_rope, test_fused_equals_sequence)
        x, w, b, q, k, cs, sn = data()
        ulp_equal(outs["rms"], O.rms_norm(x, w), 2e-3, 2)
        ulp_equal(outs["ln"], O.layer_norm(x, w, b), 5e-3, 2, 1e-4)
        for kind in ("cossin", "txtlast"):
            rq, rk = O.apply_qk_rope(q, k, cs, sn, L, kind)
            assert torch.equal(outs["q_" + kind].cpu(), rq) and torch.equal(outs["k_" + kind].cpu(), rk)
        rq, rk = O.apply_qk_rope(q.to(F16), k.to(F16), cs[:, :D // 2].contiguous(), sn[:, :D // 2].contiguous(), L, "complex")
        assert torch.equal(outs["q_complex"].cpu(), rq) and torch.equal(outs["k_complex"].cpu(), rk)
        assert torch.equal(outs["q_fused"], outs["q_txtlast"]) and torch.equal(outs["k_fused"], outs["k_txtlast"])
    return run, check


# =========================================================================================================
# transformer-block glue at (B, S, N) = (1, 19, 40) and (2, 77, 5120)
# =========================================================================================================
for _shape in ((1, 19, 40), (2, 77, 5120)):
    @row("glue/%dx%dx%d" % _shape)
    def _(shape=_shape):
        B, S, N = shape

        def data():
            g = torch.Generator().manual_seed(N + S)
            x = (torch.randn(B, S, N, generator=g) * 2 + 0.5).to(BF16)
            w, b = torch.randn(N, generator=g), torch.randn(N, generator=g)
            sc, sh, gate = (torch.randn(B, 1, N, generator=g) * 0.3 for _ in range(3))
            return x, w, b, sc, sh, gate, torch.randn(B, S, N, generator=g), torch.randn(B, S, N, generator=g).to(BF16)

        def run(nat):
            x, w, b, sc, sh, gate, xn, attn = map(gpu, data())
            return {"layernorm": nat.layernorm_forward(x, w, b, 1e-6, F32), "layernorm_plain": nat.layernorm_forward(x, None, None, 1e-6, F32),
                    "rmsnorm": nat.rmsnorm_forward(x, w.to(BF16), 1e-6),
                    "modulate_shift": nat.modulate_shift_forward(xn, sc, sh, BF16),
                    "gate_residual": nat.modulate_gate_residual_forward(x, attn, gate, BF16),
                    "gate_residual_f32": nat.modulate_gate_residual_forward(x, attn.float(), gate, F32),
                    "layernorm_modulate": nat.layernorm_modulate_forward(x, w, b, sc, sh, 1e-6)}

        def check(nat, outs):   # (tests/test_gpu_glue.py; rmsnorm: tests/test_gpu_prologue.py _triton_rmsnorm and its `close`)
            from test_gpu_prologue import _triton_rmsnorm, close

            x, w, b, sc, sh, gate, xn, attn = data()
            torch.testing.assert_close(outs["layernorm"].cpu(), O.fp32_layernorm(x, w, b, 1e-6), atol=2e-5, rtol=2e-5)
            torch.testing.assert_close(outs["layernorm_plain"].cpu(), O.fp32_layernorm(x, None, None, 1e-6), atol=2e-5, rtol=2e-5)
            close(outs["rmsnorm"], _triton_rmsnorm(x, w.to(BF16), 1e-6))
            assert torch.equal(outs["modulate_shift"].cpu(), O.modulate_shift(xn, sc, sh, BF16))
            assert torch.equal(outs["gate_residual"].cpu(), O.modulate_gate_residual(x, attn, gate, BF16))
            assert torch.equal(outs["gate_residual_f32"].cpu(), O.modulate_gate_residual(x, attn.float(), gate, F32))
            two = nat.modulate_shift_forward(nat.layernorm_forward(gpu(x), gpu(w), gpu(b), 1e-6, F32), gpu(sc), gpu(sh), BF16)
            assert torch.equal(outs["layernorm_modulate"], two)      # == the two separate kernels, bit for bit
        return run, check


# =========================================================================================================
# the two tests
# =========================================================================================================
class DoNothingLibrary:
    """Stands in for libsvgattn.so: every svg_* entry returns 0 (a small byte count for *_workspace_bytes) and touches nothing."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("svg_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 256 if name.endswith("_workspace_bytes") else 0
        return entry


IDS = [r.name for r in TABLE]
assert len(set(IDS)) == len(IDS)


@pytest.mark.parametrize("r", [r for r in TABLE if not r.in_place], ids=[r.name for r in TABLE if not r.in_place])
def test_do_nothing_library_is_caught(nat, monkeypatch, r):
    lib = DoNothingLibrary()
    monkeypatch.setattr(nat, "load", lambda strict=True: lib)
    nat.clear_workspace_cache()
    try:
        outs = r.run(nat)
        torch.cuda.synchronize()
    finally:
        nat.clear_workspace_cache()    # (workspaces sized by the stand-in)
    assert any(c for c in lib.calls if not c.endswith("_workspace_bytes") and c != "svg_debug_band_queue_cap"), "the row called no entry"
    assert outs and all((outs[n] is None) == (n in r.absent) for n in outs), sorted(outs)
    for name, t in outs.items():
        if t is None:
            continue
        if name in r.host_filled:
            assert_fully_written(t, f"{r.name}: {name} (filled by the wrapper)")
            continue
        with pytest.raises(AssertionError, match="still hold the poison pattern"):
            assert_fully_written(t, f"{r.name}: {name}")
        assert bool(unwritten(t).all()), f"{r.name}: {name} was partly written although the library did nothing"


@pytest.mark.parametrize("r", TABLE, ids=IDS)
def test_real_library_writes_everything(nat, r):
    assert nat.allocations_poisoned()
    outs = r.run(nat)
    torch.cuda.synchronize()
    assert outs and all((outs[n] is None) == (n in r.absent) for n in outs), sorted(outs)
    for name, t in outs.items():
        if t is not None:
            assert_fully_written(t, f"{r.name}: {name}")
    r.check(nat, outs)


def test_table_covers_the_wrappers(nat):
    """every public function or class of svg._native that allocates through the switch — itself or through the private helpers it calls —
    is called by some row, so a new wrapper needs a row"""
    import ast
    import inspect

    import test_gpu_band_window as W

    defs = {n.name: n for n in ast.parse(inspect.getsource(nat)).body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    calls = {name: {c.func.id for c in ast.walk(n) if isinstance(c, ast.Call) and isinstance(c.func, ast.Name)} for name, n in defs.items()}
    allocating = {"empty", "empty_like"}
    while True:
        more = {name for name, cs in calls.items() if cs & allocating} - allocating
        if not more:
            break
        allocating |= more
    public = {n for n in allocating & set(defs) if not n.startswith("_")}
    assert {"band_attention", "band_attention_switch", "varblock_attention", "cross_attention_pair", "kmeans_loop", "KmeansBuffers"} <= public
    src = inspect.getsource(inspect.getmodule(test_table_covers_the_wrappers)) + inspect.getsource(W.run_window)
    # token_major_empty: reached through token_major_out=True.  band_attention_fp8: the e4m3 bodies have bounds of their own
    # (tests/test_gpu_fp8.py, which runs poisoned like every module).
    missing = sorted(n for n in public - {"token_major_empty", "band_attention_fp8"} if f"nat.{n}(" not in src)
    assert not missing, f"wrappers of svg._native without a row in TABLE: {missing}"
