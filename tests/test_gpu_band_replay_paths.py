"""The replay of the bf16 band kernels at head_dim 128 (SPEC, csrc/attn_m16.h: the overflow test of the max-free softmax on every eighth
key tile, a validation after the tile loop, and a second pass of a q-tile that fails it) on every kernel and launch path that carries it.
tests/test_gpu_band_speculative.py drives one workgroup per q-tile into a replay; here
  1. resident workgroups of the queue kernel (svg_debug_band_queue_cap 1, 2, 3 on 14 work items) replay between other q-tiles, after
     another replay and as the last thing they do: the state of the replay (slot[2] of the workgroup's LDS) goes 0 -> 1 -> 2 -> 0;
  2. the device-switched kernel replays under either mask;
  3. the strided entry replays (q re-read and the K / V cursor restarted through the row strides of a fused QKV projection);
  4. counting launches replay: every q-tile notifies once, the counters end EXACTLY at their targets, and a consumer behind
     svg_wait_counters sees final rows of a segment whose q-tiles replayed;
  5. the magnitude of a spike crosses the border between "a lagging reference" and "an overflow" (2^120, the threshold of the
     validation, lies between 2^(112 - 10) and 2^(160 - 10)), alone and beside a second score of comparable size on the same row, where
     the answer is a weighted mean of two v rows and a sum that was let through too large, or rescaled to zero, shows;
  6. a ragged geometry: a partial last key tile, a short last q-tile of the video rows, text columns that straddle two key tiles.

The inputs come from tests/band_replay_cases.py (tests/test_band_replay_cases_cpu.py checks them on the CPU).  The reference everywhere is
O.masked_attention on the rounded inputs under O.band_mask, at the bf16 / fp16 tolerance of tests/test_gpu_kernels.py (check_attn); bit
equalities are asserted only where the project claims them (queue = static, strided = contiguous, switched = the plain launch of the
selected mask, counting = non-counting, two launches of the same inputs).  Nothing here provokes a fault: an overflow is an arithmetic
infinity inside fp32 registers, and every launch is a valid call."""
import contextlib
import functools

import pytest
import torch

import band_replay_cases as C
from oracle import svg_oracle as O
from svg import _native as nat
from test_gpu_kernels import check_attn

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu

NO_CAP = 1 << 20   # svg_debug_band_queue_cap with a cap no launch reaches: the queue also for launches of one round


@contextlib.contextmanager
def queue_cap(cap):
    """cap: None -> the default dispatch (14 work items: the static mapping), else svg_debug_band_queue_cap(cap) for the block"""
    lib = nat.load()
    if cap is not None:
        assert lib.svg_debug_band_queue_cap(cap) == 0
    try:
        yield
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0


@functools.lru_cache(maxsize=4)
def _device_inputs(case):
    g = case.geo
    return [O.head_placement(x, C.BEST, g.CTX, g.F, g.P, inverse=True).cuda().contiguous() for x in C.inputs(case)]


def device_inputs(case):
    """q, k, v of the case on the device: head 1 in its physical order"""
    return _device_inputs(case._replace(name=""))


def perm_kw(case):
    return dict(head_perm_flag=C.BEST.cuda(), vid0=0, num_frame=case.geo.F, frame_size=case.geo.P)


def to_logical(case, out):
    g = case.geo
    return O.head_placement(out.cpu(), C.BEST, g.CTX, g.F, g.P)


def band_mask(case, kind):
    return nat.BandMask(**case.geo.mask_params(kind))


def launch(case, kind, done=None, done_nseg=1, strided=False):
    """one launch into an output pre-filled with NaN -> the logical output (CPU).  done: a counting launch (the static mapping).
    strided: q, k, v as views of one [1, S, 3 H D] buffer and a token-major output (svg_band_attention_strided)."""
    q, k, v = device_inputs(case)
    kw = perm_kw(case)
    if done is not None:
        kw.update(done=done, done_nseg=done_nseg)
    if case.prescaled:
        kw.update(q_prescaled=True)
    if strided:
        H, S, D = q.shape[1:]
        qkv = torch.cat([x.transpose(1, 2).reshape(1, S, H * D) for x in (q, k, v)], dim=2)
        q, k, v = (qkv[:, :, i * H * D:(i + 1) * H * D].unflatten(2, (H, D)).transpose(1, 2) for i in range(3))
        assert not q.is_contiguous()
        out = nat.token_major_empty(q)
        out.fill_(float("nan"))
    else:
        out = torch.full_like(q, float("nan"))
    nat.band_attention(q, k, v, band_mask(case, kind), out=out, **kw)
    torch.cuda.synchronize()
    return to_logical(case, out)


def launch_counted(case, kind, **kw):
    """-> (logical output, replays of the launch)"""
    nat.band_replays(reset=True)
    o = launch(case, kind, **kw)
    return o, nat.band_replays(reset=True)


def static_launch(case, kind):
    """the static mapping whatever the cap says: a counting launch (as tests/test_gpu_band_speculative.py forces it)"""
    done = nat.notify_counters(case.geo.H, 1, torch.device("cuda"))
    o, n = launch_counted(case, kind, done=done)
    assert (done[:case.geo.H].cpu() == nat.band_notify_target(case.geo.S, band_mask(case, kind))).all()
    return o, n


def check_oracle(case, kind, o):
    assert torch.isfinite(o.float()).all()
    check_attn(o, C.oracle(case, kind), case.dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. resident workgroups that replay between other q-tiles
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", C.QUEUE_CAPS)
@pytest.mark.parametrize("subset", C.QUEUE_SUBSETS)
def test_capped_queue_replays_between_other_q_tiles(subset, cap):
    """14 work items on 1, 2 or 3 resident workgroups: each runs several q-tiles, replayed ones among them — after another replay
    (all six), between fresh ones (0, 2, 4), as its first pass (first) and as the last pass before the queue runs dry (last)"""
    case = C.queue_case(subset)
    plain = case.without_spikes()
    want = len(case.replaying_pairs())
    assert want == {"all6": 12, "024": 6, "first": 1, "last": 1}[subset]
    with queue_cap(cap):
        o, n = launch_counted(case, "band")
        o_after, n_after = launch_counted(plain, "band")    # directly behind the replays, still capped: nothing of them survives
    print(f"queue {subset} cap={cap}: replays={n} (spike-free launch behind it: {n_after})")
    check_oracle(case, "band", o)
    o_static, n_static = static_launch(case, "band")
    assert torch.equal(o, o_static)
    assert n == want and n_static == want
    o_plain, n_plain = launch_counted(plain, "band")        # uncapped
    assert n_after == 0 and n_plain == 0
    assert torch.equal(o_after, o_plain)
    check_oracle(plain, "band", o_plain)


@pytest.mark.parametrize("cap", C.QUEUE_CAPS)
@pytest.mark.parametrize("form", ["fp16", "bf16_prescaled"])
def test_capped_queue_controls_without_the_replay(form, cap):
    """fp16 and the pre-scaled bf16 form share the queue loop, without SPEC: the per-tile test handles the same spikes (fp16 holds
    q = 4 and k = mag / (4 c) = 784 exactly enough; the pre-scaled q carries softmax_q_scale(D), its spike is 4 c)"""
    case = C.queue_case("all6", torch.float16) if form == "fp16" else C.queue_case("all6", prescaled=True)
    with queue_cap(cap):
        o, n = launch_counted(case, "band")
    print(f"queue control {form} cap={cap}: replays={n}")
    check_oracle(case, "band", o)
    o_static, n_static = static_launch(case, "band")
    assert torch.equal(o, o_static)
    assert n == 0 and n_static == 0


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. the device-switched entry
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [0, 1])
def test_device_switched_entry_replays(flag):
    """band_attn_m16_switch_kernel carries SPEC for both masks; flag 0: the band mask with the head placement, flag 1: the dense mask of
    the same real_len without it (dense attention over the real rows does not depend on their order, so the oracle on the logical
    inputs holds for the token-major head too; where ITS spikes fall in the physical key order is not pinned: replays >= 1)"""
    case = C.switch_case()
    kind = "dense_real" if flag else "band"
    q, k, v = device_inputs(case)
    mask, alt = band_mask(case, "band"), band_mask(case, "dense_real")
    sw = torch.tensor([flag], device="cuda", dtype=torch.int32)
    nat.band_replays(reset=True)
    plain = torch.full_like(q, float("nan"))
    if flag:
        nat.band_attention(q, k, v, alt, out=plain)
    else:
        nat.band_attention(q, k, v, mask, out=plain, **perm_kw(case))
    n_plain = nat.band_replays(reset=True)     # 14 work items, no cap: the static mapping
    outs, counts = [], []
    for cap in (None, 2):                      # this kernel keeps the static mapping either way
        with queue_cap(cap):
            o = torch.full_like(q, float("nan"))
            nat.band_attention_switch(q, k, v, mask, alt, sw, out=o, **perm_kw(case))
            counts.append(nat.band_replays(reset=True))
        outs.append(o)
    print(f"switch flag={flag}: replays={counts[0]} (plain launch of the selected mask: {n_plain}; capped: {counts[1]})")
    for o in outs:
        assert torch.equal(o, plain)
    assert counts[0] >= 1 and counts[0] == n_plain and counts[1] == counts[0]
    if not flag:
        assert counts[0] == 12
    check_oracle(case, kind, to_logical(case, outs[0]))


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. the strided entry
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, NO_CAP, 2], ids=["static", "queue", "queue_cap2"])
def test_strided_entry_replays(cap):
    case = C.queue_case("all6")
    with queue_cap(cap):
        o_c, n_c = launch_counted(case, "band")
        o_s, n_s = launch_counted(case, "band", strided=True)
    print(f"strided cap={cap}: replays={n_s} (contiguous: {n_c})")
    assert torch.equal(o_s, o_c)
    assert n_s == n_c == 12
    check_oracle(case, "band", o_s)


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. counting launches under replay
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [1, 3])
@pytest.mark.parametrize("subset", ["all6", "024"])
def test_counters_end_exactly_at_their_targets_under_replay(subset, nseg):
    """the first pass of a replayed q-tile returns before P::notify: every q-tile notifies once, so the counters end AT the targets —
    a second notify would let svg_wait_counters release a consumer while another q-tile of the head is still running"""
    case = C.queue_case(subset)
    g = case.geo
    mask = band_mask(case, "band")
    o_ref, n_ref = launch_counted(case, "band")
    if nseg == 1:
        n, targets = 1, [nat.band_notify_target(g.S, mask)]
    else:
        n, bounds, targets = nat.band_notify_layout(g.S, mask, nseg)
        assert n >= 2 and bounds[0] == 0 and bounds[-1] == g.S and sum(targets) == nat.band_notify_target(g.S, mask)
    done = nat.notify_counters(g.H, n, torch.device("cuda"))
    o, n_rep = launch_counted(case, "band", done=done, done_nseg=n)
    print(f"counting {subset} nseg={n}: replays={n_rep} counters={done[:g.H * n].tolist()} targets={targets}")
    assert torch.equal(done[:g.H * n].cpu().view(g.H, n), torch.tensor(targets, dtype=torch.int32).expand(g.H, n))
    assert torch.equal(o, o_ref)
    assert n_rep == n_ref == len(case.replaying_pairs())
    check_oracle(case, "band", o)


def test_segment_release_under_replay():
    """The contract of the per-segment counters (tests/test_gpu_kernels.py::test_band_attention_notify_segments_with_fused_placement) on
    a launch whose q-tiles of real rows all replay: a copy behind svg_wait_counters on another stream, enqueued before the launch has
    run, sees the final rows of its segment.  `o` is poisoned first, so a release before the second pass has stored shows.  One
    iteration; the waiters carry a deadline, so a counter that never arrived fails the test instead of holding its stream."""
    case = C.queue_case("all6")
    g = case.geo
    q, k, v = device_inputs(case)
    mask = band_mask(case, "band")
    ref = torch.full_like(q, float("nan"))
    nat.band_attention(q, k, v, mask, out=ref, **perm_kw(case))
    n, bounds, targets = nat.band_notify_layout(g.S, mask, 3)
    assert n >= 2
    o = torch.full_like(q, float("nan"))
    done = nat.notify_counters(g.H, n, q.device)
    late = torch.zeros(g.H * n, device="cuda", dtype=torch.int32)
    nat.band_replays(reset=True)               # (synchronises)
    sides = [torch.cuda.Stream() for _ in range(2)]
    ev = torch.cuda.Event()
    ev.record()
    nat.band_attention(q, k, v, mask, out=o, done=done, done_nseg=n, **perm_kw(case))
    cnt = done[:g.H * n].view(g.H, n)
    seen = {}
    for i, (h, sg) in enumerate((h, sg) for h in range(g.H) for sg in range(n)):
        st = sides[i % 2]
        st.wait_event(ev)
        with torch.cuda.stream(st):
            nat.wait_counters(cnt[h, sg:sg + 1], targets[sg], timeout_ms=20000, timed_out=late[i:i + 1])
            seen[h, sg] = o[0, h, bounds[sg]:bounds[sg + 1]].clone()   # behind the waiter, beside the launch
    torch.cuda.synchronize()
    assert nat.band_replays(reset=True) == 12
    assert int(late.sum()) == 0, "a segment counter never reached its target"
    assert torch.equal(o, ref)
    for (h, sg), rows in seen.items():
        assert torch.equal(rows, ref[0, h, bounds[sg]:bounds[sg + 1]]), f"head {h} segment {sg} released early"
    assert torch.equal(cnt.cpu(), torch.tensor(targets, dtype=torch.int32).expand(g.H, n))


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. the border between "lagging reference" and "overflow"
# ------------------------------------------------------------------------------------------------------------------------------------
def test_magnitude_sweep_across_the_validation_threshold():
    """a probability is 2^(score - reference - 10): mag <= 112 stays below 2^102 whatever the (non-negative) reference, mag >= 160 is
    above 2^128 for any reference a randn tile leaves (at most about +8), and in between the q-tile replays or not depending on the row's
    reference at that tile — not asserted, printed.  More score never replays less: the count is non-decreasing in mag."""
    counts = []
    for mag in C.SWEEP_MAGS:
        case = C.sweep_case(mag)
        o, n = launch_counted(case, "band")
        print(f"sweep mag={mag}: replays={n}")
        check_oracle(case, "band", o)
        counts.append(n)
    first = next((m for m, n in zip(C.SWEEP_MAGS, counts) if n), None)
    print(f"sweep: replays by mag {dict(zip(C.SWEEP_MAGS, counts))}; first mag that replays: {first}")
    assert all(n == 0 for m, n in zip(C.SWEEP_MAGS, counts) if m <= 112)
    assert all(n >= 1 for m, n in zip(C.SWEEP_MAGS, counts) if m >= 160)
    assert counts == sorted(counts)
    assert max(counts) <= 2 * C.GEO_A.H       # the spiked rows lie in two q-tiles of each head


@pytest.mark.parametrize("where", sorted(C.PAIR_SECOND_TILE))
@pytest.mark.parametrize("m", C.PAIR_MAGS)
def test_two_large_scores_on_one_row(m, where):
    """scores m and m - 1 on one row (tests/test_band_replay_cases_cpu.py: its oracle row is the weighted mean of the two v rows, neither
    weight below 0.1): a sum or an accumulator that was let through too large, or rescaled to zero, changes the mean — with a single
    spike any error of the normalisation cancels in v[key].  on_check: the second score arrives on a check point, the rescale by alpha
    while the accumulators hold the first.  (m = 132 on a check point is the row that came out as v_b alone, with no replay, while
    alpha = 2^(old reference - new reference) was allowed to flush to zero over a sum of 2^118: csrc/attn_m16.h, exact path.)"""
    case = C.pair_case(m, where)
    o, n = launch_counted(case, "band")
    print(f"pair m={m} {where}: replays={n}")
    check_oracle(case, "band", o)
    ref = C.oracle(case, "band")
    for row, _, _ in case.pairs:     # the rows the case is about, on their own: not hidden in the norm over 2688 rows
        check_attn(o[0, :, row], ref[0, :, row], case.dtype)
    assert n <= 2 * case.geo.H
    if m <= 112:
        assert n == 0
    if m >= 160:
        assert n >= 1


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. a ragged geometry
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [NO_CAP, 2], ids=["queue", "queue_cap2"])
@pytest.mark.parametrize("kind", C.RAGGED_KINDS)
def test_ragged_geometry(kind, cap):
    """S = 1300, real_len 1240: a last key tile of 20 keys, a last video q-tile of 176 rows, text columns over key tiles 18 and 19;
    the static mapping and the queue, all S rows against the oracle (the rows behind real_len included)"""
    case = C.ragged_case()
    plain = case.without_spikes()
    g = case.geo
    o_static, n_static = static_launch(case, kind)
    with queue_cap(cap):
        o, n = launch_counted(case, kind)
        o_after, n_after = launch_counted(plain, kind)
    print(f"ragged {kind} cap={cap}: replays={n} (static: {n_static}; spike-free: {n_after})")
    check_oracle(case, kind, o_static)
    assert torch.equal(o, o_static)
    assert n == n_static
    assert 1 <= n <= g.H * C.q_tiles_of(kind, [s.row for s in case.spikes], g)
    assert n_after == 0
    check_oracle(plain, kind, o_after)
    o_plain, n_plain = static_launch(plain, kind)
    assert n_plain == 0 and torch.equal(o_after, o_plain)
