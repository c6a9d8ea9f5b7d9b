"""The bf16 band kernels at head_dim 128 run the overflow test of the max-free softmax on every eighth key tile only, validate a
q-tile's row sums and accumulators after its tile loop, and compute a q-tile that fails once more with the test on every tile
(SPEC, csrc/attn_m16.h; svg_debug_band_replays counts the replays).

Shapes: bf16, head_dim 128, two heads (head 0 contiguous, head 1 token-major), S = 2 frames x 640 + 64 = 1344, band 512 (a q-tile in
the middle of the video visits 21 key tiles and crosses two check points), and the dense mask (band = S + 1).  The reference is
oracle/svg_oracle.py at the bf16 tolerance of tests/test_gpu_kernels.py (check_attn).

Inputs are built in LOGICAL row order (what the mask speaks of) and head 1 is carried to its physical, frame-major order with the
oracle's inverse head placement, so that "key tile t of q-tile j" means the same for both heads.  The last ten dimensions of q and k
are zero except for the spikes: spike i lives in dimension 118 + i alone (one query row, one key row), so it raises exactly one score
— to `mag` in the log2 domain, against at most about +6 for everything else — and no other.

Every launch case runs on the static mapping (14 work items: one workgroup per q-tile, band_attn_m16_kernel) and through the work queue
(band_attn_m16_queue_kernel, svg_debug_band_queue_cap as in tests/test_gpu_band_queue.py): the two kernels replay by different means.
Nothing here provokes a fault: an overflow is an arithmetic infinity inside fp32 registers."""
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import svg_oracle as O
from svg import _native as nat
from band_replay_cases import BEST, GEO_A, SPIKE_DIM0, bool_mask, build, q_tiles_of, reference, replay_everywhere_spikes  # noqa: F401
from test_gpu_kernels import check_attn

from poisoned import poison_on  # noqa: E402,F401  (the suite runs on poisoned allocations)

pytestmark = pytest.mark.gpu

D, H, F_, P_, CTX, L, BAND = GEO_A
V, S, REAL = GEO_A.V, GEO_A.S, GEO_A.REAL     # S = 1344 = 21 key tiles
NO_CAP = 1 << 20
GOLDEN = Path(__file__).resolve().parent / "golden" / "band_replay_golden.npz"


def mask_params(kind):
    return GEO_A.mask_params(kind)


def launch(kind, q, k, v, path, done=None):
    """logical q, k, v -> logical output (CPU) of one launch: head 1 goes to the device in physical order and comes back"""
    phys = [O.head_placement(x, BEST, CTX, F_, P_, inverse=True).cuda().contiguous() for x in (q, k, v)]
    mask = nat.BandMask(**mask_params(kind))
    kw = dict(head_perm_flag=BEST.cuda(), vid0=0, num_frame=F_, frame_size=P_)
    lib = nat.load()
    if path == "queue":
        assert lib.svg_debug_band_queue_cap(NO_CAP) == 0
    try:
        out = torch.full_like(phys[0], float("nan"))
        if done is not None:
            kw.update(done=done, done_nseg=1)
        nat.band_attention(*phys, mask, out=out, **kw)
        torch.cuda.synchronize()
    finally:
        assert lib.svg_debug_band_queue_cap(0) == 0
    return O.head_placement(out.cpu(), BEST, CTX, F_, P_)


def run_checked(kind, spikes, seed, path):
    """-> (logical output, replays of the launch); the output is checked against the oracle"""
    q, k, v = build(kind, spikes, seed)
    nat.band_replays(reset=True)
    o = launch(kind, q, k, v, path)
    n = nat.band_replays(reset=True)
    assert torch.isfinite(o.float()).all()
    check_attn(o, reference(kind, spikes, seed), torch.bfloat16)
    print(f"{kind} {path} spikes={len(spikes)} replays={n}")
    return o, n


# Late spikes: key tile index 1 (just after a check), 7 (just before one), 8 (on one), 9 and the last tile of the q-tile, for a row of
# wave 0 and a row of wave 7, every spike on a row of its own.
#   dense: q-tile 2 (rows 512 .. 767) visits key tiles 0 .. 20 in order: tile index t holds keys [64 t, 64 t + 64).
#   band:  the wave-0 rows are rows 512 + i of q-tile 2 (keys 1 + i .. 1023 + i and the text columns 1280 .. 1319: the merged
#          schedule is again tiles 0 .. 20 in order); rows of wave 7 of that q-tile do not see key tile 1, so the wave-7 rows are
#          rows 224 + i of q-tile 0, which visits key tiles 0 .. 11 and then the text columns as its 13th and last tile.
def late_spikes(kind, mag):
    sp = []
    for i, t in enumerate((1, 7, 8, 9, 20)):
        sp.append((512 + 2 * i, 64 * t + 3 + i, mag))                                   # wave 0 of q-tile 2
    for i, t in enumerate((1, 7, 8, 9, "last")):
        if kind == "dense":
            sp.append((512 + 224 + 2 * i, 64 * (20 if t == "last" else t) + 9 + i, mag))    # wave 7 of q-tile 2
        else:
            sp.append((224 + 2 * i, (V + 9 + i) if t == "last" else 64 * t + 9 + i, mag))   # wave 7 of q-tile 0
    return sp


PATHS = ["static", "queue"]
KINDS = ["band", "dense"]


@pytest.mark.parametrize("kind", KINDS)
def test_randn_inputs_never_replay_and_the_queue_equals_the_counting_launch(kind):
    q, k, v = build(kind, [], seed=1)
    outs = {}
    for path in PATHS:
        outs[path], n = run_checked(kind, [], 1, path)
        assert n == 0
    done = nat.notify_counters(H, 1, torch.device("cuda"))
    o_count = launch(kind, q, k, v, "static", done=done)
    assert (done[:H].cpu() == nat.band_notify_target(S, nat.BandMask(**mask_params(kind)))).all()
    assert torch.equal(outs["queue"], o_count)
    assert torch.equal(outs["static"], o_count)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mag", [30.0, 120.0, 400.0])
@pytest.mark.parametrize("kind", KINDS)
def test_late_spikes(kind, mag, path):
    sp = late_spikes(kind, mag)
    _, n = run_checked(kind, sp, 2, path)
    if mag < 400.0:
        assert n == 0       # 2^(mag - 10) and its row sums stay far below 2^120: a lagging reference, no overflow
    else:
        assert 1 <= n <= H * q_tiles_of(kind, [r for r, _, _ in sp])


@pytest.mark.parametrize("path", PATHS)
def test_spike_on_a_text_row(path):
    """rows 1280 .. 1319 are full rows with a q-tile of their own: two active waves and six idle ones, which have to pass the
    barrier of the validation and follow the replay with the same number of barriers as the active ones"""
    sp = [(V + 10, 64 * 9 + 20, 400.0)]
    _, n = run_checked("band", sp, 3, path)
    assert 1 <= n <= H * q_tiles_of("band", [V + 10])


@pytest.mark.parametrize("path", PATHS)
def test_spike_after_a_partly_masked_start(path):
    """row 767 is the last row of q-tile 2, whose schedule starts at key tile 0: the first four tiles hold no key of the band of
    some row of wave 7 (keys from 256 on for row 767), so the wave stays on the exact path for several tiles before the schedule of
    the checks begins; then a +400 spike on key tile 13, between two checks"""
    sp = [(767, 64 * 13 + 30, 400.0)]
    _, n = run_checked("band", sp, 4, path)
    assert 1 <= n <= H * q_tiles_of("band", [767])


@pytest.mark.parametrize("path", PATHS)
def test_two_launches_are_equal(path):
    sp = late_spikes("band", 400.0)
    a, na = run_checked("band", sp, 2, path)
    b, nb = run_checked("band", sp, 2, path)
    assert torch.equal(a, b) and na == nb


@pytest.mark.parametrize("path", PATHS)
def test_replay_path_equals_the_kernel_before_the_change(path):
    """tests/golden/band_replay_golden.npz is the KERNEL's own output on these inputs at the commit before the overflow test left the
    tile loop (tests/golden/make_golden_band_replay.py, which checked it against the fp32 oracle when it wrote it).  The replay is that
    code tile for tile, so the q-tiles that replay reproduce it bit for bit; the rows behind real_len have one key tile, which is
    checked in both passes and never replays, and reproduce it too.  (The output has 2 x 1344 = 2688 rows; the fixture holds all.)"""
    sp = replay_everywhere_spikes()
    o, n = run_checked("band", sp, 5, path)
    assert n == H * 6            # five band q-tiles and the text q-tile of each head
    gold = torch.from_numpy(np.load(GOLDEN)["attn_out_u16"].view(np.int16)).view(torch.bfloat16)
    assert torch.equal(o.reshape(-1, D), gold)
