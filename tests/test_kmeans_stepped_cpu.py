"""The Lloyd loop in steps without a GPU (include/svg_attn_kmeans_stepped.h: svg_kmeans_stepped_workspace_bytes / _iterate / _commit /
_finish): the exports, the header and its place in svg_attn.h, the argument validation of the entries — every check runs on the host before
any launch (rows that pass placeholder pointers are skipped where a GPU is visible, as in test_adaptive_top_p_cpu.py) — and the driver
svg.kmeans_utils.lloyd_stepped with torch stand-ins for the sides (kmeans_stepped_cases.TorchSteppedSide around the oracle's iteration, as
test_svg2_batch_cpu.py drives lloyd_device_rule): one side, two sides, groups, and head shards on gloo ranks with a counted all-reduce."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

import gloo_ranks
from kmeans_stepped_cases import TorchSteppedSide, same_five
from oracle import svg_oracle as O
from svg import _native as nat

OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3   # include/svg_attn.h
PH, PA, PB, PC = 0x10000, 0x20000, 0x30000, 0x40000   # placeholder device pointers (16-byte aligned; never dereferenced by a rejected call)
ROOT = Path(__file__).resolve().parent.parent
ENTRIES = {"svg_kmeans_stepped_workspace_bytes", "svg_kmeans_stepped_iterate", "svg_kmeans_stepped_commit", "svg_kmeans_stepped_finish"}
BIG = 1 << 40


def host_only():
    if torch.cuda.is_available():
        pytest.skip("placeholder device pointers: host-only check")


def test_library_exports_the_entries():
    lib = nat.load()
    assert set(nat.KMEANS_STEPPED_SIGNATURES) == ENTRIES
    others = set()
    for name in dir(nat):
        if (name.endswith("SIGNATURES") or name.endswith("ENTRIES")) and name != "KMEANS_STEPPED_SIGNATURES" and isinstance(getattr(nat, name), dict):
            others |= set(getattr(nat, name))
    assert "svg_kmeans_loop_grouped_strided" in others and not ENTRIES & others
    for name, (res, args) in nat.KMEANS_STEPPED_SIGNATURES.items():
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == res
    assert int(lib.svg_abi_version()) == 4 and nat.SVG_ABI_VERSION == 4


def test_header_is_included_and_matches_the_signatures():
    main = (ROOT / "include" / "svg_attn.h").read_text()
    includes = re.findall(r'^#include "(svg_attn_\w+\.h)"', main, flags=re.M)
    assert "svg_attn_kmeans_stepped.h" in includes
    src = (ROOT / "include" / "svg_attn_kmeans_stepped.h").read_text()
    assert "in this order" in src and "bit for bit" in src
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    protos = re.findall(r"\b([A-Za-z_][A-Za-z0-9_ ]*?[ \*]+)(svg_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
    assert {n for _, n, _ in protos} == ENTRIES

    def c_class(t):
        for pat, c in ((r"\*", "ptr"), (r"\bsize_t\b", "size"), (r"\bint64_t\b", "i64"), (r"\b(int32_t|int)\b", "i32"), (r"\bfloat\b", "f32")):
            if re.search(pat, t):
                return c
        return "?" + t

    def py_class(a):
        if a is C.c_void_p or (isinstance(a, type) and issubclass(a, C._Pointer)):
            return "ptr"
        return {C.c_size_t: "size", C.c_int64: "i64", C.c_int32: "i32", C.c_int: "i32", C.c_float: "f32"}.get(a, "?" + repr(a))

    for ret, name, params in protos:
        ps = [x.strip() for x in params.split(",") if x.strip()]
        want = [c_class(x if x.endswith("*") else re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", x)) for x in ps]
        res, args = nat.KMEANS_STEPPED_SIGNATURES[name]
        assert [py_class(a) for a in args] == want and py_class(res) == c_class(ret), (name, want)


# ---------------------------------------------------------------------------------------------------------
# the workspace size: 0 for what the entries refuse, the grouped loop's size otherwise
# ---------------------------------------------------------------------------------------------------------
def test_workspace_bytes():
    lib = nat.load()
    need = lib.svg_kmeans_stepped_workspace_bytes
    assert need(4, 700, 129, 64, 2) == lib.svg_kmeans_loop_grouped_workspace_bytes(4, 700, 129, 64, 2) > 0
    assert need(4, 700, 129, 128, 4) == lib.svg_kmeans_loop_workspace_bytes(4, 700, 129, 128)
    for bad in ((4, 700, 129, 64, 3), (4, 700, 129, 64, 0), (4, 700, 129, 64, -2), (0, 700, 129, 64, 1), (4, 0, 129, 64, 2), (4, 700, 0, 64, 2),
                (4, 700, 8193, 64, 2), (4, 700, 129, 96, 2)):
        assert need(*bad) == 0, bad
    assert need(4, 700, 8192, 64, 2) > 0


# ---------------------------------------------------------------------------------------------------------
# the validation table: codes and their order
# ---------------------------------------------------------------------------------------------------------
def it_args(x=PH, xbs=None, c0=PA, ca=PB, cb=PC, it=0, mx=PH, B=4, N=700, K=129, D=64, dtype=0, group=2, ws=PH, nb=BIG):
    return [x, N * D if xbs is None else xbs, c0, ca, cb, it, mx, B, N, K, D, dtype, group, ws, nb, None]


def commit_args(mx=PH, lab=PH, cnt=PH, srt=PH, it=0, tol=1e-4, B=4, N=700, K=129, group=2, ws=PH, nb=BIG):
    return [mx, lab, cnt, srt, it, tol, B, N, K, group, ws, nb, None]


def fin_args(c0=PA, ca=PB, cb=PC, out=PH, n=PH, B=4, K=129, D=64, dtype=0, group=2, ws=PH, nb=BIG):
    return [c0, ca, cb, out, n, B, K, D, dtype, group, ws, nb, None]


ITERATE_CASES = [
    # 1. pointers, then sizes, group and it
    ("null_x", it_args(x=None), BAD_ARG),
    ("null_c_init", it_args(c0=None), BAD_ARG),
    ("null_work_a", it_args(ca=None), BAD_ARG),
    ("null_work_b", it_args(cb=None), BAD_ARG),
    ("null_maxima", it_args(mx=None), BAD_ARG),
    ("null_workspace", it_args(ws=None), BAD_ARG),
    ("B0", it_args(B=0), BAD_ARG),
    ("N_neg", it_args(N=-1, xbs=64), BAD_ARG),
    ("K0", it_args(K=0), BAD_ARG),
    ("group0", it_args(group=0), BAD_ARG),
    ("group_not_dividing_B", it_args(group=3), BAD_ARG),
    ("it_neg", it_args(it=-1), BAD_ARG),
    ("null_before_unsupported", it_args(mx=None, D=96), BAD_ARG),
    ("group_before_unsupported", it_args(group=3, K=9000), BAD_ARG),
    ("it_neg_before_workspace", it_args(it=-1, nb=16), BAD_ARG),
    # 2. what the kernels do not cover
    ("K8193", it_args(K=8193), UNSUPPORTED),
    ("D96", it_args(D=96, xbs=700 * 96), UNSUPPORTED),
    ("dtype_f32", it_args(dtype=2), UNSUPPORTED),
    ("unsupported_before_workspace", it_args(dtype=2, nb=16), UNSUPPORTED),
    ("unsupported_before_alias", it_args(D=96, xbs=700 * 96, ca=PA), UNSUPPORTED),
    # 3. the workspace
    ("short_workspace", it_args(nb=None), WORKSPACE),
    ("workspace_before_alias", it_args(nb=None, ca=PA), WORKSPACE),
    ("workspace_before_stride", it_args(nb=None, xbs=8), WORKSPACE),
    # 4. aliased centroid buffers
    ("c_init_is_work_a", it_args(ca=PA), BAD_ARG),
    ("c_init_is_work_b", it_args(cb=PA), BAD_ARG),
    ("work_a_is_work_b", it_args(cb=PB), BAD_ARG),
    ("alias_before_stride", it_args(cb=PB, xbs=700 * 64 + 4), BAD_ARG),
    # 5. the stride checks of svg_kmeans_loop_strided, with its codes
    ("stride_below_N_D", it_args(xbs=700 * 64 - 8), BAD_ARG),
    ("stride_not_multiple_of_8", it_args(xbs=700 * 64 + 4), UNSUPPORTED),
    ("x_not_16_byte_aligned", it_args(x=PH + 8), UNSUPPORTED),
]

COMMIT_CASES = [
    ("null_maxima", commit_args(mx=None), BAD_ARG),
    ("null_labels", commit_args(lab=None), BAD_ARG),
    ("null_counts", commit_args(cnt=None), BAD_ARG),
    ("null_sorted", commit_args(srt=None), BAD_ARG),
    ("null_workspace", commit_args(ws=None), BAD_ARG),
    ("B0", commit_args(B=0), BAD_ARG),
    ("N0", commit_args(N=0), BAD_ARG),
    ("K_neg", commit_args(K=-3), BAD_ARG),
    ("group_not_dividing_B", commit_args(group=3), BAD_ARG),
    ("it_neg", commit_args(it=-1), BAD_ARG),
    ("null_before_K", commit_args(lab=None, K=8193), BAD_ARG),
    ("K8193", commit_args(K=8193), UNSUPPORTED),
    ("K8193_before_workspace", commit_args(K=8193, nb=16), UNSUPPORTED),
    ("short_workspace", commit_args(nb=None), WORKSPACE),
]

FINISH_CASES = [
    ("null_c_init", fin_args(c0=None), BAD_ARG),
    ("null_work_a", fin_args(ca=None), BAD_ARG),
    ("null_work_b", fin_args(cb=None), BAD_ARG),
    ("null_out", fin_args(out=None), BAD_ARG),
    ("null_n_iters", fin_args(n=None), BAD_ARG),
    ("null_workspace", fin_args(ws=None), BAD_ARG),
    ("B0", fin_args(B=0), BAD_ARG),
    ("K0", fin_args(K=0), BAD_ARG),
    ("group_not_dividing_B", fin_args(group=3), BAD_ARG),
    ("group_before_D", fin_args(group=3, D=96), BAD_ARG),
    ("K8193", fin_args(K=8193), UNSUPPORTED),
    ("D96", fin_args(D=96), UNSUPPORTED),
    ("dtype_f32", fin_args(dtype=2), UNSUPPORTED),
    ("dtype_before_workspace", fin_args(dtype=2, nb=16), UNSUPPORTED),
    ("short_workspace", fin_args(nb=16), WORKSPACE),
    ("workspace_before_alias", fin_args(nb=16, out=PB), WORKSPACE),
    ("out_is_work_a", fin_args(out=PB), BAD_ARG),
    ("out_is_work_b", fin_args(out=PC), BAD_ARG),
    ("c_init_is_work_a", fin_args(ca=PA), BAD_ARG),
    ("work_a_is_work_b", fin_args(cb=PB), BAD_ARG),
]


def _short(a, pos, dims):
    """a workspace size of None: one byte less than the entry asks for"""
    if a[pos] is None:
        a = list(a)
        a[pos] = int(nat.load().svg_kmeans_stepped_workspace_bytes(*dims(a))) - 1
        assert a[pos] > 0
    return a


@pytest.mark.parametrize("a,expected", [c[1:] for c in ITERATE_CASES], ids=[c[0] for c in ITERATE_CASES])
def test_iterate_rejects(a, expected):
    host_only()
    a = _short(a, 14, lambda a: (a[7], a[8], a[9], a[10], a[12]))
    assert nat.load().svg_kmeans_stepped_iterate(*a) == expected


@pytest.mark.parametrize("a,expected", [c[1:] for c in COMMIT_CASES], ids=[c[0] for c in COMMIT_CASES])
def test_commit_rejects(a, expected):
    host_only()
    a = _short(a, 11, lambda a: (a[6], a[7], a[8], 128, a[9]))
    assert nat.load().svg_kmeans_stepped_commit(*a) == expected


@pytest.mark.parametrize("a,expected", [c[1:] for c in FINISH_CASES], ids=[c[0] for c in FINISH_CASES])
def test_finish_rejects(a, expected):
    host_only()
    assert nat.load().svg_kmeans_stepped_finish(*a) == expected


# ---------------------------------------------------------------------------------------------------------
# the driver with torch stand-ins for the sides
# ---------------------------------------------------------------------------------------------------------
def _step_fn(x):
    """one Lloyd iteration of the oracle on x [B, N, D] in the form lloyd_device_rule takes (tests/test_svg2_batch_cpu.py)"""
    xsq = O.kmeans_xsq(x)

    def step(cur, it):
        labels = O.kmeans_assign(x, xsq, cur)
        c_new, counts = O.kmeans_update(x, labels, cur)
        shift = (c_new.float() - cur.float()).norm(dim=-1).amax(dim=1)
        return c_new, labels.to(torch.int32), counts, O.stable_argsort(labels).to(torch.int32), shift

    return step


def _data(B, N, D, gen, modes=6):
    centers = torch.randn(B, modes, D, generator=gen) * 2.0
    lab = torch.randint(0, modes, (B, N), generator=gen)
    return (torch.gather(centers, 1, lab[..., None].expand(-1, -1, D)) + 0.3 * torch.randn(B, N, D, generator=gen)).to(torch.bfloat16)


def _two_videos(H, N, D, gen):
    """video 0 converges early, video 1 (noise) does not"""
    return torch.cat([_data(H, N, D, gen), torch.randn(H, N, D, generator=gen).to(torch.bfloat16)])


ITERS, TOL = 12, 1e-3


@pytest.mark.parametrize("group", [None, 3])
def test_one_side_equals_the_device_rule(group):
    from svg.kmeans_utils import lloyd_device_rule, lloyd_stepped

    x = _two_videos(3, 300, 32, torch.Generator().manual_seed(4))
    init = x[:, :5].clone()
    side = TorchSteppedSide(_step_fn(x), init, TOL, group=group)
    (got,) = lloyd_stepped([side], side.maxima, ITERS)
    want = lloyd_device_rule(_step_fn(x), init, ITERS, TOL, group=group)
    assert same_five(got, want)
    if group:
        assert int(want[4][0]) < ITERS == int(want[4][1])        # a group that stops while the other runs on
    assert side.calls == [(w, it) for it in range(ITERS) for w in ("iterate", "commit")] + [("finish",)]
    assert torch.equal(init, x[:, :5])


@pytest.mark.parametrize("group", [None, 3])
def test_two_sides_under_one_reduce_equal_two_loops(group):
    from svg.kmeans_utils import lloyd_device_rule, lloyd_stepped

    gen = torch.Generator().manual_seed(5)
    xq, xk = _two_videos(3, 300, 32, gen), _two_videos(3, 260, 32, gen).flip(0)   # (k side: the other video converges)
    iq, ik = xq[:, :5].clone(), xk[:, :7].clone()
    G = 1 if group is None else 2
    maxima = torch.full((2 * G,), float("nan"))
    seen = []

    def red(t):   # an element-wise reduce: a scripted peer that is 1.5 x our own shift
        seen.append(tuple(t.shape))
        return t.mul_(1.5)

    sides = [TorchSteppedSide(_step_fn(xq), iq, TOL, group=group, maxima=maxima[:G]),
             TorchSteppedSide(_step_fn(xk), ik, TOL, group=group, maxima=maxima[G:])]
    order = []
    got = lloyd_stepped(sides, maxima, ITERS, shift_reduce=red, beside=lambda runs: order.append(len(runs)) or [f() for f in runs])
    assert seen == [(2 * G,)] * ITERS and order == [2] * ITERS                    # ONE reduce per iteration for both sides
    one = (lambda t: t.mul_(1.5))
    assert same_five(got[0], lloyd_device_rule(_step_fn(xq), iq, ITERS, TOL, group=group, shift_reduce=one))
    assert same_five(got[1], lloyd_device_rule(_step_fn(xk), ik, ITERS, TOL, group=group, shift_reduce=one))


def test_a_reduce_that_returns_a_new_tensor_is_copied_back():
    from svg.kmeans_utils import lloyd_device_rule, lloyd_stepped

    x = _two_videos(2, 200, 32, torch.Generator().manual_seed(6))
    init = x[:, :4].clone()
    own = int(lloyd_device_rule(_step_fn(x), init, ITERS, TOL, group=2)[4][0])
    assert own + 2 < ITERS
    peer = torch.zeros(ITERS, 2)
    peer[:own + 1, 0] = 1.0                                                       # group 0's peer converges two iterations after us
    for nan_peer in (False, True):
        if nan_peer:
            peer[:, 0] = float("nan")                                             # ... or never: torch.maximum propagates the NaN

        def make():
            its = iter(range(ITERS))
            return lambda t: torch.maximum(t, peer[next(its)])

        side = TorchSteppedSide(_step_fn(x), init, TOL, group=2)
        (got,) = lloyd_stepped([side], side.maxima, ITERS, shift_reduce=make())
        want = lloyd_device_rule(_step_fn(x), init, ITERS, TOL, group=2, shift_reduce=make())
        assert same_five(got, want)
        assert int(got[3][0]) == (ITERS if nan_peer else own + 2)


def _rank_worker(rank, world):
    from svg.distributed import shard_heads
    from svg.kmeans_utils import lloyd_device_rule, lloyd_stepped

    import torch.distributed as dist

    gen = torch.Generator().manual_seed(4)
    cfg, H, N, D = 2, 5, 300, 32
    xq, xk = _two_videos(H, N, D, gen), _two_videos(H, N, D, gen)
    iq, ik = xq[:, :5].clone(), xk[:, :6].clone()
    full = [lloyd_device_rule(_step_fn(x), i, ITERS, TOL, group=H) for x, i in ((xq, iq), (xk, ik))]
    mine = shard_heads(H, rank, world)
    rows = torch.tensor([c * H + h for c in range(cfg) for h in mine])
    calls = []

    def red(t):
        calls.append(tuple(t.shape))
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t

    maxima = torch.full((2 * cfg,), float("nan"))
    sides = [TorchSteppedSide(_step_fn(xq[rows]), iq[rows], TOL, group=len(mine), maxima=maxima[:cfg]),
             TorchSteppedSide(_step_fn(xk[rows]), ik[rows], TOL, group=len(mine), maxima=maxima[cfg:])]
    got = lloyd_stepped(sides, maxima, ITERS, shift_reduce=red)
    ok = calls == [(2 * cfg,)] * ITERS                                            # max_iters all-reduces, not 2 * max_iters
    for (lab, cent, cnt, n, srt), (rl, rc, rk, rs, rn) in zip(got, full):
        ok &= torch.equal(lab, rl[rows]) and torch.equal(cent.view(torch.int16), rc[rows].view(torch.int16)) and torch.equal(cnt, rk[rows])
        ok &= torch.equal(srt, rs[rows]) and torch.equal(n.to(torch.int64), rn)
        ok &= int(rn[0]) < ITERS == int(rn[1])
    return bool(ok), len(calls)


@pytest.mark.parametrize("world", [2, 3])
def test_head_shards_on_gloo_ranks_one_all_reduce_per_iteration(world):
    got = gloo_ranks.run_ranks(_rank_worker, world, 33700)
    assert got == {r: (True, ITERS) for r in range(world)}
