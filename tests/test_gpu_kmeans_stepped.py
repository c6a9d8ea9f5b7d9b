"""The Lloyd loop in steps on the GPU (include/svg_attn_kmeans_stepped.h; csrc/kmeans.hip: kmeans_commit_kernel<true>,
kmeans_group_maxima_kernel and the host steps kmeans_loop_impl shares with the three entries; svg._kmeans_stepped.KmeansSteppedSide,
svg.kmeans_utils.lloyd_stepped, svg.models._core.kmeans_clustering under a head shard).

1. With the maxima untouched the five results are those of _native.kmeans_loop(group=), bit for bit: shapes that are no multiple of a tile
   and have more than one workgroup per batch, both head_dims and dtypes, 1 / 2 / 5 iterations (the three roles of the centroid buffers),
   contiguous x and batches (N + 40) * D apart; every word of every output written on poisoned allocations, c_init untouched.
2. Early convergence: groups that stop, and a group that stops while another runs on, against the grouped loop and against each group alone.
3. An external reduce with a scripted peer (never converges, converges two iterations after us, NaN) and our own NaN shift, against
   lloyd_device_rule under the same reduce (batch_kmeans_Euclid with the switch off).
4. The layer-call under a head shard in one process: the bits of the unsharded call, and a transcript of the library calls.
5. Two gloo ranks on one GPU, head-shard and token-shard mode: every rank's rows equal the single-process call, one all-reduce per iteration.

Every comparison is torch.equal: a rank runs the single-GPU kernels, nothing has a tolerance."""
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import kmeans_exact_cases as KC
from poisoned import assert_fully_written

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TOL = 1e-4


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def _bits(t):
    return t.view(torch.int16)


def _stepped(nat, x, c0, iters, group, tol=TOL, reduce=None):
    """one side through the driver -> (labels, centroids, counts, n_iters, sorted_idx), the side"""
    from svg._kmeans_stepped import KmeansSteppedSide
    from svg.kmeans_utils import lloyd_stepped

    side = KmeansSteppedSide(x, c0, tol, group=group)
    (out,) = lloyd_stepped([side], side.maxima, iters, shift_reduce=reduce)
    return out, side


def _same_as_loop(got, want):
    lab, cent, cnt, n, srt = got
    wl, wc, wk, wn, ws = want
    return (torch.equal(lab, wl) and torch.equal(_bits(cent), _bits(wc)) and torch.equal(cnt, wk) and torch.equal(srt, ws)
            and n.shape == wn.shape and n.dtype == wn.dtype and torch.equal(n, wn))


# ---------------------------------------------------------------------------------------------------------
# 1. identity reduce: the bits of the grouped library loop
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "batch_strided"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(2, 257, 65, 128, 2), (4, 700, 129, 64, 2), (3, 4000, 24, 128, 3)], ids=lambda s: "x".join(map(str, s)))
def test_identity_reduce_equals_the_library_loop(nat, shape, dtype, strided):
    B, N, K, D, group = shape
    g = torch.Generator().manual_seed(B * N + K)
    base = torch.randn(B, N + 40, D, generator=g).to(dtype).cuda()
    x = base[:, :N] if strided else base[:, :N].contiguous()
    assert x.stride(0) == ((N + 40) * D if strided else N * D)
    c0 = x[:, :K].contiguous()
    c0_before = c0.clone()
    for iters in (1, 2, 5):
        want = nat.kmeans_loop(x, None, c0, iters, TOL, group=group)
        got, side = _stepped(nat, x, c0, iters, group)
        torch.cuda.synchronize()
        assert side.x.data_ptr() == x.data_ptr()                                   # read in place
        for name, t in zip(("labels", "centroids", "counts", "n_iters", "sorted_idx"), got):
            assert_fully_written(t, f"{name} after {iters} iterations")
        assert_fully_written(side.maxima, "maxima")
        assert _same_as_loop(got, want), (shape, dtype, strided, iters)
        assert torch.equal(_bits(c0), _bits(c0_before))


# ---------------------------------------------------------------------------------------------------------
# 2. early convergence
# ---------------------------------------------------------------------------------------------------------
def _early_exit_case():
    """the blobs and c0 of tests/test_gpu_kernels.py test_kmeans_loop_early_exit"""
    B, N, K, D = 4, 3000, 16, 128
    x, centers = KC._blobs(B, N, K, D, 0.3, seed=5)
    c0 = (centers.float() + 0.2 * torch.randn(B, K, D, generator=torch.Generator().manual_seed(6))).to(torch.bfloat16)
    return x.cuda(), c0.cuda(), K


def test_groups_that_converge_stop_where_the_library_loop_stops(nat):
    x, c0, K = _early_exit_case()
    want = nat.kmeans_loop(x, None, c0, 20, TOL, group=2)
    got, _ = _stepped(nat, x, c0, 20, 2)
    torch.cuda.synchronize()
    assert _same_as_loop(got, want)
    assert got[3].shape == (2,) and 2 <= int(got[3].min()) and int(got[3].max()) <= 6   # (the oracle's range of that test)


def test_a_group_that_stops_while_another_runs_on(nat):
    """group 0: the separated blobs started next to their centres (stops after two iterations on the oracle); group 1: spread 1.2, started
    from its own first rows (the oracle's shift is 17.9 at iteration 3 and 0 from iteration 5 on)"""
    N, K, D = 3000, 16, 128
    xa, ca = KC._blobs(2, N, K, D, 0.3, seed=5)
    xb, _ = KC._blobs(2, N, K, D, 1.2, seed=7)
    c0a = (ca.float() + 0.2 * torch.randn(2, K, D, generator=torch.Generator().manual_seed(6))).to(torch.bfloat16)
    x, c0 = torch.cat([xa, xb]).cuda(), torch.cat([c0a, xb[:, :K]]).cuda()
    want = nat.kmeans_loop(x, None, c0, 8, TOL, group=2)
    got, _ = _stepped(nat, x, c0, 8, 2)
    torch.cuda.synchronize()
    assert _same_as_loop(got, want)
    n = got[3].tolist()
    assert n[0] < n[1] <= 8 and n[0] <= 6, n
    for g in (0, 1):   # ... and a call on each group alone
        sl = slice(2 * g, 2 * g + 2)
        alone, _ = _stepped(nat, x[sl], c0[sl], 8, None)
        torch.cuda.synchronize()
        assert alone[3].shape == () and int(alone[3]) == n[g]
        for i in (0, 1, 2, 4):
            assert torch.equal(_bits(alone[i]) if i == 1 else alone[i], _bits(got[i][sl]) if i == 1 else got[i][sl]), (g, i)


# ---------------------------------------------------------------------------------------------------------
# 3. an external reduce: lloyd_device_rule under the same reduce
# ---------------------------------------------------------------------------------------------------------
def _both_paths(monkeypatch, x, c0, K, iters, make_reduce, group, tol=TOL):
    """batch_kmeans_Euclid(check_every=0, shift_reduce=) with the switch on (the stepped driver) and off (lloyd_device_rule on
    svg_kmeans_iter) -> the two results, each (labels, centroids, counts, n_iters, sorted indices)"""
    from svg import kmeans_utils as ku

    ran = {"rule": 0, "stepped": 0}
    real_rule, real_stepped = ku.lloyd_device_rule, ku.lloyd_stepped
    monkeypatch.setattr(ku, "lloyd_device_rule", lambda *a, **kw: (ran.__setitem__("rule", ran["rule"] + 1), real_rule(*a, **kw))[1])
    monkeypatch.setattr(ku, "lloyd_stepped", lambda *a, **kw: (ran.__setitem__("stepped", ran["stepped"] + 1), real_stepped(*a, **kw))[1])
    out = []
    for on in (True, False):
        monkeypatch.setattr(ku, "STEPPED_LOOP_UNDER_SHARDS", on)
        out.append(ku.batch_kmeans_Euclid(x, K, max_iters=iters, tol=tol, init_centroids=c0, check_every=0, return_sorted_indices=True,
                                          shift_reduce=make_reduce(), group=group))
        assert ran == ({"rule": 0, "stepped": 1} if on else {"rule": 1, "stepped": 1}), (on, ran)
    torch.cuda.synchronize()
    return out


def _equal_results(a, b):
    return all(torch.equal(_bits(s) if s.dtype in (torch.bfloat16, torch.float16) else s, _bits(t) if t.dtype in (torch.bfloat16, torch.float16) else t)
               and s.shape == t.shape and s.dtype == t.dtype for s, t in zip(a, b))


def _scripted(peer):
    """shift_reduce = max(t, peer[it]) — a new tensor, which the driver copies back; torch.maximum propagates a NaN of the peer"""
    def make():
        its = iter(range(len(peer)))
        return lambda t: torch.maximum(t, peer[next(its)].view(t.shape))
    return make


@pytest.mark.parametrize("strided", [False, True], ids=["contiguous", "batch_strided"])
def test_scripted_peers(nat, monkeypatch, strided):
    x, c0, K = _early_exit_case()
    if strided:
        base = torch.zeros(4, 3040, 128, dtype=x.dtype, device="cuda")
        base[:, :3000] = x
        x = base[:, :3000]
    iters = 10
    own = nat.kmeans_loop(x, None, c0, iters, TOL, group=2)
    n_own = own[3].tolist()
    assert max(n_own) + 2 < iters
    # a peer that never converges: every iteration runs, the centroids are one update ahead of the labels
    never = torch.ones(iters, 2, device="cuda")
    a, b = _both_paths(monkeypatch, x, c0, K, iters, _scripted(never), 2)
    assert _equal_results(a, b) and a[3].tolist() == [iters, iters]
    assert int(a[2].min()) > 0                                                      # (no empty cluster: the update does not read the old centroids)
    ahead = nat.kmeans_update(x.contiguous(), a[0].to(torch.int32).contiguous(), c0)[0]
    assert torch.equal(_bits(a[1]), _bits(ahead))                                  # the update of the returned labels
    # a peer that converges two iterations after us: the loop stops there
    later = torch.zeros(iters, 2, device="cuda")
    for g in (0, 1):
        later[:n_own[g] + 1, g] = 1.0
    a, b = _both_paths(monkeypatch, x, c0, K, iters, _scripted(later), 2)
    assert _equal_results(a, b) and a[3].tolist() == [n + 2 for n in n_own]
    # a NaN peer on group 1: that group never stops, group 0 stops on its own
    nan = torch.zeros(iters, 2, device="cuda")
    nan[:, 1] = float("nan")
    a, b = _both_paths(monkeypatch, x, c0, K, iters, _scripted(nan), 2)
    assert _equal_results(a, b) and a[3].tolist() == [n_own[0], iters]
    # one stopping rule over all batches: the reduce sees a 0-dim maximum on both paths
    a, b = _both_paths(monkeypatch, x, c0, K, iters, _scripted(later[:, 0]), None)
    assert _equal_results(a, b) and a[3].shape == () and int(a[3]) == max(n_own[0] + 2, max(n_own))


@pytest.mark.parametrize("pattern", sorted(KC.NAN_PATTERNS))
def test_our_own_nan_shift_never_converges(nat, monkeypatch, pattern):
    s = KC.NAN_SHAPE
    x, c0 = (t.cuda() for t in KC.nan_case())
    xn = KC.nan_case(pattern)[0].cuda()
    clean = nat.kmeans_loop(x, None, c0, KC.NAN_MAX_ITERS, KC.NAN_TOL, group=1)[3].tolist()
    assert max(clean) < KC.NAN_MAX_ITERS
    a, b = _both_paths(monkeypatch, xn, c0, s["K"], KC.NAN_MAX_ITERS, lambda: (lambda t: t), 1, tol=KC.NAN_TOL)
    assert _equal_results(a, b) and a[3].tolist() == [clean[0], KC.NAN_MAX_ITERS]
    a, b = _both_paths(monkeypatch, xn, c0, s["K"], KC.NAN_MAX_ITERS, lambda: (lambda t: t), None, tol=KC.NAN_TOL)
    assert _equal_results(a, b) and int(a[3]) == KC.NAN_MAX_ITERS


# ---------------------------------------------------------------------------------------------------------
# 4. the layer-call under a head shard, one process
# ---------------------------------------------------------------------------------------------------------
class RecordingLibrary:
    """passes every call on to libsvgattn and keeps (name, args)"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def entry(*args):
            self.calls.append((name, args))
            return fn(*args)
        return entry


GEOMETRIES = {"wan": dict(H=3, F=5, P=300, ctx=0, L=0), "hunyuan": dict(H=3, F=4, P=200, ctx=40, L=11)}
ITER_INIT, ITER_STEP, QC, KC_ = 3, 2, 12, 30


def _qkv(cfg, H, S, D, seed, dev="cuda"):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(cfg, H, S, D, generator=g).to(torch.bfloat16).to(dev) for _ in range(3))


def _layer_calls(_core, q, k, v, geo, L, **kw):
    """a first call (random initial points, ITER_INIT iterations) and a warm-started call (ITER_STEP) of one layer"""
    store, outs = _core.CentroidStore(), []
    for call in range(2):
        torch.manual_seed(5 + call)
        torch.cuda.manual_seed(5 + call)
        outs.append(_core.svg2_sparse_attention(q, k, v, geo, store, 0, QC, KC_, 0.9, 0.1, ITER_INIT, ITER_STEP, prompt_length=L, **kw))
    return outs


@pytest.mark.parametrize("cfg", [1, 2])
@pytest.mark.parametrize("model", sorted(GEOMETRIES))
def test_layer_call_under_a_head_shard_in_one_process(nat, monkeypatch, model, cfg):
    from svg import distributed as sd
    from svg import kmeans_utils as ku
    from svg.models import _core

    geo_ = GEOMETRIES[model]
    H, D, ctx, L = geo_["H"], 128, geo_["ctx"], geo_["L"]
    S = geo_["F"] * geo_["P"] + ctx
    q, k, v = _qkv(cfg, H, S, D, 3)
    geo = _core.Geometry(ctx, geo_["F"], geo_["P"])
    maps = []
    real_map = _core.identify_dynamic_map
    monkeypatch.setattr(_core, "identify_dynamic_map", lambda *a, **kw: (maps.append(real_map(*a, **kw)), maps[-1])[1])
    want = _layer_calls(_core, q, k, v, geo, L)
    want_maps, maps[:] = list(maps), []
    reduces = []
    monkeypatch.setattr(sd, "all_reduce_max_", lambda t: (reduces.append(tuple(t.shape)), t)[1])
    rule_calls = []
    real_rule = ku.lloyd_device_rule
    monkeypatch.setattr(ku, "lloyd_device_rule", lambda *a, **kw: (rule_calls.append(1), real_rule(*a, **kw))[1])
    lib = RecordingLibrary(nat.load())
    monkeypatch.setattr(nat, "load", lambda strict=True: lib)
    G = 1 if cfg == 1 else cfg
    for on in (True, False):
        monkeypatch.setattr(ku, "STEPPED_LOOP_UNDER_SHARDS", on)
        lib.calls.clear(), reduces.clear(), rule_calls.clear(), maps.clear()
        got = _layer_calls(_core, q, k, v, geo, L, _head_shard=(0, H, H))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(got, want)) and all(torch.equal(a, b) for a, b in zip(maps, want_maps)), (model, cfg, on)
        assert len(maps) == 2
        km = [(n, a) for n, a in lib.calls if n.startswith("svg_kmeans") and not n.endswith("_workspace_bytes")]
        names = [n for n, _ in km]
        if on:
            per_call = lambda iters: (["svg_kmeans_stepped_iterate"] * 2 + ["svg_kmeans_stepped_commit"] * 2) * iters \
                + ["svg_kmeans_stepped_finish"] * 2                                                                        # noqa: E731
            assert names == per_call(ITER_INIT) + per_call(ITER_STEP) and not rule_calls
            assert reduces == [(2 * G,)] * (ITER_INIT + ITER_STEP)                 # one shift_reduce per iteration, both sides in it
            strides = {a[1] for n, a in km if n == "svg_kmeans_stepped_iterate"}
            assert strides == {S * D}                                              # heads S * D apart: with text behind the video, read in place
            its = [a[5] for n, a in km if n == "svg_kmeans_stepped_iterate"]
            assert its == [i for n_ in (ITER_INIT, ITER_STEP) for i in range(n_) for _ in (0, 1)]
        else:
            assert set(names) == {"svg_kmeans_iter"} and len(names) == 2 * (ITER_INIT + ITER_STEP) and len(rule_calls) == 4
            assert reduces == [(G,) if cfg > 1 else ()] * (2 * (ITER_INIT + ITER_STEP))


# ---------------------------------------------------------------------------------------------------------
# 5. two gloo ranks on one GPU, a fresh child process per rank
# ---------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, ret, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT), str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from svg import _native as nat_
    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    from svg import distributed as sd
    from svg import kmeans_utils as ku
    from svg.models import _core

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    ku.STEPPED_LOOP_UNDER_SHARDS = True       # (what this module tests, whatever the default is)
    reduces = []
    real = sd.dist.all_reduce

    def counting(t, *a, **kw):
        reduces.append(tuple(t.shape))
        return real(t, *a, **kw)

    res = {}
    for model, g_ in sorted(GEOMETRIES.items()):
        H, D, ctx, L = 5, 128, g_["ctx"], g_["L"]
        S = g_["F"] * g_["P"] + ctx
        q, k, v = _qkv(1, H, S, D, 3)
        geo = _core.Geometry(ctx, g_["F"], g_["P"])
        whole = _layer_calls(_core, q, k, v, geo, L)
        sd.dist.all_reduce = counting
        reduces.clear()
        if mode == "heads":
            sd.enable()
            got = _layer_calls(_core, q, k, v, geo, L)
            a, b = 0, S
        else:
            sd.enable_token_shards(unit=128)
            a, b = sd.token_shard_range(S)
            got = _layer_calls(_core, *(x[:, :, a:b].contiguous() for x in (q, k, v)), geo, L)
        sd.disable()
        sd.dist.all_reduce = real
        torch.cuda.synchronize()
        res[model] = dict(equal=[bool(torch.equal(x, y[:, :, a:b])) and bool(torch.isfinite(x.float()).all()) for x, y in zip(got, whole)],
                          reduces=list(reduces))
    ret[rank] = res
    dist.destroy_process_group()


@pytest.mark.parametrize("mode", ["heads", "tokens"])
def test_two_ranks_one_gpu(mode):
    world = 2
    ret = mp.Manager().dict()
    port = 41500 + (os.getpid() % 2000) + ["heads", "tokens"].index(mode)
    mp.spawn(_rank_worker, args=(world, port, ret, mode), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == [0, 1]
    for r in (0, 1):
        for model in GEOMETRIES:
            assert got[r][model]["equal"] == [True, True], (mode, r, model)
            # all-reduce calls per layer-call = its iterations, each over the q side's and the k side's maximum
            assert got[r][model]["reduces"] == [(2,)] * (ITER_INIT + ITER_STEP), (mode, r, model, got[r][model]["reduces"])
