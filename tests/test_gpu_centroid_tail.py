"""The centroid tail on the GPU (include/svg_attn_centroid_tail.h) against the float64 statements of tests/centroid_tail_cases.py, on
poisoned allocations: svg_cluster_means (exact on integers, within one rounding step on real values, views read in place),
svg_centroid_tail_attention_lse (what it writes and what it leaves), the protocol sparse + tail + merge, the case where that protocol IS
dense attention, and svg2_sparse_attention(centroid_tail=True) against the statement rebuilt from the call's own labels and map.  The
bounds are those of tests/sparse_lse_cases.py (T_SINGLE, check_lse, merged_limit with the factor 2 of its two-part merges)."""
import json

import pytest
import torch

import centroid_tail_cases as TC
from poisoned import assert_fully_written, unwritten
from sparse_lse_cases import T_SINGLE, check_lse, merged_limit, rel_l2
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
NINF = float("-inf")


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def opt(t):
    return None if t is None else dev(t)


# ---------------------------------------------------------------------------------------------------------
# 1. svg_cluster_means
# ---------------------------------------------------------------------------------------------------------
POW2 = [1, 2, 4, 0, 8, 16, 32, 64, 128, 256, 0, 512]        # 1022 rows and two empty clusters; + one row no cluster owns


def means_case(Dm, dtype, integers, B=3):
    g = torch.Generator().manual_seed(Dm + (1 if integers else 0) + (3 if dtype == torch.float16 else 0))
    N = sum(POW2) + 1
    sizes = torch.stack([torch.tensor(POW2)[torch.randperm(len(POW2), generator=g)] for _ in range(B)]).to(torch.int32)
    x = (torch.randint(-8, 9, (B, N, Dm), generator=g).float() if integers else torch.randn(B, N, Dm, generator=g)).to(dtype)
    idx = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).to(torch.int32)
    return x, idx, sizes, TC.means64(x, TC.labels_from_sizes(sizes, idx, N), len(POW2))


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
@pytest.mark.parametrize("Dm", [64, 128])
def test_cluster_means_is_the_float64_mean_rounded_once_on_integers(nat, Dm, dtype):
    x, idx, sizes, ref = means_case(Dm, dtype, True)
    got = nat.cluster_means(dev(x), dev(idx), dev(sizes))
    assert_fully_written(got, "means")
    assert got.shape == (3, len(POW2), Dm) and got.dtype == dtype
    assert torch.equal(got.cpu(), ref.to(dtype))
    assert (got.cpu()[sizes == 0] == 0).all() and int((sizes == 0).sum()) == 6              # empty clusters: zeros


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
@pytest.mark.parametrize("Dm", [64, 128])
def test_cluster_means_on_real_values_is_that_value_or_an_adjacent_one(nat, Dm, dtype):
    x, idx, sizes, ref = means_case(Dm, dtype, False)
    got = nat.cluster_means(dev(x), dev(idx), dev(sizes)).cpu()
    want = ref.to(dtype)
    step = (got.view(torch.int16).int() - want.view(torch.int16).int()).abs()               # one step of the format, same sign
    same_sign = (got.view(torch.int16) < 0) == (want.view(torch.int16) < 0)
    ok = (got == want) | (same_sign & (step <= 1))
    print(f"cluster_means D {Dm} {dtype}: {int((got != want).sum())} of {got.numel()} elements one step from the rounded float64 mean")
    assert ok.all(), int((~ok).sum())


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
def test_cluster_means_reads_a_token_major_view_in_place(nat, dtype):
    cfg, Hh, N, K = 2, 2, 333, 7
    g = torch.Generator().manual_seed(9)
    store = torch.randn(cfg, N, Hh, TC.D, generator=g).to(dtype).cuda()
    view = store.permute(0, 2, 1, 3)                                                        # [cfg, H, N, D], token-major in memory
    assert not view.is_contiguous()
    lab = torch.randint(0, K, (cfg * Hh, N), generator=g)
    idx = torch.argsort(lab, dim=1, stable=True).to(torch.int32)
    sizes = torch.stack([torch.bincount(l, minlength=K) for l in lab]).to(torch.int32)
    a = nat.cluster_means(view, dev(idx), dev(sizes))
    b = nat.cluster_means(view.contiguous().reshape(cfg * Hh, N, TC.D), dev(idx), dev(sizes))
    assert torch.equal(a, b)
    want = TC.means64(view.reshape(cfg * Hh, N, TC.D).cpu(), lab, K)
    assert rel_l2(a.cpu(), want) <= T_SINGLE[dtype]


# ---------------------------------------------------------------------------------------------------------
# 2. the tail entry against the float64 statement
# ---------------------------------------------------------------------------------------------------------
def run_tail(nat, c, **over):
    a = dict(c, **over)
    return nat.centroid_tail_attention(dev(a["q"]) if not a["q"].is_cuda else a["q"], dev(a["kbar"]), dev(a["vbar"]), dev(a["bmap"]),
                                       dev(a["q_sizes"]), dev(a["k_sizes"]), q_row_idx=opt(a["idx"]))


@pytest.mark.parametrize("with_idx", [False, True], ids=["sorted", "q_row_idx"])
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
@pytest.mark.parametrize("KC", TC.KCS)
def test_tail_matches_the_float64_statement(nat, KC, dtype, with_idx):
    c = TC.kernel_case(KC, dtype, with_idx, short=True)
    o_ref, lse_ref, cov = TC.kernel_reference(KC, dtype, with_idx, short=True)
    o, lse = run_tail(nat, c)
    assert o.shape == c["q"].shape and o.dtype == dtype and lse.shape == (TC.H, TC.S) and lse.dtype == torch.float32
    o, lse = o.cpu(), lse.cpu()
    # rows no block-row covers — and there is no row of the empty block-row — keep the poison; every other element is written
    assert int((~cov).sum()) == sum(TC.Q_SIZES) - (sum(TC.Q_SIZES[:-1]) + TC.SHORT_LAST)
    assert unwritten(o)[~cov].all() and unwritten(lse)[~cov].all()
    assert not unwritten(o)[cov].any() and not unwritten(lse)[cov].any()
    for h in range(TC.H):
        err = rel_l2(o[h][cov[h]], o_ref[h][cov[h]])
        print(f"tail KC {KC} {dtype} head {h}: rel_l2 {err:.3e} (limit {T_SINGLE[dtype]:.1e})")
        assert err <= T_SINGLE[dtype]
    check_lse(lse[cov], lse_ref[cov], dtype, f"tail KC {KC}")
    ones = TC.labels_from_sizes(c["q_sizes"], c["idx"], TC.S) == TC.ONES_ROW                # every cluster selected: nothing left for the tail
    assert int(ones.sum()) == TC.H * TC.Q_SIZES[TC.ONES_ROW]
    assert (lse[ones] == NINF).all() and (o[ones] == 0).all()
    assert torch.isfinite(lse[cov & ~ones]).all()


@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
def test_tail_reads_a_wider_map_and_a_strided_q_in_place(nat, dtype):
    """HunyuanVideo's map has two further columns; q may be a token-major view: the bits of the plain call"""
    KC = 70
    c = TC.kernel_case(KC, dtype, True)
    o, lse = run_tail(nat, c)
    assert_fully_written(o, "o")
    assert_fully_written(lse, "lse")
    wide = torch.cat([c["bmap"], ~c["bmap"][:, :, :2]], dim=2)
    o_w, lse_w = run_tail(nat, c, bmap=wide)
    assert torch.equal(o, o_w) and torch.equal(lse, lse_w)
    store = c["q"].transpose(0, 1).contiguous().cuda()                                      # [S, H, D]
    view = store.transpose(0, 1)
    assert not view.is_contiguous()
    o_v, lse_v = run_tail(nat, c, q=view)
    assert o_v.is_contiguous() and torch.equal(o, o_v) and torch.equal(lse, lse_v)
    q4 = c["q"].cuda().reshape(1, TC.H, TC.S, TC.D)                                         # [cfg, H, S, D]: the shape of q
    o_4, lse_4 = run_tail(nat, c, q=q4)
    assert o_4.shape == q4.shape and lse_4.shape == q4.shape[:-1] and torch.equal(o, o_4[0]) and torch.equal(lse, lse_4[0])


# ---------------------------------------------------------------------------------------------------------
# 3. the merge protocol: varblock_attention(return_lse=True) + tail + merge_attention_states
# ---------------------------------------------------------------------------------------------------------
def protocol(nat, c, q_idx, kv_idx):
    q, k, v, bmap, qs, ks = (dev(c[n]) for n in ("q", "k", "v", "bmap", "q_sizes", "k_sizes"))
    o_s, lse_s = nat.varblock_attention(q, k, v, bmap, qs, ks, q_row_idx=opt(q_idx), kv_row_idx=opt(kv_idx), return_lse=True)
    o_t, lse_t = nat.centroid_tail_attention(q, dev(c["kbar"]), dev(c["vbar"]), bmap, qs, ks, q_row_idx=opt(q_idx))
    o, lse = nat.merge_attention_states([o_s, o_t], [lse_s, lse_t], return_lse=True)
    return o, lse, o_s, lse_s, lse_t


@pytest.mark.parametrize("with_idx", [False, True], ids=["sorted", "row_idx"])
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
@pytest.mark.parametrize("KC", TC.KCS)
def test_sparse_plus_tail_merged_matches_the_float64_statement(nat, KC, dtype, with_idx):
    c = TC.merge_case(KC, dtype, with_idx)
    st = TC.merge_reference(KC, dtype, with_idx)
    o, lse, o_s, lse_s, lse_t = protocol(nat, c, c["q_idx"], c["kv_idx"])
    limit, r = merged_limit(st["o"].float(), dtype)
    err = rel_l2(o.cpu(), st["o"].float())
    print(f"sparse + tail KC {KC} {dtype}: merged rel_l2 {err:.3e} (limit {limit:.3e}; one rounding {r:.3e})")
    assert err <= limit
    check_lse(lse, st["lse"], dtype, f"merged KC {KC}", factor=2.0)
    ql = TC.labels_from_sizes(c["q_sizes"], c["q_idx"], TC.S)
    ones, zeros = ql == TC.ONES_ROW, ql == TC.ZEROS_ROW
    assert (lse_t.cpu()[ones] == NINF).all() and torch.equal(o.cpu()[ones], o_s.cpu()[ones])          # no tail: the sparse part's bits
    assert torch.equal(lse.cpu()[ones], lse_s.cpu()[ones])
    assert (lse_s.cpu()[zeros] == NINF).all() and torch.isfinite(lse.cpu()[zeros]).all()              # no sparse key: the tail alone
    got = nat.cluster_means(dev(c["k"]), dev(torch.argsort(TC.labels_from_sizes(c["k_sizes"], c["kv_idx"], TC.S), dim=1, stable=True).to(torch.int32)),
                            dev(c["k_sizes"]))
    assert rel_l2(got.cpu(), c["kbar"]) <= 2.0 ** -8                                                 # the library's means are the statement's


# ---------------------------------------------------------------------------------------------------------
# 4. exact by construction: the protocol IS dense attention
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", TC.DTYPES, ids=str)
def test_on_clusters_of_identical_rows_the_protocol_is_dense_attention(nat, dtype):
    c = TC.exact_case(dtype)
    o_d, lse_d = TC.exact_reference(dtype)
    o, lse, o_s, lse_s, lse_t = protocol(nat, c, None, None)
    assert_fully_written(o, "o")
    limit, r = merged_limit(o_d.float(), dtype)
    err, err_s = rel_l2(o.cpu(), o_d.float()), rel_l2(o_s.cpu(), o_d.float())
    print(f"exact {dtype}: merged rel_l2 to DENSE {err:.3e} (limit {limit:.3e}; one rounding {r:.3e}); the sparse part alone {err_s:.3e}")
    assert err <= limit < err_s
    check_lse(lse, lse_d, dtype, "exact merged", factor=2.0)
    assert torch.isfinite(lse_t).all() and torch.isfinite(lse_s).all()


# ---------------------------------------------------------------------------------------------------------
# layer level: svg2_sparse_attention(centroid_tail=True)
# ---------------------------------------------------------------------------------------------------------
def layer_call(_core, kind, q, k, v, **kw):
    geo = TC.GEOMETRIES[kind]
    torch.manual_seed(5)
    torch.cuda.manual_seed(5)
    return _core.svg2_sparse_attention(q, k, v, _core.Geometry(geo["ctx"], TC.F_, TC.P_), _core.CentroidStore(), 0, TC.QC, TC.KC_LAYER, TC.TOP_P,
                                       TC.MIN_KC_RATIO, TC.ITER_INIT, TC.ITER_STEP, prompt_length=geo["prompt"], **kw)


@pytest.fixture
def captured(monkeypatch):
    """the labels and the map of every svg2_sparse_attention call, as the call itself computed them"""
    from svg.models import _core

    seen = []
    km, dm = _core.kmeans_clustering, _core.identify_dynamic_map

    def kmeans(*a, **kw):
        res = km(*a, **kw)
        seen.append(dict(ql=res[0][0].long().cpu(), kl=res[1][0].long().cpu()))
        return res

    def dynmap(*a, **kw):
        res = dm(*a, **kw)
        seen[-1]["map"] = res.bool().cpu()
        return res

    monkeypatch.setattr(_core, "kmeans_clustering", kmeans)
    monkeypatch.setattr(_core, "identify_dynamic_map", dynmap)
    return seen


@pytest.mark.parametrize("cfg", [1, 2])
@pytest.mark.parametrize("kind", sorted(TC.GEOMETRIES))
def test_layer_call_matches_the_statement_rebuilt_from_its_own_labels(nat, captured, kind, cfg):
    from svg.models import _core

    dtype = torch.bfloat16
    geo = TC.GEOMETRIES[kind]
    q, k, v = TC.layer_inputs(kind, cfg, dtype)
    qd, kd, vd = dev(q), dev(k), dev(v)
    never = layer_call(_core, kind, qd, kd, vd)
    off = layer_call(_core, kind, qd, kd, vd, centroid_tail=False)
    on = layer_call(_core, kind, qd, kd, vd, centroid_tail=True)
    assert torch.equal(off, never)                                                                    # off: the bits of a call without the keyword
    assert on.shape == q.shape and not unwritten(on).any()
    assert all(torch.equal(captured[0][n], c[n]) for c in captured[1:] for n in ("ql", "kl", "map"))  # the three calls clustered alike
    cap, Hh, real = captured[2], TC.LAYER_H, TC.V + geo["prompt"]
    assert not bool(cap["map"].all())
    for b in range(cfg):
        hs = slice(b * Hh, (b + 1) * Hh)
        st = TC.layer_statement(kind, q[b], k[b], v[b], cap["ql"].reshape(cfg * Hh, -1)[hs], cap["kl"].reshape(cfg * Hh, -1)[hs], cap["map"][b], dtype)
        limit, r = merged_limit(st["o"].float(), dtype)
        err = rel_l2(on[b].cpu(), st["o"].float())
        o_d, _ = TC.dense64(q[b][:, :real], k[b][:, :real], v[b][:, :real])
        e_on, e_off = rel_l2(on[b].cpu()[:, :TC.V], o_d[:, :TC.V]), rel_l2(off[b].cpu()[:, :TC.V], o_d[:, :TC.V])
        print(f"{kind} cfg {cfg} video {b}: rel_l2 to the statement {err:.3e} (limit {limit:.3e}; one rounding {r:.3e}); to dense attention on "
              f"the video rows: off {e_off:.4f} -> on {e_on:.4f}")
        assert err <= limit
        assert e_on < e_off
    if geo["ctx"]:   # the unused-prompt rows get no tail: the sparse part's values; the prompt rows select every video cluster: likewise
        assert torch.equal(on[:, :, real:], off[:, :, real:]) and torch.equal(on[:, :, TC.V:real], off[:, :, TC.V:real])
    assert not torch.equal(on[:, :, :TC.V], off[:, :, :TC.V])


def test_quality_record_is_measured_on_the_merged_state_and_says_so(nat, tmp_path):
    from svg.models import _core

    dtype = torch.bfloat16
    qd, kd, vd = (dev(x) for x in TC.layer_inputs("wan", 1, dtype))
    recs = {}
    for on in (False, True):
        path = tmp_path / f"quality_{int(on)}.jsonl"
        layer_call(_core, "wan", qd, kd, vd, quality=_core.QualityRequest(str(path), 64), **({"centroid_tail": True} if on else {}))
        _core.flush_quality_log()
        recs[on] = json.loads(path.read_text().splitlines()[-1])
    assert "centroid_tail" not in recs[False] and recs[True]["centroid_tail"] is True
    kept = {on: torch.tensor(recs[on]["kept_mass"]).mean().item() for on in recs}
    err = {on: torch.tensor(recs[on]["rel_l2"]).mean().item() for on in recs}
    print(f"quality records: kept mass {kept[False]:.4f} -> {kept[True]:.4f}, rel. L2 {err[False]:.4f} -> {err[True]:.4f}")
    assert kept[True] > kept[False] and err[True] < err[False]
    assert recs[True]["density"] == recs[False]["density"]
