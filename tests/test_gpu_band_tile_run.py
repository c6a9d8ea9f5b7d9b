"""The 16x16x32 band kernels with tile runs (csrc/band_policy.h BandPolicy::tile_run: inside a run the vector phase makes none of its
per-tile scalar decisions — tests/test_band_tile_run_cpu.py walks the runs of the same geometries on the host, tests/band_tile_run_cases.py)
against the fp32 oracle, at the tolerances of tests/test_gpu_m16.py.  Every case runs four heads of alternating kinds (contiguous,
token-major, token-major, contiguous) with the fused placement, in bf16 and fp16: the four model masks at three bands, text-first rows,
both dense modes, ragged lengths, a 16-row last q-tile, bands so short that a run is empty or one tile, and q-tiles of fewer key tiles than
the request distance needs.  The queue, switch, LSE and fp32-row entries run on a long-run, a merged-column, a short-run and a ragged
geometry; late spikes and very negative rows enter and leave runs on the exact path of the softmax and under replay.  The window entry
over the whole sequence opts out of runs and computes the same rows: its output and log-sum-exp are bit-identical to the LSE entry's."""
import functools

import pytest
import torch

import band_tile_run_cases as G
from oracle import svg_oracle as O
from test_gpu_kernels import check_attn, dev

pytestmark = pytest.mark.gpu
D = 128
BEST = torch.tensor([[0, 1, 1, 0]])   # head kinds: contiguous, token-major, token-major, contiguous
DTYPES = [torch.bfloat16, torch.float16]


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


def placed_reference(q, k, v, mask, best, ctx, F_, P_, tf):
    """the oracle's output for heads of the kinds `best`, in the order the device tensors are in"""
    qp, kp, vp = (O.head_placement(x, best, ctx, F_, P_, text_first=tf) for x in (q, k, v))
    return O.head_placement(O.masked_attention(qp, kp, vp, mask), best, ctx, F_, P_, inverse=True, text_first=tf)


@functools.lru_cache(maxsize=None)
def case(name, dtype):
    """-> S, mask parameters, placement keywords, (q, k, v) [1, 4, S, D] on the CPU, the oracle's output: computed once, never written to"""
    S, prm, vid0, F_, P_, ctx, tf = G.geometry(name)
    torch.manual_seed(len(name) * 131 + S)
    q, k, v = (torch.randn(1, 4, S, D).to(dtype) for _ in range(3))
    ref = placed_reference(q, k, v, O.band_mask(S, **prm), BEST, ctx, F_, P_, tf)
    return S, prm, dict(vid0=vid0, num_frame=F_, frame_size=P_), (q, k, v), ref


def perm_kw(kw, best=BEST):
    return dict(kw, head_perm_flag=dev(best))


def ids(dt):
    return str(dt)[6:]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", G.ALL_CASES)
def test_plain_entry(nat, name, dtype):
    S, prm, kw, (q, k, v), ref = case(name, dtype)
    nat.band_replays(reset=True)
    o = nat.band_attention(dev(q), dev(k), dev(v), nat.BandMask(**prm), **perm_kw(kw))
    print(f"{name} {ids(dtype)}: replays={nat.band_replays(reset=True)}")
    assert torch.isfinite(o.float()).all()
    check_attn(o, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_queue_entry(nat, dtype):
    """24 heads of the F = 5, P = 600 geometry: 312 q-tiles, more than the device has compute units — the resident kernel.  The heads are
    the four of the shared case, six times over; every copy must be the launch of four heads bit for bit, and that one meets the oracle."""
    S, prm, kw, (q, k, v), ref = case("hy_640", dtype)
    m = nat.BandMask(**prm)
    q24, k24, v24 = (dev(x.repeat(1, 6, 1, 1)) for x in (q, k, v))
    nat.band_replays(reset=True)
    o24 = nat.band_attention(q24, k24, v24, m, **perm_kw(kw, BEST.repeat(1, 6)))
    print(f"queue {ids(dtype)}: replays={nat.band_replays(reset=True)}")
    o4 = nat.band_attention(dev(q), dev(k), dev(v), m, **perm_kw(kw))
    check_attn(o4, ref, dtype)
    for r in range(6):
        assert torch.equal(o24[:, 4 * r:4 * r + 4], o4), r


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
@pytest.mark.parametrize("name", G.ENTRY_CASES)
def test_switch_lse_and_f32_entries(nat, name, dtype):
    S, prm, kw, (q, k, v), ref = case(name, dtype)
    m, alt = nat.BandMask(**prm), nat.BandMask(**O.dense_band_params(S))
    dq, dk, dv = dev(q), dev(k), dev(v)
    pk = perm_kw(kw)
    o = nat.band_attention(dq, dk, dv, m, **pk)
    check_attn(o, ref, dtype)
    # the device switch: flag 0 = the mask with the placement, flag 1 = the other mask without it; each the plain launch bit for bit
    for flag, want in ((0, o), (1, nat.band_attention(dq, dk, dv, alt))):
        got = nat.band_attention_switch(dq, dk, dv, m, alt, torch.tensor([flag], dtype=torch.int32, device="cuda"), **pk)
        assert torch.equal(got, want), flag
    # LSE form: the same rows bit for bit; fp32 rows: the same result before its rounding
    o_l, lse = nat.band_attention(dq, dk, dv, m, return_lse=True, **pk)
    assert torch.equal(o_l, o) and torch.isfinite(lse).all()
    o32, lse32 = nat.band_attention(dq, dk, dv, m, return_lse=True, out_dtype=torch.float32, **pk)
    assert o32.dtype == torch.float32 and torch.equal(lse32, lse)
    check_attn(o32, ref, dtype)


@pytest.mark.parametrize("name", ["hy_640", "dense_valid", "short_161", "last16"])
def test_window_over_the_whole_sequence_has_the_same_bits(nat, name):
    """the window policy keeps the per-tile decisions (no runs); over the whole sequence it computes what the LSE entry computes"""
    S, prm, _, (q, k, v), _ = case(name, torch.bfloat16)
    m = nat.BandMask(**prm)
    dq, dk, dv = dev(q), dev(k), dev(v)
    o, lse = nat.band_attention(dq, dk, dv, m, return_lse=True)       # every head contiguous: the window entry has no placement
    ow, lsew = nat.band_window_attention(dq, dk, dv, m, S, 0, 0)
    assert torch.equal(ow, o) and torch.equal(lsew, lse)
    check_attn(o, O.masked_attention(q, k, v, O.band_mask(S, **prm)), torch.bfloat16)


@pytest.mark.parametrize("spike", [30.0, 120.0, 400.0])
def test_late_spikes_inside_runs(nat, spike):
    """the spikes of tests/test_gpu_m16.py on a dense mask (one run over the whole segment), heads of both kinds: a run is left for the
    exact path of the softmax and re-entered; the largest ones overflow between two check points and the q-tile is replayed"""
    torch.manual_seed(11)
    F_, P_, H = 5, 300, 4
    S = F_ * P_
    q, k, v = (torch.randn(1, H, S, D) for _ in range(3))
    scale = 1.0 / D ** 0.5
    for (qi, ki) in [(5, 900), (300, 1340), (301, 70), (1400, 1499), (1401, 3), (17, 18), (31, 1200)]:
        for h in range(H):
            qd = q[0, h, qi]
            k[0, h, ki] = qd / qd.norm() ** 2 * (spike / scale)
    q, k, v = (x.to(torch.bfloat16) for x in (q, k, v))
    nat.band_replays(reset=True)
    o = nat.band_attention(dev(q), dev(k), dev(v), nat.BandMask(**O.dense_band_params(S)), vid0=0, num_frame=F_, frame_size=P_,
                           head_perm_flag=dev(BEST))
    print(f"spike {spike}: replays={nat.band_replays(reset=True)}")
    assert torch.isfinite(o.float()).all()
    check_attn(o, placed_reference(q, k, v, None, BEST, 0, F_, P_, False), torch.bfloat16)


def test_very_negative_rows(nat):
    torch.manual_seed(13)
    F_, P_, H = 4, 300, 4
    S = F_ * P_
    u = torch.randn(D)
    u = u / u.norm()
    a = (150.0 * D ** 0.5) ** 0.5
    q = (-a * u + 0.5 * torch.randn(1, H, S, D)).to(torch.bfloat16)
    k = (a * u + 0.5 * torch.randn(1, H, S, D)).to(torch.bfloat16)
    v = torch.randn(1, H, S, D).to(torch.bfloat16)
    for prm in (O.dense_band_params(S), dict(real_len=S, band=200, colfull_lo=0, colfull_hi=0, rowfull_lo=0, rowfull_hi=0)):
        nat.band_replays(reset=True)
        o = nat.band_attention(dev(q), dev(k), dev(v), nat.BandMask(**prm), vid0=0, num_frame=F_, frame_size=P_, head_perm_flag=dev(BEST))
        print(f"very negative rows, band {prm['band']}: replays={nat.band_replays(reset=True)}")
        ref = placed_reference(q, k, v, O.band_mask(S, **prm), BEST, 0, F_, P_, False)
        assert torch.isfinite(o.float()).all() and o.float().abs().max() > 0
        torch.testing.assert_close(o.float().cpu(), ref, atol=6e-2, rtol=6e-2)
