"""Band attention on row shards on the GPU (include/svg_attn_band_row_shard.h; BandRowShardOf of csrc/band_policy.h; cases:
tests/band_row_shard_cases.py): whole frames against the frame-shard entries and the whole sequence against svg_band_attention_lse[_f32],
bit for bit; merged fp32 parts against float64 and the single call with the bounds tests/test_gpu_band_shard.py puts on them (T_SINGLE,
check_attn, check_lse with factor 2); rows without a key; the token-major o layout; balance="rows" on two gloo ranks sharing the GPU."""
import functools

import pytest
import torch

import band_row_shard_cases as RC
from gloo_ranks import run_ranks
from sparse_lse_cases import DTYPES, T_SINGLE, check_lse, rel_l2
from test_gpu_kernels import check_attn, dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def nat():
    from poisoned import load_native

    return load_native()


@functools.lru_cache(maxsize=None)
def device_rows(dtype, shard):
    return tuple(dev(x[:, :, RC.shard_rows(shard)]) for x in RC.inputs(dtype))


def run_pair(nat, mask, dtype, qs, ks, **kw):
    q, (_, k, v) = device_rows(dtype, qs)[0], device_rows(dtype, ks)
    flags = torch.tensor(RC.FLAGS, dtype=torch.int64, device="cuda")
    return nat.band_row_shard_attention(q, k, v, nat.BandMask(**RC.MASKS[mask]), RC.GEO, qs, ks, flags=flags, **kw)


@functools.lru_cache(maxsize=None)
def whole_call(nat, mask, dtype, f32):
    q, k, v = (dev(x) for x in RC.inputs(dtype))
    return nat.band_attention(q, k, v, nat.BandMask(**RC.MASKS[mask]), head_perm_flag=torch.tensor(RC.FLAGS, dtype=torch.int64, device="cuda"),
                              vid0=0, num_frame=RC.F, frame_size=RC.P, return_lse=True, out_dtype=torch.float32 if f32 else None)


@pytest.mark.parametrize("f32", [False, True], ids=["lse", "lse_f32"])
@pytest.mark.parametrize("mask", list(RC.MASKS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_frames_are_the_frame_shard_entries_bit_for_bit(nat, dtype, mask, f32):
    kw = dict(out_dtype=torch.float32) if f32 else {}
    flags = torch.tensor(RC.FLAGS, dtype=torch.int64, device="cuda")
    for (qa, qn), (ka, kn) in (((1, 2), (2, 3)), ((3, 2), (0, 2)), ((0, 5), (0, 5))):       # frames [a, a + n), the tail where they end the video
        qs, ks = ((a * RC.P, n * RC.P, RC.V, RC.S - RC.V if a + n == RC.F else 0) for a, n in ((qa, qn), (ka, kn)))
        o, lse = run_pair(nat, mask, dtype, qs, ks, **kw)
        q, (_, k, v) = device_rows(dtype, qs)[0], device_rows(dtype, ks)
        o_f, lse_f = nat.band_shard_attention(q, k, v, nat.BandMask(**RC.MASKS[mask]), RC.S, (0, RC.F, RC.P), (qa, qn) + qs[2:], (ka, kn) + ks[2:],
                                              flags=flags, **kw)
        assert torch.equal(o, o_f) and torch.equal(lse, lse_f), (qs, ks)
    o_w, lse_w = whole_call(nat, mask, dtype, f32)                                            # (the last pair: one shard over everything)
    assert torch.equal(o, o_w) and torch.equal(lse, lse_w)


@pytest.mark.parametrize("cuts", list(RC.CUTS))
@pytest.mark.parametrize("mask", list(RC.MASKS))
@pytest.mark.parametrize("dtype", DTYPES)
def test_merged_parts_equal_the_whole_sequence(nat, dtype, mask, cuts):
    sh = RC.shards(RC.CUTS[cuts])
    o_ref, lse_ref = RC.reference(mask, dtype)
    o_w = whole_call(nat, mask, dtype, True)[0].cpu()
    unseen = 0
    for qs in sh:
        rows = RC.shard_rows(qs)
        parts = [run_pair(nat, mask, dtype, qs, ks, out_dtype=torch.float32) for ks in sh]
        for ks, (o32, lse) in zip(sh, parts):         # rows that see no key of a part: lse = -inf and o = 0, exactly those
            none = torch.stack([~RC.pair_mask(mask, qs, ks, bool(f)).any(dim=1) for f in RC.FLAGS])[None]
            assert torch.equal(torch.isneginf(lse).cpu(), none) and not bool(o32.cpu()[none].any()), (qs, ks)
            unseen += int(none.sum())
        o, lse = nat.merge_attention_states([p[0] for p in parts], [p[1] for p in parts], return_lse=True, out_dtype=dtype)
        e, d = rel_l2(o.float().cpu(), o_ref[:, :, rows]), rel_l2(o.float().cpu(), o_w[:, :, rows])
        print(f"{mask} {dtype} cuts {cuts} q shard {qs}: merged fp32 parts rel_l2 {e:.3e} against float64, {d:.3e} against the single call "
              f"(limit {T_SINGLE[dtype]:.1e})")
        assert e <= T_SINGLE[dtype] and d <= T_SINGLE[dtype], (e, d)
        check_attn(o, o_ref[:, :, rows].float(), dtype)
        check_lse(lse, lse_ref[:, :, rows], dtype, f"merged {mask} q shard {qs}", factor=2.0)
    assert unseen > 0                                 # (the outer shards' video rows in logical order see no video key of each other)


@pytest.mark.parametrize("dtype", DTYPES)
def test_token_major_o_layout_is_the_contiguous_call_bit_for_bit(nat, dtype):
    qs, ks = RC.shards(RC.CUTS["640"])[1:]
    q = device_rows(dtype, qs)[0]
    o_c, lse_c = run_pair(nat, "hy", dtype, qs, ks)
    out = nat.token_major_empty(q)
    out.fill_(float("nan"))
    o, lse = run_pair(nat, "hy", dtype, qs, ks, out=out)
    assert o is out and not out.is_contiguous() and out.transpose(1, 2).is_contiguous()
    assert torch.equal(o, o_c) and torch.equal(lse, lse_c)


def _worker(rank, world):
    from svg import _native as nat_
    from svg import distributed as sd

    nat_.poison_allocations(True)   # (a spawned process: the switch of tests/poisoned.py does not reach it)
    torch.cuda.set_device(0)
    dtype, mask = torch.bfloat16, nat_.BandMask(**RC.MASKS["hy"])
    flags = torch.tensor(RC.FLAGS, dtype=torch.int64, device="cuda")
    sd.enable_frame_shards(balance="rows")
    sh = [sd.row_shard(RC.GEO, r, world).as_tuple() for r in range(world)]
    rows = RC.shard_rows(sh[rank])
    ql, kl, vl = (x[:, :, rows].contiguous().cuda() for x in RC.inputs(dtype))
    o = sd.token_sharded_svg1_attention(ql, kl, vl, mask, flags, RC.GEO)           # (balance: what enable_frame_shards set)
    torch.cuda.synchronize()
    sd.disable()
    return dict(shard=sh[rank], shape=o.shape == ql.shape and o.dtype == dtype, err=rel_l2(o.float().cpu(), RC.reference("hy", dtype)[0][:, :, rows]))


def test_token_sharded_svg1_attention_rows_two_ranks_one_gpu():
    got = run_ranks(_worker, 2, 48900)
    assert [got[r]["shard"] for r in (0, 1)] == [(0, 512, 960, 0), (512, 448, 960, 40)]      # 4 + 3 units of 128, the rest and the text
    for r in (0, 1):
        assert got[r]["shape"] and got[r]["err"] <= T_SINGLE[torch.bfloat16], got[r]
