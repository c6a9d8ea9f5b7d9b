"""The quality probe without a GPU (svg/models/_core.py: sparse_quality, log_quality, the processors' quality_log):
  * the float64 identity it rests on: exp(lse_masked - lse_dense) is the masked share of the dense softmax row, for a band mask and for a
    block map;
  * the figures of sparse_quality on CPU tensors against numpy;
  * the deferred writer: nothing is written before the copy's event completes or flush(), records of dense steps are dropped, the fields;
  * the probe's generator: drawing from it advances neither the global CPU stream nor the switched path's generator;
  * the refusals under the three modes of svg.distributed: NotImplementedError on the first call, before any collective."""
import json
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import sparse_lse_cases as SC
from oracle import svg_oracle as O
from svg import _native as nat
from svg.models import _core


# ---------------------------------------------------------------------------------------------------------
# the identity
# ---------------------------------------------------------------------------------------------------------
def _masked_share(q, k, mask):
    """share of the dense softmax row on the keys of the mask, float64"""
    s = torch.matmul(q.double(), k.double().transpose(-1, -2)) / q.shape[-1] ** 0.5
    p = torch.softmax(s, dim=-1)
    return (p * mask).sum(-1)


def test_kept_mass_is_the_masked_share_of_the_dense_row_band_mask():
    S, prm, mask, _ = SC.band_case("hy")
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(1, 2, S, 128, generator=g, dtype=torch.float64) for _ in range(3))
    dense = O.band_mask(S, **O.dense_band_params(S))
    assert dense.all()
    _, lse_d = SC.masked_attention_lse(q, k, v, dense)
    _, lse_m = SC.masked_attention_lse(q, k, v, mask)
    share = _masked_share(q, k, mask)
    fin = torch.isfinite(lse_m)
    assert fin.any() and (torch.exp(lse_m - lse_d)[fin] - share[fin]).abs().max() < 1e-12
    assert (share[~fin] == 0).all() and (torch.exp(lse_m - lse_d)[~fin] == 0).all()      # a row without keys: kept mass 0
    assert (share <= 1 + 1e-12).all() and share[fin].min() < 0.999                          # and it is a share: the mask drops something


def test_kept_mass_is_the_masked_share_of_the_dense_row_block_map():
    hq, hkv, S, MB, NB = 4, 2, 300, 6, 15
    gen = torch.Generator().manual_seed(4)
    rsz = SC.random_partition_batch(S, MB, hkv, gen)
    csz = SC.random_partition_batch(S, NB, hkv, gen)
    bmap = torch.rand(hkv, MB, NB, generator=gen) < 0.5
    bmap[:, 1] = False                           # block-row 1: no key at all
    q = torch.randn(hq, S, 128, generator=gen, dtype=torch.float64)
    k, v = (torch.randn(hkv, S, 128, generator=gen, dtype=torch.float64) for _ in range(2))
    _, lse_m = SC.vb_reference_of(q, k, v, bmap, rsz, csz)
    g = hq // hkv
    for h in range(hkv):
        em = O.block_mask_to_element_mask(bmap[h], rsz[h], csz[h])
        hs = slice(h * g, (h + 1) * g)
        _, lse_d = SC.masked_attention_lse(q[hs], k[h:h + 1], v[h:h + 1], None)
        kept = torch.exp(lse_m[hs] - lse_d)
        share = _masked_share(q[hs], k[h:h + 1], em)
        assert (kept - share).abs().max() < 1e-12
        r0, r1 = int(rsz[h, 0]), int(rsz[h, :2].sum())
        assert (kept[:, r0:r1] == 0).all()


# ---------------------------------------------------------------------------------------------------------
# the figures
# ---------------------------------------------------------------------------------------------------------
def test_quality_figures_against_numpy():
    g = torch.Generator().manual_seed(5)
    cfg, H, R, D = 2, 3, 17, 64
    o_d = torch.randn(cfg, H, R, D, generator=g)
    o_s = (o_d + 0.05 * torch.randn(cfg, H, R, D, generator=g)).to(torch.bfloat16)
    lse_d = torch.randn(cfg, H, R, generator=g) + 5
    lse_s = lse_d - torch.rand(cfg, H, R, generator=g)
    lse_s[1, 2, 3] = float("-inf")                       # a row the sparse form gave no key
    f = _core.quality_figures(o_s, lse_s, o_d, lse_d)
    a, b = o_s.float().double().numpy(), o_d.double().numpy()
    rel = np.sqrt(((a - b) ** 2).sum(axis=(2, 3)) / (b ** 2).sum(axis=(2, 3)))
    mse = ((a - b) ** 2).mean(axis=(2, 3))
    kept = np.exp(lse_s.double().numpy() - lse_d.double().numpy()).mean(axis=2)
    assert f["rel_l2"].shape == f["mse"].shape == f["kept_mass"].shape == (cfg, H)
    np.testing.assert_allclose(f["rel_l2"].numpy(), rel, rtol=1e-5)
    np.testing.assert_allclose(f["mse"].numpy(), mse, rtol=1e-5)
    np.testing.assert_allclose(f["kept_mass"].numpy(), kept, rtol=1e-5)
    assert np.isfinite(kept).all() and kept[1, 2] < kept[1, 1] + 1     # (-inf contributes exp(-inf) = 0, never NaN)
    assert _core.quality_figures(o_s, None, o_d, lse_d)["kept_mass"] is None
    same = _core.quality_figures(o_d, lse_d, o_d, lse_d)
    assert (same["rel_l2"] == 0).all() and (same["mse"] == 0).all() and (same["kept_mass"] == 1).all()


def test_sparse_quality_refuses_cpu_tensors_like_every_native_op():
    q = torch.zeros(1, 2, 70, 128, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="GPU"):
        _core.sparse_quality(q, None, q, q, q, torch.tensor([0, 1]))


# ---------------------------------------------------------------------------------------------------------
# the writer
# ---------------------------------------------------------------------------------------------------------
class _Event:
    def __init__(self):
        self.done = False
        self.synced = 0

    def query(self):
        return self.done

    def synchronize(self):
        self.synced += 1
        self.done = True


def _figures(cfg=1, H=2, kept=True, base=0.0):
    t = torch.arange(cfg * H, dtype=torch.float32).reshape(cfg, H) + base
    return {"rel_l2": t + 0.25, "mse": t + 0.5, "kept_mass": (t + 0.75) if kept else None}


def test_quality_log_writes_deferred_and_drops_dense_steps(tmp_path):
    log = _core._QualityLog()
    path = str(tmp_path / "q.jsonl")
    # CPU tensors: no event, written at once; fields and their order
    log.push(path, {"timestep": 3.0, "layer": 7}, _figures())
    rec = [json.loads(x) for x in open(path)]
    assert len(rec) == 1 and list(rec[0]) == ["timestep", "layer", "rel_l2", "mse", "kept_mass"]
    assert rec[0] == {"timestep": 3.0, "layer": 7, "rel_l2": [[0.25, 1.25]], "mse": [[0.5, 1.5]], "kept_mass": [[0.75, 1.75]]}
    # no LSE form: null; SVG2: the densities ride along
    log.push(path, {"timestep": None, "layer": 0}, _figures(cfg=2, kept=False), density=torch.full((2, 2), 0.125))
    rec = [json.loads(x) for x in open(path)]
    assert rec[1]["kept_mass"] is None and rec[1]["density"] == [[0.125, 0.125]] * 2 and rec[1]["rel_l2"] == [[0.25, 1.25], [2.25, 3.25]]
    assert list(rec[1]) == ["timestep", "layer", "rel_l2", "mse", "kept_mass", "density"]
    # the device-switch flag: a dense step leaves no line, a sparse one does; the device timestep is read with the figures
    log.push(path, {"timestep": None, "layer": 1}, _figures(), dense_flag=torch.ones(1, dtype=torch.int32), timestep=torch.tensor([981.0]))
    log.push(path, {"timestep": None, "layer": 2}, _figures(), dense_flag=torch.zeros(1, dtype=torch.int32), timestep=torch.tensor([961.0]))
    rec = [json.loads(x) for x in open(path)]
    assert len(rec) == 3 and rec[2]["layer"] == 2 and rec[2]["timestep"] == 961.0 and rec[2]["kept_mass"] == [[0.75, 1.75]]
    assert not log.pending
    # a pending copy: nothing is written until its event has completed, then in order; flush() waits
    ev1, ev2 = _Event(), _Event()
    for i, ev in enumerate((ev1, ev2)):
        host = torch.cat([v.reshape(-1) for v in _figures(base=10.0 * (i + 1)).values()])
        log.pending.append((path, {"timestep": 1.0, "layer": 10 + i}, (1, 2), True, False, False, False, host, ev))
    log.flush(wait=False)
    assert len(open(path).readlines()) == 3 and len(log.pending) == 2 and ev1.synced == 0
    ev2.done = True                                     # the later copy alone does not overtake the earlier one
    log.flush(wait=False)
    assert len(open(path).readlines()) == 3
    ev1.done = True
    log.flush(wait=False)
    rec = [json.loads(x) for x in open(path)]
    assert [r["layer"] for r in rec[3:]] == [10, 11] and rec[4]["mse"] == [[20.5, 21.5]] and not log.pending
    ev3 = _Event()
    log.pending.append((path, {"timestep": 1.0, "layer": 12}, (1, 2), True, False, False, False, host, ev3))
    log.flush()
    assert ev3.synced == 1 and len(open(path).readlines()) == 6


def test_flush_quality_log_is_the_module_writers_flush_and_registered_at_exit(tmp_path):
    path = str(tmp_path / "q.jsonl")
    ev = _Event()
    host = torch.cat([v.reshape(-1) for v in _figures().values()])
    _core.QUALITY_LOG.pending.append((path, {"timestep": None, "layer": 0}, (1, 2), True, False, False, False, host, ev))
    _core.flush_quality_log()
    assert ev.synced == 1 and len(open(path).readlines()) == 1 and not _core.QUALITY_LOG.pending
    import atexit

    atexit.unregister(_core.flush_quality_log)          # (it was registered: unregistering and registering again leaves one entry)
    atexit.register(_core.flush_quality_log)


# ---------------------------------------------------------------------------------------------------------
# the probe's generator
# ---------------------------------------------------------------------------------------------------------
def test_probe_generator_leaves_the_other_streams_alone():
    torch.manual_seed(1234)
    _core.reseed_switch_generator()
    want_global = torch.randint(0, 1000, (8,))
    want_switch = torch.randint(0, 1000, (8,), generator=_core._switch_generator())
    torch.manual_seed(1234)
    _core.reseed_switch_generator()
    first = torch.randint(0, 1000, (8,), generator=_core._probe_generator())
    second = torch.randint(0, 1000, (8,), generator=_core._probe_generator())
    assert not torch.equal(first, second)                                    # it is a stream of its own ...
    assert torch.equal(torch.randint(0, 1000, (8,)), want_global)            # ... and neither of the others moved
    assert torch.equal(torch.randint(0, 1000, (8,), generator=_core._switch_generator()), want_switch)
    assert not torch.equal(first, want_switch)                               # not the switched path's rows either
    torch.manual_seed(1234)                                                  # the same global seed: the same probe rows again
    _core.reseed_probe_generator()
    assert torch.equal(torch.randint(0, 1000, (8,), generator=_core._probe_generator()), first)
    torch.manual_seed(99)                                                    # another seed is seen without a hook
    assert not torch.equal(torch.randint(0, 1000, (8,), generator=_core._probe_generator()), first)


def test_log_quality_draws_rows_from_the_probe_generator_over_the_valid_rows(monkeypatch, tmp_path):
    """the rows are uniform over the valid rows, one draw and one native call per group of videos with equal lengths"""
    calls = []

    def fake(o, lse, q, k, v, rows, valid_len=None, sm_scale=None):
        calls.append((q.shape[0], rows.clone(), valid_len, sm_scale, lse is not None))
        z = torch.zeros(q.shape[0], q.shape[1])
        return {"rel_l2": z, "mse": z, "kept_mass": z + 1 if lse is not None else None}

    monkeypatch.setattr(_core, "sparse_quality", fake)
    monkeypatch.setattr(_core, "QUALITY_LOG", _core._QualityLog())
    path = str(tmp_path / "q.jsonl")
    q = torch.zeros(3, 2, 100, 8)
    torch.manual_seed(7)
    before = torch.get_rng_state()
    _core.log_quality(_core.QualityRequest(path, 64, (90, 90, 40), 5.0, 3), q, torch.zeros(3, 2, 100), q, q, q)
    assert torch.equal(torch.get_rng_state(), before)
    assert [(c[0], c[2]) for c in calls] == [(2, 90), (1, 40)]
    assert all(len(c[1]) == 64 and c[1].dtype == torch.int64 and 0 <= int(c[1].min()) and int(c[1].max()) < c[2] for c in calls)
    assert calls[1][1].numel() == 64 and calls[0][3] is None and calls[0][4]
    rec = json.loads(open(path).read())
    assert rec["timestep"] == 5.0 and rec["layer"] == 3 and rec["kept_mass"] == [[1.0, 1.0]] * 3
    calls.clear()
    _core.log_quality(_core.QualityRequest(path, 200, None, None, 0), q[:1], None, q[:1], q[:1], q[:1], q_prescaled=True)
    assert len(calls) == 1 and calls[0][2] is None and len(calls[0][1]) == 64 and int(calls[0][1].max()) < 100     # at most 64 rows a call
    assert calls[0][3] == _core.LN2 and not calls[0][4]                      # a pre-scaled q: the kernel's scale is ln 2, as for sample_mse
    _core.log_quality(_core.QualityRequest(path, 64, 100, None, 0), q[:1], None, q[:1], q[:1], q[:1])
    assert calls[-1][2] is None                                              # valid_len == S: one segment


# ---------------------------------------------------------------------------------------------------------
# the processors: attributes, and the refusals under svg.distributed
# ---------------------------------------------------------------------------------------------------------
def _processors():
    from svg.models.cog.attention import CogVideoX_SparseAttn_Processor2_0
    from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor, Cosmos_SVG_AttnProcessor2_0
    from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0, Hunyuan_SVGAttn_Processor2_0
    from svg.models.wan.attention import WanAttn_SAPAttn_Processor, WanAttn_SVGAttn_Processor2_0

    return {"hy1": Hunyuan_SVGAttn_Processor2_0, "hy2": Hunyuan_SAPAttn_Processor2_0, "wan1": WanAttn_SVGAttn_Processor2_0,
            "wan2": WanAttn_SAPAttn_Processor, "cog": CogVideoX_SparseAttn_Processor2_0, "cosmos1": Cosmos_SVG_AttnProcessor2_0,
            "cosmos2": Cosmos_SAPAttn_Processor}


def test_every_processor_has_the_two_attributes_and_off_is_the_default():
    for name, cls in _processors().items():
        assert cls.quality_log is None and cls.quality_rows == 64, name
    assert _core.quality_request("x", None, 64) is None
    r = _core.quality_request("x", "a.jsonl", 32, 90, 5.0, 2)
    assert (r.path, r.rows, r.valid_len, r.timestep, r.layer) == ("a.jsonl", 32, 90, 5.0, 2)


@pytest.fixture
def one_rank_group():
    from svg import distributed as sd

    port = 38500 + (os.getpid() % 2000)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        yield sd
    finally:
        sd.disable()
        dist.destroy_process_group()


def _no_collectives(monkeypatch):
    for name in ("all_reduce", "all_to_all_single", "all_gather_into_tensor", "broadcast", "all_gather"):
        monkeypatch.setattr(dist, name, lambda *a, _n=name, **k: pytest.fail(f"{_n}: a collective ran before the refusal"))


@pytest.mark.parametrize("mode", ["enable", "frame_shards", "token_shards"])
def test_quality_log_is_refused_under_every_distributed_mode(one_rank_group, monkeypatch, tmp_path, mode):
    sd = one_rank_group
    {"enable": sd.enable, "frame_shards": sd.enable_frame_shards, "token_shards": sd.enable_token_shards}[mode]()
    _no_collectives(monkeypatch)
    path = str(tmp_path / "q.jsonl")
    # the core calls
    geo = _core.Geometry(0, 2, 64)
    S = geo.seq_len
    q = torch.zeros(1, 2, S, 128, dtype=torch.bfloat16)
    m = nat.BandMask(**O.dense_band_params(S))
    prof = nat.ProfileDesc(0, 2, 64, 0)
    req = _core.QualityRequest(path)
    with pytest.raises(NotImplementedError, match="quality_log"):
        _core.quality_request("x", path, 64)
    with pytest.raises(NotImplementedError, match="quality_log"):
        _core.svg1_sparse_attention(q, q, q, geo, m, prof, 8, S, quality=req)
    with pytest.raises(NotImplementedError, match="quality_log"):
        _core.svg1_attention_device_switch(q, q, q, geo, m, m, prof, 8, S, torch.zeros(1, dtype=torch.int32), quality=req)
    with pytest.raises(NotImplementedError, match="quality_log"):
        _core.svg2_sparse_attention(q, q, q, geo, _core.CentroidStore(), 0, 4, 4, 0.9, 0.1, 2, 1, quality=req)
    # the processors, on their first call (frame-shard mode has a form for the SVG1 processors of HunyuanVideo and Wan only: the others
    # refuse the mode itself first, as before)
    procs = _processors()
    names = ["hy1", "wan1"] if mode == "frame_shards" else list(procs)
    t = torch.tensor([500.0])
    for name in names:
        cls = procs[name]
        for attr, val in (("quality_log", path), ("num_frame", 2), ("frame_size", 64), ("context_length", 0), ("prompt_length", 0)):
            monkeypatch.setattr(cls, attr, val, raising=False)
        args = (q, q, q, t, 0, None) if name.startswith("hy") else (q, q, q, t)
        with pytest.raises(NotImplementedError, match="quality_log"):
            cls(0).attention_core_logic(*args)
    assert not os.path.exists(path)
