"""The SVG1 / SVG2 layer-call of svg.models._core and of the processors, pinned as a CALL TRANSCRIPT: what the two `_core` functions
(svg1_attention_device_switch, svg1_sparse_attention) and the seven processors' attention_core_logic call below themselves — every
`_native`, `_adaptive_band`, `_probe` and `svg.distributed` function, `log_quality`, the band store's `get` — with which of the caller's
tensors, which scalars, masks and keywords, which sampled rows, under which timer labels, what they leave in the three CPU generators and
what they return; for a refusal the exception, its message and what had run before it.  `svg/_native.py` and the library below it decide
every launch from these calls alone, so equal transcripts are equal launches and equal bits.

tests/golden/svg1_layer_calls.json was recorded by tests/golden/make_golden_svg1_layer_calls.py on the commit that script names, the last
one on which the layer-call was written out once per function and once per processor.  It is the reference for the one body they share
now and is NOT regenerated from newer code: a transcript that differs is a behaviour change, to be explained or undone.

No GPU and no library: the tensors are CPU tensors of a subclass that says `is_cuda` (the stand-in style of
tests/test_band_lse_forms_cpu.py), everything below the recorded boundary is a stand-in."""
import __future__

import contextlib
import dataclasses
import hashlib
import inspect
import json
import textwrap
from pathlib import Path
from unittest import mock

import pytest
import torch

from svg import _adaptive_band, _probe, timer
from svg import _native as nat
from svg.models import _core
from svg.models.cog.attention import CogVideoX_SparseAttn_Processor2_0 as Cog
from svg.models.cosmos.attention import Cosmos_SAPAttn_Processor as CosmosSAP
from svg.models.cosmos.attention import Cosmos_SVG_AttnProcessor2_0 as CosmosSVG
from svg.models.hyvideo.attention import Hunyuan_SAPAttn_Processor2_0 as HySAP
from svg.models.hyvideo.attention import Hunyuan_SVGAttn_Processor2_0 as HySVG
from svg.models.wan.attention import WanAttn_SAPAttn_Processor as WanSAP
from svg.models.wan.attention import WanAttn_SVGAttn_Processor2_0 as WanSVG

GOLDEN = Path(__file__).resolve().parent / "golden" / "svg1_layer_calls.json"
SEED = 20240
CFG, H, F_, P_, CTX = 2, 2, 3, 16, 16          # two videos, two heads, 3 frames of 16 tokens, 16 text rows behind them: S = 64
S = CTX + F_ * P_


class _GpuT(torch.Tensor):
    """a CPU tensor that says it lives on the GPU: the gates open, the arithmetic around the launches runs"""
    is_cuda = property(lambda self: True)


def _gpu(*shape, dtype=torch.bfloat16, fill=0):
    return torch.full(shape, fill, dtype=dtype).as_subclass(_GpuT)


def _h(state) -> str:
    return hashlib.sha1(state.numpy().tobytes()).hexdigest()[:8]


_DT = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32", torch.int32: "i32", torch.int64: "i64", torch.bool: "b"}


class Rec:
    """the transcript of one case"""

    def __init__(self):
        self.events, self.names, self.objs, self.keep = [], {}, {}, []

    def name(self, x, label):
        if torch.is_tensor(x):
            self.names[x.untyped_storage().data_ptr()] = (label, tuple(x.shape))
        else:
            self.objs[id(x)] = label
        self.keep.append(x)
        return x

    def out(self, label, shape, dtype):
        return self.name(_gpu(*shape, dtype=dtype), f"{label}@{len(self.events)}")

    def d(self, x):
        if torch.is_tensor(x):
            ent = self.names.get(x.untyped_storage().data_ptr())
            if ent is not None:
                same = tuple(x.shape) == ent[1] and x.is_contiguous()
                return ent[0] if same else f"{ent[0]}{list(x.shape)}{'' if x.is_contiguous() else '~'}"
            vals = ",".join(f"{y:g}" for y in x.flatten().tolist()) if x.numel() <= 64 else "..."
            return f"{_DT.get(x.dtype, x.dtype)}{list(x.shape)}={vals}"
        if id(x) in self.objs:
            return self.objs[id(x)]
        if x is None or isinstance(x, (bool, int, float, str)):
            return x
        if isinstance(x, nat.BandMask):
            return {"mask": list(x.as_tuple())}
        if isinstance(x, nat.ProfileDesc):
            return {"prof": hashlib.sha1(bytes(x)).hexdigest()[:8]}
        if isinstance(x, _core.Geometry):
            return {"geo": [x.context_length, x.num_frame, x.frame_size, x.text_first]}
        if dataclasses.is_dataclass(x):
            return {type(x).__name__: {f.name: self.d(getattr(x, f.name)) for f in dataclasses.fields(x)}}
        if isinstance(x, (list, tuple)):
            return [self.d(y) for y in x]
        if isinstance(x, dict):
            return {k: self.d(v) for k, v in x.items()}
        if isinstance(x, slice):
            return f"{x.start}:{x.stop}"
        if isinstance(x, (torch.dtype, torch.device)):
            return str(x)
        if callable(x):
            return "<fn>"
        return f"<{type(x).__name__}>"

    def call(self, label, a, kw):
        self.events.append([label, self.d(list(a)), self.d(kw)] if kw else [label, self.d(list(a))])


# ---------------------------------------------------------------------------------------------------------
# the stand-ins below the recorded boundary
# ---------------------------------------------------------------------------------------------------------
def _attn(rec, label):
    def f(q, *a, **kw):
        rec.call(label, (q,) + a, kw)
        o = rec.out("o", q.shape, kw.get("out_dtype") or q.dtype)
        if kw.get("return_lse", label.startswith("ab.")):
            return o, rec.out("lse", q.shape[:3], torch.float32)
        return o
    return f


def _sample_mse(rec):
    def f(q, k, v, rows, prof, **kw):
        rec.call("sample_mse", (q, k, v, rows, prof), kw)
        n = 2 * q.shape[0] * q.shape[1]
        return ((torch.arange(n) * 7) % 5).float().reshape(2, -1)   # (argmin over the two masks: 0, 1, 1, 0 on four heads)
    return f


def _void(rec, label, ret=None):
    def f(*a, **kw):
        rec.call(label, a, kw)
        return ret(*a, **kw) if ret is not None else None
    return f


@contextlib.contextmanager
def harness(rec, mode=None, world=2, fp8=False, level_b=False):
    """everything the layer-call calls, replaced by recording stand-ins; `mode`: a mode of svg.distributed switched on without a process
    group (heads: enable(), tokens: enable_token_shards(), frames: enable_frame_shards()) over `world` ranks, this one rank 0"""
    sd, td = _core._dist, torch.distributed
    with contextlib.ExitStack() as st:
        P = lambda obj, name, val: st.enter_context(mock.patch.object(obj, name, val))   # noqa: E731
        for name in ("band_attention", "band_attention_switch", "band_attention_groups", "band_attention_fp8"):
            P(nat, name, _attn(rec, name))
        P(nat, "sample_mse", _sample_mse(rec))
        P(nat, "head_placement", _void(rec, "head_placement"))
        P(nat, "band_width_update", _void(rec, "band_width_update"))
        P(nat, "empty_like", _void(rec, "empty_like", lambda x, **kw: rec.out("e", x.shape, x.dtype)))
        P(nat, "empty", _void(rec, "empty", lambda shape, dtype=None, **kw: rec.out("e", tuple(shape), dtype)))
        P(_adaptive_band, "band_attention_per_head", _attn(rec, "ab.band_attention_per_head"))
        P(_adaptive_band, "band_attention_switch_per_head", _attn(rec, "ab.band_attention_switch_per_head"))
        P(_probe, "sample_dense_lse", _void(rec, "probe.sample_dense_lse",
                                            lambda q, k, rows, vl: rec.out("lse_d", (q.shape[0], q.shape[1], rows.numel()), torch.float32)))
        P(sd, "run_sharded", _void(rec, "dist.run_sharded", lambda fn, ts, group=None: fn(*ts)))
        P(sd, "run_token_sharded", _void(rec, "dist.run_token_sharded", lambda fn, ts, seq_len, group=None: fn(*ts)))
        P(sd, "token_sharded_svg1_layer_call", _void(rec, "dist.token_sharded_svg1_layer_call", lambda q, *a, **kw: (
            rec.out("o", q.shape, q.dtype), torch.tensor([1, 0, 0, 1][:q.shape[0] * q.shape[1]]))))
        P(sd, "token_sharded_svg1_attention", _void(rec, "dist.token_sharded_svg1_attention", lambda q, *a, **kw: rec.out("o", q.shape, q.dtype)))
        P(_core, "log_quality", _void(rec, "log_quality", lambda quality, out, lse, q, *a, **kw: (
            [rec.out("lse_q", (q.shape[0], q.shape[1], 4), torch.float32)] if kw.get("plan") is not None else [])))
        real_get = _core._KeptMassStore.get

        def get(self, layer_idx, n, init, device):
            rec.events.append(["store.get", type(self).__name__, rec.d(layer_idx), n, init, str(device)])
            return real_get(self, layer_idx, n, init, device)

        P(_core._KeptMassStore, "get", get)
        P(timer.TimeLoggingContext, "__enter__", lambda self: (rec.events.append(["T", self.operation_name]), self)[1])
        st.enter_context(mock.patch.dict(_core._ATTENTION_DTYPE, {"value": "fp8" if fp8 else "bf16"}))
        if mode is not None:
            P(td, "is_initialized", lambda: True)
            P(td, "get_world_size", lambda group=None: world)
            P(td, "get_rank", lambda group=None: 0)
            P(td, "get_backend", lambda group=None: "gloo")
            P(td, "broadcast", lambda *a, **k: None)
            st.enter_context(mock.patch.dict(sd._STATE, {{"heads": "enabled", "tokens": "tokens", "frames": "frames"}[mode]: True}))
        if level_b:
            P(_core, "dense_attention", _spy(rec, "core.dense_attention", _core.dense_attention))
            for name in ("svg1_attention_device_switch", "svg1_sparse_attention"):
                P(_core, name, _void(rec, "core." + name, lambda q, *a, **kw: (
                    rec.out("o", q.shape, q.dtype), torch.tensor([[0, 1], [1, 0]][:q.shape[0]]))))
            P(_core, "svg2_sparse_attention", _void(rec, "core.svg2_sparse_attention", lambda q, *a, **kw: rec.out("o", q.shape, q.dtype)))
            P(_core, "kmeans_clustering", _void(rec, "core.kmeans_clustering"))
        yield


def _spy(rec, label, real):
    def f(*a, **kw):
        rec.call(label, a, kw)
        return real(*a, **kw)
    return f


def _generators():
    """(global CPU generator, the switched path's, the probe's): a hash of each state"""
    return [_h(torch.get_rng_state()), _h(_core._switch_generator().get_state()), _h(_core._probe_generator().get_state())]


def record(rec, run, **how):
    """one case: fresh generators, the call inside the harness -> its record"""
    torch.manual_seed(SEED)
    _core._SWITCH_GEN = _core._PROBE_GEN = None
    with harness(rec, **how):
        before = _generators()
        try:
            res = {"returns": rec.d(run())}
        except Exception as e:  # noqa: BLE001 — a refusal is a result: type, full message, what ran before it
            res = {"raises": [type(e).__name__, str(e)]}
        after = _generators()
    _core._SWITCH_GEN = _core._PROBE_GEN = None
    drawn = [name for name, a, b in zip(("global", "switch", "probe"), after, before) if a != b]
    if drawn:   # (the states, which count the draws; generators nobody drew from are left out of the record, like an empty call list)
        res.update(drawn=drawn, generators=" ".join(after))
    return dict(res, calls=rec.events) if rec.events else res


# ---------------------------------------------------------------------------------------------------------
# level A: the two _core functions
# ---------------------------------------------------------------------------------------------------------
M1 = dict(real_len=60, band=33, colfull_lo=0, colfull_hi=16, rowfull_lo=48, rowfull_hi=60)


def core_case(fn, masks="one", dense="one", D=128, dtype=torch.bfloat16, cuda=True, n=6, max_row=40, flag=0, geo=None, quality=False,
              adaptive=None, store=True, mode=None, world=2, fp8=False, **kw):
    """fn: "switch" / "sparse"; masks, dense: "one" / "equal" / "differ" / "three" (a list of the wrong length); adaptive: None or the
    AdaptiveBand's keywords; the rest are the functions' own keywords"""
    def run(rec):
        mk = (lambda *shape, **k: _gpu(*shape, **k)) if cuda else (lambda *shape, dtype=torch.bfloat16, fill=0: torch.full(shape, fill, dtype=dtype))
        q, k, v = (rec.name(mk(CFG, H, S, D, dtype=dtype), nm) for nm in "qkv")
        g = rec.name(geo or _core.Geometry(CTX, F_, P_), "geo")
        prof = rec.name(nat.ProfileDesc(0, F_, P_, 1), "prof")
        m, m2 = rec.name(nat.BandMask(**M1), "m"), rec.name(nat.BandMask(**dict(M1, real_len=56)), "m2")
        d, d2 = rec.name(nat.BandMask(60, S + 1, 0, 0, 0, 0), "d"), rec.name(nat.BandMask(56, S + 1, 0, 0, 0, 0), "d2")
        pick = lambda a, b, how: {"one": a, "equal": [a, nat.BandMask(*a.as_tuple())], "differ": (a, b), "three": [a, a, a]}[how]   # noqa: E731
        extra = dict(kw)
        if quality:
            extra["quality"] = _core.QualityRequest("quality.jsonl", 4, None, None, 3)
        if adaptive is not None:
            extra.update(adaptive=_core.AdaptiveBand(**dict(dict(target=0.9, quantum=16, rows=4), **adaptive)), layer_idx=3)
            if store:
                extra["band_store"] = rec.name(_core.BandStore(), "band_store")
        if fn == "switch":
            dflag = rec.name(mk(1, dtype=torch.int32, fill=flag), "flag")
            return lambda: _core.svg1_attention_device_switch(q, k, v, g, pick(m, m2, masks), pick(d, d2, dense), prof, n, max_row, dflag, **extra)
        return lambda: _core.svg1_sparse_attention(q, k, v, g, pick(m, m2, masks), prof, n, max_row, **extra)

    def go():
        rec = Rec()
        return record(rec, run(rec), mode=mode, world=world, fp8=fp8)
    return go


def _core_cases():
    c = {}
    for fn in ("switch", "sparse"):
        A = lambda name, **kw: c.__setitem__(f"A/{fn}/{name}", core_case(fn, **kw))   # noqa: E731
        A("one_mask")
        A("equal_masks", masks="equal", dense="equal")
        A("differing_masks", masks="differ")
        A("mask_list_of_the_wrong_length", masks="three")
        A("D64", D=64)
        for lse, od in ((True, None), (True, torch.float32), (False, torch.float32)):
            for masks in ("one", "differ"):
                A(f"return_lse={lse},out_dtype={'f32' if od else None},{masks}", masks=masks, return_lse=lse, out_dtype=od)
        A("q_prescaled", q_prescaled=True)
        A("q_prescaled,return_lse", q_prescaled=True, return_lse=True)
        A("fp8", fp8=True)
        A("fp8,q_prescaled", fp8=True, q_prescaled=True)
        A("fp8,differ", fp8=True, masks="differ")
        A("fp8,return_lse", fp8=True, return_lse=True)
        A("quality", quality=True)
        A("quality,differ", quality=True, masks="differ")
        A("quality,return_lse", quality=True, return_lse=True)
        A("quality,D64", quality=True, D=64)
        A("quality,q_prescaled", quality=True, q_prescaled=True)
        A("adaptive", adaptive={})
        A("adaptive,equal_masks", adaptive={}, masks="equal", dense="equal")
        A("adaptive,no_store", adaptive={}, store=False)
        A("adaptive,quality", adaptive={}, quality=True)
        A("adaptive,return_lse", adaptive={}, return_lse=True)
        A("adaptive,differ", adaptive={}, masks="differ")
        A("adaptive,D64", adaptive={}, D=64)
        A("adaptive,q_prescaled", adaptive={}, q_prescaled=True)
        A("adaptive,out_dtype", adaptive={}, return_lse=True, out_dtype=torch.float32)
        A("adaptive,band_min_not_congruent", adaptive=dict(band_min=2))
        A("cpu_tensors", cuda=False)
        A("local", _local=True)
        A("local,return_lse", _local=True, return_lse=True)
        for mode in ("heads", "tokens"):
            A(f"{mode}", mode=mode)
            A(f"{mode},differ", mode=mode, masks="differ")
            A(f"{mode},return_lse", mode=mode, return_lse=True)
            A(f"{mode},quality", mode=mode, quality=True)
            A(f"{mode},adaptive", mode=mode, adaptive={})
            A(f"{mode},local", mode=mode, _local=True)
        hy = dict(mode="frames", world=1)
        A("frames", **hy)
        A("frames,flag1", flag=1, **hy)
        A("frames,equal_masks", masks="equal", dense="equal", **hy)
        A("frames,differ", masks="differ", **hy)
        A("frames,q_prescaled", q_prescaled=True, **hy)
        A("frames,fp8", fp8=True, **hy)
        A("frames,return_lse", return_lse=True, **hy)
        A("frames,fp16", dtype=torch.float16, **hy)
        A("frames,D64", D=64, **hy)
        A("frames,65_rows", n=65, geo=_core.Geometry(CTX, F_, 32), **hy)
        A("frames,text_first", geo=_core.Geometry(CTX, F_, P_, text_first=True), **hy)
        A("frames,9_ranks", mode="frames", world=9)
        A("frames,cpu", cuda=False, **hy)
        A("frames,quality", quality=True, **hy)
        A("frames,adaptive", adaptive={}, **hy)
    S_ = lambda name, **kw: c.__setitem__(f"A/switch/{name}", core_case("switch", **kw))   # noqa: E731
    S_("flag1", flag=1)
    S_("flag1,differ", flag=1, masks="differ")
    S_("flag1,adaptive,quality", flag=1, adaptive={}, quality=True)
    S_("differing_dense_masks", dense="differ")
    S_("dense_list_of_the_wrong_length", dense="three")
    S_("both_differ", masks="differ", dense="differ")
    S_("adaptive,dense_differ", adaptive={}, dense="differ")
    S_("frames,dense_differ", dense="differ", mode="frames", world=1)
    S_("heads,dense_differ", dense="differ", mode="heads")
    H_ = lambda name, **kw: c.__setitem__(f"A/sparse/{name}", core_case("sparse", **kw))   # noqa: E731
    H_("unfused", fused=False)
    H_("unfused,differ", fused=False, masks="differ")
    H_("unfused,quality", fused=False, quality=True)
    H_("unfused,q_prescaled", fused=False, q_prescaled=True)
    H_("unfused,return_lse", fused=False, return_lse=True)
    H_("unfused,adaptive", fused=False, adaptive={})
    H_("unfused,fp8", fused=False, fp8=True)
    H_("unfused,heads", fused=False, mode="heads")
    H_("unfused,tokens,local", fused=False, mode="tokens", _local=True)
    H_("unfused,frames", fused=False, mode="frames", world=1)
    return c


# ---------------------------------------------------------------------------------------------------------
# level B: the processors
# ---------------------------------------------------------------------------------------------------------
# (every class attribute the layer-call reads is set, defaults included: install hooks run by other tests leave theirs behind)
SVG1 = dict(num_frame=F_, frame_size=P_, first_layers_fp=1, first_times_fp=900, num_sampled_rows=6, device_switch=True, fused_placement=True,
            quality_log=None, quality_rows=64)
BAND = dict(sample_mse_max_row=10000, adaptive_band=None)   # (CogVideoX has neither)
SAP = dict(SVG1, **BAND, num_q_centroids=4, num_k_centroids=5, top_p_kmeans=0.9, min_kc_ratio=0.1, kmeans_iter_init=2, kmeans_iter_step=1,
           logging_file="density.jsonl", zero_step_kmeans_init=False, adaptive_top_p=None)
FAMILY = {   # class -> (its configuration, context_length, hunyuan's two extra arguments?)
    "hy_svg1": (HySVG, dict(SVG1, **BAND, context_length=CTX, prompt_length=4), True),
    "hy_sap": (HySAP, dict(SAP, context_length=CTX, prompt_length=4), True),
    "wan_svg1": (WanSVG, dict(SVG1, **BAND, context_length=0), False),
    "wan_sap": (WanSAP, dict(SAP, context_length=0), False),
    "cog": (Cog, dict(SVG1, context_length=CTX, first_layers_fp=1 / 42, first_times_fp=0.1), False),
    "cosmos_svg1": (CosmosSVG, dict(SVG1, **BAND, context_length=0), False),
    "cosmos_sap": (CosmosSAP, dict(SAP, context_length=0), False),
}


def proc_case(family, layer=2, t=500.0, t_gpu=False, mask="set", rows=None, cu=None, pre=False, mode=None, world=2, fp8=False, **attrs):
    """one attention_core_logic call of the family's processor at `layer`, timestep t (a CPU tensor, or the stand-in GPU tensor),
    block_mask "set" / None / a tuple, `rows` rows instead of the geometry's, Hunyuan's cu_max_seqlens, class attributes `attrs`"""
    cls, base, hy = FAMILY[family]

    def go():
        rec = Rec()
        conf = dict(base, **attrs)
        with contextlib.ExitStack() as st:
            if "SVG" in cls.__name__ or cls is Cog:
                conf["block_mask"] = rec.name(nat.BandMask(**M1), "m") if isinstance(mask, str) else mask
            for name, val in conf.items():
                st.enter_context(mock.patch.object(cls, name, val, create=True))   # (create: CogVideoX has no sample_mse_max_row)
            for name in ("band_store", "top_p_store", "centroid_store"):
                if hasattr(cls, name):
                    rec.name(getattr(cls, name), f"{cls.__name__}.{name}")
            proc = cls(layer)
            for name in ("top_p_store", "centroid_store"):
                if name in vars(proc):
                    rec.name(getattr(proc, name), f"proc.{name}")
            proc._q_prescaled = pre
            n = proc.geometry().seq_len if rows is None else rows
            q, k, v = (rec.name(_gpu(CFG, H, n, 128), nm) for nm in "qkv")
            ts = rec.name(torch.tensor([t]).as_subclass(_GpuT) if t_gpu else torch.tensor([t]), "timestep")
            args = (q, k, v, ts, 7, cu) if hy else (q, k, v, ts)   # (Hunyuan: layer_idx = 7, not the processor's own)

            def run():
                out = proc.attention_core_logic(*args)
                return [out, getattr(proc, "last_best_mask_idx", None)]

            return record(rec, run, mode=mode, world=world, fp8=fp8, level_b=True)
    return go


def _proc_cases():
    c = {}
    for fam, (cls, _, hy) in FAMILY.items():
        B = lambda name, **kw: c.__setitem__(f"B/{fam}/{name}", proc_case(fam, **kw))   # noqa: E731
        svg1 = "sap" not in fam
        knob = {"adaptive_band": _core.AdaptiveBand(target=0.9, quantum=16, rows=4, valid_len=11)} if svg1 else \
            {"adaptive_top_p": _core.AdaptiveTopP(target=0.9, rows=4, valid_len=11)}
        B("dense_by_layer", layer=0)
        B("sparse_host", sample_mse_max_row=40)
        B("sparse_switched", t_gpu=True)
        B("frames", mode="frames", world=1)
        if svg1:
            B("block_mask_unset", mask=None)
        else:
            B("zero_step_kmeans_init", layer=0, zero_step_kmeans_init=True)
        if "cosmos" in fam:   # (the Wan processors' attention_core_logic under another __call__: the cases above)
            continue
        B("dense_by_timestep,prescaled", t=950.0, pre=True)
        B("sparse_host,default_max_row")
        B("quality_log", quality_log="quality.jsonl", quality_rows=5)
        B("quality_log,heads", quality_log="quality.jsonl", mode="heads")
        B("knob", **knob)
        B("knob,dense", layer=0, **knob)
        B("knob,heads", mode="heads", **knob)
        B("wrong_row_count", rows=40)
        if svg1:
            B("sparse_switched,prescaled,max_row_40", t_gpu=True, pre=True, sample_mse_max_row=40)
            B("gpu_timestep,switch_off", t_gpu=True, device_switch=False)
            B("gpu_timestep,fp8", t_gpu=True, fp8=True)
            B("gpu_timestep,first_layers", layer=0, t_gpu=True)
            B("quality_log,switched", quality_log="quality.jsonl", t_gpu=True)
            B("knob,switched", t_gpu=True, **knob)
            B("block_mask_unset,gpu_timestep", mask=None, t_gpu=True)
            B("block_mask_unset,dense", mask=None, layer=0)
            B("unfused", fused_placement=False)
            B("unfused,gpu_timestep", fused_placement=False, t_gpu=True)
        else:
            B("zero_step_kmeans_init,sparse", zero_step_kmeans_init=True)
        if hy:
            B("valid_from_the_mask", cu=(50, S))
            B("valid_from_the_mask,dense", cu=(50, S), layer=0)
            B("valid_per_video,switched", cu=((50, 56), S), t_gpu=True)
            B("valid_per_video,dense", cu=((50, 56), S), layer=0)
            B("valid_per_video,knob,quality", cu=((50, 56), S), quality_log="quality.jsonl", **knob)
            B("mask_rows_of_the_wrong_count", cu=((50, 56, 60), S))
            B("prompt_length_tuple", prompt_length=(4, 9))
            B("prompt_length_tuple,switched", prompt_length=(4, 9), t_gpu=True)
            B("prompt_length_tuple,dense", prompt_length=(4, 9), layer=0)
            B("prompt_length_tuple_of_the_wrong_length", prompt_length=(4, 9, 9))
            if svg1:
                m, m2 = nat.BandMask(**M1), nat.BandMask(**dict(M1, real_len=56))
                B("block_mask_tuple", mask=(m, m2))
                B("block_mask_tuple,switched", mask=(m, m2), t_gpu=True)
                B("block_mask_tuple_of_the_wrong_length", mask=(m, m2, m2))
                B("block_mask_tuple_of_the_wrong_length,dense", mask=(m, m2, m2), layer=0)
    return c


CASES = {**_core_cases(), **_proc_cases()}


def dumps(records) -> str:
    """one line per case: a difference shows as one changed line"""
    return "{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, sort_keys=True, separators=(',', ':'))}" for k, v in records.items()) + "\n}\n"


def record_all() -> dict:
    return {name: json.loads(json.dumps(go())) for name, go in CASES.items()}


def _golden() -> dict:
    return json.loads(GOLDEN.read_text())


def _differing(records, golden):
    return sorted(k for k in set(records) | set(golden) if records.get(k) != golden.get(k))


# ---------------------------------------------------------------------------------------------------------
# the harness sees what it must see: six mutants of the production code, each caught by at least one case
# ---------------------------------------------------------------------------------------------------------
def _mutate(monkeypatch, fn_name: str, old: str, new: str):
    """`_core.<fn_name>` with `old` replaced by `new` in its source text"""
    src = textwrap.dedent(inspect.getsource(getattr(_core, fn_name)))
    assert src.count(old) >= 1, (fn_name, old)
    ns = {}
    exec(compile(src.replace(old, new), _core.__file__, "exec", flags=__future__.annotations.compiler_flag), vars(_core), ns)
    monkeypatch.setattr(_core, fn_name, ns[fn_name])


def _host_branch_draws_from_the_switch_generator(mp):
    real = _core.sample_mse
    mp.setattr(_core, "sample_mse", lambda *a, generator=None, **kw: real(*a, generator=generator or _core._switch_generator(), **kw))


def _cogs_thresholds_unscaled(mp):
    real = _core.svg1_core_logic
    mp.setattr(_core, "svg1_core_logic", lambda *a, thresholds=None, **kw: real(*a, **kw))


MUTANTS = {
    "host_branch_draws_from_the_switch_generator": _host_branch_draws_from_the_switch_generator,
    "max_row_not_clamped_to_the_sequence": lambda mp: _mutate(mp, "svg1_core_logic", "min(proc.sample_mse_max_row, total)", "proc.sample_mse_max_row"),
    "switched_best_without_minus_one": lambda mp: _mutate(mp, "_svg1_layer_call", "torch.where(dense_flag.reshape(()) != 0, torch.full_like(best_mask_idx, -1), best_mask_idx)", "best_mask_idx"),
    "local_override_of_token_major_out_dropped": lambda mp: _mutate(mp, "_svg1_layer_call", "if _local:", "if False:"),
    "cogs_thresholds_unscaled": _cogs_thresholds_unscaled,
    "valid_len_not_carried_into_the_adaptive_band": lambda mp: _mutate(mp, "_knob", "dataclasses.replace(knob, valid_len=valid)", "knob"),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_transcript_catches_the_mutant(mutant, monkeypatch):
    golden = _golden()
    assert not _differing(record_all(), golden)            # (clean before: what fails below is the mutant's doing)
    MUTANTS[mutant](monkeypatch)
    caught = _differing(record_all(), golden)
    assert caught, f"no case of the transcript sees the mutant {mutant}"
    print(mutant, "caught by", len(caught), "cases, e.g.", caught[:3])


def test_layer_calls_equal_the_golden_transcript():
    """Every case replayed on this tree must give the record of tests/golden/svg1_layer_calls.json, which was written on the commit named
    in tests/golden/make_golden_svg1_layer_calls.py and is not regenerated from newer code."""
    golden = _golden()
    records = record_all()
    assert set(records) == set(golden)
    bad = _differing(records, golden)
    for k in bad[:5]:
        print(k, "\n  now   ", json.dumps(records[k], sort_keys=True), "\n  golden", json.dumps(golden[k], sort_keys=True))
    assert not bad, f"{len(bad)} of {len(golden)} cases differ from the transcript: {bad[:20]}"


def test_the_transcript_covers_what_it_claims():
    golden = _golden()
    assert GOLDEN.stat().st_size <= (GOLDEN.parent / "wrapper_calls.json").stat().st_size
    raised = {tuple(r["raises"])[0] + ": " + r["raises"][1] for r in golden.values() if "raises" in r}
    for part in ("needs a band_store", "the per-head band runs", "per-video masks that differ (the groups launch)", "quality_log under svg.distributed",
                 "adaptive_band under svg.distributed", "fp32 rows go with return_lse=True", "the fused 16-bit path with a plain q",
                 "exchange o only", "no CPU fallback", "per-video values for a batch of", "token-shard mode (svg.distributed.enable_token_shards) with",
                 "head sharding (svg.distributed) with", "fp8 attention with per-video lengths", "takes ONE mask", "takes a plain q",
                 "runs the 16-bit kernels only", "is the fused path only", "returns o only", "the shard profiler is bfloat16", "takes head_dim 128",
                 "samples at most 64 rows", "needs the video at row 0", "at most 8 parts", "is not congruent", "block_mask is not set",
                 "block_mask has 3 entries", "attention_mask rows has 3 entries", "prompt_length has 3 entries", "Query Shape",
                 "SVG1 processors of HunyuanVideo and Wan only", "adaptive_top_p under svg.distributed"):
        assert any(part in r for r in raised), part
    # every refusal of the two functions comes before the first draw; the frame-shard rows come from the switched path's generator
    for name, r in golden.items():
        if "raises" in r and name.startswith("A/") and "fp8,differ" not in name:
            assert "drawn" not in r and not any(e[0] == "sample_mse" for e in r.get("calls", [])), name
    assert golden["A/sparse/one_mask"]["drawn"] == ["global"] and golden["A/switch/one_mask"]["drawn"] == ["switch"]
    assert golden["A/sparse/frames"]["drawn"] == ["switch"] and golden["A/switch/frames"]["drawn"] == ["switch"]
    assert golden["A/sparse/adaptive"]["drawn"] == ["global", "probe"] and golden["A/switch/adaptive"]["drawn"] == ["switch", "probe"]
