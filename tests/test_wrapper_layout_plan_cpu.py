"""The layout decisions of the attention wrappers of svg._native / svg._probe / svg._adaptive, pinned as a call transcript (CPU only).

The wrappers run on CPU tensors once `_gpu` / `_dev` are no-ops, `_stream` returns 0 and `load` returns a stand-in that records every
entry it is asked for and launches nothing.  One record per case then says which entries a wrapper called and in which order, which of
the caller's tensors every pointer argument is (or `new`: a copy or a fresh allocation; `ret<i>`: the i-th tensor the wrapper returns),
the svg_attn_layout_t it passed (NULL or heads + twelve strides), every integer / float / mask argument by value, what it returned
(shape, dtype, strides, is it the caller's `out`) and what it filled on the host (the allocation hook hands out tensors full of a
sentinel: `zero`, `-inf`, `untouched`).  A case a wrapper refuses records the exception, its message and whether `load` had been called.

tests/golden/wrapper_calls.json holds the transcript of the code BEFORE the wrappers shared one layout plan
(tests/golden/make_golden_wrapper_calls.py names the commit).  It is the definition of "the wrappers behave as they did", quirks
included; it is never regenerated from newer code."""
import ctypes as C
import json
from pathlib import Path

import pytest
import torch

from svg import _adaptive, _native as nat, _probe

GOLDEN = Path(__file__).resolve().parent / "golden" / "wrapper_calls.json"
SENTINEL = 7
H, S, NF, FS = 2, 192, 4, 48            # heads per video, rows, and the video of the window / shard / profiler cases: 4 frames of 48 rows
SUB = 2 * FS                            # rows of a window / a shard
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


# ------------------------------------------------------------------------------------------------------
# tensors of every kind the wrappers distinguish
# ------------------------------------------------------------------------------------------------------
def make(kind, shape, dtype=BF16, fill=0):
    """A [B, H, S, D] (or [BH, S, D]) tensor: c contiguous, tm token-major view, bad stride(-1) != 1, odd a token-major view that
    starts at an odd element (describable but for its 16-byte alignment)"""
    *lead, s, d = shape
    n = 1
    for x in shape:
        n *= x
    head = len(lead)                       # the head dimension: 1 of [B, H, S, D], 0 of [BH, S, D]
    tm_shape = (*lead[:-1], s, lead[-1], d)
    if kind == "c":
        t = torch.empty(shape, dtype=dtype)
    elif kind == "tm":
        t = torch.empty(tm_shape, dtype=dtype).transpose(head - 1, head)
    elif kind == "bad":
        t = torch.empty((*lead, s, 2 * d), dtype=dtype)[..., ::2]
    elif kind == "odd":
        t = torch.empty(n + 8, dtype=dtype)[1:1 + n].view(tm_shape).transpose(head - 1, head)
    else:
        raise KeyError(kind)
    assert tuple(t.shape) == tuple(shape)
    t.fill_(fill)
    return t


def qkv(kind, B, D, sq=S, sk=None, dtype=BF16, dim3=False):
    """(q, k, v) of an input kind; mixed: q a view, k / v contiguous; 3d: contiguous [BH, S, D]"""
    sk = sq if sk is None else sk
    lead = (B * H,) if (dim3 or kind == "3d") else (B, H)
    kq = {"mixed": "tm", "3d": "c"}.get(kind, kind)
    kk = {"mixed": "c", "3d": "c"}.get(kind, kind)
    return make(kq, (*lead, sq, D), dtype), make(kk, (*lead, sk, D), dtype), make(kk, (*lead, sk, D), dtype)


IN_KINDS = ("c", "tm", "bad", "odd", "mixed", "3d")
OUT_KINDS = ("none", "flag", "c", "tm", "bad")           # flag: token_major_out=True


def out_kw(okind, q, dtype=None, flag=True):
    """the out / token_major_out keywords of an output kind, `out` full of the sentinel"""
    if okind == "none":
        return {}
    if okind == "flag":
        assert flag
        return {"token_major_out": True}
    return {"out": make(okind, tuple(q.shape), dtype or q.dtype, SENTINEL)}


# ------------------------------------------------------------------------------------------------------
# the recording stand-in
# ------------------------------------------------------------------------------------------------------
class Ptr:
    """a pointer argument, named once the wrapper has returned"""

    def __init__(self, value):
        self.value = value


def all_signatures():
    table = {}
    for name in dir(nat):
        if name.endswith("SIGNATURES") and isinstance(getattr(nat, name), dict):
            table.update(getattr(nat, name))
    return table


def decode(obj, ctype=None):
    """a ctypes argument by value: pointers as Ptr, structures and arrays as lists"""
    if obj is None:
        return None
    if hasattr(obj, "_obj"):                 # C.byref(x)
        obj = obj._obj
    if isinstance(obj, C.Array):
        return [decode(x, obj._type_) for x in obj]
    if isinstance(obj, C.Structure):
        return [decode(getattr(obj, f), t) for f, t in obj._fields_]
    if ctype is C.c_void_p:
        return Ptr(obj)
    if isinstance(obj, float):
        return C.c_float(obj).value if ctype is C.c_float else obj
    return int(obj)


class RecordingLibrary:
    """Stands in for libsvgattn.so as DoNothingLibrary of tests/test_gpu_poison.py does — every svg_* entry returns 0, *_workspace_bytes
    256 — and keeps what every other entry was called with."""

    def __init__(self):
        self.calls = []
        self.sigs = all_signatures()

    def __getattr__(self, name):
        if not name.startswith("svg_"):
            raise AttributeError(name)
        if name.endswith("_workspace_bytes"):
            return lambda *args: 256
        argtypes = self.sigs[name][1]

        def entry(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            rec = []
            for a, t in zip(args, argtypes):
                if t is C.c_void_p and isinstance(a, C.c_void_p):     # an array of part pointers (merge_attention_states)
                    rec.append(decode((C.c_void_p * nat.MERGE_MAX_PARTS).from_address(a.value)))
                elif t is C.c_void_p:
                    rec.append(None if a is None else Ptr(int(a)))
                elif t is C.c_float:
                    rec.append(float(f"{a:.7g}"))
                else:
                    rec.append(decode(a))
            self.calls.append([name, rec])
            return 0
        return entry


class Patched:
    """svg._native on the CPU: no device checks, stream 0, the recording library, allocations full of the sentinel and kept alive"""

    NAMES = ("_gpu", "_dev", "_stream", "load", "empty", "empty_like")

    def __enter__(self):
        self.saved = {n: getattr(nat, n) for n in self.NAMES}
        self.lib, self.loaded, self.alive = RecordingLibrary(), False, []

        def load(strict=True):
            self.loaded = True
            return self.lib

        def hook(fn):
            def alloc(*args, **kwargs):
                t = fn(*args, **kwargs)
                if t.numel():
                    torch.zeros(0, dtype=t.dtype).set_(t.untyped_storage()).fill_(SENTINEL)
                self.alive.append(t)
                return t
            return alloc

        nat._gpu = nat._dev = lambda *ts: None
        nat._stream = lambda: 0
        nat.load = load
        nat.empty, nat.empty_like = hook(torch.empty), hook(torch.empty_like)
        nat._F8_WS.clear()
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(nat, n, f)
        nat._F8_WS.clear()
        return False


def fill_state(t):
    if t.numel() == 0:
        return "empty"
    f = t.float()
    for name, value in (("untouched", float(SENTINEL)), ("zero", 0.0), ("-inf", float("-inf"))):
        if bool((f == value).all()):
            return name
    return "mixed"


def transcript(fn, kwargs):
    """run fn(**kwargs) under the stand-in -> the record of the case"""
    tensors = {n: t for n, t in kwargs.items() if isinstance(t, torch.Tensor)}
    for n, ts in kwargs.items():
        if isinstance(ts, (list, tuple)) and ts and isinstance(ts[0], torch.Tensor):
            tensors.update({f"{n}{i}": t for i, t in enumerate(ts)})
    with Patched() as p:
        try:
            ret = fn(**kwargs)
        except (ValueError, AssertionError, RuntimeError, AttributeError, TypeError) as e:
            return {"raises": [type(e).__name__, str(e)[:120], p.loaded]}
        rets = list(ret) if isinstance(ret, tuple) else [ret]
        names = {}
        for i, t in reversed(list(enumerate(rets))):
            if t is not None:
                names[t.data_ptr()] = f"ret{i}"
        for n, t in reversed(list(tensors.items())):
            names[t.data_ptr()] = n

        def resolve(x):
            if isinstance(x, Ptr):
                return None if x.value is None else names.get(x.value, "new")
            return [resolve(y) for y in x] if isinstance(x, list) else x

        out = kwargs.get("out")
        return {"calls": resolve(p.lib.calls),
                "ret": [None if t is None else [list(t.shape), str(t.dtype).replace("torch.", ""), list(t.stride()), fill_state(t),
                                                bool(out is not None and t is out)] for t in rets]}


# ------------------------------------------------------------------------------------------------------
# the cases: (input kind, output kind) pairs per wrapper form.  Output kinds that no wrapper tells apart are not repeated on every form:
# FULL on the plain forms that own a fall-back of their own, LITE — every path once: NULL layout, views, copies, a stand-in for out,
# the flag with and without a usable layout — on the others
# ------------------------------------------------------------------------------------------------------
FULL = [(i, o) for i in ("c", "tm", "bad", "3d") for o in OUT_KINDS] + [(i, o) for i in ("odd", "mixed") for o in ("none", "flag", "c")]
LITE = [("c", "none"), ("c", "flag"), ("tm", "none"), ("tm", "flag"), ("tm", "tm"), ("bad", "flag"), ("bad", "tm"), ("tm", "bad")]
INS = [(i, "none") for i in IN_KINDS]
VIDEO = dict(vid0=0, num_frame=NF, frame_size=FS)


def mask(real=S):
    return nat.BandMask(real, 64, 0, 16, 0, 16)


def i32(*v):
    return torch.tensor(v, dtype=torch.int32)


def flag64(B):
    return torch.zeros(B * H, dtype=torch.int64)


def rows8():
    return torch.arange(8, dtype=torch.int64)


def prof():
    p = nat.ProfileDesc(0, NF, FS, 1)
    p.variant[0] = nat.ProfileVariant(0, 0, S, 1, 0, 0, 0)
    p.variant[1] = nat.ProfileVariant(1, 0, S, 1, 0, 0, 0)
    return p


def band_kw(ik, ok, B, D, done=False, **extra):
    q, k, v = qkv(ik, B, D)
    kw = dict(q=q, k=k, v=v, mask=mask(), head_perm_flag=flag64(B), **VIDEO, **extra, **out_kw(ok, q))
    if done:
        kw["done"] = torch.zeros(B * H * 2, dtype=torch.int32)
    return kw


def switch_kw(ik, ok, B, D, **extra):
    return dict(band_kw(ik, ok, B, D, **extra), alt_mask=mask(S - 1), use_alt_flag=i32(0))


def groups_kw(ik, ok, B, D, split=False, **extra):
    kw = band_kw(ik, ok, B, D, **extra)
    gh = [1, B * H - 1] if split else [H] * B
    kw.pop("mask")
    return dict(kw, masks=[mask()] * len(gh), group_heads=gh)


def sub_kw(ik, ok, B, D, sk=SUB):
    """q, k, v of a window / a shard; output kind f32: out_dtype=torch.float32"""
    q, k, v = qkv(ik, B, D, SUB, sk)
    return dict(q=q, k=k, v=v, mask=mask(), num_tokens=S, **({"out_dtype": F32} if ok == "f32" else out_kw(ok, q, flag=False)))


def window_kw(ik, ok, B, D, **extra):
    return dict(sub_kw(ik, ok, B, D, **extra), q_begin=FS, k_begin=64)


def shard_kw(ik, ok, B, D):
    return dict(sub_kw(ik, ok, B, D), perm=(0, NF, FS), q_shard=(1, 2, 0, 0), k_shard=(0, 2, 0, 0), flags=flag64(B))


def shard_switch_kw(ik, ok, B, D):
    return dict(shard_kw(ik, ok, B, D), alt_mask=mask(S - 1), use_alt_flag=i32(1))


def cross_kw(ik, ok, B, D, keyrange=False, **extra):
    q, k, v = qkv(ik, B, D, S, 64)
    kr = dict(kv_end=i32(*[64] * B), kv_begin=i32(*[0] * B)) if keyrange else {}
    return dict(q=q, k=k, v=v, **kr, **extra, **out_kw(ok, q))


def pair_kw(ik, ok, B, D, bk="c"):
    q, k, v = qkv(ik, B, D, S, 64)
    _, kb, vb = qkv("c" if ik == "3d" else bk, B, D, S, 32, dim3=ik == "3d")   # (the second key set has its own describability)
    return dict(q=q, k_a=k, v_a=v, k_b=kb, v_b=vb, **out_kw(ok, q))


def merge_kw(ik, ok, B, D, pdt=BF16, lse=False):
    lead = (B * H,) if ik == "3d" else (B, H)
    parts = [make("c" if ik == "3d" else ik, (*lead, S, D), pdt) for _ in range(2)]
    kw = dict(o_parts=parts, lse_parts=[torch.zeros((*lead, S), dtype=F32) for _ in range(2)], return_lse=lse, **out_kw(ok, parts[0], BF16))
    if pdt == F32 and "out" not in kw:
        kw["out_dtype"] = BF16
    return kw


def varblock_kw(ik, ok, B, D, QB=1, cov=True, **extra):
    """S = 192: 160 * QB <= S for one block-row only"""
    q, k, v = qkv(ik, B, D)
    BH = B * H
    return dict(q=q, k=k, v=v, block_map=torch.ones((BH, QB, 2), dtype=torch.bool), q_sizes=torch.full((BH, QB), S // QB, dtype=torch.int32),
                k_sizes=torch.full((BH, 2), S // 2, dtype=torch.int32), rows_covered=cov, **extra, **out_kw(ok, q))


def mse_kw(ik, ok, B, D, dtype=BF16, skip=False):
    q, k, v = qkv(ik, B, D, dtype=dtype)
    return dict(q=q, k=k, v=v, rows=rows8(), prof=prof(), skip_flag=i32(0) if skip else None)


def partial_kw(ik, ok, B, D, skip=False):
    _, k, v = qkv("tm", B, D, SUB, SUB) if ik == "4d" else qkv(ik, B, D, SUB, SUB, dim3=True)
    return dict(q_rows=make("tm" if ik == "tm" else "c", (B * H, 8, D)), k=k, v=v, rows=rows8(), prof=prof(), k_shard=(0, 2, 0, 0),
                num_tokens=S, skip_flag=i32(0) if skip else None)


def rows_kw(ik, ok, B, D):
    q, k, v = qkv(ik, B, D)
    return dict(q=q, k=k, v=v, rows=rows8(), valid_len=S - 8)


def lse_kw(ik, ok, B, D):
    kw = rows_kw(ik, ok, B, D)
    kw.pop("v")
    return kw


LSE, F32P = {"return_lse": True}, {"return_lse": True, "out_dtype": F32}
NONE3 = [("c", "none"), ("tm", "none"), ("bad", "none")]
FEW = [("c", "none"), ("c", "flag"), ("c", "tm"), ("tm", "none"), ("tm", "flag")]
SMALL = [("c", "none"), ("tm", "flag")]          # what runs again at B = 1 and at D = 64

# (id prefix, wrapper, keyword builder, (input, output) pairs, (B, D), the builder's own keywords)
TABLE = [
    ("band.plain", "band_attention", band_kw, FULL, (2, 128), {}),
    ("band.lse", "band_attention", band_kw, LITE + INS[3:], (2, 128), LSE),
    ("band.f32", "band_attention", band_kw, INS + [("c", "flag"), ("c", "c")], (2, 128), F32P),      # (the last two are refused)
    ("band.prescaled", "band_attention", band_kw, LITE, (2, 128), {"q_prescaled": True}),
    ("band.done", "band_attention", band_kw, [("c", "none"), ("tm", "none"), ("c", "tm")], (2, 128), {"done": True}),
    ("band.prescaled_done", "band_attention", band_kw, [("c", "none")], (2, 128), {"done": True, "q_prescaled": True}),
    ("band.variant3", "band_attention", band_kw, [("c", "none"), ("tm", "flag"), ("c", "tm")], (2, 128), {"variant": 3}),
    ("switch.plain", "band_attention_switch", switch_kw, LITE, (2, 128), {}),
    ("switch.prescaled", "band_attention_switch", switch_kw, SMALL, (2, 128), {"q_prescaled": True}),
    ("switch.lse", "band_attention_switch", switch_kw, LITE, (2, 128), LSE),
    ("switch.f32", "band_attention_switch", switch_kw, NONE3, (2, 128), F32P),
    ("groups.whole.plain", "band_attention_groups", groups_kw, LITE + [("3d", "flag")], (2, 128), {}),
    ("groups.whole.prescaled", "band_attention_groups", groups_kw, SMALL, (2, 128), {"q_prescaled": True}),
    ("groups.whole.lse", "band_attention_groups", groups_kw, LITE, (2, 128), LSE),
    ("groups.whole.f32", "band_attention_groups", groups_kw, NONE3, (2, 128), F32P),
    ("groups.split.plain", "band_attention_groups", groups_kw, FEW, (2, 128), {"split": True}),
    ("groups.split.lse", "band_attention_groups", groups_kw, FEW, (2, 128), dict(LSE, split=True)),
    ("groups.split.f32", "band_attention_groups", groups_kw, [("tm", "none")], (2, 128), dict(F32P, split=True)),
    ("window", "band_window_attention", window_kw, [(i, o) for i in ("c", "tm", "bad", "3d") for o in ("none", "c", "tm", "bad")]
     + [("odd", "none"), ("mixed", "none")] + [(i, "f32") for i in ("c", "tm", "bad")], (2, 128), {}),
    ("window.nokeys", "band_window_attention", window_kw, [("c", "none")], (2, 128), {"sk": 0}),    # answered without a launch
    ("shard", "band_shard_attention", shard_kw, NONE3 + [("tm", "tm"), ("bad", "tm"), ("tm", "bad"), ("c", "f32"), ("tm", "f32")], (2, 128), {}),
    ("shard_switch", "band_shard_attention_switch", shard_switch_kw, [("c", "none"), ("tm", "tm"), ("tm", "bad"), ("tm", "f32")], (2, 128), {}),
    ("cross.plain", "cross_attention", cross_kw, FULL, (2, 128), {}),
    ("cross.lse", "cross_attention", cross_kw, LITE, (2, 128), LSE),
    ("cross.f32", "cross_attention", cross_kw, NONE3, (2, 128), F32P),
    ("keyrange.plain", "cross_attention_keyrange", cross_kw, SMALL + [("bad", "tm"), ("tm", "bad")], (2, 128), {"keyrange": True}),
    ("keyrange.lse", "cross_attention_keyrange", cross_kw, SMALL, (2, 128), dict(LSE, keyrange=True)),
    ("keyrange.f32", "cross_attention_keyrange", cross_kw, SMALL[:1] + [("tm", "none")], (2, 128), dict(F32P, keyrange=True)),
    ("pair", "cross_attention_pair", pair_kw, LITE + [("3d", "flag")], (2, 128), {}),
    ("pair.b_tm", "cross_attention_pair", pair_kw, [("c", "none"), ("tm", "flag"), ("tm", "tm")], (2, 128), {"bk": "tm"}),
    ("pair.b_bad", "cross_attention_pair", pair_kw, [("c", "none"), ("tm", "flag"), ("tm", "tm")], (2, 128), {"bk": "bad"}),
    ("merge.bf16", "merge_attention_states", merge_kw, [("c", o) for o in OUT_KINDS] + [("tm", "none"), ("tm", "flag"), ("3d", "none"), ("3d", "flag")],
     (2, 128), {}),
    ("merge.bf16.lse", "merge_attention_states", merge_kw, [("c", "none"), ("c", "bad")], (2, 128), {"lse": True}),
    ("merge.f32", "merge_attention_states", merge_kw, [("c", o) for o in OUT_KINDS] + [("tm", "none"), ("tm", "flag"), ("3d", "none"), ("3d", "flag")],
     (2, 128), {"pdt": F32}),
    ("merge.f32.lse", "merge_attention_states", merge_kw, [("c", "none"), ("c", "bad")], (2, 128), {"pdt": F32, "lse": True}),
    ("varblock.plain", "varblock_attention", varblock_kw, [(i, o) for i in IN_KINDS for o in ("none", "flag")], (2, 128), {}),
    ("varblock.plain.cov0", "varblock_attention", varblock_kw, [("c", "none"), ("tm", "flag"), ("bad", "flag")], (2, 128), {"cov": False}),
    ("varblock.plain.QB2", "varblock_attention", varblock_kw, [("c", "flag"), ("tm", "none"), ("tm", "flag")], (2, 128), {"QB": 2}),
    ("varblock.fp8", "varblock_attention", varblock_kw, [("c", "none"), ("c", "flag"), ("tm", "flag")], (2, 128), {"fp8": True}),
    ("varblock.fp8.cov0", "varblock_attention", varblock_kw, [("tm", "none")], (2, 128), {"fp8": True, "cov": False}),
    ("varblock.variant0", "varblock_attention", varblock_kw, [("c", "none"), ("c", "flag"), ("tm", "flag")], (2, 128), {"variant": 0}),
    ("varblock.lse", "varblock_attention", varblock_kw, [(i, o) for i in IN_KINDS for o in ("none", "flag")], (2, 128), LSE),
    ("varblock.lse.cov0", "varblock_attention", varblock_kw, [("c", "none"), ("tm", "flag"), ("bad", "flag")], (2, 128), dict(LSE, cov=False)),
    ("varblock.lse.QB2", "varblock_attention", varblock_kw, [("c", "flag"), ("tm", "none")], (2, 128), dict(LSE, QB=2)),
    ("varblock.f32", "varblock_attention", varblock_kw, NONE3, (2, 128), F32P),
    ("varblock.f32.cov0", "varblock_attention", varblock_kw, [("tm", "none")], (2, 128), dict(F32P, cov=False)),
    ("sample_mse.bf16", "sample_mse", mse_kw, INS, (2, 128), {}),
    ("sample_mse.bf16.skip", "sample_mse", mse_kw, [("c", "none"), ("tm", "none")], (2, 128), {"skip": True}),
    ("sample_mse.fp16", "sample_mse", mse_kw, NONE3, (2, 128), {"dtype": F16}),
    ("sample_mse.fp16.skip", "sample_mse", mse_kw, [("tm", "none")], (2, 128), {"dtype": F16, "skip": True}),
    ("shard_partial", "sample_mse_shard_partial", partial_kw, [(i, "none") for i in ("c", "tm", "bad", "odd", "4d")], (2, 128), {}),
    ("shard_partial.skip", "sample_mse_shard_partial", partial_kw, [("tm", "none")], (2, 128), {"skip": True}),
    ("dense_rows", "sample_dense_rows", rows_kw, INS[:5], (2, 128), {}),
    ("dense_lse", "sample_dense_lse", lse_kw, INS[:5], (2, 128), {}),
]
# B = 1 and D = 64 where the wrapper takes it (the LSE forms refuse D = 64: one refusal each pins the message)
for B, D in ((1, 128), (2, 64)):
    TABLE += [(f"{name}.B{B}.D{D}", fn, kw, SMALL if extra is not LSE else SMALL[1:], (B, D), extra) for name, fn, kw, extra in (
        ("band.plain", "band_attention", band_kw, {}), ("band.lse", "band_attention", band_kw, LSE),
        ("switch.lse", "band_attention_switch", switch_kw, LSE), ("groups.whole.lse", "band_attention_groups", groups_kw, LSE),
        ("cross.plain", "cross_attention", cross_kw, {}), ("pair", "cross_attention_pair", pair_kw, {}),
        ("varblock.plain", "varblock_attention", varblock_kw, {}), ("varblock.lse", "varblock_attention", varblock_kw, LSE),
        ("dense_rows", "sample_dense_rows", rows_kw, {}), ("dense_lse", "sample_dense_lse", lse_kw, {}))]


def cases():
    """-> [(id, wrapper, keyword builder)]; a builder makes fresh tensors, so no case sees what another left"""
    import functools

    out = []
    for name, fn, kw, pairs, (B, D), extra in TABLE:
        wrapper = getattr(_adaptive if fn == "sample_dense_lse" else _probe if fn == "sample_dense_rows" else nat, fn)
        out += [(f"{name}.{ik}.{ok}", wrapper, functools.partial(kw, ik, ok, B, D, **extra)) for ik, ok in pairs]
    assert len({c[0] for c in out}) == len(out)
    return out


def record_all():
    return {cid: transcript(fn, build()) for cid, fn, build in cases()}


def dumps(records):
    """one record per line, no indentation"""
    return "{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, separators=(',', ':'))}" for k, v in records.items()) + "\n}\n"


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_golden_holds_these_cases_and_no_others(golden):
    assert sorted(golden) == sorted(c[0] for c in cases())


def test_every_wrapper_is_in_the_transcript(golden):
    called = {c[0] for r in golden.values() for c in r.get("calls", [])}
    attention = {n for n in all_signatures() if ("attention" in n or n.startswith("svg_sample_")) and not n.endswith("_workspace_bytes")}
    # outside this file's wrappers: the fp8 band entry, the completion-counter queries and the plain notify entry (band_attention takes the
    # segmented one), the combine over profiler partials
    attention -= {"svg_band_attention_fp8", "svg_band_attention_fp8_stage", "svg_band_attention_notify_target", "svg_band_attention_notify",
                  "svg_band_attention_notify_layout", "svg_sample_mse_from_parts"}
    assert attention <= called, sorted(attention - called)


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_wrapper_calls_equal_the_golden(golden, case):
    cid, fn, build = case
    got = json.loads(json.dumps(transcript(fn, build())))
    assert got == golden[cid]
