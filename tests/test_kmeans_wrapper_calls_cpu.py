"""What the k-means wrappers of svg._native, svg._kmeans_e4m3, svg._kmeans_metric and svg._kmeans_stepped pass to the library, pinned as
a call transcript (CPU only) with the recording stand-in of tests/test_wrapper_layout_plan_cpu.py: per wrapper call, every entry it
called in order — the *_workspace_bytes entries included, with their arguments —, every integer and float argument by value, every
pointer as the caller's tensor it is (`x`, `c_init`, ...), `ret<i>` (the i-th tensor that call returns), `new` (an allocation or a copy
first seen in this call) or `cached` (one an earlier call of the case made: the scratch of a WorkspaceCache, the buffers of a
KmeansSteppedSide), and the shapes and dtypes returned.  No kernel runs, so only strides and alignment matter.

tests/golden/kmeans_wrapper_calls.json holds the transcript of the code BEFORE the three loop wrappers shared one helper
(tests/golden/make_golden_kmeans_wrapper_calls.py names the commit); it is never regenerated from newer code."""
import functools
import json
from pathlib import Path
from unittest import mock

import pytest
import torch

import test_wrapper_layout_plan_cpu as T
from svg import _kmeans_stepped, _native as nat

GOLDEN = Path(__file__).resolve().parent / "golden" / "kmeans_wrapper_calls.json"
B, N, K, D = 4, 24, 3, 64
BF16 = torch.bfloat16


class Library(T.RecordingLibrary):
    """the stand-in, keeping the *_workspace_bytes calls as well (they still answer 256)"""

    def __init__(self):
        super().__init__()
        self.sigs.update(nat.KMEANS_METRIC_ENTRIES)      # (a table all_signatures() does not collect: it is named ..._ENTRIES)

    def __getattr__(self, name):
        if name.startswith("svg_") and name.endswith("_workspace_bytes"):
            def ws_bytes(*args):
                self.calls.append([name, [int(a) for a in args]])
                return 256
            return ws_bytes
        return super().__getattr__(name)


def make_x(kind):
    """c contiguous; bs the batch-strided view [:, :N] of [B, N + 40, D] (read in place); rs rows 2 D apart (copied); odd the bs view from a
    base 8 bytes off a 16-byte boundary (copied)"""
    if kind == "c":
        return torch.zeros(B, N, D, dtype=BF16)
    if kind == "bs":
        return torch.zeros(B, N + 40, D, dtype=BF16)[:, :N]
    if kind == "rs":
        return torch.zeros(B, N, 2 * D, dtype=BF16)[:, :, :D]
    if kind == "odd":
        n = B * (N + 40) * D
        x = torch.zeros(n + 8, dtype=BF16)[4:4 + n].view(B, N + 40, D)[:, :N]
        assert x.data_ptr() % 16 == 8
        return x
    raise KeyError(kind)


def transcript(build):
    """build() -> (the caller's tensors by name, [thunk]): every thunk is one wrapper call -> one record per thunk"""
    with T.Patched() as p:
        p.lib = Library()
        contiguous = torch.Tensor.contiguous

        def keep(self, *a, **kw):      # a copy stays alive for the whole case, so a later allocation cannot take its address
            t = contiguous(self, *a, **kw)
            p.alive.append(t)
            return t

        with mock.patch.object(torch.Tensor, "contiguous", keep):
            tensors, thunks = build()
            seen, out = set(), []
            for thunk in thunks:
                n0 = len(p.lib.calls)
                ret = thunk()
                rets = [] if ret is None else list(ret) if isinstance(ret, tuple) else [ret]
                names = {t.data_ptr(): f"ret{i}" for i, t in reversed(list(enumerate(rets)))}
                names.update({t.data_ptr(): n for n, t in reversed(list(tensors.items()))})
                fresh = set()

                def resolve(a):
                    if isinstance(a, T.Ptr):
                        if not a.value:          # (the stream of the stand-in)
                            return None
                        if a.value in names:
                            return names[a.value]
                        fresh.add(a.value)
                        return "cached" if a.value in seen else "new"
                    return [resolve(y) for y in a] if isinstance(a, list) else a

                out.append({"calls": resolve(p.lib.calls[n0:]), "ret": [[list(t.shape), str(t.dtype).replace("torch.", "")] for t in rets]})
                seen |= fresh
    return out


def cents():
    return torch.zeros(B, K, D, dtype=BF16)


def loop_case(fn, xkind, group, cached):
    x, c_init = make_x(xkind), cents()
    tensors = {"x": x, "c_init": c_init}
    work = nat.WorkspaceCache() if cached else None
    if fn == "kmeans_loop":
        tensors["xsq"] = torch.zeros(B, N)
        call = lambda: nat.kmeans_loop(x, tensors["xsq"], c_init, 5, 1e-4, work=work, group=group)  # noqa: E731
    elif fn == "kmeans_loop_e4m3":
        call = lambda: nat.kmeans_loop_e4m3(x, c_init, 5, 1e-4, 2, work=work, group=group)  # noqa: E731
    else:
        call = lambda: nat.kmeans_loop_metric(x, c_init, 5, 1e-4, "dot", work=work, group=group)  # noqa: E731
    return tensors, [call, call] if cached else [call]


def half_case(fn, **kw):
    x, c = make_x("c"), cents()
    tensors = {"x": x, "centroids": c}
    if "update" in fn:
        tensors["labels"] = torch.zeros(B, N, dtype=torch.int32)
        return tensors, [lambda: getattr(nat, fn)(x, tensors["labels"], c, **kw)]
    if kw.pop("mu", False):
        tensors["mu"] = torch.zeros(B, D)
        kw["mu"] = tensors["mu"]
    return tensors, [lambda: getattr(nat, fn)(x, c, **kw)]


def stepped_case(xkind, group, own_maxima):
    x, c_init = make_x(xkind), cents()
    tensors = {"x": x, "c_init": c_init}
    if own_maxima:
        tensors["maxima"] = torch.zeros(B // group if group else 1)
    side = []

    def iterate():
        side.append(_kmeans_stepped.KmeansSteppedSide(x, c_init, 1e-4, group=group, maxima=tensors.get("maxima")))
        side[0].iterate(0)

    return tensors, [iterate, lambda: side[0].commit(0), lambda: side[0].finish()]


def cases():
    """-> [(id, builder)]; a builder makes fresh tensors, so no case sees what another left"""
    out = []
    for fn in ("kmeans_loop", "kmeans_loop_e4m3", "kmeans_loop_metric"):
        out += [(f"{fn}.{xk}.group{g}.{'cache_twice' if w else 'fresh'}", functools.partial(loop_case, fn, xk, g, w))
                for xk in ("c", "bs", "rs", "odd") for g in (None, 2) for w in (False, True)]
    out += [(f"{fn}{''.join(f'.{k}_{v}' for k, v in kw.items())}", functools.partial(half_case, fn, **kw)) for fn, kw in (
        ("kmeans_assign", {}), ("kmeans_assign_metric", {"metric": "cosine"}), ("kmeans_assign_metric", {"metric": "dot"}),
        ("kmeans_update", {}), ("kmeans_update_metric", {"metric": "cosine"}), ("kmeans_update_metric", {"metric": "dot"}),
        ("kmeans_assign_e4m3", {}), ("kmeans_assign_e4m3", {"mu": True}))]
    out += [(f"stepped.{xk}.group{g}.{'own' if m else 'new'}_maxima", functools.partial(stepped_case, xk, g, m))
            for xk in ("c", "bs", "rs", "odd") for g in (None, 2) for m in (False, True)]
    assert len({c[0] for c in out}) == len(out)
    return out


def record_all():
    return {cid: transcript(build) for cid, build in cases()}


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_golden_holds_these_cases_and_no_others(golden):
    assert sorted(golden) == sorted(c[0] for c in cases())
    called = {c[0] for steps in golden.values() for s in steps for c in s["calls"]}
    kmeans = {n for n in T.all_signatures() if n.startswith("svg_kmeans_")} | set(nat.KMEANS_METRIC_ENTRIES)
    # outside these wrappers: the buffer-reusing single iteration (KmeansBuffers), |x|^2, the centre on its own
    assert kmeans - called == {"svg_kmeans_iter", "svg_kmeans_xsq", "svg_kmeans_centre"}, sorted(kmeans - called)


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_wrapper_calls_equal_the_golden(golden, case):
    cid, build = case
    assert json.loads(json.dumps(transcript(build))) == golden[cid]
