#!/usr/bin/env python3
"""Host time per call of the attention wrappers of svg._native, this tree against another revision's _native.py, without a GPU: both
modules run on CPU tensors against a stand-in library that launches nothing (tests/test_wrapper_layout_plan_cpu.py describes the
patching), so what is timed is the wrapper — checks, layout decision, allocations, argument marshalling.

    git show <revision>:sparse-videogen_amd/svg/_native.py > /tmp/_native_parent.py
    python tools/wrapper_host_overhead.py /tmp/_native_parent.py > profiles/<name>.txt

7 runs of 2000 calls per wrapper, input kind and module, the two modules alternating run by run; the table gives each module's median
and min..max in microseconds per call.  The rule: this tree's median may exceed the other's by no more than the other's own spread."""
import importlib.util
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "sparse-videogen_amd"))
import torch  # noqa: E402
from svg import _native as here  # noqa: E402

RUNS, CALLS = 7, 2000
B, H, S, D, NF, FS = 2, 2, 192, 128, 4, 48


class DoNothingLibrary:
    def __getattr__(self, name):
        if not name.startswith("svg_"):
            raise AttributeError(name)
        rc = 256 if name.endswith("_workspace_bytes") else 0
        return lambda *args: rc


def on_cpu(path=None):
    """svg._native (or the _native.py at `path`, loaded beside it) with the device checks off and the stand-in library"""
    if path is None:
        nat = here
    else:
        spec = importlib.util.spec_from_file_location("svg._native_other", path)
        nat = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(nat)
    lib = DoNothingLibrary()
    nat._gpu = nat._dev = lambda *ts: None
    nat._stream = lambda: 0
    nat.load = lambda strict=True: lib
    return nat


def tensors(kind, s=S):
    if kind == "contiguous":
        return [torch.zeros(B, H, s, D, dtype=torch.bfloat16) for _ in range(3)]
    return [torch.zeros(B, s, H, D, dtype=torch.bfloat16).transpose(1, 2) for _ in range(3)]


def workloads(nat, kind):
    q, k, v = tensors(kind)
    mask = nat.BandMask(S, 64, 0, 16, 0, 16)
    yield "band_attention", lambda: nat.band_attention(q, k, v, mask)
    yield "band_attention(return_lse=True)", lambda: nat.band_attention(q, k, v, mask, return_lse=True)
    yield "cross_attention", lambda: nat.cross_attention(q, k, v)
    bm = torch.ones(B * H, 1, 2, dtype=torch.bool)
    qs, ks = torch.full((B * H, 1), S, dtype=torch.int32), torch.full((B * H, 2), S // 2, dtype=torch.int32)
    yield "varblock_attention(rows_covered=True)", lambda: nat.varblock_attention(q, k, v, bm, qs, ks, rows_covered=True)
    qw, kw, vw = tensors(kind, 2 * FS)
    yield "band_shard_attention", lambda: nat.band_shard_attention(qw, kw, vw, mask, S, (0, NF, FS), (1, 2, 0, 0), (0, 2, 0, 0))


def main():
    other = on_cpu(sys.argv[1])
    this = on_cpu()
    print(f"# microseconds per call on the host (no GPU, stand-in library), {RUNS} runs of {CALLS} calls; other = {sys.argv[1]}")
    print(f"# torch {torch.__version__}, {torch.get_num_threads()} threads; q, k, v [{B}, {H}, {S}, {D}] bf16 (shard: {2 * FS} rows)")
    print(f"{'wrapper':40s} {'inputs':12s} {'other median':>12s} {'other min..max':>16s} {'this median':>12s} {'this min..max':>16s} "
          f"{'this - other':>12s} {'margin':>8s}  verdict")
    for kind in ("contiguous", "token-major"):
        for (name, f_other), (_, f_this) in zip(workloads(other, kind), workloads(this, kind)):
            times = {"other": [], "this": []}
            for f in (f_other, f_this):
                for _ in range(200):
                    f()
            for _ in range(RUNS):
                for who, f in (("other", f_other), ("this", f_this)):
                    t0 = time.perf_counter()
                    for _ in range(CALLS):
                        f()
                    times[who].append((time.perf_counter() - t0) / CALLS * 1e6)
            mo, mt = statistics.median(times["other"]), statistics.median(times["this"])
            spread = max(times["other"]) - min(times["other"])
            print(f"{name:40s} {kind:12s} {mo:12.2f} {min(times['other']):7.2f}..{max(times['other']):7.2f} {mt:12.2f} "
                  f"{min(times['this']):7.2f}..{max(times['this']):7.2f} {mt - mo:+12.2f} {spread:8.2f}  "
                  f"{'within' if mt - mo <= spread else 'SLOWER'}")


if __name__ == "__main__":
    main()
