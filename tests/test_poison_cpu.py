"""The allocation switch of svg/_native.py (poison_allocations): what it fills, what it is when off, and that no source of the package
allocates uninitialised memory round it."""
import ast
from pathlib import Path

import pytest
import torch

from svg import _native as nat

PKG = Path(__file__).resolve().parent.parent / "sparse-videogen_amd" / "svg"
DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.int32, torch.int64, torch.uint8]


@pytest.fixture
def poisoned():
    """the switch on for one test, and back to what it was"""
    was = nat.allocations_poisoned()
    nat.poison_allocations(True)
    yield nat
    nat.poison_allocations(was)


def storage_bytes(t):
    return torch.empty(0, dtype=torch.uint8).set_(t.untyped_storage())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_every_storage_byte_is_ff(poisoned, dtype):
    like = torch.zeros(3, 5, dtype=dtype)
    for t in (nat.empty((3, 5, 7), dtype=dtype), nat.empty(11, dtype=dtype, device="cpu"), nat.empty_like(like),
              nat.empty_like(like.t(), memory_format=torch.contiguous_format)):
        b = storage_bytes(t)
        assert b.numel() == t.numel() * t.element_size() and bool((b == 0xFF).all()), (dtype, tuple(t.shape))
    t = nat.empty((4, 6), dtype=dtype)
    if dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
    elif dtype == torch.uint8:
        assert bool((t == 255).all())
    else:
        assert bool((t == -1).all())
    assert nat.empty(0, dtype=dtype).numel() == 0   # nothing to fill


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=lambda d: str(d).split(".")[-1])
def test_token_major_view_poisons_the_whole_storage(poisoned, dtype):
    like = torch.zeros(2, 3, 5, 8, dtype=dtype)
    o = nat.token_major_empty(like)
    assert o.shape == like.shape and o.stride() == (5 * 3 * 8, 8, 3 * 8, 1)   # [B, H, S, D] stored [B, S, H, D]
    b = storage_bytes(o)
    assert b.numel() == like.numel() * like.element_size() and bool((b == 0xFF).all())
    # a slice of a larger allocation: poison_storage covers what was allocated, not the logical elements
    base = torch.zeros(64, dtype=dtype)
    nat.poison_storage(base[8:16])
    assert bool((storage_bytes(base) == 0xFF).all())


def test_caller_tensors_are_not_touched(poisoned):
    x = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    y = nat.empty_like(x)
    assert bool(torch.isnan(y).all()) and x.tolist() == torch.arange(12, dtype=torch.float32).reshape(3, 4).tolist()


def test_off_is_torch_itself():
    was = nat.allocations_poisoned()
    try:
        nat.poison_allocations(False)
        assert nat.empty is torch.empty and nat.empty_like is torch.empty_like and not nat.allocations_poisoned()
        nat.poison_allocations(True)
        assert nat.empty is not torch.empty and nat.empty_like is not torch.empty_like and nat.allocations_poisoned()
        nat.poison_allocations(False)
        assert nat.empty is torch.empty and nat.empty_like is torch.empty_like
    finally:
        nat.poison_allocations(was)


def test_default_is_off():
    """a fresh interpreter: the production path and bench.py allocate with torch's own functions"""
    import subprocess
    import sys

    code = ("import sys, torch; sys.path.insert(0, sys.argv[1]); from svg import _native as n; "
            "assert n.empty is torch.empty and n.empty_like is torch.empty_like and not n.allocations_poisoned()")
    r = subprocess.run([sys.executable, "-c", code, str(PKG.parent)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


# the two callables are defined by these functions of svg/_native.py; nothing else may call torch's uninitialised allocators
ALLOWED = {("_native.py", "_poisoned_empty"), ("_native.py", "_poisoned_empty_like")}
BANNED_TORCH = {"empty", "empty_like", "empty_strided"}
BANNED_METHODS = {"new_empty", "new_empty_strided"}


def _offenders(path: Path):
    tree = ast.parse(path.read_text(), filename=str(path))
    out = []

    def walk(node, func):
        for child in ast.iter_child_nodes(node):
            f = child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) else func
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute):
                a = child.func
                torch_call = a.attr in BANNED_TORCH and isinstance(a.value, ast.Name) and a.value.id == "torch"
                if (torch_call or a.attr in BANNED_METHODS) and (path.name, func) not in ALLOWED:
                    out.append(f"{path}:{child.lineno}: {ast.unparse(a)}(...) in {func or '<module>'}")
            walk(child, f)

    walk(tree, None)
    return out


def test_no_allocation_goes_round_the_switch():
    files = sorted(PKG.rglob("*.py"))
    assert any(p.name == "_native.py" for p in files) and len(files) > 10
    bad = [line for p in files for line in _offenders(p)]
    assert not bad, "uninitialised allocations that bypass svg._native.empty / empty_like:\n" + "\n".join(bad)


def test_the_walk_sees_what_it_should(tmp_path):
    src = ("import torch\n\ndef f(x):\n    a = torch.empty(3)\n    b = x.new_empty(2)\n    c = torch.empty_strided((2,), (1,))\n"
           "    return torch.empty_like(x), a, b, c\n\nclass K:\n    def g(self):\n        return [torch.empty(1) for _ in range(2)]\n")
    p = tmp_path / "m.py"
    p.write_text(src)
    got = _offenders(p)
    assert len(got) == 5 and [int(s.split(":")[-2]) for s in got] == [4, 5, 6, 7, 11], got
