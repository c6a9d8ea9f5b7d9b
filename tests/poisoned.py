"""The GPU suite runs on poisoned allocations: every output and workspace the package allocates is filled with the byte 0xFF (NaN in
bf16 / fp16 / fp32, -1 in int32 / int64, 255 in uint8) before the launch, so rows, counts or workspace words that a kernel leaves unwritten
fail the oracle comparison instead of passing on what the caching allocator left there — the right answer of the previous case, or the
zeros of fresh memory.

Every GPU test module gets its `_native` from load_native() (its `nat` fixture returns it), or, where it imports `svg._native` at module
level for collection-time names, imports the autouse fixture `poison_on`.  Worker functions of spawned processes call
`_native.poison_allocations(True)` themselves; subprocesses that time something or run bench.py stay at the default (off).

fill_poison / assert_fully_written are for tests that allocate outputs or workspaces of raw C-ABI calls themselves."""
import pytest
import torch

POISON_BYTE = 0xFF


def load_native():
    from svg import _native

    _native.load()   # raises loudly if the HIP library is missing
    assert torch.cuda.is_available()
    _native.poison_allocations(True)
    return _native


@pytest.fixture(scope="module", autouse=True)
def poison_on():
    """for modules that import svg._native at module level: `from poisoned import poison_on  # noqa: F401`"""
    return load_native()


def fill_poison(t: torch.Tensor) -> torch.Tensor:
    """every byte of t's storage = 0xFF, as the package's poisoned allocations; -> t"""
    from svg import _native

    return _native.poison_storage(t)


def poisoned(*shape, dtype, device="cuda") -> torch.Tensor:
    """torch.empty(shape) with every byte 0xFF: outputs and workspaces of raw lib.svg_* calls"""
    return fill_poison(torch.empty(*shape, dtype=dtype, device=device))


def poisoned_like(t: torch.Tensor) -> torch.Tensor:
    return fill_poison(torch.empty_like(t))


_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def unwritten(t: torch.Tensor) -> torch.Tensor:
    """bool tensor of t's shape: the elements that still hold the all-ones pattern.  Compared on an integer view, so a NaN that
    arithmetic produced (0x7FC0 in bf16, 0x7FC00000 in fp32 ...) is not taken for poison.  (-1 in an integer tensor and 255 in a uint8 one ARE
    the pattern: tables use it only where those are not legitimate results.)"""
    if t.dtype == torch.bool:
        t = t.view(torch.uint8)
    if t.dtype == torch.uint8:
        return t == POISON_BYTE
    return t.view(_INT_VIEW[t.element_size()]) == -1


def assert_fully_written(t: torch.Tensor, what: str = "tensor") -> None:
    bad = unwritten(t)
    n = int(bad.sum().item())
    if n:
        first = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n} of {t.numel()} elements of {tuple(t.shape)} {t.dtype} still hold the poison pattern "
                             f"(first at {first}): nothing wrote them")
