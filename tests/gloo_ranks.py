"""The harness of the CPU rank tests of svg.distributed's schedules: gloo ranks of a worker in spawned processes, and a counting stand-in for
the all_to_all_single those schedules post.  A plain module, imported by the test files and again inside every spawned rank."""
import os
import sys
from pathlib import Path

import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent


def _rank_main(rank, world, port, worker, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (str(ROOT / "sparse-videogen_amd"), str(ROOT / "tests"), str(ROOT)):
        if p not in sys.path:
            sys.path.insert(0, p)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ret[rank] = worker(rank, world)
    dist.destroy_process_group()


def run_ranks(worker, world, port_base):
    """worker(rank, world) -> a picklable result, on `world` gloo ranks (a module-level function: the ranks are spawned) -> {rank: result}.
    port_base: the caller's own, so that tests which run side by side do not meet on a port."""
    mgr = mp.Manager()
    ret = mgr.dict()
    port = port_base + (os.getpid() % 2000) + world
    mp.spawn(_rank_main, args=(world, port, worker, ret), nprocs=world, join=True)
    got = dict(ret)
    assert sorted(got) == list(range(world))
    return got


class CountingAllToAll:
    """Installs itself as svg.distributed.dist.all_to_all_single (in a spawned rank: nothing puts the real one back) and passes every call
    on.  received: bytes of the output splits so far; splits: (input_split_sizes, output_split_sizes) of every call; reset() clears both."""

    def __init__(self):
        from svg import distributed as sd

        self.reset()
        real = sd.dist.all_to_all_single

        def counting(out, inp, output_split_sizes=None, input_split_sizes=None, **kw):
            self.received += sum(output_split_sizes) * out.element_size()
            self.splits.append((list(input_split_sizes), list(output_split_sizes)))
            assert out.numel() == sum(output_split_sizes) and inp.numel() == sum(input_split_sizes)
            return real(out, inp, output_split_sizes=output_split_sizes, input_split_sizes=input_split_sizes, **kw)

        sd.dist.all_to_all_single = counting

    def reset(self):
        self.received, self.splits = 0, []
