"""What tests/test_kmeans_stepped_cpu.py and tests/test_gpu_kmeans_stepped.py share (include/svg_attn_kmeans_stepped.h, svg.kmeans_utils
lloyd_stepped).  Plain module, no GPU."""
import torch


class TorchSteppedSide:
    """A side of svg.kmeans_utils.lloyd_stepped as a torch statement on any device: the state machine of svg_kmeans_stepped_iterate / _commit /
    _finish (csrc/kmeans.hip: stopped flags, n_iters, the selector among c_init and the two work buffers) around a `step(cur, it)` of the
    form lloyd_device_rule takes.  maxima: this side's slice, float [G] (G = 1 without a group)."""

    def __init__(self, step, c_init, tol, group=None, maxima=None):
        self.step, self.c_init, self.tol = step, c_init, tol
        self.B = c_init.shape[0]
        self.grouped = group is not None
        self.group = self.B if group is None else group
        self.G = self.B // self.group
        self.maxima = torch.full((self.G,), float("nan"), device=c_init.device) if maxima is None else maxima
        assert self.maxima.shape == (self.G,)
        self.c = [c_init, None, None]          # what the selector indexes: 0 initial, 1 / 2 the two work buffers
        self.calls = []

    def _mask(self, flag, nd):
        return flag.repeat_interleave(self.group).view((self.B,) + (1,) * (nd - 1))

    def iterate(self, it):
        self.calls.append(("iterate", it))
        if it == 0:
            self.stopped = torch.zeros(self.G, dtype=torch.bool, device=self.c_init.device)
            self.n = torch.zeros(self.G, dtype=torch.int32, device=self.c_init.device)
            self.sel = torch.zeros(self.G, dtype=torch.int64, device=self.c_init.device)
        cur = self.c[0 if it == 0 else (1 if it & 1 else 2)]
        c_out, labels, counts, sorted_idx, shift = self.step(cur, it)
        self.c[2 if it & 1 else 1] = c_out.clone()
        self.scratch = (labels.clone(), counts.clone(), sorted_idx.clone())
        self.maxima.copy_(shift.view(self.G, self.group).max(dim=1).values)   # (torch.max propagates a NaN)
        return self.maxima

    def commit(self, it):
        self.calls.append(("commit", it))
        conv = self.maxima < self.tol                                          # (NaN < tol is False)
        sel_cur, sel_out = (0 if it == 0 else (1 if it & 1 else 2)), (2 if it & 1 else 1)
        run = ~self.stopped
        if it == 0:
            self.labels, self.counts, self.sorted_idx = self.scratch
        else:
            self.labels, self.counts, self.sorted_idx = (torch.where(self._mask(run, 2), new, old) for new, old in
                                                         zip(self.scratch, (self.labels, self.counts, self.sorted_idx)))
        self.n = self.n + run.to(torch.int32)
        self.sel = torch.where(run, torch.where(conv, sel_cur, sel_out), self.sel)
        self.stopped = self.stopped | conv

    def finish(self):
        self.calls.append(("finish",))
        cent = self.c_init.clone()
        for s in (1, 2):
            if self.c[s] is not None:
                cent = torch.where(self._mask(self.sel == s, 3), self.c[s], cent)
        n = self.n if self.grouped else self.n.view(())
        return self.labels, cent, self.counts, n, self.sorted_idx


def same_five(stepped, rule):
    """(labels, centroids, counts, n_iters, sorted) of a side's finish() against lloyd_device_rule's (labels, centroids, counts, sorted,
    n_iters): all five bit for bit (centroids on their integer view: NaN included)"""
    lab, cent, cnt, n, srt = stepped
    rl, rc, rk, rs, rn = rule
    return (torch.equal(lab.to(torch.int64), rl.to(torch.int64)) and torch.equal(cent.view(torch.int16), rc.view(torch.int16))
            and torch.equal(cnt, rk) and torch.equal(srt, rs) and n.shape == rn.shape and torch.equal(n.to(torch.int64), rn.to(torch.int64)))
