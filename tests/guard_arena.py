"""Shared by the op-level ``-m gpu`` suites that call a C entry on raw buffers: one NaN-filled device buffer with regions carved out
of it and guard bands between them, so that a write outside a region -- or past what the entry should write of it -- is seen."""
import ctypes as C

import numpy as np
import torch

GUARD = 256                     # floats on either side of every region


def to_device(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class Arena:
    """Regions of ``sizes`` floats; offsets are multiples of 64 floats, so every region is 256-byte aligned like a fresh allocation."""

    def __init__(self, sizes):
        self.spans, at = [], GUARD
        for n in sizes:
            self.spans.append((at, n))
            at += ((n + 63) // 64) * 64 + GUARD
        self.buf = torch.full((at,), float("nan"), dtype=torch.float32, device="cuda")

    def region(self, i):
        at, n = self.spans[i]
        return self.buf[at:at + n]

    def assert_guards_untouched(self, written):
        """Everything outside the regions is still NaN; region i is NaN beyond its first ``written[i]`` floats."""
        keep = torch.ones_like(self.buf, dtype=torch.bool)
        for (at, _n), w in zip(self.spans, written):
            keep[at:at + w] = False
        assert bool(torch.isnan(self.buf[keep]).all()), "a guard band was written"
