"""Guarded device buffers for the tests that call the C ABI with raw pointers (a plain helper module, no fixtures).

A caller of include/ge2e_hip.h may pass buffers of exactly the documented sizes.  torch's caching allocator rounds every
allocation up, so a store one row past the end of a tensor of its own lands in slack nobody looks at.  Here every buffer
is a slice out of the middle of a larger allocation, with guard bands either side that must come back untouched:

    Buf        float32 (or float64): NaN guards; inputs carry data, outputs NaN poison (a read outside an input
               shows as a NaN result)
    IntBuf     int32 (or int64): a sentinel in the guards (and in outputs, as poison)
    Workspace  bytes:   the inner region starts 256-byte aligned, is exactly `nbytes` long, has >= 256 guard bytes either
                        side; the whole allocation is filled with one byte pattern and the guards are compared byte for byte
"""
import numpy as np
import torch

G = 64                   # guard elements either side of Buf / IntBuf (256 bytes: keeps 16-byte alignment)
WS_GUARD = 256           # guard bytes either side of a Workspace (keeps its 256-byte alignment)
SENTINEL = -1234567891   # int32 guard / poison value: no count, index or offset of any test reaches it


def dev():
    return torch.device("cuda:0")


def same_bits(a, b):
    """Two float32 arrays a caller fetched: the same shape and the same bits (NaN payloads and the sign of zero included)."""
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class _Guarded:
    """n elements between two guard bands of `FILL`; inputs carry data, outputs `FILL` as poison.  `offset` shifts the inner
    region by that many elements (offset = 1: one element past a 16-byte boundary).  Subclasses say what a guard is."""
    FILL = None
    DTYPE = None

    def __init__(self, shape, data=None, offset=0, dtype=None):
        dtype = dtype or self.DTYPE
        self.shape = tuple(int(s) for s in shape)
        self.n = int(np.prod(self.shape))
        self.lo = G + offset
        self.buf = torch.full((self.n + 2 * G + offset,), self.FILL, device=dev(), dtype=dtype)
        self.t = self.buf[self.lo:self.lo + self.n].view(self.shape)
        if data is not None:
            self.t.copy_(torch.as_tensor(np.ascontiguousarray(data)).to(dtype).view(self.shape))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool(self.is_fill(self.buf[:self.lo]).all()) and bool(self.is_fill(self.buf[self.lo + self.n:]).all())

    def _fetch(self, what):
        torch.cuda.synchronize()
        assert self.guards_intact(), f"{what}: guard band overwritten"
        return self.t.cpu().numpy()


class Buf(_Guarded):
    """Floats (float32 unless `dtype` says float64) between NaN guards; outputs are NaN-poisoned."""
    FILL, DTYPE, is_fill = float("nan"), torch.float32, staticmethod(torch.isnan)

    def get(self, what, finite=True):
        out = self._fetch(what)
        if finite:
            assert bool(torch.isfinite(self.t).all()), f"{what}: NaN poison (or inf) left in the output"
        return out


class IntBuf(_Guarded):
    """Integers (int32 unless `dtype` says int64) between guards of SENTINEL; outputs hold SENTINEL as poison."""
    FILL, DTYPE, is_fill = SENTINEL, torch.int32, staticmethod(lambda t: t == SENTINEL)

    def get(self, what, written=True):
        out = self._fetch(what)
        if written:
            assert not bool((self.t == SENTINEL).any()), f"{what}: sentinel poison left in the output"
        return out


class Workspace:
    """Exactly `nbytes` bytes, 256-byte aligned, between guards of WS_GUARD bytes; `fill(pattern)` writes one byte value
    over the whole allocation (guards included), `guards_intact()` compares the guards with it byte for byte."""

    def __init__(self, nbytes, pattern=0xFF):
        self.nbytes = int(nbytes)
        self.buf = torch.empty((self.nbytes + 2 * WS_GUARD + 256,), device=dev(), dtype=torch.uint8)
        self.lo = WS_GUARD + (-(self.buf.data_ptr() + WS_GUARD)) % 256
        self.t = self.buf[self.lo:self.lo + self.nbytes]
        assert self.ptr % 256 == 0, "workspace not 256-byte aligned"
        assert self.lo >= WS_GUARD and self.buf.numel() - (self.lo + self.nbytes) >= WS_GUARD
        self.fill(pattern)

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.lo          # (a zero-length slice has no data_ptr of its own)

    def fill(self, pattern):
        self.pattern = int(pattern)
        self.buf.fill_(self.pattern)

    def guards_intact(self):
        return bool((self.buf[:self.lo] == self.pattern).all()) and bool((self.buf[self.lo + self.nbytes:] == self.pattern).all())

    def check(self, what):
        torch.cuda.synchronize()
        assert self.guards_intact(), f"{what}: workspace guard band overwritten ({self.nbytes} bytes advertised)"
