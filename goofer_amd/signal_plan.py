"""What the plans of the stages over finished audio share (phrase, bus, rate, eq, compress, loudness, limit): one blob per plan
for one upload, cut into typed views on the device; the signals' lengths as a CSR with the refusals every stage makes; the
capacity protocol of the library's host planners (include/goofer_hip.h); and the cover table of the two mixers."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np


class BlobPlan:
    """Base of a plan dataclass: ``blob`` holds the arrays named by ``BLOB`` back to back, in that order, then ``PAD`` zero
    bytes, for one upload."""
    BLOB = ()
    PAD = 0

    def __post_init__(self):
        parts = [np.ascontiguousarray(getattr(self, k)).view(np.uint8).ravel() for k in self.BLOB]
        self.blob = np.concatenate(parts + [np.zeros(self.PAD, dtype=np.uint8)])
        self._dev = {}

    def _tables(self, ctx):
        """the arrays of ``BLOB`` on ``ctx``'s device, then the blob they are views of: uploaded on first use, kept per device.
        A view has its array's dtype (bytes where torch has none) and is flat; the last one runs to the blob's end."""
        import torch
        hit = self._dev.get(ctx.device)
        if hit is None:
            d = ctx.tensor(self.blob)
            views, at = [], 0
            for k in self.BLOB:
                a = getattr(self, k)
                v = d[at:] if k == self.BLOB[-1] else d[at:at + a.nbytes]
                dt = getattr(torch, a.dtype.name, None)
                views.append(v if dt is None else v.view(dt))
                at += a.nbytes
            hit = self._dev[ctx.device] = (*views, d)
        return hit

    def device_tables(self, ctx):
        """The arrays of ``BLOB``, in that order, on ``ctx``'s device: views of the blob, uploaded on first use."""
        return self._tables(ctx)[:len(self.BLOB)]


@dataclass
class CoverPlan(BlobPlan):
    """Base of the plan of a gather-sum mix (phrase, bus): ``n`` records, the ``total_out`` samples of the time line they are
    summed onto and its rate ``sr``; the plan adds its records and the cover table (``cover``), which ``BLOB`` names, and the blob
    ends in a pad word (no empty tensor on the device: an empty table still has an address)."""
    n: int
    total_out: int
    sr: int
    PAD = 4


class SignalPlan(BlobPlan):
    """Base of the plan of a ragged batch of signals lying back to back: ``in_off``, their int64 CSR ``[n + 1]``, and where the
    stage works by tiles ``tiles`` (int32 [n_tiles, 2]: signal, tile of the signal)."""

    @property
    def total(self) -> int:
        return int(self.in_off[-1])

    @property
    def n_tiles(self) -> int:
        return len(self.tiles)


def offsets(who, lengths, *rates):
    """The CSR ``in_off`` (int64 [n + 1]) of signals of ``lengths`` samples.  Raises ValueError, in ``who``'s name, for a negative
    length and for one of ``rates`` that is not a whole number of Hz."""
    lengths = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
    if lengths.size and lengths.min() < 0:
        raise ValueError("%s: a negative length" % who)
    if any(int(sr) != sr for sr in rates):
        raise ValueError("%s: the sample rate is a whole number of Hz" % who)
    in_off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=in_off[1:])
    return in_off


def cap(a):
    """an output array as a host planner takes it: (pointer, or NULL for an empty one; capacity in rows)"""
    return (a.ctypes.data if a.size else None), len(a)


def fit(call, bufs, grown, refused):
    """The capacity protocol of the host planners: ``call(*bufs)``; where it answers 1 the arrays are too short, ``grown()``
    makes them of the sizes the call reported and it is called once more.  Returns the arrays the call filled.  Anything but 0
    raises ValueError(refused(rc))."""
    rc = call(*bufs)
    if rc == 1:
        bufs = grown()
        rc = call(*bufs)
    if rc != 0:
        raise ValueError(refused(rc))
    return bufs


def cover(planner, records, extra, total_out, tile, refused):
    """The cover table of a gather-sum mix by one of the library's planners (goofer_host_phrase_plan, goofer_host_bus_plan):
    ``planner(records, *extra, n, total_out, tile_off, tile_list, cap, need)`` checks the ``records`` (a contiguous array) and
    lists per tile of ``tile`` samples the records that reach it.  Returns (tile_off int64 [tiles + 1], tile_list int32).
    Raises ValueError(refused(rc)) for what the planner refuses."""
    total_out = int(total_out)
    tile_off = np.zeros((total_out + tile - 1) // tile + 1 if total_out > 0 else 1, dtype=np.int64)
    need = C.c_int64(0)
    tile_list, = fit(lambda tile_list: planner(records.ctypes.data if len(records) else None, *extra, len(records), total_out,
                                               tile_off.ctypes.data, *cap(tile_list), C.byref(need)),
                     (np.zeros(max(len(records), 1), dtype=np.int32),), lambda: (np.zeros(int(need.value), dtype=np.int32),), refused)
    return tile_off, tile_list[:int(need.value)]
