"""A numpy model of the replay ring (include/aac_learn.h: aac_replay_push / _push_at / _gather),
kept as bits: a ``cap x row_width`` array that starts as the arena's canary, plus ``[pos, size]``.

    push     rows (pos + e) % cap, e < E, field f of transition e at columns offset[f] .. + width[f]
             (uint8 sources converted to float32); ``zero_pad``: the padded row tail row_width - sum(widths)
             is +0.0 (aac_replay_push_at) or left as it was (aac_replay_push);
             then [pos, size] = [(pos + E) % cap, min(size + E, cap)]
    gather   field f of ring rows idx -> [B][width[f]]

tests/test_ring_ref_cpu.py pins it against a scalar loop.  Works for float32 (int32 bits) and float64
(int64 bits) rings.
"""
import numpy as np
import torch

from tests.arena import CANARY_BITS

_BITS = {np.dtype(np.float32): (np.int32, CANARY_BITS[torch.float32]),
         np.dtype(np.float64): (np.int64, CANARY_BITS[torch.float64])}


class RingModel:
    def __init__(self, cap, row_width, dtype=np.float32):
        self.cap, self.rw, self.dtype = int(cap), int(row_width), np.dtype(dtype)
        self.idt, canary = _BITS[self.dtype]
        self.bits = np.full((self.cap, self.rw), canary, dtype=self.idt)
        self.pos, self.size = 0, 0

    @property
    def meta(self):
        return [self.pos, self.size]

    def push(self, srcs, widths, zero_pad):
        """srcs[f]: array [E][widths[f]] (any leading shape with E first), float or uint8."""
        E = len(srcs[0])
        assert 1 <= E <= self.cap and sum(widths) <= self.rw
        rows = (self.pos + np.arange(E)) % self.cap
        off = 0
        for s, w in zip(srcs, widths):
            v = np.asarray(s).reshape(E, w).astype(self.dtype)
            self.bits[rows, off:off + w] = v.view(self.idt)
            off += w
        if zero_pad:
            self.bits[rows, off:] = 0                      # +0.0
        self.pos = (self.pos + E) % self.cap
        self.size = min(self.size + E, self.cap)
        return rows

    def gather(self, idx, widths):
        """[bits of ring[idx][field f]] for every field."""
        idx = np.asarray(idx).astype(np.int64)
        out, off = [], 0
        for w in widths:
            out.append(self.bits[idx, off:off + w].copy())
            off += w
        return out

    def wraps_inside_group(self, E, group):
        """Whether a push of E rows from the present position wraps between two transitions of one
        ``group``-transition workgroup (the kernel's e0 = workgroup x group, rows (pos + e0 + r) % cap)."""
        k = self.cap - self.pos                            # the first transition that lands on row 0
        return 0 < k < E and k % group != 0
