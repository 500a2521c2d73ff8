"""The numpy ring model behind tests/test_replay_ring_gpu.py, pinned without a GPU against a scalar
loop over transitions and columns, and through a CPU arena region holding the ring."""
import numpy as np
import pytest
import torch

from tests.arena import CANARY_BITS, Arena
from tests.ring_ref import RingModel

CAN32 = CANARY_BITS[torch.float32]


def _scalar_ring(cap, rw, pushes, widths, zero_pad):
    """Row by row, column by column; floats kept as Python / numpy scalars (None = never written)."""
    ring = [[None] * rw for _ in range(cap)]
    pos = size = 0
    for srcs in pushes:
        E = len(srcs[0])
        for e in range(E):
            row = (pos + e) % cap
            c = 0
            for s, w in zip(srcs, widths):
                for j in range(w):
                    ring[row][c] = np.float32(s[e][j])
                    c += 1
            if zero_pad:
                for j in range(c, rw):
                    ring[row][j] = np.float32(0.0)
        pos = (pos + E) % cap
        size = min(size + E, cap)
    return ring, pos, size


@pytest.mark.parametrize("zero_pad", [True, False])
@pytest.mark.parametrize("rw", [11, 12, 16])
def test_ring_model_matches_scalar_loop(rw, zero_pad):
    cap, widths = 13, [3, 1, 5, 2]
    rng = np.random.default_rng(rw)
    model = RingModel(cap, rw)
    pushes = []
    wrapped = False
    for E in (1, 3, 4, 5, 7, 13):
        srcs = [rng.standard_normal((E, 3)).astype(np.float32), rng.integers(0, 256, (E, 1)).astype(np.uint8),
                rng.standard_normal((E, 5)).astype(np.float32), rng.integers(0, 2, (E, 2)).astype(np.uint8)]
        wrapped |= model.wraps_inside_group(E, 4)
        rows = model.push(srcs, widths, zero_pad)
        assert list(rows) == [(model.pos - E + e) % cap for e in range(E)]
        pushes.append(srcs)
        ring, pos, size = _scalar_ring(cap, rw, pushes, widths, zero_pad)
        assert model.meta == [pos, size]
        for r in range(cap):
            for c in range(rw):
                want = CAN32 if ring[r][c] is None else int(np.float32(ring[r][c]).view(np.int32))
                assert int(model.bits[r, c]) == want, (E, r, c)
    assert wrapped and model.size == cap
    idx = [0, cap - 1, 5, 5, 0]
    got = model.gather(idx, widths)
    off = 0
    for f, w in enumerate(widths):
        for b, i in enumerate(idx):
            assert list(got[f][b]) == list(model.bits[i, off:off + w])
        off += w
    assert [g.shape for g in got] == [(len(idx), w) for w in widths]        # no pad column reaches a field


def test_wraps_inside_group():
    m = RingModel(10, 4)
    m.pos = 7
    assert m.wraps_inside_group(8, 4)          # transition 3 lands on row 0: inside the first group of 4
    m.pos = 6
    assert not m.wraps_inside_group(8, 4)      # transition 4: the group boundary
    assert not m.wraps_inside_group(4, 4)      # no wrap at all (rows 6 .. 9)
    assert m.wraps_inside_group(8, 3)


def test_ring_model_agrees_with_a_cpu_arena_region():
    """The model's bits against an arena region written the same way on the CPU: rows never pushed and
    (without zero_pad) pad columns keep the canary in both, and Arena.check sees a stray row."""
    cap, rw, widths = 9, 8, [5, 2]
    ar = Arena(cap * rw + 64, torch.float32, "cpu", max_ld=rw)
    ring = ar.take(cap, rw, name="ring")
    model = RingModel(cap, rw)
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(4, 5, generator=g), torch.randn(4, 2, generator=g)
    rows = model.push([a.numpy(), b.numpy()], widths, zero_pad=False)
    v = ring.view
    v[torch.as_tensor(rows), :5] = a
    v[torch.as_tensor(rows), 5:7] = b
    ar.check(writable=[ring], all_written=False)
    assert np.array_equal(ring.get().numpy().view(np.int32), model.bits)
    assert (model.bits[rows, 7] == CAN32).all() and (model.bits[4:] == CAN32).all()
    ar.buf[ring.base - 1] = 0.0                # one element in front of the ring
    with pytest.raises(AssertionError, match="modified"):
        ar.check(writable=[ring], all_written=False)
