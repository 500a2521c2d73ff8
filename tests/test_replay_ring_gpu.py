"""The replay ring's entry points called directly against the numpy ring model (tests/ring_ref.py),
bit for bit on integer views: aac_replay_push_at (LDS-assembled rows, float4 and scalar store paths,
ragged last workgroup, ring wrap inside a workgroup, uint8 fields, zeroed row tail), aac_replay_push
(position from device meta, row tail untouched), aac_replay_gather / _gather_strided, and the float64
aac_uam_push_io / aac_uam_gather.  The ring is an arena region (ld = row_width): rows never pushed, pad
columns that a kernel must leave, and both guards keep the canary."""
import ctypes

import numpy as np
import pytest
import torch

from tests.arena import CANARY_BITS, Arena
from tests.ring_ref import RingModel

pytestmark = pytest.mark.gpu
DEV = "cuda"
vp = ctypes.c_void_p

# field tables: (widths, dtypes 0 = fp32 / 1 = uint8)
T4 = ([3, 1, 5, 2], [0, 1, 0, 1])                                                  # 11 data columns, odd widths
T16 = ([1, 2, 3, 1, 4, 1, 1, 5, 2, 1, 3, 1, 7, 1, 2, 1], [0, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0])   # 36, 16 fields
T1 = ([1], [0])
TWIDE = ([4099, 1001], [0, 1])                                                      # 5100: 3 transitions per workgroup
# (table, row_width): row_width % 4 == 0 -> float4 stores, else scalar; == data width or padded
PUSH_CASES = [(T4, 11), (T4, 12), (T4, 13), (T4, 16), (T16, 36), (T16, 37), (T16, 40), (T1, 1), (T1, 4), (T1, 2),
              (TWIDE, 5100), (TWIDE, 5101)]


def _pt(rw):
    """Transitions per workgroup: aac_replay_push_at's PT = max(1, min(4, 65536 / (4 row_width)))."""
    return max(1, min(4, 65536 // (4 * rw)))


def _sources(widths, dtypes, E, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for w, d in zip(widths, dtypes):
        if d == 1:
            out.append(torch.randint(0, 256, (E, w), dtype=torch.uint8, generator=g))
        else:
            out.append(torch.randn(E, w, generator=g))
    return out


def _push_sizes(cap, PT):
    """E = 1, PT - 1, PT, PT + 1, a ragged last workgroup, a push that wraps, E = cap (size saturates)."""
    sizes = [1] + [e for e in (PT - 1, PT, PT + 1) if e > 1] + [5 * PT + PT // 2 + 1, cap // 2, cap]
    return sizes


def _ring_bits(ring):
    return ring.get().numpy().view(np.int32)


@pytest.mark.parametrize("at", [True, False], ids=["push_at", "push"])
@pytest.mark.parametrize("table,rw", PUSH_CASES, ids=[f"{len(t[0])}f-rw{rw}" for t, rw in PUSH_CASES])
def test_replay_push_sequences(native_lib, table, rw, at):
    """A sequence of pushes into a canary ring of cap = 61 rows (41 for the wide rows), the whole region
    compared with the model after every push, meta = [(pos + E) % cap, min(size + E, cap)].
    push_at zero-fills the padded row tail; push leaves it (canary here)."""
    from multi_agent_aac_amd import ops
    widths, dtypes = table
    assert sum(widths) <= rw
    PT = _pt(rw)
    assert PT == (3 if rw > 4096 else 4)
    cap = 41 if rw > 4096 else 61
    ar = Arena(cap * rw + 64, torch.float32, DEV, max_ld=rw)
    ring = ar.take(cap, rw, name="ring")
    rv = ring.view
    assert rv.is_contiguous() and rv.data_ptr() == ring.ptr and ring.ptr % 16 == 0
    model = RingModel(cap, rw)
    meta = torch.zeros(2, dtype=torch.int64, device=DEV)
    wrapped = ragged = False
    for k, E in enumerate(_push_sizes(cap, PT)):
        srcs = _sources(widths, dtypes, E, 31 * rw + k)
        dsrc = [s.to(DEV).contiguous() for s in srcs]
        wrapped |= model.wraps_inside_group(E, PT)
        ragged |= E % PT != 0 and E > PT
        ar.inside(ring.ptr, cap * rw, "ring")
        if at:
            ops.replay_push_at(rv, meta, model.pos, model.size, dsrc, widths, dtypes, E)
        else:
            assert meta.cpu().tolist() == model.meta          # the launch reads its position here
            ops.replay_push(rv, meta, dsrc, widths, dtypes, E)
        model.push([s.numpy() for s in srcs], widths, zero_pad=at)
        ar.check(writable=[ring], all_written=False)
        assert np.array_equal(_ring_bits(ring), model.bits), (k, E)
        assert meta.cpu().tolist() == model.meta, (k, E)
    assert wrapped and ragged and model.size == cap
    pad = model.bits[:, sum(widths):]
    if at:
        assert (pad == 0).all()                               # +0.0 bits in every pushed row (all rows by now)
    else:
        assert (pad == CANARY_BITS[torch.float32]).all()


def test_replay_push_rejects_bad_arguments(native_lib):
    """The launchers' argument checks (no launch): E > capacity, a misaligned ring, pos / size out of range."""
    from multi_agent_aac_amd import ops
    ring = torch.zeros(8, 8, device=DEV)
    meta = torch.zeros(2, dtype=torch.int64, device=DEV)
    src = [torch.zeros(9, 4, device=DEV)]
    with pytest.raises(RuntimeError):
        ops.replay_push_at(ring, meta, 0, 0, src, [4], [0], 9)
    with pytest.raises(RuntimeError):
        ops.replay_push_at(ring, meta, 8, 0, src, [4], [0], 2)
    with pytest.raises(RuntimeError):
        ops.replay_push_at(ring.view(-1)[1:57].view(7, 8), meta, 0, 0, src, [4], [0], 2)
    with pytest.raises(RuntimeError):
        ops.replay_push_at(ring, meta, 0, 0, src, [9], [0], 2)
    torch.cuda.synchronize()
    assert float(ring.abs().sum()) == 0 and meta.cpu().tolist() == [0, 0]


def _filled_ring(ar, cap, rw, seed):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(cap, rw, generator=g)                  # pad columns too: they must never arrive
    ring = ar.take(cap, rw, data=data, name="ring")
    model = RingModel(cap, rw)
    model.bits[:] = data.numpy().view(np.int32)
    return ring, model


def _indices(B, cap, seed):
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, cap, (B,), dtype=torch.int32, generator=g)
    if B >= 4:
        idx[0], idx[1], idx[2], idx[B - 1] = cap - 1, 0, idx[3], 0      # both ends and repeats
    else:
        idx[0] = cap - 1
    return idx


@pytest.mark.parametrize("B", [1, 33, 256])
@pytest.mark.parametrize("table,rw", [(T4, 11), (T4, 16), (T16, 40)], ids=["4f-rw11", "4f-rw16", "16f-rw40"])
def test_replay_gather(native_lib, table, rw, B):
    """aac_replay_gather: contiguous [B][w] destinations in the arena, indices with row 0, row cap - 1
    and repeats; aac_replay_gather_strided: destination rows ld > w apart, a second destination set, and a
    field split into chunks."""
    from multi_agent_aac_amd import fused, ops
    widths = table[0]
    cap = 97
    ar = Arena(cap * rw + 8 * sum(B * (w + 8) + 64 for w in widths), torch.float32, DEV,
               max_ld=max(rw, max(widths) + 3))
    ring, model = _filled_ring(ar, cap, rw, rw + B)
    idx = _indices(B, cap, B)
    idx_d = idx.to(DEV)
    want = model.gather(idx.numpy(), widths)
    # contiguous destinations
    dst = [ar.take(B, w, name=f"dst {f}") for f, w in enumerate(widths)]
    for d, w in zip(dst, widths):
        ar.inside(d.ptr, B * w, d.name)
    ops.replay_gather(ring.view, idx_d, [d.view for d in dst], widths)
    ar.check(writable=dst)
    for d, w_ in zip(dst, want):
        assert np.array_equal(d.get().numpy().view(np.int32), w_), d.name
    ar.freeze(dst)
    # strided destinations (chunk = the field, rows ld apart), two sets
    s1 = [ar.take(B, w, ld=w + 3, name=f"strided {f}") for f, w in enumerate(widths)]
    s2 = [ar.take(B, w, ld=w + 3, name=f"strided second {f}") for f, w in enumerate(widths)]
    for d, w in zip(s1 + s2, widths + widths):
        ar.inside_mat(d.ptr, B, w, w + 3, d.name)
    fused.gather_strided(ring.view, idx_d, [d.ptr for d in s1], widths, widths, [w + 3 for w in widths],
                         dsts2=[d.ptr for d in s2])
    ar.check(writable=s1 + s2)
    for a, b, w_ in zip(s1, s2, want):
        assert np.array_equal(a.get().numpy().view(np.int32), w_), a.name
        assert np.array_equal(b.get().numpy().view(np.int32), w_), b.name
    ar.freeze(s1 + s2)
    # one field in chunks of `ch` columns landing `ds` apart (the per-agent form)
    comp = [i for i, x in enumerate(widths) if x >= 4 and x % 2 == 0]
    f = comp[0] if comp else int(np.argmax(widths))          # an even width in chunks of 2, else the widest in 1s
    w = widths[f]
    ch = 2 if comp else 1
    ds = ch + 3
    nch = w // ch
    assert nch > 1
    chunked = ar.take(B * nch, ch, ld=ds, name="chunked")
    rest = [ar.take(B, x, name=f"rest {i}") for i, x in enumerate(widths)]
    ptrs = [d.ptr for d in rest]
    ptrs[f] = chunked.ptr
    chunks = list(widths)
    chunks[f] = ch
    strides = list(widths)
    strides[f] = ds
    ar.inside_mat(chunked.ptr, B * nch, ch, ds, "chunked")
    fused.gather_strided(ring.view, idx_d, ptrs, widths, chunks, strides)
    outs = [chunked] + [d for i, d in enumerate(rest) if i != f]
    ar.check(writable=outs)
    assert np.array_equal(chunked.get().numpy().view(np.int32).reshape(B, w), want[f])
    for i, d in enumerate(rest):
        if i != f:
            assert np.array_equal(d.get().numpy().view(np.int32), want[i]), d.name


# ============================================================================ float64 UAM ring
def test_uam_push_io_and_gather(native_lib):
    """aac_uam_push_io into a float64 arena ring of 150 rows, 70 transitions a push (a ragged second
    workgroup), the two position words alternating over two wraps, done as uint8 and as float64; then
    aac_uam_gather: rows, xc = [own | a], xt = own', xp = own against slices of the model's rows, the two
    pad columns of the 9-wide xt / xp rows unchanged (they are row gaps of arena regions)."""
    from multi_agent_aac_amd import fused
    from multi_agent_aac_amd import uam_learner as UL
    L = UL._learn_lib()
    cap, M, ROW = 150, 70, 54
    assert UL.ROW == ROW
    widths = [7, 18, 2, 1, 1, 7, 18]
    ar = Arena(cap * ROW + 4 * (256 * ROW + 64) + 64, torch.float64, DEV, max_ld=ROW)
    ring = ar.take(cap, ROW, name="ring")
    model = RingModel(cap, ROW, np.float64)
    meta = torch.zeros(2, dtype=torch.int64, device=DEV)
    words = torch.zeros(2, dtype=torch.int64, device=DEV)
    wraps = 0
    for k in range(5):
        g = torch.Generator().manual_seed(k)
        srcs = [torch.randn(M, w, dtype=torch.float64, generator=g) for w in widths]
        u8 = k % 2 == 0
        srcs[4] = torch.randint(0, 2, (M, 1), generator=g).to(torch.uint8 if u8 else torch.float64)
        d = [s.to(DEV).contiguous() for s in srcs]
        pin, pout = words[k % 2:k % 2 + 1], words[1 - k % 2:2 - k % 2]
        assert int(pin.item()) == model.pos
        wraps += model.pos + M >= cap
        ar.inside(ring.ptr, cap * ROW, "ring")
        UL._ok(L.aac_uam_push_io(vp(ring.ptr), cap, M, *[vp(t.data_ptr()) for t in d[:5]], int(u8),
                                 vp(d[5].data_ptr()), vp(d[6].data_ptr()), vp(meta.data_ptr()),
                                 vp(pin.data_ptr()), vp(pout.data_ptr()), fused._stream()), "aac_uam_push_io")
        model.push([s.numpy() for s in srcs], widths, zero_pad=False)
        ar.check(writable=[ring], all_written=False)
        assert np.array_equal(ring.get().numpy().view(np.int64), model.bits), k
        assert meta.cpu().tolist() == model.meta and int(pout.item()) == model.pos, k
    assert wraps == 2 and model.size == cap
    ar.freeze([ring])
    for B in (1, 33, 256):
        idx = _indices(B, cap, B)
        rows = ar.take(B, ROW, name=f"rows {B}")
        xc = ar.take(B, 9, name=f"xc {B}")
        xt = ar.take(B, 7, ld=9, name=f"xt {B}")
        xp = ar.take(B, 7, ld=9, name=f"xp {B}")
        for r in (rows, xc, xt, xp):
            ar.inside_mat(r.ptr, B, r.cols, r.ld, r.name)
        idx_d = idx.to(DEV)
        UL._ok(L.aac_uam_gather(vp(ring.ptr), vp(idx_d.data_ptr()), B, vp(rows.ptr), vp(xc.ptr), vp(xt.ptr),
                                vp(xp.ptr), fused._stream()), "aac_uam_gather")
        ar.check(writable=[rows, xc, xt, xp])
        ar.freeze([rows, xc, xt, xp])
        want = model.bits[idx.numpy().astype(np.int64)]
        bits = lambda r: r.get().numpy().view(np.int64)      # noqa: E731
        assert np.array_equal(bits(rows), want)
        assert np.array_equal(bits(xc), np.concatenate([want[:, 0:7], want[:, 25:27]], 1))
        assert np.array_equal(bits(xt), want[:, 29:36])
        assert np.array_equal(bits(xp), want[:, 0:7])
