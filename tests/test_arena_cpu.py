"""The poisoned arena (tests/arena.py) can fail: on CPU tensors, each kind of stray write that the
GPU layout tests rely on it to see is made by hand, one at a time, and ``check`` must name it.  This
is the proof that the harness detects what it claims; no deliberately broken kernel ever runs."""
import pytest
import torch

from tests.arena import CANARY_BITS, Arena

DTYPES = [torch.float32, torch.float64]


def _setup(dtype):
    """An input A (5 x 3, ld 7, shifted by one element), a container of two adjacent 4 x 6 column
    blocks (ld 16) and a bias; block0 is the launch's output."""
    ar = Arena(400, dtype, "cpu", max_ld=16)
    a = torch.arange(15, dtype=dtype).reshape(5, 3) - 7
    A = ar.take(5, 3, ld=7, misalign=1, name="A", data=a)
    f = ar.take(4, 12, ld=16, name="f", payload=False)
    c0 = f.sub(0, 0, 4, 6, name="block0")
    c1 = f.sub(0, 6, 4, 6, name="block1", data=torch.ones(4, 6, dtype=dtype))
    bias = ar.vec(6, name="bias", data=torch.full((6,), -0.0, dtype=dtype))
    return ar, A, f, c0, c1, bias


def _write_result(c0):
    c0.view.copy_(torch.arange(24, dtype=c0.arena.dtype).reshape(4, 6))


@pytest.mark.parametrize("dtype", DTYPES)
def test_clean_launch_passes_and_layout_is_as_asked(dtype):
    ar, A, f, c0, c1, bias = _setup(dtype)
    q = ar.q
    assert A.base % q == 1 and f.base % q == 0 and bias.base % q == 0
    assert A.ptr == ar.buf.data_ptr() + A.base * ar.itemsize and c1.ptr == f.ptr + 6 * ar.itemsize
    assert c0.at(2, 3) == f.ptr + (2 * 16 + 3) * ar.itemsize
    assert torch.equal(A.get(), torch.arange(15, dtype=dtype).reshape(5, 3) - 7)
    # the row gaps of an input, and everything unwritten, are the canary NaN
    raw = ar.buf.view(ar.idt)
    assert int(raw[A.base + 3]) == CANARY_BITS[dtype] and bool(torch.isnan(ar.buf[A.base + 3]))
    assert bool(torch.isnan(c0.view).all())
    # a 64-row tile at the largest ld fits in each guard
    assert ar.guard >= 64 * 16 and ar.regions[0].base >= ar.guard
    assert ar.cursor <= ar.guard + ar.capacity
    with pytest.raises(AssertionError, match="still holds the canary"):
        ar.check(writable=[c0])                        # nothing written yet
    ar.check(writable=[c0], all_written=False)
    _write_result(c0)
    ar.check(writable=[c0])
    # -0.0 inputs are kept as bits: +0.0 over them is a modification
    bias.view[0, 2] = 0.0
    with pytest.raises(AssertionError, match=r"input payload modified .*\(row 0, col 2\) of region 'bias'"):
        ar.check(writable=[c0])


STRAYS = {
    # name: (where to write, expected message)
    "row_gap": (lambda ar, A, f, c0, c1: c0.base + 1 * 16 + 13, r"canary modified .*\(row 1, col 7\) of region 'block1'"),
    "column_past_n": (lambda ar, A, f, c0, c1: A.base + 2 * 7 + 3, r"canary modified .*\(row 2, col 3\) of region 'A'"),
    "neighbour_first_column": (lambda ar, A, f, c0, c1: c0.base + 3 * 16 + 6,
                               r"input payload modified .*\(row 3, col 0\) of region 'block1'"),
    "front_guard": (lambda ar, A, f, c0, c1: ar.guard - 5, r"front guard modified .*\(row -1, col 1\) of region 'A'"),
    "back_guard": (lambda ar, A, f, c0, c1: ar.guard + ar.capacity + 9, r"back guard modified"),
    "modified_input": (lambda ar, A, f, c0, c1: A.base + 4 * 7 + 2, r"input payload modified .*\(row 4, col 2\) of region 'A'"),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", list(STRAYS))
def test_each_stray_write_is_detected(dtype, kind):
    ar, A, f, c0, c1, bias = _setup(dtype)
    _write_result(c0)
    ar.check(writable=[c0])
    where, msg = STRAYS[kind]
    ar.buf[where(ar, A, f, c0, c1)] = 3.5
    with pytest.raises(AssertionError, match=msg):
        ar.check(writable=[c0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_second_output_must_be_declared(dtype):
    """A write into a payload region that the test did not declare writable is a failure even
    though the region is an output of some other launch."""
    ar, A, f, c0, c1, bias = _setup(dtype)
    _write_result(c0)
    c1.view[1, 1] = 2.0
    with pytest.raises(AssertionError, match=r"\(row 1, col 1\) of region 'block1'"):
        ar.check(writable=[c0])
    ar.check(writable=[c0, c1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_canary_valued_write_is_invisible(dtype):
    """The limitation, pinned: a stray store of the canary's own bit pattern over a canary cannot
    be told from no store at all (nor can a stray read that is discarded).  Every other NaN
    payload, and every finite value, is seen."""
    ar, A, f, c0, c1, bias = _setup(dtype)
    _write_result(c0)
    gap = c0.base + 2 * 16 + 14
    ar.buf.view(ar.idt)[gap] = CANARY_BITS[dtype]
    ar.check(writable=[c0])                               # passes: undetectable
    ar.buf[gap] = float("nan")                            # the default NaN has other bits
    with pytest.raises(AssertionError, match="canary modified"):
        ar.check(writable=[c0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_finite_canary_operand_and_extent_asserts(dtype):
    ar = Arena(300, dtype, "cpu", max_ld=12)
    B = ar.take(3, 5, ld=9, name="B", data=torch.zeros(3, 5, dtype=dtype), canary=1e30)
    assert float(ar.buf[B.base + 6]) == pytest.approx(1e30, rel=1e-6) and float(ar.buf[B.base + 9]) == 0.0
    ar.check()
    ar.buf[B.base + 6] = 0.0
    with pytest.raises(AssertionError, match=r"\(row 0, col 6\) of region 'B'"):
        ar.check()
    # extents handed to a kernel must lie between the guards
    ar.inside_mat(B.ptr, 3, 5, 9)
    with pytest.raises(AssertionError, match="leaves the arena"):
        ar.inside_mat(B.ptr, 3, 5, 200)
    with pytest.raises(AssertionError, match="leaves the arena"):
        ar.inside(B.ptr - 64 * ar.itemsize, 4)
    with pytest.raises(AssertionError, match="arena too small"):
        ar.take(40, 12)
