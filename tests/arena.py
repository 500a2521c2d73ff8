"""A poisoned arena for kernel tests: every operand of a launch is carved from ONE allocation that
is pre-filled with a canary NaN bit pattern, so that what a kernel must not touch can be checked.

    ar = Arena(20000, torch.float32, "cuda", max_ld=200)
    A = ar.take(37, 24, ld=28, data=a)                  # input: payload = a, the row gaps stay canary
    f = ar.take(37, 384, ld=388, payload=False)         # a container: nothing in it is payload yet
    C = f.sub(0, 128, 37, 128)                          # output: a column block of the container
    ar.launch(fused.GemmLaunch([fused.prob(A.ptr, ..., C.ptr, ...)]))   # extents asserted, then launched
    torch.cuda.synchronize()
    ar.check(writable=[C])

What the canary proves: after ``check`` every element of the arena that is not payload of a region
declared writable has the canary's bits -- row gaps, the columns past N, neighbouring blocks, the
guards in front of and behind all regions -- and every input payload has the bits it was filled
with; a kernel that folds a pad element into a result produces NaN there, which the value
comparison of the test sees.  What it cannot prove: a stray write of the canary's own value over a
canary is invisible (tests/test_arena_cpu.py pins this), and so is a stray read whose value is
discarded.  The guards only keep a stray store in owned memory where it is no farther off than one
64-row tile at the largest leading dimension; nothing here makes a wild store safe.

Works on CPU and GPU tensors, float32 and float64.  Checks compare the integer view, so -0.0 and
NaN payloads count as bits.
"""
import contextlib

import torch

# one quiet-NaN payload per dtype (sign 0, quiet bit set, a recognisable mantissa)
CANARY_BITS = {torch.float32: 0x7FC5A5A5, torch.float64: 0x7FF8A5A5A5A5A5A5}
_INT = {torch.float32: torch.int32, torch.float64: torch.int64}
GAP = 32            # canary elements between two carved regions


class Region:
    """``rows`` x ``cols`` elements at element offset ``base`` of the arena, row stride ``ld``."""

    def __init__(self, arena, name, base, rows, cols, ld, payload):
        self.arena, self.name, self.base, self.rows, self.cols, self.ld = arena, name, base, rows, cols, ld
        self.payload = payload

    @property
    def span(self):
        return (self.rows - 1) * self.ld + self.cols

    @property
    def ptr(self):
        """Device address of element (0, 0): what ``fused.ptr`` / ``p64`` give for a tensor."""
        return self.arena.buf.data_ptr() + self.base * self.arena.itemsize

    def at(self, r, c=0):
        """Device address of element (r, c)."""
        return self.ptr + (r * self.ld + c) * self.arena.itemsize

    @property
    def view(self):
        return torch.as_strided(self.arena.buf, (self.rows, self.cols), (self.ld, 1), self.base)

    def _strided(self, flat):
        return torch.as_strided(flat, (self.rows, self.cols), (self.ld, 1), self.base)

    def fill(self, data):
        """Make ``data`` the region's input payload (and its snapshot for ``check``)."""
        data = torch.as_tensor(data, dtype=self.arena.dtype).reshape(self.rows, self.cols)
        self.view.copy_(data)
        self._strided(self.arena.expected).copy_(data.detach().cpu().contiguous().view(self.arena.idt))
        return self

    def sub(self, r0, c0, rows, cols, name=None, data=None):
        """A payload sub-block (rows r0 .. r0+rows, columns c0 .. c0+cols) of this region."""
        assert 0 <= r0 and r0 + rows <= self.rows and 0 <= c0 and c0 + cols <= self.cols and rows > 0 and cols > 0
        reg = Region(self.arena, name or f"{self.name}[{r0}:{r0 + rows},{c0}:{c0 + cols}]",
                     self.base + r0 * self.ld + c0, rows, cols, self.ld, True)
        self.arena.regions.append(reg)
        return reg if data is None else reg.fill(data)

    def carve(self, offset, rows, cols, ld=None, name=None, data=None):
        """A payload region of its own shape and ``ld`` at element ``offset`` of this region's span
        (a split-K copy, or a matrix inside a flat buffer)."""
        ld = cols if ld is None else ld
        reg = Region(self.arena, name or f"{self.name}+{offset}", self.base + offset, rows, cols, ld, True)
        assert offset >= 0 and offset + reg.span <= self.span and ld >= cols
        self.arena.regions.append(reg)
        return reg if data is None else reg.fill(data)

    def get(self):
        """The payload as a contiguous tensor on the CPU."""
        return self.view.detach().cpu().clone()


class Arena:
    """One allocation of ``capacity`` elements between two guards, all canary.  ``max_ld``: the
    largest leading dimension of any region; each guard holds 64 rows of it (a stray store of a
    whole 64-row tile before the first or past the last region stays inside the allocation)."""

    def __init__(self, capacity, dtype=torch.float32, device="cpu", max_ld=256):
        assert dtype in CANARY_BITS
        self.dtype, self.idt, self.device = dtype, _INT[dtype], device
        self.itemsize = 4 if dtype == torch.float32 else 8
        self.q = 16 // self.itemsize                       # elements per 16 bytes
        self.max_ld = max_ld
        self.guard = (64 * max_ld + 64 + self.q - 1) // self.q * self.q
        self.capacity = capacity
        self.n = 2 * self.guard + capacity
        self.canary = CANARY_BITS[dtype]                   # sign bit clear: fits the signed integer view
        self.buf = torch.empty(self.n, dtype=dtype, device=device)
        assert self.buf.data_ptr() % 16 == 0
        self.buf.view(self.idt).fill_(self.canary)
        self.expected = torch.full((self.n,), self.canary, dtype=self.idt)     # CPU image of what must not change
        self.cursor = self.guard
        self.regions = []

    # ------------------------------------------------------------------ carving
    def take(self, rows, cols, ld=None, misalign=0, name=None, data=None, payload=True, canary=None):
        """Carve ``rows`` x ``cols`` at a 16-B aligned base plus ``misalign`` elements, row stride
        ``ld`` (default cols).  ``payload=False`` carves a container whose payload regions are its
        ``sub`` blocks.  ``canary`` (a finite value, e.g. 1e30): the region's row gaps hold that value
        instead of the NaN, for an operand whose padding a kernel reads and discards by design."""
        ld = cols if ld is None else ld
        assert rows > 0 and cols > 0 and ld >= cols and (rows == 1 or ld <= self.max_ld) and 0 <= misalign < 16
        base = (self.cursor + self.q - 1) // self.q * self.q + misalign
        reg = Region(self, name or f"region{len(self.regions)}", base, rows, cols, ld, payload)
        assert base + reg.span + GAP <= self.guard + self.capacity, "arena too small"
        self.cursor = base + reg.span + GAP
        self.regions.append(reg)
        if canary is not None:
            fill = torch.full((reg.span,), canary, dtype=self.dtype)
            self.buf[base:base + reg.span] = fill.to(self.device)
            self.expected[base:base + reg.span] = fill.view(self.idt)
        return reg if data is None else reg.fill(data)

    def vec(self, n, misalign=0, name=None, data=None):
        """A one-row region of ``n`` elements (bias, dvec, a flat buffer)."""
        return self.take(1, n, misalign=misalign, name=name, data=data)

    # ------------------------------------------------------------------ before a launch
    def inside(self, ptr, span, what="extent"):
        """Assert that ``span`` elements from device address ``ptr`` lie between the guards."""
        if not ptr:
            return
        lo = self.buf.data_ptr() + self.guard * self.itemsize
        hi = self.buf.data_ptr() + (self.guard + self.capacity) * self.itemsize
        assert span > 0 and lo <= ptr and ptr + span * self.itemsize <= hi and (ptr - lo) % self.itemsize == 0, \
            f"{what}: [{ptr:#x}, +{span}) leaves the arena [{lo:#x}, {hi:#x})"

    def inside_mat(self, ptr, rows, cols, ld, what="matrix"):
        self.inside(ptr, (rows - 1) * ld + cols if ptr else 0, what)

    def inside_prob(self, p, i=0):
        """Every operand extent of one grouped-GEMM problem (GemmProb / Gemm64Prob) is in the arena."""
        nr, ks = p.N - p.ones, max(1, p.ksplit)
        w = f"product {i} "
        self.inside_mat(p.A, p.K if p.ta else p.M, p.M if p.ta else p.K, p.lda, w + "A")
        if nr > 0:
            self.inside_mat(p.B, nr if p.tb else p.K, p.K if p.tb else nr, p.ldb, w + "B")
        for s in range(ks):
            off = s * p.split_stride * self.itemsize
            if nr > 0:
                self.inside_mat(p.C + off, p.M, nr, p.ldc, w + f"C split {s}")
            if p.ones:
                self.inside(p.cextra + off, p.M, w + f"cextra split {s}")
        if p.bias:
            self.inside(p.bias, nr, w + "bias")
        if p.addend:
            self.inside_mat(p.addend, p.M, nr, p.ldadd, w + "addend")
        if p.mask:
            self.inside_mat(p.mask, p.M, nr, p.ldmask, w + "mask")
        if p.C2:
            self.inside_mat(p.C2, p.M, nr, p.ldc, w + "C2")
            self.inside(p.dvec, nr, w + "dvec")

    def launch(self, gemm_launch):
        """Assert the extents of a ``fused.GemmLaunch``'s products, then launch it."""
        for i in range(gemm_launch.n):
            self.inside_prob(gemm_launch.arr[i], i)
        gemm_launch()

    # ------------------------------------------------------------------ after a launch
    def _locate(self, idx):
        """(region, row, col) of flat element ``idx`` relative to the nearest carved payload region."""
        best = None
        for reg in self.regions:
            row, col = divmod(idx - reg.base, reg.ld)
            if 0 <= row < reg.rows:
                d = 0 if col < reg.cols else col - reg.cols + 1
            else:
                d = (1 << 40) + (reg.base - idx if idx < reg.base else idx - (reg.base + reg.span) + 1)
            d = 2 * d + (0 if reg.payload else 1)          # a payload block before its container
            if best is None or d < best[0]:
                best = (d, reg, row, col)
        return best[1:] if best else (None, 0, idx)

    def freeze(self, regions):
        """Outputs of a checked launch become inputs of the next: their present bits are the snapshot."""
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        cur = self.buf.view(self.idt).cpu()
        for reg in regions:
            reg._strided(self.expected).copy_(reg._strided(cur))

    def check(self, writable=(), all_written=True):
        """After the device has finished: everything outside the payload of the ``writable`` regions
        has the bits it had (canary, or an input's snapshot).  ``all_written``: moreover no element
        of a writable payload still holds the canary (the kernel wrote all of it)."""
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        cur = self.buf.view(self.idt).cpu()
        prot = torch.ones(self.n, dtype=torch.bool)
        for reg in writable:
            assert reg.payload and reg.arena is self
            reg._strided(prot).fill_(False)
        bad = (cur != self.expected) & prot
        if bool(bad.any()):
            idx = int(bad.nonzero()[0])
            reg, row, col = self._locate(idx)
            if idx < self.guard:
                where = "front guard"
            elif idx >= self.guard + self.capacity:
                where = "back guard"
            elif int(self.expected[idx]) == self.canary:
                where = "canary"
            else:
                where = "input payload"
            got = self.buf[idx:idx + 1].cpu().item()
            raise AssertionError(
                f"arena: {where} modified at element {idx} = (row {row}, col {col}) of region "
                f"'{reg.name if reg else None}' ({reg.rows} x {reg.cols}, ld {reg.ld}): bits "
                f"{int(cur[idx]) & ((1 << (8 * self.itemsize)) - 1):#x} ({got!r}); {int(bad.sum())} elements differ")
        if all_written:
            for reg in writable:
                left = reg._strided(cur) == self.canary
                if bool(left.any()):
                    r, c = (int(v) for v in left.nonzero()[0])
                    raise AssertionError(f"arena: writable region '{reg.name}' still holds the canary at (row {r}, col {c}); "
                                         f"{int(left.sum())} of {reg.rows * reg.cols} elements unwritten")


@contextlib.contextmanager
def lds_policy(tile):
    """Every eligible aac_gemm_batch product on LDS workgroup tile ``tile`` (0 64x64, 1 64x32, 2 32x64,
    3 32x32), or none (``tile`` = 4 / "registers": the register path); the default policy afterwards."""
    from multi_agent_aac_amd import fused
    tile = 4 if tile == "registers" else tile
    fused.set_lds_policy(-1 - tile if tile < 4 else 1 << 30)
    try:
        yield tile
    finally:
        fused.set_lds_policy()
