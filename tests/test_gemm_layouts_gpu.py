"""aac_gemm_batch (include/aac_fused.h) inside the poisoned arena (tests/arena.py): leading
dimensions above the natural ones, base pointers off the 16-B grid, outputs that are column blocks
of a wider matrix, split-K copies with gaps -- the layouts the learner launches (fused.py) and the
ones that flip each alignment decision of the planner.  Every case compares with the fp64 product of
the upcast payloads (the epilogue in fp64, the tolerance of test_gemm_batch_epilogues: atol =
2e-6 sqrt(K) + 1e-6, rtol = 1e-5; split-K sums at 2e-4) and then runs ``arena.check``: nothing but
the declared outputs changed, row gaps and guards included, and the outputs were written in full."""
import numpy as np
import pytest
import torch

from tests.arena import Arena, lds_policy

pytestmark = pytest.mark.gpu
DEV = "cuda"
DSCALE = -0.125        # a power of two: dscale * dvec[n] is exact in both precisions


def reference(a, b, ta, tb, bias=None, addend=None, act=0, mask=None, mact=0):
    """(pre-activation, C) of the grouped GEMM's epilogue in fp64 from the stored operands."""
    opa = a.double().t() if ta else a.double()
    opb = b.double().t() if tb else b.double()
    pre = opa @ opb
    if addend is not None:
        pre = pre + addend.double()
    if bias is not None:
        pre = pre + bias.double()
    out = pre.clamp_min(0) if act == 1 else (torch.tanh(pre) if act == 2 else pre)
    if mact == 1:
        out = out * (mask > 0)
    elif mact == 2:
        out = out * (1 - mask.double() ** 2)
    return pre, out


def tol_of(K, dtype=torch.float32):
    return dict(atol=2e-6 * np.sqrt(K) + 1e-6, rtol=1e-5) if dtype == torch.float32 else dict(atol=1e-12, rtol=1e-12)


class Product:
    """One product with all its operands carved from an arena (its own unless ``ar`` is given), its
    problem struct (``cls``: fused.GemmProb or uam_learner.Gemm64Prob) and its fp64 reference.
    N counts the real columns (a ones column is added to the struct's N).  ``pad``: added to every
    ld; ``shift``: names of operands whose base moves one element off the 16-B grid; split-K copies
    are ``stride_extra`` elements farther apart than a copy (C rows, then cextra)."""

    def __init__(self, cls, M, N, K, ta=0, tb=0, pad=0, ones=0, act=0, mact=0, bias=False, addend=False, dual=False,
                 ksplit=1, stride_extra=0, shift=(), seed=0, data=None, ar=None, dtype=torch.float32):
        self.M, self.N, self.K, self.ks, self.ones, self.dual = M, N, K, ksplit, ones, dual
        g = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + N * 31 + K)
        rnd = lambda *s: torch.rand(*s, generator=g, dtype=dtype) * 2 - 1   # noqa: E731
        d = dict(data or {})
        sh = lambda k: 1 if k in shift else 0                               # noqa: E731
        ldc = N + pad
        copy = M * ldc + (M if ones else 0)
        stride = copy + stride_extra
        if ar is None:
            nc = ksplit + bool(addend) + bool(mact) + bool(dual)
            cap = M * K + (M + K) * pad + K * N + (K + N) * pad + nc * (M * (N + pad) + M + stride_extra) + 4 * (M + N) + 2048
            ar = Arena(cap, dtype, DEV, max_ld=max(M, N, K) + pad + 4)
        self.ar = ar
        a = d.get("A", rnd(K, M) if ta else rnd(M, K))
        b = d.get("B", rnd(N, K) if tb else rnd(K, N))
        self.A = ar.take(*a.shape, ld=a.shape[1] + pad, misalign=sh("A"), name="A", data=a)
        self.B = ar.take(*b.shape, ld=b.shape[1] + pad, misalign=sh("B"), name="B", data=b)
        bv = d.get("bias", rnd(N)) if bias else None
        ad = d.get("addend", rnd(M, N)) if addend else None
        mk = d.get("mask", rnd(M, N)) if mact else None
        dv = d.get("dvec", rnd(N)) if dual else None
        self.bias = ar.vec(N, misalign=sh("bias"), name="bias", data=bv) if bias else None
        self.addend = ar.take(M, N, ld=ldc, misalign=sh("addend"), name="addend", data=ad) if addend else None
        self.mask = ar.take(M, N, ld=ldc, misalign=sh("mask"), name="mask", data=mk) if mact else None
        self.dvec = ar.vec(N, misalign=sh("dvec"), name="dvec", data=dv) if dual else None
        self.C2 = ar.take(M, N, ld=ldc, misalign=sh("C2"), name="C2") if dual else None
        if ksplit > 1:
            part = ar.take(1, ksplit * stride, misalign=sh("C"), name="part", payload=False)
            self.part = part
            self.Cs = [part.carve(s * stride, M, N, ldc, name=f"C.split{s}") for s in range(ksplit)]
            self.cxs = [part.carve(s * stride + M * ldc, 1, M, name=f"cextra.split{s}") for s in range(ksplit)] if ones else []
        else:
            self.Cs = [ar.take(M, N, ld=ldc, misalign=sh("C"), name="C")]
            self.cxs = [ar.vec(M, misalign=sh("cextra"), name="cextra")] if ones else []
        p = lambda r: r.ptr if r is not None else None                      # noqa: E731
        self.prob = cls(self.A.ptr, self.B.ptr, self.Cs[0].ptr, p(self.bias), p(self.addend), p(self.mask),
                        self.cxs[0].ptr if ones else None, stride if ksplit > 1 else 0, M, N + ones, K, self.A.ld,
                        self.B.ld, ldc, ldc if addend else 0, ldc if mact else 0, ta, tb, act, mact, ones, ksplit,
                        p(self.dvec), p(self.C2), DSCALE if dual else 0.0)
        self.stride = stride
        self.pre, self.want = reference(a, b, ta, tb, bv, ad, act, mk, mact)
        self.want_cx = (a.double().t() if ta else a.double()).sum(1)
        self.want2 = (self.want > 0) * (DSCALE * dv.double()) if dual else None
        self.dtype = dtype

    def writable(self):
        return self.Cs + self.cxs + ([self.C2] if self.dual else [])

    def verify(self, what=""):
        if self.ks > 1:
            got = sum(c.get().double() for c in self.Cs)
            kw = dict(atol=2e-4, rtol=0) if self.dtype == torch.float32 else tol_of(self.K, self.dtype)
        else:
            got, kw = self.Cs[0].get().double(), tol_of(self.K, self.dtype)
        np.testing.assert_allclose(got, self.want, err_msg=f"C {what}", **kw)
        if self.ones:
            gx = sum(c.get().double() for c in self.cxs).reshape(-1)
            np.testing.assert_allclose(gx, self.want_cx, err_msg=f"cextra {what}", **kw)
        if self.dual:
            # C2 = (C > 0) dscale dvec[n] exactly; a pre-activation within the rounding error of zero
            # (but not exactly zero) may have either sign in fp32, so it is left out
            sure = (self.pre.abs() > kw["atol"]) | (self.pre == 0)
            g2 = self.C2.get().double()
            assert torch.equal(g2[sure], self.want2[sure]), f"C2 {what}"
            c = self.Cs[0].get()
            assert torch.equal(g2, ((c > 0) * (DSCALE * self.dvec.get().reshape(-1))).double()), f"C2 vs C {what}"


def run(products, ar=None):
    """One launch of the products (one arena), values verified, then the arena checked.  Returns
    the plan's per-product tile modes."""
    from multi_agent_aac_amd import fused
    ar = ar or products[0].ar
    launch = fused.GemmLaunch([p.prob for p in products])
    cfg = launch.plan()[0]
    ar.launch(launch)
    torch.cuda.synchronize()
    for i, p in enumerate(products):
        p.verify(f"(product {i}: M {p.M} N {p.N} K {p.K}, plan {cfg})")
    ar.check(writable=[r for p in products for r in p.writable()])
    return cfg


def P32(*a, **k):
    from multi_agent_aac_amd import fused
    return Product(fused.GemmProb, *a, **k)


# ------------------------------------------------------------------ 1. the learner's strided forms
def _rnd(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.rand(*s, generator=g) * 2 - 1


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("rows", [37, 70])
def test_learner_encoder_products_fill_adjacent_blocks(native_lib, rows, pad):
    """critic_forward_stages: N products in one launch read A = X + n Din (lda = N Din) and write
    C = f + 128 n (ldc = 128 N): each block's neighbours are the other products' outputs."""
    from multi_agent_aac_amd import fused
    N, Din = 3, 24
    r = _rnd(rows + pad)
    ar = Arena(rows * (N * Din + pad) + N * 128 * (Din + 1) + rows * (128 * N + pad) + 2048, torch.float32, DEV,
               max_ld=128 * N + pad)
    X = ar.take(rows, N * Din, ld=N * Din + pad, name="X", payload=False)
    f = ar.take(rows, 128 * N, ld=128 * N + pad, name="f", payload=False)
    xs = [X.sub(0, n * Din, rows, Din, name=f"x{n}", data=r(rows, Din)) for n in range(N)]
    ws = [ar.take(128, Din, name=f"W{n}", data=r(128, Din) * 0.3) for n in range(N)]
    bs = [ar.vec(128, name=f"b{n}", data=r(128) * 0.1) for n in range(N)]
    fs = [f.sub(0, n * 128, rows, 128, name=f"f{n}") for n in range(N)]
    probs = [fused.prob(xs[n].ptr, ws[n].ptr, fs[n].ptr, rows, 128, Din, X.ld, Din, f.ld, tb=1, bias=bs[n].ptr,
                        act=fused.RELU) for n in range(N)]
    assert all(probs[n].A == X.ptr + 4 * n * Din and probs[n].C == f.ptr + 4 * 128 * n for n in range(N))
    ar.launch(fused.GemmLaunch(probs))
    torch.cuda.synchronize()
    for n in range(N):
        _, want = reference(xs[n].get(), ws[n].get(), 0, 1, bias=bs[n].get().reshape(-1), act=1)
        np.testing.assert_allclose(fs[n].get().double(), want, err_msg=f"block {n}", **tol_of(Din))
    ar.check(writable=fs)


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("rows", [37, 70])
def test_learner_merge_data_gradients_read_weight_column_slices(native_lib, rows, pad):
    """_actor_stages wgrad1: three data gradients read B = Wm + 64 j (ldb = 192, 64 columns each);
    the middle one is masked by cat + 64 (ldmask = 192).  cat's other columns are never read: they
    keep the canary, and a NaN folded into a result would show."""
    from multi_agent_aac_amd import fused
    r = _rnd(rows + pad + 1)
    ar = Arena(rows * (256 + 192 + 3 * 68 + 3 * pad) + 256 * (192 + pad) + 2048, torch.float32, DEV, max_ld=256 + pad)
    dha = ar.take(rows, 256, ld=256 + pad, name="dha", data=r(rows, 256))
    Wm = ar.take(256, 192, ld=192 + pad, name="Wm", payload=False)
    wj = [Wm.sub(0, 64 * j, 256, 64, name=f"Wm{j}", data=r(256, 64) * 0.1) for j in range(3)]
    cat = ar.take(rows, 192, ld=192 + pad, name="cat", payload=False)
    eg = torch.relu(r(rows, 64))                       # a relu output: zeros and positives
    mask = cat.sub(0, 64, rows, 64, name="cat[:, 64:128]", data=eg)
    outs = [ar.take(rows, 64, ld=64 + pad, name=n) for n in ("dcat_o", "dcat_g", "dv")]
    probs = [fused.prob(dha.ptr, wj[0].ptr, outs[0].ptr, rows, 64, 256, dha.ld, Wm.ld, outs[0].ld),
             fused.prob(dha.ptr, wj[1].ptr, outs[1].ptr, rows, 64, 256, dha.ld, Wm.ld, outs[1].ld, mask=mask.ptr,
                        ldmask=cat.ld, mact=fused.RELU),
             fused.prob(dha.ptr, wj[2].ptr, outs[2].ptr, rows, 64, 256, dha.ld, Wm.ld, outs[2].ld)]
    assert probs[1].B == Wm.ptr + 4 * 64 and probs[2].B == Wm.ptr + 4 * 128 and probs[1].mask == cat.ptr + 4 * 64
    ar.launch(fused.GemmLaunch(probs))
    torch.cuda.synchronize()
    for j in range(3):
        _, want = reference(dha.get(), wj[j].get(), 0, 0, mask=eg if j == 1 else None, mact=1 if j == 1 else 0)
        np.testing.assert_allclose(outs[j].get().double(), want, err_msg=f"slice {j}", **tol_of(256))
    ar.check(writable=outs)


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("rows", [37, 70])
def test_learner_encoder_weight_gradients(native_lib, rows, pad):
    """_critic_stages encw: N weight gradients in one launch, A = df + 128 n with ta = 1 and lda =
    128 N, B = X + n Din (ldb = N Din), the ones column into cextra, split-K copies one flat-
    gradient stride apart (the last split of 4 owns no K chunk at 37 rows: a copy of zeros)."""
    from multi_agent_aac_amd import fused
    N, Din, S = 3, 24, 4
    r = _rnd(rows + pad + 2)
    per = 128 * Din + 128                               # W_n | b_n, consecutive in the flat gradient
    nC = fused.padded(N * per) + 8
    ar = Arena(rows * (128 * N + N * Din + 2 * pad) + S * nC + 2048, torch.float32, DEV, max_ld=128 * N + pad)
    df = ar.take(rows, 128 * N, ld=128 * N + pad, name="df", payload=False)
    X = ar.take(rows, N * Din, ld=N * Din + pad, name="X", payload=False)
    dfs = [df.sub(0, 128 * n, rows, 128, name=f"df{n}", data=r(rows, 128)) for n in range(N)]
    xs = [X.sub(0, n * Din, rows, Din, name=f"x{n}", data=r(rows, Din)) for n in range(N)]
    g = ar.take(1, S * nC, name="gC", payload=False)
    gw = [[g.carve(s * nC + n * per, 128, Din, name=f"dW{n}.split{s}") for s in range(S)] for n in range(N)]
    gb = [[g.carve(s * nC + n * per + 128 * Din, 1, 128, name=f"db{n}.split{s}") for s in range(S)] for n in range(N)]
    probs = [fused.prob(dfs[n].ptr, xs[n].ptr, gw[n][0].ptr, 128, Din, rows, df.ld, X.ld, Din, ta=1, ones=1,
                        cextra=gb[n][0].ptr, ksplit=S, split_stride=nC) for n in range(N)]
    ar.launch(fused.GemmLaunch(probs))
    torch.cuda.synchronize()
    for n in range(N):
        _, want = reference(dfs[n].get(), xs[n].get(), 1, 0)
        np.testing.assert_allclose(sum(c.get().double() for c in gw[n]), want, atol=2e-4, rtol=0, err_msg=f"dW{n}")
        np.testing.assert_allclose(sum(c.get().double() for c in gb[n]).reshape(-1), dfs[n].get().double().sum(0),
                                   atol=2e-4, rtol=0, err_msg=f"db{n}")
    if rows == 37:
        assert all(float(gw[n][S - 1].get().abs().max()) == 0.0 for n in range(N))
    ar.check(writable=[c for n in range(N) for c in gw[n] + gb[n]])


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("rows", [37, 70])
def test_learner_dwq_reads_cat_columns(native_lib, rows, pad):
    """_actor_stages wgrad2 dWq: A = dq (ta = 1), B = the first 64 columns of cat at ldb = 192,
    two split-K copies."""
    from multi_agent_aac_amd import fused
    r = _rnd(rows + pad + 3)
    stride = 64 * 64 + 12
    ar = Arena(rows * (64 + 192 + 2 * pad) + 2 * stride + 2048, torch.float32, DEV, max_ld=192 + pad)
    dq = ar.take(rows, 64, ld=64 + pad, name="dq", data=r(rows, 64))
    cat = ar.take(rows, 192, ld=192 + pad, name="cat", payload=False)
    eo = cat.sub(0, 0, rows, 64, name="cat[:, :64]", data=torch.relu(r(rows, 64)))
    g = ar.take(1, 2 * stride, name="gA", payload=False)
    cs = [g.carve(s * stride, 64, 64, name=f"dWq.split{s}") for s in range(2)]
    ar.launch(fused.GemmLaunch([fused.prob(dq.ptr, eo.ptr, cs[0].ptr, 64, 64, rows, dq.ld, cat.ld, 64, ta=1, ksplit=2,
                                           split_stride=stride)]))
    torch.cuda.synchronize()
    _, want = reference(dq.get(), eo.get(), 1, 0)
    np.testing.assert_allclose(sum(c.get().double() for c in cs), want, atol=2e-4, rtol=0)
    ar.check(writable=cs)


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("rows", [37, 70])
def test_learner_combine_layer_with_dual_output(native_lib, rows, pad):
    """_actor_stages ccomb: h = relu(f Wc^T + bc) with the second output dh = (h > 0) dscale wq."""
    p = P32(rows, 256, 128 * 3, tb=1, pad=pad, bias=True, act=1, dual=True, seed=5)
    run([p])


# ------------------------------------------------------------------ 2. layout sweep, register path
EPI = [dict(), dict(bias=True), dict(addend=True), dict(mact=1), dict(mact=2), dict(act=2, bias=True), dict(ones=1),
       dict(act=1, bias=True, addend=True, mact=1), dict(act=1, bias=True, dual=True)]


@pytest.mark.parametrize("pad", [0, 4, 1], ids=["natural", "pad4", "pad1"])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_layout_sweep_register_path(native_lib, ta, tb, pad):
    """M, N in {1, 31, 33, 65} x K in {1, 3, 4, 33, 260} (260: the prefetch ring) on the register
    path; natural ld, every ld + 4 (all 16-B conditions kept), every ld + 1 (all broken); the
    epilogue rotates through bias / addend / masks / tanh / ones column / dual output."""
    i = ta * 2 + tb + 4 * pad
    n = 0
    with lds_policy("registers"):
        for M in (1, 31, 33, 65):
            for N in (1, 31, 33, 65):
                for K in (1, 3, 4, 33, 260):
                    epi = EPI[i % len(EPI)]
                    i += 1
                    cfg = run([P32(M, N, K, ta=ta, tb=tb, pad=pad, seed=i, **epi)])
                    assert cfg == [0], (M, N, K, epi)
                    n += 1
    assert n == 80


def test_wide_mode_product_with_padded_rows(native_lib):
    """>= 2048 wave tiles: one tile per wave, the 16-B staged epilogue; ldc = N + 4."""
    with lds_policy("registers"):
        assert run([P32(16400, 128, 36, tb=1, pad=4, bias=True, act=1, seed=9)]) == [0]


# ------------------------------------------------------------------ 3. the same on each LDS tile
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("tile", [0, 1, 2, 3], ids=["t64x64", "t64x32", "t32x64", "t32x32"])
def test_layout_sweep_lds_tiles(native_lib, tile, ta, tb):
    """Each forced LDS workgroup tile on the smallest eligible shapes with every ld + 4 (ldc > N:
    interior and edge epilogue both run); with every ld + 1 the operands no longer load as 16-B
    segments and the plan must fall back to the register path."""
    lay = (2 if ta else 0) + (0 if tb else 1)
    i = tile * 4 + ta * 2 + tb
    with lds_policy(tile):
        for M, N in ((64, 64), (68, 64), (100, 100), (132, 36)):
            for K in (64, 68, 100):
                epi = EPI[i % len(EPI)]
                i += 1
                if epi.get("ones") and tb:
                    epi = dict(bias=True, mact=2)      # a K-contiguous B takes no ones column on the LDS path
                cfg = run([P32(M, N, K, ta=ta, tb=tb, pad=4, seed=i, **epi)])
                if epi.get("dual"):
                    assert cfg == [0], (M, N, K, epi)  # the dual output stays on the register path
                else:
                    assert cfg == [1 + 4 * tile + lay], (M, N, K, epi, cfg)
                cfg = run([P32(M, N, K, ta=ta, tb=tb, pad=1, seed=i, **epi)])
                assert cfg == [0], (M, N, K, epi, cfg)


# ------------------------------------------------------------------ 4. one operand off the 16-B grid
FULL = dict(M=100, N=100, K=68, ta=0, tb=1, pad=4, bias=True, addend=True, mact=1, act=1)


@pytest.mark.parametrize("which", ["none", "A", "B", "C", "bias", "addend", "mask"])
def test_one_operand_off_the_16_byte_grid(native_lib, which):
    """A fully aligned product (LDS tile, vector epilogue); then one base pointer at a time moves
    by one float.  A or B off the grid: no 16-B operand segments, the register path; C / bias /
    addend / mask: the LDS tile stays, its epilogue goes element by element."""
    with lds_policy(0):
        cfg = run([P32(**FULL, shift=() if which == "none" else (which,), seed=11)])
        assert (cfg == [0]) == (which in ("A", "B")), cfg
    with lds_policy("registers"):
        assert run([P32(**FULL, shift=() if which == "none" else (which,), seed=12)]) == [0]


@pytest.mark.parametrize("which", ["none", "dvec", "C2", "C"])
def test_dual_output_operand_off_the_16_byte_grid(native_lib, which):
    run([P32(100, 100, 68, tb=1, pad=4, bias=True, act=1, dual=True, shift=() if which == "none" else (which,), seed=13)])


@pytest.mark.parametrize("policy", [0, "registers"])
@pytest.mark.parametrize("extra", [8, 1, 3])
def test_split_stride_off_the_16_byte_grid(native_lib, policy, extra):
    """split_stride % 4 != 0 puts every odd copy off the grid: no 16-B stores into the copies."""
    with lds_policy(policy):
        cfg = run([P32(64, 64, 256, ta=1, ones=1, ksplit=4, stride_extra=extra, seed=14)])
        assert (cfg != [0]) == (policy == 0)


# ------------------------------------------------------------------ 5. split-K edges
@pytest.mark.parametrize("policy,K", [("registers", 40), (0, 64)])
def test_more_splits_than_chunks(native_lib, policy, K):
    """ksplit = 8 over K = 40 (three 16-wide chunks; on the LDS tile K = 64, two 32-wide chunks): the
    splits that own no chunk write copies of zeros; the gaps between the copies stay canary."""
    with lds_policy(policy):
        p = P32(64, 64, K, ta=1, ones=1, ksplit=8, stride_extra=20, seed=15)
        cfg = run([p])
        assert (cfg != [0]) == (policy == 0)
    empty = [s for s in range(8) if float(p.Cs[s].get().abs().max()) == 0.0 and float(p.cxs[s].get().abs().max()) == 0.0]
    assert len(empty) == 8 - (3 if K == 40 else 2), empty


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("aligned_stride", [True, False])
@pytest.mark.parametrize("M,N", [(4, 7), (5, 4), (3, 4)])           # n = M (N + 1) = 32, 25, 15: n % 4 = 0, 1, 3
def test_split_copies_summed_and_stepped_in_the_arena(native_lib, M, N, aligned_stride, shift):
    """The split-K copies of a weight gradient (gstride > n), then aac_sum_partials_strided and
    aac_adam_flat_sum_strided over them: the copy-parallel kernels (gstride % 4 == 0, aligned gpart)
    read the pad words of a copy and discard them, the element kernels otherwise; pad words, the
    parameter / moment buffers' surroundings and the guards stay untouched.  Sum: against the fp64
    sum of the fp32 copies within the rounding of ns fp32 additions; Adam (from zero moments, step 1)
    in fp64 from the summed gradient, tolerances of test_adam_sum_matches_torch."""
    import ctypes
    from multi_agent_aac_amd import fused
    n, ns, K = M * (N + 1), 8, 40
    extra = (fused.padded(n) - n + 4) if aligned_stride else (fused.padded(n) - n + 5)
    p = P32(M, N, K, ta=1, ones=1, ksplit=ns, stride_extra=extra, shift=("C",) if shift else (), seed=16)
    ar = p.ar
    gstride = p.stride
    assert gstride > n and (gstride % 4 == 0) == aligned_stride and (p.part.ptr % 16 == 0) == (not shift)
    run([p])
    r = _rnd(n)
    p0 = r(n) * 2
    out, gout = ar.vec(n, name="out"), ar.vec(n, name="gout")
    par = ar.vec(n, name="param", data=p0)
    m = ar.vec(n, name="exp_avg", data=torch.zeros(n))
    v = ar.vec(n, name="exp_avg_sq", data=torch.zeros(n))
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    vp = ctypes.c_void_p
    for reg, span in ((p.part, (ns - 1) * gstride + n), (out, n), (gout, n), (par, n), (m, n), (v, n)):
        ar.inside(reg.ptr, span)
    fused._chk(fused.lib().aac_sum_partials_strided(vp(out.ptr), vp(p.part.ptr), ns, gstride, n, fused._stream()), "sum")
    fused._chk(fused.lib().aac_adam_flat_sum_strided(vp(par.ptr), vp(p.part.ptr), ns, gstride, vp(gout.ptr), vp(m.ptr),
                                                     vp(v.ptr), n, 1e-3, 0.9, 0.999, 1e-3, vp(step.data_ptr()), 1,
                                                     fused._stream()), "adam")
    torch.cuda.synchronize()
    copies = torch.stack([torch.cat([c.get().reshape(-1), x.get().reshape(-1)]) for c, x in zip(p.Cs, p.cxs)]).double()
    g64 = copies.sum(0)
    bound = ns * 2.0 ** -24 * copies.abs().sum(0) + 1e-30
    assert bool(((gout.get().double().reshape(-1) - g64).abs() <= bound).all())
    assert torch.equal(out.get(), gout.get())           # one summation order for both entry points
    gd = gout.get().double().reshape(-1)
    m_ref, v_ref = 0.1 * gd, 0.001 * gd * gd
    p_ref = p0.double() - 1e-3 / (1 - 0.9) * m_ref / (v_ref.sqrt() / np.sqrt(1 - 0.999) + 1e-3)
    np.testing.assert_allclose(m.get().double().reshape(-1), m_ref, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(v.get().double().reshape(-1), v_ref, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(par.get().double().reshape(-1), p_ref, rtol=0, atol=1e-6)
    ar.check(writable=p.writable() + [out, gout, par, m, v])


# ------------------------------------------------------------------ 6. exact zeros
@pytest.mark.parametrize("policy", [0, "registers"])
@pytest.mark.parametrize("mact", [1, 2])
def test_exact_zero_semantics(native_lib, policy, mact):
    """The ABI's rule is ``> 0``.  Rows 0-3 of A are +0 and rows 4-7 are -0, the bias is +0 on even
    and -0 on odd columns: those ReLU pre-activations are exact zeros in the fp64 reference (sums of
    +0 and -0 products plus a +-0 bias; whichever sign the accumulation order leaves, the output is 0).
    mact = 1 mask elements +0, -0, +-denormal (a positive denormal is > 0); mact = 2 mask
    elements +-1 (the derivative 1 - t^2 is exactly 0).  On the LDS tile's vector epilogue and on the
    register path."""
    M = N = K = 64
    r = _rnd(40 + mact)
    a = r(M, K)
    a[0:4] = 0.0
    a[4:8] = -0.0
    bias = torch.zeros(N)
    bias[1::2] = -0.0
    mask = r(M, N)
    if mact == 1:
        for c, val in enumerate((0.0, -0.0, 1e-40, -1e-40, 1e-45, -1e-45)):
            mask[:, c::8] = val
    else:
        mask[:, 0::4] = 1.0
        mask[:, 1::4] = -1.0
    with lds_policy(policy):
        p = P32(M, N, K, pad=4, bias=True, act=1, mact=mact, data=dict(A=a, bias=bias, mask=mask), seed=17)
        assert bool((p.pre[0:8] == 0).all())
        cfg = run([p])
        assert (cfg != [0]) == (policy == 0)
    got = p.Cs[0].get()
    assert float(got[0:8].abs().max()) == 0.0
    if mact == 1:
        keep = got[8:, 2::8] != 0                       # the positive denormal keeps the (positive) values
        assert bool((keep == (p.want[8:, 2::8] != 0)).all()) and bool(keep.any())
        for c in (0, 1, 3, 5):
            assert float(got[:, c::8].abs().max()) == 0.0
    else:
        assert float(got[:, 0::4].abs().max()) == 0.0 and float(got[:, 1::4].abs().max()) == 0.0


def test_exact_zero_dual_output(native_lib):
    """Dual output where C == 0 exactly (zero rows of A, zero bias, ReLU): C2 is 0 there, not
    dscale dvec[n]; rows whose pre-activation is negative give 0 as well."""
    M, N, K = 33, 65, 33
    r = _rnd(50)
    a = r(M, K)
    a[0:3] = 0.0
    a[3:6] = -0.0
    bias = torch.zeros(N)
    bias[1::2] = -0.0
    for pad in (0, 4, 1):
        p = P32(M, N, K, tb=1, pad=pad, bias=True, act=1, dual=True, data=dict(A=a, bias=bias), seed=18)
        run([p])
        assert float(p.C2.get()[0:6].abs().max()) == 0.0 and float(p.C2.get().abs().max()) > 0.0
