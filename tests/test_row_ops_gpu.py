"""aac_act_bgrad, aac_bias_act and the flat optimiser kernels called directly, every operand in the
poisoned arena (tests/arena.py): strided rows and ragged tiles for the ticketed bias reduction, and
element counts on both sides of one full trip of the capped elementwise grid.

Bounds: identity / ReLU backward are selections (bit-exact); the tanh backward g (1 - t t) is two or
three float32 roundings of a value <= |g| for |t| <= 1, so |error| <= 4 x 2^-24 |gy|; the bias
gradient is a float32 sum of M terms in some order, |error| <= M 2^-24 sum |gm| (the plain
recursive-summation bound, which holds for any order); tanhf forward 1e-6 and Adam against
torch.optim.Adam 1e-6 as in test_learner_gpu / test_fused_gpu."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
SHAPES = [(1, 1), (31, 63), (32, 64), (33, 65), (257, 200)]
vp = ctypes.c_void_p


def _stream():
    return vp(torch.cuda.current_stream().cuda_stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ============================================================================ aac_act_bgrad
def _y_for(act, M, O, seed):
    y = _rand((M, O), seed)
    if act == 1:
        y[::3, ::2] = 0.0                  # exact zeros: y > 0 is false there
    if act == 2:
        y = torch.tanh(y)
    return y


@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,O", SHAPES)
def test_act_bgrad_strided_forms(native_lib, M, O, act):
    """gm only (db NULL), db only (gm NULL) and both, each operand with its own row stride > O; M on
    both sides of the 32-row workgroup tile, O of the 64-column one; two launches of each db form on
    the same ws / tickets (the second relies on the tickets the first left zeroed)."""
    from multi_agent_aac_amd import ops
    L = ops.lib()
    gy, y = _rand((M, O), 100 * M + O), _y_for(act, M, O, M + O + act)
    nrb, ncb = (M + 31) // 32, (O + 63) // 64
    ar = Arena(8 * (M * (O + 9) + 64) + 6 * (nrb * O + O + 64), torch.float32, DEV, max_ld=O + 9)
    GY = ar.take(M, O, ld=O + 3, data=gy, name="gy")
    Y = ar.take(M, O, ld=O + 5, data=y, name="y")
    tickets = torch.zeros(ncb + 8, dtype=torch.int32, device=DEV)
    tickets[ncb:] = 0x5A5A                               # behind the tickets the launch owns
    gy_n, y_n = gy.numpy(), y.numpy()
    if act == 0:
        want = gy_n
    elif act == 1:
        want = np.where(y_n > 0, gy_n, np.float32(0))
    else:
        want = gy_n.astype(np.float64) * (1.0 - y_n.astype(np.float64) ** 2)

    def launch(gm, db, ws):
        for reg in (GY, Y, gm):
            if reg is not None:
                ar.inside_mat(reg.ptr, M, O, reg.ld, reg.name)
        if db is not None:
            ar.inside(db.ptr, O, "db")
            ar.inside(ws.ptr, nrb * O, "ws")
        rc = L.aac_act_bgrad(vp(GY.ptr), GY.ld, vp(Y.ptr), Y.ld, vp(gm.ptr) if gm else None, gm.ld if gm else 0,
                             vp(db.ptr) if db else None, M, O, act, vp(ws.ptr) if ws else None,
                             vp(tickets.data_ptr()), _stream())
        assert rc == 0, L.aac_learn_last_error()

    def check_tickets():
        t = tickets.cpu().numpy()
        assert (t[:ncb] == 0).all() and (t[ncb:] == 0x5A5A).all(), t

    def check_gm(gm):
        got = gm.get().numpy()
        if act in (0, 1):
            assert np.array_equal(_bits(got), _bits(want))
        else:
            err = np.abs(got.astype(np.float64) - want)
            assert (err <= 4 * U * np.abs(gy_n.astype(np.float64))).all(), float(err.max())
        return got

    # gm only
    GM0 = ar.take(M, O, ld=O + 7, name="gm (db NULL)")
    launch(GM0, None, None)
    ar.check(writable=[GM0])
    gm_bits = check_gm(GM0)
    ar.freeze([GM0])
    check_tickets()                                      # untouched without db
    colsum = gm_bits.astype(np.float64).sum(0)
    bound = M * U * np.abs(gm_bits.astype(np.float64)).sum(0)

    def check_db(db):
        got = db.get().numpy().reshape(-1)
        assert (np.abs(got.astype(np.float64) - colsum) <= bound).all(), float(np.abs(got - colsum).max())
        return got

    # db only, twice on the same workspace and tickets
    DB1, WS1 = ar.vec(O, name="db (gm NULL)"), ar.vec(nrb * O, name="ws 1")
    launch(None, DB1, WS1)
    ar.check(writable=[DB1, WS1])
    check_tickets()
    first = check_db(DB1)
    ar.freeze([DB1])
    DB1b = ar.vec(O, name="db (gm NULL) again")
    launch(None, DB1b, WS1)
    ar.check(writable=[WS1, DB1b])
    check_tickets()
    assert np.array_equal(_bits(DB1b.get().numpy().reshape(-1)), _bits(first))
    ar.freeze([WS1, DB1b])
    # both, twice
    GM2, DB2, WS2 = ar.take(M, O, ld=O + 9, name="gm"), ar.vec(O, name="db"), ar.vec(nrb * O, name="ws 2")
    launch(GM2, DB2, WS2)
    ar.check(writable=[GM2, DB2, WS2])
    check_tickets()
    assert np.array_equal(_bits(check_gm(GM2)), _bits(gm_bits))
    both = check_db(DB2)
    assert np.array_equal(_bits(both), _bits(first))     # the same reduction with or without the gm store
    ar.freeze([GM2, DB2, WS2])
    GM2b, DB2b = ar.take(M, O, ld=O + 1, name="gm again"), ar.vec(O, name="db again")
    launch(GM2b, DB2b, WS2)
    ar.check(writable=[GM2b, DB2b, WS2])
    check_tickets()
    assert np.array_equal(_bits(GM2b.get().numpy()), _bits(gm_bits))
    assert np.array_equal(_bits(DB2b.get().numpy().reshape(-1)), _bits(first))


# ============================================================================ aac_bias_act
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("M,O", SHAPES)
def test_bias_act_in_place(native_lib, M, O, act):
    """y = act(y + b) in place on a contiguous [M][O] arena region: identity and ReLU to the bit
    (a float32 sum is the rounded float64 sum), tanh within 1e-6 of float64."""
    from multi_agent_aac_amd import ops
    L = ops.lib()
    y0, b = _rand((M, O), 7 * M + O), _rand((O,), O)
    ar = Arena(M * O + O + 256, torch.float32, DEV, max_ld=max(O, 1))
    Y, B = ar.take(M, O, data=y0, name="y"), ar.vec(O, data=b, name="b")
    ar.inside(Y.ptr, M * O, "y")
    ar.inside(B.ptr, O, "b")
    rc = L.aac_bias_act(vp(Y.ptr), vp(B.ptr), M, O, act, _stream())
    assert rc == 0, L.aac_learn_last_error()
    ar.check(writable=[Y])
    got = Y.get().numpy()
    s = y0.numpy().astype(np.float64) + b.numpy().astype(np.float64)
    if act == 0:
        assert np.array_equal(_bits(got), _bits(s.astype(np.float32)))
    elif act == 1:
        s32 = s.astype(np.float32)
        assert np.array_equal(_bits(got), _bits(np.where(s32 > 0, s32, np.float32(0))))
    else:
        np.testing.assert_allclose(got.astype(np.float64), np.tanh(s), rtol=0, atol=1e-6)


# ============================================================================ flat optimiser kernels
def _grid_cap():
    """Elements of one full trip of the elementwise kernels' grid, from the launcher's own text:
    grid_for() in csrc/aac_learn.hip caps the grid (``b < 2048 ? ... : 2048``) of LEARN_BLOCK-thread
    workgroups, so element cap x LEARN_BLOCK is the first one a thread reaches on its second trip."""
    import multi_agent_aac_amd
    src = open(os.path.join(os.path.dirname(multi_agent_aac_amd.__file__), "csrc", "aac_learn.hip")).read()
    block = int(re.search(r"constexpr int LEARN_BLOCK = (\d+);", src).group(1))
    body = re.search(r"int grid_for\(int64_t n\) \{(.*?)\n\}", src, re.S).group(1)
    caps = set(re.findall(r"\b(\d{3,})\b", body))
    assert len(caps) == 1 and "LEARN_BLOCK" in body, body
    return int(caps.pop()) * block


def _sizes():
    cap = _grid_cap()
    assert cap == 2048 * 256 == 524288
    return [1, 255, 257, cap + 257]


SIZES = [1, 255, 257, 524288 + 257]          # = _sizes(), asserted in test_grid_cap_is_the_launchers


def test_grid_cap_is_the_launchers(native_lib):
    assert _sizes() == SIZES


def _adam_call(name, P, G, Mo, V, n, step, step_add=None, gscale=None, off=0, lr=1e-3):
    """One Adam launch on elements [off, off + n) of the four arena vectors."""
    from multi_agent_aac_amd import fused
    L = fused.lib()
    for reg in (P, G, Mo, V):
        reg.arena.inside(reg.ptr + 4 * off, n, reg.name)
    a = [vp(r.ptr + 4 * off) for r in (P, G, Mo, V)] + [n, lr, 0.9, 0.999, 1e-8, vp(step.data_ptr())]
    if name == "aac_adam_flat":
        L.aac_adam_flat.argtypes = [vp] * 4 + [ctypes.c_int64] + [ctypes.c_float] * 4 + [vp, vp]
        rc = L.aac_adam_flat(*a, _stream())
    elif name == "aac_adam_flat_at":
        rc = L.aac_adam_flat_at(*a, step_add, _stream())
    else:
        rc = L.aac_adam_flat_at_scaled(*a, step_add, gscale, _stream())
    assert rc == 0, name


def _adam_state(ar, n, p0, tag):
    z = torch.zeros(n)
    return (ar.vec(n, data=p0, name=f"param {tag}"), ar.vec(n, name=f"grad {tag}"),
            ar.vec(n, data=z, name=f"exp_avg {tag}"), ar.vec(n, data=z, name=f"exp_avg_sq {tag}"))


def _same(ar, A, B):
    for a, b in zip(A, B):
        assert torch.equal(a.view.view(torch.int32), b.view.view(torch.int32)), (a.name, b.name)


@pytest.mark.parametrize("n", SIZES)
def test_adam_flat_forms(native_lib, n):
    """Three Adam steps of aac_adam_flat against torch.optim.Adam on the CPU (1e-6), buffers in the
    arena (the element past n keeps the canary).  Beside it, bit for bit: aac_adam_flat_at with the
    step counter fixed at 0 and step_add = k (the k-th step of the plain form), aac_adam_flat_at_scaled
    with gscale = 0.5 on the doubled gradient (an exact power of two), and the same data as two
    launches of about n / 2 (the kernel does not depend on the element's position; at n = cap + 257
    the single launch takes its second grid-stride trip and neither half does)."""
    p0 = _rand((n,), n)
    ref = p0.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=1e-3)
    ar = Arena(16 * (n + 64), torch.float32, DEV)
    plain, at, scaled, halves = (_adam_state(ar, n, p0, t) for t in ("plain", "at", "scaled", "halves"))
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    h = n // 2
    for k in range(1, 4):
        g = _rand((n,), 1000 * k + n)
        ref.grad = g.clone()
        opt.step()
        for st in (plain, at, halves):
            st[1].fill(g)
        scaled[1].fill(2 * g)
        step.fill_(k)
        _adam_call("aac_adam_flat", *plain, n, step)
        _adam_call("aac_adam_flat_at", *at, n, zero, step_add=k)
        _adam_call("aac_adam_flat_at_scaled", *scaled, n, zero, step_add=k, gscale=0.5)
        if h:
            _adam_call("aac_adam_flat", *halves, h, step)
        _adam_call("aac_adam_flat", *halves, n - h, step, off=h)
        ar.check(writable=[r for st in (plain, at, scaled, halves) for r in (st[0], st[2], st[3])])
        ar.freeze([r for st in (plain, at, scaled, halves) for r in (st[0], st[2], st[3])])
        for other in (at, halves):
            _same(ar, plain, other)
        for i in (0, 2, 3):
            _same(ar, [plain[i]], [scaled[i]])
    np.testing.assert_allclose(plain[0].get().numpy().reshape(-1), ref.detach().numpy(), atol=1e-6, rtol=1e-6)
    assert int(step.item()) == 3 and int(zero.item()) == 0          # the kernels only read the counter


@pytest.mark.parametrize("n", SIZES)
def test_polyak_flat_forms(native_lib, n):
    """aac_polyak_flat against float64 (1e-7 / 1e-6 as test_learner_gpu), aac_polyak_flat_step and
    both slots of aac_polyak_flat2 bit-equal to it with their counters advanced, and the same data as
    two launches of about n / 2; arena buffers, so one element past n keeps the canary."""
    from multi_agent_aac_amd import ops
    L = ops.lib()
    tau = 0.01
    t0, s0 = _rand((n,), n + 1), _rand((n,), n + 2)
    n2 = 257 if n != 257 else SIZES[-1]                    # the other network of the two-network launch
    u0, v0 = _rand((n2,), n + 3), _rand((n2,), n + 4)
    ar = Arena(8 * (n + 64) + 6 * (n2 + 64), torch.float32, DEV)
    S = ar.vec(n, data=s0, name="src")
    T1, T2, T3, T4, T5 = (ar.vec(n, data=t0, name=f"tgt {k}") for k in ("plain", "step", "halves", "flat2 a", "flat2 b"))
    S2 = ar.vec(n2, data=v0, name="src other")
    U1, U4, U5 = (ar.vec(n2, data=u0, name=f"tgt other {k}") for k in ("plain", "flat2 a", "flat2 b"))
    st = torch.tensor([3, 10, 20, 30, 40], dtype=torch.int32, device=DEV)
    sp = lambda i: vp(st.data_ptr() + 4 * i)               # noqa: E731

    def call(fn, *a):
        assert fn(*a, _stream()) == 0, L.aac_learn_last_error()

    for reg, k in ((S, n), (T1, n), (T2, n), (T3, n), (T4, n), (T5, n), (S2, n2), (U1, n2), (U4, n2), (U5, n2)):
        ar.inside(reg.ptr, k, reg.name)
    call(L.aac_polyak_flat, vp(T1.ptr), vp(S.ptr), n, tau)
    call(L.aac_polyak_flat, vp(U1.ptr), vp(S2.ptr), n2, tau)
    call(L.aac_polyak_flat_step, vp(T2.ptr), vp(S.ptr), n, tau, sp(0), 5)
    h = n // 2
    if h:
        call(L.aac_polyak_flat, vp(T3.ptr), vp(S.ptr), h, tau)
    call(L.aac_polyak_flat, vp(T3.ptr + 4 * h), vp(S.ptr + 4 * h), n - h, tau)
    # the two-network launch with this network in the first slot, then in the second
    call(L.aac_polyak_flat2, vp(T4.ptr), vp(S.ptr), n, sp(1), vp(U4.ptr), vp(S2.ptr), n2, sp(2), tau, 7)
    call(L.aac_polyak_flat2, vp(U5.ptr), vp(S2.ptr), n2, sp(3), vp(T5.ptr), vp(S.ptr), n, sp(4), tau, 9)
    ar.check(writable=[T1, T2, T3, T4, T5, U1, U4, U5])
    want = (1 - tau) * t0.double() + tau * s0.double()
    np.testing.assert_allclose(T1.get().numpy().reshape(-1), want.numpy(), atol=1e-7, rtol=1e-6)
    _same(ar, [T1] * 4, [T2, T3, T4, T5])
    _same(ar, [U1] * 2, [U4, U5])
    assert st.cpu().tolist() == [8, 17, 27, 39, 49]
