"""The exploration maps' raw entry (aac_visits_accumulate, include/aac_visits.h) on synthetic inputs,
bit-equal to the numpy restatement (tests/visits_ref.py).

Row counts: a workgroup owns CHUNK = 1024 consecutive rows of E * N, so the cases are 1 row, CHUNK - 1
(N = 3), CHUNK (N = 16), CHUNK + 1 (N = 5) and, past three full workgroups, 3 CHUNK + 7 (prime: N = 1)
with its neighbours at N = 17 (181 x 17 = 3 CHUNK + 5, 182 x 17 = 3 CHUNK + 22).  Every case holds rows on
every edge and 1 ulp either side of it, at ``hi`` exactly, outside the range and at NaN / +-Inf, float
actions whose double differs from the double edge (float32(0.1)), episodes on both sides of
``explore_until``, a mixed ``map_idx`` over 3 maps with out-of-range entries, and a ``sel`` with gaps.
A position table of at most 10240 bins (all planes) is kept in LDS by each workgroup, a larger one takes
its adds in global memory: 3 maps x 50 x 50 is past the threshold, one map and the small grids are below it.
The tables are slices of a larger int64 tensor filled with a sentinel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import visits_ref

pytestmark = pytest.mark.gpu

CHUNK = 1024
SENTINEL = -0x0123456789ABCDEF
UNTIL = 7
XR, YR, AR = (455.0, 680.0), (255.0, 385.0), (-1.0, 1.0)
#         E      N   f64 act  n_maps  GX  GY  A
CASES = {"r1": (1, 1, False, 1, 50, 50, 20),
         "chunk_m1_n3": (341, 3, False, 3, 50, 50, 20),
         "chunk_n16": (64, 16, True, 3, 7, 11, 32),
         "chunk_p1_n5": (205, 5, False, 3, 50, 50, 20),
         "3chunk_p7_n1": (3 * CHUNK + 7, 1, True, 3, 50, 50, 20),
         "3chunk_p5_n17": (181, 17, False, 3, 13, 50, 3),
         "3chunk_p22_n17": (182, 17, True, 1, 50, 50, 20),
         "uam_bound_n5": (420, 5, True, 1, 50, 50, 20),
         # the largest position table a workgroup keeps in LDS (2 x 64 x 80 = 10240 bins) and the first
         # one past it, whose adds go straight to global memory
         "pos_lds_last": (300, 5, False, 1, 64, 80, 20),
         "pos_lds_past": (300, 5, True, 1, 5121, 1, 20)}


def _specials(lo, hi, G, f32):
    e = visits_ref.edges(lo, hi, G)
    s = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                        [hi, lo, lo - 1.0, hi + 1.0, np.nan, np.inf, -np.inf, 2.0 * hi + 5.0, -1e300, 1e300]])
    if f32:     # the floats nearest the edges, and 1 float ulp either side: their doubles are not the edges
        f = e.astype(np.float32)
        with np.errstate(over="ignore"):
            s = np.concatenate([f, np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf)),
                                s.astype(np.float32), np.float32([0.1, -0.1, 0.7, 0.3])]).astype(np.float32)
    return s


def gen(name, call=0):
    """Inputs of accumulate call ``call`` of a case: uniform rows a little wider than the ranges, with a
    third of the coordinates replaced by the special values."""
    E, N, f64, n_maps, GX, GY, A = CASES[name]
    xr, yr = ((0.0, 40.0), (0.0, 40.0)) if name.startswith("uam") else (XR, YR)
    rng = np.random.default_rng([len(name), E, N, call])

    def axis(lo, hi, G, f32, size):
        v = rng.uniform(lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo), size)
        sp = _specials(lo, hi, G, f32)
        pick = rng.random(size) < 1 / 3
        v = v.astype(np.float32) if f32 else v
        v[pick] = sp[rng.integers(0, len(sp), int(pick.sum()))]
        return v
    pos = np.stack([axis(*xr, GX, False, (E, N)), axis(*yr, GY, False, (E, N))], axis=-1)
    act = np.stack([axis(*AR, A, not f64, (E, N)), axis(*AR, A, not f64, (E, N))], axis=-1)
    episode = rng.choice(np.int32([1, UNTIL - 1, UNTIL, UNTIL + 1, UNTIL + 50]), E).astype(np.int32)
    map_idx = rng.integers(0, n_maps, E).astype(np.int32)
    map_idx[rng.random(E) < 0.05] = rng.choice(np.int32([-1, n_maps, n_maps + 5, -2 ** 31, 2 ** 31 - 1]))
    sel = (rng.random(E) < 0.8).astype(np.uint8)
    if E == 1:
        sel[:] = 1
        map_idx[:] = 0
    return dict(pos=pos, act=act, episode=episode, map_idx=map_idx, sel=sel, xr=xr, yr=yr)


@functools.lru_cache(maxsize=None)
def reference(name, calls=2, use_map=True, use_sel=True):
    E, N, f64, n_maps, GX, GY, A = CASES[name]
    xs = [gen(name, c) for c in range(calls)]
    ref = visits_ref.VisitsRef(n_maps, GX, GY, A, xs[0]["xr"], xs[0]["yr"], AR)
    for x in xs:
        ref.accumulate(x["pos"], x["act"], x["episode"], UNTIL, x["map_idx"] if use_map else None,
                       x["sel"] if use_sel else None)
    return xs, ref


class Tables:
    """pos_hist, act_hist and counters as slices of one sentinel-filled int64 tensor, with the state struct."""

    def __init__(self, n_maps, GX, GY, A, xr, yr, ar=AR, guard=257):
        from multi_agent_aac_amd import _native
        P = 2 * n_maps
        self.sizes = [P * GX * GY, 2 * A * A, P * 4]
        self.shapes = [(P, GX, GY), (2, A, A), (P, 4)]
        self.guard = guard
        self.buf = torch.full((sum(self.sizes) + 4 * guard,), SENTINEL, dtype=torch.int64, device="cuda")
        self.views, off = [], guard
        for n in self.sizes:
            self.views.append(self.buf[off:off + n])
            self.views[-1].zero_()
            off += n + guard
        st = _native.VisitsState()
        st.pos_hist, st.act_hist, st.counters = (v.data_ptr() for v in self.views)
        st.GX, st.GY, st.A, st.n_maps = GX, GY, A, n_maps
        (st.x0, st.x1), (st.y0, st.y1), (st.a0, st.a1) = xr, yr, ar
        self.st = st

    def read(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        out, off, inside = [], self.guard, np.zeros(len(b), dtype=bool)
        for n, shp in zip(self.sizes, self.shapes):
            out.append(b[off:off + n].reshape(shp).copy())
            inside[off:off + n] = True
            off += n + self.guard
        assert np.all(b[~inside] == SENTINEL), "a write outside the tables"
        return out


class Step:
    def __init__(self, x, use_map=True, use_sel=True, until=UNTIL):
        from multi_agent_aac_amd import _native
        self.t = {k: torch.from_numpy(np.ascontiguousarray(x[k])).cuda() for k in ("pos", "act", "episode", "map_idx", "sel")}
        p = _native.VisitsStep()
        p.pos, p.act, p.episode = (self.t[k].data_ptr() for k in ("pos", "act", "episode"))
        p.map_idx = self.t["map_idx"].data_ptr() if use_map else None
        p.sel = self.t["sel"].data_ptr() if use_sel else None
        p.act_f64 = int(x["act"].dtype == np.float64)
        p.E, p.N = x["pos"].shape[:2]
        p.explore_until = until
        self.p = p


def launch(lib, tab, step):
    rc = lib.aac_visits_accumulate(ctypes.byref(tab.st), ctypes.byref(step.p), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib.aac_visits_last_error())


def check(tab, ref):
    pos, act, cnt = tab.read()
    assert np.array_equal(cnt, ref.cnt), (cnt.tolist(), ref.cnt.tolist())
    assert np.array_equal(act, ref.act)
    assert np.array_equal(pos, ref.pos)
    return pos, act, cnt


@pytest.mark.parametrize("name", sorted(CASES))
def test_two_calls_equal_the_restatement(native_lib, name):
    E, N, f64, n_maps, GX, GY, A = CASES[name]
    xs, ref = reference(name)
    tab = Tables(n_maps, GX, GY, A, xs[0]["xr"], xs[0]["yr"])
    steps = [Step(x) for x in xs]
    launch(native_lib, tab, steps[0])
    first = tab.read()[2].copy()
    launch(native_lib, tab, steps[1])
    pos, act, cnt = check(tab, ref)
    assert first[:, 0].sum() == int(xs[0]["sel"].astype(bool)[(xs[0]["map_idx"] >= 0) & (xs[0]["map_idx"] < n_maps)].sum()) * N
    # samples == the selected rows of a valid map; every sample is in a position bin or in pos_outside
    good = sum(int(((x["sel"] != 0) & (x["map_idx"] >= 0) & (x["map_idx"] < n_maps)).sum()) for x in xs) * N
    bad = sum(int(((x["sel"] != 0) & ((x["map_idx"] < 0) | (x["map_idx"] >= n_maps))).sum()) for x in xs) * N
    assert cnt[:, 0].sum() == good and cnt[0, 3] == bad and np.all(cnt[1:, 3] == 0)
    assert np.array_equal(pos.sum(axis=(1, 2)) + cnt[:, 1], cnt[:, 0])
    assert act.sum() + cnt[:, 2].sum() == good
    if E * N >= CHUNK - 1:      # the case exercises what it is for
        assert cnt[:, 1].sum() > 0 and cnt[:, 2].sum() > 0
        assert (pos[:, -1, :].sum() > 0 or GX > 64) and act[0].sum() > 0 and act[1].sum() > 0
        assert n_maps == 1 or bad > 0


@pytest.mark.parametrize("name", ["chunk_p1_n5", "chunk_n16"])
def test_null_map_idx_and_sel(native_lib, name):
    """map_idx NULL: every row in map 0; sel NULL: every env."""
    E, N, f64, n_maps, GX, GY, A = CASES[name]
    xs, ref = reference(name, calls=1, use_map=False, use_sel=False)
    tab = Tables(n_maps, GX, GY, A, xs[0]["xr"], xs[0]["yr"])
    launch(native_lib, tab, Step(xs[0], use_map=False, use_sel=False))
    pos, act, cnt = check(tab, ref)
    assert cnt[:, 0].sum() == E * N and cnt[2:].sum() == 0 and pos[2:].sum() == 0


def test_explore_until_boundary(native_lib):
    """episode == explore_until is the last "explore" episode, explore_until + 1 the first "exploit" one."""
    E, N = 6, 3
    x = dict(pos=np.tile(np.float64([500.0, 300.0]), (E, N, 1)), act=np.zeros((E, N, 2), dtype=np.float32),
             episode=np.int32([UNTIL, UNTIL + 1, UNTIL, UNTIL - 1, UNTIL + 1, 2 ** 31 - 1]),
             map_idx=np.zeros(E, dtype=np.int32), sel=np.ones(E, dtype=np.uint8))
    tab = Tables(1, 50, 50, 20, XR, YR)
    launch(native_lib, tab, Step(x))
    pos, act, cnt = tab.read()
    assert cnt[:, 0].tolist() == [3 * N, 3 * N] and act.sum(axis=(1, 2)).tolist() == [3 * N, 3 * N]
    assert pos.sum(axis=(1, 2)).tolist() == [3 * N, 3 * N] and pos[0, 10, 17] == 3 * N


@pytest.mark.parametrize("f64", [False, True])
def test_all_rows_in_one_bin(native_lib, f64):
    """4096 rows in one position bin and one action bin: no update is lost."""
    E, N = 1024, 4
    x = dict(pos=np.tile(np.float64([679.0, 256.0]), (E, N, 1)),
             act=np.tile(np.array([1.0, -1.0], dtype=np.float64 if f64 else np.float32), (E, N, 1)),
             episode=np.ones(E, dtype=np.int32), map_idx=np.zeros(E, dtype=np.int32), sel=np.ones(E, dtype=np.uint8))
    tab = Tables(1, 50, 50, 20, XR, YR)
    st = Step(x)
    for _ in range(3):
        launch(native_lib, tab, st)
    pos, act, cnt = tab.read()
    assert pos[0, 49, 0] == 3 * E * N == pos.sum() and act[0, 19, 0] == 3 * E * N == act.sum()
    assert cnt.tolist() == [[3 * E * N, 0, 0, 0], [0, 0, 0, 0]]


def test_planes_past_the_lds_counter_table(native_lib):
    """140 maps: the counters of planes >= 128 are added by the waves directly."""
    E, N, n_maps = 700, 3, 140
    rng = np.random.default_rng(5)
    x = dict(pos=np.stack([rng.uniform(440, 690, (E, N)), rng.uniform(250, 390, (E, N))], axis=-1),
             act=rng.uniform(-1.1, 1.1, (E, N, 2)).astype(np.float32),
             episode=rng.integers(UNTIL - 1, UNTIL + 3, E).astype(np.int32),
             map_idx=(np.arange(E) % n_maps).astype(np.int32), sel=np.ones(E, dtype=np.uint8))
    ref = visits_ref.VisitsRef(n_maps, 5, 4, 20, XR, YR)
    ref.accumulate(x["pos"], x["act"], x["episode"], UNTIL, x["map_idx"], x["sel"])
    tab = Tables(n_maps, 5, 4, 20, XR, YR)
    launch(native_lib, tab, Step(x))
    _, _, cnt = check(tab, ref)
    assert cnt[128:, 0].sum() > 0 and cnt[128:, 1].sum() > 0 and cnt[128:, 2].sum() > 0


def test_graph_replays_equal_eager_calls(native_lib):
    name, k = "3chunk_p5_n17", 3
    E, N, f64, n_maps, GX, GY, A = CASES[name]
    x = gen(name)
    eager, graph = (Tables(n_maps, GX, GY, A, x["xr"], x["yr"]) for _ in range(2))
    st = Step(x)
    for _ in range(k):
        launch(native_lib, eager, st)
    want = eager.read()
    torch.cuda.synchronize()
    from multi_agent_aac_amd import graphs
    g = torch.cuda.CUDAGraph()
    with graphs.capture(g):
        launch(native_lib, graph, st)
    assert all(int(t.sum()) == 0 for t in graph.read())       # nothing ran during the capture
    for _ in range(k):
        g.replay()
    got = graph.read()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert want[2][:, 0].sum() > 0


def test_invalid_arguments_launch_nothing(native_lib):
    from multi_agent_aac_amd import _native
    x = gen("chunk_p1_n5")
    nan = float("nan")

    def attempt(what, st_edit=None, p_edit=None, null=None):
        tab = Tables(3, 50, 50, 20, XR, YR)
        step = Step(x)
        if st_edit:
            st_edit(tab.st)
        if p_edit:
            p_edit(step.p)
        a = None if null == "state" else ctypes.byref(tab.st)
        b = None if null == "step" else ctypes.byref(step.p)
        rc = native_lib.aac_visits_accumulate(a, b, torch.cuda.current_stream().cuda_stream)
        msg = native_lib.aac_visits_last_error().decode()
        assert rc < 0 and msg.startswith("visits_accumulate:") and len(msg) > 20, (what, rc, msg)
        assert all(int(t.sum()) == 0 for t in tab.read()), what

    def setter(**kw):
        return lambda s: [setattr(s, k, v) for k, v in kw.items()]
    for what, edit in [("GX 0", setter(GX=0)), ("GY -1", setter(GY=-1)), ("GX too large", setter(GX=65537)),
                       ("A 0", setter(A=0)), ("A 33", setter(A=33)), ("n_maps 0", setter(n_maps=0)),
                       ("x empty", setter(x0=680.0)), ("x reversed", setter(x0=700.0)), ("y empty", setter(y1=255.0)),
                       ("a empty", setter(a0=1.0)), ("x nan", setter(x0=nan)), ("y inf", setter(y1=float("inf"))),
                       ("a overflow", setter(a0=-1.7e308, a1=1.7e308)),
                       ("null pos_hist", setter(pos_hist=None)), ("null act_hist", setter(act_hist=None)),
                       ("null counters", setter(counters=None))]:
        attempt(what, st_edit=edit)
    for what, edit in [("E 0", setter(E=0)), ("N 0", setter(N=0)), ("E * N overflow", setter(E=2 ** 31 - 1, N=2)),
                       ("null pos", setter(pos=None)), ("null act", setter(act=None)), ("null episode", setter(episode=None)),
                       ("pos alignment", lambda p: setattr(p, "pos", p.pos + 8)),
                       ("act alignment", lambda p: setattr(p, "act", p.act + 4))]:
        attempt(what, p_edit=edit)
    attempt("null state", null="state")
    attempt("null step", null="step")
    assert ctypes.sizeof(_native.VisitsState) == 88
