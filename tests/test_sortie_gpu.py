"""The sortie statistics' raw entries (aac_sortie_accumulate / aac_sortie_reduce, include/aac_sortie.h) on
synthetic inputs, against the plain-Python restatement (tests/sortie_ref.py).

Shapes: a workgroup owns EPW = 32 consecutive envs and a wave holds 64 / AP envs side by side (AP the
power of two >= N), so the cases are one lane (1, 1), two and three envs of a wave (3, 2), (7, 5: AP = 8
with idle lanes), one env past a workgroup at four envs a wave (EPW + 1, 16), and one env short of two
workgroups at one env a wave (2 EPW - 1, 64).  Every case plays 30 calls of random positions with
scripted episodes of 1 to 12 steps (episode_length 10: 11 is a timeout), random mask bits in both bit
layouts (aac_env.h and aac_uam.h), collisions, start == goal (a degenerate ratio), a 1e200 jump (a flown
length that is not finite), per-env quotas that stop some envs early, and a log ring shorter than the rows
of one call; the histogram is also run at the limit of the workgroup's LDS table and one past it.  Counters, collide_hist, running state and log rows are compared bit for bit; the six double
sums within n * 2^-52 relative (n summands: the bound of a reordered sum of same-signed terms); min / max
exactly.  All buffers are slices of one sentinel-filled allocation."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sortie_ref

pytestmark = pytest.mark.gpu

EPW = 32
EP_LEN = 10
CALLS = 30
LOG = 50
SENT = 0xA5
#         E            N   bits   margin
CASES = {"e1_n1": (1, 1, "env", 0.0),
         "e3_n2": (3, 2, "uam", 5.0),
         "e7_n5": (7, 5, "env", 5.0),
         "epw_p1_n16": (EPW + 1, 16, "uam", 5.0),
         "2epw_m1_n64": (2 * EPW - 1, 64, "env", 0.25)}
BITS = {"env": sortie_ref.BITS_ENV, "uam": sortie_ref.BITS_UAM}


@functools.lru_cache(maxsize=None)
def gen(name):
    """The inputs of every call of a case (numpy), the quota and the per-call episode counters."""
    E, N, layout, _ = CASES[name]
    rng = np.random.default_rng([len(name), E, N])
    bits = BITS[layout]
    start, goal = rng.uniform(0, 40, (E, N, 2)), rng.uniform(0, 40, (E, N, 2))
    left = rng.integers(1, 13, E)          # steps left in the running episode
    episode = rng.integers(1, 500, E).astype(np.int32)
    calls = []
    for c in range(CALLS):
        pos = rng.uniform(0, 40, (E, N, 2))
        pos[rng.random((E, N)) < 0.01, 0] = 1e200          # dx * dx overflows: the flown length is inf
        parked = rng.random((E, N)) < 0.1
        if calls:
            pos[parked] = calls[-1]["pos"][parked]
        mask = np.zeros((E, N), dtype=np.uint8)
        for b in range(8):
            p = 0.15 if b == bits["goal_bit"] else 0.03
            mask |= ((rng.random((E, N)) < p).astype(np.uint8) << b).astype(np.uint8)
        left -= 1
        env_done = (left == 0).astype(np.uint8)
        done = ((rng.random((E, N)) < 0.2) & (env_done[:, None] != 0)).astype(np.uint8)
        calls.append(dict(pos=pos, start=start.copy(), goal=goal.copy(), done=done, mask=mask, env_done=env_done,
                          episode=episode.copy()))
        for e in np.nonzero(env_done)[0]:      # the next episode's OD; now and then start == goal
            start[e], goal[e] = rng.uniform(0, 40, (N, 2)), rng.uniform(0, 40, (N, 2))
            same = rng.random(N) < 0.1
            goal[e][same] = start[e][same]
            left[e] = rng.integers(1, 13)
            episode[e] += 1
    quota = rng.integers(1, 5, E).astype(np.int32)
    if E > 1:
        quota[0] = 1000
    return calls, quota


@functools.lru_cache(maxsize=None)
def reference(name, use_quota=True, use_episode=True, ep_len=EP_LEN):
    E, N, layout, margin = CASES[name]
    calls, quota = gen(name)
    ref = sortie_ref.SortieRef(E, N, ep_len, margin, **BITS[layout])
    for x in calls:
        ref.accumulate(x["pos"], x["start"], x["goal"], x["done"], x["mask"], x["env_done"],
                       quota if use_quota else None, x["episode"] if use_episode else None)
    return ref


class State:
    """Every buffer of aac_sortie_state and the totals record as 256-byte-aligned slices of one
    sentinel-filled byte tensor, a guard band either side of each."""

    def __init__(self, E, N, log=LOG, guard=512, ep_len=EP_LEN):
        from multi_agent_aac_amd import _native
        from multi_agent_aac_amd.sorties import FIELDS, ROW
        G = (E + EPW - 1) // EPW
        self.E, self.N, self.L = E, N, log
        spec = [("straight", np.float64, (E, N)), ("first_seg", np.float64, (E, N)), ("run_dist", np.float64, (E, N)),
                ("last_pos", np.float64, (E, N, 2)), ("run_flags", np.uint8, (E, N)), ("reach_step", np.int32, (E, N)),
                ("run_len", np.int32, (E,)), ("ep_count", np.int32, (E,)), ("slots", np.int64, (G, FIELDS)),
                ("collide_hist", np.int64, (ep_len + 2,)), ("totals", np.int64, (FIELDS,))]
        if log:
            spec += [("log", ROW, (log,)), ("log_meta", np.int64, (2,)), ("fin_flag", np.uint8, (E,)),
                     ("fin_row", ROW, (E * N,)), ("fin_list", np.int32, (E + 1,))]
        self.spec, self.off, off = spec, {}, guard
        for k, dt, shp in spec:
            self.off[k] = off
            off += (int(np.prod(shp)) * np.dtype(dt).itemsize + 255) // 256 * 256 + guard
        self.buf = torch.full((off,), SENT, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 256 == 0
        for k, dt, shp in spec:
            self.buf[self.off[k]:self.off[k] + int(np.prod(shp)) * np.dtype(dt).itemsize].zero_()
        n = G * FIELDS * 8
        sl = self.buf[self.off["slots"]:self.off["slots"] + n].view(torch.float64).view(G, FIELDS)
        sl[:, 11], sl[:, 12] = float("inf"), float("-inf")      # ratio_min, ratio_max of an empty slot
        st = _native.SortieState()
        base = self.buf.data_ptr()
        for k, _, _ in spec:
            if k != "totals":
                setattr(st, k, base + self.off[k])
        st.hist_len, st.log_len = ep_len + 2, log
        self.st, self.totals_ptr = st, base + self.off["totals"]

    def read(self):
        torch.cuda.synchronize()
        b = self.buf.cpu().numpy()
        out, inside = {}, np.zeros(len(b), dtype=bool)
        for k, dt, shp in self.spec:
            n = int(np.prod(shp)) * np.dtype(dt).itemsize
            out[k] = b[self.off[k]:self.off[k] + n].view(dt).reshape(shp).copy()
            inside[self.off[k]:self.off[k] + n] = True
        assert np.all(b[~inside] == SENT), "a write outside the state's buffers"
        return out

    def log_rows(self, out):
        n, rows = int(out["log_meta"][0]), out["log"]
        return rows[:n] if n <= self.L else np.roll(rows, -(n % self.L))


class Step:
    def __init__(self, name, x, quota, use_episode=True, ep_len=EP_LEN):
        from multi_agent_aac_amd import _native
        E, N, layout, margin = CASES[name]
        self.t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in x.items()}
        self.t["quota"] = quota
        p = _native.SortieStep()
        for k in ("pos", "start", "goal", "done", "mask", "env_done"):
            setattr(p, k, self.t[k].data_ptr())
        p.episode = self.t["episode"].data_ptr() if use_episode else None
        p.quota = None if quota is None else quota.data_ptr()
        p.E, p.N, p.episode_length, p.reach_margin = E, N, ep_len, margin
        for k, v in BITS[layout].items():
            setattr(p, k, v)
        self.p = p


def steps_of(name, use_quota=True, use_episode=True, ep_len=EP_LEN):
    calls, quota = gen(name)
    q = torch.from_numpy(quota).cuda() if use_quota else None
    return [Step(name, x, q, use_episode, ep_len) for x in calls]


def launch(lib, state, step):
    rc = lib.aac_sortie_accumulate(ctypes.byref(state.st), ctypes.byref(step.p), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib.aac_sortie_last_error())


def reduce(lib, state, clear=0):
    rc = lib.aac_sortie_reduce(ctypes.byref(state.st), state.E, ctypes.c_void_p(state.totals_ptr), clear,
                               torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (rc, lib.aac_sortie_last_error())


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check(state, out, ref):
    from multi_agent_aac_amd.sorties import COUNTERS, DOUBLES
    tot = out["totals"]
    got = {k: int(tot[i]) for i, k in enumerate(COUNTERS)}
    assert got == ref.cnt, (got, ref.cnt)
    assert np.array_equal(out["collide_hist"], ref.collide_hist), (out["collide_hist"], ref.collide_hist)
    for k, v in ref.running().items():
        assert same_bits(out[k], v.astype(out[k].dtype)), k
    want, n = ref.sums()
    d = tot.view(np.float64)
    for i, k in enumerate(DOUBLES):
        g, w = float(d[len(COUNTERS) + i]), want[k]
        print(f"{k}: got {g!r} want {w!r} n {n}")
        if k in ("ratio_min", "ratio_max"):
            assert g == w, (k, g, w)
        else:
            assert abs(g - w) <= n * 2.0 ** -52 * abs(w), (k, g, w, n)
    assert n == got["reached"] - got["degenerate"]
    if state.L:
        rows, wr = state.log_rows(out), ref.log_rows(state.L)
        assert int(out["log_meta"][0]) == len(ref.rows) and int(out["log_meta"][1]) == CALLS
        assert rows.dtype == wr.dtype and same_bits(rows, wr), [(a, b) for a, b in zip(rows, wr) if a.tobytes() != b.tobytes()][:3]


@pytest.mark.parametrize("name", sorted(CASES))
def test_calls_equal_the_restatement(native_lib, name):
    E, N, layout, margin = CASES[name]
    ref = reference(name)
    state, steps = State(E, N), steps_of(name)
    for s in steps:
        launch(native_lib, state, s)
    reduce(native_lib, state)
    out = state.read()
    check(state, out, ref)
    c = ref.cnt
    assert c["sorties"] == N * c["episodes"] == sum(c[k] for k in sortie_ref.CLASSES) > 0
    if E >= EPW:       # the case exercises what it is for
        assert all(c[k] > 0 for k in sortie_ref.CLASSES) and c["degenerate"] > 0 and ref.collide_hist.sum() > 0
        assert len(ref.rows) > LOG and c["reached"] > c["degenerate"]
        _, quota = gen(name)
        assert np.any(ref.ep_count == quota) and np.any(ref.ep_count < quota)
    # a second run gives the same bytes, the doubles included
    again = State(E, N)
    for s in steps:
        launch(native_lib, again, s)
    reduce(native_lib, again)
    out2 = again.read()
    for k in out:
        assert same_bits(out[k], out2[k]), k


@pytest.mark.parametrize("name", ["e7_n5", "epw_p1_n16"])
def test_no_quota_no_episode_no_log(native_lib, name):
    """quota NULL: every env counts on; episode NULL: the rows carry ep_count; log NULL: one launch."""
    E, N, layout, margin = CASES[name]
    ref = reference(name, use_quota=False, use_episode=False)
    state, nolog = State(E, N), State(E, N, log=0)
    for s in steps_of(name, use_quota=False, use_episode=False):
        launch(native_lib, state, s)
        launch(native_lib, nolog, s)
    reduce(native_lib, state)
    reduce(native_lib, nolog)
    out, out0 = state.read(), nolog.read()
    check(state, out, ref)
    check(nolog, out0, ref)
    assert same_bits(out["totals"], out0["totals"]) and same_bits(out["slots"], out0["slots"])


@pytest.mark.parametrize("ep_len", [2046, 2047])
def test_histogram_at_the_lds_table_limit(native_lib, ep_len):
    """A workgroup gathers its collide_hist adds in a 2048-bin LDS table: hist_len 2048 is the last that
    fits, 2049 takes its adds in global memory.  No episode is a timeout here: every ending with a done
    flag is counted."""
    name = "epw_p1_n16"
    E, N, layout, margin = CASES[name]
    ref = reference(name, ep_len=ep_len)
    state = State(E, N, ep_len=ep_len)
    for s in steps_of(name, ep_len=ep_len):
        launch(native_lib, state, s)
    reduce(native_lib, state)
    check(state, state.read(), ref)
    assert ref.collide_hist.sum() > reference(name).collide_hist.sum() and ref.collide_hist[11:13].sum() > 0


def test_graph_replay_equals_eager_calls(native_lib):
    name = "epw_p1_n16"
    E, N, layout, margin = CASES[name]
    eager, graph = State(E, N), State(E, N)
    steps = steps_of(name)
    for s in steps:
        launch(native_lib, eager, s)
    reduce(native_lib, eager)
    want = eager.read()
    from multi_agent_aac_amd import graphs
    g = torch.cuda.CUDAGraph()
    with graphs.capture(g):
        for s in steps:
            launch(native_lib, graph, s)
        reduce(native_lib, graph)
    idle = graph.read()
    assert int(idle["ep_count"].sum()) == 0 and int(idle["log_meta"].sum()) == 0     # nothing ran during the capture
    g.replay()
    got = graph.read()
    for k in want:
        assert same_bits(got[k], want[k]), k
    assert int(want["totals"][0]) > 0


def test_reduce_clear_empties_slots_and_histogram(native_lib):
    name = "2epw_m1_n64"
    E, N, layout, margin = CASES[name]
    state = State(E, N)
    for s in steps_of(name):
        launch(native_lib, state, s)
    reduce(native_lib, state, clear=1)
    out = state.read()
    check(state, dict(out, collide_hist=reference(name).collide_hist), reference(name))
    assert int(out["collide_hist"].sum()) == 0
    fresh = State(E, N).read()
    assert same_bits(out["slots"], fresh["slots"])
    reduce(native_lib, state)
    tot = state.read()["totals"]
    assert tot[:9].tolist() == [0] * 9 and tot.view(np.float64)[9:].tolist() == [0.0, 0.0, np.inf, -np.inf, 0.0, 0.0]


def test_invalid_arguments_launch_nothing(native_lib):
    name = "e7_n5"
    E, N, layout, margin = CASES[name]
    calls, quota = gen(name)
    x = next(c for c in calls if c["env_done"].any())

    def attempt(what, st_edit=None, p_edit=None, null=None, fn="accumulate"):
        state, step = State(E, N), Step(name, x, None)
        before = state.read()
        if st_edit:
            st_edit(state.st)
        if p_edit:
            p_edit(step.p)
        a = None if null == "state" else ctypes.byref(state.st)
        b = None if null == "step" else ctypes.byref(step.p)
        stream = torch.cuda.current_stream().cuda_stream
        if fn == "accumulate":
            rc = native_lib.aac_sortie_accumulate(a, b, stream)
        else:
            rc = native_lib.aac_sortie_reduce(a, step.p.E, None if null == "totals" else ctypes.c_void_p(state.totals_ptr),
                                              0, stream)
        msg = native_lib.aac_sortie_last_error().decode()
        assert rc == -1 and msg.startswith("sortie_" + fn + ":") and len(msg) > len("sortie_accumulate: "), (what, rc, msg)      # AAC_E_INVALID
        after = state.read()
        for k in before:
            assert same_bits(before[k], after[k]), (what, k)

    def setter(**kw):
        return lambda s: [setattr(s, k, v) for k, v in kw.items()]
    for k in ("straight", "first_seg", "run_dist", "last_pos", "run_flags", "reach_step", "run_len", "ep_count", "slots",
              "collide_hist", "log_meta", "fin_flag", "fin_row", "fin_list"):
        attempt("null " + k, st_edit=setter(**{k: None}))
    for what, edit in [("hist_len short", setter(hist_len=EP_LEN + 1)), ("hist_len 0", setter(hist_len=0)),
                       ("log_len 0", setter(log_len=0)), ("log_len -1", setter(log_len=-1))]:
        attempt(what, st_edit=edit)
    for k in ("pos", "start", "goal", "done", "mask", "env_done"):
        attempt("null " + k, p_edit=setter(**{k: None}))
    for what, edit in [("E 0", setter(E=0)), ("E -1", setter(E=-1)), ("N 0", setter(N=0)), ("N 65", setter(N=65)),
                       ("E * N overflow", setter(E=2 ** 31 - 1, N=2)), ("episode_length 0", setter(episode_length=0)),
                       ("episode_length past hist_len", setter(episode_length=EP_LEN + 1)),
                       ("bound_bit 8", setter(bound_bit=8)), ("obstacle_bit -1", setter(obstacle_bit=-1)),
                       ("drone_bit 8", setter(drone_bit=8)), ("goal_bit 9", setter(goal_bit=9)),
                       ("margin nan", setter(reach_margin=float("nan"))), ("margin inf", setter(reach_margin=float("inf")))]:
        attempt(what, p_edit=edit)
    attempt("null state", null="state")
    attempt("null step", null="step")
    attempt("reduce: null state", null="state", fn="reduce")
    attempt("reduce: null totals", null="totals", fn="reduce")
    attempt("reduce: E 0", p_edit=setter(E=0), fn="reduce")
    attempt("reduce: null slots", st_edit=setter(slots=None), fn="reduce")
