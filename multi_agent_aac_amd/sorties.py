"""Sortie statistics on the device (include/aac_sortie.h): the reference's evaluation "by sortie"
(``evaluation_by_episode = False``, UAM/main:1130-1144, :1194-1200), kept beside a loop that never
leaves the GPU.  Every aircraft of every finished episode lands in one class -- crashed into the bound,
into an obstacle, into another aircraft, reached its destination, idle -- and the aircraft that reached
their goals add their flight-distance ratio (``obtain_euclidean_dist_list_all_AC``, UAM/util:53-68:
flown path length over the straight origin-destination distance; mean and std printed at
UAM/main:1191-1193).  ``collide_hist`` is the histogram of ``steps_before_collide`` (UAM/main:360, :1073).

``SortieStats.accumulate(bufs)`` is one small launch (two with a log) on torch's current stream, after the
env step launch and BEFORE the auto-reset of that step: it reads the env's live post-step positions, so
the fused ``step_tail`` (which resets inside the step launch) leaves nothing to call it on.  It may be
captured in a HIP graph with the step.  Everything the kernels write is a torch tensor this object owns
(``tensors()``), so a resumed run continues its tallies exactly.  With several ranks each rank keeps
its own.

Classes and the reference's printed lines:
  bound      "Collision to bound"         obstacle   "Collision to building" / cloud, runway (UAM)
  drone      "Collision to drones"        reached    "Destination reached"       idle   "Idle UAV"
One known difference, stated rather than imitated: the UAM reference's sortie loop tests
``building_collision``, which ``ss_reward_Mar_changeskin`` never sets, so its cloud / runway conflicts
fall through to reached / idle.  Here they are the ``obstacle`` class.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native

EPW = 32              # AAC_SORTIE_EPW: envs per workgroup (= per slot)
FIELDS = 15           # AAC_SORTIE_FIELDS
CLASSES = ("bound", "obstacle", "drone", "reached", "idle")
COUNTERS = ("sorties",) + CLASSES + ("degenerate", "episodes", "reach_step_sum")
DOUBLES = ("ratio_sum", "ratio_sqsum", "ratio_min", "ratio_max", "flown_sum", "straight_sum")
F_MIN, F_MAX = 11, 12
BITS = {"env": dict(bound_bit=0, drone_bit=1, obstacle_bit=3, goal_bit=5),     # aac_env.h mask bits
        "uam": dict(bound_bit=0, obstacle_bit=1, drone_bit=2, goal_bit=4)}     # aac_uam.h
ROW = np.dtype([("env", "<i4"), ("agent", "<i4"), ("episode", "<i4"), ("cls", "<i4"), ("len", "<i4"),
                ("reach_step", "<i4"), ("flown", "<f8"), ("straight", "<f8"), ("ratio", "<f8")])   # aac_sortie_row
assert ROW.itemsize == 48 and len(COUNTERS) + len(DOUBLES) == FIELDS


class SortieStats:
    """Per-aircraft running state + totals for the E envs x N aircraft of a ``BatchedEnv`` (``for_env``)
    or a ``BatchedUAM`` (``for_uam``).

    log            > 0: keep the last ``log`` finished sorties as rows, in (call, env, aircraft) order
    reach_margin   added to the flown length of a sortie (the reference's UAM code adds 5: reaching the
                   protective zone counts as reaching the goal)
    """

    def __init__(self, env, log=0, reach_margin=0.0):
        from .uam import BatchedUAM
        self.env, self.uam = env, isinstance(env, BatchedUAM)
        self.E, self.N = int(env.E), int(env.N)
        if not 1 <= self.N <= 64:
            raise ValueError("SortieStats: 1 <= N <= 64")
        self.episode_length = int(env.cfg.episode_length)
        self.reach_margin = float(reach_margin)
        if not math.isfinite(self.reach_margin):
            raise ValueError("SortieStats: reach_margin must be finite")
        self.bits = BITS["uam" if self.uam else "env"]
        self.L = int(log)
        d = self.device = env.device
        E, N, G = self.E, self.N, (self.E + EPW - 1) // EPW
        f64, i32, i64 = (dict(dtype=t, device=d) for t in (torch.float64, torch.int32, torch.int64))
        self.straight, self.first_seg, self.run_dist = (torch.zeros(E, N, **f64) for _ in range(3))
        self.last_pos = torch.zeros(E, N, 2, **f64)
        self.run_flags = torch.zeros(E, N, dtype=torch.uint8, device=d)
        self.reach_step = torch.zeros(E, N, **i32)
        self.run_len, self.ep_count = torch.zeros(E, **i32), torch.zeros(E, **i32)
        self.slots = torch.zeros(G, FIELDS, **i64)
        self.collide_hist = torch.zeros(self.episode_length + 2, **i64)
        self.totals = torch.zeros(FIELDS, **i64)
        self.quota = torch.zeros(E, **i32)              # used by accumulate(quota=<int>)
        self.log = self.log_meta = None
        st = _native.SortieState()
        for k in ("straight", "first_seg", "run_dist", "last_pos", "run_flags", "reach_step", "run_len", "ep_count",
                  "slots", "collide_hist"):
            setattr(st, k, getattr(self, k).data_ptr())
        st.hist_len = self.episode_length + 2
        if self.L:
            self.log = torch.zeros(self.L, ROW.itemsize, dtype=torch.uint8, device=d)
            self.log_meta = torch.zeros(2, **i64)
            self._fin = (torch.zeros(E, dtype=torch.uint8, device=d),
                         torch.zeros(E * N, ROW.itemsize, dtype=torch.uint8, device=d), torch.zeros(E + 1, **i32))
            st.log, st.log_len, st.log_meta = self.log.data_ptr(), self.L, self.log_meta.data_ptr()
            st.fin_flag, st.fin_row, st.fin_list = (t.data_ptr() for t in self._fin)
        self._st, self._st_ref = st, ctypes.byref(st)
        L = _native.lib()
        self._call = L.aac_uam_sorties if self.uam else L.aac_env_sorties
        self._err = L.aac_uam_last_error if self.uam else L.aac_last_error
        self._steps = {}        # id(bufs), quota pointer -> SortieStep
        self.reset()

    @classmethod
    def for_env(cls, env, log=0, reach_margin=0.0):
        """For a ``BatchedEnv`` (att or wgru): bound bit 0, drone 1, building 3 (``obstacle``), goal 5."""
        from .uam import BatchedUAM
        if isinstance(env, BatchedUAM):
            raise TypeError("SortieStats.for_env: a BatchedUAM takes SortieStats.for_uam")
        return cls(env, log, reach_margin)

    @classmethod
    def for_uam(cls, env, log=0, reach_margin=5.0):
        """For a ``BatchedUAM``: bound bit 0, cloud / runway 1 (``obstacle``), drone 2, goal 4; the
        reference's margin of 5 (UAM/util:66)."""
        from .uam import BatchedUAM
        if not isinstance(env, BatchedUAM):
            raise TypeError("SortieStats.for_uam: not a BatchedUAM")
        return cls(env, log, reach_margin)

    # ------------------------------------------------------------------- state
    def reset(self):
        """Empty totals, running state, episode counts, histogram and log."""
        for t in (self.straight, self.first_seg, self.run_dist, self.last_pos, self.run_flags, self.reach_step,
                  self.run_len, self.ep_count, self.slots, self.collide_hist):
            t.zero_()
        sd = self.slots.view(torch.float64)
        sd[:, F_MIN] = math.inf
        sd[:, F_MAX] = -math.inf
        if self.L:
            self.log.zero_()
            self.log_meta.zero_()

    def tensors(self):
        """Everything the kernels write that a checkpoint must carry (loaded in place)."""
        t = {k: getattr(self, k) for k in ("straight", "first_seg", "run_dist", "last_pos", "run_flags", "reach_step",
                                           "run_len", "ep_count", "slots", "collide_hist")}
        if self.L:
            t["log"], t["log_meta"] = self.log, self.log_meta
        return t

    # ------------------------------------------------------------------- calls
    def accumulate(self, bufs, quota=None):
        """Tally the step whose outputs are in ``bufs`` (a ``StepBuffers`` / ``UamBuffers``: done, mask,
        env_done), after the env step launch and before the auto-reset, on the same stream.  ``quota``:
        int32 [E] tensor (or an int, kept in ``self.quota``): an env with that many finished episodes
        contributes nothing more.  A buffer set's tensors are taken as fixed: its launch arguments are
        built on the first call."""
        if isinstance(quota, int):
            self.quota.fill_(quota)
            quota = self.quota
        key = (id(bufs), None if quota is None else quota.data_ptr())
        hit = self._steps.get(key)
        if hit is None or hit[0] is not bufs:
            for name, shape in (("done", (self.E, self.N)), ("mask", (self.E, self.N)), ("env_done", (self.E,))):
                t = getattr(bufs, name)
                if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                    raise ValueError(f"{name} {tuple(t.shape)} {t.dtype}: expected {shape} uint8 on {self.device}")
            if quota is not None and (quota.dtype != torch.int32 or tuple(quota.shape) != (self.E,)
                                      or not quota.is_contiguous()):
                raise ValueError("quota: int32 [E]")
            p = _native.SortieStep()
            p.done, p.mask, p.env_done = bufs.done.data_ptr(), bufs.mask.data_ptr(), bufs.env_done.data_ptr()
            p.quota = None if quota is None else quota.data_ptr()
            p.E, p.N, p.episode_length = self.E, self.N, self.episode_length
            for k, v in self.bits.items():
                setattr(p, k, v)
            p.reach_margin = self.reach_margin
            if len(self._steps) > 64:
                self._steps.clear()
            hit = self._steps[key] = (bufs, ctypes.byref(p), quota, p)
        rc = self._call(self.env._h, self._st_ref, hit[1], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aac_sortie_accumulate failed ({rc}): {self._err().decode(errors='replace')}")

    def read(self, clear=False):
        """Totals as a dict of numpy / Python values (synchronises): the counters (``sorties``, the five
        classes, ``degenerate``, ``episodes``, ``reach_step_sum``), ``collide_hist`` (int64
        [episode_length + 2], indexed by the length of the colliding episode), the sums, ``ratio_mean`` /
        ``ratio_std`` (population, as ``np.mean`` / ``np.std`` of the reference's flight-ratio list; NaN
        while no sortie is counted), ``ratio_min`` / ``ratio_max`` and ``mean_reach_step``.  ``clear``
        empties the totals and the histogram afterwards (a per-window report); running episodes carry on."""
        hist = self.collide_hist.cpu().numpy()      # before the reduce launch, which clears it
        rc = _native.lib().aac_sortie_reduce(self._st_ref, self.E, ctypes.c_void_p(self.totals.data_ptr()),
                                             int(bool(clear)), torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            msg = _native.lib().aac_sortie_last_error().decode(errors="replace")
            raise RuntimeError(f"aac_sortie_reduce failed ({rc}): {msg}")
        raw = self.totals.cpu().numpy()
        out = {k: int(raw[i]) for i, k in enumerate(COUNTERS)}
        d = raw.view(np.float64)
        for i, k in enumerate(DOUBLES):
            out[k] = float(d[len(COUNTERS) + i])
        out["collide_hist"] = hist
        n = out["reached"] - out["degenerate"]
        if not n:
            out["ratio_min"] = out["ratio_max"] = math.nan
        mean = out["ratio_sum"] / n if n else math.nan
        out["ratio_mean"] = mean
        out["ratio_std"] = math.sqrt(max(out["ratio_sqsum"] / n - mean * mean, 0.0)) if n else math.nan
        out["mean_reach_step"] = out["reach_step_sum"] / out["reached"] if out["reached"] else math.nan
        return out

    def log_rows(self):
        """The logged sorties, oldest first, as a numpy structured array (fields of ``ROW``)."""
        if not self.L:
            return np.zeros(0, dtype=ROW)
        n = int(self.log_meta[0])
        rows = self.log.cpu().numpy().view(ROW).reshape(-1)
        if n <= self.L:
            return rows[:n].copy()
        return np.roll(rows, -(n % self.L)).copy()
