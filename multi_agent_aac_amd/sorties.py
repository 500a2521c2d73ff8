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
import math

import numpy as np
import torch

from . import _native
from .tally import SlotTally

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


class SortieStats(SlotTally):
    """Per-aircraft running state + totals for the E envs x N aircraft of a ``BatchedEnv`` (``for_env``)
    or a ``BatchedUAM`` (``for_uam``).

    log            > 0: keep the last ``log`` finished sorties as rows, in (call, env, aircraft) order
    reach_margin   added to the flown length of a sortie (the reference's UAM code adds 5: reaching the
                   protective zone counts as reaching the goal)
    """
    EPW, FIELDS, ROW = EPW, FIELDS, ROW
    MIN, MAX = slice(F_MIN, F_MIN + 1), slice(F_MAX, F_MAX + 1)
    STATE = ("straight", "first_seg", "run_dist", "last_pos", "run_flags", "reach_step", "run_len", "ep_count", "slots",
             "collide_hist")
    REDUCE, ERROR = "aac_sortie_reduce", "aac_sortie_last_error"

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
        d = self.device = env.device
        E, N = self.E, self.N
        f64, i32 = dict(dtype=torch.float64, device=d), dict(dtype=torch.int32, device=d)
        self.straight, self.first_seg, self.run_dist = (torch.zeros(E, N, **f64) for _ in range(3))
        self.last_pos = torch.zeros(E, N, 2, **f64)
        self.run_flags = torch.zeros(E, N, dtype=torch.uint8, device=d)
        self.reach_step = torch.zeros(E, N, **i32)
        self.run_len, self.ep_count = torch.zeros(E, **i32), torch.zeros(E, **i32)
        self.collide_hist = torch.zeros(self.episode_length + 2, dtype=torch.int64, device=d)
        st = _native.SortieState()
        st.hist_len = self.episode_length + 2
        L = _native.lib()
        self._call = L.aac_uam_sorties if self.uam else L.aac_env_sorties
        self._err = L.aac_uam_last_error if self.uam else L.aac_last_error
        self._alloc(st, log, rows_per_env=N)

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

    def accumulate(self, bufs, quota=None):
        """Tally the step whose outputs are in ``bufs`` (a ``StepBuffers`` / ``UamBuffers``: done, mask,
        env_done), after the env step launch and before the auto-reset, on the same stream.  ``quota``:
        int32 [E] tensor (or an int, kept in ``self.quota``): an env with that many finished episodes
        contributes nothing more.  A buffer set's tensors are taken as fixed: its launch arguments are
        built on the first call."""
        args = self._args(bufs, self._quota(quota))
        rc = self._call(self.env._h, self._st_ref, args, torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aac_sortie_accumulate failed ({rc}): {self._err().decode(errors='replace')}")

    def _build(self, bufs, quota):
        for name, shape in (("done", (self.E, self.N)), ("mask", (self.E, self.N)), ("env_done", (self.E,))):
            t = getattr(bufs, name)
            if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{name} {tuple(t.shape)} {t.dtype}: expected {shape} uint8 on {self.device}")
        p = _native.SortieStep()
        p.quota = self._quota_ptr(quota)
        p.done, p.mask, p.env_done = bufs.done.data_ptr(), bufs.mask.data_ptr(), bufs.env_done.data_ptr()
        p.E, p.N, p.episode_length = self.E, self.N, self.episode_length
        for k, v in self.bits.items():
            setattr(p, k, v)
        p.reach_margin = self.reach_margin
        return p

    def read(self, clear=False):
        """Totals as a dict of numpy / Python values (synchronises): the counters (``sorties``, the five
        classes, ``degenerate``, ``episodes``, ``reach_step_sum``), ``collide_hist`` (int64
        [episode_length + 2], indexed by the length of the colliding episode), the sums, ``ratio_mean`` /
        ``ratio_std`` (population, as ``np.mean`` / ``np.std`` of the reference's flight-ratio list; NaN
        while no sortie is counted), ``ratio_min`` / ``ratio_max`` and ``mean_reach_step``.  ``clear``
        empties the totals and the histogram afterwards (a per-window report); running episodes carry on."""
        hist = self.collide_hist.cpu().numpy()      # before the reduce launch, which clears it
        raw = self._reduce(clear)
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
