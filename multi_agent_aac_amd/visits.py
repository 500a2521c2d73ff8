"""Exploration maps on the device (include/aac_visits.h): the arrays behind the reference's
``display_exploration_expolitation`` (ATT/util:776-866, UAM/util:1484: a heat map of every position
flown in training, split into "explore" episodes, ``epsIDX <= eps_period``, and "exploit" episodes) and
``action_selection_statistics`` (ATT/util:869-897, UAM/util:1572: a 2-D histogram of every action
taken), kept beside a loop that never leaves the GPU.  Plots are left to the caller.

``VisitMap.accumulate(act)`` is one small launch on torch's current stream, between the act launch and
the env step launch; it may be captured in a HIP graph with the step.  It reads the env's live
positions -- the position each action is taken from -- together with that action.  The fused step tail
resets a finished env inside its own launch, so the post-step position of a finished episode does not
exist afterwards: an episode of ``len`` steps contributes its reset position and ``len - 1`` flown
positions per agent, and its terminal position is not counted.

A row (env e, agent i) falls into period 0 ("explore") while the env's own 1-based episode counter is
``<= explore_until`` and into period 1 ("exploit") afterwards: the comparison the noise schedules make
(``maddpg._noise_scale``, ``gru._scale``, ``uam_learner.noise_scale``).  Everything the kernel writes is
a torch tensor this object owns (``tensors()``), so a resumed run continues its maps exactly.  With
several ranks each rank keeps its own maps.
"""
import ctypes

import numpy as np
import torch

from . import _native

MAX_A = 32            # AAC_VISITS_MAX_A
MAX_G = 65536         # AAC_VISITS_MAX_G
CHUNK = 1024          # AAC_VISITS_CHUNK: rows per workgroup
COUNTERS = ("samples", "pos_outside", "act_outside", "bad_map")     # counters[plane][0..3]; bad_map: plane 0 only
EXPLORE_UNTIL = {"env": 8000, "uam": 10000}     # the default eps_end of maddpg / gru ``act`` and of uam_learner's


def edges(lo, hi, G):
    """The G + 1 bin edges of one axis, by the header's rule: lo + k * ((hi - lo) / G), the last one hi
    (``np.linspace(lo, hi, G + 1)``)."""
    e = np.float64(lo) + np.arange(G + 1, dtype=np.float64) * ((np.float64(hi) - np.float64(lo)) / np.float64(G))
    e[G] = hi
    return e


class VisitMap:
    """Position and action histograms of the rows of a ``BatchedEnv`` (``for_env``) or a ``BatchedUAM``
    (``for_uam``).

    grid            (GX, GY) position bins over the env's bound
    act_bins        A: action bins per axis over [-1, 1]
    explore_until   the last episode of the "explore" period; None: the default ``eps_end`` of the
                    model's ``act`` (8000 for ATT and GRU, 10000 for UAM).  It may be reassigned between
                    calls (a captured launch keeps the value it was captured with).
    """

    def __init__(self, env, grid=(50, 50), act_bins=20, explore_until=None):
        from .uam import BatchedUAM
        self.env, self.uam = env, isinstance(env, BatchedUAM)
        self.E, self.N = int(env.E), int(env.N)
        self.GX, self.GY, self.A = int(grid[0]), int(grid[1]), int(act_bins)
        if not (1 <= self.GX <= MAX_G and 1 <= self.GY <= MAX_G):
            raise ValueError(f"VisitMap: 1 <= grid <= {MAX_G}")
        if not 1 <= self.A <= MAX_A:
            raise ValueError(f"VisitMap: 1 <= act_bins <= {MAX_A}")
        self.n_maps = 1 if self.uam else int(env.cfg.n_maps)
        self.explore_until = int(EXPLORE_UNTIL["uam" if self.uam else "env"] if explore_until is None
                                 else explore_until)
        self.act_dtype = torch.float64 if self.uam else torch.float32
        self.bound = tuple(float(b) for b in env.cfg.bound)
        d = self.device = env.device
        P = 2 * self.n_maps
        self.pos_hist = torch.zeros(P, self.GX, self.GY, dtype=torch.int64, device=d)
        self.act_hist = torch.zeros(2, self.A, self.A, dtype=torch.int64, device=d)
        self.counters = torch.zeros(P, len(COUNTERS), dtype=torch.int64, device=d)
        st = _native.VisitsState()
        st.pos_hist, st.act_hist, st.counters = (self.pos_hist.data_ptr(), self.act_hist.data_ptr(),
                                                 self.counters.data_ptr())
        st.GX, st.GY, st.A, st.n_maps = self.GX, self.GY, self.A, self.n_maps
        st.x0, st.x1, st.y0, st.y1 = self.bound
        st.a0, st.a1 = -1.0, 1.0
        self._st, self._st_ref = st, ctypes.byref(st)
        L = _native.lib()
        self._call = L.aac_uam_visits if self.uam else L.aac_env_visits
        self._err = L.aac_uam_last_error if self.uam else L.aac_last_error
        self._steps = {}        # act pointer, sel pointer, explore_until -> VisitsStep

    @classmethod
    def for_env(cls, env, grid=(50, 50), act_bins=20, explore_until=None):
        """For a ``BatchedEnv`` (att or wgru): float32 actions, one pair of planes per map of its stack."""
        from .uam import BatchedUAM
        if isinstance(env, BatchedUAM):
            raise TypeError("VisitMap.for_env: a BatchedUAM takes VisitMap.for_uam")
        return cls(env, grid, act_bins, explore_until)

    @classmethod
    def for_uam(cls, env, grid=(50, 50), act_bins=20, explore_until=None):
        """For a ``BatchedUAM``: float64 actions, one map."""
        from .uam import BatchedUAM
        if not isinstance(env, BatchedUAM):
            raise TypeError("VisitMap.for_uam: not a BatchedUAM")
        return cls(env, grid, act_bins, explore_until)

    # ------------------------------------------------------------------- state
    def reset(self):
        """Empty tables and counters."""
        for t in (self.pos_hist, self.act_hist, self.counters):
            t.zero_()

    def tensors(self):
        """The device tensors a checkpoint must carry (loaded in place)."""
        return {"pos_hist": self.pos_hist, "act_hist": self.act_hist, "counters": self.counters}

    # ------------------------------------------------------------------- calls
    def accumulate(self, act, sel=None, period=None):
        """Count the env's live positions with the actions ``act`` ([E][N][2], float32 / float64 for
        UAM) about to be applied to them: after the act launch and before the env step launch, on the
        same stream.  ``sel``: uint8 [E], only the envs with ``sel[e] != 0`` (None: all).  ``period`` 0 / 1
        puts every row into that period whatever its env's counter says (an evaluation rollout, whose env
        counts episodes of its own).  The launch arguments of an ``act`` tensor are built on its first
        call (the loops alternate two)."""
        until = self.explore_until if period is None else (2 ** 31 - 1, -2 ** 31)[int(period)]
        if act.dtype != self.act_dtype or tuple(act.shape) != (self.E, self.N, 2) or not act.is_contiguous() \
                or act.device != self.device:
            raise ValueError(f"act {tuple(act.shape)} {act.dtype}: expected ({self.E}, {self.N}, 2) "
                             f"{self.act_dtype}, contiguous, on {self.device}")
        if sel is not None and (sel.dtype != torch.uint8 or tuple(sel.shape) != (self.E,)
                                or not sel.is_contiguous() or sel.device != self.device):
            raise ValueError("sel: uint8 [E]")
        # the cached entry keeps its tensors alive, so their addresses name them
        key = (act.data_ptr(), None if sel is None else sel.data_ptr(), until)
        hit = self._steps.get(key)
        if hit is None:
            p = _native.VisitsStep()
            p.act, p.act_f64 = act.data_ptr(), int(act.dtype == torch.float64)
            p.sel = None if sel is None else sel.data_ptr()
            p.explore_until = until
            if len(self._steps) > 64:
                self._steps.clear()
            hit = self._steps[key] = (act, sel, ctypes.byref(p), p)
        rc = self._call(self.env._h, self._st_ref, hit[2], torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aac_visits_accumulate failed ({rc}): {self._err().decode(errors='replace')}")

    def edges(self):
        """(x edges [GX + 1], y edges [GY + 1], action edges [A + 1]) as float64 arrays."""
        x0, x1, y0, y1 = self.bound
        return edges(x0, x1, self.GX), edges(y0, y1, self.GY), edges(-1.0, 1.0, self.A)

    def read(self, clear=False):
        """The maps as a dict of numpy arrays (synchronises):
          pos        int64 [n_maps][2][GX][GY]   [map][period]: 0 explore, 1 exploit
          act        int64 [2][A][A]             [period][first action component][second]
          samples / pos_outside / act_outside    int64 [n_maps][2]: rows counted, rows whose position /
                     action was outside its range (or not finite) and is in no bin
          bad_map    rows whose map_idx was outside [0, n_maps): counted nowhere else
          x_edges / y_edges / act_edges          the bin edges (``np.histogram2d``'s)
          explore_until
        ``clear`` empties tables and counters afterwards (a per-window report)."""
        pos = self.pos_hist.cpu().numpy().reshape(self.n_maps, 2, self.GX, self.GY)
        act = self.act_hist.cpu().numpy()
        cnt = self.counters.cpu().numpy().reshape(self.n_maps, 2, len(COUNTERS))
        if clear:
            self.reset()
        xe, ye, ae = self.edges()
        out = {"pos": pos, "act": act, "x_edges": xe, "y_edges": ye, "act_edges": ae,
               "explore_until": self.explore_until}
        for k, name in enumerate(COUNTERS[:3]):
            out[name] = cnt[:, :, k].copy()
        out["bad_map"] = int(cnt[0, 0, 3])
        return out
