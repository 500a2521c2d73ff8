"""Reward map (include/aac_rmap.h): ``ss_reward`` of the ATT / WGRU environment at any test position --
the reference's ``generate_reward_map`` sweep (ATT/main:255-354, WGRU/ma_main:494-...; ``env.ss_reward(...,
pos_to_test)``, ATT/env:2133-2138) as one launch over M rows.

``RewardMap.for_env(env)`` binds a ``BatchedEnv``.  ``at(points, env, agent, pre, rmin)`` evaluates M rows:
row m is what ``ss_reward`` would hand agent ``agent[m]`` of env ``env[m]`` if it now stood at ``points[m]``
with ``pre_pos = pre[m]`` (None: the point itself, the reference's map mode; ``"live"``: the subject's live
position, which makes the progress term visible -- with ``pre = point`` it is identically 0 in ATT).
Everything else is the env's live state.  ``grid()`` is the reference's 50 x 50 sweep over ``cfg.bound``.
One launch on torch's current stream after ``env.step`` / ``reset`` / ``auto_reset``; capturable.  ``read()``
is plain numpy:

    reward [M]      float64: the subject's own reward (before any team sum)
    terms  [M][12]  float64: the row of include/aac_terms.h (``ledger.NAMES``)
    mask   [M]      uint8: the step's mask bits (bound, drone, goal, building, waypoint, check_goal)
    done   [M]      uint8
    bbc    [M][4]   uint8: bound_building_check as this agent alone would set it

Read-only, unlike the reference's sweep: no waypoint is popped, agent 0 stays where it is, and the WGRU +3
waypoint bonus is kept (slot 1 is what a step would earn).  WGRU near-building penalty: ``rmin=None`` computes
the exact 18-ray obstacle radar at each point; a given ``rmin`` is used verbatim (``held_rmin(bufs)`` gives
the minimum of the subject's held radar row, which is what the reference's map mode uses).

``UamRewardMap.for_uam(env)`` is the same for a ``BatchedUAM`` (include/aac_uam_rmap.h), with ``flags`` and
``rays`` as further outputs and ``prev2`` as a further input; ``uam_step_rows`` turns the N map rows of one env
into the rows a step hands out.
"""
import ctypes

import numpy as np

FIELDS = (("reward", "float64", ()), ("terms", "float64", (12,)), ("mask", "uint8", ()), ("done", "uint8", ()),
          ("bbc", "uint8", (4,)))


class RewardMap:
    FIELDS = FIELDS
    OPTIONAL = ("terms",)           # outputs a caller's ``out`` may leave out

    def __init__(self, env):
        import torch
        from . import _native
        from .env import BatchedEnv
        if not isinstance(env, BatchedEnv):
            raise TypeError("RewardMap: a BatchedEnv (the UAM env has no reward map yet)")
        self.env, self.E, self.N = env, env.E, env.N
        self._torch, self._native = torch, _native
        self._bufs = {}                         # at(): one set of outputs per M
        self._last = None
        self._keep = None

    @classmethod
    def for_env(cls, env):
        return cls(env)

    def _alloc(self, M):
        torch = self._torch
        return {k: torch.zeros(M, *shp, dtype=getattr(torch, dt), device=self.env.device) for k, dt, shp in self.FIELDS}

    def _check_out(self, out, M):
        torch = self._torch
        for k, dt, shp in self.FIELDS:
            t = out.get(k)
            if t is None and k in self.OPTIONAL:
                continue
            if t is None or t.dtype != getattr(torch, dt) or t.numel() != M * int(np.prod(shp, dtype=np.int64)) \
                    or not t.is_contiguous() or t.device != self.env.device:
                raise ValueError(f"reward map output {k}: {dt} [{M}]{list(shp)}, contiguous, on {self.env.device}")

    def _index(self, v, M, hi, name):
        """A scalar or [M] array of env / agent indices as an int32 device tensor (None for all-zero)."""
        torch = self._torch
        if isinstance(v, (int, np.integer)):
            if not 0 <= int(v) < hi:
                raise ValueError(f"{name}: {v} outside [0, {hi})")
            return None if int(v) == 0 else torch.full((M,), int(v), dtype=torch.int32, device=self.env.device)
        t = torch.as_tensor(v, dtype=torch.int32, device=self.env.device).contiguous()
        if tuple(t.shape) != (M,):
            raise ValueError(f"{name}: a scalar or int32 [{M}]")
        return t

    def _prepare(self, points, env, agent, pre, rmin, out):
        """The arguments of ``at`` as contiguous device tensors: (points, M, env, agent, pre, rmin, out)."""
        torch = self._torch
        d = self.env.device
        pts = torch.as_tensor(points, dtype=torch.float64, device=d).contiguous()
        if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1:
            raise ValueError("points: [M][2]")
        M = int(pts.shape[0])
        ei, ai = self._index(env, M, self.E, "env"), self._index(agent, M, self.N, "agent")
        if isinstance(pre, str):
            if pre != "live":
                raise ValueError("pre: None, 'live' or [M][2]")
            pos = self.env.get_state()["pos"]
            e_l = ei.long() if ei is not None else torch.zeros(M, dtype=torch.long, device=d)
            a_l = ai.long() if ai is not None else torch.zeros(M, dtype=torch.long, device=d)
            pre = pos[e_l.clamp(0, self.E - 1), a_l.clamp(0, self.N - 1)].contiguous()
        elif pre is not None:
            pre = torch.as_tensor(pre, dtype=torch.float64, device=d).contiguous()
            if tuple(pre.shape) != (M, 2):
                raise ValueError(f"pre: [{M}][2]")
        if rmin is not None:
            rmin = torch.as_tensor(rmin, dtype=torch.float64, device=d)
            rmin = (rmin.expand(M) if rmin.ndim == 0 else rmin).contiguous()
            if tuple(rmin.shape) != (M,):
                raise ValueError(f"rmin: a scalar or float64 [{M}]")
        if out is None:
            out = self._bufs.get(M)
            if out is None:
                if len(self._bufs) >= 8:
                    self._bufs.clear()
                out = self._bufs[M] = self._alloc(M)
        else:
            self._check_out(out, M)
        return pts, M, ei, ai, pre, rmin, out

    def at(self, points, env=0, agent=0, pre=None, rmin=None, out=None):
        """Evaluate M rows (module docstring).  ``points`` [M][2]; ``env`` / ``agent`` scalars or [M];
        ``pre`` None, ``"live"`` or [M][2]; ``rmin`` None, a scalar or [M] (WGRU only; ignored by the ATT
        reward).  The outputs are this object's tensors for M rows (allocated on first use, reused
        after), or the caller's ``out`` (a dict of contiguous device tensors named as in ``read()``; it
        may leave ``terms`` out).  Returns the dict of device tensors."""
        torch = self._torch
        pts, M, ei, ai, pre, rmin, out = self._prepare(points, env, agent, pre, rmin, out)
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        o = self._native.RmapOut(*[None if out.get(k) is None else out[k].data_ptr() for k, _, _ in FIELDS])
        self._native.check(self._native.lib().aac_env_reward_map(
            self.env._h, p(pts), p(pre), p(ei), p(ai), p(rmin), M, ctypes.byref(o),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "aac_env_reward_map")
        self._keep = (pts, pre, ei, ai, rmin, out)      # alive until the stream has consumed them
        self._last = out
        return out

    def grid(self, nx=50, ny=50, env=0, agent=0, pre=None, rmin=None, out=None):
        """The reference's grid (ATT/main:287-289): ``np.linspace`` over ``cfg.bound``, ``meshgrid`` order.
        Returns ``(X, Y, out)``: X, Y [ny][nx] numpy, ``out`` the device tensors of ``at`` viewed
        [ny][nx]...; ``read(out)`` gives them as numpy."""
        X, Y, pts, pre, rmin = self._grid_args(nx, ny, pre, rmin)
        flat = self.at(pts, env=env, agent=agent, pre=pre, rmin=rmin, out=out)
        return X, Y, self._grid_view(flat, ny, nx)

    def _grid_args(self, nx, ny, pre, rmin):
        b = [float(v) for v in self.env.cfg.bound]
        X, Y = np.meshgrid(np.linspace(b[0], b[1], nx), np.linspace(b[2], b[3], ny))
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
        if pre is not None and not isinstance(pre, str):
            pre = np.asarray(pre, dtype=np.float64).reshape(ny * nx, 2)
        if rmin is not None and np.ndim(rmin):
            rmin = np.asarray(rmin, dtype=np.float64).reshape(ny * nx)
        return X, Y, pts, pre, rmin

    @staticmethod
    def _grid_view(flat, ny, nx):
        return {k: v.view(ny, nx, *v.shape[1:]) for k, v in flat.items() if v is not None}

    def read(self, out=None):
        """The rows of the last ``at`` / ``grid`` (or of ``out``) as numpy arrays (synchronises)."""
        out = self._last if out is None else out
        return {k: v.cpu().numpy() for k, v in out.items() if v is not None}

    def held_rmin(self, bufs=None, env=0, agent=0):
        """The minimum of the subject's held float radar row (``bufs.radar`` of the last step / reset), as
        float64: the radar minimum the reference's map mode uses at every test position."""
        bufs = self.env.bufs if bufs is None else bufs
        return float(bufs.radar[env, agent].min().double().item())


# ================================================================================ UAM (config 5)
UAM_FIELDS = FIELDS + (("flags", "uint8", ()), ("rays", "float64", (18,)))
BAND, BAND_DBL, CRASH_DBL, PREV_TWO = 1, 2, 4, 8          # the ``flags`` bits (include/aac_uam_rmap.h)


class UamRewardMap(RewardMap):
    """``ss_reward_Mar_changeskin`` of the UAM environment at any test position (include/aac_uam_rmap.h;
    the reference's sweep: UAM/main:434-505, UAM/env:3939-3944) -- ``RewardMap`` for a ``BatchedUAM``, the
    same calls and shapes.  ``read()`` has two more arrays:

        flags  [M]      uint8: bit0 nearest neighbour in the near-drone band, bit1 its bearing doubles the
                        coefficient, bit2 the collision bearing doubles the crash penalty, bit3 a collider is
                        one of the two previous nearest
        rays   [M][18]  float64: the fp64 radar row at the point (not written when ``rmin`` is given)

    A row is the subject evaluated alone, as the reference's map mode evaluates drone 0 alone: crash 50 and
    near-drone coefficient 2, doubled by the row's own bearings only.  ``uam_step_rows`` applies what a step
    carries over from the earlier aircraft of the call.  ``rmin=None`` computes the radar at the point; the
    reference uses the held row (``held_rmin``).  ``prev2`` [M][2] uint8 names the "previous nearest two"
    (255: none); None takes the live ``top2``, which is what the next step would read.  Read-only: aircraft 0
    stays where it is; ``me`` is the live ``reach`` or the goal touch at the point (the reference keeps the
    sticky flag of the live position); neighbours are ordered by distance from the point (the reference keeps
    the held order, which matters for exact ties only)."""
    FIELDS = UAM_FIELDS
    OPTIONAL = ("terms", "rays")

    def __init__(self, env):
        import torch
        from . import _native, uam
        if not isinstance(env, uam.BatchedUAM):
            raise TypeError("UamRewardMap: a BatchedUAM (RewardMap.for_env binds a BatchedEnv)")
        self.env, self.E, self.N = env, env.E, env.N
        self._torch, self._native, self._uam = torch, _native, uam
        self._bufs = {}
        self._last = None
        self._keep = None

    @classmethod
    def for_uam(cls, env):
        return cls(env)

    def at(self, points, env=0, agent=0, pre=None, rmin=None, prev2=None, out=None):
        """Evaluate M rows; arguments as ``RewardMap.at`` plus ``prev2`` (None or uint8 [M][2]).  ``out``
        may leave ``terms`` and ``rays`` out.  Returns the dict of device tensors."""
        torch = self._torch
        pts, M, ei, ai, pre, rmin, out = self._prepare(points, env, agent, pre, rmin, out)
        if prev2 is not None:
            prev2 = torch.as_tensor(prev2, dtype=torch.uint8, device=self.env.device).contiguous()
            if tuple(prev2.shape) != (M, 2):
                raise ValueError(f"prev2: uint8 [{M}][2]")
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        o = self._native.UamRmapOut(*[None if out.get(k) is None else out[k].data_ptr() for k, _, _ in UAM_FIELDS])
        self._uam._chk(self._uam.lib().aac_uam_reward_map(
            self.env._h, p(pts), p(pre), p(ei), p(ai), p(rmin), p(prev2), M, ctypes.byref(o),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "aac_uam_reward_map")
        self._keep = (pts, pre, ei, ai, rmin, prev2, out)
        self._last = out
        return out

    def grid(self, nx=50, ny=50, env=0, agent=0, pre=None, rmin=None, prev2=None, out=None):
        """The reference's grid (UAM/main:466-468) over ``cfg.bound``; returns ``(X, Y, out)`` as
        ``RewardMap.grid``.  ``prev2`` None or one pair [2] for every point."""
        X, Y, pts, pre, rmin = self._grid_args(nx, ny, pre, rmin)
        if prev2 is not None:
            prev2 = np.broadcast_to(np.asarray(prev2, dtype=np.uint8).reshape(-1, 2), (ny * nx, 2)).copy()
        flat = self.at(pts, env=env, agent=agent, pre=pre, rmin=rmin, prev2=prev2, out=out)
        return X, Y, self._grid_view(flat, ny, nx)

    def held_rmin(self, bufs=None, env=0, agent=0):
        """The minimum of the subject's held radar row (``bufs.radar`` of the last step / reset): the radar
        minimum the reference's map mode uses at every test position."""
        bufs = self.env.bufs if bufs is None else bufs
        return float(bufs.radar[env, agent].min().item())


def uam_step_rows(rows, flags, mask):
    """What a UAM step hands the N aircraft of ONE env, from their map rows at (pos, pre_pos, pre-step top2).
    The step walks the aircraft in index order and keeps the crash penalty and the near-drone coefficient
    doubled for the later aircraft of the call (UAM/env:4320, :4546); a map row carries its own doubling
    only.  Every doubling is an exact multiplication by 2: aircraft j's crash value (slot 0 of the bound,
    cloud and drone branches, not the goal's +50) is scaled by 2^(drone-branch rows with CRASH_DBL among
    0..j-1), its slot 6 by 2^(rows with BAND and BAND_DBL among 0..j-1, whatever their branch).
    ``rows`` [N][12], ``flags`` [N], ``mask`` [N] numpy; returns (rows [N][12], reward [N]), the reward the
    left-to-right sum of slots 0..6 as the kernel forms it."""
    rows = np.array(rows, dtype=np.float64)
    flags, mask = np.asarray(flags).astype(np.int64), np.asarray(mask).astype(np.int64)
    crashed = (mask & 7) != 0
    drone = ((mask & 3) == 0) & ((mask & 4) != 0)
    crash_dbl = (drone & ((flags & CRASH_DBL) != 0)).astype(np.int64)
    band_dbl = (((flags & BAND) != 0) & ((flags & BAND_DBL) != 0)).astype(np.int64)
    before_c = np.cumsum(crash_dbl) - crash_dbl
    before_b = np.cumsum(band_dbl) - band_dbl
    rows[:, 0] = np.where(crashed, np.ldexp(rows[:, 0], before_c), rows[:, 0])
    rows[:, 6] = np.ldexp(rows[:, 6], before_b)
    reward = rows[:, 0].copy()
    for k in range(1, 7):
        reward = reward + rows[:, k]
    return rows, reward
