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
"""
import ctypes

import numpy as np

FIELDS = (("reward", "float64", ()), ("terms", "float64", (12,)), ("mask", "uint8", ()), ("done", "uint8", ()),
          ("bbc", "uint8", (4,)))


class RewardMap:
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
        return {k: torch.zeros(M, *shp, dtype=getattr(torch, dt), device=self.env.device) for k, dt, shp in FIELDS}

    def _check_out(self, out, M):
        torch = self._torch
        for k, dt, shp in FIELDS:
            t = out.get(k)
            if t is None and k == "terms":
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

    def at(self, points, env=0, agent=0, pre=None, rmin=None, out=None):
        """Evaluate M rows (module docstring).  ``points`` [M][2]; ``env`` / ``agent`` scalars or [M];
        ``pre`` None, ``"live"`` or [M][2]; ``rmin`` None, a scalar or [M] (WGRU only; ignored by the ATT
        reward).  The outputs are this object's tensors for M rows (allocated on first use, reused
        after), or the caller's ``out`` (a dict of contiguous device tensors named as in ``read()``; it
        may leave ``terms`` out).  Returns the dict of device tensors."""
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
        b = [float(v) for v in self.env.cfg.bound]
        X, Y = np.meshgrid(np.linspace(b[0], b[1], nx), np.linspace(b[2], b[3], ny))
        pts = np.stack([X.reshape(-1), Y.reshape(-1)], axis=1)
        if pre is not None and not isinstance(pre, str):
            pre = np.asarray(pre, dtype=np.float64).reshape(ny * nx, 2)
        if rmin is not None and np.ndim(rmin):
            rmin = np.asarray(rmin, dtype=np.float64).reshape(ny * nx)
        flat = self.at(pts, env=env, agent=agent, pre=pre, rmin=rmin, out=out)
        return X, Y, {k: v.view(ny, nx, *v.shape[1:]) for k, v in flat.items() if v is not None}

    def read(self, out=None):
        """The rows of the last ``at`` / ``grid`` (or of ``out``) as numpy arrays (synchronises)."""
        out = self._last if out is None else out
        return {k: v.cpu().numpy() for k, v in out.items() if v is not None}

    def held_rmin(self, bufs=None, env=0, agent=0):
        """The minimum of the subject's held float radar row (``bufs.radar`` of the last step / reset), as
        float64: the radar minimum the reference's map mode uses at every test position."""
        bufs = self.env.bufs if bufs is None else bufs
        return float(bufs.radar[env, agent].min().double().item())
