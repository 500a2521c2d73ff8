"""Radar probes (include/aac_probe.h): for every radar ray of the ATT / WGRU environment, what it ended
on and where -- the probe segments and nearest intersection points the reference's ``env.step``
returns beside the state (ATT/env:1051-1170, :2720, :2815; OM/env:1049-1148).

``RadarProbe.for_env(env)`` owns the output tensors for the env's E rows; ``run()`` is one launch on
torch's current stream after ``env.step`` / ``reset`` / ``auto_reset`` and may be captured in a HIP
graph.  ``at(pos)`` probes any rows of positions on the env's maps, ``for_trajectories`` the recorded
positions of a ``record.Trajectories``.  ``read()`` is plain numpy:

    dist   [M][N][18]     float64: ``float32(dist)`` is the env's ``radar`` output bit for bit
    point  [M][N][18][2]  the hit point (no hit: the ray end); ``|point - pos| == dist`` bit for bit
    end    [M][N][18][2]  the ray end
    kind   [M][N][18]     uint8 index into ``KINDS``
    id     [M][N][18]     int32: drone index j / cell ``ci * grid_h + cj`` / bound line k / -1

Among candidates at bit-equal distance the lowest (kind, id) is taken.  Off unless called: the env's
own launches are not changed by any of this.

``UamRadarProbe.for_uam(env)`` is the same for a ``uam.BatchedUAM`` (include/aac_uam_probe.h; UAM/env:1346-1495):
the same calls and arrays, ``dist`` the env's float64 ``radar`` output bit for bit, kinds ``UAM_KINDS`` with
``id`` 0 for the runway, the bound segment k (x = bound[0], x = bound[1], y = bound[3], y = bound[2]), the cloud
k or the aircraft j.  ``at`` takes ``clouds`` [M][2][2] and ``env_idx`` [M] instead of ``map_idx``;
``for_uam_trajectories`` probes a UAM recording.
"""
import ctypes

import numpy as np

KINDS = ("none", "drone", "cell", "bound")
N_RAYS = 18
FIELDS = (("dist", "float64", ()), ("point", "float64", (2,)), ("end", "float64", (2,)), ("kind", "uint8", ()),
          ("id", "int32", ()))


class RadarProbe:
    KINDS = KINDS

    def __init__(self, env):
        import torch
        from . import _native
        from .env import BatchedEnv
        if not isinstance(env, BatchedEnv):
            raise TypeError("RadarProbe: a BatchedEnv (UamRadarProbe.for_uam probes a BatchedUAM)")
        self.env, self.E, self.N = env, env.E, env.N
        self._torch, self._native = torch, _native
        self._live = self._alloc(self.E)
        self._at_bufs = {}                      # at(): one set per M
        self._last = self._live
        self._keep = None

    @classmethod
    def for_env(cls, env):
        return cls(env)

    def _alloc(self, M):
        torch = self._torch
        return {k: torch.zeros(M, self.N, N_RAYS, *shp, dtype=getattr(torch, dt), device=self.env.device)
                for k, dt, shp in FIELDS}

    def _check_out(self, out, M):
        torch = self._torch
        for k, dt, shp in FIELDS:
            t = out[k]
            if t.dtype != getattr(torch, dt) or t.numel() != M * self.N * N_RAYS * int(np.prod(shp, dtype=np.int64)) \
                    or not t.is_contiguous() or t.device != self.env.device:
                raise ValueError(f"probe output {k}: {dt} [{M}][{self.N}][{N_RAYS}]{list(shp)}, contiguous, on {self.env.device}")

    def _launch(self, pos, map_idx, M, sel, out):
        torch = self._torch
        if sel is not None and (sel.dtype != torch.uint8 or tuple(sel.shape) != (M,) or not sel.is_contiguous()
                                or sel.device != self.env.device):
            raise ValueError(f"sel: uint8 [{M}] on {self.env.device}")
        o = self._native.ProbeOut(*[out[k].data_ptr() for k, _, _ in FIELDS])
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        self._native.check(self._native.lib().aac_env_probe(
            self.env._h, p(pos), p(map_idx), M, p(sel), ctypes.byref(o),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "aac_env_probe")
        self._keep = (pos, map_idx, sel, out)       # alive until the stream has consumed them
        self._last = out
        return out

    def run(self, sel=None):
        """Probe the env's live state (``sel``: uint8 [E], rows with 0 are skipped and keep their old
        records).  Returns the device tensors, which ``for_env`` allocated once."""
        if sel is not None:
            sel = self._torch.as_tensor(sel, dtype=self._torch.uint8, device=self.env.device).contiguous()
        return self._launch(None, None, self.E, sel, self._live)

    def at(self, pos, map_idx=None, sel=None, out=None):
        """Probe M rows of positions ``pos`` [M][N][2] on the maps ``map_idx`` [M] (None: map 0).  The
        outputs are this object's tensors for M rows (allocated on first use, reused after), or the
        caller's ``out`` (a dict of contiguous device tensors named as in ``read()``)."""
        torch = self._torch
        d = self.env.device
        pos = torch.as_tensor(pos, dtype=torch.float64, device=d).contiguous()
        if pos.ndim != 3 or tuple(pos.shape[1:]) != (self.N, 2) or pos.shape[0] < 1:
            raise ValueError(f"pos: [M][{self.N}][2]")
        M = int(pos.shape[0])
        if map_idx is not None:
            map_idx = torch.as_tensor(map_idx, dtype=torch.int32, device=d).contiguous()
            if tuple(map_idx.shape) != (M,):
                raise ValueError(f"map_idx: int32 [{M}]")
        if sel is not None:
            sel = torch.as_tensor(sel, dtype=torch.uint8, device=d).contiguous()
        if out is None:
            out = self._at_bufs.get(M)
            if out is None:
                if len(self._at_bufs) >= 8:
                    self._at_bufs.clear()
                out = self._at_bufs[M] = self._alloc(M)
        else:
            self._check_out(out, M)
        return self._launch(pos, map_idx, M, sel, out)

    def read(self, out=None):
        """The records of the last ``run`` / ``at`` (or of ``out``) as numpy arrays (synchronises)."""
        out = self._last if out is None else out
        M = out["dist"].numel() // (self.N * N_RAYS)
        return {k: out[k].cpu().numpy().reshape((M, self.N, N_RAYS) + shp) for k, _, shp in FIELDS}

    def summary(self, out=None):
        """Rays per kind of the last probe: ``{"none": n, "drone": n, "cell": n, "bound": n}``."""
        kind = (self._last if out is None else out)["kind"]
        c = self._torch.bincount(kind.reshape(-1).to(self._torch.int64), minlength=len(self.KINDS)).cpu().numpy()
        return {k: int(c[i]) for i, k in enumerate(self.KINDS)}


def for_trajectories(env, tj, probe=None):
    """Probe every recorded position of a ``record.Trajectories`` of ``env`` (rows r < cursor[k] of track
    k, on the map of the row header) in one launch.  Returns ``dist`` / ``point`` / ``end`` / ``kind`` /
    ``id`` as [T][S][N][18]... numpy arrays and ``valid`` [T][S]; rows that are not valid hold zeros
    (kind 0, id 0)."""
    import torch
    probe = probe or RadarProbe.for_env(env)
    pos, hdr = tj.rows["pos"], tj.rows["header"]
    T, S, N = pos.shape[0], pos.shape[1], pos.shape[2]
    if N != env.N:
        raise ValueError("for_trajectories: the recording has another N than the env")
    valid = np.arange(S)[None, :] < np.asarray(tj.cursor)[:, None]
    out = probe._alloc(T * S)
    probe.at(np.ascontiguousarray(pos.reshape(T * S, N, 2)),
             map_idx=np.ascontiguousarray(hdr[..., 3].reshape(T * S).astype(np.int32)),
             sel=torch.as_tensor(valid.reshape(-1).astype(np.uint8)), out=out)
    res = {k: v.reshape((T, S) + v.shape[1:]) for k, v in probe.read(out).items()}
    res["valid"] = valid
    return res


# ================================================================================ UAM (config 5)
UAM_KINDS = ("none", "runway", "bound", "cloud", "aircraft")


class UamRadarProbe(RadarProbe):
    """Radar probes of a ``uam.BatchedUAM`` (include/aac_uam_probe.h): ``RadarProbe``'s calls and arrays.  The
    candidates of a ray are tested in the reference's order (runway, the four bound segments, the two clouds,
    the other aircraft by index, finished ones included), each on a strict ``<``: the record is the first that
    attains the minimum, and a candidate bit-equal to the ray length leaves it ``none``."""
    KINDS = UAM_KINDS

    def __init__(self, env):
        import torch
        from . import _native, uam
        if not isinstance(env, uam.BatchedUAM):
            raise TypeError("UamRadarProbe: a BatchedUAM (RadarProbe.for_env binds a BatchedEnv)")
        self.env, self.E, self.N = env, env.E, env.N
        self._torch, self._native, self._uam = torch, _native, uam
        self._live = self._alloc(self.E)
        self._at_bufs = {}
        self._last = self._live
        self._keep = None

    @classmethod
    def for_uam(cls, env):
        return cls(env)

    def _launch(self, pos, clouds, env_idx, M, sel, out):
        torch = self._torch
        if sel is not None and (sel.dtype != torch.uint8 or tuple(sel.shape) != (M,) or not sel.is_contiguous()
                                or sel.device != self.env.device):
            raise ValueError(f"sel: uint8 [{M}] on {self.env.device}")
        o = self._native.UamProbeOut(*[out[k].data_ptr() for k, _, _ in FIELDS])
        p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
        self._uam._chk(self._uam.lib().aac_uam_probe(
            self.env._h, p(pos), p(clouds), p(env_idx), M, p(sel), ctypes.byref(o),
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "aac_uam_probe")
        self._keep = (pos, clouds, env_idx, sel, out)       # alive until the stream has consumed them
        self._last = out
        return out

    def run(self, sel=None):
        """Probe the env's live state (``sel``: uint8 [E], rows with 0 are skipped and keep their old
        records).  Returns the device tensors, which ``for_uam`` allocated once."""
        if sel is not None:
            sel = self._torch.as_tensor(sel, dtype=self._torch.uint8, device=self.env.device).contiguous()
        return self._launch(None, None, None, self.E, sel, self._live)

    def at(self, pos, clouds=None, env_idx=None, sel=None, out=None):
        """Probe M rows of positions ``pos`` [M][N][2].  ``clouds`` [M][2][2]: the rows' cloud centres (None:
        the live centres of env ``env_idx[m]``; ``env_idx`` None: env m mod E).  Outputs as ``RadarProbe.at``."""
        torch = self._torch
        d = self.env.device
        pos = torch.as_tensor(pos, dtype=torch.float64, device=d).contiguous()
        if pos.ndim != 3 or tuple(pos.shape[1:]) != (self.N, 2) or pos.shape[0] < 1:
            raise ValueError(f"pos: [M][{self.N}][2]")
        M = int(pos.shape[0])
        if clouds is not None:
            clouds = torch.as_tensor(clouds, dtype=torch.float64, device=d).contiguous()
            if tuple(clouds.shape) != (M, 2, 2):
                raise ValueError(f"clouds: float64 [{M}][2][2]")
        if env_idx is not None:
            env_idx = torch.as_tensor(env_idx, dtype=torch.int32, device=d).contiguous()
            if tuple(env_idx.shape) != (M,):
                raise ValueError(f"env_idx: int32 [{M}]")
        if sel is not None:
            sel = torch.as_tensor(sel, dtype=torch.uint8, device=d).contiguous()
        if out is None:
            out = self._at_bufs.get(M)
            if out is None:
                if len(self._at_bufs) >= 8:
                    self._at_bufs.clear()
                out = self._at_bufs[M] = self._alloc(M)
        else:
            self._check_out(out, M)
        return self._launch(pos, clouds, env_idx, M, sel, out)


def for_uam_trajectories(env, tj, probe=None):
    """Probe every recorded row of a UAM ``record.Trajectories`` of ``env`` (rows r < cursor[k] of track k,
    positions from ``rows["pos"]``, cloud centres from ``rows["clouds"]``) in one launch.  Returns ``dist`` /
    ``point`` / ``end`` / ``kind`` / ``id`` as [T][S][N][18]... numpy arrays and ``valid`` [T][S]; rows that are
    not valid hold zeros (kind 0, id 0)."""
    import torch
    probe = probe or UamRadarProbe.for_uam(env)
    pos, clouds = tj.rows["pos"], tj.rows["clouds"]
    T, S, N = pos.shape[0], pos.shape[1], pos.shape[2]
    if N != env.N:
        raise ValueError("for_uam_trajectories: the recording has another N than the env")
    valid = np.arange(S)[None, :] < np.asarray(tj.cursor)[:, None]
    out = probe._alloc(T * S)
    probe.at(np.ascontiguousarray(pos.reshape(T * S, N, 2)), clouds=np.ascontiguousarray(clouds.reshape(T * S, 2, 2)),
             sel=torch.as_tensor(valid.reshape(-1).astype(np.uint8)), out=out)
    res = {k: v.reshape((T, S) + v.shape[1:]) for k, v in probe.read(out).items()}
    res["valid"] = valid
    return res
