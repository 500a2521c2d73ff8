"""Flight recorder (include/aac_record.h): the flown paths and per-step status of evaluation rollouts,
kept on the device -- what the reference's eval mode collects on the host as ``traj_step_list`` /
``trajectory_eachPlay`` (ATT/main:700) and ``eps_status_holder``, plus every aircraft's distance to
its nearest neighbour (the quantity behind ``near_drone_penalty``).

``FlightRecorder.for_env(env, env_ids, steps, episodes)`` owns the device tensors of T tracks (one
per followed env); ``after_reset`` / ``after_step`` are one launch each on torch's current stream and
may be captured in a HIP graph with the step.  ``read()`` downloads everything into a
``Trajectories``, which is plain numpy: it loads, slices and saves on a machine with no GPU and no
native library.  Plots stay out of scope; the arrays are what a plot needs.
"""
import ctypes
import math

import numpy as np

ROW_ENV_DONE, ROW_RESET = 1, 2          # header flags (AAC_RECORD_ROW_*)
EP_ANY_DONE, EP_DROPPED = 1, 2          # summary flags (AAC_RECORD_EP_*)
PHASE_RESET, PHASE_STEP = 0, 1
MAX_AGENTS = 64
EPISODE = np.dtype([("ret", "<f8"), ("min_sep", "<f8"), ("min_sep_t", "<i4"), ("row0", "<i4"), ("rows", "<i4"),
                    ("len", "<i4"), ("episode", "<i4"), ("env", "<i4"), ("flags", "<i4"), ("pad", "<i4")])
assert EPISODE.itemsize == 48           # aac_record_episode

# per-track running state: name -> dtype
TRACK_FIELDS = (("cursor", "<i4"), ("ep_seen", "<i4"), ("dropped", "<i4"), ("run_len", "<i4"), ("row0", "<i4"),
                ("run_min_t", "<i4"), ("run_flags", "<i4"), ("run_return", "<f8"), ("run_min_sep", "<f8"))


def row_fields(N, heading=False, clouds=False, terms=False):
    """name -> (dtype, shape of one row) of the [T][S]-major row arrays."""
    f = {"header": ("<i4", (4,)), "pos": ("<f8", (N, 2)), "vel": ("<f8", (N, 2)), "goal": ("<f8", (N, 2)),
         "act": ("<f4", (N, 2)), "reward": ("<f8", (N,)), "done": ("u1", (N,)), "mask": ("u1", (N,)),
         "nearest": ("<f8", (N,)), "nearest_idx": ("<i4", (N,)), "min_sep": ("<f8", ())}
    if heading:
        f["heading"] = ("<f8", (N,))
    if clouds:
        f["clouds"] = ("<f8", (2, 2))
    if terms:
        f["terms"] = ("<f8", (N, 12))       # the reward terms of the step (include/aac_terms.h); zeros in a reset row
    return f


class Trajectories:
    """The downloaded recording of T tracks: ``rows[name]`` is [T][S]..., ``summaries`` is [T][P] of
    ``EPISODE``; row r of track k is valid for r < ``cursor[k]``, summary p for p < ``ep_seen[k]``.

    tracks            the followed env indices, [T]
    dropped           rows that found their track full, [T]
    episodes(track)   the finished episodes (of track index ``track``, or of all tracks in track order)
    min_separation()  their ``min_sep``, in the same order
    """

    def __init__(self, tracks, cursor, ep_seen, dropped, summaries, rows):
        self.tracks = np.asarray(tracks, dtype=np.int32)
        self.cursor = np.asarray(cursor, dtype=np.int32)
        self.ep_seen = np.asarray(ep_seen, dtype=np.int32)
        self.dropped = np.asarray(dropped, dtype=np.int32)
        self.summaries = np.asarray(summaries, dtype=EPISODE)
        self.rows = {k: np.asarray(v) for k, v in rows.items()}
        T = len(self.tracks)
        assert self.summaries.ndim == 2 and self.summaries.shape[0] == T
        for k in ("header", "pos", "vel", "goal", "act", "reward", "done", "mask", "nearest", "nearest_idx", "min_sep"):
            assert k in self.rows and self.rows[k].shape[0] == T, k
        self.S = self.rows["header"].shape[1]
        self.N = self.rows["pos"].shape[2]

    @property
    def terms(self):
        """[T][S][N][12] reward terms of every recorded step (``terms.names()``; the left-to-right sum of
        slots 0..7 is the agent's own reward), or None when the env had no terms buffer."""
        return self.rows.get("terms")

    def episodes(self, track=None):
        """A list of dicts, one per finished episode: the summary fields (``ret``, ``min_sep``,
        ``min_sep_t``, ``row0``, ``rows``, ``len``, ``episode``, ``env``, ``flags``), ``track``,
        ``truncated`` (rows of it were dropped), ``any_done``, ``t`` and ``row_flags`` (from the row
        headers), ``map_idx``, and every row array sliced to the episode's rows (``pos`` [rows][N][2],
        ...; the per-row ``min_sep`` as ``min_sep_row``).  A complete episode has ``len + 1`` rows: the reset row, then one per step."""
        out = []
        for k in (range(len(self.tracks)) if track is None else [int(track)]):
            for p in range(int(self.ep_seen[k])):
                s = self.summaries[k, p]
                ep = {n: (float(s[n]) if n in ("ret", "min_sep") else int(s[n])) for n in EPISODE.names if n != "pad"}
                r0, r1 = ep["row0"], ep["row0"] + ep["rows"]
                ep["track"] = k
                ep["truncated"] = bool(ep["flags"] & EP_DROPPED)
                ep["any_done"] = bool(ep["flags"] & EP_ANY_DONE)
                for name, a in self.rows.items():
                    if name != "header":
                        ep["min_sep_row" if name == "min_sep" else name] = a[k, r0:r1]
                h = self.rows["header"][k, r0:r1]
                ep["t"], ep["row_flags"], ep["map_idx"] = h[:, 1], h[:, 2], h[:, 3]
                out.append(ep)
        return out

    def min_separation(self):
        """Closest approach of every finished episode (the order of ``episodes()``), float64."""
        return np.array([self.summaries[k, p]["min_sep"] for k in range(len(self.tracks))
                         for p in range(int(self.ep_seen[k]))], dtype=np.float64)

    # ------------------------------------------------------------------- files
    def _arrays(self):
        a = {"tracks": self.tracks, "cursor": self.cursor, "ep_seen": self.ep_seen, "dropped": self.dropped,
             "summaries": self.summaries.view(np.uint8).reshape(self.summaries.shape + (EPISODE.itemsize,))}
        a.update({"row_" + k: v for k, v in self.rows.items()})
        return a

    def save(self, path):
        """Write an ``.npz`` (the summaries as raw bytes); ``Trajectories.load`` reads it back equal."""
        np.savez(path, **self._arrays())

    @classmethod
    def load(cls, path):
        with np.load(path) as z:
            a = {k: z[k] for k in z.files}
        summ = np.ascontiguousarray(a["summaries"]).view(EPISODE)[..., 0]
        return cls(a["tracks"], a["cursor"], a["ep_seen"], a["dropped"], summ,
                   {k[4:]: v for k, v in a.items() if k.startswith("row_")})

    def __eq__(self, other):
        """Bit-for-bit: the same arrays with the same bytes."""
        if not isinstance(other, Trajectories):
            return NotImplemented
        a, b = self._arrays(), other._arrays()
        return a.keys() == b.keys() and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
                                            and a[k].tobytes() == b[k].tobytes() for k in a)

    __hash__ = None


class FlightRecorder:
    """Device recorder of T tracks x ``steps`` rows x ``episodes`` summaries for a ``BatchedEnv`` or a
    ``BatchedUAM``.  Call ``after_reset(sel)`` after every (auto-)reset and ``after_step(bufs, actions)``
    after every ``env.step`` and before the reset that follows it, on the env's stream."""

    def __init__(self, env, env_ids=None, steps=64, episodes=1):
        import torch
        from . import _native
        from .uam import BatchedUAM
        self.env, self.uam = env, isinstance(env, BatchedUAM)
        E, N = env.E, env.N
        if not 1 <= N <= MAX_AGENTS:
            raise ValueError("FlightRecorder: 1 <= N <= 64")
        ids = np.arange(E, dtype=np.int32) if env_ids is None else np.asarray(env_ids, dtype=np.int32).reshape(-1)
        if len(ids) < 1 or ids.min() < 0 or ids.max() >= E or len(np.unique(ids)) != len(ids):
            raise ValueError("FlightRecorder: env_ids must be distinct env indices")
        self.T, self.S, self.P, self.N, self.E = len(ids), int(steps), int(episodes), N, E
        if self.S < 1 or self.P < 1:
            raise ValueError("FlightRecorder: steps, episodes >= 1")
        d = self.device = env.device
        self.return_mode = 0 if self.uam else (1 if env.cfg.team_reward else 0)
        self.env_ids = torch.as_tensor(ids, device=d)
        tt = {"<i4": torch.int32, "<f8": torch.float64, "<f4": torch.float32, "u1": torch.uint8}
        self.track = {k: torch.zeros(self.T, dtype=tt[dt], device=d) for k, dt in TRACK_FIELDS}
        # an env with a reward-terms buffer (use_terms_buffer) attached when the recorder is
        # built: its rows are recorded too
        self.terms_src = getattr(env, "terms", None)
        self.rows = {k: torch.zeros(self.T, self.S, *shp, dtype=tt[dt], device=d)
                     for k, (dt, shp) in row_fields(N, heading=self.uam, clouds=self.uam,
                                                    terms=self.terms_src is not None).items()}
        self.summaries = torch.zeros(self.T, self.P, EPISODE.itemsize, dtype=torch.uint8, device=d)
        st = _native.RecordState()
        st.env_ids, st.T, st.S, st.P, st.N = self.env_ids.data_ptr(), self.T, self.S, self.P, N
        for k, t in list(self.track.items()) + list(self.rows.items()):
            if k != "terms":
                setattr(st, k, t.data_ptr())
        st.episodes = self.summaries.data_ptr()
        self._st, self._st_ref = st, ctypes.byref(st)
        L = _native.lib()
        self._call = L.aac_uam_record if self.uam else L.aac_env_record
        self._err = L.aac_uam_last_error if self.uam else L.aac_last_error
        self._steps = {}        # (id(bufs), actions pointer) or ("reset", sel pointer) -> RecordStep
        self._tsteps = {}       # phase, sel pointer -> TermsRecord (the terms rows' own launch)
        self._torch, self._native = torch, _native
        self.reset()

    @classmethod
    def for_env(cls, env, env_ids=None, steps=64, episodes=1):
        """``env_ids`` None: every env.  ``steps``: rows kept per track (reset rows included; a row
        that finds its track full is counted in ``dropped``).  ``episodes``: summaries per track; a
        track that has finished that many is left alone."""
        return cls(env, env_ids, steps, episodes)

    def reset(self):
        """Forget everything recorded: cursors and episode counts to zero, running min-sep to +inf.
        Rows and summaries are not cleared (they are valid only below the cursors)."""
        for t in self.track.values():
            t.zero_()
        self.track["run_min_sep"].fill_(math.inf)

    def _launch_terms(self, phase, sel=None):
        """The terms rows of this step / reset, before the record launch advances the cursors."""
        key = (phase, None if sel is None else sel.data_ptr())
        hit = self._tsteps.get(key)
        if hit is None or hit[0] is not sel:
            a = self._native.TermsRecord()
            a.env_ids, a.cursor, a.ep_seen = (self.env_ids.data_ptr(), self.track["cursor"].data_ptr(),
                                              self.track["ep_seen"].data_ptr())
            a.sel = None if sel is None else sel.data_ptr()
            a.terms, a.rows = self.terms_src.data_ptr(), self.rows["terms"].data_ptr()
            a.T, a.S, a.N, a.E, a.max_episodes, a.phase = self.T, self.S, self.N, self.E, self.P, phase
            hit = self._tsteps[key] = (sel, ctypes.byref(a), a)
        L = self._native.lib()
        rc = L.aac_terms_record(hit[1], self._torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aac_terms_record failed ({rc}): {L.aac_terms_last_error().decode(errors='replace')}")

    def _launch(self, hit):
        rc = self._call(self.env._h, self._st_ref, hit[1], self._torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"aac_record failed ({rc}): {self._err().decode(errors='replace')}")

    def _cached(self, key, owners, fill):
        hit = self._steps.get(key)
        if hit is None or any(a is not b for a, b in zip(hit[0], owners)):
            p = self._native.RecordStep()
            p.return_mode, p.max_episodes = self.return_mode, self.P
            fill(p)
            if len(self._steps) > 64:
                self._steps.clear()
            hit = self._steps[key] = (owners, ctypes.byref(p), p)
        return hit

    def after_reset(self, sel=None):
        """Begin an episode (its t = 0 row) in the tracks whose env has ``sel[e] != 0`` (uint8 [E]; None:
        all), after the reset that redrew them."""
        torch = self._torch
        if sel is not None and (sel.dtype != torch.uint8 or tuple(sel.shape) != (self.E,) or not sel.is_contiguous()):
            raise ValueError("sel: uint8 [E]")

        def fill(p):
            p.phase = PHASE_RESET
            p.sel = None if sel is None else sel.data_ptr()
        if self.terms_src is not None:
            self._launch_terms(PHASE_RESET, sel)
        self._launch(self._cached(("reset", None if sel is None else sel.data_ptr()), (sel,), fill))

    def after_step(self, bufs, actions):
        """Record the step whose outputs are in ``bufs`` (``StepBuffers`` / ``UamBuffers``) and whose
        applied actions were ``actions`` ([E][N][2], float32 or float64), after ``env.step`` and
        before the auto-reset.  The argument struct of a (buffer set, action tensor) pair is built once."""
        torch = self._torch

        def fill(p):
            a, r = actions, bufs.reward
            if a.dtype not in (torch.float32, torch.float64) or tuple(a.shape) != (self.E, self.N, 2) \
                    or not a.is_contiguous():
                raise ValueError(f"actions {tuple(a.shape)} {a.dtype}: expected ({self.E}, {self.N}, 2) float")
            if r.dtype not in (torch.float32, torch.float64) or tuple(r.shape) != (self.E, self.N) \
                    or not r.is_contiguous():
                raise ValueError(f"reward {tuple(r.shape)} {r.dtype}: expected ({self.E}, {self.N}) float")
            for name, shape in (("done", (self.E, self.N)), ("mask", (self.E, self.N)), ("env_done", (self.E,))):
                t = getattr(bufs, name)
                if t.dtype != torch.uint8 or tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"{name} {tuple(t.shape)} {t.dtype}: expected {shape} uint8")
            p.phase = PHASE_STEP
            p.act, p.act_f64 = a.data_ptr(), int(a.dtype == torch.float64)
            p.reward, p.reward_f64 = r.data_ptr(), int(r.dtype == torch.float64)
            p.done, p.mask, p.env_done = bufs.done.data_ptr(), bufs.mask.data_ptr(), bufs.env_done.data_ptr()
        if self.terms_src is not None:
            self._launch_terms(PHASE_STEP)
        self._launch(self._cached((id(bufs), actions.data_ptr()), (bufs, actions), fill))

    def read(self):
        """Download the recording (synchronises)."""
        np_ = lambda t: t.cpu().numpy()      # noqa: E731
        tr = {k: np_(v) for k, v in self.track.items()}
        summ = np_(self.summaries).view(EPISODE)[..., 0]
        return Trajectories(np_(self.env_ids), tr["cursor"], tr["ep_seen"], tr["dropped"], summ,
                            {k: np_(v) for k, v in self.rows.items()})
