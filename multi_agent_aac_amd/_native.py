"""ctypes binding of libaac_env.so (the C ABI declared in include/aac_env.h).

The library must be the in-tree build (``multi_agent_aac_amd/libaac_env.so``, made by
``__graft_entry__.build()``).  There is no fallback: if it is missing or a call fails,
a RuntimeError is raised.  torch is imported first so that the HIP runtime torch ships
(SONAME libamdhip64.so.7) is the one the library binds to, which lets the kernels run on
torch's streams and write into torch tensors.
"""
import ctypes
import os

import torch  # noqa: F401  (load torch's HIP runtime before ours)

_HERE = os.path.dirname(os.path.abspath(__file__))
# AAC_LIB: load another build of the same library (kernel experiments); default = the in-tree build
LIB_PATH = os.environ.get("AAC_LIB") or os.path.join(_HERE, "libaac_env.so")

EXPORTS = (
    "aac_env_create", "aac_env_destroy", "aac_last_error", "aac_env_reset", "aac_env_step", "aac_env_step_tail",
    "aac_env_set_od_bank", "aac_env_set_od_banks", "aac_env_auto_reset", "aac_env_set_reset_compact", "aac_env_use_episode_buffer", "aac_env_get_state", "aac_env_set_state",
    "aac_env_band_max", "aac_astar", "aac_od_bank_build",
    "aac_stats_last_error", "aac_stats_accumulate", "aac_stats_reduce",
    "aac_record_last_error", "aac_record", "aac_env_record", "aac_uam_record",
    "aac_monitor_last_error", "aac_monitor_vec", "aac_monitor_commit",
    "aac_env_set_terms_buffer", "aac_terms_last_error", "aac_terms_names", "aac_terms_accumulate", "aac_terms_reduce",
    "aac_terms_record",
    "aac_clip_last_error", "aac_clip_partials", "aac_clip_sumsq", "aac_adam_flat_clip",
    "aac_env_probe",
    "aac_env_reward_map",
    "aac_uam_reward_map",
    "aac_uam_probe",
    "aac_visits_last_error", "aac_visits_accumulate", "aac_env_visits", "aac_uam_visits",
    "aac_sortie_last_error", "aac_sortie_accumulate", "aac_sortie_reduce", "aac_env_sorties", "aac_uam_sorties",
)

vp = ctypes.c_void_p
i32 = ctypes.c_int32


class EnvCfg(ctypes.Structure):
    _fields_ = [("E", i32), ("N", i32), ("R", i32), ("radar_mode", i32), ("compat", i32), ("team_reward", i32),
                ("max_wp", i32),
                ("episode_length", i32), ("grid_w", i32), ("grid_h", i32), ("n_maps", i32),
                ("dt", ctypes.c_double), ("acc_max", ctypes.c_double), ("vmax", ctypes.c_double),
                ("pB", ctypes.c_double), ("radar_len", ctypes.c_double), ("bound", ctypes.c_double * 4),
                ("cell", ctypes.c_double), ("occ", vp), ("variant", i32)]


class StepOut(ctypes.Structure):
    _fields_ = [(n, vp) for n in ("own", "radar", "nei", "reward", "done", "mask", "env_done", "bbc",
                                  "tcpa", "dcpa", "conf_cur", "conf_pre")]


class StepTail(ctypes.Structure):
    _fields_ = [("ring", vp), ("row_width", i32), ("capacity", ctypes.c_int64), ("pos", ctypes.c_int64),
                ("size", ctypes.c_int64), ("meta", vp), ("n_fields", i32), ("srcs", ctypes.POINTER(vp)),
                ("widths", ctypes.POINTER(i32)), ("dtypes", ctypes.POINTER(i32)), ("zero_rows", vp),
                ("zero_width", i32), ("auto_reset", i32), ("pos_in", vp), ("pos_out", vp)]


class StatsState(ctypes.Structure):        # aac_stats_state (include/aac_stats.h)
    _fields_ = [("run_return", vp), ("run_len", vp), ("run_reach", vp), ("ep_count", vp), ("slots", vp),
                ("log", vp), ("log_len", i32), ("log_meta", vp), ("fin_flag", vp), ("fin_row", vp), ("fin_list", vp)]


class StatsStep(ctypes.Structure):         # aac_stats_step
    _fields_ = [("reward", vp), ("reward_f64", i32), ("done", vp), ("mask", vp), ("env_done", vp), ("bbc", vp),
                ("E", i32), ("N", i32), ("episode_length", i32), ("goal_bit", i32), ("return_mode", i32),
                ("quota", vp), ("step_index", ctypes.c_int64)]


class TermsState(ctypes.Structure):        # aac_terms_state (include/aac_terms.h)
    _fields_ = [("run", vp), ("ep_count", vp), ("slots", vp)]


class TermsStep(ctypes.Structure):         # aac_terms_step
    _fields_ = [("terms", vp), ("env_done", vp), ("E", i32), ("N", i32), ("quota", vp)]


class TermsRecord(ctypes.Structure):       # aac_terms_record_args
    _fields_ = [("env_ids", vp), ("cursor", vp), ("ep_seen", vp), ("sel", vp), ("terms", vp), ("rows", vp),
                ("T", i32), ("S", i32), ("N", i32), ("E", i32), ("max_episodes", i32), ("phase", i32)]


class RecordEpisode(ctypes.Structure):     # aac_record_episode (include/aac_record.h)
    _fields_ = [("ret", ctypes.c_double), ("min_sep", ctypes.c_double)] + \
               [(n, i32) for n in ("min_sep_t", "row0", "rows", "len", "episode", "env", "flags", "pad")]


class RecordState(ctypes.Structure):       # aac_record_state
    _fields_ = [("env_ids", vp), ("T", i32), ("S", i32), ("P", i32), ("N", i32)] + \
               [(n, vp) for n in ("cursor", "ep_seen", "dropped", "run_len", "row0", "run_min_t", "run_flags",
                                  "run_return", "run_min_sep", "header", "pos", "vel", "goal", "act", "reward",
                                  "done", "mask", "nearest", "nearest_idx", "min_sep", "heading", "clouds",
                                  "episodes")]


class RecordStep(ctypes.Structure):        # aac_record_step
    _fields_ = [("phase", i32), ("E", i32)] + \
               [(n, vp) for n in ("pos", "vel", "goal", "episode", "map_idx", "heading", "clouds", "act", "reward")] + \
               [("act_f64", i32), ("reward_f64", i32), ("done", vp), ("mask", vp), ("env_done", vp), ("sel", vp),
                ("return_mode", i32), ("max_episodes", i32)]


class MonitorVecJob(ctypes.Structure):     # aac_monitor_vec_job (include/aac_monitor.h)
    _fields_ = [("g", vp), ("param", vp), ("n", ctypes.c_int64), ("gstride", ctypes.c_int64),
                ("seg_stride", ctypes.c_int64)] + \
               [(n, i32) for n in ("nsplit", "nseg", "order", "col0", "net", "cols")] + \
               [("gscale", ctypes.c_double), ("scratch", vp)]


class MonitorRows(ctypes.Structure):       # aac_monitor_rows
    _fields_ = [("p", vp), ("col_stride", ctypes.c_int64), ("row_stride", ctypes.c_int64)]


class MonitorCommitArgs(ctypes.Structure):  # aac_monitor_commit_args
    _fields_ = [(n, MonitorRows) for n in ("q", "y", "q_a", "reward", "qn", "done")] + \
               [(n, i32) for n in ("done_width", "f64", "A", "B", "R")] + \
               [("a_off", ctypes.c_double), ("gamma", ctypes.c_double)] + \
               [(n, vp) for n in ("scratch", "rec", "ring", "ring_update", "agg", "state")]


class ClipJob(ctypes.Structure):           # aac_clip_job (include/aac_clip.h)
    _fields_ = [(n, vp) for n in ("g", "grad_out", "param", "exp_avg", "exp_avg_sq", "step", "partials", "record")] + \
               [(n, ctypes.c_int64) for n in ("n", "gstride", "seg_stride")] + \
               [(n, i32) for n in ("nsplit", "nseg", "order", "step_add")] + \
               [(n, ctypes.c_double) for n in ("gscale", "max_norm", "lr", "beta1", "beta2", "eps")]


class ProbeOut(ctypes.Structure):          # aac_probe_out (include/aac_probe.h)
    _fields_ = [(n, vp) for n in ("dist", "point", "end", "kind", "id")]


class UamProbeOut(ctypes.Structure):       # aac_uam_probe_out (include/aac_uam_probe.h)
    _fields_ = [(n, vp) for n in ("dist", "point", "end", "kind", "id")]


class RmapOut(ctypes.Structure):           # aac_rmap_out (include/aac_rmap.h)
    _fields_ = [(n, vp) for n in ("reward", "terms", "mask", "done", "bbc")]


class UamRmapOut(ctypes.Structure):        # aac_uam_rmap_out (include/aac_uam_rmap.h)
    _fields_ = [(n, vp) for n in ("reward", "terms", "mask", "done", "bbc", "flags", "rays")]


class VisitsState(ctypes.Structure):       # aac_visits_state (include/aac_visits.h)
    _fields_ = [("pos_hist", vp), ("act_hist", vp), ("counters", vp)] + \
               [(n, i32) for n in ("GX", "GY", "A", "n_maps")] + \
               [(n, ctypes.c_double) for n in ("x0", "x1", "y0", "y1", "a0", "a1")]


class VisitsStep(ctypes.Structure):        # aac_visits_step
    _fields_ = [(n, vp) for n in ("pos", "act", "episode", "map_idx", "sel")] + \
               [(n, i32) for n in ("act_f64", "E", "N", "explore_until")]


class SortieState(ctypes.Structure):       # aac_sortie_state (include/aac_sortie.h)
    _fields_ = [(n, vp) for n in ("straight", "first_seg", "run_dist", "last_pos", "run_flags", "reach_step",
                                  "run_len", "ep_count", "slots", "collide_hist")] + \
               [("hist_len", i32), ("log", vp), ("log_len", i32)] + \
               [(n, vp) for n in ("log_meta", "fin_flag", "fin_row", "fin_list")]


class SortieStep(ctypes.Structure):        # aac_sortie_step
    _fields_ = [(n, vp) for n in ("pos", "start", "goal", "episode", "done", "mask", "env_done", "quota")] + \
               [(n, i32) for n in ("E", "N", "episode_length", "bound_bit", "obstacle_bit", "drone_bit", "goal_bit",
                                   "pad")] + \
               [("reach_margin", ctypes.c_double)]


_lib = None


def lib():
    """Load libaac_env.so (in-tree) and declare signatures.  Raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH)
    L.aac_last_error.restype = ctypes.c_char_p
    L.aac_env_create.argtypes = [ctypes.POINTER(EnvCfg), ctypes.c_int, ctypes.POINTER(vp)]
    L.aac_env_destroy.argtypes = [vp]
    L.aac_env_destroy.restype = None
    L.aac_env_reset.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.POINTER(StepOut), vp]
    L.aac_env_step.argtypes = [vp, vp, ctypes.POINTER(StepOut), vp]
    L.aac_env_step_tail.argtypes = [vp, vp, ctypes.POINTER(StepOut), ctypes.POINTER(StepTail), vp]
    L.aac_env_set_od_bank.argtypes = [vp, vp, vp, vp, i32, ctypes.c_uint64]
    L.aac_env_set_od_banks.argtypes = [vp, i32, vp, vp, vp, vp, ctypes.c_uint64]
    L.aac_env_auto_reset.argtypes = [vp, vp, ctypes.POINTER(StepOut), vp]
    L.aac_env_set_reset_compact.argtypes = [ctypes.c_int32]
    L.aac_env_set_reset_compact.restype = None
    L.aac_env_use_episode_buffer.argtypes = [vp, vp, vp]
    if hasattr(L, "aac_env_band_max") or not os.environ.get("AAC_LIB"):   # (older A/B builds lack it)
        L.aac_env_band_max.argtypes = [vp, vp, vp, vp]
    L.aac_env_get_state.argtypes = [vp] + [vp] * 13 + [vp]
    L.aac_env_set_state.argtypes = [vp] + [vp] * 13 + [vp]
    L.aac_astar.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, i32]
    L.aac_od_bank_build.argtypes = [vp, i32, i32, vp, ctypes.c_double, i32, ctypes.c_uint64, i32, vp, vp, vp]
    if hasattr(L, "aac_stats_accumulate") or not os.environ.get("AAC_LIB"):
        L.aac_stats_last_error.restype = ctypes.c_char_p
        L.aac_stats_accumulate.argtypes = [ctypes.POINTER(StatsState), ctypes.POINTER(StatsStep), vp]
        L.aac_stats_reduce.argtypes = [ctypes.POINTER(StatsState), i32, vp, i32, vp]
    if hasattr(L, "aac_record") or not os.environ.get("AAC_LIB"):
        rec = [ctypes.POINTER(RecordState), ctypes.POINTER(RecordStep), vp]
        L.aac_record_last_error.restype = ctypes.c_char_p
        L.aac_uam_last_error.restype = ctypes.c_char_p
        L.aac_record.argtypes = rec
        L.aac_env_record.argtypes = [vp] + rec
        L.aac_uam_record.argtypes = [vp] + rec
    if hasattr(L, "aac_monitor_vec") or not os.environ.get("AAC_LIB"):
        L.aac_monitor_last_error.restype = ctypes.c_char_p
        L.aac_monitor_vec.argtypes = [ctypes.POINTER(MonitorVecJob), i32, i32, vp]
        L.aac_monitor_commit.argtypes = [ctypes.POINTER(MonitorCommitArgs), vp]
    if hasattr(L, "aac_terms_accumulate") or not os.environ.get("AAC_LIB"):
        L.aac_env_set_terms_buffer.argtypes = [vp, vp]
        L.aac_terms_last_error.restype = ctypes.c_char_p
        L.aac_terms_names.restype = ctypes.c_char_p
        L.aac_terms_accumulate.argtypes = [ctypes.POINTER(TermsState), ctypes.POINTER(TermsStep), vp]
        L.aac_terms_reduce.argtypes = [ctypes.POINTER(TermsState), i32, vp, i32, vp]
        L.aac_terms_record.argtypes = [ctypes.POINTER(TermsRecord), vp]
    if hasattr(L, "aac_clip_sumsq") or not os.environ.get("AAC_LIB"):
        L.aac_clip_last_error.restype = ctypes.c_char_p
        L.aac_clip_partials.argtypes = [ctypes.c_int64]
        L.aac_clip_partials.restype = ctypes.c_int64
        L.aac_clip_sumsq.argtypes = [ctypes.POINTER(ClipJob), i32, i32, vp]
        L.aac_adam_flat_clip.argtypes = [ctypes.POINTER(ClipJob), i32, i32, vp]
    if hasattr(L, "aac_env_probe") or not os.environ.get("AAC_LIB"):
        L.aac_env_probe.argtypes = [vp, vp, vp, ctypes.c_int64, vp, ctypes.POINTER(ProbeOut), vp]
    if hasattr(L, "aac_env_reward_map") or not os.environ.get("AAC_LIB"):
        L.aac_env_reward_map.argtypes = [vp, vp, vp, vp, vp, vp, ctypes.c_int64, ctypes.POINTER(RmapOut), vp]
    if hasattr(L, "aac_uam_reward_map") or not os.environ.get("AAC_LIB"):
        L.aac_uam_reward_map.argtypes = [vp, vp, vp, vp, vp, vp, vp, ctypes.c_int64, ctypes.POINTER(UamRmapOut), vp]
    if hasattr(L, "aac_uam_probe") or not os.environ.get("AAC_LIB"):
        L.aac_uam_probe.argtypes = [vp, vp, vp, vp, ctypes.c_int64, vp, ctypes.POINTER(UamProbeOut), vp]
    if hasattr(L, "aac_visits_accumulate") or not os.environ.get("AAC_LIB"):
        vis = [ctypes.POINTER(VisitsState), ctypes.POINTER(VisitsStep), vp]
        L.aac_visits_last_error.restype = ctypes.c_char_p
        L.aac_visits_accumulate.argtypes = vis
        L.aac_env_visits.argtypes = [vp] + vis
        L.aac_uam_visits.argtypes = [vp] + vis
    if hasattr(L, "aac_sortie_accumulate") or not os.environ.get("AAC_LIB"):
        sor = [ctypes.POINTER(SortieState), ctypes.POINTER(SortieStep), vp]
        L.aac_sortie_last_error.restype = ctypes.c_char_p
        L.aac_sortie_accumulate.argtypes = sor
        L.aac_sortie_reduce.argtypes = [ctypes.POINTER(SortieState), i32, vp, i32, vp]
        L.aac_env_sorties.argtypes = [vp] + sor
        L.aac_uam_sorties.argtypes = [vp] + sor
    for name in EXPORTS:
        if os.environ.get("AAC_LIB") and not hasattr(L, name):
            continue          # an A/B experiment build of an earlier revision
        getattr(L, name)
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        msg = lib().aac_last_error().decode(errors="replace")
        raise RuntimeError(f"{what} failed ({rc}): {msg}")
    return rc
