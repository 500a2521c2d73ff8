/* aac_record.h -- flight recorder: device-side trajectories of evaluation rollouts (libaac_env.so,
 * MI355X / gfx950).
 *
 * The reference's eval mode keeps the flown paths (traj_step_list / trajectory_eachPlay, ATT/main:700,
 * for save_gif and view_static_traj) and the per-step status of every aircraft (eps_status_holder,
 * the nearest-neighbour distance behind near_drone_penalty) on the host.  A rollout that never leaves
 * the GPU resets a finished env before the host could look, so these entry points copy the rows on
 * the device: one launch after each env step and one after each reset, on the same stream.
 * Conventions as aac_stats.h: plain pointers, ``stream`` is a hipStream_t passed as void*, 0 or a
 * negative AAC_E* code is returned and aac_record_last_error() holds the message.  There is no handle:
 * the whole state is the caller's buffers.  One launch per call, no synchronisation, capturable.
 *
 * A recorder follows T tracks; track k is env env_ids[k] (distinct, any order).  It keeps up to S rows
 * per track, one per recorded step, struct-of-arrays and [T][S]-major, and up to P episode summaries.
 * One wave owns a track and nothing else writes its rows: no atomics, results bit-identical between
 * runs and between eager and graph launches.
 *
 * Row (track k, row r; N agents):
 *   header   int32[4]     the env's episode counter, t (step within the episode, 0 = the reset row),
 *                         flags (AAC_RECORD_ROW_*), map_idx (0 without a map_idx source: UAM)
 *   pos / vel / goal      double[N][2], copied bit-exactly from the env state
 *   act      float[N][2]  the applied action; aac_uam.h's double actions are CONVERTED to float
 *                         (round to nearest); zero on a reset row
 *   reward   double[N]    float rewards widened exactly; zero on a reset row
 *   done / mask           uint8[N] as the step wrote them; zero on a reset row
 *   nearest  double[N], nearest_idx int32[N]   distance to the nearest other agent and its index
 *   min_sep  double       min over agents of nearest
 *   heading  double[N], clouds double[2][2]    optional (NULL skips them), aac_uam.h only
 * Separation: d2(i,j) = (xi-xj)*(xi-xj) + (yi-yj)*(yi-yj) in double exactly as written (the library
 * is built with -ffp-contract=off); nearest_idx[i] is the lowest j != i attaining the minimum of d2,
 * nearest[i] = sqrt of that minimum.  N = 1: nearest = +inf, nearest_idx = -1, min_sep = +inf.
 *
 * Two phases; track k (env e = env_ids[k]) takes part only while ep_seen[k] < max_episodes.
 *   RESET (sel uint8[E], NULL = all envs), for tracks with sel[e] != 0, after the env's reset:
 *     run_len = 0, run_return = 0, run_flags = 0, run_min_sep = +inf, run_min_t = 0, row0 = cursor;
 *     the t = 0 row is written from the freshly reset state.
 *   STEP, after the env step and before any reset: run_len += 1 and the row with t = run_len is
 *     written; run_return accumulates in double by the aac_stats.h rule (return_mode 1: agent 0's
 *     reward, 0: the sum over agents in index order); if env_done[e], the summary is stored at
 *     episodes[k][ep_seen[k]] and ep_seen[k] += 1.
 *   Either phase: run_min_sep and run_min_t keep the smallest min_sep of the episode's rows and the
 *   first t that attains it (the reset row counts; a dropped row counts too).
 * A row is written at the cursor, which then advances.  With the cursor at S the row is not written,
 * dropped[k] += 1 and the episode is flagged; episode accounting carries on all the same.  Nothing is
 * written outside [k][0..S) of any row buffer or [k][0..P) of the summaries.
 */
#ifndef AAC_RECORD_H
#define AAC_RECORD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_RECORD_MAX_AGENTS 64   /* = AAC_STATS_MAX_AGENTS: one wave per track, lane = agent */
#define AAC_RECORD_RESET 0         /* phases */
#define AAC_RECORD_STEP 1
#define AAC_RECORD_ROW_ENV_DONE 1  /* header flags */
#define AAC_RECORD_ROW_RESET 2
#define AAC_RECORD_EP_ANY_DONE 1   /* summary flags: some agent's done was set on some step */
#define AAC_RECORD_EP_DROPPED 2    /* some row of the episode was dropped */
#define AAC_RECORD_CLOUDS 2        /* C of aac_uam.h */

/* sizes the ctypes binding is checked against */
#define AAC_RECORD_EPISODE_BYTES 48
#define AAC_RECORD_STATE_BYTES 208
#define AAC_RECORD_STEP_BYTES 128

/* One finished episode of a track. */
typedef struct {
    double ret, min_sep;
    int32_t min_sep_t;         /* the first t whose row attains min_sep */
    int32_t row0, rows;        /* its rows are [row0, row0 + rows) of the track */
    int32_t len;               /* steps (rows + dropped rows = len + 1) */
    int32_t episode, env, flags, pad;
} aac_record_episode;

/* Caller-owned device buffers. */
typedef struct {
    const int32_t *env_ids;    /* [T] */
    int32_t T, S, P, N;
    /* running state, [T]: zeros, run_min_sep = +inf */
    int32_t *cursor, *ep_seen, *dropped, *run_len, *row0, *run_min_t, *run_flags;
    double *run_return, *run_min_sep;
    /* rows, [T][S]... */
    int32_t *header;           /* [T][S][4] */
    double *pos, *vel, *goal;  /* [T][S][N][2] */
    float *act;                /* [T][S][N][2] */
    double *reward;            /* [T][S][N] */
    uint8_t *done, *mask;      /* [T][S][N] */
    double *nearest;           /* [T][S][N] */
    int32_t *nearest_idx;      /* [T][S][N] */
    double *min_sep;           /* [T][S] */
    double *heading;           /* [T][S][N] or NULL */
    double *clouds;            /* [T][S][2][2] or NULL */
    aac_record_episode *episodes;   /* [T][P] */
} aac_record_state;

/* The sources of one call (device pointers).  aac_env_record / aac_uam_record overwrite E and the
 * state sources (pos, vel, goal, episode, map_idx, heading, clouds) from the handle. */
typedef struct {
    int32_t phase, E;
    const double *pos, *vel, *goal;    /* [E][N][2] */
    const int32_t *episode;            /* [E] */
    const int32_t *map_idx;            /* [E] or NULL (0) */
    const double *heading, *clouds;    /* [E][N], [E][2][2]; read only where the state has the buffer */
    const void *act;                   /* STEP: float[E][N][2] or double[E][N][2] */
    const void *reward;                /* STEP: float[E][N] or double[E][N] */
    int32_t act_f64, reward_f64;
    const uint8_t *done, *mask, *env_done;   /* STEP: [E][N], [E][N], [E] */
    const uint8_t *sel;                /* RESET: [E] or NULL */
    int32_t return_mode;               /* 1: agent 0's reward; 0: the sum over agents */
    int32_t max_episodes;              /* 1 <= max_episodes <= P */
} aac_record_step;

const char *aac_record_last_error(void);
int aac_record(const aac_record_state *state, const aac_record_step *step, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_RECORD_H */
