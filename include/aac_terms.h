/* aac_terms.h -- reward ledger: the per-term breakdown of the shaped reward, kept on the device
 * (libaac_env.so, MI355X / gfx950).
 *
 * The reference hands its loop the pieces of every reward (ATT/env:2590 step_reward_record,
 * :2596-2620 eps_status_holder; WGRU/env:1666-2039).  With a terms buffer attached
 * (aac_env_set_terms_buffer, aac_env.h) the step kernels of variants 0 (ATT) and 1 (WGRU), and the UAM step
 * kernel (below), store one row of AAC_TERMS_W doubles per (env, agent): double terms[E][N][AAC_TERMS_W].
 *
 * Contribution slots 0..7: what the taken branch added to the agent's own reward, sign included, 0
 * where the branch leaves the term out.  The left-to-right double sum ((((((s0+s1)+s2)+s3)+s4)+s5)+s6)
 * equals, as a value, the per-agent reward the kernel forms (before the team sum, if any).
 *   slot  name       ATT (ATT/env:2414-2458)                  WGRU (WGRU/env:1800-2039)
 *   0     event      -20 bound / collision, +20 goal           -5 bound / building, +5 goal
 *   1     waypoint   0                                         +3: waypoint reached with more to go
 *   2     path       0                                         cross-track reward dref
 *   3     progress   dtg (normal branch only)                  dtg
 *   4     speed      0                                         - small-step penalty
 *   5     building   0                                         - near-building penalty
 *   6     drone      - near-drone penalty (collision, normal)  0
 *   7     reserved   0                                         0
 * Gauge slots 8..11 (not summed into anything):
 *   8 cross_track  cross-track distance (0 in ATT)        9 speed_norm  |v| after the step
 *   10 goal_dist   distance after the step to the point the progress term measures against
 *                  (goal[-1] in ATT, the next waypoint in WGRU)
 *   11 radar_min   the radar minimum the near-building penalty used (0 in ATT)
 * UAM (aac_uam_set_terms_buffer, aac_uam.h; UAM/env:3892-4629), the same slots:
 *   0 event     -crash on a bound crash, a cloud / runway conflict or a drone collision, +50 on the goal
 *               branch; crash = 50 * 2^(collision-bearing doublings among aircraft 0..i of this call)
 *   3 progress  dist_to_goal, 5 building  -near_building, 6 drone  -near_drone = -(ndc * (m * shortest + c))
 *               or -(ndc * 0) with the doubled ndc in effect for this aircraft: normal branch only, else 0
 *   1, 2, 4, 7  0
 *   8 cross_track  distance to the nearest point of the reference line start -> goal
 *   9 speed_norm, 10 goal_dist (to goal[-1]), 11 radar_min (over the 18 rays): every branch
 * A finished env keeps its terminal step's rows: resets (in-launch or not) never write terms.  The
 * exact-threshold fix-up that rewrites a WGRU reward rewrites that row's slots 5 and 11 with it.
 *
 * The ledger (this header) keeps per-episode totals of slots 0..7 in caller-owned device buffers,
 * in the shape of aac_stats.h: one accumulate launch per env step after the step launch on the same
 * stream, a reduce launch when the host asks.  Per env e (unless quota[e] of its episodes finished):
 *   1. run[e][i][k] += terms[e][i][k] in double, every agent i, slot k < 8;
 *   2. if env_done[e]: t[k] = sum_i run[e][i][k], agents in index order; count, sum, sum of squares,
 *      min and max of each t[k] are folded into the totals; run[e] is cleared; ep_count[e] += 1.
 * Determinism as aac_stats.h: workgroup g owns envs [g * AAC_STATS_EPW, (g + 1) * AAC_STATS_EPW),
 * folds its finished episodes over a fixed tree (entry j with j + s, s = 128, 64, .. 1; an env that did
 * not finish counts as 0 / +inf / -inf) into slot g; aac_terms_reduce folds the slots (thread t takes
 * slots t, t + 256, .. in order, then the same tree).  No floating-point atomics: for a fixed E and
 * input sequence the totals are bit-identical between runs and between eager and graph launches.
 * Conventions as aac_env.h; aac_terms_last_error() holds the message of a failed call.
 */
#ifndef AAC_TERMS_H
#define AAC_TERMS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_TERMS_W 12             /* doubles per (env, agent) row */
#define AAC_TERMS_SLOTS 8          /* contribution slots (summed); the rest are gauges */
#define AAC_TERMS_FIELDS 33        /* 8-byte fields of one totals record / slot */
/* the slot names, in row order (aac_terms_names() returns this string) */
#define AAC_TERMS_NAMES "event,waypoint,path,progress,speed,building,drone,reserved,cross_track,speed_norm,goal_dist,radar_min"

/* One totals record; a slot has the same layout.  min / max: +inf / -inf while empty. */
typedef struct {
    int64_t episodes;
    double sum[AAC_TERMS_SLOTS], sqsum[AAC_TERMS_SLOTS], min[AAC_TERMS_SLOTS], max[AAC_TERMS_SLOTS];
} aac_terms_totals;

/* Caller-owned device buffers.  slots must start as zeros with min = +inf, max = -inf
 * (aac_terms_reduce with clear = 1 leaves them so). */
typedef struct {
    double *run;               /* [E][N][AAC_TERMS_SLOTS] running per-agent sums of the current episode */
    int32_t *ep_count;         /* [E] finished episodes (the ledger's own count, for the quota) */
    int64_t *slots;            /* [ceil(E / AAC_STATS_EPW)][AAC_TERMS_FIELDS] */
} aac_terms_state;

/* The inputs of one step (device pointers). */
typedef struct {
    const double *terms;       /* [E][N][AAC_TERMS_W], the buffer attached to the env */
    const uint8_t *env_done;   /* [E] */
    int32_t E, N;              /* 1 <= N <= 256 */
    const int32_t *quota;      /* [E] or NULL */
} aac_terms_step;

const char *aac_terms_last_error(void);
const char *aac_terms_names(void);
int aac_terms_accumulate(const aac_terms_state *state, const aac_terms_step *step, void *stream);
/* Folds the slots into *totals_dev (a device pointer); clear != 0 then empties the slots.  Running
 * state and ep_count stay. */
int aac_terms_reduce(const aac_terms_state *state, int32_t E, aac_terms_totals *totals_dev, int32_t clear,
                     void *stream);

/* Flight recorder companion (aac_record.h): the terms rows of the tracked envs into
 * rows double[T][S][N][AAC_TERMS_W], at the row the aac_record call that FOLLOWS on the same stream
 * writes (row cursor[k] of track k), under that call's rules: a track that has finished
 * max_episodes, an env id outside [0, E) or a full track (cursor[k] >= S) is left alone.  phase
 * AAC_RECORD_STEP (1) copies terms[env_ids[k]]; phase AAC_RECORD_RESET (0) writes a zero row for the
 * tracks with sel[env] != 0 (sel NULL: all).  One launch, capturable; enqueue it before the
 * aac_record / aac_env_record call of the same step, which advances the cursors. */
typedef struct {
    const int32_t *env_ids;    /* [T] */
    const int32_t *cursor, *ep_seen;   /* [T] the recorder's running state */
    const uint8_t *sel;        /* [E] or NULL (reset phase) */
    const double *terms;       /* [E][N][AAC_TERMS_W] (step phase) */
    double *rows;              /* [T][S][N][AAC_TERMS_W] */
    int32_t T, S, N, E, max_episodes, phase;
} aac_terms_record_args;
int aac_terms_record(const aac_terms_record_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_TERMS_H */
