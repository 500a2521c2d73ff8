/* aac_stats.h -- episode statistics kept on the device (libaac_env.so, MI355X / gfx950).
 *
 * The reference tallies every finished episode on the host (ATT/main:563-637: score_history,
 * collision_count, crash_to_bound / _building / _drone, crash_due_to_nearest, all_steps_used,
 * one / two / all_drone_reach), which a loop that never leaves the GPU cannot do.  These entry
 * points keep the same tallies in caller-owned device buffers: one accumulate launch per env step,
 * enqueued after the step (tail) launch on the same stream, and a reduce launch when the host asks.
 * Conventions as aac_env.h: plain pointers, ``stream`` is a hipStream_t passed as void*, 0 or a
 * negative AAC_E* code is returned and aac_stats_last_error() holds the message.  There is no
 * handle: the whole state is the caller's buffers (torch tensors; a checkpoint saves them as is).
 *
 * Per-env rule of one accumulate call (env e, unless quota[e] episodes of it have finished):
 *   1. run_return[e] += reward[e][i] in double, i = 0..N-1 in order (return_mode 0), or
 *      run_return[e] += reward[e][0] (return_mode 1, the team reward of ATT/main:431-432);
 *   2. run_len[e] += 1; run_reach[e] |= bit i for every agent i with mask[e][i] bit ``goal_bit`` set;
 *   3. if env_done[e]: the episode (return = run_return, len = run_len) is added to the totals,
 *      ep_count[e] += 1, and run_return / run_len / run_reach are cleared.
 * End reason (exclusive, ATT/main:448-462): timeout if episode_length < len; else crash if any
 * done[e][i]; else goal.  Crash subtype (ATT/main:581-595): if any done and len < episode_length,
 * collision_count += 1 and the first of bbc[0] -> bound, bbc[1] -> building, bbc[2] -> drone (and
 * nearest if bbc[3]) counts; otherwise all_steps_used += 1.  reach_hist[popcount(run_reach)] += 1.
 *
 * Determinism: workgroup g owns envs [g * AAC_STATS_EPW, (g + 1) * AAC_STATS_EPW) and adds its
 * finished episodes, reduced over a fixed tree, into slot g of ``slots``; aac_stats_reduce folds the
 * slots over another fixed tree.  No floating-point atomics: for a fixed E and input sequence the
 * totals are bit-identical between runs and between eager and graph launches.
 */
#ifndef AAC_STATS_H
#define AAC_STATS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_STATS_EPW 256          /* envs per workgroup (= per slot) */
#define AAC_STATS_MAX_AGENTS 64
#define AAC_STATS_FIELDS 81        /* 8-byte fields of one totals record / slot */

/* One totals record; a slot has the same layout.  under_quota is a level, not a tally: the number of
 * envs whose finished-episode count was below its quota after the last accumulate call (E without a
 * quota); a clear leaves it. */
typedef struct {
    int64_t episodes, steps, timeout, crash, goal, collision_count, crash_bound, crash_building, crash_drone,
        crash_nearest, all_steps_used, under_quota;
    double return_sum, return_sqsum, return_min, return_max;   /* min / max: +inf / -inf while empty */
    int64_t reach_hist[AAC_STATS_MAX_AGENTS + 1];
} aac_stats_totals;

#define AAC_STATS_TIMEOUT 0
#define AAC_STATS_CRASH 1
#define AAC_STATS_GOAL 2
/* crash subtype of a log row: 0 all_steps_used, 1 bound, 2 building, 3 drone, 4 drone + nearest,
 * 5 a collision with no bbc flag set (counted in collision_count only) */

/* One finished episode of the log (32 bytes). */
typedef struct {
    double ret;
    int64_t step;          /* the accumulate call's step index */
    int32_t len, env, reason;
    int16_t crash, reach;  /* crash subtype, popcount(run_reach) */
} aac_stats_row;

/* Caller-owned device buffers.  slots must start as zeros with return_min = +inf, return_max = -inf
 * (aac_stats_reduce with clear = 1 leaves them so).  The log is optional (log = NULL): a ring of the
 * last log_len finished episodes, appended in (step, ascending env) order by a second
 * single-workgroup launch; log_meta[0] counts the rows ever appended (write position = count mod
 * log_len), log_meta[1] the accumulate calls so far. */
typedef struct {
    double *run_return;        /* [E] */
    int32_t *run_len;          /* [E] */
    uint64_t *run_reach;       /* [E] */
    int32_t *ep_count;         /* [E] */
    int64_t *slots;            /* [ceil(E / AAC_STATS_EPW)][AAC_STATS_FIELDS] */
    aac_stats_row *log;        /* [log_len] or NULL */
    int32_t log_len;
    int64_t *log_meta;         /* [2] */
    uint8_t *fin_flag;         /* [E] scratch: env finished an episode in this call */
    aac_stats_row *fin_row;    /* [E] scratch: its row */
    int32_t *fin_list;         /* [E + 1] scratch: ordered list of the finished envs */
} aac_stats_state;

/* The inputs of one step (device pointers; the outputs of aac_env_step* / aac_uam_step). */
typedef struct {
    const void *reward;        /* float[E][N] or double[E][N] */
    int32_t reward_f64;        /* 1: double (aac_uam.h) */
    const uint8_t *done, *mask, *env_done, *bbc;   /* [E][N], [E][N], [E], [E][4] */
    int32_t E, N;              /* 1 <= N <= AAC_STATS_MAX_AGENTS */
    int32_t episode_length;
    int32_t goal_bit;          /* 5 for aac_env.h, 4 for aac_uam.h */
    int32_t return_mode;       /* 1: agent 0's reward; 0: the sum over agents */
    const int32_t *quota;      /* [E] or NULL */
    int64_t step_index;        /* logged with the rows; < 0: log_meta[1] (the calls so far) */
} aac_stats_step;

const char *aac_stats_last_error(void);
int aac_stats_accumulate(const aac_stats_state *state, const aac_stats_step *step, void *stream);
/* Folds the slots into *totals_dev (a device pointer, or host memory the device can write); clear != 0
 * then empties the slots (a "per window" report).  Running state and ep_count stay. */
int aac_stats_reduce(const aac_stats_state *state, int32_t E, aac_stats_totals *totals_dev, int32_t clear,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_STATS_H */
