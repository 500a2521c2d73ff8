/* aac_sortie.h -- sortie statistics kept on the device (libaac_env.so, MI355X / gfx950).
 *
 * The reference's evaluation "by sortie" (evaluation_by_episode = False, UAM/main:1130-1144 and
 * :1194-1200) puts every aircraft of every finished episode into one class -- crashed into the bound,
 * into an obstacle, into another aircraft, reached its destination, or idle -- and adds two efficiency
 * measures: the flight-distance ratio of the aircraft that reached their goals
 * (obtain_euclidean_dist_list_all_AC, UAM/util:53-68: flown path length over the straight
 * origin-destination distance) and steps_before_collide (UAM/main:360, :1073).  A loop that never
 * leaves the GPU has lost the paths once the device resets the env, so these entry points keep the
 * same tallies in caller-owned device buffers.  Conventions as aac_stats.h: plain pointers, ``stream``
 * is a hipStream_t passed as void*, 0 or a negative AAC_E* code is returned and aac_sortie_last_error()
 * holds the message.  There is no handle: the whole state is the caller's buffers.  No synchronisation,
 * capturable.
 *
 * ONE accumulate call per env step, enqueued after the env step launch and before any reset of that
 * step: the post-step, pre-reset positions must still be in the env state.  A fused
 * aac_env_step_tail(auto_reset = 1) resets the finished envs inside the step launch and leaves nothing
 * to call it on; use aac_env_step, this call, then aac_env_auto_reset.
 *
 * Rule of one accumulate call for env e, unless quota is given and ep_count[e] >= quota[e] (the
 * aac_stats.h rule: both objects count the same episode set).  norm(d) is sqrt(dx*dx + dy*dy) in double,
 * as written, no contraction.  For every aircraft i:
 *   1. if run_len[e] == 0 (the first step of the episode): straight[e][i] = norm(goal - start),
 *      first_seg[e][i] = norm(pos - start), run_dist[e][i] = 0;
 *      otherwise run_dist[e][i] += norm(pos - last_pos[e][i]);
 *   2. last_pos[e][i] = pos;
 *   3. run_flags[e][i] |= mask[e][i];
 *   4. if mask bit ``goal_bit`` is set and reach_step[e][i] == 0: reach_step[e][i] = run_len[e] + 1;
 *   5. run_len[e] += 1 (once per env; len below is the new value);
 *   6. if env_done[e], every aircraft of the env is one finished sortie:
 *      class   the first that holds of run_flags bit bound_bit -> BOUND, obstacle_bit -> OBSTACLE,
 *              drone_bit -> DRONE, goal_bit -> REACHED, else IDLE (the reference's elif order);
 *      flown = (run_dist + first_seg) + reach_margin (the reference's order of additions: the later
 *              segments, then the start segment, then the constant), ratio = flown / straight.  A
 *              REACHED sortie adds its reach_step to reach_step_sum; it enters the double sums and
 *              min / max only if straight > 0 and flown is finite, otherwise degenerate += 1 (it still
 *              counts as reached);
 *      if any done[e][.] is set and len < episode_length (the condition of collision_count in
 *              aac_stats.h): collide_hist[len] += 1 (len is range-checked against hist_len first);
 *      then ep_count[e] += 1 and run_len, run_flags and reach_step of the env are cleared.
 * Bits: aac_env.h (ATT / WGRU) bound 0, drone 1, building (obstacle) 3, goal 5; aac_uam.h bound 0,
 * cloud / runway (obstacle) 1, drone 2, goal 4.
 *
 * Determinism: workgroup g owns envs [g * AAC_SORTIE_EPW, (g + 1) * AAC_SORTIE_EPW); a thread adds the
 * finished sorties of its fixed (env, aircraft) lanes in pass order, the threads are folded over a fixed
 * tree into slot g of ``slots``, which no other workgroup touches; aac_sortie_reduce folds the slots
 * over another fixed tree.  collide_hist takes integer adds only.  No floating-point atomics: for a
 * fixed E, N and input sequence every output is bit-identical between runs and between eager and
 * graph launches.  Nothing is written outside the state's buffers.
 */
#ifndef AAC_SORTIE_H
#define AAC_SORTIE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_SORTIE_EPW 32          /* envs per workgroup (= per slot) */
#define AAC_SORTIE_MAX_AGENTS 64   /* lane = aircraft */
#define AAC_SORTIE_FIELDS 15       /* 8-byte fields of one totals record / slot */

/* sizes the ctypes binding is checked against */
#define AAC_SORTIE_STATE_BYTES 136
#define AAC_SORTIE_STEP_BYTES 104
#define AAC_SORTIE_ROW_BYTES 48

/* One totals record; a slot has the same layout.  sorties = bound + obstacle + drone + reached + idle;
 * degenerate counts the reached sorties left out of the double sums; episodes the finished episodes;
 * reach_step_sum is over the reached sorties, the doubles over the counted ones (reached - degenerate). */
typedef struct {
    int64_t sorties, bound, obstacle, drone, reached, idle, degenerate, episodes, reach_step_sum;
    double ratio_sum, ratio_sqsum, ratio_min, ratio_max;   /* min / max: +inf / -inf while empty */
    double flown_sum, straight_sum;
} aac_sortie_totals;

#define AAC_SORTIE_BOUND 0
#define AAC_SORTIE_OBSTACLE 1
#define AAC_SORTIE_DRONE 2
#define AAC_SORTIE_REACHED 3
#define AAC_SORTIE_IDLE 4

/* One finished sortie of the log.  episode is episode[e] of the step (the env's own counter) or, without
 * one, the env's ep_count before this episode was added; flown and straight are given for every class
 * by the same formula; ratio is NaN unless the sortie entered the sums. */
typedef struct {
    int32_t env, agent, episode, cls, len, reach_step;
    double flown, straight, ratio;
} aac_sortie_row;

/* Caller-owned device buffers.  Everything starts as zeros, slots with ratio_min = +inf and ratio_max =
 * -inf (aac_sortie_reduce with clear = 1 leaves them so).  hist_len >= episode_length + 2.  The log is
 * optional (log = NULL): a ring of the last log_len finished sorties, appended in (call, ascending env,
 * ascending aircraft) order by a second single-workgroup launch; log_meta[0] counts the rows ever
 * appended (write position = count mod log_len), log_meta[1] the accumulate calls so far. */
typedef struct {
    double *straight, *first_seg, *run_dist;   /* [E][N] */
    double *last_pos;          /* [E][N][2] */
    uint8_t *run_flags;        /* [E][N] */
    int32_t *reach_step;       /* [E][N] */
    int32_t *run_len;          /* [E] */
    int32_t *ep_count;         /* [E] */
    int64_t *slots;            /* [ceil(E / AAC_SORTIE_EPW)][AAC_SORTIE_FIELDS] */
    int64_t *collide_hist;     /* [hist_len] */
    int32_t hist_len;
    aac_sortie_row *log;       /* [log_len] or NULL */
    int32_t log_len;
    int64_t *log_meta;         /* [2] */
    uint8_t *fin_flag;         /* [E] scratch: env finished an episode in this call */
    aac_sortie_row *fin_row;   /* [E][N] scratch: its rows */
    int32_t *fin_list;         /* [E + 1] scratch: ordered list of the finished envs */
} aac_sortie_state;

/* The inputs of one step (device pointers): the env state after the step and before any reset, and the
 * step's outputs.  aac_env_sorties / aac_uam_sorties overwrite E, N, pos, start, goal and episode from
 * the handle.  E * N < 2^31. */
typedef struct {
    const double *pos, *start, *goal;       /* [E][N][2] */
    const int32_t *episode;                 /* [E] or NULL: logged with the rows */
    const uint8_t *done, *mask, *env_done;  /* [E][N], [E][N], [E] */
    const int32_t *quota;                   /* [E] or NULL */
    int32_t E, N;                           /* 1 <= N <= AAC_SORTIE_MAX_AGENTS */
    int32_t episode_length;
    int32_t bound_bit, obstacle_bit, drone_bit, goal_bit;   /* 0..7 each */
    int32_t pad;
    double reach_margin;                    /* finite; 5.0 is the literal of UAM/util:66 */
} aac_sortie_step;

const char *aac_sortie_last_error(void);
int aac_sortie_accumulate(const aac_sortie_state *state, const aac_sortie_step *step, void *stream);
/* Folds the slots into *totals_dev (a device pointer, or host memory the device can write); clear != 0
 * then empties the slots and collide_hist (a "per window" report: copy collide_hist first).  Running
 * state, ep_count and the log stay. */
int aac_sortie_reduce(const aac_sortie_state *state, int32_t E, aac_sortie_totals *totals_dev, int32_t clear,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_SORTIE_H */
