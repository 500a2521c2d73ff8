/* aac_monitor.h -- the learner's records kept on the device (libaac_env.so, MI355X / gfx950).
 *
 * The reference logs, per gradient iteration of update_myown, the critic / actor loss (c_loss / a_loss,
 * ATT/main:575-580), the target Q before and after the reward with the min / max of each
 * (single_eps_critic_cal_record, ATT/maddpg:372-379) and every parameter's gradient norm with a NaN /
 * Inf flag (has_gradients, ATT/maddpg:442-453) -- on the host.  These entry points keep the same
 * quantities in caller-owned device buffers, fed by small launches inside the update's launch list,
 * so they also run inside the captured update and whole-step graphs.  Conventions as aac_stats.h: plain
 * pointers, ``stream`` is a hipStream_t passed as void*, 0 or a negative AAC_E* code is returned and
 * aac_monitor_last_error() holds the message; there is no handle, the whole state is the caller's
 * buffers (torch tensors; a checkpoint saves them as is).
 *
 * Determinism: no floating-point atomics and no "last block done" tickets.  aac_monitor_vec writes
 * per-workgroup partials into fixed slots of ``scratch``; aac_monitor_commit, a later launch on the same
 * stream, folds the slots over a fixed tree of the slot index.  The grid sizes are the constants below,
 * never functions of the device: for fixed inputs the records are bit-identical between runs, between
 * machines and between eager and graph launches.
 *
 * One update = A columns (ATT: the N gradient iterations; GRU: the N agents; UAM: 1) of
 * AAC_MONITOR_FIELDS doubles each.  Field order of a column's record:
 *
 *    0 loss_q          mean (q - y)^2 over the finite rows
 *    1 loss_a          a_off - mean q_a
 *    2 q_mean   3 q_min   4 q_max         the critic's Q(s, a) of the critic step
 *    5 y_mean   6 y_min   7 y_max         the TD target (tar_Q_after_rew)
 *    8 r_mean   9 r_min  10 r_max         the reward of the TD target
 *   11 td_absmax       max |q - y|
 *   12 pre_min 13 pre_max                 (gamma * qn) * (1 - any_done) evaluated in float in that
 *                                         order (tar_Q_before_rew); NaN where qn is not supplied
 *   14 rows_nonfinite  rows with a non-finite q, y or q_a (left out of every sum, min and max above;
 *                      the means divide by the number of finite rows)
 *   15 critic_grad_sumsq   16 critic_grad_absmax   17 critic_grad_nonfinite
 *   18 critic_param_sumsq  19 critic_param_absmax  20 critic_param_nonfinite
 *   21 actor_grad_sumsq    22 actor_grad_absmax    23 actor_grad_nonfinite
 *   24 actor_param_sumsq   25 actor_param_absmax   26 actor_param_nonfinite
 *
 * The sums of squares and maxima run over the finite elements, the *_nonfinite fields count the others.
 * Norms are square roots of the sums of squares and are taken by the host.
 */
#ifndef AAC_MONITOR_H
#define AAC_MONITOR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_MONITOR_FIELDS 27
#ifndef AAC_MONITOR_VEC_WG
#define AAC_MONITOR_VEC_WG 64      /* workgroups (= scratch slots) per segment of a vec job */
#endif
#define AAC_MONITOR_VEC_VALUES 6   /* doubles per slot: grad sumsq, absmax, nonfinite; param the same */
#define AAC_MONITOR_NETS 2         /* 0 critic, 1 actor */
#define AAC_MONITOR_MAX_COLS 64
#define AAC_MONITOR_AGG 5          /* running aggregates per field and column: count, sum, sumsq, min, max */

#define AAC_MONITOR_F_ROWS_NONFINITE 14
#define AAC_MONITOR_F_NET0 15      /* first of the six per-network fields of net 0; net 1 follows */

/* One network's gradient and parameters as ``nseg`` equal segments of ``n`` elements (float, or double
 * with f64).  The gradient is the sum of ``nsplit`` partial copies ``gstride`` elements apart, formed in
 * the element type: order 0 sums the copies 0, 1, 2, ... in sequence (aac_sum64_partials, aac_adam64_sum
 * and the scalar float Adam); order 1 sums the four groups s % 4 each in sequence and then
 * (g0 + g1) + (g2 + g3) (the copy-parallel float Adam / aac_sum_partials; aac_copy_sum_order in
 * aac_fused.h says which of the two the float kernels take for a set of copies, and
 * csrc/aac_copysum.h holds both sums for every kernel).  The sum is multiplied by
 * gscale in the element type.  Segment s starts at g + s * seg_stride and param + s * seg_stride and
 * lands in column col0 + s; its AAC_MONITOR_VEC_WG slots of AAC_MONITOR_VEC_VALUES doubles are
 * scratch[((col0 + s) * AAC_MONITOR_NETS + net) * AAC_MONITOR_VEC_WG + w].  Pointers need only the
 * element type's alignment: 16-byte loads are used where the addresses allow. */
typedef struct {
    const void *g, *param;
    int64_t n, gstride, seg_stride;
    int32_t nsplit, nseg, order, col0, net, cols;   /* cols: columns of scratch (col0 + nseg <= cols) */
    double gscale;
    double *scratch;
} aac_monitor_vec_job;

/* B rows of one field per column: row b of column c is p[c * col_stride + b * row_stride]. */
typedef struct {
    const void *p;
    int64_t col_stride, row_stride;
} aac_monitor_rows;

/* The end of an update: the record of its A columns from the row fields and the vec partials, written to
 * ring[counter % R] with ring_update[counter % R] = counter; every finite field value added to the
 * aggregates agg[k][c][f] (k: count, sum, sum of squares, min, max); state[1] (the first non-finite
 * update, -1 while there is none) set to the counter if it holds -1 and any *_nonfinite field of the
 * record is non-zero; state[0] (the counter) incremented.  No argument varies between updates. */
typedef struct {
    aac_monitor_rows q, y, q_a, reward;
    aac_monitor_rows qn;           /* p = NULL: no pre-reward target */
    aac_monitor_rows done;         /* [B][done_width] rows per column (with qn); 1.0 = done */
    int32_t done_width, f64, A, B, R;
    double a_off, gamma;
    const double *scratch;         /* [A][AAC_MONITOR_NETS][AAC_MONITOR_VEC_WG][AAC_MONITOR_VEC_VALUES] */
    double *rec;                   /* [A][AAC_MONITOR_FIELDS] staging of the record between the two launches */
    double *ring;                  /* [R][A][AAC_MONITOR_FIELDS] */
    int64_t *ring_update;          /* [R] */
    double *agg;                   /* [AAC_MONITOR_AGG][A][AAC_MONITOR_FIELDS] */
    int64_t *state;                /* [2]: update counter, first non-finite update */
} aac_monitor_commit_args;

const char *aac_monitor_last_error(void);
/* One launch over one or two jobs (njobs); f64: double elements. */
int aac_monitor_vec(const aac_monitor_vec_job *jobs, int32_t njobs, int32_t f64, void *stream);
/* Two launches: one workgroup per column for the rows, one workgroup for the ring and the aggregates. */
int aac_monitor_commit(const aac_monitor_commit_args *args, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_MONITOR_H */
