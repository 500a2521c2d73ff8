/* aac_visits.h -- exploration maps: visit and action histograms kept on the device (libaac_env.so,
 * MI355X / gfx950).
 *
 * The reference builds two diagnostics from host lists a loop that never leaves the GPU cannot keep:
 * display_exploration_expolitation (ATT/util:776-866, UAM/util:1484), a 50-bin heat map of every
 * position flown in training, split into "explore" episodes (epsIDX <= eps_period) and "exploit"
 * episodes, and action_selection_statistics (ATT/util:869-897, UAM/util:1572), a 20 x 20 2-D histogram
 * of every action taken.  These entry points keep the arrays behind both in caller-owned device
 * buffers: one accumulate launch per env step, enqueued between the act launch and the env step launch
 * on the same stream, so that a row is the position an action was taken from together with that action.
 * Conventions as aac_stats.h: plain pointers, ``stream`` is a hipStream_t passed as void*, 0 or a
 * negative AAC_E* code is returned and aac_visits_last_error() holds the message.  There is no handle:
 * the whole state is the caller's buffers.  One launch per call, no synchronisation, capturable.
 *
 * Rule of one accumulate call, per row (env e, agent i) of an env with sel[e] != 0 (sel NULL: every env):
 *   map    = map_idx[e] (0 without map_idx).  A map outside [0, n_maps) makes the row count nowhere
 *            except counters[0][3] (+= 1).
 *   period = episode[e] <= explore_until ? 0 : 1, the comparison the noise schedules make on the env's
 *            own 1-based episode counter; plane = 2 * map + period.
 *   counters[plane][0] (samples) += 1.
 *   Position (x, y) = pos[e][i]: if x is in [x0, x1] and y in [y0, y1], pos_hist[plane][bx][by] += 1,
 *            else (either coordinate outside its range, or not finite) counters[plane][1] (pos_outside)
 *            += 1 and no bin changes.
 *   Action (u, v) = act[e][i], a float widened to double exactly: if both are in [a0, a1],
 *            act_hist[period][bu][bv] += 1, else counters[plane][2] (act_outside) += 1 and no bin changes.
 * Bins of one axis with G bins over [lo, hi], all in double with no contraction:
 *   edge[k] = lo + k * ((hi - lo) / G) for k < G, edge[G] = hi  (np.linspace(lo, hi, G + 1));
 *   v falls in bin k iff edge[k] <= v < edge[k + 1]; the last bin is closed (v == hi gives bin G - 1).
 *   This is np.histogram2d(x, y, bins=[edges_x, edges_y]).  The bin is a floor guess corrected against
 *   the neighbouring edges; the range test comes before any float-to-integer conversion or index
 *   arithmetic, so no index is ever formed from an unchecked value.
 *
 * Determinism: every sum is an integer add, and integer adds commute.  For a given input sequence the
 * tables are bit-identical between runs and between eager and graph launches.  No floating-point atomics.
 * Nothing is written outside the three tables.
 */
#ifndef AAC_VISITS_H
#define AAC_VISITS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_VISITS_MAX_A 32        /* action bins per axis: the workgroup's table is uint32 [2][A][A] in LDS */
#define AAC_VISITS_MAX_G 65536     /* position bins per axis */
#define AAC_VISITS_CHUNK 1024      /* consecutive rows of [E * N] per workgroup */
#define AAC_VISITS_COUNTERS 4      /* per plane: samples, pos_outside, act_outside, reserved */

/* sizes the ctypes binding is checked against */
#define AAC_VISITS_STATE_BYTES 88
#define AAC_VISITS_STEP_BYTES 56

/* Caller-owned device buffers, zero-initialised, and the geometry: GX, GY in [1, AAC_VISITS_MAX_G],
 * A in [1, AAC_VISITS_MAX_A], n_maps >= 1; finite ranges x0 < x1, y0 < y1, a0 < a1 (the facades pass
 * the env's bound and [-1, 1]).  planes = 2 * n_maps. */
typedef struct {
    int64_t *pos_hist;         /* [planes][GX][GY], plane = 2 * map + period */
    int64_t *act_hist;         /* [2][A][A], one table per period */
    int64_t *counters;         /* [planes][AAC_VISITS_COUNTERS] */
    int32_t GX, GY, A, n_maps;
    double x0, x1, y0, y1, a0, a1;
} aac_visits_state;

/* The inputs of one call (device pointers).  pos and a double act are 16-byte aligned, a float act
 * 8-byte aligned.  aac_env_visits / aac_uam_visits overwrite pos, episode, map_idx and E from the
 * handle.  E * N < 2^31. */
typedef struct {
    const double *pos;         /* [E][N][2] */
    const void *act;           /* float[E][N][2] or double[E][N][2] */
    const int32_t *episode;    /* [E] */
    const int32_t *map_idx;    /* [E] or NULL (0) */
    const uint8_t *sel;        /* [E] or NULL (every env) */
    int32_t act_f64;           /* 1: double (aac_uam.h) */
    int32_t E, N;
    int32_t explore_until;     /* the last episode of the "explore" period */
} aac_visits_step;

const char *aac_visits_last_error(void);
int aac_visits_accumulate(const aac_visits_state *state, const aac_visits_step *step, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_VISITS_H */
