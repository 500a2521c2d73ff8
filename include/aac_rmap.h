/* aac_rmap.h -- reward map of the ATT / WGRU environment (libaac_env.so): ss_reward evaluated at any
 * test position.  The reference's training loops carry a generate_reward_map switch (ATT/main:255-354,
 * WGRU/ma_main:494-...): a 50 x 50 grid over the map bound, env.ss_reward(..., pos_to_test) per point
 * (ATT/env:2133-2138, WGRU/env:1687-1692: drone 0 only, pos = pre_pos = xy), reward[0] drawn as a heat
 * map.  aac_env_reward_map is that evaluation as one launch over M rows.
 *
 * Row m holds what ss_reward would hand agent agent[m] of env env_idx[m] if it now stood at points[m]
 * with pre_pos = pre[m] (pre NULL: pre_pos = points[m], the reference's map mode).  Everything else is
 * the handle's live state: the subject's velocity, goal, waypoint list with its wp_cur index (ATT) or
 * removed-waypoint bits (WGRU) and start; the other agents' positions; the env's map of the stack.
 * The variant is the handle's: the ATT reward of the step's phase 3-4 (ATT/env:2133-2603: event,
 * progress, near-drone penalty) or the WGRU reward (WGRU/env:1666-2039: waypoint search, progress to the
 * found waypoint, cross-track, small-step and near-building penalties).  Both are the step kernel's own
 * device functions, compiled for the map with their state writes left out.
 *
 * WGRU near-building penalty: with rmin NULL the launch computes the 18-ray obstacle radar at the point,
 * its threshold-band rays decided exactly (as the band fix and aac_env_probe do), so the minimum is the
 * one a step landing there ends up with after its fix-up.  A given rmin[m] is used verbatim.
 *
 * Read-only: the launch writes nothing but ``out`` -- no waypoint pop, no reach or wall counter, no goal
 * rewrite, no band or fix-up list entry.  This departs from the reference, whose sweep leaves drone 0 on
 * the last grid point, pops WGRU waypoints as it passes them and drops the +3 waypoint bonus in map
 * mode (WGRU/env:2004): here every row sees the same state and slot 1 holds what a step would earn.
 */
#ifndef AAC_RMAP_H
#define AAC_RMAP_H

#include <stdint.h>

#include "aac_env.h"
#include "aac_terms.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_RMAP_OUT_BYTES 40    /* sizeof(aac_rmap_out), for bindings in other languages */

/* Caller-owned device outputs of M rows. */
typedef struct {
    double  *reward;  /* [M]     the subject's own reward (before any team sum) */
    double  *terms;   /* [M][AAC_TERMS_W] rows as include/aac_terms.h, or NULL */
    uint8_t *mask;    /* [M]     the step's mask bits (aac_env.h: bound, drone, goal, building, wp, check_goal) */
    uint8_t *done;    /* [M] */
    uint8_t *bbc;     /* [M][4]  bound_building_check as this agent alone would set it */
} aac_rmap_out;

/* points double[M][2]; pre double[M][2] or NULL; env_idx int32[M] or NULL (env 0); agent int32[M] or NULL
 * (agent 0); rmin double[M] or NULL: all device pointers, the double arrays 8-byte aligned.  env_idx /
 * agent values outside the handle's range are clamped into it.  One launch on ``stream``, no
 * synchronisation, capturable; valid after aac_env_step / reset / auto_reset on the same stream.
 * M < 1 or a NULL points / out->reward / mask / done / bbc returns AAC_E_INVALID (aac_last_error()). */
int aac_env_reward_map(aac_env *env, const double *points, const double *pre, const int32_t *env_idx,
                       const int32_t *agent, const double *rmin, int64_t M, const aac_rmap_out *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_RMAP_H */
