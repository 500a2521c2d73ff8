/* aac_uam_rmap.h -- reward map of the UAM environment (libaac_env.so): ss_reward_Mar_changeskin evaluated
 * at any test position.  The UAM reference carries the same generate_reward_map sweep as the ATT and WGRU
 * variants (UAM/main:434-505: a 50 x 50 np.linspace grid over the bound, env.ss_reward_Mar_changeskin(...,
 * pos_to_test) per point, UAM/env:3939-3944: drone 0 only, pos = pre_pos = xy; reward[0] as a heat map).
 * aac_uam_reward_map is that evaluation as one launch over M rows; aac_rmap.h is the ATT / WGRU one.
 *
 * Row m holds what phases 5-6 of the step kernel would hand aircraft agent[m] of env env_idx[m] if it now
 * stood at points[m] with pre_pos = pre[m] (pre NULL: pre_pos = points[m], the reference's map mode).
 * Everything else is the handle's live state: the subject's vel, goal, start and reach; the other
 * aircraft's pos and reach; the env's two cloud centres as they stand (no drift); the bound, the runway.
 * Phase 5 after the neighbour walk is the step kernel's own device function (phase5_tail); the neighbour
 * scan, the radar and the single-aircraft phase 6 are the map's.
 *
 *   radar      rmin NULL: the 18-ray fp64 radar at the point (ray length, runway, the four bound segments,
 *              both clouds, the N - 1 other aircraft), the step kernel's functions in its expression order:
 *              at a step's own (pos, state) the row equals the step's radar row bit for bit.  A given
 *              rmin[m] is used verbatim as the radar minimum (the reference's map mode uses the held row)
 *              and ``rays`` is not written.
 *   neighbours by np.linalg.norm distance from the point: nearest = the minimum of (d, j); the collider
 *              whose bearing decides the crash doubling = the maximum of (d, j) among the colliders
 *              (d <= 2 pB, neither side reached); prev_two = a collider among prev2[m] (prev2 NULL: the
 *              live top2 of the subject, what the next step would read).
 *   me         the subject's live reach OR the goal touch at the point (the step's semantics).
 *   coefficients  the subject alone: crash 50 and near-drone 2, each doubled once if the row's own bearing
 *              says so.  The doubling a step carries over from the earlier aircraft of the same call is
 *              NOT applied; ``flags`` reports the row's own doublings.  Every doubling is an exact
 *              multiplication by 2, so the step's row of aircraft j is this row with the crash value of
 *              slot 0 scaled by 2^(crash doublings among aircraft 0..j-1) and slot 6 by 2^(near-drone
 *              doublings among aircraft 0..j-1), bit for bit (rewardmap.uam_step_rows does that).
 *
 * Read-only: the launch writes nothing but ``out`` -- no reach, top2, cloud, step counter, env_done, nor the
 * handle's reward and terms buffers.  The reference's sweep leaves drone 0 on the last grid point, uses its
 * sticky reach_target from the live position, keeps the held neighbour dict's order (which matters for exact
 * distance ties only) and the held radar row (here: rmin).
 */
#ifndef AAC_UAM_RMAP_H
#define AAC_UAM_RMAP_H

#include <stdint.h>

#include "aac_terms.h"
#include "aac_uam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_UAM_RMAP_OUT_BYTES 56    /* sizeof(aac_uam_rmap_out), for bindings in other languages */
#define AAC_UAM_RMAP_ROWS 14         /* rows per 256-thread workgroup: one work item per (row, ray) */

/* flags bits (the step kernel's per-aircraft flag byte) */
#define AAC_UAM_RMAP_BAND      1     /* the nearest neighbour is in the near-drone band [2, 5] */
#define AAC_UAM_RMAP_BAND_DBL  2     /* ... and its bearing in [90, 180] doubles the near-drone coefficient */
#define AAC_UAM_RMAP_CRASH_DBL 4     /* drone branch: the collider's bearing doubles the crash penalty */
#define AAC_UAM_RMAP_PREV_TWO  8     /* drone branch: a collider is one of the two previous nearest */

/* Caller-owned device outputs of M rows. */
typedef struct {
    double  *reward;  /* [M]     the subject's own reward */
    double  *terms;   /* [M][AAC_TERMS_W] rows as include/aac_terms.h (UAM slots 0, 3, 5, 6, 8-11), or NULL */
    uint8_t *mask;    /* [M]     the step's mask bits 0-5 (aac_uam.h) */
    uint8_t *done;    /* [M] */
    uint8_t *bbc;     /* [M][4]  bound_building_check as this aircraft alone would set it */
    uint8_t *flags;   /* [M]     AAC_UAM_RMAP_* bits */
    double  *rays;    /* [M][18] the radar row at the point, or NULL; not written when rmin is given */
} aac_uam_rmap_out;

/* points double[M][2]; pre double[M][2] or NULL; env_idx int32[M] or NULL (env 0); agent int32[M] or NULL
 * (aircraft 0); rmin double[M] or NULL; prev2 uint8[M][2] or NULL (255 = none): all device pointers, the
 * double arrays 8-byte aligned.  env_idx / agent values outside the handle's range are clamped into it.
 * One launch on ``stream``, no synchronisation, capturable; valid after aac_uam_step / reset / auto_reset
 * on the same stream.  M < 1, a NULL env / points / out->reward / mask / done / bbc / flags or a misaligned
 * double array returns AAC_E_INVALID (aac_uam_last_error()). */
int aac_uam_reward_map(aac_uam *env, const double *points, const double *pre, const int32_t *env_idx,
                       const int32_t *agent, const double *rmin, const uint8_t *prev2, int64_t M,
                       const aac_uam_rmap_out *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_UAM_RMAP_H */
