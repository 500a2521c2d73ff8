/* aac_probe.h -- radar probes of the ATT / WGRU environment (libaac_env.so): for every radar ray, what
 * it ended on and where.  The reference's env.step returns these beside the state (ATT/env:1051-1170,
 * :2720, :2815; OM/env:1049-1148): the probe segments and each ray's nearest intersection point, which
 * save_gif / view_static_traj draw.  The step, reset and band-fix launches keep one float32 distance per
 * ray; aac_env_probe re-runs the radar of given positions and keeps the record.
 *
 * One record per (row, agent, ray), R = 18 rays; with p the agent's position, end = p + radar_len (cos,
 * sin) and len = |end - p| as the radar forms them, the candidates of the ray are
 *   drone j != i   whose 64-gon the segment enters, at its distance d_j  (modes DRONES, COMBINED)
 *   occupied cells whose square the segment crosses at d <= len          (modes OBSTACLES, COMBINED)
 *   bound line k   (order of cfg.bound) crossed at d < len               (modes OBSTACLES, COMBINED)
 * and
 *   dist   the radar value D of the ray, in double: (float)dist is the step / reset / band-fix launches'
 *          ``radar`` output bit for bit (threshold-band cases are decided exactly here, as the band fix does)
 *   kind   AAC_PROBE_NONE / DRONE / CELL / BOUND
 *   id     drone: j; cell: ci * grid_h + cj in the row's map; bound: k; none: -1
 *   point  the hit point the taken candidate's distance was formed from (none: end); |point - p| == dist
 *   end    the ray end
 * Among the candidates whose distance equals D bit for bit the lowest (kind, id) is taken; if none
 * attains D (nothing hit, or COMBINED with a drone hit that rounds above len) the record is NONE.
 */
#ifndef AAC_PROBE_H
#define AAC_PROBE_H

#include <stdint.h>

#include "aac_env.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_PROBE_RAYS 18
#define AAC_PROBE_NONE 0
#define AAC_PROBE_DRONE 1
#define AAC_PROBE_CELL 2
#define AAC_PROBE_BOUND 3
#define AAC_PROBE_OUT_BYTES 40   /* sizeof(aac_probe_out), for bindings in other languages */

/* Caller-owned device outputs of M rows x N agents x 18 rays. */
typedef struct {
    double *dist;     /* [M][N][18]                  */
    double *point;    /* [M][N][18][2], 16-B aligned */
    double *end;      /* [M][N][18][2], 16-B aligned; or NULL */
    uint8_t *kind;    /* [M][N][18]                  */
    int32_t *id;      /* [M][N][18]                  */
} aac_probe_out;

/* pos_dev NULL: the handle's live positions and map_idx (M must be E) -- after aac_env_step / reset /
 * auto_reset on the same stream.  Otherwise M arbitrary rows double[M][N][2] with map_idx_dev int32[M]
 * (NULL: map 0; an index outside the handle's stack is clamped into it).  sel_dev uint8[M] (NULL: all):
 * rows with sel == 0 are skipped and their outputs left as they are.  One launch on ``stream``, no
 * synchronisation, capturable; it writes nothing but ``out`` and only reads the handle. */
int aac_env_probe(aac_env *env, const double *pos_dev, const int32_t *map_idx_dev, int64_t M,
                  const uint8_t *sel_dev, const aac_probe_out *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_PROBE_H */
