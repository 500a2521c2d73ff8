/* aac_uam_probe.h -- radar probes of the UAM environment (libaac_env.so): for every radar ray, what it ended
 * on and where.  The UAM reference's env.step returns these beside the state (UAM/env:1316-1320, :1346-1495,
 * :4809, :4904): the probe segments, and per ray the end point overwritten with the nearest intersection.
 * The step and reset launches keep one distance per ray; aac_uam_probe re-runs the 18-ray fp64 radar of given
 * positions and keeps the record.  aac_probe.h is the ATT / WGRU one.
 *
 * One record per (row m, aircraft i, ray r), R = 18 rays.  With p = pos[m][i], end = p + radar_len (cos, sin)
 * of the kernel's ray table and the default distance gdist(end, p), the candidates are the ones the step's
 * radar tests, formed by the same functions in the same expression order, each taken on a strict < against
 * the running minimum in this order (UAM/env:1385-1486):
 *
 *   kind                 id         candidate
 *   AAC_UAM_PROBE_NONE      0  -1        the ray's own length; point = end
 *   AAC_UAM_PROBE_RUNWAY    1  0         the runway rectangle's boundary (bounding-box gate, then the slab test)
 *   AAC_UAM_PROBE_BOUND     2  k = 0..3  x = bound[0], x = bound[1], y = bound[3], y = bound[2]
 *   AAC_UAM_PROBE_CLOUD     3  k = 0, 1  the 64-gon of cloud k, radius of the world table
 *   AAC_UAM_PROBE_AIRCRAFT  4  j != i    the 64-gon of radius pB of every other aircraft, finished ones included
 *
 * So the record is the first candidate, in table order and ascending id, that attains the minimum: the lowest
 * (kind, id) among bit-equal distances; a candidate bit-equal to the ray length leaves the record NONE.
 *
 *   dist   the radar value of the ray: at a step's own (pos, clouds) the step's ``radar`` output bit for bit
 *   point  the hit point the distance was formed from (none: end); |point - p| == dist bit for bit
 *   end    the ray end
 */
#ifndef AAC_UAM_PROBE_H
#define AAC_UAM_PROBE_H

#include <stdint.h>

#include "aac_uam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_UAM_PROBE_RAYS 18
#define AAC_UAM_PROBE_NONE 0
#define AAC_UAM_PROBE_RUNWAY 1
#define AAC_UAM_PROBE_BOUND 2
#define AAC_UAM_PROBE_CLOUD 3
#define AAC_UAM_PROBE_AIRCRAFT 4
#define AAC_UAM_PROBE_OUT_BYTES 40   /* sizeof(aac_uam_probe_out), for bindings in other languages */
#define AAC_UAM_PROBE_PAIRS 14       /* (row, aircraft) pairs per 256-thread workgroup: one work item per (pair, ray) */

/* Caller-owned device outputs of M rows x N aircraft x 18 rays. */
typedef struct {
    double *dist;     /* [M][N][18]                  */
    double *point;    /* [M][N][18][2], 16-B aligned */
    double *end;      /* [M][N][18][2], 16-B aligned; or NULL */
    uint8_t *kind;    /* [M][N][18]                  */
    int32_t *id;      /* [M][N][18]                  */
} aac_uam_probe_out;

/* All device pointers.  pos double[M][N][2], 16-B aligned; NULL: the handle's live positions (M must be E, row
 * m is env m).  clouds double[M][2][2], 16-B aligned; NULL: the live cloud centres of env env_idx[m].  env_idx
 * int32[M]; NULL: row m mod E (values outside the handle's range are clamped into it); not read when pos is
 * NULL.  sel uint8[M] (NULL: all): rows with sel == 0 are skipped and their outputs left as they are.
 * One launch on ``stream``, no synchronisation, capturable; valid after aac_uam_step / reset / auto_reset on
 * the same stream.  It writes nothing but ``out`` and only reads the handle; every record is written by exactly
 * one work item.  M < 1, a NULL env / out / dist / point / kind / id, a misaligned array or pos NULL with
 * M != E returns AAC_E_INVALID (aac_uam_last_error()). */
int aac_uam_probe(aac_uam *env, const double *pos, const double *clouds, const int32_t *env_idx, int64_t M,
                  const uint8_t *sel, const aac_uam_probe_out *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_UAM_PROBE_H */
