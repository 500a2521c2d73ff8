/* aac_clip.h -- gradient-norm clipping inside the learners' launch lists (libaac_env.so, MI355X / gfx950).
 *
 * The reference clips every network's gradient before its optimiser step
 * (torch.nn.utils.clip_grad_norm_(net.parameters(), 1), ATT/maddpg:187, :205-206).  On the fused path the
 * gradient exists only as split-K partial copies and the update is one captured graph, so the norm and
 * the scaling live in two launches that replace an Adam launch:
 *
 *   aac_clip_sumsq       sums the copies as the Adam kernels do (csrc/aac_copysum.h holds the sum for
 *                        both; the sum goes to grad_out when asked), squares gscale * g in double and leaves one partial per workgroup;
 *   aac_adam_flat_clip   every workgroup folds its segment's partials over the same fixed tree (the same
 *                        bits everywhere), forms coef = min(1, max_norm / (sqrt(sum) + 1e-6)) in double,
 *                        rounds it to the element type once and runs the Adam step on (gscale * g) * coef.
 *
 * Semantics: clip_grad_norm_(norm_type=2, error_if_nonfinite=False) per segment ("unit").  coef lives in
 * registers: no gradient buffer is rewritten, so grad_out and the learner monitor show the pre-clip
 * gradient.  coef == 1 reproduces aac_adam_flat_at_scaled / aac_adam64_sum_scaled bit for bit.
 *
 * Determinism: no floating-point atomics.  Workgroup w of a segment takes elements
 * [w * AAC_CLIP_CHUNK, (w + 1) * AAC_CLIP_CHUNK) and P = aac_clip_partials(n) depends on n alone, never
 * on the device; every fold is a fixed tree.  16-byte loads are used where every copy of a segment (and
 * grad_out) is 16-byte aligned, scalar loads otherwise: the same sums in the same order.
 *
 * Conventions as aac_monitor.h: plain pointers, ``stream`` is a hipStream_t passed as void*, 0 or a
 * negative AAC_E* code is returned and aac_clip_last_error() holds the message.
 */
#ifndef AAC_CLIP_H
#define AAC_CLIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AAC_CLIP_THREADS 256       /* threads of a workgroup (both kernels) */
#define AAC_CLIP_CHUNK 1024        /* elements of one sumsq workgroup = of one partial */
#define AAC_CLIP_ADAM_MAX_WG 1024  /* aac_adam_flat_clip: workgroups per segment, min(ceil(n / 256), this) */
#define AAC_CLIP_RECORD 6          /* doubles per unit: the fields below */

#define AAC_CLIP_R_STEPS 0         /* clipped Adam steps taken */
#define AAC_CLIP_R_CLIPPED 1       /* steps with coef < 1 (total_norm == max_norm included, as in torch) */
#define AAC_CLIP_R_NONFINITE 2     /* steps whose norm was not finite */
#define AAC_CLIP_R_LAST_NORM 3     /* total_norm of the last step */
#define AAC_CLIP_R_LAST_COEF 4     /* its coef, in double (before the rounding to the element type) */
#define AAC_CLIP_R_MAX_NORM_SEEN 5 /* largest total_norm so far (NaN norms are not kept) */

/* One network as ``nseg`` segments ("units") of ``n`` elements (float, or double with f64), segment s at
 * offset s * seg_stride of g, grad_out, param, exp_avg and exp_avg_sq alike.
 *
 * aac_clip_sumsq reads g as ``nsplit`` copies ``gstride`` elements apart, summed in the element type:
 * order 0 the copies 0, 1, 2, ... in sequence, order 1 the four groups s % 4 each in sequence from zero
 * and then (g0 + g1) + (g2 + g3) (aac_monitor.h has the kernels each belongs to).  grad_out (optional)
 * receives that sum, unscaled.  partials[s * P + w] receives the sum of squares of gscale * g (the
 * product formed in the element type, squared in double) over workgroup w's elements.
 *
 * aac_adam_flat_clip reads the summed gradient (grad_out, or g itself when grad_out is NULL, which needs
 * nsplit == 1), the partials and max_norm, and takes Adam step ``*step + step_add`` with lr, beta1,
 * beta2, eps rounded to the element type.  record[s * AAC_CLIP_RECORD + field] is unit s's record,
 * updated by one lane of the segment's first workgroup. */
typedef struct {
    const void *g;
    void *grad_out;
    void *param, *exp_avg, *exp_avg_sq;
    const int32_t *step;
    double *partials;              /* [nseg][aac_clip_partials(n)] */
    double *record;                /* [nseg][AAC_CLIP_RECORD] */
    int64_t n, gstride, seg_stride;
    int32_t nsplit, nseg, order, step_add;
    double gscale, max_norm, lr, beta1, beta2, eps;
} aac_clip_job;

const char *aac_clip_last_error(void);
/* P: partials per segment of n elements. */
int64_t aac_clip_partials(int64_t n);
/* One launch over one or two jobs (njobs); f64: double elements. */
int aac_clip_sumsq(const aac_clip_job *jobs, int32_t njobs, int32_t f64, void *stream);
int aac_adam_flat_clip(const aac_clip_job *jobs, int32_t njobs, int32_t f64, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AAC_CLIP_H */
