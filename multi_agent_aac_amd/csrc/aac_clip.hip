// aac_clip.hip -- gradient-norm clipping inside the learners' launch lists (include/aac_clip.h): the
// reference's clip_grad_norm_(net.parameters(), max_norm) ahead of every optimiser step
// (ATT/maddpg:187, :205-206), as two launches that stand where an Adam launch stood.
//
// clip_sumsq_kernel      one workgroup per AAC_CLIP_CHUNK elements of a segment (one or two jobs a launch).
//                        Thread t takes the 16-byte units t, t + 256, ... of the chunk (float: one): the copies summed
//                        in the element type by sum_unit (aac_copysum.h, where the Adam kernels' sums
//                        live too; one 16-byte load per copy where the segment's copies and grad_out
//                        are aligned, scalar loads otherwise -- the same
//                        elements to the same thread either way), the sum stored to grad_out, gscale * g
//                        squared and accumulated in double.  A butterfly folds each wave, thread 0 the
//                        four wave results in order: one partial per workgroup, one writer per partial.
// adam_clip_kernel       a grid-stride Adam over each segment.  Every workgroup folds the segment's P
//                        partials over the same tree (thread t: partials t, t + 256, ... in order, wave
//                        butterflies, the waves in order), so all of them hold the same coef; it is
//                        rounded to the element type once and multiplies the gradient in registers.
//                        Thread 0 of the segment's first workgroup keeps the unit's record.
// No atomics and no tickets; grids and element ranges are functions of n alone.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "aac_adam_bc.h"
#include "aac_clip.h"
#include "aac_copysum.h"
#include "aac_env.h"

namespace {

thread_local std::string s_err;

int cfail(int code, const std::string &m) {
    s_err = m;
    return code;
}

constexpr int NT = AAC_CLIP_THREADS, NW = NT / 64, CHUNK = AAC_CLIP_CHUNK, NR = AAC_CLIP_RECORD;
constexpr int ADAM_MAX_WG = AAC_CLIP_ADAM_MAX_WG;
static_assert(CHUNK % (NT * 4) == 0, "a chunk is whole trips of the workgroup, float and double");

struct ClipArgs {
    aac_clip_job j0, j1;
    int first;          // workgroups of job 0
    int per0, per1;     // workgroups per segment of each job
};

using aaccs::addr16;
using aaccs::wave_sum;
constexpr int DEPTH = 8;      // copy loads in flight per step of a unit's sum

template <typename T>
__global__ __launch_bounds__(NT) void clip_sumsq_kernel(ClipArgs A) {
    constexpr int V = 16 / (int)sizeof(T);
    typedef T VT __attribute__((ext_vector_type(V)));
    __shared__ double s_red[NW];
    const bool second = (int)blockIdx.x >= A.first;
    const int blk = second ? (int)blockIdx.x - A.first : (int)blockIdx.x, P = second ? A.per1 : A.per0;
    const int seg = blk / P, w = blk % P, t = threadIdx.x;
    const aac_clip_job &j = second ? A.j1 : A.j0;
    const int64_t n = j.n, gs = j.gstride, sstride = j.seg_stride;
    const int ns = j.nsplit, order = j.order;
    const T gscale = (T)j.gscale;
    const T *__restrict__ g = (const T *)j.g + seg * sstride;
    T *gout = (T *)j.grad_out;
    if (gout) gout += seg * sstride;
    double *partials = j.partials;
    // 16-byte accesses need every copy of the segment, and grad_out, on the 16-byte grid
    const bool wide = (ns == 1 || (gs * (int64_t)sizeof(T)) % 16 == 0) && addr16(g) == 0 && (!gout || addr16(gout) == 0);
    const int64_t c0 = (int64_t)w * CHUNK, c1 = c0 + CHUNK < n ? c0 + CHUNK : n;
    double ss = 0.0;
    for (int64_t i0 = c0 + (int64_t)t * V; i0 < c1; i0 += NT * V) {
        const int cnt = c1 - i0 < V ? (int)(c1 - i0) : V;
        const bool full = cnt == V;
        T x[V];
        aaccs::sum_unit<T, V, DEPTH>(g + i0, ns, gs, order, wide && full, cnt, x);
        if (gout) {
            if (wide && full) {
                VT q;
#pragma unroll
                for (int c = 0; c < V; ++c) q[c] = x[c];
                *reinterpret_cast<VT *>(gout + i0) = q;
            } else {
#pragma unroll
                for (int c = 0; c < V; ++c)
                    if (c < cnt) gout[i0 + c] = x[c];
            }
        }
#pragma unroll
        for (int c = 0; c < V; ++c) {
            if (c < cnt) {
                const double d = (double)(x[c] * gscale);
                ss += d * d;
            }
        }
    }
    ss = wave_sum(ss);
    if ((t & 63) == 0) s_red[t >> 6] = ss;
    __syncthreads();
    if (t == 0) {
        double a = s_red[0];
        for (int wv = 1; wv < NW; ++wv) a += s_red[wv];
        partials[(size_t)seg * P + w] = a;
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void adam_clip_kernel(ClipArgs A) {
    __shared__ T bc[2];
    __shared__ double s_red[NW];
    const bool second = (int)blockIdx.x >= A.first;
    const int blk = second ? (int)blockIdx.x - A.first : (int)blockIdx.x, G = second ? A.per1 : A.per0;
    const int seg = blk / G, b = blk % G, t = threadIdx.x;
    const aac_clip_job &j = second ? A.j1 : A.j0;
    const int64_t n = j.n, sstride = j.seg_stride;
    const T *__restrict__ g = (const T *)(j.grad_out ? j.grad_out : j.g) + seg * sstride;
    T *p = (T *)j.param + seg * sstride;
    T *m = (T *)j.exp_avg + seg * sstride;
    T *v = (T *)j.exp_avg_sq + seg * sstride;
    const T gscale = (T)j.gscale;
    const T lr = (T)j.lr, b1 = (T)j.beta1, b2 = (T)j.beta2, eps = (T)j.eps;
    const double max_norm = j.max_norm;
    const int tstep = *j.step + j.step_add;
    const int64_t P = (n + CHUNK - 1) / CHUNK;
    const double *__restrict__ part = j.partials + (size_t)seg * P;
    const int64_t stride = (int64_t)G * NT;
    int64_t i = (int64_t)b * NT + t;
    // the first trip's loads go out ahead of the fold and the bias corrections (clamped index,
    // unconditional: a thread past n still reaches the barrier in adam_bias_bcast)
    const int64_t ic = i < n ? i : n - 1;
    T g0 = g[ic], m0 = m[ic], v0 = v[ic], p0 = p[ic];
    double s = 0.0;
    for (int64_t k = t; k < P; k += NT) s += part[k];
    s = wave_sum(s);
    if ((t & 63) == 0) s_red[t >> 6] = s;
    T step_size, bc2s;
    adam_bias_bcast(bc, lr, b1, b2, tstep, step_size, bc2s);      // (its barrier also publishes s_red)
    double tot = s_red[0];
    for (int wv = 1; wv < NW; ++wv) tot += s_red[wv];
    // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1 (a NaN stays NaN)
    const double norm = sqrt(tot);
    const double c = max_norm / (norm + 1e-6);
    const double coefd = c >= 1.0 ? 1.0 : c;
    const T coef = (T)coefd;
    while (i < n) {
        const T gi = (g0 * gscale) * coef;
        adam_elem(p0, m0, v0, gi, b1, b2, eps, step_size, bc2s);
        p[i] = p0;
        m[i] = m0;
        v[i] = v0;
        i += stride;
        if (i >= n) break;
        g0 = g[i], m0 = m[i], v0 = v[i], p0 = p[i];
    }
    if (b == 0 && t == 0) {
        double *rec = j.record + (size_t)seg * NR;
        rec[AAC_CLIP_R_STEPS] += 1.0;
        if (coefd < 1.0) rec[AAC_CLIP_R_CLIPPED] += 1.0;
        if (!__builtin_isfinite(norm)) rec[AAC_CLIP_R_NONFINITE] += 1.0;
        rec[AAC_CLIP_R_LAST_NORM] = norm;
        rec[AAC_CLIP_R_LAST_COEF] = coefd;
        rec[AAC_CLIP_R_MAX_NORM_SEEN] = fmax(rec[AAC_CLIP_R_MAX_NORM_SEEN], norm);
    }
}

int check_job(const aac_clip_job &j, size_t esz, bool adam, const char *what) {
    const std::string w = what;
    if (!j.g || !j.partials) return cfail(AAC_E_INVALID, w + ": g and partials");
    if (j.n < 1 || j.nsplit < 1 || j.nseg < 1) return cfail(AAC_E_INVALID, w + ": n, nsplit, nseg >= 1");
    if (j.nsplit > 1 && j.gstride < j.n) return cfail(AAC_E_INVALID, w + ": copy stride < n");
    if (j.nseg > 1 && j.seg_stride < j.n) return cfail(AAC_E_INVALID, w + ": segment stride < n");
    if (j.order != 0 && j.order != 1) return cfail(AAC_E_INVALID, w + ": order 0 / 1");
    if ((uintptr_t)j.g % esz || (uintptr_t)j.grad_out % esz || (uintptr_t)j.partials % 8)
        return cfail(AAC_E_INVALID, w + ": pointers aligned to the element type");
    if ((j.n + CHUNK - 1) / CHUNK * j.nseg > (int64_t)1 << 30) return cfail(AAC_E_INVALID, w + ": too many partials");
    if (adam) {
        if (!j.param || !j.exp_avg || !j.exp_avg_sq || !j.step || !j.record)
            return cfail(AAC_E_INVALID, w + ": param, exp_avg, exp_avg_sq, step and record");
        if (!j.grad_out && j.nsplit != 1) return cfail(AAC_E_INVALID, w + ": nsplit > 1 needs grad_out (the summed gradient)");
        if ((uintptr_t)j.param % esz || (uintptr_t)j.exp_avg % esz || (uintptr_t)j.exp_avg_sq % esz ||
            (uintptr_t)j.step % 4 || (uintptr_t)j.record % 8)
            return cfail(AAC_E_INVALID, w + ": pointers aligned to the element type");
        if (j.max_norm != j.max_norm || j.max_norm < 0.0) return cfail(AAC_E_INVALID, w + ": max_norm >= 0");
    }
    return 0;
}

int adam_wgs(int64_t n) {
    const int64_t g = (n + NT - 1) / NT;
    return (int)(g < ADAM_MAX_WG ? g : ADAM_MAX_WG);
}

template <typename KF, typename KD>
int launch(const aac_clip_job *jobs, int32_t njobs, int32_t f64, void *stream, bool adam, const char *what, KF kf, KD kd) {
    if (!jobs || njobs < 1 || njobs > 2) return cfail(AAC_E_INVALID, std::string(what) + ": one or two jobs");
    for (int k = 0; k < njobs; ++k)
        if (int rc = check_job(jobs[k], f64 ? 8 : 4, adam, what)) return rc;
    ClipArgs A;
    A.j0 = jobs[0];
    A.j1 = jobs[njobs - 1];
    A.per0 = adam ? adam_wgs(A.j0.n) : (int)aac_clip_partials(A.j0.n);
    A.per1 = adam ? adam_wgs(A.j1.n) : (int)aac_clip_partials(A.j1.n);
    A.first = A.j0.nseg * A.per0;
    const int64_t grid = (int64_t)A.first + (njobs == 2 ? (int64_t)A.j1.nseg * A.per1 : 0);
    if (grid > (int64_t)1 << 30) return cfail(AAC_E_INVALID, std::string(what) + ": grid too large");
    hipStream_t st = (hipStream_t)stream;
    if (f64)
        hipLaunchKernelGGL(kd, dim3((unsigned)grid), dim3(NT), 0, st, A);
    else
        hipLaunchKernelGGL(kf, dim3((unsigned)grid), dim3(NT), 0, st, A);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : cfail(AAC_E_HIP, std::string(what) + ": " + hipGetErrorString(err));
}

}  // namespace

extern "C" {

const char *aac_clip_last_error(void) { return s_err.c_str(); }

int64_t aac_clip_partials(int64_t n) { return n < 1 ? 0 : (n + CHUNK - 1) / CHUNK; }

int aac_clip_sumsq(const aac_clip_job *jobs, int32_t njobs, int32_t f64, void *stream) {
    return launch(jobs, njobs, f64, stream, false, "clip_sumsq", clip_sumsq_kernel<float>, clip_sumsq_kernel<double>);
}

int aac_adam_flat_clip(const aac_clip_job *jobs, int32_t njobs, int32_t f64, void *stream) {
    return launch(jobs, njobs, f64, stream, true, "adam_flat_clip", adam_clip_kernel<float>, adam_clip_kernel<double>);
}

}  // extern "C"
