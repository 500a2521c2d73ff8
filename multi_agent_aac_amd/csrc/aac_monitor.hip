// aac_monitor.hip -- the learner's records on the device (include/aac_monitor.h): losses, Q / target
// ranges and gradient / parameter norms of every update, from small launches inside the update's
// launch list.
//
// monitor_vec_kernel     AAC_MONITOR_VEC_WG workgroups per segment of a job (one or two jobs a launch).
//                        A segment is cut into 16-byte units after a scalar head that brings the
//                        gradient's address to a 16-byte boundary; workgroup w takes a contiguous run
//                        of units, thread t every 256th of them.  A unit is one 16-byte load per copy
//                        where the copies (and the parameters) are aligned alike, scalar loads
//                        otherwise and in the tail.  The copies are summed in the element type by
//                        sum_unit (aac_copysum.h, where the Adam kernels' sums live too), then
//                        everything accumulates in double per thread
//                        and folds over a fixed tree (wave butterflies, then the waves in order) into the workgroup's own slot.
// monitor_rows_kernel    one workgroup of 16 waves per column: thread t walks rows t, t + 1024, ... of the
//                        column's row fields, a fixed butterfly folds each wave and then the 16 wave
//                        results; two waves fold the column's vec partials.  The column's
//                        record goes to a staging row.
// monitor_fold_kernel    one workgroup: the staged record into the ring slot and the running aggregates,
//                        the sticky word and the counter.
// No atomics and no tickets: every partial has one writer and a fixed place, every fold a fixed tree.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "aac_copysum.h"
#include "aac_env.h"
#include "aac_monitor.h"

namespace {

thread_local std::string s_err;

int mfail(int code, const std::string &m) {
    s_err = m;
    return code;
}

constexpr int WG = AAC_MONITOR_VEC_WG, NV = AAC_MONITOR_VEC_VALUES, NETS = AAC_MONITOR_NETS, NF = AAC_MONITOR_FIELDS;
constexpr int NT = 256;                 // threads of a vec workgroup
constexpr int CT = 1024, CW = CT / 64;  // threads / waves of the commit workgroup
static_assert(WG >= 1 && WG <= 1024, "slots per segment");
static_assert(AAC_MONITOR_F_NET0 + NETS * NV == NF, "field order");
enum { F_LOSS_Q, F_LOSS_A, F_Q_MEAN, F_Q_MIN, F_Q_MAX, F_Y_MEAN, F_Y_MIN, F_Y_MAX, F_R_MEAN, F_R_MIN, F_R_MAX,
       F_TD_ABSMAX, F_PRE_MIN, F_PRE_MAX, F_ROWS_NONFINITE };
static_assert(F_ROWS_NONFINITE == AAC_MONITOR_F_ROWS_NONFINITE, "field order");

struct VecArgs {
    aac_monitor_vec_job j0, j1;
    int first;        // workgroups of job 0
};

// sumsq / absmax / non-finite count of a stream of values
struct Acc {
    double ss = 0.0, mx = 0.0;
    unsigned nf = 0;
    __device__ __forceinline__ void add(double d) {
        if (__builtin_isfinite(d)) {
            ss += d * d;
            mx = fmax(mx, fabs(d));
        } else {
            ++nf;
        }
    }
};

using aaccs::addr16;
using aaccs::load_unit;
using aaccs::wave_sum;
constexpr int DEPTH = 4;      // copy loads in flight per step of a unit's sum

template <typename T>
__global__ __launch_bounds__(NT) void monitor_vec_kernel(VecArgs A) {
    constexpr int V = 16 / (int)sizeof(T);
    __shared__ double s_red[NT / 64][NV];
    const bool second = (int)blockIdx.x >= A.first;
    const int blk = second ? (int)blockIdx.x - A.first : (int)blockIdx.x;
    const int seg = blk / WG, w = blk % WG, t = threadIdx.x;
    const aac_monitor_vec_job &j = second ? A.j1 : A.j0;
    const int64_t n = j.n, gs = j.gstride, sstride = j.seg_stride;
    const int ns = j.nsplit, order = j.order;
    const int col = j.col0 + seg, net = j.net;
    const T gscale = (T)j.gscale;
    double *scratch = j.scratch;
    const T *__restrict__ g = (const T *)j.g + seg * sstride, *__restrict__ p = (const T *)j.param + seg * sstride;
    // 16-byte loads of the gradient need every copy aligned alike; the head is counted from the
    // gradient then, else from the parameters
    const bool gcopies = ns == 1 || (gs * (int64_t)sizeof(T)) % 16 == 0;
    int64_t h = ((16u - addr16(gcopies ? (const void *)g : (const void *)p)) & 15u) / sizeof(T);
    if (h > n) h = n;
    const bool wide_g = gcopies && addr16(g + h) == 0, wide_p = addr16(p + h) == 0;
    Acc ag, ap;
    if (w == 0 && t < h) {      // the scalar head
        T x[V], y[V];
        aaccs::sum_unit<T, V, DEPTH>(g + t, ns, gs, order, false, 1, x);
        load_unit<T, V>(p + t, false, 1, y);
        ag.add((double)(x[0] * gscale));
        ap.add((double)y[0]);
    }
    const int64_t nun = (n - h + V - 1) / V, upw = (nun + WG - 1) / WG;
    const int64_t u1 = (w + 1) * upw < nun ? (w + 1) * upw : nun;
    for (int64_t u = w * upw + t; u < u1; u += NT) {
        const int64_t i0 = h + u * V;
        const int cnt = n - i0 < V ? (int)(n - i0) : V;
        const bool full = cnt == V;
        T x[V], y[V];
        aaccs::sum_unit<T, V, DEPTH>(g + i0, ns, gs, order, wide_g && full, cnt, x);
        load_unit<T, V>(p + i0, wide_p && full, cnt, y);
#pragma unroll
        for (int c = 0; c < V; ++c) {
            if (c < cnt) {
                ag.add((double)(x[c] * gscale));
                ap.add((double)y[c]);
            }
        }
    }
    // a fixed butterfly folds each wave, thread k < 6 then the four wave results in wave order
    double r[NV] = {ag.ss, ag.mx, (double)ag.nf, ap.ss, ap.mx, (double)ap.nf};
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(r[k], o, 64);
            r[k] = (k % 3 == 1) ? fmax(r[k], other) : r[k] + other;
        }
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) s_red[t >> 6][k] = r[k];
    }
    __syncthreads();
    if (t < NV) {
        double a = s_red[0][t];
        for (int wv = 1; wv < NT / 64; ++wv) a = (t % 3 == 1) ? fmax(a, s_red[wv][t]) : a + s_red[wv][t];
        scratch[(((size_t)col * NETS + net) * WG + w) * NV + t] = a;
    }
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// the 16 reduced quantities of a column's rows: sums, then maxima, then minima
enum { R_SE2, R_SQA, R_SQ, R_SY, R_SR, R_NOK, R_NBAD, R_TDM, R_QMX, R_YMX, R_RMX, R_PMX, R_QMN, R_YMN, R_RMN, R_PMN, R_N };
constexpr int R_MAX0 = R_TDM, R_MIN0 = R_QMN;

template <int K>
__device__ __forceinline__ double fold2(double a, double b) {
    return K < R_MAX0 ? a + b : (K < R_MIN0 ? fmax(a, b) : fmin(a, b));
}
template <int K>
__device__ __forceinline__ double identity() {
    return K < R_MAX0 ? 0.0 : (K < R_MIN0 ? -(double)INFINITY : (double)INFINITY);
}

// v[k] folded over the lanes lane ^ o, o = FROM, FROM / 2, ..., 1: a fixed butterfly
template <int FROM, int K = 0>
__device__ __forceinline__ void butterfly(double (&v)[R_N]) {
    if constexpr (K < R_N) {
#pragma unroll
        for (int o = FROM; o > 0; o >>= 1) v[K] = fold2<K>(v[K], __shfl_xor(v[K], o, 64));
        butterfly<FROM, K + 1>(v);
    }
}
template <int K = 0>
__device__ __forceinline__ void set_identity(double (&v)[R_N]) {
    if constexpr (K < R_N) {
        v[K] = identity<K>();
        set_identity<K + 1>(v);
    }
}

// One workgroup per column: thread t takes rows t, t + 1024, ...; a butterfly folds each wave, the 16
// wave results meet in LDS and the first 16 lanes of wave 0 fold them.  Waves 14 / 15 fold the column's
// vec partials of net 0 / 1 (lane l: slots l, l + 64, ...), their loads issued before the rows'.  The column's record
// goes to rec[c] for monitor_fold_kernel.
template <typename T>
__global__ __launch_bounds__(CT) void monitor_rows_kernel(aac_monitor_commit_args P, double *__restrict__ rec_out) {
    __shared__ double s_part[CW][R_N];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, c = blockIdx.x, B = P.B;
    double *rec = rec_out + (size_t)c * NF;
    const int net = wave - (CW - NETS);
    double pv[NV] = {};
    if (net >= 0) {
        // lane l takes slots l, l + 64, ... in order
        for (int sl = lane; sl < WG; sl += 64) {
            const double *x = P.scratch + (((size_t)c * NETS + net) * WG + sl) * NV;
#pragma unroll
            for (int k = 0; k < NV; ++k) pv[k] = (k % 3 == 1) ? fmax(pv[k], x[k]) : pv[k] + x[k];
        }
    }
    const T *q = (const T *)P.q.p + c * P.q.col_stride, *y = (const T *)P.y.p + c * P.y.col_stride;
    const T *qa = (const T *)P.q_a.p + c * P.q_a.col_stride, *rw = (const T *)P.reward.p + c * P.reward.col_stride;
    const T *qn = P.qn.p ? (const T *)P.qn.p + c * P.qn.col_stride : nullptr;
    const T *dn = P.qn.p ? (const T *)P.done.p + c * P.done.col_stride : nullptr;
    const float gf = (float)P.gamma;
    const int dw = P.done_width;
    double v[R_N];
    set_identity(v);
    float pmn = INFINITY, pmx = -INFINITY;
    for (int b = t; b < B; b += CT) {
        // every row is converted to double before any arithmetic
        const double qv = (double)q[b * P.q.row_stride], yv = (double)y[b * P.y.row_stride];
        const double av = (double)qa[b * P.q_a.row_stride], rv = (double)rw[b * P.reward.row_stride];
        float qnv = 0.0f;
        bool any = false;
        if (qn) {
            qnv = (float)qn[b * P.qn.row_stride];
            const T *d = dn + b * P.done.row_stride;
            for (int j0 = 0; j0 < dw; j0 += 8) {       // eight loads in flight (clamped index: repeats are harmless)
                T x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = d[j0 + u < dw ? j0 + u : dw - 1];
#pragma unroll
                for (int u = 0; u < 8; ++u) any |= x[u] == T(1);
            }
        }
        if (__builtin_isfinite(qv) && __builtin_isfinite(yv) && __builtin_isfinite(av)) {
            const double e = qv - yv;
            v[R_SE2] += e * e;
            v[R_SQA] += av;
            v[R_SQ] += qv;
            v[R_SY] += yv;
            v[R_SR] += rv;
            v[R_NOK] += 1.0;
            v[R_TDM] = fmax(v[R_TDM], fabs(e));
            v[R_QMN] = fmin(v[R_QMN], qv);
            v[R_QMX] = fmax(v[R_QMX], qv);
            v[R_YMN] = fmin(v[R_YMN], yv);
            v[R_YMX] = fmax(v[R_YMX], yv);
            v[R_RMN] = fmin(v[R_RMN], rv);
            v[R_RMX] = fmax(v[R_RMX], rv);
            if (qn) {
                // (gamma * Q') * (1 - any done) in float, the TD head's own operation order
                const float pre = (gf * qnv) * (1.0f - (any ? 1.0f : 0.0f));
                pmn = fminf(pmn, pre);
                pmx = fmaxf(pmx, pre);
            }
        } else {
            v[R_NBAD] += 1.0;
        }
    }
    v[R_TDM] = v[R_TDM] < 0.0 ? 0.0 : v[R_TDM];      // (the maximum of no rows is 0)
    v[R_PMN] = (double)pmn;
    v[R_PMX] = (double)pmx;
    butterfly<32>(v);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < R_N; ++k) s_part[wave][k] = v[k];
    }
    if (net >= 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) pv[k] = (k % 3 == 1) ? wave_max(pv[k]) : wave_sum(pv[k]);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < NV; ++k) rec[AAC_MONITOR_F_NET0 + net * NV + k] = pv[k];
        }
    }
    __syncthreads();
    if (wave != 0) return;
    set_identity(v);
    if (lane < CW) {
#pragma unroll
        for (int k = 0; k < R_N; ++k) v[k] = s_part[lane][k];
    }
    butterfly<CW / 2>(v);
    if (lane == 0) {
        const double nok = v[R_NOK];
        rec[F_LOSS_Q] = v[R_SE2] / nok;
        rec[F_LOSS_A] = P.a_off - v[R_SQA] / nok;
        rec[F_Q_MEAN] = v[R_SQ] / nok;
        rec[F_Q_MIN] = v[R_QMN];
        rec[F_Q_MAX] = v[R_QMX];
        rec[F_Y_MEAN] = v[R_SY] / nok;
        rec[F_Y_MIN] = v[R_YMN];
        rec[F_Y_MAX] = v[R_YMX];
        rec[F_R_MEAN] = v[R_SR] / nok;
        rec[F_R_MIN] = v[R_RMN];
        rec[F_R_MAX] = v[R_RMX];
        rec[F_TD_ABSMAX] = v[R_TDM];
        rec[F_PRE_MIN] = qn ? v[R_PMN] : (double)NAN;
        rec[F_PRE_MAX] = qn ? v[R_PMX] : (double)NAN;
        rec[F_ROWS_NONFINITE] = v[R_NBAD];
    }
}

// One workgroup: the record rec[A][NF] into the ring slot and the running aggregates, the sticky word
// and the counter.
__global__ __launch_bounds__(CT) void monitor_fold_kernel(aac_monitor_commit_args P, const double *__restrict__ rec) {
    const int t = threadIdx.x, A = P.A;
    const int64_t counter = P.state[0];
    const int slot = (int)(counter % P.R);
    const size_t st = (size_t)A * NF;
    bool bad = false;
    for (int i = t; i < A * NF; i += CT) {
        const int f = i % NF;
        const double v = rec[i];
        P.ring[(size_t)slot * st + i] = v;
        if (__builtin_isfinite(v)) {
            double *ag = P.agg + i;
            ag[0] += 1.0;
            ag[st] += v;
            ag[2 * st] += v * v;
            ag[3 * st] = fmin(ag[3 * st], v);
            ag[4 * st] = fmax(ag[4 * st], v);
        }
        const bool count_field = f == F_ROWS_NONFINITE || (f >= AAC_MONITOR_F_NET0 && (f - AAC_MONITOR_F_NET0) % 3 == 2);
        bad |= count_field && v != 0.0;
    }
    const int any_bad = __syncthreads_or(bad);       // (also: every thread has read the counter)
    if (t == 0) {
        P.ring_update[slot] = counter;
        if (any_bad && P.state[1] == -1) P.state[1] = counter;
        P.state[0] = counter + 1;
    }
}

int check_rows(const aac_monitor_rows &r, const char *name, bool optional) {
    if (!r.p && !optional) return mfail(AAC_E_INVALID, std::string("monitor_commit: ") + name + " rows");
    if (r.p && (r.col_stride < 0 || r.row_stride < 0))
        return mfail(AAC_E_INVALID, std::string("monitor_commit: ") + name + " strides >= 0");
    return 0;
}

}  // namespace

extern "C" {

const char *aac_monitor_last_error(void) { return s_err.c_str(); }

int aac_monitor_vec(const aac_monitor_vec_job *jobs, int32_t njobs, int32_t f64, void *stream) {
    if (!jobs || njobs < 1 || njobs > 2) return mfail(AAC_E_INVALID, "monitor_vec: one or two jobs");
    const size_t esz = f64 ? 8 : 4;
    for (int k = 0; k < njobs; ++k) {
        const aac_monitor_vec_job &j = jobs[k];
        if (!j.g || !j.param || !j.scratch) return mfail(AAC_E_INVALID, "monitor_vec: g, param and scratch");
        if (j.n < 1 || j.nsplit < 1 || j.nseg < 1) return mfail(AAC_E_INVALID, "monitor_vec: n, nsplit, nseg >= 1");
        if (j.nsplit > 1 && j.gstride < j.n) return mfail(AAC_E_INVALID, "monitor_vec: copy stride < n");
        if (j.nseg > 1 && j.seg_stride < j.n) return mfail(AAC_E_INVALID, "monitor_vec: segment stride < n");
        if (j.order != 0 && j.order != 1) return mfail(AAC_E_INVALID, "monitor_vec: order 0 / 1");
        if (j.net < 0 || j.net >= NETS) return mfail(AAC_E_INVALID, "monitor_vec: net 0 / 1");
        if (j.cols < 1 || j.cols > AAC_MONITOR_MAX_COLS || j.col0 < 0 || j.col0 + j.nseg > j.cols)
            return mfail(AAC_E_INVALID, "monitor_vec: 0 <= col0, col0 + nseg <= cols <= 64");
        if ((uintptr_t)j.g % esz || (uintptr_t)j.param % esz || (uintptr_t)j.scratch % 8)
            return mfail(AAC_E_INVALID, "monitor_vec: pointers aligned to the element type");
    }
    VecArgs A;
    A.j0 = jobs[0];
    A.j1 = jobs[njobs - 1];
    A.first = jobs[0].nseg * WG;
    const int grid = A.first + (njobs == 2 ? jobs[1].nseg * WG : 0);
    hipStream_t st = (hipStream_t)stream;
    if (f64)
        hipLaunchKernelGGL(monitor_vec_kernel<double>, dim3(grid), dim3(NT), 0, st, A);
    else
        hipLaunchKernelGGL(monitor_vec_kernel<float>, dim3(grid), dim3(NT), 0, st, A);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : mfail(AAC_E_HIP, std::string("monitor_vec: ") + hipGetErrorString(err));
}

int aac_monitor_commit(const aac_monitor_commit_args *a, void *stream) {
    if (!a) return mfail(AAC_E_INVALID, "monitor_commit: args");
    if (a->A < 1 || a->A > AAC_MONITOR_MAX_COLS) return mfail(AAC_E_INVALID, "monitor_commit: 1 <= A <= 64");
    if (a->B < 1 || a->R < 1) return mfail(AAC_E_INVALID, "monitor_commit: B, R >= 1");
    if (int rc = check_rows(a->q, "q", false)) return rc;
    if (int rc = check_rows(a->y, "y", false)) return rc;
    if (int rc = check_rows(a->q_a, "q_a", false)) return rc;
    if (int rc = check_rows(a->reward, "reward", false)) return rc;
    if (int rc = check_rows(a->qn, "qn", true)) return rc;
    if (a->qn.p) {
        if (int rc = check_rows(a->done, "done", false)) return rc;
        if (a->done_width < 1) return mfail(AAC_E_INVALID, "monitor_commit: done_width >= 1 with qn");
    }
    if (!a->scratch || !a->rec || !a->ring || !a->ring_update || !a->agg || !a->state)
        return mfail(AAC_E_INVALID, "monitor_commit: scratch, rec, ring, ring_update, agg and state");
    hipStream_t st = (hipStream_t)stream;
    if (a->f64)
        hipLaunchKernelGGL(monitor_rows_kernel<double>, dim3(a->A), dim3(CT), 0, st, *a, a->rec);
    else
        hipLaunchKernelGGL(monitor_rows_kernel<float>, dim3(a->A), dim3(CT), 0, st, *a, a->rec);
    hipLaunchKernelGGL(monitor_fold_kernel, dim3(1), dim3(CT), 0, st, *a, (const double *)a->rec);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : mfail(AAC_E_HIP, std::string("monitor_commit: ") + hipGetErrorString(err));
}

}  // extern "C"
