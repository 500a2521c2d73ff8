// aac_terms.hip -- the reward ledger (include/aac_terms.h): per-episode totals of the reward terms the
// env step kernels emit, one small launch per env step.
//
// terms_accum_kernel   one workgroup of 1024 threads per 256 consecutive envs (AAC_STATS_EPW, the slot
//                      granularity of aac_stats.hip).  Thread (env, slot k): 8 neighbouring lanes read the
//                      64 contiguous bytes of an agent's contribution slots and walk the env's agents in
//                      index order; 128 envs a pass, two passes.  The finished episodes' vectors go to
//                      LDS and are folded over a fixed tree (thread order) into the workgroup's own slot,
//                      which no other workgroup touches: no floating-point atomics, nothing depends on
//                      scheduling.
// terms_reduce_kernel  one workgroup per 8-byte field: slots folded in a fixed order (aacs::slot_reduce).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "aac_env.h"
#include "aac_slots.h"
#include "aac_stats.h"
#include "aac_terms.h"

namespace {

thread_local std::string s_err;

int tfail(int code, const std::string &m) {
    s_err = m;
    return code;
}

constexpr int EPW = AAC_STATS_EPW, NS = AAC_TERMS_SLOTS, TW = AAC_TERMS_W, NF = AAC_TERMS_FIELDS;
constexpr int NT = 1024, HALF = EPW / 2;
constexpr int F_SUM = 1, F_SQ = F_SUM + NS, F_MIN = F_SQ + NS, F_MAX = F_MIN + NS;
static_assert(NT == HALF * NS, "one thread per (slot, pair of envs) in the tree; per (env, slot) in a pass");
static_assert(sizeof(aac_terms_totals) == NF * 8 && F_MAX + NS == NF, "totals record = AAC_TERMS_FIELDS 8-byte fields");
static_assert(offsetof(aac_terms_totals, sum) == F_SUM * 8 && offsetof(aac_terms_totals, sqsum) == F_SQ * 8 &&
                  offsetof(aac_terms_totals, min) == F_MIN * 8 && offsetof(aac_terms_totals, max) == F_MAX * 8,
              "field order");

__global__ __launch_bounds__(NT) void terms_accum_kernel(aac_terms_state S, aac_terms_step P) {
    __shared__ double s_t[NS][EPW];      // the finished envs' episode vectors (0 for the others)
    __shared__ double r_sum[NS][HALF], r_sq[NS][HALF], r_min[NS][HALF], r_max[NS][HALF];
    __shared__ uint8_t s_fin[EPW];
    const int t = threadIdx.x, g = blockIdx.x, N = P.N;
    const int e0 = g * EPW;
    {
        const int k = t & (NS - 1);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int le = p * HALF + (t >> 3), e = e0 + le;
            // an env at its quota contributes nothing more
            const bool on = e < P.E && (!P.quota || S.ep_count[e] < P.quota[e]);
            const bool fin = on && P.env_done[e] != 0;
            double tk = 0.0;
            if (on) {
                const double *__restrict__ tr = P.terms + (size_t)e * N * TW + k;
                double *__restrict__ rn = S.run + (size_t)e * N * NS + k;
                for (int i = 0; i < N; ++i) {
                    const double v = rn[(size_t)i * NS] + tr[(size_t)i * TW];
                    tk += v;
                    rn[(size_t)i * NS] = fin ? 0.0 : v;
                }
            }
            s_t[k][le] = fin ? tk : 0.0;
            if (k == 0) s_fin[le] = fin ? 1 : 0;
        }
    }
    // (ep_count is read above by every thread of the env and advanced below, after this barrier)
    __syncthreads();      // s_t, s_fin written (the count below evaluates its predicate before its barrier)
    const int nfin = __syncthreads_count(t < EPW && s_fin[t]);
    if (!nfin) return;
    if (t < EPW && s_fin[t]) S.ep_count[e0 + t] += 1;
    // the workgroup's finished episodes, folded in thread order over a fixed tree
    const int k = t >> 7, j = t & (HALF - 1);
    {
        const double a = s_t[k][j], b = s_t[k][j + HALF];
        const bool fa = s_fin[j] != 0, fb = s_fin[j + HALF] != 0;
        r_sum[k][j] = a + b;
        r_sq[k][j] = a * a + b * b;
        r_min[k][j] = fmin(fa ? a : INFINITY, fb ? b : INFINITY);
        r_max[k][j] = fmax(fa ? a : -INFINITY, fb ? b : -INFINITY);
    }
    aacs::fold_tree<HALF, 2>({r_sum[k], r_sq[k]}, r_min[k], r_max[k], j);
    if (j == 0) {      // reads its own tree root
        int64_t *slot = S.slots + (size_t)g * NF;
        double *slotd = (double *)slot;
        if (k == 0) slot[0] += nfin;
        slotd[F_SUM + k] += r_sum[k][0];
        slotd[F_SQ + k] += r_sq[k][0];
        slotd[F_MIN + k] = fmin(slotd[F_MIN + k], r_min[k][0]);
        slotd[F_MAX + k] = fmax(slotd[F_MAX + k], r_max[k][0]);
    }
}

constexpr aacs::Kind field_kind(int f) {
    return f < F_SUM ? aacs::INT_SUM : f < F_MIN ? aacs::DBL_SUM : f < F_MAX ? aacs::DBL_MIN : aacs::DBL_MAX;
}

__global__ __launch_bounds__(256) void terms_reduce_kernel(int64_t *slots, int G, int64_t *totals, int clear) {
    aacs::slot_reduce<NF, field_kind>(slots, G, totals, clear);
}

// one workgroup per track: the env's N rows are contiguous, copied as 16-B pieces
__global__ __launch_bounds__(256) void terms_record_kernel(aac_terms_record_args A) {
    const int k = blockIdx.x;
    const int e = A.env_ids[k], c = A.cursor[k];
    const bool step = A.phase == 1;
    if (e < 0 || e >= A.E || A.ep_seen[k] >= A.max_episodes || c >= A.S) return;
    if (!step && A.sel && A.sel[e] == 0) return;
    const int n2 = A.N * TW / 2;
    double2 *dst = reinterpret_cast<double2 *>(A.rows + ((size_t)k * A.S + c) * A.N * TW);
    const double2 *src = reinterpret_cast<const double2 *>(A.terms + (size_t)e * A.N * TW);
    for (int q = threadIdx.x; q < n2; q += 256) dst[q] = step ? src[q] : make_double2(0.0, 0.0);
}

int check_state(const aac_terms_state *s, const char *what) {
    if (!s) return tfail(AAC_E_INVALID, std::string(what) + ": state");
    if (!s->run || !s->ep_count || !s->slots) return tfail(AAC_E_INVALID, std::string(what) + ": running-state and slot buffers");
    return 0;
}

}  // namespace

extern "C" {

const char *aac_terms_last_error(void) { return s_err.c_str(); }

const char *aac_terms_names(void) { return AAC_TERMS_NAMES; }

int aac_terms_accumulate(const aac_terms_state *s, const aac_terms_step *p, void *stream) {
    if (int rc = check_state(s, "terms_accumulate")) return rc;
    if (!p) return tfail(AAC_E_INVALID, "terms_accumulate: step");
    if (p->E <= 0) return tfail(AAC_E_INVALID, "terms_accumulate: E > 0");
    if (p->N < 1 || p->N > 256) return tfail(AAC_E_INVALID, "terms_accumulate: 1 <= N <= 256");
    if (!p->terms || !p->env_done) return tfail(AAC_E_INVALID, "terms_accumulate: step inputs");
    const int G = (p->E + EPW - 1) / EPW;
    hipLaunchKernelGGL(terms_accum_kernel, dim3(G), dim3(NT), 0, (hipStream_t)stream, *s, *p);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : tfail(AAC_E_HIP, std::string("terms_accumulate: ") + hipGetErrorString(err));
}

int aac_terms_reduce(const aac_terms_state *s, int32_t E, aac_terms_totals *totals, int32_t clear, void *stream) {
    if (int rc = check_state(s, "terms_reduce")) return rc;
    if (E <= 0) return tfail(AAC_E_INVALID, "terms_reduce: E > 0");
    if (!totals) return tfail(AAC_E_INVALID, "terms_reduce: totals");
    const int G = (E + EPW - 1) / EPW;
    hipLaunchKernelGGL(terms_reduce_kernel, dim3(NF), dim3(256), 0, (hipStream_t)stream, s->slots, G, (int64_t *)totals,
                       clear ? 1 : 0);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : tfail(AAC_E_HIP, std::string("terms_reduce: ") + hipGetErrorString(err));
}

int aac_terms_record(const aac_terms_record_args *a, void *stream) {
    if (!a) return tfail(AAC_E_INVALID, "terms_record: args");
    if (a->T < 1 || a->S < 1 || a->N < 1 || a->E < 1 || a->max_episodes < 1)
        return tfail(AAC_E_INVALID, "terms_record: T, S, N, E, max_episodes >= 1");
    if (a->phase != 0 && a->phase != 1) return tfail(AAC_E_INVALID, "terms_record: phase 0 (reset) / 1 (step)");
    if (!a->env_ids || !a->cursor || !a->ep_seen || !a->rows) return tfail(AAC_E_INVALID, "terms_record: buffers");
    if (a->phase == 1 && !a->terms) return tfail(AAC_E_INVALID, "terms_record: a step needs the terms buffer");
    if ((reinterpret_cast<uintptr_t>(a->rows) | reinterpret_cast<uintptr_t>(a->terms)) & 15)
        return tfail(AAC_E_INVALID, "terms_record: 16-byte aligned buffers");
    hipLaunchKernelGGL(terms_record_kernel, dim3(a->T), dim3(256), 0, (hipStream_t)stream, *a);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : tfail(AAC_E_HIP, std::string("terms_record: ") + hipGetErrorString(err));
}

}  // extern "C"
