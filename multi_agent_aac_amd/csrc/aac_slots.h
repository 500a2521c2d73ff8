// aac_slots.h -- device code shared by the slot-based tallies (aac_stats.hip, aac_terms.hip,
// aac_sortie.hip): every accumulate workgroup folds its finished episodes over a fixed tree into a slot
// of its own (fold_tree), a single-workgroup launch appends the finished rows to the log ring
// (log_finished), and the reduce launch folds the slots, field by field, in a fixed order (slot_reduce).
// No floating-point atomics anywhere: for a fixed E and input sequence every total is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "aac_wave.h"

namespace aacs {

// what an 8-byte field of a slot record is, and how slots of it combine
enum Kind { INT_SUM, INT_SUM_KEPT /* not emptied by clear */, DBL_SUM, DBL_MIN, DBL_MAX };

__device__ __forceinline__ double identity(Kind k) { return k == DBL_MIN ? INFINITY : k == DBL_MAX ? -INFINITY : 0.0; }

__device__ __forceinline__ double combine(Kind k, double a, double b) {
    return k == DBL_MIN ? fmin(a, b) : k == DBL_MAX ? fmax(a, b) : a + b;
}

// The body of a reduce kernel: one workgroup of 256 threads per field f = blockIdx.x of the NF-field
// records.  Thread t takes slots t, t + 256, ... in ascending order, then entry t is folded with t + 128,
// 64, ... 1 in LDS; the total goes to totals[f].  clear: each slot is rewritten with its identity.
template <int NF, Kind (*KIND)(int)>
__device__ __forceinline__ void slot_reduce(int64_t *slots, int G, int64_t *totals, int clear) {
    __shared__ int64_t s_i[256];
    __shared__ double s_d[256];
    const int f = blockIdx.x, t = threadIdx.x;
    const Kind kind = KIND(f);
    const bool is_d = kind >= DBL_SUM;
    int64_t ai = 0;
    double ad = identity(kind);
    for (int g = t; g < G; g += 256) {
        int64_t *p = slots + (size_t)g * NF + f;
        if (is_d) {
            ad = combine(kind, ad, *(double *)p);
            if (clear) *(double *)p = identity(kind);
        } else {
            ai += *p;
            if (clear && kind != INT_SUM_KEPT) *p = 0;
        }
    }
    s_i[t] = ai;
    s_d[t] = ad;
    for (int s = 128; s > 0; s >>= 1) {
        __syncthreads();
        if (t < s) {
            s_i[t] += s_i[t + s];
            s_d[t] = combine(kind, s_d[t], s_d[t + s]);
        }
    }
    if (t == 0) {
        if (is_d)
            ((double *)totals)[f] = s_d[0];
        else
            totals[f] = s_i[0];
    }
}

// The body of a log kernel (one workgroup of 1024 threads) over a state struct with the fin_* scratch and
// the log ring: ordered list of the envs that finished (aacw::compact_flags), their rows_per_env rows each
// appended to the ring in that order, stamp(row, calls so far) applied to each; log_meta advances.
template <typename State, typename Stamp>
__device__ __forceinline__ void log_finished(const State &S, int E, int rows_per_env, Stamp stamp) {
    aacw::compact_flags(S.fin_flag, E, S.fin_list);
    __syncthreads();
    const int64_t n = (int64_t)S.fin_list[0] * rows_per_env, L = S.log_len;
    const int64_t pos = S.log_meta[0], calls = S.log_meta[1];
    // more rows than the ring holds: only the last L of them stay
    for (int64_t k = threadIdx.x; k < n; k += 1024) {
        if (k < n - L) continue;
        const int64_t j = k / rows_per_env, i = k - j * rows_per_env;
        auto row = S.fin_row[(size_t)S.fin_list[1 + j] * rows_per_env + i];
        stamp(row, calls);
        S.log[(pos + k) % L] = row;
    }
    __syncthreads();      // every thread has read log_meta
    if (threadIdx.x == 0) {
        S.log_meta[0] = pos + n;
        S.log_meta[1] = calls + 1;
    }
}

// The tree of an accumulate kernel: N entries (a power of two) of NSUM sums, a minimum and a maximum in
// LDS, entry j folded with j + N/2, ... 1; the roots are entry 0.  Every thread of the workgroup calls it
// (it holds barriers; a thread with j >= N/2 only waits), and the caller orders its own read of the roots.
template <int N, int NSUM>
__device__ __forceinline__ void fold_tree(double *const (&sum)[NSUM], double *mn, double *mx, int j) {
    for (int s = N / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (j < s) {
#pragma unroll
            for (int q = 0; q < NSUM; ++q) sum[q][j] += sum[q][j + s];
            mn[j] = fmin(mn[j], mn[j + s]);
            mx[j] = fmax(mx[j], mx[j + s]);
        }
    }
}

}  // namespace aacs
