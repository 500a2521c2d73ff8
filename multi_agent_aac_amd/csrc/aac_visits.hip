// aac_visits.hip -- exploration maps on the device (include/aac_visits.h): the position heat map of
// display_exploration_expolitation (ATT/util:776-866) and the action table of
// action_selection_statistics (ATT/util:869-897) for E x N rows, one small launch per env step.
//
// visits_kernel   workgroup g owns rows [g * CHUNK, (g + 1) * CHUNK) of the E * N rows: 256 threads, four
//                 rows a thread at a stride of 256 (coalesced 16-byte position loads), every load of a
//                 thread issued before the first bin is worked out.
//                 The action table has few bins and heavy collisions (a saturated actor puts every row
//                 into one corner): it is a private uint32 [2][A][A] LDS histogram of the workgroup,
//                 flushed with one 64-bit agent-scope relaxed global add per non-zero bin.
//                 The position table: where planes x GX x GY is at most POS_BINS (the default 50 x 50 grid
//                 on one or two maps) it is a private uint32 LDS histogram of the workgroup too, flushed
//                 the same way -- a fleet crowds into few bins (config 5: 333 of 5000), and 131 072 rows
//                 adding straight to those few global words took 72 us against 9 us for the episode
//                 statistics' launch.  A larger table is sparse per workgroup and its
//                 adds go straight to global 64-bit atomics (POS_LDS = false).
//                 The counters: per wave, the lanes of one plane are found by ballot and counted by
//                 popcount; the plane's first lane adds the three counts to an LDS table (the first
//                 CNT_PLANES planes; later planes, which no trainer here has, take the wave's counts
//                 straight to global), flushed once per workgroup and plane.
//                 Integer adds only: the tables do not depend on scheduling.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <type_traits>

#include "aac_env.h"
#include "aac_visits.h"

namespace {

thread_local std::string s_err;

int vfail(int code, const std::string &m) {
    s_err = m;
    return code;
}

constexpr int CHUNK = AAC_VISITS_CHUNK, NT = 256, PER = CHUNK / NT, MAX_A = AAC_VISITS_MAX_A, NC = AAC_VISITS_COUNTERS;
constexpr int CNT_PLANES = 128;     // planes whose counters are reduced in LDS
constexpr int POS_BINS = 10240;     // position bins (all planes) a workgroup can keep in LDS: 40 KB
enum { C_SAMPLES, C_POS_OUT, C_ACT_OUT, C_RESERVED };
static_assert(sizeof(aac_visits_state) == AAC_VISITS_STATE_BYTES, "aac_visits_state");
static_assert(sizeof(aac_visits_step) == AAC_VISITS_STEP_BYTES, "aac_visits_step");
static_assert(CHUNK % NT == 0 && NT % 64 == 0, "whole waves, whole passes");

struct KArgs {
    aac_visits_state s;
    aac_visits_step p;
    double wx, wy, wa;      // bin widths (hi - lo) / G
    int64_t rows;           // E * N
};

__device__ __forceinline__ void gadd(int64_t *p, int64_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The bin of v, which the caller has found inside [lo, hi]: then (v - lo) / w lies in [0, G] up to
// rounding, so the conversion is defined.  The guess is corrected against the edges lo + k * w on
// both sides (edge[G] = hi is never needed: the last bin is closed).
__device__ __forceinline__ int bin_of(double v, double lo, double w, int G) {
    int k = min((int)((v - lo) / w), G - 1);
    while (k > 0 && v < lo + k * w) --k;
    while (k < G - 1 && v >= lo + (k + 1) * w) ++k;
    return k;
}

__device__ __forceinline__ void cadd(uint32_t *s_cnt, int64_t *counters, int plane, int c, int n) {
    if (plane < CNT_PLANES)
        atomicAdd(&s_cnt[plane * NC + c], (uint32_t)n);
    else
        gadd(counters + (size_t)plane * NC + c, n);
}

template <typename AT, bool POS_LDS>
__global__ __launch_bounds__(NT) void visits_kernel(KArgs K) {
    __shared__ uint32_t s_act[2 * MAX_A * MAX_A];
    __shared__ uint32_t s_cnt[CNT_PLANES * NC];
    __shared__ uint32_t s_pos[POS_LDS ? POS_BINS : 1];
    const aac_visits_state &S = K.s;
    const aac_visits_step &P = K.p;
    const int t = threadIdx.x, lane = t & 63, A = S.A, N = P.N;
    const int n_act = 2 * A * A, n_cnt = min(2 * S.n_maps, CNT_PLANES) * NC;
    for (int b = t; b < n_act; b += NT) s_act[b] = 0;
    for (int b = t; b < n_cnt; b += NT) s_cnt[b] = 0;
    const int n_pos = POS_LDS ? 2 * S.n_maps * S.GX * S.GY : 0;      // <= POS_BINS (the host chose the form)
    for (int b = t; b < n_pos; b += NT) s_pos[b] = 0;
    const int64_t r0 = (int64_t)blockIdx.x * CHUNK;
    using AT2 = typename std::conditional<sizeof(AT) == 8, double2, float2>::type;
    const double2 *__restrict__ pos = (const double2 *)P.pos;
    const AT2 *__restrict__ act = (const AT2 *)P.act;
    // every load of the thread's rows first: one memory round trip
    double2 pv[PER];
    AT2 av[PER];
    int ep[PER], mp[PER];
    bool on[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int64_t r = r0 + t + k * NT;
        on[k] = r < K.rows;
        pv[k] = double2{0.0, 0.0};
        av[k] = AT2{0, 0};
        ep[k] = mp[k] = 0;
        if (on[k]) {
            const int e = (int)(r / N);
            on[k] = !P.sel || P.sel[e] != 0;
            if (on[k]) {
                pv[k] = pos[r];
                av[k] = act[r];
                ep[k] = P.episode[e];
                if (P.map_idx) mp[k] = P.map_idx[e];
            }
        }
    }
    __syncthreads();      // the LDS tables are zero
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const bool bad = on[k] && (mp[k] < 0 || mp[k] >= S.n_maps);
        const bool ok = on[k] && !bad;
        const int period = ep[k] <= P.explore_until ? 0 : 1;
        const int plane = ok ? 2 * mp[k] + period : 0;
        const double x = pv[k].x, y = pv[k].y, u = (double)av[k].x, v = (double)av[k].y;
        // the range tests (false for NaN) come before any conversion to an index
        const bool pin = ok && x >= S.x0 && x <= S.x1 && y >= S.y0 && y <= S.y1;
        const bool ain = ok && u >= S.a0 && u <= S.a1 && v >= S.a0 && v <= S.a1;
        if (pin) {
            const int bx = bin_of(x, S.x0, K.wx, S.GX), by = bin_of(y, S.y0, K.wy, S.GY);
            if (POS_LDS)
                atomicAdd(&s_pos[(plane * S.GX + bx) * S.GY + by], 1u);
            else
                gadd(S.pos_hist + ((size_t)plane * S.GX + bx) * S.GY + by, 1);
        }
        if (ain) {
            const int bu = bin_of(u, S.a0, K.wa, A), bv = bin_of(v, S.a0, K.wa, A);
            atomicAdd(&s_act[(period * A + bu) * A + bv], 1u);
        }
        // the wave's rows, plane by plane: ballot and popcount, one lane adds
        unsigned long long todo = __ballot(ok);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int pl = __shfl(plane, leader, 64);
            const bool mine = ok && plane == pl;
            const unsigned long long same = __ballot(mine);
            const int n_pos = __popcll(__ballot(mine && !pin)), n_act_out = __popcll(__ballot(mine && !ain));
            if (lane == leader) {
                cadd(s_cnt, S.counters, pl, C_SAMPLES, __popcll(same));
                if (n_pos) cadd(s_cnt, S.counters, pl, C_POS_OUT, n_pos);
                if (n_act_out) cadd(s_cnt, S.counters, pl, C_ACT_OUT, n_act_out);
            }
            todo &= ~same;
        }
        const unsigned long long nb = __ballot(bad);
        if (nb && lane == 0) cadd(s_cnt, S.counters, 0, C_RESERVED, __popcll(nb));
    }
    __syncthreads();
    for (int b = t; b < n_act; b += NT) {
        const uint32_t c = s_act[b];
        if (c) gadd(S.act_hist + b, c);
    }
    for (int b = t; b < n_cnt; b += NT) {
        const uint32_t c = s_cnt[b];
        if (c) gadd(S.counters + b, c);
    }
    for (int b = t; b < n_pos; b += NT) {
        const uint32_t c = s_pos[b];
        if (c) gadd(S.pos_hist + b, c);
    }
}

// a range [lo, hi] split into G bins of a width the kernel can divide by
bool range_ok(double lo, double hi, int G, double *w) {
    if (!(lo < hi) || !std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(hi - lo)) return false;
    *w = (hi - lo) / G;
    return *w > 0.0;
}

}  // namespace

extern "C" {

const char *aac_visits_last_error(void) { return s_err.c_str(); }

int aac_visits_accumulate(const aac_visits_state *s, const aac_visits_step *p, void *stream) {
    if (!s) return vfail(AAC_E_INVALID, "visits_accumulate: state");
    if (!p) return vfail(AAC_E_INVALID, "visits_accumulate: step");
    if (!s->pos_hist || !s->act_hist || !s->counters)
        return vfail(AAC_E_INVALID, "visits_accumulate: pos_hist, act_hist and counters tables");
    if (s->GX < 1 || s->GY < 1 || s->GX > AAC_VISITS_MAX_G || s->GY > AAC_VISITS_MAX_G)
        return vfail(AAC_E_INVALID, "visits_accumulate: 1 <= GX, GY <= 65536");
    if (s->A < 1 || s->A > AAC_VISITS_MAX_A) return vfail(AAC_E_INVALID, "visits_accumulate: 1 <= A <= 32");
    if (s->n_maps < 1 || s->n_maps > INT32_MAX / 2) return vfail(AAC_E_INVALID, "visits_accumulate: n_maps >= 1");
    KArgs K;
    if (!range_ok(s->x0, s->x1, s->GX, &K.wx)) return vfail(AAC_E_INVALID, "visits_accumulate: finite x0 < x1");
    if (!range_ok(s->y0, s->y1, s->GY, &K.wy)) return vfail(AAC_E_INVALID, "visits_accumulate: finite y0 < y1");
    if (!range_ok(s->a0, s->a1, s->A, &K.wa)) return vfail(AAC_E_INVALID, "visits_accumulate: finite a0 < a1");
    if (p->E < 1 || p->N < 1) return vfail(AAC_E_INVALID, "visits_accumulate: E, N >= 1");
    K.rows = (int64_t)p->E * p->N;
    if (K.rows > INT32_MAX) return vfail(AAC_E_INVALID, "visits_accumulate: E * N < 2^31");
    if (!p->pos || !p->act || !p->episode) return vfail(AAC_E_INVALID, "visits_accumulate: pos, act and episode");
    if ((reinterpret_cast<uintptr_t>(p->pos) & 15) || (reinterpret_cast<uintptr_t>(p->act) & (p->act_f64 ? 15 : 7)))
        return vfail(AAC_E_INVALID, "visits_accumulate: pos (and a double act) 16-byte, a float act 8-byte aligned");
    K.s = *s;
    K.p = *p;
    const int G = (int)((K.rows + CHUNK - 1) / CHUNK);
    hipStream_t st = (hipStream_t)stream;
    const bool pos_lds = 2 * (int64_t)s->n_maps * s->GX * s->GY <= POS_BINS;
    if (p->act_f64) {
        if (pos_lds)
            hipLaunchKernelGGL((visits_kernel<double, true>), dim3(G), dim3(NT), 0, st, K);
        else
            hipLaunchKernelGGL((visits_kernel<double, false>), dim3(G), dim3(NT), 0, st, K);
    } else {
        if (pos_lds)
            hipLaunchKernelGGL((visits_kernel<float, true>), dim3(G), dim3(NT), 0, st, K);
        else
            hipLaunchKernelGGL((visits_kernel<float, false>), dim3(G), dim3(NT), 0, st, K);
    }
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : vfail(AAC_E_HIP, std::string("visits_accumulate: ") + hipGetErrorString(err));
}

}  // extern "C"
