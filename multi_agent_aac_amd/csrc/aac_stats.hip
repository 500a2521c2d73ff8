// aac_stats.hip -- episode statistics on the device (include/aac_stats.h): the tallies of
// ATT/main:563-637 for E envs, one small launch per env step.
//
// stats_accum_kernel   one workgroup per 256 consecutive envs.  Its reward / done / mask rows are one
//                      contiguous block of the [E][N] arrays: all 1024 threads copy it to LDS with
//                      coalesced loads (16 agents per pass, 4 elements a thread), then thread e < 256
//                      walks the row of env e in LDS.  Finished episodes are reduced over a
//                      fixed LDS tree (thread order) and added to the workgroup's own slot, which no
//                      other workgroup touches: no floating-point atomics, no ordering between
//                      workgroups, so the slots do not depend on scheduling.
// stats_log_kernel     one workgroup: the finished envs' rows appended to the ring in env order, stamped
//                      with the step (aacs::log_finished).
// stats_reduce_kernel  one workgroup per 8-byte field: slots folded in a fixed order (aacs::slot_reduce).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "aac_env.h"
#include "aac_slots.h"
#include "aac_stats.h"

namespace {

thread_local std::string s_err;

int sfail(int code, const std::string &m) {
    s_err = m;
    return code;
}

constexpr int EPW = AAC_STATS_EPW, NC = 16, LD = NC + 1, NF = AAC_STATS_FIELDS;
constexpr int NT = 1024, PER = EPW * NC / NT;      // threads of a workgroup, elements each stages per pass
constexpr int F_UNDER = 11, F_SUM = 12, F_SQ = 13, F_MIN = 14, F_MAX = 15, F_HIST = 16;
static_assert(sizeof(aac_stats_totals) == NF * 8, "totals record = AAC_STATS_FIELDS 8-byte fields");
static_assert(offsetof(aac_stats_totals, under_quota) == F_UNDER * 8 && offsetof(aac_stats_totals, return_sum) == F_SUM * 8 &&
                  offsetof(aac_stats_totals, reach_hist) == F_HIST * 8,
              "field order");
static_assert(sizeof(aac_stats_row) == 32, "log row");
// counters of a slot, in record order
enum { C_EPISODES, C_STEPS, C_TIMEOUT, C_CRASH, C_GOAL, C_COLLISION, C_BOUND, C_BUILDING, C_DRONE, C_NEAREST, C_ALLSTEPS, C_N };

struct KArgs {
    aac_stats_state s;
    aac_stats_step p;
};

template <typename RT>
__global__ __launch_bounds__(NT) void stats_accum_kernel(KArgs A) {
    __shared__ double s_rew[EPW * LD];      // the reward rows of a pass; afterwards the reduction tree
    __shared__ uint8_t s_dn[EPW * LD], s_mk[EPW * LD];
    __shared__ int s_cnt[C_N], s_hist[AAC_STATS_MAX_AGENTS + 1];
    const aac_stats_step &P = A.p;
    const int t = threadIdx.x, g = blockIdx.x, N = P.N;
    const int e0 = g * EPW, ne = min(EPW, P.E - e0), e = e0 + t;
    const RT *__restrict__ reward = (const RT *)P.reward;
    if (t < C_N) s_cnt[t] = 0;
    if (t <= AAC_STATS_MAX_AGENTS) s_hist[t] = 0;
    // an env at its quota contributes nothing more
    const bool on = t < ne && (!P.quota || A.s.ep_count[e] < P.quota[e]);
    double ret = on ? A.s.run_return[e] : 0.0;
    uint64_t reach = 0;
    bool anyd = false;
    for (int c0 = 0; c0 < N; c0 += NC) {
        const int w = min(NC, N - c0), cnt = ne * w;
        // rows [e0, e0 + ne) x agents [c0, c0 + w): the whole contiguous block when N <= 16.  All of
        // a thread's loads are issued before the first LDS store (one memory round trip per pass)
        RT rv[PER] = {};
        uint8_t dv[PER] = {}, mv[PER] = {};
        int at[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int idx = t + k * NT;
            at[k] = -1;
            if (idx < cnt) {
                const int r = idx / w, c = idx - r * w;
                const size_t gi = (size_t)(e0 + r) * N + c0 + c;
                at[k] = r * LD + c;
                rv[k] = reward[gi];
                dv[k] = P.done[gi];
                mv[k] = P.mask[gi];
            }
        }
        if (c0) __syncthreads();      // the previous pass has been read
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (at[k] >= 0) {
                s_rew[at[k]] = (double)rv[k];
                s_dn[at[k]] = dv[k];
                s_mk[at[k]] = mv[k];
            }
        }
        __syncthreads();
        if (on) {
            for (int c = 0; c < w; ++c) {
                if (P.return_mode == 0 || c0 + c == 0) ret += s_rew[t * LD + c];
                anyd |= s_dn[t * LD + c] != 0;
                reach |= (uint64_t)((s_mk[t * LD + c] >> P.goal_bit) & 1) << (c0 + c);
            }
        }
    }
    bool fin = false;
    bool under = on;
    if (on) {
        const int len = A.s.run_len[e] + 1;
        reach |= A.s.run_reach[e];
        fin = P.env_done[e] != 0;
        if (fin) {
            const int k = __popcll(reach);
            const int reason = P.episode_length < len ? AAC_STATS_TIMEOUT : anyd ? AAC_STATS_CRASH : AAC_STATS_GOAL;
            int crash = 0;
            atomicAdd(&s_cnt[C_EPISODES], 1);
            atomicAdd(&s_cnt[C_STEPS], len);
            atomicAdd(&s_cnt[C_TIMEOUT + reason], 1);
            if (anyd && len < P.episode_length) {
                const uint8_t *b = P.bbc + 4 * (size_t)e;
                atomicAdd(&s_cnt[C_COLLISION], 1);
                crash = 5;
                if (b[0]) {
                    crash = 1;
                    atomicAdd(&s_cnt[C_BOUND], 1);
                } else if (b[1]) {
                    crash = 2;
                    atomicAdd(&s_cnt[C_BUILDING], 1);
                } else if (b[2]) {
                    crash = 3;
                    atomicAdd(&s_cnt[C_DRONE], 1);
                    if (b[3]) {
                        crash = 4;
                        atomicAdd(&s_cnt[C_NEAREST], 1);
                    }
                }
            } else {
                atomicAdd(&s_cnt[C_ALLSTEPS], 1);
            }
            atomicAdd(&s_hist[k], 1);
            const int done_eps = A.s.ep_count[e] + 1;
            A.s.ep_count[e] = done_eps;
            A.s.run_return[e] = 0.0;
            A.s.run_len[e] = 0;
            A.s.run_reach[e] = 0;
            under = !P.quota || done_eps < P.quota[e];
            if (A.s.log) {
                aac_stats_row row;
                row.ret = ret;
                row.step = 0;
                row.len = len;
                row.env = e;
                row.reason = reason;
                row.crash = (int16_t)crash;
                row.reach = (int16_t)k;
                A.s.fin_row[e] = row;
            }
        } else {
            A.s.run_return[e] = ret;
            A.s.run_len[e] = len;
            A.s.run_reach[e] = reach;
        }
    }
    if (A.s.log && t < ne) A.s.fin_flag[e] = fin ? 1 : 0;
    int64_t *slot = A.s.slots + (size_t)g * NF;
    const int n_under = __syncthreads_count(under);
    if (t == F_UNDER) slot[F_UNDER] = n_under;
    if (!__syncthreads_or(fin)) return;
    // the workgroup's finished episodes, folded in thread order over a fixed tree
    double *r_sum = s_rew, *r_sq = s_rew + EPW, *r_min = s_rew + 2 * EPW, *r_max = s_rew + 3 * EPW;
    if (t < EPW) {
        r_sum[t] = fin ? ret : 0.0;
        r_sq[t] = fin ? ret * ret : 0.0;
        r_min[t] = fin ? ret : INFINITY;
        r_max[t] = fin ? ret : -INFINITY;
    }
    aacs::fold_tree<EPW, 2>({r_sum, r_sq}, r_min, r_max, t);
    __syncthreads();
    double *slotd = (double *)slot;
    if (t < C_N) {
        slot[t] += s_cnt[t];
    } else if (t == F_SUM) {
        slotd[t] += r_sum[0];
    } else if (t == F_SQ) {
        slotd[t] += r_sq[0];
    } else if (t == F_MIN) {
        slotd[t] = fmin(slotd[t], r_min[0]);
    } else if (t == F_MAX) {
        slotd[t] = fmax(slotd[t], r_max[0]);
    } else if (t >= F_HIST && t < NF) {
        slot[t] += s_hist[t - F_HIST];
    }
}

__global__ __launch_bounds__(1024) void stats_log_kernel(aac_stats_state S, int E, int64_t step_index) {
    // one row per env, stamped with the caller's step index or the calls so far
    aacs::log_finished(S, E, 1,
                       [=](aac_stats_row &row, int64_t calls) { row.step = step_index < 0 ? calls : step_index; });
}

constexpr aacs::Kind field_kind(int f) {
    return f == F_UNDER ? aacs::INT_SUM_KEPT      // rewritten whole by every accumulate launch
           : f == F_SUM || f == F_SQ ? aacs::DBL_SUM
           : f == F_MIN ? aacs::DBL_MIN
           : f == F_MAX ? aacs::DBL_MAX
                        : aacs::INT_SUM;
}

__global__ __launch_bounds__(256) void stats_reduce_kernel(int64_t *slots, int G, int64_t *totals, int clear) {
    aacs::slot_reduce<NF, field_kind>(slots, G, totals, clear);
}

int check_state(const aac_stats_state *s, const char *what) {
    if (!s) return sfail(AAC_E_INVALID, std::string(what) + ": state");
    if (!s->run_return || !s->run_len || !s->run_reach || !s->ep_count || !s->slots)
        return sfail(AAC_E_INVALID, std::string(what) + ": running-state and slot buffers");
    return 0;
}

}  // namespace

extern "C" {

const char *aac_stats_last_error(void) { return s_err.c_str(); }

int aac_stats_accumulate(const aac_stats_state *s, const aac_stats_step *p, void *stream) {
    if (int rc = check_state(s, "stats_accumulate")) return rc;
    if (!p) return sfail(AAC_E_INVALID, "stats_accumulate: step");
    if (p->E <= 0) return sfail(AAC_E_INVALID, "stats_accumulate: E > 0");
    if (p->N < 1 || p->N > AAC_STATS_MAX_AGENTS) return sfail(AAC_E_INVALID, "stats_accumulate: 1 <= N <= 64");
    if (!p->reward || !p->done || !p->mask || !p->env_done || !p->bbc)
        return sfail(AAC_E_INVALID, "stats_accumulate: step inputs");
    if (p->goal_bit < 0 || p->goal_bit > 7) return sfail(AAC_E_INVALID, "stats_accumulate: 0 <= goal_bit <= 7");
    if (p->return_mode != 0 && p->return_mode != 1) return sfail(AAC_E_INVALID, "stats_accumulate: return_mode 0 / 1");
    if (p->episode_length < 1) return sfail(AAC_E_INVALID, "stats_accumulate: episode_length >= 1");
    if (s->log && (s->log_len < 1 || !s->log_meta || !s->fin_flag || !s->fin_row || !s->fin_list))
        return sfail(AAC_E_INVALID, "stats_accumulate: a log needs log_len >= 1, log_meta and the fin_* scratch");
    KArgs A;
    A.s = *s;
    A.p = *p;
    const int G = (p->E + EPW - 1) / EPW;
    hipStream_t st = (hipStream_t)stream;
    if (p->reward_f64)
        hipLaunchKernelGGL(stats_accum_kernel<double>, dim3(G), dim3(NT), 0, st, A);
    else
        hipLaunchKernelGGL(stats_accum_kernel<float>, dim3(G), dim3(NT), 0, st, A);
    if (s->log) hipLaunchKernelGGL(stats_log_kernel, dim3(1), dim3(1024), 0, st, *s, p->E, p->step_index);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : sfail(AAC_E_HIP, std::string("stats_accumulate: ") + hipGetErrorString(err));
}

int aac_stats_reduce(const aac_stats_state *s, int32_t E, aac_stats_totals *totals, int32_t clear, void *stream) {
    if (int rc = check_state(s, "stats_reduce")) return rc;
    if (E <= 0) return sfail(AAC_E_INVALID, "stats_reduce: E > 0");
    if (!totals) return sfail(AAC_E_INVALID, "stats_reduce: totals");
    const int G = (E + EPW - 1) / EPW;
    hipLaunchKernelGGL(stats_reduce_kernel, dim3(NF), dim3(256), 0, (hipStream_t)stream, s->slots, G, (int64_t *)totals,
                       clear ? 1 : 0);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : sfail(AAC_E_HIP, std::string("stats_reduce: ") + hipGetErrorString(err));
}

}  // extern "C"
