// aac_sortie.hip -- sortie statistics on the device (include/aac_sortie.h): the by-sortie outcome
// classes of UAM/main:1130-1144, the flight-distance ratio of UAM/util:53-68 and steps_before_collide,
// for E envs x N aircraft, one small launch per env step between the step and the reset.
//
// sortie_accum_kernel   one workgroup of 4 waves per 32 consecutive envs.  Lane = aircraft: a wave
//                       holds 64 / AP envs side by side, AP the power of two >= N, so the workgroup
//                       walks its envs in passes of 4 * 64 / AP and a lane keeps the same aircraft slot
//                       in every pass.  All loads of a pass are issued before their first use.  The
//                       per-env words (run_len, env_done, ep_count, quota) are read by every lane of the
//                       env and then written by its lane 0; "any done" of an env is a ballot masked to
//                       the env's lanes.  A thread adds its finished sorties in pass
//                       order; the threads are folded over a fixed LDS tree into the workgroup's own
//                       slot, which no other workgroup touches: no floating-point atomics.  collide_hist
//                       adds are gathered in an LDS histogram (up to 2048 bins; a longer one takes them
//                       in global memory) and flushed with one 64-bit integer add per non-zero bin: many
//                       envs end at the same length, and their adds would queue on one word in L2.
// sortie_log_kernel     one workgroup: the finished envs' N rows each appended to the ring in env order
//                       (aacs::log_finished).
// sortie_reduce_kernel  one workgroup per 8-byte field: slots folded in a fixed order (aacs::slot_reduce);
//                       with clear it also empties collide_hist.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "aac_env.h"
#include "aac_slots.h"
#include "aac_sortie.h"

namespace {

thread_local std::string s_err;

int sfail(int code, const std::string &m) {
    s_err = m;
    return code;
}

constexpr int EPW = AAC_SORTIE_EPW, NF = AAC_SORTIE_FIELDS, NT = 256, NW = NT / 64, HB = 2048;
// counters of a slot, in record order; then the doubles
enum { C_SORTIES, C_BOUND, C_OBSTACLE, C_DRONE, C_REACHED, C_IDLE, C_DEGENERATE, C_EPISODES, C_REACHSTEP, C_N };
constexpr int F_SUM = 9, F_SQ = 10, F_MIN = 11, F_MAX = 12, F_FLOWN = 13, F_STRAIGHT = 14;
static_assert(sizeof(aac_sortie_totals) == NF * 8, "totals record = AAC_SORTIE_FIELDS 8-byte fields");
static_assert(offsetof(aac_sortie_totals, reach_step_sum) == C_REACHSTEP * 8 && offsetof(aac_sortie_totals, ratio_sum) == F_SUM * 8 &&
                  offsetof(aac_sortie_totals, ratio_min) == F_MIN * 8 && offsetof(aac_sortie_totals, straight_sum) == F_STRAIGHT * 8,
              "field order");
static_assert(C_BOUND == 1 + AAC_SORTIE_BOUND && C_IDLE == 1 + AAC_SORTIE_IDLE, "class counters follow sorties in class order");
static_assert(sizeof(aac_sortie_state) == AAC_SORTIE_STATE_BYTES, "state struct");
static_assert(sizeof(aac_sortie_step) == AAC_SORTIE_STEP_BYTES, "step struct");
static_assert(sizeof(aac_sortie_row) == AAC_SORTIE_ROW_BYTES, "log row");
static_assert(EPW % NW == 0 && AAC_SORTIE_MAX_AGENTS == 64, "a wave holds whole envs");

struct KArgs {
    aac_sortie_state s;
    aac_sortie_step p;
};

__device__ __forceinline__ double norm2(double dx, double dy) { return sqrt(dx * dx + dy * dy); }

__global__ __launch_bounds__(NT) void sortie_accum_kernel(KArgs A, int AP) {
    __shared__ double s_d[6][NT];
    __shared__ int s_cnt[C_N];
    __shared__ int s_hist[HB];      // the workgroup's collide_hist adds (hist_len <= HB), one global add per bin
    const aac_sortie_state &S = A.s;
    const aac_sortie_step &P = A.p;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, N = P.N;
    const int i = lane & (AP - 1), sub = lane / AP, epv = 64 / AP;      // aircraft, env slot of the wave
    const int e0 = blockIdx.x * EPW, e1 = min(e0 + EPW, P.E);
    // the lanes of this lane's env: AP consecutive bits of the wave's ballot
    const unsigned long long grp = (AP == 64 ? ~0ull : ((1ull << AP) - 1)) << (lane & ~(AP - 1));
    if (t < C_N) s_cnt[t] = 0;
    const int hb = S.hist_len <= HB ? S.hist_len : 0;
    for (int j = t; j < hb; j += NT) s_hist[j] = 0;
    __syncthreads();
    double a_sum = 0.0, a_sq = 0.0, a_min = INFINITY, a_max = -INFINITY, a_flown = 0.0, a_straight = 0.0;
    bool anyfin = false;
    for (int eb = e0; eb < e1; eb += NW * epv) {
        const int e = eb + w * epv + sub;
        const bool valid = e < e1 && i < N;
        const size_t r = valid ? (size_t)e * N + i : 0;
        // every load of the pass is issued before the first use (one memory round trip): the values of
        // a continuing episode are read on its first step too, and dropped
        int epc = 0, quota = 1, rl = 0, rs = 0, epi = 0;
        uint8_t edn = 0, dnb = 0, mk = 0, fl0 = 0;
        double px = 0.0, py = 0.0, sx = 0.0, sy = 0.0, gx = 0.0, gy = 0.0, lx = 0.0, ly = 0.0;
        double straight = 0.0, first = 0.0, dist = 0.0;
        if (valid) {
            epc = S.ep_count[e];
            if (P.quota) quota = P.quota[e];
            if (P.episode) epi = P.episode[e];
            rl = S.run_len[e];
            edn = P.env_done[e];
            dnb = P.done[r];
            mk = P.mask[r];
            px = P.pos[2 * r], py = P.pos[2 * r + 1];
            sx = P.start[2 * r], sy = P.start[2 * r + 1];
            gx = P.goal[2 * r], gy = P.goal[2 * r + 1];
            lx = S.last_pos[2 * r], ly = S.last_pos[2 * r + 1];
            straight = S.straight[r];
            first = S.first_seg[r];
            dist = S.run_dist[r];
            fl0 = S.run_flags[r];
            rs = S.reach_step[r];
        }
        const bool env_on = e < e1 && (!P.quota || epc < quota);
        const bool on = env_on && i < N;
        bool dn = false, fin = false;
        int len = 0;
        if (on) {
            len = rl + 1;
            fin = edn != 0;
            dn = dnb != 0;
            const bool head = rl == 0;      // the first step of the episode
            const double seg = norm2(px - (head ? sx : lx), py - (head ? sy : ly));
            if (head) {
                straight = norm2(gx - sx, gy - sy);
                first = seg;
                dist = 0.0;
                S.straight[r] = straight;
                S.first_seg[r] = first;
            } else {
                dist = dist + seg;
            }
            S.run_dist[r] = dist;
            S.last_pos[2 * r] = px;
            S.last_pos[2 * r + 1] = py;
            const int flags = fl0 | mk;
            if (((mk >> P.goal_bit) & 1) && rs == 0) rs = len;
            if (!fin) {
                S.run_flags[r] = (uint8_t)flags;
                S.reach_step[r] = rs;
            } else {
                S.run_flags[r] = 0;
                S.reach_step[r] = 0;
                const int cls = (flags >> P.bound_bit) & 1      ? AAC_SORTIE_BOUND
                                : (flags >> P.obstacle_bit) & 1 ? AAC_SORTIE_OBSTACLE
                                : (flags >> P.drone_bit) & 1    ? AAC_SORTIE_DRONE
                                : (flags >> P.goal_bit) & 1     ? AAC_SORTIE_REACHED
                                                                : AAC_SORTIE_IDLE;
                const double flown = (dist + first) + P.reach_margin;
                double ratio = NAN;
                atomicAdd(&s_cnt[C_SORTIES], 1);
                atomicAdd(&s_cnt[1 + cls], 1);
                if (cls == AAC_SORTIE_REACHED) {
                    atomicAdd(&s_cnt[C_REACHSTEP], rs);
                    if (straight > 0.0 && isfinite(flown)) {
                        ratio = flown / straight;
                        a_sum += ratio;
                        a_sq += ratio * ratio;
                        a_min = fmin(a_min, ratio);
                        a_max = fmax(a_max, ratio);
                        a_flown += flown;
                        a_straight += straight;
                    } else {
                        atomicAdd(&s_cnt[C_DEGENERATE], 1);
                    }
                }
                if (S.log) {
                    aac_sortie_row *q = S.fin_row + r;
                    q->env = e;
                    q->agent = i;
                    q->episode = P.episode ? epi : epc;
                    q->cls = cls;
                    q->len = len;
                    q->reach_step = rs;
                    q->flown = flown;
                    q->straight = straight;
                    q->ratio = ratio;
                }
            }
        }
        const unsigned long long dmask = __ballot(dn);
        if (env_on && i == 0) {
            if (fin) {
                atomicAdd(&s_cnt[C_EPISODES], 1);
                if ((dmask & grp) && len < P.episode_length && len >= 0 && len < S.hist_len) {
                    if (hb) atomicAdd(&s_hist[len], 1);
                    else atomicAdd((unsigned long long *)S.collide_hist + len, 1ull);
                }
                S.ep_count[e] = epc + 1;
                S.run_len[e] = 0;
            } else {
                S.run_len[e] = len;
            }
        }
        if (S.log && e < e1 && i == 0) S.fin_flag[e] = fin ? 1 : 0;
        anyfin |= fin;
    }
    if (!__syncthreads_or(anyfin)) return;
    for (int j = t; j < hb; j += NT)
        if (s_hist[j]) atomicAdd((unsigned long long *)S.collide_hist + j, (unsigned long long)s_hist[j]);
    // the workgroup's finished sorties, folded in thread order over a fixed tree
    s_d[0][t] = a_sum;
    s_d[1][t] = a_sq;
    s_d[2][t] = a_min;
    s_d[3][t] = a_max;
    s_d[4][t] = a_flown;
    s_d[5][t] = a_straight;
    aacs::fold_tree<NT, 4>({s_d[0], s_d[1], s_d[4], s_d[5]}, s_d[2], s_d[3], t);
    __syncthreads();
    int64_t *slot = S.slots + (size_t)blockIdx.x * NF;
    double *slotd = (double *)slot;
    if (t < C_N) {
        slot[t] += s_cnt[t];
    } else if (t == F_MIN) {
        slotd[t] = fmin(slotd[t], s_d[2][0]);
    } else if (t == F_MAX) {
        slotd[t] = fmax(slotd[t], s_d[3][0]);
    } else if (t < NF) {
        slotd[t] += s_d[t == F_SUM ? 0 : t == F_SQ ? 1 : t == F_FLOWN ? 4 : 5][0];
    }
}

__global__ __launch_bounds__(1024) void sortie_log_kernel(aac_sortie_state S, int E, int N) {
    aacs::log_finished(S, E, N, [](aac_sortie_row &, int64_t) {});
}

constexpr aacs::Kind field_kind(int f) {
    return f < F_SUM ? aacs::INT_SUM : f == F_MIN ? aacs::DBL_MIN : f == F_MAX ? aacs::DBL_MAX : aacs::DBL_SUM;
}

__global__ __launch_bounds__(256) void sortie_reduce_kernel(int64_t *slots, int G, int64_t *totals, int clear,
                                                             int64_t *hist, int hist_len) {
    // the histogram is emptied beside the fold: no ordering between the two
    if (clear)
        for (int j = blockIdx.x * 256 + threadIdx.x; j < hist_len; j += NF * 256) hist[j] = 0;
    aacs::slot_reduce<NF, field_kind>(slots, G, totals, clear);
}

int check_state(const aac_sortie_state *s, const char *what) {
    if (!s) return sfail(AAC_E_INVALID, std::string(what) + ": state is null");
    if (!s->straight || !s->first_seg || !s->run_dist || !s->last_pos || !s->run_flags || !s->reach_step || !s->run_len ||
        !s->ep_count || !s->slots || !s->collide_hist)
        return sfail(AAC_E_INVALID, std::string(what) + ": running-state, slot and collide_hist buffers");
    if (s->hist_len < 1) return sfail(AAC_E_INVALID, std::string(what) + ": hist_len >= 1");
    return 0;
}

bool bit_ok(int b) { return b >= 0 && b <= 7; }

}  // namespace

extern "C" {

const char *aac_sortie_last_error(void) { return s_err.c_str(); }

int aac_sortie_accumulate(const aac_sortie_state *s, const aac_sortie_step *p, void *stream) {
    if (int rc = check_state(s, "sortie_accumulate")) return rc;
    if (!p) return sfail(AAC_E_INVALID, "sortie_accumulate: step is null");
    if (p->E <= 0) return sfail(AAC_E_INVALID, "sortie_accumulate: E > 0");
    if (p->N < 1 || p->N > AAC_SORTIE_MAX_AGENTS) return sfail(AAC_E_INVALID, "sortie_accumulate: 1 <= N <= 64");
    if ((int64_t)p->E * p->N >= (int64_t)1 << 31) return sfail(AAC_E_INVALID, "sortie_accumulate: E * N < 2^31");
    if (!p->pos || !p->start || !p->goal || !p->done || !p->mask || !p->env_done)
        return sfail(AAC_E_INVALID, "sortie_accumulate: step inputs (pos, start, goal, done, mask, env_done)");
    if (!bit_ok(p->bound_bit) || !bit_ok(p->obstacle_bit) || !bit_ok(p->drone_bit) || !bit_ok(p->goal_bit))
        return sfail(AAC_E_INVALID, "sortie_accumulate: 0 <= bound_bit, obstacle_bit, drone_bit, goal_bit <= 7");
    if (p->episode_length < 1) return sfail(AAC_E_INVALID, "sortie_accumulate: episode_length >= 1");
    if ((int64_t)s->hist_len < (int64_t)p->episode_length + 2)
        return sfail(AAC_E_INVALID, "sortie_accumulate: hist_len >= episode_length + 2");
    if (!std::isfinite(p->reach_margin)) return sfail(AAC_E_INVALID, "sortie_accumulate: reach_margin is finite");
    if (s->log && (s->log_len < 1 || !s->log_meta || !s->fin_flag || !s->fin_row || !s->fin_list))
        return sfail(AAC_E_INVALID, "sortie_accumulate: a log needs log_len >= 1, log_meta and the fin_* scratch");
    KArgs A;
    A.s = *s;
    A.p = *p;
    int AP = 1;
    while (AP < p->N) AP <<= 1;
    const int G = (p->E + EPW - 1) / EPW;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sortie_accum_kernel, dim3(G), dim3(NT), 0, st, A, AP);
    if (s->log) hipLaunchKernelGGL(sortie_log_kernel, dim3(1), dim3(1024), 0, st, *s, p->E, p->N);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : sfail(AAC_E_HIP, std::string("sortie_accumulate: ") + hipGetErrorString(err));
}

int aac_sortie_reduce(const aac_sortie_state *s, int32_t E, aac_sortie_totals *totals, int32_t clear, void *stream) {
    if (int rc = check_state(s, "sortie_reduce")) return rc;
    if (E <= 0) return sfail(AAC_E_INVALID, "sortie_reduce: E > 0");
    if (!totals) return sfail(AAC_E_INVALID, "sortie_reduce: totals is null");
    const int G = (E + EPW - 1) / EPW;
    hipLaunchKernelGGL(sortie_reduce_kernel, dim3(NF), dim3(256), 0, (hipStream_t)stream, s->slots, G, (int64_t *)totals,
                       clear ? 1 : 0, s->collide_hist, s->hist_len);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : sfail(AAC_E_HIP, std::string("sortie_reduce: ") + hipGetErrorString(err));
}

}  // extern "C"
