// aac_record.hip -- flight recorder (include/aac_record.h): the rows and episode summaries of T
// tracked envs, one small launch after each env step / reset.
//
// record_kernel   one wave per track, lane = agent (N <= 64), four tracks per 256-thread workgroup.
//                 The track's positions (and, for a step, its rewards widened to double) are staged
//                 once in LDS; lane i takes the minimum of d2(i, j) over j in index order, the wave
//                 folds the per-lane roots with a cross-lane double min.  Every field's N elements
//                 go out as one contiguous store of the wave; lane 0 keeps the track's running state
//                 and writes the header and the summary.  A track belongs to one wave, so nothing is
//                 shared between waves but the staging barrier: no atomics, no ordering.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "aac_env.h"
#include "aac_record.h"

namespace {

thread_local std::string s_err;

int rfail(int code, const std::string &m) {
    s_err = m;
    return code;
}

constexpr int MAXA = AAC_RECORD_MAX_AGENTS, TPW = 4;      // tracks per workgroup (one wave each)
static_assert(MAXA == 64, "lane = agent");
static_assert(sizeof(aac_record_episode) == AAC_RECORD_EPISODE_BYTES, "summary record");
static_assert(sizeof(aac_record_state) == AAC_RECORD_STATE_BYTES, "aac_record_state");
static_assert(sizeof(aac_record_step) == AAC_RECORD_STEP_BYTES, "aac_record_step");

struct KArgs {
    aac_record_state s;
    aac_record_step p;
};

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(TPW * 64) void record_kernel(KArgs A) {
    __shared__ double2 s_pos[TPW][MAXA];
    __shared__ double s_rew[TPW][MAXA];
    const aac_record_state &S = A.s;
    const aac_record_step &P = A.p;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, k = blockIdx.x * TPW + w, N = S.N;
    const bool step = P.phase == AAC_RECORD_STEP;
    int e = 0, seen = 0;
    bool on = false;
    if (k < S.T) {
        e = S.env_ids[k];
        seen = S.ep_seen[k];
        // a finished track, an env the reset did not touch, or an env id outside the sources: left alone
        on = e >= 0 && e < P.E && seen < P.max_episodes && (step || !P.sel || P.sel[e] != 0);
    }
    const bool mine = on && lane < N;
    const size_t src = (size_t)e * N + lane;
    double2 p = make_double2(0.0, 0.0);
    double r = 0.0;
    if (mine) {
        p = ((const double2 *)P.pos)[src];
        if (step) r = P.reward_f64 ? ((const double *)P.reward)[src] : (double)((const float *)P.reward)[src];
    }
    s_pos[w][lane] = p;
    s_rew[w][lane] = r;
    __syncthreads();
    if (!on) return;

    // nearest other agent: the lowest j attaining the minimum of d2
    double best = INFINITY;
    int bj = -1;
    if (mine) {
        for (int j = 0; j < N; ++j) {
            const double2 q = s_pos[w][j];
            const double dx = p.x - q.x, dy = p.y - q.y;
            const double d2 = dx * dx + dy * dy;
            if (j != lane && d2 < best) {
                best = d2;
                bj = j;
            }
        }
    }
    const double near = sqrt(best);
    const double sep = wave_min(mine ? near : INFINITY);

    // running state of the track (the same for every lane)
    const int c = S.cursor[k];
    int len = 0, min_t = 0, flags = 0, row0 = c;
    double ret = 0.0, run_min = INFINITY;
    if (step) {
        len = S.run_len[k] + 1;
        ret = S.run_return[k];
        if (P.return_mode == 1) {
            ret += s_rew[w][0];
        } else {
            for (int i = 0; i < N; ++i) ret += s_rew[w][i];
        }
        run_min = S.run_min_sep[k];
        min_t = S.run_min_t[k];
        flags = S.run_flags[k];
        row0 = S.row0[k];
    }
    if (sep < run_min) {
        run_min = sep;
        min_t = len;
    }
    const uint8_t dn = mine && step ? P.done[src] : 0;
    if (__ballot(dn != 0) != 0) flags |= AAC_RECORD_EP_ANY_DONE;
    const bool fin = step && P.env_done[e] != 0;
    const bool wr = c < S.S;
    if (!wr) flags |= AAC_RECORD_EP_DROPPED;

    if (wr) {
        const size_t row = (size_t)k * S.S + c, dst = row * N + lane;
        if (mine) {
            ((double2 *)S.pos)[dst] = p;
            ((double2 *)S.vel)[dst] = ((const double2 *)P.vel)[src];
            ((double2 *)S.goal)[dst] = ((const double2 *)P.goal)[src];
            float2 a = make_float2(0.f, 0.f);
            if (step) {
                if (P.act_f64) {
                    const double2 ad = ((const double2 *)P.act)[src];
                    a = make_float2((float)ad.x, (float)ad.y);
                } else {
                    a = ((const float2 *)P.act)[src];
                }
            }
            ((float2 *)S.act)[dst] = a;
            S.reward[dst] = r;
            S.done[dst] = dn;
            S.mask[dst] = step ? P.mask[src] : (uint8_t)0;
            S.nearest[dst] = near;
            S.nearest_idx[dst] = bj;
            if (S.heading) S.heading[dst] = P.heading[src];
        }
        if (S.clouds && lane < 2 * AAC_RECORD_CLOUDS)
            S.clouds[row * (2 * AAC_RECORD_CLOUDS) + lane] = P.clouds[(size_t)e * (2 * AAC_RECORD_CLOUDS) + lane];
        if (lane == 0) {
            S.min_sep[row] = sep;
            ((int4 *)S.header)[row] = make_int4(P.episode[e], len, (fin ? AAC_RECORD_ROW_ENV_DONE : 0) | (step ? 0 : AAC_RECORD_ROW_RESET),
                                                P.map_idx ? P.map_idx[e] : 0);
        }
    }
    if (lane != 0) return;
    const int cn = wr ? c + 1 : c;
    S.cursor[k] = cn;
    if (!wr) S.dropped[k] += 1;
    S.run_len[k] = len;
    S.run_return[k] = ret;
    S.run_min_sep[k] = run_min;
    S.run_min_t[k] = min_t;
    S.run_flags[k] = flags;
    if (!step) S.row0[k] = row0;
    if (fin) {
        aac_record_episode ep;
        ep.ret = ret;
        ep.min_sep = run_min;
        ep.min_sep_t = min_t;
        ep.row0 = row0;
        ep.rows = cn - row0;
        ep.len = len;
        ep.episode = P.episode[e];
        ep.env = e;
        ep.flags = flags;
        ep.pad = 0;
        S.episodes[(size_t)k * S.P + seen] = ep;
        S.ep_seen[k] = seen + 1;
    }
}

}  // namespace

extern "C" {

const char *aac_record_last_error(void) { return s_err.c_str(); }

int aac_record(const aac_record_state *s, const aac_record_step *p, void *stream) {
    if (!s) return rfail(AAC_E_INVALID, "record: state");
    if (!p) return rfail(AAC_E_INVALID, "record: step");
    if (s->N < 1 || s->N > MAXA) return rfail(AAC_E_INVALID, "record: 1 <= N <= 64");
    if (s->T < 1 || s->S < 1 || s->P < 1) return rfail(AAC_E_INVALID, "record: T, S, P >= 1");
    if (!s->env_ids || !s->cursor || !s->ep_seen || !s->dropped || !s->run_len || !s->row0 || !s->run_min_t ||
        !s->run_flags || !s->run_return || !s->run_min_sep)
        return rfail(AAC_E_INVALID, "record: env_ids and running-state buffers");
    if (!s->header || !s->pos || !s->vel || !s->goal || !s->act || !s->reward || !s->done || !s->mask || !s->nearest ||
        !s->nearest_idx || !s->min_sep || !s->episodes)
        return rfail(AAC_E_INVALID, "record: row and summary buffers");
    if (p->phase != AAC_RECORD_RESET && p->phase != AAC_RECORD_STEP)
        return rfail(AAC_E_INVALID, "record: phase AAC_RECORD_RESET / AAC_RECORD_STEP");
    if (p->E <= 0) return rfail(AAC_E_INVALID, "record: E > 0");
    if (!p->pos || !p->vel || !p->goal || !p->episode) return rfail(AAC_E_INVALID, "record: state sources");
    if ((s->heading && !p->heading) || (s->clouds && !p->clouds))
        return rfail(AAC_E_INVALID, "record: heading / clouds rows need their sources");
    if (p->phase == AAC_RECORD_STEP && (!p->act || !p->reward || !p->done || !p->mask || !p->env_done))
        return rfail(AAC_E_INVALID, "record: step inputs");
    if (p->return_mode != 0 && p->return_mode != 1) return rfail(AAC_E_INVALID, "record: return_mode 0 / 1");
    if (p->max_episodes < 1 || p->max_episodes > s->P) return rfail(AAC_E_INVALID, "record: 1 <= max_episodes <= P");
    KArgs A;
    A.s = *s;
    A.p = *p;
    hipLaunchKernelGGL(record_kernel, dim3((s->T + TPW - 1) / TPW), dim3(TPW * 64), 0, (hipStream_t)stream, A);
    hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : rfail(AAC_E_HIP, std::string("record: ") + hipGetErrorString(err));
}

}  // extern "C"
