// aac_fused.hip -- grouped fp32 MFMA GEMM with fused epilogues, the critic head and the
// interleaving replay gather of the fused MADDPG learner (include/aac_fused.h).
//
// GEMM: one 256-thread workgroup per (product, 32x32 output tile, K split).  Each of its four
// waves accumulates the whole 32x32 tile = 2x2 tiles of v_mfma_f32_16x16x4_f32 (exact f32 fma
// chains, MI355X_MICROARCH.md "Matrix cores") over every fourth K chunk of 16, loading its MFMA
// fragments straight from global memory with the next chunk's loads in flight; the four
// partial tiles are summed through LDS in wave order (one barrier) and each wave runs the
// epilogue of one 16x16 quadrant.  The short dependent K chains of these small products are
// what bounds them, so K is cut four ways inside the workgroup before any split across them.
// Fragment k order is permuted so that lane group g = lane>>4 holds k = 4g..4g+3 of the chunk
// (the MFMA sums over k, so any order consistent between A and B is the same product): an
// operand that is contiguous along K with 16-B aligned rows is read as one float4 per fragment
// pair of k steps, any other as scalars whose 16 lanes cover 64 contiguous bytes.  Products
// with a large K and a small output (weight gradients) split K into partial copies of C that the
// optimiser sums (aac_adam_flat_sum), so there is no cross-workgroup reduction in the launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/aac_fused.h"
#include "aac_wave.h"
#include "aac_adam_bc.h"
#include "aac_copysum.h"

namespace {

thread_local std::string f_err;

int ffail(const std::string &m) {
    f_err = m;
    return -1;
}

#define FHIP(x)                                                                    \
    do {                                                                           \
        hipError_t e_ = (x);                                                       \
        if (e_ != hipSuccess) return ffail(std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int WT = 32;      // output tile edge per wave
constexpr int KC = 16;      // K chunk

struct GProb {
    const float *A, *B;
    float *C;
    const float *bias, *addend, *mask;
    float *cextra;
    int64_t sstride;
    int M, N, K;
    int lda, ldb, ldc, ldadd, ldmask;
    int ta, tb, act, mact, ones, ks;
    int amode, bmode;          // fragment load modes LV / LS / LT / LW
    int deep;                  // 4-deep prefetch ring (long chains) or none
    int wide;                  // one tile per wave, four adjacent tiles per workgroup
    int vec;                   // the epilogue may read / write 4 columns at once (16-B aligned rows)
    int tiles_n, w_begin;      // first workgroup of this product
    int lds;                   // 0: register fragments; 1 + cfg: LDS-staged workgroup tile (gemm_lds)
    int xcd;                   // LDS tile: XCD-aware workgroup order
    const float *dvec;         // dual output: C2[m][n] = C[m][n] > 0 ? dscale * dvec[n] : 0
    float *C2;
    float dscale;
};

using aacw::wsum;

struct HeadJob {          // aac_critic_head arguments (one wave per row, four rows per workgroup)
    const float *h, *w, *b, *y, *rew, *done;
    float *q, *dq, *dh, *yout;
    int ldh, M, mode, B, N;
    float gamma;
    // mode 2 only: the critic step's mse head (mode 0) on rows r < M2 of h2, chained on the TD
    // target just computed for row r (the critic step 0 of update_myown needs exactly y[0, B))
    const float *h2, *w2, *b2;
    float *q2, *dq2, *dh2;
    int M2;
};

__device__ __forceinline__ void mse_head_row(const float *h, int ldh, const float *w, const float *b, int M, int r,
                                             float y, float *q, float *dq, float *dh) {
    const int lane = threadIdx.x & 63;
    float hv[4], wv[4];
    float part = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hv[j] = h[(size_t)r * ldh + lane + 64 * j];
        wv[j] = w[lane + 64 * j];
        part = fmaf(hv[j], wv[j], part);
    }
    const float qv = wsum(part) + b[0];
    if (q && lane == 0) q[r] = qv;
    const float g = (2.0f / (float)M) * (qv - y);
    if (dq && lane == 0) dq[r] = g;
#pragma unroll
    for (int j = 0; j < 4; ++j) dh[(size_t)r * 256 + lane + 64 * j] = hv[j] > 0.0f ? g * wv[j] : 0.0f;
}

// CHAIN: the mode-2 job's chained mse head is compiled in (the standalone head kernel only; inside
// gemm_kernel the extra code made the compiler keep the by-value GBatch in scratch, 3.2 KB per lane)
template <bool CHAIN>
__device__ __forceinline__ void head_rows(const HeadJob &J, int blk) {
    const int r = blk * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= J.M) return;
    float hv[4], wv[4];
    float part = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        hv[j] = J.h[(size_t)r * J.ldh + lane + 64 * j];
        wv[j] = J.w[lane + 64 * j];
        part = fmaf(hv[j], wv[j], part);
    }
    const float qv = wsum(part) + J.b[0];
    if (J.q && lane == 0) J.q[r] = qv;
    if (J.mode == 2) {
        const int it = r / J.B;
        bool any = false;
        for (int n = 0; n < J.N; ++n) any |= J.done[(size_t)r * J.N + n] == 1.0f;
        const float yv = J.rew[(size_t)r * J.N + it] + (J.gamma * qv) * (1.0f - (any ? 1.0f : 0.0f));
        if (lane == 0) J.yout[r] = yv;
        if (CHAIN && r < J.M2) mse_head_row(J.h2, J.ldh, J.w2, J.b2, J.M2, r, yv, J.q2, J.dq2, J.dh2);
        return;
    }
    const float g = J.mode == 0 ? (2.0f / (float)J.M) * (qv - J.y[r]) : -(1.0f / (float)J.M);
    if (J.dq && lane == 0) J.dq[r] = g;
#pragma unroll
    for (int j = 0; j < 4; ++j) J.dh[(size_t)r * 256 + lane + 64 * j] = hv[j] > 0.0f ? g * wv[j] : 0.0f;
}

constexpr int HEAD_MAX = 1;   // critic-head row jobs that may ride along in one GEMM launch

struct GBatch {
    int wb[AAC_GEMM_MAX];      // first workgroup of each product (INT_MAX past n): the product
                               // select reads these 64 B with independent scalar loads
    int n, waves;
    int xcd_all;               // launch-wide XCD-aware workgroup order (AAC_GEMM_XCD_ALL)
    int hb[HEAD_MAX + 1];      // head jobs: workgroups [hb[j], hb[j + 1]) (hb[0] = waves of the products)
    int nh;
    GProb p[AAC_GEMM_MAX];
    HeadJob h[HEAD_MAX];
};

#ifdef AAC_GEMM_STAMPS
// diagnostic build only (tools/gemm_stamps.py): per-workgroup phase stamps of one launch, wave 0
// lane 0: [s_memrealtime at entry, s_memtime at entry / after the MFMA loop / at exit, XCC id]
constexpr int STAMP_WG = 16384;
__device__ unsigned long long g_gemm_st[STAMP_WG][5];
#define GSTAMP(k, v)                                                                                       \
    do {                                                                                                  \
        if (threadIdx.x == 0 && blockIdx.x < STAMP_WG) g_gemm_st[blockIdx.x][k] = (v);                   \
    } while (0)
#else
#define GSTAMP(k, v) \
    do {             \
    } while (0)
#endif

__device__ __forceinline__ void epilogue(const GProb &P, float *C, float *cx, int m, int n, float v) {
    if (m >= P.M || n >= P.N) return;
#ifdef AAC_DBG_NO_STORE      // timing probes only (a round-3 probe script, in the git history): keep the value live, store ~never
    if (v != 1234.5678f) return;
#endif
    if (P.ones && n == P.N - 1) {
        cx[m] = v;
        return;
    }
    if (P.addend) v += P.addend[(size_t)m * P.ldadd + n];
    if (P.bias) v += P.bias[n];
    if (P.act == 1) v = v > 0.0f ? v : 0.0f;
    else if (P.act == 2) v = tanhf(v);
    if (P.mact == 1) v = P.mask[(size_t)m * P.ldmask + n] > 0.0f ? v : 0.0f;
    else if (P.mact == 2) {
        const float t = P.mask[(size_t)m * P.ldmask + n];
        v = v * (1.0f - t * t);
    }
    C[(size_t)m * P.ldc + n] = v;
    if (P.C2) P.C2[(size_t)m * P.ldc + n] = v > 0.0f ? P.dscale * P.dvec[n] : 0.0f;
}

// Four adjacent columns n..n+3 of row m (n % 4 == 0): one 16-B load of the addend / mask / bias
// and one 16-B store when the product allows it (P.vec, every column real), else element-wise.
__device__ __forceinline__ void epilogue4(const GProb &P, float *C, float *cx, int m, int n, const float v[4]) {
    if (m >= P.M) return;
    if (!P.vec || n + 3 >= P.N - P.ones) {
#pragma unroll
        for (int t = 0; t < 4; ++t) epilogue(P, C, cx, m, n + t, v[t]);
        return;
    }
#ifdef AAC_DBG_NO_STORE
    if (v[0] != 1234.5678f) return;
#endif
    f4 x = {v[0], v[1], v[2], v[3]};
    if (P.addend) x += *reinterpret_cast<const f4 *>(P.addend + (size_t)m * P.ldadd + n);
    if (P.bias) x += *reinterpret_cast<const f4 *>(P.bias + n);
    if (P.act == 1) {
        x.x = x.x > 0.0f ? x.x : 0.0f;
        x.y = x.y > 0.0f ? x.y : 0.0f;
        x.z = x.z > 0.0f ? x.z : 0.0f;
        x.w = x.w > 0.0f ? x.w : 0.0f;
    } else if (P.act == 2) {
        x = f4{tanhf(x.x), tanhf(x.y), tanhf(x.z), tanhf(x.w)};
    }
    if (P.mact) {
        const f4 t = *reinterpret_cast<const f4 *>(P.mask + (size_t)m * P.ldmask + n);
        if (P.mact == 1) {
            x.x = t.x > 0.0f ? x.x : 0.0f;
            x.y = t.y > 0.0f ? x.y : 0.0f;
            x.z = t.z > 0.0f ? x.z : 0.0f;
            x.w = t.w > 0.0f ? x.w : 0.0f;
        } else {
            x = f4{x.x * (1.0f - t.x * t.x), x.y * (1.0f - t.y * t.y), x.z * (1.0f - t.z * t.z),
                   x.w * (1.0f - t.w * t.w)};
        }
    }
    *reinterpret_cast<f4 *>(C + (size_t)m * P.ldc + n) = x;
    if (P.C2) {      // the critic head's actor-loss gradient (dq = -1/B constant): dh = dq w (h > 0)
        const f4 w = *reinterpret_cast<const f4 *>(P.dvec + n);
        const float g = P.dscale;
        *reinterpret_cast<f4 *>(P.C2 + (size_t)m * P.ldc + n) =
            f4{x.x > 0.0f ? g * w.x : 0.0f, x.y > 0.0f ? g * w.y : 0.0f, x.z > 0.0f ? g * w.z : 0.0f,
               x.w > 0.0f ? g * w.w : 0.0f};
    }
}

// Fragment load modes of an operand whose rows are the MFMA row index (m for A, n for B):
//   LV  K-contiguous rows, ld % 4 == 0, K % 4 == 0, 16-B aligned: one 16-B load per row
//   LS  K-contiguous rows, otherwise: four 4-B loads
//   LT  row-contiguous (stored [k][row]): four 4-B loads, 16 lanes cover 64 contiguous bytes
//   LW  row-contiguous, rows % T == 0, ld % T == 0, 4T-B aligned: lane lr loads the T consecutive
//       rows T*lr .. T*lr + T-1 at one k with one 4T-B load (16 lanes cover 16T*4 contiguous
//       bytes, whole lines), so 16x16 block i holds the rows T*lr + i: the tile's rows are
//       permuted and the epilogue undoes it
// Loads are raw buffer loads; an element outside the operand (row >= rows, k >= K, or a chunk
// this wave does not own) gets an out-of-range offset and the hardware returns 0, so nothing
// touches a loaded value before its MFMA and the compiler's vmcnt tracking stays exact across
// the prefetch ring.  f[i][t] = op(X)[row0 + 16 i + lr][kc + 4 lk + t].
enum { LV = 0, LS = 1, LT = 2, LW = 3 };
constexpr int OOB = 0x7ffffff0;     // byte offset past every operand (= num_records)

typedef int i4 __attribute__((ext_vector_type(4)));
// the LLVM buffer-load intrinsics (the clang b128 builtin lowers to a single dword here)
__device__ f4 buf_load_x4(i4 rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.v4f32");
__device__ float buf_load_x1(i4 rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.f32");
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ f2 buf_load_x2(i4 rsrc, int voff, int soff, int aux) __asm("llvm.amdgcn.raw.buffer.load.v2f32");

__device__ __forceinline__ i4 rsrc_of(const float *p) {
    const uint64_t a = reinterpret_cast<uint64_t>(p);
    i4 r;
    r.x = __builtin_amdgcn_readfirstlane((int)(a & 0xffffffffu));
    r.y = __builtin_amdgcn_readfirstlane((int)(a >> 32));     // stride 0
    r.z = OOB;                                                 // num_records (bytes)
    r.w = 0x00020000;                                          // gfx9 dword3: 32-bit data format
    return r;
}

template <int MODE, int T>
__device__ __forceinline__ void load_frag(i4 X, int ld, int rows, int K, int kc, int row0,
                                          int lr, int lk, bool on, float f[T][4]) {
    const int k0 = kc + 4 * lk;
#ifdef AAC_DBG_NO_LOAD       // timing probes only: fragments from registers
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int t = 0; t < 4; ++t) f[i][t] = (float)(k0 + t + i) * 1e-3f;
    return;
#endif
    if (MODE == LW) {
        const int r = row0 + T * lr;
        const bool rin = on && r < rows;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int k = k0 + t;
            const int off = (rin && k < K) ? (k * ld + r) * 4 : OOB;
            if (T == 4) {
                const f4 v = buf_load_x4(X, off, 0, 0);
                f[0][t] = v.x;
                f[1 % T][t] = v.y;
                f[2 % T][t] = v.z;
                f[3 % T][t] = v.w;
            } else {
                const f2 v = buf_load_x2(X, off, 0, 0);
                f[0][t] = v.x;
                f[1 % T][t] = v.y;
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int r = row0 + 16 * i + lr;
        const bool rin = on && r < rows;
        if (MODE == LV) {
            const int off = (rin && k0 < K) ? (r * ld + k0) * 4 : OOB;
            const f4 v = buf_load_x4(X, off, 0, 0);
            f[i][0] = v.x;
            f[i][1] = v.y;
            f[i][2] = v.z;
            f[i][3] = v.w;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k = k0 + t;
                const int off = (rin && k < K) ? (MODE == LT ? k * ld + r : r * ld + k) * 4 : OOB;
                f[i][t] = buf_load_x1(X, off, 0, 0);
            }
        }
    }
}

// one (16T)x(16T) tile over this wave's chunks c0, c0+cstep, ... < c1 (D-deep register ring: the
// loads of the next D-1 chunks are in flight while one is multiplied; these chains are
// latency-bound).  The virtual ones row of op(B) (bias gradient) is a constant fragment: extra
// MFMAs in the one tile column that holds it.
template <int AM, int BM, int D, int T>
__device__ __forceinline__ void tile_mma(const GProb &P, int m0, int n0, int c0, int c1, int cstep, int lr,
                                         int lk, f4 acc[T][T]) {
    const int nreal = P.N - P.ones;
    const i4 ra = rsrc_of(P.A), rb = rsrc_of(P.B);
    const bool has_one = P.ones && nreal >= n0 && nreal < n0 + 16 * T;      // wave-uniform
    float one[T];
#pragma unroll
    for (int j = 0; j < T; ++j) one[j] = ((BM == LW ? n0 + T * lr + j : n0 + 16 * j + lr) == nreal) ? 1.0f : 0.0f;
    float fa[D][T][4], fb[D][T][4];
    const int nmine = c0 < c1 ? (c1 - c0 + cstep - 1) / cstep : 0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const bool on = d < nmine;
        const int kc = (c0 + cstep * d) * KC;
        load_frag<AM, T>(ra, P.lda, P.M, P.K, kc, m0, lr, lk, on, fa[d]);
        load_frag<BM, T>(rb, P.ldb, nreal, P.K, kc, n0, lr, lk, on, fb[d]);
    }
    for (int q0 = 0; q0 < nmine; q0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < T; ++i)
#pragma unroll
                    for (int j = 0; j < T; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[d][i][t], fb[d][j][t], acc[i][j], 0, 0, 0);
            if (has_one) {
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int i = 0; i < T; ++i)
#pragma unroll
                        for (int j = 0; j < T; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[d][i][t], one[j], acc[i][j], 0, 0, 0);
            }
            const int qn = q0 + d + D;
            const bool on = qn < nmine;
            const int kc = (c0 + cstep * qn) * KC;
            load_frag<AM, T>(ra, P.lda, P.M, P.K, kc, m0, lr, lk, on, fa[d]);
            load_frag<BM, T>(rb, P.ldb, nreal, P.K, kc, n0, lr, lk, on, fb[d]);
            // keep the refill issued here: left to itself the scheduler sinks it below the next
            // stage's wait, and the ring holds one chunk in flight instead of D
            if (D > 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// One workgroup's share of product P with (16T)x(16T) wave tiles.
template <int T, int DEPTH>
__device__ __forceinline__ void gemm_tile(const GProb &P, int local, f4 (*red)[4][64], float *tile) {
    constexpr int TW = 16 * T;
    const int s = local % P.ks;
    const int w = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int lr = lane & 15, lk = lane >> 4;
    const int nch = (P.K + KC - 1) / KC;
    const int per = (nch + P.ks - 1) / P.ks;
    int m0, n0, c0, cstep;
    if (P.wide) {
        // wide: the four waves take four adjacent tiles of one row block (A rows shared through
        // L1), each over the whole K range of the split
        const int grp = local / P.ks;
        const int gpr = (P.tiles_n + 3) / 4;
        const int tn = (grp % gpr) * 4 + w;
        if (tn >= P.tiles_n) return;
        m0 = (grp / gpr) * TW;
        n0 = tn * TW;
        c0 = s * per;
        cstep = 1;
    } else {
        // the four waves share one tile and take every fourth chunk of the split
        const int tile = local / P.ks;
        m0 = (tile / P.tiles_n) * TW;
        n0 = (tile % P.tiles_n) * TW;
        c0 = s * per + w;
        cstep = 4;
    }
    const int c1 = min(nch, s * per + per);

    f4 acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    // the deep-ring instantiations need more VGPRs; launches without a long-K product use the
    // shallow kernel so the large memory-bound products keep their occupancy
#define TM(a, b)                                                                                            \
    case (a * 4 + b) * 2 + 0: tile_mma<a, b, 1, T>(P, m0, n0, c0, c1, cstep, lr, lk, acc); break;          \
    case (a * 4 + b) * 2 + 1: tile_mma<a, b, DEPTH, T>(P, m0, n0, c0, c1, cstep, lr, lk, acc); break;
    switch ((P.amode * 4 + P.bmode) * 2 + P.deep) {
        TM(LV, LV) TM(LV, LS) TM(LV, LT) TM(LV, LW) TM(LS, LV) TM(LS, LS) TM(LS, LT) TM(LS, LW)
        TM(LT, LV) TM(LT, LS) TM(LT, LT) TM(LT, LW) TM(LW, LV) TM(LW, LS) TM(LW, LT) TM(LW, LW)
    }
#undef TM
    GSTAMP(2, __builtin_amdgcn_s_memtime());
    float *C = P.C ? P.C + (int64_t)s * P.sstride : nullptr;
    float *cx = P.cextra ? P.cextra + (int64_t)s * P.sstride : nullptr;
    // output row / column of element (block, position) of the tile (LW operands permute them)
    const bool pa = P.amode == LW, pb = P.bmode == LW;
    auto row_of = [&](int i, int rho) { return pa ? m0 + T * rho + i : m0 + 16 * i + rho; };
    auto col_of = [&](int j, int c) { return pb ? n0 + T * c + j : n0 + 16 * j + c; };
    if (P.wide) {
        // stage the wave's tile in its quarter of the reduction buffer at its true (row, col)
        // position, then write whole 16-B row segments (the fragment layout would store single
        // floats, 64 B per row group)
        float *st = reinterpret_cast<float *>(red[w]);
#pragma unroll
        for (int i = 0; i < T; ++i)
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    st[(row_of(i, lk * 4 + r) - m0) * TW + (col_of(j, lr) - n0)] = acc[i][j][r];
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");       // one wave's LDS operations run in order
#pragma unroll
        for (int q = 0; q < TW * TW / 256; ++q) {
            const int idx = q * 64 + lane;
            const int rr = idx / (TW / 4), c4 = (idx % (TW / 4)) * 4;
            const f4 x = *reinterpret_cast<const f4 *>(st + rr * TW + c4);
            const float v[4] = {x.x, x.y, x.z, x.w};
            epilogue4(P, C, cx, m0 + rr, n0 + c4, v);
        }
        return;
    }
    // reduce the four waves' partial tiles in wave order, four 16x16 blocks per round; in round
    // r wave q finishes block 4r + q
    if (T == 2) {
        // one round; the reduced tile is staged at its true (row, col) positions so that every
        // thread writes one 16-B row segment (the fragment layout would store single floats)
#pragma unroll
        for (int q = 0; q < 4; ++q) red[w][q][lane] = acc[q / T][q % T];
        __syncthreads();
        const f4 v = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
        const int i = w / T, j = w % T;
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(row_of(i, lk * 4 + r) - m0) * TW + (col_of(j, lr) - n0)] = v[r];
        __syncthreads();
        const int rr = threadIdx.x / (TW / 4), c4 = (threadIdx.x % (TW / 4)) * 4;
        const f4 x = *reinterpret_cast<const f4 *>(tile + rr * TW + c4);
        const float vv[4] = {x.x, x.y, x.z, x.w};
        epilogue4(P, C, cx, m0 + rr, n0 + c4, vv);
        return;
    }
#pragma unroll
    for (int r0 = 0; r0 < T * T; r0 += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) red[w][q][lane] = acc[(r0 + q) / T][(r0 + q) % T];
        __syncthreads();
        const f4 v = ((red[0][w][lane] + red[1][w][lane]) + red[2][w][lane]) + red[3][w][lane];
        const int i = (r0 + w) / T, j = (r0 + w) % T;
#pragma unroll
        for (int r = 0; r < 4; ++r) epilogue(P, C, cx, row_of(i, lk * 4 + r), col_of(j, lr), v[r]);
        if (r0 + 4 < T * T) __syncthreads();
    }
}

// ---------------------------------------------------------------- LDS-staged workgroup tiles
// Products whose operands load as 16-B segments take (32 TI) x (32 TJ) workgroup tiles: 2 x 2 waves
// of (16 TI) x (16 TJ).  K goes in chunks of LBK = 32 through an S-stage LDS ring filled by LDS-DMA
// (buffer_load_dwordx4 ... lds: no VGPRs, no ds_write): S - 1 chunks are in flight while one is
// multiplied, one barrier per chunk, counted vmcnt waits.  Every operand byte crosses L2 once per
// workgroup tile instead of once per wave tile.  A DMA instruction fills 64 consecutive 16-B slots
// (lane-linear), so the swizzles live in the per-lane source addresses:
//   K-contiguous operand ([row][k]): slot = row * 8 + (k/4 ^ (row & 7)); one ds_read_b128 per
//     fragment, conflict-free for the lane groups of ds_read_b128; a DMA instruction reads 8 whole
//     128-B row lines
//   row-contiguous operand ([k][row]): slot = k * rows/4 + (row/4 ^ 4 ((k/4) & 1)); four ds_read_b32
//     per fragment, the 32 lanes of each on distinct banks; a DMA instruction reads 4 (8) whole rows
// (tools enumerate both: tests/test_fused_gpu.py covers every layout.)  Lane (lr, lk) multiplies
// k = 16 h + 4 lk + t at step (h, t) -- one permutation of the chunk for both operands.  The ones
// column of op(B) (bias gradient) reads as 0 from its out-of-range segment and is set to 1 in the
// fragment of the lane that holds it.
constexpr int LBK = 32;
typedef __attribute__((address_space(3))) void *lds_vp;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t brsrc_of(const float *p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), (short)0, OOB, 0x00020000);
}

template <int TI, int TJ>
struct LCfg {
    static constexpr int BM = 32 * TI, BN = 32 * TJ;
    static constexpr int STAGE = (BM + BN) * LBK;                     // floats per ring stage
#ifdef AAC_LDS_STAGES
    static constexpr int S = AAC_LDS_STAGES;
#else
    // ring stages: 2 (32 / 24 / 24 / 16 KB) -- more workgroups per CU beat a deeper ring on every
    // learner shape (3 / 4 stages: +3 / +6 % over the large shapes, tools/mb_lds.py)
    static constexpr int S = 2;
#endif
    static constexpr int PW = (BM + BN) / 32;                         // DMA instructions per wave per chunk
    static constexpr int BYTES = S * STAGE * 4;
};

// one operand image (ROWS rows x LBK k) per chunk: ROWS / 8 DMA instructions, wave w issues w,
// w + 4, ...  The per-lane source offsets are set up once (LDma::init); a chunk adds a uniform
// step and checks the K bound (the last chunk may be partial)
template <int ROWS, bool KC>
struct LDma {
    static constexpr int NI = ROWS / 32;      // instructions per wave
    int base[NI];                             // byte offset at chunk 0, or OOB (row out of range)
    int kx[NI];                               // the lane's k within a chunk (its segment's first k)
    __device__ __forceinline__ void init(int ld, int rows, int row0, int w, int lane) {
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int sl = 64 * (w + 4 * i) + lane;
            if (KC) {
                const int row = sl >> 3, seg = (sl & 7) ^ (row & 7);
                const int gr = row0 + row;
                base[i] = gr < rows ? (gr * ld + 4 * seg) * 4 : OOB;
                kx[i] = 4 * seg;
            } else {
                const int k = sl / (ROWS / 4), seg = (sl % (ROWS / 4)) ^ (((k >> 2) & 1) << 2);
                const int gr = row0 + 4 * seg;
                base[i] = gr < rows ? (k * ld + gr) * 4 : OOB;
                kx[i] = k;
            }
        }
    }
    __device__ __forceinline__ void issue(__amdgpu_buffer_rsrc_t X, int ld, int K, int kc, float *img, int w) const {
        const int step = KC ? kc * 4 : kc * ld * 4;        // uniform
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int off = (base[i] != OOB && kx[i] < K - kc) ? base[i] + step : OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(X, (lds_vp)(img + 256 * (w + 4 * i)), 16, off, 0, 0, 0);
        }
    }
};

template <int ROWS, bool KC, int T>
__device__ __forceinline__ void lds_frag(const float *img, int rbase, int h, int lr, int lk, float (&f)[T][4]) {
#pragma unroll
    for (int i = 0; i < T; ++i) {
        const int row = rbase + 16 * i + lr;
        if (KC) {
            const int seg = 4 * h + lk;
            const f4 v = *reinterpret_cast<const f4 *>(img + 4 * (row * 8 + (seg ^ (row & 7))));
            f[i][0] = v.x;
            f[i][1] = v.y;
            f[i][2] = v.z;
            f[i][3] = v.w;
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int k = 16 * h + 4 * lk + t;
                f[i][t] = img[4 * (k * (ROWS / 4) + ((row >> 2) ^ (((k >> 2) & 1) << 2))) + (row & 3)];
            }
        }
    }
}

// s_waitcnt vmcnt(n) for a small run-time n (the immediate must be a constant)
__device__ __forceinline__ void vm_wait(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" ::: "memory"); break;
        case 10: asm volatile("s_waitcnt vmcnt(10)" ::: "memory"); break;
        case 11: asm volatile("s_waitcnt vmcnt(11)" ::: "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    }
}

template <int TI, int TJ, bool AK, bool BKC>
__device__ __forceinline__ void gemm_lds(const GProb &P, int local, float *smem) {
    using L = LCfg<TI, TJ>;
    constexpr int BM = L::BM, BN = L::BN, S = L::S, ST = L::STAGE, SA = BM * LBK;
    static_assert((S - 2) * L::PW <= 12, "vm_wait range");
    if (P.xcd) {
        // XCD-aware order: workgroup b runs on XCD b % 8 (round-robin dispatch), so hand each XCD a
        // contiguous range of tiles -- the column tiles of a row block then share that XCD's L2
        // (bijective also when the count is not a multiple of 8)
        const int n = P.tiles_n * ((P.M + BM - 1) / BM) * P.ks;
        const int q = n / 8, r = n % 8, x = local % 8, o = local / 8;
        local = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + o;
    }
    const int s = local % P.ks, tile = local / P.ks;
    const int m0 = (tile / P.tiles_n) * BM, n0 = (tile % P.tiles_n) * BN;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int lr = lane & 15, lk = lane >> 4;
    const int wm = (w >> 1) * 16 * TI, wn = (w & 1) * 16 * TJ;
    const int nreal = P.N - P.ones;
    const int nch = (P.K + LBK - 1) / LBK, per = (nch + P.ks - 1) / P.ks;
    const int c0 = s * per, c1 = min(nch, c0 + per);
    const __amdgpu_buffer_rsrc_t ra = brsrc_of(P.A), rb = brsrc_of(P.B);
    const int one_col = (P.ones && nreal >= n0 && nreal < n0 + BN) ? nreal - n0 : -1;
    LDma<BM, AK> da;
    LDma<BN, BKC> db;
    da.init(P.lda, P.M, m0, w, lane);
    db.init(P.ldb, nreal, n0, w, lane);
    auto issue = [&](int c) {
        float *img = smem + ((c - c0) % S) * ST;
        da.issue(ra, P.lda, P.K, c * LBK, img, w);
        db.issue(rb, P.ldb, P.K, c * LBK, img + SA, w);
    };
    f4 acc[TI][TJ];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j) acc[i][j] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int q = 0; q < S - 1; ++q)
        if (c0 + q < c1) issue(c0 + q);
    for (int c = c0; c < c1; ++c) {
        // this wave's DMAs of chunk c have landed (the younger ones may still fly), then every
        // wave's have, and every wave is done with chunk c - 1, whose stage chunk c + S - 1 reuses
        vm_wait(min(S - 2, c1 - 1 - c) * L::PW);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");      // no LDS access moves above the barrier
        const float *cur = smem + ((c - c0) % S) * ST;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float fa[TI][4], fb[TJ][4];
            lds_frag<BM, AK, TI>(cur, wm, h, lr, lk, fa);
            lds_frag<BN, BKC, TJ>(cur + SA, wn, h, lr, lk, fb);
            // the next DMA behind the first fragment reads (their latency covers its issue)
            if (h == 0 && c + S - 1 < c1) issue(c + S - 1);
            if (one_col >= 0) {
#pragma unroll
                for (int j = 0; j < TJ; ++j)
#pragma unroll
                    for (int t = 0; t < 4; ++t) fb[j][t] = wn + 16 * j + lr == one_col ? 1.0f : fb[j][t];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int i = 0; i < TI; ++i)
#pragma unroll
                    for (int j = 0; j < TJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][t], fb[j][t], acc[i][j], 0, 0, 0);
        }
    }
    GSTAMP(2, __builtin_amdgcn_s_memtime());
    // every wave is done reading the ring: the tile through LDS (rows of BN + 4 floats) for 16-B
    // row segments in the epilogue
    aacw::lds_barrier();
    float *ct = smem;
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int j = 0; j < TJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) ct[(wm + 16 * i + 4 * lk + r) * (BN + 4) + wn + 16 * j + lr] = acc[i][j][r];
    aacw::lds_barrier();
    float *C = P.C ? P.C + (int64_t)s * P.sstride : nullptr;
    float *cx = P.cextra ? P.cextra + (int64_t)s * P.sstride : nullptr;
    constexpr int RPI = 256 / (BN / 4);          // rows per pass; a thread keeps its 4 columns
    const int c4 = (threadIdx.x % (BN / 4)) * 4, r0 = threadIdx.x / (BN / 4);
    if (P.vec && !P.C2 && m0 + BM <= P.M && n0 + BN <= nreal) {
        // interior tile, 16-B rows: the bias once, every pass's addend / mask loads issued before
        // the first store (element-by-element the loop waited on each load in turn)
        f4 bias = f4{0.0f, 0.0f, 0.0f, 0.0f};
        if (P.bias) bias = *reinterpret_cast<const f4 *>(P.bias + n0 + c4);
        f4 add[BM / RPI], msk[BM / RPI];
#pragma unroll
        for (int it = 0; it < BM / RPI; ++it) {
            const int m = m0 + r0 + RPI * it;
            add[it] = P.addend ? *reinterpret_cast<const f4 *>(P.addend + (size_t)m * P.ldadd + n0 + c4)
                               : f4{0.0f, 0.0f, 0.0f, 0.0f};
            msk[it] = P.mact ? *reinterpret_cast<const f4 *>(P.mask + (size_t)m * P.ldmask + n0 + c4)
                             : f4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int it = 0; it < BM / RPI; ++it) {
            const int rr = r0 + RPI * it;
            f4 x = *reinterpret_cast<const f4 *>(ct + rr * (BN + 4) + c4);
            // the operation order of epilogue(): addend, then bias, then the activations
            if (P.addend) x += add[it];
            if (P.bias) x += bias;
            if (P.act == 1) {
                x.x = x.x > 0.0f ? x.x : 0.0f;
                x.y = x.y > 0.0f ? x.y : 0.0f;
                x.z = x.z > 0.0f ? x.z : 0.0f;
                x.w = x.w > 0.0f ? x.w : 0.0f;
            } else if (P.act == 2) {
                x = f4{tanhf(x.x), tanhf(x.y), tanhf(x.z), tanhf(x.w)};
            }
            const f4 t = msk[it];
            if (P.mact == 1) {
                x.x = t.x > 0.0f ? x.x : 0.0f;
                x.y = t.y > 0.0f ? x.y : 0.0f;
                x.z = t.z > 0.0f ? x.z : 0.0f;
                x.w = t.w > 0.0f ? x.w : 0.0f;
            } else if (P.mact == 2) {
                x = f4{x.x * (1.0f - t.x * t.x), x.y * (1.0f - t.y * t.y), x.z * (1.0f - t.z * t.z),
                       x.w * (1.0f - t.w * t.w)};
            }
            *reinterpret_cast<f4 *>(C + (size_t)(m0 + rr) * P.ldc + n0 + c4) = x;
        }
        return;
    }
#pragma unroll
    for (int it = 0; it < BM / RPI; ++it) {
        const int rr = r0 + RPI * it;
        const f4 x = *reinterpret_cast<const f4 *>(ct + rr * (BN + 4) + c4);
        const float v[4] = {x.x, x.y, x.z, x.w};
        epilogue4(P, C, cx, m0 + rr, n0 + c4, v);
    }
}

static_assert(LCfg<2, 2>::BYTES >= 64 * 68 * 4 && LCfg<2, 1>::BYTES >= 64 * 36 * 4 && LCfg<1, 2>::BYTES >= 32 * 68 * 4 &&
                  LCfg<1, 1>::BYTES >= 32 * 36 * 4,
              "the epilogue tile fits the ring");
constexpr int REG_LDS_BYTES = 4 * 4 * 64 * 16 + 32 * 32 * 4;    // the register path's reduction buffers

template <int TI, int TJ>
__device__ __forceinline__ void gemm_lds_layout(const GProb &P, int local, float *smem, int lay) {
    switch (lay) {
        case 0: gemm_lds<TI, TJ, true, true>(P, local, smem); break;
        case 1: gemm_lds<TI, TJ, true, false>(P, local, smem); break;
        case 2: gemm_lds<TI, TJ, false, true>(P, local, smem); break;
        default: gemm_lds<TI, TJ, false, false>(P, local, smem); break;
    }
}

extern __shared__ float4 g_dyn_lds[];

// 5 waves per SIMD (<= 102 registers: 94, no scratch): 5 workgroups per CU instead of 4 (the 77 + 24
// accumulation registers of the default allocation) -- +0.8 % config 3; 6 spilled (52 B) and lost 4 %
template <int DEPTH, bool LDST>
__global__ void __launch_bounds__(256, 5) gemm_kernel(GBatch g) {
    // LDST: the launch holds LDS-tile products: ONE dynamic LDS array (sized for the launch's largest
    // ring; a second __shared__ object would make the compiler drain the DMAs before every ds_read),
    // the register path's buffers alias it
    __shared__ float4 smem_static[LDST ? 1 : REG_LDS_BYTES / 16];
    float *smem = reinterpret_cast<float *>(LDST ? g_dyn_lds : smem_static);
    f4 (*red)[4][64] = reinterpret_cast<f4 (*)[4][64]>(smem);     // [wave][block of the round][lane]
    float *tile = smem + 4 * 4 * 64 * 4;                             // the reduced 32x32 tile
#ifdef AAC_DBG_EMPTY                   // timing probes only: the launch floor of this grid
    if (g.n > 0) return;
#endif
    GSTAMP(0, __builtin_amdgcn_s_memrealtime());
    GSTAMP(1, __builtin_amdgcn_s_memtime());
    int wg = blockIdx.x;
    if (g.xcd_all) {
        // workgroup b is dispatched to XCD b % 8: give each XCD a contiguous range of the launch's
        // workgroups, so that the tiles of one product share an XCD's L2 (bijective for any count)
        const int n = gridDim.x, q = n / 8, r = n % 8, x = wg % 8, o = wg / 8;
        wg = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + o;
    }
    if (wg >= g.hb[0]) {       // a critic-head job riding along (independent of the products)
        // static indices, copied by value: a dynamically indexed reference into the by-value
        // kernel argument made the compiler copy the whole GBatch to scratch (3.4 KB per lane)
        const HeadJob J = g.h[0];
        head_rows<false>(J, wg - g.hb[0]);
        return;
    }
    // product of this workgroup: count the products that start at or before it (wb is ascending,
    // wb[0] = 0); independent loads instead of a dependent scan of the kernel arguments
    int pi = 0;
#pragma unroll
    for (int k = 1; k < AAC_GEMM_MAX; ++k) pi += wg >= g.wb[k] ? 1 : 0;
    if (LDST && g.p[pi].lds) {
        const GProb P = g.p[pi];       // by value: a reference would make the compiler copy g to scratch
        const int cfg = P.lds - 1, lay = cfg & 3;
        switch (cfg >> 2) {      // (TI, TJ): 64x64, 64x32, 32x64, 32x32 workgroup tiles
            case 0: gemm_lds_layout<2, 2>(P, wg - P.w_begin, smem, lay); break;
            case 1: gemm_lds_layout<2, 1>(P, wg - P.w_begin, smem, lay); break;
            case 2: gemm_lds_layout<1, 2>(P, wg - P.w_begin, smem, lay); break;
            default: gemm_lds_layout<1, 1>(P, wg - P.w_begin, smem, lay); break;
        }
    } else {
        const GProb &P = g.p[pi];
        gemm_tile<2, DEPTH>(P, wg - P.w_begin, red, tile);
    }
    GSTAMP(3, __builtin_amdgcn_s_memtime());
    GSTAMP(4, __builtin_amdgcn_s_memrealtime());
}

// ------------------------------------------------------------------------------ optimiser
// the copies in sequence (aac_copysum.h, order 0), one element per thread
using aaccs::copy_sum_seq;

__global__ void adam_sum_kernel(float *p, const float *__restrict__ gpart, int ns, int64_t gs, float *gout, float *m,
                                float *v, int64_t n, float lr, float b1, float b2, float eps, const int32_t *step, int step_add) {
    __shared__ float bc[2];
    const int t = *step + step_add;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    // the first trip's loads go out ahead of the bias corrections (clamped index, unconditional: a
    // thread past n still reaches the barrier in adam_bias_bcast)
    const int64_t ic = i < n ? i : n - 1;
    float m0 = m[ic], v0 = v[ic], p0 = p[ic];
    const float g0 = gpart[ic];
    float step_size, bc2s;
    adam_bias_bcast(bc, lr, b1, b2, t, step_size, bc2s);
    float gi = copy_sum_seq(gpart, ns, gs, ic, g0);
    while (i < n) {
        if (gout) gout[i] = gi;
        adam_elem(p0, m0, v0, gi, b1, b2, eps, step_size, bc2s);
        p[i] = p0;
        m[i] = m0;
        v[i] = v0;
        i += stride;
        if (i >= n) break;
        m0 = m[i], v0 = v[i], p0 = p[i];
        gi = copy_sum_seq(gpart, ns, gs, i, gpart[i]);
    }
}

// Copy-parallel form of the four-group order (aac_copysum.h, order 1), for copy stride gs % 4 == 0
// (the learners pad it) and 16-B aligned copies: a wave takes 64 consecutive elements; lane
// (g = lane / 16, e4 = lane % 16) sums copies g, g + 4, g + 8, ... of elements 4 e4 .. 4 e4 + 3 with
// 16-B loads (each copy's 64 elements are one 256-B line; up to eight loads in flight per lane), two
// xor shuffles combine the groups, and lane (g, e4) updates element 4 e4 + g.  The split-K copies of one
// network are 8-32 x its size, so this kernel is bound by how many of their loads are in flight.
//
// the eight loads of copies s0, s0 + 4, .. s0 + 28 (clamped copy index, unconditional: selected when
// they are summed -- a select around each load would make the compiler branch and drain per load)
__device__ __forceinline__ void copy_load8(const float *__restrict__ gpart, int ns, int64_t gs, int64_t ii, int s0,
                                           f4 (&x)[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int sc = s0 + 4 * u;
        x[u] = *reinterpret_cast<const f4 *>(gpart + (int64_t)(sc < ns ? sc : 0) * gs + ii);
    }
}

// x: copy_load8 of s0 = g, issued by the caller (as early as it likes)
__device__ __forceinline__ f4 copy_sum4(const float *__restrict__ gpart, int ns, int64_t gs, int64_t ii, int g,
                                        f4 (&x)[8]) {
    f4 acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int s0 = g; s0 < ns; s0 += 32) {
        if (s0 != g) copy_load8(gpart, ns, gs, ii, s0, x);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (s0 + 4 * u < ns) acc += x[u];
    }
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {
        acc.x += __shfl_xor(acc.x, d, 64);
        acc.y += __shfl_xor(acc.y, d, 64);
        acc.z += __shfl_xor(acc.z, d, 64);
        acc.w += __shfl_xor(acc.w, d, 64);
    }
    return acc;
}

__device__ __forceinline__ f4 copy_sum4(const float *__restrict__ gpart, int ns, int64_t gs, int64_t ii, int g) {
    f4 x[8];
    copy_load8(gpart, ns, gs, ii, g, x);
    return copy_sum4(gpart, ns, gs, ii, g, x);
}

struct Adam4 {         // one network's Adam over its split-K copies (copy stride gs % 4 == 0)
    float *p;
    const float *gpart;
    float *gout, *m, *v;
    const int32_t *step;
    int64_t gs, n;
    float lr, b1, b2, eps;
    int ns, step_add;
};

// the copy-parallel Adam of one network by workgroups blk = 0 .. nblk-1 (bc: two floats of LDS).
// Every thread of the workgroup comes through here, a wave with no element (base >= n) included:
// adam_bias_bcast holds the workgroup barrier, and the loop with its exits starts only after it.
__device__ __forceinline__ void adam4_body(const Adam4 &P, int64_t blk, int64_t nblk, float *bc) {
    const int lane = threadIdx.x & 63, g = lane >> 4, e4 = lane & 15;
    const int64_t wave = blk * 4 + (threadIdx.x >> 6), nwaves = nblk * 4;
    const int t = *P.step + P.step_add;
    int64_t base = wave * 64;
    int64_t i = base + 4 * e4, k = i + g;
    // the first trip's loads ahead of the bias corrections: the element's optimiser state (clamped
    // index, unconditional) in flight with the copy loads instead of after their sum
    int64_t kc = k < P.n ? k : P.n - 1, ic = i < P.n ? i : 0;
    float m0 = P.m[kc], v0 = P.v[kc], p0 = P.p[kc];
    f4 x[8];
    copy_load8(P.gpart, P.ns, P.gs, ic, g, x);
    float step_size, bc2s;
    adam_bias_bcast(bc, P.lr, P.b1, P.b2, t, step_size, bc2s);
    while (base < P.n) {
        const f4 acc = copy_sum4(P.gpart, P.ns, P.gs, ic, g, x);
        if (k < P.n) {
            const float gi = g == 0 ? acc.x : (g == 1 ? acc.y : (g == 2 ? acc.z : acc.w));
            if (P.gout) P.gout[k] = gi;
            adam_elem(p0, m0, v0, gi, P.b1, P.b2, P.eps, step_size, bc2s);
            P.p[k] = p0;
            P.m[k] = m0;
            P.v[k] = v0;
        }
        base += nwaves * 64;
        if (base >= P.n) break;
        i = base + 4 * e4, k = i + g;
        kc = k < P.n ? k : P.n - 1, ic = i < P.n ? i : 0;
        m0 = P.m[kc], v0 = P.v[kc], p0 = P.p[kc];
        copy_load8(P.gpart, P.ns, P.gs, ic, g, x);
    }
}

__global__ void __launch_bounds__(256) adam_sum4_kernel(Adam4 P) {
    __shared__ float bc[2];
    adam4_body(P, blockIdx.x, gridDim.x, bc);
}

// two networks in one launch (the critic step of iteration i+1 and the actor step of iteration i
// end together): workgroups [0, g1) take the first, the rest the second (a workgroup-uniform branch,
// so each side's barrier is reached by whole workgroups)
__global__ void __launch_bounds__(256) adam_sum4_pair_kernel(Adam4 P0, Adam4 P1, int g1) {
    __shared__ float bc[2];
    if ((int)blockIdx.x < g1) adam4_body(P0, blockIdx.x, g1, bc);
    else adam4_body(P1, blockIdx.x - g1, gridDim.x - g1, bc);
}

__global__ void __launch_bounds__(256) sum_partials4_kernel(float *out, const float *__restrict__ gpart, int ns,
                                                            int64_t gs, int64_t n) {
    const int lane = threadIdx.x & 63, g = lane >> 4, e4 = lane & 15;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    for (int64_t base = wave * 64; base < n; base += nwaves * 64) {
        const int64_t i = base + 4 * e4;
        const f4 acc = copy_sum4(gpart, ns, gs, i < n ? i : 0, g);
        const int64_t k = i + g;
        if (k < n) out[k] = g == 0 ? acc.x : (g == 1 ? acc.y : (g == 2 ? acc.z : acc.w));
    }
}

__global__ void sum_partials_kernel(float *out, const float *__restrict__ gpart, int ns, int64_t gs, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = copy_sum_seq(gpart, ns, gs, i, gpart[i]);
}

// ------------------------------------------------------------------------------ critic head
using aacw::wsum;
using aacw::wsum_n;


__global__ void __launch_bounds__(256) head_kernel(HeadJob J) { head_rows<true>(J, blockIdx.x); }

// ------------------------------------------------------------------------------ actor output backward
// Gradient through the critic's action inputs into the actor's tanh output layer, one wave per
// actor row r = b*N + n (ATT/maddpg:421-425 backward):
//   da_j   = sum_k df[b][n*128 + k] W_enc_n[k][D0 + j]       (d loss / d a_j via encoder n)
//   dout_j = da_j (1 - a_j^2)                                 (tanh, ATT/nets:184)
//   dh_a   = (dout_0 Wa[0] + dout_1 Wa[1]) * (h_a > 0)         (act_out + merge ReLU)
__global__ void __launch_bounds__(256) actor_out_bwd_kernel(const float *__restrict__ df, int ldf,
                                                            const float *__restrict__ wenc, int din, int d0,
                                                            const float *__restrict__ X, const float *__restrict__ wa,
                                                            const float *__restrict__ ha, int N, int R, float *dout,
                                                            float *dha) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= R) return;
    const int b = r / N, n = r - b * N;
    const float *dfr = df + (size_t)b * ldf + n * 128;
    const float *w = wenc + (size_t)n * 128 * din + d0;
    float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int k = lane + 64 * q;
        const float g = dfr[k];
        p0 = fmaf(g, w[k * din], p0);
        p1 = fmaf(g, w[k * din + 1], p1);
    }
    const float da0 = wsum(p0), da1 = wsum(p1);
    const float *a = X + ((size_t)b * N + n) * din + d0;
    const float a0 = a[0], a1 = a[1];
    const float o0 = da0 * (1.0f - a0 * a0), o1 = da1 * (1.0f - a1 * a1);
    if (lane == 0) {
        dout[(size_t)r * 2] = o0;
        dout[(size_t)r * 2 + 1] = o1;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c = lane + 64 * q;
        const float v = o0 * wa[c] + o1 * wa[256 + c];
        dha[(size_t)r * 256 + c] = ha[(size_t)r * 256 + c] > 0.0f ? v : 0.0f;
    }
}

// ------------------------------------------------------------------------------ attention block
// Inference form of the actor's neighbour attention (ATT/nets:186-210) for one row per wave
// iteration, lane = feature:
//   x_j   = relu(Wn nei_j + bn)                       (neighbour encoder, on the fly from the
//                                                      6-wide rows: no [rows*K][64] tensor)
//   s_j   = (Wk x_j) . (Wq e_o) / 8 = x_j . (Wqk e_o) / 8,   Wqk = Wk^T Wq (precomputed)
//   a     = softmax over the valid j (nei_j.mean() != 0), 0 for the masked ones
//   v_att = sum_j a_j (Wv x_j) = Wv (sum_j a_j x_j)  (no [rows*K][128] k|v tensor)
// The workgroup stages Wqk and Wv in LDS once ([row][68]: lane c reads row c with 16-B loads,
// conflict-free) and its four waves walk the rows; the vector being multiplied is broadcast
// from a 64-float LDS slot of the wave.
constexpr int WS = 68;
__device__ __forceinline__ float matvec_row(const float *w, const f4 *x4, int lane) {
    const f4 *wr = reinterpret_cast<const f4 *>(w + lane * WS);
    // four independent chains as two packed pairs: the (x, y) and (z, w) halves of the 16-B LDS
    // reads are register pairs already, so each step is two v_pk_fma_f32 with no operand moves
    // (four scalar chains made the compiler re-pair them, ~3x the VALU instructions)
    f2 p = {0.0f, 0.0f}, q = {0.0f, 0.0f};
#pragma unroll
    for (int o4 = 0; o4 < 16; ++o4) {
        const f4 a = wr[o4], b = x4[o4];
        p = __builtin_elementwise_fma(a.xy, b.xy, p);
        q = __builtin_elementwise_fma(a.zw, b.zw, q);
    }
    return (p.x + p.y) + (q.x + q.y);
}

// Weight staging: a 64x64 row-major matrix is 1024 float4 loads, four per thread.  Every load of
// the workgroup's share is issued before the first LDS store (stage_load for all matrices, then
// stage_store): interleaved, the compiler waits on each load before its store and the staging
// pays one memory round trip per 512 floats, ~10 us before the first row.
__device__ __forceinline__ void stage_load(const float *src, f4 (&v)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e4 = threadIdx.x + 256 * i;
        v[i] = *reinterpret_cast<const f4 *>(src + (e4 >> 4) * 64 + (e4 & 15) * 4);
    }
}

__device__ __forceinline__ void stage_store(float *dst, const f4 (&v)[4], bool transpose) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e4 = threadIdx.x + 256 * i, r = e4 >> 4, c = (e4 & 15) * 4;
        if (transpose) {
            dst[(c + 0) * WS + r] = v[i].x;
            dst[(c + 1) * WS + r] = v[i].y;
            dst[(c + 2) * WS + r] = v[i].z;
            dst[(c + 3) * WS + r] = v[i].w;
        } else {
            *reinterpret_cast<f4 *>(dst + r * WS + c) = v[i];
        }
    }
}

template <int KM>
__global__ void __launch_bounds__(256) attn_block_kernel(const float *__restrict__ eo, int lde,
                                                         const float *__restrict__ nei,
                                                         const float *__restrict__ Wn,
                                                         const float *__restrict__ bn,
                                                         const float *__restrict__ Wqk,
                                                         const float *__restrict__ Wv, float *__restrict__ out, int ldo,
                                                         int R, int K) {
    __shared__ f4 wq4[64 * WS / 4], wv4[64 * WS / 4];
    __shared__ f4 buf4[4][16];
    float *wqs = reinterpret_cast<float *>(wq4), *wvs = reinterpret_cast<float *>(wv4);
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    float *buf = reinterpret_cast<float *>(buf4[wv]);
    float wn[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) wn[i] = Wn[lane * 6 + i];
    const float bnl = bn[lane];
    const int nwaves = gridDim.x * 4;
    int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv);
    // software pipeline: the next row's e_o and neighbour rows load while this row is computed
    float e_n = 0.0f, nb_n[KM][6];
    auto fetch = [&](int rr) {
        e_n = eo[(size_t)rr * lde + lane];
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
#pragma unroll
            for (int i = 0; i < 6; ++i) nb_n[j][i] = nei[((size_t)rr * K + j) * 6 + i];
        }
    };
    if (r < R) fetch(r);
    // the first row loads above are in flight while the weights stage
    {
        f4 a[4], b[4];
        stage_load(Wqk, a);
        stage_load(Wv, b);
        stage_store(wqs, a, false);
        stage_store(wvs, b, false);
    }
    __syncthreads();
    for (; r < R; r += nwaves) {
        float nb[KM][6];
        const float ev = e_n;
#pragma unroll
        for (int j = 0; j < KM; ++j)
#pragma unroll
            for (int i = 0; i < 6; ++i) nb[j][i] = nb_n[j][i];
        if (r + nwaves < R) fetch(r + nwaves);
        buf[lane] = ev;
        const float qk = matvec_row(wqs, buf4[wv], lane);
        float x[KM], sc[KM];
        float mx = -INFINITY;
        unsigned valid = 0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            float h = bnl;
            float sum = nb[j][0];
#pragma unroll
            for (int i = 0; i < 6; ++i) h = fmaf(wn[i], nb[j][i], h);
#pragma unroll
            for (int i = 1; i < 6; ++i) sum += nb[j][i];
            x[j] = h > 0.0f ? h : 0.0f;
            sc[j] = wsum(x[j] * qk) / 8.0f;
            if (sum != 0.0f) {
                valid |= 1u << j;
                mx = sc[j] > mx ? sc[j] : mx;
            }
        }
        float den = 0.0f;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            const float e = (valid >> j & 1) ? expf(sc[j] - mx) : 0.0f;
            sc[j] = e;
            den += e;
        }
        float xb = 0.0f;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            const float a = (valid >> j & 1) ? sc[j] / den : 0.0f;
            xb = fmaf(a, x[j], xb);
        }
        buf[lane] = xb;
        out[(size_t)r * ldo + lane] = matvec_row(wvs, buf4[wv], lane);
    }
}

// ------------------------------------------------------------------------------ training attention
// Training form of the same attention (ATT/nets:186-210), one row per wave iteration, lane =
// feature, with every 64x64 projection done in-kernel from LDS-staged weights:
//   forward   q = Wq e_o, qk = Wk^T q, a = masked softmax(x_j . qk / 8), xb = sum a_j x_j,
//             v_att = Wv xb                              (saves q, qk, a, xb for the backward)
//   backward  dxb = Wv^T dv; da_j = x_j . dxb; S = sum a_j da_j; ds_j = a_j (da_j - S) / 8;
//             dqk = sum ds_j x_j; dx_j = (a_j dxb + ds_j qk) * (x_j > 0)   (-> dW_n via GEMM);
//             dq = Wk dqk; de_o = (dcat_o + Wq^T dq) * (e_o > 0)
// (k_j.q = x_j.(Wk^T q) and sum a_j v_j = Wv sum a_j x_j), so the [rows*K][128] k|v tensor and
// its three GEMMs (forward, dW_kv, dx) are never formed; the weight gradients dWv = dv^T xb,
// dWk = q^T dqk, dWq = dq^T e_o are GEMM products of the saved rows.
template <int KM>
__global__ void __launch_bounds__(256) attn_train_fwd_kernel(const float *__restrict__ eo, int lde,
                                                             const float *__restrict__ xn,
                                                             const float *__restrict__ nei,
                                                             const float *__restrict__ Wq, const float *__restrict__ Wk,
                                                             const float *__restrict__ Wv, float *__restrict__ q_out,
                                                             float *__restrict__ qk_out, float *__restrict__ alpha,
                                                             float *__restrict__ xb_out, float *__restrict__ vout,
                                                             int ldv, int R, int K) {
    __shared__ f4 w4[3][64 * WS / 4];
    __shared__ f4 buf4[4][16];
    float *wq = reinterpret_cast<float *>(w4[0]), *wkt = reinterpret_cast<float *>(w4[1]),
          *wv = reinterpret_cast<float *>(w4[2]);
    const int lane = threadIdx.x & 63, wvi = threadIdx.x >> 6;
    float *buf = reinterpret_cast<float *>(buf4[wvi]);
    const int nwaves = gridDim.x * 4;
    int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wvi);
    // software pipeline over the wave's rows: the next row's e_o / x_j / mask are loaded while
    // the current row is computed
    // (small K keeps the six raw features of each neighbour slot: summing them inside fetch would
    // wait for the prefetch right where it is issued)
    constexpr bool RAW = KM <= 8;
    float e_n = 0.0f, x_n[KM], m_n[KM], nb_n[RAW ? KM : 1][6];
    auto fetch = [&](int rr) {
        e_n = eo[(size_t)rr * lde + lane];
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            x_n[j] = xn[((size_t)rr * K + j) * 64 + lane];
            const float *nb = nei + ((size_t)rr * K + j) * 6;
            if constexpr (RAW) {
#pragma unroll
                for (int i = 0; i < 6; ++i) nb_n[j][i] = nb[i];
            } else {
                float sum = nb[0];
#pragma unroll
                for (int i = 1; i < 6; ++i) sum += nb[i];
                m_n[j] = sum;
            }
        }
    };
    auto mask_sum = [&](int j) {
        if constexpr (RAW) {
            float sum = nb_n[j][0];
#pragma unroll
            for (int i = 1; i < 6; ++i) sum += nb_n[j][i];
            return sum;
        } else {
            return m_n[j];
        }
    };
    if (r < R) fetch(r);
    // the first row loads above are in flight while the weights stage
    {
        f4 a[4], b[4], c[4];
        stage_load(Wq, a);
        stage_load(Wk, b);
        stage_load(Wv, c);
        stage_store(wq, a, false);
        stage_store(wkt, b, true);
        stage_store(wv, c, false);
    }
    __syncthreads();
    for (; r < R; r += nwaves) {
        // keep the weight rows in LDS (re-read per row) instead of 192 hoisted VGPRs: occupancy
        asm volatile("" ::: "memory");
        float x[KM], msum[KM];
        const float ev = e_n;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            x[j] = x_n[j];
            msum[j] = j < K ? mask_sum(j) : 0.0f;
        }
        if (r + nwaves < R) fetch(r + nwaves);
        buf[lane] = ev;
        const float qv = matvec_row(wq, buf4[wvi], lane);
        q_out[(size_t)r * 64 + lane] = qv;
        buf[lane] = qv;
        const float qk = matvec_row(wkt, buf4[wvi], lane);
        qk_out[(size_t)r * 64 + lane] = qk;
        float sc[KM];
        float mx = -INFINITY;
        unsigned valid = 0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            sc[j] = wsum(x[j] * qk) / 8.0f;
            if (msum[j] != 0.0f) {
                valid |= 1u << j;
                mx = sc[j] > mx ? sc[j] : mx;
            }
        }
        float den = 0.0f;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            const float e = (valid >> j & 1) ? expf(sc[j] - mx) : 0.0f;
            sc[j] = e;
            den += e;
        }
        float xb = 0.0f;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            const float a = (valid >> j & 1) ? sc[j] / den : 0.0f;
            xb = fmaf(a, x[j], xb);
            if (lane == j) alpha[(size_t)r * K + j] = a;
        }
        xb_out[(size_t)r * 64 + lane] = xb;
        buf[lane] = xb;
        vout[(size_t)r * ldv + lane] = matvec_row(wv, buf4[wvi], lane);
    }
}

template <int KM>
__global__ void __launch_bounds__(256) attn_train_bwd_kernel(const float *__restrict__ dv, int lddv,
                                                             const float *__restrict__ xn,
                                                             const float *__restrict__ alpha,
                                                             const float *__restrict__ qk_in,
                                                             const float *__restrict__ eo, int lde,
                                                             const float *__restrict__ dcat_o, int ldd,
                                                             const float *__restrict__ Wq, const float *__restrict__ Wk,
                                                             const float *__restrict__ Wv, float *__restrict__ dxn,
                                                             float *__restrict__ dqk_out, float *__restrict__ dq_out,
                                                             float *__restrict__ deo_out, int R, int K) {
    __shared__ f4 w4[3][64 * WS / 4];
    __shared__ f4 buf4[4][16];
    float *wvt = reinterpret_cast<float *>(w4[0]), *wk = reinterpret_cast<float *>(w4[1]),
          *wqt = reinterpret_cast<float *>(w4[2]);
    const int lane = threadIdx.x & 63, wvi = threadIdx.x >> 6;
    float *buf = reinterpret_cast<float *>(buf4[wvi]);
    const int nwaves = gridDim.x * 4;
    int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wvi);
    float dv_n = 0.0f, qk_n = 0.0f, e_n = 0.0f, dc_n = 0.0f, x_n[KM], a_n[KM];
    auto fetch = [&](int rr) {
        dv_n = dv[(size_t)rr * lddv + lane];
        qk_n = qk_in[(size_t)rr * 64 + lane];
        e_n = eo[(size_t)rr * lde + lane];
        dc_n = dcat_o[(size_t)rr * ldd + lane];
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            x_n[j] = xn[((size_t)rr * K + j) * 64 + lane];
            a_n[j] = alpha[(size_t)rr * K + j];
        }
    };
    if (r < R) fetch(r);
    // the first row loads above are in flight while the weights stage
    {
        f4 a[4], b[4], c[4];
        stage_load(Wv, a);
        stage_load(Wk, b);
        stage_load(Wq, c);
        stage_store(wvt, a, true);
        stage_store(wk, b, false);
        stage_store(wqt, c, true);
    }
    __syncthreads();
    for (; r < R; r += nwaves) {
        asm volatile("" ::: "memory");     // weight rows stay in LDS (see the forward)
        const float dvv = dv_n, qk = qk_n, e = e_n, dc = dc_n;
        float x[KM], a[KM], da[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            x[j] = x_n[j];
            a[j] = a_n[j];
        }
        if (r + nwaves < R) fetch(r + nwaves);
        buf[lane] = dvv;
        const float dxb = matvec_row(wvt, buf4[wvi], lane);
        float S = 0.0f;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            da[j] = wsum(x[j] * dxb);
            S += a[j] * da[j];
        }
        float dqk = 0.0f;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if (j >= K) continue;
            const float ds = a[j] * (da[j] - S) / 8.0f;
            const float g = a[j] * dxb + ds * qk;
            dxn[((size_t)r * K + j) * 64 + lane] = x[j] > 0.0f ? g : 0.0f;
            dqk = fmaf(ds, x[j], dqk);
        }
        dqk_out[(size_t)r * 64 + lane] = dqk;
        buf[lane] = dqk;
        const float dq = matvec_row(wk, buf4[wvi], lane);
        dq_out[(size_t)r * 64 + lane] = dq;
        buf[lane] = dq;
        const float t = matvec_row(wqt, buf4[wvi], lane);
        deo_out[(size_t)r * 64 + lane] = e > 0.0f ? dc + t : 0.0f;
    }
}

// ------------------------------------------------------------------------------ MFMA training attention
// The same forward / backward with the three 64x64 projections on v_mfma_f32_16x16x4_f32 (K <= 8).
// A workgroup takes 16 rows per block and wave w owns output features 16w..16w+15 of every
// projection.  The projections run transposed (Y^T = W X^T, the block's rows on the MFMA's n axis),
// so a result lands with lane & 15 = row and four consecutive features per lane (16-B stores), and
// the next projection reads it back from a [feature][row] LDS image as its B operand.  The weight
// fragments (16 floats per projection per lane) are loaded once per workgroup; the per-row form
// above re-reads each 16 KB weight matrix from LDS for every row (LDS-bound).  In step s, lane
// group h = lane >> 4 carries k index 16h + s, so fragments that are contiguous along k are four
// 16-B loads.  The softmax stage keeps the per-row form (wave w: rows 4w..4w+3, lane = feature);
// its neighbour rows are loaded at the start of the block so their latency hides under the
// projections.
#ifdef AAC_ATTN_STAMPS
// phase timestamps of workgroup 0 (probe builds only: tools/variant_lib.sh + tools/attn_enc_stamps.py)
__device__ unsigned long long g_attn_st[16];
#define ASTAMP(i)                                                                                        \
    do {                                                                                                  \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_attn_st[i] = __builtin_amdgcn_s_memtime();           \
    } while (0)
#else
#define ASTAMP(i) \
    do {          \
    } while (0)
#endif
constexpr int TS = 17;          // row stride of the [feature][16 rows] LDS images (conflict-free reads)
constexpr int QS = 68;          // row stride of the [16 rows][feature] LDS images (16-B aligned rows)

__device__ __forceinline__ void ld16(const float *p, float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f4 t = *reinterpret_cast<const f4 *>(p + 4 * i);
        v[4 * i] = t.x;
        v[4 * i + 1] = t.y;
        v[4 * i + 2] = t.z;
        v[4 * i + 3] = t.w;
    }
}

// weight fragments: 16 scalar loads (the parameter views of the flat buffers need not be 16-B aligned)
__device__ __forceinline__ void ld16w(const float *p, float (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = p[i];
}

// one 16x16 output tile over k = 64: a k-ordered f32 fma chain per element
__device__ __forceinline__ f4 mfma_k64(const float (&a)[16], const float (&b)[16]) {
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}

// B fragments from a [feature][row] LDS image
__device__ __forceinline__ void lds_bfrag(const float *img, int h, int n, float (&b)[16]) {
#pragma unroll
    for (int s = 0; s < 16; ++s) b[s] = img[(16 * h + s) * TS + n];
}

// ------------------------------------------------------- critic data gradient + actor output backward
// The actor step's critic data gradient df = (dh Wc) * (f > 0) and actor_out_bwd in one launch
// (aac_actor_dcomb_out_bwd): workgroup (sample block sb, agent n) computes the 16 x 128 tile
// df[b0 + i][n*128 + c] on MFMA (A = dh rows, B = the Wc column block staged in LDS one 64-row k chunk
// at a time, the next chunk in flight in registers), and never stores it: its only consumer is
//   da_j[b] = sum_c df[b][n*128 + c] W_enc_n[c][d0 + j]      (reduced over lanes, then waves in order)
//   dout_j  = da_j (1 - a_j^2),  dh_a = (dout_0 Wa[0] + dout_1 Wa[1]) * (h_a > 0)   for r = b*N + n
// (ATT/maddpg:421-425 backward; the critic weight gradients of the actor step are never used).  The
// k order of the MFMA chain is k = 64 c + 16 h + s (lane group h, step s): dh rows load as 16-B vectors.
constexpr int DAOB_WST = 144;          // LDS row stride of the staged Wc chunk (2 lanes per bank per read)
struct DaobArgs {
    const float *dh, *Wc, *f, *wenc, *X, *wa, *ha;
    float *dout, *dha;
    int ldw, din, d0, N, B;
};

// RT row tiles of 16 samples per workgroup: 2 when one tile per workgroup would put more workgroups
// than CUs in the launch (B = 1 024, N = 5: 320 -> 160; 64 CUs ran two of the 320 at once, one round
// more), each workgroup then streams its W_c slice once for 32 samples
template <int RT>
__global__ void __launch_bounds__(256) actor_dcomb_out_bwd_kernel(DaobArgs P, int hstart, HeadJob J) {
    if ((int)blockIdx.x >= hstart) {           // the riding critic-head job
        head_rows<false>(J, blockIdx.x - hstart);
        return;
    }
    __shared__ f4 sW4[64 * DAOB_WST / 4];
    __shared__ float sP[4][16 * RT][2];
    __shared__ float sD[16 * RT][2];
    __shared__ f4 sWa4[128];                    // the actor output layer's weights [2][256]
    float *sW = reinterpret_cast<float *>(sW4);
    if (threadIdx.x < 128) sWa4[threadIdx.x] = reinterpret_cast<const f4 *>(P.wa)[threadIdx.x];
    const int N = P.N;
    const int sb = blockIdx.x / N, n = blockIdx.x - sb * N;
    const int b0 = sb * 16 * RT;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, ln = lane & 15, h = lane >> 4;
    const float *wcol = P.Wc + (size_t)n * 128;       // column block of agent n
    // staging map: item e = t + 256 u (u < 8) -> chunk row e / 32, 4 columns (e % 32) * 4; two chunks
    // in flight (a ring of two register buffers, compile-time indexed: the chunk loop is unrolled)
    f4 pre[2][8];
    auto load_chunk = [&](int c, f4 (&dst)[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = t + 256 * u, row = e >> 5, c4 = (e & 31) * 4;
            dst[u] = *reinterpret_cast<const f4 *>(wcol + (size_t)(64 * c + row) * P.ldw + c4);
        }
    };
    auto store_chunk = [&](const f4 (&src)[8]) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = t + 256 * u, row = e >> 5, c4 = (e & 31) * 4;
            *reinterpret_cast<f4 *>(sW + row * DAOB_WST + c4) = src[u];
        }
    };
    load_chunk(0, pre[0]);
    load_chunk(1, pre[1]);
    // A fragments: the 16 consecutive dh values of row b0 + 16 rt + ln at k = 64 c + 16 h .. + 15 (all
    // chunks for one tile; with two tiles, chunk by chunk)
    int bl[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) bl[rt] = b0 + 16 * rt + ln < P.B ? b0 + 16 * rt + ln : P.B - 1;
    float a[RT == 1 ? 4 : 1][RT][16];
    if (RT == 1) {
#pragma unroll
        for (int c = 0; c < 4; ++c) ld16(P.dh + (size_t)bl[0] * 256 + 64 * c + 16 * h, a[RT == 1 ? c : 0][0]);
    }
    // the epilogue's operands, in flight across the MFMA chain: mask f, W_enc_n action columns, actions
    const int fo0 = 32 * w + ln, fo1 = fo0 + 16;            // this lane's two features of agent n
    float fm[RT][2][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = b0 + 16 * rt + 4 * h + j, bc = b < P.B ? b : P.B - 1;
            fm[rt][0][j] = P.f[(size_t)bc * P.ldw + n * 128 + fo0];
            fm[rt][1][j] = P.f[(size_t)bc * P.ldw + n * 128 + fo1];
        }
    const float *we = P.wenc + (size_t)n * 128 * P.din + P.d0;
    const float we00 = we[(size_t)fo0 * P.din], we01 = we[(size_t)fo0 * P.din + 1];
    const float we10 = we[(size_t)fo1 * P.din], we11 = we[(size_t)fo1 * P.din + 1];
    f4 acc0[RT], acc1[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc0[rt] = acc1[rt] = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (RT > 1) {
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) ld16(P.dh + (size_t)bl[rt] * 256 + 64 * c + 16 * h, a[0][rt]);
        }
        store_chunk(pre[c & 1]);
        __syncthreads();
        if (c + 2 < 4) load_chunk(c + 2, pre[c & 1]);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const float *rowp = sW + (16 * h + s) * DAOB_WST + 32 * w + ln;
            const float w0v = rowp[0], w1v = rowp[16];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const float av_ = a[RT == 1 ? c : 0][rt][s];
                acc0[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_, w0v, acc0[rt], 0, 0, 0);
                acc1[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av_, w1v, acc1[rt], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    // lane (ln, h): df[b0 + 16 rt + 4h + j][n*128 + fo] = acc[rt][j] (masked); da partials over the
    // lane's features
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float p0[4], p1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g0 = fm[rt][0][j] > 0.0f ? acc0[rt][j] : 0.0f;
            const float g1 = fm[rt][1][j] > 0.0f ? acc1[rt][j] : 0.0f;
            p0[j] = fmaf(g1, we10, g0 * we00);
            p1[j] = fmaf(g1, we11, g0 * we01);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {        // over the 16 lanes of the row group (features 0..15 of a tile)
            p0[j] = aacw::rsum16(p0[j]);
            p1[j] = aacw::rsum16(p1[j]);
        }
        if (ln == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sP[w][16 * rt + 4 * h + j][0] = p0[j];
                sP[w][16 * rt + 4 * h + j][1] = p1[j];
            }
        }
    }
    __syncthreads();
    if (t < 32 * RT) {   // the four waves' partials in wave order, then the tanh backward
        const int s = t >> 1, j = t & 1, b = b0 + s, bc = b < P.B ? b : P.B - 1;
        const float av = P.X[((size_t)bc * N + n) * P.din + P.d0 + j];
        const float da = ((sP[0][s][j] + sP[1][s][j]) + sP[2][s][j]) + sP[3][s][j];
        const float o = da * (1.0f - av * av);
        sD[s][j] = o;
        if (b < P.B) P.dout[((size_t)b * N + n) * 2 + j] = o;
    }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {   // dh_a rows: thread (row s, 16 columns)
        const int s = 16 * rt + (t >> 4), c0 = (t & 15) * 16, b = b0 + s;
        if (b < P.B) {
            const size_t r = (size_t)b * N + n;
            const float o0 = sD[s][0], o1 = sD[s][1];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = c0 + 4 * q;
                const f4 hv = *reinterpret_cast<const f4 *>(P.ha + r * 256 + c);
                const f4 w0 = sWa4[c >> 2];
                const f4 w1 = sWa4[64 + (c >> 2)];
                f4 v;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float x = o0 * w0[u] + o1 * w1[u];
                    v[u] = hv[u] > 0.0f ? x : 0.0f;
                }
                *reinterpret_cast<f4 *>(P.dha + r * 256 + c) = v;
            }
        }
    }
}

// the six neighbour features of slot `lane` of row `row` (lanes >= K hold zeros), for the mask sum
__device__ __forceinline__ void ld_nei6(const float *nei, int row, int K, int lane, float (&nb)[6]) {
    if (lane < K) {
        const f2 *p = reinterpret_cast<const f2 *>(nei + ((size_t)row * K + lane) * 6);
        const f2 a = p[0], b = p[1], c = p[2];
        nb[0] = a.x;
        nb[1] = a.y;
        nb[2] = b.x;
        nb[3] = b.y;
        nb[4] = c.x;
        nb[5] = c.y;
    } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) nb[i] = 0.0f;
    }
}

template <int KM>
__global__ void __launch_bounds__(256) attn_mfma_fwd_kernel(const float *__restrict__ eo, int lde,
                                                            const float *__restrict__ xn,
                                                            const float *__restrict__ nei,
                                                            const float *__restrict__ Wq, const float *__restrict__ Wk,
                                                            const float *__restrict__ Wv, float *__restrict__ q_out,
                                                            float *__restrict__ qk_out, float *__restrict__ alpha,
                                                            float *__restrict__ xb_out, float *__restrict__ vout,
                                                            int ldv, int R, int K) {
    __shared__ float sQ[64 * TS], sX[64 * TS];
    __shared__ f4 sQK4[16 * QS / 4];
    float *sQK = reinterpret_cast<float *>(sQK4);
    ASTAMP(0);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, h = lane >> 4;
    const int fo = 16 * w + 4 * h;                   // this lane's four output features
    const int nblk = (R + 15) / 16;
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int r0 = blk * 16, r = r0 + n;
        const bool rin = r < R;
        const int rc = rin ? r : R - 1;
        // loads in the order the stages consume them (the wave's load counter retires in order):
        // e_o rows and Wq fragments, then Wk (stage 2), the softmax stage's rows, Wv (stage 3).
        // Out-of-range rows / slots read a clamped in-range address; a row >= R only feeds its own
        // (discarded) MFMA column, and slots j >= K are masked where they are consumed (a select
        // here would wait for each load right after issuing it).
        // A fragments: q^T = Wq e^T (A = Wq[o][k]), qk^T = Wk^T q^T (A = Wk[o][i] at [i][o]), v^T = Wv xb^T
        float b[16], aq[16], ak[16], av[16];
        ld16(eo + (size_t)rc * lde + 16 * h, b);
        ld16w(Wq + (16 * w + n) * 64 + 16 * h, aq);
#pragma unroll
        for (int s = 0; s < 16; ++s) ak[s] = Wk[(16 * h + s) * 64 + 16 * w + n];
        float x[4][KM], nb[4][6];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 4 * w + i;
            const bool ok = row < R;
            const int rr = ok ? row : R - 1;
#pragma unroll
            for (int j = 0; j < KM; ++j) x[i][j] = xn[((size_t)rr * K + (j < K ? j : K - 1)) * 64 + lane];
            const f2 *pn = reinterpret_cast<const f2 *>(nei + ((size_t)rr * K + (lane < K ? lane : K - 1)) * 6);
            const f2 n0 = pn[0], n1 = pn[1], n2 = pn[2];
            nb[i][0] = n0.x;
            nb[i][1] = n0.y;
            nb[i][2] = n1.x;
            nb[i][3] = n1.y;
            nb[i][4] = n2.x;
            nb[i][5] = n2.y;
        }
        ld16w(Wv + (16 * w + n) * 64 + 16 * h, av);
        // q^T = Wq e_o^T
        f4 acc = mfma_k64(aq, b);
        ASTAMP(1);
        if (rin) *reinterpret_cast<f4 *>(q_out + (size_t)r * 64 + fo) = acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) sQ[(fo + j) * TS + n] = acc[j];
        __syncthreads();
        // qk^T = Wk^T q^T
        ASTAMP(2);
        lds_bfrag(sQ, h, n, b);
        acc = mfma_k64(ak, b);
        if (rin) *reinterpret_cast<f4 *>(qk_out + (size_t)r * 64 + fo) = acc;
        *reinterpret_cast<f4 *>(sQK + n * QS + fo) = acc;
        __syncthreads();
        ASTAMP(3);
        // masked softmax and xb = sum_j a_j x_j for the wave's four rows at once, lane = feature: the
        // 4 KM scores are one batched DPP reduction, and slots j >= K (zero x, zero mask) drop out
        // arithmetically, so the stage has no branches on K
        {
            float p[4 * KM], qk4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) qk4[i] = sQK[(4 * w + i) * QS + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    x[i][j] = j < K ? x[i][j] : 0.0f;
                    p[i * KM + j] = x[i][j] * qk4[i];
                }
            wsum_n(p);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = 4 * w + i, row = r0 + rl;
                float ms = nb[i][0];
#pragma unroll
                for (int t = 1; t < 6; ++t) ms += nb[i][t];
                float sc[KM];
                float mx = -INFINITY;
                unsigned valid = 0;
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    sc[j] = p[i * KM + j] / 8.0f;
                    const bool v =
                        j < K && __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ms), j)) != 0.0f;
                    valid |= (v ? 1u : 0u) << j;
                    mx = (v && sc[j] > mx) ? sc[j] : mx;
                }
                float den = 0.0f;
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    const float e = (valid >> j & 1) ? __expf(sc[j] - mx) : 0.0f;
                    sc[j] = e;
                    den += e;
                }
                float xb = 0.0f, al = 0.0f;
                const float inv = 1.0f / den;
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    const float a = (valid >> j & 1) ? sc[j] * inv : 0.0f;
                    xb = fmaf(a, x[i][j], xb);
                    al = lane == j ? a : al;
                }
                if (row < R) {
                    if (lane < K) alpha[(size_t)row * K + lane] = al;
                    xb_out[(size_t)row * 64 + lane] = xb;
                }
                sX[lane * TS + rl] = xb;
            }
        }
        __syncthreads();
        ASTAMP(4);
        // v^T = Wv xb^T
        lds_bfrag(sX, h, n, b);
        acc = mfma_k64(av, b);
        if (rin) *reinterpret_cast<f4 *>(vout + (size_t)r * ldv + fo) = acc;
        ASTAMP(5);
    }
}

template <int KM>
__global__ void __launch_bounds__(256, KM > 4 ? 2 : 3) attn_mfma_bwd_kernel(const float *__restrict__ dv, int lddv,
                                                            const float *__restrict__ xn,
                                                            const float *__restrict__ alpha,
                                                            const float *__restrict__ qk_in,
                                                            const float *__restrict__ eo, int lde,
                                                            const float *__restrict__ dcat_o, int ldd,
                                                            const float *__restrict__ Wq, const float *__restrict__ Wk,
                                                            const float *__restrict__ Wv, float *__restrict__ dxn,
                                                            float *__restrict__ dqk_out, float *__restrict__ dq_out,
                                                            float *__restrict__ deo_out, int R, int K,
                                                            const float *__restrict__ nei, float *__restrict__ pwn) {
    __shared__ float sA[64 * TS], sB[64 * TS];
    __shared__ f4 sD4[16 * QS / 4];
    __shared__ float sN[16 * KM * 6];         // pwn: the block's neighbour rows
    __shared__ float sW[4 * 7 * 64];          // pwn: the waves' partial dWn rows
    float *sD = reinterpret_cast<float *>(sD4);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, h = lane >> 4;
    const int fo = 16 * w + 4 * h;
    const int nblk = (R + 15) / 16;
    // pwn != NULL: the neighbour encoder's weight gradient dWn = sum_(r, j) dx_j^T [nei_j | 1] (64 x 7)
    // accumulated by this workgroup (lane = feature), written as one partial row of pwn
    // ([gridDim][64 * 6 + 64]: weights f * 6 + c, then the bias); dxn may then be NULL.  It replaces
    // the 20 480-row GEMM product whose chain was the longest of its launch.
    float gw[7] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int r0 = blk * 16, r = r0 + n;
        const bool rin = r < R;
        const int rc = rin ? r : R - 1;
        // loads in consumption order (see the forward): dv rows + Wv^T, the softmax-backward rows,
        // Wk, Wq^T, and the e_o / dcat_o rows of the last stage
        // dxb^T = Wv^T dv^T (A = Wv[o][i] at [i][o]), dq^T = Wk dqk^T (A = Wk[o][i]), t^T = Wq^T dq^T
        float b[16], avt[16], ak[16], aqt[16];
        ld16(dv + (size_t)rc * lddv + 16 * h, b);
#pragma unroll
        for (int s = 0; s < 16; ++s) avt[s] = Wv[(16 * h + s) * 64 + 16 * w + n];
        float x[4][KM], al[4][KM], qkv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 4 * w + i;
            const int rr = row < R ? row : R - 1;
            qkv[i] = qk_in[(size_t)rr * 64 + lane];
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                const int jj = j < K ? j : K - 1;
                x[i][j] = xn[((size_t)rr * K + jj) * 64 + lane];
                al[i][j] = alpha[(size_t)rr * K + jj];
            }
        }
        ld16w(Wk + (16 * w + n) * 64 + 16 * h, ak);
#pragma unroll
        for (int s = 0; s < 16; ++s) aqt[s] = Wq[(16 * h + s) * 64 + 16 * w + n];
        const f4 e = *reinterpret_cast<const f4 *>(eo + (size_t)rc * lde + fo);
        const f4 dc = *reinterpret_cast<const f4 *>(dcat_o + (size_t)rc * ldd + fo);
        if (pwn) {      // the block's neighbour rows (slots j >= K zero)
            for (int i = threadIdx.x; i < 16 * KM * 6; i += 256) {
                const int rl = i / (KM * 6), jc = i - rl * KM * 6, j = jc / 6;
                const int row = r0 + rl;
                sN[i] = (row < R && j < K) ? nei[((size_t)row * K + j) * 6 + (jc - j * 6)] : 0.0f;
            }
        }
        // dxb^T = Wv^T dv^T
        f4 acc = mfma_k64(avt, b);
        *reinterpret_cast<f4 *>(sD + n * QS + fo) = acc;
        __syncthreads();
        // softmax backward for the wave's four rows at once, lane = feature (batched da sums; slots
        // j >= K get zero alpha, so they add nothing)
        {
            float p[4 * KM], dxb4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) dxb4[i] = sD[(4 * w + i) * QS + lane];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    al[i][j] = j < K ? al[i][j] : 0.0f;
                    p[i * KM + j] = x[i][j] * dxb4[i];
                }
            wsum_n(p);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int rl = 4 * w + i, row = r0 + rl;
                const float dxb = dxb4[i], qk = qkv[i];
                float S = 0.0f;
#pragma unroll
                for (int j = 0; j < KM; ++j) S += al[i][j] * p[i * KM + j];
                float dqk = 0.0f;
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    const float ds = al[i][j] * (p[i * KM + j] - S) / 8.0f;
                    const float g = al[i][j] * dxb + ds * qk;
                    const float gx = x[i][j] > 0.0f ? g : 0.0f;
                    if (dxn && j < K && row < R) dxn[((size_t)row * K + j) * 64 + lane] = gx;
                    if (pwn && j < K && row < R) {
                        const float *nr = sN + (rl * KM + j) * 6;
#pragma unroll
                        for (int c = 0; c < 6; ++c) gw[c] = fmaf(gx, nr[c], gw[c]);
                        gw[6] += gx;
                    }
                    dqk = fmaf(ds, x[i][j], dqk);
                }
                if (row < R) dqk_out[(size_t)row * 64 + lane] = dqk;
                sA[lane * TS + rl] = dqk;
            }
        }
        __syncthreads();
        // dq^T = Wk dqk^T
        lds_bfrag(sA, h, n, b);
        acc = mfma_k64(ak, b);
        if (rin) *reinterpret_cast<f4 *>(dq_out + (size_t)r * 64 + fo) = acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) sB[(fo + j) * TS + n] = acc[j];
        __syncthreads();
        // de_o = (dcat_o + Wq^T dq) * (e_o > 0)
        lds_bfrag(sB, h, n, b);
        acc = mfma_k64(aqt, b);
        if (rin) {
            f4 o;
            o.x = e.x > 0.0f ? dc.x + acc.x : 0.0f;
            o.y = e.y > 0.0f ? dc.y + acc.y : 0.0f;
            o.z = e.z > 0.0f ? dc.z + acc.z : 0.0f;
            o.w = e.w > 0.0f ? dc.w + acc.w : 0.0f;
            *reinterpret_cast<f4 *>(deo_out + (size_t)r * 64 + fo) = o;
        }
    }
    if (pwn) {          // the four waves' partials, summed in wave order
#pragma unroll
        for (int c = 0; c < 7; ++c) sW[(w * 7 + c) * 64 + lane] = gw[c];
        __syncthreads();
        if (w == 0) {
            float *o = pwn + (size_t)blockIdx.x * 448;
#pragma unroll
            for (int c = 0; c < 7; ++c) {
                const float v = ((sW[c * 64 + lane] + sW[(7 + c) * 64 + lane]) + sW[(14 + c) * 64 + lane]) +
                                sW[(21 + c) * 64 + lane];
                if (c < 6) o[lane * 6 + c] = v;
                else o[384 + lane] = v;
            }
        }
    }
}

// Inference attention block (aac_attn_block, K <= 4) on the same transposed 16-row MFMA scheme:
// qk^T = Wqk e_o^T, then x_j = relu(Wn nei_j + bn), the masked softmax and xb per row (lane =
// feature, the wave's four rows at once), then v^T = Wv xb^T.  The neighbour rows (6 floats per
// slot, the same in every lane) are loaded at the start of the block.
template <int KM>
__global__ void __launch_bounds__(256) attn_mfma_block_kernel(const float *__restrict__ eo, int lde,
                                                              const float *__restrict__ nei,
                                                              const float *__restrict__ Wn,
                                                              const float *__restrict__ bn,
                                                              const float *__restrict__ Wqk,
                                                              const float *__restrict__ Wv, float *__restrict__ out,
                                                              int ldo, int R, int K) {
    __shared__ float sX[64 * TS];
    __shared__ f4 sQK4[16 * QS / 4];
    float *sQK = reinterpret_cast<float *>(sQK4);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, h = lane >> 4;
    const int fo = 16 * w + 4 * h;
    float wn[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) wn[t] = Wn[lane * 6 + t];
    const float bnl = bn[lane];
    const int nblk = (R + 15) / 16;
    for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int r0 = blk * 16, r = r0 + n;
        const bool rin = r < R;
        const int rc = rin ? r : R - 1;
        // loads in consumption order: e_o rows + Wqk, the neighbour rows, Wv (clamped addresses:
        // rows >= R only feed their own discarded column, slots j >= K are masked at use)
        float b[16], aq[16], av[16];
        ld16(eo + (size_t)rc * lde + 16 * h, b);
        ld16w(Wqk + (16 * w + n) * 64 + 16 * h, aq);
        float nb[4][KM][6];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = r0 + 4 * w + i, rr = row < R ? row : R - 1;
#pragma unroll
            for (int j = 0; j < KM; ++j)
#pragma unroll
                for (int t = 0; t < 6; ++t) nb[i][j][t] = nei[((size_t)rr * K + (j < K ? j : K - 1)) * 6 + t];
        }
        ld16w(Wv + (16 * w + n) * 64 + 16 * h, av);
        // qk^T = Wqk e_o^T
        f4 acc = mfma_k64(aq, b);
        *reinterpret_cast<f4 *>(sQK + n * QS + fo) = acc;
        __syncthreads();
        {
            float p[4 * KM], x[4][KM];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float qk = sQK[(4 * w + i) * QS + lane];
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    float hh = bnl;
#pragma unroll
                    for (int t = 0; t < 6; ++t) hh = fmaf(wn[t], nb[i][j][t], hh);
                    x[i][j] = (j < K && hh > 0.0f) ? hh : 0.0f;
                    p[i * KM + j] = x[i][j] * qk;
                }
            }
            wsum_n(p);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float sc[KM];
                float mx = -INFINITY;
                unsigned valid = 0;
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    float sum = nb[i][j][0];
#pragma unroll
                    for (int t = 1; t < 6; ++t) sum += nb[i][j][t];
                    sc[j] = p[i * KM + j] / 8.0f;
                    const bool v = j < K && sum != 0.0f;
                    valid |= (v ? 1u : 0u) << j;
                    mx = (v && sc[j] > mx) ? sc[j] : mx;
                }
                float den = 0.0f;
#pragma unroll
                for (int j = 0; j < KM; ++j) {
                    const float e = (valid >> j & 1) ? __expf(sc[j] - mx) : 0.0f;
                    sc[j] = e;
                    den += e;
                }
                const float inv = 1.0f / den;
                float xb = 0.0f;
#pragma unroll
                for (int j = 0; j < KM; ++j) xb = fmaf((valid >> j & 1) ? sc[j] * inv : 0.0f, x[i][j], xb);
                sX[lane * TS + 4 * w + i] = xb;
            }
        }
        __syncthreads();
        // v^T = Wv xb^T
        lds_bfrag(sX, h, n, b);
        acc = mfma_k64(av, b);
        if (rin) *reinterpret_cast<f4 *>(out + (size_t)r * ldo + fo) = acc;
    }
}

// ------------------------------------------------- encoders fused into the attention (aac_attn_enc_fwd)
// The encoder weights and a block's input rows are small contiguous arrays: the workgroup stages them
// in LDS with coalesced loads (rows zero-padded to a multiple of 4), and the MFMA fragments come from
// there.  (Fragment loads straight from global memory -- 16 rows x 4 scattered floats per lane and
// step -- made the launch bound on vector-memory instructions, not on the arithmetic.)
constexpr int ENC_DMAX = 40;                 // own rows / critic-input rows up to 40 floats (K <= 8)
// LDS row strides: the fragment reads cover k < round4(K); an odd stride spreads the 16 rows of a
// read over distinct banks (a multiple of 8 put them on 4 banks or fewer)
__device__ __forceinline__ int enc_stride(int k) { return ((k + 3) & ~3) + 1; }
constexpr int ENC_SMAX = ENC_DMAX + 1, ENC_SG = 21, ENC_SN = 9;       // own / critic rows, radar, neighbour
constexpr int ENC_W_FLOATS = 64 * ENC_SMAX + 64 * ENC_SG + 64 * ENC_SN + 192;   // Wo | Wg | Wn | bo bg bn
constexpr int ENC_OFF_WG = 64 * ENC_SMAX, ENC_OFF_WN = ENC_OFF_WG + 64 * ENC_SG, ENC_OFF_B = ENC_OFF_WN + 64 * ENC_SN;

// Staging into LDS rows of stride Kp >= K (zero-padded), in two halves so that every load of several
// blocks is in flight before the first LDS store (a loop that stored each value right after loading
// it waited a full memory latency per iteration).  No integer divisions on the item index: a
// contiguous [rows][K] weight matrix goes linearly (row = item * ceil(2^32 / K) >> 32, exact for
// items < 2^16 and K <= 64), a block of 16 strided input rows as 16 threads per row.  Out-of-range
// items load src[0].
template <int MAXI>
struct Stage {
    float v[MAXI];
};

__device__ __forceinline__ uint64_t div_magic(int K) { return ((1ull << 32) + (uint64_t)K - 1) / (uint64_t)K; }

template <int MAXI>
__device__ __forceinline__ void stage_w_load(Stage<MAXI> &st, const float *__restrict__ src, int n) {
#pragma unroll
    for (int u = 0; u < MAXI; ++u) {
        const int g = threadIdx.x + 256 * u;
        const float v = src[g < n ? g : 0];
        st.v[u] = v;
    }
}

// store the linear items of a [rows][K] matrix as LDS rows of stride Kp, and zero the pad columns
template <int MAXI>
__device__ __forceinline__ void stage_w_store(const Stage<MAXI> &st, float *dst, int K, int Kp, int rows) {
    const uint64_t m = div_magic(K);
    const int n = rows * K;
#pragma unroll
    for (int u = 0; u < MAXI; ++u) {
        const int g = threadIdx.x + 256 * u;
        const int r = (int)(((uint64_t)g * m) >> 32);
        if (g < n) dst[r * Kp + (g - r * K)] = st.v[u];
    }
    for (int i = threadIdx.x; i < rows * 4; i += 256) {
        const int r = i >> 2, c = i & 3;
        if (K + c < Kp) dst[r * Kp + K + c] = 0.0f;
    }
}

// 16 input rows (global row stride ld, K used columns) -> LDS rows of stride Kp; rows >= nrows zero
template <int MAXI>
__device__ __forceinline__ void stage_r_load(Stage<MAXI> &st, const float *__restrict__ src, int ld, int K, int nrows) {
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
    for (int u = 0; u < MAXI; ++u) {
        const int k = c + 16 * u;
        const bool ok = k < K && r < nrows;
        const float v = src[ok ? (size_t)r * ld + k : 0];
        st.v[u] = ok ? v : 0.0f;
    }
}

template <int MAXI>
__device__ __forceinline__ void stage_r_store(const Stage<MAXI> &st, float *dst, int Kp) {
    const int r = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
    for (int u = 0; u < MAXI; ++u) {
        const int k = c + 16 * u;
        if (k < Kp) dst[r * Kp + k] = st.v[u];
    }
}

// 16 x 16 tile of e^T = W x^T over K inputs from LDS (k = 4 s + h; A = W[f0 + n][k], B = x[row n][k],
// W rows of stride Kw, x rows of stride Kx, both zero-padded past K); lane (n, h) gets the
// pre-activations of features f0 + 4 h .. + 3 of row n.  All KS steps run: the steps past ceil(K / 4)
// read zeros for both operands (a select, not a branch: branches around every LDS read serialised
// their latencies) and add exact zeros, so the result is that of the ceil(K / 4)-step chain.
template <int KS>
__device__ __forceinline__ f4 enc_lds(const float *sW, int Kw, const float *sx, int Kx, int K, int f0, int n, int h) {
    float a[KS], b[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const bool on = 4 * s < K;
        const int k = on ? 4 * s + h : h;
        const float wa = sW[(f0 + n) * Kw + k], xb = sx[n * Kx + k];
        a[s] = on ? wa : 0.0f;
        b[s] = on ? xb : 0.0f;
    }
    f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
    return acc;
}

__device__ __forceinline__ f4 relu_bias4(f4 v, const float *b) {
    f4 r;
    r.x = v.x + b[0];
    r.y = v.y + b[1];
    r.z = v.z + b[2];
    r.w = v.w + b[3];
    r.x = r.x > 0.0f ? r.x : 0.0f;
    r.y = r.y > 0.0f ? r.y : 0.0f;
    r.z = r.z > 0.0f ? r.z : 0.0f;
    r.w = r.w > 0.0f ? r.w : 0.0f;
    return r;
}

// the riding job: the critic encoders of row blocks jb, jb + rjobs, ... of one agent (16 rows each:
// eight 16-feature tiles, two per wave), W_n and b_n staged in LDS once per job, the next block's
// input rows (and its folded actor outputs) loaded while the current block is multiplied.
// KSO = the encoder's k steps (ceil(Din / 4) <= KSO)
template <int KSO>
__device__ void critic_enc_rows(const aac_attn_enc_args &A, int job, int rjobs, float *smem) {
    const int nrb = (A.c_rows + 15) / 16;
    const int ag = job / rjobs, jb = job - ag * rjobs;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, h = lane >> 4;
    const int Din = A.c_din, Dp = enc_stride(Din);
    float *sW = smem, *sx = smem + 128 * ENC_SMAX, *sb = sx + 16 * ENC_SMAX;
    Stage<128 * 4 * KSO / 256> gw;
    Stage<(ENC_SMAX + 15) / 16> gx;
    stage_w_load(gw, A.cW + (size_t)ag * 128 * Din, 128 * Din);
    // the 16 input rows of block rb into gx; with the actor's output layer folded in, lanes (row rr,
    // c) take columns 16 c .. 16 c + 15 of the 256-wide ha row, a 16-lane butterfly sums them (every
    // lane of the row gets the same total), and the lanes that stage the two action columns put
    // tanh(. + b) in their staged values
    auto load_x = [&](int rb) {
        const int r0 = rb * 16;
        stage_r_load(gx, A.cx + (size_t)r0 * A.cx_ld + (size_t)ag * Din, A.cx_ld, Din, A.c_rows - r0);
        if (A.o_h) {
            const int rr = threadIdx.x >> 4, c = threadIdx.x & 15, r = r0 + rr;
            const bool rok = r < A.c_rows;
            const f4 *hp = reinterpret_cast<const f4 *>(A.o_h + ((size_t)(rok ? r : 0) * A.c_n + ag) * 256 + 16 * c);
            const f4 *w0 = reinterpret_cast<const f4 *>(A.o_w + 16 * c), *w1 = reinterpret_cast<const f4 *>(A.o_w + 256 + 16 * c);
            f4 hv[4], wa[4], wb[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                hv[q] = hp[q];
                wa[q] = w0[q];
                wb[q] = w1[q];
            }
            const float b0 = A.o_b[0], b1 = A.o_b[1];
            float p0 = 0.0f, p1 = 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    p0 = fmaf(hv[q][t], wa[q][t], p0);
                    p1 = fmaf(hv[q][t], wb[q][t], p1);
                }
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) {
                p0 += __shfl_xor(p0, o, 16);
                p1 += __shfl_xor(p1, o, 16);
            }
            const float a0 = tanhf(p0 + b0), a1 = tanhf(p1 + b1);
            const int d0 = A.o_d0;
#pragma unroll
            for (int u = 0; u < (ENC_SMAX + 15) / 16; ++u) {
                const int k = c + 16 * u;
                if (rok && k == d0) gx.v[u] = a0;
                if (rok && k == d0 + 1) gx.v[u] = a1;
            }
            if (rok && c == 0) {
                float *xo = A.o_x + (size_t)r * A.cx_ld + (size_t)ag * Din + d0;
                xo[0] = a0;
                xo[1] = a1;
            }
        }
    };
    const float bias = A.cb[ag * 128 + (threadIdx.x & 127)];
    load_x(jb);
    stage_w_store(gw, sW, Din, Dp, 128);
    if (threadIdx.x < 128) sb[threadIdx.x] = bias;
    for (int rb = jb; rb < nrb; rb += rjobs) {
        stage_r_store(gx, sx, Dp);
        __syncthreads();
        if (rb + rjobs < nrb) load_x(rb + rjobs);        // in flight under this block's products
        const int r = rb * 16 + n;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int f0 = 32 * w + 16 * t;
            const f4 v = relu_bias4(enc_lds<KSO>(sW, Dp, sx, Dp, Din, f0, n, h), sb + f0 + 4 * h);
            if (r < A.c_rows) *reinterpret_cast<f4 *>(A.cf + (size_t)r * A.c_n * 128 + ag * 128 + f0 + 4 * h) = v;
        }
        __syncthreads();       // every wave is done with sx before the next block's rows land there
    }
}

// up to two independent sets (e.g. the target actor's inference attention and a training one) in one
// launch; set s owns workgroups [start[s], start[s] + nattn[s]) for its attention blocks and the next
// nride[s] for its riding critic-encoder jobs
struct AttnEncBatch {
    aac_attn_enc_args a[2];
    int start[2], nattn[2], nride[2], rjobs[2];     // rjobs: riding jobs per agent
    int nset;
    int hstart;               // workgroups >= hstart run the critic-head job (INT_MAX: none)
    HeadJob hj;
};

// LDS (floats): encoder weights | region U (the block's staged input rows, later sQ) | sE (later sX) |
// sP (the four waves' partial scores [wave][row][slot])
template <int KM>
struct AttnEncLds {
    static constexpr int NS = 8 * KM + 1;        // staged neighbour rows: slot j at j * 8, odd row stride
    static constexpr int IN = 16 * ENC_SMAX + 16 * ENC_SG + 16 * NS;
    static constexpr int U = IN > 64 * TS ? IN : 64 * TS;
    static constexpr int OFF_U = ENC_W_FLOATS, OFF_E = OFF_U + ((U + 3) & ~3), OFF_P = OFF_E + ((64 * TS + 3) & ~3);
    static constexpr int TOTAL = OFF_P + 4 * 16 * KM;
};
static_assert(AttnEncLds<4>::TOTAL >= 128 * ENC_SMAX + 16 * ENC_SMAX + 128, "ride job fits in the attention's LDS");

// KM: neighbour slots (>= K); KSO: k steps of the own-row and critic-row encoders (6: <= 24 inputs, 10:
// <= 40).  3 waves per SIMD at the config-3 shapes (the LDS allows 5; 4 spilled and measured slower)
template <int KM, int KSO>
__global__ void __launch_bounds__(256, (KM > 4 || KSO > 6) ? 2 : 3) attn_enc_kernel(AttnEncBatch P) {
    using L = AttnEncLds<KM>;
    __shared__ f4 smem4[L::TOTAL / 4];
    float *smem = reinterpret_cast<float *>(smem4);
    if ((int)blockIdx.x >= P.hstart) {       // the riding critic-head job (copied by value: static indices)
        const HeadJob J = P.hj;
        head_rows<false>(J, blockIdx.x - P.hstart);
        return;
    }
    const int s = (P.nset > 1 && (int)blockIdx.x >= P.start[1]) ? 1 : 0;
    const aac_attn_enc_args &A = P.a[s];
    const int nattn = P.nattn[s];
    const int lb = blockIdx.x - P.start[s];
    if (lb >= nattn) {
        critic_enc_rows<KSO>(A, lb - nattn, P.rjobs[s], smem);
        return;
    }
    ASTAMP(0);
    const bool train = A.xn != nullptr;       // uniform: inference leaves the backward's operands NULL
    float *sWo = smem, *sWg = smem + ENC_OFF_WG, *sWn = smem + ENC_OFF_WN, *sB = smem + ENC_OFF_B;
    float *sOwn = smem + L::OFF_U, *sRad = sOwn + 16 * ENC_SMAX, *sNei = sRad + 16 * ENC_SG;
    float *sQ = smem + L::OFF_U;                                // aliases the staged rows (dead by then)
    float *sE = smem + L::OFF_E, *sX = sE;                      // sE dead after the q stage
    float *sP = smem + L::OFF_P;                                // partial scores [wave][row][slot]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = lane & 15, h = lane >> 4;
    const int fo = 16 * w + 4 * h;
    const int R = A.R, K = A.K, Do = A.d_own, Dop = enc_stride(Do);
    constexpr int NS = L::NS, NNEI = KM * 8 / 16;
    // the block's input rows (own, radar: rows of the LDS images; neighbours: slot j of row r at
    // r * NS + 8 j), all loads in flight before the stores
    struct In {
        Stage<(ENC_SMAX + 15) / 16> o;
        Stage<(ENC_SG + 15) / 16> g;
        float nv[NNEI];
    } in;
    auto load_in = [&](int r0) {
        stage_r_load(in.o, A.own + (size_t)r0 * A.ld_own, A.ld_own, Do, R - r0);
        stage_r_load(in.g, A.radar + (size_t)r0 * A.ld_radar, A.ld_radar, 18, R - r0);
        // neighbour rows: 16 threads per row over its KM * 8 (slot, k) items
        const int row = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
        for (int u = 0; u < NNEI; ++u) {
            const int e = c + 16 * u, j = e >> 3, k = e & 7;
            const bool ok = k < 6 && j < K && r0 + row < R;
            const float v = A.nei[ok ? ((size_t)(r0 + row) * K + j) * 6 + k : 0];
            in.nv[u] = ok ? v : 0.0f;
        }
    };
    auto store_in = [&]() {
        stage_r_store(in.o, sOwn, Dop);
        stage_r_store(in.g, sRad, ENC_SG);
        const int row = threadIdx.x >> 4, c = threadIdx.x & 15;
#pragma unroll
        for (int u = 0; u < NNEI; ++u) sNei[row * NS + c + 16 * u] = in.nv[u];
    };
    // the encoder weights, once per workgroup, loaded together with the first block's rows
    {
        Stage<64 * ENC_DMAX / 256> go;
        Stage<(64 * 18 + 255) / 256> gg;
        Stage<(64 * 6 + 255) / 256> gn;
        stage_w_load(go, A.Wo, 64 * Do);
        stage_w_load(gg, A.Wg, 64 * 18);
        stage_w_load(gn, A.Wn, 64 * 6);
        const int k = threadIdx.x;
        const float bias = k < 64 ? A.bo[k] : (k < 128 ? A.bg[k - 64] : A.bn[k < 192 ? k - 128 : 0]);
        load_in(lb * 16);
        stage_w_store(go, sWo, Do, Dop, 64);
        stage_w_store(gg, sWg, 18, ENC_SG, 64);
        stage_w_store(gn, sWn, 6, ENC_SN, 64);
        if (k < 192) sB[k] = bias;
    }
    const int nblk = (R + 15) / 16;
    for (int blk = lb; blk < nblk; blk += nattn) {
        const int r0 = blk * 16, r = r0 + n;
        const bool rin = r < R;
        // (region U was last read in the previous block's qk stage, before its score barrier)
        if (blk != lb) load_in(r0);
        store_in();
        // the q projection's weight fragments (in flight across the staging barrier); those of qk and v
        // are issued one stage ahead of their use (registers: 4 waves per SIMD)
        float b[16], aq[16], ak[16], av[16];
        ld16w(A.Wq + (16 * w + n) * 64 + 16 * h, aq);
        ASTAMP(1);
        __syncthreads();
        ASTAMP(2);
#pragma unroll
        for (int t = 0; t < 16; ++t) ak[t] = A.Wk[(16 * h + t) * 64 + 16 * w + n];
        // encoders: this wave's 16 features of e_o, e_g and of every x_j (transposed, rows on n); the
        // x_j stay in registers: lane (n, h) holds features fo .. fo + 3 of row n, the layout of qk below
        const f4 eo = relu_bias4(enc_lds<KSO>(sWo, Dop, sOwn, Dop, Do, 16 * w, n, h), sB + fo);
        const f4 eg = relu_bias4(enc_lds<5>(sWg, ENC_SG, sRad, ENC_SG, 18, 16 * w, n, h), sB + 64 + fo);
        f4 xj[KM];
#pragma unroll
        for (int j = 0; j < KM; ++j)
            xj[j] = relu_bias4(enc_lds<2>(sWn, ENC_SN, sNei + j * 8, NS, 6, 16 * w, n, h), sB + 128 + fo);
        // the valid-neighbour mask of row n (every lane), read before region U is overwritten
        unsigned valid = 0;
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            const float *pn = sNei + n * NS + j * 8;
            const float m = ((((pn[0] + pn[1]) + pn[2]) + pn[3]) + pn[4]) + pn[5];
            valid |= (j < K && m != 0.0f ? 1u : 0u) << j;
        }
        float *crow = A.cat + (size_t)r * A.ld_cat;
        if (rin) {
            *reinterpret_cast<f4 *>(crow + fo) = eo;
            *reinterpret_cast<f4 *>(crow + 64 + fo) = eg;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) sE[(fo + j) * TS + n] = eo[j];
        if (train && rin) {
#pragma unroll
            for (int j = 0; j < KM; ++j)
                if (j < K) *reinterpret_cast<f4 *>(A.xn + ((size_t)r * K + j) * 64 + fo) = xj[j];
        }
        ASTAMP(3);
        __syncthreads();
        ASTAMP(4);
        // q^T = Wq e_o^T
        lds_bfrag(sE, h, n, b);
        f4 acc = mfma_k64(aq, b);
        if (train && rin) *reinterpret_cast<f4 *>(A.q + (size_t)r * 64 + fo) = acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) sQ[(fo + j) * TS + n] = acc[j];
        __syncthreads();
        ASTAMP(5);
        ld16w(A.Wv + (16 * w + n) * 64 + 16 * h, av);
        // qk^T = Wk^T q^T: lane (n, h) holds qk[n][fo .. fo + 3], beside its x_j features
        lds_bfrag(sQ, h, n, b);
        acc = mfma_k64(ak, b);
        if (train && rin) *reinterpret_cast<f4 *>(A.qk + (size_t)r * 64 + fo) = acc;
        // scores s[n][j] = x_j[n] . qk[n]: the lane's 4 features, the wave's 16 over the lane groups h
        // (xor 16, 32), the four waves' partials through LDS in wave order
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            float p = xj[j][0] * acc[0];
            p = fmaf(xj[j][1], acc[1], p);
            p = fmaf(xj[j][2], acc[2], p);
            p = fmaf(xj[j][3], acc[3], p);
            p += __shfl_xor(p, 16);
            p += __shfl_xor(p, 32);
            if (h == 0) sP[(w * 16 + n) * KM + j] = p;
        }
        __syncthreads();
        ASTAMP(6);
        // masked softmax of row n in every lane; xb = sum_j alpha_j x_j for the lane's features
        {
            float sc[KM];
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                sc[j] = (((sP[n * KM + j] + sP[(16 + n) * KM + j]) + sP[(32 + n) * KM + j]) + sP[(48 + n) * KM + j]) / 8.0f;
                mx = ((valid >> j & 1) && sc[j] > mx) ? sc[j] : mx;
            }
            float den = 0.0f;
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                const float e = (valid >> j & 1) ? __expf(sc[j] - mx) : 0.0f;
                sc[j] = e;
                den += e;
            }
            const float inv = 1.0f / den;
            f4 xb = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                const float a = (valid >> j & 1) ? sc[j] * inv : 0.0f;
                if (train && rin && w == 0 && h == 0 && j < K) A.alpha[(size_t)r * K + j] = a;
#pragma unroll
                for (int t = 0; t < 4; ++t) xb[t] = fmaf(a, xj[j][t], xb[t]);
            }
            if (train && rin) *reinterpret_cast<f4 *>(A.xb + (size_t)r * 64 + fo) = xb;
#pragma unroll
            for (int t = 0; t < 4; ++t) sX[(fo + t) * TS + n] = xb[t];
        }
        __syncthreads();
        ASTAMP(7);
        // v^T = Wv xb^T -> cat[r][128:192]
        lds_bfrag(sX, h, n, b);
        acc = mfma_k64(av, b);
        if (rin) *reinterpret_cast<f4 *>(crow + 128 + fo) = acc;
        ASTAMP(8);
    }
}

// ------------------------------------------------------------------------------ gather
struct SFields {
    float *dst[16];
    float *dst2[16];
    int width[16], chunk[16], dstride[16];
    int offset[17];
    int n;
};

// GR sampled rows per workgroup: a thread's columns map to the same (field, destination offset)
// in every row, so the field search and the index arithmetic run once per column, and the GR
// row loads of a column are in flight together (one workgroup per row issued one load per thread)
constexpr int GR = 8;

__global__ void __launch_bounds__(256) gather_strided_kernel(const float *ring, int rw, const int32_t *idx, int B,
                                                             SFields F) {
    const int b0 = blockIdx.x * GR;
    const int nb = min(GR, B - b0);
    int64_t src[GR];
#pragma unroll
    for (int r = 0; r < GR; ++r) src[r] = (int64_t)idx[b0 + (r < nb ? r : 0)] * rw;
    for (int c = threadIdx.x; c < F.offset[F.n]; c += 256) {
        int f = 0;
        while (c >= F.offset[f + 1]) ++f;
        const int cc = c - F.offset[f];
        const int ch = F.chunk[f], ds = F.dstride[f];
        const int64_t per = (int64_t)(F.width[f] / ch) * ds;      // destination floats per sampled row
        const int64_t rel = (int64_t)(cc / ch) * ds + cc % ch;
        float v[GR];
#pragma unroll
        for (int r = 0; r < GR; ++r) v[r] = ring[src[r] + c];
        float *d1 = F.dst[f], *d2 = F.dst2[f];
#pragma unroll
        for (int r = 0; r < GR; ++r) {
            if (r >= nb) break;
            const int64_t o = (int64_t)(b0 + r) * per + rel;
            d1[o] = v[r];
            if (d2) d2[o] = v[r];
        }
    }
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// tuning knobs (environment, read once): prefetch-ring depth 1..4 for long K chains, and the
// tile count from which a product runs one tile per wave
int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v ? atoi(v) : dflt;
}
// (depth 3 / 4 rings measured slower: 1.296 / 1.353 vs 1.235 ms per bench step)
const int g_depth = std::min(2, std::max(1, env_int("AAC_GEMM_DEPTH", 2)));
// the ring on every product with a chain > 2 chunks: 1.263 -> 1.230 ms per step since the
// epilogue / attention changes (it had measured slower on small products before them)
const int g_deep_tiles = env_int("AAC_GEMM_DEEP_TILES", 0);
const int g_deep_chain = env_int("AAC_GEMM_DEEP_CHAIN", 2);     // ring only for chains longer than this
const int g_wide_tiles = env_int("AAC_GEMM_WIDE_TILES", 2048);
// wide mode for one-chunk products with >= g_wide_kch_tiles tiles: within run-to-run noise on
// configs 3 / 4 (knob_sweep: 1.230 vs 1.230-1.236 ms, 0.687 vs 0.687-0.689 ms), so off by default;
// with small products too (128 tiles) the GRU step got 2 % slower
const int g_wide_kch = env_int("AAC_GEMM_WIDE_KCH", 0);
const int g_wide_kch_tiles = env_int("AAC_GEMM_WIDE_KCH_TILES", 512);
const int g_lw = env_int("AAC_GEMM_LW", 1);                  // row-contiguous operands by 4T-B loads
const int g_vec = env_int("AAC_GEMM_VEC", 1);                // 16-B epilogue rows
const int g_lds = env_int("AAC_GEMM_LDS", 1);                // LDS-staged workgroup tiles
const int g_lds_min_k = env_int("AAC_GEMM_LDS_MIN_K", 64);   // ... for products with K >= this
int g_lds_min_wg = env_int("AAC_GEMM_LDS_MIN_WG", 256);  // tile choice: largest tile with this many workgroups
const int g_lds_min_wg_many = env_int("AAC_GEMM_LDS_MIN_WG_MANY", 48);   // ... in launches of >= 12 products
const long g_lds_min_mn = env_int("AAC_GEMM_LDS_MIN_MN", 64 * 64);
const int g_lds_pref_wg = env_int("AAC_GEMM_LDS_PREF_WG", 512);   // first choice: largest tile with this many
int g_lds_small = env_int("AAC_GEMM_LDS_SMALL", 0);         // allow 32x32 LDS workgroup tiles
const int g_xcd = env_int("AAC_GEMM_XCD", 0);                // XCD-aware order of the LDS tiles
const int g_xcd_all = env_int("AAC_GEMM_XCD_ALL", 0);        // ... of every workgroup of a launch
const int g_adam4 = env_int("AAC_ADAM4", 1);                 // copy-parallel Adam over split-K copies
int g_dump = env_int("AAC_GEMM_DUMP", 0);      // print the plans of the first g_dump launches

int plan(const aac_gemm_prob *in, int n, GBatch &g, bool allow_empty = false) {
    if (n < (allow_empty ? 0 : 1) || n > AAC_GEMM_MAX) return ffail("gemm_batch: 1 <= n <= AAC_GEMM_MAX");
    g.n = n;
    int waves = 0;
    // launches of many independent products (the GRU learner's per-agent groups: 16 products of
    // 512 x 192) fill the chip together, so each product takes LDS tiles from 48 workgroups on
    // (config 4: 0.564 -> 0.558 ms per step; config 3's launches of <= 11 products keep the default)
    // (only launches without split-K products: the tile choice of a product must not depend on
    // which other products share its launch in the ATT learner, whose merged and serial schedules
    // group them differently and must stay bit-identical)
    bool nosplit = true;
    for (int i = 0; i < n; ++i) nosplit &= in[i].ksplit <= 1;
    const int min_wg = (g_lds_min_wg > 0 && g_lds_min_wg <= 512 && n >= 12 && nosplit)
                           ? std::min(g_lds_min_wg, g_lds_min_wg_many) : g_lds_min_wg;
    for (int i = 0; i < n; ++i) {
        const aac_gemm_prob &s = in[i];
        GProb &d = g.p[i];
        const std::string who = "gemm_batch product " + std::to_string(i) + ": ";
        if (s.M <= 0 || s.N <= 0 || s.K <= 0) return ffail(who + "empty product");
        if (!s.A || !s.B) return ffail(who + "NULL operand");
        if (s.ones && !s.cextra) return ffail(who + "ones column needs cextra");
        if (s.N - s.ones > 0 && !s.C) return ffail(who + "NULL C");
        if (s.mact && !s.mask) return ffail(who + "mact needs mask");
        if (s.act < 0 || s.act > 2 || s.mact < 0 || s.mact > 2) return ffail(who + "bad act/mact");
        if (s.C2 && (!s.dvec || s.ksplit > 1 || s.ones || !s.C)) return ffail(who + "dual output needs dvec, C, no split / ones");
        const int ks = s.ksplit > 1 ? s.ksplit : 1;
        if (ks > 1 && (s.split_stride <= 0 || s.addend || s.bias || s.act || s.mact))
            return ffail(who + "ksplit > 1 needs split_stride and a plain epilogue");
        d.A = s.A; d.B = s.B; d.C = s.C; d.bias = s.bias; d.addend = s.addend; d.mask = s.mask;
        d.cextra = s.cextra;
        d.dvec = s.dvec;
        d.C2 = s.C2;
        d.dscale = s.dscale;
        d.sstride = s.split_stride;
        d.M = s.M; d.N = s.N; d.K = s.K;
        d.lda = s.lda; d.ldb = s.ldb; d.ldc = s.ldc; d.ldadd = s.ldadd; d.ldmask = s.ldmask;
        d.ta = s.ta; d.tb = s.tb; d.act = s.act; d.mact = s.mact; d.ones = s.ones;
        d.ks = ks;
        // 32x32 wave tiles (T = 2 blocks of 16 per edge); 64x64 ones measured slower on every
        // learner launch (fewer waves per SIMD to hide the load latency)
        constexpr int T = 2;
        // op(A) rows (m) are K-contiguous unless ta; op(B) rows (n) are K-contiguous iff tb; a
        // row-contiguous operand is read T rows per lane (LW) where its shape allows
        auto lw_ok = [&](const float *X, int ld, int rows) {
            return g_lw && ld % T == 0 && rows % T == 0 && (reinterpret_cast<uintptr_t>(X) & (4 * T - 1)) == 0;
        };
        d.amode = s.ta ? (lw_ok(s.A, s.lda, s.M) ? LW : LT)
                       : (s.lda % 4 == 0 && s.K % 4 == 0 && aligned16(s.A) ? LV : LS);
        d.bmode = !s.tb ? (lw_ok(s.B, s.ldb, s.N - s.ones) ? LW : LT)
                        : (!s.ones && s.ldb % 4 == 0 && s.K % 4 == 0 && aligned16(s.B) ? LV : LS);
        const int tm = (s.M + WT - 1) / WT, tn = (s.N + WT - 1) / WT;
        d.tiles_n = tn;
        d.vec = g_vec && (!s.C || (aligned16(s.C) && s.ldc % 4 == 0)) && (!s.addend || (aligned16(s.addend) && s.ldadd % 4 == 0)) &&
                (!s.mask || (aligned16(s.mask) && s.ldmask % 4 == 0)) && (!s.bias || aligned16(s.bias)) &&
                (ks <= 1 || (s.split_stride % 4 == 0)) && (!s.C2 || (aligned16(s.C2) && aligned16(s.dvec)));
        // large products need no K cut inside a workgroup: one tile per wave; nor do short chains
        // (<= g_wide_kch chunks), where splitting K leaves waves idle and adds the LDS reduction
        const int nch_all = (s.K + KC - 1) / KC;
        d.wide = ks == 1 && (tm * tn >= g_wide_tiles || (nch_all <= g_wide_kch && tm * tn >= g_wide_kch_tiles));
        {
            const int nch = (s.K + KC - 1) / KC;
            const int per = (nch + ks - 1) / ks;
            const int chain = d.wide ? per : (per + 3) / 4;      // chunks per wave
            // the prefetch ring for chains longer than g_deep_chain chunks (whole-step A/B,
            // tools/knob_sweep.sh; a tile-count threshold is kept as a knob)
            d.deep = g_depth > 1 && chain > g_deep_chain && tm * tn >= g_deep_tiles;
        }
        d.w_begin = waves;          // in workgroups
        g.wb[i] = waves;
        // LDS-staged workgroup tiles where both operands load as 16-B segments
        const bool a16 = s.lda % 4 == 0 && aligned16(s.A) && (s.ta ? s.M % 4 == 0 : s.K % 4 == 0);
        const bool b16 = s.ldb % 4 == 0 && aligned16(s.B) && (s.tb ? (s.K % 4 == 0 && !s.ones) : (s.N - s.ones) % 4 == 0);
        d.lds = 0;
        int pick = -1;
        // candidates, largest first; 32x64 before 64x32 on every learner shape (tools/mb_lds.py:
        // 5120x256x640 25.5 vs 27.1 us); forced tiles (g_lds_min_wg < 0) index cand_force
        static const int cand_pref[4][2] = {{2, 2}, {1, 2}, {2, 1}, {1, 1}};
        static const int cand_force[4][2] = {{2, 2}, {2, 1}, {1, 2}, {1, 1}};
        const int(*cand)[2] = cand_pref;
        if (g_lds && !s.C2 && a16 && b16 && s.K >= g_lds_min_k && (long)s.M * s.N >= g_lds_min_mn && s.M >= 32 &&
            s.N - s.ones >= 32) {
            // 32x32 workgroup tiles re-read the operands 2x more than 64-wide ones and lose to the
            // register path's split-K waves on these shapes (tools/mb_lds.py): only with the knob
            // g_lds_min_wg < 0 forces tile -1 - g_lds_min_wg of cand_tall (tests)
            if (g_lds_min_wg < 0) cand = cand_force;
            // two passes: the largest tile giving >= g_lds_pref_wg workgroups (two or more per CU: a
            // product of 320 64x64 tiles left 64 CUs with two workgroups and 192 with one, 30 -> 26 us
            // for 5120x256x640 as 640 32x64 tiles), else the largest with >= min_wg
            const int nc = g_lds_min_wg < 0 ? 0 : (g_lds_small ? 4 : 3);
            // (not in launches of many products, whose tiles fill the chip together: min_wg_many)
            for (int pass = (g_lds_pref_wg > min_wg && min_wg == g_lds_min_wg ? 0 : 1); pass < 2 && pick < 0; ++pass)
                for (int c = 0; c < nc; ++c) {
                    const long nt = (long)((s.M + 32 * cand[c][0] - 1) / (32 * cand[c][0])) *
                                    ((s.N + 32 * cand[c][1] - 1) / (32 * cand[c][1])) * ks;
                    if (nt >= (pass == 0 ? g_lds_pref_wg : min_wg)) {
                        pick = c;
                        break;
                    }
                }
            if (pick < 0 && g_lds_small) pick = 3;
            if (g_lds_min_wg < 0) pick = std::min(3, -1 - g_lds_min_wg);
        }
        if (pick >= 0) {
            const int TI = cand[pick][0], TJ = cand[pick][1];
            const int cfg = (TI == 2 && TJ == 2) ? 0 : (TI == 2 ? 1 : (TJ == 2 ? 2 : 3));
            const int lay = (s.ta ? 2 : 0) + (s.tb ? 0 : 1);       // bit 1: A row-contiguous, bit 0: B row-contiguous
            d.lds = 1 + cfg * 4 + lay;
            d.xcd = g_xcd;
            d.wide = 0;
            d.deep = 0;
            d.tiles_n = (s.N + 32 * TJ - 1) / (32 * TJ);
            waves += ((s.M + 32 * TI - 1) / (32 * TI)) * d.tiles_n * ks;
            continue;
        }
        waves += (d.wide ? tm * ((tn + 3) / 4) : tm * tn) * ks;
    }
    g.waves = waves;
    g.xcd_all = g_xcd_all == 1 || (g_xcd_all == 2 && n >= 12);   // 2: launches of many products only
    g.nh = 0;
    g.hb[0] = g.hb[1] = waves;
    for (int i = n; i < AAC_GEMM_MAX; ++i) g.wb[i] = 0x7fffffff;
    if (g_dump > 0) {
        --g_dump;
        fprintf(stderr, "gemm_batch n=%d wg=%d\n", n, waves);
        for (int i = 0; i < n; ++i) {
            const GProb &d = g.p[i];
            fprintf(stderr, "  M=%d N=%d K=%d ta=%d tb=%d ones=%d ks=%d amode=%d bmode=%d wide=%d deep=%d lds=%d act=%d mact=%d add=%d\n",
                    d.M, d.N, d.K, d.ta, d.tb, d.ones, d.ks, d.amode, d.bmode, d.wide, d.deep, d.lds, d.act, d.mact,
                    d.addend != nullptr);
        }
    }
    return 0;
}

}  // namespace

extern "C" {

const char *aac_fused_last_error(void) { return f_err.c_str(); }

// diagnostic builds with -DAAC_GEMM_STAMPS: copy the per-workgroup stamps of the last gemm launch
int aac_gemm_stamps(unsigned long long *out, int32_t n_wg) {
#ifdef AAC_GEMM_STAMPS
    FHIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gemm_st), sizeof(unsigned long long) * 5 * std::min(n_wg, STAMP_WG)));
    static unsigned long long zero[STAMP_WG][5];
    FHIP(hipMemcpyToSymbol(HIP_SYMBOL(g_gemm_st), zero, sizeof(zero)));
    return 0;
#else
    (void)out;
    (void)n_wg;
    return ffail("built without AAC_GEMM_STAMPS");
#endif
}

void aac_gemm_set_lds_policy(int32_t min_workgroups, int32_t small_tiles) {
    g_lds_min_wg = min_workgroups;
    g_lds_small = small_tiles;
}

int aac_gemm_plan(const aac_gemm_prob *probs, int32_t n, int32_t *lds_cfg, int32_t *workgroups) {
    GBatch g{};
    if (plan(probs, n, g)) return -1;
    for (int i = 0; i < g.n; ++i) lds_cfg[i] = g.p[i].lds;
    if (workgroups) *workgroups = g.waves;
    return 0;
}

static int head_check(const aac_head_job &j) {
    if (j.mode < 0 || j.mode > 2) return ffail("critic_head: mode 0, 1 or 2");
    if (j.mode == 0 && !j.y) return ffail("critic_head: mode 0 needs y");
    if (j.mode < 2 && !j.dh) return ffail("critic_head: modes 0/1 need dh");
    if (j.mode == 2 && (!j.rew || !j.done || !j.yout || j.B <= 0 || j.N <= 0))
        return ffail("critic_head: mode 2 needs rew/done/yout");
    if (!j.h || !j.w || !j.b) return ffail("critic_head: NULL h / w / b");
    if (j.M2 > 0 && (j.mode != 2 || !j.h2 || !j.w2 || !j.b2 || !j.dh2 || j.M2 > j.M))
        return ffail("critic_head: a chained mse head needs mode 2, h2 / w2 / b2 / dh2 and M2 <= M");
    return 0;
}

static HeadJob head_job(const aac_head_job &j) {
    HeadJob J;
    J.h = j.h; J.w = j.w; J.b = j.b; J.y = j.y; J.rew = j.rew; J.done = j.done;
    J.q = j.q; J.dq = j.dq; J.dh = j.dh; J.yout = j.yout;
    J.ldh = j.ldh; J.M = j.M; J.mode = j.mode; J.B = j.B; J.N = j.N; J.gamma = j.gamma;
    J.h2 = j.h2; J.w2 = j.w2; J.b2 = j.b2; J.q2 = j.q2; J.dq2 = j.dq2; J.dh2 = j.dh2; J.M2 = j.M2 > 0 ? j.M2 : 0;
    return J;
}

static int launch_batch(GBatch &g, hipStream_t st);

int aac_gemm_batch_heads(const aac_gemm_prob *probs, int32_t n, const aac_head_job *heads, int32_t nh, void *stream) {
    if (nh < 0 || nh > HEAD_MAX || (nh > 0 && !heads)) return ffail("gemm_batch_heads: 0 <= nh <= AAC_HEAD_MAX");
    if (n + nh < 1) return ffail("gemm_batch_heads: nothing to launch");
    GBatch g{};
    if (plan(probs, n, g, true)) return -1;
    int wb = g.waves;
    for (int j = 0; j < nh; ++j) {
        if (head_check(heads[j])) return -1;
        if (heads[j].M2 > 0) return ffail("gemm_batch_heads: a chained head job runs alone (aac_critic_head_job)");
        g.h[j] = head_job(heads[j]);
        g.hb[j] = wb;
        wb += (std::max(heads[j].M, 0) + 3) / 4;
    }
    for (int j = nh; j <= HEAD_MAX; ++j) g.hb[j] = wb;
    g.nh = nh;
    g.waves = wb;
    if (wb == 0) return 0;
    return launch_batch(g, (hipStream_t)stream);
}

int aac_gemm_batch(const aac_gemm_prob *probs, int32_t n, void *stream) {
    GBatch g{};
    if (plan(probs, n, g)) return -1;
    return launch_batch(g, (hipStream_t)stream);
}

int aac_gemm_batch_ordered(const aac_gemm_prob *probs, int32_t n, int32_t xcd_order, void *stream) {
    GBatch g{};
    if (plan(probs, n, g)) return -1;
    g.xcd_all = xcd_order ? 1 : 0;      // explicit: overrides AAC_GEMM_XCD_ALL either way
    return launch_batch(g, (hipStream_t)stream);
}

static int launch_batch(GBatch &g, hipStream_t st) {
    bool deep = false, lds = false;
    for (int i = 0; i < g.n; ++i) {
        deep |= g.p[i].deep != 0;
        lds |= g.p[i].lds != 0;
    }
    const dim3 grid(g.waves), block(256);
    if (lds) {
        // the launch's LDS: the largest ring among its LDS-tile products (>= the register path's buffers)
        static const int ring_bytes[4] = {LCfg<2, 2>::BYTES, LCfg<2, 1>::BYTES, LCfg<1, 2>::BYTES, LCfg<1, 1>::BYTES};
        size_t bytes = REG_LDS_BYTES;
        for (int i = 0; i < g.n; ++i)
            if (g.p[i].lds) bytes = std::max(bytes, (size_t)ring_bytes[(g.p[i].lds - 1) >> 2]);
        if (deep && g_depth == 2) hipLaunchKernelGGL((gemm_kernel<2, true>), grid, block, bytes, st, g);
        else hipLaunchKernelGGL((gemm_kernel<1, true>), grid, block, bytes, st, g);
    } else {
        if (deep && g_depth == 2) hipLaunchKernelGGL((gemm_kernel<2, false>), grid, block, 0, st, g);
        else hipLaunchKernelGGL((gemm_kernel<1, false>), grid, block, 0, st, g);
    }
    FHIP(hipGetLastError());
    return 0;
}

static int grid_for(int64_t n) {
    int64_t b = (n + 255) / 256;
    return (int)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

// the copy-parallel sum (adam_sum4_kernel, sum_partials4_kernel) when the copies allow 16-B loads;
// both entry points pick by the same rule, so their sums are the same bits
static bool use_sum4(const float *gpart, int ns, int64_t gstride) {
    return g_adam4 && gstride % 4 == 0 && aligned16(gpart) && ns > 1;
}

int32_t aac_copy_sum_order(const float *gpart, int32_t nsplit, int64_t gstride) {
    return use_sum4(gpart, nsplit, gstride) ? 1 : 0;
}

static int sum4_grid(int64_t n) { return (int)std::min<int64_t>(((n + 63) / 64 + 3) / 4, 8192); }

int aac_adam_flat_sum(float *p, const float *gpart, int32_t ns, float *gout, float *m, float *v, int64_t n, float lr,
                      float b1, float b2, float eps, const int32_t *step, int32_t step_add, void *stream) {
    return aac_adam_flat_sum_strided(p, gpart, ns, n, gout, m, v, n, lr, b1, b2, eps, step, step_add, stream);
}

int aac_adam_flat_sum_strided(float *p, const float *gpart, int32_t ns, int64_t gstride, float *gout, float *m, float *v,
                              int64_t n, float lr, float b1, float b2, float eps, const int32_t *step, int32_t step_add,
                              void *stream) {
    if (ns < 1) return ffail("adam_flat_sum: nsplit >= 1");
    if (gstride < n) return ffail("adam_flat_sum: copy stride < n");
    if (n < 1) return 0;            // the kernels load element min(i, n - 1) unconditionally
    if (use_sum4(gpart, ns, gstride)) {
        const Adam4 P{p, gpart, gout, m, v, step, gstride, n, lr, b1, b2, eps, ns, step_add};
        hipLaunchKernelGGL(adam_sum4_kernel, dim3(sum4_grid(n)), dim3(256), 0, (hipStream_t)stream, P);
    } else {
        hipLaunchKernelGGL(adam_sum_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, gpart, ns, gstride, gout,
                           m, v, n, lr, b1, b2, eps, step, step_add);
    }
    FHIP(hipGetLastError());
    return 0;
}

int aac_adam_flat_sum_pair(const aac_adam_job *a, const aac_adam_job *b, void *stream) {
    if (!a || !b) return ffail("adam_flat_sum_pair: two jobs");
    const aac_adam_job *jj[2] = {a, b};
    Adam4 P[2];
    for (int q = 0; q < 2; ++q) {
        const aac_adam_job &j = *jj[q];
        if (j.nsplit < 2 || j.gstride < j.n || !use_sum4(j.gpart, j.nsplit, j.gstride) || j.n < 1)
            return ffail("adam_flat_sum_pair: each job needs >= 2 copies at a 16-B aligned stride >= n "
                         "(else two aac_adam_flat_sum_strided calls)");
        P[q] = Adam4{j.param, j.gpart, j.grad_out, j.exp_avg, j.exp_avg_sq, j.step, j.gstride, j.n, j.lr, j.beta1,
                     j.beta2, j.eps, j.nsplit, j.step_add};
    }
    const int g1 = sum4_grid(a->n), g2 = sum4_grid(b->n);
    hipLaunchKernelGGL(adam_sum4_pair_kernel, dim3(g1 + g2), dim3(256), 0, (hipStream_t)stream, P[0], P[1], g1);
    FHIP(hipGetLastError());
    return 0;
}

int aac_sum_partials(float *out, const float *gpart, int32_t ns, int64_t n, void *stream) {
    return aac_sum_partials_strided(out, gpart, ns, n, n, stream);
}

int aac_sum_partials_strided(float *out, const float *gpart, int32_t ns, int64_t gstride, int64_t n, void *stream) {
    if (ns < 1) return ffail("sum_partials: nsplit >= 1");
    if (gstride < n) return ffail("sum_partials: copy stride < n");
    if (use_sum4(gpart, ns, gstride))
        hipLaunchKernelGGL(sum_partials4_kernel, dim3(sum4_grid(n)), dim3(256), 0, (hipStream_t)stream, out, gpart, ns,
                           gstride, n);
    else
        hipLaunchKernelGGL(sum_partials_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, out, gpart, ns,
                           gstride, n);
    FHIP(hipGetLastError());
    return 0;
}

int aac_critic_head(const float *h, int32_t ldh, int32_t M, const float *w, const float *b, int32_t mode,
                    const float *y, const float *rew, const float *done, int32_t B, int32_t N, float gamma, float *q,
                    float *dq, float *dh, float *yout, void *stream) {
    if (M <= 0) return 0;
    if (mode < 0 || mode > 2) return ffail("critic_head: mode 0, 1 or 2");
    if (mode == 0 && !y) return ffail("critic_head: mode 0 needs y");
    if (mode < 2 && !dh) return ffail("critic_head: modes 0/1 need dh");
    if (mode == 2 && (!rew || !done || !yout || B <= 0 || N <= 0)) return ffail("critic_head: mode 2 needs rew/done/yout");
    const aac_head_job j{h, ldh, M, w, b, mode, y, rew, done, B, N, gamma, q, dq, dh, yout,
                         nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if (head_check(j)) return -1;
    hipLaunchKernelGGL(head_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, head_job(j));
    FHIP(hipGetLastError());
    return 0;
}

int aac_critic_head_job(const aac_head_job *job, void *stream) {
    if (!job) return ffail("critic_head_job: NULL job");
    if (job->M <= 0) return 0;
    if (head_check(*job)) return -1;
    hipLaunchKernelGGL(head_kernel, dim3((job->M + 3) / 4), dim3(256), 0, (hipStream_t)stream, head_job(*job));
    FHIP(hipGetLastError());
    return 0;
}

int aac_actor_dcomb_out_bwd(const aac_dcomb_aob_args *a, const aac_head_job *head, void *stream) {
    if (!a) return ffail("actor_dcomb_out_bwd: null args");
    if (a->B <= 0) return 0;
    if (a->N <= 0 || a->din < a->d0 + 2 || a->ldw != 128 * a->N) return ffail("actor_dcomb_out_bwd: need N > 0, din >= d0 + 2, ldw = 128 N");
    if (!a->dh || !a->Wc || !a->f || !a->wenc || !a->X || !a->wa || !a->ha || !a->dout || !a->dha)
        return ffail("actor_dcomb_out_bwd: null operand");
    if (!aligned16(a->dh) || !aligned16(a->Wc) || !aligned16(a->ha) || !aligned16(a->dha) || !aligned16(a->wa))
        return ffail("actor_dcomb_out_bwd: dh, Wc, ha, dha, wa must be 16-B aligned");
    DaobArgs P{a->dh, a->Wc, a->f, a->wenc, a->X, a->wa, a->ha, a->dout, a->dha, a->ldw, a->din, a->d0, a->N, a->B};
    // two 16-sample tiles per workgroup when one per workgroup would exceed the CUs (AAC_DAOB_RT: force)
    static const int rt_env = env_int("AAC_DAOB_RT", 0);
    const int rt = rt_env == 1 || rt_env == 2 ? rt_env : (((a->B + 15) / 16) * a->N > 256 ? 2 : 1);
    const int nwg = ((a->B + 16 * rt - 1) / (16 * rt)) * a->N;
    HeadJob J{};
    int total = nwg;
    if (head) {
        if (head_check(*head)) return -1;
        if (head->M2 > 0) return ffail("actor_dcomb_out_bwd: a chained head job runs alone (aac_critic_head_job)");
        J = head_job(*head);
        total += (std::max(head->M, 0) + 3) / 4;
    }
    if (rt == 2) hipLaunchKernelGGL(actor_dcomb_out_bwd_kernel<2>, dim3(total), dim3(256), 0, (hipStream_t)stream, P, nwg, J);
    else hipLaunchKernelGGL(actor_dcomb_out_bwd_kernel<1>, dim3(total), dim3(256), 0, (hipStream_t)stream, P, nwg, J);
    FHIP(hipGetLastError());
    return 0;
}

int aac_actor_out_bwd(const float *df, int32_t ldf, const float *wenc, int32_t din, int32_t d0, const float *X,
                      const float *wa, const float *ha, int32_t N, int32_t R, float *dout, float *dha, void *stream) {
    if (R <= 0) return 0;
    if (N <= 0 || din < d0 + 2) return ffail("actor_out_bwd: need N > 0 and din >= d0 + 2");
    hipLaunchKernelGGL(actor_out_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, df, ldf, wenc,
                       din, d0, X, wa, ha, N, R, dout, dha);
    FHIP(hipGetLastError());
    return 0;
}

// MFMA training attention: 16-row blocks, a workgroup walks blocks after loading its weight fragments
const int g_attn_mfma = env_int("AAC_ATTN_MFMA", 1);
static int mfma_attn_grid(int R) {
    static const int cap = std::max(1, env_int("AAC_ATTN_WGS", 1024));
    const int nblk = (R + 15) / 16;
    return nblk < cap ? nblk : cap;
}

// riding critic-encoder jobs per agent: every 16-row block its own job up to AAC_RIDE_JOBS jobs in all
// (then each job walks several blocks, the weights staged once)
static int ride_jobs(int rows, int n) {
    static const int cap = std::max(1, env_int("AAC_RIDE_JOBS", 512));
    const int nrb = (rows + 15) / 16, per = std::max(1, cap / std::max(n, 1));
    return nrb < per ? nrb : per;
}

static int attn_grid(int R) {
    static const int rows = std::max(4, env_int("AAC_ATTN_ROWS", 16));
    int wgs = (R + rows - 1) / rows;  // ~4 rows per wave
    return wgs < 1 ? 1 : (wgs > 2048 ? 2048 : wgs);
}

#ifdef AAC_ATTN_STAMPS
int aac_attn_stamps(unsigned long long *out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_attn_st), sizeof(g_attn_st)) == hipSuccess ? 0 : -1;
}
#endif

int aac_attn_train_fwd(const float *eo, int32_t lde, const float *xn, const float *nei, const float *Wq,
                       const float *Wk, const float *Wv, float *q, float *qk, float *alpha, float *xb, float *vout,
                       int32_t ldv, int32_t R, int32_t K, void *stream) {
    if (R <= 0) return 0;
    if (K < 1 || K > 32) return ffail("attn_train_fwd: 1 <= K <= 32");
    hipStream_t st = (hipStream_t)stream;
    if (g_attn_mfma && K <= 8 && aligned16(eo) && lde % 4 == 0 && aligned16(q) &&
        aligned16(qk) && aligned16(vout) && ldv % 4 == 0 && (reinterpret_cast<uintptr_t>(nei) & 7) == 0) {
        const dim3 g(mfma_attn_grid(R)), b(256);
        if (K <= 4)
            hipLaunchKernelGGL(attn_mfma_fwd_kernel<4>, g, b, 0, st, eo, lde, xn, nei, Wq, Wk, Wv, q, qk, alpha, xb,
                               vout, ldv, R, K);
        else
            hipLaunchKernelGGL(attn_mfma_fwd_kernel<8>, g, b, 0, st, eo, lde, xn, nei, Wq, Wk, Wv, q, qk, alpha, xb,
                               vout, ldv, R, K);
        FHIP(hipGetLastError());
        return 0;
    }
    const dim3 grid(attn_grid(R)), block(256);
#define ATF(KM) hipLaunchKernelGGL(attn_train_fwd_kernel<KM>, grid, block, 0, st, eo, lde, xn, nei, Wq, Wk, Wv, q, qk, \
                                   alpha, xb, vout, ldv, R, K)
    if (K <= 4) ATF(4);
    else if (K <= 8) ATF(8);
    else if (K <= 16) ATF(16);
    else ATF(32);
#undef ATF
    FHIP(hipGetLastError());
    return 0;
}

static bool attn_bwd_mfma_ok(const float *dv, int32_t lddv, const float *eo, int32_t lde, const float *dcat_o,
                             int32_t ldd, const float *dq, const float *deo, int32_t K) {
    return g_attn_mfma && K <= 8 && aligned16(dv) && lddv % 4 == 0 && aligned16(eo) && lde % 4 == 0 &&
           aligned16(dcat_o) && ldd % 4 == 0 && aligned16(dq) && aligned16(deo);
}

// the backward's grid: a 16-row block per workgroup up to AAC_ATTN_BWD_WGS workgroups (default: the
// forward's cap), then each walks several (160 at B = 1 024, N = 5: -2 %, so off)
static int attn_bwd_grid(int R) {
    static const int cap = env_int("AAC_ATTN_BWD_WGS", 0);
    const int nblk = (R + 15) / 16;
    return cap > 0 && nblk > cap ? cap : mfma_attn_grid(R);
}

int32_t aac_attn_train_bwd_partials(int32_t R) { return R > 0 ? attn_bwd_grid(R) : 0; }

int aac_attn_train_bwd_wn(const float *dv, int32_t lddv, const float *xn, const float *alpha, const float *qk,
                          const float *eo, int32_t lde, const float *dcat_o, int32_t ldd, const float *Wq,
                          const float *Wk, const float *Wv, float *dxn, float *dqk, float *dq, float *deo, int32_t R,
                          int32_t K, const float *nei, float *pwn, void *stream) {
    if (R <= 0) return 0;
    if (K < 1 || K > 32) return ffail("attn_train_bwd: 1 <= K <= 32");
    hipStream_t st = (hipStream_t)stream;
    const bool mfma = attn_bwd_mfma_ok(dv, lddv, eo, lde, dcat_o, ldd, dq, deo, K);
    if (pwn && (!nei || !mfma)) return ffail("attn_train_bwd: the dWn partials need nei and the MFMA path (K <= 8)");
    if (!pwn && !dxn) return ffail("attn_train_bwd: dxn (or the dWn partials) required");
    if (mfma) {
        const dim3 g(attn_bwd_grid(R)), b(256);
        if (K <= 4)
            hipLaunchKernelGGL(attn_mfma_bwd_kernel<4>, g, b, 0, st, dv, lddv, xn, alpha, qk, eo, lde, dcat_o, ldd, Wq,
                               Wk, Wv, dxn, dqk, dq, deo, R, K, nei, pwn);
        else
            hipLaunchKernelGGL(attn_mfma_bwd_kernel<8>, g, b, 0, st, dv, lddv, xn, alpha, qk, eo, lde, dcat_o, ldd, Wq,
                               Wk, Wv, dxn, dqk, dq, deo, R, K, nei, pwn);
        FHIP(hipGetLastError());
        return 0;
    }
    const dim3 grid(attn_grid(R)), block(256);
#define ATB(KM) hipLaunchKernelGGL(attn_train_bwd_kernel<KM>, grid, block, 0, st, dv, lddv, xn, alpha, qk, eo, lde, \
                                   dcat_o, ldd, Wq, Wk, Wv, dxn, dqk, dq, deo, R, K)
    if (K <= 4) ATB(4);
    else if (K <= 8) ATB(8);
    else if (K <= 16) ATB(16);
    else ATB(32);
#undef ATB
    FHIP(hipGetLastError());
    return 0;
}

int aac_attn_train_bwd(const float *dv, int32_t lddv, const float *xn, const float *alpha, const float *qk,
                       const float *eo, int32_t lde, const float *dcat_o, int32_t ldd, const float *Wq, const float *Wk,
                       const float *Wv, float *dxn, float *dqk, float *dq, float *deo, int32_t R, int32_t K,
                       void *stream) {
    return aac_attn_train_bwd_wn(dv, lddv, xn, alpha, qk, eo, lde, dcat_o, ldd, Wq, Wk, Wv, dxn, dqk, dq, deo, R, K,
                                 nullptr, nullptr, stream);
}

int aac_attn_block(const float *eo, int32_t lde, const float *nei, const float *Wn, const float *bn,
                   const float *Wqk, const float *Wv, float *out, int32_t ldo, int32_t R, int32_t K, void *stream) {
    if (R <= 0) return 0;
    if (K < 1 || K > 32) return ffail("attn_block: 1 <= K <= 32");
    if (g_attn_mfma && K <= 4 && aligned16(eo) && lde % 4 == 0 && aligned16(out) && ldo % 4 == 0) {
        hipLaunchKernelGGL(attn_mfma_block_kernel<4>, dim3(mfma_attn_grid(R)), dim3(256), 0, (hipStream_t)stream, eo,
                           lde, nei, Wn, bn, Wqk, Wv, out, ldo, R, K);
        FHIP(hipGetLastError());
        return 0;
    }
    // ~16 rows per wave: the 34 KB weight staging per workgroup stays small next to the rows
    int wgs = (R + 63) / 64;
    wgs = wgs < 1 ? 1 : (wgs > 2048 ? 2048 : wgs);
    const dim3 grid(wgs), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (K <= 4) hipLaunchKernelGGL(attn_block_kernel<4>, grid, block, 0, st, eo, lde, nei, Wn, bn, Wqk, Wv, out, ldo, R, K);
    else if (K <= 8) hipLaunchKernelGGL(attn_block_kernel<8>, grid, block, 0, st, eo, lde, nei, Wn, bn, Wqk, Wv, out, ldo, R, K);
    else if (K <= 16) hipLaunchKernelGGL(attn_block_kernel<16>, grid, block, 0, st, eo, lde, nei, Wn, bn, Wqk, Wv, out, ldo, R, K);
    else hipLaunchKernelGGL(attn_block_kernel<32>, grid, block, 0, st, eo, lde, nei, Wn, bn, Wqk, Wv, out, ldo, R, K);
    FHIP(hipGetLastError());
    return 0;
}

static int attn_enc_check(const aac_attn_enc_args &A) {
    const bool train = A.xn != nullptr;
    if (A.R > 0) {
        if (A.K < 1 || A.K > 8) return ffail("attn_enc_fwd: 1 <= K <= 8");
        if (!A.own || !A.radar || !A.nei || !A.Wo || !A.bo || !A.Wg || !A.bg || !A.Wn || !A.bn || !A.Wq || !A.Wk ||
            !A.Wv || !A.cat || A.d_own < 1)
            return ffail("attn_enc_fwd: null operand");
        if (!aligned16(A.cat) || A.ld_cat % 4 != 0 || (reinterpret_cast<uintptr_t>(A.nei) & 7) != 0)
            return ffail("attn_enc_fwd: cat rows must be 16-B aligned, nei 8-B aligned");
        if (A.d_own > ENC_DMAX) return ffail("attn_enc_fwd: d_own <= 40");
        if (train && (!A.q || !A.qk || !A.alpha || !A.xb || !aligned16(A.q) || !aligned16(A.qk) || !aligned16(A.xn)))
            return ffail("attn_enc_fwd: training outputs q, qk, alpha, xb (16-B aligned q, qk, xn)");
    }
    if (A.c_rows > 0 && (!A.cx || !A.cW || !A.cb || !A.cf || A.c_n < 1 || A.c_din < 1 || A.c_din > ENC_DMAX ||
                         !aligned16(A.cf)))
        return ffail("attn_enc_fwd: critic-encoder job operands (c_din <= 40, 16-B aligned cf)");
    if (A.c_rows > 0 && A.o_h && (!A.o_w || !A.o_b || !A.o_x || A.o_d0 < 0 || A.o_d0 + 2 > A.c_din ||
                                  !aligned16(A.o_h) || !aligned16(A.o_w)))
        return ffail("attn_enc_fwd: folded output layer (16-B aligned o_h / o_w, o_d0 + 2 <= c_din)");
    return 0;
}

int aac_attn_enc_fwd(const aac_attn_enc_args *args, int32_t nset, void *stream) {
    return aac_attn_enc_fwd_head(args, nset, nullptr, stream);
}

int aac_attn_enc_fwd_head(const aac_attn_enc_args *args, int32_t nset, const aac_head_job *head, void *stream) {
    if (!args || nset < 1 || nset > 2) return ffail("attn_enc_fwd: 1 or 2 argument sets");
    AttnEncBatch P{};
    P.nset = nset;
    int total = 0, kmax = 1, dmax = 0;
    for (int s = 0; s < nset; ++s) {
        if (attn_enc_check(args[s])) return -1;
        P.a[s] = args[s];
        P.start[s] = total;
        P.nattn[s] = args[s].R > 0 ? mfma_attn_grid(args[s].R) : 0;
        P.rjobs[s] = args[s].c_rows > 0 ? ride_jobs(args[s].c_rows, args[s].c_n) : 1;
        P.nride[s] = args[s].c_rows > 0 ? args[s].c_n * P.rjobs[s] : 0;
        total += P.nattn[s] + P.nride[s];
        if (args[s].R > 0 && args[s].K > kmax) kmax = args[s].K;
        if (args[s].R > 0 && args[s].d_own > dmax) dmax = args[s].d_own;
        if (args[s].c_rows > 0 && args[s].c_din > dmax) dmax = args[s].c_din;
    }
    P.hstart = INT_MAX;
    if (head) {
        if (head_check(*head)) return -1;
        if (head->M2 > 0) return ffail("attn_enc_fwd_head: a chained head job runs alone (aac_critic_head_job)");
        P.hj = head_job(*head);
        P.hstart = total;
        total += (std::max(head->M, 0) + 3) / 4;
    }
    if (total == 0) return 0;
    const dim3 g(total), b(256);
    hipStream_t st = (hipStream_t)stream;
    if (kmax > 4) {
        if (dmax > 24) hipLaunchKernelGGL((attn_enc_kernel<8, ENC_DMAX / 4>), g, b, 0, st, P);
        else hipLaunchKernelGGL((attn_enc_kernel<8, 6>), g, b, 0, st, P);
    } else {
        if (dmax > 24) hipLaunchKernelGGL((attn_enc_kernel<4, ENC_DMAX / 4>), g, b, 0, st, P);
        else hipLaunchKernelGGL((attn_enc_kernel<4, 6>), g, b, 0, st, P);
    }
    FHIP(hipGetLastError());
    return 0;
}

int aac_replay_gather_strided(const float *ring, int32_t rw, const int32_t *idx, int32_t B, int32_t n,
                              float *const *dsts, float *const *dsts2, const int32_t *widths,
                              const int32_t *chunks, const int32_t *dstrides, void *stream) {
    if (n < 1 || n > 16) return ffail("gather_strided: 1 <= n_fields <= 16");
    SFields F{};
    F.n = n;
    F.offset[0] = 0;
    for (int f = 0; f < n; ++f) {
        if (widths[f] <= 0 || chunks[f] <= 0 || widths[f] % chunks[f] || dstrides[f] < chunks[f])
            return ffail("gather_strided: bad width/chunk/dstride for field " + std::to_string(f));
        F.dst[f] = dsts[f];
        F.dst2[f] = dsts2 ? dsts2[f] : nullptr;
        F.width[f] = widths[f];
        F.chunk[f] = chunks[f];
        F.dstride[f] = dstrides[f];
        F.offset[f + 1] = F.offset[f] + widths[f];
    }
    if (F.offset[n] > rw) return ffail("gather_strided: fields wider than the ring row");
    if (B <= 0) return 0;
    hipLaunchKernelGGL(gather_strided_kernel, dim3((B + GR - 1) / GR), dim3(256), 0, (hipStream_t)stream, ring, rw, idx, B, F);
    FHIP(hipGetLastError());
    return 0;
}

}  // extern "C"
