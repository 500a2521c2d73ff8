// aac_copysum.h -- the sum of a weight gradient's ns split-K partial copies, for every kernel that
// forms it: the Adam kernels (aac_fused.hip, aac_uam_learn.hip), the partial sums ahead of an
// all-reduce, the clip kernels (aac_clip.hip) and the learner monitor (aac_monitor.hip).  The copies are
// summed in the element type, in one of two orders, and every kernel that sums in an order produces
// the same bits: how many loads are in flight (DEPTH) changes the schedule, never the additions.
//
//   order 0   copies 0, 1, 2, ... in sequence, starting from copy 0's value.
//   order 1   the four copy groups s % 4, each summed from zero in increasing s, then
//             (g0 + g1) + (g2 + g3).  copy_sum4 (aac_fused.hip) is the lane-parallel form of this
//             order: 16 lanes per group, the groups combined by two xor shuffles.
//
// Which order the float Adam / partial-sum kernels take for a set of copies is aac_copy_sum_order
// (include/aac_fused.h); the double kernels take order 0.  Device-only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace aaccs {

// V consecutive elements at p (cnt of them exist): one 16-byte load where allowed
template <typename T, int V>
__device__ __forceinline__ void load_unit(const T *__restrict__ p, bool wide, int cnt, T (&x)[V]) {
    typedef T VT __attribute__((ext_vector_type(V)));
    if (wide) {
        const VT q = *reinterpret_cast<const VT *>(p);
#pragma unroll
        for (int c = 0; c < V; ++c) x[c] = q[c];
    } else {
#pragma unroll
        for (int c = 0; c < V; ++c) x[c] = c < cnt ? p[c] : T(0);
    }
}

// order 0 from copy 1 on: out holds copy 0's unit on entry (a caller may have loaded it earlier).
// DEPTH independent loads in flight per step instead of a dependent chain of ns.
template <typename T, int V, int DEPTH>
__device__ __forceinline__ void seq_unit(const T *__restrict__ g, int ns, int64_t gs, bool wide, int cnt, T (&out)[V]) {
    int s = 1;
    for (; s + DEPTH <= ns; s += DEPTH) {
        T x[DEPTH][V];
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) load_unit<T, V>(g + (int64_t)(s + u) * gs, wide, cnt, x[u]);
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
#pragma unroll
            for (int c = 0; c < V; ++c) out[c] += x[u][c];
    }
    for (; s < ns; ++s) {
        T x[V];
        load_unit<T, V>(g + (int64_t)s * gs, wide, cnt, x);
#pragma unroll
        for (int c = 0; c < V; ++c) out[c] += x[c];
    }
}

// order 0 of element i of copies gs apart, one element per thread (gi: copy 0's value)
template <typename T>
__device__ __forceinline__ T copy_sum_seq(const T *__restrict__ gpart, int ns, int64_t gs, int64_t i, T gi) {
    T out[1] = {gi};
    seq_unit<T, 1, 8>(gpart + i, ns, gs, false, 1, out);
    return out[0];
}

// the summed gradient of V consecutive elements at g, in either order
template <typename T, int V, int DEPTH>
__device__ __forceinline__ void sum_unit(const T *__restrict__ g, int ns, int64_t gs, int order, bool wide, int cnt,
                                         T (&out)[V]) {
    static_assert(DEPTH % 4 == 0, "a step holds whole rounds of the four groups");
    if (order == 0) {
        load_unit<T, V>(g, wide, cnt, out);
        seq_unit<T, V, DEPTH>(g, ns, gs, wide, cnt, out);
        return;
    }
    T x[DEPTH][V], a[4][V];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < V; ++c) a[u][c] = T(0);
    int s = 0;
    for (; s + DEPTH <= ns; s += DEPTH) {
#pragma unroll
        for (int u = 0; u < DEPTH; ++u) load_unit<T, V>(g + (int64_t)(s + u) * gs, wide, cnt, x[u]);
#pragma unroll
        for (int u = 0; u < DEPTH; ++u)
#pragma unroll
            for (int c = 0; c < V; ++c) a[u & 3][c] += x[u][c];
    }
    // the last ns % DEPTH copies: their loads, then their adds
#pragma unroll
    for (int u = 0; u < DEPTH - 1; ++u) {
        if (s + u < ns) load_unit<T, V>(g + (int64_t)(s + u) * gs, wide, cnt, x[u]);
    }
#pragma unroll
    for (int u = 0; u < DEPTH - 1; ++u) {
        if (s + u < ns) {
#pragma unroll
            for (int c = 0; c < V; ++c) a[u & 3][c] += x[u][c];
        }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) out[c] = (a[0][c] + a[1][c]) + (a[2][c] + a[3][c]);
}

__device__ __forceinline__ unsigned addr16(const void *p) { return (unsigned)((uintptr_t)p & 15u); }

// a fixed butterfly: every lane holds the wave's sum
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace aaccs
