// Adam's bias corrections and element step for the optimiser kernels (aac_fused.hip, aac_learn.hip,
// aac_uam_learn.hip, aac_clip.hip).
//
// step_size = lr / (1 - b1^t) and bc2s = sqrt(1 - b2^t) are the same two numbers for every thread of
// a launch, and their double pow / divide / sqrt is some 330 fp64 VALU instructions in one dependent
// chain.  Evaluated by every wave ahead of its first load (as these kernels used to) that arithmetic
// is what a short optimiser launch spends most of its time on.  adam_bias_bcast has wave 0 of a
// workgroup evaluate step_size and wave 1 bc2s (the two chains side by side on two SIMDs; wave 0 both
// in a one-wave workgroup), after every wave has issued the loads of its first trip, and hands them to
// the other waves through LDS behind one workgroup barrier.
//
// The expressions are the ones the kernels always used, so the results are the same bits.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float adam_step_size(float lr, float b1, int t) {
    const double bc1 = 1.0 - pow((double)b1, (double)t);
    return (float)((double)lr / bc1);
}

__device__ __forceinline__ float adam_bc2_sqrt(float b2, int t) {
    const double bc2 = 1.0 - pow((double)b2, (double)t);
    return (float)sqrt(bc2);
}

__device__ __forceinline__ double adam_step_size(double lr, double b1, int t) {
    const double bc1 = 1.0 - pow(b1, (double)t);
    return lr / bc1;
}

__device__ __forceinline__ double adam_bc2_sqrt(double b2, int t) {
    const double bc2 = 1.0 - pow(b2, (double)t);
    return sqrt(bc2);
}

// One element's Adam step on gradient gi: the only place the element arithmetic is written.  Every
// optimiser kernel calls it -- adam_kernel (aac_learn.hip), adam_sum_kernel and adam4_body
// (aac_fused.hip), adam64_kernel (aac_uam_learn.hip), adam_clip_kernel (aac_clip.hip) -- so their
// steps on equal inputs are the same bits.  The float form follows torch's operation order, the
// double form the UAM learner's b1 * m + (1 - b1) * g.
__device__ __forceinline__ void adam_elem(float &p, float &m, float &v, float gi, float b1, float b2, float eps,
                                          float step_size, float bc2s) {
    const float w1 = (float)(1.0 - (double)b1), w2 = (float)(1.0 - (double)b2);
    float mi = m;
    mi = mi + w1 * (gi - mi);               // exp_avg.lerp_(grad, 1 - beta1)
    float vi = v * b2;                      // exp_avg_sq.mul_(beta2)
    vi = vi + w2 * (gi * gi);               //   .addcmul_(grad, grad, 1 - beta2)
    const float den = sqrtf(vi) / bc2s + eps;
    p = p + (-step_size) * (mi / den);      // param.addcdiv_(exp_avg, denom, -step_size)
    m = mi;
    v = vi;
}

__device__ __forceinline__ void adam_elem(double &p, double &m, double &v, double gi, double b1, double b2,
                                          double eps, double step_size, double bc2s) {
    const double mi = b1 * m + (1.0 - b1) * gi;
    const double vi = b2 * v + (1.0 - b2) * gi * gi;
    const double den = sqrt(vi) / bc2s + eps;
    p = p - step_size * mi / den;
    m = mi;
    v = vi;
}

// Every thread of the workgroup calls this exactly once, outside any divergent branch or loop (it
// holds the workgroup barrier), after issuing its first loads.  sh: two T in LDS.  The branches are
// wave-uniform.  The sched_barrier keeps the compiler from sinking those loads below the fp64 block.
template <typename T>
__device__ __forceinline__ void adam_bias_bcast(T *sh, T lr, T b1, T b2, int t, T &step_size, T &bc2s) {
    asm volatile("" ::"s"(t));      // the counter's scalar load up here with the others, not inside a wave's branch
    __builtin_amdgcn_sched_barrier(0);
    const int w = threadIdx.x >> 6, w2 = blockDim.x > 64 ? 1 : 0;
    if (w == 0) {
        const T s = adam_step_size(lr, b1, t);
        if (threadIdx.x == 0) sh[0] = s;
    }
    if (w == w2) {
        const T c = adam_bc2_sqrt(b2, t);
        if ((threadIdx.x & 63) == 0) sh[1] = c;
    }
    __syncthreads();
    step_size = sh[0];
    bc2s = sh[1];
}
