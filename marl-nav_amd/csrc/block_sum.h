// block_sum.h - the fp64 sum of a block in a fixed order, the reduction of the
// rollout's and the PPO kernels' statistics. Included inside each translation
// unit's anonymous namespace, after its kWaves (the waves of its blocks).
#pragma once

// wave partial sums (fixed shuffle tree), then the waves in order; valid in
// thread 0. sh: kWaves doubles of LDS.
__device__ __forceinline__ double block_sum(double v, double *sh)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < kWaves; ++i) t += sh[i];
    __syncthreads();
    return t;
}
