// The hash the three RANSACs (pnp_kernels.hip, detector/detector.hip, mapping/mapping.hip) draw their minimal sets with.  The
// integer sequence is restated by the oracles' sampler (oracle/ransac_common.py) and must not change.
#pragma once
#include <hip/hip_runtime.h>

namespace sampling {

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// draw number `ctr` of hypothesis `hyp`: an index in [0, n)
__device__ __forceinline__ int draw(unsigned long long seed, int hyp, unsigned long long ctr, int n) {
    return (int)((splitmix64((seed << 40) ^ ((unsigned long long)hyp << 8) ^ ctr) >> 11) % (unsigned long long)n);
}

// K distinct indices in [0, n), n >= K: the draws ctr = 0, 1, .. of hypothesis `hyp` in turn, one that repeats an earlier index
// rejected (it still consumes its counter value).  Oracle: sample_indices.  Every idx subscript is a compile-time constant.
template <int K>
__device__ __forceinline__ void distinct(unsigned long long seed, int hyp, int n, int (&idx)[K]) {
    unsigned long long ctr = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        bool dup;
        do {
            idx[k] = draw(seed, hyp, ctr++, n);
            dup = false;
#pragma unroll
            for (int j = 0; j < k; ++j) dup |= idx[j] == idx[k];
        } while (dup);
    }
}

}  // namespace sampling
