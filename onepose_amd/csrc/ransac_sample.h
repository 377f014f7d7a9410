// The hash both RANSACs (pnp_kernels.hip, detector/detector.hip) draw their minimal sets with.  The integer sequence is
// restated by their oracles (oracle/pnp_oracle.py, tests/detector_oracle.py) and must not change.
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

}  // namespace sampling
