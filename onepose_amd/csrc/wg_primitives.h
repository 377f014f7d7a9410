// Workgroup primitives of the small latency-bound kernels: the geometry files (pnp_kernels.hip, detector/detector.hip,
// detector/flow.hip, mapping/mapping.hip, mapping/bundle_adjust.hip, mapping/track_update.hip), spp_detect_kernels.hip and
// gatsspg_train_kernels.hip.  Integer arithmetic and floating-point additions only: nothing here can be contracted into an FMA, so
// a primitive means the same in a file compiled with the default contraction and in one that sets fp contract(off).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace wg {

// Exclusive prefix sum of one int per thread over the NT threads of the workgroup, in thread order: returns the sum of v over the
// threads before this one, total = the sum over all of them.  wsum: NT / 64 ints of LDS.  Every thread of the workgroup calls it;
// one barrier before wsum is written (it may be called in a loop) and one after.
template <int NT>
__device__ __forceinline__ int excl_scan(int v, int* wsum, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    __syncthreads();
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const int t = wsum[w];
        if (w < wave) before += t;
        total += t;
    }
    return before + inc - v;
}

// Sum of one integer (int, long long, ..) per lane over the 64 lanes of the wave (xor butterfly), the same on every lane.
template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_integral<T>::value, "integers only: a floating-point sum depends on the order of the butterfly");
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// Sum of Q doubles per thread over the NT threads of the workgroup through red (Q * NT doubles of LDS), in the fixed order
//   red[q][t] += red[q][t + s]  for s = NT / 2, NT / 4, .., 1
// (oracle: lane_tree_sum).  On return v[q] holds the total on every thread.  Every thread calls it; it starts with a barrier, so
// two calls may follow each other on the same red.
template <int NT, int Q>
__device__ __forceinline__ void tree_sum(double (&v)[Q], double* red) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q * NT + t] = v[q];
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int q = 0; q < Q; ++q) red[q * NT + t] += red[q * NT + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = red[q * NT];
}

}  // namespace wg
