// wave64.hpp -- the small helpers of the one-wave-per-problem kernels: the fence + barrier that orders a wave's LDS / global
// traffic, wave-wide reductions by shuffles (all 64 lanes active) and the binary search in a sorted block of edge keys.
// Every helper lives in an unnamed namespace: each kernel file compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>

namespace gnnmp {

namespace {

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o < k ? o : k;
    }
    return k;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off, 64);
        k = o > k ? o : k;
    }
    return k;
}
// first slot q in [lo, hi) with key[q] >= x (key sorted ascending), hi when none
__device__ __forceinline__ int lower_bound(const long long* key, int lo, int hi, long long x) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace

}  // namespace gnnmp
