// rng_kernels.hip -- numpy's legacy generator (np.random.RandomState: MT19937) on the device, bit for bit, one independent
// stream per planning problem.  The streams planner (planner.plan_maze_rounds_batch, eval_gnn.py:191-247 for a batch) gives
// every problem the draws np.random.seed(s_b) followed by the reference's uniform_sample calls would give it
// (environment/maze_env.py uniform_sample -> np.random.uniform(-LIMITS, LIMITS)); B independent generators are parallel work,
// so the draws need not come from the host.  What is reproduced, exactly:
//   * init_genrand seeding: key[0] = seed, key[i] = 1812433253 * (key[i-1] ^ (key[i-1] >> 30)) + i, pos = 624;
//   * the 624-word twist (N = 624, M = 397, matrix 0x9908b0df) and the tempering of every word;
//   * random_double: two consecutive words a, b -> ((a >> 5) * 67108864.0 + (b >> 6)) / 9007199254740992.0;
//   * uniform with array bounds: low[c] + range[c] * d with range = high - low taken once (by the caller, in double),
//     elements in C order;
//   * numpy's LAZY twist: a block is regenerated when a word is needed and pos == 624, never before, so a stream that
//     consumed exactly to the end of a block keeps pos = 624 and the old key -- the state compares equal to get_state().
// A stream's state is uint32 key[624] followed by int32 pos: 625 words, the layout of RandomState.get_state()[1:3].
#include <hip/hip_runtime.h>
#include "kernels.hpp"

// low + range * d is two rounded operations in numpy: a fused multiply-add changes about half of the draws of a column
// whose bounds are not powers of two (the stick robot's z: low = -0.4, range = 0.8).
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kMtN = 624, kMtM = 397, kMtWords = 625;
constexpr int kMtThreads = 256;

__device__ __forceinline__ unsigned mt_temper(unsigned y) {
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}

// the part of new[i] that comes from (old[i], old[i + 1]): genrand's y >> 1 ^ mag01[y & 1]
__device__ __forceinline__ unsigned mt_mix(unsigned u, unsigned v) {
    const unsigned y = (u & 0x80000000u) | (v & 0x7fffffffu);
    return (y >> 1) ^ ((v & 1u) ? 0x9908b0dfu : 0u);
}

// One block of 624 words in place.  new[i] = new-or-old[(i + 397) % 624] ^ mix(old[i], old[i + 1]): every mix of two OLD
// words is taken into registers first (old[i + 1] is another lane's to overwrite), then the words are written in the three
// dependent segments: [0, 227) reads old [397, 624); [227, 454) reads new [0, 227); [454, 623) reads new [227, 396); word 623
// mixes old[623] with NEW[0] and reads new[396], both written by then.  Called by all kMtThreads threads.
__device__ __forceinline__ void mt_twist(unsigned* mt, int tid) {
    unsigned mix[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = tid + k * kMtThreads;
        mix[k] = i < kMtN - 1 ? mt_mix(mt[i], mt[i + 1]) : 0u;
    }
    __syncthreads();
    if (tid < kMtN - kMtM) mt[tid] = mt[tid + kMtM] ^ mix[0];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = tid + k * kMtThreads;
        if (i >= kMtN - kMtM && i < 2 * (kMtN - kMtM)) mt[i] = mt[i - (kMtN - kMtM)] ^ mix[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 1; k < 3; ++k) {
        const int i = tid + k * kMtThreads;
        if (i >= 2 * (kMtN - kMtM) && i < kMtN - 1) mt[i] = mt[i - (kMtN - kMtM)] ^ mix[k];
        else if (i == kMtN - 1) mt[i] = mt[kMtM - 1] ^ mt_mix(mt[i], mt[0]);
    }
    __syncthreads();
}

}  // namespace

// One thread per stream: the recurrence is 623 dependent steps.
__global__ __launch_bounds__(64) void mt_seed_kernel(int n, const unsigned* __restrict__ seeds, unsigned* __restrict__ state) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    unsigned* key = state + (size_t)s * kMtWords;
    unsigned x = seeds[s];
    key[0] = x;
    for (int i = 1; i < kMtN; ++i) {
        x = 1812433253u * (x ^ (x >> 30)) + (unsigned)i;
        key[i] = x;
    }
    key[kMtN] = (unsigned)kMtN;
}

// One workgroup per stream, the key in LDS.  The stream yields counts[b] * dim doubles = twice as many words from wherever its
// pos stands (any value in [0, 624], odd ones included: a double may take word 623 of one block and word 0 of the next, which
// the `carry` word below bridges).  out != nullptr: element e of the stream's rows goes to out[out_ptr[b] * dim + e];
// commit: the advanced state is stored; out == nullptr with commit: the rows are skipped (no tempering, no stores).
__global__ __launch_bounds__(kMtThreads) void mt_uniform_kernel(MtUniformParams p) {
    __shared__ unsigned mt[kMtN];
    __shared__ double s_low[3], s_range[3];                      // indexed by column: LDS, not a run-time index into registers
    const int b = blockIdx.x, tid = threadIdx.x;
    if (p.active && !p.active[b]) return;
    unsigned* st = p.state + (size_t)b * kMtWords;
    const long long cnt = p.counts[b];
    int pos = (int)st[kMtN];
    long long o0 = 0;
    bool bad = cnt < 0 || pos < 0 || pos > kMtN;
    if (p.out && !bad) {
        o0 = p.out_ptr[b];
        bad = o0 < 0 || o0 > p.out_rows || cnt > p.out_rows - o0;
    }
    if (bad) {                                                   // nothing of this stream is touched
        if (tid == 0) p.status[b] = 2;
        return;
    }
    for (int i = tid; i < kMtN; i += kMtThreads) mt[i] = st[i];
    if (tid == 0) {
        s_low[0] = p.low0; s_low[1] = p.low1; s_low[2] = p.low2;
        s_range[0] = p.range0; s_range[1] = p.range1; s_range[2] = p.range2;
    }
    __syncthreads();
    const int dim = p.dim;
    double* out = p.out ? p.out + (size_t)o0 * dim : nullptr;
    const long long total = cnt * dim;                           // doubles to yield
    long long done = 0;
    bool have_carry = false;
    unsigned carry = 0;                                          // tempered word 623 of the block before, first half of a double
    while (done < total) {
        if (pos == kMtN) {                                       // a word is needed and the block is used up
            mt_twist(mt, tid);
            pos = 0;
        }
        int c0 = (int)(done % dim);                              // column of element `done` (uniform: one 64-bit modulo per block)
        if (have_carry) {
            if (out && tid == 0) {
                const unsigned a = carry, w = mt_temper(mt[pos]);
                const double d = ((double)(a >> 5) * 67108864.0 + (double)(w >> 6)) / 9007199254740992.0;
                out[done] = s_low[c0] + s_range[c0] * d;
            }
            pos += 1; done += 1; have_carry = false;
            c0 = c0 + 1 == dim ? 0 : c0 + 1;
        }
        const long long left = total - done;
        const int pairs = (int)(left < (kMtN - pos) / 2 ? left : (kMtN - pos) / 2);
        if (out) {
            for (int t = tid; t < pairs; t += kMtThreads) {
                const unsigned a = mt_temper(mt[pos + 2 * t]), w = mt_temper(mt[pos + 2 * t + 1]);
                const double d = ((double)(a >> 5) * 67108864.0 + (double)(w >> 6)) / 9007199254740992.0;
                const int c = (c0 + t) % dim;
                out[done + t] = s_low[c] + s_range[c] * d;
            }
        }
        pos += 2 * pairs; done += pairs;
        if (done < total && pos == kMtN - 1) {                   // the next double starts on the block's last word
            carry = mt_temper(mt[kMtN - 1]);
            have_carry = true;
            pos = kMtN;
        }
        __syncthreads();                                         // every read of this block is done before the next twist
    }
    if (p.commit) {
        for (int i = tid; i < kMtN; i += kMtThreads) st[i] = mt[i];
        if (tid == 0) st[kMtN] = (unsigned)pos;
    }
    if (tid == 0) p.status[b] = 0;
}

hipError_t launch_mt_seed(int n, const unsigned* seeds, unsigned* state, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(mt_seed_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n, seeds, state);
    return hipGetLastError();
}

hipError_t launch_mt_uniform(const MtUniformParams& p, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(mt_uniform_kernel, dim3(p.n), dim3(kMtThreads), 0, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
