// explorer_replay_kernels.hip -- what the explorer's training loop (train_explorer.py:96-210) needs around one optimizer step on
// the device: the batch of a group of labelled graphs gathered out of a device-resident dataset (algorithm/dijkstra.py:91-97),
// and the policy loss of :172 with its gradient with respect to the per-edge scores.
//
//   episode_dataset_gather_kernel   one workgroup (256 threads) per group entry.  Wave 0 of EVERY workgroup runs the same
//       exclusive scan over the G selected problems' node / edge / obstacle counts (integers, shuffles, no atomics), so each
//       workgroup knows its own three destination offsets and the three totals without reading a word another one writes.  The
//       workgroup then copies its problem's rows: v [N, C] float32, points64 [N, C] float64, the two rows of edge_index (int64,
//       graph-local, so a plain copy), edge_free, edge_cost, obstacles [O, S], and writes entry g + 1 of the three prefix
//       arrays (workgroup 0 also entry 0 and the status word).
//   episode_frontier_loss_kernel    one workgroup of ONE wave per problem.  The wave walks the problem's frontier list three
//       times: (1) the maximum of the listed scores and, per edge of the problem, how often it is listed (integer atomics on a
//       count array in LDS); (2) sum exp(s - max) in double over the LIST, so an edge listed twice counts twice: lane l adds
//       the entries l, l + 64, ... in ascending order and the 64 partial sums meet in a fixed butterfly; (3) over the problem's
//       EDGES: dscores = (count * exp(s - max) / sum - [label's edge]) / divisor in double, rounded once, exactly 0 for an edge
//       that is not listed.  terms[b] = (float)(log(sum) - (s_label - max)), log_softmax's own order.
//   episode_frontier_loss_sum_kernel   one lane: loss = (terms[0] + terms[1] + ..., ascending, in double) / divisor.
//
// No floating-point atomics (the only atomics are the integer counts in LDS and the integer OR that sets a bit of the loss's
// `bad` word), no scratch, vector stores only; every launch is on the caller's stream and nothing is allocated or
// waited for.  Two runs give the same bits.
//
// Bounds (every guard of these kernels):
//   * gather, index outside [0, n_problems): the slot has the sizes 0, 0, 0 -- nothing is read or copied for it, its prefix
//     entries repeat the previous ones -- and status bit 1 is set.  The index is not clamped.  A repeated index is copied again.
//   * gather, prefix entries of a selected problem that do not ascend inside [0, total] of the store, or totals of the
//     selection that differ from the caller's: status bit 2 and NOTHING is written, so every destination row lies inside the
//     caller's arrays.  The sums are 64-bit.
//   * loss, a problem that is not counted (status != 0, frontier_len == 0, label < 0): term 0, counted 0, dscores 0 over its
//     edge range; its frontier is not read.
//   * loss, edge_ptr entries that do not ascend inside [0, total_edges]: bad bit 2, term 0, counted 0, nothing else written.
//   * loss, frontier_len outside [0, 2 E + 1] (the slot problem b owns in `frontier`), label >= frontier_len, or the label's
//     entry outside the problem's edge range: bad bit 1, the problem is not counted (as above).
//   * loss, a frontier entry outside [edge_ptr[b], edge_ptr[b + 1]): bad bit 1, the entry contributes nothing (no maximum, no
//     sum, no count); the rest of the list is used.
//   * loss, more than 16384 edges in one problem (the count array): bad bit 4, the problem is not counted.
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "wave64.hpp"

// the float64 restatement rounds every operation on its own
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kEdBadIndex = 1, kEdBadGather = 2;
constexpr int kFlBadEntry = 1, kFlBadRange = 2, kFlTooLarge = 4;
constexpr int kEdThreads = 256;
constexpr int kFlCap = 16384;             // edges of one problem the count array holds (64 KB of LDS)

__device__ __forceinline__ long long ed_wave_sum(long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ long long ed_wave_incl(long long x, int lane) {      // inclusive prefix sum over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = __shfl_up(x, off, 64);
        if (lane >= off) x += o;
    }
    return x;
}

struct EdSizes { int n0, e0, o0, N, E, O; };

// the rows of stored problem idx[j]: zeros and bad_index for an index outside the store, zeros and bad_store for prefix entries
// that do not ascend inside the store's totals
__device__ __forceinline__ EdSizes ed_stored(const EpisodeDatasetStore& st, const int* idx, int j, bool& bad_index, bool& bad_store) {
    EdSizes r = {0, 0, 0, 0, 0, 0};
    const int i = idx[j];
    if (i < 0 || i >= st.n) { bad_index = true; return r; }
    const int n0 = st.node_ptr[i], n1 = st.node_ptr[i + 1], e0 = st.edge_ptr[i], e1 = st.edge_ptr[i + 1];
    const int o0 = st.obs_ptr[i], o1 = st.obs_ptr[i + 1];
    if (n0 < 0 || n1 < n0 || n1 > st.total_nodes || e0 < 0 || e1 < e0 || e1 > st.total_edges || o0 < 0 || o1 < o0 ||
        o1 > st.total_obs) {
        bad_store = true;
        return r;
    }
    r.n0 = n0; r.e0 = e0; r.o0 = o0; r.N = n1 - n0; r.E = e1 - e0; r.O = o1 - o0;
    return r;
}

__global__ __launch_bounds__(kEdThreads) void episode_dataset_gather_kernel(EpisodeDatasetStore st, EpisodeGatherParams p) {
    __shared__ int sh[10];            // ok; source rows n0, e0, o0; sizes N, E, O; destination rows of nodes, edges, obstacles
    const int g = blockIdx.x, tid = threadIdx.x;
    if (tid < 64) {
        const int lane = tid;
        bool bad_index = false, bad_store = false;
        long long tn = 0, te = 0, to = 0, run_n = 0, run_e = 0, run_o = 0;
        for (int base = 0; base < p.G; base += 64) {
            const int j = base + lane;
            EdSizes r = {0, 0, 0, 0, 0, 0};
            if (j < p.G) r = ed_stored(st, p.idx, j, bad_index, bad_store);
            const long long in_n = ed_wave_incl(r.N, lane), in_e = ed_wave_incl(r.E, lane), in_o = ed_wave_incl(r.O, lane);
            if (j == g) {
                sh[1] = r.n0; sh[2] = r.e0; sh[3] = r.o0; sh[4] = r.N; sh[5] = r.E; sh[6] = r.O;
                // below 2^31 whenever the totals agree with the caller's, and unused otherwise
                sh[7] = (int)(run_n + in_n - r.N); sh[8] = (int)(run_e + in_e - r.E); sh[9] = (int)(run_o + in_o - r.O);
            }
            run_n += __shfl(in_n, 63, 64); run_e += __shfl(in_e, 63, 64); run_o += __shfl(in_o, 63, 64);
            tn += r.N; te += r.E; to += r.O;
        }
        tn = ed_wave_sum(tn); te = ed_wave_sum(te); to = ed_wave_sum(to);
        bad_index = __ballot(bad_index) != 0ull;
        bad_store = __ballot(bad_store) != 0ull;
        const bool ok = !bad_store && tn == p.total_nodes && te == p.total_edges && to == p.total_obs;
        if (lane == 0) {
            sh[0] = ok ? 1 : 0;
            const int bits = (bad_index ? kEdBadIndex : 0) | (ok ? 0 : kEdBadGather);
            if (g == 0 && bits != 0) st.status[0] = st.status[0] | bits;
        }
    }
    __syncthreads();
    if (sh[0] == 0) return;
    const int C = st.C, S = st.S, N = sh[4], E = sh[5], O = sh[6];
    const long long sn = (long long)sh[1] * C, dn = (long long)sh[7] * C;
    const long long se = sh[2], de = sh[8];
    const long long so = (long long)sh[3] * S, dob = (long long)sh[9] * S;
    // validated by the scan: every row read lies inside the store, every row written inside the caller's arrays
    for (long long e = tid; e < (long long)N * C; e += kEdThreads) {
        p.v[dn + e] = st.v[sn + e];
        p.points64[dn + e] = st.points64[sn + e];
    }
    for (long long e = tid; e < E; e += kEdThreads) {
        p.edge_index[de + e] = st.edge_index[se + e];
        p.edge_index[(long long)p.total_edges + de + e] = st.edge_index[(long long)st.total_edges + se + e];
        p.edge_free[de + e] = st.edge_free[se + e];
        p.edge_cost[de + e] = st.edge_cost[se + e];
    }
    for (long long e = tid; e < (long long)O * S; e += kEdThreads) p.obstacles[dob + e] = st.obstacles[so + e];
    if (tid == 0) {
        if (g == 0) { p.node_ptr[0] = 0; p.edge_ptr[0] = 0; p.obs_ptr[0] = 0; }
        p.node_ptr[g + 1] = sh[7] + N; p.edge_ptr[g + 1] = sh[8] + E; p.obs_ptr[g + 1] = sh[9] + O;
    }
}

__device__ __forceinline__ float fl_wave_max(float x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmaxf(x, __shfl_xor(x, off, 64));
    return x;
}
__device__ __forceinline__ double fl_wave_sum(double x) {           // a fixed butterfly: the same order in every launch
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = x + __shfl_xor(x, off, 64);
    return x;
}

__global__ __launch_bounds__(64) void episode_frontier_loss_kernel(EpisodeFrontierLossParams p) {
    __shared__ int cnt[kFlCap];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long e0 = p.edge_ptr[b], e1 = p.edge_ptr[b + 1];
    int bits = 0;
    bool counted = false;
    const bool range_ok = e0 >= 0 && e1 >= e0 && e1 <= p.total_edges;
    const long long E = e1 - e0;
    const long long base = 2 * e0 + b;                            // the start of problem b's slot in frontier
    const int n = p.frontier_len[b], lab = p.label[b];
    long long el = -1;                                             // the label's edge
    if (!range_ok) {
        bits |= kFlBadRange;
    } else if (p.status[b] == 0 && n != 0 && lab >= 0) {
        if (n < 0 || n > 2 * E + 1 || lab >= n) {
            bits |= kFlBadEntry;
        } else if (E > kFlCap) {
            bits |= kFlTooLarge;
        } else {
            el = p.frontier[base + lab];
            if (el < e0 || el >= e1) bits |= kFlBadEntry; else counted = true;
        }
    }
    // everything above is the same in every lane
    if (!counted) {
        if (range_ok)
            for (long long j = lane; j < E; j += 64) p.dscores[e0 + j] = 0.0f;
        if (lane == 0) {
            p.terms[b] = 0.0f;
            p.counted[b] = 0;
            if (bits != 0) atomicOr(p.bad, bits);
        }
        return;
    }
    for (int j = lane; j < (int)E; j += 64) cnt[j] = 0;
    __syncthreads();
    // (1) the maximum over the list and the count of every edge
    float m = -INFINITY;
    bool bad_entry = false;
    for (int k = lane; k < n; k += 64) {
        const long long e = p.frontier[base + k];
        if (e < e0 || e >= e1) { bad_entry = true; continue; }
        m = fmaxf(m, p.scores[e]);
        atomicAdd(&cnt[(int)(e - e0)], 1);
    }
    m = fl_wave_max(m);                                           // finite: the label's entry is in range
    if (__ballot(bad_entry) != 0ull) bits |= kFlBadEntry;
    // (2) the sum over the list, lane l its entries in ascending order, then the butterfly
    double part = 0.0;
    for (int k = lane; k < n; k += 64) {
        const long long e = p.frontier[base + k];
        if (e < e0 || e >= e1) continue;
        part = part + exp((double)p.scores[e] - (double)m);
    }
    const double sum = fl_wave_sum(part);
    __syncthreads();
    // (3) the gradient over the problem's edges
    for (int j = lane; j < (int)E; j += 64) {
        const int c = cnt[j];
        float d = 0.0f;
        if (c > 0) {
            const double soft = (double)c * exp((double)p.scores[e0 + j] - (double)m) / sum;
            d = (float)((e0 + j == el ? soft - 1.0 : soft) / p.divisor);
        }
        p.dscores[e0 + j] = d;
    }
    if (lane == 0) {
        p.terms[b] = (float)(log(sum) - ((double)p.scores[el] - (double)m));
        p.counted[b] = 1;
        if (bits != 0) atomicOr(p.bad, bits);
    }
}

__global__ __launch_bounds__(64) void episode_frontier_loss_sum_kernel(EpisodeFrontierLossParams p) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double total = 0.0;
    for (int b = 0; b < p.B; ++b) total = total + (double)p.terms[b];
    p.loss[0] = (float)(total / p.divisor);
}

}  // namespace

hipError_t launch_episode_dataset_gather(const EpisodeDatasetStore& st, const EpisodeGatherParams& p, hipStream_t stream) {
    if (p.G <= 0) return hipSuccess;
    hipLaunchKernelGGL(episode_dataset_gather_kernel, dim3(p.G), dim3(kEdThreads), 0, stream, st, p);
    return hipGetLastError();
}

hipError_t launch_episode_frontier_loss(const EpisodeFrontierLossParams& p, hipStream_t stream) {
    if (p.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(episode_frontier_loss_kernel, dim3(p.B), dim3(64), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(episode_frontier_loss_sum_kernel, dim3(1), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace gnnmp
