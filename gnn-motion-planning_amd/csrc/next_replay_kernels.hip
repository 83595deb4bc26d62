// next_replay_kernels.hip -- the replay of NEXT's training loop on the device (train_next.py:25-68, 88-108): the store of
// (problem, path) samples with get_label's actions and values, filled straight from the trees of gnnmp_next_plan or from packed
// paths, and the loss train() differentiates with its gradient with respect to the network's output.
//
//   next_replay_scan_kernel<TREES>   one wave.  The ONE exclusive scan of an append call: the source paths in ascending source
//       index get consecutive path slots and state offsets behind counts[].  Pass 1 sums the paths and states the call would add
//       and validates the source; when they do not fit (status bit 1) or the source is malformed (bit 2) NOTHING else is
//       written.  Pass 2 writes path_ptr[slot + 1], parks the SOURCE index of every new path in problem[slot], records
//       {first slot, first state, new paths, new states} in pending[] and moves counts[].  Integers only; no atomics.
//   next_replay_label_kernel<TREES, DIM>   one wave per new path (waves beyond pending[2] leave at once).  Copies the path's
//       float64 rows (trees: states[b, path[b, j]]; packed: paths64[ptr[p] + j]), their float32 roundings, and runs get_label
//       in float64: the edge cost is np.linalg.norm(next - prev) (mz_cost: the fused dot product of numpy's BLAS), the action
//       interpolate(prev, next, RRT_EPS / edge) - prev when edge > RRT_EPS (rrt_steer's interpolation: the stick robot wraps the
//       orientation gap and the result by one period) and next - prev otherwise, zero for the last state; the running cost is ONE
//       serial left-to-right chain, cost[k + 1] = cost[k] + edge[k], carried across the 64-row chunks in a register every lane
//       holds, and value[k] = cost[k] - cost[last].  The chain runs twice (first for cost[last], then for the values): no
//       buffer, the same additions, the same bits.  Everything is rounded to float32 once, at the store.  Last, lane 0
//       replaces the parked source index in problem[slot] by problem_ids[source].
//   next_path_loss_kernel<DIM>   one wave per path of a group: term_value = mean_s (values - y[:, dim])^2 and term_action =
//       mean_{s, j} (actions - y[:, :dim])^2, every sum ONE ascending chain in double (rows ascending, columns ascending inside
//       a row), and dy = the gradient of (sum of all terms) / divisor with respect to y, rounded to float32 once.
//   next_path_loss_sum_kernel   one lane: loss = (((0 + v_0) + a_0) + v_1) + ... / divisor, train()'s own order, in double.
//
// No floating-point atomics, no LDS, no scratch; every launch is on the caller's stream and nothing is allocated or waited for.
// Two runs give the same bits.
//
// Bounds (every guard of these kernels):
//   * scan: counts[] outside [0, cap] -> bit 2, nothing written.  Trees: a path_len outside [0, t_max + 1] -> bit 2; a problem
//     with success == 0 or path_len == 0 adds nothing.  Packed: path_ptr[0] != 0, path_ptr[P] != n_states or a path with fewer
//     than one state -> bit 2.  The sums are 64-bit; the fit test is counts + new <= cap for paths and for states.
//   * label: a wave at or beyond pending[2] returns before reading anything.  Every destination row lies in
//     [pending[1], pending[1] + pending[3]) <= cap_states by the scan's test.  Trees: a node id outside [0, t_max] sets status bit
//     4, is not read, and its row is stored as zeros.  Packed rows lie in [0, n_states) by the scan's validation.
//   * the chunk loops run ceil(len / 64) times with all 64 lanes; lanes beyond the path compute on zeros and store nothing.
//   * path loss: a path with ptr[g] < 0, ptr[g + 1] > n_states or no rows reads and writes no row; its terms are NaN (the mean
//     over nothing).  Rows of dy outside every path are not written.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "wave64.hpp"
#include "maze_f64.hpp"
#include "rrt_tree.hpp"

// numpy rounds every float64 operation on its own; the one fused chain is the dot product of np.linalg.norm (mz_cost)
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kReplayFull = 1, kReplayBadSource = 2, kReplayBadNode = 4;

__device__ __forceinline__ long long wave_sum_ll(long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}
__device__ __forceinline__ bool wave_any(bool x) { return __ballot(x) != 0ull; }

// the states source path i of an append call adds (0: none), `bad` raised for a malformed source
template <bool TREES>
__device__ __forceinline__ int replay_src_len(const NextReplaySrc& s, int i, bool& bad) {
    if (TREES) {
        const int pl = s.path_len[i];
        if (pl < 0 || pl > s.t1) { bad = true; return 0; }
        return s.success[i] != 0 ? pl : 0;
    }
    const long long len = (long long)s.ptr[i + 1] - (long long)s.ptr[i];
    if (len < 1 || len > s.n_rows) { bad = true; return 0; }
    return (int)len;
}

template <bool TREES>
__global__ __launch_bounds__(64) void next_replay_scan_kernel(NextReplayStore st, NextReplaySrc s) {
    const int lane = threadIdx.x;
    const int P0 = st.counts[0], S0 = st.counts[1];
    bool bad = P0 < 0 || P0 > st.cap_paths || S0 < 0 || S0 > st.cap_states;
    if (!TREES) bad = bad || s.ptr[0] != 0 || (long long)s.ptr[s.n] != s.n_rows;
    long long np = 0, ns = 0;
    for (int base = 0; base < s.n; base += 64) {
        const int i = base + lane;
        const int len = i < s.n ? replay_src_len<TREES>(s, i, bad) : 0;
        np += len > 0;
        ns += len;
    }
    np = wave_sum_ll(np);
    ns = wave_sum_ll(ns);
    bad = wave_any(bad);
    const bool fit = !bad && (long long)P0 + np <= st.cap_paths && (long long)S0 + ns <= st.cap_states;
    if (!fit) {                                                  // nothing appended: counts and the rows stay as they are
        if (lane == 0) {
            st.status[0] = st.status[0] | (bad ? kReplayBadSource : kReplayFull);
            st.pending[0] = P0; st.pending[1] = S0; st.pending[2] = 0; st.pending[3] = 0;
        }
        return;
    }
    int run_p = P0, run_s = S0;
    for (int base = 0; base < s.n; base += 64) {
        const int i = base + lane;
        bool unused = false;
        const int len = i < s.n ? replay_src_len<TREES>(s, i, unused) : 0;
        const unsigned long long take = __ballot(len > 0);
        const int pre_p = __builtin_popcountll(take & ((1ull << lane) - 1ull));
        int incl = len;                                          // inclusive prefix sum of len over the lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (len > 0) {
            const int slot = run_p + pre_p;
            st.path_ptr[slot + 1] = run_s + incl;
            st.problem[slot] = i;                                // the source index, until the label kernel has read it
        }
        run_p += __builtin_popcountll(take);
        run_s += __shfl(incl, 63, 64);
    }
    if (lane == 0) {
        st.pending[0] = P0; st.pending[1] = S0; st.pending[2] = (int)np; st.pending[3] = (int)ns;
        if (np > 0) {
            st.path_ptr[P0] = S0;
            st.counts[0] = P0 + (int)np;
            st.counts[1] = S0 + (int)ns;
        }
    }
}

// row j of source path `src` -> q; false (q = 0) for a node id outside the tree
template <bool TREES, int DIM>
__device__ __forceinline__ bool replay_row(const NextReplaySrc& s, int src, int j, double* q) {
    long long row;
    if (TREES) {
        const int id = s.path[(long long)src * s.t1 + j];
        if (id < 0 || id >= s.t1) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) q[c] = 0.0;
            return false;
        }
        row = (long long)src * s.t1 + id;
    } else {
        row = (long long)s.ptr[src] + j;
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) q[c] = s.rows[row * DIM + c];
    return true;
}

// lane i's value of x in every lane (i the same in every lane)
__device__ __forceinline__ double lane_value(double x, int i) {
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, i);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), i);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// the edge costs of a chunk of `rows` rows (1 .. 64) added to the running cost in lane order, `n_edges` of them: -> this lane's
// cost BEFORE its own edge
__device__ __forceinline__ double replay_chain(double edge, int rows, int n_edges, int lane, double& run) {
    double mine = 0.0;
    for (int i = 0; i < rows; ++i) {
        if (lane == i) mine = run;
        if (i < n_edges) run = run + lane_value(edge, i);
    }
    return mine;
}

template <bool TREES, int DIM>
__global__ __launch_bounds__(64) void next_replay_label_kernel(NextReplayStore st, NextReplaySrc s) {
    const int lane = threadIdx.x, w = blockIdx.x;
    if (w >= st.pending[2]) return;
    const int slot = st.pending[0] + w;
    const int src = st.problem[slot];
    const int d0 = st.path_ptr[slot];
    const int len = st.path_ptr[slot + 1] - d0;
    bool bad_node = false;
    // pass 1: cost[last], the chain alone
    double total = 0.0;
    for (int base = 0; base < len; base += 64) {
        const int r = base + lane;
        double edge = 0.0;
        if (r < len - 1) {
            double prev[DIM], next[DIM];
            replay_row<TREES, DIM>(s, src, r, prev);
            replay_row<TREES, DIM>(s, src, r + 1, next);
            edge = mz_cost<DIM>(prev, next);
        }
        replay_chain(edge, len - base < 64 ? len - base : 64, len - 1 - base, lane, total);
    }
    // pass 2: the rows, the actions, and the same chain again for the values
    double run = 0.0;
    for (int base = 0; base < len; base += 64) {
        const int r = base + lane;
        double prev[DIM], act[DIM], edge = 0.0;
#pragma unroll
        for (int c = 0; c < DIM; ++c) { prev[c] = 0.0; act[c] = 0.0; }
        if (r < len) bad_node = !replay_row<TREES, DIM>(s, src, r, prev) || bad_node;
        if (r < len - 1) {
            double next[DIM];
            replay_row<TREES, DIM>(s, src, r + 1, next);
            edge = mz_cost<DIM>(prev, next);
            if (edge > kRrtEps) {
                double nw[DIM];
                rrt_steer<DIM>(prev, next, edge, nw);            // edge >= RRT_EPS: its interpolate branch
#pragma unroll
                for (int c = 0; c < DIM; ++c) act[c] = nw[c] - prev[c];
            } else {
#pragma unroll
                for (int c = 0; c < DIM; ++c) act[c] = next[c] - prev[c];
            }
        }
        const double cost = replay_chain(edge, len - base < 64 ? len - base : 64, len - 1 - base, lane, run);
        if (r < len) {
            const long long o = (long long)(d0 + r);
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                st.states64[o * DIM + c] = prev[c];
                st.states32[o * DIM + c] = (float)prev[c];
                st.actions[o * DIM + c] = (float)act[c];
            }
            st.values[o] = (float)(cost - total);
        }
    }
    if (bad_node) atomicOr(st.status, kReplayBadNode);
    if (lane == 0) st.problem[slot] = s.problem_ids[src];
}

template <int DIM>
__global__ __launch_bounds__(64) void next_path_loss_kernel(NextPathLossParams p) {
    const int lane = threadIdx.x, g = blockIdx.x;
    const int a = p.ptr[g], b = p.ptr[g + 1];
    const int n = b - a;
    if (a < 0 || b > p.S || n <= 0) {
        if (lane == 0 && p.terms) p.terms[2 * g] = p.terms[2 * g + 1] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double den_v = (double)n * (double)p.divisor, den_a = (double)n * (double)DIM * (double)p.divisor;
    double sum_v = 0.0, sum_a = 0.0;
    for (int base = 0; base < n; base += 64) {
        const int r = base + lane;
        double sq_v = 0.0, sq_a[DIM];
#pragma unroll
        for (int c = 0; c < DIM; ++c) sq_a[c] = 0.0;
        if (r < n) {
            const long long o = (long long)(a + r);
            const double dv = (double)p.values[o] - (double)p.y[o * (DIM + 1) + DIM];
            sq_v = dv * dv;
            if (p.dy) p.dy[o * (DIM + 1) + DIM] = (float)(-2.0 * dv / den_v);
#pragma unroll
            for (int c = 0; c < DIM; ++c) {
                const double da = (double)p.actions[o * DIM + c] - (double)p.y[o * (DIM + 1) + c];
                sq_a[c] = da * da;
                if (p.dy) p.dy[o * (DIM + 1) + c] = (float)(-2.0 * da / den_a);
            }
        }
        const int cnt = n - base < 64 ? n - base : 64;
        for (int i = 0; i < cnt; ++i) {
            sum_v = sum_v + lane_value(sq_v, i);
#pragma unroll
            for (int c = 0; c < DIM; ++c) sum_a = sum_a + lane_value(sq_a[c], i);
        }
    }
    if (lane == 0 && p.terms) {
        p.terms[2 * g] = sum_v / (double)n;
        p.terms[2 * g + 1] = sum_a / ((double)n * (double)DIM);
    }
}

__global__ __launch_bounds__(64) void next_path_loss_sum_kernel(NextPathLossParams p) {
    if (threadIdx.x != 0) return;
    double total = 0.0;
    for (int g = 0; g < p.G; ++g) total = (total + p.terms[2 * g]) + p.terms[2 * g + 1];
    p.loss[0] = total / (double)p.divisor;
}

template <bool TREES>
hipError_t replay_append(const NextReplayStore& st, const NextReplaySrc& s, hipStream_t stream) {
    hipLaunchKernelGGL((next_replay_scan_kernel<TREES>), dim3(1), dim3(64), 0, stream, st, s);
    if (st.dim == 3) hipLaunchKernelGGL((next_replay_label_kernel<TREES, 3>), dim3(s.n), dim3(64), 0, stream, st, s);
    else hipLaunchKernelGGL((next_replay_label_kernel<TREES, 2>), dim3(s.n), dim3(64), 0, stream, st, s);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_next_replay_append(const NextReplayStore& st, const NextReplaySrc& s, bool trees, hipStream_t stream) {
    if (s.n <= 0) return hipSuccess;
    return trees ? replay_append<true>(st, s, stream) : replay_append<false>(st, s, stream);
}

hipError_t launch_next_path_loss(const NextPathLossParams& p, hipStream_t stream) {
    if (p.G <= 0 || (!p.terms && !p.dy)) return hipSuccess;
    if (p.dim == 3) hipLaunchKernelGGL((next_path_loss_kernel<3>), dim3(p.G), dim3(64), 0, stream, p);
    else hipLaunchKernelGGL((next_path_loss_kernel<2>), dim3(p.G), dim3(64), 0, stream, p);
    if (p.loss) hipLaunchKernelGGL(next_path_loss_sum_kernel, dim3(1), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace gnnmp
