// rrtstar_kernels.hip -- the RRT* baseline planner for batches of maze problems, every problem on its own sample stream:
// NEXT_plan(env, model=None, T, g_explore_eps=1., stop_when_success) of algorithm/tsa.py:12-139, 222-281 over
// algorithm/search_tree.py:5-98 and environment/maze_env.py:127-208, 266-347 -- what eval_rrt.py runs.  One wave per problem,
// the whole t_max loop in one launch; no wave ever waits on another workgroup, no atomics.  Per iteration:
//   sample     1 or 2 + DIM raw doubles of the problem's block: rand() < 0.05 -> the goal state, else one more dropped and
//              low + (high - low) * d per coordinate (tsa.py:47-56, maze_env.py:131);
//   nearest    over the NON-TERMINAL nodes (free, not in the goal region): each lane owns nodes lane, lane + 64, ..., a wave
//              minimum of (distance bits, id) = np.argmin's first minimum;
//   steer      the sample itself within RRT_EPS, else interpolate(nearest, sample, RRT_EPS / dist) (tsa.py:97-101);
//   step       clip / wrap, _edge_fp(nearest, new) with every in-bounds point query counted, and for a free edge the goal
//              test, which counts one more _state_fp(new) within RRT_EPS of the goal (maze_env.py:181-208).  Point robot: the
//              stackless bisection walk, the same in every lane; stick robot: the K interpolated sticks over the 64 lanes;
//   insert     EVERY new state joins the tree, collided ones too (search_tree.py:65-81);
//   rewire     RRTS_rewire_last: a collided newest node gets cost 2.  Otherwise the distances to ALL earlier nodes go to the
//              lanes 64 at a time, near = d < 3 RRT_EPS; pass 1 walks the free near nodes that beat the minimum at the start
//              of their group in index order (ballot, lowest bit first) against the RUNNING minimum, one edge check each
//              (the minimum only falls, so a node that fails the test at the start of its group fails it later too); pass 2
//              checks every near node -- collided ones included, their cost is 2 -- that the new node would improve: point
//              robot one candidate per lane (the checks are independent, their counts add up), stick robot one candidate at
//              a time over the lanes.  A node that improves gets its cost and rewired parent; descendants keep their costs.
// Node state (coordinates, cost, flags: 8 DIM + 9 bytes a node) lives in LDS up to kRrtLdsNodes nodes and in the caller's
// workspace beyond it.  Loop bounds: t_max iterations; ceil(n / 64) groups of at most 64 candidates per pass; the bisection
// walk has at most 2^level nodes per level with level <= kMzMaxLevel (maze_f64.hpp); K = int(d / 0.015) <= 190 because both
// ends passed _valid_state (d <= sqrt(4 + 4 + 0.16)); the path walk stops after n nodes (status bit 2).
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "maze_f64.hpp"
#include "rrt_tree.hpp"

// numpy rounds every float64 operation on its own
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kRrtLdsNodes = 1024;       // t_max + 1 <= this: 33 KB (stick) of node state per wave next to the 4 KB map

template <bool LDS, int DIM>
__device__ __forceinline__ void rrt_body(const RrtParams& p, double* s_x, double* s_y, double* s_z, double* s_c, unsigned char* s_f,
                                         unsigned char* occ) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T1 = p.t_max + 1;
    const size_t row = (size_t)b * T1;
    double* nx = LDS ? s_x : p.ws_x + row;
    double* ny = LDS ? s_y : p.ws_y + row;
    double* nz = LDS ? s_z : p.ws_z + row;                       // (unused for the point robot)
    double* nc = LDS ? s_c : p.ws_c + row;
    unsigned char* nf = LDS ? s_f : p.ws_f + row;
    int* parents = p.parents + row;
    int* rewired = p.rewired + row;
    double* plen_out = p.path_lengths + row;
    long long* cum = p.cum_checks + row;
    const double* draws = p.draws + (size_t)b * p.draw_len;
    const MzMaze m = mz_maze(p.maps + (size_t)b * p.w * p.w, p.w, occ, lane);
    double goal[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < DIM; ++c) goal[c] = p.goal_states[(size_t)b * DIM + c];
    if (lane == 0) {                                             // search_tree.py:7-15
        nx[0] = p.init_states[(size_t)b * DIM];
        ny[0] = p.init_states[(size_t)b * DIM + 1];
        if (DIM == 3) nz[0] = p.init_states[(size_t)b * DIM + 2];
        nc[0] = 0.0;
        nf[0] = kRrtFree;
        parents[0] = -1; rewired[0] = -1; plen_out[0] = -1.0; cum[0] = 0;
    }
    wave_sync();
    const RrtNodes<DIM> tree{nx, ny, nz, nc, nf};
    int n = 1, status = 0, last_i = -1;
    long long checks = 0, pos = 0;
    bool success = false;
    double plen = -1.0;
    for (int it = 0; it < p.t_max; ++it) {
        // ---- the sample
        double smp[3] = {0.0, 0.0, 0.0};
        if (pos + 1 > p.draw_len) { status |= 1; break; }
        if (draws[pos] < kRrtModelEps) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) smp[c] = goal[c];
            pos += 1;
        } else {
            if (pos + 2 + DIM > p.draw_len) { status |= 1; break; }
            smp[0] = -1.0 + 2.0 * draws[pos + 2];
            smp[1] = -1.0 + 2.0 * draws[pos + 3];
            if (DIM == 3) smp[2] = -0.4 + 0.8 * draws[pos + 4];
            pos += 2 + DIM;
        }
        // ---- nearest non-terminal node, RRT_steer, then step's clip and wrap
        double dmin, near[3], nw[3] = {0.0, 0.0, 0.0};
        const int ni = rrt_nearest<DIM>(tree, n, lane, smp, dmin);
        tree.get(ni, near);
        rrt_steer<DIM>(near, smp, dmin, nw);
        rrt_clip<DIM>(nw);
        const bool near_goal = rrt_dist<DIM>(nw, goal) < kRrtEps;
        const bool fr = rrt_step<DIM>(m, lane, near, nw, near_goal, checks);
        const bool done = fr && near_goal;                       // (_state_fp(new) holds: the free edge checked it)
        success = success || done;
        // ---- insert_new_state
        if (lane == 0) {
            nx[n] = nw[0]; ny[n] = nw[1];
            if (DIM == 3) nz[n] = nw[2];
            nf[n] = (unsigned char)((fr ? kRrtFree : 0) | (done ? kRrtGoal : 0));
            nc[n] = kRrtObsCost;                                 // a collided node's cost; a free one's is set below
            parents[n] = ni; rewired[n] = ni;
        }
        if (fr) rrt_rewire<DIM>(m, lane, tree, rewired, n, ni, near, nw, near_goal, done, plen, checks);      // RRTS_rewire_last
        if (lane == 0) { plen_out[n] = plen; cum[n] = checks; }
        ++n;
        last_i = it;
        wave_sync();
        if (success && p.stop) break;
    }
    // ---- the tree comes out; search_tree.path(): from the last node along rewired_parents to the root
    double* states = p.states + row * DIM;
    for (int j = lane; j < n; j += 64) {
        states[(size_t)j * DIM] = nx[j];
        states[(size_t)j * DIM + 1] = ny[j];
        if (DIM == 3) states[(size_t)j * DIM + 2] = nz[j];
        p.costs[row + j] = nc[j];
        p.flags[row + j] = nf[j];
    }
    if (lane == 0) {
        bool cycle;
        const int L = rrt_path(nf, rewired, n, p.path + row, cycle);
        if (cycle) status |= 2;                                  // the reference would not return
        p.n_nodes[b] = n;
        p.success[b] = success ? 1 : 0;
        p.last_iter[b] = last_i;
        p.used[b] = (int)pos;
        p.path_len[b] = L;
        p.status[b] = status;
    }
}

}  // namespace

// LDS: the node state of trees up to kRrtLdsNodes nodes; otherwise it lives in the workspace and only the map is staged
template <bool LDS, int DIM>
__global__ __launch_bounds__(64) void rrtstar_plan_kernel(RrtParams p) {
    constexpr int kNodes = LDS ? kRrtLdsNodes : 1;
    __shared__ double s_x[kNodes], s_y[kNodes], s_z[DIM == 3 ? kNodes : 1], s_c[kNodes];
    __shared__ unsigned char s_f[kNodes];
    __shared__ unsigned char occ[kMzLdsCells];
    rrt_body<LDS, DIM>(p, s_x, s_y, s_z, s_c, s_f, occ);
}

hipError_t launch_rrtstar_plan(const RrtParams& p, hipStream_t st) {
    if (p.B <= 0) return hipSuccess;
    const bool lds = (long long)p.t_max + 1 <= kRrtLdsNodes;
    if (p.dim == 3) {
        if (lds) hipLaunchKernelGGL((rrtstar_plan_kernel<true, 3>), dim3(p.B), dim3(64), 0, st, p);
        else hipLaunchKernelGGL((rrtstar_plan_kernel<false, 3>), dim3(p.B), dim3(64), 0, st, p);
    } else {
        if (lds) hipLaunchKernelGGL((rrtstar_plan_kernel<true, 2>), dim3(p.B), dim3(64), 0, st, p);
        else hipLaunchKernelGGL((rrtstar_plan_kernel<false, 2>), dim3(p.B), dim3(64), 0, st, p);
    }
    return hipGetLastError();
}

int rrtstar_lds_nodes() { return kRrtLdsNodes; }

}  // namespace gnnmp
