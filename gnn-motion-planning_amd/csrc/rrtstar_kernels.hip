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
// walk has at most 2^level nodes per level with level <= kLspMaxLevel (maze_f64.hpp); K = int(d / 0.015) <= 190 because both
// ends passed _valid_state (d <= sqrt(4 + 4 + 0.16)); the path walk stops after n nodes (status bit 2).
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "maze_f64.hpp"

// numpy rounds every float64 operation on its own
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kRrtLdsNodes = 1024;       // t_max + 1 <= this: 33 KB (stick) of node state per wave next to the 4 KB map
constexpr double kRrtEps = 5e-2;         // env_config.py RRT_EPS: steering step and goal radius
constexpr double kRrtModelEps = 0.05;    // tsa.py:13 model_eps
constexpr double kRrtNearR = 5e-2 * 3;   // tsa.py:234 env.RRT_EPS * 3, rounded as Python rounds it
constexpr double kRrtObsCost = 2.0;      // tsa.py:222 obs_cost
constexpr unsigned char kRrtFree = 1, kRrtGoal = 2;

// env.distance: |b - a| per coordinate, the orientation gap the short way round, sqrt((dx^2 + dy^2) + dz^2)
template <int DIM>
__device__ __forceinline__ double rrt_dist(const double* a, const double* b) {
    const double a0 = fabs(b[0] - a[0]), a1 = fabs(b[1] - a[1]);
    double s = a0 * a0 + a1 * a1;
    if (DIM == 3) {
        double a2 = fabs(b[2] - a[2]);
        const double w2 = fabs(a2 - 0.8);
        a2 = w2 < a2 ? w2 : a2;                                  // np.min((d, |d - 0.8|))
        s = s + a2 * a2;
    }
    return sqrt(s);
}
__device__ __forceinline__ double rrt_wrap(double z) {           // maze_env.py:155-159: one period back into [-0.4, 0.4]
    if (fabs(z) > 0.4) z = z > 0.0 ? z - 0.8 : z + 0.8;
    return z;
}
// env.step(s, new_state = t) by all 64 lanes, s and t the same in every lane (t already clipped and wrapped): -> no_collision,
// the same in every lane; `checks` grows by what the call counts, the goal test of a free edge included.
template <int DIM>
__device__ __forceinline__ bool rrt_step(const LspMaze& m, int lane, const double* s, const double* t, bool near_goal, long long& checks) {
    bool fr;
    if (DIM == 2) {
        int cnt = 0;
        fr = lsp_edge2(m, s[0], s[1], t[0], t[1], cnt);
        if (fr && near_goal) lsp_point(m, t[0], t[1], cnt);
        checks += cnt;
    } else {
        fr = lsp_stick_edge_wave(m, lane, s, t, checks);
        if (fr && near_goal) {
            int cnt = 0;
            lsp_stick(m, t[0], t[1], t[2], cnt);
            checks += cnt;
        }
    }
    return fr;
}

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
    const LspMaze m = lsp_maze(p.maps + (size_t)b * p.w * p.w, p.w, occ, lane);
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
    lsp_sync();
    auto node = [&](int j, double* out) {
        out[0] = nx[j]; out[1] = ny[j];
        if (DIM == 3) out[2] = nz[j];
    };
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
        // ---- nearest non-terminal node
        unsigned long long best = ~0ull;
        int bi = 0x7fffffff;
        for (int j = lane; j < n; j += 64) {
            if (nf[j] != kRrtFree) continue;
            double q[3];
            node(j, q);
            const unsigned long long k = (unsigned long long)__double_as_longlong(rrt_dist<DIM>(q, smp));      // d >= 0: bit order
            if (k < best) { best = k; bi = j; }                  // ascending ids: the first strict minimum
        }
        const unsigned long long wmin = lsp_wave_min_u64(best);
        const int ni = (int)lsp_wave_min_u64(best == wmin ? (unsigned long long)(unsigned)bi : ~0ull);
        const double dmin = __longlong_as_double((long long)wmin);
        double near[3], nw[3] = {0.0, 0.0, 0.0};
        node(ni, near);
        // ---- RRT_steer, then step's clip and wrap
        if (dmin < kRrtEps) {
#pragma unroll
            for (int c = 0; c < DIM; ++c) nw[c] = smp[c];
        } else {
            const double ratio = kRrtEps / dmin;
            nw[0] = near[0] + (smp[0] - near[0]) * ratio;
            nw[1] = near[1] + (smp[1] - near[1]) * ratio;
            if (DIM == 3) nw[2] = rrt_wrap(near[2] + rrt_wrap(smp[2] - near[2]) * ratio);
        }
        nw[0] = fmin(fmax(nw[0], -1.0), 1.0);
        nw[1] = fmin(fmax(nw[1], -1.0), 1.0);
        if (DIM == 3) nw[2] = rrt_wrap(nw[2]);
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
        if (fr) {
            // ---- RRTS_rewire_last, pass 1: the cheapest free neighbour with a free edge becomes the parent
            double min_cost = rrt_dist<DIM>(near, nw) + nc[ni];
            int min_j = ni;
            for (int base = 0; base < n; base += 64) {
                const int j = base + lane;
                bool cand = false;
                if (j < n && (nf[j] & kRrtFree)) {
                    double q[3];
                    node(j, q);
                    const double d = rrt_dist<DIM>(q, nw);
                    cand = d < kRrtNearR && d + nc[j] < min_cost;
                }
                unsigned long long todo = __builtin_amdgcn_ballot_w64(cand);
                while (todo) {                                   // at most 64 bits, lowest index first
                    const int jj = base + __builtin_ctzll(todo);
                    todo &= todo - 1;
                    double q[3];
                    node(jj, q);
                    const double cost_new = rrt_dist<DIM>(q, nw) + nc[jj];
                    if (cost_new < min_cost && rrt_step<DIM>(m, lane, q, nw, near_goal, checks)) { min_cost = cost_new; min_j = jj; }
                }
            }
            if (done && (plen < 0.0 || plen > min_cost)) plen = min_cost;      // set_cost (search_tree.py:56-63)
            // ---- pass 2: every near node the new one improves, collided ones included
            for (int base = 0; base < n; base += 64) {
                const int j = base + lane;
                bool cand = false;
                double q[3] = {0.0, 0.0, 0.0}, cost_new = 0.0;
                if (j < n) {
                    node(j, q);
                    const double d = rrt_dist<DIM>(q, nw);
                    cost_new = min_cost + d;
                    cand = d < kRrtNearR && cost_new < nc[j];
                }
                if (DIM == 2) {
                    int cnt = 0;
                    if (cand) {
                        const bool ok = lsp_edge2(m, q[0], q[1], nw[0], nw[1], cnt);
                        if (ok && near_goal) lsp_point(m, nw[0], nw[1], cnt);
                        if (ok) { nc[j] = cost_new; rewired[j] = n; }
                    }
                    checks += lsp_wave_sum(cnt);
                } else {
                    unsigned long long todo = __builtin_amdgcn_ballot_w64(cand);
                    while (todo) {
                        const int src = __builtin_ctzll(todo), jj = base + src;
                        todo &= todo - 1;
                        double qq[3];
                        node(jj, qq);
                        const bool ok = rrt_step<DIM>(m, lane, qq, nw, near_goal, checks);
                        if (ok && lane == src) { nc[j] = cost_new; rewired[j] = n; }
                    }
                }
            }
            if (lane == 0) { nc[n] = min_cost; rewired[n] = min_j; }
        }
        if (lane == 0) { plen_out[n] = plen; cum[n] = checks; }
        ++n;
        last_i = it;
        lsp_sync();
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
        int L = 0;
        if (nf[n - 1] & kRrtGoal) {
            int cur = n - 1;
            L = 1;
            while (cur != 0 && L <= n) {
                cur = rewired[cur];
                if (cur < 0 || cur >= n) { L = n + 1; break; }
                ++L;
            }
            if (L > n) { status |= 2; L = 0; }                   // a cycle: the reference would not return
            int* path = p.path + row;
            cur = n - 1;
            for (int k = L - 1; k >= 0; --k) { path[k] = cur; cur = rewired[cur]; }
        }
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
    __shared__ unsigned char occ[kLspLdsCells];
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
