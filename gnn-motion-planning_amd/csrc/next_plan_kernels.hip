// next_plan_kernels.hip -- NEXT's guided planner for batches of maze problems, every problem on its own streams:
// NEXT_plan(env, model, T, g_explore_eps, stop_when_success, c, k) of algorithm/tsa.py:12-81, 141-220 over
// algorithm/search_tree.py -- what eval_next.py runs -- as gnnmp.next_plan.plan_host restates it.  One workgroup of 256 threads
// (4 waves) per problem, the whole t_max loop in one launch; no wave ever waits on another workgroup, no atomics.  The
// problem's pb_rep (57.6 KB), the node state (coordinates, cost, w: 40 bytes a node, value 4, flags 1; 1024 nodes), the map and
// the network's scratch live in LDS: about 109 KB, one workgroup a CU.  Per iteration:
//   branch     raw double r0 < 0.05 -> the sample is the goal state (1 double); else r1 < g_explore_eps -> the RRT step (2 + DIM
//              doubles), else the guided step (2 doubles).  Goal and RRT step: rrt_tree.hpp's nearest / steer / step by wave 0,
//              exactly rrtstar_plan_kernel's;
//   guided     select = the first maximum over the non-terminal nodes of value + c sqrt(log(w_sum) / w) (all threads, a block
//              arg-max on (score, lowest id)); one network evaluation of the parent -> the action mean; k actions
//              fl32(mean + fl32(scale eps)); candidates parent + action with x, y clipped and the angle wrapped; per candidate
//              one network evaluation (its value) and w over the tree as it stands; the first maximum of the same score; the
//              counted env.step(parent, candidate) by wave 0;
//   insert     EVERY new state joins the tree; one network evaluation gives its value; visits[parent] += 1;
//              w_sum -= w[parent]; w[parent] over the tree INCLUDING the new state; w_sum += w[parent]; w[new] over the same
//              tree; w_sum += w[new] -- three separately rounded operations;
//   rewire     RRTS_rewire_last by wave 0, unchanged.
// Every thread carries the scalar state of the loop (node count, stream position, w_sum, ...) and derives it from values that
// are the same for the whole workgroup (the draws, LDS words written before a barrier), so every branch is uniform and every
// barrier is reached by all 256 threads.  A network evaluation is next_net.hpp's next_state_readout, the body of
// next_state_kernel: a value has the bits gnnmp_next_state_forward gives for that state.  w(s) = sum over the nodes of
// max(exp(-(dist / 0.05)^2), 1e-3): node j goes to thread j % 256, a wave sum, the four waves in order -- fixed.
// Loop bounds: t_max iterations, t_max + 1 <= kNodes and k <= 16 (checked by gnnmp_next_plan); everything else as rrtstar_kernels.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include "kernels.hpp"
#include "maze_f64.hpp"
#include "next_net.hpp"
#include "rrt_tree.hpp"

// numpy rounds every float64 operation on its own (and the two float32 roundings of an action stay two)
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

constexpr int kNodes = 1024;             // t_max + 1 <= this
constexpr int kNpThreads = kStThreads;   // 256: next_state_readout's workgroup

struct NextPlanLds {
    double x[kNodes], y[kNodes], z[kNodes], c[kNodes], w[kNodes];
    NextStateScratch sc;
    double wred[4], sel_s[4], bc[4];
    int sel_i[4], ibc[4];
    float pb[kLat * kCells];
    float sv[kNodes];
    float st[4], yv[4];
    unsigned char f[kNodes];
    unsigned char occ[256];
};
static_assert(sizeof(NextPlanLds) <= 160 * 1024, "one workgroup's LDS");

__device__ __forceinline__ bool not_finite(double v) {           // on the bits: the build does not honour NaNs in comparisons
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

// compute_w(tree[0 .. n), q) for the whole workgroup: the same double in every thread
template <int DIM>
__device__ __forceinline__ double block_w(const RrtNodes<DIM>& t, int n, const double* q, int tid, double* wred) {
    double acc = 0.0;
    for (int j = tid; j < n; j += kNpThreads) {
        double a[3];
        t.get(j, a);
        const double d = rrt_dist<DIM>(a, q) / kRrtEps;
        const double e = exp(-(d * d) * 1.0);
        acc = acc + (e > 1e-3 ? e : 1e-3);
    }
    acc = wave_sum(acc);
    if ((tid & 63) == 0) wred[tid >> 6] = acc;
    __syncthreads();
    const double tot = ((wred[0] + wred[1]) + wred[2]) + wred[3];
    __syncthreads();
    return tot;
}

// the first maximum of (score, id) over the workgroup: the larger score, among equals the lower id
__device__ __forceinline__ void block_argmax(double sc, int id, int tid, NextPlanLds& S, double& best, int& best_id) {
    for (int o = 32; o; o >>= 1) {
        const double os = __shfl_xor(sc, o);
        const int oi = __shfl_xor(id, o);
        if (os > sc || (os == sc && oi < id)) { sc = os; id = oi; }
    }
    if ((tid & 63) == 0) { S.sel_s[tid >> 6] = sc; S.sel_i[tid >> 6] = id; }
    __syncthreads();
    best = S.sel_s[0];
    best_id = S.sel_i[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const double os = S.sel_s[w];
        const int oi = S.sel_i[w];
        if (os > best || (os == best && oi < best_id)) { best = os; best_id = oi; }
    }
    __syncthreads();
}

template <int DIM>
__global__ __launch_bounds__(kNpThreads) void next_plan_kernel(NextPlanParams p) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    NextPlanLds& S = *reinterpret_cast<NextPlanLds*>(lds_raw);
    const RrtParams& q = p.t;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T1 = q.t_max + 1;
    const size_t row = (size_t)b * T1;
    int* parents = q.parents + row;
    int* rewired = q.rewired + row;
    double* plen_out = q.path_lengths + row;
    long long* cum = q.cum_checks + row;
    signed char* by_rrt = p.by_rrt + row;
    int* visits = p.visits + row;
    const double* draws = q.draws + (size_t)b * q.draw_len;
    const float* __restrict__ W = p.weights;
    const float* eps = p.eps + (size_t)b * p.eps_rows * p.k * DIM;
    const double* map = q.maps + (size_t)b * kCells;

    {
        const float* pbg = p.pb_rep + (size_t)b * (kLat * kCells);
        for (int i = tid; i < kLat * kCells; i += kNpThreads) S.pb[i] = pbg[i];
        for (int i = tid; i < kCells; i += kNpThreads) S.occ[i] = map[i] == 0.0 ? 0 : 1;
    }
    const MzMaze m{S.occ, map, kW};
    const RrtNodes<DIM> tree{S.x, S.y, S.z, S.c, S.f};
    double goal[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < DIM; ++c) goal[c] = q.goal_states[(size_t)b * DIM + c];
    if (tid == 0) {                                              // SearchTree.__init__ with a model (search_tree.py:5-28)
        S.x[0] = q.init_states[(size_t)b * DIM];
        S.y[0] = q.init_states[(size_t)b * DIM + 1];
        S.z[0] = DIM == 3 ? q.init_states[(size_t)b * DIM + 2] : 0.0;
        S.c[0] = 0.0;
        S.f[0] = kRrtFree;
        parents[0] = -1; rewired[0] = -1; plen_out[0] = -1.0; cum[0] = 0;
        by_rrt[0] = -1; visits[0] = 1;
        S.st[0] = (float)S.x[0]; S.st[1] = (float)S.y[0];
        if (DIM == 3) S.st[2] = (float)S.z[0];
    }
    __syncthreads();
    next_state_readout(W, S.st, DIM, tid, S.pb, S.sc, S.yv);
    __syncthreads();
    double w_sum;
    {
        double s0[3];
        tree.get(0, s0);
        w_sum = block_w<DIM>(tree, 1, s0, tid, S.wred);
        if (tid == 0) { S.sv[0] = S.yv[DIM]; S.w[0] = w_sum; }
    }
    __syncthreads();

    int n = 1, status = 0, last_i = -1, g = 0;
    long long checks = 0, pos = 0;                               // checks and plen: wave 0's
    bool success = false;
    double plen = -1.0;
    for (int it = 0; it < q.t_max; ++it) {
        // ---- the branch: 0 = the goal state, 1 = a uniform sample, 2 = guided
        if (pos + 1 > q.draw_len) { status |= 1; break; }
        int mode = 0;
        if (!(draws[pos] < kRrtModelEps)) {
            if (pos + 2 > q.draw_len) { status |= 1; break; }
            mode = draws[pos + 1] < p.g_explore_eps ? 1 : 2;
            if (mode == 1 && pos + 2 + DIM > q.draw_len) { status |= 1; break; }
            if (mode == 2 && g >= p.eps_rows) { status |= 4; break; }
        }
        double near[3] = {0.0, 0.0, 0.0}, nw[3] = {0.0, 0.0, 0.0};      // wave 0's until the broadcast
        int ni = 0;
        bool near_goal = false, fr = false;
        if (mode != 2) {
            if (wave == 0) {
                double smp[3] = {0.0, 0.0, 0.0};
                if (mode == 0) {
#pragma unroll
                    for (int c = 0; c < DIM; ++c) smp[c] = goal[c];
                } else {
                    smp[0] = -1.0 + 2.0 * draws[pos + 2];
                    smp[1] = -1.0 + 2.0 * draws[pos + 3];
                    if (DIM == 3) smp[2] = -0.4 + 0.8 * draws[pos + 4];
                }
                double dmin;
                ni = rrt_nearest<DIM>(tree, n, lane, smp, dmin);
                tree.get(ni, near);
                rrt_steer<DIM>(near, smp, dmin, nw);
            }
            pos += mode == 0 ? 1 : 2 + DIM;
        } else {
            // ---- select (tsa.py:141-165)
            double sc = -INFINITY;
            int id = 0x7fffffff;
            const double lw = log(w_sum);
            for (int j = tid; j < n; j += kNpThreads) {
                if (S.f[j] != kRrtFree) continue;
                double v = (double)S.sv[j] + p.c * sqrt(lw / S.w[j]);
                if (not_finite(v)) v = INFINITY;                 // wins, and is reported below
                if (v > sc) { sc = v; id = j; }                  // ascending ids: the first maximum
            }
            double best;
            block_argmax(sc, id, tid, S, best, ni);
            if (not_finite(best) || ni < 0 || ni >= n) { status |= 8; break; }
            double par[3] = {0.0, 0.0, 0.0};
            tree.get(ni, par);
            // ---- expand (tsa.py:167-220): the action mean of the parent, k candidates, their values and weights
            if (tid == 0) {
                S.st[0] = (float)par[0]; S.st[1] = (float)par[1];
                if (DIM == 3) S.st[2] = (float)par[2];
            }
            __syncthreads();
            next_state_readout(W, S.st, DIM, tid, S.pb, S.sc, S.yv);
            __syncthreads();
            float mean[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DIM; ++c) mean[c] = S.yv[c];
            const float* erow = eps + (size_t)g * p.k * DIM;
            double bsc = -INFINITY;
            bool bad = false;
            for (int j = 0; j < p.k; ++j) {
                double cand[3] = {0.0, 0.0, 0.0};
#pragma unroll
                for (int c = 0; c < DIM; ++c) {
                    const float step = p.scale * erow[j * DIM + c];
                    const float a = mean[c] + step;
                    cand[c] = par[c] + (double)a;
                }
                rrt_clip<DIM>(cand);                             // env.step(state, action, check_collision=False)
                double v = 0.0;
                if (p.k > 1) {
                    __syncthreads();                             // the mean / the previous value has been read
                    if (tid == 0) {
                        S.st[0] = (float)cand[0]; S.st[1] = (float)cand[1];
                        if (DIM == 3) S.st[2] = (float)cand[2];
                    }
                    __syncthreads();
                    next_state_readout(W, S.st, DIM, tid, S.pb, S.sc, S.yv);
                    __syncthreads();
                    const double wj = block_w<DIM>(tree, n, cand, tid, S.wred);
                    v = (double)S.yv[DIM] + p.c * sqrt(lw / wj);
                    bad = bad || not_finite(v);
                }
                if (j == 0 || v > bsc) {                         // the first maximum
                    bsc = v;
#pragma unroll
                    for (int c = 0; c < DIM; ++c) nw[c] = cand[c];
                }
            }
            if (bad) { status |= 8; break; }
#pragma unroll
            for (int c = 0; c < DIM; ++c) near[c] = par[c];
            pos += 2;                                            // only now: an iteration given up with a status consumed nothing
            ++g;
        }
        // ---- env.step(parent, new state): wave 0, then everybody learns the outcome
        __syncthreads();
        if (wave == 0) {
            rrt_clip<DIM>(nw);
            near_goal = rrt_dist<DIM>(nw, goal) < kRrtEps;
            fr = rrt_step<DIM>(m, lane, near, nw, near_goal, checks);
            if (lane == 0) {
                S.bc[0] = nw[0]; S.bc[1] = nw[1]; S.bc[2] = nw[2];
                S.ibc[0] = ni; S.ibc[1] = fr ? 1 : 0; S.ibc[2] = near_goal ? 1 : 0;
            }
        }
        __syncthreads();
        nw[0] = S.bc[0]; nw[1] = S.bc[1]; nw[2] = S.bc[2];
        ni = S.ibc[0];
        fr = S.ibc[1] != 0;
        near_goal = S.ibc[2] != 0;
        const bool done = fr && near_goal;                       // (_state_fp(new) holds: the free edge checked it)
        success = success || done;
        // ---- insert_new_state (search_tree.py:65-98)
        const double w_old = S.w[ni];
        if (tid == 0) {
            S.x[n] = nw[0]; S.y[n] = nw[1]; S.z[n] = nw[2];
            S.f[n] = (unsigned char)((fr ? kRrtFree : 0) | (done ? kRrtGoal : 0));
            S.c[n] = kRrtObsCost;                                // a collided node's cost; a free one's is set by the rewiring
            parents[n] = ni; rewired[n] = ni;
            by_rrt[n] = mode == 2 ? 0 : 1;
            visits[ni] += 1;
            visits[n] = 0;
            S.st[0] = (float)nw[0]; S.st[1] = (float)nw[1];
            if (DIM == 3) S.st[2] = (float)nw[2];
        }
        __syncthreads();
        next_state_readout(W, S.st, DIM, tid, S.pb, S.sc, S.yv);
        __syncthreads();
        {
            double par[3] = {0.0, 0.0, 0.0};
            tree.get(ni, par);
            const double wp = block_w<DIM>(tree, n + 1, par, tid, S.wred);
            const double wn = block_w<DIM>(tree, n + 1, nw, tid, S.wred);
            w_sum = w_sum - w_old;
            w_sum = w_sum + wp;
            w_sum = w_sum + wn;
            if (tid == 0) { S.sv[n] = S.yv[DIM]; S.w[ni] = wp; S.w[n] = wn; }
        }
        // ---- RRTS_rewire_last
        if (wave == 0) {
            if (fr) {
                tree.get(ni, near);
                rrt_rewire<DIM>(m, lane, tree, rewired, n, ni, near, nw, near_goal, done, plen, checks);
            }
            if (lane == 0) { plen_out[n] = plen; cum[n] = checks; }
        }
        ++n;
        last_i = it;
        __syncthreads();
        if (success && q.stop) break;
    }
    __syncthreads();
    // ---- the tree comes out; search_tree.path(): from the last node along rewired_parents to the root
    double* states = q.states + row * DIM;
    for (int j = tid; j < n; j += kNpThreads) {
        states[(size_t)j * DIM] = S.x[j];
        states[(size_t)j * DIM + 1] = S.y[j];
        if (DIM == 3) states[(size_t)j * DIM + 2] = S.z[j];
        q.costs[row + j] = S.c[j];
        q.flags[row + j] = S.f[j];
        p.state_values[row + j] = S.sv[j];
        p.w[row + j] = S.w[j];
    }
    if (tid == 0) {
        bool cycle;
        const int L = rrt_path(S.f, rewired, n, q.path + row, cycle);
        if (cycle) status |= 2;                                  // the reference would not return
        q.n_nodes[b] = n;
        q.success[b] = success ? 1 : 0;
        q.last_iter[b] = last_i;
        q.used[b] = (int)pos;
        q.path_len[b] = L;
        q.status[b] = status;
        p.w_sum[b] = w_sum;
        p.guided[b] = g;
    }
}

}  // namespace

int next_plan_max_nodes() { return kNodes; }

hipError_t launch_next_plan(const NextPlanParams& p, hipStream_t st) {
    if (p.t.B <= 0) return hipSuccess;
    const size_t lds = sizeof(NextPlanLds);
    const void* fn = p.t.dim == 3 ? reinterpret_cast<const void*>(next_plan_kernel<3>) : reinterpret_cast<const void*>(next_plan_kernel<2>);
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    if (p.t.dim == 3) hipLaunchKernelGGL(next_plan_kernel<3>, dim3(p.t.B), dim3(kNpThreads), lds, st, p);
    else hipLaunchKernelGGL(next_plan_kernel<2>, dim3(p.t.B), dim3(kNpThreads), lds, st, p);
    return hipGetLastError();
}

}  // namespace gnnmp
