// rrt_tree.hpp -- the tree steps of NEXT_plan's RRT branch for one wave, shared by rrtstar_kernels.hip (the RRT* baseline) and
// next_plan_kernels.hip (NEXT's guided loop, whose wave 0 runs them): env.distance, the wrap of the angle, the counted
// env.step, the nearest non-terminal node, RRT_steer with step's clip and wrap, and RRTS_rewire_last's two passes
// (algorithm/tsa.py:83-139, 222-281, environment/maze_env.py:137-208).  All 64 lanes of the wave call every function with the
// same arguments.  Every helper lives in an unnamed namespace: each kernel file compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "maze_f64.hpp"

// numpy rounds every float64 operation on its own
#pragma clang fp contract(off)

namespace gnnmp {

namespace {

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
__device__ __forceinline__ bool rrt_step(const MzMaze& m, int lane, const double* s, const double* t, bool near_goal, long long& checks) {
    bool fr;
    if (DIM == 2) {
        int cnt = 0;
        fr = mz_edge2(m, s[0], s[1], t[0], t[1], cnt);
        if (fr && near_goal) mz_point(m, t[0], t[1], cnt);
        checks += cnt;
    } else {
        fr = mz_stick_edge_wave(m, lane, s, t, checks);
        if (fr && near_goal) {
            int cnt = 0;
            mz_stick(m, t[0], t[1], t[2], cnt);
            checks += cnt;
        }
    }
    return fr;
}

// the node state of one tree: coordinates, cost and flags by node id (LDS or global memory)
template <int DIM>
struct RrtNodes {
    double *x, *y, *z, *c;                                       // (z unused for the point robot)
    unsigned char* f;
    __device__ __forceinline__ void get(int j, double* out) const {
        out[0] = x[j]; out[1] = y[j];
        if (DIM == 3) out[2] = z[j];
    }
};

// the nearest NON-TERMINAL node of `smp` among nodes 0 .. n - 1: each lane owns nodes lane, lane + 64, ..., a wave minimum of
// (distance bits, id) = np.argmin's first minimum.  -> its id, the distance in `dmin`.
template <int DIM>
__device__ __forceinline__ int rrt_nearest(const RrtNodes<DIM>& t, int n, int lane, const double* smp, double& dmin) {
    unsigned long long best = ~0ull;
    int bi = 0x7fffffff;
    for (int j = lane; j < n; j += 64) {
        if (t.f[j] != kRrtFree) continue;
        double q[3];
        t.get(j, q);
        const unsigned long long k = (unsigned long long)__double_as_longlong(rrt_dist<DIM>(q, smp));      // d >= 0: bit order
        if (k < best) { best = k; bi = j; }                      // ascending ids: the first strict minimum
    }
    const unsigned long long wmin = wave_min_u64(best);
    const int ni = (int)wave_min_u64(best == wmin ? (unsigned long long)(unsigned)bi : ~0ull);
    dmin = __longlong_as_double((long long)wmin);
    return ni;
}

// RRT_steer from `near` towards `smp` (the sample itself within RRT_EPS, else interpolate(near, smp, RRT_EPS / dmin))
template <int DIM>
__device__ __forceinline__ void rrt_steer(const double* near, const double* smp, double dmin, double* nw) {
    if (dmin < kRrtEps) {
#pragma unroll
        for (int c = 0; c < DIM; ++c) nw[c] = smp[c];
    } else {
        const double ratio = kRrtEps / dmin;
        nw[0] = near[0] + (smp[0] - near[0]) * ratio;
        nw[1] = near[1] + (smp[1] - near[1]) * ratio;
        if (DIM == 3) nw[2] = rrt_wrap(near[2] + rrt_wrap(smp[2] - near[2]) * ratio);
    }
}
// env.step's clip of x and y and wrap of the angle, in place
template <int DIM>
__device__ __forceinline__ void rrt_clip(double* nw) {
    nw[0] = fmin(fmax(nw[0], -1.0), 1.0);
    nw[1] = fmin(fmax(nw[1], -1.0), 1.0);
    if (DIM == 3) nw[2] = rrt_wrap(nw[2]);
}

// RRTS_rewire_last for the FREE newest node n (state nw, grown from node ni with state near; its coordinates, flags and
// rewired[n] = ni are stored already): pass 1 walks the free near nodes that beat the minimum at the start of their group in
// index order (ballot, lowest bit first) against the RUNNING minimum, one edge check each (the minimum only falls, so a node
// that fails the test at the start of its group fails it later too); pass 2 checks every near node -- collided ones
// included, their cost is 2 -- that the new node would improve: point robot one candidate per lane (the checks are
// independent, their counts add up), stick robot one candidate at a time over the lanes.  Lane 0 stores the new node's cost
// and rewired parent; `plen` follows set_cost (search_tree.py:56-63).
template <int DIM>
__device__ __forceinline__ void rrt_rewire(const MzMaze& m, int lane, const RrtNodes<DIM>& t, int* rewired, int n, int ni, const double* near,
                                           const double* nw, bool near_goal, bool done, double& plen, long long& checks) {
    double* nc = t.c;
    // ---- pass 1: the cheapest free neighbour with a free edge becomes the parent
    double min_cost = rrt_dist<DIM>(near, nw) + nc[ni];
    int min_j = ni;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        bool cand = false;
        if (j < n && (t.f[j] & kRrtFree)) {
            double q[3];
            t.get(j, q);
            const double d = rrt_dist<DIM>(q, nw);
            cand = d < kRrtNearR && d + nc[j] < min_cost;
        }
        unsigned long long todo = __builtin_amdgcn_ballot_w64(cand);
        while (todo) {                                           // at most 64 bits, lowest index first
            const int jj = base + __builtin_ctzll(todo);
            todo &= todo - 1;
            double q[3];
            t.get(jj, q);
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
            t.get(j, q);
            const double d = rrt_dist<DIM>(q, nw);
            cost_new = min_cost + d;
            cand = d < kRrtNearR && cost_new < nc[j];
        }
        if (DIM == 2) {
            int cnt = 0;
            if (cand) {
                const bool ok = mz_edge2(m, q[0], q[1], nw[0], nw[1], cnt);
                if (ok && near_goal) mz_point(m, nw[0], nw[1], cnt);
                if (ok) { nc[j] = cost_new; rewired[j] = n; }
            }
            checks += wave_sum(cnt);
        } else {
            unsigned long long todo = __builtin_amdgcn_ballot_w64(cand);
            while (todo) {
                const int src = __builtin_ctzll(todo), jj = base + src;
                todo &= todo - 1;
                double qq[3];
                t.get(jj, qq);
                const bool ok = rrt_step<DIM>(m, lane, qq, nw, near_goal, checks);
                if (ok && lane == src) { nc[j] = cost_new; rewired[j] = n; }
            }
        }
    }
    if (lane == 0) { nc[n] = min_cost; rewired[n] = min_j; }
}

// search_tree.path(): node ids root -> node n - 1 along rewired (one lane calls this).  -> the length, 0 unless the last node
// is in the goal region; a walk longer than the node count (a cycle: the reference would not return) sets `cycle`.
__device__ __forceinline__ int rrt_path(const unsigned char* nf, const int* rewired, int n, int* path, bool& cycle) {
    int L = 0;
    cycle = false;
    if (nf[n - 1] & kRrtGoal) {
        int cur = n - 1;
        L = 1;
        while (cur != 0 && L <= n) {
            cur = rewired[cur];
            if (cur < 0 || cur >= n) { L = n + 1; break; }
            ++L;
        }
        if (L > n) { cycle = true; L = 0; }
        cur = n - 1;
        for (int k = L - 1; k >= 0; --k) { path[k] = cur; cur = rewired[cur]; }
    }
    return L;
}

}  // namespace

}  // namespace gnnmp
